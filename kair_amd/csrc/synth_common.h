// Device helpers shared by the training-data synthesis kernels (synth.hip, synth_usr.hip): the 8-way
// augment map and the counter-based normal generator.
#pragma once
#include "common.h"

// Augment modes (utils_image.augment_img, utils_image.py:387-405) are the 8 dihedral maps of a
// square n x n patch: out(i, j) = src(si, sj) with (p, q) = mode&1 ? (j, i) : (i, j),
// si = mode&2 ? n-1-p : p, sj = mode&4 ? n-1-q : q  (checked mode by mode against the numpy code).
KAIR_DEV void aug_src(int mode, int i, int j, int n, int& si, int& sj) {
  int p = i, q = j;
  if (mode & 1) { p = j; q = i; }
  si = (mode & 2) ? n - 1 - p : p;
  sj = (mode & 4) ? n - 1 - q : q;
}

// Philox-4x32-10 (Salmon et al., SC'11)
KAIR_DEV uint4 philox(uint4 ctr, uint2 key) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * ctr.x;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * ctr.z;
    const unsigned h0 = (unsigned)(p0 >> 32), l0 = (unsigned)p0, h1 = (unsigned)(p1 >> 32), l1 = (unsigned)p1;
    ctr = make_uint4(h1 ^ ctr.y ^ key.x, l1, h0 ^ ctr.w ^ key.y, l0);
    key.x += 0x9E3779B9u;
    key.y += 0xBB67AE85u;
  }
  return ctr;
}

// N(0, 1) keyed by (seed, step), counter = element index, Box-Muller
KAIR_DEV float normal_at(unsigned long long idx, unsigned long long seed, unsigned long long step) {
  const uint4 r = philox(make_uint4((unsigned)idx, (unsigned)(idx >> 32), (unsigned)step, (unsigned)(step >> 32)),
                         make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
  const float u1 = ((r.x >> 8) + 1) * (1.0f / 16777216.0f);   // (0, 1]
  const float u2 = (r.y >> 8) * (1.0f / 16777216.0f);         // [0, 1)
  return sqrtf(-2.f * __logf(u1)) * __cosf(6.283185307179586f * u2);
}
