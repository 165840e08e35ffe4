"""Blind-SR (BSRGAN degradation) batch synthesis beside the training steps it feeds.

    python tools/bench_blindsr_synth.py [--reps 20] [--no-step]

Two shapes: B 32, H_size 256, lq 64 (the real-world SwinIR's option file) and B 16, H_size 320, lq 72 (BSRNet's), both
x4.  Every batch draws a new program, so the time is a mean over `reps` different batches: device time between two HIP
events around PatchSynth.next (the fixed launch sequence of csrc/synth_blindsr.hip and kair_jpeg_roundtrip_var), the
wall time of the same calls (host draws and the table upload included), and a per-kernel table from the library's
kernel timing window over `reps` further batches.  With the step: the RRDBNet C5 fp32x3 step
(tools/bench_models.py rrdbnet: B 16, 32-px LQ) in the same process.  One JSON line."""
import argparse
import collections
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kair_amd import _hip as H  # noqa: E402
from kair_amd.data.gpu_synth import PatchSynth, synthetic_pool  # noqa: E402


def measure(B, PS, lq, reps, dev):
    pool = synthetic_pool(16, 3, PS + 64, PS + 64, seed=99, device=dev)
    s = PatchSynth(pool, task="blindsr", scale=4, H_size=PS, lq_patchsize=lq, seed=1000)
    for _ in range(3):
        s.next(B)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        s.next(B)
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps
    out = {"B": B, "H_size": PS, "lq": lq, "device_ms": round(e0.elapsed_time(e1) / reps, 3),
           "next_wall_ms": round(wall * 1e3, 3)}
    H.ktime_begin(64 * reps)
    for _ in range(reps):
        s.next(B)
    torch.cuda.synchronize()
    per = collections.defaultdict(lambda: [0, 0.0])
    for i in range(H.ktime_count()):
        ms, name = H.ktime_read(i)
        per[name][0] += 1
        per[name][1] += ms
    H.ktime_end()
    out["kernels_ms_per_batch"] = {k: [n // reps, round(t / reps, 4)] for k, (n, t) in sorted(per.items())}
    out["kernels_sum_ms"] = round(sum(t for _, t in per.values()) / reps, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="skip the RRDBNet C5 training step")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"swinir_realworld": measure(32, 256, 64, a.reps, dev), "bsrnet": measure(16, 320, 72, a.reps, dev)}
    if not a.no_step:
        import bench_models
        Bs, dt, loss = bench_models.run("rrdbnet", 10, 4, dev, "fp32x3")
        out["c5_fp32x3_step_ms"] = round(dt * 1e3, 3)
        out["bsrnet_share_of_step"] = round(out["bsrnet"]["device_ms"] / (dt * 1e3), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
