"""PatchSynth(task="fdncnn") / kair_synth_dn_map on the MI355X: the FDnCNN / DRUNet batch (noisy patch + noise-level
map) made by one launch, against the host replay of the crop and augment, the parameter table, and kair_synth_dn's
noise stream (bit for bit at equal levels)."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.data.gpu_synth import PatchSynth, synthetic_pool  # noqa: E402
from kair_amd.utils import utils_image as util  # noqa: E402

dev = torch.device("cuda")
PS, B = 24, 4


def pool_of(C):
    return synthetic_pool(3, C, 40, 48, seed=8 + C)


def table(rows, levels):
    """[B, 5] int32 device table: {image, rnd_h, rnd_w, mode} + the float32 bits of the level."""
    t = torch.zeros(len(rows), 5, dtype=torch.int32)
    t[:, :4] = torch.tensor(rows, dtype=torch.int32)
    t[:, 4:] = torch.tensor(levels, dtype=torch.float32).view(-1, 1).view(torch.int32)
    return t.to(dev)


def run_map(pool, par, seed, step):
    C = pool.shape[1]
    Hp, Lp = torch.empty(B, C, PS, PS, device=dev), torch.empty(B, C + 1, PS, PS, device=dev)
    H.synth_dn_map(pool, par, B, PS, seed, step, Hp, Lp)
    return Lp, Hp


def run_dn(pool, par, sigma, seed, step):
    C = pool.shape[1]
    Hp, Lp = torch.empty(B, C, PS, PS, device=dev), torch.empty(B, C, PS, PS, device=dev)
    H.synth_dn(pool, par[:, :4].contiguous(), B, PS, sigma, seed, step, Hp, Lp)
    return Lp, Hp


ROWS = [(0, 0, 0, 0), (2, 16, 24, 5), (1, 7, 3, 3), (2, 11, 19, 6)]   # corners of the crop range, four augment modes


@pytest.mark.parametrize("C", [1, 3])
def test_replay_map_channel_and_draw_order(C):
    pool = pool_of(C)
    s = PatchSynth(pool, task="fdncnn", H_size=PS, sigma=(5, 50), seed=9)
    L, Hh = s.next(B)
    assert L.shape == (B, C + 1, PS, PS) and Hh.shape == (B, C, PS, PS)
    par = s.last_params.cpu()
    assert par.shape == (B, 5) and par.dtype == torch.int32
    lev = par[:, 4:].view(torch.float32).flatten()
    cpu = pool.cpu().numpy()
    for b, (img, rh, rw, mode) in enumerate(par[:, :4].tolist()):
        patch = np.transpose(cpu[img][:, rh:rh + PS, rw:rw + PS], (1, 2, 0))                 # HWC, as the dataset's
        want = np.ascontiguousarray(np.transpose(util.augment_img(patch, mode), (2, 0, 1)))
        assert torch.equal(Hh[b].cpu(), torch.from_numpy(want))
        assert torch.equal(L[b, C].cpu(), torch.full((PS, PS), lev[b].item()))               # the table's level, exactly
    # last_params reproduces the host draws in the documented order: image, rnd_h, rnd_w, mode, sigma
    rng = random.Random(9)
    order = torch.randperm(3, generator=torch.Generator().manual_seed(9)).tolist()
    order += torch.randperm(3, generator=torch.Generator().manual_seed(10)).tolist()
    for b in range(B):
        row = [order[b], rng.randint(0, 40 - PS), rng.randint(0, 48 - PS), rng.randint(0, 7)]
        sig = rng.uniform(5, 50)
        assert par[b, :4].tolist() == row
        assert lev[b].item() == np.float32(sig / 255.0).item()
    assert (lev >= 5 / 255.0 - 1e-7).all() and (lev <= 50 / 255.0 + 1e-7).all() and len(set(lev.tolist())) == B
    # the stream: two next() calls differ, two synths with one seed agree bit for bit
    L2, H2 = s.next(B)
    assert not torch.equal(L2, L)
    s2 = PatchSynth(pool, task="fdncnn", H_size=PS, sigma=(5, 50), seed=9)
    L3, H3 = s2.next(B)
    assert torch.equal(L3, L) and torch.equal(H3, Hh)
    L4, H4 = s2.next(B)
    assert torch.equal(L4, L2) and torch.equal(H4, H2)
    d = PatchSynth(pool, task="fdncnn", H_size=PS, sigma=(5, 50), seed=9).next_dict(B)
    assert set(d) == {"L", "H"} and torch.equal(d["L"], L) and torch.equal(d["H"], Hh)


@pytest.mark.parametrize("C", [1, 3])
def test_equal_levels_reproduce_synth_dn_bits(C):
    pool = pool_of(C)
    s = 25 / 255.0
    par = table(ROWS, [s] * B)
    L, Hh = run_map(pool, par, 77, 5)
    Ld, Hd = run_dn(pool, par, s, 77, 5)
    assert torch.equal(Hh, Hd)
    assert torch.equal(L[:, :C], Ld)
    assert torch.equal(L[:, C], torch.full((B, PS, PS), np.float32(s).item(), device=dev))
    assert not torch.equal(run_map(pool, par, 77, 6)[0], L) and not torch.equal(run_map(pool, par, 78, 5)[0], L)


@pytest.mark.parametrize("C", [1, 3])
def test_unequal_and_zero_levels(C):
    pool = pool_of(C)
    levels = [0.0, 50 / 255.0, 3 / 255.0, 17.5 / 255.0]
    par = table(ROWS, levels)
    L, Hh = run_map(pool, par, 21, 2)
    L1, H1 = run_dn(pool, par, 1.0, 21, 2)
    assert torch.equal(Hh, H1)
    n = L1 - H1                                         # the normals, to fp32 rounding of |H + n| <= ~6
    assert 2.5 < n.abs().max().item() < 6.5 and abs(n.std().item() - 1.0) < 0.05
    lev = torch.tensor(levels, device=dev).view(B, 1, 1, 1)
    assert ((L[:, :C] - Hh) - lev * n).abs().max().item() < 1e-6
    assert torch.equal(L[0, :C], Hh[0])                 # sigma_b == 0 adds nothing
    assert not torch.equal(L[1, :C], Hh[1])
    for b in range(B):
        assert torch.equal(L[b, C], torch.full((PS, PS), np.float32(levels[b]).item(), device=dev))


def test_wrapper_rejects_bad_tables():
    pool = pool_of(1)
    Hp, Lp = torch.empty(B, 1, PS, PS, device=dev), torch.empty(B, 2, PS, PS, device=dev)
    with pytest.raises(ValueError):
        H.synth_dn_map(pool, table(ROWS, [0.1] * B)[:, :4], B, PS, 0, 0, Hp, Lp)              # no level column
    with pytest.raises(ValueError):
        H.synth_dn_map(pool, table(ROWS, [0.1] * B), B, PS, 0, 0, Hp, Hp)                     # L without the map channel
    with pytest.raises(ValueError):
        PatchSynth(pool, task="fdncnn", H_size=PS, sigma=(50, 5))
