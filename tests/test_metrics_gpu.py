"""kair_image_metrics / tensor_metrics / ModelPlain.test_metrics / main_train_psnr on the MI355X.  The reference is
always the host path (tensor2uint -> [Y] -> calculate_psnr / calculate_ssim, float64 numpy) on the same tensors copied
to the CPU.

Bars.  PSNR: `==`: the SSE is an exact integer on both sides and the dB come from the same float64 formula.  SSIM:
|device - host| <= 1e-6: the driver prints SSIM to four decimals and the bar is 1/50 of that print's half unit; it is
what separates the kernel's fp64 moments from plain fp32 on 0..255 data (65025 * 2^-24 = 4e-3 against C2 = 58.5).
Every test prints its figures before it asserts.

Measured on the MI355X.  SSE: equal to the host's in every case, the 2^24 Y triples and the half-level image included.
SSIM: largest |device - host| 1.7e-13 (the checkerboard pair; 8.9e-16 over the random cases).  PSNR: torch's float64
log10 on the device differs from the host C library's in the last place on 18 % of values (36864 of 200000 sampled
(sse, count) pairs; sqrt and the divisions never differ) -- with it the 'plain' hook test gave 15.450549682733882
against the host's 15.450549682733886 -- so the dB come from kair_psnr_db, which computes log10 the way the host
library does (fdlibm's formula around a correctly rounded log).  It equals the host except where the host's own log is
misrounded (16 of 30000 sampled values on the CPU; 0 of 1204 here); every PSNR of this file equals the host's."""
import functools
import io
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip  # noqa: E402
from kair_amd.utils import utils_image as U  # noqa: E402
from test_metrics_cpu import (ROOT, driver_overrides, host_metrics, nudge_ties, random_pair,  # noqa: E402
                              recompute_on_the_host, sse_count_samples)

dev = torch.device("cuda")
SSIM_BAR = 1e-6

# (B, C, H, W, border, y_channel, ssim)
CASES = [(1, 1, 11, 11, 0, False, True),     # a single window
         (1, 1, 19, 19, 4, False, True),     # an 11 x 11 region after the crop
         (1, 1, 12, 33, 0, False, True),     # one tile plus one column
         (2, 3, 45, 70, 4, False, True),     # several partial tiles, a border and a batch
         (3, 1, 64, 64, 2, False, True),
         (1, 3, 37, 64, 0, True, True),      # Y, ties nudged off
         (1, 1, 5, 7, 0, False, False)]      # PSNR only, smaller than the window


@functools.lru_cache(maxsize=None)
def case(spec):
    """The inputs of a case and their host reference: computed once, shared, never modified."""
    B, C, Hh, Ww, border, y, ssim = spec
    E, Ht = random_pair((B, C, Hh, Ww), 1000 + Hh * Ww + border)
    if y:
        E, Ht = nudge_ties(E)[0], nudge_ties(Ht)[0]
    return E, Ht, host_metrics(E, Ht, border, y_channel=y, ssim=ssim)


def check(got, want, ssim=True, what=""):
    """got: device [B, 2]; want: the host list of (psnr, ssim).  Prints each figure before asserting."""
    got = got.cpu()
    assert got.dtype == torch.float64 and got.shape == (len(want), 2)
    worst = 0.0
    for b, (p, s) in enumerate(want):
        d = abs(got[b, 1].item() - s) if ssim else 0.0
        worst = max(worst, d)
        print(f"{what} image {b}: psnr device {got[b, 0].item()!r} host {p!r}; ssim device {got[b, 1].item()!r} "
              f"host {s!r} diff {d:.3g}")
    for b, (p, s) in enumerate(want):
        assert got[b, 0].item() == p, (what, b, got[b, 0].item(), p)
        if ssim:
            assert abs(got[b, 1].item() - s) <= SSIM_BAR, (what, b, got[b, 1].item(), s)
        else:
            assert math.isnan(got[b, 1].item())
    return worst


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_tensor_metrics_against_the_host_path(spec):
    B, C, Hh, Ww, border, y, ssim = spec
    E, Ht, want = case(spec)
    got = U.tensor_metrics(E.to(dev), Ht.to(dev), border=border, y_channel=y, ssim=ssim)
    assert got.is_cuda
    check(got, want, ssim, str(spec))


def test_rounding_of_half_levels_and_the_clamp():
    """(k + 0.5) / 255 in fp32 for k = 0 .. 254 with -0.3, 1.7, 0 and 1: x * 255 lands on or beside the half-way points,
    where an FMA, a reciprocal or round-half-away would move the level.  (259 values: a 17 x 16 image, the last 13
    pixels repeating 0.5 -- 16 x 16 holds only 256.)  SSE against H = 0 and H = 1 equals the host's exactly."""
    v = torch.cat([(torch.arange(255, dtype=torch.float32) + 0.5) / 255.0, torch.tensor([-0.3, 1.7, 0.0, 1.0]),
                   torch.full((13,), 0.5)])
    E = v.view(1, 1, 17, 16)
    for level in (0.0, 1.0):
        Ht = torch.full_like(E, level)
        he, hh = U.tensor2uint(E).astype(np.int64), U.tensor2uint(Ht).astype(np.int64)
        sse = int(((he - hh) ** 2).sum())
        out = torch.zeros(1, 2, dtype=torch.float64, device=dev)
        ws = _hip.image_metrics_workspace(1, 1, 17, 16, 0, 0, dev)
        _hip.image_metrics(E.to(dev), Ht.to(dev), out, 1, 1, 17, 16, 0, 0, ws)
        print(f"H = {level}: device sse {out[0, 0].item()!r}, host {sse}")
        assert out[0, 0].item() == float(sse) and out[0, 1].item() == 0.0   # (column 1 untouched without SSIM)
        check(U.tensor_metrics(E.to(dev), Ht.to(dev)), host_metrics(E, Ht), what=f"half levels, H = {level}")


def test_cancellation_on_flat_and_checkerboard_images():
    """E = 200 / 255 against H = 201 / 255: the variances are exact zeros taken as differences of numbers near 40000
    against C2 = 58.5; then +-1-level checkerboards in opposite phase on both."""
    E, Ht = torch.full((1, 1, 40, 40), 200 / 255.0), torch.full((1, 1, 40, 40), 201 / 255.0)
    check(U.tensor_metrics(E.to(dev), Ht.to(dev)), host_metrics(E, Ht), what="flat 200 / 201")
    yy, xx = torch.meshgrid(torch.arange(40), torch.arange(40), indexing="ij")
    cb = (((yy + xx) % 2) * 2 - 1).float().view(1, 1, 40, 40)
    E2, H2 = (200 + cb) / 255.0, (201 - cb) / 255.0
    check(U.tensor_metrics(E2.to(dev), H2.to(dev)), host_metrics(E2, H2), what="checkerboard 200 / 201")
    E3 = E.expand(1, 3, 40, 40).clone()
    H3 = torch.cat([Ht, H2, E2], dim=1)
    check(U.tensor_metrics(E3.to(dev), H3.to(dev), border=3), host_metrics(E3, H3, 3), what="flat / checkerboard, C = 3")


def test_identical_images():
    E = case(CASES[3])[0].to(dev)
    got = U.tensor_metrics(E, E.clone(), border=4).cpu()
    print("identical:", got.tolist())
    assert (got[:, 0] == math.inf).all()
    assert ((got[:, 1] - 1.0).abs() <= SSIM_BAR).all()


def test_y_channel_over_every_rgb_triple():
    """All 2^24 triples as 16 images of 3 x 1024 x 1024 against a constant gray: each image's Y SSE equals the host's
    from rgb2y_uint8 (so does every tie: the integer rule is the definition)."""
    lv = (torch.arange(256, dtype=torch.float32) / 255.0).to(dev)
    t = torch.arange(1 << 24, device=dev).view(16, 1, 1024, 1024)
    E = lv[torch.cat([t >> 16, (t >> 8) & 255, t & 255], dim=1)]
    del t
    Ht = torch.full((1, 1, 1, 1), 128 / 255.0, device=dev).expand(16, 3, 1024, 1024).contiguous()
    out = torch.zeros(16, 2, dtype=torch.float64, device=dev)
    ws = _hip.image_metrics_workspace(16, 3, 1024, 1024, 0, _hip.METRIC_Y, dev)
    _hip.image_metrics(E, Ht, out, 16, 3, 1024, 1024, 0, _hip.METRIC_Y, ws)
    got = out[:, 0].cpu()
    n = np.arange(1 << 24, dtype=np.int64)
    tri = np.stack([n >> 16, (n >> 8) & 255, n & 255], axis=-1).astype(np.uint8)
    y = U.rgb2y_uint8(tri).astype(np.int64).reshape(16, -1)
    yh = int(U.rgb2y_uint8(np.array([128, 128, 128], np.uint8)))
    want = ((y - yh) ** 2).sum(axis=1)
    print("device", got.tolist(), "host", want.tolist())
    assert got.tolist() == [float(w) for w in want]


def test_psnr_db_kernel_gives_the_host_instance_bits():
    """kair_psnr_db on the device against kair_psnr_db_ref, the same source on the host (tests/test_metrics_cpu.py holds
    that one to its definition): `==` on every sample, through strided and in-place calls; and against the host C
    library's calculate_psnr arithmetic, where only the values its own log misrounds may differ (<= 3.8 %, see there)."""
    samples = sse_count_samples(4000, 11)
    by_count = {}
    for s, c in samples[:40]:
        by_count.setdefault(c, []).append(s)
    c0 = 3 * 37 * 62
    by_count[c0] = [0] + [s for s, _ in sse_count_samples(4000, 12) if s <= 65025 * c0][:3000] + [65025 * c0]
    differ = total = 0
    for c, ss in by_count.items():
        buf = torch.zeros(len(ss), 2, dtype=torch.float64)
        buf[:, 0] = torch.tensor(ss, dtype=torch.float64)
        buf = buf.to(dev)
        out = torch.empty(len(ss), dtype=torch.float64, device=dev)
        _hip.psnr_db(buf[:, 0], out, c)             # strided in, dense out
        _hip.psnr_db(buf[:, 0], buf[:, 0], c)       # in place
        assert torch.equal(out, buf[:, 0]) and (buf[:, 1] == 0).all()
        got = out.cpu().tolist()
        assert got == [_hip.psnr_db_ref(s, c) for s in ss]
        differ += sum(g != (math.inf if s == 0 else 20 * math.log10(255.0 / math.sqrt(s / c))) for g, s in zip(got, ss))
        total += len(ss)
    print(f"kair_psnr_db against the host libm: {differ} of {total} differ")
    assert differ <= 0.038 * total


def test_repeated_calls_streams_and_views_give_the_same_bits():
    E, Ht, _ = case(CASES[3])
    E, Ht = E.to(dev), Ht.to(dev)
    a = U.tensor_metrics(E, Ht, border=4)
    b = U.tensor_metrics(E, Ht, border=4)
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = U.tensor_metrics(E, Ht, border=4)
    s.synchronize()
    assert torch.equal(a, c)
    wide = torch.zeros(2, 3, 45, 140, device=dev)
    wide[..., ::2] = E
    view = wide[..., ::2]
    assert not view.is_contiguous()
    assert torch.equal(a, U.tensor_metrics(view, Ht, border=4))
    assert torch.equal(a[1:], U.tensor_metrics(E[1], Ht[1], border=4))              # [C, H, W]
    assert torch.equal(a, U.tensor_metrics(E.double(), Ht.double(), border=4))      # fp32 values in a wider dtype
    y1 = U.tensor_metrics(E, Ht, border=4, y_channel=True)
    assert torch.equal(y1, U.tensor_metrics(E, Ht, border=4, y_channel=True)) and not torch.equal(y1, a)


def test_errors_raise_before_any_launch():
    E, Ht = (t.to(dev) for t in random_pair((1, 3, 10, 30), 6))
    with pytest.raises(ValueError):
        U.tensor_metrics(E, Ht)
    with pytest.raises(ValueError):
        U.tensor_metrics(E, Ht[..., :29], ssim=False)
    with pytest.raises(ValueError):
        U.tensor_metrics(E[:, :2], Ht[:, :2], ssim=False)
    with pytest.raises(ValueError):
        U.tensor_metrics(E[:, :1], Ht[:, :1], y_channel=True, ssim=False)
    ok = U.tensor_metrics(E, Ht, ssim=False).cpu()                  # the same region is accepted without SSIM
    assert math.isfinite(ok[0, 0].item()) and torch.isnan(ok[0, 1])
    out = torch.zeros(1, 2, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="image_metrics"):
        _hip.image_metrics(E, Ht, out, 1, 3, 10, 30, 5, 0, torch.empty(64, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="workspace too small"):
        _hip.image_metrics(E, Ht, out, 1, 3, 10, 30, 0, 0, torch.empty(16, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the model hook and the driver
# ---------------------------------------------------------------------------------------------------------------------
def _model(kind, netG):
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    opt = {"model": kind, "is_train": True, "dist": False, "gpu_ids": [0], "scale": 1, "path": {"models": "/tmp/k"},
           "netG": dict(netG, init_type="orthogonal", init_bn_type="uniform", init_gain=1.0),
           "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                     "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                     "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                     "G_scheduler_gamma": 0.5, "E_decay": 0, "G_param_strict": True, "E_param_strict": True}}
    torch.manual_seed(61)
    model = define_Model(dict_to_nonedict(opt))
    model.init_train()
    return model


@pytest.mark.parametrize("kind", ["plain", "plain2"])
def test_model_hook_against_the_host_functions(kind):
    """A small DnCNN ('plain'; nc 8 is the narrowest the engine takes) and a small FFDNet ('plain2', which feeds C too):
    feed_data, test(), test_metrics(border=2) against the host functions on current_results()."""
    if kind == "plain":
        model = _model(kind, {"net_type": "dncnn", "in_nc": 1, "out_nc": 1, "nc": 8, "nb": 3, "act_mode": "R"})
    else:
        model = _model(kind, {"net_type": "ffdnet", "in_nc": 1, "out_nc": 1, "nc": 16, "nb": 4, "act_mode": "R"})
    g = torch.Generator().manual_seed(62)
    Ht = torch.rand(2, 1, 24, 24, generator=g)
    L = Ht + 0.1 * torch.randn(2, 1, 24, 24, generator=g)
    model.feed_data({"L": L, "H": Ht, "C": torch.tensor([25.0, 10.0]).view(2, 1, 1, 1) / 255})
    model.test()
    got = model.test_metrics(border=2)
    assert got.is_cuda
    res = model.current_results()
    assert res["E"].shape == (2, 1, 24, 24)
    check(got, host_metrics(res["E"], res["H"], 2), what=f"{kind} hook")
    nos = model.test_metrics(border=2, ssim=False).cpu()
    assert torch.equal(nos[:, 0], got[:, 0].cpu()) and torch.isnan(nos[:, 1]).all()


def test_main_train_psnr_on_the_gpu(tmp_path):
    """The driver with the tiny files of the CPU test: the device averages equal the host recomputation of the same
    test phase (PSNR ==, SSIM within the bar)."""
    from kair_amd.main_train_psnr import main
    log = io.StringIO()
    path = os.path.join(ROOT, "options", "train_dncnn.json")
    model, hist = main(path, driver_overrides(str(tmp_path), [0], 4, test_ssim=True), log_stream=log)
    assert model.device.type == "cuda" and model.trainer is not None
    assert len(hist["loss"]) == 4 and all(np.isfinite(hist["loss"]))
    assert [s for s, _ in hist["psnr"]] == [2, 4] and [s for s, _ in hist["ssim"]] == [2, 4]
    psnr, ssim, n = recompute_on_the_host(model, border=1)
    print(f"driver: psnr device {hist['psnr'][-1][1]!r} host {psnr!r}; ssim device {hist['ssim'][-1][1]!r} host {ssim!r} "
          f"diff {abs(hist['ssim'][-1][1] - ssim):.3g}")
    assert n == 3 and hist["psnr"][-1] == (4, psnr)
    assert abs(hist["ssim"][-1][1] - ssim) <= SSIM_BAR
    assert "Average PSNR : {:<.2f}dB, Average SSIM : {:<.4f}".format(psnr, hist["ssim"][-1][1]) in log.getvalue()
