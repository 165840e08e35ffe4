"""JPEG CAR training data on the GPU (csrc/synth_jpeg.hip, PatchSynth(task="jpeg"), utils_jpeg.jpeg_compress) against
the host statement of the same integer arithmetic (utils_jpeg.jpeg_roundtrip_np, itself equal to Pillow's libjpeg in
tests/test_jpeg_cpu.py).  Compared as integers, rint(255 out), with equality required; and |out - u / 255| <= 1e-7
(one fp32 division of an integer in 0..255 is within 2^-25 of it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.data.gpu_synth import PatchSynth  # noqa: E402
from kair_amd.utils import utils_image as util  # noqa: E402
from kair_amd.utils import utils_jpeg as jpg  # noqa: E402

dev = torch.device("cuda")
QUALITIES = [1, 10, 40, 75, 100]


def smooth(h, w, c):
    y, x = np.mgrid[0:h, 0:w]
    ch = [127 + 100 * np.sin(x / (3.0 + k) + k) * np.cos(y / (4.0 + k)) for k in range(c)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def noise(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def to_t(u):
    """uint8 [N, H, W, C] -> fp32 [N, C, H, W] / 255"""
    return torch.from_numpy(np.ascontiguousarray(u)).permute(0, 3, 1, 2).contiguous().float().div(255.0)


def same_u8(out, want_u8, what=""):
    """out fp32 [N, C, H, W] (device) against uint8 [N, H, W, C]"""
    out = out.cpu()
    want = torch.from_numpy(np.ascontiguousarray(want_u8)).permute(0, 3, 1, 2).to(torch.int32)
    got = (out.double() * 255).round().to(torch.int32)
    nbad = int((got != want).sum())
    assert nbad == 0, (what, nbad, int((got - want).abs().max()))
    assert float((out.double() - want.double() / 255).abs().max()) <= 1e-7, what


def roundtrip(x, qs):
    out = torch.full(x.shape, -1.0, device=dev)
    H.jpeg_roundtrip(x.to(dev).contiguous(), torch.tensor(qs, dtype=torch.int32, device=dev), out)
    torch.cuda.synchronize()
    return out


# ---- 1. whole images ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,size", [(1, s) for s in [(8, 8), (13, 21), (16, 24), (134, 134)]] +
                         [(3, s) for s in [(6, 5), (9, 9), (17, 7), (30, 18), (134, 134)]])
def test_roundtrip_vs_numpy(c, size):
    h, w = size
    imgs = [smooth(h, w, c), noise(h, w, c, 3 * h + w + c)]
    for q in QUALITIES:
        want = np.stack([jpg.jpeg_roundtrip_np(im, q) for im in imgs])
        same_u8(roundtrip(to_t(np.stack(imgs)), [q]), want, (c, size, q))


@pytest.mark.parametrize("c", [1, 3])
def test_roundtrip_per_sample_quality(c):
    imgs = [noise(19, 27, c, 40 + n) if n != 1 else smooth(19, 27, c) for n in range(3)]
    qs = [5, 60, 92]
    want = np.stack([jpg.jpeg_roundtrip_np(im, q) for im, q in zip(imgs, qs)])
    same_u8(roundtrip(to_t(np.stack(imgs)), qs), want, c)
    # out-of-range device qualities are clamped to 1..100, values outside [0, 1] to the range
    x = to_t(np.stack(imgs))
    same_u8(roundtrip(x * 1.5 - 0.2, [0, 100, 1000]),
            np.stack([jpg.jpeg_roundtrip_np(((x[n] * 1.5 - 0.2).clamp(0, 1) * 255).round().to(torch.uint8)
                                            .permute(1, 2, 0).numpy(), q) for n, q in enumerate([1, 100, 100])]), c)


def test_roundtrip_refuses_narrow_colour_and_bad_arguments():
    x = torch.rand(1, 3, 8, 4, device=dev)
    out = torch.full_like(x, -1.0)
    q = torch.tensor([40], dtype=torch.int32, device=dev)
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    L, p = H.lib(), H.ptr
    assert L.kair_jpeg_roundtrip(p(x), 1, 3, 8, 4, p(q), 0, p(out), p(ws), H.stream_ptr()) == -1   # KAIR_ERR_ARG
    assert b"width" in L.kair_last_error()
    assert L.kair_jpeg_roundtrip(p(x), 1, 2, 8, 4, p(q), 0, p(out), p(ws), H.stream_ptr()) == -1    # C not in {1, 3}
    assert L.kair_jpeg_roundtrip(p(x), 1, 1, 8, 4, None, 0, p(out), None, H.stream_ptr()) == -1     # null quality
    x5 = torch.rand(1, 3, 8, 5, device=dev)
    assert L.kair_jpeg_roundtrip(p(x5), 1, 3, 8, 5, p(q), 0, p(out), None, H.stream_ptr()) == -1    # colour, no workspace
    torch.cuda.synchronize()
    assert float(out.max()) == -1.0 and float(out.min()) == -1.0   # nothing was launched
    with pytest.raises(RuntimeError, match="width"):
        H.jpeg_roundtrip(x, q, out)
    assert L.kair_jpeg_workspace_bytes(2, 3, 17, 7) == 2 * 64 * (3 * 1 + 2 * 2 * 1)
    assert L.kair_jpeg_workspace_bytes(2, 1, 17, 7) == 0


# ---- 2. gray conversions -------------------------------------------------------------------------------------------
def test_rgb2gray8_all_triples():
    idx = torch.arange(1 << 24, dtype=torch.int32).reshape(4096, 4096)
    u = torch.stack([idx >> 16, (idx >> 8) & 255, idx & 255])   # [3, 4096, 4096]
    x = (u.float() / 255.0)[None].to(dev)
    out = torch.empty(1, 1, 4096, 4096, device=dev)
    R, G, B = (u[k].long() for k in range(3))
    got = []
    for mode in (0, 1):
        H.rgb2gray8(x, mode, out)
        o = out[0, 0].cpu()
        g = (o.double() * 255).round().long()
        assert float((o.double() - g.double() / 255).abs().max()) <= 1e-7
        got.append(g)
    assert torch.equal(got[1], (4899 * R + 9617 * G + 1868 * B + 8192) >> 14)
    want = torch.from_numpy(util.rgb2ycbcr(u.permute(1, 2, 0).to(torch.uint8).numpy())).long()
    tie = (65481 * R + 128553 * G + 24966 * B) % 255000 == 127500
    assert int(tie.sum()) <= 194
    assert torch.equal(got[0][~tie], want[~tie])
    assert int((got[0][tie] - want[tie]).abs().max()) <= 1
    del x, out
    with pytest.raises(RuntimeError):
        H.check(H.lib().kair_rgb2gray8(None, 1, 4, 4, 0, None, H.stream_ptr()), "rgb2gray8")


# ---- 3. the batch kernel -------------------------------------------------------------------------------------------
def host_synth(pool, par, PS, is_color):
    """crop, augment_img_tensor4, uint8, gray conversion (util.rgb2ycbcr / jpg.rgb2gray_cv), jpeg_roundtrip_np,
    second crop: uint8 (L, H) [B, PS, PS, C]."""
    Ls, Hs = [], []
    P = PS + 8
    for img, rh, rw, mode, gm, q, rh2, rw2 in par.tolist():
        crop = util.augment_img_tensor4(pool[img:img + 1, :, rh:rh + P, rw:rw + P], mode)
        assert crop.shape[-2:] == (P, P)
        u = (crop[0].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
        if not is_color and u.shape[2] == 3:
            if gm == 0:
                w = u.astype(np.int64)
                s = 65481 * w[..., 0] + 128553 * w[..., 1] + 24966 * w[..., 2]
                # an exact tie (12 in a million triples) rounds up on the device (kair_hip.h); rgb2ycbcr's float64
                # rounding of one depends on the evaluation order
                tie = s % 255000 == 127500
                u = np.where(tie, 16 + (s + 127500) // 255000, util.rgb2ycbcr(u)).astype(np.uint8)[..., None]
            else:
                u = jpg.rgb2gray_cv(u)[..., None]
        dec = jpg.jpeg_roundtrip_np(u, q)
        Hs.append(u[rh2:rh2 + PS, rw2:rw2 + PS])
        Ls.append(dec[rh2:rh2 + PS, rw2:rw2 + PS])
    return np.stack(Ls), np.stack(Hs)


def make_pool(N, C, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(N, C, Hs // 4, Ws // 4, generator=g)
    x = torch.nn.functional.interpolate(base, size=(Hs, Ws), mode="bicubic", align_corners=False)
    x = x + 0.1 * torch.randn(x.shape, generator=g)
    x[0] = torch.rand(C, Hs, Ws, generator=g) * 1.2 - 0.1   # one noise image, with values to clamp
    return x.contiguous()


def synth_rows(N, Hs, Ws, PS):
    """16 rows: all 8 modes, both gray modes, rh2 / rw2 over {0, 3, 8}, a crop at the pool's last row and column."""
    P = PS + 8
    offs = [0, 3, 8]
    rows = []
    for b in range(16):
        rh, rw = (7 * b) % (Hs - P + 1), (5 * b + 1) % (Ws - P + 1)
        if b == 5:
            rh, rw = Hs - P, Ws - P
        rows.append([b % N, rh, rw, b % 8, (b // 8 + b) % 2, [1, 10, 40, 75, 100][b % 5], offs[b % 3], offs[(b // 3) % 3]])
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("C,PS,is_color", [(3, 8, False), (3, 14, False), (3, 24, False), (1, 14, False), (1, 24, False),
                                           (3, 10, True), (3, 24, True)])
def test_synth_vs_host(C, PS, is_color):
    pool = make_pool(3, C, 40, 56, seed=PS + C)
    par = synth_rows(3, 40, 56, PS)
    assert {r[3] for r in par.tolist()} == set(range(8)) and {r[4] for r in par.tolist()} == {0, 1}
    assert {r[6] for r in par.tolist()} == {r[7] for r in par.tolist()} == {0, 3, 8}
    B, Co = par.shape[0], 3 if is_color else 1
    Hp = torch.full((B, Co, PS, PS), -1.0, device=dev)
    Lp = torch.full((B, Co, PS, PS), -1.0, device=dev)
    H.synth_jpeg(pool.to(dev), par.to(dev), B, PS, is_color, Hp, Lp)
    torch.cuda.synchronize()
    wantL, wantH = host_synth(pool, par, PS, is_color)
    same_u8(Hp, wantH, "H")
    same_u8(Lp, wantL, "L")
    assert not torch.equal(Lp, Hp)


def test_synth_refuses_bad_arguments():
    pool = torch.rand(2, 3, 30, 30, device=dev)
    par = synth_rows(2, 40, 40, 8).to(dev)
    o1, o3 = torch.empty(16, 1, 24, 24, device=dev), torch.empty(16, 3, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match="smaller"):
        H.synth_jpeg(pool, par, 16, 24, False, o1, o1.clone())          # 24 + 8 > 30
    with pytest.raises(RuntimeError, match="3-channel"):
        H.synth_jpeg(pool[:, :1].contiguous(), par, 16, 8, True, o3, o3.clone())
    with pytest.raises(ValueError):
        H.synth_jpeg(pool, par[:, :4].contiguous(), 16, 8, True, o3, o3.clone())   # 4 columns


# ---- 4. PatchSynth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_color", [False, True])
def test_patchsynth_jpeg(is_color):
    pool = make_pool(5, 3, 40, 56, seed=21)
    qs = [10, 30, 50]
    a = PatchSynth(pool.to(dev), task="jpeg", H_size=16, quality_factor=qs, is_color=is_color, seed=4)
    b = PatchSynth(pool.to(dev), task="jpeg", H_size=16, quality_factor=qs, is_color=is_color, seed=4)
    seen_q, pars = set(), []
    for _ in range(4):
        La, Ha = a.next(16)
        Lb, Hb = b.next(16)
        assert torch.equal(La, Lb) and torch.equal(Ha, Hb) and torch.equal(a.last_params, b.last_params)
        par = a.last_params.cpu()
        assert par.shape == (16, 8) and par.dtype == torch.int32
        wantL, wantH = host_synth(pool, par, 16, is_color)
        same_u8(La, wantL, "L")
        same_u8(Ha, wantH, "H")
        pars.append(par)
    par = torch.cat(pars)   # 64 draws
    assert set(par[:, 5].tolist()) == set(qs)
    assert int(par[:, 6:].min()) >= 0 and int(par[:, 6:].max()) <= 8 and int(par[:, 6:].max()) > 0
    assert int(par[:, 1].max()) <= 40 - 24 and int(par[:, 2].max()) <= 56 - 24 and set(par[:, 3].tolist()) == set(range(8))
    assert set(par[:, 4].tolist()) == ({0} if is_color else {0, 1})
    assert La.shape == (16, 3 if is_color else 1, 16, 16)


def test_patchsynth_jpeg_int_quality_and_small_pool():
    pool = make_pool(2, 1, 24, 30, seed=2).to(dev)
    s = PatchSynth(pool, task="jpeg", H_size=16, quality_factor=35, seed=1)
    L, Hh = s.next(4)
    assert set(s.last_params[:, 5].tolist()) == {35} and L.shape == Hh.shape == (4, 1, 16, 16)
    with pytest.raises(ValueError):
        PatchSynth(pool, task="jpeg", H_size=17)            # 17 + 8 > 24
    with pytest.raises(ValueError):
        PatchSynth(pool, task="jpeg", H_size=16, is_color=True)   # 1-channel pool
    with pytest.raises(ValueError):
        PatchSynth(pool, task="jpeg", H_size=16, quality_factor=[40, 101])


# ---- 5. the tensor-level entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_jpeg_compress_device_equals_cpu(c):
    g = torch.Generator().manual_seed(9)
    x = torch.rand(3, c, 21, 29, generator=g)
    for q in (40, [15, 55, 95]):
        assert torch.equal(jpg.jpeg_compress(x.to(dev), q).cpu(), jpg.jpeg_compress(x, q))


# ---- 6. one training step -----------------------------------------------------------------------------------------
def test_patchsynth_jpeg_feeds_modelplain(tmp_path):
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    opt = {"model": "plain", "is_train": True, "dist": False, "gpu_ids": [0], "scale": 1, "n_channels": 1,
           "path": {"models": str(tmp_path)},
           "netG": {"net_type": "swinir", "upscale": 1, "in_chans": 1, "img_size": 14, "window_size": 7,
                    "img_range": 255.0, "depths": [2, 2], "embed_dim": 60, "num_heads": [6, 6], "mlp_ratio": 2,
                    "upsampler": "", "resi_connection": "1conv", "init_type": "default", "drop_path_rate": 0.0},
           "train": {"G_lossfn_type": "charbonnier", "G_lossfn_weight": 1.0, "G_charbonnier_eps": 1e-9,
                     "G_optimizer_type": "adam", "G_optimizer_lr": 2e-4, "G_optimizer_betas": [0.9, 0.999],
                     "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                     "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                     "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True}}
    torch.manual_seed(0)
    model = define_Model(dict_to_nonedict(opt))
    model.init_train()
    pool = make_pool(4, 3, 40, 40, seed=12).to(dev)
    s = PatchSynth(pool, task="jpeg", H_size=14, quality_factor=10, seed=5)
    L, Hh = s.next(2)
    assert L.shape == Hh.shape == (2, 1, 14, 14) and not torch.equal(L, Hh)
    before = {k: v.detach().clone() for k, v in model.netG.state_dict().items()}
    model.feed_data({"L": L, "H": Hh})
    model.optimize_parameters(1)
    loss = model.log_dict["G_loss"]
    assert np.isfinite(loss) and loss > 0
    after = model.netG.state_dict()
    assert any((after[k] - before[k]).abs().max() > 0 for k in before)
