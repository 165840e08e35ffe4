"""USRNet training data on the GPU (csrc/synth_usr.hip, PatchSynth(task="usrnet"), utils_sisr.degrade) against
float64 torch expressions written here.

Forward model: L0[i, j] = sum_{u, v} k[u, v] H[(i sf + kh//2 - u) mod PS, (j sf + kw//2 - v) mod PS], i.e. the
circular convolution F.conv2d(F.pad(H, circular), k.flip(-1, -2)) sampled at [::sf, ::sf] (taken here as the conv's
stride, which is the same numbers).  Bound for L0: 625 fp32 fmafs of inputs in [0, 1] and a kernel summing to 1
stay within n u max = 625 * 2^-24 * 1 = 3.7e-5 < 4e-5 of the exact sum.  The Philox noise has no bitwise pin, so it
is checked statistically at the bars of tests/test_data_gpu.py."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from kair_amd import _hip as H  # noqa: E402
from kair_amd.data.gpu_synth import PatchSynth, synthetic_pool  # noqa: E402
from kair_amd.utils import utils_image as util  # noqa: E402
from kair_amd.utils import utils_sisr as sisr  # noqa: E402

dev = torch.device("cuda")
TOL = 4e-5


def aug4(x, mode):
    return util.augment_img_tensor4(x, mode)


def ref_blur(Hh, k, sf):
    """float64 reference: Hh [B, C, PH, PW], k [B, 1, kh, kw] (or [1, 1, kh, kw] for all) -> L0."""
    B, C, PH, PW = Hh.shape
    kh, kw = k.shape[-2:]
    x = F.pad(Hh.double(), (kw - 1 - kw // 2, kw // 2, kh - 1 - kh // 2, kh // 2), mode="circular")
    w = k.double().flip(-1, -2).expand(B, 1, kh, kw).repeat_interleave(C, 0)
    return F.conv2d(x.reshape(1, B * C, *x.shape[-2:]), w, stride=sf, groups=B * C).reshape(B, C, -(-PH // sf), -(-PW // sf))


def rand_kernels(B, ks, g):
    k = torch.rand(B, 1, ks, ks, generator=g) ** 3
    return (k / k.sum((-2, -1), keepdim=True)).float()


def crops(pool, par, PS):
    """The augmented crops the parameter rows describe, on the host."""
    return torch.cat([aug4(pool[i:i + 1, :, rh:rh + PS, rw:rw + PS], m) for i, rh, rw, m in par.tolist()])


def run_synth(pool, par, k, sf, PS, sigma=None, trunc8=False, seed=0, step=0, direct=False):
    B, C = par.shape[0], pool.shape[1]
    Hp = torch.empty(B, C, PS, PS, device=dev)
    Lp = torch.empty(B, C, PS // sf, PS // sf, device=dev)
    H.synth_usr(pool.to(dev), par.to(dev), B, PS, sf, k.to(dev), None if sigma is None else sigma.to(dev), trunc8, seed,
                step, Hp, Lp, direct=direct)
    torch.cuda.synchronize()
    return Lp.cpu(), Hp.cpu()


def rand_params(N, Hs, Ws, PS, B, g, mode0=0):
    rows = [[int(torch.randint(0, N, (1,), generator=g)), int(torch.randint(0, Hs - PS + 1, (1,), generator=g)),
             int(torch.randint(0, Ws - PS + 1, (1,), generator=g)), (mode0 + b) % 8] for b in range(B)]
    return torch.tensor(rows, dtype=torch.int32)


def gauss_ref(ks, l1, l2, th, sf_k, mode_k):
    """The float64 formula of utils_sisr.gen_kernel, written out with Sigma itself and a matrix inverse."""
    cs, sn = math.cos(th), math.sin(th)
    Q = torch.tensor([[cs, -sn], [sn, cs]], dtype=torch.float64)
    Sigma = Q @ torch.diag(torch.tensor([l1, l2], dtype=torch.float64)) @ Q.T
    inv = torch.linalg.inv(Sigma)
    mu = ks // 2 + 0.5 * (sf_k - ks % 2)
    ax = torch.arange(ks, dtype=torch.float64) - mu
    zy, zx = torch.meshgrid(ax, ax, indexing="ij")
    z = torch.stack([zx, zy], -1)
    raw = torch.exp(-0.5 * torch.einsum("yxi,ij,yxj->yx", z, inv, z))
    return aug4((raw / raw.sum())[None, None], mode_k)[0, 0]


# ---- 1. kernels -------------------------------------------------------------------------------------------------
def test_gauss_kernels_and_bank():
    g = torch.Generator().manual_seed(11)
    lam = [0.6, 12.0, 3.7]
    rows_f, rows_i = [], []
    for b in range(16):   # sf_k 1..4 x all 8 modes (twice over), lambda at both ends
        l1, l2 = lam[b % 2], lam[(b // 2 + 1) % 3]
        rows_f.append([l1, l2, float(torch.rand(1, generator=g)) * math.pi])
        rows_i.append([0, 0, b % 4 + 1, (b // 2 + b) % 8])
    assert {r[3] for r in rows_i} == set(range(8)) and {(r[0], r[1]) for r in rows_f} >= {(0.6, 0.6), (12.0, 12.0)}
    bank = torch.rand(3, 25, 25, generator=g) * 5
    for b, idx in enumerate([2, 0, 1, 2]):   # bank rows: copied, renormalised, not augmented (mode_k ignored)
        rows_f.append([1.0, 1.0, 0.0])
        rows_i.append([1, idx, 1, 3 + b])
    gpar, kpar = torch.tensor(rows_f, dtype=torch.float32), torch.tensor(rows_i, dtype=torch.int32)
    out = torch.empty(20, 1, 25, 25, device=dev)
    H.usr_gauss_kernels(gpar.to(dev), kpar.to(dev), bank.to(dev), out)
    torch.cuda.synchronize()
    out = out.cpu().double()
    for b in range(20):
        l1, l2, th = gpar[b].double().tolist()   # the float32 values the device read
        if kpar[b, 0] == 0:
            want = gauss_ref(25, l1, l2, th, int(kpar[b, 2]), int(kpar[b, 3]))
            assert (sisr.gen_kernel(25, l1, l2, th, int(kpar[b, 2]), int(kpar[b, 3])) - want).abs().max() < 1e-12
        else:
            want = bank[kpar[b, 1]].double() / bank[kpar[b, 1]].double().sum()
        assert (out[b, 0] - want).abs().max() < 1e-6, b
        assert abs(out[b, 0].sum().item() - 1.0) < 1e-6, b
    # without a bank a 'bank' row falls back to the Gaussian of its parameters
    out2 = torch.empty(20, 1, 25, 25, device=dev)
    H.usr_gauss_kernels(gpar.to(dev), kpar.to(dev), None, out2)
    assert (out2[16, 0].cpu().double() - gauss_ref(25, 1.0, 1.0, 0.0, 1, 3)).abs().max() < 1e-6


# ---- 2. blur + decimation, noise off ----------------------------------------------------------------------------
@pytest.mark.parametrize("sf", [1, 2, 3, 4])
def test_blur_ps12_wraps_twice_all_modes(sf):
    g = torch.Generator().manual_seed(20 + sf)
    pool = torch.rand(3, 3, 20, 17, generator=g)   # non-square pool
    par = rand_params(3, 20, 17, 12, 8, g)
    k = rand_kernels(8, 25, g)
    L, Hh = run_synth(pool, par, k, sf, 12)
    want_H = crops(pool, par, 12)
    assert torch.equal(Hh, want_H)
    err = (L.double() - ref_blur(want_H, k, sf)).abs().max().item()
    print(f"PS 12 sf {sf}: max err {err:.3e}")
    assert err < TOL
    Ld, Hd = run_synth(pool, par, k, sf, 12, direct=True)
    assert torch.equal(Ld, L) and torch.equal(Hd, Hh)   # the fallback kernel: the same fmaf chain


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("sf", [1, 2, 3, 4])
def test_blur_ps96(sf, C):
    g = torch.Generator().manual_seed(40 + sf + 10 * C)
    pool = torch.rand(2, C, 110, 128, generator=g)
    par = rand_params(2, 110, 128, 96, 4, g, mode0=2 * sf + C)
    k = rand_kernels(4, 25, g)
    L, Hh = run_synth(pool, par, k, sf, 96)
    want_H = crops(pool, par, 96)
    assert torch.equal(Hh, want_H)
    err = (L.double() - ref_blur(want_H, k, sf)).abs().max().item()
    print(f"PS 96 sf {sf} C {C}: max err {err:.3e}")
    assert err < TOL


def test_blur_ps512_sf4_banded():
    """The C3 width: 536-column bands staged in LDS."""
    g = torch.Generator().manual_seed(60)
    pool = torch.rand(2, 3, 520, 530, generator=g)
    par = torch.tensor([[1, 8, 18, 5], [0, 3, 0, 2]], dtype=torch.int32)
    k = rand_kernels(2, 25, g)
    L, Hh = run_synth(pool, par, k, 4, 512)
    want_H = crops(pool, par, 512)
    assert torch.equal(Hh, want_H)
    err = (L.double() - ref_blur(want_H, k, 4)).abs().max().item()
    print(f"PS 512 sf 4: max err {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("sf,PS,B", [(1, 48, 90), (4, 96, 30)])
def test_blur_multi_row_bands(sf, PS, B):
    """A batch large enough that a band holds several L rows and a thread several outputs (B C > 2048 / rows):
    bit-equal to the one-thread-per-output kernel on every sample, and within the bound on the first and last."""
    g = torch.Generator().manual_seed(70 + sf)
    pool = torch.rand(4, 3, PS + 9, PS + 2, generator=g)
    par = rand_params(4, PS + 9, PS + 2, PS, B, g)
    k = rand_kernels(B, 25, g)
    L, Hh = run_synth(pool, par, k, sf, PS)
    Ld, Hd = run_synth(pool, par, k, sf, PS, direct=True)
    assert torch.equal(L, Ld) and torch.equal(Hh, Hd)
    sel = [0, 1, B - 2, B - 1]
    want_H = crops(pool, par[sel], PS)
    assert torch.equal(Hh[sel], want_H)
    assert (L[sel].double() - ref_blur(want_H, k[sel], sf)).abs().max() < TOL


@pytest.mark.parametrize("sf", [1, 2, 3, 4])
def test_delta_kernel_is_decimation(sf):
    g = torch.Generator().manual_seed(80)
    pool = torch.rand(2, 3, 30, 26, generator=g)
    par = rand_params(2, 30, 26, 24, 8, g)
    k = torch.zeros(8, 1, 25, 25)
    k[:, :, 12, 12] = 1.0
    L, Hh = run_synth(pool, par, k, sf, 24)
    assert torch.equal(L, Hh[..., ::sf, ::sf])


# ---- 3. the centring USRNet's data step assumes ------------------------------------------------------------------
def p2o(psf, shape):
    """utils_sisr.p2o: zero-pad the kernel to the image, roll its centre tap to (0, 0), fft2."""
    kh, kw = psf.shape[-2:]
    otf = torch.zeros(psf.shape[:-2] + tuple(shape), dtype=psf.dtype)
    otf[..., :kh, :kw] = psf
    return torch.fft.fft2(torch.roll(otf, (-(kh // 2), -(kw // 2)), dims=(-2, -1)))


@pytest.mark.parametrize("sf", [3, 4])
def test_forward_model_matches_p2o(sf):
    g = torch.Generator().manual_seed(90 + sf)
    pool = torch.rand(2, 3, 100, 96, generator=g)
    par = rand_params(2, 100, 96, 96, 3, g, mode0=sf)
    k = rand_kernels(3, 25, g)
    L, Hh = run_synth(pool, par, k, sf, 96)
    blurred = torch.fft.ifft2(torch.fft.fft2(Hh.double()) * p2o(k.double(), (96, 96))).real
    assert (L.double() - blurred[..., ::sf, ::sf]).abs().max() < TOL


# ---- 4. uint8 truncation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sf", [1, 3])
def test_trunc8(sf):
    g = torch.Generator().manual_seed(100 + sf)
    pool = torch.rand(2, 3, 60, 64, generator=g)
    par = rand_params(2, 60, 64, 48, 6, g)
    k = rand_kernels(6, 25, g)
    L, Hh = run_synth(pool, par, k, sf, 48, trunc8=True)
    v = 255.0 * L.double()
    assert (v - v.round()).abs().max() < 1e-4
    n = v.round()
    r = 255.0 * ref_blur(Hh, k, sf)
    m = r.round()
    near = (r - m).abs() < 1e-2   # 625 * 2^-24 * 255 = 9.5e-3: the fp32 sum may sit on the other side of an integer
    ok = (n == r.floor()) | (near & ((n == m) | (n == m - 1)))
    assert bool(ok.all()), int((~ok).sum())


# ---- 5. noise ---------------------------------------------------------------------------------------------------
def test_noise_statistics_and_determinism():
    g = torch.Generator().manual_seed(110)
    B = 20
    pool = torch.rand(3, 3, 100, 120, generator=g)
    par = rand_params(3, 100, 120, 96, B, g)
    k = rand_kernels(B, 25, g)
    sigma = torch.tensor([0.0 if b % 5 == 2 else (1 + b) / 255.0 for b in range(B)], dtype=torch.float32)
    L0, _ = run_synth(pool, par, k, 2, 96)
    L, _ = run_synth(pool, par, k, 2, 96, sigma=sigma, seed=5, step=7)
    zero = sigma == 0
    assert int(zero.sum()) == 4 and torch.equal(L[zero], L0[zero])
    n = ((L[~zero] - L0[~zero]).double() / sigma[~zero].double().view(-1, 1, 1, 1)).flatten()
    assert n.numel() >= 100000
    mean, std, m4 = n.mean().item(), n.std().item(), (n ** 4).mean().item()
    print(f"noise: mean {mean:.4f} std {std:.4f} m4 {m4:.4f} max {n.abs().max().item():.2f}")
    assert abs(mean) < 0.01 and abs(std - 1.0) < 0.01 and abs(m4 - 3.0) < 0.1
    L2, _ = run_synth(pool, par, k, 2, 96, sigma=sigma, seed=5, step=7)
    assert torch.equal(L2, L)
    L3, _ = run_synth(pool, par, k, 2, 96, sigma=sigma, seed=5, step=8)
    assert not torch.equal(L3[~zero], L[~zero]) and torch.equal(L3[zero], L0[zero])
    # a per-sample sigma read from a column of a wider table
    tab = torch.zeros(B, 4)
    tab[:, 3] = sigma
    Hp, Lp = torch.empty(B, 3, 96, 96, device=dev), torch.empty(B, 3, 48, 48, device=dev)
    H.synth_usr(pool.to(dev), par.to(dev), B, 96, 2, k.to(dev), tab.to(dev)[:, 3], False, 5, 7, Hp, Lp)
    assert torch.equal(Lp.cpu(), L)


# ---- 6. whole (rectangular) images ------------------------------------------------------------------------------
def test_degrade_rectangular():
    g = torch.Generator().manual_seed(120)
    x = torch.rand(2, 3, 50, 37, generator=g)
    k = rand_kernels(2, 25, g)
    L = sisr.degrade(x.to(dev), k.to(dev), 3).cpu()
    assert L.shape == (2, 3, 17, 13)
    assert (L.double() - ref_blur(x, k, 3)).abs().max() < TOL
    L1 = sisr.degrade(x.to(dev), k[0, 0].to(dev), 3).cpu()   # one kernel for every image
    assert (L1.double() - ref_blur(x, k[:1], 3)).abs().max() < TOL
    # noise and truncation through the function: sigma 0 adds nothing; a tensor of levels is per image
    Ln = sisr.degrade(x.to(dev), k.to(dev), 3, sigma=torch.tensor([0.0, 0.1]), seed=1, step=2).cpu()
    assert torch.equal(Ln[0], L[0]) and 0.05 < (Ln[1] - L[1]).std().item() < 0.15
    Lt = sisr.degrade(x.to(dev), k.to(dev), 3, trunc8=True).cpu().double() * 255
    assert (Lt - Lt.round()).abs().max() < 1e-4 and (Lt / 255 - L.double()).abs().max() < 1 / 255 + 1e-6


@pytest.mark.parametrize("Ws,sf", [(1400, 1), (1600, 1), (1601, 2)])
def test_degrade_wide_rows(Ws, sf):
    """1400 columns: more outputs per band than one pass of a workgroup; 1600: a 25-row band no longer fits in
    LDS and the one-thread-per-output kernel runs."""
    g = torch.Generator().manual_seed(130)
    x = torch.rand(1, 1, 30, Ws, generator=g)
    k = rand_kernels(1, 25, g)
    L = sisr.degrade(x.to(dev), k.to(dev), sf).cpu()
    assert (L.double() - ref_blur(x, k, sf)).abs().max() < TOL
    Ld = torch.empty_like(L, device=dev)
    H.usr_degrade(x.to(dev), k.to(dev), sf, None, False, 0, 0, Ld, direct=True)
    assert torch.equal(Ld.cpu(), L)


# ---- 7. PatchSynth ----------------------------------------------------------------------------------------------
def test_patchsynth_usrnet_rebuild():
    pool = synthetic_pool(5, 3, 64, 80, seed=4)
    g = torch.Generator().manual_seed(140)
    bank = torch.rand(3, 25, 25, generator=g)
    s = PatchSynth(pool, task="usrnet", H_size=48, scales=[1, 2, 3, 4], sigma_max=25, kernel_bank=bank, seed=1)
    cpu = pool.cpu()
    sfs = []
    for _ in range(2):
        d = s.next_dict(8)
        torch.cuda.synchronize()
        noise_step = s.step - 1   # the noise key of this batch
        assert d["sf"].dtype == torch.int64 and d["sf"].shape == (8,) and len(set(d["sf"].tolist())) == 1
        sf = int(d["sf"][0])
        sfs.append(sf)
        par = s.last_params.cpu()
        ints, fl = par[:, :8], par[:, 8:].view(torch.float32)
        L, Hh, k, sigma = d["L"].cpu(), d["H"].cpu(), d["k"].cpu(), d["sigma"].cpu()
        assert L.shape == (8, 3, 48 // sf, 48 // sf) and k.shape == (8, 1, 25, 25) and sigma.shape == (8, 1, 1, 1)
        assert torch.equal(sigma.flatten(), fl[:, 3])
        s255 = sigma.flatten().double() * 255
        assert (s255 - s255.round()).abs().max() < 1e-4 and s255.round().min() >= 0 and s255.round().max() < 25
        want_H = crops(cpu, ints[:, :4], 48)
        assert torch.equal(Hh, want_H)
        for b in range(8):
            src, idx, sf_k, mode_k = ints[b, 4:8].tolist()
            if src:
                want_k = bank[idx].double() / bank[idx].double().sum()
            else:
                want_k = sisr.gen_kernel(25, *fl[b, :3].double().tolist(), sf_k, mode_k)
            assert (k[b, 0].double() - want_k).abs().max() < 1e-6
        # the blur of the rebuilt H with the rebuilt k, then the batch's own noise on top
        L0, _ = run_synth(cpu, ints[:, :4].contiguous(), k, sf, 48)
        assert (L0.double() - ref_blur(want_H, k, sf)).abs().max() < TOL
        Ln, _ = run_synth(cpu, ints[:, :4].contiguous(), k, sf, 48, sigma=fl[:, 3].contiguous(), seed=1,
                          step=noise_step)
        assert torch.equal(Ln, L)
        zero = fl[:, 3] == 0
        assert torch.equal(L[zero], L0[zero])
        tup = s.next(8)
        assert len(tup) == 5 and isinstance(tup[3], int) and tup[0].shape[-1] * tup[3] == 48
    assert sfs[0] != sfs[1]   # seed 1: the two batches draw different scale factors
    assert {0, 1} == set(s.last_params[:, 4].tolist())   # both kernel sources in a batch of 8
    with pytest.raises(ValueError):
        PatchSynth(pool, task="usrnet", H_size=100, scales=[1, 2, 3, 4])
    with pytest.raises(ValueError):
        s.__class__(pool, task="sr", scale=4, H_size=48).next_dict(2)


def test_patchsynth_usrnet_no_bank_trunc8():
    pool = synthetic_pool(3, 1, 40, 40, seed=6)
    s = PatchSynth(pool, task="usrnet", H_size=24, scales=[2], sigma_max=1, trunc8=True, seed=3)
    L, Hh, k, sf, sigma = s.next(16)
    assert sf == 2 and float(sigma.abs().max()) == 0.0   # sigma_max 1: randint(0, 0)
    assert int(s.last_params[:, 4].sum()) == 0           # no bank: every kernel Gaussian
    v = L.double().cpu() * 255
    assert (v - v.round()).abs().max() < 1e-4


# ---- 8. end to end ----------------------------------------------------------------------------------------------
def test_patchsynth_feeds_modelplain4(tmp_path):
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    opt = {"model": "plain4", "is_train": True, "dist": False, "gpu_ids": [0], "scale": 4,
           "path": {"models": str(tmp_path)},
           "netG": {"net_type": "usrnet", "n_iter": 2, "h_nc": 32, "in_nc": 4, "out_nc": 3, "nc": [16, 32, 64, 64],
                    "nb": 2, "act_mode": "R", "downsample_mode": "strideconv", "upsample_mode": "convtranspose",
                    "init_type": "orthogonal", "init_bn_type": "uniform", "init_gain": 0.2},
           "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                     "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                     "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                     "G_scheduler_gamma": 0.5, "E_decay": 0, "G_param_strict": True, "E_param_strict": True}}
    model = define_Model(dict_to_nonedict(opt))
    model.init_train()
    pool = synthetic_pool(4, 3, 64, 64, seed=8)
    s = PatchSynth(pool, task="usrnet", H_size=48, seed=7)
    before = {k: v.detach().clone() for k, v in model.netG.state_dict().items()}
    losses, sfs, step = [], [], 0
    for _ in range(2):
        data = s.next_dict(2)
        sfs.append(int(data["sf"][0]))
        for _ in range(3):   # the third step on a batch shape records and replays the graph
            model.feed_data(data)
            model.optimize_parameters(step)
            losses.append(model.log_dict["G_loss"])
            step += 1
        assert model.sf == sfs[-1] and model.trainer is not None and model.trainer.graph is not None
    assert sfs[0] != sfs[1]   # seed 7: sf 3 then sf 4, so the second batch re-records
    assert all(torch.isfinite(torch.tensor(losses)))
    after = model.netG.state_dict()
    assert any((after[k] - before[k]).abs().max() > 0 for k in before)
