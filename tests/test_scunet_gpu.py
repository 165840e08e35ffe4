"""SCUNet on the MI355X (kair_amd/engine/scunet_engine.py) against RefSCUNet, the float64 plain-torch reference of
tests/test_scunet_cpu.py, loaded with load_state_dict(strict=True) from the kair_amd module's state_dict().

Every case uses dim = 64 (the smallest dim head dim 32 allows) and config = [2] * 7, so each level has one 'W' and one
'SW' block at 1 / 2 / 4 / 8 heads.  Tolerances are the ones tests/test_drunet_gpu.py holds for the shared skeleton:
fp32 -- output within 1e-4 relative (L2), every parameter gradient within 5e-3 and their mean within 1e-3; bf16 -- 2e-2 /
0.2 / 5e-2.  The input gradient passes through the same chain as the head conv's weight gradient and is held to the
single-gradient bar (5e-3 / 0.2).  The fused ModelPlain step is held to test_drunet_gpu.py's trainer bars: loss within
1e-4 relative per step, netG and netE parameters within 1e-4 relative (1e-3 for vectors).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from test_scunet_cpu import RefSCUNet, ref_of  # noqa: E402

from kair_amd.models.network_scunet import SCUNet  # noqa: E402

dev = torch.device("cuda")
TOL = {"fp32": (1e-4, 5e-3, 1e-3), "bf16": (2e-2, 0.2, 5e-2)}   # out, worst grad, mean grad


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


CASES = {
    # window grids 8x8, 4x4, 2x2, 1x1: the body level is one shifted window holding all four mask regions
    "A": dict(B=1, in_nc=3, hw=(64, 64), res=256),
    # pads to 64 x 128: non-square, both pads non-zero, one window in height at the body level
    "B": dict(B=2, in_nc=1, hw=(40, 72), res=256),
    # input_resolution 64: the body Blocks are forced to 'W'
    "C": dict(B=1, in_nc=3, hw=(64, 64), res=64),
}
CONFIG = [2] * 7


def randomized(net, seed):
    """Parameters away from their initial values (zero biases, unit LayerNorm weights, tiny tables), so that every
    gradient path carries signal."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("relative_position_params"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif "ln" in n and n.endswith("weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 2:   # the Linears: trunc_normal(0.02) leaves the transformer branch nearly silent
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p.shape[1]) ** 0.5)
    return net


KINK = 2e-7   # see case_ref
DRAW = {"A": 9, "B": 10, "C": 0}   # the first draw index of each case whose reference keeps KINK (case_ref)


def _min_relu_preact(ref, x):
    """Smallest |pre-activation| over every conv-branch ReLU of one float64 forward (forward hooks on conv_block.0)."""
    lo, hooks = [], []
    for nm, m in ref.named_modules():
        if nm.endswith("conv_block.0"):
            hooks.append(m.register_forward_hook(lambda m, i, o: lo.append(o.detach().abs().min().item())))
    with torch.no_grad():
        ref(x)
    for h in hooks:
        h.remove()
    return min(lo)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(state_dict, x, R, float64 output, float64 parameter gradients, float64 input gradient): computed once.

    ReLU' is discontinuous: where a conv-branch pre-activation lies within fp32 rounding of 0, the exact-fp32 engine and
    float64 may legitimately take different sides, and that one flipped element moves its conv's weight gradient by
    percents (measured on the first draw of case B: one element of 131072 in m_up3.2 at pre = 6.1e-8, engine 9.9e-8,
    m_up3.2.conv_block.0.weight 1.2e-2 off, every other gradient within 5e-4).  The comparison is only defined away from
    the kinks, so each case uses a pinned input draw (DRAW: the first seed index, searched once, at which the float64
    reference has no such pre-activation within KINK; asserted here, not searched) with
    KINK = 2e-7 of 0: fp32's 6e-8 relative rounding over the ~sqrt(9C) <= 48 effective terms of a pre-activation whose
    products are of order 0.05 gives ~1.5e-7 (every draw has elements within 1e-7 of 0, so a wider margin leaves no
    draw; a dozen draws reach 2e-7 for each case).  A property of the reference alone; the bars are unchanged."""
    c = CASES[name]
    torch.manual_seed(100 + ord(name))
    net = randomized(SCUNet(c["in_nc"], CONFIG, 64, 0.0, c["res"]), 200 + ord(name))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ref = ref_of(net)
    g = torch.Generator().manual_seed(300 + ord(name) + 1000 * DRAW[name])
    x = torch.rand(c["B"], c["in_nc"], *c["hw"], generator=g)
    lo = _min_relu_preact(ref, x.double())
    assert lo > KINK, f"case {name}: a reference ReLU pre-activation at {lo:.2e}; pin another draw"
    xd = x.double().requires_grad_(True)
    out = ref(xd)
    R = torch.randn(out.shape, generator=g)
    (out * R.double()).sum().backward()
    return sd, x, R, out.detach(), {n: p.grad.clone() for n, p in ref.named_parameters()}, xd.grad.clone()


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_vs_float64(name, dt):
    c = CASES[name]
    sd, x, R, out_ref, grads_ref, gx_ref = case_ref(name)
    net = SCUNet(c["in_nc"], CONFIG, 64, 0.0, c["res"], compute_dtype=dt)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    xg = x.to(dev).requires_grad_(True)
    out = net(xg)
    assert out.shape == out_ref.shape
    e_out = rel(out, out_ref)
    (out * R.to(dev)).sum().backward()
    errs = {n: rel(p.grad, grads_ref[n]) for n, p in net.named_parameters()}
    e_gx = rel(xg.grad, gx_ref)
    mean = sum(errs.values()) / len(errs)
    print(f"{name} {dt}: out {e_out:.3e} worst grad {max(errs.values()):.3e} mean grad {mean:.3e} input grad {e_gx:.3e}")
    assert e_out < TOL[dt][0]
    bad = {k: e for k, e in errs.items() if not e <= TOL[dt][1]}
    assert not bad, bad
    assert mean < TOL[dt][2], sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    assert e_gx < TOL[dt][1]


def test_table_gradient_eight_heads_2x3_windows():
    """relative_position_params.grad in the parameter's [nh][15][15] layout (kair_table_transpose) at nh = 8 on a 2 x 3
    window grid (128 x 192 input: the body level is 16 x 24 tokens), one 'W' and one 'SW' block; the 1 x 1 grid is
    case A's body level."""
    torch.manual_seed(7)
    cfg = [1, 1, 1, 2, 1, 1, 1]
    net = randomized(SCUNet(1, cfg, 64, 0.0, 256), 8)
    ref = ref_of(net)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(1, 1, 128, 192, generator=g)
    out_ref = ref(x.double())
    R = torch.randn(out_ref.shape, generator=g)
    (out_ref * R.double()).sum().backward()
    net = net.to(dev).train()
    out = net(x.to(dev))
    (out * R.to(dev)).sum().backward()
    assert rel(out, out_ref) < TOL["fp32"][0]
    want = dict(ref.named_parameters())
    for i in (0, 1):
        key = f"m_body.{i}.trans_block.msa.relative_position_params"
        got = dict(net.named_parameters())[key].grad
        assert got.shape == (8, 15, 15)
        e = rel(got, want[key].grad)
        print(key, f"{e:.3e}")
        assert e < TOL["fp32"][1], key
    for key in ("m_down1.0.trans_block.msa.relative_position_params",          # one head: written without a transpose
                "m_down2.0.trans_block.msa.embedding_layer.bias"):           # kair_qkvblk_colsum at two heads
        assert rel(dict(net.named_parameters())[key].grad, want[key].grad) < TOL["fp32"][1], key


def test_table_gradient_eight_heads_1x1_window():
    """The same at a 1 x 1 window grid: case A's body level (8 x 8 tokens, nh = 8; block 1 is 'SW', so its one window
    holds all four mask regions), asserted on the two tables by name."""
    c = CASES["A"]
    sd, x, R, out_ref, grads_ref, _ = case_ref("A")
    net = SCUNet(c["in_nc"], CONFIG, 64, 0.0, c["res"])
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    (net(x.to(dev)) * R.to(dev)).sum().backward()
    assert [b.trans_block.type for b in net.m_body] == ["W", "SW"]
    for i in (0, 1):
        key = f"m_body.{i}.trans_block.msa.relative_position_params"
        got = dict(net.named_parameters())[key].grad
        assert got.shape == (8, 15, 15)
        e = rel(got, grads_ref[key])
        print(key, f"{e:.3e}")
        assert e < TOL["fp32"][1], key


def _opt(use_graph):
    return {"model": "plain", "is_train": True, "dist": False, "gpu_ids": [0], "scale": 1, "path": {"models": "/tmp/k"},
            "netG": {"net_type": "scunet", "in_nc": 3, "config": CONFIG, "dim": 64, "drop_path_rate": 0.0,
                     "input_resolution": 256, "init_type": "default"},
            "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                      "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                      "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [100],
                      "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True,
                      "use_hip_graph": use_graph}}


def test_modelplain_steps_vs_float64_adam_and_graph_equals_eager():
    """define_Model('plain') trains SCUNet on FusedTrainer: four steps (L1, Adam, EMA 0.999) on case A's shape against
    RefSCUNet under torch.optim.Adam with the same EMA; the graph-captured and the eager step are bit-equal."""
    from kair_amd.engine.trainer import FusedTrainer
    from kair_amd.models.select_model import define_Model
    from kair_amd.utils.utils_option import dict_to_nonedict
    models = []
    for use_graph in (True, False):
        torch.manual_seed(51)
        m = define_Model(dict_to_nonedict(_opt(use_graph)))
        m.init_train()
        assert isinstance(m.trainer, FusedTrainer) and m.trainer.engine.tdt == torch.float32
        models.append(m)
    ref, ref_e = (ref_of(models[0].netG) for _ in range(2))
    adam = torch.optim.Adam(ref.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    g = torch.Generator().manual_seed(52)
    for step in range(4):
        L, Hh = torch.rand(1, 3, 64, 64, generator=g), torch.rand(1, 3, 64, 64, generator=g)
        for m in models:
            m.feed_data({"L": L, "H": Hh})
            m.optimize_parameters(step)
        adam.zero_grad()
        lo = (ref(L.double()) - Hh.double()).abs().mean()
        lo.backward()
        adam.step()
        with torch.no_grad():
            for pe, pg in zip(ref_e.parameters(), ref.parameters()):
                pe.mul_(0.999).add_(pg, alpha=1 - 0.999)
        loss = models[0].log_dict["G_loss"]
        print(step, loss, lo.item())
        assert abs(loss - lo.item()) < 1e-4 * abs(lo.item()), (step, loss, lo.item())
        assert models[1].log_dict["G_loss"] == loss
    assert models[0].trainer.graph is not None and models[1].trainer.graph is None
    for mine, theirs in ((models[0].netG, ref), (models[0].netE, ref_e)):
        sd, sdr = mine.state_dict(), theirs.state_dict()
        assert list(sd) == list(sdr)
        for key in sdr:
            assert rel(sd[key], sdr[key]) < (1e-3 if sdr[key].dim() == 1 else 1e-4), key
    for a, b in ((models[0].netG, models[1].netG), (models[0].netE, models[1].netE)):
        for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
            assert torch.equal(va, vb), k


def test_segmented_graphs_match_the_single_graph():
    """One graph per gradient segment (grad_segments: the multi-GPU capture) gives the single graph's parameters."""
    from kair_amd.engine.trainer import FusedTrainer
    nets = []
    g = torch.Generator().manual_seed(77)
    L, Hh = torch.rand(1, 3, 64, 64, generator=g).to(dev), torch.rand(1, 3, 64, 64, generator=g).to(dev)
    for seg in (False, True):
        torch.manual_seed(76)
        net = randomized(SCUNet(3, [1] * 7, 64), 78).to(dev).train()
        tr = FusedTrainer(net, None, lr=1e-4, use_graph=True, segment_graphs=seg)
        for _ in range(4):
            tr.step(L, Hh)
        torch.cuda.synchronize()
        if seg:
            assert tr.graph is not None and len(tr.graph[0]) == 7
        nets.append(net)
    for (k, va), vb in zip(nets[0].state_dict().items(), nets[1].state_dict().values()):
        assert torch.equal(va, vb), k


def test_load_state_dict_round_trip_and_x8():
    """Weights loaded from a RefSCUNet state_dict; test_x8 on a 50 x 70 image (the pad to 64 is the network's own, at
    both orientations)."""
    from kair_amd.utils.utils_model import test_x8
    torch.manual_seed(91)
    src = RefSCUNet(3, [1] * 7, 64, 256)
    net = SCUNet(3, [1] * 7, 64, 0.0, 256)
    net.load_state_dict(src.state_dict(), strict=True)
    ref = src.double()
    net = net.to(dev).eval()
    x = torch.rand(1, 3, 50, 70, generator=torch.Generator().manual_seed(92))
    with torch.no_grad():
        E = test_x8(net, x.to(dev))
        want = test_x8(ref, x.double())
        assert E.shape == (1, 3, 50, 70)
        assert rel(E, want) < TOL["fp32"][0]
        assert rel(net(x.to(dev)), ref(x.double())) < TOL["fp32"][0]
    # eval and training plans compute the same forward
    a = net(x.to(dev).requires_grad_(True))
    with torch.no_grad():
        assert torch.equal(a.detach(), net(x.to(dev)))


def test_input_checks():
    net = SCUNet(3, [1] * 7, 64).to(dev)
    with pytest.raises(ValueError, match="channels"):
        net(torch.rand(1, 1, 64, 64, device=dev))
    with pytest.raises(RuntimeError):
        net(torch.rand(1, 3, 64, 64))


def _write_rgb(d, n, size, seed):
    import os
    import numpy as np
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    rs = np.random.RandomState(seed)
    for i in range(n):
        img = np.kron(rs.rand(size // 8, size // 8, 3), np.ones((8, 8, 1))) + 0.03 * rs.randn(size, size, 3)
        Image.fromarray(np.uint8(np.clip(img, 0, 1) * 255)).save(os.path.join(d, f"im{i}.png"))


def test_option_file_trains_20_steps_and_test_driver_restores_a_folder(tmp_path):
    """options/train_scunet.json through main_train_psnr on the fused trainer for 20 steps (the file's network and patch
    size, batch 2, generated images), then main_test_scunet on a folder with the checkpoint it saved."""
    import os
    from kair_amd.engine.trainer import FusedTrainer
    from kair_amd.main_test_scunet import main as test_main
    from kair_amd.main_train_psnr import main
    tmp = str(tmp_path)
    tr_dir, te_dir = os.path.join(tmp, "trainH"), os.path.join(tmp, "testH")
    _write_rgb(tr_dir, 4, 160, 0)
    _write_rgb(te_dir, 2, 72, 1)

    def over(opt):
        task = os.path.join(tmp, opt["task"])
        opt["gpu_ids"] = [0]
        opt["path"].update(root=tmp, models=os.path.join(task, "models"), options=os.path.join(task, "options"),
                           log=task, task=task, images=os.path.join(task, "images"))
        d = opt["datasets"]["train"]
        d["dataroot_H"], d["dataloader_batch_size"], d["dataloader_num_workers"] = tr_dir, 2, 0
        opt["datasets"]["test"]["dataroot_H"] = te_dir
        opt["train"].update(max_iter=20, checkpoint_test=20, checkpoint_save=20, checkpoint_print=5, manual_seed=0)

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model, hist = main(os.path.join(root, "options", "train_scunet.json"), over)
    assert isinstance(model.trainer, FusedTrainer) and model.trainer.graph is not None
    assert model.opt["netG"]["config"] == [4] * 7 and model.opt["datasets"]["train"]["H_size"] == 128
    assert len(hist["loss"]) == 20 and all(torch.isfinite(torch.tensor(hist["loss"])))
    ckpt = os.path.join(tmp, "scunet_color_25", "models", "20_G.pth")
    assert os.path.exists(ckpt)
    out = test_main(["--model_path", ckpt, "--input", te_dir, "--noise_level", "25", "--n_channels", "3",
                     "--output", os.path.join(tmp, "restored")])
    assert [n for n, _ in out] == ["im0", "im1"] and all(p is not None and p == p for _, p in out)
    assert sorted(os.listdir(os.path.join(tmp, "restored"))) == ["im0_scunet.png", "im1_scunet.png"]


@pytest.mark.parametrize("name", ["A", "B"])
def test_fused_block_eval_forward_on_and_off(name):
    """bf16 eval forwards with the one-launch Block (kair_scu_block_fwd) on and off at both narrow widths (levels 0 and 1:
    trans_dim 32 and 64, 'W' and 'SW' blocks): each within the bf16 output bar of float64, the pair within twice it."""
    c = CASES[name]
    sd, x, _, out_ref, _, _ = case_ref(name)
    outs = {}
    for fused in (False, True):
        net = SCUNet(c["in_nc"], CONFIG, 64, 0.0, c["res"], compute_dtype="bf16").set_fused_block(fused)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).eval()
        with torch.no_grad():
            outs[fused] = net(x.to(dev)).clone()
        assert net.engine().fused_block == {32: fused, 64: fused}
        e = rel(outs[fused], out_ref)
        print(f"{name} fused {fused}: out {e:.3e}")
        assert e < TOL["bf16"][0]
    pair = rel(outs[True], outs[False])
    print(f"{name} fused vs unfused {pair:.3e}")
    assert pair < 2 * TOL["bf16"][0]
    assert not torch.equal(outs[True], outs[False])   # the switch does select another path


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("C", [32, 64])
def test_scu_block_fwd_kernel_vs_float64_block(C, shift):
    """kair_scu_block_fwd on one level's buffer -- 2 images of 16 x 24 tokens, the trans_x columns of an [M, 2C] buffer,
    written back in place -- against the float64 Block of tests/test_scunet_cpu.py, within the bf16 output bar."""
    from test_scunet_cpu import RefBlock
    from kair_amd import _hip as H
    B, Hh, Ww = 2, 16, 24
    torch.manual_seed(500 + C + shift)
    blk = RefBlock(C, C, 32, 8, "SW" if shift else "W", 256).double()
    g = torch.Generator().manual_seed(600 + C + shift)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if n.endswith("relative_position_params"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif n.startswith("ln") and n.endswith("weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p.shape[1]) ** 0.5)
    x = torch.randn(B, Hh, Ww, C, generator=g)
    with torch.no_grad():
        want = blk(x.double())
    f = lambda t: t.detach().float().to(dev).contiguous()           # noqa: E731
    w = lambda t: t.detach().to(dev, torch.bfloat16).contiguous()   # noqa: E731
    buf = torch.full((B * Hh * Ww, 2 * C), 7.0, device=dev)
    buf[:, C:] = x.view(-1, C).to(dev)
    view = buf[:, C:]
    ln1 = torch.nn.LayerNorm(C).to(dev)
    ln2 = torch.nn.LayerNorm(C).to(dev)
    ln1.load_state_dict({k: f(v) for k, v in blk.ln1.state_dict().items()})
    ln2.load_state_dict({k: f(v) for k, v in blk.ln2.state_dict().items()})
    table = f(blk.msa.relative_position_params.reshape(C // 32, -1).t())       # [(2ws-1)^2][nh]
    H.scu_block_fwd(view, 2 * C, view, 2 * C, ln1, ln2, w(blk.msa.embedding_layer.weight), f(blk.msa.embedding_layer.bias),
                    w(blk.msa.linear.weight), f(blk.msa.linear.bias), w(blk.mlp[0].weight), f(blk.mlp[0].bias),
                    w(blk.mlp[2].weight), f(blk.mlp[2].bias), table, blk.msa.scale, B, Hh, Ww, C, shift)
    torch.cuda.synchronize()
    assert torch.all(buf[:, :C] == 7.0)                                         # the conv columns are untouched
    e = rel(buf[:, C:].reshape(B, Hh, Ww, C), want)
    print(f"C {C} shift {shift}: {e:.3e}")
    assert e < TOL["bf16"][0]
