"""Bit-level record of the step programs, for refactors that must not change what they compute.

    python tools/engine_digest.py [--only SUBSTRING] > digest.txt

One line per case: the case name, SHA-256 of the output E, of the loss and of the flat gradient buffer, then (SwinIR)
P["conv_wr"] and (embed 180 cases) the kair_conv3x3_wr tiles of the tail shapes, which say what tail kernels ran.
The step is deterministic (fixed weight-gradient partial planes, deterministic finalize), so two trees that issue
the same launches on the same arguments print the same file; `diff` is the check.  Uses only SwinIR(...),
SwinIREngine(net, dt, side_stream=..., ...), forward, backward_from_loss and backward_from_grad; the conv.* cases
(RRDBNet, DnCNN, FFDNet, DRUNet, USRNet) the network constructors, net.engine() and the same three engine calls, the
USRNet ones net(x, k, sf, sigma) and .backward() as well.
"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kair_amd import _hip as H  # noqa: E402
from kair_amd.engine.swinir_engine import SwinIREngine  # noqa: E402
from kair_amd.models.network_swinir import SwinIR  # noqa: E402

B = 2
TAILS = [("ps_x2", "pixelshuffle", 2, 3, "1conv"), ("ps_x3", "pixelshuffle", 3, 3, "1conv"),
         ("ps_x4", "pixelshuffle", 4, 3, "1conv"), ("direct_x2", "pixelshuffledirect", 2, 3, "1conv"),
         ("nearest_x4", "nearest+conv", 4, 3, "1conv"), ("none_c1", None, 1, 1, "1conv"), ("plain_3conv", "", 1, 3, "3conv")]
DTYPES = ("bf16", "fp32", "fp32x3")


def sha(t):
    return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def cases():
    """(name, network kwargs, LR side, compute dtype, engine kwargs, conv_wr_min_tiles or None, from_grad)"""
    for tag, ups, sc, ch, resi in TAILS:
        kw = dict(upscale=sc, in_chans=ch, embed_dim=60, upsampler=ups, resi_connection=resi)
        for dt in DTYPES:
            yield f"small.{tag}.{dt}.loss", kw, 16, dt, dict(side_stream=False), None, False
            if tag in ("ps_x2", "direct_x2"):
                yield f"small.{tag}.{dt}.grad", kw, 16, dt, dict(side_stream=False), None, True
    # (x4 at 32 x 32 tiles for no kair_conv3x3_wr form; at 24 x 24 both upsampling stages take the pair form)
    for sc, lr in ((2, 24), (4, 32), (4, 24)):
        kw = dict(upscale=sc, in_chans=3, embed_dim=180, upsampler="pixelshuffle", resi_connection="1conv")
        for dt in ("bf16", "fp32x3"):
            for mt in (0, None):
                yield (f"cp192.ps_x{sc}.lr{lr}.{dt}.min_tiles_{'default' if mt is None else mt}", kw, lr, dt,
                       dict(side_stream=False), mt, False)
    kw = dict(upscale=2, in_chans=3, embed_dim=60, upsampler="pixelshuffle", resi_connection="1conv")
    yield "stream.ps_x2.bf16.default_engine", kw, 16, "bf16", {}, None, False


def run(name, kw, lr, dt, ekw, min_tiles, from_grad, dev):
    torch.manual_seed(1234)
    net = SwinIR(img_size=lr, window_size=8, img_range=1.0, depths=[2, 2], num_heads=[6, 6], mlp_ratio=2,
                 drop_path_rate=0.0, compute_dtype=dt, **kw).to(dev).train()
    g = torch.Generator().manual_seed(99)
    sc, ch = kw["upscale"], kw["in_chans"]
    x = torch.rand(B, ch, lr, lr, generator=g).to(dev)
    tgt = torch.rand(B, ch, lr * sc, lr * sc, generator=g).to(dev)
    eng = SwinIREngine(net, dt, **ekw)
    if min_tiles is not None:
        eng.conv_wr_min_tiles = min_tiles
    params = list(net.parameters())
    flat = torch.zeros(sum(p.numel() for p in params), device=dev)
    grads, off = {}, 0
    for p in params:
        grads[p] = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    E = eng.forward(x)
    hE = sha(E)
    if from_grad:
        eng.backward_from_grad((tgt - 0.5) / tgt.numel(), grads)
        loss = torch.zeros(1)
    else:
        loss = eng.backward_from_loss(tgt, grads)
    torch.cuda.synchronize()
    extra = f"conv_wr={eng.cur.get('conv_wr')}"
    if kw["embed_dim"] == 180:   # forward / input-gradient tiles of conv_before_upsample and each upsampling conv
        Cp, t = eng.Cp, []
        t += [H.conv3x3_wr_tile(1, B, lr, lr, Cp, 64), H.conv3x3_wr_tile(0, B, lr, lr, 64, Cp)]
        for i in range(sc // 2):
            s = lr << i
            t += [H.conv3x3_wr_tile(1, B, s, s, 64, 256), H.conv3x3_wr_tile(0, B, s, s, 256, 64)]
        extra += f" min_tiles={eng.conv_wr_min_tiles} tail_tiles={t} x3_tile={H.conv3x3_wr_x3_tile(B, lr, lr, Cp, Cp)}"
    print(f"{name} E={hE} loss={sha(loss)} grad={sha(flat)} finite={bool(torch.isfinite(flat).all())} {extra}", flush=True)


def _usr_kernel(g):
    k = torch.rand(B, 1, 25, 25, generator=g)
    return k / k.sum((-2, -1), keepdim=True)


def conv_cases():
    """(name, engine class, network factory(compute dtype), input shape, extra forward inputs(generator), modes): the
    conv step programs at the small configurations of their tests, B = 2, run in every dtype the engine implements.
    modes: "loss" (backward_from_loss), "grad" (backward_from_grad), "module" (the nn.Module and .backward(): the
    autograd node)."""
    from kair_amd.engine.dncnn_engine import DnCNNEngine, FFDNetEngine
    from kair_amd.engine.drunet_engine import DRUNetEngine
    from kair_amd.engine.rrdbnet_engine import RRDBNetEngine
    from kair_amd.engine.usrnet_engine import USRNetEngine
    from kair_amd.models.network_dncnn import DnCNN
    from kair_amd.models.network_ffdnet import FFDNet
    from kair_amd.models.network_rrdbnet import RRDBNet
    from kair_amd.models.network_unet import UNetRes
    from kair_amd.models.network_usrnet import USRNet
    none = lambda g: ()
    sigma = lambda g: ((torch.tensor([5.0, 50.0]) / 255).view(B, 1, 1, 1),)
    usr = lambda sf: (lambda g: (_usr_kernel(g), sf, torch.rand(B, 1, 1, 1, generator=g) * (25.0 / 255)))
    usrnet = lambda dt: USRNet(n_iter=2, h_nc=32, in_nc=4, out_nc=3, nc=[16, 32, 64, 64], nb=2, compute_dtype=dt)
    both = ("loss", "grad")
    for sf in (2, 4):
        yield (f"rrdbnet_x{sf}", RRDBNetEngine, (lambda dt, sf=sf: RRDBNet(3, 3, 32, 1, 16, sf, compute_dtype=dt)),
               (B, 3, 12, 12), none, both)
    for tag, act in (("bn", "BR"), ("nobn", "R")):
        yield (f"dncnn_{tag}", DnCNNEngine, (lambda dt, act=act: DnCNN(1, 1, 32, 5, act, compute_dtype=dt)),
               (B, 1, 16, 20), none, both)
    yield ("ffdnet_even", FFDNetEngine, (lambda dt: FFDNet(1, 1, 16, 4, "R", compute_dtype=dt)), (B, 1, 12, 20), sigma,
           both)
    # (an odd size has no fused loss: forward and backward_from_grad)
    yield ("ffdnet_odd", FFDNetEngine, (lambda dt: FFDNet(3, 3, 16, 3, "R", compute_dtype=dt)), (B, 3, 9, 11), sigma,
           ("grad",))
    yield ("drunet", DRUNetEngine, (lambda dt: UNetRes(2, 1, (16, 32, 48, 64), 2, compute_dtype=dt)), (B, 2, 16, 24),
           none, both)
    # USRNet, 2 iterations: sf 2 on a 32 x 32 HR grid; sf 3 at 18 x 18 -> 54 x 54, which needs the replicate pad
    yield "usrnet_sf2", USRNetEngine, usrnet, (B, 3, 16, 16), usr(2), both + ("module",)
    yield "usrnet_pad", USRNetEngine, usrnet, (B, 3, 18, 18), usr(3), both + ("module",)


def run_conv(name, make, shape, cond_of, mode, dt, dev):
    torch.manual_seed(1234)
    net = make(dt).to(dev).train()
    g = torch.Generator().manual_seed(99)
    x = torch.rand(*shape, generator=g).to(dev)
    cond = tuple(c.to(dev) if torch.is_tensor(c) else c for c in cond_of(g))
    params = list(net.parameters())
    if mode == "module":
        E = net(x, *cond)
        hE = sha(E)
        tgt = torch.rand(*E.shape, generator=g).to(dev)
        E.backward((tgt - 0.5) / tgt.numel())
        loss, flat = torch.zeros(1), torch.cat([p.grad.reshape(-1) for p in params])
    else:
        eng = net.engine()
        flat = torch.zeros(sum(p.numel() for p in params), device=dev)
        grads, off = {}, 0
        for p in params:
            grads[p] = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        E = eng.forward(x, *cond)
        hE = sha(E)
        tgt = torch.rand(*E.shape, generator=g).to(dev)
        if mode == "grad":
            eng.backward_from_grad((tgt - 0.5) / tgt.numel(), grads)
            loss = torch.zeros(1)
        else:
            loss = eng.backward_from_loss(tgt, grads)
    torch.cuda.synchronize()
    print(f"conv.{name}.{dt}.{mode} E={hE} loss={sha(loss)} grad={sha(flat)} finite={bool(torch.isfinite(flat).all())}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for c in cases():
        if a.only in c[0]:
            run(*c, dev)
    for name, engine_cls, make, shape, cond_of, modes in conv_cases():
        for dt in engine_cls.COMPUTE_DTYPES:
            for mode in modes:
                if a.only in f"conv.{name}.{dt}.{mode}":
                    run_conv(name, make, shape, cond_of, mode, dt, dev)


if __name__ == "__main__":
    main()
