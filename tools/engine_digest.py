"""Bit-level record of the SwinIR step program, for refactors that must not change what it computes.

    python tools/engine_digest.py [--only SUBSTRING] > digest.txt

One line per case: the case name, SHA-256 of the output E, of the loss and of the flat gradient buffer, then
P["conv_wr"] and (embed 180 cases) the kair_conv3x3_wr tiles of the tail shapes, which say what tail kernels ran.
The step is deterministic (fixed weight-gradient partial planes, deterministic finalize), so two trees that issue
the same launches on the same arguments print the same file; `diff` is the check.  Uses only SwinIR(...),
SwinIREngine(net, dt, side_stream=..., ...), forward, backward_from_loss and backward_from_grad.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for c in cases():
        if a.only in c[0]:
            run(*c, dev)


if __name__ == "__main__":
    main()
