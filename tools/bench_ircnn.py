"""IRCNN (gray, nc 64) training at the option file's shape (B 64, 40-px patches, sigma 25), one-image evaluation, and the
dilated conv kernel against the generic dilated im2col GEMM.

    python tools/bench_ircnn.py [--batch 64] [--ps 40] [--steps 20] [--rounds 3] [--out profiles/ircnn_bench.txt]

(1) The fused, graph-captured training step (FusedTrainer: L1, Adam, EMA) with a fresh PatchSynth(task="dn") batch every
step, on the fp32 engine, the bf16 engine with kair_conv3x3_dil (dil_kernel on) and without it (off), and the same module
list on plain torch (nn.Conv2d with dilation / ReLU, fp32: MIOpen; L1Loss, torch.optim.Adam, no EMA) on the same batches:
alternating rounds, the median of the rounds is reported.  (2) Eval milliseconds for one 1 x 1 x 256 x 256 image, the
same four.  (3) Per dilation 2 / 3 / 4, the forward of one 64 -> 64 layer (bias + ReLU, bf16 rows) at the training
shape's M = B ps^2 on kair_conv3x3_dil and on kair_gemm_nt over H.im2col(dil=), between HIP events, alternating.  One
JSON line per run, then one summary line; everything is also written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kair_amd import _hip as H  # noqa: E402
from kair_amd.data.gpu_synth import PatchSynth, synthetic_pool  # noqa: E402
from kair_amd.engine.trainer import FusedTrainer  # noqa: E402
from kair_amd.models.network_dncnn import IRCNN, IRCNN_DILATIONS  # noqa: E402


def event_us(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def torch_modules(C, nc):
    mods = []
    for li, d in enumerate(IRCNN_DILATIONS):
        last = li == len(IRCNN_DILATIONS) - 1
        mods.append(nn.Conv2d(C if li == 0 else nc, C if last else nc, 3, 1, padding=d, dilation=d))
        if not last:
            mods.append(nn.ReLU(inplace=True))
    return nn.Sequential(*mods)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ps", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join("profiles", "ircnn_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, PS, C, nc = a.batch, a.ps, 1, 64
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    # (3) one dilated layer: the new kernel against the generic path, alternating rounds
    M, K = B * PS * PS, 9 * nc
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, nc, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(nc, nc, 3, 3, generator=g) * 0.05).to(dev)
    bias = torch.zeros(nc, device=dev)
    W15 = torch.empty(nc * 2 * 9 * nc, device=dev, dtype=torch.bfloat16)
    H.pack_weight(w, W15, H.wmap(15, nc, nc, (1, nc, nc), (1, nc, nc)))
    W1 = torch.empty(nc, K, device=dev, dtype=torch.bfloat16)
    H.pack_weight(w, W1, H.wmap(1, nc, nc, (1, nc, nc), (1, nc, nc)))
    out = torch.empty(M, nc, device=dev, dtype=torch.bfloat16)
    layer = {}
    for d in (2, 3, 4):
        fast = lambda d=d: H.conv3x3_dil(x, nc, d, False, W15, 15, bias, out, B, PS, PS, nc, nc, act=H.ACT_RELU)   # noqa: E731
        gen = lambda d=d: H.gemm_nt(H.im2col(x, PS, PS, nc, dil=d), H.rows(W1),                                    # noqa: E731
                                    H.epilogue(out, bias=bias, act=H.ACT_RELU), M, nc, K, H.BF16)
        tf, tg = [], []
        for _ in range(a.rounds):
            tf.append(event_us(fast, a.reps))
            tg.append(event_us(gen, a.reps))
        layer[d] = (statistics.median(tf), statistics.median(tg))
        emit({"layer_forward": {"dil": d, "B": B, "H": PS, "W": PS, "C": nc, "N": nc}, "conv3x3_dil_us": round(layer[d][0], 2),
              "gemm_nt_im2col_dil_us": round(layer[d][1], 2), "generic_over_dil_kernel": round(layer[d][1] / layer[d][0], 3)})

    # (1) training
    pool = synthetic_pool(64, C, PS + 64, PS + 64, seed=99, device=dev)
    synth = PatchSynth(pool, task="dn", H_size=PS, sigma=25, seed=1000)
    steppers, evals = {}, {}
    for name, dt, dk in (("fp32", "fp32", True), ("bf16_dil_kernel", "bf16", True), ("bf16_generic", "bf16", False)):
        torch.manual_seed(0)
        mk = lambda: IRCNN(C, C, nc, compute_dtype=dt).set_dil_kernel(dk).to(dev)   # noqa: E731
        net, ema = mk().train(), mk().eval()
        ema.load_state_dict(net.state_dict())
        tr = FusedTrainer(net, ema, lr=1e-4, E_decay=0.999, use_graph=True)
        steppers[name] = lambda tr=tr: tr.step(*synth.next(B))
        evals[name] = mk().eval()
    torch.manual_seed(0)
    ref = torch_modules(C, nc).to(dev).train()
    adam = torch.optim.Adam(ref.parameters(), lr=1e-4)

    def torch_step():
        Lb, Hb = synth.next(B)
        adam.zero_grad(set_to_none=True)
        loss = ((Lb - ref(Lb)) - Hb).abs().mean()
        loss.backward()
        adam.step()
        return loss

    steppers["torch_fp32"] = torch_step
    for fn in steppers.values():
        for _ in range(4):   # two eager steps, the capture, one replay (torch: MIOpen's algorithm search)
            fn()
    torch.cuda.synchronize()
    runs = {name: [] for name in steppers}
    for r in range(a.rounds):
        for name, fn in steppers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / a.steps * 1e3
            runs[name].append(ms)
            emit({"round": r, "step": name, "ms_per_step": round(ms, 3), "patches_per_s": round(B / ms * 1e3, 1),
                  "loss": round(float(loss), 6)})
    med = {name: statistics.median(v) for name, v in runs.items()}

    # (2) one 256 x 256 image
    img = torch.rand(1, C, 256, 256, device=dev)
    tnet = torch_modules(C, nc).to(dev).eval()
    evals["torch_fp32"] = lambda t: t - tnet(t)
    ev = {name: [] for name in evals}
    with torch.no_grad():
        for r in range(a.rounds):
            for name, fn in evals.items():
                ev[name].append(event_us(lambda: fn(img), 20) / 1e3)
    evm = {name: round(statistics.median(v), 4) for name, v in ev.items()}
    emit({"median_ms_per_step": {n: round(m, 3) for n, m in med.items()},
          "median_patches_per_s": {n: round(B / m * 1e3, 1) for n, m in med.items()},
          "fp32_over_torch_fp32": round(med["torch_fp32"] / med["fp32"], 3),
          "bf16_dil_kernel_over_torch_fp32": round(med["torch_fp32"] / med["bf16_dil_kernel"], 3),
          "bf16_dil_kernel_over_bf16_generic": round(med["bf16_generic"] / med["bf16_dil_kernel"], 3),
          "eval_ms_1x1x256x256": evm,
          "layer_forward_generic_over_dil_kernel": {str(d): round(t[1] / t[0], 3) for d, t in layer.items()}})
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
