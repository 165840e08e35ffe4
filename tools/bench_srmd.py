"""SRMD x4 training at the option file's shape (in_nc 19, nc 128, nb 12; B 64, 24-px LR / 96-px H patches), fed by the
on-device degradation synthesis.

    python tools/bench_srmd.py [--batch 64] [--ps 96] [--sf 4] [--steps 20] [--rounds 3] [--out profiles/srmd_bench.txt]

Times (1) the two synthesis launches (kair_srmd_kernels; kair_synth_srmd: crop, augment, 15 x 15 circular blur, bicubic
x1/sf, AWGN, map channels) between HIP events, beside task "sr"'s one launch (kair_synth_sr) for the same batch in the
same run -- the blur and the map are the added work -- and the wall time of PatchSynth.next with its host draws; (2)
the fused, graph-captured training step (FusedTrainer: L1, Adam, EMA) with a fresh synthesised batch every step, on the
fp32 and bf16 engines, and the same step with the network run as plain torch modules (nn.Conv2d / ReLU / PixelShuffle,
fp32: MIOpen; L1Loss, torch.optim.Adam, no EMA) on the same batches.  The three are run in alternating rounds and the
median of the rounds is reported.  One JSON line per run, then one summary line; everything is also written to --out."""
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
from kair_amd.models.network_srmd import SRMD  # noqa: E402


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


def torch_modules(in_nc, out_nc, nc, nb, sf):
    mods = [nn.Conv2d(in_nc, nc, 3, 1, 1), nn.ReLU(inplace=True)]
    for _ in range(nb - 2):
        mods += [nn.Conv2d(nc, nc, 3, 1, 1), nn.ReLU(inplace=True)]
    return nn.Sequential(*mods, nn.Conv2d(nc, out_nc * sf * sf, 3, 1, 1), nn.PixelShuffle(sf))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ps", type=int, default=96)
    ap.add_argument("--sf", type=int, default=4)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "srmd_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, PS, sf, C = a.batch, a.ps, a.sf, a.channels
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    pool = synthetic_pool(64, C, PS + 64, PS + 64, seed=99, device=dev)
    synth = PatchSynth(pool, task="srmd", H_size=PS, scale=sf, sigma=(0, 50), seed=1000)
    sr = PatchSynth(pool, task="sr", H_size=PS, scale=sf, seed=1000)
    L, Hh = synth.next(B)
    par, kind = synth.last_params, synth.kind
    fl = par[:, 4:].view(torch.float32)
    k, code = synth.last_kernels, synth.last_codes
    Ls, Hs = sr.next(B)
    spar = sr.last_params
    out = {"shape": {"B": B, "C": C, "PS": PS, "sf": sf, "in_nc": C + 16, "nc": 128, "nb": 12},
           "srmd_kernels_us": round(event_us(lambda: H.srmd_kernels(fl, kind.pca, k, code), a.reps), 2),
           "synth_srmd_us": round(event_us(lambda: H.synth_srmd(synth.pool, par, B, PS, sf, k, code, True, kind.taps, 1000, 1,
                                                               Hh, L, sigma_col=7), a.reps), 2),
           "synth_sr_us": round(event_us(lambda: H.synth_sr(sr.pool, spar, B, PS, sf, sr.kind.taps_h, sr.kind.taps_w, Hs, Ls),
                                         a.reps), 2)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        synth.next(B)
    torch.cuda.synchronize()
    out["next_wall_us"] = round((time.perf_counter() - t0) / a.reps * 1e6, 1)
    emit(out)
    synth_us = out["srmd_kernels_us"] + out["synth_srmd_us"]

    steppers = {}
    for dt in ("fp32", "bf16"):
        torch.manual_seed(0)
        mk = lambda: SRMD(C + 16, C, 128, 12, sf, compute_dtype=dt).to(dev)   # noqa: E731
        net, ema = mk().train(), mk().eval()
        ema.load_state_dict(net.state_dict())
        tr = FusedTrainer(net, ema, lr=1e-4, E_decay=0.999, use_graph=True)
        steppers[dt] = lambda tr=tr: tr.step(*synth.next(B))
    torch.manual_seed(0)
    ref = torch_modules(C + 16, C, 128, 12, sf).to(dev).train()
    adam = torch.optim.Adam(ref.parameters(), lr=1e-4)

    def torch_step():
        Lb, Hb = synth.next(B)
        adam.zero_grad(set_to_none=True)
        loss = (ref(Lb) - Hb).abs().mean()
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
                  "loss": round(loss.item(), 6)})
    med = {name: statistics.median(v) for name, v in runs.items()}
    emit({"median_ms_per_step": {n: round(m, 3) for n, m in med.items()},
          "median_patches_per_s": {n: round(B / m * 1e3, 1) for n, m in med.items()},
          "fp32_over_torch_fp32": round(med["torch_fp32"] / med["fp32"], 3),
          "bf16_over_torch_fp32": round(med["torch_fp32"] / med["bf16"], 3),
          "synth_us": round(synth_us, 2), "synth_over_sr_task": round(synth_us / out["synth_sr_us"], 2),
          "synth_share_of_step": {n: round(synth_us / (m * 1e3), 5) for n, m in med.items()}})
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
