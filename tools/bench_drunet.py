"""DRUNet training at the reference option file's shape (gray: in_nc 2, out_nc 1, nc 64/128/256/512, nb 4; B 64,
128-px patches), fed by the on-device noise-map synthesis.

    python tools/bench_drunet.py [--batch 64] [--ps 128] [--steps 6] [--rounds 3] [--dtypes fp32,fp32x3,bf16]

Times (1) the synthesis launch alone (kair_synth_dn_map: crop, augment, per-sample AWGN, map channel) between two HIP
events, and the wall time of PatchSynth.next with its host draws; (2) the fused, graph-captured training step
(FusedTrainer: L1, Adam, EMA) with a fresh synthesised batch every step, for each compute dtype.  The dtypes are run
in alternating rounds (fp32, fp32x3, bf16, fp32, ...) and the median of the rounds is reported, so a drift of the
machine does not favour one of them.  One JSON line per run, then one summary line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kair_amd import _hip as H  # noqa: E402
from kair_amd.data.gpu_synth import PatchSynth, synthetic_pool  # noqa: E402
from kair_amd.engine.trainer import FusedTrainer  # noqa: E402
from kair_amd.models.network_unet import UNetRes  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ps", type=int, default=128)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--dtypes", default="fp32,fp32x3,bf16")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, PS, C = a.batch, a.ps, a.channels
    pool = synthetic_pool(64, C, PS + 64, PS + 64, seed=99, device=dev)
    synth = PatchSynth(pool, task="fdncnn", H_size=PS, sigma=(0, 50), seed=1000)
    L, Hh = synth.next(B)
    par = synth.last_params
    out = {"shape": {"B": B, "C": C, "PS": PS, "nc": [64, 128, 256, 512], "nb": 4},
           "synth_us": round(event_us(lambda: H.synth_dn_map(synth.pool, par, B, PS, 1000, 1, Hh, L), a.reps), 2)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        synth.next(B)
    torch.cuda.synchronize()
    out["next_wall_us"] = round((time.perf_counter() - t0) / a.reps * 1e6, 1)
    print(json.dumps(out), flush=True)

    dtypes = [d for d in a.dtypes.split(",") if d]
    trainers = {}
    for dt in dtypes:
        torch.manual_seed(0)
        mk = lambda: UNetRes(C + 1, C, (64, 128, 256, 512), 4, compute_dtype=dt).to(dev)   # noqa: E731
        net, ema = mk().train(), mk().eval()
        ema.load_state_dict(net.state_dict())
        tr = FusedTrainer(net, ema, lr=1e-4, E_decay=0.999, use_graph=True)
        for _ in range(4):   # two eager steps, the capture, one replay
            loss = tr.step(*synth.next(B))
        tr.check_range()
        torch.cuda.synchronize()
        trainers[dt] = tr
    runs = {dt: [] for dt in dtypes}
    for r in range(a.rounds):
        for dt in dtypes:
            tr = trainers[dt]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = tr.step(*synth.next(B))
            tr.check_range()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / a.steps * 1e3
            runs[dt].append(ms)
            print(json.dumps({"round": r, "dtype": dt, "ms_per_step": round(ms, 3), "patches_per_s": round(B / ms * 1e3, 2),
                              "loss": round(loss.item(), 6), "range_events": len(tr.range_events)}), flush=True)
    med = {dt: statistics.median(v) for dt, v in runs.items()}
    summary = {"median_ms_per_step": {dt: round(m, 3) for dt, m in med.items()},
               "median_patches_per_s": {dt: round(B / m * 1e3, 2) for dt, m in med.items()},
               "synth_share_of_step": {dt: round(out["synth_us"] / (m * 1e3), 6) for dt, m in med.items()}}
    if "fp32" in med and "fp32x3" in med:
        summary["fp32x3_over_fp32"] = round(med["fp32"] / med["fp32x3"], 3)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
