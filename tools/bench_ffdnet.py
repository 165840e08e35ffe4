"""FFDNet training at the reference option files' shapes (gray: in_nc 1, nc 64, nb 15; colour: in_nc 3, nc 96, nb 12;
B 64, 64-px patches), fed by the on-device synthesis, next to FDnCNN(in_nc + 1, out_nc, same nc, same nb) on the same
engine and patch size.

    python tools/bench_ffdnet.py [--batch 64] [--ps 64] [--steps 20] [--rounds 3] [--dtypes bf16,fp32] [--out FILE]

Times (1) the head kernel alone (kair_ffd_pack, input mode, bf16 and fp32 rows) between two HIP events, with the rate
its algorithmic bytes (the image read once, the packed rows written once) give against the 8.0 TB/s HBM peak; (2) the
fused, graph-captured training step (FusedTrainer: L1, Adam, EMA) with a fresh synthesised batch every step
(PatchSynth task "ffdnet" / "fdncnn").  The (network, dtype) pairs run in alternating rounds and the median of the rounds
is reported, so a drift of the machine does not favour one of them.  One JSON line per run, then one summary line per
variant; --out also writes the lines to a file (profiles/ffdnet_bench.txt is the committed record)."""
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
from kair_amd.models.network_dncnn import FDnCNN  # noqa: E402
from kair_amd.models.network_ffdnet import FFDNet  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s (MI355X HBM3E specification)
VARIANTS = {"gray": (1, 64, 15), "colour": (3, 96, 12)}   # in_nc = out_nc, nc, nb


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
    ap.add_argument("--ps", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--variants", default="gray,colour")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, PS = a.batch, a.ps
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    dtypes = [d for d in a.dtypes.split(",") if d]
    for var in [v for v in a.variants.split(",") if v]:
        C, nc, nb = VARIANTS[var]
        pool = synthetic_pool(64, C, PS + 64, PS + 64, seed=99, device=dev)
        synths = {"ffdnet": PatchSynth(pool, task="ffdnet", H_size=PS, sigma=(0, 75), seed=1000),
                  "fdncnn": PatchSynth(pool, task="fdncnn", H_size=PS, sigma=(0, 75), seed=1000)}
        # (1) the head kernel alone
        L, _, lev = synths["ffdnet"].next(B)
        lev = lev.view(B).contiguous()
        ldc = (4 * C + 1 + 7) // 8 * 8
        M = B * (PS // 2) ** 2
        for dt, size in ((torch.bfloat16, 2), (torch.float32, 4)):
            rows = torch.empty(M, ldc, device=dev, dtype=dt)
            us = event_us(lambda: H.ffd_pack(L, lev, rows, ldc, B, C, PS, PS), a.reps)
            nbytes = L.numel() * 4 + B * 4 + M * ldc * size
            emit({"variant": var, "kernel": "kair_ffd_pack", "rows": str(dt).replace("torch.", ""), "B": B, "C": C, "PS": PS,
                  "ldc": ldc, "us": round(us, 2), "algorithmic_bytes": nbytes,
                  "bytes_per_s": round(nbytes / (us * 1e-6), 0), "share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)})
        # (2) the training step, FFDNet next to FDnCNN
        trainers = {}
        for kind in ("ffdnet", "fdncnn"):
            for dt in dtypes:
                torch.manual_seed(0)
                mk = ((lambda: FFDNet(C, C, nc, nb, "R", compute_dtype=dt).to(dev)) if kind == "ffdnet" else
                      (lambda: FDnCNN(C + 1, C, nc, nb, "R", compute_dtype=dt).to(dev)))
                net, ema = mk().train(), mk().eval()
                ema.load_state_dict(net.state_dict())
                tr = FusedTrainer(net, ema, lr=1e-4, E_decay=0.999, use_graph=True)
                for _ in range(4):   # two eager steps, the capture, one replay
                    tr.step(*synths[kind].next(B))
                torch.cuda.synchronize()
                trainers[kind, dt] = tr
        runs = {k: [] for k in trainers}
        for r in range(a.rounds):
            for (kind, dt), tr in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loss = tr.step(*synths[kind].next(B))
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                runs[kind, dt].append(ms)
                emit({"variant": var, "round": r, "net": kind, "dtype": dt, "ms_per_step": round(ms, 3),
                      "patches_per_s": round(B / ms * 1e3, 1), "loss": round(loss.item(), 6)})
        med = {k: statistics.median(v) for k, v in runs.items()}
        emit({"variant": var, "nc": nc, "nb": nb, "B": B, "PS": PS,
              "median_patches_per_s": {f"{k}.{dt}": round(B / m * 1e3, 1) for (k, dt), m in med.items()},
              "ffdnet_over_fdncnn": {dt: round(med["fdncnn", dt] / med["ffdnet", dt], 3) for dt in dtypes}})
        del trainers
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
