"""JPEG CAR batch synthesis at the training shape beside the SwinIR JPEG step it feeds.

    python tools/bench_jpeg_synth.py [--batch 8] [--ps 126] [--quality 40] [--reps 40] [--no-step] [--dtype fp32x3]

Device time of one batch (kair_synth_jpeg: (PS + 8)^2 crop, augment, uint8 / gray conversion, JPEG round trip, second
crop) between two HIP events over `reps` launches after warm-up, gray (the reference's configuration) and colour; the
wall time of PatchSynth.next (host draws included); the whole-image round trip (kair_jpeg_roundtrip) of the same
pixels; and the swinir_jpeg step of tools/bench_models.py (B 8, gray 126 px, window 7) in the same process.  One JSON
line; not pass / fail."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kair_amd import _hip as H  # noqa: E402
from kair_amd.data.gpu_synth import PatchSynth, synthetic_pool  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ps", type=int, default=126)
    ap.add_argument("--quality", type=int, default=40)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--dtype", default="fp32x3", help="engine of the training step")
    ap.add_argument("--no-step", action="store_true", help="skip the swinir_jpeg training step")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, PS = a.batch, a.ps
    pool = synthetic_pool(16, 3, PS + 72, PS + 72, seed=99, device=dev)
    out = {"shape": {"B": B, "PS": PS, "quality": a.quality}}
    for color in (False, True):
        s = PatchSynth(pool, task="jpeg", H_size=PS, quality_factor=a.quality, is_color=color, seed=1000)
        Lp, Hp = s.next(B)
        par = s.last_params
        key = "color" if color else "gray"
        out[f"synth_{key}_us"] = round(event_us(lambda: H.synth_jpeg(s.pool, par, B, PS, color, Hp, Lp), a.reps), 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            s.next(B)
        torch.cuda.synchronize()
        out[f"next_{key}_wall_us"] = round((time.perf_counter() - t0) / a.reps * 1e6, 1)
        x = pool[:B, :3 if color else 1, :PS + 8, :PS + 8].contiguous()
        q = torch.full((1,), a.quality, dtype=torch.int32, device=dev)
        y = torch.empty_like(x)
        out[f"roundtrip_{key}_us"] = round(event_us(lambda: H.jpeg_roundtrip(x, q, y), a.reps), 1)
    if not a.no_step:
        import bench_models
        Bs, dt, loss = bench_models.run("swinir_jpeg", 10, 4, dev, a.dtype)
        out["swinir_jpeg_step_ms"] = round(dt * 1e3, 3)
        out["step_dtype"] = a.dtype
        out["synth_gray_share_of_step"] = round(out["synth_gray_us"] / (dt * 1e6), 6)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
