"""USRNet batch synthesis at the C3 shape beside the C3 training step it feeds.

    python tools/bench_usr_synth.py [--batch 48] [--ps 512] [--sf 4] [--reps 40] [--no-step]

Device time of one batch (kair_usr_gauss_kernels + kair_synth_usr: crop, augment, 25x25 circular blur, [0::sf]
decimation, AWGN) between two HIP events over `reps` launches after warm-up, with the banded kernel and with the
one-thread-per-output kernel it falls back to; the wall time of PatchSynth.next (host draws included); and the C3
bf16 step (tools/bench_models.py usrnet: B 48, 128-px LQ, n_iter 6) in the same process.  One JSON line."""
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
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--ps", type=int, default=512)
    ap.add_argument("--sf", type=int, default=4)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--no-step", action="store_true", help="skip the C3 training step")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, PS, sf = a.batch, a.ps, a.sf
    pool = synthetic_pool(16, a.channels, PS + 64, PS + 64, seed=99, device=dev)
    s = PatchSynth(pool, task="usrnet", H_size=PS, scales=[sf], seed=1000)
    s.next(B)
    par = s.last_params
    fl = par[:, 8:].view(torch.float32)
    k = torch.empty(B, 1, 25, 25, device=dev)
    Hp = torch.empty(B, a.channels, PS, PS, device=dev)
    Lp = torch.empty(B, a.channels, PS // sf, PS // sf, device=dev)

    def launch(direct):
        H.usr_gauss_kernels(fl, par[:, 4:8], None, k)
        H.synth_usr(s.pool, par, B, PS, sf, k, fl[:, 3], False, 1000, 1, Hp, Lp, direct=direct)

    out = {"shape": {"B": B, "C": a.channels, "PS": PS, "sf": sf, "taps": 625},
           "synth_us": round(event_us(lambda: launch(False), a.reps), 1),
           "synth_direct_us": round(event_us(lambda: launch(True), max(3, a.reps // 8), warmup=1), 1),
           "kernels_only_us": round(event_us(lambda: H.usr_gauss_kernels(fl, par[:, 4:8], None, k), a.reps), 1)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        s.next(B)
    torch.cuda.synchronize()
    out["next_wall_us"] = round((time.perf_counter() - t0) / a.reps * 1e6, 1)
    if not a.no_step:
        import bench_models
        Bs, dt, loss = bench_models.run_usrnet(10, 4, dev, "bf16")
        out["c3_bf16_step_ms"] = round(dt * 1e3, 3)
        out["synth_share_of_step"] = round(out["synth_us"] / (dt * 1e6), 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
