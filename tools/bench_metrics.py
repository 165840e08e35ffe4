"""The on-device evaluation metrics (utils_image.tensor_metrics -> kair_image_metrics) next to the host path they
replace on the training drivers' test phase (.cpu() + tensor2uint + calculate_psnr [+ calculate_ssim]).

    python tools/bench_metrics.py [--rounds 5] [--reps 200] [--host-reps 3] [--out FILE]

Shapes 1x3x512x512 and 1x1x256x256, border 4, with and without SSIM.  The two sides alternate over --rounds rounds and
the medians are reported.  Device side: tensor_metrics on device tensors (the output fill, kair_image_metrics and
kair_psnr_db), --reps calls inside one window closed by a stream synchronise (host clock around the
window; device events over the same window are printed beside it).  Host side: what main_train_dncnn's test phase does
per image, starting from the same device tensors, so the device -> host copies are in it; --host-reps calls.  One JSON
line per round and side, then one summary line per case; --out also writes the lines to a file
(profiles/metrics_bench.txt is the committed record).  The values of both sides are compared in the summary."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kair_amd.utils import utils_image as U  # noqa: E402


def image_pair(shape, dev, seed):
    """A smooth target + noise, and an estimate a little off it, in [0, 1]."""
    B, C, Hh, Ww = shape
    g = torch.Generator(device=dev).manual_seed(seed)
    yy = torch.linspace(0, 1, Hh, device=dev).view(1, 1, Hh, 1)
    xx = torch.linspace(0, 1, Ww, device=dev).view(1, 1, 1, Ww)
    Ht = (0.2 + 0.3 * yy + 0.3 * xx + 0.1 * torch.rand(B, C, Hh, Ww, device=dev, generator=g)).clamp(0, 1)
    E = (Ht + 0.05 * (2 * torch.rand(B, C, Hh, Ww, device=dev, generator=g) - 1)).clamp(0, 1)
    return E.contiguous(), Ht.contiguous()


def device_us(E, Ht, border, ssim, reps):
    """(host-clock us per call over a synchronised window, device-event us per call over the same window, result)."""
    for _ in range(5):
        U.tensor_metrics(E, Ht, border=border, ssim=ssim)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        out = U.tensor_metrics(E, Ht, border=border, ssim=ssim)
    e1.record()
    torch.cuda.current_stream().synchronize()
    t1 = time.perf_counter()
    return (t1 - t0) / reps * 1e6, e0.elapsed_time(e1) / reps * 1e3, out


def host_us(E, Ht, border, ssim, reps):
    """The test phase of main_train_dncnn per image: copy off the device, quantise with numpy, the host functions."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        e, h = U.tensor2uint(E[0].detach().float().cpu()), U.tensor2uint(Ht[0].detach().float().cpu())
        p = U.calculate_psnr(e, h, border=border)
        s = float(U.calculate_ssim(e, h, border=border)) if ssim else float("nan")
    return (time.perf_counter() - t0) / reps * 1e6, (p, s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs the HIP device: a host run measures nothing")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    border = 4
    for shape in ((1, 3, 512, 512), (1, 1, 256, 256)):
        E, Ht = image_pair(shape, dev, 1)
        for ssim in (True, False):
            dus, eus, hus = [], [], []
            for r in range(a.rounds):
                d, ev, out = device_us(E, Ht, border, ssim, a.reps)
                h, ref = host_us(E, Ht, border, ssim, a.host_reps)
                dus.append(d), eus.append(ev), hus.append(h)
                emit({"shape": list(shape), "border": border, "ssim": ssim, "round": r, "device_us": round(d, 2),
                      "device_event_us": round(ev, 2), "host_us": round(h, 1)})
            got = out[0].tolist()
            md, mh = statistics.median(dus), statistics.median(hus)
            emit({"shape": list(shape), "border": border, "ssim": ssim, "median_device_us": round(md, 2),
                  "median_device_event_us": round(statistics.median(eus), 2), "median_host_us": round(mh, 1),
                  "host_over_device": round(mh / md, 1), "psnr_equal": got[0] == ref[0],
                  "ssim_abs_diff": abs(got[1] - ref[1]) if ssim else None})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
