"""DPIR loop times on the MI355X: 8-iteration deblurring and 24-iteration x4 super-resolution with the option-file DRUNet
(nc 64/128/256/512, nb 4) on the fp32 and bf16 engines, at 256 x 256 gray and 481 x 321 colour (x4: the HR grid is
modcropped to 480 x 320), split into data-step and denoiser time, with the HIP data step (utils_sisr.DataStep) and, as
a comparison, the same loop with the data step done by torch.fft on the device (utils_sisr.HostDataStep).

    python tools/bench_dpir.py [--rounds 5] [--out profiles/dpir_bench.txt]

Per configuration the two variants alternate for --rounds rounds after one warm-up each (the engines plan both
orientations of the x8 loop there); the medians are reported.  Times are device times from events recorded around each
phase; nothing is read back inside a loop.  Random weights: the times do not depend on them.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kair_amd.main_dpir import _unaugment  # noqa: E402
from kair_amd.models.network_unet import UNetRes  # noqa: E402
from kair_amd.utils import utils_image as util  # noqa: E402
from kair_amd.utils import utils_model, utils_pnp, utils_sisr  # noqa: E402

dev = torch.device("cuda")


def timed_loop(net, data, x, rhos, sigmas):
    """(total, data-step, denoiser) ms of one restoration; the loop of main_dpir.dpir_restore with events around its phases."""
    n = len(rhos)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
    end = torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for i in range(n):
            ev[i][0].record()
            x = data.solve(x, rhos[i:i + 1])
            ev[i][1].record()
            x = util.augment_img_tensor4(x, i % 8)
            m = x.new_full((x.shape[0], 1) + tuple(x.shape[-2:]), float(sigmas[i]))
            ev[i][2].record()
            x = utils_model.test_mode(net, torch.cat((x, m), dim=1), mode=1, modulo=8)
            x = _unaugment(x, i % 8)
        end.record()
    torch.cuda.synchronize()
    t_data = sum(ev[i][0].elapsed_time(ev[i][1]) for i in range(n))
    t_den = sum(ev[i][2].elapsed_time(ev[i + 1][0] if i + 1 < n else end) for i in range(n))
    return ev[0][0].elapsed_time(end), t_data, t_den


def bench(task, hw, C, dt, rounds, lines):
    sf, iters = (1, 8) if task == "deblur" else (4, 24)
    Hh, Ww = hw[0] - hw[0] % sf, hw[1] - hw[1] % sf
    torch.manual_seed(0)
    net = UNetRes(C + 1, C, (64, 128, 256, 512), 4, compute_dtype=dt).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    L = torch.rand(1, C, Hh // sf, Ww // sf, generator=g).to(dev)
    k = torch.rand(25, 25, generator=g)
    k = (k / k.sum()).to(dev)
    sigma = 7.65 / 255 if task == "deblur" else 0.0
    rhos, sigmas = utils_pnp.get_rho_sigma(max(0.255 / 255, sigma), iters, 49.0, max(0.255, 255 * sigma), 1.0)
    rhos = torch.tensor([float(r) for r in rhos]).to(dev)
    x0 = L if sf == 1 else util.imresize(L, sf)
    steps = {"hip": utils_sisr.DataStep(L, k, sf), "torch.fft": utils_sisr.HostDataStep(L, k, sf)}
    res = {name: [] for name in steps}
    for name, data in steps.items():
        timed_loop(net, data, x0, rhos, sigmas)                       # warm-up: plans, both orientations
    for _ in range(rounds):
        for name, data in steps.items():
            res[name].append(timed_loop(net, data, x0, rhos, sigmas))
    for name in steps:
        tot, dat, den = (statistics.median(r[j] for r in res[name]) for j in range(3))
        lo, hi = min(r[0] for r in res[name]), max(r[0] for r in res[name])
        line = (f"{task:6s} x{sf} {iters:2d} it  {Hh}x{Ww} C{C}  {dt:5s}  data step {name:9s}: total {tot:8.2f} ms "
                f"(min {lo:.2f}, max {hi:.2f}), data step {dat:7.2f} ms ({dat / iters * 1e3:6.0f} us/it), "
                f"denoiser {den:8.2f} ms ({den / iters:6.2f} ms/it)")
        print(line, flush=True)
        lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "dpir_bench.txt"))
    a = ap.parse_args()
    lines = [f"# tools/bench_dpir.py --rounds {a.rounds}: medians of alternating rounds, device times (events), batch 1, "
             f"DRUNet nc 64/128/256/512 nb 4, x8 loop, {torch.cuda.get_device_name(0)}"]
    for dt in ("fp32", "bf16"):
        for hw, C in (((256, 256), 1), ((481, 321), 3)):
            for task in ("deblur", "sisr"):
                bench(task, hw, C, dt, a.rounds, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
