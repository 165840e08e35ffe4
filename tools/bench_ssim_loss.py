"""The SSIM loss (G_lossfn_type 'ssim', kair_ssim_loss) next to the L1 loss (kair_l1_loss): the loss launches alone and
the fused training step.

    python tools/bench_ssim_loss.py [--steps 10] [--rounds 5] [--reps 200] [--skip-swinir] [--out FILE]

(1) The loss call alone at 32 x 3 x 192 x 192 (the classical x4 SwinIR step's output), between two HIP events: the
three SSIM launches (statistics, gradient, sum) against kair_l1_loss on the same bf16 rows of 16 slots, fp32 rows of 4
slots (the fp32x3 tail) and -- SSIM only -- the NCHW form, with the rate the algorithmic bytes give (E and H read by both
launches, the three workspace planes written and read once, the gradient written once).
(2) The fused, graph-captured step with 'ssim' against 'l1' on DnCNN (17 layers, BN, B 64, 40 px, fp32) and on the
classical x4 SwinIR (B 32, 48 px, fp32x3): the two trainers of a network run in alternating rounds on the same batch
and the median of the rounds is reported, so a drift of the machine does not favour one of them.  One JSON line per
run, then one summary line per network; --out also writes the lines to a file (profiles/ssim_loss_bench.txt is the
committed record)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kair_amd import _hip as H  # noqa: E402
from kair_amd.engine.trainer import FusedTrainer  # noqa: E402
from kair_amd.models.network_dncnn import DnCNN  # noqa: E402
from kair_amd.models.network_swinir import SwinIR  # noqa: E402


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


def image_pair(B, C, Hh, Ww, dev, seed):
    """A smooth target + noise, and an estimate a little off it, in [0, 1]."""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy = torch.linspace(0, 1, Hh, device=dev).view(1, 1, Hh, 1)
    xx = torch.linspace(0, 1, Ww, device=dev).view(1, 1, 1, Ww)
    Ht = (0.2 + 0.3 * yy + 0.3 * xx + 0.1 * torch.rand(B, C, Hh, Ww, device=dev, generator=g)).clamp(0, 1)
    E = (Ht + 0.05 * (2 * torch.rand(B, C, Hh, Ww, device=dev, generator=g) - 1)).clamp(0, 1)
    return E.contiguous(), Ht.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--skip-swinir", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    # (1) the loss launches alone
    B, C, Hh, Ww = 32, 3, 192, 192
    E, Ht = image_pair(B, C, Hh, Ww, dev, 1)
    loss, ws1, ws = torch.empty(1, device=dev), torch.empty(1024, device=dev), H.ssim_workspace(B, C, Hh, Ww, dev)
    n = E.numel()
    for name, dt, ldc in (("bf16 rows 16", torch.bfloat16, 16), ("fp32 rows 4", torch.float32, 4), ("nchw", torch.float32, None)):
        dE = torch.empty(B * Hh * Ww, ldc, device=dev, dtype=dt) if ldc else torch.empty_like(E)
        gbytes = dE.numel() * dE.element_size()
        us_s = event_us(lambda: H.ssim_loss(E, Ht, loss, dE, ldc, -1.0, B, C, Hh, Ww, ws), a.reps)
        sbytes = 2 * 2 * n * 4 + 2 * 3 * n * 4 + gbytes
        d = {"kernel": "kair_ssim_loss", "gradient": name, "shape": [B, C, Hh, Ww], "us": round(us_s, 2),
             "algorithmic_bytes": sbytes, "bytes_per_s": round(sbytes / (us_s * 1e-6), 0)}
        if ldc:
            us_l = event_us(lambda: H.l1_loss(E, Ht, loss, dE, ldc, 1.0, B, C, Hh, Ww, ws1), a.reps)
            d.update({"l1_us": round(us_l, 2), "ssim_over_l1": round(us_s / us_l, 2)})
        emit(d)

    # (2) the training step
    def dncnn():
        torch.manual_seed(0)
        return DnCNN(1, 1, 64, 17, "BR", compute_dtype="fp32").to(dev)

    def swinir():
        torch.manual_seed(0)
        return SwinIR(upscale=4, in_chans=3, img_size=48, window_size=8, img_range=1.0, depths=[6] * 6, embed_dim=180,
                      num_heads=[6] * 6, mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv",
                      compute_dtype="fp32x3").to(dev)

    nets = [("dncnn B64 40px fp32", dncnn, (64, 1, 40, 40), 1)]
    if not a.skip_swinir:
        nets.append(("swinir classical x4 B32 48px fp32x3", swinir, (32, 3, 192, 192), 4))
    for name, mk, shape, sf in nets:
        Eh, Hh_ = image_pair(*shape, dev, 2)
        L = torch.nn.functional.avg_pool2d(Hh_, sf) if sf > 1 else Eh
        trainers = {}
        for lt in ("l1", "ssim"):
            net, ema = mk().train(), mk().eval()
            ema.load_state_dict(net.state_dict())
            tr = FusedTrainer(net, ema, lr=1e-4, E_decay=0.999, use_graph=True, loss_type=lt,
                              loss_weight=-1.0 if lt == "ssim" else 1.0)
            for _ in range(4):   # two eager steps, the capture, one replay
                tr.step(L, Hh_)
            tr.check_range()
            torch.cuda.synchronize()
            trainers[lt] = tr
        runs = {k: [] for k in trainers}
        for r in range(a.rounds):
            for lt, tr in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    lo = tr.step(L, Hh_)
                tr.check_range()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                runs[lt].append(ms)
                emit({"net": name, "round": r, "loss_type": lt, "ms_per_step": round(ms, 3), "loss": round(lo.item(), 6),
                      "range_events": len(tr.range_events)})
        med = {k: statistics.median(v) for k, v in runs.items()}
        emit({"net": name, "median_ms_per_step": {k: round(v, 3) for k, v in med.items()},
              "ssim_over_l1": round(med["ssim"] / med["l1"], 4)})
        del trainers
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
