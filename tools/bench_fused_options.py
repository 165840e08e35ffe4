"""The option keys that used to drop a run off the fused step -- G_lossfn_type 'l2' and G_optimizer_clipgrad -- timed
on the fused trainer and on the autograd path (train.use_fused_trainer false), through ModelPlain.

    python tools/bench_fused_options.py [--steps 10] [--rounds 5] [--skip-swinir] [--clipgrad 0.05] [--out FILE]

Two groups of four models, each built by define_Model from an option dict and stepped with feed_data +
optimize_parameters (the training loop's calls, the loss read included) on one fixed batch:
  DnCNN (17 layers, BN, B 64, 40 px, fp32):            'l1' and 'l2', fused and not;
  classical x4 SwinIR (B 32, 48 px -> 192 px, fp32x3):  without and with G_optimizer_clipgrad, fused and not.
The four models of a group run in alternating rounds and the median of the rounds is reported, so a drift of the
machine does not favour one of them.  One JSON line per run, then one summary line per group with the ratios;
--out also writes the lines to a file (profiles/fused_options_bench.txt is the committed record)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kair_amd.engine.trainer import FusedTrainer  # noqa: E402
from kair_amd.models.select_model import define_Model  # noqa: E402
from kair_amd.utils.utils_option import dict_to_nonedict  # noqa: E402

DNCNN = {"net_type": "dncnn", "in_nc": 1, "out_nc": 1, "nc": 64, "nb": 17, "act_mode": "BR", "init_type": "orthogonal",
         "init_bn_type": "uniform", "init_gain": 0.2, "compute_dtype": "fp32"}
SWINIR = {"net_type": "swinir", "upscale": 4, "in_chans": 3, "img_size": 48, "window_size": 8, "img_range": 1.0,
          "depths": [6] * 6, "embed_dim": 180, "num_heads": [6] * 6, "mlp_ratio": 2, "upsampler": "pixelshuffle",
          "resi_connection": "1conv", "init_type": "default", "compute_dtype": "fp32x3"}


def options(netG, scale, models_dir, **train):
    return {"model": "plain", "is_train": True, "dist": False, "gpu_ids": [0], "scale": scale,
            "path": {"models": models_dir}, "netG": dict(netG),
            "train": {"G_lossfn_type": "l1", "G_lossfn_weight": 1.0, "G_optimizer_type": "adam", "G_optimizer_lr": 1e-4,
                      "G_optimizer_betas": [0.9, 0.999], "G_optimizer_wd": 0, "G_optimizer_clipgrad": None,
                      "G_optimizer_reuse": False, "G_scheduler_type": "MultiStepLR", "G_scheduler_milestones": [10 ** 6],
                      "G_scheduler_gamma": 0.5, "E_decay": 0.999, "G_param_strict": True, "E_param_strict": True, **train}}


def batch(shape, sf, dev, seed):
    """A smooth target + noise in [0, 1]; the input is its average-pooled (sf > 1) or noisy (sf 1) version."""
    g = torch.Generator(device=dev).manual_seed(seed)
    B, C, Hh, Ww = shape
    yy = torch.linspace(0, 1, Hh, device=dev).view(1, 1, Hh, 1)
    xx = torch.linspace(0, 1, Ww, device=dev).view(1, 1, 1, Ww)
    Ht = (0.2 + 0.3 * yy + 0.3 * xx + 0.1 * torch.rand(B, C, Hh, Ww, device=dev, generator=g)).clamp(0, 1).contiguous()
    if sf > 1:
        return torch.nn.functional.avg_pool2d(Ht, sf).contiguous(), Ht
    return (Ht + 0.1 * torch.randn(B, C, Hh, Ww, device=dev, generator=g)).contiguous(), Ht


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-swinir", action="store_true")
    ap.add_argument("--clipgrad", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    groups = [("dncnn B64 40px fp32", DNCNN, 1, (64, 1, 40, 40),
               {"l1": {"G_lossfn_type": "l1"}, "l2": {"G_lossfn_type": "l2"}})]
    if not a.skip_swinir:
        groups.append(("swinir classical x4 B32 48px fp32x3", SWINIR, 4, (32, 3, 192, 192),
                       {"noclip": {}, "clip": {"G_optimizer_clipgrad": a.clipgrad}}))
    with tempfile.TemporaryDirectory() as models_dir:
        for name, netG, sf, shape, variants in groups:
            L, Ht = batch(shape, sf, dev, 2)
            models = {}
            for vname, train in variants.items():
                for fused in (True, False):
                    torch.manual_seed(0)
                    m = define_Model(dict_to_nonedict(options(netG, sf, models_dir, use_fused_trainer=fused, **train)))
                    m.init_train()
                    if isinstance(m.trainer, FusedTrainer) != fused:
                        raise RuntimeError(f"{name} {vname}: fused {fused}, trainer {type(m.trainer).__name__}")
                    for s in range(4):   # fused: two eager steps, the capture, one replay
                        m.feed_data({"L": L, "H": Ht})
                        m.optimize_parameters(s)
                    torch.cuda.synchronize()
                    models[(vname, "fused" if fused else "autograd")] = m
            runs = {k: [] for k in models}
            for r in range(a.rounds):
                for key, m in models.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for s in range(a.steps):
                        m.feed_data({"L": L, "H": Ht})
                        m.optimize_parameters(s)
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) / a.steps * 1e3
                    runs[key].append(ms)
                    d = {"net": name, "round": r, "options": key[0], "path": key[1], "ms_per_step": round(ms, 3),
                         "loss": round(m.log_dict["G_loss"], 6)}
                    if m.trainer is not None:
                        d["range_events"] = len(m.trainer.range_events)
                        if m.trainer.gnorm is not None:
                            d["gnorm"] = round(m.trainer.gnorm.item(), 6)
                    emit(d)
            med = {k: statistics.median(v) for k, v in runs.items()}
            va, vb = list(variants)
            emit({"net": name, "median_ms_per_step": {f"{k[0]} {k[1]}": round(v, 3) for k, v in med.items()},
                  f"fused {vb} over {va}": round(med[(vb, "fused")] / med[(va, "fused")], 4),
                  "autograd over fused": {v: round(med[(v, "autograd")] / med[(v, "fused")], 3) for v in variants}})
            del models
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
