"""MSRResNet x4, IMDN x4 and the DPSR prior x4 on ResSREngine: training steps and eval forwards against the same networks
as plain torch modules, and the DPSR synthesis launch.

    python tools/bench_ressr.py [--batch 16] [--ps 96] [--steps 20] [--rounds 3] [--out profiles/ressr_bench.txt]

Times (1) kair_synth_dpsr between HIP events beside task "sr"'s one launch (kair_synth_sr) for the same batch; (2) per
network the fused, graph-captured training step (FusedTrainer: L1, Adam, EMA) with a fresh PatchSynth batch every step
(task "sr"; "dpsr" for the prior), on the fp32 and bf16 engines, and the same step with the network's module list run by
torch (net.model: nn.Conv2d / ReLU / Upsample / PixelShuffle, fp32: MIOpen; L1, torch.optim.Adam, no EMA) on the same
batches, in alternating rounds, medians reported; (3) the eval forward in ms per image at 1 x in_nc x 256 x 256 LR
(main_challenge_sr.py's measure), engine fp32 / bf16 and torch fp32.  One JSON line per run, then a summary line per
network; everything is also written to --out."""
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
from kair_amd.models.network_dpsr import MSRResNet_prior  # noqa: E402
from kair_amd.models.network_imdn import IMDN  # noqa: E402
from kair_amd.models.network_msrresnet import MSRResNet0  # noqa: E402

NETS = {"msrresnet": (MSRResNet0, dict(in_nc=3, out_nc=3, nc=64, nb=16, upscale=4), "sr"),
        "imdn": (IMDN, dict(in_nc=3, out_nc=3, nc=64, nb=8, upscale=4), "sr"),
        "dpsr": (MSRResNet_prior, dict(in_nc=4, out_nc=3, nc=96, nb=16, upscale=4), "dpsr")}


def event_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--ps", type=int, default=96)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--eval_size", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "ressr_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, PS, sf = a.batch, a.ps, 4
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    pool = synthetic_pool(64, 3, PS + 64, PS + 64, seed=99, device=dev)
    synths = {"sr": PatchSynth(pool, task="sr", H_size=PS, scale=sf, seed=1000),
              "dpsr": PatchSynth(pool, task="dpsr", H_size=PS, scale=sf, sigma=(0, 50), seed=1000)}
    dp, sr = synths["dpsr"], synths["sr"]
    L, Hh = dp.next(B)
    Ls, Hs = sr.next(B)
    par, spar = dp.last_params, sr.last_params
    out = {"shape": {"B": B, "C": 3, "PS": PS, "sf": sf},
           "synth_dpsr_us": round(1e3 * event_ms(lambda: H.synth_dpsr(dp.pool, par, B, PS, sf, dp.kind.taps_h, dp.kind.taps_w,
                                                                      1000, 1, Hh, L), a.reps), 2),
           "synth_sr_us": round(1e3 * event_ms(lambda: H.synth_sr(sr.pool, spar, B, PS, sf, sr.kind.taps_h, sr.kind.taps_w,
                                                                  Hs, Ls), a.reps), 2)}
    emit(out)

    for name, (cls, kw, task) in NETS.items():
        synth = synths[task]
        steppers, evals = {}, {}
        x = torch.rand(1, kw["in_nc"], a.eval_size, a.eval_size, device=dev)
        for dt in ("fp32", "bf16"):
            torch.manual_seed(0)
            mk = lambda: cls(**kw, compute_dtype=dt).to(dev)   # noqa: E731
            net, ema = mk().train(), mk().eval()
            ema.load_state_dict(net.state_dict())
            tr = FusedTrainer(net, ema, lr=1e-4, E_decay=0.999, use_graph=True)
            steppers[dt] = lambda tr=tr, synth=synth: tr.step(*synth.next(B))
            evals[dt] = lambda ema=ema: ema(x)
        torch.manual_seed(0)
        ref = cls(**kw).to(dev).train()
        adam = torch.optim.Adam(ref.parameters(), lr=1e-4)

        def torch_step(ref=ref, adam=adam, synth=synth):
            Lb, Hb = synth.next(B)
            adam.zero_grad(set_to_none=True)
            loss = (ref.model(Lb) - Hb).abs().mean()
            loss.backward()
            adam.step()
            return loss

        steppers["torch_fp32"] = torch_step
        evals["torch_fp32"] = lambda ref=ref: ref.model(x)
        for fn in steppers.values():
            for _ in range(4):   # two eager steps, the capture, one replay (torch: MIOpen's algorithm search)
                fn()
        torch.cuda.synchronize()
        runs = {n: [] for n in steppers}
        for r in range(a.rounds):
            for n, fn in steppers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loss = fn()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                runs[n].append(ms)
                emit({"net": name, "round": r, "step": n, "ms_per_step": round(ms, 3),
                      "patches_per_s": round(B / ms * 1e3, 1), "loss": round(float(loss), 6)})
        med = {n: statistics.median(v) for n, v in runs.items()}
        with torch.no_grad():
            ev = {n: round(event_ms(fn, 20), 3) for n, fn in evals.items()}
        emit({"net": name, "params": sum(p.numel() for p in ref.parameters()),
              "median_ms_per_step": {n: round(m, 3) for n, m in med.items()},
              "median_patches_per_s": {n: round(B / m * 1e3, 1) for n, m in med.items()},
              "fp32_over_torch_fp32": round(med["torch_fp32"] / med["fp32"], 3),
              "bf16_over_torch_fp32": round(med["torch_fp32"] / med["bf16"], 3),
              "eval_ms_per_image": ev, "eval_lr": [1, kw["in_nc"], a.eval_size, a.eval_size]})
        del steppers, evals, ref, adam
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
