"""SCUNet (colour, config [4] * 7, dim 64) on one MI355X, after tools/bench_drunet.py.

    python tools/bench_scunet.py [--batch 16] [--ps 128] [--steps 4] [--rounds 3] [--dtypes fp32,bf16]

Times (1) the fused, graph-captured training step (FusedTrainer: L1, Adam, EMA) with a fresh PatchSynth(task="dn",
sigma 25) batch every step, for each compute dtype; (2) the eval forward of one 1 x 3 x 256 x 256 image; (3) the same
module list as plain torch modules in fp32 (RefSCUNet of tests/test_scunet_cpu.py on the device: eager autograd step
with torch Adam, and its eval forward) as the comparison; (4) the bf16 eval forward with the one-launch narrow Block
(kair_scu_block_fwd) off, on at trans_dim 32, on at 64 and on at both: the A/B behind SCUNetEngine.FUSED_BLOCK_DEFAULT.  The variants run in alternating rounds and the median of the
rounds is reported, so a drift of the machine does not favour one of them.  One JSON line per run, then a summary line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from kair_amd.data.gpu_synth import PatchSynth, synthetic_pool  # noqa: E402
from kair_amd.engine.trainer import FusedTrainer  # noqa: E402
from kair_amd.models.network_scunet import SCUNet  # noqa: E402


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--ps", type=int, default=128)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--eval_reps", type=int, default=10)
    ap.add_argument("--config", default="4,4,4,4,4,4,4")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--no_torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, PS = a.batch, a.ps
    config = [int(v) for v in a.config.split(",")]
    pool = synthetic_pool(64, 3, PS + 64, PS + 64, seed=99, device=dev)
    synth = PatchSynth(pool, task="dn", H_size=PS, sigma=25, seed=1000)
    print(json.dumps({"shape": {"B": B, "C": 3, "PS": PS, "config": config, "dim": 64, "eval": [1, 3, 256, 256]}}),
          flush=True)
    x_eval = torch.rand(1, 3, 256, 256, device=dev)
    train, evalf, ab = {}, {}, {}
    for dt in [d for d in a.dtypes.split(",") if d]:
        torch.manual_seed(0)
        mk = lambda: SCUNet(3, config, 64, compute_dtype=dt).to(dev)   # noqa: E731
        net, ema = mk().train(), mk().eval()
        ema.load_state_dict(net.state_dict())
        tr = FusedTrainer(net, ema, lr=1e-4, E_decay=0.999, use_graph=True)
        for _ in range(4):   # two eager steps, the capture, one replay
            tr.step(*synth.next(B))
        train[dt] = (lambda tr=tr: tr.step(*synth.next(B)))
        ev = mk().eval()

        def fwd(ev=ev):
            with torch.no_grad():
                return ev(x_eval)
        fwd()
        evalf[dt] = fwd
        if dt == "bf16":   # the A/B of the one-launch narrow Block: the same weights and image, one width at a time
            for tag, fb in (("bf16_unfused", False), ("bf16_fused32", {32: True}), ("bf16_fused64", {64: True}),
                            ("bf16_fused32+64", True)):
                evf = mk().eval().set_fused_block(fb)
                evf.load_state_dict(ev.state_dict())

                def fwdf(evf=evf):
                    with torch.no_grad():
                        return evf(x_eval)
                fwdf()
                ab[tag] = fwdf
    if not a.no_torch:
        from test_scunet_cpu import RefSCUNet   # the reference lives only in that test file: moving it breaks this tool
        torch.manual_seed(0)
        ref = RefSCUNet(3, config, 64).to(dev).train()
        opt = torch.optim.Adam(ref.parameters(), lr=1e-4)

        def torch_step():
            L, Hh = synth.next(B)
            opt.zero_grad(set_to_none=True)
            loss = (ref(L) - Hh).abs().mean()
            loss.backward()
            opt.step()
            return loss

        def torch_fwd():
            with torch.no_grad():
                return ref(x_eval)
        torch_step(), torch_fwd()
        train["torch_fp32"], evalf["torch_fp32"] = torch_step, torch_fwd
    runs_t, runs_e, runs_ab = {k: [] for k in train}, {k: [] for k in evalf}, {}
    for r in range(a.rounds):
        for k in train:
            ms = wall_ms(train[k], a.steps)
            runs_t[k].append(ms)
            ems = wall_ms(evalf[k], a.eval_reps)
            runs_e[k].append(ems)
            print(json.dumps({"round": r, "variant": k, "train_ms_per_step": round(ms, 3),
                              "patches_per_s": round(B / ms * 1e3, 2), "eval_ms_per_image": round(ems, 3)}), flush=True)
        for k in ab:   # eval only
            runs_ab.setdefault(k, []).append(wall_ms(ab[k], a.eval_reps))
            print(json.dumps({"round": r, "variant": k, "eval_ms_per_image": round(runs_ab[k][-1], 3)}), flush=True)
    if runs_ab:
        print(json.dumps({"median_eval_ms_per_image_fused_ab": {k: round(statistics.median(v), 3)
                                                                 for k, v in runs_ab.items()}}), flush=True)
    med_t = {k: statistics.median(v) for k, v in runs_t.items()}
    med_e = {k: statistics.median(v) for k, v in runs_e.items()}
    print(json.dumps({"median_train_ms_per_step": {k: round(m, 3) for k, m in med_t.items()},
                      "median_patches_per_s": {k: round(B / m * 1e3, 2) for k, m in med_t.items()},
                      "median_eval_ms_per_image": {k: round(m, 3) for k, m in med_e.items()}}), flush=True)


if __name__ == "__main__":
    main()
