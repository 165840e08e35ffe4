"""Gradient-norm clipping under data parallel, on the one GPU, in the structure of tests/test_dist_gpu.py: two gloo
ranks (spawned before they touch the GPU) run FusedTrainer with clip_grad on 2-patch shards, one single process runs
it on the 4-patch batch -- three processes in all.  The norm is taken after the all-reduce and its 1 / world, so it
is the norm of the averaged gradient: both ranks compute the same coefficient (what DDP followed by clip_grad_norm_
does) and stay in lockstep, and the world-2 run equals the single process at the "fp32-small" configuration's own
tolerances (test_dist_gpu.CONFIGS: 1e-5 parameters / EMA, 1e-4 updates)."""
import os
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from test_dist_gpu import B, CONFIGS, STEPS, _data, _net, _port  # noqa: E402

NAME = "fp32-small"
CLIP = 1e-3   # far below the gradient norm of these steps (asserted from the recorded norms): every step clips


def _run(rank, world, port, out_dir):
    import torch.distributed as dist
    from kair_amd.engine.trainer import FusedTrainer
    if world > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        cfg = CONFIGS[NAME]
        net, ema = _net(cfg), _net(cfg)
        ema.load_state_dict(net.state_dict())
        net, ema = net.to(dev).train(), ema.to(dev).eval()
        tr = FusedTrainer(net, ema, lr=1e-3, E_decay=0.9, use_graph=True, bucket_mb=0.01, clip_grad=CLIP)
        p0 = tr.flat_p.detach().cpu().clone()
        L, Hh = _data(cfg)
        per = B // world
        L, Hh = L[rank * per:(rank + 1) * per].to(dev), Hh[rank * per:(rank + 1) * per].to(dev)
        losses, norms = [], []
        for _ in range(STEPS + 2):   # 2 warm-up steps, then graph replays
            losses.append(float(tr.step(L, Hh)))
            norms.append(float(tr.gnorm))
        torch.save({"losses": losses, "gnorm": norms, "p": tr.flat_p.cpu(), "e": tr.flat_e.cpu(), "p0": p0,
                    "g": tr.flat_g.cpu(), "segmented": tr.graph is not None and tr.graph[1] is not None,
                    "buckets": len(tr.buckets or [])}, os.path.join(out_dir, f"r{rank}_w{world}.pt"))
    finally:
        if world > 1:
            dist.destroy_process_group()


def test_clipped_world2_matches_single_process():
    with tempfile.TemporaryDirectory() as d:
        ctx = mp.get_context("spawn")
        port = _port()
        procs = [ctx.Process(target=_run, args=(r, 2, port, d)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=180)
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        single = ctx.Process(target=_run, args=(0, 1, 0, d))
        single.start()
        single.join(timeout=180)
        assert single.exitcode == 0
        r0, r1, s = (torch.load(os.path.join(d, f), weights_only=True) for f in ("r0_w2.pt", "r1_w2.pt", "r0_w1.pt"))
    assert r0["segmented"] and r0["buckets"] > 1   # the overlapped per-bucket all-reduce path ran
    # every step clipped, on the same norm on both ranks: the norm of the averaged gradient
    assert r0["gnorm"] == r1["gnorm"], (r0["gnorm"], r1["gnorm"])
    assert all(v > 2 * CLIP for v in r0["gnorm"] + s["gnorm"]), (r0["gnorm"], s["gnorm"])
    for a, b in zip(r0["gnorm"], s["gnorm"]):
        assert abs(a - b) < 1e-4 * b, (r0["gnorm"], s["gnorm"])
    # the ranks stay in lockstep, the clipped gradient left in the flat buffer included
    assert torch.equal(r0["p"], r1["p"]) and torch.equal(r0["e"], r1["e"]) and torch.equal(r0["g"], r1["g"])
    assert abs(r0["g"].double().norm().item() - CLIP) < 1e-3 * CLIP
    for a, b, c in zip(r0["losses"], r1["losses"], s["losses"]):
        assert abs(0.5 * (a + b) - c) < 1e-5 * max(1.0, abs(c)), (a, b, c)
    rel = lambda x, y: ((x - y).norm() / y.norm()).item()
    tol, tol_upd = CONFIGS[NAME]["tol"], CONFIGS[NAME]["tol_upd"]
    assert torch.equal(r0["p0"], s["p0"])
    du = rel(r0["p"] - r0["p0"], s["p"] - s["p0"])
    print(NAME, "clip", CLIP, "gnorm", r0["gnorm"], "params", rel(r0["p"], s["p"]), "updates", du, "ema", rel(r0["e"], s["e"]))
    assert rel(r0["p"], s["p"]) < tol
    assert rel(r0["e"], s["e"]) < tol
    assert du < tol_upd
