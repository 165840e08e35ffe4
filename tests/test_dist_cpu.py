"""Data-parallel exchange on CPU (gloo, world_size 2): the same code the trainer runs over RCCL.

* bucket_bounds tiles the flat buffer exactly, last layers first;
* allreduce_mean_ of the flat gradient buffer == the mean over ranks for any bucket size;
* SURVEY §8e equivalence: two ranks with 2-patch shards, grads flattened + all-reduced through the
  trainer's exchange == the 4-patch single-process gradient (oracle network, L1 mean).
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from kair_amd.engine.comm import allreduce_mean_, bucket_bounds, broadcast_params_


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bucket_bounds_tile_reverse():
    for n, b in [(10, 3), (9, 3), (1, 5), (1000, 1000), (1001, 1000)]:
        bb = bucket_bounds(n, b)
        assert bb[0][1] == n and bb[-1][0] == 0
        assert all(hi - lo <= b for lo, hi in bb)
        assert all(bb[i][0] == bb[i + 1][1] for i in range(len(bb) - 1))


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {}
        # (1) plain mean for several bucket sizes
        for b in (1, 7, 64, 10 ** 6):
            g = torch.arange(100, dtype=torch.float32) * (rank + 1)
            allreduce_mean_(g, b)
            res[f"mean{b}"] = g.clone()
        # (2) broadcast makes rank 1 start from rank 0's params
        p = torch.full((5,), float(rank + 3))
        broadcast_params_(p)
        res["bcast"] = p.clone()
        # (3) DP equivalence on the oracle SwinIR
        from oracle import swinir as osw
        torch.manual_seed(0)
        net = osw.SwinIR(2, 3, 16, 8, 1.0, [2], 60, [6], 2, "pixelshuffledirect")
        g = torch.Generator().manual_seed(5)
        L = torch.rand(4, 3, 16, 16, generator=g)
        Hh = torch.rand(4, 3, 32, 32, generator=g)
        sl = slice(2 * rank, 2 * rank + 2)
        loss = torch.nn.functional.l1_loss(net(L[sl]), Hh[sl])
        loss.backward()
        flat = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
        allreduce_mean_(flat, 4096)
        res["dp_grad"] = flat
        q.put((rank, {k: v.numpy() for k, v in res.items()}))   # by value (no shared-memory fds)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_gloo_world2_allreduce_and_dp_equivalence():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = {r: {k: torch.from_numpy(v) for k, v in d.items()} for r, d in (q.get(timeout=240) for _ in range(world))}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    want = torch.arange(100, dtype=torch.float32) * 1.5
    for r in range(world):
        for b in (1, 7, 64, 10 ** 6):
            torch.testing.assert_close(out[r][f"mean{b}"], want)
        torch.testing.assert_close(out[r]["bcast"], torch.full((5,), 3.0))
    torch.testing.assert_close(out[0]["dp_grad"], out[1]["dp_grad"])
    # single-process full-batch reference
    from oracle import swinir as osw
    torch.manual_seed(0)
    net = osw.SwinIR(2, 3, 16, 8, 1.0, [2], 60, [6], 2, "pixelshuffledirect")
    g = torch.Generator().manual_seed(5)
    L = torch.rand(4, 3, 16, 16, generator=g)
    Hh = torch.rand(4, 3, 32, 32, generator=g)
    torch.nn.functional.l1_loss(net(L), Hh).backward()
    full = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    torch.testing.assert_close(out[0]["dp_grad"], full, rtol=1e-4, atol=1e-6)


# the small network (embed 60, depths [2, 2], img 16) in every tail configuration: (upsampler, scale, channels,
# resi_connection) -> (len(convs()), len(pack_jobs())) of the bf16 engine before the tails became objects
SMALL_TAILS = {
    "pixelshuffle-x2": (("pixelshuffle", 2, 3, "1conv"), (7, 69)),
    "pixelshuffle-x3": (("pixelshuffle", 3, 3, "1conv"), (7, 69)),
    "pixelshuffle-x4": (("pixelshuffle", 4, 3, "1conv"), (8, 72)),
    "pixelshuffledirect-x2": (("pixelshuffledirect", 2, 3, "1conv"), (5, 62)),
    "nearest+conv-x4": (("nearest+conv", 4, 3, "1conv"), (9, 74)),
    "None-1ch": ((None, 1, 1, "1conv"), (5, 62)),
    "empty-3conv": (("", 1, 3, "3conv"), (5, 80)),
}


@pytest.mark.parametrize("ups", ["pixelshuffle", "pixelshuffledirect"] + list(SMALL_TAILS))
def test_swinir_gradient_segments_tile_the_flat_buffer(ups):
    """The all-reduce buckets the trainer overlaps with backward: the engine's gradient segments are
    contiguous in parameter order, tile the flat buffer and come last layer first.  The layer objects and the weight
    packs are counted too: the order of convs() is the pack-job order."""
    from kair_amd.engine.swinir_engine import SwinIREngine
    from kair_amd.engine.trainer import segment_buckets
    from kair_amd.models.network_swinir import SwinIR
    if ups in SMALL_TAILS:
        (kind, sc, ch, resi), counts = SMALL_TAILS[ups]
        net = SwinIR(upscale=sc, in_chans=ch, img_size=16, window_size=8, img_range=1.0, depths=[2, 2], embed_dim=60,
                     num_heads=[6, 6], mlp_ratio=2, upsampler=kind, resi_connection=resi)
    else:
        counts = {"pixelshuffle": (12, 488), "pixelshuffledirect": (9, 472)}[ups]
        net = SwinIR(upscale=4 if ups == "pixelshuffle" else 2, in_chans=3, img_size=48, window_size=8, img_range=1.0,
                     depths=[6] * 6, embed_dim=180, num_heads=[6] * 6, mlp_ratio=2, upsampler=ups, resi_connection="1conv")
    eng = SwinIREngine(net, "bf16")
    params = list(net.parameters())
    b = segment_buckets(params, eng.grad_segments())
    assert b is not None and len(b) == len(net.layers) + 1
    assert b[0][1] == sum(p.numel() for p in params)      # the tail bucket ends the buffer
    assert [lo for lo, _ in b] == sorted([lo for lo, _ in b], reverse=True)
    assert b[-1][0] == 0
    assert (len(eng.convs()), len(eng.pack_jobs())) == counts
    net.upsampler = "bicubic"
    with pytest.raises(NotImplementedError, match="bicubic"):
        SwinIREngine(net, "bf16")
