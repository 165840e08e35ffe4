"""The host half of PatchSynth (kair_amd/data/gpu_synth.py: patch_draws and the task classes) without a device: the
int32 tables every task draws, and the option checks.

The expected tables were recorded from the commit before the task classes existed, by calling its PatchSynth._draw*
methods unbound on a types.SimpleNamespace that carried the sampler fields and a fresh random.Random(seed): three
consecutive batches per case, the first 16 hex digits of sha256(table.numpy().tobytes()).  They pin the image order
(N = 7, B = 9: the first batch crosses an epoch boundary), the crop bounds, the augment mode and every per-task extra
draw, which is what has to agree with the Dataset* classes draw for draw."""
import hashlib

import pytest
import torch

from kair_amd.data.gpu_synth import TASKS, patch_draws

N, HS, WS, SEED, B = 7, 80, 72, 5, 9

# case: (task, C, H_size, options, sampler, digests of three batches, usrnet's drawn scale factors)
CASES = {
    "dn": ("dn", 3, 32, {}, {},
           ["81bde7e30230ad88", "264e6f1a279ef1ad", "f091dcbf326d3cf1"], None),
    "dn_rank1of3": ("dn", 3, 32, {}, {"rank": 1, "world": 3},
                    ["869f232d51e4e402", "5bf06950b76107df", "bb5dff35372294e5"], None),
    "sr": ("sr", 3, 32, {"scale": 4}, {},
           ["56b27895be78c819", "9c953dbbdc174218", "5259d925636e1a67"], None),
    "fdncnn": ("fdncnn", 3, 32, {"sigma": (5, 50)}, {},
               ["a299795d6dc047db", "15c1e0e1351571b0", "8cb3ead54df7f67e"], None),
    "ffdnet": ("ffdnet", 3, 32, {"sigma": (5, 50)}, {},
               ["a299795d6dc047db", "15c1e0e1351571b0", "8cb3ead54df7f67e"], None),
    "jpeg_list": ("jpeg", 1, 32, {"quality_factor": [10, 40, 90]}, {},
                  ["219d4307cc675c03", "4eff9dece2ce7123", "1988e44320c77b08"], None),
    "jpeg_int": ("jpeg", 1, 32, {"quality_factor": 40}, {},
                 ["3daab9a8ca3d3cd0", "5bb8a25147091877", "cc5df85a2c77b31d"], None),
    "jpeg_color": ("jpeg", 3, 32, {"quality_factor": [10, 40, 90], "is_color": True}, {},
                   ["d6277ed996b8c577", "6fc3b47fd63fe897", "5145337aa32013d3"], None),
    "usrnet_nobank": ("usrnet", 3, 32, {"scales": [1, 2, 4], "sigma_max": 25}, {},
                      ["15e8b909f542c863", "1b6bfd63b57f1e18", "42f3dcb139e539ed"], [4, 2, 2]),
    "usrnet_bank": ("usrnet", 3, 32, {"scales": [1, 2, 4], "sigma_max": 25, "kernel_bank": torch.zeros(5, 25, 25)}, {},
                    ["0abd001139acbe16", "9cc8c60fabdf71d9", "a6e5d5a491856570"], [4, 2, 4]),
    "blindsr": ("blindsr", 3, 64, {"scale": 4, "lq_patchsize": 16}, {},
                ["47d9dc3dd31b3b2c", "feb4a6b02a4aac8e", "92016f38c9fa0f60"], None),
}
COLS = {"dn": 4, "sr": 4, "fdncnn": 5, "ffdnet": 5, "jpeg": 8, "usrnet": 12, "blindsr": 136}

# the first dn batch as numbers: images 1 0 4 2 6 5 3 end the first epoch, 2 4 begin the second
DN_FIRST = [[1, 39, 16, 5], [0, 44, 33, 0], [4, 29, 15, 0], [2, 10, 7, 5], [6, 30, 15, 6], [5, 34, 6, 3],
            [3, 0, 13, 6], [2, 17, 11, 6], [4, 10, 4, 2]]


def digest(t):
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()[:16]


def three_batches(name):
    task, C, PS, options, sampler, _, _ = CASES[name]
    d = patch_draws(task, N, C, HS, WS, H_size=PS, seed=SEED, **sampler, **options)
    return [d.draw(B) for _ in range(3)]


def test_cases_cover_every_task():
    assert {c[0] for c in CASES.values()} == set(TASKS)


@pytest.mark.parametrize("name", list(CASES))
def test_tables_equal_the_parents(name):
    task, _, _, _, _, want, want_sf = CASES[name]
    got = three_batches(name)
    for t, _ in got:
        assert t.dtype == torch.int32 and t.shape == (B, COLS[task]) and t.is_contiguous()
    assert [digest(t) for t, _ in got] == want
    if want_sf is not None:
        assert [sf for _, sf in got] == want_sf
    if name == "dn":
        assert got[0][0].tolist() == DN_FIRST
    if name == "usrnet_bank":   # the r > 3 branch drew bank rows, and the other branch Gaussians
        assert {0, 1} == set(got[0][0][:, 4].tolist())
    if name == "jpeg_int":
        assert all(set(t[:, 5].tolist()) == {40} for t, _ in got)


def test_fdncnn_and_ffdnet_draw_one_table():
    for (a, _), (b, _) in zip(three_batches("fdncnn"), three_batches("ffdnet")):
        assert torch.equal(a, b)
    lev = three_batches("ffdnet")[0][0][:, 4:].view(torch.float32) * 255
    assert 5 <= float(lev.min()) and float(lev.max()) <= 50


REFUSED = [
    ("usrnet", (5, 3, 128, 128), {"H_size": 100, "scales": [1, 2, 3, 4]}, "divisible by the scales"),
    ("ffdnet", (3, 1, 40, 36), {"H_size": 16, "sigma": (60, 5)}, "task 'ffdnet' takes sigma"),
    ("fdncnn", (3, 1, 40, 36), {"H_size": 16, "sigma": (50, 5)}, "task 'fdncnn' takes sigma"),
    ("jpeg", (2, 1, 24, 24), {"H_size": 16, "quality_factor": [40, 101]}, "quality_factor"),
    ("jpeg", (2, 1, 24, 24), {"H_size": 17}, r"H_size \+ 8 = 25"),
    ("jpeg", (2, 1, 24, 24), {"H_size": 16, "is_color": True}, "3 with is_color"),
    ("blindsr", (2, 3, 80, 72), {"H_size": 66, "lq_patchsize": 16, "scale": 4}, "not a positive multiple"),
    ("blindsr", (2, 3, 80, 72), {"H_size": 64, "lq_patchsize": 17, "scale": 4}, "exceeds H_size"),
    ("blindsr", (2, 3, 80, 72), {"H_size": 76, "lq_patchsize": 16, "scale": 4}, "larger than the pool images"),
    ("blindsr", (2, 1, 80, 72), {"H_size": 64, "lq_patchsize": 16, "scale": 4}, "3-channel pool"),
    ("blindsr", (2, 3, 80, 72), {"H_size": 63, "lq_patchsize": 16, "scale": 3}, "scale must be 2 or 4"),
    ("deblur", (2, 3, 80, 72), {"H_size": 32}, "deblur"),
]


@pytest.mark.parametrize("task,shape,options,fragment", REFUSED)
def test_refused_on_the_host(task, shape, options, fragment):
    with pytest.raises(ValueError, match=fragment):
        patch_draws(task, *shape, **options)


def test_an_option_of_another_task_is_refused():
    with pytest.raises(TypeError, match="quality_factor"):
        patch_draws("sr", 2, 3, 80, 72, H_size=32, scale=4, quality_factor=40)
