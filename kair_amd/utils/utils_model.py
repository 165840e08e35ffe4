"""Full-image inference helpers (restatement of /root/reference/utils/utils_model.py:51-230 and the
tiling / padding of /root/reference/main_test_swinir.py:66-72, 256-284), SURVEY §8f rank 4.

test_mode(model, L, mode, refield, min_size, sf, modulo)   utils_model.py:51-89
    0 plain, 1 replicate-pad to `modulo`, 2 recursive 4-way split, 3 x8 self-ensemble,
    4 split + x8
pad_to_window(L, window_size)   main_test_swinir.py:66-72 (mirror pad to the next multiple + 1 window)
test_tiled(model, L, tile, tile_overlap, sf, window_size, tile_batch)   main_test_swinir.py:256-284
    overlapping tiles blended by their coverage count.  MI355X: the tiles of one image are run as
    batches of `tile_batch` (one forward per batch instead of one per tile); every network on
    this path is per-sample independent, so the blend is the reference's.

The model is any callable NCHW -> NCHW (the define_G networks); no_grad is the caller's business,
as in the reference.
"""
import math

import torch

from . import utils_image as util


def test_mode(model, L, mode=0, refield=32, min_size=256, sf=1, modulo=1):
    if mode == 0:
        return test(model, L)
    if mode == 1:
        return test_pad(model, L, modulo, sf)
    if mode == 2:
        return test_split(model, L, refield, min_size, sf, modulo)
    if mode == 3:
        return test_x8(model, L, modulo, sf)
    if mode == 4:
        return test_split_x8(model, L, refield, min_size, sf, modulo)
    raise ValueError(f"test_mode: mode {mode}")


def test(model, L):
    return model(L)


def test_pad(model, L, modulo=16, sf=1):
    h, w = L.shape[-2:]
    pb, pr = int(math.ceil(h / modulo) * modulo - h), int(math.ceil(w / modulo) * modulo - w)
    E = model(torch.nn.functional.pad(L, (0, pr, 0, pb), mode="replicate") if (pb or pr) else L)
    return E[..., :h * sf, :w * sf]


def test_split_fn(model, L, refield=32, min_size=256, sf=1, modulo=1):
    h, w = L.shape[-2:]
    if h * w <= min_size ** 2:
        return test_pad(model, L, modulo, sf)
    th, tw = (h // 2 // refield + 1) * refield, (w // 2 // refield + 1) * refield
    top, bottom = slice(0, th), slice(h - th, h)
    left, right = slice(0, tw), slice(w - tw, w)
    Ls = [L[..., top, left], L[..., top, right], L[..., bottom, left], L[..., bottom, right]]
    if h * w <= 4 * min_size ** 2:
        Es = [model(x) for x in Ls]
    else:
        Es = [test_split_fn(model, x, refield, min_size, sf, modulo) for x in Ls]
    b, c = Es[0].shape[:2]
    E = torch.zeros(b, c, sf * h, sf * w, dtype=L.dtype, device=L.device)
    h2, w2 = h // 2 * sf, w // 2 * sf
    E[..., :h2, :w2] = Es[0][..., :h2, :w2]
    E[..., :h2, w2:w * sf] = Es[1][..., :h2, (-w + w // 2) * sf:]
    E[..., h2:h * sf, :w2] = Es[2][..., (-h + h // 2) * sf:, :w2]
    E[..., h2:h * sf, w2:w * sf] = Es[3][..., (-h + h // 2) * sf:, (-w + w // 2) * sf:]
    return E


def test_split(model, L, refield=32, min_size=256, sf=1, modulo=1):
    return test_split_fn(model, L, refield, min_size, sf, modulo)


def _unaugment(E, i):
    return util.augment_img_tensor4(E, mode=8 - i if i in (3, 5) else i)


def test_x8(model, L, modulo=1, sf=1):
    Es = [_unaugment(test_pad(model, util.augment_img_tensor4(L, mode=i), modulo, sf), i) for i in range(8)]
    return torch.stack(Es, 0).mean(0)


def test_split_x8(model, L, refield=32, min_size=256, sf=1, modulo=1):
    Es = [_unaugment(test_split_fn(model, util.augment_img_tensor4(L, mode=i), refield, min_size, sf, modulo), i)
          for i in range(8)]
    return torch.stack(Es, 0).mean(0)


def pad_to_window(L, window_size):
    """main_test_swinir.py:66-72: mirror-extend to (h // ws + 1) * ws (always at least one row)."""
    h, w = L.shape[-2:]
    hp = (h // window_size + 1) * window_size - h
    wp = (w // window_size + 1) * window_size - w
    L = torch.cat([L, torch.flip(L, [2])], 2)[:, :, :h + hp, :]
    return torch.cat([L, torch.flip(L, [3])], 3)[:, :, :, :w + wp]


def test_tiled(model, L, tile=None, tile_overlap=32, sf=1, window_size=8, tile_batch=16):
    if tile is None:
        return model(L)
    b, c, h, w = L.shape
    tile = min(tile, h, w)
    if tile % window_size:
        raise AssertionError("tile size should be a multiple of window_size")
    stride = tile - tile_overlap
    hs = list(range(0, h - tile, stride)) + [h - tile]
    ws = list(range(0, w - tile, stride)) + [w - tile]
    pos = [(y, x) for y in hs for x in ws]
    E = W = None
    for i in range(0, len(pos), tile_batch):
        chunk = pos[i:i + tile_batch]
        batch = torch.cat([L[..., y:y + tile, x:x + tile] for y, x in chunk], 0)
        out = model(batch)
        if E is None:
            E = torch.zeros(b, out.shape[1], h * sf, w * sf, dtype=out.dtype, device=out.device)
            W = torch.zeros_like(E)
        for j, (y, x) in enumerate(chunk):
            E[..., y * sf:(y + tile) * sf, x * sf:(x + tile) * sf].add_(out[j * b:(j + 1) * b])
            W[..., y * sf:(y + tile) * sf, x * sf:(x + tile) * sf].add_(1.0)
    return E.div_(W)


def find_last_checkpoint(save_dir, net_type="G", pretrained_path=None):
    from .utils_option import find_last_checkpoint as f
    return f(save_dir, net_type, pretrained_path)


# ---- the IRCNN model bank (upstream ircnn_gray.pth / ircnn_color.pth: 25 state dicts, one per noise level) -------------
IRCNN_LEVELS = 25


def ircnn_index(sigma_255):
    """The bank entry for a noise level on the 0-255 scale: min(24, max(0, ceil(sigma / 2) - 1)) -- entry i was trained
    for sigma = 2 (i + 1)."""
    return min(IRCNN_LEVELS - 1, max(0, int(math.ceil(float(sigma_255) / 2.0)) - 1))


def _ircnn_check(sd, what):
    """in_nc of an IRCNN state dict; ValueError naming the first key or shape that is wrong."""
    from ..models.network_dncnn import IRCNN_DILATIONS
    if not isinstance(sd, dict) or "model.0.weight" not in sd:
        raise ValueError(f"{what}: not an IRCNN state dict (no 'model.0.weight')")
    w0 = sd["model.0.weight"]
    if w0.dim() != 4:
        raise ValueError(f"{what}: model.0.weight has shape {tuple(w0.shape)}, not [nc, in_nc, 3, 3]")
    nc, in_nc = w0.shape[:2]
    want, last = {}, len(IRCNN_DILATIONS) - 1
    for li in range(len(IRCNN_DILATIONS)):
        co, ci = (in_nc if li == last else nc), (in_nc if li == 0 else nc)
        want[f"model.{2 * li}.weight"], want[f"model.{2 * li}.bias"] = (co, ci, 3, 3), (co,)
    missing, extra = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if missing or extra:
        raise ValueError(f"{what}: IRCNN keys are model.{{0,2,...,12}}.{{weight,bias}}; missing {missing}, unexpected {extra}")
    for key, shape in want.items():
        if tuple(sd[key].shape) != shape:
            raise ValueError(f"{what}: {key} has shape {tuple(sd[key].shape)}, expected {shape}")
    return in_nc, nc


def load_ircnn_bank(path):
    """{index: state_dict} from a torch-saved IRCNN bank: the upstream layout, a dict of state dicts keyed "0" ... "24"
    (one per noise level), or a single state dict (a one-level bank, index 0).  `path` may also be the loaded object.
    Keys and shapes are checked against network_dncnn.IRCNN (all entries of one width); ValueError names what is wrong."""
    obj = torch.load(path, map_location="cpu") if isinstance(path, (str, bytes)) or hasattr(path, "__fspath__") else path
    if not isinstance(obj, dict) or not obj:
        raise ValueError("IRCNN bank: a dict of state dicts keyed '0' ... '24', or one state dict")
    if all(torch.is_tensor(v) for v in obj.values()):
        _ircnn_check(obj, "IRCNN bank (single state dict)")
        return {0: dict(obj)}
    bank = {}
    for key, sd in obj.items():
        if not str(key).isdigit() or not 0 <= int(key) < IRCNN_LEVELS:
            raise ValueError(f"IRCNN bank: entry key {key!r} is not one of '0' ... '{IRCNN_LEVELS - 1}'")
        bank[int(key)] = sd
    shapes = {_ircnn_check(sd, f"IRCNN bank entry {i!r}") for i, sd in sorted(bank.items())}
    if len(shapes) != 1:
        raise ValueError(f"IRCNN bank: entries of different widths (in_nc, nc): {sorted(shapes)}")
    return bank


class IRCNNBank:
    """One IRCNN network and its bank: select(sigma_255) loads entry ircnn_index(sigma_255) into the network when the
    index changes (load_state_dict copies in place, which moves the parameters' versions: the engine repacks its
    weight forms on the next forward).  A bank with fewer than 25 entries serves a level from its nearest entry at or
    below the index (a one-level bank: always entry 0).  The entries are moved to the network's device once."""

    def __init__(self, net, bank):
        if not bank:
            raise ValueError("IRCNNBank: an empty bank")
        dev = next(net.parameters()).device
        self.net = net
        self.bank = {int(i): {k: v.to(dev) for k, v in sd.items()} for i, sd in bank.items()}
        self.current = None

    def index(self, sigma_255):
        want = ircnn_index(sigma_255)
        below = [i for i in self.bank if i <= want]
        return max(below) if below else min(self.bank)

    def select(self, sigma_255):
        i = self.index(sigma_255)
        if i != self.current:
            self.net.load_state_dict(self.bank[i], strict=True)
            self.current = i
        return self.net

    def __call__(self, x, sigma_255):
        return self.select(sigma_255)(x)
