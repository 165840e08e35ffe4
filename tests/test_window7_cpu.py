"""Window size 7 without a GPU: the window-size-taking attention entry points validate their arguments on the host
(an error code and a message, no launch), and define_G builds the reference module tree of the JPEG
artifact-reduction option file (options/swinir/train_swinir_car_jpeg.json)."""
import pytest
import torch

from kair_amd import _hip as H

# dummy non-null pointers: validation fails before anything is dereferenced or launched
P = 4096


def _fwd(ws, shift, Hh, Ww):
    return H.lib().kair_window_attn_fwd_w(P, H.F32, P, P, 192, P, 6, 6, 30, 0.18, Hh, Ww, shift, -1, None, 0, 32, ws, None)


def _bwd(ws, shift, Hh, Ww):
    return H.lib().kair_window_attn_bwd_w(P, P, 192, P, 192, H.F32, P, P, P, 0, P, 0, P, 6, 6, 30, 0.18, Hh, Ww, shift,
                                          None, 0, 32, ws, None)


def _fwd_x3(ws, shift, Hh, Ww):
    return H.lib().kair_window_attn_fwd_x3_w(P, P, P, P, P, 192, P, 6, 6, 30, 0.18, Hh, Ww, shift, -1, 4, 4, ws, None)


def _bwd_x3(ws, shift, Hh, Ww):
    return H.lib().kair_window_attn_bwd_x3_w(P, P, P, P, 192, P, P, 192, P, P, P, P, P, 0, P, 6, 6, 30, 0.18, Hh, Ww, shift,
                                             4, 26, ws, None)


@pytest.mark.parametrize("call,name", [(_fwd, b"window_attn_fwd"), (_bwd, b"window_attn_bwd"),
                                       (_fwd_x3, b"window_attn_fwd_x3"), (_bwd_x3, b"window_attn_bwd_x3")])
@pytest.mark.parametrize("ws,shift,Hh,Ww", [(9, 0, 18, 27), (7, 7, 14, 21), (7, 3, 15, 21), (7, 3, 14, 20), (6, 0, 12, 18)],
                         ids=["ws9", "shift7", "H15", "W20", "ws6"])
def test_window_size_entry_points_reject_bad_geometry(call, name, ws, shift, Hh, Ww):
    rc = call(ws, shift, Hh, Ww)
    assert rc != 0
    msg = H.lib().kair_last_error()
    assert name in msg, msg


def test_bwd_ws_sizes_by_window():
    L = H.lib()
    assert L.kair_window_attn_bwd_ws_w(12, 6, 9) == 0
    n8, n7 = L.kair_window_attn_bwd_ws_w(12, 6, 8), L.kair_window_attn_bwd_ws_w(12, 6, 7)
    assert n8 == L.kair_window_attn_bwd_ws(12, 6) and n8 % 225 == 0
    assert n7 * 225 == n8 * 169
    with pytest.raises(ValueError):
        H.window_attn_bwd_ws(12, 6, ws=9)


def test_engine_names_supported_window_sizes():
    from kair_amd.engine.swinir_engine import SwinIREngine
    from kair_amd.models.network_swinir import SwinIR
    net = SwinIR(img_size=18, window_size=9, depths=[2], embed_dim=60, num_heads=[6], mlp_ratio=2, upscale=1, in_chans=1,
                 img_range=255.0, upsampler=None, resi_connection="1conv")
    with pytest.raises(NotImplementedError, match="7 and 8"):
        SwinIREngine(net, compute_dtype="fp32x3")


JPEG_NETG = {"net_type": "swinir", "upscale": 1, "in_chans": 1, "img_size": 126, "window_size": 7, "img_range": 255.0,
             "depths": [6] * 6, "embed_dim": 180, "num_heads": [6] * 6, "mlp_ratio": 2, "upsampler": None,
             "resi_connection": "1conv", "init_type": "default"}


def test_define_G_jpeg_car_matches_oracle_layout():
    from kair_amd.models.select_network import define_G
    from kair_amd.utils.utils_option import dict_to_nonedict
    from oracle import swinir as osw
    net = define_G(dict_to_nonedict({"is_train": False, "netG": dict(JPEG_NETG)}))
    ref = osw.SwinIR(1, 1, 126, 7, 255.0, [6] * 6, 180, [6] * 6, 2, None, "1conv")
    sd, sdr = net.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(sdr.keys())
    for k in sd:
        assert sd[k].shape == sdr[k].shape and sd[k].dtype == sdr[k].dtype, k
    tables = [v for k, v in sd.items() if k.endswith("relative_position_bias_table")]
    assert len(tables) == 36 and all(tuple(t.shape) == (169, 6) for t in tables)
    assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in ref.parameters())
