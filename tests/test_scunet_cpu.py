"""SCUNet without a device: the module tree's state_dict keys and shapes, the equality of its shifted-window mask and
relative-position index with the Swin forms the attention kernels implement, define_G, and RefSCUNet -- the float64
plain-torch reference (nn modules, einsum, masked_fill_(-inf)) restated from the published definition, which
tests/test_scunet_gpu.py runs the engine against.  RefSCUNet loads the module's state_dict with strict=True, which pins
the key names and shapes from the other side.
"""
import pytest
import torch
import torch.nn as nn

from kair_amd.models.network_scunet import SCUNet, WMSA
from kair_amd.models.network_swinir import _shift_mask
from kair_amd.models.select_network import compute_dtype_of, define_G


class RefWMSA(nn.Module):
    def __init__(self, input_dim, output_dim, head_dim, window_size, type):
        super().__init__()
        self.input_dim, self.output_dim, self.head_dim = input_dim, output_dim, head_dim
        self.scale = head_dim ** -0.5
        self.n_heads = input_dim // head_dim
        self.window_size, self.type = window_size, type
        self.embedding_layer = nn.Linear(input_dim, 3 * input_dim, bias=True)
        self.relative_position_params = nn.Parameter(torch.zeros(self.n_heads, 2 * window_size - 1, 2 * window_size - 1))
        self.linear = nn.Linear(input_dim, output_dim)

    def generate_mask(self, h, w, p, shift, device=None):
        m = torch.zeros(h, w, p, p, p, p, dtype=torch.bool, device=device)
        if self.type == "W":
            return m.view(1, 1, h * w, p * p, p * p)
        s = p - shift
        m[-1, :, :s, :, s:, :] = True
        m[-1, :, s:, :, :s, :] = True
        m[:, -1, :, :s, :, s:] = True
        m[:, -1, :, s:, :, :s] = True
        return m.view(1, 1, h * w, p * p, p * p)

    def relative_embedding(self):
        ws = self.window_size
        cord = torch.tensor([[i, j] for i in range(ws) for j in range(ws)])
        rel = (cord[:, None, :] - cord[None, :, :] + ws - 1).to(self.relative_position_params.device)
        return self.relative_position_params[:, rel[:, :, 0].long(), rel[:, :, 1].long()]

    def forward(self, x):   # [b, h, w, c]
        ws, nh = self.window_size, self.n_heads
        if self.type != "W":
            x = torch.roll(x, shifts=(-(ws // 2), -(ws // 2)), dims=(1, 2))
        b, H, W, c = x.shape
        hw, ww = H // ws, W // ws
        x = x.view(b, hw, ws, ww, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b, hw * ww, ws * ws, c)
        qkv = self.embedding_layer(x)                                                  # b nw np (3 nh hd)
        qkv = qkv.view(b, hw * ww, ws * ws, 3 * nh, self.head_dim).permute(3, 0, 1, 2, 4)   # (3 nh) b nw np hd
        q, k, v = qkv[:nh], qkv[nh:2 * nh], qkv[2 * nh:]
        sim = torch.einsum("hbwpc,hbwqc->hbwpq", q, k) * self.scale
        sim = sim + self.relative_embedding()[:, None, None]
        if self.type != "W":
            sim = sim.masked_fill_(self.generate_mask(hw, ww, ws, ws // 2, sim.device), float("-inf"))
        probs = torch.softmax(sim, dim=-1)
        out = torch.einsum("hbwij,hbwjc->hbwic", probs, v)
        out = out.permute(1, 2, 3, 0, 4).reshape(b, hw * ww, ws * ws, c)             # merge heads as (h c)
        out = self.linear(out)
        out = out.view(b, hw, ww, ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b, H, W, c)
        if self.type != "W":
            out = torch.roll(out, shifts=(ws // 2, ws // 2), dims=(1, 2))
        return out


class RefBlock(nn.Module):
    def __init__(self, input_dim, output_dim, head_dim, window_size, type, input_resolution):
        super().__init__()
        self.type = "W" if input_resolution <= window_size else type
        self.ln1 = nn.LayerNorm(input_dim)
        self.msa = RefWMSA(input_dim, input_dim, head_dim, window_size, self.type)
        self.ln2 = nn.LayerNorm(input_dim)
        self.mlp = nn.Sequential(nn.Linear(input_dim, 4 * input_dim), nn.GELU(), nn.Linear(4 * input_dim, output_dim))

    def forward(self, x):
        x = x + self.msa(self.ln1(x))
        return x + self.mlp(self.ln2(x))


class RefConvTransBlock(nn.Module):
    def __init__(self, conv_dim, trans_dim, head_dim, window_size, type, input_resolution):
        super().__init__()
        self.conv_dim, self.trans_dim = conv_dim, trans_dim
        c = conv_dim + trans_dim
        self.trans_block = RefBlock(trans_dim, trans_dim, head_dim, window_size, type, input_resolution)
        self.conv1_1 = nn.Conv2d(c, c, 1, 1, 0, bias=True)
        self.conv1_2 = nn.Conv2d(c, c, 1, 1, 0, bias=True)
        self.conv_block = nn.Sequential(nn.Conv2d(conv_dim, conv_dim, 3, 1, 1, bias=False), nn.ReLU(),
                                        nn.Conv2d(conv_dim, conv_dim, 3, 1, 1, bias=False))

    def forward(self, x):
        conv_x, trans_x = torch.split(self.conv1_1(x), (self.conv_dim, self.trans_dim), dim=1)
        conv_x = self.conv_block(conv_x) + conv_x
        trans_x = self.trans_block(trans_x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        return x + self.conv1_2(torch.cat((conv_x, trans_x), dim=1))


class RefSCUNet(nn.Module):
    def __init__(self, in_nc=3, config=(4, 4, 4, 4, 4, 4, 4), dim=64, input_resolution=256):
        super().__init__()
        hd, ws, res = 32, 8, input_resolution

        def blocks(n, c, r):
            return [RefConvTransBlock(c, c, hd, ws, "W" if not i % 2 else "SW", r) for i in range(n)]

        self.m_head = nn.Sequential(nn.Conv2d(in_nc, dim, 3, 1, 1, bias=False))
        self.m_down1 = nn.Sequential(*blocks(config[0], dim // 2, res), nn.Conv2d(dim, 2 * dim, 2, 2, 0, bias=False))
        self.m_down2 = nn.Sequential(*blocks(config[1], dim, res // 2), nn.Conv2d(2 * dim, 4 * dim, 2, 2, 0, bias=False))
        self.m_down3 = nn.Sequential(*blocks(config[2], 2 * dim, res // 4),
                                     nn.Conv2d(4 * dim, 8 * dim, 2, 2, 0, bias=False))
        self.m_body = nn.Sequential(*blocks(config[3], 4 * dim, res // 8))
        self.m_up3 = nn.Sequential(nn.ConvTranspose2d(8 * dim, 4 * dim, 2, 2, 0, bias=False),
                                   *blocks(config[4], 2 * dim, res // 4))
        self.m_up2 = nn.Sequential(nn.ConvTranspose2d(4 * dim, 2 * dim, 2, 2, 0, bias=False),
                                   *blocks(config[5], dim, res // 2))
        self.m_up1 = nn.Sequential(nn.ConvTranspose2d(2 * dim, dim, 2, 2, 0, bias=False), *blocks(config[6], dim // 2, res))
        self.m_tail = nn.Sequential(nn.Conv2d(dim, in_nc, 3, 1, 1, bias=False))

    def forward(self, x0):
        h, w = x0.shape[-2:]
        x0 = nn.ReplicationPad2d((0, -w % 64, 0, -h % 64))(x0)
        x1 = self.m_head(x0)
        x2 = self.m_down1(x1)
        x3 = self.m_down2(x2)
        x4 = self.m_down3(x3)
        x = self.m_body(x4)
        x = self.m_up3(x + x4)
        x = self.m_up2(x + x3)
        x = self.m_up1(x + x2)
        x = self.m_tail(x + x1)
        return x[..., :h, :w]


def ref_of(net, **kw):
    ref = RefSCUNet(in_nc=net.in_nc, config=net.config, dim=net.dim, input_resolution=net.input_resolution, **kw).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in net.state_dict().items()}, strict=True)
    return ref


def expected_keys(config, dim, in_nc):
    """(key, shape) in registration order, written out from the layout of the published definition."""
    out = [("m_head.0.weight", (dim, in_nc, 3, 3))]

    def block(p, c):
        t = f"{p}.trans_block"
        nh = c // 32
        return [(f"{t}.ln1.weight", (c,)), (f"{t}.ln1.bias", (c,)),
                (f"{t}.msa.relative_position_params", (nh, 15, 15)),
                (f"{t}.msa.embedding_layer.weight", (3 * c, c)), (f"{t}.msa.embedding_layer.bias", (3 * c,)),
                (f"{t}.msa.linear.weight", (c, c)), (f"{t}.msa.linear.bias", (c,)),
                (f"{t}.ln2.weight", (c,)), (f"{t}.ln2.bias", (c,)),
                (f"{t}.mlp.0.weight", (4 * c, c)), (f"{t}.mlp.0.bias", (4 * c,)),
                (f"{t}.mlp.2.weight", (c, 4 * c)), (f"{t}.mlp.2.bias", (c,)),
                (f"{p}.conv1_1.weight", (2 * c, 2 * c, 1, 1)), (f"{p}.conv1_1.bias", (2 * c,)),
                (f"{p}.conv1_2.weight", (2 * c, 2 * c, 1, 1)), (f"{p}.conv1_2.bias", (2 * c,)),
                (f"{p}.conv_block.0.weight", (c, c, 3, 3)), (f"{p}.conv_block.2.weight", (c, c, 3, 3))]

    for l in range(3):
        c = dim // 2 << l
        for i in range(config[l]):
            out += block(f"m_down{l + 1}.{i}", c)
        out.append((f"m_down{l + 1}.{config[l]}.weight", (4 * c, 2 * c, 2, 2)))
    for i in range(config[3]):
        out += block(f"m_body.{i}", 4 * dim)
    for k, l in enumerate((3, 2, 1)):
        c = dim // 2 << (l - 1)
        out.append((f"m_up{l}.0.weight", (4 * c, 2 * c, 2, 2)))     # ConvTranspose2d: [C_in, C_out, 2, 2]
        for i in range(config[4 + k]):
            out += block(f"m_up{l}.{1 + i}", c)
    out.append(("m_tail.0.weight", (in_nc, dim, 3, 3)))
    return out


@pytest.mark.parametrize("config,dim,in_nc", [([2] * 7, 64, 3), ([4] * 7, 64, 3), ([1, 2, 1, 3, 1, 2, 1], 128, 1)])
def test_state_dict_keys_and_shapes(config, dim, in_nc):
    net = SCUNet(in_nc=in_nc, config=config, dim=dim)
    sd = net.state_dict()
    want = expected_keys(config, dim, in_nc)
    assert list(sd) == [k for k, _ in want]
    for k, shape in want:
        assert tuple(sd[k].shape) == shape, k
    assert sd["m_down1.0.trans_block.msa.relative_position_params"].is_contiguous()
    ref_of(net)   # strict=True from the reference's side


def test_default_construction_and_block_types():
    net = SCUNet()
    assert net.config == [4] * 7 and net.dim == 64 and net.in_nc == 3
    assert [b.trans_block.type for b in list(net.m_down1)[:-1]] == ["W", "SW", "W", "SW"]
    heads = [net.m_down1[0], net.m_down2[0], net.m_down3[0], net.m_body[0]]
    assert [b.trans_block.msa.n_heads for b in heads] == [1, 2, 4, 8]
    assert [b.trans_dim for b in heads] == [32, 64, 128, 256]
    # input_resolution 64: the body level's resolution is 8 <= window_size, its Blocks are forced to 'W'
    small = SCUNet(config=[2] * 7, input_resolution=64)
    assert [b.trans_block.type for b in small.m_body] == ["W", "W"]
    assert [b.trans_block.type for b in list(small.m_up3)[1:]] == ["W", "SW"]


def test_unsupported_arguments_raise():
    with pytest.raises(NotImplementedError):
        SCUNet(drop_path_rate=0.1)
    with pytest.raises(NotImplementedError):
        SCUNet(dim=96)
    with pytest.raises(NotImplementedError):
        SCUNet(config=[2, 2, 2, 0, 2, 2, 2])
    with pytest.raises(RuntimeError):
        SCUNet(config=[1] * 7)(torch.rand(1, 3, 64, 64))     # no CPU path


@pytest.mark.parametrize("grid", [(1, 1), (1, 2), (2, 3), (4, 4)])
def test_sw_mask_equals_swin_calculate_mask(grid):
    """generate_mask(h, w, 8, 4) masks exactly the pairs Swin's calculate_mask gives -100 at shift 4 -- the partition the
    attention kernels compute analytically -- including grids one window wide."""
    h, w = grid
    m = WMSA(32, 32, 32, 8, "SW").generate_mask(h, w, 8, 4)[0, 0]             # [h*w, 64, 64] bool
    swin = _shift_mask(8 * h, 8 * w, 8, 4)                                     # [h*w, 64, 64], 0 / -100
    assert swin.shape == m.shape
    assert torch.equal(m, swin != 0)
    assert set(swin.unique().tolist()) <= {0.0, -100.0}
    assert not WMSA(32, 32, 32, 8, "W").generate_mask(h, w, 8, 4).any()
    assert torch.equal(m, RefWMSA(32, 32, 32, 8, "SW").generate_mask(h, w, 8, 4)[0, 0])


def test_relative_embedding_equals_swin_gather_on_transposed_table():
    ws, nh = 8, 4
    a = WMSA(32 * nh, 32 * nh, 32, ws, "W")
    with torch.no_grad():
        a.relative_position_params.copy_(torch.randn(nh, 15, 15))
    # Swin: relative_position_index of WindowAttention (coords[:, :, None] - coords[:, None, :], row * (2ws-1) + col)
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0) + (ws - 1)
    index = rel[:, :, 0] * (2 * ws - 1) + rel[:, :, 1]                         # [64, 64]
    ridx = a.relative_index()
    assert torch.equal(ridx[:, :, 0] * (2 * ws - 1) + ridx[:, :, 1], index)
    table = a.relative_position_params.detach().reshape(nh, -1).t().contiguous()   # the kernels' [(2ws-1)^2][nh]
    swin_bias = table[index.view(-1)].view(ws * ws, ws * ws, nh).permute(2, 0, 1)
    assert torch.equal(a.relative_embedding().detach(), swin_bias)


def test_reference_runs_in_float64_and_pads():
    torch.manual_seed(3)
    net = SCUNet(in_nc=1, config=[1] * 7, dim=64, input_resolution=64)
    ref = ref_of(net)
    x = torch.rand(1, 1, 40, 72, dtype=torch.float64)
    y = ref(x)
    assert y.shape == x.shape and y.dtype == torch.float64 and torch.isfinite(y).all()
    # the pad is the network's own: the same values as padding outside and cropping
    xp = nn.functional.pad(x, (0, 56, 0, 24), mode="replicate")
    assert torch.equal(ref(xp)[..., :40, :72], y)


def _opt(**netg):
    o = {"model": "plain", "is_train": False, "scale": 1,
         "netG": {"net_type": "scunet", "in_nc": 3, "config": [1] * 7, "dim": 64, "drop_path_rate": 0.0,
                  "input_resolution": 256, "init_type": "default"}, "train": {}}
    o["netG"].update(netg)
    return o


def test_define_g_and_compute_dtype():
    net = define_G(_opt())
    assert isinstance(net, SCUNet) and net.compute_dtype == "fp32" and net.config == [1] * 7
    o = _opt()
    o["train"]["amp_enabled"] = True
    assert compute_dtype_of(o) == "bf16" and define_G(o).compute_dtype == "bf16"
    with pytest.raises(ValueError, match="fp32x3"):
        define_G(_opt(compute_dtype="fp32x3"))
    with pytest.raises(ValueError):
        from kair_amd.engine.scunet_engine import SCUNetEngine
        SCUNetEngine(net, "fp32x3")
    with pytest.raises(NotImplementedError):
        define_G(_opt(drop_path_rate=0.2))


def test_grad_segments_tile_the_parameters():
    from kair_amd.engine.scunet_engine import SCUNetEngine
    from kair_amd.engine.trainer import segment_buckets
    net = SCUNet(config=[1] * 7)
    segs = SCUNetEngine.grad_segments(type("E", (), {"net_ref": lambda self: net})())
    buckets = segment_buckets(list(net.parameters()), segs)
    assert buckets is not None and len(buckets) == 7
    assert sum(hi - lo for lo, hi in buckets) == sum(p.numel() for p in net.parameters())
