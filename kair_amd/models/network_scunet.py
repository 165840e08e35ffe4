"""SCUNet -- the Swin-Conv-UNet denoiser (Zhang et al., "Practical Blind Denoising via Swin-Conv-UNet and Data
Synthesis"; the reference's models/network_scunet.py, the class define_G binds for net_type 'scunet').

The reference source was not available to this build: the module tree below is restated from the published definition
(WMSA / Block / ConvTransBlock / SCUNet), not read from the file.  It keeps the submodule names and parameter shapes, so
`state_dict` and scunet_color_*.pth / scunet_gray_*.pth style checkpoints load with strict=True:

  m_head.0, m_down{1,2,3}.{i} (ConvTransBlock) + m_down{l}.{config[l-1]} (2x2 stride-2 conv), m_body.{i},
  m_up{3,2,1}.0 (2x2 transposed conv) + m_up{l}.{1+i}, m_tail.0; every conv of the skeleton without bias;
  ConvTransBlock: conv1_1, conv1_2 (1x1, bias), conv_block.{0,2} (3x3, no bias), trans_block.{ln1, ln2,
  msa.{embedding_layer, linear, relative_position_params [n_heads, 2ws-1, 2ws-1]}, mlp.{0,2}}.

`forward` pads bottom / right to multiples of 64 by replication, runs the whole network as one autograd node on the HIP
step program (kair_amd/engine/scunet_engine.py) and crops back; there is no CPU path.

Departures from the reference:
  * the shifted-window mask adds -100 where the reference fills -inf (the attention kernels' constant, as for SwinIR):
    a masked pair keeps a weight of e^-100 relative to the row's largest, below every precision the engines have;
  * drop_path_rate > 0 raises NotImplementedError (the released configurations train with 0.0);
  * every entry of `config` must be >= 1 (the U-Net skips ride on the last block of a stage) and dim a multiple of 64
    (head_dim 32 at the full-resolution level);
  * relative_position_params is a contiguous [n_heads, 2ws-1, 2ws-1] Parameter initialised trunc_normal(std 0.02) (the
    reference builds the same shape as a transposed view of a [2ws-1, 2ws-1, n_heads] draw).
"""
import torch
import torch.nn as nn

from ..engine.scunet_engine import SCUNetEngine, SCUNetFunction

HEAD_DIM = 32
WINDOW_SIZE = 8
PAD_MODULO = 64


class WMSA(nn.Module):
    """Window multi-head self attention, type 'W' (plain windows) or 'SW' (windows shifted by ws // 2)."""

    def __init__(self, input_dim, output_dim, head_dim, window_size, type):
        super().__init__()
        if type not in ("W", "SW"):
            raise ValueError(f"WMSA type {type!r}")
        self.input_dim, self.output_dim, self.head_dim = input_dim, output_dim, head_dim
        self.scale = head_dim ** -0.5
        self.n_heads = input_dim // head_dim
        self.window_size = window_size
        self.type = type
        self.embedding_layer = nn.Linear(input_dim, 3 * input_dim, bias=True)
        self.relative_position_params = nn.Parameter(torch.zeros(self.n_heads, 2 * window_size - 1, 2 * window_size - 1))
        self.linear = nn.Linear(input_dim, output_dim)
        nn.init.trunc_normal_(self.relative_position_params, std=0.02)

    def generate_mask(self, h, w, p, shift):
        """Boolean mask [1, 1, h * w, p * p, p * p] (True: the pair is masked) of the 'SW' windows of an h x w window
        grid: in the last window row the pairs that straddle row s = p - shift, in the last window column those that
        straddle column s."""
        m = torch.zeros(h, w, p, p, p, p, dtype=torch.bool, device=self.relative_position_params.device)
        if self.type == "W":
            return m.view(1, 1, h * w, p * p, p * p)
        s = p - shift
        m[-1, :, :s, :, s:, :] = True
        m[-1, :, s:, :, :s, :] = True
        m[:, -1, :, :s, :, s:] = True
        m[:, -1, :, s:, :, :s] = True
        return m.view(1, 1, h * w, p * p, p * p)

    def relative_index(self):
        """[ws*ws, ws*ws, 2]: coordinate(query) - coordinate(key) + ws - 1, (row, column)."""
        ws = self.window_size
        cord = torch.tensor([[i, j] for i in range(ws) for j in range(ws)])
        return cord[:, None, :] - cord[None, :, :] + ws - 1

    def relative_embedding(self):
        """[n_heads, ws*ws, ws*ws]: the position bias of every (query, key) pair."""
        rel = self.relative_index().to(self.relative_position_params.device)
        return self.relative_position_params[:, rel[:, :, 0].long(), rel[:, :, 1].long()]


class Block(nn.Module):
    def __init__(self, input_dim, output_dim, head_dim, window_size, drop_path, type="W", input_resolution=None):
        super().__init__()
        if type not in ("W", "SW"):
            raise ValueError(f"Block type {type!r}")
        if drop_path > 0:
            raise NotImplementedError("kair_amd SCUNet: drop_path_rate > 0 is not implemented")
        self.input_dim, self.output_dim = input_dim, output_dim
        self.type = "W" if input_resolution <= window_size else type
        self.drop_path_rate = float(drop_path)
        self.ln1 = nn.LayerNorm(input_dim)
        self.msa = WMSA(input_dim, input_dim, head_dim, window_size, self.type)
        self.ln2 = nn.LayerNorm(input_dim)
        self.mlp = nn.Sequential(nn.Linear(input_dim, 4 * input_dim), nn.GELU(), nn.Linear(4 * input_dim, output_dim))


class ConvTransBlock(nn.Module):
    def __init__(self, conv_dim, trans_dim, head_dim, window_size, drop_path, type="W", input_resolution=None):
        super().__init__()
        self.conv_dim, self.trans_dim = conv_dim, trans_dim
        c = conv_dim + trans_dim
        self.trans_block = Block(trans_dim, trans_dim, head_dim, window_size, drop_path, type, input_resolution)
        self.conv1_1 = nn.Conv2d(c, c, 1, 1, 0, bias=True)
        self.conv1_2 = nn.Conv2d(c, c, 1, 1, 0, bias=True)
        self.conv_block = nn.Sequential(nn.Conv2d(conv_dim, conv_dim, 3, 1, 1, bias=False), nn.ReLU(True),
                                        nn.Conv2d(conv_dim, conv_dim, 3, 1, 1, bias=False))


class SCUNet(nn.Module):
    """compute_dtype is the engine option: 'fp32' (exact-MFMA) or 'bf16' (bf16 MFMA operands, fp32 accumulation)."""

    def __init__(self, in_nc=3, config=(4, 4, 4, 4, 4, 4, 4), dim=64, drop_path_rate=0.0, input_resolution=256,
                 compute_dtype="fp32"):
        super().__init__()
        config = list(config)
        if len(config) != 7:
            raise ValueError("SCUNet: config has seven entries (down1-3, body, up3-1)")
        if any(int(n) < 1 for n in config):
            raise NotImplementedError("kair_amd SCUNet: every config entry must be >= 1")
        if dim < 64 or dim % 64:
            raise NotImplementedError("kair_amd SCUNet: dim must be a multiple of 64")
        if in_nc > 8:
            raise NotImplementedError("kair_amd SCUNet: in_nc <= 8")
        if drop_path_rate > 0:
            raise NotImplementedError("kair_amd SCUNet: drop_path_rate > 0 is not implemented")
        self.config, self.dim, self.in_nc = config, dim, in_nc
        self.head_dim, self.window_size = HEAD_DIM, WINDOW_SIZE
        self.input_resolution = input_resolution
        hd, ws, res = HEAD_DIM, WINDOW_SIZE, input_resolution

        def blocks(n, c, r):   # c: conv_dim = trans_dim of the level
            return [ConvTransBlock(c, c, hd, ws, 0.0, "W" if not i % 2 else "SW", r) for i in range(n)]

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
        self.m_up1 = nn.Sequential(nn.ConvTranspose2d(2 * dim, dim, 2, 2, 0, bias=False),
                                   *blocks(config[6], dim // 2, res))
        self.m_tail = nn.Sequential(nn.Conv2d(dim, in_nc, 3, 1, 1, bias=False))
        self.compute_dtype = compute_dtype
        self.fused_block = None   # engine option: None (the engine's measured default), a bool, or {32: bool, 64: bool}
        self._engine = None
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def engine(self):
        if self._engine is None or self._engine.net_ref() is not self:
            self._engine = SCUNetEngine(self, self.compute_dtype, fused_block=self.fused_block)
        return self._engine

    def _apply(self, fn, *args, **kwargs):
        self._engine = None
        return super()._apply(fn, *args, **kwargs)

    def set_compute_dtype(self, dtype):
        self.compute_dtype = dtype
        self._engine = None
        return self

    def set_fused_block(self, fused_block):
        """Eval forwards of the bf16 engine with the one-launch narrow Block on / off (SCUNetEngine.fused_block)."""
        self.fused_block = fused_block
        self._engine = None
        return self

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("kair_amd SCUNet runs on the MI355X (HIP) only; got a CPU tensor (no CPU fallback)")
        return SCUNetFunction.run(self.engine(), x, list(self.parameters()))
