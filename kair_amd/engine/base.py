"""The step-program protocol: what FusedTrainer, the nn.Module wrappers and the autograd Functions expect of an
engine, and the plumbing every engine shares.

An engine is the launch sequence of one network over preallocated HBM buffers ("plans", plans.py).  Its drivers use
  forward(x, ...) -> the output buffer; sets `cur`, the plan the backward reads
  backward_from_loss(H, grads, loss_weight, charb_eps, loss_type) -> the device loss [1]    (FusedTrainer)
  backward_from_grad(gE, grads)                                                  (the autograd Functions)
  cur, plan_mode, _packed_version (reset by whoever changes the weights), repack_always
  blocks (objects with a drop-path rate .dp; empty without stochastic depth), drop_path_scales()
  x3, x3_backoff(), X3_AEXP / x3_gexp_off / x3_backoffs: the fp32x3 range guard
  seg_hook, and grad_segments() where the engine reports gradient segments (data-parallel buckets)
EngineBase holds all of it but the three launch sequences, and the GEMM launch layer they are written in (_nt, _wgrad:
the fp32x3 operand exponents are set there and nowhere else); ConvEngineBase adds the conv-net helpers.
"""
import math
import weakref

import torch

from .. import _hip as H
from .plans import Lease, PlanPool, autograd_mode, plan_mode


def _rup(x, m):
    return (x + m - 1) // m * m


class _Conv:
    """A 3x3 conv's packed forms: forward [Cop][9*Cip] and input-gradient [Cip][9*Cop].

    split (bf16 engines): the forward form holds a hi/lo bf16 pair per weight (pack kind 9,
    kair_operand.w_split), so the forward product sees the fp32 master weight to ~16 bits.  Plain
    bf16 weight rounding shifts every output pixel by the same sum(dW * a) and biases PSNR
    (DESIGN.md "parity at bf16"); activation rounding is unbiased and averages out."""

    def __init__(self, eng, mod, Cop, Cip, need_dgrad=True, split=None, n_perm=0, tied_in=False, fwd_cip=None,
                 narrow=False, wr=False, dil=1, dil_kernel=False):
        """n_perm = r*r: output channels stored sub-pixel-major for a following PixelShuffle(r)
        (kair_wmap.n_perm; the KAIR_OUT_PSHUF_SPM / PUNSHUF_SPM epilogues store 16 bytes at a time).
        tied_in: the forward form repeats the input channels in both halves of Cip (kair_wmap kG = 2),
        for an input held as a hi/lo pair in channels [0, Ci) and [Cip/2, Cip/2 + Ci)
        (kair_image_to_nhwc_hilo); the weight gradient keeps the plain map (the hi channels).
        fwd_cip: the forward form's packed input width when it differs from Cip (a [hi | lo] pair image of
        2 x Cip channels read through tied weights: the SwinIR tail under split_act).
        narrow: a 64 -> NR <= 4 conv run by the narrow-output kernels (kair_conv3x3_narrow_*): its forward
        form is pack kind 15 (16x16x32 fragment order, hi/lo halves), the backward reads the fp32 weight.
        wr: a 192 -> 192 conv also packed for kair_conv3x3_wr: forward pack kind 15, input gradient kind 16
        (fp32x3: kair_conv3x3_wr_x3's fp16 pairs, kinds 22 / 23).
        dil: the conv's dilation (padding = dilation); dil_kernel: also pack a dilated conv inside kair_conv3x3_dil's
        contract (plain bf16, dil 2..4, 64 -> 64) for that kernel: forward kind 15, input gradient kind 16."""
        self.w, self.b = mod.weight, mod.bias
        Co, Ci = self.w.shape[:2]
        self.Co, self.Ci, self.Cop, self.Cip = Co, Ci, Cop, Cip
        if split is None:
            split = getattr(eng, "split_conv", False)
        x3 = eng.x3
        self.split = (bool(split) and eng.tdt == torch.bfloat16) or x3
        self.x3 = x3
        self.n_perm = n_perm
        self.map = H.wmap(1, Co, Ci, (1, Co, Cop), (1, Ci, Cip), n_perm=n_perm)
        fcip = fwd_cip or Cip
        self.fcip = fcip
        kf_grp = (2, Ci, fcip // 2) if tied_in else (1, Ci, Cip)
        self.mapf = H.wmap(9 if self.split else 1, Co, Ci, (1, Co, Cop), kf_grp, n_perm=n_perm)
        self.mapd = H.wmap(2, Co, Ci, (1, Co, Cop), (1, Ci, Cip), n_perm=n_perm)
        self.mapb = H.wmap(4, Co, 0, (1, Co, Cop), (1, 1, 1), n_perm=n_perm)
        dev = self.w.device
        kf = 2 * _rup(9 * fcip, 64) if self.split else 9 * fcip
        self.Wf = torch.empty(Cop, kf, device=dev, dtype=torch.float16 if self.x3 else
                              (torch.bfloat16 if self.split else eng.tdt))
        self.narrow = bool(narrow)
        if self.narrow:   # the narrow kernels' forward form (their backward reads the fp32 master weight)
            self.mapn = H.wmap(15, Co, Ci, (1, Co, 16), (1, Ci, Cip))
            self.Wn = torch.empty(16, 2 * 9 * Cip, device=dev, dtype=torch.bfloat16)
        if self.x3:   # fp16 pairs of the dgrad form (pack kind 18)
            self.mapd = H.wmap(18, Co, Ci, (1, Co, Cop), (1, Ci, Cip), n_perm=n_perm)
            self.Wd = torch.empty(Cip, 2 * _rup(9 * Cop, 64), device=dev, dtype=torch.float16) if need_dgrad else None
        else:
            self.Wd = torch.empty(Cip, 9 * Cop, device=dev, dtype=eng.tdt) if need_dgrad else None
        self.bp = torch.empty(Cop, device=dev) if self.b is not None else None   # bias=False: no bias pack
        self.wr = bool(wr) and Cop == 192 and Cip == 192 and self.split
        # wr_pair: an upsampling conv (64 -> 256, sub-pixel-major rows) reading a [hi | lo] pair image
        self.wr_pair = bool(wr) and not self.wr and tied_in and Cip == 64 and fcip == 128 and Cop == 256 and self.split
        if self.wr_pair:   # + its input-gradient form (kind 16, rows = the 64 input channels)
            self.mapp = H.wmap(15, Co, Ci, (1, Co, Cop), (1, Ci, Cip), n_perm=n_perm)
            self.Wp15 = torch.empty(Cop * 2 * 9 * Cip, device=dev, dtype=torch.bfloat16)
            self.mapp16 = H.wmap(16, Co, Ci, (1, Co, Cop), (1, Ci, Cip), n_perm=n_perm)
            self.Wp16 = torch.empty(Cip * 9 * Cop, device=dev, dtype=torch.bfloat16)
        # wr_n64: conv_before_upsample (192 -> 64) on kair_conv3x3_wr's N <= 64 form
        self.wr_n64 = (bool(wr) and not self.wr and not self.wr_pair and Cop == 64 and Cip == 192 and self.split and
                       not tied_in and not self.x3)
        if self.wr_n64:
            self.mapc = H.wmap(15, Co, Ci, (1, Co, Cop), (1, Ci, Cip))
            self.Wc15 = torch.empty(Cop * 2 * 9 * Cip, device=dev, dtype=torch.bfloat16)
            self.mapc16 = H.wmap(16, Co, Ci, (1, Co, Cop), (1, Ci, Cip))
            self.Wc16 = torch.empty(Cip * 9 * Cop, device=dev, dtype=torch.bfloat16)
        self.dil = int(dil)
        self.dil_fast = (bool(dil_kernel) and self.dil > 1 and eng.tdt == torch.bfloat16 and not self.split and
                         not n_perm and not tied_in and H.conv3x3_dil_ok(self.dil, Cip, Cop))
        if self.dil_fast:
            self.mapk15 = H.wmap(15, Co, Ci, (1, Co, Cop), (1, Ci, Cip))
            self.Wk15 = torch.empty(Cop * 2 * 9 * Cip, device=dev, dtype=torch.bfloat16)
            self.mapk16 = H.wmap(16, Co, Ci, (1, Co, Cop), (1, Ci, Cip))
            self.Wk16 = torch.empty(Cip * 9 * Cop, device=dev, dtype=torch.bfloat16) if need_dgrad else None
        if self.wr and self.x3:   # fp16 pairs of w 2^KAIR_X3_WEXP in fragment order (same element counts)
            self.map15 = H.wmap(22, Co, Ci, (1, Co, Cop), (1, Ci, Cip))
            self.Wf15 = torch.empty(Cop * 2 * 9 * Cip, device=dev, dtype=torch.float16)
            self.map16 = H.wmap(23, Co, Ci, (1, Co, Cop), (1, Ci, Cip))
            self.Wd16 = torch.empty(Cip * 2 * 9 * Cop, device=dev, dtype=torch.float16)
        elif self.wr:
            self.map15 = H.wmap(15, Co, Ci, (1, Co, Cop), (1, Ci, Cip))
            self.Wf15 = torch.empty(Cop * 2 * 9 * Cip, device=dev, dtype=torch.bfloat16)
            self.map16 = H.wmap(16, Co, Ci, (1, Co, Cop), (1, Ci, Cip))
            self.Wd16 = torch.empty(Cip * 9 * Cop, device=dev, dtype=torch.bfloat16)

    def fwd(self):
        """The forward GEMM's B operand."""
        return H.rows(self.Wf, w_split=self.split)

    def pack_jobs(self):
        w = self.w.detach()
        jobs = [(w, self.Wf, self.mapf)]
        if self.b is not None:
            jobs.append((self.b.detach(), self.bp, self.mapb))
        if self.Wd is not None:
            jobs.append((w, self.Wd, self.mapd))
        if self.narrow:
            jobs.append((w, self.Wn, self.mapn))
        if self.wr:
            jobs += [(w, self.Wf15, self.map15), (w, self.Wd16, self.map16)]
        if self.wr_pair:
            jobs += [(w, self.Wp15, self.mapp), (w, self.Wp16, self.mapp16)]
        if self.wr_n64:
            jobs += [(w, self.Wc15, self.mapc), (w, self.Wc16, self.mapc16)]
        if self.dil_fast:
            jobs.append((w, self.Wk15, self.mapk15))
            if self.Wk16 is not None:
                jobs.append((w, self.Wk16, self.mapk16))
        return jobs


class EngineBase:
    COMPUTE_DTYPES = ()      # the compute dtypes the engine implements, of "bf16", "fp32", "fp32x3"
    X3_AEXP = 4              # fp32x3 activation exponent (default; per engine: self.X3_AEXP, lowered by x3_backoff)
    X3_BACKOFF_STEP = 6      # exponent drop per range-guard event (x 1/64)
    X3_BACKOFF_MAX = 4       # events before the guard gives up and raises

    def __init__(self, net, compute_dtype):
        """No device work: the subclass sets `device`, `cd` (its kernels' compute enum) and its layer objects."""
        if compute_dtype not in self.COMPUTE_DTYPES:
            raise ValueError(f"{type(self).__name__}: compute_dtype {compute_dtype!r} (implemented: {self.COMPUTE_DTYPES})")
        self.net_ref = weakref.ref(net)
        # fp32x3: the fp32 reference's arithmetic on the 16-bit matrix cores -- every contraction multiplies
        # fp16 pairs of power-of-2-scaled operands (hi.hi + hi.lo + lo.hi, fp32 accumulation; ~2^-21 relative
        # per product), activations and gradients fp32 in HBM.  Exponents put the bulk of every operand at
        # 2^2 .. 2^10 -- the lo half (2^-11 of the value) then stays a normal fp16 number (>= 2^-14) while the
        # largest values keep >= 16x headroom below fp16's 65504: weights KAIR_X3_WEXP (packs: |w| ~ 0.02 -> ~2^6),
        # activations X3_AEXP (O(1) -> 2^4), gradients P["e_g"] (the loss normalisation, _x3_grad_exp)
        self.x3 = compute_dtype == "fp32x3"
        self.tdt = torch.bfloat16 if compute_dtype == "bf16" else torch.float32
        # x3 exponents of the activation class and of the gradient class (offset over the loss normalisation);
        # lowered by x3_backoff() when the range guard sees an operand leave fp16's window
        self.X3_AEXP = type(self).X3_AEXP
        self.x3_gexp_off = 4
        self.x3_backoffs = 0
        self._ax = self.X3_AEXP   # the exponent of the GEMM A operands / fp16 outputs of the phase being issued
        self.plans = PlanPool(self._build_plan)
        self.plan_mode = "primary"
        self._packed_version = None
        self._pack_table = None
        self.blocks = []          # the blocks with stochastic depth (drop_path_scales); none in the conv nets
        self.seg_hook = None      # called between the gradient segments of backward() (grad_segments())
        # repack_always: an engine whose parameters are updated outside torch (the fused trainer's Adam
        # kernel writes the flat parameter buffer; versions do not move) and that no step graph repacks
        # -- the eval-mode twin (SwinIR.eval_engine)
        self.repack_always = False

    def convs(self):
        """The layer objects whose pack_jobs() make up the weight packs."""
        raise NotImplementedError

    def _build_plan(self, key, infer):
        raise NotImplementedError

    def plan(self, *key):
        return self.plans.get(key, self.plan_mode)

    def pack_jobs(self):
        return [j for c in self.convs() for j in c.pack_jobs()]

    def pack(self, force=False):
        """Refresh the packed weight forms (one batched launch) when a parameter's version moved."""
        net = self.net_ref()
        ver = None if force or self.repack_always else tuple(p._version for p in net.parameters())
        if ver is not None and ver == self._packed_version:
            return
        ptrs = tuple(p.data_ptr() for p in net.parameters())
        if self._pack_table is None or self._pack_table[0] != ptrs:   # params re-homed (e.g. flattened)
            self._pack_table = (ptrs, H.PackTable(self.pack_jobs()))
        self._pack_table[1].run()
        self._packed_version = ver

    def _e(self, *shape, dt=torch.float32):
        return torch.empty(*shape, device=self.device, dtype=dt)

    def _segment_done(self):
        if self.seg_hook is not None:
            self.seg_hook()

    # ---- the GEMM launch layer: kair_gemm_nt / kair_gemm_tn in the engine's arithmetic --------
    @property
    def tn_cd(self):
        """The compute enum of kair_gemm_tn (the weight gradients): `cd`, under fp32x3 KAIR_COMPUTE_X3."""
        return H.X3 if self.x3 else self.cd

    def _nt(self, A, B, E, M, N, K):
        """kair_gemm_nt in `cd`; under fp32x3 the split-fp16 arithmetic (compute KAIR_COMPUTE_X3): A is fp32 (split in
        the kernel) or an fp16 pair (its lo plane attached with H.with_lo) carrying the phase exponent `_ax` (forward
        the activation exponent, backward the gradient exponent), B a split-packed fp16 weight (2^KAIR_X3_WEXP), an
        fp16 output the pair of v 2^(phase exponent)."""
        if not self.x3:
            H.gemm_nt(A, B, E, M, N, K, self.cd)
            return
        if A.dtype == H.F16 and not A.lo_ptr:
            raise RuntimeError("fp32x3: an fp16 GEMM operand needs its lo plane")
        if A.ones_col >= 0:
            raise RuntimeError("fp32x3: no injected ones column on a GEMM A operand")
        A.x3_exp, B.x3_exp = self._ax, H.X3_WEXP
        if E.out_dtype == H.F16:
            E.x3_out_exp = self._ax
        H.gemm_nt(A, B, E, M, N, K, H.X3)

    def _wgrad(self, P, A, Bop, M, N, K, wmap, grad, bgrad=None, ones_col=-1, ws=None, max_ctas=0, acc=False,
               act_rows=False):
        """One weight gradient A^T Bop over M rows: kair_gemm_tn into split partial planes (workspace ws, default
        P["wg_ws"]), then the deterministic kair_wgrad_finalize into `grad` in the layout of wmap (added to it with
        acc; bgrad: the bias gradient from the operand's ones column ones_col).  max_ctas > 0: at most that many
        (tile, split) workgroups; < 0: -max_ctas times the splits.  fp32x3: (gradient, activation) operands, or
        (activation, gradient) with act_rows (the transposed conv)."""
        S = H.wgrad_splits(M, N, K)
        if max_ctas > 0:   # fewer row splits
            S = max(1, min(S, max_ctas // H.wgrad_tiles(N, K)))
        elif max_ctas < 0:   # more, shorter ones (>= 32 rows each)
            S = min(S * -max_ctas, -(-M // 32))
        if self.x3:
            eg, ea = P.get("e_g", 0), self.X3_AEXP
            A.x3_exp, Bop.x3_exp = (ea, eg) if act_rows else (eg, ea)
        ws = P["wg_ws"] if ws is None else ws
        H.gemm_tn(A, Bop, ws, S, M, N, K, self.tn_cd)
        H.wgrad_finalize(ws, S, wmap, grad, bgrad, ones_col, accumulate=acc)

    # ---- fp32x3 exponents and the range guard's reaction --------------------------------------
    def _x3_grad_exp(self, numel, weight=1.0, loss_type=None):
        """The fp32x3 gradient exponent: the mean-loss gradient is O(weight / numel) per output element (weight: the
        loss weight over img_range), so data gradients times 2^(log2(numel / weight) + 4) sit near 2^4 at the loss,
        2^12 below fp16's overflow.  'ssim': numel |dS/dE| is not bounded by 1 -- X3_SSIM_HEADROOM binades lower.
        'l2': the gradient 2 weight (E - H) / numel is bounded by 2 |weight| / numel for images in [0, 1], twice
        L1's |weight| / numel, so the same derivation gives L1's exponent less one binade and the bound sits at 2^4 as
        L1's constant does (typical gradients, |E - H| << 1, lie below it).  'l2sum': no division by numel, the bound
        is 2 |weight|: 'l2' at numel = 1.  The range guard stays the backstop."""
        if loss_type == "l2sum":
            numel = 1
        e = int(round(math.log2(max(numel, 1) / max(abs(weight), 1e-30)))) + self.x3_gexp_off
        if loss_type in ("l2", "l2sum"):
            return e - 1
        return e - self.X3_SSIM_HEADROOM if loss_type == "ssim" else e

    # numel |dS/dE| of the SSIM loss: <= ~4 / C2 + 1 / sqrt(C1) ~ 2^12 for images in [0, 1] (flat patches that differ
    # by a constant; 2^6.3 measured on such a pair), <= 2^5.1 measured in float64 over the SSIM tests' inputs and
    # crops of the golden test images ("SSIM loss").  6 binades put the measured worst case at
    # 2^(4 + 5.1 - 6) ~ 2^3 at the loss, beside L1's 2^4, and the analytic worst case at 2^10 < fp16's 2^16; typical
    # gradients (numel |dS/dE| ~ 1) drop to 2^-2, their lo halves (2^-13) still normal fp16 numbers (>= 2^-14).
    # The range guard stays the backstop.
    X3_SSIM_HEADROOM = 6

    def pixel_loss(self, P, E, H_img, dE, ldc, weight, C, Hh, Ww, ps_r=1, charb_eps=None, loss_type=None):
        """The one dispatch of every engine's loss hook: loss_type None / 'l1' / 'charbonnier' (charb_eps set) ->
        kair_l1_loss / kair_charbonnier_loss; 'l2' / 'l2sum' -> kair_l2_loss (mean / sum); 'ssim' -> kair_ssim_loss,
        whose workspace joins the plan on the first SSIM step (an eager warm-up step: before any capture), so L1 plans stay as they were.  Loss into P['loss'],
        gradient rows into dE."""
        if loss_type == "ssim":
            ws = P.get("ssim_ws")
            if ws is None:
                ws = P["ssim_ws"] = H.ssim_workspace(P["B"], C, Hh, Ww, self.device)
            H.ssim_loss(E, H_img, P["loss"], dE, ldc, weight, P["B"], C, Hh, Ww, ws, ps_r=ps_r)
        elif loss_type in (None, "l1", "charbonnier"):
            H.l1_loss(E, H_img, P["loss"], dE, ldc, weight, P["B"], C, Hh, Ww, P["loss_ws"], ps_r=ps_r,
                      charb_eps=charb_eps)
        elif loss_type in ("l2", "l2sum"):
            H.l2_loss(E, H_img, P["loss"], dE, ldc, weight, P["B"], C, Hh, Ww, P["loss_ws"], ps_r=ps_r,
                      reduction="sum" if loss_type == "l2sum" else "mean")
        else:
            raise NotImplementedError(f"fused pixel loss {loss_type!r}")

    @staticmethod
    def x3_upstream_grad_exp(mx):
        """The gradient exponent for an arbitrary upstream gradient of largest magnitude mx: max -> <= 2^8."""
        return 8 - int(math.ceil(math.log2(mx))) if mx > 0 and math.isfinite(mx) else 0

    def _x3_set_grad_exp(self, P, gE, scale=1.0, e_off=0):
        """backward_from_grad under fp32x3: P["e_g"] from the range of the upstream gradient scale * gE itself (one
        host sync; none off fp32x3), shifted by e_off."""
        if self.x3:
            P["e_g"] = self.x3_upstream_grad_exp(float(gE.abs().max()) * scale) + e_off

    def x3_backoff(self, step=None, act=True, grad=True):
        """Range guard reaction (kair_range_check saw an inf / NaN the split operands can cause): lower the activation
        exponent (act: a forward overflow, the loss went non-finite) and / or the gradient exponent (grad: a backward
        overflow) by `step` (default X3_BACKOFF_STEP), so that operand class gains that much headroom below fp16's
        65504 (the lo halves of its smallest values go subnormal first: an absolute error <= 2^-25 of the scaled
        unit).  The caller re-runs the step (re-captured graph).  Raises after X3_BACKOFF_MAX events: the data is not
        finite in fp32 either, or a weight left its pack window."""
        if not self.x3:
            raise RuntimeError("x3_backoff: not an fp32x3 engine")
        if self.x3_backoffs >= self.X3_BACKOFF_MAX:
            raise RuntimeError(f"fp32x3 range guard: the step is still non-finite after {self.x3_backoffs} exponent "
                               f"back-offs (activation 2^{self.X3_AEXP}, gradient offset 2^{self.x3_gexp_off}): the data "
                               f"is not finite, or a weight left its pack window |w| < 2^{16 - H.X3_WEXP}")
        step = self.X3_BACKOFF_STEP if step is None else int(step)
        if act:
            self.X3_AEXP -= step
        if grad:
            self.x3_gexp_off -= step
        self.x3_backoffs += 1
        return self.X3_AEXP, self.x3_gexp_off


class ConvEngineBase(EngineBase):
    """Shared plumbing of the conv-net step programs: the conv weight-gradient helpers.  fp32x3: cd stays F32 for the
    fp32-rows bookkeeping (gate_cast), the launches go through _nt / _wgrad with compute KAIR_COMPUTE_X3."""

    def __init__(self, net, compute_dtype):
        super().__init__(net, compute_dtype)
        self.cd = H.BF16 if compute_dtype == "bf16" else H.F32

    def conv_wgrad(self, P, c, dz, ld_dz, src_op, M, grads, bias_src=None, ld_bias=None):
        """weight + bias gradient of conv c: dz [M, Cop] rows (compute dtype), src_op its im2col input;
        bias_src: the fp32 rows dz was cast from (bias gradient summed before rounding)."""
        self._wgrad(P, H.rows(dz, ld=ld_dz), src_op, M, c.Cop, 9 * c.Cip, c.map, grads[c.w])
        if c.b is None:   # a conv without bias: no column sum, no gradient entry
            return
        if bias_src is None:
            bias_src, ld_bias = dz, ld_dz
        H.colsum(H.rows(bias_src, ld=ld_bias), M, c.Cop, c.mapb, grads[c.b], P["colsum_ws"])

    def gate_cast(self, P, G, ldg, X, ldx, out, ldo, M, C, kind, slope=0.0, scale=1.0):
        """out (compute dtype) = scale * G * act'(X).  Returns the fp32 rows to take the bias gradient
        from: `out` itself in fp32 mode, else an fp32 scratch holding the values before rounding."""
        if self.cd == H.F32:
            H.act_grad_cast(G, ldg, X, ldx, out, ldo, M, C, kind, slope, scale)
            return out, ldo
        f = P["dzf"].view(-1)[:M * C].view(M, C)
        H.act_grad_cast(G, ldg, X, ldx, f, C, M, C, kind, slope, scale)
        H.row_copy(f, C, M, C, H.copy_desc(out, ld=ldo))
        return f, C

    def wgrad_ws_size(self, shapes):
        return max(H.wgrad_splits(m, n, k) * n * k for m, n, k in shapes)


def drop_path_scales(engine, B, device, generator=None):
    """Per-block, per-branch stochastic-depth scales (timm DropPath semantics: keep-mask / keep)."""
    keep = getattr(engine, "_keep", None)
    if keep is None or keep.device != torch.device(device):   # built once, outside any graph capture
        rates = torch.tensor([b.dp for b in engine.blocks], dtype=torch.float32)
        keep = engine._keep = (1.0 - rates).view(-1, 1, 1).to(device)
    u = torch.rand(len(engine.blocks), 2, B, device=device, generator=generator)
    return (u < keep).float() / keep


def lease_grads(ctx, gE):
    """First step of an engine Function's backward: check that the node still holds its plan, make it the engine's
    current one, and carve one flat fp32 buffer into per-parameter gradient views -> (flat, {param: view})."""
    if ctx.lease is None or ctx.lease.plan is None:
        raise RuntimeError("kair_amd: backward through a forward whose activations were released "
                           "(a second backward needs retain_graph-style reuse, which is not supported)")
    flat = torch.empty(sum(p.numel() for p in ctx.params), device=gE.device)
    grads, off = {}, 0
    for p in ctx.params:
        grads[p] = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    ctx.engine.cur = ctx.lease.plan
    return flat, grads


class ConvNetFunction(torch.autograd.Function):
    """A whole conv network (RRDBNet / DnCNN / FFDNet / DRUNet / USRNet) as one autograd node on its step program; the
    node leases its plan from forward to backward (kair_amd/engine/plans.py)."""

    @classmethod
    def run(cls, engine, x, params, *cond):
        """cond: extra, non-differentiable forward inputs handed to engine.forward after x (FFDNet: sigma; USRNet: k,
        sf, sigma)."""
        return cls.apply(engine, autograd_mode(params), len(cond), x, *cond, *params)

    @staticmethod
    def forward(ctx, engine, mode, n_cond, x, *rest):
        cond, params = rest[:n_cond], rest[n_cond:]
        with plan_mode(engine, mode):
            E = engine.forward(x.float().contiguous(), *cond)
        ctx.engine, ctx.params, ctx.n_cond = engine, params, n_cond
        ctx.lease = Lease(engine.cur) if mode == "lease" else None
        return E.clone()

    @staticmethod
    def backward(ctx, gE):
        _, grads = lease_grads(ctx, gE)
        ctx.engine.backward_from_grad(gE.float(), grads)
        ctx.lease.release()
        return (None,) * (4 + ctx.n_cond) + tuple(grads[p] for p in ctx.params)
