"""Autograd over the HIP kernels -- first slice of the training path (BASELINE config 5; the reference's training step is
tools/train_video_controlnet.py:451-488: ControlNet forward + backward with fp32 master parameters under bf16 compute).

Scope of this slice ("smallest verifiable slice"): the gather-GEMM family (nn.Linear / 1x1 conv
incl. the ControlNet zero-convs, 3x3 Conv2d, (3,1,1) Conv3d) with its fused epilogue operands {bias, residual R1,
per-clip row vector V, s_acc}, GroupNorm(+SiLU) in its 4-D and 5-D forms, and the folded AlphaBlender -- i.e. a complete
`SpatioTemporalResBlock` and the zero-convs -- checked against torch.autograd on the oracle (tests/test_backward_gpu.py).

  dgrad  = the forward kernel on role-swapped weights (Linear: W^T; convs: taps reversed, channels transposed)
  wgrad  = ctrlv_gemm_wgrad (transposed-LDS-read MFMA kernel), bias / row-vector gradients = ctrlv_colsum
  norms  = ctrlv_groupnorm_bwd on the statistics the forward saved
Activations and activation gradients are 16-bit rows of ONE element type per call -- bf16, or fp16 where the input rows are fp16
(every allocation takes the type of the rows it belongs to, `ops` picks the library by it, and the cached packed forms of frozen
parameters key on it) --; parameter gradients are fp32 in the PyTorch layouts.
Second slice: LayerNorm, GEGLU, the attention cores (flash-style backward, csrc/attention_bwd.hip), the second residual
and the indexed row vector of the epilogue => a complete `TransformerSpatioTemporalModel`; stride-2 and upsample-fused
convs; LoRA factors.  The model-level training step built from these lives in ctrlv_amd/training.py.

Every GEMM of the step is one of two Functions over one forward launcher (`_gemm_forward`) and one backward
(`gemm_grads`, `_epilogue_grads`): `Gemm` (every mode, every epilogue operand, optional trailing LoRA factors; geometry
and scalars in a `GemmSpec`) and `BlendGemm` (the two AlphaBlender foldings, which add the mix-factor gradient).  Forms
derived from frozen parameters are cached in ctrlv_amd/frozen.py.
"""
import contextlib
import math
from typing import NamedTuple

import torch

from . import frozen as frozen_cache, lora as lora_mod, ops, packing
from .frozen import frozen


_ELEMENT_TYPES = (torch.bfloat16, torch.float16)


def _el(t):
    """The element type of the rows `t` belongs to: its own 16-bit type (bf16 for anything else)."""
    return t.dtype if t.dtype in _ELEMENT_TYPES else torch.bfloat16


def _rows(M, C, like):
    return torch.empty(M, C, dtype=_el(like), device=like.device)


def clear_pack_cache():
    """Drops every cached form of the frozen parameters (frozen.py).  Writes through `.data` do not bump _version: call this
    after editing a frozen model that way."""
    frozen_cache.clear()


def _packed(weight, kind, fn):
    return frozen((weight,), kind, lambda: fn(weight))


def f32(p):
    """fp32 form of a parameter for the per-clip torch ops and the norm kernels: trainable / fp32 parameters as they are
    (autograd sees them; an fp32 parameter IS its fp32 form, and a value must never be its own source), FROZEN 16-bit ones
    converted once (the UNet of the training step: ~500 small conversion kernels per step otherwise)."""
    if p.dtype == torch.float32:
        return p.float()
    return frozen((p,), "f32", lambda: p.float().contiguous())


def _geglu_bias32(bias):
    return _packed(bias, "geglu_b32", lambda b: packing.geglu_interleave(b.detach()).float().contiguous())


def _bias32(bias):
    """padded fp32 bias row of a GEMM launch (packing.pad_bias); cached for frozen parameters"""
    return _packed(bias, "bias32", packing.pad_bias)


def _pack_fwd(weight, mode, geglu=False, el=torch.bfloat16):
    """Forward GEMM layout of a parameter in the element type `el`: one kernel (ctrlv_pack_weight) where the shape allows, else
    packing.py."""
    out = ops.pack_weight(weight, 0, geglu, el) if weight.is_cuda else None
    if out is not None:
        return out
    with packing.element_dtype(el):
        if geglu:
            return packing.pack_geglu(weight, weight.new_zeros(weight.shape[0]))[0]
        return (packing.pack_linear if mode == 0 else (packing.pack_conv3x3 if mode == 1 else packing.pack_conv_temporal))(weight)


def _packed_fwd(weight, mode, el):
    """... cached per element type for frozen parameters: the same model may be stepped in either type"""
    return _packed(weight, ("fwd", mode, el), lambda w: _pack_fwd(w, mode, el=el))


def _packed_geglu(weight, el):
    return _packed(weight, ("fwd_geglu", el), lambda w: _pack_fwd(w, 0, geglu=True, el=el))


_TAPS = {0: 1, 1: 9, 2: 3}


class GemmSpec(NamedTuple):
    """Geometry and epilogue scalars of one gather-GEMM: out = s_acc * (gemm + bias) + s1 * R1 + s2 * R2 + V[idx(m)]."""
    mode: int = 0                # 0 nn.Linear / 1x1 conv, 1 3x3 Conv2d, 2 (3,1,1) Conv3d
    conv: tuple = None           # mode 1: (H, W, Ho, Wo, stride, up)
    temporal: tuple = None       # mode 2: (F, S)
    s_acc: float = 1.0
    s1: float = 1.0
    s2: float = 1.0
    vmode: int = 1               # 1: idx = (m // vdiv) % vmod;  2: ((m // vdiv) * vS + m % vS) % vmod
    vdiv: int = 1
    vmod: int = 1 << 30
    vS: int = 1
    lora: tuple = None           # (groups, s) when LoRA factors trail the inputs of Gemm

    @property
    def geom(self):
        return dict(mode=self.mode, conv=self.conv, temporal=self.temporal)


def _gemm_forward(A, weight, bias, R1, R2, V, spec):
    """The forward launch of Gemm and BlendGemm.  weight / bias: parameters in the PyTorch layout ([N, C], [N, C, 3, 3] or
    [N, C, 3, 1, 1]), any float dtype; the output is as wide as the weight, the launch's N is padded to 32."""
    mode = spec.mode
    N, cin = weight.shape[0], weight.shape[1]
    m_out = A.shape[0]
    if mode == 1:        # stride-2 / upsample-fused convs change the row count
        H, W, Ho, Wo = spec.conv[:4]
        m_out = A.shape[0] // (H * W) * Ho * Wo
    out = _rows(m_out, N, A)
    ops.gemm(A, _packed_fwd(weight, mode, _el(A)), out, N=(N + 31) // 32 * 32, cin=cin,
             taps=_TAPS[mode], mode=mode, conv=spec.conv, temporal=spec.temporal,
             bias=None if bias is None else _bias32(bias), s_acc=float(spec.s_acc), R1=R1, s1=float(spec.s1), R2=R2,
             s2=float(spec.s2), V=V, vmode=spec.vmode if V is not None else 0, vdiv=spec.vdiv, vmod=spec.vmod, vS=spec.vS)
    return out


def _scaled(dy, s):
    """s * dy as a new bf16 tensor (dy itself when s == 1)."""
    if s == 1.0:
        return dy
    out = torch.empty_like(dy)
    ops.axpby(dy, dy, float(s), 0.0, out)
    return out


def _epilogue_grads(dY, spec, need_r1, need_r2, vshape):
    """(dR1, dR2, dV) of the epilogue operands for the upstream gradient dY; vshape: V's shape, None = not wanted."""
    dR1 = _scaled(dY, spec.s1) if need_r1 else None
    dR2 = _scaled(dY, spec.s2) if need_r2 else None
    dV = None
    if vshape is not None:
        dV = torch.zeros(vshape, dtype=torch.float32, device=dY.device)
        vmod = min(spec.vmod, vshape[0])
        if spec.vmode == 1 and (spec.vdiv % 4 == 0 or not ops.DETERMINISTIC):
            ops.colsum(dY, dV, vmode=1, vdiv=spec.vdiv, vmod=vmod)
        elif spec.vmode == 2 and spec.vS % spec.vmod == 0 and spec.vdiv % spec.vmod == 0:
            # vidx = ((m // vdiv) * vS + m % vS) % vmod (the diffusers-0.27.2 (s, b) context order): with vS and
            # vdiv multiples of vmod this is m % vmod -- table row j collects every vmod-th row starting at j
            for j in range(spec.vmod):
                ops.colsum(dY[j::spec.vmod], dV[j:j + 1])
        else:
            _row_vector_grad_by_table_row(dY, dV, spec)
    return dR1, dR2, dV


def _row_vector_grad_by_table_row(dY, dV, spec):
    """dV for the index maps the two fast forms do not serve -- vmode 2 with vS or vdiv no multiple of vmod (B = 3 clips in
    the (s, b) context order), and vmode 1 with a row group that is no multiple of 4, which ctrlv_colsum serves with fp32
    atomics only: one ordered column sum per table row over the rows whose index is that row.  The row lists come from the
    host (no read of the device); shapes of this kind are small or rare, the gather copy is not on the hot path."""
    m = torch.arange(dY.shape[0])
    if spec.vmode == 1:
        idx = (m // spec.vdiv) % spec.vmod
    else:
        idx = ((m // spec.vdiv) * spec.vS + m % spec.vS) % spec.vmod
    for j in range(dV.shape[0]):
        sel = (idx == j).nonzero().flatten()
        if sel.numel():
            ops.colsum(dY.index_select(0, sel.to(dY.device)), dV[j:j + 1])


class Gemm(torch.autograd.Function):
    """out = s_acc * (gather-GEMM(A, weight) + bias) + s1 * R1 + s2 * R2 + V[idx(m)]: nn.Linear / 1x1 conv, 3x3 Conv2d
    (stride 2 and upsample-fused too) and (3,1,1) Conv3d with every epilogue operand the blocks fuse (residuals, the
    per-clip time-embedding / cross-attention vector, the frame positional embedding).  spec: GemmSpec.

    LoRA (spec.lora = (groups, s), factors = A_0, B_0, A_1, B_1, ...: one pair per group of weight's rows -- an nn.Linear,
    or the g = 3 fused q|k|v projection): forward and dgrad run on the merged weight W' = W + s . B_i . A_i (built once per
    forward in fp32 and packed to the element type, exactly how a trainable fp32 master is used); dA_i / dB_i come from
    ctrlv_lora_grad (csrc/lora.hip) without forming dW; dW of the base only if the base itself requires grad."""

    @staticmethod
    def forward(ctx, A, weight, bias, R1, R2, V, spec, *factors):
        wm = _lora_merged(weight, factors, *spec.lora) if factors else weight
        out = _gemm_forward(A, wm, bias, R1, R2, V, spec)
        ctx.save_for_backward(A, wm, *factors)
        ctx.spec, ctx.wdtype = spec, weight.dtype
        ctx.has = (bias is not None, R1 is not None, R2 is not None, None if V is None else tuple(V.shape))
        return out

    @staticmethod
    def backward(ctx, dY):
        A, wm, *factors = ctx.saved_tensors
        spec, need = ctx.spec, ctx.needs_input_grad
        has_b, has_r1, has_r2, vshape = ctx.has
        dY = dY.contiguous()
        dA, dW, db = gemm_grads(A, wm, dY, spec.geom, spec.s_acc, need[0], need[1], has_b and need[2])
        if dW is not None:
            dW = dW.to(ctx.wdtype)             # (the saved weight of an adapted layer is the fp32 W', not the base)
        dR1, dR2, dV = _epilogue_grads(dY, spec, has_r1 and need[3], has_r2 and need[4], vshape if need[5] else None)
        fgrads = [None] * len(factors)
        if any(need[7:]):
            groups, scale = spec.lora
            Acat = torch.cat([f.detach() for f in factors[0::2]], 0)
            Bcat = torch.cat([f.detach() for f in factors[1::2]], 0)
            dAc, dBc = ops.lora_grad(A, dY, Acat, Bcat, groups, scale * spec.s_acc)
            r, n = factors[0].shape[0], dY.shape[1] // groups
            for i, f in enumerate(factors):
                if need[7 + i]:
                    g = i // 2
                    fgrads[i] = (dBc[g * n:(g + 1) * n] if i % 2 else dAc[g * r:(g + 1) * r]).to(f.dtype)
        return (dA, dW, db, dR1, dR2, dV, None) + tuple(fgrads)


def _pad_cols(x, n):
    """x zero-padded to n columns (x itself when it has them)"""
    if n == x.shape[1]:
        return x
    out = torch.zeros(x.shape[0], n, dtype=x.dtype, device=x.device)
    out[:, :x.shape[1]] = x
    return out


def gemm_grads(A, weight, dY, geom, s_acc, need_dA=True, need_dW=True, need_db=True):
    """(dA, dW, dbias) of out = s_acc * (gather-GEMM(A, weight) + bias) for the upstream gradient dY (bf16 rows).
    geom: dict(mode, conv=(H, W, Ho, Wo, stride, up) | None, temporal=(F, S) | None) -- GemmSpec.geom."""
    mode = geom["mode"]
    N, cin = weight.shape[0], weight.shape[1]
    taps = _TAPS[mode]
    dA = dW = db = None
    if need_dA:
        # dgrad: the forward kernel with the weight's roles swapped.  The contraction runs over the forward's OUTPUT
        # channels: the GEMM needs a multiple of 64 of them (conv_out has 4: zero-padded).
        npad = (N + 63) // 64 * 64
        dYd = _pad_cols(dY, npad)
        conv = geom.get("conv")
        el = _el(dY)

        def swapped(_):
            direct = ops.pack_weight(weight, 1, dtype=el) if weight.is_cuda else None     # one kernel incl. the zero padding of N
            if direct is not None:
                return direct
            wd = weight.detach()
            if npad != N:
                wd = torch.cat([wd, wd.new_zeros((npad - N,) + tuple(wd.shape[1:]))], 0)
            with packing.element_dtype(el):
                if mode == 0:
                    return packing.pack_linear(wd.reshape(npad, cin).t())
                if mode == 1:
                    return packing.pack_conv3x3(wd.flip(2, 3).transpose(0, 1))
                return packing.pack_conv_temporal(wd.flip(2).transpose(0, 1))

        wt = _packed(weight, ("dgrad", mode, el), swapped)
        if mode == 1:
            H, W, Ho, Wo, stride, up = conv
            n_img = dY.shape[0] // (Ho * Wo)
            if stride == 2:
                # transposed conv = stride-1 dgrad on the zero-inserted gradient: dYz[2 yo, 2 xo] = dY[yo, xo]
                z = torch.zeros(n_img, H, W, npad, dtype=dY.dtype, device=dY.device)
                z[:, 0:2 * Ho:2, 0:2 * Wo:2] = dYd.view(n_img, Ho, Wo, npad)
                dYd = z.view(n_img * H * W, npad)
                conv = (H, W, H, W, 1, 0)
            elif up:
                conv = (Ho, Wo, Ho, Wo, 1, 0)        # dgrad on the upsampled grid, 2x2 sum-pool below
        dA = _rows(dYd.shape[0], cin, A)
        ops.gemm(dYd, wt, dA, N=(cin + 31) // 32 * 32, cin=npad, taps=taps, mode=mode, conv=conv,
                 temporal=geom.get("temporal"), s_acc=s_acc)
        if mode == 1 and geom["conv"][5]:
            H, W = geom["conv"][0], geom["conv"][1]
            n_img = A.shape[0] // (H * W)
            dA = dA.view(n_img, H, 2, W, 2, cin).float().sum((2, 4)).to(dA.dtype).view(n_img * H * W, cin)
    if need_dW:
        # one kernel: dW (scaled by s_acc) and, riding along in the workgroups that stream dY anyway, the bias gradient.
        # Linear weights are written in place; conv weights in the packed tap-major order and permuted afterwards
        # (writing [N, cin, taps] directly scatters the atomics at a 36-byte stride: A/B in DESIGN 3.6)
        direct = taps == 1
        # ctrlv_gemm_wgrad takes N % 8 == 0: an output width below that (the UNet's conv_out, N = 4, trainable in the
        # stage-1 step) runs on dY zero-padded to 8 columns, and the padded rows of dW / dbias are dropped
        nw = (N + 7) // 8 * 8
        dYw = _pad_cols(dY, nw)
        # (deterministic form: the ordered slab sum WRITES dW / dbias -- no zero fill; the atomic form accumulates)
        new = torch.empty if ops.DETERMINISTIC else torch.zeros
        dWp = new((nw,) + tuple(weight.shape[1:]) if direct else (nw, taps * cin), dtype=torch.float32, device=A.device)
        dbp = new(nw, dtype=torch.float32, device=A.device) if need_db else None
        ops.gemm_wgrad(A, dYw, dWp, N=nw, cin=cin, taps=taps, mode=mode, conv=geom.get("conv"),
                       temporal=geom.get("temporal"), dbias=dbp, scale=s_acc, torch_layout=direct, assign=ops.DETERMINISTIC)
        if nw != N:
            dWp = dWp[:N]
            dbp = dbp[:N] if dbp is not None else None
        if direct:
            dW = dWp
        elif mode == 1:
            dW = dWp.reshape(N, 3, 3, cin).permute(0, 3, 1, 2)
        else:
            dW = dWp.reshape(N, 3, cin).permute(0, 2, 1).reshape(N, cin, 3, 1, 1)
        dW = dW.to(weight.dtype)
        if need_db:
            db = dbp.to(weight.dtype)
    elif need_db:
        db = torch.zeros(N, dtype=torch.float32, device=A.device)
        ops.colsum(dY, db, scale=s_acc)
        db = db.to(weight.dtype)
    return dA, dW, db


class GroupNormSiLU(torch.autograd.Function):
    """y = [silu](GroupNorm32(x)) on channels-last rows; imgs_per_stat = 1 (4-D) or F (5-D statistics).
    skip=True: returns (y, x_skip) -- x_skip is x again, to be used by the SKIP connection around the branch this norm opens
    (the residual operand of the branch's last GEMM).  Both gradients of x then arrive in THIS backward, and the norm's
    backward kernel adds the skip's while it writes dx (ctrlv_groupnorm_bwd_add) instead of autograd summing the two in a
    separate pass over both tensors (181 such sums, 6.7 ms of the cfg5 step)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, n_img, S, imgs_per_stat, eps, silu, *opt):
        skip = bool(opt[0]) if opt else False
        ctx.n_opt = len(opt)
        C = x.shape[1]
        part = torch.empty(ops.groupnorm_scratch_floats(n_img, S, C, imgs_per_stat), dtype=torch.float32, device=x.device)
        y = torch.empty_like(x)
        g32, b32 = f32(gamma).detach().contiguous(), f32(beta).detach().contiguous()
        ops.groupnorm(x, None, n_img, S, C, imgs_per_stat, g32, b32, eps, silu, y, part)
        ctx.save_for_backward(x, g32, b32, part)
        ctx.cfg = (n_img, S, C, imgs_per_stat, silu, gamma.dtype, bool(skip))
        ctx.set_materialize_grads(False)
        return (y, x) if skip else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, g32, b32, part = ctx.saved_tensors
        n_img, S, C, ips, silu, pdt, skip = ctx.cfg
        tail = (None,) * (5 + ctx.n_opt)
        if dy is None:                    # (only the skip connection carried a gradient)
            return (dskip, None, None) + tail
        dx = torch.empty_like(x)
        dg = torch.zeros(C, dtype=torch.float32, device=x.device)
        db = torch.zeros(C, dtype=torch.float32, device=x.device)
        ops.groupnorm_bwd(x, dy.contiguous(), n_img, S, C, ips, part, g32, b32, silu, dx, dg, db,
                          add=None if dskip is None else dskip.contiguous())
        return (dx, dg.to(pdt), db.to(pdt)) + tail


_MIX_CACHE = {}      # id(mix_factor parameter) -> (version, sigmoid value); filled by prefetch_mix_factors()


def prefetch_mix_factors(*models, host_sigmoid=False):
    """ONE device-to-host copy for all AlphaBlender mix factors of the given models (about 60 scalars).  BlendGemm
    folds sigmoid(mix_factor) into GEMM epilogue scalars, i.e. needs it on the host: read one by one, that was a
    blocking sync per res block / transformer (it drained the queue ~60 times per step and serialised the backward /
    all-reduce overlap).  training.train_step calls this once per step.
    host_sigmoid: copy the raw factors and take the sigmoid on the host in double precision -- the value `_mix_alpha` reads
    one by one and the inference executor of the VAE decoder packs (vae_decoder_hip._sig), so that a training forward and
    that executor hand the kernels the same scalar (the device's fp32 sigmoid may differ from it in the last bit)."""
    ps = [p for m in models for n, p in m.named_parameters() if n.endswith("mix_factor")]
    if not ps:
        return
    if host_sigmoid:
        raw = torch.stack([p.detach().float().reshape(()) for p in ps]).cpu().tolist()
        vals = [1.0 / (1.0 + math.exp(-v)) for v in raw]
    else:
        vals = torch.sigmoid(torch.stack([p.detach().float().reshape(()) for p in ps])).cpu().tolist()
    _MIX_CACHE.clear()
    for p, v in zip(ps, vals):
        _MIX_CACHE[id(p)] = (p._version, p.data_ptr(), float(v))


def _mix_alpha(mix_factor):
    """sigmoid(mix_factor) as a python float: from the per-step cache if it is current, else one (blocking) read."""
    hit = _MIX_CACHE.get(id(mix_factor))
    if hit is not None and hit[0] == mix_factor._version and hit[1] == mix_factor.data_ptr():
        return hit[2]
    return 1.0 / (1.0 + math.exp(-float(mix_factor.detach().float().cpu())))


class BlendGemm(torch.autograd.Function):
    """An AlphaBlender folded into the GEMM that precedes it, a = sigmoid(mix_factor), in its two forms (distinct arithmetic):
      R2 is None  res block, last temporal conv:  out = xs + (1 - a) * (conv(hn) + bias)          R1 = xs
      R2 given    transformer, temporal FF output: out = a * h2 + (1 - a) * (g1 + u @ W^T + b)    R1 = g1, R2 = h2
    Gradients for A, the GEMM's parameters, R1, R2 AND mix_factor.  spec: the geometry (its scalars are derived here).
    Opt-in (a trailing True, res block form only): switch_spatial_to_temporal_mix of the VAE decoder's blender, i.e. the
    first form with mix -> -mix:  out = xs + a * (conv(hn) + bias)."""

    @staticmethod
    def forward(ctx, A, weight, bias, R1, R2, mix_factor, spec, *opt):
        a = _mix_alpha(mix_factor)
        ctx.switched, ctx.n_opt = bool(opt[0]) if opt else False, len(opt)
        if ctx.switched:
            if R2 is not None:
                raise ValueError("BlendGemm: the switched mix exists for the res block form only")
            spec = spec._replace(s_acc=a, s1=1.0, s2=1.0)
        else:
            spec = spec._replace(s_acc=1.0 - a, s1=1.0 if R2 is None else 1.0 - a, s2=a)
        out = _gemm_forward(A, weight, bias, R1, R2, None, spec)
        ctx.save_for_backward(A, weight, R1 if R2 is None else R2, out, mix_factor)
        ctx.spec, ctx.a, ctx.res_form = spec, a, R2 is None
        return out

    @staticmethod
    def backward(ctx, dY):
        A, weight, other, out, mix = ctx.saved_tensors
        a, spec, need = ctx.a, ctx.spec, ctx.needs_input_grad
        dY = dY.contiguous()
        dA, dW, db = gemm_grads(A, weight, dY, spec.geom, spec.s_acc, need[0], need[1], need[2])
        dR1, dR2, _ = _epilogue_grads(dY, spec, need[3], need[4], None)
        dmix = None
        if need[5]:
            acc = torch.zeros(1, dtype=torch.float32, device=dY.device)
            if ctx.switched:
                # dL/da = sum dY * (conv + bias) = sum dY * (out - xs) / a;  da/dmix = a (1 - a)
                ops.dot_diff(dY, out, other, acc, scale=1.0 - a)
            elif ctx.res_form:
                # dL/da = -sum dY * (conv + bias) = -sum dY * (out - xs) / (1 - a);  da/dmix = a (1 - a)
                ops.dot_diff(dY, out, other, acc, scale=-a)
            else:
                # dL/da = sum dY * (h2 - g1 - lin) = sum dY * (h2 - out) / (1 - a);  da/dmix = a (1 - a)
                ops.dot_diff(dY, other, out, acc, scale=a)
            dmix = acc.to(mix.dtype).reshape(mix.shape)
        return (dA, dW, db, dR1, dR2, dmix, None) + (None,) * ctx.n_opt


class LayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x [+ V[(m // vdiv) % vmod]]) over the channel axis (eps 1e-5); V = the frame positional embedding
    table of TransformerSpatioTemporalModel (fp32 [F, C]) or None.  skip=True: returns (y, x_skip), see GroupNormSiLU."""

    @staticmethod
    def forward(ctx, x, gamma, beta, V, vdiv, vmod, *opt):
        skip = bool(opt[0]) if opt else False
        ctx.n_opt = len(opt)
        y = torch.empty_like(x)
        g32, b32 = f32(gamma).detach().contiguous(), f32(beta).detach().contiguous()
        ops.layernorm(x, g32, b32, 1e-5, y, V=V, vdiv=vdiv, vmod=vmod)
        ctx.save_for_backward(x, g32, V if V is not None else torch.empty(0, device=x.device))
        ctx.cfg = (V is not None, vdiv, vmod, gamma.dtype)
        ctx.set_materialize_grads(False)
        return (y, x) if skip else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, g32, V = ctx.saved_tensors
        has_v, vdiv, vmod, pdt = ctx.cfg
        tail = (None,) * (2 + ctx.n_opt)
        if dy is None:
            return (dskip, None, None, None) + tail
        C = x.shape[1]
        dx = torch.empty_like(x)
        dg = torch.zeros(C, dtype=torch.float32, device=x.device)
        db = torch.zeros(C, dtype=torch.float32, device=x.device)
        dV = None
        if has_v and ctx.needs_input_grad[3]:
            # (the table's gradient is the column sum of the NORM's dx: without the skip gradient)
            ops.layernorm_bwd(x, dy.contiguous(), g32, 1e-5, dx, dg, db, V=V, vdiv=vdiv, vmod=vmod)
            dV = torch.zeros_like(V)
            if vdiv % 4 == 0 or not ops.DETERMINISTIC:
                ops.colsum(dx, dV, vmode=1, vdiv=vdiv, vmod=vmod)
            else:       # (a row group that is no multiple of 4 has no ordered form in ctrlv_colsum: see _epilogue_grads)
                _row_vector_grad_by_table_row(dx, dV, GemmSpec(vmode=1, vdiv=vdiv, vmod=vmod))
            if dskip is not None:
                dx = dx + dskip
        else:
            ops.layernorm_bwd(x, dy.contiguous(), g32, 1e-5, dx, dg, db, V=V if has_v else None, vdiv=vdiv, vmod=vmod,
                              add=None if dskip is None else dskip.contiguous())
        return (dx, dg.to(pdt), db.to(pdt), dV) + tail


# ---- gradient checkpointing of the GEGLU feed-forwards (`enable_gradient_checkpointing()`, reference:
# tools/train_video_controlnet.py:185-186).  The two 4C / 8C-wide intermediates of a feed-forward -- u (saved by the
# output projection for its wgrad) and the raw projection (saved for the GEGLU backward) -- are 31 GB of the step's 101 GB
# at the reference's size.  Checkpointed, NEITHER is kept: the forward does not even write the raw projection, and the
# backward recomputes both with the forward's own launch (one GEGLU GEMM with raw_out: the same bits).  u is saved by
# whichever Function consumes it (Gemm / BlendGemm), so it is swapped for a recompute cell by a saved-tensor hook
# that is active around the feed-forward pair only.
_CKPT = [False]


@contextlib.contextmanager
def gradient_checkpointing(enabled):
    """Training forwards built inside run their GEGLU feed-forwards checkpointed (see above)."""
    prev = _CKPT[0]
    _CKPT[0] = bool(enabled)
    try:
        yield
    finally:
        _CKPT[0] = prev


class _GegluCell:
    """Recompute cell of one checkpointed GEGLU projection: holds its small inputs, hands out u / raw once each."""

    def __init__(self, x, weight, bias):
        self.x, self.w, self.b = x, weight, bias
        self.u = self.raw = None
        self.done = False
        self.u_ptr = 0

    def _recompute(self):
        if self.done:
            return
        two_i = self.w.shape[0]
        wp, bp = _packed_geglu(self.w, _el(self.x)), _geglu_bias32(self.b)
        M = self.x.shape[0]
        self.u, self.raw = _rows(M, two_i // 2, self.x), _rows(M, two_i, self.x)
        ops.gemm(self.x, wp, self.u, N=two_i, cin=wp.shape[1], bias=bp, geglu=1, raw_out=self.raw)
        self.done = True

    def take(self, which):
        """Hands out u / raw once per recompute: a second take of the same tensor (ctx.saved_tensors read twice,
        backward(retain_graph=True) run again) recomputes instead of returning None."""
        if self.done and getattr(self, which) is None:
            self.done = False                        # that tensor was already handed out: run the projection again
            self.u = self.raw = None
        self._recompute()
        t = getattr(self, which)
        setattr(self, which, None)
        return t


_REC = [True]        # grad mode of the caller of the current feed-forward region (set by _ff_region)
_CELLS = {}          # data_ptr of a live checkpointed u -> its cell (only while the feed-forward pair is being built)


def _ckpt_pack(t):
    cell = _CELLS.pop(t.data_ptr(), None) if t.is_cuda else None
    return (cell,) if cell is not None else t


def _ckpt_unpack(obj):
    return obj[0].take("u") if isinstance(obj, tuple) else obj


@contextlib.contextmanager
def _ff_region():
    """Around one GEGLU projection + its output projection: under checkpointing the consumer's saved u becomes a cell."""
    prev, _REC[0] = _REC[0], torch.is_grad_enabled()
    try:
        yield from _ff_region_body()
    finally:
        _REC[0] = prev


def _ff_region_body():
    if not _CKPT[0]:
        yield
        return
    with torch.autograd.graph.saved_tensors_hooks(_ckpt_pack, _ckpt_unpack):
        try:
            yield
        finally:
            # every checkpointed u must have been claimed by its consumer's save_for_backward: a consumer that saved a copy
            # (a .contiguous() / reshaped u) would silently keep the tensor and make checkpointing a no-op
            leaked, _ = len(_CELLS), _CELLS.clear()
        if leaked:
            raise RuntimeError(f"gradient checkpointing: {leaked} GEGLU intermediate(s) were not claimed by the output "
                               "projection's saved tensors (the consumer saved a copy?)")


class GegluProj(torch.autograd.Function):
    """u = a * gelu_erf(g), (a | g) = x @ W^T + b   (diffusers GEGLU: `proj` Linear(C -> 2 I), chunk, exact gelu).  The
    forward is ONE GEMM with the GEGLU epilogue that ALSO writes the raw projection (bf16, packed column order) for the
    backward -- u itself comes from the fp32 accumulators exactly as in the inference path; shapes the ping-pong tiles do
    not serve (K < 128) recompute the raw projection in the backward instead.  Under gradient checkpointing (above) the
    raw projection is neither written nor kept: the backward takes it from the recompute cell."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        two_i, cin = weight.shape
        wp, bp = _packed_geglu(weight, _el(x)), _geglu_bias32(bias)
        u = _rows(x.shape[0], two_i // 2, x)
        # (a cell only where a backward will run: under torch.no_grad() / with no input requiring grad -- an evaluation pass
        #  inside a checkpointed training context -- Function.forward still executes, but no consumer ever saves u, so a cell
        #  registered here would stay unclaimed and _ff_region would report it as leaked.  ADVICE r05.  Grad mode is always
        #  off INSIDE a Function.forward: _ff_region records the caller's.)
        records = _REC[0] and any(ctx.needs_input_grad)
        ckpt = _CKPT[0] and records and cin >= 128 and cin % 32 == 0
        raw = _rows(x.shape[0], two_i, x) if (records and cin >= 128 and cin % 32 == 0 and not ckpt) else None
        ops.gemm(x, wp, u, N=two_i, cin=wp.shape[1], bias=bp, geglu=1, raw_out=raw)
        ctx.cell = None
        if ckpt:
            ctx.cell = _GegluCell(x, weight, bias)
            _CELLS[u.data_ptr()] = ctx.cell
        ctx.save_for_backward(x, weight, bias, raw if raw is not None else torch.empty(0, device=x.device))
        ctx.has_raw = raw is not None
        return u

    @staticmethod
    def backward(ctx, du):
        x, weight, bias, raw = ctx.saved_tensors
        two_i, cin = weight.shape
        inner = two_i // 2
        # rows in the packed (value, gate) block order
        wi = frozen((weight,), "geglu_il", lambda: packing.geglu_interleave(weight.detach()), derived=True)
        if ctx.cell is not None:
            raw = ctx.cell.take("raw")                                 # (recomputed together with u: one launch)
            ctx.cell = None
        elif not ctx.has_raw:
            with packing.element_dtype(_el(x)):
                wp, bp = packing.pack_geglu(weight, bias)
            raw = _rows(x.shape[0], two_i, x)
            ops.gemm(x, wp, raw, N=two_i, cin=wp.shape[1], bias=bp)    # activation recompute (no GEGLU epilogue)
        draw = torch.empty_like(raw)
        ops.geglu_bwd(raw, du.contiguous(), draw)
        dx, dwi, dbi = gemm_grads(x, wi, draw, dict(mode=0), 1.0, ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                  ctx.needs_input_grad[2])
        # un-interleave the rows: interleaved row ((r >> 4) * 2 + is_gate) * 16 + (r & 15)  <-  original row r (+ inner)
        idx = torch.arange(two_i, device=x.device)
        isg, r = (idx >= inner).long(), idx % inner
        src = ((r >> 4) * 2 + isg) * 16 + (r & 15)
        dw = dwi[src] if dwi is not None else None
        db = dbi[src] if dbi is not None else None
        return dx, dw, db


def res_block_train_forward(block, x, temb_tables, B, F, H, W):
    """Training-mode forward of a `ctrlv_amd.models.blocks.SpatioTemporalResBlock` (no skip-concat input) built from the
    autograd functions above; same kernels, same fusion as `block.run` (bit-identical output), but every op records
    what its backward needs.  x: bf16 rows [B*F*H*W, cin] (requires_grad for dgrad); temb_tables: (fp32 [B, cout],
    fp32 [B, cout]) = time_emb_proj(silu(emb)) of the spatial / temporal half (per-clip vectors: computed by the caller,
    with torch autograd if their gradients are wanted)."""
    s, t = block.spatial_res_block, block.temporal_res_block
    N, S = B * F, H * W
    g2d = dict(mode=1, conv=(H, W, H, W, 1, 0), vdiv=F * S)
    g3d = dict(mode=2, temporal=(F, S), vdiv=F * S)
    gn = GroupNormSiLU.apply
    # (x and xs each feed a norm AND the skip connection around the branch it opens: the norm hands the skip its alias, so
    #  that both gradients meet in the norm's backward kernel -- GroupNormSiLU, skip=True)
    if s.conv_shortcut is None:
        xn, res = gn(x, s.norm1.weight, s.norm1.bias, N, S, 1, block.eps, True, True)
    else:
        xn = gn(x, s.norm1.weight, s.norm1.bias, N, S, 1, block.eps, True)
    h = gemm(xn, s.conv1.weight, s.conv1.bias, V=temb_tables[0], **g2d)
    hn = gn(h, s.norm2.weight, s.norm2.bias, N, S, 1, block.eps, True)
    if s.conv_shortcut is not None:      # (the shortcut conv reads x itself: autograd sums its gradient and the norm's)
        res = gemm(x, s.conv_shortcut.weight.reshape(block.cout, block.cin), s.conv_shortcut.bias)
    xs = gemm(hn, s.conv2.weight, s.conv2.bias, res, **g2d)
    hn, xs = gn(xs, t.norm1.weight, t.norm1.bias, N, S, F, block.eps, True, True)
    h = gemm(hn, t.conv1.weight, t.conv1.bias, V=temb_tables[1], **g3d)
    hn = gn(h, t.norm2.weight, t.norm2.bias, N, S, F, block.eps, True)
    return BlendGemm.apply(hn, t.conv2.weight, t.conv2.bias, xs, None, block.time_mixer.mix_factor, GemmSpec(**g3d))


def zero_conv_train_forward(conv, x, scale=1.0):
    """A ControlNet zero-conv (1x1) times conditioning_scale (controlnet.py:331-344) with gradients."""
    C = conv.weight.shape[0]
    return gemm(x, conv.weight.reshape(C, -1), conv.bias, s_acc=float(scale))


# =============================================================================== transformer (second slice)
def _lora_merged(weight, factors, groups, scale):
    """fp32 W' = W + s . B_i . A_i for the `groups` row blocks of `weight` (ctrlv_lora_merge, one launch per group).  Kept
    (as a frozen Parameter, so that its packed layouts are kept too) only while W and every factor are frozen parameters."""
    def build():
        out = torch.empty(weight.shape, dtype=torch.float32, device=weight.device)
        n = weight.shape[0] // groups
        for i in range(groups):
            ops.lora_merge(weight[i * n:(i + 1) * n], factors[2 * i], factors[2 * i + 1], scale, out=out[i * n:(i + 1) * n])
        return out
    return frozen((weight,) + tuple(factors), ("lora_merged", float(scale)), build, derived=True)


def _lora_operands(linears):
    """(groups, s) and the trailing factor inputs of Gemm for these nn.Linears (side by side along N), or None when none is
    adapted.  A member without an adapter takes frozen zero factors of the same rank (W' = W exactly)."""
    fs = [lora_mod.factors(lin) for lin in linears]
    live = [f for f in fs if f is not None]
    if not live:
        return None
    r, s = live[0][0].shape[0], live[0][2]
    out = []
    for lin, f in zip(linears, fs):
        if f is None:
            z = lin.weight.new_zeros((), dtype=torch.float32)
            f = (z.expand(r, lin.in_features), z.expand(lin.out_features, r), s)
        if f[0].shape[0] != r or f[2] != s:
            raise ValueError("the adapted projections of one fused GEMM must share the rank and lora_alpha")
        out += [f[0], f[1]]
    return (len(linears), s), out


def gemm(A, weight, bias, R1=None, R2=None, V=None, linears=(), **spec):
    """Gemm.apply with the GemmSpec fields as keywords.  linears: the nn.Linears whose weights `weight` is / stacks (side by
    side along N) -- when one of them carries a LoRA adapter, the factors of all of them trail the inputs."""
    lo = _lora_operands(linears) if linears else None
    if lo is None:
        return Gemm.apply(A, weight, bias, R1, R2, V, GemmSpec(**spec))
    return Gemm.apply(A, weight, bias, R1, R2, V, GemmSpec(lora=lo[0], **spec), *lo[1])


def lora_weight_f32(linear):
    """fp32 weight of a small per-clip torch op with torch autograd through the LoRA factors (attn2's to_v / to_out)."""
    w = f32(linear.weight)
    f = lora_mod.factors(linear)
    if f is None:
        return w
    return w + f[2] * (f[1].float() @ f[0].float())


class SpatialAttention(torch.autograd.Function):
    """softmax(q k^T / 8) v per (image, head) on qkv rows [n_img * S, 3C] (BasicTransformerBlock.attn1 core)."""

    @staticmethod
    def forward(ctx, qkv, n_img, S, C):
        out = _rows(qkv.shape[0], C, qkv)
        lse = torch.empty(n_img, C // 64, S, dtype=torch.float32, device=qkv.device)
        ops.attention_spatial_lse(qkv, out, lse, n_img, S, C)
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (n_img, S, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        n_img, S, C = ctx.cfg
        dqkv = torch.empty_like(qkv)
        ops.attention_spatial_bwd(qkv, out, dout.contiguous(), lse, dqkv, n_img, S, C)
        return dqkv, None, None, None


class TemporalAttention(torch.autograd.Function):
    """Attention over the F frames of every (clip, pixel); rows ordered (b, f, s) (TemporalBasicTransformerBlock.attn1)."""

    @staticmethod
    def forward(ctx, qkv, B, F, S, C):
        out = _rows(qkv.shape[0], C, qkv)
        ops.attention_temporal(qkv, out, B, F, S, C)
        ctx.save_for_backward(qkv, out)
        ctx.cfg = (B, F, S, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out = ctx.saved_tensors
        B, F, S, C = ctx.cfg
        dqkv = torch.empty_like(qkv)
        ops.attention_temporal_bwd(qkv, out, dout.contiguous(), dqkv, B, F, S, C)
        return dqkv, None, None, None, None


def sinusoid(t, dim):
    """diffusers `Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0)` in fp32: [cos | sin]."""
    half = dim // 2
    freq = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=t.device) / half)
    arg = t.float()[:, None] * freq[None]
    return torch.cat([torch.cos(arg), torch.sin(arg)], dim=-1)


def transformer_train_forward(tr, x, ehs, B, F, H, W, time_context_order="sb"):
    """Training-mode forward of `ctrlv_amd.models.blocks.TransformerSpatioTemporalModel`: the same kernels and fusion as
    `tr.run` with every op recording its backward.  x: bf16 rows [B*F*H*W, C]; ehs: fp32 [B, cross_dim] (the single CLIP
    token per clip).  The tiny per-clip tensors (the two degenerate cross-attention vectors to_out(to_v(ehs)) and the
    frame positional embedding MLP) are plain fp32 torch ops, so their parameters get gradients through torch autograd;
    to_q / to_k / norm2 of the cross-attentions receive exactly zero gradient (softmax over one key is constant)."""
    import torch.nn.functional as Fn
    sb, tb = tr.transformer_blocks[0], tr.temporal_transformer_blocks[0]
    N, S, C = B * F, H * W, tr.C
    quirk = time_context_order == "sb" and B > 1       # diffusers 0.27.2: time_context rows (s, b), tokens (b, s) -- H1

    def xvec(attn):
        return Fn.linear(Fn.linear(ehs.float(), lora_weight_f32(attn.to_v)), lora_weight_f32(attn.to_out[0]),
                         f32(attn.to_out[0].bias)).contiguous()

    tpe = tr.time_pos_embed
    emb = Fn.linear(Fn.silu(Fn.linear(sinusoid(torch.arange(F, device=x.device), C), f32(tpe.linear_1.weight),
                                      f32(tpe.linear_1.bias))), f32(tpe.linear_2.weight),
                    f32(tpe.linear_2.bias)).contiguous()                                   # fp32 [F, C]
    big = 1 << 30

    def lns(h, n, V=None, vdiv=1, vmod=big):             # (normed rows, the alias of h for the skip connection)
        return LayerNormFn.apply(h, n.weight, n.bias, V, vdiv, vmod, True)

    def qkv(n, attn):
        # the fused q|k|v weight is kept only while ALL THREE are frozen (partial freezing is a public mode of the UNet step)
        ws = (attn.to_q.weight, attn.to_k.weight, attn.to_v.weight)
        w = frozen(ws, "qkv_cat", lambda: torch.cat(ws, 0), derived=True)
        return gemm(n, w, None, linears=[attn.to_q, attn.to_k, attn.to_v])

    def out_proj(a, attn, R1, **spec):
        lin = attn.to_out[0]
        return gemm(a, lin.weight, lin.bias, R1, linears=[lin], **spec)

    # Every trunk tensor (x, h0, h1, h2, g0, g1) feeds the norm that opens a branch AND the skip connection around it: the norm
    # hands the skip its alias (skip=True), so both gradients meet in the norm's backward kernel instead of a separate sum.
    t, x = GroupNormSiLU.apply(x, tr.norm.weight, tr.norm.bias, N, S, 1, 1e-6, False, True)
    h0 = gemm(t, tr.proj_in.weight, tr.proj_in.bias)
    # ---- spatial BasicTransformerBlock
    n, h0 = lns(h0, sb.norm1)
    a = SpatialAttention.apply(qkv(n, sb.attn1), N, S, C)
    h1 = out_proj(a, sb.attn1, h0, V=xvec(sb.attn2), vdiv=F * S)
    with _ff_region():
        n, h1 = lns(h1, sb.norm3)
        u = GegluProj.apply(n, sb.ff.net[0].proj.weight, sb.ff.net[0].proj.bias)
        h2 = gemm(u, sb.ff.net[2].weight, sb.ff.net[2].bias, h1)
    del u
    # ---- temporal block: rows stay ordered (b, f, s); the frame embedding is added inside the consumers
    with _ff_region():
        n, h2 = lns(h2, tb.norm_in, emb, S, F)
        u = GegluProj.apply(n, tb.ff_in.net[0].proj.weight, tb.ff_in.net[0].proj.bias)
        g0 = gemm(u, tb.ff_in.net[2].weight, tb.ff_in.net[2].bias, h2, V=emb, vdiv=S, vmod=F)
    del u
    n, g0 = lns(g0, tb.norm1)
    a = TemporalAttention.apply(qkv(n, tb.attn1), B, F, S, C)
    vspec = dict(vmode=2, vdiv=F * S, vS=S, vmod=B) if quirk else dict(vdiv=F * S)
    g1 = out_proj(a, tb.attn1, g0, V=xvec(tb.attn2), **vspec)
    with _ff_region():
        n, g1 = lns(g1, tb.norm3)
        u = GegluProj.apply(n, tb.ff.net[0].proj.weight, tb.ff.net[0].proj.bias)
        h3 = BlendGemm.apply(u, tb.ff.net[2].weight, tb.ff.net[2].bias, g1, h2, tr.time_mixer.mix_factor, GemmSpec())
    del u, n
    return gemm(h3, tr.proj_out.weight, tr.proj_out.bias, x)


# =============================================================================== VAE temporal decoder (fine-tuning)
# tools/train_vae_finetuning.py:303-320 trains every `decoder.*` parameter of AutoencoderKLTemporalDecoder.  The blocks below
# run the launches of ctrlv_amd/models/vae_decoder_hip.py (`_res`, `_attn`, the tail) -- the same bits forward -- with every
# op recording its backward.  Rows are ordered (clip, frame, pixel); n_clips clips of F frames run in one walk.
def vae_res_block_train_forward(block, x, n_clips, F, H, W):
    """Training-mode forward of the VAE decoder's `SpatioTemporalResBlock` (no time embedding; eps 1e-6 in the spatial half,
    1e-5 in the temporal one; a 1x1 `conv_shortcut` where cin != cout; blender with switch_spatial_to_temporal_mix:
    out = xs + sigmoid(mix) * h).  x: bf16 rows [n_clips*F*H*W, cin]."""
    s, t = block.spatial_res_block, block.temporal_res_block
    N, S = n_clips * F, H * W
    cout, cin = s.conv1.weight.shape[:2]
    g2d = dict(mode=1, conv=(H, W, H, W, 1, 0))
    g3d = dict(mode=2, temporal=(F, S))
    eps_s, eps_t = s.norm1.eps, t.norm1.eps
    gn = GroupNormSiLU.apply
    if s.conv_shortcut is None:
        xn, res = gn(x, s.norm1.weight, s.norm1.bias, N, S, 1, eps_s, True, True)
    else:
        xn = gn(x, s.norm1.weight, s.norm1.bias, N, S, 1, eps_s, True)
    h = gemm(xn, s.conv1.weight, s.conv1.bias, **g2d)
    hn = gn(h, s.norm2.weight, s.norm2.bias, N, S, 1, eps_s, True)
    if s.conv_shortcut is not None:
        res = gemm(x, s.conv_shortcut.weight.reshape(cout, cin), s.conv_shortcut.bias)
    xs = gemm(hn, s.conv2.weight, s.conv2.bias, res, **g2d)
    hn, xs = gn(xs, t.norm1.weight, t.norm1.bias, N, S, F, eps_t, True, True)
    h = gemm(hn, t.conv1.weight, t.conv1.bias, **g3d)
    hn = gn(h, t.norm2.weight, t.norm2.bias, N, S, F, eps_t, True)
    return BlendGemm.apply(hn, t.conv2.weight, t.conv2.bias, xs, None, block.time_mixer.mix_factor, GemmSpec(**g3d), True)


def _rows16(weight, el=torch.bfloat16):
    """element-type copy of a [N, K] parameter in its own layout (the A operand of a role-swapped GEMM)"""
    return _packed(weight, ("rows16", el), lambda w: w.detach().to(el).contiguous())


class VaeAttentionCore(torch.autograd.Function):
    """softmax(q k^T / sqrt(C)) v per frame for ONE head of dim C (the VAE mid block: C = 512, which the 64-wide attention
    cores do not serve), v = t @ Wv^T without its bias (the caller folds b_v into the output projection's bias: rows of P
    sum to one).  Forward = the launches of vae_decoder_hip._attn: scores GEMM with fp32 output and the scale folded in,
    ctrlv_softmax_rows, V^T = Wv t^T by a role-swapped GEMM, P.V with K = S.  Nothing S x S is kept: the backward runs the
    first two launches again per frame, then
        dP = dO V^T (fp32)   dS = ctrlv_softmax_rows_bwd(P, dP)   dQ = dS K        forward GEMMs (weight operand V / K^T)
        dV = P^T dO          dK = dS^T Q                                           ctrlv_gemm_wgrad (dY = P / dS, A = dO / Q)
    and the Linear backward of the v projection on dV.  Gradients for q, k, t and Wv."""

    @staticmethod
    def forward(ctx, q, k, t, wv, n, S):
        C, dev = q.shape[1], q.device
        o = _rows(n * S, C, q)
        scores = torch.empty(S, S, dtype=torch.float32, device=dev)
        el = _el(q)
        probs = torch.empty(S, S, dtype=el, device=dev)
        vt = torch.empty(C, S, dtype=el, device=dev)
        wv_rows = _rows16(wv, el)
        for f in range(n):
            r0, r1 = f * S, (f + 1) * S
            ops.gemm(q[r0:r1], k[r0:r1], scores, N=S, cin=C, s_acc=C ** -0.5, out_f32=True)
            ops.softmax_rows(scores, probs)
            ops.gemm(wv_rows, t[r0:r1], vt, N=S, cin=C)
            ops.gemm(probs, vt, o[r0:r1], N=C, cin=S)
        ctx.save_for_backward(q, k, t, wv)
        ctx.cfg = (n, S)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, t, wv = ctx.saved_tensors
        n, S = ctx.cfg
        C, dev, M = q.shape[1], q.device, q.shape[0]
        scale = C ** -0.5
        do = do.contiguous()
        v = _rows(M, C, q)                                                          # V rows of every frame: one GEMM
        el = _el(q)
        ops.gemm(t, _packed_fwd(wv, 0, el), v, N=C, cin=C)
        new = torch.empty if ops.DETERMINISTIC else torch.zeros
        dq = _rows(M, C, q)
        dk32 = new(M, C, dtype=torch.float32, device=dev)
        dv32 = new(M, C, dtype=torch.float32, device=dev)
        scores = torch.empty(S, S, dtype=torch.float32, device=dev)
        dp = torch.empty(S, S, dtype=torch.float32, device=dev)
        probs = torch.empty(S, S, dtype=el, device=dev)
        ds = torch.empty(S, S, dtype=el, device=dev)
        flat = dict(N=S, cin=C, torch_layout=True, assign=ops.DETERMINISTIC)
        for f in range(n):
            r0, r1 = f * S, (f + 1) * S
            ops.gemm(q[r0:r1], k[r0:r1], scores, N=S, cin=C, s_acc=scale, out_f32=True)
            ops.softmax_rows(scores, probs)
            ops.gemm(do[r0:r1], v[r0:r1], dp, N=S, cin=C, out_f32=True)             # dP = dO V^T
            ops.softmax_rows_bwd(probs, dp, scale, ds)
            ops.gemm(ds, k[r0:r1].t().contiguous(), dq[r0:r1], N=C, cin=S)          # dQ = dS K  (weight operand K^T [C, S])
            ops.gemm_wgrad(q[r0:r1], ds, dk32[r0:r1], **flat)                       # dK = dS^T Q
            ops.gemm_wgrad(do[r0:r1], probs, dv32[r0:r1], **flat)                   # dV = P^T dO
        need = ctx.needs_input_grad
        dt, dwv, _ = gemm_grads(t, wv, dv32.to(el), dict(mode=0), 1.0, need[2], need[3], False)
        return dq, dk32.to(el), dt, dwv, None, None


class _ExactZeroGrad(torch.autograd.Function):
    """Identity on a parameter whose gradient is identically zero by the structure of the graph: the backward hands back
    exact zeros instead of the rounding noise a computed path would leave."""

    @staticmethod
    def forward(ctx, p):
        return p.detach().clone()

    @staticmethod
    def backward(ctx, g):
        return torch.zeros_like(g)


def vae_attention_train_forward(attn, x, n, H, W):
    """Training-mode forward of the VAE mid block's `Attention` (one head of dim C): GroupNorm (no SiLU) -> q, k -> the core
    above -> to_out + x, with vae_decoder_hip._attn's launches and its folding of b_v into b_o (P (V + 1 b_v^T) W_o^T =
    P V W_o^T + W_o b_v; the fold is a differentiable torch op on [C]-sized tensors, so b_v and W_o get its gradient).
    x: bf16 rows [n*H*W, C].  to_k.bias shifts every score of a row by the same q . b_k, which the softmax removes: its
    gradient is identically zero, and it is returned as exact zeros (the computed path, the column sum of dK, would leave
    the rounding noise of the bf16 dS rows, which sum to zero only in exact arithmetic)."""
    if attn.heads != 1:
        raise ValueError("the HIP VAE attention is specialised for the SVD VAE's single head")
    S, C = H * W, x.shape[1]
    if S % 64 or S > 16384:
        raise ValueError(f"HIP VAE attention: {H}x{W} latent pixels per frame must be a multiple of 64 and <= 16384")
    gnm, lin_o = attn.group_norm, attn.to_out[0]
    t, x = GroupNormSiLU.apply(x, gnm.weight, gnm.bias, n, S, 1, gnm.eps, False, True)
    q = gemm(t, attn.to_q.weight, attn.to_q.bias)
    k = gemm(t, attn.to_k.weight, _ExactZeroGrad.apply(attn.to_k.bias))
    o = VaeAttentionCore.apply(q, k, t, attn.to_v.weight, n, S)
    bo = lin_o.bias.float() + lin_o.weight.float() @ attn.to_v.bias.float()
    return gemm(o, lin_o.weight, bo.contiguous(), x)


class TimeConvOut(torch.autograd.Function):
    """`time_conv_out` of the VAE decoder -- Conv3d(C, C, (3,1,1)) over the frames of each clip, C <= 4 -- fused with rows ->
    NCHW: rows [n_clips*F*HW, ldc] bf16 (conv_out's output) -> (n_clips*F, C, H, W) fp32, one ctrlv_time_conv_rows_to_nchw
    launch per clip; backward = ctrlv_time_conv_rows_to_nchw_bwd (ordered parameter sums)."""

    @staticmethod
    def forward(ctx, rows, weight, bias, n_clips, F, H, W):
        C, HW = weight.shape[0], H * W
        w32 = weight.detach().float()[:, :, :, 0, 0].contiguous()                  # [o, c, t]
        b32 = bias.detach().float().contiguous()
        out = torch.empty(n_clips * F, C, H, W, dtype=torch.float32, device=rows.device)
        for c in range(n_clips):
            ops.time_conv_rows_to_nchw(rows[c * F * HW:(c + 1) * F * HW], F, C, HW, w32, b32, out[c * F:(c + 1) * F])
        ctx.save_for_backward(rows, w32)
        ctx.cfg = (n_clips, F, C, HW, weight.dtype, bias.dtype, tuple(weight.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        rows, w32 = ctx.saved_tensors
        n_clips, F, C, HW, wdt, bdt, wshape = ctx.cfg
        drows = torch.empty_like(rows)
        dw = torch.empty(C, C, 3, dtype=torch.float32, device=rows.device)
        db = torch.empty(C, dtype=torch.float32, device=rows.device)
        ops.time_conv_rows_to_nchw_bwd(dout.float().contiguous(), rows, n_clips * F, F, C, HW, w32, drows, dw, db)
        return drows, dw.reshape(wshape).to(wdt), db.to(bdt), None, None, None, None
