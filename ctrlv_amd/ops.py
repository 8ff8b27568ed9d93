"""Tensor-level wrappers over the C ABI (include/ctrlv_hip.h).  Inputs are torch CUDA tensors used purely as
device-memory handles; every call enqueues on torch's current HIP stream.  No wrapper has a fallback."""
import ctypes

import torch

from . import _lib, profiler as _prof
from ._lib import GemmDesc, check

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _L(*tensors):
    """The library that serves these element tensors: libctrlv_hip_f16.so when they are fp16, else the bf16 library."""
    els = {t.dtype for t in tensors if t is not None and t.dtype in (torch.float16, torch.bfloat16)}
    if len(els) > 1:
        raise ValueError("ctrlv_amd: one call mixes bf16 and fp16 element tensors (a library serves ONE element type)")
    return _lib.load(torch.float16 if torch.float16 in els else None)


def _need_gpu(t, name="tensor"):
    if not t.is_cuda:
        raise _lib.CtrlvHipError(f"ctrlv_amd: {name} must live on a HIP device (got {t.device}); there is no CPU path")


def _need_dense(fn, **named):
    """The kernel behind `fn` takes no row pitch for these tensors: a view that is not contiguous (a column slice of a wider
    buffer) would be read as if it were, so it is refused by name."""
    for name, t in named.items():
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous -- the kernel takes no row pitch for it (shape {tuple(t.shape)}, "
                             f"strides {tuple(t.stride())})")


def _need_rows(fn, **named):
    """Pitched operands: the row pitch is passed (stride(0)), the column stride must be 1."""
    for name, t in named.items():
        if t is not None and t.dim() >= 1 and t.stride(-1) != 1:
            raise ValueError(f"{fn}: {name} must have unit column stride (shape {tuple(t.shape)}, strides {tuple(t.stride())})")


# Parameter-gradient reductions of the training step (wgrad, bias / row-vector column sums, the mixing-weight dot product):
# True = ordered sums through scratch buffers (bit-reproducible gradients), False = fp32 atomics.
DETERMINISTIC = __import__("os").environ.get("CTRLV_DETERMINISTIC", "1") != "0"
_SCRATCH = {}


def _scratch(device, nbytes, tag, floor=1 << 20):
    """Kernel scratch, one buffer per (device, stream, purpose) of at least `floor` bytes, grown on demand: the launches of
    one stream are ordered, two streams (the ControlNet beside the UNet encoder) must not share it."""
    key = (device, torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), floor), dtype=torch.uint8, device=device)
        _SCRATCH[key] = buf
    return buf


def gemm_wgrad(A, dY, dW, *, N, cin, taps=1, mode=0, A2=None, c_split=0, conv=None, temporal=None, dbias=None, scale=1.0,
               torch_layout=False, assign=False):
    """dW[N, taps*cin] (fp32, packed tap-major K order) += scale * dY^T . gather(A) for the forward GEMM of the same
    geometry; dbias[N] (fp32, optional) += scale * column sums of dY.  torch_layout: dW is [N, cin, taps] (the conv
    parameter's own layout) instead of the packed [N, taps*cin].  assign (deterministic form only): dW / dbias are
    written, not accumulated into -- they need no zero fill."""
    _need_rows("gemm_wgrad", A=A, A2=A2, dY=dY)
    _need_dense("gemm_wgrad", dW=dW, dbias=dbias)
    _need_gpu(A, "A")
    d = GemmDesc()
    d.A, d.A2 = _p(A), _p(A2)
    d.M, d.N, d.Cin, d.taps, d.mode = dY.shape[0], N, cin, taps, mode
    d.lda = A.stride(0)
    d.lda2 = A2.stride(0) if A2 is not None else 0
    d.c_split = c_split
    if conv is not None:
        d.H, d.Wd, d.Ho, d.Wo, d.stride, d.up = conv
    if temporal is not None:
        d.F, d.S = temporal
    lib = _L(A, dY)
    # deterministic by default (DETERMINISTIC = False: fp32 atomics, arrival order): slab partials + an ordered sum
    scratch, nbytes = None, 0
    if DETERMINISTIC:
        nbytes = lib.ctrlv_gemm_wgrad_scratch_bytes(ctypes.byref(d))
        scratch = _scratch(A.device, nbytes, "wgrad")
    check(lib.ctrlv_gemm_wgrad(ctypes.byref(d), _p(dY), dY.stride(0), _p(dW), _p(dbias), float(scale),
                               (1 if torch_layout else 0) | (2 if assign else 0), _p(scratch), nbytes, _stream()),
          "ctrlv_gemm_wgrad")
    return dW


def pack_weight(weight, form=0, geglu=False, dtype=torch.bfloat16):
    """Element-type (`dtype`: bf16 / fp16) GEMM layout of a PyTorch-layout parameter in ONE kernel (ctrlv_pack_weight): form 0 = forward
    [N32, taps*C], form 1 = role-swapped dgrad [C32, taps*N64].  Returns None when the shape needs the torch packer
    (K not a multiple of 64 for Linear, odd channel counts)."""
    w = weight.detach()
    if not (w.is_cuda and w.is_contiguous() and w.dtype in _DT):
        return None
    N, C = w.shape[0], w.shape[1]
    taps = w.numel() // (N * C)
    if form == 0:
        if (taps == 1 and C % 64) or C % 8:
            return None
        rows, ld = (N + 31) // 32 * 32, taps * C
    else:
        if C % 32:
            return None
        rows, ld = C, taps * ((N + 63) // 64 * 64)
    dst = (torch.zeros if rows != (N if form == 0 else C) else torch.empty)(rows, ld, dtype=dtype, device=w.device)
    check(_L(dst).ctrlv_pack_weight(_p(w), _DT[w.dtype], N, C, taps, form, 1 if geglu else 0, _p(dst), ld, _stream()),
          "ctrlv_pack_weight")
    return dst


def lora_grad(X, dY, A, B, groups=1, scale=1.0):
    """Factor gradients of `groups` LoRA adapters side by side along dY's columns (ctrlv_lora_grad, deterministic):
    X [M, Cin] and dY [M, N] element rows; A fp32 [groups * r, Cin] (the groups' A factors stacked), B fp32 [N, r] (the
    groups' B factors stacked).  Returns (dA [groups * r, Cin], dB [N, r]) fp32 = scale * (G^T X, dY^T H) per group."""
    _need_gpu(X, "X")
    if X.stride(1) != 1 or dY.stride(1) != 1:
        raise ValueError("lora_grad: X and dY must be row-major (unit column stride)")
    A = A.detach().float().contiguous()
    B = B.detach().float().contiguous()
    M, cin = X.shape
    N, r = B.shape
    dA = torch.empty(A.shape, dtype=torch.float32, device=X.device)
    dB = torch.empty(N, r, dtype=torch.float32, device=X.device)
    d = _lib.LoraDesc()
    d.X, d.dY, d.A, d.B, d.dA, d.dB = _p(X), _p(dY), _p(A), _p(B), _p(dA), _p(dB)
    d.M, d.Cin, d.N, d.g, d.r = M, cin, N, groups, r
    d.ldx, d.ldy, d.scale = X.stride(0), dY.stride(0), float(scale)
    if A.shape[0] != groups * r or A.shape[1] != cin or dY.shape[0] != M or dY.shape[1] != N:
        raise ValueError(f"lora_grad: shapes X {tuple(X.shape)}, dY {tuple(dY.shape)}, A {tuple(A.shape)}, B {tuple(B.shape)}"
                         f" do not fit {groups} group(s)")
    lib = _L(X, dY)
    nbytes = lib.ctrlv_lora_grad_scratch_bytes(ctypes.byref(d))
    if nbytes == 0:
        check(lib.ctrlv_lora_grad(ctypes.byref(d), None, 0, _stream()), "ctrlv_lora_grad")      # (raises: the reason)
    scratch = _scratch(X.device, nbytes, "lora")
    check(lib.ctrlv_lora_grad(ctypes.byref(d), _p(scratch), nbytes, _stream()), "ctrlv_lora_grad")
    return dA, dB


def lora_merge(W, A, B, scale, out=None):
    """W + scale * B @ A in fp32, torch layout [N, Cin] (ctrlv_lora_merge).  W: any float dtype; A [r, Cin], B [N, r]."""
    _need_gpu(W, "W")
    W = W.detach().contiguous()
    A = A.detach().float().contiguous()
    B = B.detach().float().contiguous()
    N, cin = W.shape
    if A.shape[1] != cin or B.shape[0] != N or A.shape[0] != B.shape[1]:
        raise ValueError(f"lora_merge: W {tuple(W.shape)}, A {tuple(A.shape)}, B {tuple(B.shape)}")
    if out is None:
        out = torch.empty(N, cin, dtype=torch.float32, device=W.device)
    check(_L(W).ctrlv_lora_merge(_p(W), _DT[W.dtype], _p(A), _p(B), N, cin, A.shape[0], float(scale), _p(out), _stream()),
          "ctrlv_lora_merge")
    return out


def colsum(x, out, vmode=0, vdiv=1, vmod=1, scale=1.0):
    """out[idx(m), :N] += scale * sum_m x[m, :]  (fp32, atomics): bias gradients (vmode 0) / per-clip row-vector gradients."""
    _need_rows("colsum", x=x, out=out)
    _need_gpu(x, "x")
    lib = _L(x)
    scratch = None
    if DETERMINISTIC:
        nfl = lib.ctrlv_colsum_scratch_floats(x.shape[0], x.shape[1], vmode, vdiv)
        if nfl:
            scratch = _scratch(x.device, nfl * 4, "colsum")
    check(lib.ctrlv_colsum(_p(x), x.shape[0], x.shape[1], x.stride(0), vmode, vdiv, vmod, float(scale), _p(out),
                           out.stride(0) if out.dim() > 1 else x.shape[1], _p(scratch), _stream()), "ctrlv_colsum")
    return out


def dot_diff(dy, p, q, out, scale=1.0):
    _need_gpu(dy, "dy")
    scratch = _scratch(dy.device, 4096, "dot_diff") if DETERMINISTIC else None
    check(_L(dy).ctrlv_dot_diff(_p(dy), _p(p), _p(q), dy.numel(), float(scale), _p(out), _p(scratch), _stream()),
          "ctrlv_dot_diff")
    return out


def groupnorm_bwd(x, dy, n_img, S, C, imgs_per_stat, fwd_partials, gamma, beta, silu, dx, dgamma, dbeta, add=None):
    """add (rows like dy, optional): dx = (norm backward) + add -- the gradient of the skip connection around the branch the norm
    opens, summed in the same pass (ctrlv_groupnorm_bwd_add)."""
    _need_dense("groupnorm_bwd", x=x, dy=dy, add=add, fwd_partials=fwd_partials, gamma=gamma, beta=beta, dx=dx, dgamma=dgamma,
                dbeta=dbeta)
    _need_gpu(x, "x")
    lib = _L(x)
    n = lib.ctrlv_groupnorm_bwd_scratch_floats(n_img, S, C, imgs_per_stat)
    if n < 0:
        check(n, "ctrlv_groupnorm_bwd_scratch_floats")
    scratch = torch.empty(n, dtype=torch.float32, device=x.device)
    check(lib.ctrlv_groupnorm_bwd_add(_p(x), _p(dy), _p(add), n_img, S, C, imgs_per_stat, _p(fwd_partials), _p(gamma), _p(beta),
                                      1 if silu else 0, _p(dx), _p(dgamma), _p(dbeta), _p(scratch), _stream()),
          "ctrlv_groupnorm_bwd_add")
    return dx


def layernorm_bwd(x, dy, gamma, eps, dx, dgamma, dbeta, V=None, vdiv=1, vmod=1 << 30, add=None):
    _need_dense("layernorm_bwd", x=x, dy=dy, add=add, gamma=gamma, dx=dx, dgamma=dgamma, dbeta=dbeta)
    _need_rows("layernorm_bwd", V=V)
    _need_gpu(x, "x")
    M, C = x.shape
    lib = _L(x)
    scratch = torch.empty(lib.ctrlv_layernorm_bwd_scratch_floats(M, C), dtype=torch.float32, device=x.device)
    check(lib.ctrlv_layernorm_bwd_add(_p(x), _p(dy), _p(add), M, C, _p(gamma), eps, _p(V), vdiv, vmod,
                                      V.stride(0) if V is not None else 0, _p(dx), _p(dgamma), _p(dbeta), _p(scratch),
                                      _stream()), "ctrlv_layernorm_bwd_add")
    return dx


def geglu_bwd(raw, du, draw):
    _need_dense("geglu_bwd", raw=raw, du=du, draw=draw)
    _need_gpu(raw, "raw")
    check(_L(raw).ctrlv_geglu_bwd(_p(raw), _p(du), du.shape[0], du.shape[1], _p(draw), _stream()), "ctrlv_geglu_bwd")
    return draw


def _gemm_desc(A, W, out, *, N, cin, taps=1, mode=0, bias=None, A2=None, c_split=0, conv=None, temporal=None,
               R1=None, s1=1.0, R2=None, s2=1.0, s_acc=1.0, V=None, vmode=0, vdiv=1, vmod=1 << 30, vS=1,
               act=0, geglu=0, out_f32=False, n_store=None, M=None, tile=0, raw_out=None, n_scale2=0, s_acc2=1.0, _dbg=0,
               gn_partials=None, splitk=True, rows_per_image=0, R1_lo=None, R2_lo=None, out_lo=None, pad_br=False):
    _need_rows("gemm", A=A, A2=A2, out=out, R1=R1, R2=R2, V=V, raw_out=raw_out, R1_lo=R1_lo, R2_lo=R2_lo, out_lo=out_lo)
    d = GemmDesc()
    d.A, d.A2, d.W, d.out = _p(A), _p(A2), _p(W), _p(out)
    d.bias, d.R1, d.R2, d.V = _p(bias), _p(R1), _p(R2), _p(V)
    d.M = out.shape[0] if M is None else M
    d.N, d.Cin, d.taps = N, cin, taps
    d.lda = A.stride(0)
    d.lda2 = A2.stride(0) if A2 is not None else 0
    d.c_split = c_split
    d.mode = mode
    if conv is not None:
        d.H, d.Wd, d.Ho, d.Wo, d.stride, d.up = conv
    if temporal is not None:
        d.F, d.S = temporal
    elif mode == 0 and rows_per_image:
        d.S = rows_per_image          # mode 0: the split plan's shape key (rows per image)
    d.ldo = out.stride(0)
    d.n_store = out.shape[1] if n_store is None else n_store
    d.ldr1 = R1.stride(0) if R1 is not None else 0
    d.ldr2 = R2.stride(0) if R2 is not None else 0
    d.s_acc, d.s1, d.s2 = s_acc, s1, s2
    d.vmode = vmode if V is not None else 0
    d.vdiv, d.vmod, d.vS = vdiv, vmod, vS
    d.ldv = V.stride(0) if V is not None else 0
    d.act, d.geglu, d.out_f32, d.tile = act, geglu, (_dbg if _dbg else (1 if out_f32 else 0)), tile
    if raw_out is not None:
        d.raw_out, d.ld_raw = _p(raw_out), raw_out.stride(0)
    d.n_scale2, d.s_acc2 = n_scale2, s_acc2
    d.gn_partials = _p(gn_partials)
    # split residual-trunk planes (fp16 library; include/ctrlv_hip.h): same shapes / pitches as R1 / R2 / out
    d.R1_lo, d.R2_lo, d.out_lo = _p(R1_lo), _p(R2_lo), _p(out_lo)
    d.pad_br = int(pad_br)            # mode 1, stride 2: padding on the bottom / right only (the VAE encoder's down-samplers)
    return d


def gemm_splitk_slices(A, W, out, **kw):
    """K slices `gemm(A, W, out, **kw)` runs this launch in (1 = not split): scratch bytes / (M * N * 4)."""
    d = _gemm_desc(A, W, out, **kw)
    return max(1, _L(A, W).ctrlv_gemm_splitk_ws_bytes(ctypes.byref(d)) // (d.M * d.N * 4))


def gemm_gn_partials_serves(A, W, out, **kw):
    """Whether `gemm(A, W, out, **kw, gn_partials=...)` writes GroupNorm chunk partials of `out` (the launcher's own
    predicate: a function of the layer's shape, never of the batch size)."""
    return bool(_L(A, W).ctrlv_gemm_gn_partials_serves(ctypes.byref(_gemm_desc(A, W, out, **kw))))


def gemm_up_phase_serves(A, W, out, **kw):
    """Whether the nearest-x2 upsampler conv `gemm(A, W, out, **kw)` (mode 1, conv = (H, W, 2H, 2W, 1, 1 or 2)) is served in
    phase form, i.e. with conv[5] = 2 and W = `pack_up_phase_weight(...)` -- the launcher's own predicate: a function of
    the layer's shape, never of the image count."""
    return bool(_L(A, W).ctrlv_gemm_up_phase_serves(ctypes.byref(_gemm_desc(A, W, out, **kw))))


def pack_up_phase_weight(weight, dtype=torch.bfloat16):
    """The four 2x2 phase panels [4, N, 4*Cin] (element type `dtype`) of an upsampler conv's parameter [N, Cin, 3, 3] for
    `gemm(..., conv=(H, W, 2H, 2W, 1, 2))`: the taps of each phase summed in fp32 and rounded once
    (ctrlv_pack_up_phase_weight)."""
    w = weight.detach().contiguous()
    _need_gpu(w, "weight")
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.dtype not in _DT:
        raise ValueError(f"pack_up_phase_weight: expected a float [N, Cin, 3, 3] parameter, got {tuple(w.shape)} {w.dtype}")
    N, C = w.shape[:2]
    dst = torch.empty(4, N, 4 * C, dtype=dtype, device=w.device)
    check(_L(dst).ctrlv_pack_up_phase_weight(_p(w), _DT[w.dtype], N, C, _p(dst), _stream()), "ctrlv_pack_up_phase_weight")
    return dst


def gemm(A, W, out, **kw):
    """out = epilogue(gather-GEMM(A[, A2], W)).  `conv` = (H, W, Ho, Wo, stride, up); `temporal` = (F, S).
    Keywords: see `_gemm_desc` (the fields of ctrlv_gemm_desc)."""
    d = _gemm_desc(A, W, out, **kw)
    _need_gpu(A, "A")
    lib = _L(A, W)
    if kw.get("splitk", True):
        # split contraction of the small-image long-K convs (csrc/gemm.hip splitk_plan): the scratch is what enables it, and
        # it is offered to EVERY launch -- the plan is a function of the layer's shape, so a clip takes the same path alone
        # and in a batch
        need = lib.ctrlv_gemm_splitk_ws_bytes(ctypes.byref(d))
        if need:
            d.splitk_ws = _p(_scratch(A.device, need, "splitk", floor=64 << 20))      # (fp32 partials of the K slices)
    cin, taps, mode, geglu = d.Cin, d.taps, d.mode, d.geglu
    wf = 1
    if mode == 1 and d.up == 2:         # phase form of the upsampler conv: 2x2 taps per output pixel, four weight panels
        taps, wf = 4, 4
    R1, R2, raw_out, act = kw.get("R1"), kw.get("R2"), kw.get("raw_out"), kw.get("act", 0)
    out_f32 = kw.get("out_f32", False)
    ev = _prof.begin()
    check(lib.ctrlv_gemm(ctypes.byref(d), _stream()), "ctrlv_gemm")
    if ev is not None:
        n_alg = d.N if geglu else min(d.N, d.n_store)
        fam = "gemm_conv3x3" if mode == 1 else ("gemm_conv_temporal" if mode == 2 else "gemm_linear")
        esz = 4 if out_f32 else 2
        n_out = d.n_store if not geglu else min(d.n_store, d.N // 2)
        nbytes = (d.M * cin * 2 * (1 if mode == 0 else 1) + d.M * n_out * esz + d.N * taps * cin * 2 * wf
                  + (d.M * n_out * 2 if R1 is not None else 0) + (d.M * n_out * 2 if R2 is not None else 0)
                  + (d.M * n_out * 2 if raw_out is not None else 0))
        _prof.end(ev, fam, 2.0 * d.M * n_alg * taps * cin, float(nbytes),
                  detail=(fam, d.M, d.N, taps * cin, int(geglu), int(R1 is not None) + int(R2 is not None), d.vmode, act))
    return out


def quant_rows_f8(x, q=None, scale=None, ln=None, V=None, vdiv=1, vmod=1 << 30):
    """Row quantisation to OCP e4m3 (torch.float8_e4m3fn codes as uint8) with one fp32 scale per row: scale[m] = max|y[m]| /
    448 (1 for an all-zero row), q[m, k] = e4m3(y[m, k] / scale[m]), y = x or -- ln = (gamma, beta, eps) -- the fp32 value
    of `layernorm(x + V[...])`, never rounded to 16 bits (csrc/quant_f8.hip).  x: [M, K] element rows (row stride a
    multiple of 8); q: uint8 [M, >= K] (allocated when None), scale: fp32 [M].  Returns (q, scale).  Weights [N, K] are
    quantised by the same call."""
    _need_gpu(x, "x")
    M, K = x.shape
    if x.stride(1) != 1:
        raise ValueError("quant_rows_f8: rows must be contiguous")
    if q is None:
        q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    if scale is None:
        scale = torch.empty(M, dtype=torch.float32, device=x.device)
    if q.dtype != torch.uint8 or scale.dtype != torch.float32 or q.shape[0] != M or scale.numel() < M or q.stride(1) != 1:
        raise ValueError("quant_rows_f8: q must be uint8 [M, >= K] and scale fp32 [M]")
    g, b, eps = (ln[0], ln[1], float(ln[2])) if ln is not None else (None, None, 0.0)
    ev = _prof.begin()
    check(_L(x).ctrlv_quant_rows_f8(_p(x), M, K, x.stride(0), _p(g), _p(b), eps, _p(V), vdiv, vmod,
                                    V.stride(0) if V is not None else 0, _p(q), q.stride(0), _p(scale), _stream()),
          "ctrlv_quant_rows_f8")
    _prof.end(ev, "layernorm", 0.0, 3.0 * M * K, detail=("quant_rows_f8", M, K, 0, 0, 0, 0, 0))
    return q, scale


def _gemm_f8_desc(A, W, out, *, N, cin, el=None, **kw):
    """(descriptor, library): the element library is the one of `out` / R1 / R2, or -- fp32 output without residuals -- `el`"""
    if A.dtype != torch.uint8 or W.dtype != torch.uint8:
        raise ValueError("gemm_f8: A and W hold e4m3 codes as uint8 (quant_rows_f8)")
    lib = _lib.load(el) if el is not None else _L(out, kw.get("R1"), kw.get("R2"))
    return _gemm_desc(A, W, out, N=N, cin=cin, **kw), lib


def gemm_f8_serves(A, W, out, **kw):
    """Whether `gemm_f8(A, W, out, ...)` is served (the launcher's own predicate, host code: csrc/gemm_f8.hip) -- mode 0, no
    lo planes, K a multiple of 128 (so not the C = 320 feed-forward, which keeps ff_fused), N a multiple of 32, 16-byte pitches:
    a function of the layer's shape only."""
    d, lib = _gemm_f8_desc(A, W, out, **kw)
    return bool(lib.ctrlv_gemm_f8_serves(ctypes.byref(d)))


def gemm_f8(A, a_scale, W, w_scale, out, **kw):
    """out = epilogue(a_scale[m] w_scale[n] (A @ W^T)[m, n] + bias[n]) with A [M, K], W [N, K] e4m3 codes (uint8) and fp32 row
    scales (quant_rows_f8), on the K = 64 block-scaled MFMA at twice the 16-bit rate; epilogue keywords as `gemm` (bias, geglu,
    R1 / R2 / s1 / s2 / s_acc, V with vmode 1 / 2, n_store, out_f32).  The element library is the one of `out` / R1 / R2; an
    fp32 output without residuals names it with el=torch.float16 / torch.bfloat16 (default bf16)."""
    d, lib = _gemm_f8_desc(A, W, out, **kw)
    _need_gpu(A, "A")
    ev = _prof.begin()
    check(lib.ctrlv_gemm_f8(ctypes.byref(d), _p(a_scale), _p(w_scale), _stream()), "ctrlv_gemm_f8")
    if ev is not None:
        n_out = d.n_store if not d.geglu else min(d.n_store, d.N // 2)
        R1, R2 = kw.get("R1"), kw.get("R2")
        nbytes = d.M * d.Cin + d.N * d.Cin + d.M * n_out * (4 if kw.get("out_f32") else 2) * (1 + (R1 is not None) + (R2 is not None))
        _prof.end(ev, "gemm_linear", 2.0 * d.M * d.N * d.Cin, float(nbytes),
                  detail=("gemm_f8", d.M, d.N, d.Cin, int(d.geglu), int(R1 is not None) + int(R2 is not None), d.vmode, 0))
    return out


def ff_fused_pack(w1_packed, b1, w2_packed):
    """Fragment-major copies (w1f, w2f) of a C = 320 feed-forward's packed weights for `ff_fused`: w1_packed = the GEGLU
    projection in the interleaved packed form [2560, 320], b1 = its bias (fp32 [2560], same row order; carried inside w1f),
    w2_packed = the output projection [320, 1280]."""
    _need_gpu(w1_packed, "w1_packed")
    assert tuple(w1_packed.shape) == (2560, 320) and tuple(w2_packed.shape) == (320, 1280) and b1.numel() == 2560
    assert w1_packed.dtype in (torch.bfloat16, torch.float16) and w2_packed.dtype == w1_packed.dtype and b1.dtype == torch.float32
    assert w1_packed.is_contiguous() and w2_packed.is_contiguous() and b1.is_contiguous()
    lib = _L(w1_packed)
    w1f = torch.empty(lib.ctrlv_ff_fused_w1f_bytes() // 2, dtype=w1_packed.dtype, device=w1_packed.device)
    w2f = torch.empty_like(w2_packed)
    check(lib.ctrlv_ff_fused_pack(_p(w1_packed), _p(b1), _p(w2_packed), _p(w1f), _p(w2f), _stream()), "ctrlv_ff_fused_pack")
    return w1f, w2f


def _ff_out_desc(out, bias=None, R1=None, s1=1.0, R2=None, s2=1.0, s_acc=1.0, V=None, vmode=0, vdiv=1, vmod=1 << 30, vS=1,
                 R1_lo=None, R2_lo=None, out_lo=None):
    """The second projection's descriptor of a C = 320 feed-forward (what ctrlv_ff_fused / ctrlv_ff_fused_serves take)."""
    _need_rows("ff_fused", out=out, R1=R1, R2=R2, V=V, R1_lo=R1_lo, R2_lo=R2_lo, out_lo=out_lo)
    d = GemmDesc()
    d.out, d.bias, d.R1, d.R2, d.V = _p(out), _p(bias), _p(R1), _p(R2), _p(V)
    d.R1_lo, d.R2_lo, d.out_lo = _p(R1_lo), _p(R2_lo), _p(out_lo)
    d.M, d.N, d.Cin, d.taps, d.mode = out.shape[0], out.shape[1], 4 * out.shape[1], 1, 0
    d.ldo, d.n_store = out.stride(0), out.shape[1]
    d.ldr1 = R1.stride(0) if R1 is not None else 0
    d.ldr2 = R2.stride(0) if R2 is not None else 0
    d.s_acc, d.s1, d.s2 = s_acc, s1, s2
    d.vmode = vmode if V is not None else 0
    d.vdiv, d.vmod, d.vS = vdiv, vmod, vS
    d.ldv = V.stride(0) if V is not None else 0
    return d


def ff_fused_serves(x, out, **epi):
    """Whether `ff_fused(x, ..., out, **epi)` is served by the fused kernel (else: the two `gemm` launches) -- the
    launcher's own conditions (csrc/ff_fused.hip ff_check)."""
    d = _ff_out_desc(out, **{k: v for k, v in epi.items() if k != "bias"})
    return bool(_L(x).ctrlv_ff_fused_serves(ctypes.byref(d), x.stride(0)))


def ff_fused(x, w1f, w2f, out, *, bias=None, R1=None, s1=1.0, R2=None, s2=1.0, s_acc=1.0, V=None, vmode=0, vdiv=1,
             vmod=1 << 30, vS=1, ln=None, ln_V=None, ln_vdiv=1, ln_vmod=1 << 30, R1_lo=None, R2_lo=None, out_lo=None):
    """out = s_acc * (GEGLU(x W1^T + b1) W2^T + bias) + s1 R1 + s2 R2 + V[idx(m)] for a C = 320 feed-forward, the 4C-wide
    intermediate kept on chip (csrc/ff_fused.hip).  The epilogue operands are those of `gemm`."""
    _need_rows("ff_fused", x=x, ln_V=ln_V)
    d = _ff_out_desc(out, bias, R1, s1, R2, s2, s_acc, V, vmode, vdiv, vmod, vS, R1_lo, R2_lo, out_lo)
    _need_gpu(x, "x")
    ev = _prof.begin()
    if ln is None:        # ln = (gamma, beta, eps): the LayerNorm in front of the feed-forward, folded into the kernel
        check(_L(x).ctrlv_ff_fused(_p(x), x.stride(0), _p(w1f), _p(w2f), ctypes.byref(d), _stream()),
              "ctrlv_ff_fused")
    else:
        check(_L(x).ctrlv_ff_fused_ln(_p(x), x.stride(0), _p(ln[0]), _p(ln[1]), float(ln[2]), _p(ln_V), ln_vdiv,
                                      ln_vmod, ln_V.stride(0) if ln_V is not None else 0, _p(w1f), _p(w2f),
                                      ctypes.byref(d), _stream()), "ctrlv_ff_fused_ln")
    if ev is not None:
        M = out.shape[0]
        nbytes = M * 320 * 2 * (2 + (R1 is not None) + (R2 is not None))
        _prof.end(ev, "gemm_linear", 2.0 * M * 320 * (2560 + 1280), float(nbytes),
                  detail=("ff_fused", M, 320, 320, 1, int(R1 is not None) + int(R2 is not None), d.vmode, 0))
    return out


def groupnorm_chunks(n_img, S, C, imgs_per_stat):
    rc = _lib.load().ctrlv_groupnorm_chunks(n_img, S, C, imgs_per_stat)
    if rc < 0:
        check(rc, "ctrlv_groupnorm_chunks")
    return rc


def groupnorm_scratch_floats(n_img, S, C, imgs_per_stat):
    """fp32 elements `groupnorm` needs in `partials`: chunk partials + the (mean, rstd) table behind them."""
    return (n_img * groupnorm_chunks(n_img, S, C, imgs_per_stat) + n_img // imgs_per_stat) * 64


def groupnorm_fused_scratch_floats(n_img, S, imgs_per_stat):
    """fp32 elements of `partials` for `gemm(..., gn_partials=)` + `groupnorm_from_partials` (64-row chunks)."""
    return (n_img * (S // 64) + n_img // imgs_per_stat) * 64


def groupnorm_from_partials(x, n_img, S, C, imgs_per_stat, gamma, beta, eps, silu, y, partials, x_lo=None):
    """GroupNorm(+SiLU) of a tensor whose producing `gemm` wrote the chunk partials: finalize + apply.  x_lo: the lo plane of
    a SPLIT tensor (the launch wrote out_lo and gn_partials together; the normalised value is x + x_lo)."""
    _need_dense("groupnorm_from_partials", x=x, x_lo=x_lo, y=y, partials=partials, gamma=gamma, beta=beta)
    _need_gpu(x, "x")
    assert partials.numel() >= groupnorm_fused_scratch_floats(n_img, S, imgs_per_stat)
    ev = _prof.begin()
    check(_L(x).ctrlv_groupnorm_from_partials_split(_p(x), _p(x_lo), n_img, S, C, imgs_per_stat, eps, _p(partials), _p(gamma),
                                                    _p(beta), 1 if silu else 0, _p(y), _stream()),
          "ctrlv_groupnorm_from_partials")
    _prof.end(ev, "groupnorm", 0.0, 2.0 * 2 * n_img * S * C)
    return y


def groupnorm(x, x2, n_img, S, C, imgs_per_stat, gamma, beta, eps, silu, y, partials, x_lo=None, x2_lo=None):
    """Two-pass GroupNorm(32)(+SiLU) over channels-last rows; (x | x2) is a channel concat when x2 is given.  x_lo / x2_lo:
    the lo planes of a SPLIT input (the normalised value is x + x_lo)."""
    _need_dense("groupnorm", x=x, x2=x2, x_lo=x_lo, x2_lo=x2_lo, y=y, partials=partials, gamma=gamma, beta=beta)
    _need_gpu(x, "x")
    lib = _L(x)
    c_split = x.shape[1] if x2 is not None else 0
    st = _stream()
    ev = _prof.begin()
    check(lib.ctrlv_groupnorm_stats_split(_p(x), _p(x_lo), _p(x2), _p(x2_lo), c_split, n_img, S, C, imgs_per_stat, eps,
                                          _p(partials), st), "ctrlv_groupnorm_stats")
    check(lib.ctrlv_groupnorm_apply_split(_p(x), _p(x_lo), _p(x2), _p(x2_lo), c_split, n_img, S, C, imgs_per_stat,
                                          _p(partials), _p(gamma), _p(beta), 1 if silu else 0, _p(y), st),
          "ctrlv_groupnorm_apply")
    _prof.end(ev, "groupnorm", 0.0, 2.0 * 2 * n_img * S * C)       # algorithmic: 1 read + 1 write, bf16
    return y


def layernorm(x, gamma, beta, eps, y, V=None, vdiv=1, vmod=1 << 30, x_lo=None):
    _need_dense("layernorm", x=x, x_lo=x_lo, y=y, gamma=gamma, beta=beta)
    _need_rows("layernorm", V=V)
    _need_gpu(x, "x")
    M, C = x.shape
    ev = _prof.begin()
    check(_L(x).ctrlv_layernorm_split(_p(x), _p(x_lo), M, C, _p(gamma), _p(beta), eps, _p(V), vdiv, vmod,
                                      V.stride(0) if V is not None else 0, _p(y), _stream()), "ctrlv_layernorm")
    _prof.end(ev, "layernorm", 0.0, 2.0 * 2 * M * C)
    return y


Q_PRESCALE = 0.125 * 1.44269504088896340736      # (1/sqrt(64)) * log2(e): the q block scale of the prescaled core


def attention_spatial(qkv, out, n_img, S, C, prescaled=False):
    """prescaled: the q columns already carry Q_PRESCALE (gemm(..., n_scale2=C, s_acc2=Q_PRESCALE))."""
    _need_dense("attention_spatial", qkv=qkv, out=out)
    _need_gpu(qkv, "qkv")
    ev = _prof.begin()
    fn = _L(qkv).ctrlv_attention_spatial_prescaled if prescaled else _L(qkv).ctrlv_attention_spatial
    check(fn(_p(qkv), _p(out), n_img, S, C, _stream()), "ctrlv_attention_spatial")
    _prof.end(ev, "attention_spatial", 4.0 * n_img * (C // 64) * S * S * 64, 2.0 * 4 * n_img * S * C)
    return out


def attention_spatial_lse(qkv, out, lse, n_img, S, C):
    """Training forward: also writes lse [n_img, C/64, S] fp32 (log2-domain log-sum-exp of the scaled scores)."""
    _need_dense("attention_spatial_lse", qkv=qkv, out=out, lse=lse)
    _need_gpu(qkv, "qkv")
    ev = _prof.begin()
    check(_L(qkv).ctrlv_attention_spatial_lse(_p(qkv), _p(out), _p(lse), n_img, S, C, _stream()),
          "ctrlv_attention_spatial_lse")
    _prof.end(ev, "attention_spatial", 4.0 * n_img * (C // 64) * S * S * 64, 2.0 * 4 * n_img * S * C)
    return out


def attention_spatial_bwd(qkv, out, dout, lse, dqkv, n_img, S, C):
    _need_dense("attention_spatial_bwd", qkv=qkv, out=out, dout=dout, lse=lse, dqkv=dqkv)
    _need_gpu(qkv, "qkv")
    delta = torch.empty(_L(qkv).ctrlv_attention_bwd_scratch_floats(n_img, S, C), dtype=torch.float32, device=qkv.device)
    ev = _prof.begin()
    check(_L(qkv).ctrlv_attention_spatial_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), _p(delta), n_img, S, C,
                                                  _stream()), "ctrlv_attention_spatial_bwd")
    _prof.end(ev, "attention_spatial_bwd", 14.0 * n_img * (C // 64) * S * S * 64, 2.0 * 8 * n_img * S * C)
    return dqkv


def attention_temporal_bwd(qkv, out, dout, dqkv, B, F, S, C):
    _need_dense("attention_temporal_bwd", qkv=qkv, out=out, dout=dout, dqkv=dqkv)
    _need_gpu(qkv, "qkv")
    ev = _prof.begin()
    check(_L(qkv).ctrlv_attention_temporal_bwd(_p(qkv), _p(out), _p(dout), _p(dqkv), B, F, S, C, _stream()),
          "ctrlv_attention_temporal_bwd")
    _prof.end(ev, "attention_temporal_bwd", 14.0 * B * S * (C // 64) * F * F * 64, 2.0 * 8 * B * F * S * C)
    return dqkv


def attention_temporal(qkv, out, B, F, S, C):
    _need_dense("attention_temporal", qkv=qkv, out=out)
    _need_gpu(qkv, "qkv")
    ev = _prof.begin()
    check(_L(qkv).ctrlv_attention_temporal(_p(qkv), _p(out), B, F, S, C, _stream()), "ctrlv_attention_temporal")
    _prof.end(ev, "attention_temporal", 4.0 * B * S * (C // 64) * F * F * 64, 2.0 * 4 * B * F * S * C)
    return out


def attention_tokens(qkv, out, n_img, S, C, head_dim):
    """Self-attention over the S tokens of each image at any 1 <= S <= 4096 and head_dim 16..128 (a multiple of 16): the CLIP
    vision tower's core (ctrlv_attention_tokens; qkv [n_img*S, 3C] with q | k | v column blocks, out [n_img*S, C])."""
    _need_gpu(qkv, "qkv")
    if qkv.stride(0) != 3 * C or out.stride(0) != C or qkv.stride(1) != 1 or out.stride(1) != 1:
        raise ValueError("attention_tokens: qkv [rows, 3C] and out [rows, C] must be dense row-major")
    if qkv.shape[0] < n_img * S or out.shape[0] < n_img * S:
        raise ValueError(f"attention_tokens: {n_img} x {S} rows do not fit qkv {tuple(qkv.shape)} / out {tuple(out.shape)}")
    ev = _prof.begin()
    check(_L(qkv, out).ctrlv_attention_tokens(_p(qkv), _p(out), n_img, S, C, head_dim, _stream()), "ctrlv_attention_tokens")
    _prof.end(ev, "attention_tokens", 4.0 * n_img * S * S * C, 2.0 * 4 * n_img * S * C)
    return out


def clip_patch_rows(pixels, patch, rows):
    """pixels: contiguous (n, 3, H, W) fp32 / fp16 / bf16 -> rows [n * (H/patch) * (W/patch), ld] in the element type, columns in
    (c, dy, dx) order, columns >= 3 patch^2 zero (ctrlv_clip_patch_rows)."""
    _need_gpu(pixels, "pixels")
    if pixels.dim() != 4 or pixels.shape[1] != 3 or not pixels.is_contiguous() or pixels.dtype not in _DT:
        raise ValueError("clip_patch_rows: pixels must be contiguous (n, 3, H, W) in fp32 / fp16 / bf16")
    n, _, H, W = pixels.shape
    if patch <= 0 or H % patch or W % patch or rows.shape[0] != n * (H // patch) * (W // patch) or rows.stride(1) != 1:
        raise ValueError(f"clip_patch_rows: image {H}x{W}, patch {patch}, rows {tuple(rows.shape)}")
    ev = _prof.begin()
    check(_L(rows).ctrlv_clip_patch_rows(_p(pixels), _DT[pixels.dtype], n, H, W, patch, _p(rows), rows.stride(0), _stream()),
          "ctrlv_clip_patch_rows")
    _prof.end(ev, "clip_patch_rows", 0.0, float(pixels.numel() * pixels.element_size() + rows.numel() * 2))
    return rows


def clip_tokens(patch_out, class_emb, pos_emb, n, out):
    """out [n * (P + 1), C] = (class_emb + pos_emb[0] | patch_out[p] + pos_emb[p + 1]) per image: fp32 sum, one rounding
    (ctrlv_clip_tokens).  patch_out [n * P, C] elements; class_emb fp32 [C]; pos_emb fp32 [P + 1, C]."""
    _need_gpu(patch_out, "patch_out")
    P, C = pos_emb.shape[0] - 1, pos_emb.shape[1]
    if (class_emb.dtype != torch.float32 or pos_emb.dtype != torch.float32 or not class_emb.is_contiguous()
            or not pos_emb.is_contiguous() or not patch_out.is_contiguous() or not out.is_contiguous()
            or tuple(patch_out.shape) != (n * P, C) or tuple(out.shape) != (n * (P + 1), C) or class_emb.numel() != C):
        raise ValueError("clip_tokens: dense patch_out [n*P, C], out [n*(P+1), C]; fp32 class_emb [C], pos_emb [P+1, C]")
    ev = _prof.begin()
    check(_L(patch_out, out).ctrlv_clip_tokens(_p(patch_out), _p(class_emb), _p(pos_emb), n, P, C, _p(out), _stream()),
          "ctrlv_clip_tokens")
    _prof.end(ev, "clip_tokens", 0.0, 2.0 * (patch_out.numel() + out.numel()))
    return out


ACT_KINDS = {"gelu": 0, "quick_gelu": 1}


def act_rows(x, kind):
    """In place on the element rows x [M, N] (any row pitch that is a multiple of 8): "gelu" (erf form) or "quick_gelu"
    (x sigmoid(1.702 x)); fp32 arithmetic, one rounding (ctrlv_act_rows)."""
    _need_gpu(x, "x")
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("act_rows: x must be 2-D with unit column stride")
    ev = _prof.begin()
    check(_L(x).ctrlv_act_rows(_p(x), x.shape[0], x.shape[1], x.stride(0), ACT_KINDS[kind] if isinstance(kind, str) else kind,
                               _stream()), "ctrlv_act_rows")
    _prof.end(ev, "act_rows", 0.0, 2.0 * 2 * x.shape[0] * x.shape[1])
    return x


TOKEN_ACTS = {None: 0, "none": 0, "gelu": 1, "quick_gelu": 2}


def gemm_tokens_plan(N, K, dtype=None):
    """(bn, slices) of ctrlv_gemm_tokens for a weight [N, K]: a function of (N, K) only."""
    bn, sl = ctypes.c_int32(), ctypes.c_int32()
    check(_lib.load(dtype).ctrlv_gemm_tokens_plan(N, K, ctypes.byref(bn), ctypes.byref(sl)), "ctrlv_gemm_tokens_plan")
    return bn.value, sl.value


def gemm_tokens(A, W, out, *, N, K, bias=None, R1=None, act=None, M=None, workspace=None, ws_zeroed=False):
    """out[m, n] = act(sum_k A[m, k] W[n, k] + bias[n]) + R1[m, n] for a few hundred rows (ctrlv_gemm_tokens): W elements
    [N, K] as packing.pack_linear makes them, bias fp32, act None / "gelu" (erf form) / "quick_gelu" evaluated in fp32 before the
    one rounding.  K slices are combined inside the launch through `workspace` (a uint8 tensor of at least
    ctrlv_gemm_tokens_ws_bytes; default: this stream's scratch).  ws_zeroed: the caller vouches that the counter words at the
    head of `workspace` are zero -- they are after every call of the same (N, K) into it -- and no memset is enqueued."""
    _need_gpu(A, "A")
    if W.dim() != 2 or W.stride(1) != 1 or W.stride(0) != K or W.shape[0] < N:
        raise ValueError(f"gemm_tokens: W must be dense [>= N, K] rows (got {tuple(W.shape)}, strides {tuple(W.stride())}; N={N}, K={K})")
    if ws_zeroed and workspace is None:
        raise ValueError("gemm_tokens: ws_zeroed needs the caller's own workspace")
    lib = _L(A, W, out, R1)
    d = _lib.GemmTokensDesc()
    d.A, d.W, d.bias, d.R1, d.out = _p(A), _p(W), _p(bias), _p(R1), _p(out)
    d.M = out.shape[0] if M is None else M
    d.N, d.K = N, K
    d.lda, d.ldo = A.stride(0), out.stride(0)
    d.ldr1 = R1.stride(0) if R1 is not None else 0
    d.act = TOKEN_ACTS[act] if (act is None or isinstance(act, str)) else act
    d.ws_zeroed = 1 if ws_zeroed else 0
    if workspace is None and d.M >= 1 and N > 0 and K > 0 and N % 32 == 0 and K % 64 == 0:
        need = lib.ctrlv_gemm_tokens_ws_bytes(d.M, N, K)
        if need:
            workspace = _scratch(A.device, need, "gemm_tokens", floor=16 << 20)
    if workspace is not None:
        d.workspace, d.workspace_bytes = _p(workspace), workspace.numel() * workspace.element_size()
    ev = _prof.begin()
    check(lib.ctrlv_gemm_tokens(ctypes.byref(d), _stream()), "ctrlv_gemm_tokens")
    if ev is not None:
        nbytes = 2.0 * (d.M * K + N * K + d.M * N * (2 if R1 is not None else 1))
        _prof.end(ev, "gemm_linear", 2.0 * d.M * N * K, nbytes, detail=("gemm_tokens", d.M, N, K, 0, int(R1 is not None), 0, d.act))
    return out


def temporal_fused_pack(wqkv_packed, wo_packed):
    """Fragment-major weights of `temporal_fused` from the packed [960, >= 320] q|k|v projection and [320, >= 320] to_out."""
    _need_gpu(wqkv_packed, "wqkv_packed")
    assert wqkv_packed.shape[0] == 960 and wo_packed.shape[0] == 320 and wqkv_packed.dtype == wo_packed.dtype
    lib = _L(wqkv_packed)
    wf = torch.empty(lib.ctrlv_temporal_fused_weight_bytes() // 2, dtype=wqkv_packed.dtype, device=wqkv_packed.device)
    check(lib.ctrlv_temporal_fused_pack(_p(wqkv_packed), wqkv_packed.stride(0), _p(wo_packed), wo_packed.stride(0), _p(wf),
                                        _stream()), "ctrlv_temporal_fused_pack")
    return wf


def _temporal_fused_desc(x, wf, out, B, F, S, bias=None, R1=None, V=None, vmode=0, vdiv=1, vmod=1 << 30, vS=1, R1_lo=None,
                         out_lo=None, ln=None):
    from ._lib import TemporalFusedDesc
    _need_rows("temporal_fused", x=x, out=out, R1=R1, V=V, R1_lo=R1_lo, out_lo=out_lo)
    d = TemporalFusedDesc()
    d.x, d.ldx, d.wf, d.bias = _p(x), x.stride(0), _p(wf), _p(bias)
    d.R1, d.R1_lo, d.ldr1 = _p(R1), _p(R1_lo), (R1.stride(0) if R1 is not None else 0)
    d.V, d.vmode, d.vdiv, d.vmod, d.vS = _p(V), (vmode if V is not None else 0), vdiv, vmod, vS
    d.ldv = V.stride(0) if V is not None else 0
    d.out, d.out_lo, d.ldo = _p(out), _p(out_lo), out.stride(0)
    d.B, d.F, d.S, d.C = B, F, S, x.shape[1]
    if ln is not None:                       # (gamma, beta, eps): x holds the raw rows, the kernel normalises them
        d.ln_gamma, d.ln_beta, d.ln_eps = _p(ln[0]), _p(ln[1]), float(ln[2])
    return d


def temporal_fused_serves(x, wf, out, B, F, S, **kw):
    return wf is not None and bool(_L(x).ctrlv_temporal_fused_serves(ctypes.byref(_temporal_fused_desc(x, wf, out, B, F, S, **kw))))


def temporal_fused(x, wf, out, B, F, S, **kw):
    """out = R1 + to_out(softmax_f(q k^T / 8) v) + bias + V[clip], (q|k|v) = x W_qkv^T, over the F frames of every pixel:
    the temporal self-attention block at C = 320 in one launch (csrc/temporal_fused.hip)."""
    d = _temporal_fused_desc(x, wf, out, B, F, S, **kw)
    _need_gpu(x, "x")
    ev = _prof.begin()
    check(_L(x).ctrlv_temporal_fused(ctypes.byref(d), _stream()), "ctrlv_temporal_fused")
    M, C = B * F * S, x.shape[1]
    _prof.end(ev, "gemm_temporal_block", 2.0 * M * C * 4 * C + 4.0 * B * S * (C // 64) * F * F * 64,
              2.0 * (2 if kw.get("ln") is not None else 3) * M * C)
    return out


def spatial_entry_fused_pack(win_packed, wqkv_packed):
    """Fragment-major weights of `spatial_entry_fused` from the packed [320, >= 320] proj_in and [960, >= 320] q|k|v projection."""
    _need_gpu(win_packed, "win_packed")
    assert win_packed.shape[0] == 320 and wqkv_packed.shape[0] == 960 and wqkv_packed.dtype == win_packed.dtype
    lib = _L(win_packed)
    wf = torch.empty(lib.ctrlv_spatial_entry_fused_weight_bytes() // 2, dtype=win_packed.dtype, device=win_packed.device)
    check(lib.ctrlv_spatial_entry_fused_pack(_p(win_packed), win_packed.stride(0), _p(wqkv_packed), wqkv_packed.stride(0), _p(wf),
                                             _stream()), "ctrlv_spatial_entry_fused_pack")
    return wf


def _spatial_entry_desc(x, wf, stats, gn, ln, h0, qkv, n_img, S, bias_in=None, bias_qkv=None, x_lo=None, h0_lo=None,
                        head_dim=64, q_scale=None):
    from ._lib import SpatialEntryDesc
    _need_rows("spatial_entry_fused", x=x, h0=h0, qkv=qkv)
    d = SpatialEntryDesc()
    d.x, d.x_lo, d.ldx, d.wf = _p(x), _p(x_lo), x.stride(0), _p(wf)
    d.bias_in, d.bias_qkv, d.stats = _p(bias_in), _p(bias_qkv), _p(stats)
    d.gn_gamma, d.gn_beta = _p(gn[0]), _p(gn[1])
    d.ln_gamma, d.ln_beta, d.ln_eps = _p(ln[0]), _p(ln[1]), float(ln[2])
    d.h0, d.h0_lo, d.ldh = _p(h0), _p(h0_lo), h0.stride(0)
    d.qkv, d.ldq = _p(qkv), qkv.stride(0)
    d.n_img, d.S, d.C, d.head_dim = n_img, S, x.shape[1], head_dim
    d.q_scale = Q_PRESCALE if q_scale is None else q_scale
    return d


def spatial_entry_fused_serves(x, wf, stats, gn, ln, h0, qkv, n_img, S, **kw):
    return wf is not None and bool(_L(x).ctrlv_spatial_entry_fused_serves(
        ctypes.byref(_spatial_entry_desc(x, wf, stats, gn, ln, h0, qkv, n_img, S, **kw))))


def spatial_entry_fused(x, wf, stats, gn, ln, h0, qkv, n_img, S, **kw):
    """h0 = el(el(GN(x)) W_in^T + bias_in), qkv = el(el(LN(h0)) W_qkv^T + bias_qkv) with the q block scaled by q_scale: the
    opening of the spatial transformer block at C = 320 in one launch (csrc/spatial_entry_fused.hip).  stats: the finalized
    (mean, rstd) table fp32 [n_img, 32, 2] (`groupnorm_stats` / `groupnorm_finalize`); gn = (gamma, beta), ln = (gamma, beta, eps)."""
    d = _spatial_entry_desc(x, wf, stats, gn, ln, h0, qkv, n_img, S, **kw)
    _need_gpu(x, "x")
    assert stats.dtype == torch.float32 and stats.numel() >= n_img * 64
    ev = _prof.begin()
    check(_L(x).ctrlv_spatial_entry_fused(ctypes.byref(d), _stream()), "ctrlv_spatial_entry_fused")
    M, C = n_img * S, x.shape[1]
    _prof.end(ev, "gemm_spatial_entry", 2.0 * M * C * 4 * C, 2.0 * 5 * M * C)
    return h0, qkv


def groupnorm_stats(x, n_img, S, C, imgs_per_stat, eps, partials, x_lo=None):
    """The statistics pass of `groupnorm` alone (with its finalize); returns the (mean, rstd) table behind the chunk partials,
    fp32 [n_img / imgs_per_stat, 32, 2] (a view of `partials`)."""
    _need_dense("groupnorm_stats", x=x, x_lo=x_lo, partials=partials)
    _need_gpu(x, "x")
    ev = _prof.begin()
    check(_L(x).ctrlv_groupnorm_stats_split(_p(x), _p(x_lo), None, None, 0, n_img, S, C, imgs_per_stat, eps, _p(partials),
                                            _stream()), "ctrlv_groupnorm_stats")
    _prof.end(ev, "groupnorm", 0.0, 2.0 * n_img * S * C)           # algorithmic: 1 read
    off = n_img * groupnorm_chunks(n_img, S, C, imgs_per_stat) * 64
    return partials.view(-1)[off:off + (n_img // imgs_per_stat) * 64]


def groupnorm_apply(x, n_img, S, C, imgs_per_stat, gamma, beta, silu, y, partials, x_lo=None):
    """The apply pass of `groupnorm` alone, on the statistics `groupnorm_stats` left in `partials`."""
    _need_dense("groupnorm_apply", x=x, x_lo=x_lo, y=y, partials=partials, gamma=gamma, beta=beta)
    _need_gpu(x, "x")
    ev = _prof.begin()
    check(_L(x).ctrlv_groupnorm_apply_split(_p(x), _p(x_lo), None, None, 0, n_img, S, C, imgs_per_stat, _p(partials), _p(gamma),
                                            _p(beta), 1 if silu else 0, _p(y), _stream()), "ctrlv_groupnorm_apply")
    _prof.end(ev, "groupnorm", 0.0, 2.0 * 2 * n_img * S * C)
    return y


def groupnorm_finalize(x, n_img, S, C, imgs_per_stat, eps, partials):
    """The finalize step of `groupnorm_from_partials` alone; returns the (mean, rstd) table behind the producer's partials.
    x: the normalised tensor (selects the element library only)."""
    _need_dense("groupnorm_finalize", partials=partials)
    _need_gpu(partials, "partials")
    assert partials.numel() >= groupnorm_fused_scratch_floats(n_img, S, imgs_per_stat)
    ev = _prof.begin()
    check(_L(x).ctrlv_groupnorm_finalize(n_img, S, C, imgs_per_stat, eps, _p(partials), _stream()), "ctrlv_groupnorm_finalize")
    _prof.end(ev, "groupnorm", 0.0, 0.0)
    off = n_img * (S // 64) * 64
    return partials.view(-1)[off:off + (n_img // imgs_per_stat) * 64]


def nchw_to_rows(src, dst, c_off=0):
    """src: contiguous (n_img, C, H, W) fp32/fp16/bf16 -> dst rows [n_img*H*W, ldc] bf16, channels [c_off, c_off+C)."""
    _need_dense("nchw_to_rows", src=src)
    _need_rows("nchw_to_rows", dst=dst)
    _need_gpu(src, "src")
    n_img, C = src.shape[0], src.shape[1]
    HW = src.shape[2] * src.shape[3]
    check(_L(dst).ctrlv_nchw_to_rows(_p(src), _DT[src.dtype], n_img, C, HW, _p(dst), dst.stride(0), c_off,
                                         _stream()), "ctrlv_nchw_to_rows")
    return dst


def rows_to_nchw(src, dst, C=None):
    """src rows [n_img*H*W, ldc] bf16 -> dst contiguous (n_img, C, H, W) of dst.dtype."""
    _need_rows("rows_to_nchw", src=src)
    _need_dense("rows_to_nchw", dst=dst)
    _need_gpu(src, "src")
    n_img, Cd = dst.shape[0], dst.shape[1]
    HW = dst.shape[2] * dst.shape[3]
    check(_L(src).ctrlv_rows_to_nchw(_p(src), src.stride(0), n_img, Cd if C is None else C, HW, _p(dst),
                                         _DT[dst.dtype], _stream()), "ctrlv_rows_to_nchw")
    return dst


def vae_posterior(rows, n_img, L, HW, quant_weight, quant_bias, noise=None, scale=1.0, moments=None, latents=None):
    """quant_conv + posterior on the encoder's conv_out rows [n_img * HW, ld >= 2 L] (ctrlv_vae_posterior): `moments`
    (n_img, 2 L, H, W) and / or `latents` (n_img, L, H, W), contiguous, of one dtype; `noise` fp32 (n_img, L, H, W) or None
    for the distribution's mode.  quant_weight [2 L, 2 L] / quant_bias [2 L] fp32."""
    _need_gpu(rows, "rows")
    outs = [t for t in (moments, latents) if t is not None]
    if len({t.dtype for t in outs}) > 1:
        raise ValueError("vae_posterior: moments and latents must have one dtype")
    dt = _DT[outs[0].dtype] if outs else 0
    check(_L(rows).ctrlv_vae_posterior(_p(rows), rows.stride(0), n_img, L, HW, _p(quant_weight), _p(quant_bias), _p(noise),
                                       float(scale), _p(moments), _p(latents), dt, _stream()), "ctrlv_vae_posterior")
    return moments, latents


def im2col3x3(x, n_img, H, W, col):
    _need_gpu(x, "x")
    check(_L(x).ctrlv_im2col3x3(_p(x), n_img, H, W, x.shape[1], _p(col), col.shape[1], _stream()),
          "ctrlv_im2col3x3")
    return col


def axpby(x, r, a, b, y):
    _need_gpu(x, "x")
    ev = _prof.begin()
    check(_L(x).ctrlv_axpby(_p(x), _p(r), a, b, _p(y), x.numel(), _stream()), "ctrlv_axpby")
    _prof.end(ev, "residual_add", 0.0, 2.0 * 3 * x.numel())
    return y


def axpby_split(x, x_lo, r, a, b, y, y_lo):
    """(y, y_lo) = split(a * (x + x_lo) + b * r): the residual add on a SPLIT trunk tensor (x_lo may be None)."""
    _need_gpu(x, "x")
    check(_L(x).ctrlv_axpby_split(_p(x), _p(x_lo), _p(r), a, b, _p(y), _p(y_lo), x.numel(), _stream()), "ctrlv_axpby_split")
    return y, y_lo


def silu(x, y):
    _need_gpu(x, "x")
    check(_L(x).ctrlv_silu(_p(x), _p(y), x.numel(), _stream()), "ctrlv_silu")
    return y


def timestep_embedding(t, dim, out):
    """t: fp32 [n] -> out [n, dim] bf16 = [cos | sin] (Timesteps(dim, flip_sin_to_cos=True, shift 0))."""
    _need_gpu(t, "t")
    check(_L(out).ctrlv_timestep_embedding(_p(t), t.numel(), dim, _p(out), _stream()),
          "ctrlv_timestep_embedding")
    return out


def cfg_euler_step(latents, noise_pred, guidance, sigma, sigma_next, scaled_next=None):
    """In-place fused CFG combine + Euler v-prediction update (pipeline_video_control.py:327-332)."""
    _need_gpu(latents, "latents")
    B, F = latents.shape[0], latents.shape[1]
    chw = latents[0, 0].numel()
    cfg = 1 if noise_pred.shape[0] == 2 * B else 0
    check(_L(scaled_next).ctrlv_cfg_euler_step(_p(latents), _p(noise_pred), _DT[noise_pred.dtype], cfg, _p(guidance), B,
                                           F, chw, float(sigma), float(sigma_next), _p(scaled_next), _stream()),
          "ctrlv_cfg_euler_step")
    return latents


def time_conv_rows_to_nchw(rows, n_frames, C, HW, weight, bias, out):
    """Conv3d(C, C, (3,1,1)) over the frames of one clip on channels-last rows, written as NCHW `out` (the VAE decoder's
    time_conv_out)."""
    _need_rows("time_conv_rows_to_nchw", rows=rows)
    _need_dense("time_conv_rows_to_nchw", weight=weight, bias=bias, out=out)
    _need_gpu(rows, "rows")
    check(_L(rows).ctrlv_time_conv_rows_to_nchw(_p(rows), rows.stride(0), n_frames, C, HW, _p(weight), _p(bias), _p(out),
                                                   _DT[out.dtype], _stream()), "ctrlv_time_conv_rows_to_nchw")
    return out


def softmax_rows(scores, probs):
    """probs (bf16) = row softmax of fp32 `scores` (both 2-D, unit inner stride)."""
    _need_rows("softmax_rows", scores=scores, probs=probs)
    _need_gpu(scores, "scores")
    check(_L(probs).ctrlv_softmax_rows(_p(scores), scores.shape[0], scores.shape[1], scores.stride(0), _p(probs),
                                         probs.stride(0), _stream()), "ctrlv_softmax_rows")
    return probs


def softmax_rows_bwd(probs, dprobs, scale, dscores):
    """dscores (element type) = scale * probs o (dprobs - rowsum(probs o dprobs)): the backward of `softmax_rows` for scores
    that carry `scale` (probs: what the forward wrote; dprobs fp32; all 2-D with unit inner stride)."""
    _need_gpu(probs, "probs")
    if dprobs.dtype != torch.float32 or probs.shape != dprobs.shape or probs.shape != dscores.shape:
        raise ValueError("softmax_rows_bwd: probs / dscores in the element type and fp32 dprobs of one shape")
    check(_L(probs, dscores).ctrlv_softmax_rows_bwd(_p(probs), probs.stride(0), _p(dprobs), dprobs.stride(0), probs.shape[0],
                                                    probs.shape[1], float(scale), _p(dscores), dscores.stride(0), _stream()),
          "ctrlv_softmax_rows_bwd")
    return dscores


TIME_CONV_BWD_SCRATCH_FLOATS = 16384       # CTRLV_TIME_CONV_BWD_SCRATCH_FLOATS of include/ctrlv_hip.h


def time_conv_rows_to_nchw_bwd(dout, rows, n_frames, clip_frames, C, HW, weight, drows, dweight, dbias):
    """Backward of `time_conv_rows_to_nchw` over whole clips of `clip_frames`: dout fp32 (n_frames, C, H, W), rows / weight the
    forward's operands -> drows [n_frames * HW, ldc] (element type, every column written), dweight fp32 [C, C, 3], dbias
    fp32 [C]; ordered sums (bit-reproducible)."""
    _need_gpu(rows, "rows")
    if dout.dtype != torch.float32 or not dout.is_contiguous():
        raise ValueError("time_conv_rows_to_nchw_bwd: dout must be contiguous fp32 NCHW")
    scratch = _scratch(rows.device, TIME_CONV_BWD_SCRATCH_FLOATS * 4, "time_conv_bwd", floor=TIME_CONV_BWD_SCRATCH_FLOATS * 4)
    check(_L(rows, drows).ctrlv_time_conv_rows_to_nchw_bwd(_p(dout), _p(rows), rows.stride(0), n_frames, clip_frames, C, HW,
                                                           _p(weight), _p(drows), drows.stride(0), _p(dweight), _p(dbias),
                                                           _p(scratch), _stream()), "ctrlv_time_conv_rows_to_nchw_bwd")
    return drows


def resize_antialias(image, size, mean=None, std=None, out_dtype=torch.float32, clamp=False):
    """`_resize_with_antialiasing(image, size)` (Gaussian pre-blur + bicubic, align_corners) as one kernel
    (ctrlv_resize_antialias).  image: (n, H, W, 3) uint8 -- read as (v / 255) * 2 - 1 -- or (n, 3, H, W) fp32.  mean / std
    (three floats each): the epilogue ((y + 1) / 2 - mean) / std.  clamp=True (ctrlv_resize_antialias_clamped; needs mean / std):
    (y + 1) / 2 is limited to [0, 1] first, as the training loops' encode_video_image does.  Returns (n, 3, h, w) in fp32 or in
    an element type (the fp32 value rounded once)."""
    _need_gpu(image, "image")
    u8 = image.dtype == torch.uint8
    if image.dim() != 4 or (image.shape[3] if u8 else image.shape[1]) != 3 or (not u8 and image.dtype != torch.float32):
        raise ValueError("resize_antialias: image must be (n, H, W, 3) uint8 or (n, 3, H, W) fp32")
    if (mean is None) != (std is None):
        raise ValueError("resize_antialias: mean and std come together")
    if clamp and mean is None:
        raise ValueError("resize_antialias: clamp=True belongs to the normalising epilogue (give mean and std)")
    image = image.contiguous()
    n = image.shape[0]
    H, W = (image.shape[1], image.shape[2]) if u8 else (image.shape[2], image.shape[3])
    out = torch.empty(n, 3, int(size[0]), int(size[1]), dtype=out_dtype, device=image.device)
    f3 = ctypes.c_float * 3
    m = f3(*[float(v) for v in mean]) if mean is not None else None
    sd = f3(*[float(v) for v in std]) if std is not None else None
    symbol = "ctrlv_resize_antialias_clamped" if clamp else "ctrlv_resize_antialias"
    check(getattr(_L(out), symbol)(_p(image), 1 if u8 else 0, n, H, W, _p(out), _DT[out_dtype], int(size[0]), int(size[1]), m, sd,
                                   _stream()), symbol)
    return out


def pixels_prepare(image_u8, noise=None, strength=0.0, dtype=torch.bfloat16):
    """(n, H, W, 3) uint8 -> (n, 3, H, W) of the element type `dtype`: 2 * (v / 255) - 1 + strength * noise, noise fp32
    (n, 3, H, W) or None (ctrlv_pixels_prepare): VaeImageProcessor.preprocess + the noise augmentation + the cast."""
    _need_gpu(image_u8, "image_u8")
    if image_u8.dtype != torch.uint8 or image_u8.dim() != 4 or image_u8.shape[3] != 3:
        raise ValueError("pixels_prepare: image_u8 must be (n, H, W, 3) uint8")
    image_u8 = image_u8.contiguous()
    n, H, W, _ = image_u8.shape
    if noise is not None:
        if noise.dtype != torch.float32 or tuple(noise.shape) != (n, 3, H, W) or noise.device != image_u8.device:
            raise ValueError(f"pixels_prepare: noise must be fp32 {(n, 3, H, W)} on the image's device")
        noise = noise.contiguous()
    out = torch.empty(n, 3, H, W, dtype=dtype, device=image_u8.device)
    check(_L(out).ctrlv_pixels_prepare(_p(image_u8), _p(noise), float(strength), n, H, W, _p(out), _stream()),
          "ctrlv_pixels_prepare")
    return out


def frames_to_u8(frames):
    """(m, 3, H, W) element frames in [-1, 1] -> (m, H, W, 3) uint8: rint(clamp(x / 2 + 0.5, 0, 1) * 255)
    (ctrlv_frames_to_u8): VaeImageProcessor.postprocess + numpy_to_pil's rounding."""
    _need_gpu(frames, "frames")
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("frames_to_u8: frames must be (m, 3, H, W) fp16 / bf16")
    frames = frames.contiguous()
    m, _, H, W = frames.shape
    out = torch.empty(m, H, W, 3, dtype=torch.uint8, device=frames.device)
    check(_L(frames).ctrlv_frames_to_u8(_p(frames), m, H, W, _p(out), _stream()), "ctrlv_frames_to_u8")
    return out


def _out_arg(arg, shape, dtype, device, fn, name):
    """True: a fresh tensor; a tensor: that one (dense, of the shape and type); None / False: not asked for."""
    if arg is None or arg is False:
        return None
    if arg is True:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(arg.shape) != tuple(shape) or arg.dtype != dtype or arg.device != device:
        raise ValueError(f"{fn}: {name} must be {tuple(shape)} {dtype} on {device}")
    _need_dense(fn, **{name: arg})
    return arg


def box_frames_post(frames, num_frames, threshold=50.0, pt=True, cond=True, u8=True):
    """Decoded box frames (n F, 3, H, W) fp16 / bf16 -> (pt, cond, u8) (ctrlv_box_frames_post), each None unless asked for
    (True, or a dense tensor to write into): pt = clamp(x / 2 + 0.5, 0, 1) and cond = 2 * (pt - 0.5), (n F, 3, H, W) in the
    element type, every operation rounded; u8 (n, F, 3, H, W) uint8 = the cleaned frames of eval_overall.py:96-105 -- pixels
    with channel sum < threshold and interior frames without such a pixel zeroed, the rest truncated.  No host sync."""
    fn = "box_frames_post"
    _need_gpu(frames, "frames")
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{fn}: frames must be (n F, 3, H, W) fp16 / bf16")
    F = int(num_frames)
    m, _, H, W = frames.shape
    if F < 1 or m % F:
        raise ValueError(f"{fn}: {m} frames are not clips of {F}")
    _need_dense(fn, frames=frames)
    n, dev = m // F, frames.device
    pt = _out_arg(pt, (m, 3, H, W), frames.dtype, dev, fn, "pt")
    cond = _out_arg(cond, (m, 3, H, W), frames.dtype, dev, fn, "cond")
    u8 = _out_arg(u8, (n, F, 3, H, W), torch.uint8, dev, fn, "u8")
    lib = _L(frames)
    ws = torch.empty(lib.ctrlv_box_frames_post_ws_bytes(n, F), dtype=torch.uint8, device=dev) if u8 is not None else None
    check(lib.ctrlv_box_frames_post(_p(frames), n, F, H, W, float(threshold), _p(pt), _p(cond), _p(u8), _p(ws),
                                    ws.numel() if ws is not None else 0, _stream()), "ctrlv_box_frames_post")
    return pt, cond, u8


def mask_counts(gt_u8, pred_u8, out=None):
    """gt_u8, pred_u8 (n, F, 3, H, W) uint8 -> int64 (n, 2, 3) on the device (ctrlv_mask_counts): per clip {gt area, pred
    area, intersection} of the any-channel-nonzero masks, over all frames and over the frames {0, F - 1}."""
    fn = "mask_counts"
    _need_gpu(gt_u8, "gt_u8")
    if gt_u8.dim() != 5 or gt_u8.shape[2] != 3 or gt_u8.dtype != torch.uint8:
        raise ValueError(f"{fn}: gt_u8 must be (n, F, 3, H, W) uint8")
    if tuple(pred_u8.shape) != tuple(gt_u8.shape) or pred_u8.dtype != torch.uint8 or pred_u8.device != gt_u8.device:
        raise ValueError(f"{fn}: pred_u8 must be uint8 {tuple(gt_u8.shape)} on {gt_u8.device}")
    _need_dense(fn, gt_u8=gt_u8, pred_u8=pred_u8)
    n, F, _, H, W = gt_u8.shape
    out = _out_arg(True if out is None else out, (n, 2, 3), torch.int64, gt_u8.device, fn, "out")
    check(_lib.load().ctrlv_mask_counts(_p(gt_u8), _p(pred_u8), n, F, H, W, _p(out), _stream()), "ctrlv_mask_counts")
    return out


def best_candidate(counts, out=None):
    """counts int64 (C, n, 2, 3) on the device, block c what `mask_counts` gives for candidate c -> int32 (n): per clip the
    candidate with the largest all-frames IoU, a tie to the highest c (ctrlv_best_candidate; metrics.best_of restates it)."""
    fn = "best_candidate"
    _need_gpu(counts, "counts")
    if counts.dim() != 4 or tuple(counts.shape[2:]) != (2, 3) or counts.dtype != torch.int64:
        raise ValueError(f"{fn}: counts must be int64 (C, n, 2, 3)")
    _need_dense(fn, counts=counts)
    C, n = counts.shape[:2]
    out = _out_arg(True if out is None else out, (n,), torch.int32, counts.device, fn, "out")
    check(_lib.load().ctrlv_best_candidate(_p(counts), n, C, _p(out), _stream()), "ctrlv_best_candidate")
    return out


def gather_clips(src, winner, out=None):
    """src (C, n, ...) of any dtype, winner int32 (n) on the device -> (n, ...): out[i] = src[winner[i]][i], the index read on
    the device and clamped into [0, C) (ctrlv_gather_clips).  No host sync."""
    fn = "gather_clips"
    _need_gpu(src, "src")
    if src.dim() < 2:
        raise ValueError(f"{fn}: src must be (C, n, ...)")
    C, n = src.shape[:2]
    if winner.dtype != torch.int32 or tuple(winner.shape) != (n,) or winner.device != src.device:
        raise ValueError(f"{fn}: winner must be int32 ({n},) on {src.device}")
    _need_dense(fn, src=src, winner=winner)
    out = _out_arg(True if out is None else out, tuple(src.shape[1:]), src.dtype, src.device, fn, "out")
    per = src[0, 0].numel() * src.element_size()
    check(_lib.load().ctrlv_gather_clips(_p(src), _p(winner), n, C, per, _p(out), _stream()), "ctrlv_gather_clips")
    return out


def boundary_counts(gt_u8, pred_u8, radius, mask_mode=1, out=None):
    """gt_u8, pred_u8 (n, F, 3, H, W) uint8 -> int64 (n, F, 4) on the device (ctrlv_boundary_counts): per frame {n_fg, n_gt,
    fg_match, gt_match} of f_measure -- the boundary pixels of the predicted and the ground-truth mask and how many of each lie
    within `radius` pixels (a disk) of the other's.  mask_mode 0: any channel nonzero; 1: PIL's luma != 0."""
    fn = "boundary_counts"
    _need_gpu(gt_u8, "gt_u8")
    if gt_u8.dim() != 5 or gt_u8.shape[2] != 3 or gt_u8.dtype != torch.uint8:
        raise ValueError(f"{fn}: gt_u8 must be (n, F, 3, H, W) uint8")
    if tuple(pred_u8.shape) != tuple(gt_u8.shape) or pred_u8.dtype != torch.uint8 or pred_u8.device != gt_u8.device:
        raise ValueError(f"{fn}: pred_u8 must be uint8 {tuple(gt_u8.shape)} on {gt_u8.device}")
    _need_dense(fn, gt_u8=gt_u8, pred_u8=pred_u8)
    n, F, _, H, W = gt_u8.shape
    out = _out_arg(True if out is None else out, (n, F, 4), torch.int64, gt_u8.device, fn, "out")
    check(_lib.load().ctrlv_boundary_counts(_p(gt_u8), _p(pred_u8), n, F, H, W, int(mask_mode), int(radius), _p(out), _stream()),
          "ctrlv_boundary_counts")
    return out


def randn(seed, shape, *, clip0=0, call=0, stream_id=0, scale=1.0, round_el=False, dtype=torch.float32, el=None, device=None,
          out=None):
    """Counter-based Gaussian noise (ctrlv_randn): shape (n_clips, ...) -- element e of row i is a pure function of (seed,
    clip0 + i, call, stream_id, e): Philox4x32-10, fp32 uniforms, Box-Muller.  dtype: fp32 or an element type (bf16 / fp16).
    round_el=False: scale * z in fp32; round_el=True: rne_el(rne_el(z) * scale) in the element type `el` (default: dtype when it
    is an element type, else bf16) -- torch's element-typed randn times a Python scalar.  `out`: a dense tensor of the shape and
    dtype to write into (any element alignment), else a fresh one on `device` (default: the current HIP device)."""
    shape = tuple(int(v) for v in shape)
    if len(shape) < 1 or any(v < 1 for v in shape):
        raise ValueError(f"randn: shape {shape} must have positive sizes, clips first")
    if dtype not in _DT:
        raise ValueError(f"randn: dtype {dtype} (fp32, fp16 or bf16)")
    if el is None:
        el = dtype if dtype != torch.float32 else torch.bfloat16
    if dtype != torch.float32 and el != dtype:
        raise ValueError(f"randn: an output in {dtype} comes from the library of that element type, not {el}")
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    elif tuple(out.shape) != shape or out.dtype != dtype:
        raise ValueError(f"randn: out must be {shape} {dtype}")
    _need_gpu(out, "out")
    _need_dense("randn", out=out)
    per = 1
    for v in shape[1:]:
        per *= v
    check(_lib.load(el).ctrlv_randn(int(seed) & 0xFFFFFFFFFFFFFFFF, int(clip0), int(call), int(stream_id), shape[0], per,
                                    float(scale), 1 if round_el else 0, _p(out), _DT[dtype], _stream()), "ctrlv_randn")
    return out


def train_draws(seed, n_clips, sigma_table, timestep_table, *, clip0=0, call=0, dropout_prob=None, el=None):
    """The per-clip draws of a training step (ctrlv_train_draws): one Philox block per clip, keyed on (seed, clip0 + i, call).
    sigma_table / timestep_table: fp32 [T] on the device (EulerDiscreteScheduler().sigmas[:T] and .timesteps).  Returns a dict
    of device tensors of n_clips entries: indices (int32), sigmas, timesteps, random_p, prompt_keep, image_mask (fp32; the masks
    are 0 or 1, all ones for dropout_prob=None).  el: the element type whose library runs it (both export it; default bf16).  No
    host sync."""
    fn = "train_draws"
    _need_gpu(sigma_table, "sigma_table")
    T = sigma_table.numel()
    for name, t in (("sigma_table", sigma_table), ("timestep_table", timestep_table)):
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != T or t.device != sigma_table.device:
            raise ValueError(f"{fn}: {name} must be fp32 ({T},) on {sigma_table.device}")
    _need_dense(fn, sigma_table=sigma_table, timestep_table=timestep_table)
    n, dev = int(n_clips), sigma_table.device
    out = {k: torch.empty(max(n, 0), dtype=torch.int32 if k == "indices" else torch.float32, device=dev)
           for k in ("indices", "sigmas", "timesteps", "random_p", "prompt_keep", "image_mask")}
    check(_lib.load(el).ctrlv_train_draws(int(seed) & 0xFFFFFFFFFFFFFFFF, int(clip0), int(call), n, _p(sigma_table),
                                          _p(timestep_table), T, -1.0 if dropout_prob is None else float(dropout_prob),
                                          *[_p(t) for t in out.values()], _stream()), "ctrlv_train_draws")
    return out


def train_assemble(target, sigmas, cond_image, *, noise=None, image_mask=None, cond_frames=None, layout=0, num_cond_frames=0,
                   seed=0, clip0=0, call=0, sample_dtype=torch.bfloat16, return_noise=False, el=None):
    """One pass over the latents of a batch (ctrlv_train_assemble).  target fp32 (n, F, L, h, w): the clean, scaled latents;
    noise the same, or None: drawn in the kernel as `randn(seed, target.shape, clip0=, call=, stream_id=3)`; sigmas, image_mask
    fp32 (n); cond_image fp32 (n, L, h, w); cond_frames fp32 like target (layout 1: frames [0, num_cond_frames) and F - 1 of the
    conditioning channels come from it).  Returns (noisy fp32, sample (n, F, 2 L, h, w) of sample_dtype -- fp32 or an element
    type --, noise_out or None): noisy = target + noise * sigma, sample = [noisy / sqrt(sigma^2 + 1) | image_mask * c], every
    operation rounded on its own.  el: the library that serves an fp32 sample (default bf16's).  Tensors are taken as they are (any
    element alignment); no host sync."""
    fn = "train_assemble"
    _need_gpu(target, "target")
    if target.dim() != 5 or target.dtype != torch.float32:
        raise ValueError(f"{fn}: target must be fp32 (n, F, L, h, w)")
    n, F, L, h, w = target.shape
    dev = target.device
    for name, t, shape in (("noise", noise, (n, F, L, h, w)), ("sigmas", sigmas, (n,)), ("image_mask", image_mask, (n,)),
                           ("cond_frames", cond_frames, (n, F, L, h, w)), ("cond_image", cond_image, (n, L, h, w))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != dev):
            raise ValueError(f"{fn}: {name} must be fp32 {shape} on {dev}")
    if sample_dtype not in _DT:
        raise ValueError(f"{fn}: sample_dtype {sample_dtype} (fp32, fp16 or bf16)")
    _need_dense(fn, target=target, noise=noise, sigmas=sigmas, image_mask=image_mask, cond_frames=cond_frames, cond_image=cond_image)
    noisy = torch.empty_like(target)
    sample = torch.empty(n, F, 2 * L, h, w, dtype=sample_dtype, device=dev)
    noise_out = torch.empty_like(target) if return_noise else None
    lib = _lib.load(el) if sample_dtype == torch.float32 else _L(sample)
    check(lib.ctrlv_train_assemble(_p(target), _p(noise), _p(sigmas), _p(image_mask), _p(cond_frames), _p(cond_image), int(layout),
                                   int(num_cond_frames), n, F, L, h, w, int(seed) & 0xFFFFFFFFFFFFFFFF, int(clip0), int(call),
                                   _p(noisy), _p(sample), _DT[sample_dtype], _p(noise_out), _stream()), "ctrlv_train_assemble")
    return noisy, sample, noise_out


def resize_lanczos_u8(image_u8, h, w, out=None, workspace=None):
    """(n, H, W, 3) uint8 -> (n, h, w, 3) uint8 = PIL.Image.resize((w, h), resample=LANCZOS) of every image, byte for byte
    (ctrlv_resize_lanczos_u8: integer arithmetic on weight tables built on the host).  out / workspace: dense uint8 tensors to
    use (the workspace 16-byte aligned, at least ctrlv_resize_lanczos_ws_bytes long), else fresh ones."""
    _need_gpu(image_u8, "image_u8")
    if image_u8.dtype != torch.uint8 or image_u8.dim() != 4 or image_u8.shape[3] != 3:
        raise ValueError("resize_lanczos_u8: image_u8 must be (n, H, W, 3) uint8")
    image_u8 = image_u8.contiguous()
    n, H, W, _ = image_u8.shape
    lib = _lib.load()
    need = lib.ctrlv_resize_lanczos_ws_bytes(n, H, W, int(h), int(w))
    if need == 0:
        check(-2, "ctrlv_resize_lanczos_ws_bytes", lib=lib)
    ws = torch.empty(need, dtype=torch.uint8, device=image_u8.device) if workspace is None else workspace
    out = _out_arg(True if out is None else out, (n, int(h), int(w), 3), torch.uint8, image_u8.device, "resize_lanczos_u8", "out")
    _need_dense("resize_lanczos_u8", workspace=ws)
    check(lib.ctrlv_resize_lanczos_u8(_p(image_u8), n, H, W, _p(out), int(h), int(w), _p(ws), ws.numel(), _stream()),
          "ctrlv_resize_lanczos_u8")
    return out


def _frame_pair(fn, gt_u8, gen_u8):
    _need_gpu(gt_u8, "gt_u8")
    if gt_u8.dim() != 5 or gt_u8.shape[2] != 3 or gt_u8.dtype != torch.uint8:
        raise ValueError(f"{fn}: gt_u8 must be (n, F, 3, H, W) uint8")
    if tuple(gen_u8.shape) != tuple(gt_u8.shape) or gen_u8.dtype != torch.uint8 or gen_u8.device != gt_u8.device:
        raise ValueError(f"{fn}: gen_u8 must be uint8 {tuple(gt_u8.shape)} on {gt_u8.device}")
    _need_dense(fn, gt_u8=gt_u8, gen_u8=gen_u8)
    n, F, _, H, W = gt_u8.shape
    return n, F, H, W


def frame_stats(gt_u8, gen_u8, out=None):
    """gt_u8, gen_u8 (n, F, 3, H, W) uint8 -> int64 (n, F, 3) on the device (ctrlv_frame_stats): per frame {min byte, max byte,
    sum of (gt - gen)^2} over the three channels of both frames -- the integers of PSNR (metrics.psnr_from_stats) and the value
    range `frame_ssim` scales by.  Exact; no host sync."""
    fn = "frame_stats"
    n, F, H, W = _frame_pair(fn, gt_u8, gen_u8)
    out = _out_arg(True if out is None else out, (n, F, 3), torch.int64, gt_u8.device, fn, "out")
    check(_lib.load().ctrlv_frame_stats(_p(gt_u8), _p(gen_u8), n, F, H, W, _p(out), _stream()), "ctrlv_frame_stats")
    return out


def frame_ssim(gt_u8, gen_u8, stats=None, out=None, workspace=None):
    """gt_u8, gen_u8 (n, F, 3, H, W) uint8 -> float64 (n, F) on the device (ctrlv_frame_ssim): scikit-image's
    structural_similarity(channel_axis=0, data_range=R, gaussian_weights=True, sigma=1.5) of every frame, R the joint value range
    of the two frames.  stats: what `frame_stats` gave for these frames (computed here when None).  out / workspace: dense
    tensors to use (the workspace uint8, 8-byte aligned, at least ctrlv_frame_ssim_ws_bytes long), else fresh ones.  A frame pair
    of one constant value is NaN.  No host sync."""
    fn = "frame_ssim"
    n, F, H, W = _frame_pair(fn, gt_u8, gen_u8)
    dev = gt_u8.device
    if stats is None:
        stats = frame_stats(gt_u8, gen_u8)
    elif tuple(stats.shape) != (n, F, 3) or stats.dtype != torch.int64 or stats.device != dev:
        raise ValueError(f"{fn}: stats must be int64 {(n, F, 3)} on {dev}")
    _need_dense(fn, stats=stats)
    lib = _lib.load()
    need = lib.ctrlv_frame_ssim_ws_bytes(n, F, H, W)
    if need == 0:
        check(-2, "ctrlv_frame_ssim_ws_bytes", lib=lib)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if workspace is None else workspace
    _need_dense(fn, workspace=ws)
    out = _out_arg(True if out is None else out, (n, F), torch.float64, dev, fn, "out")
    check(lib.ctrlv_frame_ssim(_p(gt_u8), _p(gen_u8), n, F, H, W, _p(stats), _p(out), _p(ws), ws.numel() * ws.element_size(),
                               _stream()), "ctrlv_frame_ssim")
    return out


RESAMPLE = {"lanczos": 1, "bilinear": 2, "bicubic": 3}       # PIL's Image.Resampling codes


def resize_frames_u8(frames_u8, h, w, resample="bicubic", out=None, workspace=None):
    """(..., H, W) uint8 planes -> (..., h, w) uint8 = PIL.Image.resize((w, h), resample=...) of every plane, byte for byte
    (ctrlv_resize_frames_u8); on (n, F, 3, H, W) frames that is PIL's resize of every RGB frame.  resample: "bicubic", "bilinear",
    "lanczos" or PIL's integer code.  out / workspace: dense uint8 tensors to use (the workspace 16-byte aligned, at least
    ctrlv_resize_frames_ws_bytes long), else fresh ones."""
    fn = "resize_frames_u8"
    _need_gpu(frames_u8, "frames_u8")
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() < 2:
        raise ValueError(f"{fn}: frames_u8 must be (..., H, W) uint8")
    code = RESAMPLE.get(resample, resample) if isinstance(resample, str) else int(resample)
    if not isinstance(code, int):
        raise ValueError(f"{fn}: resample {resample!r} must be one of {sorted(RESAMPLE)} or PIL's integer code")
    frames_u8 = frames_u8.contiguous()
    lead, (H, W) = tuple(frames_u8.shape[:-2]), frames_u8.shape[-2:]
    planes = 1
    for v in lead:
        planes *= v
    lib = _lib.load()
    need = lib.ctrlv_resize_frames_ws_bytes(planes, H, W, int(h), int(w), code)
    if need == 0:
        check(-2, "ctrlv_resize_frames_ws_bytes", lib=lib)
    ws = torch.empty(need, dtype=torch.uint8, device=frames_u8.device) if workspace is None else workspace
    _need_dense(fn, workspace=ws)
    out = _out_arg(True if out is None else out, lead + (int(h), int(w)), torch.uint8, frames_u8.device, fn, "out")
    check(lib.ctrlv_resize_frames_u8(_p(frames_u8), planes, H, W, _p(out), int(h), int(w), code, _p(ws), ws.numel(), _stream()),
          "ctrlv_resize_frames_u8")
    return out


# ---- box and trajectory frames from coordinates (csrc/box_render.hip)
def _box_table(fn, table):
    for name, t in (("objects", table.objects), ("frames", table.frames)):
        _need_gpu(t, f"table.{name}")
        _need_dense(fn, **{name: t})
    if table.frames.device != table.objects.device:
        raise ValueError(f"{fn}: the two tables live on {table.objects.device} and {table.frames.device}")
    return table.n_objects, table.n_frames, (table.n_clips, table.num_frames)


def render_box_frames(table, source_size, out=None):
    """A `ctrlv_amd.boxes.BoxTable` on the device -> (n, F, 3, Hs, Ws) uint8 box / trajectory frames at source_size = (Hs, Ws)
    (ctrlv_render_box_frames: the integer geometry of include/ctrlv_hip.h, not OpenCV's raster)."""
    fn = "render_box_frames"
    n_obj, n_fr, lead = _box_table(fn, table)
    Hs, Ws = int(source_size[0]), int(source_size[1])
    lib = _lib.load()
    out = _out_arg(True if out is None else out, lead + (3, Hs, Ws), torch.uint8, table.device, fn, "out")
    with torch.cuda.device(table.device):
        check(lib.ctrlv_render_box_frames(_p(table.objects), n_obj, _p(table.frames), n_fr, Hs, Ws, _p(out), _stream()),
              "ctrlv_render_box_frames")
    return out


def box_frames_cond(table, source_size, size, dtype=torch.bfloat16, out=None, return_u8=False, workspace=None):
    """A `BoxTable` -> the ControlNet's condition (n, F, 3, H, W) at size = (H, W) in `dtype` (fp32, or bf16 / fp16: the library of
    that element type): the frames rendered at source_size, PIL's BILINEAR resize, (v / 255 - 0.5) / 0.5 (ctrlv_box_frames_cond).
    return_u8: also the rendered (n, F, 3, Hs, Ws) uint8 frames."""
    fn = "box_frames_cond"
    n_obj, n_fr, lead = _box_table(fn, table)
    (Hs, Ws), (H, W) = (int(v) for v in source_size), (int(v) for v in size)
    if dtype not in _DT:
        raise ValueError(f"{fn}: dtype {dtype} must be fp32, fp16 or bf16")
    lib = _lib.load(None if dtype == torch.float32 else dtype)
    need = lib.ctrlv_box_frames_cond_ws_bytes(n_fr, Hs, Ws, H, W)
    if need == 0:
        check(-2, "ctrlv_box_frames_cond_ws_bytes", lib=lib)
    dev = table.device
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if workspace is None else workspace
    _need_dense(fn, workspace=ws)
    out = _out_arg(True if out is None else out, lead + (3, H, W), dtype, dev, fn, "out")
    u8 = torch.empty(lead + (3, Hs, Ws), dtype=torch.uint8, device=dev) if return_u8 else None
    with torch.cuda.device(dev):
        check(lib.ctrlv_box_frames_cond(_p(table.objects), n_obj, _p(table.frames), n_fr, Hs, Ws, H, W, _p(out), _DT[dtype], _p(u8),
                                        _p(ws), ws.numel(), _stream()), "ctrlv_box_frames_cond")
    return (out, u8) if return_u8 else out


# ---- LPIPS (csrc/lpips.hip): the split-operand im2col, the pool on fp32 rows and the per-layer distance
LPIPS_SRC = {torch.float32: 0, torch.uint8: 3}       # src_dtype codes of the first-layer im2col and of ctrlv_lpips_frames


def lpips_kp(C, k):
    """Columns of one block of a split im2col row: k k C rounded up to a multiple of 64."""
    return (k * k * C + 63) // 64 * 64


def lpips_im2col_split(src, k=11, hw=None, dtype=torch.bfloat16, out=None):
    """The A operand of one LPIPS convolution as element rows [M, 3 Kp] = lo | hi | hi (ctrlv_lpips_im2col_split), hi = rne(x),
    lo = rne(x - hi) in the element type `dtype`.
    src (m, 3, H, W) uint8 or fp32 in [-1, 1], k = 11: the first layer -- the scaling layer in fp32, 11 x 11 windows of stride 4
    and padding 2, columns (c, ky, kx); M = m Ho Wo.
    src fp32 rows [m H W, C] (unit column stride) with hw = (m, H, W), k = 3 or 5: a later layer -- max(v, 0) on read, stride 1,
    padding (k - 1) / 2, columns (ky, kx, c); M = m H W."""
    fn = "lpips_im2col_split"
    _need_gpu(src, "src")
    lib = _lib.load(dtype)
    if src.dim() == 4:
        if src.shape[1] != 3 or src.dtype not in LPIPS_SRC or k != 11:
            raise ValueError(f"{fn}: the first layer takes (m, 3, H, W) uint8 / fp32 frames and k = 11")
        _need_dense(fn, src=src)
        m, C, H, W = src.shape
        if H < 7 or W < 7:
            raise ValueError(f"{fn}: a {H} x {W} frame is smaller than the window")
        M, form, code, ld = m * ((H - 7) // 4 + 1) * ((W - 7) // 4 + 1), 0, LPIPS_SRC[src.dtype], 0
    else:
        if src.dim() != 2 or src.dtype != torch.float32 or hw is None:
            raise ValueError(f"{fn}: later layers take fp32 rows [m H W, C] and hw = (m, H, W)")
        _need_rows(fn, src=src)
        m, H, W = (int(v) for v in hw)
        C, ld = src.shape[1], src.stride(0)
        if src.shape[0] != m * H * W:
            raise ValueError(f"{fn}: {src.shape[0]} rows are not {m} x {H} x {W} pixels")
        M, form, code = m * H * W, 1, 0
    out = _out_arg(True if out is None else out, (M, 3 * lpips_kp(C, k)), dtype, src.device, fn, "out")
    check(lib.ctrlv_lpips_im2col_split(_p(src), form, code, m, H, W, C, ld, int(k), _p(out), _stream()), "ctrlv_lpips_im2col_split")
    return out


def lpips_pack_weight(weight, order, dtype=torch.bfloat16):
    """A convolution's parameter (N, C, k, k) -> element rows [N, 3 Kp] = whi | wlo | whi in the column order of the matching
    im2col: order 0 (c, ky, kx), 1 (ky, kx, c) (ctrlv_lpips_pack_weight)."""
    w = weight.detach().contiguous()
    _need_gpu(w, "weight")
    if w.dim() != 4 or w.shape[2] != w.shape[3] or w.dtype not in _DT:
        raise ValueError(f"lpips_pack_weight: expected a float (N, C, k, k) parameter, got {tuple(w.shape)} {w.dtype}")
    N, C, k, _ = w.shape
    dst = torch.empty(N, 3 * lpips_kp(C, k), dtype=dtype, device=w.device)
    check(_lib.load(dtype).ctrlv_lpips_pack_weight(_p(w), _DT[w.dtype], N, C, k, int(order), _p(dst), _stream()),
          "ctrlv_lpips_pack_weight")
    return dst


def relu_maxpool_rows(x, hw, out=None):
    """fp32 rows [m H W, C] with hw = (m, H, W) -> fp32 rows [m Ho Wo, C] = max_pool2d(relu(x), 3, stride 2), floor mode, no
    padding (ctrlv_relu_maxpool_rows); exact."""
    fn = "relu_maxpool_rows"
    _need_gpu(x, "x")
    m, H, W = (int(v) for v in hw)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] != m * H * W:
        raise ValueError(f"{fn}: x must be fp32 rows [{m} x {H} x {W}, C], got {tuple(x.shape)} {x.dtype}")
    _need_rows(fn, x=x)
    if H < 3 or W < 3:
        raise ValueError(f"{fn}: a {H} x {W} image holds no 3 x 3 window")
    C = x.shape[1]
    out = _out_arg(True if out is None else out, (m * ((H - 3) // 2 + 1) * ((W - 3) // 2 + 1), C), torch.float32, x.device, fn, "out")
    check(_lib.load().ctrlv_relu_maxpool_rows(_p(x), m, H, W, C, x.stride(0), _p(out), out.stride(0), _stream()),
          "ctrlv_relu_maxpool_rows")
    return out


def lpips_layer_distance(gt, gen, lin, frames):
    """gt, gen fp32 rows [frames pix, C] of one layer (pre-ReLU), lin fp32 [C] -> float64 [frames, ceil(pix / 64)] per-block partial
    sums of d = sum_c lin[c] (n_gt - n_gen)^2 over a frame's pixels, n = relu(x) / (|relu(x)|_2 + 1e-10)
    (ctrlv_lpips_layer_distance).  `lpips_finish` adds them."""
    fn = "lpips_layer_distance"
    _need_gpu(gt, "gt")
    frames = int(frames)
    if (gt.dim() != 2 or gt.dtype != torch.float32 or gen.dtype != torch.float32 or tuple(gen.shape) != tuple(gt.shape)
            or gen.stride(0) != gt.stride(0) or frames < 1 or gt.shape[0] % frames):
        raise ValueError(f"{fn}: gt and gen must be fp32 rows of one shape and pitch, a whole number of pixels per frame")
    _need_rows(fn, gt=gt, gen=gen)
    C, pix = gt.shape[1], gt.shape[0] // frames
    if lin.dtype != torch.float32 or lin.numel() != C or not lin.is_contiguous():
        raise ValueError(f"{fn}: lin must be dense fp32 [{C}]")
    lib = _lib.load()
    out = torch.empty(frames, lib.ctrlv_lpips_distance_blocks(pix), dtype=torch.float64, device=gt.device)
    check(lib.ctrlv_lpips_layer_distance(_p(gt), _p(gen), gt.stride(0), _p(lin), frames, pix, C, _p(out), _stream()),
          "ctrlv_lpips_layer_distance")
    return out


def lpips_finish(partials, pix):
    """partials: the layers' float64 [frames, blocks] arrays of `lpips_layer_distance`; pix: their pixel counts -> float64 [frames]
    = sum over the layers of (the frame's partials added in block order) / pix (ctrlv_lpips_finish)."""
    frames = partials[0].shape[0]
    flat = torch.cat([p.reshape(-1) for p in partials])
    arr = (ctypes.c_int32 * len(pix))(*[int(v) for v in pix])
    out = torch.empty(frames, dtype=torch.float64, device=flat.device)
    check(_lib.load().ctrlv_lpips_finish(_p(flat), frames, len(pix), arr, _p(out), _stream()), "ctrlv_lpips_finish")
    return out
