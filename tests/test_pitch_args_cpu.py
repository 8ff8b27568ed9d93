"""Host-side tests (no GPU) of the row-pitch rules (include/ctrlv_hip.h, next to the pitch fields of ctrlv_gemm_desc): a pitch
covers its row.  ctrlv_gemm, ctrlv_gemm_f8 and ctrlv_ff_fused refuse a smaller one before anything is launched (the pointers
here are never dereferenced), the boundary value ld == width does not draw the pitch error, and the ops.py wrappers of the
kernels that take no pitch refuse a view that is not contiguous, by the argument's name."""
import ctypes

import pytest
import torch

import __graft_entry__ as g

P = 0x1000          # a non-null, 16-byte aligned address that is never dereferenced (validation fails first)
PITCH_ERR = "row pitch"


def _libs():
    g.build()
    from ctrlv_amd import _lib
    return _lib, (_lib.load(), _lib.load(torch.float16))


def _desc(_lib, **kw):
    """Every pitched operand present: M = 8, N = 64, Cin = 128 (A2 from channel 64 on).  mode = 7 does not exist: a descriptor
    that passes the pitch rules is refused by the mode check behind them (BAD_ARG), so nothing is ever launched."""
    d = _lib.GemmDesc()
    base = dict(A=P, A2=P, W=P, out=P, bias=P, R1=P, R2=P, V=P, M=8, N=64, Cin=128, taps=1, mode=7, lda=64, lda2=64, c_split=64,
                ldo=64, n_store=64, ldr1=64, ldr2=64, ldv=64, vmode=1, vdiv=1, vmod=1, vS=1, s_acc=1.0, s1=1.0, s2=1.0)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


GEMM_RULES = [          # (field, smaller pitch, what else the descriptor says)
    ("lda", 56, {}),                                      # >= c_split with A2
    ("lda", 120, dict(A2=None, c_split=0)),               # >= Cin without
    ("lda2", 56, {}),                                     # >= Cin - c_split
    ("ldo", 56, {}),
    ("ldr1", 56, {}),
    ("ldr2", 56, {}),
    ("ldv", 56, {}),
    ("ldo", 24, dict(n_store=32)),                        # the stored columns are n_store, not N
    ("ldo", 24, dict(geglu=1, R1=None, R2=None, V=None, vmode=0, A2=None, c_split=0, lda=128)),     # GEGLU: min(n_store, N / 2) = 32
]


def test_gemm_refuses_a_pitch_smaller_than_its_row():
    _lib, libs = _libs()
    for lib in libs:
        for field, small, kw in GEMM_RULES:
            d = _desc(_lib, **dict(kw, **{field: small}))
            rc = lib.ctrlv_gemm(ctypes.byref(d), None)
            err = _lib.last_error(lib)
            assert rc == -2 and PITCH_ERR in err and f"{field}={small}" in err, (field, kw, rc, err)
        # the boundary (ld == width) passes every pitch rule: the call gets as far as the (unknown) mode
        for kw in ({}, dict(A2=None, c_split=0, lda=128), dict(n_store=32, ldo=32, ldr1=32, ldr2=32, ldv=32),
                   dict(geglu=1, R1=None, R2=None, V=None, vmode=0, A2=None, c_split=0, lda=128, ldo=32)):
            d = _desc(_lib, **kw)
            rc = lib.ctrlv_gemm(ctypes.byref(d), None)
            err = _lib.last_error(lib)
            assert rc == -1 and "unknown mode 7" in err and PITCH_ERR not in err, (kw, rc, err)
        # operands that are absent are not judged by their pitch fields
        d = _desc(_lib, R1=None, R2=None, V=None, vmode=0, A2=None, c_split=0, lda=128, ldr1=0, ldr2=0, ldv=0, lda2=0)
        assert lib.ctrlv_gemm(ctypes.byref(d), None) == -1 and "unknown mode 7" in _lib.last_error(lib)


def _f8_desc(_lib, **kw):
    return _desc(_lib, **dict(dict(A2=None, c_split=0, lda=128, lda2=0, mode=0), **kw))


def test_gemm_f8_refuses_a_pitch_smaller_than_its_row():
    _lib, libs = _libs()
    for lib in libs:
        for field, small, kw in [("ldo", 56, {}), ("ldr1", 56, {}), ("ldr2", 56, {}), ("ldv", 56, {}),
                                 ("ldo", 24, dict(geglu=1, R1=None, R2=None, V=None, vmode=0)), ("lda", 112, {})]:
            d = _f8_desc(_lib, **dict(kw, **{field: small}))
            assert lib.ctrlv_gemm_f8_serves(ctypes.byref(d)) == 0, (field, kw)       # (asserted first: what follows never launches)
            rc = lib.ctrlv_gemm_f8(ctypes.byref(d), P, P, None)
            err = _lib.last_error(lib)
            assert rc == -2 and (PITCH_ERR in err or "lda must be" in err) and field[:3] in err, (field, rc, err)
        # the boundary values are served (the predicate is pure host code)
        for kw in ({}, dict(geglu=1, R1=None, R2=None, V=None, vmode=0, ldo=32), dict(n_store=32, ldo=32, ldr1=32, ldr2=32, ldv=32)):
            d = _f8_desc(_lib, **kw)
            assert lib.ctrlv_gemm_f8_serves(ctypes.byref(d)) == 1, kw


def _ff_desc(_lib, **kw):
    d = _lib.GemmDesc()
    base = dict(out=P, bias=P, R1=P, R2=P, M=8, N=320, Cin=1280, taps=1, mode=0, ldo=320, n_store=320, ldr1=320, ldr2=320,
                s_acc=1.0, s1=1.0, s2=1.0)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_ff_fused_refuses_a_pitch_smaller_than_its_row():
    _lib, libs = _libs()
    for lib in libs:
        for field in ("ldo", "ldr1", "ldr2"):
            d = _ff_desc(_lib, **{field: 312})
            assert lib.ctrlv_ff_fused_serves(ctypes.byref(d), 320) == 0, field
            rc = lib.ctrlv_ff_fused(P, 320, P, P, ctypes.byref(d), None)
            err = _lib.last_error(lib)
            assert rc == -2 and PITCH_ERR in err and f"{field}=312" in err, (field, rc, err)
        assert lib.ctrlv_ff_fused_serves(ctypes.byref(_ff_desc(_lib)), 320) == 1                # ld == 320
        assert lib.ctrlv_ff_fused_serves(ctypes.byref(_ff_desc(_lib, R1=None, R2=None, ldr1=0, ldr2=0)), 320) == 1
        assert lib.ctrlv_ff_fused_serves(ctypes.byref(_ff_desc(_lib)), 312) == 0                # x: ldx >= 320 (as before)


# ---- ops.py: tensors whose pitch a kernel cannot be told must be contiguous; pitched ones need a unit column stride
def _wide(rows, cols, dtype=torch.bfloat16):
    """a column slice of a wider buffer: right shape, wrong pitch"""
    return torch.zeros(rows, cols + 8, dtype=dtype)[:, :cols]


def _z(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


def _dense_only_calls(ops):
    """(function name, the argument sliced, a call) -- one per tensor argument of every wrapper of a dense-only kernel"""
    f32 = torch.float32
    M, C = 16, 64
    x, w, vec, part = lambda: _z(M, C), lambda: _wide(M, C), lambda: _z(C, dtype=f32), lambda: _z(4096, dtype=f32)   # noqa: E731
    qkv, wqkv = lambda: _z(M, 3 * C), lambda: _wide(M, 3 * C)                                                        # noqa: E731
    lse, wlse = lambda: _z(1, 1, M, dtype=f32), lambda: torch.zeros(1, 1, 2 * M, dtype=f32)[:, :, ::2]               # noqa: E731
    calls = []
    for name in ("x", "y", "x_lo"):
        a = dict(x=x(), y=x(), x_lo=None)
        a[name] = w()
        calls.append(("layernorm", name, lambda a=a: ops.layernorm(a["x"], vec(), vec(), 1e-5, a["y"], x_lo=a["x_lo"])))
    for name in ("x", "x2", "y", "x_lo", "x2_lo"):
        a = dict(x=x(), x2=x(), y=_z(M, 2 * C), x_lo=None, x2_lo=None)
        a[name] = _wide(M, 2 * C) if name == "y" else w()
        calls.append(("groupnorm", name, lambda a=a: ops.groupnorm(a["x"], a["x2"], 1, M, 2 * C, 1, vec(), vec(), 1e-5, False, a["y"],
                                                                    part(), x_lo=a["x_lo"], x2_lo=a["x2_lo"])))
    for name in ("x", "y", "x_lo"):
        a = dict(x=x(), y=x(), x_lo=None)
        a[name] = w()
        calls.append(("groupnorm_from_partials", name, lambda a=a: ops.groupnorm_from_partials(a["x"], 1, M, C, 1, vec(), vec(), 1e-5, False,
                                                                                                a["y"], part(), x_lo=a["x_lo"])))
    for name in ("qkv", "out"):
        a = dict(qkv=qkv(), out=x())
        a[name] = wqkv() if name == "qkv" else w()
        calls.append(("attention_spatial", name, lambda a=a: ops.attention_spatial(a["qkv"], a["out"], 1, M, C)))
        calls.append(("attention_temporal", name, lambda a=a: ops.attention_temporal(a["qkv"], a["out"], 1, 4, 4, C)))
    for name in ("qkv", "out", "lse"):
        a = dict(qkv=qkv(), out=x(), lse=lse())
        a[name] = dict(qkv=wqkv, out=w, lse=wlse)[name]()
        calls.append(("attention_spatial_lse", name, lambda a=a: ops.attention_spatial_lse(a["qkv"], a["out"], a["lse"], 1, M, C)))
    for name in ("qkv", "out", "dout", "lse", "dqkv"):
        a = dict(qkv=qkv(), out=x(), dout=x(), lse=lse(), dqkv=qkv())
        a[name] = dict(qkv=wqkv, out=w, dout=w, lse=wlse, dqkv=wqkv)[name]()
        calls.append(("attention_spatial_bwd", name, lambda a=a: ops.attention_spatial_bwd(a["qkv"], a["out"], a["dout"], a["lse"], a["dqkv"],
                                                                                            1, M, C)))
    for name in ("qkv", "out", "dout", "dqkv"):
        a = dict(qkv=qkv(), out=x(), dout=x(), dqkv=qkv())
        a[name] = dict(qkv=wqkv, out=w, dout=w, dqkv=wqkv)[name]()
        calls.append(("attention_temporal_bwd", name, lambda a=a: ops.attention_temporal_bwd(a["qkv"], a["out"], a["dout"], a["dqkv"], 1, 4, 4, C)))
    for name in ("raw", "du", "draw"):
        a = dict(raw=_z(M, 2 * C), du=x(), draw=_z(M, 2 * C))
        a[name] = w() if name == "du" else _wide(M, 2 * C)
        calls.append(("geglu_bwd", name, lambda a=a: ops.geglu_bwd(a["raw"], a["du"], a["draw"])))
    for name in ("x", "dy", "dx", "add"):
        a = dict(x=x(), dy=x(), dx=x(), add=None)
        a[name] = w()
        calls.append(("groupnorm_bwd", name, lambda a=a: ops.groupnorm_bwd(a["x"], a["dy"], 1, M, C, 1, part(), vec(), vec(), False, a["dx"],
                                                                            vec(), vec(), add=a["add"])))
        calls.append(("layernorm_bwd", name, lambda a=a: ops.layernorm_bwd(a["x"], a["dy"], vec(), 1e-5, a["dx"], vec(), vec(), add=a["add"])))
    return calls


def test_dense_only_wrappers_refuse_a_sliced_view():
    g.build()
    from ctrlv_amd import ops
    calls = _dense_only_calls(ops)
    assert {c[0] for c in calls} == {"layernorm", "groupnorm", "groupnorm_from_partials", "attention_spatial", "attention_spatial_lse",
                                     "attention_spatial_bwd", "attention_temporal", "attention_temporal_bwd", "geglu_bwd",
                                     "groupnorm_bwd", "layernorm_bwd"}
    for fn, name, call in calls:
        with pytest.raises(ValueError, match=rf"{fn}: {name} must be contiguous"):
            call()


def test_dense_operands_still_reach_the_device_check():
    """the same calls with contiguous tensors pass the new checks: they get as far as `there is no CPU path`"""
    g.build()
    from ctrlv_amd import ops, _lib
    f32 = torch.float32
    x, vec = _z(16, 64), _z(64, dtype=f32)
    with pytest.raises(_lib.CtrlvHipError, match="no CPU path"):
        ops.layernorm(x, vec, vec, 1e-5, x.clone(), V=_wide(2, 64, f32), vdiv=8, vmod=2)          # V is pitched: a slice is fine
    with pytest.raises(_lib.CtrlvHipError, match="no CPU path"):
        ops.attention_spatial(_z(16, 192), x, 1, 16, 64)
    with pytest.raises(_lib.CtrlvHipError, match="no CPU path"):
        ops.gemm(_wide(16, 64), x, _wide(16, 64), N=64, cin=64, R1=_wide(16, 64), V=_wide(2, 64, f32), vmode=1)


def test_pitched_wrappers_need_a_unit_column_stride():
    g.build()
    from ctrlv_amd import ops
    f32 = torch.float32
    x, t = _z(16, 64), torch.zeros(64, 16, dtype=torch.bfloat16).t()       # t: [16, 64] with strides (1, 16)
    tf = torch.zeros(64, 2, dtype=f32).t()
    for name, call in [
        ("A", lambda: ops.gemm(t, x, x, N=64, cin=64)),
        ("out", lambda: ops.gemm(x, x, t, N=64, cin=64)),
        ("R1", lambda: ops.gemm(x, x, x, N=64, cin=64, R1=t)),
        ("R2", lambda: ops.gemm(x, x, x, N=64, cin=64, R2=t)),
        ("A2", lambda: ops.gemm(x, x, x, N=64, cin=128, A2=t, c_split=64)),
        ("V", lambda: ops.gemm(x, x, x, N=64, cin=64, V=tf, vmode=1)),
        ("raw_out", lambda: ops.gemm(x, x, x, N=64, cin=64, raw_out=t)),
        ("V", lambda: ops.layernorm(x, _z(64, dtype=f32), _z(64, dtype=f32), 1e-5, x.clone(), V=tf)),
        ("x", lambda: ops.ff_fused(t, x, x, x)),
        ("out", lambda: ops.ff_fused(x, x, x, t)),
        ("x", lambda: ops.temporal_fused(t, x, x, 1, 4, 4)),
        ("R1", lambda: ops.temporal_fused(x, x, x, 1, 4, 4, R1=t)),
        ("scores", lambda: ops.softmax_rows(torch.zeros(64, 16, dtype=f32).t(), x)),
        ("probs", lambda: ops.softmax_rows(_z(16, 64, dtype=f32), t)),
        ("x", lambda: ops.colsum(t, _z(64, dtype=f32))),
        ("A", lambda: ops.gemm_wgrad(t, x, _z(64, 64, dtype=f32), N=64, cin=64)),
        ("dY", lambda: ops.gemm_wgrad(x, t, _z(64, 64, dtype=f32), N=64, cin=64)),
        ("rows", lambda: ops.time_conv_rows_to_nchw(t, 1, 64, 16, x, x, x)),
        ("dst", lambda: ops.nchw_to_rows(_z(1, 64, 4, 4), t)),
        ("src", lambda: ops.rows_to_nchw(t, _z(1, 64, 4, 4))),
    ]:
        with pytest.raises(ValueError, match=rf"{name} must have unit column stride"):
            call()
