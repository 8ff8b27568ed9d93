"""Pitched views and guard bands for every kernel that takes a row pitch (tests/guarded.py), both element libraries.

Every case runs the kernel twice on the same values: run A on dense operands into a dense output (what the rest of the suite
does), run B with every pitched operand inside a poison-filled guarded view and every output inside a sentinel-filled guarded
view -- each operand of a launch with a pitch and a column offset of its own, so that a swap cannot cancel -- and asserts
  (a) the bits of B's view equal A's output (a pitch changes addresses, never the summation order: no tolerance),
  (b) no byte outside an output view changed and no sentinel is left inside it (check_written_only_inside), for every output,
  (c) parity_err(A, fp32 reference) below the bound the corresponding test of tests/test_ops_gpu.py /
      tests/test_backward_gpu.py states (tol(3e-3); 1e-4 for fp32 forward outputs; attention tol(5e-3)).
Dense-only operands (no pitch in the ABI) keep row guards; packed weights stay dense with a poison row behind them.

STORE PATHS REACHED (csrc/), per launcher
  ctrlv_gemm
    2-stage kernel, scalar epilogue (gemm.hip) ......... test_gemm_mode0 tiles 1-4 (all epilogues, fp32 out, SiLU, vmode 2,
                                                         n_scale2), test_gemm_pitch_4_mod_8 (the only path for such pitches),
                                                         test_gemm_conv_out_padding, mode 1 / 2 tests on tiles 1 / 4, split
                                                         planes on tile 1, A2 / c_split on tile 0
    2-stage kernel, GEGLU store ......................... test_gemm_geglu tile 1
    gemm_epilogue.h + ping-pong LDS epilogue (gemm_pp_*) test_gemm_mode0 tiles 5-8, test_gemm_geglu tiles 5 / 6 (+ raw_out),
                                                         test_gemm_concat tiles 5 / 6, test_gemm_conv3x3 / _row_halo / _pad_br /
                                                         _temporal tiles 5 / 6 / 10, split planes on tile 6
    w16 register epilogue (gemm_w16*) ................... test_gemm_mode0 tiles 12 / 13, test_gemm_geglu tile 12,
                                                         test_gemm_conv3x3 / _pad_br tile 12
    gemv_small_kernel (tile 11) ......................... test_gemm_per_clip_rows
    splitk_reduce_kernel ................................ test_gemm_split_contraction
    up-phase kernel (gemm_pp_up.hip) .................... test_gemm_up_phase
    GroupNorm-partials writer ........................... test_gemm_gn_partials
  ctrlv_gemm_f8 (gemm_f8.hip) ........................... test_gemm_f8 (128- and 256-wide tiles, GEGLU with n_store = N / 2)
  ctrlv_ff_fused / _ln (ff_fused.hip) ................... test_ff_fused (shared epilogue, the folded row vector, lo planes in fp16)
  ctrlv_temporal_fused (temporal_fused.hip) ............. test_temporal_fused (+ lo planes in fp16)
  quant_rows_f8, softmax_rows, time_conv_rows_to_nchw, nchw_to_rows, gemm_wgrad (both kernels), colsum, layernorm_bwd and
  the dense-only kernels: the tests named after them.

ASSERTED REFUSALS (the launcher's documented conditions; the dense and the guarded run must both raise ValueError)
  * the phase form of the upsampler conv with an R1 operand (bias-only epilogue) -- REFUSALS below, test_gemm_up_phase;
  * R1_lo / out_lo planes in the bf16 library (test_gemm_split_planes, test_ff_fused[r1_lo], test_temporal_fused[lo_planes]);
  * a forced ping-pong tile with pitches that are 4 (mod 8) (test_gemm_pitch_4_mod_8).
Every other combination of every test's matrix runs: `settle` fails a test whose refusals are not exactly the listed ones."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import f8_ref
from tests.guarded import (as_int, check_written_only_inside, fill_, guard_rows, guarded, guarded_flat, put)
from tests.parity_utils import parity_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ELS = [torch.bfloat16, torch.float16]
LO = torch.float8_e5m2
F32 = torch.float32

# (extra columns >= 64, column offset) per operand name: all different, multiples of 8 elements (uint8: of 16 bytes)
PITCH = {"A": (88, 8), "A2": (152, 16), "out": (104, 24), "R1": (72, 32), "R2": (120, 40), "V": (80, 48), "raw_out": (136, 56),
         "x": (88, 8), "ln_V": (96, 64), "dY": (112, 72), "q": (96, 16), "scores": (72, 8), "probs": (104, 24), "rows": (88, 8),
         "dst": (104, 24), "A8": (96, 16)}
PITCH["out_lo"], PITCH["R1_lo"] = PITCH["out"], PITCH["R1"]          # a lo plane has the pitch of its hi plane

# Combinations a launcher refuses by its documented conditions (asserted: both the dense and the guarded run raise ValueError)
REFUSALS = {
    "up_phase": ["r1"],          # the phase form of the upsampler conv takes a bias-only epilogue (ctrlv_gemm_up_phase_serves)
}


@pytest.fixture(scope="module", params=ELS, ids=["bf16", "fp16"])
def el(request, hip_lib):
    return request.param


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _pack_in_the_element_type(el):
    from ctrlv_amd import packing
    with packing.element_dtype(el):
        yield


def tol(bf16_bound, el):
    """tests/test_ops_gpu.py tol(): the stated bf16 bound, a sixth of it for fp16 outputs"""
    return bf16_bound if el == torch.bfloat16 else bf16_bound / 6.0


def g(seed):
    return torch.Generator().manual_seed(seed)


def rows_from_nchw(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def settle(key, refused):
    """the refusals of a test are exactly the ones listed for it"""
    print(f"  refused in {key}: {sorted(refused)}")
    assert sorted(refused) == sorted(REFUSALS.get(key, [])), (key, sorted(refused))


# ------------------------------------------------------------------------------------------------ the A / B harness
def _run(launch, t):
    """launch + synchronize; a HIP failure (not an argument error) ends the session: nothing more is started on a device
    that has reported a fault"""
    try:
        launch(t)
        torch.cuda.synchronize()
    except ValueError:
        raise
    except RuntimeError as e:
        pytest.exit(f"HIP failure, session ended: {e}", returncode=3)


def _dense_run(launch, ins, outs, zero):
    t = {k: v.to(DEV) for k, v in ins.items() if v is not None}
    for k, (shape, dt) in outs.items():
        t[k] = fill_(torch.empty(shape, dtype=dt, device=DEV), "sentinel")
        if k in zero:
            t[k].zero_()
    _run(launch, t)
    return {k: t[k] for k in outs}


def _place(name, shape, dt, fill, pitched, pad, P):
    """(buf, tensor to pass, 2-D view for the checker) of one operand in its guarded buffer"""
    if name == "W":                                     # packed weights stay dense: one poison panel row behind them
        cols = shape[-1]
        rows = math.prod(shape) // cols
        buf = fill_(torch.empty(rows + 1, cols, dtype=dt, device=DEV), fill)
        return buf, buf[:rows].view(shape), buf[:rows]
    if len(shape) == 2 and name in pitched:
        ex, off = P[name]
        buf, view = guarded(shape[0], shape[1], dt, DEV, pitch=shape[1] + ex, col_off=off, pad_rows=pad, fill=fill)
        return buf, view, view
    if len(shape) == 2:                                 # dense-only 2-D operand: row guards
        buf, view = guarded(shape[0], shape[1], dt, DEV, pad_rows=pad, fill=fill)
        return buf, view, view
    n = math.prod(shape)
    buf, flat = guarded_flat(n, dt, DEV, fill=fill)
    return buf, flat.view(shape), flat.view(1, n)


def ab(launch, ins, outs, *, pitched=(), W=0, zero=(), override=None, dense=None):
    """Run A (dense) and run B (guarded) of `launch(t)`, t = {name: device tensor}.  ins: name -> CPU tensor (None: absent);
    outs: name -> (shape, dtype); pitched: the names whose pitch the kernel is told; W: image width (sizes the row guards);
    zero: outputs the kernel accumulates into (zeroed inside the view); override: {name: (extra, offset)}; dense: a dict of
    dense results to compare against in place of run A.  Asserts (a) and (b); returns A's outputs, or None when the
    launcher refuses the combination (then it must refuse the guarded one as well)."""
    P = dict(PITCH, **(override or {}))
    pad = guard_rows(W)
    if dense is None:
        try:
            dense = _dense_run(launch, ins, outs, zero)
        except ValueError:
            dense = None
    t, placed = {}, {}
    for k, v in ins.items():
        if v is not None:
            _, t[k], _ = _place(k, tuple(v.shape), v.dtype, "poison", pitched, pad, P)
            put(t[k], v.to(DEV))
    for k, (shape, dt) in outs.items():
        buf, t[k], view2 = _place(k, tuple(shape), dt, "sentinel", pitched, pad, P)
        if k in zero:
            view2.zero_()
        placed[k] = (buf, view2, buf.clone())
    if dense is None:
        with pytest.raises(ValueError):
            _run(launch, t)
        return None
    _run(launch, t)
    for k, (buf, view2, before) in placed.items():
        want = dense[k].reshape(view2.shape)
        bad = as_int(view2) != as_int(want)
        assert not bool(bad.any()), (f"{k}: {int(bad.sum())} elements of the guarded view differ from the dense run, first at "
                                     f"{[int(i) for i in bad.nonzero()[0]]}")
        check_written_only_inside(before, buf, view2, expected=want, what=k)
    return dense


def gemm_launch(ops, **static):
    def run(t):
        ops.gemm(t["A"], t["W"], t["out"], **{k: v for k, v in t.items() if k not in ("A", "W", "out")}, **static)
    return run


GEMM_PITCHED = ("A", "A2", "out", "R1", "R2", "V", "raw_out", "out_lo", "R1_lo")


# ------------------------------------------------------------------------------------------------ ops.gemm, mode 0
@functools.lru_cache(maxsize=None)
def lin_case(el, M, N, K):
    from ctrlv_amd import packing
    with packing.element_dtype(el):
        A = torch.randn(M, K, generator=g(1)).to(el)
        Wt = torch.randn(N, K, generator=g(2)) / math.sqrt(K)
        Wp = packing.pack_linear(Wt)
    bias = torch.randn(N, generator=g(3))
    c = dict(A=A, W=Wp, bias=bias, R1=torch.randn(M, N, generator=g(4)).to(el), R2=torch.randn(M, N, generator=g(5)).to(el),
             V=torch.randn(7, N, generator=g(6)), lin=A.float() @ Wp[:N].float().T + bias)
    m = torch.arange(M)
    c["vidx"], c["vidx2"] = (m // 13) % 7, ((m // 50) * 10 + (m % 10)) % 7
    return c


def mode0_epilogues(c, tile):
    """name -> (operand names, static keywords, fp32 reference, output dtype or None for the element type)"""
    lin, R1, R2, V = c["lin"], c["R1"].float(), c["R2"].float(), c["V"]
    N = lin.shape[1]
    e = {"r1r2": (("bias", "R1", "R2"), dict(s1=0.5, s2=-0.25, s_acc=0.7), 0.7 * lin + 0.5 * R1 - 0.25 * R2, None),
         "r1v": (("bias", "R1", "V"), dict(vmode=1, vdiv=13, vmod=7), lin + R1 + V[c["vidx"]], None)}
    if tile in (1, 6):
        e["r1v2"] = (("bias", "R1", "V"), dict(vmode=2, vdiv=50, vS=10, vmod=7), lin + R1 + V[c["vidx2"]], None)
    if 1 <= tile <= 4:
        e["v_silu_f32"] = (("bias", "V"), dict(vmode=1, vdiv=13, vmod=7, act=1, out_f32=True), F.silu(lin + V[c["vidx"]]), F32)
    if tile in (1, 5):
        n2 = N // 64 * 32
        e["n_scale2"] = (("bias",), dict(s_acc=1.5, n_scale2=n2, s_acc2=0.25), lin * torch.where(torch.arange(N) < n2, 0.25, 1.5), None)
    return e


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13])
def test_gemm_mode0(ops, el, tile):
    """M = 300 is ragged against the 128- and the 256-row tiles, N = 320 against the 256-wide ones, K / 32 = 4 is the
    ping-pong minimum."""
    M, N, K = 300, 320, 128
    c = lin_case(el, M, N, K)
    refused = []
    for name, (opnds, static, ref, dt) in mode0_epilogues(c, tile).items():
        ins = dict(A=c["A"], W=c["W"], **{k: c[k] for k in opnds})
        got = ab(gemm_launch(ops, N=N, cin=K, tile=tile, **static), ins, dict(out=((M, N), dt or el)), pitched=GEMM_PITCHED)
        if got is None:
            refused.append(name)
            continue
        assert parity_err(got["out"], ref, f"mode 0 tile {tile} {name}") < (1e-4 if dt == F32 else tol(3e-3, el))
    settle(f"mode0[{tile}]", refused)


def test_gemm_pitch_4_mod_8(ops, el):
    """ldo, ldr1, ldv = 4 (mod 8): the ping-pong epilogue moves 8 columns per lane, so the automatic choice falls back to
    the 128 x 128 2-stage kernel (M = 1100 would take a ping-pong tile otherwise); the forced tiles 1-4 serve such
    pitches themselves.  Bit for bit the dense launch on forced tile 1."""
    M, N, K = 1100, 320, 128
    c = lin_case(el, M, N, K)
    ins = dict(A=c["A"], W=c["W"], bias=c["bias"], R1=c["R1"], V=c["V"])
    static = dict(N=N, cin=K, vmode=1, vdiv=13, vmod=7)
    outs = dict(out=((M, N), el))
    dense = _dense_run(gemm_launch(ops, tile=1, **static), ins, outs, ())
    assert parity_err(dense["out"], c["lin"] + c["R1"].float() + c["V"][c["vidx"]], "pitch 4 mod 8") < tol(3e-3, el)
    odd = dict(out=(100, 24), R1=(68, 32), V=(84, 48))
    for tile in (0, 1, 2, 3, 4):
        assert ab(gemm_launch(ops, tile=tile, **static), ins, outs, pitched=GEMM_PITCHED, override=odd, dense=dense) is not None
    with pytest.raises(ValueError):          # a forced ping-pong tile says so
        ab(gemm_launch(ops, tile=5, **static), ins, outs, pitched=GEMM_PITCHED, override=odd, dense=dense)


@functools.lru_cache(maxsize=None)
def geglu_case(el):
    from ctrlv_amd import packing
    M, C = 333, 320
    with packing.element_dtype(el):
        A = torch.randn(M, C, generator=g(1)).to(el)
        Wt = torch.randn(8 * C, C, generator=g(2)) / math.sqrt(C)
        b = torch.randn(8 * C, generator=g(3))
        Wp, bp = packing.pack_geglu(Wt, b)
    proj = A.float() @ Wt.to(el).float().T + b
    raw = A.float() @ Wp.float().T + bp.float()
    return dict(A=A, W=Wp, bias=bp.float().contiguous(), ref=proj[:, :4 * C] * F.gelu(proj[:, 4 * C:]), raw=raw)


@pytest.mark.parametrize("tile", [1, 5, 6, 12])
def test_gemm_geglu(ops, el, tile):
    M, C = 333, 320
    c = geglu_case(el)
    ins = dict(A=c["A"], W=c["W"], bias=c["bias"])
    refused = []
    got = ab(gemm_launch(ops, N=8 * C, cin=C, geglu=1, tile=tile), ins, dict(out=((M, 4 * C), el)), pitched=GEMM_PITCHED)
    if got is None:
        refused.append("geglu")
    else:
        assert parity_err(got["out"], c["ref"], f"geglu tile {tile}") < tol(3e-3, el)
    if tile in (5, 6):          # the training forward's second output: the projection before the gate, packed column order
        got = ab(gemm_launch(ops, N=8 * C, cin=C, geglu=1, tile=tile), ins,
                 dict(out=((M, 4 * C), el), raw_out=((M, 8 * C), el)), pitched=GEMM_PITCHED)
        if got is None:
            refused.append("raw_out")
        else:
            assert parity_err(got["out"], c["ref"], "geglu + raw_out: u") < tol(3e-3, el)
            assert parity_err(got["raw_out"], c["raw"], "geglu + raw_out: raw") < tol(3e-3, el)
    settle(f"geglu[{tile}]", refused)


@pytest.mark.parametrize("tile", [0, 5, 6])
def test_gemm_concat(ops, el, tile):
    """A2 / c_split: the skip-concat read of the up blocks' 1x1 shortcuts (tests/test_ops_gpu.py test_gemm_concat_split)."""
    from ctrlv_amd import packing
    M, C1, C2, N = 500, 128, 64, 128
    a1, a2 = torch.randn(M, C1, generator=g(1)).to(el), torch.randn(M, C2, generator=g(2)).to(el)
    wt = torch.randn(N, C1 + C2, generator=g(3)) / math.sqrt(C1 + C2)
    bias = torch.randn(N, generator=g(4))
    ref = torch.cat([a1, a2], 1).float() @ wt.to(el).float().T + bias
    ins = dict(A=a1, A2=a2, W=packing.pack_linear(wt), bias=bias)
    got = ab(gemm_launch(ops, N=N, cin=C1 + C2, c_split=C1, tile=tile), ins, dict(out=((M, N), el)), pitched=GEMM_PITCHED)
    assert got is not None
    assert parity_err(got["out"], ref, f"concat tile {tile}") < tol(3e-3, el)


def test_gemm_per_clip_rows(ops, el):
    """Tile 11 (gemv_small_kernel) the way the conditioning path runs it (models/encoder.py, the xattn GEMMs): one 1280-wide
    block out of a wider A into one block of a wider output."""
    M, K, N = 5, 1024, 1280
    c = lin_case(el, M, N, K)
    lin, R1, V = c["lin"], c["R1"].float(), c["V"][:3]
    vi = torch.arange(M) % 3
    cases = {"bias": ((), {}, lin, None),
             "r1_silu": (("R1",), dict(s1=0.5, s_acc=0.75, act=1), F.silu(0.75 * lin + 0.5 * R1), None),
             "v": (("V",), dict(vmode=1, vdiv=1, vmod=3), lin + V[vi], None),
             "f32": ((), dict(out_f32=True), lin, F32)}
    wide = dict(A=(1280 + 256, 256), out=(2560 + 64, 1280))          # (column blocks of the v_all / xattn tables)
    for name, (opnds, static, ref, dt) in cases.items():
        ins = dict(A=c["A"], W=c["W"], bias=c["bias"], **{k: (V if k == "V" else c[k]) for k in opnds})
        got = ab(gemm_launch(ops, N=N, cin=K, tile=11, **static), ins, dict(out=((M, N), dt or el)), pitched=GEMM_PITCHED,
                 override=wide)
        assert got is not None, name
        assert parity_err(got["out"], ref, f"tile 11 {name}") < (1e-4 if dt == F32 else tol(3e-3, el))


def test_gemm_conv_out_padding(ops, el):
    """N padded to 32 with n_store = 4 (conv_out), ldo = 12: columns [4, 12) of every row and [4, 32) of the weight's padding
    stay out of the output."""
    from ctrlv_amd import packing
    A = torch.randn(2, 256, generator=g(1)).to(el)
    wt = torch.randn(4, 256, generator=g(2)) / 16
    b = torch.randn(4, generator=g(3))
    ins = dict(A=A, W=packing.pack_linear(wt), bias=packing.pad_bias(b))
    got = ab(gemm_launch(ops, N=32, cin=256, n_store=4), ins, dict(out=((2, 4), el)), pitched=GEMM_PITCHED,
             override=dict(out=(8, 4)))
    assert got is not None
    assert parity_err(got["out"], A.float() @ wt.to(el).float().T + b) < tol(3e-3, el)


# ------------------------------------------------------------------------------------------------ ops.gemm, mode 1
@functools.lru_cache(maxsize=None)
def conv_case(el, n, cin, cout, H, W, stride=1, up=0, pad_br=False):
    from ctrlv_amd import packing
    with packing.element_dtype(el):
        x = torch.randn(n, cin, H, W, generator=g(1)).to(el)
        wt = torch.randn(cout, cin, 3, 3, generator=g(2)) / math.sqrt(9 * cin)
        Wp = packing.pack_conv3x3(wt)
    b = torch.randn(cout, generator=g(3))
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if up else x.float()
    if pad_br:
        ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), wt.to(el).float(), b, stride=2)
    else:
        ref = F.conv2d(xin, wt.to(el).float(), b, stride=stride, padding=1)
    Ho, Wo = ref.shape[-2:]
    M = n * Ho * Wo
    return dict(A=rows_from_nchw(x), W=Wp, wt=wt, bias=packing.pad_bias(b) if Wp.shape[0] != cout else b, ref=rows_from_nchw(ref),
                Ho=Ho, Wo=Wo, M=M, R1=torch.randn(M, cout, generator=g(4)).to(el), V=torch.randn(n, cout, generator=g(5)), x=x, b=b)


def conv_ab(ops, el, c, cin, cout, H, W, stride, up, tile, epi="bias", extra=None, outs=None, **static):
    """the launch of a 3x3 conv case with the epilogue {bias} / {bias, R1} / {bias, V}: (dense outputs or None, reference)"""
    ins = dict(A=c["A"], W=c["W"], bias=c["bias"])
    ref = c["ref"]
    if epi == "r1":
        ins["R1"] = c["R1"]
        static.update(s1=0.5, s_acc=0.75)
        ref = 0.75 * ref + 0.5 * c["R1"].float()
    elif epi == "v":
        ins["V"] = c["V"]
        static.update(vmode=1, vdiv=c["Ho"] * c["Wo"])
        ref = ref + c["V"][torch.arange(c["M"]) // (c["Ho"] * c["Wo"])]
    ins.update(extra or {})
    o = dict(out=((c["M"], cout), el), **(outs or {}))
    got = ab(gemm_launch(ops, N=c["W"].shape[-2], cin=cin, taps=9, mode=1, conv=(H, W, c["Ho"], c["Wo"], stride, up), n_store=cout,
                         tile=tile, **static), ins, o, pitched=GEMM_PITCHED, W=max(W, c["Wo"]))
    return got, ref


@pytest.mark.parametrize("tile", [1, 5, 6, 10, 12])
@pytest.mark.parametrize("stride,up", [(1, 0), (2, 0), (1, 1)])
def test_gemm_conv3x3(ops, el, tile, stride, up):
    """3 images of 8 x 12: image borders inside a tile; the input's guard rows catch an unmasked halo read before image 0 or
    behind the last image (a NaN would reach the border pixels)."""
    n, cin, cout, H, W = 3, 64, 96, 8, 12
    c = conv_case(el, n, cin, cout, H, W, stride, up)
    refused = []
    for epi in ("bias", "r1"):
        got, ref = conv_ab(ops, el, c, cin, cout, H, W, stride, up, tile, epi)
        if got is None:
            refused.append(epi)
            continue
        assert parity_err(got["out"], ref, f"conv3x3 s{stride} up{up} tile {tile} {epi}") < tol(3e-3, el)
    settle(f"conv3x3[{stride},{up},{tile}]", refused)


@pytest.mark.parametrize("tile", [0, 1, 5, 6, 10, 12])
def test_gemm_pad_br(ops, el, tile):
    """bottom / right padded stride-2 conv (tests/test_gemm_pad_br_gpu.py, the `edges` geometry)"""
    n, cin, cout, H, W = 3, 64, 96, 8, 12
    c = conv_case(el, n, cin, cout, H, W, 2, 0, True)
    refused = []
    for epi in ("bias", "r1", "v"):
        got, ref = conv_ab(ops, el, c, cin, cout, H, W, 2, 0, tile, epi, pad_br=True)
        if got is None:
            refused.append(epi)
            continue
        assert parity_err(got["out"], ref, f"pad_br tile {tile} {epi}") < tol(3e-3, el)
    settle(f"pad_br[{tile}]", refused)


@pytest.mark.parametrize("tile", [1, 5, 6, 10])
def test_gemm_conv3x3_row_halo(ops, el, tile):
    """The row-halo kernels (stride 1, row width dividing the 256-row tile): tiles that straddle images, ragged last tile."""
    H, W, n, cin, cout = 10, 64, 3, 64, 320
    c = conv_case(el, n, cin, cout, H, W)
    refused = []
    for epi in ("bias", "r1"):
        got, ref = conv_ab(ops, el, c, cin, cout, H, W, 1, 0, tile, epi)
        if got is None:
            refused.append(epi)
            continue
        assert parity_err(got["out"], ref, f"row halo tile {tile} {epi}") < tol(3e-3, el)
    settle(f"row_halo[{tile}]", refused)


@pytest.mark.parametrize("n,H,W,cin,cout", [(3, 3, 16, 64, 64), (2, 9, 32, 64, 320)])
def test_gemm_up_phase(ops, el, n, H, W, cin, cout):
    """The phase form of the upsampler conv (gemm_pp_up.hip) at the W = 16 shape tests/test_up_phase_gpu.py serves, and at its
    N = 320 shape, where the fp16 library also writes the out_lo plane.  The phase form takes a bias-only epilogue: R1 is an
    asserted refusal."""
    c = conv_case(el, n, cin, cout, H, W, 1, 1)
    wph = ops.pack_up_phase_weight(c["wt"].to(DEV), el).cpu()
    kw = dict(N=cout, cin=cin, taps=9, mode=1, conv=(H, W, 2 * H, 2 * W, 1, 2))
    probe = torch.empty(c["M"], cout, dtype=el, device=DEV)
    assert ops.gemm_up_phase_serves(c["A"].to(DEV), wph.to(DEV), probe, bias=c["b"].to(DEV), **kw)
    refused = []
    for epi in ("bias", "r1", "lo"):
        ins = dict(A=c["A"], W=wph, bias=c["b"])
        outs, static = dict(out=((c["M"], cout), el)), {}
        if epi == "r1":
            ins["R1"], static = c["R1"], dict(s1=0.5, s_acc=0.75)
        if epi == "lo":
            if el != torch.float16 or cout % 320:
                continue
            outs["out_lo"] = ((c["M"], cout), LO)
        got = ab(gemm_launch(ops, **kw, **static), ins, outs, pitched=GEMM_PITCHED, W=2 * W)
        if got is None:
            refused.append(epi)
            continue
        # (the phase weights are sums of taps rounded once more: tests/test_up_phase_gpu.py test_rounding bounds the launch
        #  against the fp64 convs of its own packed weights by tol(3e-3); so does this)
        assert parity_err(got["out"], _phase_ref(c, wph, epi), f"up phase {epi}") < tol(3e-3, el)
    settle("up_phase", refused)


def _phase_ref(c, wph, epi):
    x, b = c["x"], c["b"]
    n, C, H, W = x.shape
    N = wph.shape[1]
    xp = F.pad(x.double(), (1, 1, 1, 1))
    out = torch.empty(n, N, 2 * H, 2 * W, dtype=torch.float64)
    for p in range(4):
        py, px = p >> 1, p & 1
        w = wph[p].double().reshape(N, 2, 2, C).permute(0, 3, 1, 2)
        out[:, :, py::2, px::2] = F.conv2d(xp, w, b.double())[:, :, py:py + H, px:px + W]
    ref = rows_from_nchw(out)
    return (0.75 * ref + 0.5 * c["R1"].double() if epi == "r1" else ref).float()


def test_gemm_gn_partials(ops, el):
    """The GroupNorm-partials writer of the 256 x 320 ping-pong tile: the partials buffer [M / 64][32][2] is guarded too (its
    (mean, rstd) table behind belongs to ctrlv_groupnorm_from_partials, not to this launch)."""
    H, W, n, cin, cout = 8, 32, 6, 64, 320
    c = conv_case(el, n, cin, cout, H, W)
    kw = dict(N=cout, cin=cin, taps=9, mode=1, conv=(H, W, H, W, 1, 0))
    probe = torch.empty(c["M"], cout, dtype=el, device=DEV)
    assert ops.gemm_gn_partials_serves(c["A"].to(DEV), c["W"].to(DEV), probe, bias=c["b"].to(DEV), R1=c["R1"].to(DEV), s1=0.5,
                                       s_acc=0.75, **kw)
    got, ref = conv_ab(ops, el, c, cin, cout, H, W, 1, 0, 0, "r1", outs=dict(gn_partials=((c["M"] // 64 * 64,), F32)))
    assert got is not None
    assert parity_err(got["out"], 0.75 * c["ref"] + 0.5 * c["R1"].float(), "gn partials: out") < tol(3e-3, el)
    # the partials against the stored output: per 64-row chunk and group, (mean, M2) -- fp32 statistics, bound 1e-4
    o = got["out"].float().cpu().reshape(c["M"] // 64, 64, 32, cout // 32)
    p = got["gn_partials"].cpu().reshape(c["M"] // 64, 32, 2)
    mean = o.mean(dim=(1, 3))
    assert parity_err(p[:, :, 0], mean, "gn partials: chunk means") < tol(3e-3, el)       # (of the values BEFORE the output rounding)


def test_gemm_split_contraction(ops, el):
    """splitk_reduce_kernel's ldo / ldr1: the long-K conv at 5 x 8 runs in K slices + the streaming sum / epilogue kernel."""
    H, W, n, cin, cout = 5, 8, 6, 1280, 1280
    c = conv_case(el, n, cin, cout, H, W)
    kw = dict(N=cout, cin=cin, taps=9, mode=1, conv=(H, W, H, W, 1, 0))
    probe = torch.empty(c["M"], cout, dtype=el, device=DEV)
    assert ops.gemm_splitk_slices(c["A"].to(DEV), c["W"].to(DEV), probe, bias=c["b"].to(DEV), R1=c["R1"].to(DEV), **kw) > 1
    got, ref = conv_ab(ops, el, c, cin, cout, H, W, 1, 0, 0, "r1")
    assert got is not None
    assert parity_err(got["out"], ref, "split contraction") < tol(3e-3, el)


# ------------------------------------------------------------------------------------------------ ops.gemm, mode 2
@pytest.mark.parametrize("tile", [1, 4, 5, 6, 10])
def test_gemm_temporal(ops, el, tile):
    from ctrlv_amd import packing
    B, Fr, S, C = 2, 5, 24, 64
    M = B * Fr * S
    x = torch.randn(B, C, Fr, S, 1, generator=g(1)).to(el)
    wt = torch.randn(C, C, 3, 1, 1, generator=g(2)) / math.sqrt(3 * C)
    b = torch.randn(C, generator=g(3))
    R1 = torch.randn(M, C, generator=g(4)).to(el)
    conv = F.conv3d(x.float(), wt.to(el).float(), b, padding=(1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(M, C)
    rows = x.permute(0, 2, 3, 4, 1).reshape(M, C).contiguous()
    Wp = packing.pack_conv_temporal(wt)
    refused = []
    for epi, ref in (("bias", conv), ("r1", 0.75 * conv + 0.5 * R1.float())):
        ins = dict(A=rows, W=Wp, bias=b)
        static = {}
        if epi == "r1":
            ins["R1"], static = R1, dict(s1=0.5, s_acc=0.75)
        got = ab(gemm_launch(ops, N=C, cin=C, taps=3, mode=2, temporal=(Fr, S), tile=tile, **static), ins, dict(out=((M, C), el)),
                 pitched=GEMM_PITCHED, W=S)
        if got is None:
            refused.append(epi)
            continue
        assert parity_err(got["out"], ref, f"temporal conv tile {tile} {epi}") < tol(3e-3, el)
    settle(f"temporal[{tile}]", refused)


# ------------------------------------------------------------------------------------------------ split planes (fp16)
@pytest.mark.parametrize("tile", [1, 6])
def test_gemm_split_planes(ops, el, tile):
    """fp16 library: out_lo and R1_lo ride in guarded byte planes with the pitches of out / R1 (the bf16 library refuses the
    planes: asserted)."""
    from tests.split_planes import split
    M, N, K = 300, 320, 128
    c = lin_case(el, M, N, K)
    r1 = torch.randn(M, N, generator=g(9)) * 3
    r1_hi, r1_lo = split(r1)
    r1_hi = r1_hi.to(el)
    ins = dict(A=c["A"], W=c["W"], bias=c["bias"], R1=r1_hi, R1_lo=r1_lo)
    got = ab(gemm_launch(ops, N=N, cin=K, tile=tile, s1=0.5), ins, dict(out=((M, N), el), out_lo=((M, N), LO)), pitched=GEMM_PITCHED)
    if el != torch.float16:
        assert got is None, "split planes are served by the fp16 library only"
        return
    assert got is not None
    ref = c["lin"].double() + 0.5 * (r1_hi.double() + r1_lo.double())
    assert parity_err(got["out"], ref.float(), f"split planes tile {tile}: hi") < tol(3e-3, el)
    both = got["out"].double().cpu() + got["out_lo"].cpu().double()
    assert parity_err(both.float(), ref.float(), "hi + lo") < tol(3e-3, el)


# ------------------------------------------------------------------------------------------------ ops.gemm_f8
@functools.lru_cache(maxsize=None)
def f8_case(M, N, K):
    A = torch.randn(M, K, generator=g(1)) * (1.0 + torch.arange(M).float().unsqueeze(1) % 7)
    W = torch.randn(N, K, generator=g(2)) / math.sqrt(K) * (0.5 + torch.arange(N).float().unsqueeze(1) % 5)
    (qa, sa), (qw, sw) = f8_ref.quant_rows(A), f8_ref.quant_rows(W)
    bias = torch.randn(N, generator=g(3))
    lin = (qa.double() @ qw.double().T) * sa.double().unsqueeze(1) * sw.double().unsqueeze(0) + bias.double()
    return dict(A8=qa.view(torch.uint8).contiguous(), sa=sa, W=qw.view(torch.uint8).contiguous(), sw=sw, bias=bias, lin=lin,
                R1=torch.randn(M, N, generator=g(4)), R2=torch.randn(M, N, generator=g(5)), V=torch.randn(7, N, generator=g(6)))


@pytest.mark.parametrize("tile", [1, 2])
def test_gemm_f8(ops, el, tile):
    M, N, K = 200, 256, 128
    c = f8_case(M, N, K)
    R1, R2 = c["R1"].to(el), c["R2"].to(el)
    vidx = (torch.arange(M) // 13) % 7

    def launch(**static):
        def run(t):
            ops.gemm_f8(t["A8"], t["sa"], t["W"], t["sw"], t["out"],
                        **{k: v for k, v in t.items() if k not in ("A8", "sa", "W", "sw", "out")}, N=N, cin=K, tile=tile, **static)
        return run
    base = dict(A8=c["A8"], sa=c["sa"], W=c["W"], sw=c["sw"], bias=c["bias"])
    pitched = ("A8", "out", "R1", "R2", "V")
    lin = c["lin"]
    for name, extra, static, ref, shape in [
            ("r1r2", dict(R1=R1, R2=R2), dict(s1=0.5, s2=-0.25, s_acc=0.7), 0.7 * lin + 0.5 * R1.double() - 0.25 * R2.double(), (M, N)),
            ("r1v", dict(R1=R1, V=c["V"]), dict(vmode=1, vdiv=13, vmod=7), lin + R1.double() + c["V"][vidx].double(), (M, N)),
            ("geglu", {}, dict(geglu=1, n_store=N // 2), _geglu_ref(lin), (M, N // 2))]:
        got = ab(launch(**static), dict(base, **extra), dict(out=(shape, el)), pitched=pitched)
        assert got is not None, name
        assert parity_err(got["out"], ref.float(), f"gemm_f8 tile {tile} {name}") < tol(3e-3, el)


def _geglu_ref(lin):
    M, N = lin.shape
    b = lin.reshape(M, N // 32, 2, 16)
    return (b[:, :, 0] * F.gelu(b[:, :, 1])).reshape(M, N // 2)


# ------------------------------------------------------------------------------------------------ ops.ff_fused (+ ln)
@functools.lru_cache(maxsize=None)
def ff_case(el):
    C, I = 320, 1280
    return dict(w1=torch.randn(2 * I, C, generator=g(1)) / C ** 0.5, b1=torch.randn(2 * I, generator=g(2)) * 0.5,
                w2=torch.randn(C, I, generator=g(3)) / I ** 0.5, b2=torch.randn(C, generator=g(4)))


@pytest.fixture(scope="module")
def ff_weights(ops, el):
    from ctrlv_amd import packing
    c = ff_case(el)
    with packing.element_dtype(el):
        w1p, b1p = packing.pack_geglu(c["w1"].to(DEV), c["b1"].to(DEV))
        w2p = packing.pack_linear(c["w2"].to(DEV))
    return ops.ff_fused_pack(w1p, b1p.float().contiguous(), w2p)


def _ff_ref(c, el, x, kw, r1, r2, V, vidx):
    a, gt = (x.double() @ c["w1"].to(el).double().t() + c["b1"].double()).chunk(2, dim=-1)
    uu = (a * F.gelu(gt)).float().to(el).double()
    ref = kw.get("s_acc", 1.0) * (uu @ c["w2"].to(el).double().t() + c["b2"].double())
    if "R1" in kw:
        ref = ref + kw.get("s1", 1.0) * r1.double()
    if "R2" in kw:
        ref = ref + kw["s2"] * r2.double()
    if vidx is not None:
        ref = ref + V.double()[vidx]
    return ref.float()


@pytest.mark.parametrize("M", [300, 2 * 256 + 72])
@pytest.mark.parametrize("epi", ["r1", "r1r2", "r1v", "r1v_epi", "ln", "ln_v", "r1_lo"])
def test_ff_fused(ops, el, ff_weights, M, epi):
    """x, out, R1, R2, V and ln_V each with a pitch of its own; r1v: the row vector folded into the accumulator start (vdiv a
    multiple of 256) -- ln_v: the LayerNorm prologue's row-vector table -- r1_lo: the split trunk planes R1_lo / out_lo (fp16
    library; the bf16 library refuses them: asserted)."""
    from tests.split_planes import split
    C = 320
    c = ff_case(el)
    w1f, w2f = ff_weights
    x = (torch.randn(M, C, generator=g(5)) * (2.0 if epi.startswith("ln") else 1.0) + (0.7 if epi.startswith("ln") else 0.0)).to(el)
    r1, r2 = torch.randn(M, C, generator=g(6)).to(el), torch.randn(M, C, generator=g(7)).to(el)
    V = torch.randn(5, C, generator=g(8))
    ins, static, vidx, xin = dict(x=x, bias=c["b2"], R1=r1), {}, None, x
    outs = dict(out=((M, C), el))
    if epi == "r1_lo":
        hi, ins["R1_lo"] = split(torch.randn(M, C, generator=g(6)) * 3)
        ins["R1"] = hi.to(el)
        r1 = ins["R1"].double() + ins["R1_lo"].double()
        outs["out_lo"] = ((M, C), LO)
    if epi == "r1r2":
        ins["R2"], static = r2, dict(s2=0.25, s_acc=0.75, s1=0.75)
    elif epi == "r1v":
        ins["V"], static, vidx = V, dict(vmode=1, vdiv=256, vmod=5), (torch.arange(M) // 256) % 5
    elif epi == "r1v_epi":      # vdiv no multiple of the tile: the shared epilogue's row-vector operand
        ins["V"], static, vidx = V, dict(vmode=1, vdiv=200, vmod=5, s_acc=0.5), (torch.arange(M) // 200) % 5
    elif epi.startswith("ln"):
        gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g(9)), 0.3 * torch.randn(C, generator=g(10))
        lnin = x.float()
        if epi == "ln_v":
            ins["ln_V"], static = V[:3], dict(ln_vdiv=256, ln_vmod=3)
            lnin = lnin + V[:3][(torch.arange(M) // 256) % 3]
        ins.update(gamma=gamma, beta=beta)
        xin = F.layer_norm(lnin, (C,), gamma, beta, 1e-5).to(el)

    def run(t):
        kw = {k: v for k, v in t.items() if k not in ("x", "out", "gamma", "beta")}
        if "gamma" in t:
            kw["ln"] = (t["gamma"], t["beta"], 1e-5)
        ops.ff_fused(t["x"], w1f, w2f, t["out"], **kw, **static)
    got = ab(run, ins, outs, pitched=("x", "out", "R1", "R2", "V", "ln_V", "R1_lo", "out_lo"))
    if epi == "r1_lo" and el != torch.float16:
        assert got is None, "split planes are served by the fp16 library only"
        return
    assert got is not None
    ref = _ff_ref(c, el, xin, dict(ins, **static), r1, r2, V, vidx)
    res = got["out"].double().cpu() + (got["out_lo"].cpu().double() if epi == "r1_lo" else 0.0)
    assert parity_err(res.float(), ref, f"ff_fused M {M} {epi}") < tol(3e-3, el)


# ------------------------------------------------------------------------------------------------ ops.temporal_fused
@pytest.mark.parametrize("B,Fr,S,vm", [(2, 25, 8, 2), (1, 3, 40, 0)])
@pytest.mark.parametrize("planes", [False, True], ids=["plain", "lo_planes"])
def test_temporal_fused(ops, el, B, Fr, S, vm, planes):
    """x, out, R1, V pitched; in fp16 also with the R1_lo / out_lo byte planes (the bf16 library refuses them: asserted)."""
    from ctrlv_amd import packing
    from tests.split_planes import split
    C, heads, M = 320, 5, B * Fr * S
    x = torch.randn(M, C, generator=g(1)).to(el)
    r1f = torch.randn(M, C, generator=g(2)) * 2
    wq, wk, wv = (torch.randn(C, C, generator=g(3 + i)) / math.sqrt(C) for i in range(3))
    wo, bo = torch.randn(C, C, generator=g(7)) / math.sqrt(C), torch.randn(C, generator=g(8))
    vt = torch.randn(B, C, generator=g(9)) if vm else None
    wf = ops.temporal_fused_pack(packing.pack_qkv(wq, wk, wv).to(DEV), packing.pack_linear(wo).to(DEV))
    ins = dict(x=x, bias=bo, R1=r1f.to(el), V=vt)
    outs = dict(out=((M, C), el))
    r1 = ins["R1"].double()
    if planes:
        ins["R1"], ins["R1_lo"] = split(r1f)
        ins["R1"] = ins["R1"].to(el)
        outs["out_lo"] = ((M, C), LO)
        r1 = ins["R1"].double() + ins["R1_lo"].double()
    static = {} if not vm else dict(vmode=2, vdiv=Fr * S, vS=S, vmod=B)

    def run(t):
        ops.temporal_fused(t["x"], wf, t["out"], B, Fr, S, **{k: v for k, v in t.items() if k not in ("x", "out")}, **static)
    got = ab(run, ins, outs, pitched=("x", "out", "R1", "V", "R1_lo", "out_lo"), W=S)
    if planes and el != torch.float16:
        assert got is None, "split planes are served by the fp16 library only"
        return
    assert got is not None
    bf = lambda t: t.to(el)      # noqa: E731
    q, k, v = (bf(x.float() @ bf(w).float().T).float() for w in (wq, wk, wv))

    def tok(t):
        return t.reshape(B, Fr, S, heads, 64).permute(0, 2, 3, 1, 4).reshape(B * S, heads, Fr, 64)
    att = F.scaled_dot_product_attention(tok(q), tok(k), tok(v)).reshape(B, S, heads, Fr, 64).permute(0, 3, 1, 2, 4).reshape(M, C)
    ref = bf(att).double() @ bf(wo).double().T + bo.double() + r1
    if vm:
        m = torch.arange(M)
        ref = ref + vt.double()[((m // (Fr * S)) * S + m % S) % B]
    res = got["out"].double().cpu() + (got["out_lo"].cpu().double() if planes else 0.0)
    assert parity_err(res.float(), ref.float(), f"temporal_fused B{B} F{Fr} S{S}") < tol(5e-3, el)


# ------------------------------------------------------------------------------------------------ other pitched kernels
@pytest.mark.parametrize("M,K", [(7, 128), (333, 640)])
def test_quant_rows_f8(ops, el, M, K):
    x = (torch.randn(M, K, generator=g(K)) * (0.01 + torch.arange(M).float().unsqueeze(1) % 5)).to(el)
    x[M // 2] = 0

    def run(t):
        ops.quant_rows_f8(t["x"], t["q"], t["scale"])
    got = ab(run, dict(x=x), dict(q=((M, K), torch.uint8), scale=((M,), F32)), pitched=("x", "q"))
    assert got is not None
    a = x.float().abs().amax(1)
    assert torch.equal(got["scale"].cpu(), torch.where(a > 0, a / 448.0, torch.ones_like(a)))       # (one IEEE division: exact)
    deq = got["q"].cpu().view(torch.float8_e4m3fn).float() * got["scale"].cpu().unsqueeze(1)
    assert float(((deq - x.float()).abs() / a.clamp_min(1e-30).unsqueeze(1)).max()) <= 2.0 ** -4        # half an e4m3 ulp at the top


@pytest.mark.parametrize("rows,cols", [(5, 64), (2, 1000)])
def test_softmax_rows(ops, el, rows, cols):
    s = torch.randn(rows, cols, generator=g(1)) * 6.0
    s[0, cols // 2] = 40.0
    got = ab(lambda t: ops.softmax_rows(t["scores"], t["probs"]), dict(scores=s), dict(probs=((rows, cols), el)),
             pitched=("scores", "probs"))
    assert got is not None
    assert parity_err(got["probs"], torch.softmax(s.double(), dim=-1).float()) < tol(3e-3, el)


def test_time_conv_rows_to_nchw(ops, el):
    n, co, H, W = 5, 3, 6, 10
    y = torch.randn(n * H * W, 4, generator=g(2)).to(el)
    wt, b = torch.randn(co, co, 3, generator=g(3)), torch.randn(co, generator=g(4))
    x5 = y.float()[:, :co].reshape(1, n, H, W, co).permute(0, 4, 1, 2, 3)
    ref = F.conv3d(x5, wt[:, :, :, None, None], b, padding=(1, 0, 0))[0].permute(1, 0, 2, 3)
    for dt, bound in ((F32, 1e-5), (el, tol(3e-3, el))):
        got = ab(lambda t: ops.time_conv_rows_to_nchw(t["rows"], n, co, H * W, t["weight"], t["bias"], t["out"]),
                 dict(rows=y, weight=wt, bias=b), dict(out=((n, co, H, W), dt)), pitched=("rows",), W=H * W)
        assert got is not None
        assert parity_err(got["out"], ref, f"time_conv {dt}") < bound


@pytest.mark.parametrize("C", [4, 320])
def test_nchw_to_rows(ops, el, C):
    """channels [c_off, c_off + C) of wider rows: the view IS the column block, everything around it must stay"""
    n, H, W = 3, 8, 12
    x = torch.randn(n, C, H, W, generator=g(1))
    got = ab(lambda t: ops.nchw_to_rows(t["src"], t["dst"], 0), dict(src=x), dict(dst=((n * H * W, C), el)), pitched=("dst",))
    assert got is not None
    assert torch.equal(got["dst"].cpu(), rows_from_nchw(x).to(el))


# ------------------------------------------------------------------------------------------------ backward
def test_wgrad_linear(ops, el):
    M, N, K = 1000, 128, 64
    A, dY = torch.randn(M, K, generator=g(1)).to(el), torch.randn(M, N, generator=g(2)).to(el)
    got = ab(lambda t: ops.gemm_wgrad(t["A"], t["dY"], t["dW"], N=N, cin=K, dbias=t["dbias"], scale=0.75, assign=True),
             dict(A=A, dY=dY), dict(dW=((N, K), F32), dbias=((N,), F32)), pitched=("A", "dY"))
    assert got is not None
    assert parity_err(got["dW"], 0.75 * dY.float().T @ A.float(), "linear wgrad") < 2e-3
    assert parity_err(got["dbias"], 0.75 * dY.float().sum(0), "fused bias grad") < 2e-3


def test_wgrad_conv3x3(ops, el):
    n, cin, cout, H, W = 3, 64, 96, 8, 12
    x, dy = torch.randn(n, cin, H, W, generator=g(1)).to(el), torch.randn(n, cout, H, W, generator=g(2)).to(el)
    w = torch.zeros(cout, cin, 3, 3, requires_grad=True)
    F.conv2d(x.float(), w, None, padding=1).backward(dy.float())
    got = ab(lambda t: ops.gemm_wgrad(t["A"], t["dY"], t["dW"], N=cout, cin=cin, taps=9, mode=1, conv=(H, W, H, W, 1, 0), assign=True),
             dict(A=rows_from_nchw(x), dY=rows_from_nchw(dy)), dict(dW=((cout, 9 * cin), F32)), pitched=("A", "dY"), W=W)
    assert got is not None
    assert parity_err(got["dW"].reshape(cout, 3, 3, cin).permute(0, 3, 1, 2), w.grad, "conv3x3 wgrad") < 2e-3


def test_wgrad_lds_dma(ops, el):
    """csrc/wgrad_pp.hip (M >= 1024, N and Cin multiples of 64): the M = 2048, N = 320, K = 64 case of
    tests/test_backward_gpu.py test_wgrad_lds_dma_kernel"""
    M, N, K = 2048, 320, 64
    A, dY = torch.randn(M, K, generator=g(11)).to(el), torch.randn(M, N, generator=g(12)).to(el)
    got = ab(lambda t: ops.gemm_wgrad(t["A"], t["dY"], t["dW"], N=N, cin=K, dbias=t["dbias"], scale=0.5, assign=True),
             dict(A=A, dY=dY), dict(dW=((N, K), F32), dbias=((N,), F32)), pitched=("A", "dY"))
    assert got is not None
    assert parity_err(got["dW"], 0.5 * dY.float().T @ A.float(), "wgrad_pp") < 2e-3
    assert parity_err(got["dbias"], 0.5 * dY.float().sum(0), "wgrad_pp bias") < 2e-3


@pytest.mark.parametrize("M", [3, 259])
def test_colsum(ops, el, M):
    N = 72
    dY = torch.randn(M, N, generator=g(M)).to(el)
    got = ab(lambda t: (ops.colsum(t["x"], t["db"], scale=0.5), ops.colsum(t["x"], t["dV"], vmode=1, vdiv=1 << 20, vmod=1)),
             dict(x=dY), dict(db=((N,), F32), dV=((1, N), F32)), pitched=("x",), zero=("db", "dV"))
    assert got is not None
    ref = dY.float().sum(0)
    assert parity_err(got["db"], 0.5 * ref, "colsum bias") < 1e-5 and parity_err(got["dV"][0], ref, "colsum row vector") < 1e-5


def test_layernorm_bwd(ops, el):
    M, C, Fr, S = 600, 320, 3, 25
    x, dy = (torch.randn(M, C, generator=g(1)) * 1.3 + 0.2).to(el), torch.randn(M, C, generator=g(2)).to(el)
    gamma, beta = torch.randn(C, generator=g(3), requires_grad=True), torch.randn(C, generator=g(4), requires_grad=True)
    V = torch.randn(Fr, C, generator=g(5))
    xr = x.float().requires_grad_(True)
    F.layer_norm(xr + V[(torch.arange(M) // S) % Fr], (C,), gamma, beta, 1e-5).backward(dy.float())
    got = ab(lambda t: ops.layernorm_bwd(t["x"], t["dy"], t["gamma"], 1e-5, t["dx"], t["dgamma"], t["dbeta"], V=t["V"], vdiv=S, vmod=Fr),
             dict(x=x, dy=dy, gamma=gamma.detach(), V=V), dict(dx=((M, C), el), dgamma=((C,), F32), dbeta=((C,), F32)),
             pitched=("V",), zero=("dgamma", "dbeta"))
    assert got is not None
    assert parity_err(got["dx"], xr.grad, "LN dx") < 4e-3
    assert parity_err(got["dgamma"], gamma.grad, "LN dgamma") < 2e-3 and parity_err(got["dbeta"], beta.grad, "LN dbeta") < 2e-3


# ------------------------------------------------------------------------------------------------ dense-only kernels
@pytest.mark.parametrize("C", [64, 320, 1280])
@pytest.mark.parametrize("with_v", [False, True])
def test_layernorm(ops, el, C, with_v):
    M = 77
    x = (torch.randn(M, C, generator=g(1)) * 1.5 + 0.3).to(el)
    gamma, beta = torch.randn(C, generator=g(2)), torch.randn(C, generator=g(3))
    V = torch.randn(5, C, generator=g(4)) if with_v else None
    got = ab(lambda t: ops.layernorm(t["x"], t["gamma"], t["beta"], 1e-5, t["y"], V=t.get("V"), vdiv=20, vmod=5),
             dict(x=x, gamma=gamma, beta=beta, V=V), dict(y=((M, C), el)), pitched=("V",))
    assert got is not None
    xin = x.float() + (V[(torch.arange(M) // 20) % 5] if with_v else 0.0)
    assert parity_err(got["y"], F.layer_norm(xin, (C,), gamma, beta, 1e-5)) < tol(3e-3, el)
    # a column-sliced view of a dense-only operand is refused by name, not computed on
    wide = torch.zeros(M, C + 8, dtype=el, device=DEV)
    with pytest.raises(ValueError, match="layernorm: x must be contiguous"):
        ops.layernorm(wide[:, :C], gamma.to(DEV), beta.to(DEV), 1e-5, torch.empty(M, C, dtype=el, device=DEV))


def test_groupnorm(ops, el):
    C, H, W, n, ips = 320, 9, 16, 6, 3
    S = H * W
    x = (torch.randn(n, C, H, W, generator=g(1)) * 2 + 0.5).to(el)
    gamma, beta = torch.randn(C, generator=g(2)), torch.randn(C, generator=g(3))
    x5 = x.float().reshape(n // ips, ips, C, H, W).permute(0, 2, 1, 3, 4)
    ref = F.silu(F.group_norm(x5, 32, gamma, beta, 1e-5).permute(0, 2, 1, 3, 4).reshape(n, C, H, W))
    nfl = ops.groupnorm_scratch_floats(n, S, C, ips)
    got = ab(lambda t: ops.groupnorm(t["x"], None, n, S, C, ips, t["gamma"], t["beta"], 1e-5, True, t["y"], t["partials"]),
             dict(x=rows_from_nchw(x), gamma=gamma, beta=beta), dict(y=((n * S, C), el), partials=((nfl,), F32)), W=W)
    assert got is not None
    assert parity_err(got["y"], rows_from_nchw(ref), "groupnorm") < tol(3e-3, el)


def test_groupnorm_concat(ops, el):
    n, C1, C2, H, W = 4, 128, 64, 6, 6
    x1, x2 = torch.randn(n, C1, H, W, generator=g(1)).to(el), (torch.randn(n, C2, H, W, generator=g(2)) * 3).to(el)
    C = C1 + C2
    gamma, beta = torch.randn(C, generator=g(3)), torch.randn(C, generator=g(4))
    ref = F.silu(F.group_norm(torch.cat([x1, x2], 1).float(), 32, gamma, beta, 1e-6))
    nfl = ops.groupnorm_scratch_floats(n, H * W, C, 1)
    got = ab(lambda t: ops.groupnorm(t["x"], t["x2"], n, H * W, C, 1, t["gamma"], t["beta"], 1e-6, True, t["y"], t["partials"]),
             dict(x=rows_from_nchw(x1), x2=rows_from_nchw(x2), gamma=gamma, beta=beta),
             dict(y=((n * H * W, C), el), partials=((nfl,), F32)), W=W)
    assert got is not None
    assert parity_err(got["y"], rows_from_nchw(ref), "groupnorm concat") < tol(3e-3, el)


def test_groupnorm_from_partials(ops, el):
    """The consumer of the GEMM's chunk partials: x and y dense with row guards; the partials buffer is read (chunk part) and
    written (the (mean, rstd) table behind it) in place, so it is an input here and checked against the dense run."""
    H, W, n, cin, cout, ips = 8, 32, 6, 64, 320, 1
    S, M = H * W, n * H * W
    c = conv_case(el, n, cin, cout, H, W)
    out = torch.empty(M, cout, dtype=el, device=DEV)
    part = torch.zeros(ops.groupnorm_fused_scratch_floats(n, S, ips), dtype=F32, device=DEV)
    ops.gemm(c["A"].to(DEV), c["W"].to(DEV), out, N=cout, cin=cin, taps=9, mode=1, conv=(H, W, H, W, 1, 0), bias=c["b"].to(DEV),
             R1=c["R1"].to(DEV), s1=0.5, gn_partials=part)
    torch.cuda.synchronize()
    gamma, beta = torch.randn(cout, generator=g(6)), torch.randn(cout, generator=g(7))
    got = ab(lambda t: ops.groupnorm_from_partials(t["x"], n, S, cout, ips, t["gamma"], t["beta"], 1e-6, True, t["y"], t["partials"]),
             dict(x=out.cpu(), gamma=gamma, beta=beta, partials=part.cpu()), dict(y=((M, cout), el)), W=W)
    assert got is not None
    xo = out.float().cpu().reshape(n, H, W, cout).permute(0, 3, 1, 2)
    ref = F.silu(F.group_norm(xo, 32, gamma, beta, 1e-6))
    assert parity_err(got["y"], rows_from_nchw(ref), "groupnorm_from_partials") < tol(3e-3, el)


def _sdpa_rows(qkv, n_seq, L, C):
    heads = C // 64
    f = qkv.float().reshape(n_seq, L, 3, heads, 64)
    q, k, v = (f[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    return F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(n_seq * L, C)


@pytest.mark.parametrize("n_img,S,C", [(2, 200, 128), (1, 16, 64)])
def test_attention_spatial(ops, el, n_img, S, C):
    """the last image's K / V tail tile reads past the tensor: into poison here"""
    qkv = torch.randn(n_img * S, 3 * C, generator=g(1)).to(el)
    ref = _sdpa_rows(qkv, n_img, S, C)
    got = ab(lambda t: ops.attention_spatial(t["qkv"], t["out"], n_img, S, C), dict(qkv=qkv), dict(out=((n_img * S, C), el)))
    assert got is not None
    assert parity_err(got["out"], ref, "attention_spatial") < tol(5e-3, el)
    got = ab(lambda t: ops.attention_spatial_lse(t["qkv"], t["out"], t["lse"], n_img, S, C), dict(qkv=qkv),
             dict(out=((n_img * S, C), el), lse=((n_img, C // 64, S), F32)))
    assert got is not None
    assert parity_err(got["out"], ref, "attention_spatial_lse") < tol(5e-3, el)
    f = qkv.float().reshape(n_img, S, 3, C // 64, 64)
    q, k = f[:, :, 0].permute(0, 2, 1, 3), f[:, :, 1].permute(0, 2, 1, 3)
    lse = torch.logsumexp((q @ k.transpose(-1, -2)) * 0.125, dim=-1) * math.log2(math.e)
    assert float((got["lse"].cpu() - lse).abs().max()) < 2e-3          # (tests/test_backward_gpu.py's bound)


def test_attention_temporal(ops, el):
    B, Fr, S, C = 1, 3, 7, 64
    qkv = torch.randn(B * Fr * S, 3 * C, generator=g(1)).to(el)
    perm = qkv.reshape(B, Fr, S, 3 * C).permute(0, 2, 1, 3).reshape(B * S * Fr, 3 * C)
    ref = _sdpa_rows(perm, B * S, Fr, C).reshape(B, S, Fr, C).permute(0, 2, 1, 3).reshape(B * Fr * S, C)
    got = ab(lambda t: ops.attention_temporal(t["qkv"], t["out"], B, Fr, S, C), dict(qkv=qkv), dict(out=((B * Fr * S, C), el)))
    assert got is not None
    assert parity_err(got["out"], ref, "attention_temporal") < tol(5e-3, el)


def _attn_grad(qkv, dout, n_seq, L, C):
    x = qkv.float().clone().requires_grad_(True)
    with torch.enable_grad():
        _sdpa_rows(x, n_seq, L, C).backward(dout.float())
    return x.grad


def test_attention_spatial_bwd(ops, el):
    n_img, S, C = 2, 200, 128
    qkv, dout = torch.randn(n_img * S, 3 * C, generator=g(1)).to(el), torch.randn(n_img * S, C, generator=g(2)).to(el)
    ref = _attn_grad(qkv, dout, n_img, S, C)
    out = torch.empty(n_img * S, C, dtype=el, device=DEV)
    lse = torch.empty(n_img, C // 64, S, dtype=F32, device=DEV)
    ops.attention_spatial_lse(qkv.to(DEV), out, lse, n_img, S, C)
    torch.cuda.synchronize()
    got = ab(lambda t: ops.attention_spatial_bwd(t["qkv"], t["o"], t["dout"], t["lse"], t["dqkv"], n_img, S, C),
             dict(qkv=qkv, o=out.cpu(), dout=dout, lse=lse.cpu()), dict(dqkv=((n_img * S, 3 * C), el)))
    assert got is not None
    for i, name in enumerate(("dq", "dk", "dv")):
        assert parity_err(got["dqkv"][:, i * C:(i + 1) * C], ref[:, i * C:(i + 1) * C], name) < 1e-2


def test_attention_temporal_bwd(ops, el):
    B, Fr, S, C = 3, 7, 5, 64
    M = B * Fr * S
    qkv, dout = torch.randn(M, 3 * C, generator=g(1)).to(el), torch.randn(M, C, generator=g(2)).to(el)
    perm = qkv.reshape(B, Fr, S, 3 * C).permute(0, 2, 1, 3).reshape(M, 3 * C)
    dperm = dout.reshape(B, Fr, S, C).permute(0, 2, 1, 3).reshape(M, C)
    ref = _attn_grad(perm, dperm, B * S, Fr, C).reshape(B, S, Fr, 3 * C).permute(0, 2, 1, 3).reshape(M, 3 * C)
    out = torch.empty(M, C, dtype=el, device=DEV)
    ops.attention_temporal(qkv.to(DEV), out, B, Fr, S, C)
    torch.cuda.synchronize()
    got = ab(lambda t: ops.attention_temporal_bwd(t["qkv"], t["o"], t["dout"], t["dqkv"], B, Fr, S, C),
             dict(qkv=qkv, o=out.cpu(), dout=dout), dict(dqkv=((M, 3 * C), el)))
    assert got is not None
    for i, name in enumerate(("dq", "dk", "dv")):
        assert parity_err(got["dqkv"][:, i * C:(i + 1) * C], ref[:, i * C:(i + 1) * C], name) < 1e-2
