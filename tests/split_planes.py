"""Host model of the SPLIT trunk's two planes (csrc/common.h split_lo8 / unpack_lo4) and the per-element
checks the split-aware kernels are held to.  Not a test module: tests/test_split_planes_cpu.py tests it, the GPU tests
use it.

A split tensor stores v as hi = rne_fp16(v) and lo = rne_e5m2(v - hi).  The residual v - hi is exact in fp32, so both
planes are a function of v alone: for a v known exactly, `expect_split_exact` gives the one correct pair of planes.  For
a v known only to within a reference's uncertainty, `check_split` states what the pair must satisfy element by element.
"""
import torch

EL = torch.float16
LO = torch.float8_e5m2          # one byte per element: fp16's sign, exponent and two top mantissa bits

E5M2_MIN_NORMAL_EXP = -14       # fp16's exponent range: 2^-14 is the smallest normal value
E5M2_MAN_BITS = 2
E5M2_MAX = 57344.0              # 1.75 * 2^15


def e5m2_rne(x):
    """x (any float dtype) -> the nearest e5m2 value as float64: round to nearest, ties to an even mantissa; below 2^-14
    the values are the subnormals k * 2^-16 (k = 0..3), so |x| < 2^-17 gives zero, |x| = 2^-17 ties to zero and
    2^-17 < |x| < 2^-16 gives 2^-16; overflow (|x| >= 1.875 * 2^15, the midpoint above the largest finite value) gives inf.
    NaN stays NaN.  This is the conversion the kernels' v_cvt_pk_bf8_f32 performs (tests/test_split_exact_gpu.py checks it
    byte for byte) and the one torch's float8_e5m2 cast performs."""
    x = x.double()
    a = x.abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** E5M2_MIN_NORMAL_EXP))).clamp_min(E5M2_MIN_NORMAL_EXP)
    q = torch.exp2(e - E5M2_MAN_BITS)                 # spacing of the binade (the subnormals share the lowest one's)
    r = torch.round(a / q) * q                        # torch.round: half to even; a / q and the product are exact
    r = torch.where(r > E5M2_MAX, torch.full_like(r, float("inf")), r)
    r = torch.where(torch.isnan(x), x, torch.copysign(r, x))
    return r


def e5m2_bytes(v):
    """e5m2-representable float64 values -> their bytes (uint8): the top byte of the fp16 encoding."""
    return (v.to(EL).view(torch.int16) >> 8).to(torch.uint8)


def lo_bytes(lo):
    return lo.view(torch.uint8) if lo.dtype == LO else lo


def decode_lo(lo):
    """lo plane (e5m2 tensor or its bytes) -> float64"""
    return lo_bytes(lo).view(LO).double()


def expect_split_exact(v):
    """Expected (hi fp16, lo uint8) planes for values v that are known EXACTLY (float64 holding fp32-representable values:
    the kernel's fp32 result has no rounding of its own)."""
    v = v.double()
    assert torch.equal(v.float().double(), v), "expect_split_exact: values must be exact in fp32"
    hi = v.float().to(EL)             # (exact in fp32, so the one rounding is to fp16: round to nearest even)
    res = v - hi.double()             # exact
    return hi, e5m2_bytes(e5m2_rne(res))


def fp16_ulp(hi):
    """ulp of fp16 values (as float64): 2^(e - 10) for a normal value, 2^-24 below 2^-14."""
    a = hi.double().abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def _where(mask, shape):
    idx = torch.nonzero(mask.reshape(shape))[0].tolist()
    if len(idx) == 1:
        return f"element {idx[0]} (32-element block {idx[0] // 32})"
    r, c = idx[-2], idx[-1]
    lead = f"{tuple(idx[:-2])} " if len(idx) > 2 else ""
    return f"{lead}row {r}, column {c} (32-column block {c // 32}, 256-row tile {r // 256})"


def check_split(hi, lo, v64, err64=None, where="split planes", min_tight=0.95):
    """Per-element check of a kernel's split output (hi fp16, lo e5m2 / bytes) against a reference v64 (float64) whose own
    uncertainty is err64 (float64, per element or scalar; None = exact):
        |hi - v64|      <= ulp(hi) / 2 + err                       (hi is v rounded to fp16)
        |hi + lo - v64| <= 2^-3 |v64 - hi| + 2^-17 + 1.125 err     (lo is v - hi rounded to e5m2: 3 significant bits,
                                                                     absolute 2^-17 in the subnormals)
    The 1.125: the kernel rounds v32 - hi, and |v32 - hi| <= |v64 - hi| + err.  err must stay below ulp(hi) / 16 on at least
    `min_tight` of the elements -- a reference too loose to see the lo plane makes the check vacuous, and that is an error
    of the test.  On failure: the first failing element, its 32-column block and its 256-row tile."""
    hi_c, lo_c = hi.detach().cpu(), lo_bytes(lo.detach().cpu())
    assert hi_c.dtype == EL and lo_c.dtype == torch.uint8 and hi_c.shape == lo_c.shape == v64.shape, where
    h, l, v = hi_c.double(), decode_lo(lo_c), v64.double().cpu()
    err = torch.zeros_like(v) if err64 is None else torch.as_tensor(err64, dtype=torch.float64).cpu().expand_as(v)
    ulp = fp16_ulp(hi_c)
    tight = (err < ulp / 16).double().mean().item()
    assert tight >= min_tight, f"{where}: reference uncertainty too large to see the lo plane ({tight:.3f} tight elements)"
    assert torch.isfinite(h).all() and torch.isfinite(l).all(), f"{where}: non-finite plane at {_where(~(torch.isfinite(h) & torch.isfinite(l)), v.shape)}"
    bad_hi = (h - v).abs() > ulp / 2 + err
    if bad_hi.any():
        raise AssertionError(f"{where}: hi plane is not v rounded to fp16 at {_where(bad_hi, v.shape)} "
                             f"({int(bad_hi.sum())} elements)")
    bad_lo = (h + l - v).abs() > 2.0 ** -3 * (v - h).abs() + 2.0 ** -17 + 1.125 * err
    if bad_lo.any():
        raise AssertionError(f"{where}: lo plane is not v - hi rounded to e5m2 at {_where(bad_lo, v.shape)} "
                             f"({int(bad_lo.sum())} elements)")


def assert_planes_equal(hi, lo, hi_exp, lo_exp, where="split planes"):
    """Bit-exact comparison of both planes; on failure: the first differing element, its block and tile."""
    hi_c, lo_c = hi.detach().cpu(), lo_bytes(lo.detach().cpu())
    for name, got, exp in (("hi", hi_c.view(torch.int16), hi_exp.view(torch.int16)), ("lo", lo_c, lo_bytes(lo_exp))):
        bad = got != exp
        if bad.any():
            raise AssertionError(f"{where}: {name} plane differs at {_where(bad, got.shape)} ({int(bad.sum())} elements)")


def split(v):
    """fp32 tensor -> (hi fp16, lo e5m2) planes the way the kernels store them."""
    v = v.float()
    hi = v.to(EL)
    lo = e5m2_bytes(e5m2_rne(v.double() - hi.double())).view(LO)
    return hi, lo
