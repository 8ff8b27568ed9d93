"""tests/f16_ref.py without a GPU: the fp16 twins of the cached reference builders round the operands to fp16, share nothing with
the bf16 cases other tests use, are computed once, and leave the reference modules as they found them."""
import torch

from tests import autograd_ref as A
from tests import backward_ref as B
from tests.f16_ref import fp16
from tests.parity_utils import parity_err


def test_backward_cases_are_rounded_to_fp16_and_the_bf16_ones_stay():
    bf_case, bf_ref = B.gn_case("w960"), B.gn_reference("w960", True)
    c, ref = fp16(B, "gn_case", "w960"), fp16(B, "gn_reference", "w960", True)
    assert c["x"].dtype == torch.float16 and c["dy"].dtype == torch.float16 and c["gamma"].dtype == torch.float32
    assert B.gn_case("w960") is bf_case and B.gn_reference("w960", True) is bf_ref and bf_case["x"].dtype == torch.bfloat16
    assert fp16(B, "gn_case", "w960") is c and fp16(B, "gn_reference", "w960", True) is ref          # computed once
    assert B.bf(torch.ones(1)).dtype == torch.bfloat16 and hasattr(B.gn_case, "cache_info")
    # the same seeds: the fp16 operands are the bf16 ones before rounding, to bf16 resolution; the references are close, not equal
    assert float((c["x"].float() - bf_case["x"].float()).abs().max()) <= 2.0 ** -8 * float(c["x"].float().abs().max())
    assert torch.equal(c["gamma"], bf_case["gamma"])
    e = parity_err(ref["dx"], bf_ref["dx"])
    assert 0.0 < e < 1e-2
    q = fp16(B, "spatial_case", "large")
    assert q["qkv"].dtype == torch.float16 and bool(torch.isfinite(q["qkv"]).all()) and q["peaked"]
    t = fp16(B, "temporal_reference", "peaked")
    assert all(bool(torch.isfinite(x).all()) for x in t)


def test_autograd_cases_are_rounded_to_fp16():
    cb, rb = A.case_reference("L-zero")
    c, r = fp16(A, "case_reference", "L-zero")
    assert c["A"].dtype == torch.float16 and cb["A"].dtype == torch.bfloat16 and c["weight"].dtype == torch.float32
    assert torch.equal(c["weight"], cb["weight"]) and A.case_reference("L-zero")[0] is cb
    # dY is a 16-bit number of the route's type; the weight is rounded to that type inside the reference
    assert torch.equal(r["dY"], r["dY"].to(torch.float16).double()) and torch.equal(rb["dY"], rb["dY"].to(torch.bfloat16).double())
    assert 0.0 < parity_err(r["dW"], rb["dW"]) < 1e-2
    assert A.bf(torch.ones(1)).dtype == torch.bfloat16
