"""Every gradient of the two training GEMM Functions (`Gemm`, `BlendGemm`) with fp16 ELEMENTS: the cases of tests/autograd_ref.py
against the same fp64 autograd reference on operands rounded to fp16 instead of bf16 (tests/f16_ref.py).  Rows, upstream gradient
and activation gradients are fp16; parameters are fp32 masters on the device, their packed forms fp16.

The bounds are the bf16 bounds of tests/test_autograd_ops_gpu.py, unchanged (3e-3 for 16-bit results, 2e-3 for fp32 sums, 1e-3 for
LoRA factor gradients, `dmix_bound` with its bf16 rounding term): conditions here, fp16 rounds eight times finer.  A second run
must give the same bits.  The worst figures are printed by the last test; measured on an MI355X: DESIGN 3.9."""
import math

import pytest
import torch

from tests import autograd_ref as R
from tests.f16_ref import fp16
from tests.parity_utils import parity_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = torch.float16
TOL_EL, TOL_F32, TOL_LORA = 3e-3, 2e-3, 1e-3
WORST = {}


@pytest.fixture(scope="module")
def ag(hip_lib):
    from ctrlv_amd import autograd
    return autograd


def _leaf(x, frozen=False):
    if x is None:
        return None
    return x.to(DEV).detach().clone().requires_grad_(not frozen)


def _run(ag, c, dY):
    t = dict(A=_leaf(c["A"]), weight=_leaf(c["weight"], c.get("base_frozen", False)), bias=_leaf(c["bias"]), R1=_leaf(c["R1"]),
             R2=_leaf(c["R2"]), V=_leaf(c["V"]), mix=_leaf(c["mix"]), factors=[_leaf(f) for f in c["factors"]])
    if c.get("blend"):
        spec = ag.GemmSpec(**c["spec"])
        opt = (True,) if c["blend"] == "sw" else ()
        out = ag.BlendGemm.apply(t["A"], t["weight"], t["bias"], t["R1"], t["R2"], t["mix"], spec, *opt)
    else:
        spec = ag.GemmSpec(lora=c.get("lora"), **c["spec"])
        out = ag.Gemm.apply(t["A"], t["weight"], t["bias"], t["R1"], t["R2"], t["V"], spec, *t["factors"])
    out.backward(dY.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), t


def _all_grads(t):
    return [t[k].grad for k in ("A", "weight", "bias", "R1", "R2", "V", "mix") if t[k] is not None and t[k].requires_grad] \
        + [f.grad for f in t["factors"]]


@pytest.mark.parametrize("cid", list(R.CASES))
def test_gemm_gradients_match_fp64_autograd_f16(ag, cid):
    c, ref = fp16(R, "case_reference", cid)
    assert c["A"].dtype == H and c["weight"].dtype == torch.float32
    dY = ref["dY"].to(H)
    out, t = _run(ag, c, dY)
    print()
    assert out.dtype == H
    errs = {"out": (parity_err(out, ref["out"], f"fp16 {cid} out"), TOL_EL)}
    for key, leaf, tol in (("dA", "A", TOL_EL), ("dW", "weight", TOL_F32), ("db", "bias", TOL_F32), ("dR1", "R1", TOL_EL),
                           ("dR2", "R2", TOL_EL), ("dV", "V", TOL_F32)):
        if t[leaf] is None:
            continue
        if key == "dW" and c.get("base_frozen"):
            assert t[leaf].grad is None
            continue
        g = t[leaf].grad
        assert g is not None and g.shape == t[leaf].shape and g.dtype == t[leaf].dtype, key
        errs[key] = (parity_err(g, ref[key], f"fp16 {cid} {key}"), tol)
    for i, f in enumerate(t["factors"]):
        assert f.grad is not None and f.grad.shape == f.shape and f.grad.dtype == torch.float32
        name = f"d{'AB'[i % 2]}_{i // 2}"
        errs[name] = (parity_err(f.grad, ref["factors"][i], f"fp16 {cid} {name}"), TOL_LORA)
    for k, (e, _) in errs.items():
        kind = "LoRA" if k[:2] in ("dA", "dB") and "_" in k else ("16-bit" if k in ("out", "dA", "dR1", "dR2") else "fp32")
        if kind not in WORST or e > WORST[kind][0]:
            WORST[kind] = (e, f"{cid} {k}")
    if c.get("blend"):
        got, want, bound = float(t["mix"].grad), float(ref["dmix"]), R.dmix_bound(ref, c["blend"])
        print(f"  fp16 {cid} dmix: {got:+.6e} vs {want:+.6e}  |diff| {abs(got - want):.3e}  bound {bound:.3e}")
        assert t["mix"].grad.shape == t["mix"].shape and math.isfinite(got)
        assert abs(got - want) <= bound
        rel = abs(got - want) / bound
        if "dmix / bound" not in WORST or rel > WORST["dmix / bound"][0]:
            WORST["dmix / bound"] = (rel, cid)
    bad = {k: v for k, v in errs.items() if not v[0] < v[1]}
    assert not bad, bad
    out2, t2 = _run(ag, c, dY)                                                   # a second run: the same bits
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(_all_grads(t), _all_grads(t2)))


def test_one_weight_serves_both_element_types(ag):
    """A FROZEN base (its packed forms are cached) run in bf16, in fp16 and in bf16 again: each type's output has its own type
    and the bits it has alone -- the caches key on the element type."""
    from tests.parity_utils import parity_err as pe
    c16, ref16 = fp16(R, "case_reference", "G3")
    cbf, refbf = R.case_reference("G3")
    w = torch.nn.Parameter(cbf["weight"].to(DEV), requires_grad=False)
    facs = [f.to(DEV) for f in cbf["factors"]]

    def run(c, dY):
        A = c["A"].to(DEV).requires_grad_(True)
        fl = [torch.nn.Parameter(f.clone(), requires_grad=False) for f in facs]
        out = ag.Gemm.apply(A, w, None, None, None, None, ag.GemmSpec(lora=c["lora"], **c["spec"]), *fl)
        out.backward(dY.to(DEV))
        return out.detach(), A.grad

    a = run(cbf, refbf["dY"].to(torch.bfloat16))
    b = run(c16, ref16["dY"].to(H))
    a2 = run(cbf, refbf["dY"].to(torch.bfloat16))
    b2 = run(c16, ref16["dY"].to(H))
    torch.cuda.synchronize()
    assert a[0].dtype == torch.bfloat16 and a[1].dtype == torch.bfloat16 and b[0].dtype == H and b[1].dtype == H
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1]) and torch.equal(b[0], b2[0]) and torch.equal(b[1], b2[1])
    print()
    assert pe(b[0], ref16["out"], "fp16 after bf16, frozen base: out") < TOL_EL
    assert pe(b[1], ref16["dA"], "fp16 after bf16, frozen base: dA") < TOL_EL
    assert pe(a2[0], refbf["out"], "bf16 after fp16, frozen base: out") < TOL_EL
    assert pe(a2[1], refbf["dA"], "bf16 after fp16, frozen base: dA") < TOL_EL


def test_worst_figures():
    assert R.bf(torch.ones(1)).dtype == torch.bfloat16 and R.case_reference("L-zero")[0]["A"].dtype == torch.bfloat16
    print()
    for kind, (e, where) in WORST.items():
        print(f"  fp16 worst, GEMM gradients, {kind}: {e:.2e} ({where})")
