"""Every gradient of the two training GEMM Functions (ctrlv_amd/autograd.py: `Gemm`, `BlendGemm` -> `gemm_grads`,
`_epilogue_grads`), op by op, against the fp64 autograd reference of tests/autograd_ref.py on the same rounded operands.

One call per case, every differentiable input requires grad (parameters are fp32 masters on the device), a bf16 upstream
gradient dY = bf16(out_ref + 0.5 noise) is backpropagated, and the forward output and each gradient are compared with
`parity_err` (rel-L2 AND the element bound).  Bounds, none of them measured on the code under test:
  bf16 results (out, dA, dR1, dR2)   3e-3   test_ops_gpu.py's bound for a bf16 output rounded once from fp32 accumulation; dgrad
                                            is that kernel.  C-up's dA is rounded twice (the GEMM's store, then the 2x2 sum's):
                                            the reference alone puts those two roundings at rel-L2 1.97e-3 / max-elem 9.8e-4
                                            (tests/test_autograd_ref_cpu.py::test_c_up_two_rounding_figure), inside 3e-3 too
  fp32 results (dW, db, dV)          2e-3   test_backward_gpu.py's kernel-level bound
  LoRA factor gradients              1e-3   test_lora_gpu.py's bound on ops.lora_grad
  dmix                               |dmix - ref| <= scale * (2^-9 + 2^-12) * sum |dY * out_ref|, scale = a (res and transformer
                                     form) or 1 - a (switched): `out` is rounded once to bf16 before dot_diff forms
                                     sum dY (out - xs); |ref| >= 20 x that bound in every case (asserted on the CPU)
tests/test_autograd_ref_cpu.py shows, with the reference on both sides, that a wrong dA row, a dropped dW tap, swapped
s1 / s2, a dV table row missing a row range and dmix off by (1 - a) / a each land over these bounds in every case.
"""
import math

import pytest
import torch

from tests import autograd_ref as R
from tests.parity_utils import parity_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_EL, TOL_F32, TOL_LORA = 3e-3, 2e-3, 1e-3


@pytest.fixture(scope="module")
def ag(hip_lib):
    from ctrlv_amd import autograd
    return autograd


def _leaf(x, frozen=False):
    if x is None:
        return None
    return x.to(DEV).detach().clone().requires_grad_(not frozen)


def _run(ag, c, dY, dY_view=None):
    """One forward + backward of the case on the device.  Returns (out, dict of the leaves)."""
    t = dict(A=_leaf(c["A"]), weight=_leaf(c["weight"], c.get("base_frozen", False)), bias=_leaf(c["bias"]), R1=_leaf(c["R1"]),
             R2=_leaf(c["R2"]), V=_leaf(c["V"]), mix=_leaf(c["mix"]), factors=[_leaf(f) for f in c["factors"]])
    if c.get("blend"):
        spec = ag.GemmSpec(**c["spec"])
        opt = (True,) if c["blend"] == "sw" else ()
        out = ag.BlendGemm.apply(t["A"], t["weight"], t["bias"], t["R1"], t["R2"], t["mix"], spec, *opt)
    else:
        spec = ag.GemmSpec(lora=c.get("lora"), **c["spec"])
        out = ag.Gemm.apply(t["A"], t["weight"], t["bias"], t["R1"], t["R2"], t["V"], spec, *t["factors"])
    out.backward(dY_view if dY_view is not None else dY.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), t


def _all_grads(t):
    return [t[k].grad for k in ("A", "weight", "bias", "R1", "R2", "V", "mix") if t[k] is not None] + [f.grad for f in t["factors"]]


def _dgrad_splitk_slices(ag, c):
    """K slices of the dgrad launch gemm_grads builds for this conv case (its own descriptor: the gradient rows -- zero-inserted
    to the input grid for stride 2 -- as A, the role-swapped weight, N and cin exchanged, stride 1)."""
    from ctrlv_amd import ops
    H, W, Ho, Wo, stride, up = c["spec"]["conv"]
    N, cin = c["N"], c["cin"]
    npad = (N + 63) // 64 * 64
    rows = c["M"] if stride == 2 else c["Mo"]
    dYd = torch.zeros(rows, npad, dtype=torch.bfloat16, device=DEV)
    wt = ops.pack_weight(c["weight"].to(DEV), 1)
    dA = torch.empty(rows, cin, dtype=torch.bfloat16, device=DEV)
    return ops.gemm_splitk_slices(dYd, wt, dA, N=(cin + 31) // 32 * 32, cin=npad, taps=9, mode=1, conv=(H, W, H, W, 1, 0),
                                  s_acc=float(c["spec"].get("s_acc", 1.0)))


@pytest.mark.parametrize("cid", list(R.CASES))
def test_gemm_gradients_match_fp64_autograd(ag, cid):
    """Worst figures measured on an MI355X are listed in DESIGN 3.9 (op-level gradient parity)."""
    c, ref = R.case_reference(cid)
    if cid.startswith("C-long"):
        assert _dgrad_splitk_slices(ag, c) >= 2                       # the dgrad launch takes the split-contraction plan
    out, t = _run(ag, c, ref["dY"].to(torch.bfloat16))
    print()
    errs = {"out": (parity_err(out, ref["out"], f"{cid} out"), TOL_EL)}
    for key, leaf, tol in (("dA", "A", TOL_EL), ("dW", "weight", TOL_F32), ("db", "bias", TOL_F32), ("dR1", "R1", TOL_EL),
                           ("dR2", "R2", TOL_EL), ("dV", "V", TOL_F32)):
        if t[leaf] is None:
            continue
        if key == "dW" and c.get("base_frozen"):
            assert t[leaf].grad is None                                # a frozen base gets no gradient
            continue
        g = t[leaf].grad
        assert g is not None and g.shape == t[leaf].shape and g.dtype == t[leaf].dtype, key
        errs[key] = (parity_err(g, ref[key], f"{cid} {key}"), tol)
    for i, f in enumerate(t["factors"]):
        assert f.grad is not None and f.grad.shape == f.shape and f.grad.dtype == torch.float32
        name = f"d{'AB'[i % 2]}_{i // 2}"
        errs[name] = (parity_err(f.grad, ref["factors"][i], f"{cid} {name}"), TOL_LORA)
    if c.get("blend"):
        got, want, bound = float(t["mix"].grad), float(ref["dmix"]), R.dmix_bound(ref, c["blend"])
        print(f"  {cid} dmix: {got:+.6e} vs {want:+.6e}  |diff| {abs(got - want):.3e}  bound {bound:.3e}  "
              f"(|ref| / bound {abs(want) / bound:.0f})")
        assert t["mix"].grad.shape == t["mix"].shape and math.isfinite(got)
        assert abs(got - want) <= bound
    bad = {k: v for k, v in errs.items() if not v[0] < v[1]}
    assert not bad, bad


def test_non_contiguous_upstream_gradient_gives_the_same_bits(ag):
    """L-all with dY handed in as a column slice of a wider buffer: every gradient bit for bit as in the contiguous run (the
    row-vector gradient included: its row groups of 111 rows take the ordered per-table-row sums, not atomics)."""
    c, ref = R.case_reference("L-all")
    dY = ref["dY"].to(torch.bfloat16).to(DEV)
    wide = torch.randn(dY.shape[0], dY.shape[1] + 40, device=DEV).to(torch.bfloat16)
    wide[:, 24:24 + dY.shape[1]] = dY
    view = wide[:, 24:24 + dY.shape[1]]
    assert not view.is_contiguous() and torch.equal(view, dY)
    out0, t0 = _run(ag, c, dY)
    out1, t1 = _run(ag, c, dY, dY_view=view)
    assert torch.equal(out0, out1)
    g0, g1 = _all_grads(t0), _all_grads(t1)
    assert len(g0) == 6 and all(a is not None and torch.equal(a, b) for a, b in zip(g0, g1))


def test_tiny_lora_step_is_bit_reproducible(hip_lib):
    """The stage-1 step with a LoRA adapter at the tiny configuration and B = 2 (the shape of
    test_lora_gpu.py::test_unet_train_step_with_lora_matches_oracle), HIP side only, twice in one process with the gradients
    cleared in between: the loss and every factor gradient are equal bit for bit."""
    from ctrlv_amd.models import UNetSpatioTemporalConditionModel
    from ctrlv_amd.training import unet_train_step
    from ctrlv_amd.utils import random_init_
    from tests.test_lora_gpu import _cfg, _random_B
    from tests.test_train_unet_gpu import _batch
    config = dict(sample_size=16, block_out_channels=(64, 128, 128, 128), addition_time_embed_dim=32,
                  projection_class_embeddings_input_dim=96, cross_attention_dim=64, num_attention_heads=(1, 2, 2, 2),
                  num_frames=3)
    hu = UNetSpatioTemporalConditionModel(**config)
    random_init_(hu, seed=3)
    with torch.no_grad():
        for p in hu.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    hu.to(device=DEV, dtype=torch.float32).eval()
    hu.add_adapter(_cfg(r=4, alpha=8))
    hu.to(device=DEV)
    _random_B(hu)
    b = {k: v.to(DEV) for k, v in _batch(config, 2, 3, 16, 16, drop=(0,)).items()}
    params = [(n, p) for n, p in hu.named_parameters() if ".lora_" in n]
    assert len(params) == 512 and all(p.requires_grad for _, p in params)
    runs = []
    for _ in range(2):
        for _, p in params:
            p.grad = None
        loss = unet_train_step(hu, b)
        torch.cuda.synchronize()
        runs.append((loss.clone(), [p.grad.clone() for _, p in params]))
    (l0, g0), (l1, g1) = runs
    assert math.isfinite(float(l0)) and all(bool(torch.isfinite(g).all()) for g in g0)
    assert sum(float(g.abs().max()) > 0 for g in g0) >= 512 - 128          # (all but attn2.to_q / to_k: exact zeros)
    differ = [n for (n, _), a, c in zip(params, g0, g1) if not torch.equal(a, c)]
    print(f"\n  loss {float(l0):.6f} / {float(l1):.6f}; factor gradients that differ between the runs: {len(differ)} of {len(params)}")
    assert torch.equal(l0, l1) and not differ, differ[:8]
