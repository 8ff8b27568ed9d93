"""The fp64 reference of tests/autograd_ref.py and the comparison tests/test_autograd_ops_gpu.py makes with it, checked without
a GPU: gradcheck of the reference's forward per mode and blend form, its index maps against the expressions
test_ops_gpu.py::test_gemm_plain_epilogue spells out, the signal condition of the mix-factor gradient, and -- with the
reference on both sides -- that every defect the op-level tests exist for (a wrong dA row, a dropped dW tap, dR1 scaled by s2,
a dV table row that misses a row range, dmix off by (1 - a) / a) lands over the bound the GPU test uses, in every case."""
import pytest
import torch

from tests import autograd_ref as R
from tests.parity_utils import parity_err

TOL_EL, TOL_F32, TOL_LORA = 3e-3, 2e-3, 1e-3          # the bounds of tests/test_autograd_ops_gpu.py


def _d(*shape, seed=0, scale=1.0):
    return (scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)).requires_grad_(True)


GRADCHECK = {
    "linear": dict(M=6, cin=3, N=4, spec=dict(mode=0, s_acc=0.7, s1=0.5, s2=-0.25, vmode=1, vdiv=2, vmod=2), R2=True, V=2),
    "linear-vmode2": dict(M=12, cin=2, N=3, spec=dict(mode=0, vmode=2, vdiv=6, vS=2, vmod=3), V=3),
    "conv": dict(M=2 * 3 * 4, cin=2, N=3, spec=dict(mode=1, conv=(3, 4, 3, 4, 1, 0), s_acc=0.8, vmode=1, vdiv=12), V=2),
    "conv-s2": dict(M=2 * 5 * 4, Mo=2 * 3 * 2, cin=2, N=3, spec=dict(mode=1, conv=(5, 4, 3, 2, 2, 0))),
    "conv-up": dict(M=2 * 2 * 3, Mo=2 * 4 * 6, cin=2, N=3, spec=dict(mode=1, conv=(2, 3, 4, 6, 1, 1))),
    "temporal": dict(M=2 * 3 * 2, cin=2, N=2, spec=dict(mode=2, temporal=(3, 2))),
    "blend-res": dict(M=2 * 3 * 2, cin=2, N=2, spec=dict(mode=2, temporal=(3, 2)), blend="res"),
    "blend-sw": dict(M=2 * 3 * 2, cin=2, N=2, spec=dict(mode=2, temporal=(3, 2)), blend="sw"),
    "blend-tr": dict(M=5, cin=3, N=4, spec=dict(mode=0), blend="tr", R2=True),
}


@pytest.mark.parametrize("name", sorted(GRADCHECK))
def test_reference_forward_gradcheck(name):
    c = GRADCHECK[name]
    M, Mo, cin, N, mode = c["M"], c.get("Mo", c["M"]), c["cin"], c["N"], c["spec"]["mode"]
    wshape = {0: (N, cin), 1: (N, cin, 3, 3), 2: (N, cin, 3, 1, 1)}[mode]
    A, W, b, R1 = _d(M, cin, seed=1), _d(*wshape, seed=2), _d(N, seed=3), _d(Mo, N, seed=4)
    R2 = _d(Mo, N, seed=5) if c.get("R2") else None
    V = _d(c["V"], N, seed=6) if c.get("V") else None
    mix = _d(1, seed=7) if c.get("blend") else None
    ins = [t for t in (A, W, b, R1, R2, V, mix) if t is not None]

    def fn(*ts):
        it = iter(ts)
        a, w, bb, r1 = next(it), next(it), next(it), next(it)
        r2 = next(it) if R2 is not None else None
        v = next(it) if V is not None else None
        m = next(it) if mix is not None else None
        return R.forward64(a, w, bb, r1, r2, v, m, blend=c.get("blend"), **c["spec"])
    assert torch.autograd.gradcheck(fn, ins, eps=1e-6, atol=1e-7, rtol=1e-6)
    assert fn(*ins).shape == (Mo, N)


def test_reference_matches_hand_formulas():
    """reference() against gradients written out by hand for nn.Linear (one place where a transposed operand or a lost scalar in
    the reference itself would show), and the bf16 rounding of A / W / dY."""
    g = torch.Generator().manual_seed(5)
    A, W, b = torch.randn(9, 4, generator=g), torch.randn(3, 4, generator=g), torch.randn(3, generator=g)
    R1, V, dY = torch.randn(9, 3, generator=g), torch.randn(3, 3, generator=g), torch.randn(9, 3, generator=g)
    r = R.reference(A, W, b, R1, None, V, dY=dY, s_acc=0.7, s1=0.5, vmode=1, vdiv=2, vmod=3)
    a, w, y, r1 = R.bf(A).double(), R.bf(W).double(), R.bf(dY).double(), R.bf(R1).double()
    idx = torch.tensor([0, 0, 1, 1, 2, 2, 0, 0, 1])
    assert torch.allclose(r["out"], 0.7 * (a @ w.T + b.double()) + 0.5 * r1 + V.double()[idx], atol=1e-12)
    assert torch.allclose(r["dA"], 0.7 * y @ w, atol=1e-12) and torch.allclose(r["dW"], 0.7 * y.T @ a, atol=1e-12)
    assert torch.allclose(r["db"], 0.7 * y.sum(0), atol=1e-12) and torch.allclose(r["dR1"], 0.5 * y, atol=1e-12)
    assert torch.allclose(r["dV"], torch.stack([y[idx == j].sum(0) for j in range(3)]), atol=1e-12)
    assert r["dR2"] is None and r["dmix"] is None


def test_reference_lora_is_the_merged_rounded_weight_with_straight_through_factor_gradients():
    g = torch.Generator().manual_seed(6)
    X, W = torch.randn(11, 8, generator=g), torch.randn(6, 8, generator=g)
    fs = [torch.randn(2, 8, generator=g), torch.randn(3, 2, generator=g), torch.randn(2, 8, generator=g), torch.randn(3, 2, generator=g)]
    dY = torch.randn(11, 6, generator=g)
    r = R.reference(X, W, dY=dY, lora=(2, 1.5), factors=fs, s_acc=0.5)
    x, y = R.bf(X).double(), R.bf(dY).double()
    wm = R.bf(torch.cat([W[:3] + 1.5 * fs[1] @ fs[0], W[3:] + 1.5 * fs[3] @ fs[2]]))
    assert torch.allclose(r["out"], 0.5 * x @ wm.double().T, atol=1e-12) and torch.allclose(r["dA"], 0.5 * y @ wm.double(), atol=1e-12)
    dWm = 0.5 * y.T @ x
    assert torch.allclose(r["dW"], dWm, atol=1e-12)
    for i in range(2):
        assert torch.allclose(r["factors"][2 * i], 1.5 * fs[2 * i + 1].double().T @ dWm[3 * i:3 * i + 3], atol=1e-12)
        assert torch.allclose(r["factors"][2 * i + 1], 1.5 * dWm[3 * i:3 * i + 3] @ fs[2 * i].double().T, atol=1e-12)


def test_index_maps_equal_the_expressions_of_the_forward_tests():
    """vmode 1 / 2 as test_ops_gpu.py::test_gemm_plain_epilogue writes them: (m // vdiv) % vmod and ((m // vdiv) * vS + m % vS)
    % vmod, for that test's own triples and for every (vdiv, vS, vmod) of the op-level cases."""
    m = torch.arange(1000)
    assert torch.equal(R.vindex(1000, 1, 13, 7), (m // 13) % 7)
    assert torch.equal(R.vindex(1000, 2, 50, 7, 10), ((m // 50) * 10 + (m % 10)) % 7)
    seen = 0
    for cid, c in R.CASES.items():
        if not c.get("V"):
            continue
        s, M = c["spec"], c.get("Mo", c["M"])
        m = torch.arange(M)
        vdiv, vmod, vS = s["vdiv"], s.get("vmod", 1 << 30), s.get("vS", 1)
        want = (m // vdiv) % vmod if s["vmode"] == 1 else ((m // vdiv) * vS + (m % vS)) % vmod
        got = R.vindex(M, s["vmode"], vdiv, vmod, vS)
        assert torch.equal(got, want) and int(got.max()) == c["V"] - 1, cid
        seen += 1
    assert seen == 6
    # L-wrap: every table row collects two disjoint row ranges; L-quirk: table row j collects the rows m % 2 == j
    idx = R.vindex(370, 1, 37, 5)
    assert all(len(_ranges(idx, j)) == 2 for j in range(5))
    assert torch.equal(R.vindex(60, 2, 30, 2, 10), torch.arange(60) % 2)


def _ranges(idx, j):
    """maximal runs [lo, hi) of consecutive rows m with idx[m] == j"""
    rows = (idx == j).nonzero().flatten().tolist()
    out = []
    for m in rows:
        if out and out[-1][1] == m:
            out[-1][1] = m + 1
        else:
            out.append([m, m + 1])
    return out


# ------------------------------------------------------------------------------------------------------ the dmix condition
@pytest.mark.parametrize("cid", R.BLEND_CASES)
def test_dmix_signal_condition(cid):
    """|dmix_ref| >= 20 x its bound in every BlendGemm case: a wrong factor or sign cannot hide inside the bound."""
    c, ref = R.case_reference(cid)
    bound, val = R.dmix_bound(ref, c["blend"]), float(ref["dmix"].abs())
    print(f"  {cid}: a {ref['a']:.4f}  dmix_ref {float(ref['dmix']):+.4e}  bound {bound:.3e}  ratio {val / bound:.1f}")
    assert val >= 20.0 * bound


# ------------------------------------------------------------------------------------------------------ sensitivity
def _mut_dA(c, ref):
    d = ref["dA"].clone()
    r = d.shape[0] // 2
    d[r] = ref["dA"][r + 1]
    return parity_err(d, ref["dA"]), TOL_EL


def _mut_dW(c, ref):
    """one tap of a conv's dW zeroed; nn.Linear has one tap: one output row of it instead"""
    d = ref["dW"].clone()
    if c["mode"] == 0:
        d[c["N"] // 2] = 0
    elif c["mode"] == 1:
        d[:, :, 2, 0] = 0
    else:
        d[:, :, 1] = 0          # (the centre frame tap: with one frame per clip the outer ones are zero anyway)
    return parity_err(d, ref["dW"]), TOL_F32


def _scalars(c, ref):
    s = c["spec"]
    if c.get("blend"):
        a = ref["a"]
        return {"res": (1.0, a), "tr": (1.0 - a, a), "sw": (1.0, 1.0)}[c["blend"]]       # (s1, s2) as BlendGemm sets them
    return s.get("s1", 1.0), s.get("s2", 1.0)


def _mut_dR1(c, ref):
    s1, s2 = _scalars(c, ref)
    return parity_err(ref["dR1"] * (s2 / s1), ref["dR1"]), TOL_EL


def _mut_dV(c, ref):
    s = c["spec"]
    idx = R.vindex(ref["dY"].shape[0], s["vmode"], s["vdiv"], s.get("vmod", 1 << 30), s.get("vS", 1))
    j = ref["dV"].shape[0] - 1
    lo, hi = _ranges(idx, j)[-1]
    d = ref["dV"].clone()
    d[j] -= ref["dY"][lo:hi].sum(0)
    return parity_err(d, ref["dV"]), TOL_F32


MUTATIONS = {"dA-row": _mut_dA, "dW-tap": _mut_dW, "dR1-s2": _mut_dR1, "dV-range": _mut_dV}


def _applies(cid, mut):
    c = R.CASES[cid]
    if mut == "dR1-s2":      # (where s1 == s2 the two scalars cannot be told apart: L-wrap, L-quirk*, C-up, G1, B-sw)
        s = c["spec"]
        return bool(c.get("R1")) and (c.get("blend") in ("res", "tr") or (not c.get("blend") and s.get("s1", 1.0) != s.get("s2", 1.0)))
    if mut == "dV-range":
        return bool(c.get("V"))
    return True


SENSITIVITY = [(cid, mut) for cid in R.CASES for mut in MUTATIONS if _applies(cid, mut)]


def test_sensitivity_covers_every_case():
    assert len(R.CASES) == 22
    assert sum(m == "dA-row" for _, m in SENSITIVITY) == 22 and sum(m == "dW-tap" for _, m in SENSITIVITY) == 22
    assert sorted(c for c, m in SENSITIVITY if m == "dR1-s2") == ["B-res-hi", "B-res-lo", "B-tr-hi", "B-tr-lo", "C-long", "L-all"]
    assert sorted(c for c, m in SENSITIVITY if m == "dV-range") == ["C-s1", "L-all", "L-quirk", "L-quirk3", "L-wrap", "T"]


@pytest.mark.parametrize("cid,mut", SENSITIVITY)
def test_comparison_sees_the_defect(cid, mut):
    c, ref = R.case_reference(cid)
    err, bound = MUTATIONS[mut](c, ref)
    print(f"  {cid} {mut}: parity_err {err:.3e} (bound {bound:.0e})")
    assert err > bound


@pytest.mark.parametrize("cid", R.BLEND_CASES)
def test_dmix_check_sees_a_swapped_factor(cid):
    c, ref = R.case_reference(cid)
    a, val = ref["a"], float(ref["dmix"])
    assert abs(val * (1 - a) / a - val) > R.dmix_bound(ref, c["blend"])
    assert abs(-val - val) > R.dmix_bound(ref, c["blend"])


def test_lora_factor_comparison_sees_a_lost_scale():
    """s * s_acc in the factor gradients (G1): dropping s_acc lands over the 1e-3 bound."""
    c, ref = R.case_reference("G1")
    for f in ref["factors"]:
        assert parity_err(f / c["spec"]["s_acc"], f) > TOL_LORA


def test_c_up_two_rounding_figure():
    """C-up rounds dA twice (the GEMM's store on the upsampled grid, then the 2x2 sum's): the error of exactly that against the
    exact pooled gradient, from the reference alone: rel-L2 1.97e-3, max-element 9.8e-4 -- inside the 3e-3 of a once-rounded
    bf16 output, which therefore also bounds C-up's dA on the GPU (no wider bound is needed)."""
    c, ref = R.case_reference("C-up")
    fig = parity_err(R.pooled_twice_rounded(ref, c), ref["dA"], "C-up dA, two roundings (reference only)")
    assert fig < TOL_EL
