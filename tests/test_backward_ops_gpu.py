"""The backward kernels that are not GEMMs -- ctrlv_groupnorm_bwd[_add], ctrlv_layernorm_bwd[_add], ctrlv_geglu_bwd,
ctrlv_attention_spatial_bwd, ctrlv_attention_temporal_bwd -- and the forward GELU table, op by op through ctrlv_amd.ops against
the fp64 references of tests/backward_ref.py on the same bf16-rounded operands, at the shapes where the launchers take another
branch (the case tables there say which).

Per case: outputs start NaN-filled (parameter gradients from the case's initial values: += is the contract), are compared with
`parity_err` (rel-L2 AND the element bound), and a second run must give the same bits (no kernel here uses atomics).  Bounds,
none of them measured on the code under test:
  dx / draw (bf16, rounded once)        4e-3   test_backward_gpu.py's bound for the norm backward
  dgamma / dbeta / dV (fp32 sums)       2e-3   test_backward_gpu.py's kernel-level bound
  dq | dk | dv on plain data            1e-2   test_attention_spatial_backward (P and dS are rounded to bf16 before their MFMAs)
  dq | dk | dv on large / peaked logits 2 x the error of the rounding-point reference (the fp64 formulas with the kernel's own
                                        roundings) against the exact one, measured on the CPU, not below 1e-2: 2.43e-2 for the
                                        spatial large-logit case (1.21e-2 measured), 5.27e-2 for the peaked temporal case
                                        (2.64e-2 measured).  The factor two is the head-room test_attention_spatial_backward_peaked
                                        keeps (1.3e-2 under 2e-2): fp32 statistics and summation order on top of the roundings
  GEGLU forward on the gate grid        3e-3   test_ops_gpu.py::test_gemm_geglu
tests/test_backward_ref_cpu.py shows, with the reference on both sides, that the defects these cases exist for land over the
bounds.  Worst figures measured on an MI355X: DESIGN 3.9 (backward kernels, op level).
"""
import pytest
import torch

from tests import backward_ref as R
from tests.parity_utils import parity_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


def nans(*shape, dtype=BF):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def dev(t):
    return None if t is None else t.to(DEV)


def _check(errs):
    bad = {k: v for k, v in errs.items() if not v[0] < v[1]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("cid", list(R.GN_CASES))
def test_groupnorm_backward(ops, cid, silu):
    """Measured on an MI355X (worst over the 28 runs): dx 1.83e-3 (rows<RPP), dgamma 3.2e-6 and dbeta 3.4e-7 (mean1000-ips3)."""
    c, ref = R.gn_case(cid), R.gn_reference(cid, silu)
    C, n, S, ips = c["C"], c["n"], c["S"], c["ips"]
    x, dy, add, gamma, beta = (dev(c[k]) for k in ("x", "dy", "add", "gamma", "beta"))
    part = torch.empty(ops.groupnorm_scratch_floats(n, S, C, ips), dtype=torch.float32, device=DEV)
    ops.groupnorm(x, None, n, S, C, ips, gamma, beta, 1e-5, silu, torch.empty_like(x), part)       # (the statistics table)

    def run():
        dx, dg, db = nans(n * S, C), ref["g0"].to(DEV), ref["b0"].to(DEV)
        ops.groupnorm_bwd(x, dy, n, S, C, ips, part, gamma, beta, silu, dx, dg, db, add=add)
        return dx, dg, db
    dx, dg, db = run()
    print()
    _check({"dx": (parity_err(dx, ref["dx"], f"GN {cid} silu={silu} dx"), R.TOL_DX),
            "dgamma": (parity_err(dg, ref["dgamma"], f"GN {cid} silu={silu} dgamma"), R.TOL_PARAM),
            "dbeta": (parity_err(db, ref["dbeta"], f"GN {cid} silu={silu} dbeta"), R.TOL_PARAM)})
    assert all(torch.equal(a, b) for a, b in zip(run(), (dx, dg, db)))


# ------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("cid", list(R.LN_CASES))
def test_layernorm_backward(ops, cid):
    """Measured on an MI355X (worst over the 9 cases): dx 1.69e-3 (3x64), dgamma 1.3e-6 (mean30), dbeta 6.2e-8, dV 4.6e-4
    (60x320)."""
    c, ref = R.ln_case(cid), R.ln_reference(cid)
    M, C = c["M"], c["C"]
    x, dy, add, gamma, beta, V = (dev(c[k]) for k in ("x", "dy", "add", "gamma", "beta", "V"))
    vdiv, vmod = c["vmap"] if c["vmap"] else (1, 1 << 30)

    def run():
        dx, dg, db = nans(M, C), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        ops.layernorm_bwd(x, dy, gamma, 1e-5, dx, dg, db, V=V, vdiv=vdiv, vmod=vmod, add=add)
        return dx, dg, db
    dx, dg, db = run()
    print()
    _check({"dx": (parity_err(dx, ref["dx"], f"LN {cid} dx"), R.TOL_DX),
            "dgamma": (parity_err(dg, ref["dgamma"], f"LN {cid} dgamma"), R.TOL_PARAM),
            "dbeta": (parity_err(db, ref["dbeta"], f"LN {cid} dbeta"), R.TOL_PARAM)})
    assert all(torch.equal(a, b) for a, b in zip(run(), (dx, dg, db)))
    if c["vmap"]:       # the table's gradient, through the autograd Function (column sums of the norm's own dx)
        from ctrlv_amd.autograd import LayerNormFn

        def run_fn():
            leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta, V)]
            LayerNormFn.apply(*leaves, vdiv, vmod).backward(dy)
            return [t.grad for t in leaves]
        g = run_fn()
        _check({"dx": (parity_err(g[0], ref["dx_norm"], f"LN {cid} dx (LayerNormFn)"), R.TOL_DX),
                "dV": (parity_err(g[3], ref["dV"], f"LN {cid} dV"), R.TOL_PARAM)})
        assert torch.equal(g[1], dg) and torch.equal(g[2], db)
        assert all(torch.equal(a, b) for a, b in zip(run_fn(), g))


# ------------------------------------------------------------------------------------------------------------ GEGLU
@pytest.mark.parametrize("cid", list(R.GEGLU_CASES))
def test_geglu_backward(ops, cid):
    """Measured on an MI355X (worst over the 5 cases): 1.72e-3 (grid)."""
    c, ref = R.geglu_case(cid), R.geglu_reference(cid)
    raw, du = dev(c["raw"]), dev(c["du"])
    draw = ops.geglu_bwd(raw, du, nans(*raw.shape))
    print()
    assert parity_err(draw, ref, f"GEGLU {cid} draw") < R.TOL_DX
    assert torch.equal(ops.geglu_bwd(raw, du, nans(*raw.shape)), draw)


@pytest.mark.parametrize("tile", [0, 1, 5, 12])
def test_geglu_forward_on_the_gate_grid(ops, tile):
    """gelu_phi_tab (1024 knots on [-5.12, 5.12], index clamped) with exact gates on, beside and far past both ends and the
    +-5 clamp of the polynomial it is filled from: the automatic tile, the 2-stage 128 x 128 kernel, a ping-pong tile and the
    16x16x32 core.  Measured on an MI355X: 1.66e-3, the same for every tile."""
    from ctrlv_amd import packing
    t = R.gelu_table_case()
    Wp, bp = packing.pack_geglu(t["W"], t["bias"])
    out = nans(t["M"], t["I"])
    ops.gemm(dev(t["A"]), dev(Wp), out, N=2 * t["I"], cin=t["K"], bias=dev(bp), geglu=1, tile=tile)
    print()
    assert parity_err(out, t["ref"], f"GEGLU forward on the gate grid, tile {tile}") < 3e-3


# ------------------------------------------------------------------------------------------------------------ attention
def _spatial(ops, qkv, dout, n_img, S, C):
    """forward (out, lse) + backward on the device; dqkv starts NaN-filled"""
    out = nans(n_img * S, C)
    lse = nans(n_img, C // 64, S, dtype=torch.float32)
    ops.attention_spatial_lse(qkv, out, lse, n_img, S, C)
    dqkv = nans(n_img * S, 3 * C)
    ops.attention_spatial_bwd(qkv, out, dout, lse, dqkv, n_img, S, C)
    return out, lse, dqkv


@pytest.mark.parametrize("cid", list(R.SPATIAL_CASES))
def test_attention_spatial_backward(ops, cid):
    """Measured on an MI355X: plain data 2.55e-3 at most (S33 dv; bound 1e-2); the large-logit case 1.21e-2 (dq, dk; bound 2.43e-2;
    its rounding-point reference alone: 1.21e-2); lse within 1.5e-5 of the reference everywhere."""
    c = R.spatial_case(cid)
    ref_out, ref_grad, ref_lse = R.spatial_reference(cid)
    S, C, n = c["S"], c["C"], c["n_img"]
    qkv, dout = dev(c["qkv"]), dev(c["dout"])
    out, lse, dqkv = _spatial(ops, qkv, dout, n, S, C)
    print()
    bound = R.attn_bound("spatial", cid)
    assert parity_err(out, ref_out, f"spatial {cid} out") < (6e-3 if c["peaked"] else 5e-3)      # (test_ops_gpu.py's bounds)
    d_lse = float((lse.cpu().double() - ref_lse).abs().max())
    print(f"  spatial {cid} lse: max |diff| {d_lse:.3e} (|lse| up to {float(ref_lse.abs().max()):.1f})")
    assert d_lse < 2e-3                                                                          # (test_backward_gpu.py's bound)
    _check({name: (parity_err(a, b, f"spatial {cid} {name}"), bound)
            for name, a, b in zip(("dq", "dk", "dv"), R.attn_blocks(dqkv, C), R.attn_blocks(ref_grad, C))})
    assert torch.equal(_spatial(ops, qkv, dout, n, S, C)[2], dqkv)
    if S == 1:          # one key: the softmax is constant
        assert float(dqkv[:, :2 * C].float().abs().max()) == 0.0 and torch.equal(dqkv[:, 2 * C:], dout)
    if n > 1:           # the grid is per image, nothing is reduced across images: image 0 alone gives the same bits
        alone = _spatial(ops, qkv[:S].contiguous(), dout[:S].contiguous(), 1, S, C)[2]
        assert torch.equal(alone, dqkv[:S])


def test_attention_spatial_backward_keeps_the_next_image_out_of_a_ragged_tile(ops):
    """S = 65: image 0's second tile holds one valid row, and image 1 -- at magnitude 1e4 -- lies right behind it.  Image 0's
    gradients are those of the plain case, to the bit."""
    cid = R.SPATIAL_LEAK_CASE
    c, ref_grad = R.spatial_case(cid), R.spatial_reference(cid)[1]
    S, C = c["S"], c["C"]
    assert c["n_img"] == 2 and S % 64 == 1
    qkv, dout = dev(c["qkv"]).clone(), dev(c["dout"]).clone()
    plain = _spatial(ops, qkv, dout, 2, S, C)[2]
    qkv[S:] = (qkv[S:].float() * 1e4).to(BF)
    dout[S:] = (dout[S:].float() * 1e4).to(BF)
    dqkv = _spatial(ops, qkv, dout, 2, S, C)[2]
    print()
    _check({name: (parity_err(a, b, f"spatial {cid}, image 0 in front of 1e4 x image 1: {name}"), R.TOL_ATTN)
            for name, a, b in zip(("dq", "dk", "dv"), R.attn_blocks(dqkv[:S], C), R.attn_blocks(ref_grad[:S], C))})
    assert torch.equal(dqkv[:S], plain[:S])


@pytest.mark.parametrize("cid", list(R.TEMPORAL_CASES))
def test_attention_temporal_backward(ops, cid):
    """Measured on an MI355X: plain data 4.28e-3 at most (F2 dk; bound 1e-2); the peaked case 2.64e-2 (dq; bound 5.27e-2; its
    rounding-point reference alone: 2.64e-2)."""
    c = R.temporal_case(cid)
    ref_out, ref_grad = R.temporal_reference(cid)
    B, Fr, S, C = c["B"], c["F"], c["S"], c["C"]
    qkv, dout = dev(c["qkv"]), dev(c["dout"])

    def run():
        out = nans(B * Fr * S, C)
        ops.attention_temporal(qkv, out, B, Fr, S, C)
        dqkv = nans(B * Fr * S, 3 * C)
        ops.attention_temporal_bwd(qkv, out, dout, dqkv, B, Fr, S, C)
        return out, dqkv
    out, dqkv = run()
    print()
    bound = R.attn_bound("temporal", cid)
    assert parity_err(out, ref_out, f"temporal {cid} out") < 5e-3
    _check({name: (parity_err(a, b, f"temporal {cid} {name}"), bound)
            for name, a, b in zip(("dq", "dk", "dv"), R.attn_blocks(dqkv, C), R.attn_blocks(ref_grad, C))})
    assert torch.equal(run()[1], dqkv)
    if Fr == 1:         # one key: dq and dk are exactly zero, dv is dout
        assert float(dqkv[:, :2 * C].float().abs().max()) == 0.0 and torch.equal(dqkv[:, 2 * C:], dout)
