"""The backward kernels that are not GEMMs with fp16 ELEMENTS (libctrlv_hip_f16.so): every case of tests/backward_ref.py's
GroupNorm, LayerNorm, GEGLU, spatial- and temporal-attention tables, against the same fp64 references on operands rounded to fp16
instead of bf16 (tests/f16_ref.py).

The bounds are the bf16 bounds of tests/test_backward_ops_gpu.py, unchanged -- TOL_DX 4e-3, TOL_PARAM 2e-3, 1e-2 for attention on
plain data and the two measured large-logit bounds (`attn_bound`, from the bf16 rounding-point reference).  fp16 rounds eight
times finer than bf16, so here they are conditions, not measurements.  A second run must give the same bits.  The worst figure of
each family is printed by the last test of the module; measured on an MI355X: DESIGN 3.9 (backward kernels, op level)."""
import pytest
import torch

from tests import backward_ref as R
from tests.f16_ref import fp16
from tests.parity_utils import parity_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = torch.float16
WORST = {}          # family -> {quantity: (figure, case)}


def _note(family, errs, case):
    slot = WORST.setdefault(family, {})
    for k, (e, _) in errs.items():
        if k not in slot or e > slot[k][0]:
            slot[k] = (e, case)


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


def nans(*shape, dtype=H):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def dev(t):
    return None if t is None else t.to(DEV)


def _check(errs):
    bad = {k: v for k, v in errs.items() if not v[0] < v[1]}
    assert not bad, bad


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("cid", list(R.GN_CASES))
def test_groupnorm_backward_f16(ops, cid, silu):
    c, ref = fp16(R, "gn_case", cid), fp16(R, "gn_reference", cid, silu)
    assert c["x"].dtype == H and c["dy"].dtype == H
    C, n, S, ips = c["C"], c["n"], c["S"], c["ips"]
    x, dy, add, gamma, beta = (dev(c[k]) for k in ("x", "dy", "add", "gamma", "beta"))
    part = torch.empty(ops.groupnorm_scratch_floats(n, S, C, ips), dtype=torch.float32, device=DEV)
    ops.groupnorm(x, None, n, S, C, ips, gamma, beta, 1e-5, silu, torch.empty_like(x), part)

    def run():
        dx, dg, db = nans(n * S, C), ref["g0"].to(DEV), ref["b0"].to(DEV)
        ops.groupnorm_bwd(x, dy, n, S, C, ips, part, gamma, beta, silu, dx, dg, db, add=add)
        return dx, dg, db
    dx, dg, db = run()
    print()
    errs = {"dx": (parity_err(dx, ref["dx"], f"fp16 GN {cid} silu={silu} dx"), R.TOL_DX),
            "dgamma": (parity_err(dg, ref["dgamma"], f"fp16 GN {cid} silu={silu} dgamma"), R.TOL_PARAM),
            "dbeta": (parity_err(db, ref["dbeta"], f"fp16 GN {cid} silu={silu} dbeta"), R.TOL_PARAM)}
    _note("GroupNorm", errs, f"{cid} silu={silu}")
    _check(errs)
    assert dx.dtype == H and all(torch.equal(a, b) for a, b in zip(run(), (dx, dg, db)))


@pytest.mark.parametrize("cid", list(R.LN_CASES))
def test_layernorm_backward_f16(ops, cid):
    c, ref = fp16(R, "ln_case", cid), fp16(R, "ln_reference", cid)
    assert c["x"].dtype == H
    M, C = c["M"], c["C"]
    x, dy, add, gamma, beta, V = (dev(c[k]) for k in ("x", "dy", "add", "gamma", "beta", "V"))
    vdiv, vmod = c["vmap"] if c["vmap"] else (1, 1 << 30)

    def run():
        dx, dg, db = nans(M, C), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        ops.layernorm_bwd(x, dy, gamma, 1e-5, dx, dg, db, V=V, vdiv=vdiv, vmod=vmod, add=add)
        return dx, dg, db
    dx, dg, db = run()
    print()
    errs = {"dx": (parity_err(dx, ref["dx"], f"fp16 LN {cid} dx"), R.TOL_DX),
            "dgamma": (parity_err(dg, ref["dgamma"], f"fp16 LN {cid} dgamma"), R.TOL_PARAM),
            "dbeta": (parity_err(db, ref["dbeta"], f"fp16 LN {cid} dbeta"), R.TOL_PARAM)}
    _note("LayerNorm", errs, cid)
    _check(errs)
    assert all(torch.equal(a, b) for a, b in zip(run(), (dx, dg, db)))
    if c["vmap"]:       # the table's gradient, through the autograd Function (column sums of the norm's own dx)
        from ctrlv_amd.autograd import LayerNormFn

        def run_fn():
            leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta, V)]
            LayerNormFn.apply(*leaves, vdiv, vmod).backward(dy)
            return [t.grad for t in leaves]
        g = run_fn()
        errs = {"dx": (parity_err(g[0], ref["dx_norm"], f"fp16 LN {cid} dx (LayerNormFn)"), R.TOL_DX),
                "dV": (parity_err(g[3], ref["dV"], f"fp16 LN {cid} dV"), R.TOL_PARAM)}
        _note("LayerNorm", errs, cid)
        _check(errs)
        assert g[0].dtype == H and torch.equal(g[1], dg) and torch.equal(g[2], db)
        assert all(torch.equal(a, b) for a, b in zip(run_fn(), g))


@pytest.mark.parametrize("cid", list(R.GEGLU_CASES))
def test_geglu_backward_f16(ops, cid):
    c, ref = fp16(R, "geglu_case", cid), fp16(R, "geglu_reference", cid)
    raw, du = dev(c["raw"]), dev(c["du"])
    assert raw.dtype == H and du.dtype == H
    draw = ops.geglu_bwd(raw, du, nans(*raw.shape))
    print()
    errs = {"draw": (parity_err(draw, ref, f"fp16 GEGLU {cid} draw"), R.TOL_DX)}
    _note("GEGLU", errs, cid)
    _check(errs)
    assert torch.equal(ops.geglu_bwd(raw, du, nans(*raw.shape)), draw)


def _spatial(ops, qkv, dout, n_img, S, C):
    out = nans(n_img * S, C)
    lse = nans(n_img, C // 64, S, dtype=torch.float32)
    ops.attention_spatial_lse(qkv, out, lse, n_img, S, C)
    dqkv = nans(n_img * S, 3 * C)
    ops.attention_spatial_bwd(qkv, out, dout, lse, dqkv, n_img, S, C)
    return out, lse, dqkv


@pytest.mark.parametrize("cid", list(R.SPATIAL_CASES))
def test_attention_spatial_backward_f16(ops, cid):
    c = fp16(R, "spatial_case", cid)
    ref_out, ref_grad, ref_lse = fp16(R, "spatial_reference", cid)
    S, C, n = c["S"], c["C"], c["n_img"]
    qkv, dout = dev(c["qkv"]), dev(c["dout"])
    assert qkv.dtype == H
    out, lse, dqkv = _spatial(ops, qkv, dout, n, S, C)
    print()
    bound = R.attn_bound("spatial", cid)                                       # the bf16 bound of this case
    assert parity_err(out, ref_out, f"fp16 spatial {cid} out") < (6e-3 if c["peaked"] else 5e-3)
    assert float((lse.cpu().double() - ref_lse).abs().max()) < 2e-3
    errs = {name: (parity_err(a, b, f"fp16 spatial {cid} {name}"), bound)
            for name, a, b in zip(("dq", "dk", "dv"), R.attn_blocks(dqkv, C), R.attn_blocks(ref_grad, C))}
    _note("spatial attention, large logits" if c["peaked"] else "spatial attention", errs, cid)
    _check(errs)
    assert torch.equal(_spatial(ops, qkv, dout, n, S, C)[2], dqkv)
    if S == 1:
        assert float(dqkv[:, :2 * C].float().abs().max()) == 0.0 and torch.equal(dqkv[:, 2 * C:], dout)
    if n > 1:
        assert torch.equal(_spatial(ops, qkv[:S].contiguous(), dout[:S].contiguous(), 1, S, C)[2], dqkv[:S])


@pytest.mark.parametrize("cid", list(R.TEMPORAL_CASES))
def test_attention_temporal_backward_f16(ops, cid):
    c = fp16(R, "temporal_case", cid)
    ref_out, ref_grad = fp16(R, "temporal_reference", cid)
    B, Fr, S, C = c["B"], c["F"], c["S"], c["C"]
    qkv, dout = dev(c["qkv"]), dev(c["dout"])
    assert qkv.dtype == H

    def run():
        out = nans(B * Fr * S, C)
        ops.attention_temporal(qkv, out, B, Fr, S, C)
        dqkv = nans(B * Fr * S, 3 * C)
        ops.attention_temporal_bwd(qkv, out, dout, dqkv, B, Fr, S, C)
        return out, dqkv
    out, dqkv = run()
    print()
    bound = R.attn_bound("temporal", cid)
    assert parity_err(out, ref_out, f"fp16 temporal {cid} out") < 5e-3
    errs = {name: (parity_err(a, b, f"fp16 temporal {cid} {name}"), bound)
            for name, a, b in zip(("dq", "dk", "dv"), R.attn_blocks(dqkv, C), R.attn_blocks(ref_grad, C))}
    _note("temporal attention, peaked" if c["peaked"] else "temporal attention", errs, cid)
    _check(errs)
    assert torch.equal(run()[1], dqkv)
    if Fr == 1:
        assert float(dqkv[:, :2 * C].float().abs().max()) == 0.0 and torch.equal(dqkv[:, 2 * C:], dout)


def test_the_bf16_references_were_left_alone_and_the_worst_figures():
    """The fp16 twins share nothing with the cached bf16 cases; and the worst figure per family, for DESIGN 3.9."""
    assert R.gn_case("w960")["x"].dtype == torch.bfloat16 and R.spatial_case("S65")["qkv"].dtype == torch.bfloat16
    assert R.bf(torch.ones(1)).dtype == torch.bfloat16
    print()
    for family, slot in WORST.items():
        print(f"  fp16 worst, {family}: " + ", ".join(f"{k} {e:.2e} ({case})" for k, (e, case) in slot.items()))
