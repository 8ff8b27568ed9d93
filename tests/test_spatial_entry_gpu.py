"""The fused entry of the spatial transformer block at C = 320 (csrc/spatial_entry_fused.hip): GroupNorm apply, proj_in,
LayerNorm (norm1) and the q|k|v projection in one launch, in both element libraries.

Every case is checked
  * against fp32 PyTorch with the four launches' rounding points -- el(GN(x)) -> el(. @ el(W_in).T + b) = h0, el(LN(h0)) ->
    q|k|v with the q block scaled before its one rounding -- at parity_err < tol(5e-3), and against the four launches run
    through `ops` at rel_l2 < tol(3e-3) (the bounds of test_temporal_fused for the same structure);
  * h0 bit for bit against the four-launch h0: the proj_in chains keep ctrlv_gemm's K order, start from the bias like its
    accumulators, the GroupNorm coefficients are formed by gn_apply_kernel's own expression and the normalised rows exist
    as fp32 values before their rounding (fp16: fma + convert, not the single-rounding v_fma_mix*_f16);
  * two runs into NaN-filled outputs are equal; image 0 alone equals rows [:S] of the batched run; nothing outside the M rows
    of h0 / q|k|v is written (guard bands, pitched views).
The GroupNorm input carries a per-channel offset of several sigma so that the b coefficient matters.  (n_img, S): one row group;
(2, 64); (3, 96): M = 288 -- a 256-row workgroup tile straddles images and the last tile is ragged; (2, 160).  One more case
takes the statistics from the chunk partials a producer GEMM wrote."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.guarded import check_written_only_inside, guarded
from tests.parity_utils import parity_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ELS = [torch.bfloat16, torch.float16]
C = 320
CASES = [(1, 32), (2, 64), (3, 96), (2, 160)]


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


@pytest.fixture(scope="module")
def layer(el, ops):
    """the block's parameters, packed once per element type"""
    from ctrlv_amd import packing
    with packing.element_dtype(el):
        w_in = torch.randn(C, C, generator=g(1)) / math.sqrt(C)
        wq, wk, wv = (torch.randn(C, C, generator=g(2 + i)) / math.sqrt(C) for i in range(3))
        p = dict(w_in=w_in, wqkv=torch.cat([wq, wk, wv], 0), b_in=torch.randn(C, generator=g(5)),
                 gn_g=torch.randn(C, generator=g(6)), gn_b=torch.randn(C, generator=g(7)),
                 ln_g=torch.randn(C, generator=g(8)), ln_b=torch.randn(C, generator=g(9)))
        p["win_p"] = packing.pack_linear(w_in).to(DEV)
        p["wqkv_p"] = packing.pack_qkv(wq, wk, wv).to(DEV)
        assert p["win_p"].dtype == el and tuple(p["win_p"].shape) == (C, C) and tuple(p["wqkv_p"].shape) == (3 * C, C)
        p["wf"] = ops.spatial_entry_fused_pack(p["win_p"], p["wqkv_p"])
        for k in ("b_in", "gn_g", "gn_b", "ln_g", "ln_b"):
            p[k + "_d"] = p[k].to(DEV)
    return p


def test_pack_matches_the_layout_statement(ops, el, layer):
    """the device pack kernel writes packing.spatial_entry_fragments' layout, element for element"""
    from ctrlv_amd import packing
    want = packing.spatial_entry_fragments(layer["win_p"], layer["wqkv_p"])
    assert layer["wf"].numel() == want.numel() == 40 * 20 * 512
    assert torch.equal(layer["wf"].cpu().view(torch.int16), want.view(torch.int16))


def reference(x, p, n_img, S, el):
    """fp32 PyTorch with the four launches' rounding points; x: element-type rows [n_img * S, C] on the host"""
    r = lambda t: t.to(el).float()       # noqa: E731
    xi = x.float().reshape(n_img, S, C).permute(0, 2, 1)
    y = r(F.group_norm(xi, 32, p["gn_g"], p["gn_b"], 1e-6).permute(0, 2, 1).reshape(n_img * S, C))
    h0 = r(y @ r(p["w_in"]).T + p["b_in"])
    t = r(F.layer_norm(h0, (C,), p["ln_g"], p["ln_b"], 1e-5))
    qkv = t @ r(p["wqkv"]).T
    qkv[:, :C] *= 0.125 * 1.44269504088896340736
    return h0, r(qkv)


def four_launches(ops, p, xd, n_img, S, el, stats_from=None):
    M = n_img * S
    tt = torch.empty(M, C, dtype=el, device=DEV)
    if stats_from is None:
        part = torch.empty(ops.groupnorm_scratch_floats(n_img, S, C, 1), dtype=torch.float32, device=DEV)
        ops.groupnorm(xd, None, n_img, S, C, 1, p["gn_g_d"], p["gn_b_d"], 1e-6, False, tt, part)
    else:
        ops.groupnorm_from_partials(xd, n_img, S, C, 1, p["gn_g_d"], p["gn_b_d"], 1e-6, False, tt, stats_from)
    h0 = torch.empty(M, C, dtype=el, device=DEV)
    ops.gemm(tt, p["win_p"], h0, N=C, cin=C, bias=p["b_in_d"])
    ops.layernorm(h0, p["ln_g_d"], p["ln_b_d"], 1e-5, tt)
    qkv = torch.empty(M, 3 * C, dtype=el, device=DEV)
    ops.gemm(tt, p["wqkv_p"], qkv, N=3 * C, cin=C, n_scale2=C, s_acc2=ops.Q_PRESCALE)
    return h0, qkv


def fused(ops, p, xd, stats, n_img, S, h0, qkv):
    gn, ln = (p["gn_g_d"], p["gn_b_d"]), (p["ln_g_d"], p["ln_b_d"], 1e-5)
    assert ops.spatial_entry_fused_serves(xd, p["wf"], stats, gn, ln, h0, qkv, n_img, S, bias_in=p["b_in_d"])
    ops.spatial_entry_fused(xd, p["wf"], stats, gn, ln, h0, qkv, n_img, S, bias_in=p["b_in_d"])


def nan_outputs(M, el):
    return (torch.full((M, C), float("nan"), dtype=el, device=DEV), torch.full((M, 3 * C), float("nan"), dtype=el, device=DEV))


def check_against_references(ops, p, x, xd, h0, qkv, n_img, S, el, old, what):
    h0_ref, qkv_ref = reference(x, p, n_img, S, el)
    e_h, e_q = parity_err(h0, h0_ref, what + " h0"), parity_err(qkv, qkv_ref, what + " qkv")
    r_h = rel_l2(h0.float().cpu(), old[0].float().cpu())
    r_q = rel_l2(qkv.float().cpu(), old[1].float().cpu())
    print(f"  {what}: parity h0 {e_h:.2e} qkv {e_q:.2e}; vs four launches h0 {r_h:.2e} qkv {r_q:.2e}; "
          f"h0 elements differing {int((h0 != old[0]).sum())}")
    assert e_h < tol(5e-3, el) and e_q < tol(5e-3, el)
    assert r_h < tol(3e-3, el) and r_q < tol(3e-3, el)
    # h0 bit for bit: the proj_in chains keep ctrlv_gemm's K order on bias start values, and both norms round as the launches do
    assert torch.equal(h0, old[0])


@pytest.mark.parametrize("n_img,S", CASES)
def test_spatial_entry_fused(ops, el, layer, n_img, S):
    p, M = layer, n_img * S
    x = (torch.randn(M, C, generator=g(11)) * 1.5 + 3.0 + torch.randn(C, generator=g(12)) * 2.0).to(el)
    xd = x.to(DEV)
    part = torch.empty(ops.groupnorm_scratch_floats(n_img, S, C, 1), dtype=torch.float32, device=DEV)
    stats = ops.groupnorm_stats(xd, n_img, S, C, 1, 1e-6, part)
    h0, qkv = nan_outputs(M, el)
    fused(ops, p, xd, stats, n_img, S, h0, qkv)
    old = four_launches(ops, p, xd, n_img, S, el)
    check_against_references(ops, p, x, xd, h0, qkv, n_img, S, el, old, f"spatial_entry n{n_img} S{S}")
    # run-to-run
    h0b, qkvb = nan_outputs(M, el)
    fused(ops, p, xd, stats, n_img, S, h0b, qkvb)
    assert torch.equal(h0, h0b) and torch.equal(qkv, qkvb)
    # image 0 alone
    if n_img > 1:
        x1 = xd[:S].contiguous()
        part1 = torch.empty(ops.groupnorm_scratch_floats(1, S, C, 1), dtype=torch.float32, device=DEV)
        stats1 = ops.groupnorm_stats(x1, 1, S, C, 1, 1e-6, part1)
        h01, qkv1 = nan_outputs(S, el)
        fused(ops, p, x1, stats1, 1, S, h01, qkv1)
        assert torch.equal(h01, h0[:S]) and torch.equal(qkv1, qkv[:S])
    # guard bands: pitched x / h0 / q|k|v views inside buffers whose every other byte is known
    _, xv = guarded(M, C, el, DEV, pitch=C + 88, col_off=8, fill="poison")
    xv.copy_(xd)
    hbuf, hv = guarded(M, C, el, DEV, pitch=C + 104, col_off=24)
    qbuf, qv = guarded(M, 3 * C, el, DEV, pitch=3 * C + 72, col_off=32)
    hbefore, qbefore = hbuf.clone(), qbuf.clone()
    fused(ops, p, xv, stats, n_img, S, hv, qv)
    torch.cuda.synchronize()
    check_written_only_inside(hbefore, hbuf, hv, what="h0")
    check_written_only_inside(qbefore, qbuf, qv, what="qkv")
    assert torch.equal(hv, h0) and torch.equal(qv, qkv)


def test_spatial_entry_fused_from_producer_partials(ops, el, layer):
    """x and its chunk partials come out of a 3x3 conv launch (ctrlv_gemm_desc.gn_partials, 64-row chunks); the statistics
    are the finalize step alone"""
    from ctrlv_amd import packing
    p = layer
    n_img, H, W, cin = 2, 8, 32, 64
    S, M = H * W, n_img * H * W
    a = torch.randn(n_img, cin, H, W, generator=g(21)).to(el)
    wt = torch.randn(C, cin, 3, 3, generator=g(22)) / math.sqrt(9 * cin)
    kw = dict(N=C, cin=cin, taps=9, mode=1, conv=(H, W, H, W, 1, 0), bias=(torch.randn(C, generator=g(23)) * 2 + 3).to(DEV),
              V=torch.randn(n_img, C, generator=g(24)).to(DEV), vmode=1, vdiv=S)
    ad = a.permute(0, 2, 3, 1).reshape(M, cin).contiguous().to(DEV)
    wd = packing.pack_conv3x3(wt).to(DEV)
    xd = torch.empty(M, C, dtype=el, device=DEV)
    assert ops.gemm_gn_partials_serves(ad, wd, xd, **kw)
    part = torch.full((ops.groupnorm_fused_scratch_floats(n_img, S, 1),), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm(ad, wd, xd, gn_partials=part, **kw)
    stats = ops.groupnorm_finalize(xd, n_img, S, C, 1, 1e-6, part)
    h0, qkv = nan_outputs(M, el)
    fused(ops, p, xd, stats, n_img, S, h0, qkv)
    old = four_launches(ops, p, xd, n_img, S, el, stats_from=part)
    check_against_references(ops, p, xd.cpu(), xd, h0, qkv, n_img, S, el, old, "spatial_entry from producer partials")


def test_spatial_entry_predicate_and_routing(ops, el, layer, monkeypatch):
    """`serves` is a function of shape and operands; where it says no, the block runs the four launches: the executor's
    result is then bit-identical with the switch on and off, and the fused launch is never made."""
    from ctrlv_amd.models import blocks
    from ctrlv_amd.workspace import Workspace
    p = layer
    gn, ln = (p["gn_g_d"], p["gn_b_d"]), (p["ln_g_d"], p["ln_b_d"], 1e-5)

    def serves(n_img, S, c=C, **kw):
        x = torch.empty(n_img * S, c, dtype=el, device=DEV)
        h0, qkv = torch.empty_like(x), torch.empty(n_img * S, 3 * c, dtype=el, device=DEV)
        return ops.spatial_entry_fused_serves(x, p["wf"], None, gn, ln, h0, qkv, n_img, S, **kw)

    assert serves(2, 64)
    assert not serves(2, 40)
    assert not serves(2, 64, c=640)
    assert not serves(2, 64, head_dim=32)
    assert not serves(2, 64, h0_lo=torch.empty(128, C, dtype=torch.float8_e5m2, device=DEV))
    assert not serves(2, 64, x_lo=torch.empty(128, C, dtype=torch.float8_e5m2, device=DEV))

    torch.manual_seed(3)
    B, Fr = 1, 2
    blk = blocks.TransformerSpatioTemporalModel(5, 64, C, 64).to(DEV, el)
    blk.pack()
    blk.xattn_off = (0, C)
    assert blk._pk["se_wf"] is not None
    calls = []
    real = ops.spatial_entry_fused
    monkeypatch.setattr(ops, "spatial_entry_fused", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(H, W, switch):
        monkeypatch.setattr(blocks, "_SPATIAL_ENTRY", switch)
        xattn = torch.randn(B, 2 * C, generator=g(31)).to(DEV)
        ws = Workspace(DEV, chunk_bytes=64 << 20)
        ws.el = el
        ctx = blocks.FwdCtx(ws, B, Fr, None, xattn, "sb")
        x = (torch.randn(B * Fr * H * W, C, generator=g(32)) + 1.0).to(el).to(DEV)
        with torch.no_grad():
            y = blk.run(ctx, x, H, W).clone()
        torch.cuda.synchronize()
        return y

    on, off = run(5, 8, True), run(5, 8, False)         # S = 40: not served
    assert not calls and torch.equal(on, off)
    on, off = run(8, 8, True), run(8, 8, False)         # S = 64: served
    assert len(calls) == 1
    # (same rounding points on both routes; what is left is summation order and the occasional flipped rounding: the bound
    #  tests/test_blocks_gpu.py holds a block to against the storage-point oracle)
    r = rel_l2(on.float().cpu(), off.float().cpu())
    print(f"  block output, fused entry vs four launches: rel_l2 {r:.2e}")
    assert r < tol(2e-3, el)
