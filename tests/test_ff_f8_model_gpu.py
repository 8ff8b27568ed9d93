"""Model-level tests of the FP8 feed-forward mode (ff_dtype = "f8": DESIGN.md 3.13).

With the mode set on the model instances the plan and the per-op Python executor stay bit-identical, the outputs differ from
the default mode, and the error against the fp32 oracle is bounded by what the quantisation itself costs:

    e_f8 <= 2 (e_q + e_16)        for the UNet output, the mid residual and the worst down residual (rel-L2)

e_q = the error of the oracle with its served feed-forwards fake-quantised (tests/f8_ref.py, computed here on the CPU), e_16 =
the same HIP models' error in the default mode, measured here.  The triangle inequality gives e_q + ||HIP - Q||; the second
term is the 16-bit storage error plus the e4m3 codes which that storage rounding flips -- a bf16 rounding of a LayerNorm output
flips a code with probability about 2^-8 / 2^-3.5 = 8 %, an error of about the size of the quantisation error itself: hence the
factor 2.
"""
import pytest
import torch

from tests import f8_ref
from tests.parity_utils import hip_forward, make_inputs, make_pair, oracle_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("unet", "mid", "down")


def _set_mode(models, mode):
    for m in models:
        m.ff_dtype = mode


def _n_f8_weights(model):
    """feed-forwards of the Python executor's packing that carry e4m3 weights (blocks._f8_weight)"""
    from ctrlv_amd.models.blocks import TransformerSpatioTemporalModel
    n = 0
    for m in model.modules():
        if isinstance(m, TransformerSpatioTemporalModel) and m._pk is not None:
            n += sum(hasattr(m._pk[k][0], "f8") and hasattr(m._pk[k][2], "f8") for k in ("s_ff", "t_ffin", "t_ff"))
    return n


def _bound_check(e_f8, e_q, e_16, what):
    for k in KEYS:
        print(f"  {what} {k}: e_f8 {e_f8[k]:.3e}  e_q {e_q[k]:.3e}  e_16 {e_16[k]:.3e}  bound {2 * (e_q[k] + e_16[k]):.3e}")
    for k in KEYS:
        assert e_f8[k] <= 2 * (e_q[k] + e_16[k]), (what, k, e_f8[k], e_q[k], e_16[k])


@torch.no_grad()
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_tiny_f8_mode(hip_lib, dtype):
    """TINY_CONFIG, B2 F3 16x16: the 48 feed-forwards at C = 128 of the two models are served, the C = 64 ones are not."""
    import ctrlv_ref as R
    cfg = dict(R.TINY_CONFIG)
    ou, oc, hu, hc = make_pair(cfg, DEV, dtype=dtype)
    inputs = make_inputs(cfg, 2, 3, 16, 16, dtype=dtype)
    ref = oracle_forward(ou, oc, inputs, with_unet_no_ctrl=False)
    qu, qc, n = f8_ref.quantised_copy(ou, oc)
    assert n == 48
    e_q = f8_ref.errors(oracle_forward(qu, qc, inputs, with_unet_no_ctrl=False), ref)
    same = hip_forward(hu, hc, inputs, DEV, with_unet_no_ctrl=False)
    e_16 = f8_ref.errors(same, ref)
    _set_mode((hu, hc), "f8")
    try:
        got = {}
        for ex in ("plan", "python"):
            hu.executor = hc.executor = ex
            got[ex] = hip_forward(hu, hc, inputs, DEV, with_unet_no_ctrl=False)
        assert hu._plan.ff_mode == "f8" and hc._plan.ff_mode == "f8"
        assert _n_f8_weights(hu) + _n_f8_weights(hc) == 48
        a, b = got["plan"], got["python"]
        assert torch.equal(a["unet"], b["unet"]) and torch.equal(a["mid"], b["mid"])
        assert all(torch.equal(x, y) for x, y in zip(a["down"], b["down"]))
        assert not torch.equal(a["unet"], same["unet"]) and not torch.equal(a["mid"], same["mid"])
        _bound_check(f8_ref.errors(a, ref), e_q, e_16, f"tiny {dtype}")
        # back to the default mode: the bits of the default mode
        _set_mode((hu, hc), "same")
        hu.executor = hc.executor = "plan"
        again = hip_forward(hu, hc, inputs, DEV, with_unet_no_ctrl=False)
        assert torch.equal(again["unet"], same["unet"]) and torch.equal(again["mid"], same["mid"])
    finally:
        _set_mode((hu, hc), "same")
        hu.executor = hc.executor = "plan"


@torch.no_grad()
def test_fullwidth_f8_mode(hip_lib):
    """Production widths: SVD_CONFIG with num_frames = 2, B1 F2 32x32, fp16 elements (the lean pair of
    tests/test_fullwidth_f16_gpu.py): 48 feed-forwards at C = 640 / 1280 served, the C = 320 ones keep ff_fused.  e_q must be
    what the oracle-only study gave for this configuration: 4.2e-3 / 1.4e-2 / 1.3e-2."""
    import ctrlv_ref as R
    cfg = dict(R.SVD_CONFIG, num_frames=2)
    ou, oc, hu, hc = make_pair(cfg, DEV, lean=True, dtype=torch.float16)
    inputs = make_inputs(cfg, 1, 2, 32, 32, dtype=torch.float16)
    ref = oracle_forward(ou, oc, inputs, with_unet_no_ctrl=False)
    same = hip_forward(hu, hc, inputs, DEV, with_unet_no_ctrl=False)
    e_16 = f8_ref.errors(same, ref)
    assert f8_ref.fake_quant_feed_forwards(ou) + f8_ref.fake_quant_feed_forwards(oc) == 48      # (in place: the pair is ours)
    e_q = f8_ref.errors(oracle_forward(ou, oc, inputs, with_unet_no_ctrl=False), ref)
    _set_mode((hu, hc), "f8")
    try:
        got = hip_forward(hu, hc, inputs, DEV, with_unet_no_ctrl=False)
        assert hu._plan.ff_mode == "f8" and not torch.equal(got["unet"], same["unet"])
        _bound_check(f8_ref.errors(got, ref), e_q, e_16, "full width fp16")
    finally:
        _set_mode((hu, hc), "same")
    for k, want in (("unet", 4.2e-3), ("mid", 1.4e-2), ("down", 1.3e-2)):
        assert abs(e_q[k] - want) <= 0.1 * want, (k, e_q[k], want)


@torch.no_grad()
def test_graph_replay_matches_eager_in_f8_mode(hip_lib):
    """Three scheduler steps of the tiny pair in f8 mode: HIP-graph replay (ControlNet on a side stream) gives the same
    latents as eager launches, bit for bit -- nothing allocates or synchronises inside a forward of the mode."""
    import ctrlv_ref as R
    from ctrlv_amd.pipelines.pipeline_utils import DenoiseStepper
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    cfg = dict(R.TINY_CONFIG)
    _, _, hu, hc = make_pair(cfg, DEV)
    bf, FR, H, W = torch.bfloat16, 3, 16, 16
    g = lambda s: torch.Generator(device=DEV).manual_seed(s)      # noqa: E731
    sched = EulerDiscreteScheduler()
    sched.set_timesteps(25, device=DEV)
    lat = torch.randn(1, FR, 4, H, W, generator=g(300), device=DEV) * sched.init_noise_sigma
    img = torch.randn(1, 4, H, W, generator=g(301), device=DEV)
    image_latents = torch.cat([torch.zeros_like(img), img]).unsqueeze(1).repeat(1, FR, 1, 1, 1).to(bf)
    e = torch.randn(1, 1, cfg["cross_attention_dim"], generator=g(302), device=DEV)
    ehs = torch.cat([torch.zeros_like(e), e]).to(bf)
    c = torch.randn(1, FR, 4, H, W, generator=g(303), device=DEV)
    cond = torch.cat([torch.zeros_like(c), c]).to(bf)
    ids = torch.tensor([[6.0, 127.0, 0.02]] * 2, device=DEV, dtype=bf)
    res = {}
    try:
        for mode, graph in (("f8", False), ("f8", True), ("same", False)):
            _set_mode((hu, hc), mode)
            st = DenoiseStepper(hu, hc, sched, lat.clone(), image_latents, ehs, ids, cond, 1.0, 3.0, 1.0, do_cfg=True,
                                use_hip_graph=graph)
            for i in range(3):
                st.step(i)
            torch.cuda.synchronize()
            assert torch.isfinite(st.latents).all()
            res[(mode, graph)] = st.latents.clone()
    finally:
        _set_mode((hu, hc), "same")
    assert hu._plan is not None
    assert torch.equal(res[("f8", False)], res[("f8", True)])
    assert not torch.equal(res[("f8", False)], res[("same", False)])
