"""GPU tests of ctrlv_gemm_tokens (csrc/gemm_tokens.hip) and of the CLIP plan (csrc/clip_plan.hip, ClipPlan,
clip_vision_hip.encode_plan), bf16 elements (tests/test_clip_plan_f16_gpu.py executes this file's source with EL = torch.float16).

Bounds.
  gemm_tokens   the fp32 matmul of the same 16-bit operands (+ bias, activation, residual in fp32), parity_err < tol(3e-3): the
                bound and helper tests/test_ops_gpu.py holds ctrlv_gemm to.  For the two activations the error of the existing
                two-launch route (ctrlv_gemm, then ctrlv_act_rows in place: two roundings) is printed beside it.
  model         test_clip_gpu._check_model's criterion: rel-L2 against the fp32 result within 1.5 x that of the module's own
                16-bit torch forward, for image_embeds and last_hidden_state.
Everything else is exact: bits repeat, an image has the same bits alone and in a batch, the foreign host and the captured
graph reproduce encode_plan bit for bit."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import clip_utils as U
from tests.parity_utils import parity_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EL = torch.bfloat16


def tol(bf16_bound):
    """tests/test_ops_gpu.py tol(): the stated bf16 bound, a sixth of it for fp16 elements."""
    return bf16_bound if EL == torch.bfloat16 else bf16_bound / 6.0


def g(seed=0):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    return U.load_golden()


# ------------------------------------------------------------------------------------------------ gemm_tokens
SHAPES = [(32, 64), (320, 128), (384, 320), (1280, 1280), (128, 5120)]      # (N, K): one K step, the tiny configs' widths, a
MS = [1, 17, 257, 300, 514]                                                  # sliced square, long K with narrow N
EPILOGUES = ["none", "bias", "bias+gelu", "bias+quick_gelu", "bias+R1"]
M_MAX = max(MS)
_OPERANDS = {}


def _operands(N, K):
    """A [M_MAX, K], W [N, K], bias [N], R1 [M_MAX, N] on the device (the 16-bit ones rounded to EL) and the fp32 product
    A . W^T of the rounded operands, computed once per (N, K, EL) and never modified."""
    key = (N, K, EL)
    if key not in _OPERANDS:
        A = torch.randn(M_MAX, K, generator=g(N + K)).to(EL).to(DEV)
        W = (torch.randn(N, K, generator=g(N * 3 + K)) / K ** 0.5).to(EL).to(DEV)
        bias = (0.5 * torch.randn(N, generator=g(N + 1))).to(DEV)
        R1 = torch.randn(M_MAX, N, generator=g(N + 2)).to(EL).to(DEV)
        _OPERANDS[key] = (A, W, bias, R1, A.float() @ W.float().t())
    return _OPERANDS[key]


def _act_ref(x, act):
    if act == "gelu":
        return F.gelu(x)
    if act == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    return x


def _epi(epilogue):
    return "bias" in epilogue, (epilogue.split("+")[1] if "gelu" in epilogue else None), "R1" in epilogue


@pytest.mark.parametrize("epilogue", EPILOGUES)
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemm_tokens_against_fp32_matmul(ops, N, K, epilogue):
    A, W, bias, R1, prod = _operands(N, K)
    has_bias, act, has_r1 = _epi(epilogue)
    for M in MS:
        ref = prod[:M] + bias if has_bias else prod[:M]
        ref = _act_ref(ref, act)
        if has_r1:
            ref = ref + R1[:M].float()
        out = torch.empty(M, N, dtype=EL, device=DEV)
        ops.gemm_tokens(A[:M], W, out, N=N, K=K, bias=bias if has_bias else None, R1=R1[:M] if has_r1 else None, act=act)
        err = parity_err(out, ref, f"gemm_tokens M={M} N={N} K={K} {epilogue}")
        if act is not None and M == 257:
            two = torch.empty(M, N, dtype=EL, device=DEV)
            ops.gemm(A[:M], W, two, N=N, cin=K, bias=bias)
            ops.act_rows(two, act)
            parity_err(two, ref, f"  two launches (gemm, act_rows)  M={M} N={N} K={K}")
        assert err < tol(3e-3), (M, N, K, epilogue, err)


def test_gemm_tokens_reads_no_stale_slab(ops):
    """Two calls into the SAME workspace and output buffers with different A and different W on a sliced shape: the second
    result meets the bound against its own reference and differs from the first.  A reducer that reads a slab through a stale
    L1 or L2 line returns (part of) the first call's sum."""
    N, K, M = 1280, 1280, 257
    assert ops.gemm_tokens_plan(N, K, EL)[1] > 1
    lib = ops._L(torch.empty(0, dtype=EL))
    ws = torch.empty(lib.ctrlv_gemm_tokens_ws_bytes(M, N, K), dtype=torch.uint8, device=DEV)
    out = torch.empty(M, N, dtype=EL, device=DEV)
    res = []
    for seed in (1, 2):
        A = torch.randn(M, K, generator=g(seed)).to(EL).to(DEV)
        W = (torch.randn(N, K, generator=g(seed + 10)) / K ** 0.5).to(EL).to(DEV)
        ops.gemm_tokens(A, W, out, N=N, K=K, workspace=ws)
        assert parity_err(out, A.float() @ W.float().t(), f"call {seed} into one workspace") < tol(3e-3)
        res.append(out.clone())
    assert not torch.equal(res[0], res[1])
    assert rel_l2(res[1], res[0]) > 0.5          # unrelated operands: the two results are as far apart as two random matrices


@pytest.mark.parametrize("N,K", [(1280, 1280), (128, 5120)])
def test_gemm_tokens_bits_and_bounds(ops, N, K):
    A, W, bias, R1, _ = _operands(N, K)
    assert ops.gemm_tokens_plan(N, K, EL)[1] > 1
    lib = ops._L(A)

    def run(rows, M, ws=None, out=None):
        out = torch.empty(M, N, dtype=EL, device=DEV) if out is None else out
        return ops.gemm_tokens(rows, W, out, N=N, K=K, bias=bias, R1=R1[:M], act="gelu", M=M, workspace=ws)

    # identical inputs, identical bits
    assert torch.equal(run(A[:300], 300), run(A[:300], 300))
    # the rows of image 0 alone (M = S) and inside M = 3 S
    for S in (17, 257):
        rows = A[:S].repeat(3, 1)
        rows[S:] = A[M_MAX - 2 * S:]                      # images 1 and 2 are other rows
        r1 = torch.cat([R1[:S], R1[M_MAX - 2 * S:]])
        alone = torch.empty(S, N, dtype=EL, device=DEV)
        ops.gemm_tokens(rows[:S], W, alone, N=N, K=K, bias=bias, R1=r1[:S], act="gelu")
        batch = torch.empty(3 * S, N, dtype=EL, device=DEV)
        ops.gemm_tokens(rows, W, batch, N=N, K=K, bias=bias, R1=r1, act="gelu")
        assert torch.equal(batch[:S], alone), S
    # ldo > N: the gap columns keep a sentinel; an output buffer longer than M rows: the tail keeps it
    M, ldo, sentinel = 257, N + 24, 777.0
    big = torch.full((M + 40, ldo), sentinel, dtype=EL, device=DEV)
    ws = torch.full((lib.ctrlv_gemm_tokens_ws_bytes(M, N, K),), 0xA5, dtype=torch.uint8, device=DEV)       # a dirty workspace
    run(A[:M], M, ws=ws, out=big[:M, :N])
    torch.cuda.synchronize()
    assert torch.equal(big[:M, :N], run(A[:M], M))
    assert (big[:M, N:] == sentinel).all() and (big[M:] == sentinel).all()
    # the counter words (one per row block x column tile, at the head of the workspace) are zero after the call
    bn, _ = ops.gemm_tokens_plan(N, K, EL)
    words = (M + 287) // 288 * (N // bn)
    assert int(ws[:words * 4].view(torch.int32).abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ the model
def _check_plan(m, px, ref_embeds, ref_hidden, what):
    """test_clip_gpu._check_model with encode_plan in place of encode."""
    from ctrlv_amd.models import clip_vision_hip as H
    assert H.supports(m, px)
    with torch.no_grad():
        t = m.torch_forward(px)
        e, h = H.encode_plan(m, px, return_hidden=True)
        eo, ho = H.encode(m, px, return_hidden=True)
    assert e.dtype == EL and e.shape == ref_embeds.shape and h.shape == ref_hidden.shape
    figs = {}
    for name, got, tor, ref in (("image_embeds", e, t.image_embeds, ref_embeds), ("last_hidden_state", h, t.last_hidden_state, ref_hidden)):
        err_hip, err_torch = rel_l2(got, ref), rel_l2(tor, ref)
        print(f"  {what} {name}: plan rel-L2 {err_hip:.3e}   torch {str(EL)[6:]} rel-L2 {err_torch:.3e}   ratio {err_hip / err_torch:.2f}")
        figs[name] = (err_hip, err_torch)
    print(f"  {what} encode_plan vs encode: image_embeds rel-L2 {rel_l2(e, eo.float()):.3e}   last_hidden_state {rel_l2(h, ho.float()):.3e}")
    for name, (err_hip, err_torch) in figs.items():
        assert err_hip <= 1.5 * err_torch, (what, name, err_hip, err_torch)
    with torch.no_grad():
        e0 = H.encode_plan(m, px[:1])                    # image 0 alone: the same bits as in the batch
        assert torch.equal(H.encode_plan(m, px), e)      # ... and the embeds do not depend on return_hidden
    assert torch.equal(e0[0], e[0])
    return e


@pytest.mark.parametrize("name", ["A", "B"])
def test_plan_parity_with_the_golden(hip_lib, golden, name):
    cfg, n, seed = U.CONFIGS[name]
    m = U.build_own(cfg, seed, EL, DEV)
    gd = golden[name]
    _check_plan(m, gd["pixel_values"].to(DEV), gd["image_embeds"], gd["last_hidden_state"], name)


def test_plan_parity_at_vit_h_widths(hip_lib):
    cfg, seed = dict(U.CONFIG_VIT_H, num_hidden_layers=2), 21
    ref = U.build_own(cfg, seed)
    px = U.seeded_pixels(cfg, 2, seed)
    with torch.no_grad():
        r = ref.torch_forward(px)
    m = ref.to(device=DEV, dtype=EL)
    _check_plan(m, px.to(DEV), r.image_embeds, r.last_hidden_state, "ViT-H x 2 layers")


def _raw_plan(lib, _lib, cfg, state_dict):
    """create -> load from HOST fp32 tensors, through raw ctypes."""
    c = _lib.ClipConfig()
    for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
              "projection_dim"):
        setattr(c, k, cfg[k])
    c.hidden_act = {"gelu": 0, "quick_gelu": 1}[cfg["hidden_act"]]
    c.layer_norm_eps = cfg["layer_norm_eps"]
    hnd = ctypes.c_void_p()
    assert lib.ctrlv_clip_plan_create(ctypes.byref(c), 0, ctypes.byref(hnd)) == 0, _lib.last_error()
    sd = {k: v.detach().float().cpu().contiguous() for k, v in state_dict.items() if v.is_floating_point()}
    arr = (_lib.TensorDesc * len(sd))()
    for i, (k, v) in enumerate(sd.items()):
        arr[i].name, arr[i].data, arr[i].dtype, arr[i].on_device, arr[i].numel = k.encode(), v.data_ptr(), 0, 0, v.numel()
    assert lib.ctrlv_clip_plan_load_weights(hnd, arr, len(sd)) == 0, _lib.last_error()
    return hnd


def test_clip_plan_from_a_foreign_host(hip_lib, golden):
    """Everything through ctypes, weights from host fp32 memory: bit-equal to encode_plan on the same module (whose plan was
    loaded from the module's 16-bit device tensors: rounding fp32 -> EL of a value that is already an EL value is exact)."""
    from ctrlv_amd import _lib
    from ctrlv_amd.models import clip_vision_hip as H
    lib = _lib.load(EL)
    cfg, n, seed = U.CONFIGS["A"]
    m = U.build_own(cfg, seed, EL, DEV)
    px = golden["A"]["pixel_values"].to(DEV)
    with torch.no_grad():
        want_e, want_h = H.encode_plan(m, px, return_hidden=True)
    hnd = _raw_plan(lib, _lib, cfg, m.state_dict())
    ws = torch.empty(lib.ctrlv_clip_plan_workspace_bytes(hnd, n), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0
    e = torch.empty(n, cfg["projection_dim"], dtype=EL, device=DEV)
    h = torch.empty(n, 17, cfg["hidden_size"], dtype=EL, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.ctrlv_clip_forward(hnd, px.data_ptr(), 0, n, e.data_ptr(), h.data_ptr(), ws.data_ptr(), ws.numel(), st)
    assert rc == 0, _lib.last_error()
    # a short workspace is refused; a missing tensor is an error
    assert lib.ctrlv_clip_forward(hnd, px.data_ptr(), 0, n, e.data_ptr(), None, ws.data_ptr(), ws.numel() - 256, st) == -5
    torch.cuda.synchronize()
    assert torch.equal(e, want_e) and torch.equal(h, want_h)
    arr = (_lib.TensorDesc * 1)()
    arr[0].name, arr[0].data, arr[0].dtype, arr[0].on_device, arr[0].numel = b"visual_projection.weight", 0x1000, 0, 1, 1
    assert lib.ctrlv_clip_plan_load_weights(hnd, arr, 1) < 0 and "missing tensor" in _lib.last_error(lib)
    assert lib.ctrlv_clip_plan_destroy(hnd) == 0


def test_clip_forward_is_graph_capturable(hip_lib, golden):
    """One ctrlv_clip_forward on config A captured in torch.cuda.graph (one stream, a single chain); replayed twice with the input
    buffer rewritten in between: both replays equal the eager results bit for bit."""
    from ctrlv_amd.models import clip_vision_hip as H
    cfg, n, seed = U.CONFIGS["A"]
    m = U.build_own(cfg, seed, EL, DEV)
    px1 = golden["A"]["pixel_values"].to(DEV)
    px2 = U.seeded_pixels(cfg, n, 77).to(DEV)
    with torch.no_grad():
        want1, want2 = H.encode_plan(m, px1).clone(), H.encode_plan(m, px2).clone()
    assert not torch.equal(want1, want2)
    plan = H._plan(m)
    buf = px1.clone()
    ws = torch.empty(plan.workspace_bytes(n), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = plan.forward(buf, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want1)
    buf.copy_(px2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want2)


def test_encode_plan_follows_an_in_place_parameter_update(hip_lib, golden):
    from ctrlv_amd.models import clip_vision_hip as H
    cfg, n, seed = U.CONFIGS["A"]
    m = U.build_own(cfg, seed, EL, DEV)
    px = golden["A"]["pixel_values"].to(DEV)
    with torch.no_grad():
        before = H.encode_plan(m, px).clone()
        assert H._plan(m) is H._plan(m)                                   # cached
        m.vision_model.encoder.layers[1].mlp.fc2.bias.add_(0.5)
        after, hidden = H.encode_plan(m, px, return_hidden=True)
        ref = U.build_own(cfg, seed)
        ref.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
        r = ref.torch_forward(px.float().cpu())
        t = m.torch_forward(px)
    assert not torch.equal(before, after)
    for name, got, tor, want in (("image_embeds", after, t.image_embeds, r.image_embeds),
                                 ("last_hidden_state", hidden, t.last_hidden_state, r.last_hidden_state)):
        err_hip, err_torch = rel_l2(got, want), rel_l2(tor, want)
        print(f"  after fc2.bias += 0.5, {name}: plan rel-L2 {err_hip:.3e}   torch rel-L2 {err_torch:.3e}")
        assert err_hip <= 1.5 * err_torch, (name, err_hip, err_torch)


def test_switch_selects_the_route(hip_lib, golden, monkeypatch):
    from ctrlv_amd.models import clip_vision_hip as H
    cfg, n, seed = U.CONFIGS["A"]
    m = U.build_own(cfg, seed, EL, DEV)
    px = golden["A"]["pixel_values"].to(DEV)
    with torch.no_grad():
        monkeypatch.setenv("CTRLV_CLIP_HIP", "plan")
        assert H.route(m, px) == "plan"
        a = m(px)
        assert torch.equal(a.image_embeds, H.encode_plan(m, px))
        assert a.last_hidden_state.shape == (n, 17, 320)
        monkeypatch.setenv("CTRLV_CLIP_HIP", "1")
        assert H.route(m, px) == "ops"
        assert torch.equal(m(px).image_embeds, H.encode(m, px))


def test_transformers_module_runs_on_the_plan(hip_lib, golden):
    """A transformers CLIPVisionModelWithProjection is served as it is (duck typing): the same bits as the project's class."""
    pytest.importorskip("transformers")
    from ctrlv_amd.models import clip_vision_hip as H
    cfg, n, seed = U.CONFIGS["B"]
    t = U.build_transformers(cfg, seed).to(device=DEV, dtype=EL)
    m = U.build_own(cfg, seed, EL, DEV)
    px = golden["B"]["pixel_values"].to(DEV)
    assert H.supports(t, px)
    with torch.no_grad():
        assert torch.equal(H.encode_plan(t, px), H.encode_plan(m, px))


PIPE_CLIP = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=128, patch_size=16,
                 projection_dim=64, hidden_act="gelu", layer_norm_eps=1e-5)        # 65 tokens; projection = cross_attention_dim


@torch.no_grad()
def test_pipeline_encodes_the_image_on_the_plan(hip_lib, monkeypatch):
    """test_pipeline_encodes_the_image_on_the_hip_kernels' construction under CTRLV_CLIP_HIP=plan."""
    import ctrlv_ref as R
    from ctrlv_amd.pipelines import StableVideoControlPipeline
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    from tests.fakes import FakeVAE, fake_feature_extractor
    from tests.parity_utils import make_pair
    cfg = dict(R.TINY_CONFIG)
    assert cfg["cross_attention_dim"] == PIPE_CLIP["projection_dim"]
    _, _, hu, hc = make_pair(cfg, DEV, dtype=EL)
    ref = U.build_own(PIPE_CLIP, 31)
    clip = U.build_own(PIPE_CLIP, 31, EL, DEV)
    pipe = StableVideoControlPipeline(FakeVAE().to(DEV, EL), clip, hu, hc, EulerDiscreteScheduler(), fake_feature_extractor)
    pipe.set_progress_bar_config(disable=True)
    image = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(11)) * 2 - 1
    want = ref.torch_forward(image.to(EL).float()).image_embeds
    from ctrlv_amd.models import clip_vision_hip as H
    monkeypatch.setenv("CTRLV_CLIP_HIP", "plan")
    on = pipe._encode_image(image.to(DEV, EL), DEV, 1, True)
    assert torch.equal(on[1, 0], H.encode_plan(clip, image.to(DEV, EL))[0])        # the plan served it
    monkeypatch.setenv("CTRLV_CLIP_HIP", "0")
    off = pipe._encode_image(image.to(DEV, EL), DEV, 1, True)
    assert on.shape == off.shape == (2, 1, 64) and on.dtype == EL
    assert (on[0] == 0).all() and (off[0] == 0).all()                  # the CFG negative half is exact zeros
    err_on, err_off = rel_l2(on[1, 0], want[0]), rel_l2(off[1, 0], want[0])
    print(f"  pipeline image_embeds: plan rel-L2 {err_on:.3e}   torch rel-L2 {err_off:.3e}")
    assert err_on <= 1.5 * err_off
