"""LoRA adapters on the GPU (csrc/lora.hip, ctrlv_amd/lora.py, autograd.Gemm): the factor-gradient kernel against fp32
torch and against the naive merged-weight chain, the merge kernel, B = 0 leaving every forward and the training loss
bit-identical, the stage-1 step with an adapter against the oracle's fp32 autograd (the oracle's nn.Linears wrapped as
base(x) + s B(A(x)), test-side), inference after optimizer steps through both executors and after fuse_lora(), the
state-dict round trip, and the full-size step."""
import copy
import math

import pytest
import torch

from tests.parity_utils import make_inputs, make_pair, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGETS = ("to_q", "to_k", "to_v", "to_out.0")


def _cfg(r=4, alpha=None):
    return dict(r=r, lora_alpha=r if alpha is None else alpha, init_lora_weights="gaussian", lora_dropout=0.0,
                target_modules=list(TARGETS))


def _ref_grads(X, dY, A, B, g, s):
    """fp32 torch: dA_i = s (dY_i B_i)^T X, dB_i = s dY_i^T (X A_i^T) (the kernel's rounding points: none beyond X, dY)"""
    X, dY = X.float(), dY.float()
    r, n = A.shape[0] // g, B.shape[0] // g
    dA, dB = [], []
    for i in range(g):
        a, b, y = A[i * r:(i + 1) * r], B[i * n:(i + 1) * n], dY[:, i * n:(i + 1) * n]
        dA.append(s * (y @ b).t() @ X)
        dB.append(s * y.t() @ (X @ a.t()))
    return torch.cat(dA), torch.cat(dB)


@pytest.mark.parametrize("el", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("g,r,cin,ng,M", [(3, 4, 320, 320, 1000), (1, 4, 320, 320, 777), (3, 16, 640, 640, 3001),
                                          (1, 64, 1280, 1280, 515), (3, 64, 1024, 320, 1200), (1, 16, 1024, 1280, 4500)])
def test_lora_grad_matches_fp32(hip_lib, el, g, r, cin, ng, M):
    from ctrlv_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(g * 1000 + r + cin + M)
    X = torch.randn(M, cin, device=DEV, generator=gen).to(el)
    dY = (0.1 * torch.randn(M, g * ng, device=DEV, generator=gen)).to(el)
    A = torch.randn(g * r, cin, device=DEV, generator=gen) / r
    B = 0.02 * torch.randn(g * ng, r, device=DEV, generator=gen)
    s = 1.5
    dA, dB = ops.lora_grad(X, dY, A, B, g, s)
    dA2, dB2 = ops.lora_grad(X, dY, A, B, g, s)
    torch.cuda.synchronize()
    rA, rB = _ref_grads(X, dY, A, B, g, s)
    ea, eb = rel_l2(dA, rA), rel_l2(dB, rB)
    print(f"  {el} g={g} r={r} Cin={cin} Ng={ng} M={M}: rel-L2 dA {ea:.2e} dB {eb:.2e}")
    assert ea <= 1e-3 and eb <= 1e-3
    assert torch.equal(dA, dA2) and torch.equal(dB, dB2)


@pytest.mark.parametrize("el", [torch.bfloat16, torch.float16])
def test_lora_grad_padded_row_pitch(hip_lib, el):
    """X and dY as column slices of wider row buffers (ldx > Cin, ldy > N): the descriptor's pitches, not the widths, step
    the rows; the result equals the one on contiguous copies bit for bit."""
    from ctrlv_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(21)
    M, cin, g, ng, r = 1337, 320, 3, 320, 8
    Xw = torch.randn(M, cin + 72, device=DEV, generator=gen).to(el)
    dYw = (0.1 * torch.randn(M, g * ng + 136, device=DEV, generator=gen)).to(el)
    X, dY = Xw[:, 64:64 + cin], dYw[:, 128:128 + g * ng]
    assert X.stride(0) == cin + 72 and dY.stride(0) == g * ng + 136
    A = torch.randn(g * r, cin, device=DEV, generator=gen) / r
    B = 0.02 * torch.randn(g * ng, r, device=DEV, generator=gen)
    dA, dB = ops.lora_grad(X, dY, A, B, g, 0.5)
    cA, cB = ops.lora_grad(X.contiguous(), dY.contiguous(), A, B, g, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(dA, cA) and torch.equal(dB, cB)
    rA, rB = _ref_grads(X, dY, A, B, g, 0.5)
    assert rel_l2(dA, rA) <= 1e-3 and rel_l2(dB, rB) <= 1e-3


def test_lora_grad_matches_the_naive_merged_weight_chain(hip_lib):
    """dA = s B^T dW', dB = s dW' A^T with dW' from ctrlv_gemm_wgrad (the chain that treats W' as a leaf)."""
    from ctrlv_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(3)
    for (M, cin, n, g, r) in ((9216, 320, 960, 3, 4), (2304, 640, 640, 1, 16), (576, 1280, 3840, 3, 8)):
        X = torch.randn(M, cin, device=DEV, generator=gen).to(torch.bfloat16)
        dY = (0.1 * torch.randn(M, n, device=DEV, generator=gen)).to(torch.bfloat16)
        A = torch.randn(g * r, cin, device=DEV, generator=gen) / r
        B = 0.02 * torch.randn(n, r, device=DEV, generator=gen)
        s = 2.0
        dA, dB = ops.lora_grad(X, dY, A, B, g, s)
        dW = torch.empty(n, cin, device=DEV)
        ops.gemm_wgrad(X, dY, dW, N=n, cin=cin, torch_layout=True, assign=ops.DETERMINISTIC)
        if not ops.DETERMINISTIC:
            dW.zero_()
            ops.gemm_wgrad(X, dY, dW, N=n, cin=cin, torch_layout=True)
        ng = n // g
        nA = torch.cat([s * B[i * ng:(i + 1) * ng].t() @ dW[i * ng:(i + 1) * ng] for i in range(g)])
        nB = torch.cat([s * dW[i * ng:(i + 1) * ng] @ A[i * r:(i + 1) * r].t() for i in range(g)])
        ea, eb = rel_l2(dA, nA), rel_l2(dB, nB)
        print(f"  M={M} Cin={cin} N={n} g={g} r={r}: rel-L2 vs naive chain dA {ea:.2e} dB {eb:.2e}")
        assert ea <= 1e-3 and eb <= 1e-3


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16, torch.float16])
def test_lora_merge_matches_fp32(hip_lib, wdt):
    from ctrlv_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(5)
    for (n, cin, r) in ((320, 320, 4), (960, 1024, 64), (1280, 640, 16)):
        W = torch.randn(n, cin, device=DEV, generator=gen).to(wdt)
        A = torch.randn(r, cin, device=DEV, generator=gen) / r
        B = torch.randn(n, r, device=DEV, generator=gen)
        out = ops.lora_merge(W, A, B, 0.75)
        ref = W.float() + 0.75 * (B.double() @ A.double()).float()
        assert out.dtype == torch.float32 and rel_l2(out, ref) <= 1e-6


def _fwd(model, executor, inputs):
    sample, t, ehs, ids = inputs
    model.executor = executor
    with torch.no_grad():
        out = model(sample, t, ehs, ids, return_dict=False)[0]
    torch.cuda.synchronize()
    return out.clone()


def _inputs(config, B=1, dtype=torch.float32):
    sample, t, ehs, ids, _ = make_inputs(config, B, 3, 16, 16)
    dev = lambda x: x.to(device=DEV, dtype=dtype)   # noqa: E731
    return dev(sample), t.to(DEV), dev(ehs), ids.to(DEV)


def _train_loss(unet, b):
    from ctrlv_amd import training
    lat, sig, noisy, ts, sample = training._noised_inputs(b)
    with torch.no_grad():
        pred = training.unet_full_train_forward(unet, sample, ts, b["encoder_hidden_states"], b["added_time_ids"])
        return training.edm_loss(pred, noisy, lat, sig)


def test_zero_B_adapter_is_bit_identical(hip_lib):
    import ctrlv_ref as R
    from tests.test_train_unet_gpu import _batch
    config = dict(R.TINY_CONFIG)
    _, _, hu, _ = make_pair(config, DEV, seed=6)
    hu.float()
    x = _inputs(config)
    bd = {k: v.to(DEV) for k, v in _batch(config, 1, 3, 16, 16, seed=9).items()}
    base = {ex: _fwd(hu, ex, x) for ex in ("plan", "python")}
    loss0 = _train_loss(hu, bd)
    hu.add_adapter(_cfg())
    for ex in ("plan", "python"):
        assert torch.equal(_fwd(hu, ex, x), base[ex]), ex
    assert torch.equal(_train_loss(hu, bd), loss0)


def _wrap_oracle(ou, hu, r, s):
    """test-side LoRA on the oracle: forward hooks out + s B(A(x)) around every target nn.Linear, factors copied from hu"""
    hp = dict(hu.named_parameters())
    facs = {}
    for n, m in ou.named_modules():
        if isinstance(m, torch.nn.Linear) and any(n == t or n.endswith("." + t) for t in TARGETS):
            p0 = next(ou.parameters())
            a = torch.nn.Parameter(hp[n + ".lora_A.default.weight"].detach().to(p0.device, p0.dtype).clone())
            b = torch.nn.Parameter(hp[n + ".lora_B.default.weight"].detach().to(p0.device, p0.dtype).clone())
            facs[n + ".lora_A.default.weight"], facs[n + ".lora_B.default.weight"] = a, b
            m.register_forward_hook(lambda _m, inp, out, a=a, b=b: out + s * torch.nn.functional.linear(
                torch.nn.functional.linear(inp[0], a), b))
    for p in ou.parameters():
        p.requires_grad_(False)
    return facs


def _clone(config, hu, adapter):
    """a fresh HIP UNet with hu's parameters (and its adapter, or only the base weights), same dtype and trunk mode"""
    from ctrlv_amd.models import UNetSpatioTemporalConditionModel
    m = UNetSpatioTemporalConditionModel(**config).to(DEV, hu.dtype).eval()
    m.trunk_dtype = hu.trunk_dtype
    sd = hu.state_dict()
    if adapter:
        m.add_adapter(_cfg(r=hu._lora["r"], alpha=hu._lora["lora_alpha"]))
        m.to(DEV, hu.dtype)
    else:
        sd = {k: v for k, v in sd.items() if ".lora_" not in k}
    m.load_state_dict(sd, strict=True)
    return m


def _random_B(hu, seed=11):
    g = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for n, p in hu.named_parameters():
            if ".lora_B." in n:
                p.copy_(0.05 * torch.randn(p.shape, generator=g, device=DEV))


@pytest.mark.parametrize("B", [1, 2])
def test_unet_train_step_with_lora_matches_oracle(hip_lib, B):
    import ctrlv_ref as R
    from ctrlv_amd.training import unet_train_step
    from tests.test_train_unet_gpu import _batch, _oracle_unet_step
    config = dict(R.TINY_CONFIG)
    ou, _, hu, _ = make_pair(config, DEV, seed=3)
    hu.float()
    hu.add_adapter(_cfg(r=4, alpha=8))
    _random_B(hu)
    b = _batch(config, B, 3, 16, 16, drop=(0,) if B == 2 else ())
    yu = copy.deepcopy(ou).to(DEV, torch.bfloat16)
    of, yf = _wrap_oracle(ou, hu, 4, 2.0), _wrap_oracle(yu, hu, 4, 2.0)
    with torch.enable_grad():
        loss_ref = float(_oracle_unet_step(ou, b))
        _oracle_unet_step(yu, b)
        loss = float(unet_train_step(hu, {k: v.to(DEV) for k, v in b.items()}))
    torch.cuda.synchronize()
    assert math.isfinite(loss) and abs(loss - loss_ref) <= 5e-3 * abs(loss_ref), (loss, loss_ref)
    hp = dict(hu.named_parameters())
    for n, p in hp.items():
        if ".lora_" not in n:
            assert not p.requires_grad and p.grad is None, n
    got, ref, yst = [], [], []
    worst = 0.0
    for n in of:
        gp = hp[n].grad
        assert gp is not None, n
        if ".attn2.to_q." in n or ".attn2.to_k." in n:
            assert float(gp.abs().max()) == 0.0, n                     # one-key cross-attention: exact zeros
            continue
        e, ye = rel_l2(gp, of[n].grad), rel_l2(yf[n].grad.float().cpu(), of[n].grad)
        worst = max(worst, e)
        # (test_train_unet_gpu's per-parameter rule against the bf16 yardstick, widened to what factor gradients need --
        #  thin projections of the weight gradient; DESIGN 3.11: the yardstick itself reaches 8.5e-2 and the worst factors
        #  measured 2.08e-1 / 3.2x the yardstick, so cap 2.2e-1 and 3.5x; the concatenated bound below is unchanged)
        assert e < 2.2e-1 and e < max(3.5 * ye, 2e-2), (n, e, ye)
        got.append(gp.float().cpu().reshape(-1)); ref.append(of[n].grad.reshape(-1)); yst.append(yf[n].grad.float().cpu().reshape(-1))
    tot, ytot = rel_l2(torch.cat(got), torch.cat(ref)), rel_l2(torch.cat(yst), torch.cat(ref))
    print(f"  B={B}: loss {loss:.6f} vs {loss_ref:.6f}; {len(got)} factor gradients rel-L2 {tot:.2e} (torch bf16 {ytot:.2e}), "
          f"worst {worst:.2e}")
    assert len(got) == 512 - 128 and tot < 3e-2 and tot < 1.5 * ytot       # (all but attn2.to_q / to_k)


@pytest.mark.parametrize("fp16", [False, True])
def test_inference_after_lora_steps_plan_python_and_fused(hip_lib, fp16):
    import ctrlv_ref as R
    from ctrlv_amd.training import unet_train_step
    from tests.test_train_unet_gpu import _batch
    config = dict(R.TINY_CONFIG)
    _, _, hu, _ = make_pair(config, DEV, seed=6)
    hu.float()
    hu.add_adapter(_cfg())
    opt = torch.optim.AdamW(hu.get_parameters_with_grad(), lr=3e-3, weight_decay=1e-2)
    bd = {k: v.to(DEV) for k, v in _batch(config, 1, 3, 16, 16, seed=9).items()}
    for _ in range(2):
        unet_train_step(hu, bd, opt)
    dt = torch.float32
    if fp16:
        dt = torch.float16
        hu.half()
        hu.trunk_dtype = "fp16x2"
    fused = _clone(config, hu, adapter=True).fuse_lora()
    assert not [k for k in fused.state_dict() if ".lora_" in k]
    base = _clone(config, hu, adapter=False)
    models = [hu, fused, base]
    x = _inputs(config, dtype=dt)
    outs = [{ex: _fwd(m, ex, x) for ex in ("plan", "python")} for m in models]
    (a, f, b) = outs
    assert torch.equal(a["plan"], a["python"])
    assert torch.equal(a["plan"], f["plan"]) and torch.equal(a["python"], f["python"])
    assert not torch.equal(a["plan"], b["plan"]) and not torch.equal(a["python"], b["python"])


def test_state_dict_round_trip_and_from_unet(hip_lib):
    import ctrlv_ref as R
    from ctrlv_amd.models import ControlNetModel, UNetSpatioTemporalConditionModel
    config = dict(R.TINY_CONFIG)
    _, _, hu, _ = make_pair(config, DEV, seed=6)
    hu.float()
    hu.add_adapter(_cfg())
    _random_B(hu)
    x = _inputs(config)
    ref = {ex: _fwd(hu, ex, x) for ex in ("plan", "python")}
    fresh = UNetSpatioTemporalConditionModel(**config).to(DEV, torch.float32).eval()
    fresh.add_adapter(_cfg())
    fresh.load_state_dict(hu.state_dict())
    for ex in ("plan", "python"):
        assert torch.equal(_fwd(fresh, ex, x), ref[ex]), ex
    with pytest.raises(ValueError, match="fuse_lora"):
        ControlNetModel.from_unet(hu)
    ControlNetModel.from_unet(_clone(config, hu, adapter=True).fuse_lora())


def test_unet_lora_train_step_full_size(hip_lib):
    """576 x 1024, 25 frames, rank 4, checkpointed: finite, factor gradients bit-identical across two runs, the loss falls
    over a few steps at a large learning rate; prints the peak memory."""
    from ctrlv_amd.models import UNetSpatioTemporalConditionModel
    from ctrlv_amd.training import unet_train_step
    from ctrlv_amd.utils import build_on_device, random_init_
    h, w, F = 72, 128, 25
    unet = build_on_device(UNetSpatioTemporalConditionModel, DEV, dtype=torch.float32, num_frames=F)
    random_init_(unet, seed=0)
    unet.add_adapter(_cfg())
    unet.enable_gradient_checkpointing()
    _random_B(unet, seed=2)
    g = torch.Generator(device=DEV).manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)      # noqa: E731
    b = dict(latents=rn(1, F, 4, h, w), noise=rn(1, F, 4, h, w), sigmas=torch.tensor([1.5], device=DEV),
             image_latents=rn(1, 1, 4, h, w).repeat(1, F, 1, 1, 1), encoder_hidden_states=rn(1, 1, 1024),
             added_time_ids=torch.tensor([[6.0, 127.0, 0.02]], device=DEV))
    params = unet.get_parameters_with_grad()
    try:
        torch.cuda.reset_peak_memory_stats()
        runs = []
        for _ in range(2):
            for p in params:
                p.grad = None
            loss = unet_train_step(unet, b)
            torch.cuda.synchronize()
            runs.append((loss.clone(), [p.grad.clone() for p in params]))
        peak = torch.cuda.max_memory_allocated() / 2**30
        (l0, g0), (l1, g1) = runs
        assert math.isfinite(float(l0)) and all(bool(torch.isfinite(x).all()) for x in g0)
        assert torch.equal(l0, l1) and all(torch.equal(a, c) for a, c in zip(g0, g1))
        del runs, g0, g1
        for p in params:
            p.grad = None
        opt = torch.optim.AdamW(params, lr=1e-2, weight_decay=0.0)
        losses = [float(unet_train_step(unet, b, opt)) for _ in range(3)] + [float(unet_train_step(unet, b))]
        print(f"  LoRA r=4 {h}x{w}, F={F}: peak {peak:.1f} GiB (checkpointed), {sum(p.numel() for p in params) / 1e6:.2f} M "
              f"factors, losses {losses}")
        assert all(math.isfinite(v) for v in losses) and losses[3] < losses[0]
    finally:
        del unet
        torch.cuda.empty_cache()
