"""The error contract of the three `*_load_weights` entry points (ctrlv_plan_load_weights, ctrlv_vae_plan_load_weights,
ctrlv_clip_plan_load_weights; csrc/weight_loader.hip), through raw ctypes on tiny models.

For each plan and each kind of broken descriptor list -- one tensor with a wrong element count, one tensor missing, one tensor
with dtype code 7 -- a plan that holds weights is loaded with the broken list: the call returns the status and message of
include/ctrlv_hip.h's convention, the plan is unloaded (its workspace query refuses), a following complete load succeeds and
one forward gives the bits of a plan that never failed.  The broken descriptor keeps its valid data pointer; the failing
lookup precedes any dereference, so nothing is launched on it.

  wrong numel    CTRLV_E_BAD_SHAPE (-2), the tensor's name and "expected"
  missing        CTRLV_E_BAD_ARG (-1), "missing tensor '<name>'"
  dtype code 7   VAE / CLIP: CTRLV_E_BAD_DTYPE (-4) naming the tensor (checked on use);
                 UNet: CTRLV_E_BAD_ARG (-1) "bad tensor descriptor" (every descriptor is checked up front)"""
import ctypes
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _unet_case(lib, _lib):
    import ctrlv_ref as R
    from ctrlv_amd.plan import config_struct
    from tests.parity_utils import make_inputs, make_pair
    cfg = dict(R.TINY_CONFIG)
    _, _, hu, _ = make_pair(cfg, DEV)
    B, F, h, w = 1, 2, 16, 16
    sample, t, ehs, ids, _ = make_inputs(cfg, B, F, h, w)
    s_d, e_d = sample.to(DEV, BF), ehs.to(DEV, BF)
    t_d, i_d = t.reshape(1).to(DEV, torch.float32), ids.to(DEV, torch.float32)
    c = config_struct("unet", hu.config, "sb")

    def create():
        hnd = ctypes.c_void_p()
        assert lib.ctrlv_plan_create(ctypes.byref(c), 0, ctypes.byref(hnd)) == 0, _lib.last_error(lib)
        return hnd

    def run(hnd):
        ws = torch.empty(lib.ctrlv_plan_workspace_bytes(hnd, B, F, h, w), dtype=torch.uint8, device=DEV)
        assert ws.numel() > 0, _lib.last_error(lib)
        out = torch.empty(B, F, 4, h, w, dtype=BF, device=DEV)
        rc = lib.ctrlv_unet_forward(hnd, s_d.data_ptr(), 2, t_d.data_ptr(), 1, e_d.data_ptr(), i_d.data_ptr(), 3, None, None,
                                    None, out.data_ptr(), B, F, h, w, ws.data_ptr(), ws.numel(), _stream())
        assert rc == 0, _lib.last_error(lib)
        return out

    return SimpleNamespace(
        create=create, run=run, load=lib.ctrlv_plan_load_weights, destroy=lib.ctrlv_plan_destroy,
        ws_bytes=lambda hnd: lib.ctrlv_plan_workspace_bytes(hnd, B, F, h, w),
        state=hu.state_dict(), victim="mid_block.resnets.0.spatial_res_block.conv1.weight",
        bad_dtype=(-1, "bad tensor descriptor"))


def _vae_case(lib, _lib):
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    torch.manual_seed(5)
    m = AutoencoderKLTemporalDecoder().eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("mix_factor"):
                p.fill_(0.4)
    m = m.to(DEV, BF)
    n, h, w = 3, 8, 8
    z = torch.randn(n, 4, h, w, generator=torch.Generator().manual_seed(3)).to(DEV, BF)
    cfg = _lib.VaeConfig()
    cfg.in_channels, cfg.out_channels, cfg.latent_channels, cfg.layers_per_block, cfg.n_blocks = 3, 3, 4, 2, 4
    for i, ch in enumerate((128, 256, 512, 512)):
        cfg.block_out_channels[i] = ch
    cfg.scaling_factor = 0.18215

    def create():
        hnd = ctypes.c_void_p()
        assert lib.ctrlv_vae_plan_create(ctypes.byref(cfg), 0, ctypes.byref(hnd)) == 0, _lib.last_error(lib)
        return hnd

    def run(hnd):
        need = lib.ctrlv_vae_plan_workspace_bytes(hnd, 1, n, n, h, w)
        assert need > 0, _lib.last_error(lib)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        out = torch.empty(n, 3, 8 * h, 8 * w, dtype=BF, device=DEV)
        rc = lib.ctrlv_vae_decode(hnd, z.data_ptr(), 2, n, n, h, w, out.data_ptr(), 2, ws.data_ptr(), need, _stream())
        assert rc == 0, _lib.last_error(lib)
        return out

    victim = "decoder.mid_block.resnets.0.spatial_res_block.conv1.weight"
    return SimpleNamespace(
        create=create, run=run, load=lib.ctrlv_vae_plan_load_weights, destroy=lib.ctrlv_vae_plan_destroy,
        ws_bytes=lambda hnd: lib.ctrlv_vae_plan_workspace_bytes(hnd, 1, n, n, h, w),
        state=m.state_dict(), victim=victim, bad_dtype=(-4, victim))


def _clip_case(lib, _lib):
    from tests import clip_utils as U
    cfg, n, seed = U.CONFIGS["A"]
    m = U.build_own(cfg, seed, BF, DEV)
    px = U.load_golden()["A"]["pixel_values"].to(DEV)
    c = _lib.ClipConfig()
    for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
              "projection_dim"):
        setattr(c, k, cfg[k])
    c.hidden_act = {"gelu": 0, "quick_gelu": 1}[cfg["hidden_act"]]
    c.layer_norm_eps = cfg["layer_norm_eps"]

    def create():
        hnd = ctypes.c_void_p()
        assert lib.ctrlv_clip_plan_create(ctypes.byref(c), 0, ctypes.byref(hnd)) == 0, _lib.last_error(lib)
        return hnd

    def run(hnd):
        need = lib.ctrlv_clip_plan_workspace_bytes(hnd, n)
        assert need > 0, _lib.last_error(lib)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        out = torch.empty(n, cfg["projection_dim"], dtype=BF, device=DEV)
        rc = lib.ctrlv_clip_forward(hnd, px.data_ptr(), _DT[px.dtype], n, out.data_ptr(), None, ws.data_ptr(), need, _stream())
        assert rc == 0, _lib.last_error(lib)
        return out

    victim = "vision_model.encoder.layers.1.mlp.fc1.weight"
    return SimpleNamespace(
        create=create, run=run, load=lib.ctrlv_clip_plan_load_weights, destroy=lib.ctrlv_clip_plan_destroy,
        ws_bytes=lambda hnd: lib.ctrlv_clip_plan_workspace_bytes(hnd, n),
        state=m.state_dict(), victim=victim, bad_dtype=(-4, victim))


def _descs(_lib, items, edit=None):
    """TensorDesc array of (name, contiguous tensor) pairs; `edit(name, desc)` may change one in place."""
    arr = (_lib.TensorDesc * len(items))()
    for i, (k, v) in enumerate(items):
        arr[i].name, arr[i].data, arr[i].dtype = k.encode(), v.data_ptr(), _DT[v.dtype]
        arr[i].on_device, arr[i].numel = 1 if v.is_cuda else 0, v.numel()
        if edit is not None:
            edit(k, arr[i])
    return arr


_CASES = {}


def _case(plan):
    """The model, its descriptors and the output of a plan that never failed: built once per plan kind, never modified."""
    if plan not in _CASES:
        from ctrlv_amd import _lib
        lib = _lib.load()
        c = {"unet": _unet_case, "vae": _vae_case, "clip": _clip_case}[plan](lib, _lib)
        c.lib, c._lib = lib, _lib
        c.items = [(k, (v if v.dtype in _DT else v.float()).detach().contiguous()) for k, v in c.state.items()
                   if torch.is_tensor(v) and v.is_floating_point()]
        assert c.victim in dict(c.items)
        hnd = c.create()
        assert c.load(hnd, _descs(_lib, c.items), len(c.items)) == 0, _lib.last_error(lib)
        c.want = c.run(hnd)
        torch.cuda.synchronize()
        assert c.destroy(hnd) == 0
        _CASES[plan] = c
    return _CASES[plan]


@torch.no_grad()
@pytest.mark.parametrize("fault", ["numel", "missing", "dtype"])
@pytest.mark.parametrize("plan", ["unet", "vae", "clip"])
def test_a_failed_load_reports_unloads_and_recovers(hip_lib, plan, fault):
    c = _case(plan)
    lib, _lib = c.lib, c._lib
    torch.cuda.synchronize()
    hnd = c.create()
    good = _descs(_lib, c.items)
    assert c.load(hnd, good, len(c.items)) == 0, _lib.last_error(lib)
    assert c.ws_bytes(hnd) > 0
    if fault == "numel":
        def edit(k, d):
            if k == c.victim:
                d.numel += 1
        bad, (want_rc, want_msgs) = _descs(_lib, c.items, edit), (-2, (c.victim, "expected"))
    elif fault == "missing":
        items = [kv for kv in c.items if kv[0] != c.victim]
        bad, (want_rc, want_msgs) = _descs(_lib, items), (-1, (f"missing tensor '{c.victim}'",))
    else:
        def edit(k, d):
            if k == c.victim:
                d.dtype = 7
        bad, (want_rc, want_msgs) = _descs(_lib, c.items, edit), (c.bad_dtype[0], (c.bad_dtype[1],))
    rc = c.load(hnd, bad, len(bad))
    msg = _lib.last_error(lib)
    print(f"{plan} / {fault}: rc {rc}, {msg!r}")
    assert rc == want_rc and all(m in msg for m in want_msgs), (rc, msg)
    # the failed load left the plan unloaded
    assert c.ws_bytes(hnd) == 0 and "not loaded" in _lib.last_error(lib)
    # ... and a complete load brings it back with the bits of a plan that never failed
    assert c.load(hnd, good, len(c.items)) == 0, _lib.last_error(lib)
    got = c.run(hnd)
    torch.cuda.synchronize()
    assert torch.equal(got, c.want)
    assert c.destroy(hnd) == 0
