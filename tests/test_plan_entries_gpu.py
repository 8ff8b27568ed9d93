"""The contract of the forward ENTRY POINTS of the C++ plan walks (csrc/plan.hip, vae_plan.hip, clip_plan.hip), through raw
ctypes on the tiny models of the other plan tests: ctrlv_unet_forward, ctrlv_unet_encoder_forward, ctrlv_controlnet_forward,
ctrlv_vae_encode, ctrlv_vae_decode, ctrlv_clip_forward.

* Refusals: a workspace one byte short of the size query (CTRLV_E_WORKSPACE, the message carries the needed size), dtype code 7
  (CTRLV_E_BAD_DTYPE), one required pointer null, a plan of the wrong kind, an unaligned workspace (CTRLV_E_BAD_ARG) -- each
  with its message, and with every output still holding the pattern it was filled with: nothing was launched.
* Exact fit: the workspace is exactly the size query's answer, carved 256-aligned out of a larger buffer between two 4 KiB
  bands of 0xA5.  The bands survive the call and every output equals the same call with a generous workspace, bit for bit.
* Sizes: ctrlv_plan_workspace_bytes / ctrlv_vae_plan_workspace_bytes for a list of shapes, both trunk modes and both
  feed-forward precisions, against the answers recorded in tests/golden/plan_workspace_bytes.json (functions of shape and mode
  only: no launch geometry enters them).  `python tests/test_plan_entries_gpu.py --record FILE` writes that file."""
import ctypes
import json
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, HF = torch.bfloat16, torch.float16
_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_workspace_bytes.json")
B, F, H, W = 2, 3, 16, 16
BAND = 4096
PLAN_SHAPES = [(2, 3, 16, 16), (1, 5, 24, 8), (1, 2, 16, 16), (2, 25, 72, 128)]
VAE_SHAPES = {0: [(1, 0, 64, 64), (2, 0, 128, 192), (1, 0, 576, 1024)],                  # encode: n images of H x W pixels
              1: [(3, 3, 8, 8), (4, 2, 8, 8), (3, 3, 16, 24), (25, 25, 72, 128)]}      # decode: n latent frames, clips of nf
# (trunk mode, FF precision) per element library: the split trunk needs fp16 elements and does not combine with FF precision 1
MODES = {"bf16": [(0, 0), (0, 1)], "f16": [(0, 0), (1, 0), (0, 1)]}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _load(_lib, lib, load, hnd, state):
    items = [(k, (v if v.dtype in _DT else v.float()).detach().contiguous()) for k, v in state.items()
             if torch.is_tensor(v) and v.is_floating_point()]
    arr = (_lib.TensorDesc * len(items))()
    for i, (k, v) in enumerate(items):
        arr[i].name, arr[i].data, arr[i].dtype = k.encode(), v.data_ptr(), _DT[v.dtype]
        arr[i].on_device, arr[i].numel = 1 if v.is_cuda else 0, v.numel()
    torch.cuda.synchronize()
    assert load(hnd, arr, len(items)) == 0, _lib.last_error(lib)


_CACHE = {}
_HANDLES = []       # (destroy, handle) of every plan this module made


@pytest.fixture(scope="module", autouse=True)
def _plans_are_destroyed_at_the_end():
    yield
    torch.cuda.synchronize()
    while _HANDLES:
        destroy, hnd = _HANDLES.pop()
        assert destroy(hnd) == 0
    _CACHE.clear()


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _world(name):
    """One element library ("bf16" / "f16"), a UNet and a ControlNet plan of the tiny configuration with weights, and the
    device tensors of one (B, F, H, W) forward.  Built once, never modified (the tests restore the modes they set)."""
    def make():
        import ctrlv_ref as R
        from ctrlv_amd import _lib
        from ctrlv_amd.plan import config_struct
        from tests.parity_utils import make_inputs, make_pair
        dt = BF if name == "bf16" else HF
        lib = _lib.load(dt)
        cfg = dict(R.TINY_CONFIG)
        _, _, hu, hc = make_pair(cfg, DEV, dtype=dt)
        w = SimpleNamespace(name=name, lib=lib, _lib=_lib, dt=dt, code=_DT[dt])
        for kind, model in (("unet", hu), ("controlnet", hc)):
            c = config_struct(kind, model.config, "sb")
            hnd = ctypes.c_void_p()
            assert lib.ctrlv_plan_create(ctypes.byref(c), 0, ctypes.byref(hnd)) == 0, _lib.last_error(lib)
            _HANDLES.append((lib.ctrlv_plan_destroy, hnd))
            _load(_lib, lib, lib.ctrlv_plan_load_weights, hnd, model.state_dict())
            setattr(w, kind, hnd)
        sample, t, ehs, ids, cond = make_inputs(cfg, B, F, H, W, dtype=dt)
        w.sample, w.cond, w.ehs = sample.to(DEV, dt), cond.to(DEV, dt), ehs.to(DEV, dt)
        w.t, w.ids = t.reshape(1).to(DEV, torch.float32), ids.to(DEV, torch.float32)
        w.n_down = lib.ctrlv_plan_num_down_residuals(w.unet)
        w.shapes = []
        for i in range(w.n_down + 1):
            m, c = ctypes.c_int64(), ctypes.c_int32()
            assert lib.ctrlv_plan_residual_shape(w.unet, i, B, F, H, W, ctypes.byref(m), ctypes.byref(c)) == 0
            w.shapes.append((m.value, c.value))
        g = torch.Generator().manual_seed(17)
        w.res = [(0.1 * torch.randn(m, c, generator=g)).to(DEV, dt) for m, c in w.shapes]
        return w
    return _cached(("world", name), make)


def _set_modes(w, hnd, trunk, ff):
    """(the two modes exclude each other: leave the one before entering the other)"""
    lib = w.lib
    assert lib.ctrlv_plan_set_ff_precision(hnd, 0) == 0 and lib.ctrlv_plan_set_trunk_mode(hnd, 0) == 0, w._lib.last_error(lib)
    assert lib.ctrlv_plan_set_trunk_mode(hnd, trunk) == 0, w._lib.last_error(lib)
    assert lib.ctrlv_plan_set_ff_precision(hnd, ff) == 0, w._lib.last_error(lib)


def _rows(w, idx):
    return [torch.empty(m, c, dtype=w.dt, device=DEV) for m, c in (w.shapes[i] for i in idx)]


def _plan_entry(entry, world):
    """args: the entry's argument list with the workspace pointer and size at [-3], [-2]; i_dtype / i_null: the positions of
    the dtype code and of one required pointer; outs: every tensor the call writes."""
    w = _world(world)
    lib, n = w.lib, w.n_down
    e = SimpleNamespace(lib=lib, _lib=w._lib, world=w, unaligned=None,
                        short=("workspace too small", "ctrlv_plan_workspace_bytes"),
                        bad_dtype="dtype must be 0 (fp32), 1 (fp16) or 2 (bf16)")
    head = [w.sample.data_ptr(), w.code, w.t.data_ptr(), 1, w.ehs.data_ptr(), w.ids.data_ptr(), 3]
    tail = [B, F, H, W, None, 0, _stream()]
    if entry == "unet":
        out = torch.empty(B, F, 4, H, W, dtype=w.dt, device=DEV)
        e.keep = (ctypes.c_void_p * n)(*[r.data_ptr() for r in w.res[:n]])
        e.fn, e.hnd, e.outs = lib.ctrlv_unet_forward, w.unet, [out]
        e.args = [w.unet] + head + [e.keep, w.res[n].data_ptr(), None, out.data_ptr()] + tail
        e.i_dtype, e.i_null, e.null = 2, 1, "unet_forward: null pointer"
        e.wrong_kind = (w.controlnet, "unet_forward: the plan is a ControlNet")
    elif entry == "encoder":
        rows = _rows(w, range(n + 1))
        e.keep = (ctypes.c_void_p * n)(*[r.data_ptr() for r in rows[:n]])
        e.fn, e.hnd, e.outs = lib.ctrlv_unet_encoder_forward, w.unet, rows
        e.args = [w.unet] + head + [e.keep, rows[n].data_ptr()] + tail
        e.i_dtype, e.i_null, e.null = 2, 9, "unet_encoder_forward: null pointer"
        e.wrong_kind = (w.controlnet, "unet_encoder_forward: the plan is a ControlNet")
    else:
        rows = _rows(w, range(n + 1))
        e.keep = (ctypes.c_void_p * n)(*[r.data_ptr() for r in rows[:n]])
        e.fn, e.hnd, e.outs = lib.ctrlv_controlnet_forward, w.controlnet, rows
        e.args = [w.controlnet, head[0], w.cond.data_ptr()] + head[1:] + [0.7, e.keep, rows[n].data_ptr()] + tail
        e.i_dtype, e.i_null, e.null = 3, 2, "controlnet_forward: null pointer (control_cond is required"
        e.wrong_kind = (w.unet, "controlnet_forward: the plan is a UNet")
    e.need = lambda: lib.ctrlv_plan_workspace_bytes(e.hnd, B, F, H, W)
    return e


def _vae_world():
    def make():
        from ctrlv_amd import _lib
        from ctrlv_amd.models import AutoencoderKLTemporalDecoder
        lib = _lib.load()
        torch.manual_seed(5)
        m = AutoencoderKLTemporalDecoder().eval()
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.endswith("mix_factor"):
                    p.fill_(0.4)
        m = m.to(DEV, BF)
        cfg = _lib.VaeConfig()
        cfg.in_channels, cfg.out_channels, cfg.latent_channels, cfg.layers_per_block, cfg.n_blocks = 3, 3, 4, 2, 4
        for i, ch in enumerate((128, 256, 512, 512)):
            cfg.block_out_channels[i] = ch
        cfg.scaling_factor = 0.18215
        hnd = ctypes.c_void_p()
        assert lib.ctrlv_vae_plan_create(ctypes.byref(cfg), 0, ctypes.byref(hnd)) == 0, _lib.last_error(lib)
        _HANDLES.append((lib.ctrlv_vae_plan_destroy, hnd))
        _load(_lib, lib, lib.ctrlv_vae_plan_load_weights, hnd, m.state_dict())
        return SimpleNamespace(lib=lib, _lib=_lib, hnd=hnd)
    return _cached("vae", make)


def _vae_entry(entry):
    w = _vae_world()
    lib = w.lib
    e = SimpleNamespace(lib=lib, _lib=w._lib, hnd=w.hnd, wrong_kind=None, short=("needed", "ctrlv_vae_plan_workspace_bytes"),
                        bad_dtype="dtype codes 7 / 2 (0 fp32, 1 fp16, 2 bf16)", i_dtype=2)
    if entry == "vae_encode":
        x = (torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(DEV, BF)
        lat, mom = torch.empty(1, 4, 8, 8, dtype=BF, device=DEV), torch.empty(1, 8, 8, 8, dtype=BF, device=DEV)
        e.keep, e.fn, e.outs = x, lib.ctrlv_vae_encode, [lat, mom]
        e.args = [w.hnd, x.data_ptr(), 2, 1, 64, 64, None, 0.5, lat.data_ptr(), mom.data_ptr(), 2, None, 0, _stream()]
        e.i_null, e.null, e.unaligned = 1, "vae_encode: null pointer", "vae_encode: workspace must be 256-byte aligned"
        e.need = lambda: lib.ctrlv_vae_plan_workspace_bytes(w.hnd, 0, 1, 0, 64, 64)
    else:
        n, h = 3, 8
        z = torch.randn(n, 4, h, h, generator=torch.Generator().manual_seed(3)).to(DEV, BF)
        out = torch.empty(n, 3, 8 * h, 8 * h, dtype=BF, device=DEV)
        e.keep, e.fn, e.outs = z, lib.ctrlv_vae_decode, [out]
        e.args = [w.hnd, z.data_ptr(), 2, n, n, h, h, out.data_ptr(), 2, None, 0, _stream()]
        e.i_null, e.null, e.unaligned = 7, "vae_decode: null pointer", "vae_decode: workspace must be 256-byte aligned"
        e.need = lambda: lib.ctrlv_vae_plan_workspace_bytes(w.hnd, 1, n, n, h, h)
    return e


def _clip_entry():
    from ctrlv_amd import _lib
    from tests import clip_utils as U
    lib = _lib.load()
    cfg, n, seed = U.CONFIGS["A"]

    def make():
        m = U.build_own(cfg, seed, BF, DEV)
        c = _lib.ClipConfig()
        for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
                  "projection_dim"):
            setattr(c, k, cfg[k])
        c.hidden_act = {"gelu": 0, "quick_gelu": 1}[cfg["hidden_act"]]
        c.layer_norm_eps = cfg["layer_norm_eps"]
        hnd = ctypes.c_void_p()
        assert lib.ctrlv_clip_plan_create(ctypes.byref(c), 0, ctypes.byref(hnd)) == 0, _lib.last_error(lib)
        _HANDLES.append((lib.ctrlv_clip_plan_destroy, hnd))
        _load(_lib, lib, lib.ctrlv_clip_plan_load_weights, hnd, m.state_dict())
        return hnd, U.load_golden()["A"]["pixel_values"].to(DEV)
    hnd, px = _cached("clip", make)
    out = torch.empty(n, cfg["projection_dim"], dtype=BF, device=DEV)
    return SimpleNamespace(
        lib=lib, _lib=_lib, hnd=hnd, keep=px, fn=lib.ctrlv_clip_forward, outs=[out], wrong_kind=None,
        args=[hnd, px.data_ptr(), _DT[px.dtype], n, out.data_ptr(), None, None, 0, _stream()], i_dtype=2, i_null=4,
        null="clip_forward: null pointer", short=("needed", "ctrlv_clip_plan_workspace_bytes"),
        bad_dtype="dtype code 7 (0 fp32, 1 fp16, 2 bf16)", unaligned="clip_forward: workspace must be 256-byte aligned",
        need=lambda: lib.ctrlv_clip_plan_workspace_bytes(hnd, n))


def _entry(entry, world="bf16"):
    if entry in ("unet", "encoder", "controlnet"):
        return _plan_entry(entry, world)
    return _clip_entry() if entry == "clip" else _vae_entry(entry)


def _call(e, ws_ptr, ws_bytes, edits=()):
    a = list(e.args)
    a[-3], a[-2] = ws_ptr, ws_bytes
    for i, v in edits:
        a[i] = v
    return e.fn(*a)


ENTRIES = ["unet", "encoder", "controlnet", "vae_encode", "vae_decode", "clip"]
# the UNet / ControlNet entries align the workspace themselves and refuse a plan of the other kind; the VAE and CLIP entries
# have one kind of plan and want the workspace aligned
REFUSALS = [(e, f) for e in ENTRIES for f in ("short", "dtype", "null")] + \
           [(e, "kind" if e in ENTRIES[:3] else "unaligned") for e in ENTRIES]


@torch.no_grad()
@pytest.mark.parametrize("entry,fault", REFUSALS)
def test_a_refused_call_reports_and_launches_nothing(hip_lib, entry, fault):
    e = _entry(entry)
    need = e.need()
    assert need > 0, e._lib.last_error(e.lib)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    off = -ws.data_ptr() % 256
    base = ws.data_ptr() + off
    for o in e.outs:
        o.fill_(7.0)
    torch.cuda.synchronize()
    if fault == "short":
        rc, want_rc, want = _call(e, base, need - 1), -5, e.short + (str(need),)
    elif fault == "dtype":
        rc, want_rc, want = _call(e, base, need, [(e.i_dtype, 7)]), -4, (e.bad_dtype,)
    elif fault == "null":
        rc, want_rc, want = _call(e, base, need, [(e.i_null, None)]), -1, (e.null,)
    elif fault == "kind":
        rc, want_rc, want = _call(e, base, need, [(0, e.wrong_kind[0])]), -1, (e.wrong_kind[1],)
    else:
        rc, want_rc, want = _call(e, base + 128, need), -1, (e.unaligned,)
    msg = e._lib.last_error(e.lib)
    print(f"{entry} / {fault}: rc {rc}, {msg!r}")
    assert rc == want_rc and all(m in msg for m in want), (rc, msg)
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in e.outs)


def _run(e, ws_ptr, ws_bytes):
    for o in e.outs:
        o.fill_(7.0)
    assert _call(e, ws_ptr, ws_bytes) == 0, e._lib.last_error(e.lib)
    torch.cuda.synchronize()
    return [o.clone() for o in e.outs]


@torch.no_grad()
@pytest.mark.parametrize("entry,world", [("unet", "bf16"), ("controlnet", "bf16"), ("unet", "f16"), ("controlnet", "f16"),
                                         ("encoder", "bf16"), ("vae_encode", "bf16"), ("vae_decode", "bf16")])
def test_a_workspace_of_exactly_the_queried_size_is_enough_and_is_not_overrun(hip_lib, entry, world):
    """(the fp16 library's plans run with the split trunk, mode 1: the workspace holds the lo planes)"""
    e = _entry(entry, world)
    split = world == "f16"
    if split:
        _set_modes(e.world, e.hnd, 1, 0)
    try:
        need = e.need()
        assert need > 0, e._lib.last_error(e.lib)
        roomy = torch.empty(need + (1 << 20), dtype=torch.uint8, device=DEV)
        want = _run(e, roomy.data_ptr(), roomy.numel())
        assert not any(bool((o == 7.0).all()) for o in want)
        big = torch.full((need + 2 * BAND + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        off = BAND + (-(big.data_ptr() + BAND)) % 256
        assert (big.data_ptr() + off) % 256 == 0
        got = _run(e, big.data_ptr() + off, need)
        assert bool((big[off - BAND:off] == 0xA5).all()) and bool((big[off + need:off + need + BAND] == 0xA5).all())
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    finally:
        if split:
            _set_modes(e.world, e.hnd, 0, 0)


def _sizes():
    """{key: bytes} of every size query on the list."""
    out = {}
    for name in ("bf16", "f16"):
        w = _world(name)
        for kind in ("unet", "controlnet"):
            hnd = getattr(w, kind)
            for trunk, ff in MODES[name]:
                _set_modes(w, hnd, trunk, ff)
                for s in PLAN_SHAPES:
                    n = w.lib.ctrlv_plan_workspace_bytes(hnd, *s)
                    assert n > 0, w._lib.last_error(w.lib)
                    out[f"{name}/{kind}/trunk{trunk}/ff{ff}/{'x'.join(map(str, s))}"] = n
            _set_modes(w, hnd, 0, 0)
    v = _vae_world()
    for what, shapes in VAE_SHAPES.items():
        for s in shapes:
            n = v.lib.ctrlv_vae_plan_workspace_bytes(v.hnd, what, *s)
            assert n > 0, v._lib.last_error(v.lib)
            out[f"bf16/vae_{'decode' if what else 'encode'}/{'x'.join(map(str, s))}"] = n
    return out


@torch.no_grad()
def test_workspace_sizes_are_the_recorded_ones(hip_lib):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _sizes()
    assert set(got) == set(want)
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, diff
    # the modes are really on: the lo planes / the e4m3 codes and scales take room
    k = "f16/unet/trunk%d/ff%d/2x3x16x16"
    assert got[k % (1, 0)] > got[k % (0, 0)] and got[k % (0, 1)] >= got[k % (0, 0)]


if __name__ == "__main__":
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_plan_entries_gpu.py --record FILE"
    with torch.no_grad():
        sizes = _sizes()
    with open(sys.argv[2], "w") as f:
        json.dump(sizes, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(sizes)} sizes into {sys.argv[2]}")
