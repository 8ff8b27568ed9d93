"""Host-side tests (no GPU) of the VAE plan (csrc/vae_plan.hip): the ABI table, plan creation and its size rules, the
"not loaded" answers, and the CTRLV_VAE_HIP route switch of AutoencoderKLTemporalDecoder.encode / decode."""
import ctypes
import os
import re
import types

import pytest
import torch

import __graft_entry__ as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ctrlv_vae_plan_create", "ctrlv_vae_plan_load_weights", "ctrlv_vae_plan_workspace_bytes", "ctrlv_vae_encode",
       "ctrlv_vae_decode", "ctrlv_vae_plan_destroy", "ctrlv_vae_posterior"]
SVD = dict(in_channels=3, out_channels=3, latent_channels=4, layers_per_block=2, block_out_channels=(128, 256, 512, 512),
           scaling_factor=0.18215)


def _libs():
    g.build()
    from ctrlv_amd import _lib
    return _lib, (_lib.load(), _lib.load(torch.float16))


def _cfg(_lib, **over):
    d = dict(SVD, **over)
    c = _lib.VaeConfig()
    for k in ("in_channels", "out_channels", "latent_channels", "layers_per_block"):
        setattr(c, k, d[k])
    c.n_blocks = len(d["block_out_channels"])
    for i, ch in enumerate(d["block_out_channels"]):
        c.block_out_channels[i] = ch
    c.scaling_factor = d["scaling_factor"]
    c.offset_limit_bytes = d.get("offset_limit_bytes", 0)
    return c


def test_new_entry_points_are_declared_bound_and_exported():
    _lib, libs = _libs()
    header = open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\b(?:int|size_t)\s+(ctrlv_\w+)\s*\(([^)]*)\)", header)}
    for name in NEW:
        assert name in _lib.SIGNATURES and name in declared, name
        assert len(declared[name].split(",")) == len(_lib.SIGNATURES[name][1]), name
        for lib in libs:
            assert getattr(lib, name) is not None
    assert _lib.ABI_VERSION == 22 and all(lib.ctrlv_abi_version() == 22 for lib in libs)       # additive entry points
    assert _lib.SIGNATURES["ctrlv_vae_plan_workspace_bytes"][0] is ctypes.c_size_t
    assert "vae_plan.hip" in g.HIP_SOURCES
    # the struct mirror: 13 int32, a float, and the 8-byte aligned limit
    assert ctypes.sizeof(_lib.VaeConfig) == 64 and _lib.VaeConfig.offset_limit_bytes.offset == 56


def test_vae_plan_create_validates_on_the_host():
    _lib, libs = _libs()
    for lib in libs:
        h = ctypes.c_void_p()
        c = _cfg(_lib)
        _lib.check(lib.ctrlv_vae_plan_create(ctypes.byref(c), 0, ctypes.byref(h)), "create")
        assert h.value
        for what in (0, 1):
            assert lib.ctrlv_vae_plan_workspace_bytes(h, what, 3, 3, 64, 64) == 0
            assert "not loaded" in _lib.last_error(lib)
        assert lib.ctrlv_vae_decode(h, 0x1000, 2, 3, 3, 8, 8, 0x1000, 2, 0x1000, 1 << 30, None) == -1
        assert "not loaded" in _lib.last_error(lib)
        assert lib.ctrlv_vae_encode(h, 0x1000, 2, 1, 64, 64, None, 1.0, 0x1000, None, 2, 0x1000, 1 << 30, None) == -1
        assert "not loaded" in _lib.last_error(lib)
        assert lib.ctrlv_vae_plan_destroy(h) == 0
        bad = [
            (dict(block_out_channels=(128, 256, 500, 512)), "block_out_channels\\[2\\]=500"),     # not a multiple of 64
            (dict(block_out_channels=(128, 256, 512)), "n_blocks=3"),                               # three down blocks
            (dict(latent_channels=9), "latent_channels=9"),
            (dict(in_channels=9), "in_channels=9"),
            (dict(out_channels=5), "out_channels=5"),
            (dict(layers_per_block=0), "layers_per_block=0"),
            (dict(offset_limit_bytes=1 << 33), "offset_limit_bytes"),
        ]
        for over, what in bad:
            h = ctypes.c_void_p()
            c = _cfg(_lib, **over)
            with pytest.raises(ValueError, match=what):
                _lib.check(lib.ctrlv_vae_plan_create(ctypes.byref(c), 0, ctypes.byref(h)), "create")
            assert not h.value
        assert lib.ctrlv_vae_plan_destroy(None) == 0
        with pytest.raises(ValueError, match="null"):
            _lib.check(lib.ctrlv_vae_plan_create(None, 0, None), "create")


def test_route_switch(monkeypatch):
    """CTRLV_VAE_HIP unset / 1 -> the per-op executors, plan -> the one-call plan, 0 -> the torch modules; a CPU tensor never
    takes a HIP route.  The executors are replaced by recorders: what is tested is the dispatch."""
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    from ctrlv_amd.models import vae_decoder_hip as vh
    from ctrlv_amd.models import vae_encoder_hip as ve
    m = AutoencoderKLTemporalDecoder(block_out_channels=(64, 64, 64, 64)).eval()
    seen = []
    mom, img = torch.zeros(2, 8, 1, 1), torch.zeros(2, 3, 8, 8)
    monkeypatch.setattr(ve, "supports", lambda *a, **k: True)
    monkeypatch.setattr(vh, "supports", lambda *a, **k: True)
    monkeypatch.setattr(ve, "encode", lambda enc, x, **k: (seen.append("ops"), mom)[1])
    monkeypatch.setattr(ve, "encode_plan", lambda vae, x, **k: (seen.append("plan"), (None, mom))[1])
    monkeypatch.setattr(vh, "decode", lambda dec, z, nf: (seen.append("ops"), img)[1])
    monkeypatch.setattr(vh, "decode_plan", lambda vae, z, nf, **k: (seen.append("plan"), img)[1])
    monkeypatch.setattr(m.encoder, "forward", lambda x: (seen.append("torch"), mom)[1])
    monkeypatch.setattr(m.decoder, "forward", lambda z, nf: (seen.append("torch"), img)[1])
    on_gpu = types.SimpleNamespace(is_cuda=True, dtype=torch.bfloat16, shape=(2, 4, 1, 1))     # only the gate reads it
    on_cpu = types.SimpleNamespace(is_cuda=False, dtype=torch.float32, shape=(2, 4, 1, 1))
    with torch.no_grad():
        for value, want in ((None, "ops"), ("1", "ops"), ("0", "torch"), ("plan", "plan")):
            if value is None:
                monkeypatch.delenv("CTRLV_VAE_HIP", raising=False)
            else:
                monkeypatch.setenv("CTRLV_VAE_HIP", value)
            assert vh.route() == want
            del seen[:]
            assert m.encode(on_gpu).latent_dist.mode().shape == (2, 4, 1, 1)
            assert m.decode(on_gpu, num_frames=2).sample is img
            assert seen == [want, want], (value, seen)
            del seen[:]
            m.encode(on_cpu), m.decode(on_cpu, num_frames=2)
            assert seen == ["torch", "torch"], (value, seen)
    # autograd keeps the torch modules, whatever the switch says
    monkeypatch.setenv("CTRLV_VAE_HIP", "plan")
    del seen[:]
    with torch.enable_grad():
        m.decode(on_gpu, num_frames=2)
    assert seen == ["torch"]
