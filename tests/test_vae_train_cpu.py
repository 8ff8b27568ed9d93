"""CPU checks of the VAE decoder fine-tuning path: the public names and signatures, the argument errors of
`vae_train_step` (raised before any kernel call), the two new C-ABI entry points in header / ctypes / library, and the
bench tool's command line."""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ctrlv_softmax_rows_bwd", "ctrlv_time_conv_rows_to_nchw_bwd")


def test_new_names_and_signatures():
    from ctrlv_amd import autograd, ops, training
    sig = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert sig(autograd.vae_res_block_train_forward) == ["block", "x", "n_clips", "F", "H", "W"]
    assert sig(autograd.vae_attention_train_forward) == ["attn", "x", "n", "H", "W"]
    assert issubclass(autograd.TimeConvOut, torch.autograd.Function)
    assert sig(training.vae_decoder_train_forward) == ["decoder", "z", "num_frames"]
    p = inspect.signature(training.vae_train_step).parameters
    assert list(p) == ["vae", "batch", "optimizer", "num_frames", "sample_posterior", "generator", "world_size", "buckets",
                       "accumulate", "loss_scale"]
    assert [p[k].default for k in list(p)[2:]] == [None, 1, True, None, 1, None, False, 1.0]
    assert callable(ops.softmax_rows_bwd) and callable(ops.time_conv_rows_to_nchw_bwd)
    # the opt-in switch of BlendGemm and the host-sigmoid prefetch are additions: the defaults are the old calls
    assert inspect.signature(autograd.prefetch_mix_factors).parameters["host_sigmoid"].default is False


def test_vae_train_step_argument_errors_come_before_any_kernel(monkeypatch):
    from ctrlv_amd import _lib
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    from ctrlv_amd.training import vae_decoder_train_forward, vae_train_step

    def no_kernels(*a, **k):
        raise AssertionError("a kernel library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_kernels)
    vae = AutoencoderKLTemporalDecoder(block_out_channels=(64, 64), down_block_types=("DownEncoderBlock2D",) * 2,
                                       layers_per_block=1)
    px = torch.zeros(4, 3, 64, 64)
    with pytest.raises(ValueError, match="whole clips"):
        vae_train_step(vae, {"pixel_values": px}, num_frames=3)
    with pytest.raises(ValueError, match="not served"):                  # (CPU tensors: vae_decoder_hip.supports refuses)
        vae_train_step(vae, {"pixel_values": px}, num_frames=2)
    with pytest.raises(ValueError, match="pixel_values"):
        vae_train_step(vae, {"pixel_values": px[:, :2]}, num_frames=2)
    with pytest.raises(ValueError, match="whole clips"):
        vae_decoder_train_forward(vae.decoder, torch.zeros(3, 4, 8, 8), 2)
    with pytest.raises(ValueError, match="not served"):
        vae_decoder_train_forward(vae.decoder, torch.zeros(4, 4, 8, 8), 2)


def test_header_ctypes_and_library_agree_on_the_new_entry_points():
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import _lib
    src = open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert _lib.ABI_VERSION == 22
    for dt in (torch.bfloat16, torch.float16):
        lib = _lib.load(dt)
        assert lib.ctrlv_abi_version() == 22
        for name in NEW:
            m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
            assert m, name
            assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
            assert getattr(lib, name) is not None
    assert re.search(r"#define\s+CTRLV_TIME_CONV_BWD_SCRATCH_FLOATS\s+(\d+)", src).group(1) == \
        str(__import__("ctrlv_amd.ops", fromlist=["x"]).TIME_CONV_BWD_SCRATCH_FLOATS)
    # host-side argument checks of the two entry points need no GPU
    import ctypes
    lib = _lib.load()
    p8 = ctypes.c_void_p(8)
    with pytest.raises(ValueError, match="multiple of 4"):
        _lib.check(lib.ctrlv_softmax_rows_bwd(p8, 64, p8, 64, 4, 62, 1.0, p8, 64, None), "softmax_rows_bwd")
    with pytest.raises(ValueError, match="whole clips"):
        _lib.check(lib.ctrlv_time_conv_rows_to_nchw_bwd(p8, p8, 4, 5, 2, 3, 64, p8, p8, 4, p8, p8, p8, None), "time_conv_bwd")
    with pytest.raises(ValueError, match="channels"):
        _lib.check(lib.ctrlv_time_conv_rows_to_nchw_bwd(p8, p8, 8, 4, 2, 5, 64, p8, p8, 8, p8, p8, p8, None), "time_conv_bwd")


def test_train_vae_bench_help_parses():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_vae_bench.py"), "--help"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--height", "--width", "--batch", "--num-frames", "--steps"):
        assert flag in out.stdout
