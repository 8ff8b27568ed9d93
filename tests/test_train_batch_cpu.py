"""Training batches (include/ctrlv_hip.h: ctrlv_train_draws, ctrlv_train_assemble, ctrlv_resize_antialias_clamped,
ctrlv_train_batch_prepare) where no GPU is needed: the numpy restatements of tests/train_batch_ref.py against known answers and
against torch's own expressions, the condition the GPU tests' seed must meet, the symbols and the struct mirror, and the
driver's host-side refusals -- each names what it refuses and comes before anything would be launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as g
from tests import seeded_ref as S
from tests import train_batch_ref as T
from tests.test_pipeline_plan_cpu import CLIP_CFG, VAE_CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ctrlv_resize_antialias_clamped", "ctrlv_train_draws", "ctrlv_train_assemble", "ctrlv_train_batch_workspace_bytes",
       "ctrlv_train_batch_prepare")
# the seed, first clip and step of the GPU tests' draws (tests/test_train_batch_gpu.py): see test_the_seed_covers_all_four_regions
SEED, CLIP0, CALL, DP, CLIPS = 0x5EEDBA7C4C0FFEE5, 5, 7, 0.25, 64


# ----------------------------------------------------------------------------------------------------------- the restatements
def test_philox_known_answers_of_the_header():
    cases = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
              (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)))
    for counter, key, want in cases:
        got = S.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
        assert tuple(int(v[0]) for v in got) == want, (counter, key)


def test_the_index_formula():
    assert int(T.index_of(0, 1000)) == 0 and int(T.index_of(0, 7)) == 0
    assert int(T.index_of(2 ** 32 - 1, 1000)) == 999 and int(T.index_of(2 ** 32 - 1, 7)) == 6
    assert int(T.index_of(2 ** 32 - 1, 1)) == 0 and int(T.index_of(2 ** 32 - 1, 65536)) == 65535
    assert int(T.index_of(2 ** 31, 7)) == 3 and int(T.index_of(2 ** 31, 1000)) == 500
    for size in (7, 1000):
        table = np.arange(size, dtype=np.float32)
        d = T.draws(SEED, 4096, table, -table, clip0=CLIP0, call=CALL)
        idx = d["indices"]
        assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < size
        assert len(np.unique(idx)) == size if size == 7 else len(np.unique(idx)) > 900       # every bucket of 7 is hit
        assert np.array_equal(d["sigmas"], table[idx]) and np.array_equal(d["timesteps"], -table[idx])
        assert d["random_p"].dtype == np.float32 and d["random_p"].min() >= 2.0 ** -33 and d["random_p"].max() <= 1.0


@pytest.mark.parametrize("dp", [0.25, 0.1, 0.3, 1.0 / 3.0])
def test_the_masks_are_torchs_expressions(dp):
    """On p values that include both fp32 neighbours of dp, 2 dp and 3 dp (and the rounded thresholds themselves): torch compares
    the fp32 tensor with the Python products 2 * dp and 3 * dp, as train_video_controlnet.py:425-439 writes them."""
    pts = [0.0, 2.0 ** -33, 1.0, 0.5]
    for t in T.thresholds(dp):
        pts += [t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(4))]
    p = np.array(pts, dtype=np.float32)
    keep, image = T.masks(p, dp)
    random_p = torch.from_numpy(p)
    prompt_mask = random_p < 2 * dp
    image_mask = 1 - ((random_p >= dp).to(torch.float32) * (random_p < 3 * dp).to(torch.float32))
    assert np.array_equal(keep, (~prompt_mask).to(torch.float32).numpy())
    assert np.array_equal(image, image_mask.numpy())
    assert set(np.unique(keep)) <= {0.0, 1.0} and set(np.unique(image)) <= {0.0, 1.0}
    ones = T.masks(p, None)
    assert ones[0].min() == 1.0 and ones[1].min() == 1.0 and T.masks(p, -1.0)[1].min() == 1.0


def test_the_assembly_is_noised_inputs_bit_for_bit():
    """The first two lines of the arithmetic against ctrlv_amd.training._noised_inputs on the CPU (layout 0, mask 1: its
    image_latents are the image latent repeated), sigmas over the scheduler's whole range; then the timesteps of the table."""
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    from ctrlv_amd.training import _noised_inputs
    sched = EulerDiscreteScheduler()
    gen = torch.Generator().manual_seed(3)
    n, F, L, h, w = 1000, 2, 4, 3, 5
    lat, noise = torch.randn(n, F, L, h, w, generator=gen), torch.randn(n, F, L, h, w, generator=gen)
    first = torch.randn(n, L, h, w, generator=gen)
    sig = sched.sigmas[:-1].clone()
    batch = {"latents": lat, "noise": noise, "sigmas": sig, "image_latents": first.unsqueeze(1).repeat(1, F, 1, 1, 1)}
    _, _, noisy, timesteps, sample = _noised_inputs(batch)
    got_noisy, got_sample = T.assemble(lat.numpy(), noise.numpy(), sig.numpy(), None, first.numpy(), el="bf16")
    assert np.array_equal(got_noisy.view(np.uint32), noisy.numpy().view(np.uint32))
    assert np.array_equal(got_sample.view(np.uint32), sample.float().numpy().view(np.uint32))
    assert np.array_equal(timesteps.numpy().view(np.uint32), sched.timesteps.numpy().view(np.uint32))
    # fp16 elements and the layouts: against the same expressions written with torch
    cond = torch.randn(n, F, L, h, w, generator=gen)
    mask = (torch.rand(n, generator=gen) < 0.5).float()
    for K in (0, 1, F):
        c = first.unsqueeze(1).repeat(1, F, 1, 1, 1)
        c[:, :K] = cond[:, :K]
        c[:, F - 1] = cond[:, F - 1]
        want = torch.cat([noisy / (sig.view(n, 1, 1, 1, 1) ** 2 + 1) ** 0.5, mask.view(n, 1, 1, 1, 1) * c], dim=2).to(torch.float16)
        got = T.assemble(lat.numpy(), noise.numpy(), sig.numpy(), mask.numpy(), first.numpy(), cond.numpy(), 1, K, el="fp16")[1]
        assert np.array_equal(got.view(np.uint32), want.float().numpy().view(np.uint32)), K


def test_the_seed_covers_all_four_regions():
    """The condition the GPU tests rely on: with dropout 0.25, the 64 clips from CLIP0 of (SEED, CALL) fall into all four regions
    of p -- both conditions dropped, the prompt alone, the image alone, neither."""
    table = np.arange(1000, dtype=np.float32)
    d = T.draws(SEED, CLIPS, table, table, clip0=CLIP0, call=CALL, dropout_prob=DP)
    p, keep, image = d["random_p"], d["prompt_keep"], d["image_mask"]
    regions = [(p < 0.25), (p >= 0.25) & (p < 0.5), (p >= 0.5) & (p < 0.75), (p >= 0.75)]
    assert all(int(r.sum()) > 0 for r in regions), [int(r.sum()) for r in regions]
    assert np.array_equal(keep, (p >= 0.5).astype(np.float32))
    assert np.array_equal(image, 1 - ((p >= 0.25) & (p < 0.75)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def libs():
    g.build()
    from ctrlv_amd import _lib
    return {torch.bfloat16: _lib.load(torch.bfloat16), torch.float16: _lib.load(torch.float16)}


def test_both_libraries_export_the_new_symbols_at_the_same_abi(libs):
    from ctrlv_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read(), flags=re.S)
    for dt, lib in libs.items():
        assert lib.ctrlv_abi_version() == 22 == _lib.ABI_VERSION
        for name in NEW:
            assert re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(", header), name
            assert name in _lib.SIGNATURES and getattr(lib, name) is not None, (dt, name)


def test_the_request_mirror_has_the_c_layout():
    """Names in header order and the offsets of the C struct's natural layout."""
    from ctrlv_amd import _lib
    src = open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read()
    body = src[src.index("typedef struct ctrlv_train_batch_request {"):src.index("} ctrlv_train_batch_request;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    sizes = {"int32_t": 4, "uint32_t": 4, "float": 4, "double": 8, "uint64_t": 8}
    off, names = 0, []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = " ".join(decl.split(",")[0].split()[:-1])
        for part in decl.split(","):
            name = part.strip().split()[-1]
            count = 1
            if "[" in name:
                name, count = name[:name.index("[")], int(name[name.index("[") + 1:-1])
            size = 8 if name.startswith("*") or base.endswith("*") else sizes[base.replace("const ", "")]
            name = name.lstrip("*")
            off = (off + size - 1) // size * size
            assert getattr(_lib.TrainBatchRequest, name).offset == off, (name, off)
            names.append(name)
            off += size * count
    assert names == [f[0] for f in _lib.TrainBatchRequest._fields_]
    assert ctypes.sizeof(_lib.TrainBatchRequest) == (off + 7) // 8 * 8


def _request(_lib, **over):
    """A request every field of which passes validation (no pointer is dereferenced on the host)."""
    r = _lib.TrainBatchRequest()
    r.n_clips, r.num_frames, r.height, r.width = 2, 3, 64, 64
    r.clips, r.box_frames, r.clips_dtype, r.box_dtype = 0x1000, 0x2000, 0, 2
    r.mode, r.num_cond_frames, r.dropout_prob = 0, 1, 0.1
    r.seed, r.clip_index0, r.call = 5, 0, 1
    r.sigma_table, r.timestep_table, r.table_size = 0x3000, 0x4000, 1000
    r.sample_dtype = 0
    for i, name in enumerate(("target_latents", "noisy_latents", "sample", "control_cond", "encoder_hidden_states", "sigmas",
                              "timesteps", "indices", "random_p")):
        setattr(r, name, 0x10000 + 0x1000 * i)
    for k, v in over.items():
        setattr(r, k, v)
    return r


def test_the_driver_refuses_by_name_before_anything_else(libs):
    """prepare and its workspace query alike.  The valid request reaches the last gate ("not loaded": these plans have no
    weights), which proves that every field check sits in front of it; the workspace is held against the driver's own buffers
    before that gate, which needs no weights either."""
    from ctrlv_amd import _lib
    from ctrlv_amd.plan import ClipPlan, VaePlan
    for dt, lib in libs.items():
        vae, clip = VaePlan(VAE_CFG, "cpu", dtype=dt), ClipPlan(CLIP_CFG, "cpu", dtype=dt)
        ws = ctypes.c_void_p(0x100000)

        def refused(r, word, code=None, ws=ws, ws_bytes=1 << 40, v=vae._h, c=clip._h, query=True):
            ref = ctypes.byref(r) if r is not None else None
            if query:
                assert lib.ctrlv_train_batch_workspace_bytes(v, c, ref) == 0
                assert word in _lib.last_error(lib), (word, _lib.last_error(lib))
            rc = lib.ctrlv_train_batch_prepare(v, c, ref, ws, ws_bytes, None)
            msg = _lib.last_error(lib)
            assert rc < 0 and word in msg, (word, rc, msg)
            assert code is None or rc == code, (word, rc)

        ok = lambda **kw: _request(_lib, **kw)        # noqa: E731
        refused(ok(), "not loaded")
        refused(ok(mode=1, box_frames=None, control_cond=None), "not loaded")
        refused(ok(mode=2, control_cond=None, num_cond_frames=3), "not loaded")               # K = F
        refused(ok(dropout_prob=-1.0, sample_dtype=lib.ctrlv_elem_dtype()), "not loaded")
        refused(ok(reserved=1), "reserved", code=-1)
        refused(ok(sigma_table=None), "sigma_table", code=-1)
        refused(ok(timestep_table=None), "timestep_table", code=-1)
        for size in (0, -1, 65537):
            refused(ok(table_size=size), "table_size", code=-2)
        for K in (-1, 4):
            refused(ok(mode=2, control_cond=None, num_cond_frames=K), "num_cond_frames", code=-2)
        refused(ok(box_frames=None), "box_frames is null", code=-1)                            # mode 0 without box frames
        refused(ok(mode=2, control_cond=None, box_frames=None), "box_frames is null", code=-1)
        refused(ok(mode=1, control_cond=None), "box_frames is set", code=-1)
        refused(ok(control_cond=None), "control_cond is null", code=-1)
        refused(ok(mode=1, box_frames=None), "control_cond is set", code=-1)
        refused(ok(mode=3), "mode", code=-1)
        refused(ok(num_frames=33), "num_frames", code=-2)
        refused(ok(n_clips=0), "n_clips", code=-2)
        refused(ok(height=36), "height", code=-2)
        refused(ok(height=8, width=8), "latent pixels", code=-2)
        refused(ok(height=32, width=32), "latent pixels", code=-2)      # 16 latent pixels: the VAE's attention takes multiples of 64
        refused(ok(clips=None), "clips is null", code=-1)
        refused(ok(clips_dtype=3), "clips_dtype", code=-4)
        refused(ok(box_dtype=-1), "box_dtype", code=-4)
        refused(ok(sample_dtype=3 - lib.ctrlv_elem_dtype()), "sample_dtype", code=-4)          # the other library's element code
        refused(ok(dropout_prob=float("nan")), "dropout_prob", code=-1)
        refused(ok(scaling_factor=-1.0), "scaling_factor", code=-1)
        refused(ok(clip_std=(ctypes.c_float * 3)(1.0, 0.0, 1.0)), "clip_std", code=-1)
        refused(ok(sigmas=None), "null output", code=-1)
        refused(ok(sample=0x10001), "aligned", code=-1)
        refused(None, "null request", code=-1)
        refused(ok(), "VAE plan is null", code=-1, v=None)
        refused(ok(), "CLIP plan is null", code=-1, c=None)
        # the workspace: null, misaligned, smaller than the driver's own buffers (host arithmetic, no weights needed)
        refused(ok(), "256-byte aligned", code=-1, ws=None, query=False)
        refused(ok(), "256-byte aligned", code=-1, ws=ctypes.c_void_p(0x100010), query=False)
        for small in (0, 256, 4096):
            refused(ok(), "ws_bytes", code=-5, ws_bytes=small, query=False)
        # (the plans of device 1 are host objects like the others)
        other = ClipPlan(CLIP_CFG, "cuda:1", dtype=dt)
        refused(ok(), "different devices", code=-1, c=other._h)


def test_the_kernels_validate_on_the_host(libs):
    from ctrlv_amd import _lib
    for lib in libs.values():
        p = ctypes.c_void_p(0x1000)
        el = lib.ctrlv_elem_dtype()
        draws = lambda *a: lib.ctrlv_train_draws(5, 0, 0, *a, None)        # noqa: E731
        assert draws(4, None, p, 7, 0.1, p, p, p, p, p, p) == -1 and "sigma_table" in _lib.last_error(lib)
        assert draws(4, p, p, 0, 0.1, p, p, p, p, p, p) == -2 and "T=0" in _lib.last_error(lib)
        assert draws(4, p, p, 65537, 0.1, p, p, p, p, p, p) == -2 and "T=" in _lib.last_error(lib)
        assert draws(0, p, p, 7, 0.1, p, p, p, p, p, p) == -2 and "n_clips" in _lib.last_error(lib)
        assert draws(4, p, p, 7, float("inf"), p, p, p, p, p, p) == -1 and "dropout_prob" in _lib.last_error(lib)
        assert draws(4, p, p, 7, 0.1, None, None, None, None, None, None) == -1 and "every output" in _lib.last_error(lib)
        asm = lambda t, cf, ci, layout, K, n, F, L, h, w, dt: lib.ctrlv_train_assemble(        # noqa: E731
            t, None, p, None, cf, ci, layout, K, n, F, L, h, w, 5, 0, 0, p, p, dt, None, None)
        assert asm(None, None, p, 0, 0, 1, 3, 4, 4, 4, 0) == -1 and "null pointer" in _lib.last_error(lib)
        assert asm(p, None, p, 2, 0, 1, 3, 4, 4, 4, 0) == -1 and "layout" in _lib.last_error(lib)
        assert asm(p, None, p, 1, 0, 1, 3, 4, 4, 4, 0) == -1 and "cond_frames" in _lib.last_error(lib)
        assert asm(p, p, p, 1, 4, 1, 3, 4, 4, 4, 0) == -2 and "K=4" in _lib.last_error(lib)
        assert asm(p, None, p, 0, 0, 1, 33, 4, 4, 4, 0) == -2 and "F=33" in _lib.last_error(lib)
        assert asm(p, None, p, 0, 0, 1, 3, 9, 4, 4, 0) == -2 and "L=9" in _lib.last_error(lib)
        assert asm(p, None, p, 0, 0, 1, 3, 4, 0, 4, 0) == -2 and "h=0" in _lib.last_error(lib)
        assert asm(p, None, p, 0, 0, 1, 3, 4, 4, 4, 3 - el) == -4 and "sample dtype" in _lib.last_error(lib)
        assert asm(ctypes.c_void_p(0x1002), None, p, 0, 0, 1, 3, 4, 4, 4, 0) == -1 and "aligned" in _lib.last_error(lib)
        f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
        assert lib.ctrlv_resize_antialias_clamped(p, 0, 1, 8, 8, p, 0, 4, 4, None, None, None) == -1
        assert "mean and std are required" in _lib.last_error(lib)
        assert lib.ctrlv_resize_antialias_clamped(p, 0, 1, 80, 8, p, 0, 4, 4, f3, f3, None) == -2        # a factor above 8
