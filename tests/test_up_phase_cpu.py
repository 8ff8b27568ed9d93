"""Phase form of the nearest-x2 upsampler conv (ctrlv_gemm_desc.up = 2), the parts that need no GPU: the identity itself in
fp64, the packer's tap-to-phase table (read from include/ctrlv_hip.h) against it, the layer predicate's independence of the
image count, and the register budget of the new ping-pong instantiations."""
import os
import re
import subprocess
import tempfile

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_tap_table():
    """KY(parity, a) -> taps, as the header documents it for ctrlv_pack_up_phase_weight"""
    src = open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read()
    doc = src[src.index("Phase weights of such a conv"):src.index("int ctrlv_pack_up_phase_weight")]
    doc = re.sub(r"\n\s*\*", " ", doc)
    table = {(int(p), int(a)): tuple(int(k) for k in ks.split(","))
             for p, a, ks in re.findall(r"KY\((\d), (\d)\)\s*=\s*\{([\d, ]+)\}", doc)}
    assert sorted(table) == [(0, 0), (0, 1), (1, 0), (1, 1)], table
    return table


def pack_phase_weights(w, table):
    """[N, C, 3, 3] -> [4, N, 4 C]: panel p = 2 py + px, column (2 a + b) C + c"""
    N, C = w.shape[:2]
    out = torch.zeros(4, N, 4 * C, dtype=w.dtype)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    s = sum(w[:, :, ky, kx] for ky in table[(py, a)] for kx in table[(px, b)])
                    out[2 * py + px, :, (2 * a + b) * C:(2 * a + b + 1) * C] = s
    return out


def phase_convs(x, wph, bias):
    """out[2 i + py, 2 j + px] = sum_{a, b} W[p][.][(2 a + b) C + c] x[i - 1 + py + a, j - 1 + px + b][c] (zero outside)"""
    n, C, H, W = x.shape
    N = wph.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.empty(n, N, 2 * H, 2 * W, dtype=x.dtype)
    for p in range(4):
        py, px = p >> 1, p & 1
        w = wph[p].reshape(N, 2, 2, C).permute(0, 3, 1, 2)
        out[:, :, py::2, px::2] = F.conv2d(xp, w, bias)[:, :, py:py + H, px:px + W]
    return out


@pytest.mark.parametrize("n,C,N,H,W", [(1, 3, 2, 1, 1), (2, 2, 3, 1, 3), (2, 4, 5, 3, 5), (1, 8, 8, 4, 16)])
def test_identity_and_tap_table_fp64(n, C, N, H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(n, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(N, C, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(N, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    got = phase_convs(x, pack_phase_weights(w, header_tap_table()), b)
    assert float((got - ref).abs().max()) < 1e-12


def test_tap_table_covers_every_tap_once_per_parity():
    t = header_tap_table()
    for p in (0, 1):
        assert sorted(t[(p, 0)] + t[(p, 1)]) == [0, 1, 2]
    # parity 0: the row above through w[0], the row itself through w[1] + w[2]; parity 1: w[0] + w[1], then w[2] below
    assert t == {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def _desc(_lib, n_img, H, W, C, N):
    d = _lib.GemmDesc()
    d.A, d.W, d.out, d.bias = 0x1000, 0x2000, 0x3000, 0x4000          # (host logic only: never dereferenced)
    d.M, d.N, d.Cin, d.taps, d.mode = n_img * 4 * H * W, N, C, 9, 1
    d.lda, d.ldo, d.n_store = C, N, N
    d.H, d.Wd, d.Ho, d.Wo, d.stride, d.up = H, W, 2 * H, 2 * W, 1, 1
    d.s_acc = d.s1 = d.s2 = 1.0
    d.vdiv, d.vmod, d.vS = 1, 1 << 30, 1
    return d


def test_predicate_is_a_function_of_the_layer():
    import ctypes

    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import _lib
    lib = _lib.load()
    serves = lambda d: lib.ctrlv_gemm_up_phase_serves(ctypes.byref(d))   # noqa: E731
    for n in (1, 2, 50, 400):
        for (H, W, C) in ((9, 16, 1280), (18, 32, 1280), (36, 64, 640), (5, 8, 1280), (3, 16, 64)):
            assert serves(_desc(_lib, n, H, W, C, C)), (n, H, W, C)
        assert not serves(_desc(_lib, n, 9, 12, 64, 64))              # row width no power of two
        assert not serves(_desc(_lib, n, 9, 16, 96, 64))              # Cin no multiple of 64
        d = _desc(_lib, n, 9, 16, 64, 64)
        d.R1, d.ldr1 = 0x5000, 64                                      # bias-only epilogue
        assert not serves(d)
        d = _desc(_lib, n, 9, 16, 64, 64)
        d.stride, d.up, d.Ho, d.Wo = 1, 0, 9, 16                       # not an up-sampler
        assert not serves(d)
    # the launch plan never splits such a conv's contraction, whatever the image is
    d = _desc(_lib, 50, 5, 8, 1280, 1280)
    d.up = 2
    assert lib.ctrlv_gemm_splitk_ws_bytes(ctypes.byref(d)) == 0


def test_phase_kernels_register_budget():
    """The 256x320 phase instantiations (csrc/gemm_pp_up.hip; plain, and with split planes in the fp16 library) keep the budget
    tests/test_build_resources.py pins for the tile: <= 256 VGPRs, two waves per SIMD, nothing in scratch."""
    procs = []
    with tempfile.TemporaryDirectory() as td:
        for defs in ([], ["-DCTRLV_ELEM_F16=1"]):
            asm = os.path.join(td, "up" + ("16" if defs else "") + ".s")
            cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                   "-Rpass-analysis=kernel-resource-usage", *defs, os.path.join(ROOT, "ctrlv_amd", "csrc", "gemm_pp_up.hip"), "-o", asm]
            procs.append((defs, asm, subprocess.Popen(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True)))
        for defs, asm, p in procs:
            err = p.communicate()[1]
            assert p.returncode == 0, err[-2000:]
            names = re.findall(r"Function Name: (\S+)", err)
            vg = [int(x) for x in re.findall(r" VGPRs: (\d+)", err)]
            sp = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", err)]
            sc = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
            occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", err)]
            kern = [(n, v, s, c, o) for n, v, s, c, o in zip(names, vg, sp, sc, occ) if "gemm_pp_kernel" in n]
            assert len(kern) == (2 if defs else 1), (defs, names)
            for n, v, s, c, o in kern:
                assert v <= 256 and o >= 2 and s == 0 and c == 0, (n, v, s, c, o)
            assert "scratch_" not in open(asm).read()
