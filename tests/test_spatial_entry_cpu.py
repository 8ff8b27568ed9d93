"""Host-side checks of the fused spatial-transformer entry (csrc/spatial_entry_fused.hip): its register budget in both element
builds and its predicate, which reads shapes and operand presence only (no device needed)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctrlv_amd", "csrc")


def test_spatial_entry_fused_register_budget():
    """A wave keeps its 32 x 320 input rows (80 registers) and the rounded h0 rows (80) beside two accumulator blocks and the
    rotating weight fragments: two waves per SIMD, and nothing spilled -- a scratch reload is a vmcnt(0) that drains the
    LDS-DMA ring."""
    procs = []
    with tempfile.TemporaryDirectory() as td:
        for defs in ([], ["-DCTRLV_ELEM_F16=1"]):
            asm = os.path.join(td, "se" + ("16" if defs else "") + ".s")
            cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                   "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", *defs, os.path.join(CSRC, "spatial_entry_fused.hip"),
                   "-o", asm]
            procs.append((defs, asm, subprocess.Popen(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True)))
        for defs, asm, p in procs:
            err = p.communicate()[1]
            assert p.returncode == 0, err[-2000:]
            names = re.findall(r"Function Name: (\S+)", err)
            vg = [int(x) for x in re.findall(r" VGPRs: (\d+)", err)]
            sp = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", err)]
            occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", err)]
            kern = [(n, v, s, o) for n, v, s, o in zip(names, vg, sp, occ) if "spatial_entry_fused_kernel" in n]
            assert len(kern) == 1, (defs, names)
            n, v, s, o = kern[0]
            assert v <= 256 and o >= 2 and s == 0, (n, v, s, o)
            text = open(asm).read()
            body = re.split(r"\n(?=_ZN\S*spatial_entry_fused_kernel\S*:)", text)[1].split("s_endpgm")[0]
            assert body.count("v_mfma") == 800            # 20 pairs x 40
            assert "scratch_" not in body


def test_spatial_entry_predicate_is_host_logic():
    from ctrlv_amd import _lib
    lib = _lib.load()

    def desc(n_img=50, S=9216, C=320, head_dim=64, **kw):
        d = _lib.SpatialEntryDesc()
        d.x, d.wf, d.h0, d.qkv = 0x1000, 0x2000, 0x3000, 0x4000       # (never dereferenced)
        d.ldx, d.ldh, d.ldq = C, C, 3 * C
        d.n_img, d.S, d.C, d.head_dim = n_img, S, C, head_dim
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    serves = lambda d: lib.ctrlv_spatial_entry_fused_serves(ctypes.byref(d))     # noqa: E731
    assert serves(desc()) == 1
    for n in (1, 2, 50, 100):                             # the batch does not decide (up to the 31-bit offsets)
        assert serves(desc(n_img=n)) == 1
    assert serves(desc(S=40)) == 0                        # a 32-row group would straddle images
    assert serves(desc(C=640)) == 0 and serves(desc(C=1280)) == 0
    assert serves(desc(head_dim=32)) == 0
    assert serves(desc(x_lo=0x5000)) == 0 and serves(desc(h0_lo=0x5000)) == 0
    assert serves(desc(ldq=3 * 320 + 4)) == 0 and serves(desc(ldx=312)) == 0
    assert serves(desc(n_img=3000)) == 0                  # q|k|v beyond 31-bit byte offsets
    assert lib.ctrlv_spatial_entry_fused_weight_bytes() == 40 * 20 * 1024
