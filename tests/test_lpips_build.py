"""Resource guard for csrc/lpips.hip (CPU only: hipcc cross-compiles gfx950), after tests/test_frame_quality_build.py.

The LPIPS kernels move bytes: a thread holds 8 values and three 16-byte units (im2col), nine units (pool) or two units of each
frame (distance).  This test compiles the unit for both element types with -Rpass-analysis=kernel-resource-usage and checks that
no kernel of it spills or touches scratch and that each stays small enough for at least four 256-thread workgroups per CU."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctrlv_amd", "csrc")


@pytest.mark.parametrize("defs", [[], ["-DCTRLV_ELEM_F16=1"]], ids=["bf16", "fp16"])
def test_lpips_kernels_use_no_scratch(defs):
    import __graft_entry__ as g
    assert "lpips.hip" in g.HIP_SOURCES
    with tempfile.TemporaryDirectory() as td:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", *g.EXTRA_FLAGS.get("lpips.hip", []), *defs,
               os.path.join(CSRC, "lpips.hip"), "-o", os.path.join(td, "lpips.s")]
        p = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True)
    err = p.stderr
    assert p.returncode == 0, err[-2000:]
    names = re.findall(r"Function Name: (\S+)", err)
    vg = [int(x) for x in re.findall(r" VGPRs: (\d+)", err)]
    sp = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", err)]
    scr = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
    # first-layer im2col x 2 sources, rows im2col, weight pack, pool, distance, finish
    assert len(names) == len(vg) == len(sp) == len(scr) == 7, names
    for n, v, s, c in zip(names, vg, sp, scr):
        assert s == 0 and c == 0, (n, s, c)
        assert v <= 128, (n, v)
    for want in ("im2col_first_kernel", "im2col_rows_kernel", "pack_split_weight_kernel", "relu_maxpool_kernel",
                 "layer_distance_kernel", "lpips_finish_kernel"):
        assert any(want in n for n in names), (want, names)
