"""Resource guard for the SSIM kernel (CPU only: hipcc cross-compiles gfx950), after tests/test_build_resources.py.

csrc/frame_quality.hip keeps a tile of both frames and the five row-filtered moment images in LDS and, per thread, the five
accumulators of four outputs and a run of 14 inputs in registers.  This test compiles the unit with
-Rpass-analysis=kernel-resource-usage and checks that no kernel of it touches scratch (a spilled accumulator would sit in the
tap loops) and that the SSIM kernel's LDS stays within the 64 KiB one workgroup may hold -- and is what the source says: the
tile, the moments and the four partial sums."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctrlv_amd", "csrc")
LDS_PER_WORKGROUP = 64 * 1024


def test_ssim_kernel_uses_no_scratch_and_fits_the_lds():
    import __graft_entry__ as g
    assert "frame_quality.hip" in g.HIP_SOURCES
    with tempfile.TemporaryDirectory() as td:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", *g.EXTRA_FLAGS.get("frame_quality.hip", []),
               os.path.join(CSRC, "frame_quality.hip"), "-o", os.path.join(td, "fq.s")]
        p = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True)
    err = p.stderr
    assert p.returncode == 0, err[-2000:]
    names = re.findall(r"Function Name: (\S+)", err)
    vg = [int(x) for x in re.findall(r" VGPRs: (\d+)", err)]
    sp = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", err)]
    scr = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", err)]
    assert len(names) == len(vg) == len(sp) == len(scr) == len(lds) == 5, names      # init, stats x 2, ssim, mean
    for n, s, c in zip(names, sp, scr):
        assert s == 0 and c == 0, (n, s, c)
    ssim = [(n, v, l) for n, v, l in zip(names, vg, lds) if "frame_ssim_kernel" in n]
    assert len(ssim) == 1, names
    _, v, l = ssim[0]
    assert v <= 128, v                                        # two workgroups of 256 threads per CU at the least
    assert l <= LDS_PER_WORKGROUP, l
    assert l == 4 * (2 * 26 * 76 + 5 * 26 * 64) + 8 * 4, l    # the tile and halo of both frames, five moments, four partial sums
