"""Build-level check of the upsampler weight-gradient kernel (csrc/wgrad_pp.hip, wgrad_pp_up_kernel: the LDS-DMA ring with
the nearest-x2 source-pixel walk) for both element types: the budget and loop shape of the other wgrad_pp instantiations --
at most 256 VGPRs, no spill, no scratch, two waves per SIMD, one chunk = 20 MFMAs with at most four transposed LDS reads
between two of them.  CPU only (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ctrlv_amd", "csrc")


def test_wgrad_pp_up_kernel_register_budget():
    procs = []
    with tempfile.TemporaryDirectory() as td:
        for defs in ([], ["-DCTRLV_ELEM_F16=1"]):
            asm = os.path.join(td, "wpu" + ("16" if defs else "") + ".s")
            cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                   "-Rpass-analysis=kernel-resource-usage", *defs, os.path.join(CSRC, "wgrad_pp.hip"), "-o", asm]
            procs.append((defs, asm, subprocess.Popen(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True)))
        for defs, asm, p in procs:
            err = p.communicate()[1]
            assert p.returncode == 0, err[-2000:]
            names = re.findall(r"Function Name: (\S+)", err)
            vg = [int(x) for x in re.findall(r" VGPRs: (\d+)", err)]
            sp = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", err)]
            scr = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
            occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", err)]
            kern = [(n, v, s, c, o) for n, v, s, c, o in zip(names, vg, sp, scr, occ) if "wgrad_pp_up_kernel" in n]
            assert len(kern) == 1, (defs, names)
            n, v, s, c, o = kern[0]
            assert v <= 256 and o >= 2 and s == 0 and c == 0, (n, v, s, c, o)
            text = open(asm).read()
            blocks = re.split(r"\n(?=\S*wgrad_pp_up_kernel\S*:)", text)[1:]
            assert len(blocks) == 1
            body = blocks[0].split("s_endpgm")[0]
            assert body.count("v_mfma") == 20                        # one chunk: two sets of 5 x 2
            run, worst, seen = 0, 0, False
            for ln in body.split("\n"):
                if "v_mfma" in ln:
                    seen, run = True, 0
                elif "ds_read_b64_tr_b16" in ln and seen:
                    run += 1
                    worst = max(worst, run)
                elif "s_barrier" in ln or "s_cbranch" in ln:
                    seen, run = False, 0
            assert 2 <= worst <= 4, worst
