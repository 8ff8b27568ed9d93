"""CPU checks of the LoRA adapters (ctrlv_amd/lora.py, csrc/lora.hip): `unet.add_adapter` names, shapes, freezing, init and
errors on the tiny configuration; the analytic work of `tools/train_unet_bench.py --mode lora`; the register budget of the
compiled kernels (hipcc cross-compiles gfx950)."""
import math
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctrlv_amd", "csrc")


def _unet(**over):
    import ctrlv_ref as R
    from ctrlv_amd.models import UNetSpatioTemporalConditionModel
    torch.manual_seed(0)
    return UNetSpatioTemporalConditionModel(**dict(R.TINY_CONFIG, **over))


def _cfg(**over):
    return dict(dict(r=4, lora_alpha=4, init_lora_weights="gaussian", lora_dropout=0.0,
                     target_modules=["to_k", "to_q", "to_v", "to_out.0"]), **over)


def _n_transformers(c):
    """transformers of the SVD layout, counted from the config: CrossAttn down blocks x layers, the mid block, CrossAttn up
    blocks x (layers + 1)"""
    n = len(c["down_block_types"])
    lpb = c["layers_per_block"] if isinstance(c["layers_per_block"], int) else c["layers_per_block"][0]
    down = sum(lpb for t in c["down_block_types"] if t.startswith("CrossAttn"))
    up = sum(lpb + 1 for t in c["up_block_types"] if t.startswith("CrossAttn"))
    assert n == 4
    return down + 1 + up


def test_add_adapter_names_shapes_and_freezing():
    import ctrlv_ref as R
    u = _unet()
    base_keys = set(u.state_dict())
    u.add_adapter(_cfg())
    sd = u.state_dict()
    lora_keys = {k for k in sd if ".lora_" in k}
    assert set(sd) - lora_keys == base_keys                        # base keys are the diffusers keys, unchanged
    # 2 attentions per block, 2 blocks (spatial, temporal) per transformer, 4 projections per attention, 2 factors each
    n_lin = _n_transformers(R.TINY_CONFIG) * 2 * 2 * 4
    assert n_lin == 256 and len(lora_keys) == 2 * n_lin
    for k in lora_keys:
        assert re.search(r"\.(to_q|to_k|to_v|to_out\.0)\.lora_[AB]\.default\.weight$", k), k
        base = sd[k.split(".lora_")[0] + ".weight"]
        if ".lora_A." in k:
            assert tuple(sd[k].shape) == (4, base.shape[1])
        else:
            assert tuple(sd[k].shape) == (base.shape[0], 4)
    trainable = {n for n, p in u.named_parameters() if p.requires_grad}
    assert trainable == lora_keys
    assert {id(p) for p in u.get_parameters_with_grad()} == {id(p) for n, p in u.named_parameters() if n in lora_keys}
    # a fresh model with the same adapter takes the state dict as is
    v = _unet()
    v.add_adapter(_cfg())
    missing, unexpected = v.load_state_dict(sd, strict=True)
    assert not missing and not unexpected


def test_init_statistics():
    torch.manual_seed(1)
    u = _unet()
    u.add_adapter(_cfg(r=16, lora_alpha=16))
    a = torch.cat([p.detach().reshape(-1) for n, p in u.named_parameters() if ".lora_A." in n])
    b = torch.cat([p.detach().reshape(-1) for n, p in u.named_parameters() if ".lora_B." in n])
    assert bool((b == 0).all())
    assert abs(float(a.std()) - 1.0 / 16) < 0.05 / 16 and abs(float(a.mean())) < 0.01 / 16        # gaussian: N(0, (1/r)^2)
    u = _unet()
    u.add_adapter(_cfg(init_lora_weights=True))
    for n, p in u.named_parameters():
        if ".lora_A." in n:                                        # kaiming_uniform(a=sqrt(5)): U(-1/sqrt(fan_in), ..)
            bound = 1.0 / math.sqrt(p.shape[1])
            assert 0.5 * bound < float(p.detach().abs().max()) <= bound, n
        elif ".lora_B." in n:
            assert float(p.abs().max()) == 0.0


def test_add_adapter_errors():
    u = _unet()
    with pytest.raises(ValueError, match="dropout"):
        u.add_adapter(_cfg(lora_dropout=0.1))
    with pytest.raises(ValueError, match="match no"):
        u.add_adapter(_cfg(target_modules=["to_q", "to_nothing"]))
    for bad in (["proj_in"], ["to_q", "proj_out"], ["linear_1"], ["2"], ["time_emb_proj"], ["proj"]):
        with pytest.raises(ValueError, match="attention"):           # layers the executors do not read merged
            u.add_adapter(_cfg(target_modules=bad))
        assert not any(p.requires_grad is False for p in u.parameters())   # (rejected before anything changed)
    u.add_adapter(_cfg(target_modules=["attn1.to_q", "to_out.0"]))
    assert {n.split(".lora_")[0].rsplit(".", 2)[-2:] == ["attn1", "to_q"] or n.split(".lora_")[0].endswith("to_out.0")
            for n, _ in u.named_parameters() if ".lora_" in n} == {True}
    with pytest.raises(ValueError, match="already"):
        u.add_adapter(_cfg(), adapter_name="second")

    class Obj:                                                     # duck-typed config object (a peft LoraConfig works so)
        r, lora_alpha, init_lora_weights, lora_dropout, target_modules = 8, 16, "gaussian", 0.0, ["to_out.0"]
    v = _unet()
    v.add_adapter(Obj())
    ks = [k for k in v.state_dict() if ".lora_A." in k]
    assert ks and all(".to_out.0." in k for k in ks)
    assert {m.lora_scaling for m in v.modules() if hasattr(m, "lora_scaling")} == {2.0}


def test_from_unet_refuses_an_adapted_unet():
    from ctrlv_amd.models import ControlNetModel
    u = _unet()
    u.add_adapter(_cfg())
    with pytest.raises(ValueError, match="fuse_lora"):
        ControlNetModel.from_unet(u)


def test_train_unet_bench_lora_work():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_unet_bench as tb
    f_tmp, b_tmp = tb.analytic_tflop(25, 72, 128, "temporal")
    f_l, b_l = tb.analytic_tflop(25, 72, 128, "lora")
    assert f_tmp < f_l < f_tmp * 1.01                              # the adapter branches add ~0.1 % to the forward
    assert f_l < f_l + b_l < f_tmp + b_tmp                         # dgrad everywhere + thin factor products, no base wgrad


def test_lora_kernels_register_budget():
    """Every kernel of csrc/lora.hip in both element types: <= 256 VGPRs (the header's budget), no spill, no scratch; the
    grad kernels run on the matrix pipe."""
    procs = []
    with tempfile.TemporaryDirectory() as td:
        for defs in ([], ["-DCTRLV_ELEM_F16=1"]):
            asm = os.path.join(td, "lora" + ("16" if defs else "") + ".s")
            cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                   "-Rpass-analysis=kernel-resource-usage", *defs, os.path.join(CSRC, "lora.hip"), "-o", asm]
            procs.append((defs, asm, subprocess.Popen(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True)))
        for defs, asm, p in procs:
            err = p.communicate()[1]
            assert p.returncode == 0, err[-2000:]
            names = re.findall(r"Function Name: (\S+)", err)
            vg = [int(x) for x in re.findall(r" VGPRs: (\d+)", err)]
            sp = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", err)]
            scr = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
            assert len(names) == 15 and len(vg) == len(sp) == len(scr) == 15, (defs, names)
            for n, v, s, c in zip(names, vg, sp, scr):
                assert v <= 256 and s == 0 and c == 0, (n, v, s, c)
            text = open(asm).read()
            mf = "v_mfma_f32_32x32x16_" + ("f16" if defs else "bf16")
            for kern in ("lora_hg_kernel", "lora_part_kernel"):
                bodies = [b.split("s_endpgm")[0] for b in re.split(r"\n(?=\S*" + kern + r"\S*:)", text)[1:]]
                assert len(bodies) == 6 and all(mf in b for b in bodies), kern      # one per padded rank 32 .. 192
