"""Host-side tests (no GPU) of the gather-GEMM's bottom / right padded stride-2 mode (`ctrlv_gemm_desc.pad_br`) and of
`ctrlv_vae_posterior`: the ABI table, and every argument error -- all of them are raised before anything is launched."""
import ctypes
import os
import re

import pytest
import torch

import __graft_entry__ as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000          # a non-null, 16-byte aligned address that is never dereferenced (validation fails first)


def _libs():
    g.build()
    from ctrlv_amd import _lib
    return _lib, (_lib.load(), _lib.load(torch.float16))


def _conv_desc(_lib, **kw):
    """The encoder down-sampler at 8 x 12 (3 images, 64 -> 96 channels), pad_br set."""
    d = _lib.GemmDesc()
    base = dict(A=P, W=P, out=P, bias=P, M=3 * 4 * 6, N=96, Cin=64, taps=9, lda=64, mode=1, H=8, Wd=12, Ho=4, Wo=6, stride=2,
                up=0, ldo=96, n_store=96, s_acc=1.0, pad_br=1)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_abi_and_the_new_symbol():
    _lib, libs = _libs()
    header = open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read()
    assert re.search(r"int32_t\s+pad_br\s*;", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    # the field fills what was alignment padding in front of raw_out: size and every other offset are those of ABI 22
    assert re.search(r"int32_t\s+ld_raw;\s*int32_t\s+pad_br;\s*void\*\s+raw_out;", code)
    D = _lib.GemmDesc
    assert ctypes.sizeof(D) == 264 and D.ld_raw.offset == 192 and D.pad_br.offset == 196 and D.raw_out.offset == 200
    assert D.out_lo.offset == 256
    declared = set(re.findall(r"\b(?:int|size_t)\s+(ctrlv_\w+)\s*\(", code))
    assert "ctrlv_vae_posterior" in declared and "ctrlv_vae_posterior" in _lib.SIGNATURES
    m = re.search(r"\bint\s+ctrlv_vae_posterior\s*\(([^)]*)\)", code)
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES["ctrlv_vae_posterior"][1])
    assert _lib.ABI_VERSION == 22
    for lib in libs:
        assert lib.ctrlv_abi_version() == 22
        assert lib.ctrlv_vae_posterior is not None
    # the ctypes stub of INTEGRATION 2b mirrors the struct
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stub = re.search(r"```python\n(import ctypes, torch.*?)```", doc, re.S).group(1)
    assert re.search(r'"ld_raw",\s*"pad_br"\)\]', stub)
    import ast
    ast.parse(stub)                       # the stub is code a reader pastes: it has to parse
    # ... and the header says what the placement costs: descriptors must be zero-initialised from now on
    assert "MUST" in header and "zero-initialised" in header


def test_pad_br_host_validation():
    _lib, libs = _libs()
    for lib in libs:
        bad = [
            (dict(H=7, M=3 * 3 * 6, Ho=3), -2, "even input"),                    # odd H
            (dict(Wd=11, Wo=5, M=3 * 4 * 5), -2, "even input"),                  # odd W
            (dict(Ho=5), -2, "M must be a multiple|half its size"),             # not half the input
            (dict(stride=1, Ho=8, Wo=12, M=3 * 96), -1, "pad_br=1 is the 3x3 conv of stride 2"),
            (dict(up=1, stride=1, Ho=16, Wo=24, M=3 * 384), -1, "pad_br=1 is the 3x3 conv of stride 2"),
            (dict(up=1), -1, "pad_br=1 is the 3x3 conv of stride 2"),
            (dict(mode=0, taps=1), -1, "pad_br=1 is the 3x3 conv of stride 2"),
            (dict(mode=2, taps=3, F=3, S=24), -1, "pad_br=1 is the 3x3 conv of stride 2"),
            (dict(pad_br=2), -1, "pad_br=2"),
        ]
        for kw, code, what in bad:
            d = _conv_desc(_lib, **kw)
            rc = lib.ctrlv_gemm(ctypes.byref(d), None)
            assert rc == code, (kw, rc, _lib.last_error(lib))
            assert re.search(what, _lib.last_error(lib)), (kw, _lib.last_error(lib))
        # a forced tile that cannot serve this launch answers as it does for the symmetric stride-2 conv: same code, same text
        for tile in (11, 99):
            texts = []
            for pad_br in (0, 1):
                d = _conv_desc(_lib, tile=tile, pad_br=pad_br)
                assert lib.ctrlv_gemm(ctypes.byref(d), None) == -1
                texts.append(_lib.last_error(lib))
            assert texts[0] == texts[1], texts
        # the two side channels are not offered, whatever else the descriptor says
        d = _conv_desc(_lib, N=640, ldo=640, n_store=640, Cin=640, lda=640, H=16, Wd=16, Ho=8, Wo=8, M=2 * 64)
        assert lib.ctrlv_gemm_gn_partials_serves(ctypes.byref(d)) == 0
        assert lib.ctrlv_gemm_splitk_ws_bytes(ctypes.byref(d)) == 0
        # inference only: the weight-gradient entry point refuses the field
        d = _conv_desc(_lib)
        rc = lib.ctrlv_gemm_wgrad(ctypes.byref(d), P, 96, P, None, 1.0, 0, None, 0, None)
        assert rc == -1 and "inference only" in _lib.last_error(lib)
    d = _conv_desc(_lib, out_lo=P)                # split trunk planes (fp16 library) are refused with pad_br
    assert libs[1].ctrlv_gemm(ctypes.byref(d), None) == -1
    assert "split planes do not combine with pad_br" in _lib.last_error(libs[1])


def test_ops_gemm_takes_pad_br():
    from ctrlv_amd import ops
    a = torch.zeros(8, 64, dtype=torch.bfloat16)
    assert ops._gemm_desc(a, a, a, N=64, cin=64).pad_br == 0
    assert ops._gemm_desc(a, a, a, N=64, cin=64, pad_br=True).pad_br == 1
    with pytest.raises(Exception, match="no CPU path"):
        ops.gemm(a, a, a, N=64, cin=64, taps=9, mode=1, conv=(2, 4, 1, 2, 2, 0), pad_br=True)
    # the training Functions have no such field: the mode cannot reach a backward
    from ctrlv_amd.autograd import GemmSpec
    assert "pad_br" not in GemmSpec._fields


def test_vae_posterior_host_validation():
    _lib, libs = _libs()
    for lib in libs:
        call = lambda **kw: lib.ctrlv_vae_posterior(*[dict(dict(rows=P, ld=8, n=2, L=4, HW=64, qw=P, qb=P, noise=None, scale=1.0,   # noqa: E731
                                                                  mom=P, lat=P, dt=2, stream=None), **kw)[k]
                                                      for k in ("rows", "ld", "n", "L", "HW", "qw", "qb", "noise", "scale", "mom",
                                                                "lat", "dt", "stream")])
        for kw, code, what in [
            (dict(mom=None, lat=None), -1, "both NULL"),
            (dict(L=9, ld=32), -2, "latent_channels=9"),
            (dict(L=0), -2, "latent_channels=0"),
            (dict(ld=4), -2, "ld=4"),
            (dict(rows=None), -1, "null"),
            (dict(qw=None), -1, "null"),
            (dict(dt=3), -1, "out_dtype=3"),
            (dict(n=0), -2, "bad shape"),
        ]:
            rc = call(**kw)
            assert rc == code and what in _lib.last_error(lib), (kw, rc, _lib.last_error(lib))
