"""fp64 reference of one training GEMM and of every gradient it hands back (ctrlv_amd/autograd.py: `Gemm`, `BlendGemm`).

    out = s_acc * (op(A, W) + bias) + s1 * R1 + s2 * R2 + V[idx(m)]

evaluated with ordinary torch ops on the CPU in float64 -- F.linear, F.conv2d(padding=1) (on the nearest-upsampled input for
`up`), F.conv3d(padding=(1, 0, 0)) -- on operands rounded exactly as the HIP side holds them (A, R1, R2, dY and W in bf16;
bias, V and the mix factor in fp32); gradients from torch.autograd.grad of (out * dY).sum().  Nothing here imports ctrlv_amd
or the oracle.  Also here: the rows <-> NCHW helpers, the table of op-level cases (tests/test_autograd_ops_gpu.py runs them
on the device, tests/test_autograd_ref_cpu.py checks this file and the comparison itself) and their seeded operands.
"""
import functools
import math

import torch
import torch.nn.functional as F

TAPS = {0: 1, 1: 9, 2: 3}


def bf(x):
    return x.to(torch.bfloat16)


def rows_from_nchw(x):
    """(n, C, H, W) -> channels-last rows [n*H*W, C]"""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c)


def nchw_from_rows(r, n, h, w):
    """channels-last rows [n*h*w, C] -> (n, C, h, w)"""
    return r.reshape(n, h, w, -1).permute(0, 3, 1, 2)


def vindex(M, vmode=1, vdiv=1, vmod=1 << 30, vS=1):
    """table row of every output row m (GemmSpec): vmode 1 (m // vdiv) % vmod, vmode 2 ((m // vdiv) * vS + m % vS) % vmod"""
    m = torch.arange(M)
    if vmode == 1:
        return (m // vdiv) % vmod
    if vmode == 2:
        return ((m // vdiv) * vS + m % vS) % vmod
    raise ValueError(f"vmode {vmode}")


def gather_gemm(A, W, mode=0, conv=None, temporal=None):
    """op(A, W) on rows, any float dtype: nn.Linear, 3x3 Conv2d (stride 2 / upsample-fused too), (3,1,1) Conv3d"""
    if mode == 0:
        return F.linear(A, W)
    if mode == 1:
        H, Wd, Ho, Wo, stride, up = conv
        n = A.shape[0] // (H * Wd)
        x = nchw_from_rows(A, n, H, Wd)
        if up:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        y = F.conv2d(x, W, None, stride=stride, padding=1)
        assert tuple(y.shape[2:]) == (Ho, Wo), (tuple(y.shape), conv)
        return rows_from_nchw(y)
    if mode == 2:
        Fr, S = temporal
        B = A.shape[0] // (Fr * S)
        x = A.reshape(B, Fr, S, 1, -1).permute(0, 4, 1, 2, 3)                 # (B, C, F, S, 1)
        y = F.conv3d(x, W, None, padding=(1, 0, 0))
        return y.permute(0, 2, 3, 4, 1).reshape(B * Fr * S, -1)
    raise ValueError(f"mode {mode}")


def forward64(A, W, bias=None, R1=None, R2=None, V=None, mix=None, *, mode=0, conv=None, temporal=None, s_acc=1.0, s1=1.0,
              s2=1.0, vmode=1, vdiv=1, vmod=1 << 30, vS=1, blend=None):
    """The epilogue formula on tensors of one dtype (differentiable in every tensor argument).  blend: None, or a = sigmoid(mix)
    sets the scalars -- "res": out = R1 + (1 - a) (op + bias); "tr": out = a R2 + (1 - a) (R1 + op + bias); "sw" (the switched
    res form): out = R1 + a (op + bias)."""
    if blend is not None:
        a = torch.sigmoid(mix).reshape(())
        s_acc, s1, s2 = {"res": (1 - a, 1.0, 1.0), "tr": (1 - a, 1 - a, a), "sw": (a, 1.0, 1.0)}[blend]
    lin = gather_gemm(A, W, mode, conv, temporal)
    if bias is not None:
        lin = lin + bias
    out = s_acc * lin
    if R1 is not None:
        out = out + s1 * R1
    if R2 is not None:
        out = out + s2 * R2
    if V is not None:
        out = out + V[vindex(out.shape[0], vmode, vdiv, vmod, vS)]
    return out


def reference(A, weight, bias=None, R1=None, R2=None, V=None, *, dY=None, noise=None, mix=None, blend=None, lora=None,
              factors=(), **spec):
    """Forward value and every gradient of one Gemm / BlendGemm call in float64.

    A, R1, R2: rows (rounded to bf16 here); weight: the parameter in its PyTorch layout (rounded to bf16 here, as the packed
    kernel layout holds it); bias, V, mix: fp32 values.  lora = (groups, s) with factors = (A_0, B_0, A_1, B_1, ...): the
    forward and dA use W' = bf16(fp32(W + s B_i A_i)); the factors (and the base) receive the gradient of the unrounded
    W + s B_i A_i.  dY: the upstream gradient (rounded to bf16), or None to take bf16(out + 0.5 * noise).
    Returns a dict: out, dY, dA, dW, db, dR1, dR2, dV, dmix, factors (a list), a (sigmoid(mix) as a float)."""
    def leaf(x, round16=True):
        if x is None:
            return None
        x = x.detach().cpu()
        return (bf(x) if round16 else x.float()).double().requires_grad_(True)

    A64, R164, R264 = leaf(A), leaf(R1), leaf(R2)
    b64, V64, m64 = leaf(bias, False), leaf(V, False), leaf(mix, False)
    f64 = [leaf(f, False) for f in factors]
    if lora is None:
        W64 = leaf(weight)
        Weff = W64
    else:
        groups, s = lora
        W64 = leaf(weight, False)
        w32 = weight.detach().cpu().float()
        n = w32.shape[0] // groups
        merged32 = torch.cat([w32[i * n:(i + 1) * n] + float(s) * (factors[2 * i + 1].detach().cpu().float()
                                                                 @ factors[2 * i].detach().cpu().float())
                              for i in range(groups)], 0)
        exact = W64 + s * torch.cat([f64[2 * i + 1] @ f64[2 * i] for i in range(groups)], 0)
        Weff = exact + (bf(merged32).double() - exact).detach()          # value: the rounded W'; gradient: straight through
    out = forward64(A64, Weff, b64, R164, R264, V64, m64, blend=blend, **spec)
    if dY is None:
        dY = out.detach() + 0.5 * noise.double()
    dY = bf(dY.detach().cpu()).double()
    wanted = {"dA": A64, "dW": W64, "db": b64, "dR1": R164, "dR2": R264, "dV": V64, "dmix": m64}
    keys = [k for k, v in wanted.items() if v is not None]
    grads = torch.autograd.grad((out * dY).sum(), [wanted[k] for k in keys] + f64)
    res = {k: None for k in wanted}
    res.update(zip(keys, grads[:len(keys)]))
    res.update(out=out.detach(), dY=dY, factors=list(grads[len(keys):]),
               a=None if mix is None else float(torch.sigmoid(m64.detach()).reshape(())))
    return res


def dmix_bound(ref, blend):
    """|dmix - ref| allowed: `out` is rounded once to bf16 (relative 2^-9) before dot_diff forms sum dY (out - xs); 2^-12 of
    headroom for the fp32 accumulation and the ordered fp32 sum.  Scale: a (res, transformer form), 1 - a (switched)."""
    a = ref["a"]
    return (1 - a if blend == "sw" else a) * (2.0 ** -9 + 2.0 ** -12) * float((ref["dY"] * ref["out"]).abs().sum())


def pooled_twice_rounded(ref, case):
    """C-up: what two roundings cost.  The exact dgrad on the upsampled grid (the gradient of the nearest-upsampled input),
    rounded to bf16, 2x2-summed in fp32 and rounded to bf16 again -- to be compared with the exact pooled gradient ref["dA"]."""
    H, Wd, Ho, Wo, stride, up = case["spec"]["conv"]
    assert up and stride == 1
    A, W = case["A"], case["weight"]
    n = A.shape[0] // (H * Wd)
    xu = F.interpolate(nchw_from_rows(bf(A).double(), n, H, Wd), scale_factor=2, mode="nearest").requires_grad_(True)
    y = rows_from_nchw(F.conv2d(xu, bf(W).double(), None, padding=1))
    (gu,) = torch.autograd.grad((y * ref["dY"] * case["spec"].get("s_acc", 1.0)).sum(), xu)
    gu = bf(rows_from_nchw(gu))                                                     # the GEMM's store
    return bf(gu.view(n, H, 2, Wd, 2, -1).float().sum((2, 4))).view(n * H * Wd, -1)  # the pooled sum's store


# ---------------------------------------------------------------------------------------------------------------- the cases
def _conv(n, H, W, cin, cout, stride=1, up=0, **kw):
    Ho, Wo = ((H << up) + 2 - 3) // stride + 1, ((W << up) + 2 - 3) // stride + 1
    return dict(mode=1, M=n * H * W, Mo=n * Ho * Wo, cin=cin, N=cout, spec=dict(mode=1, conv=(H, W, Ho, Wo, stride, up)), **kw)


def _temporal(B, Fr, S, C, **kw):
    return dict(mode=2, M=B * Fr * S, cin=C, N=C, spec=dict(mode=2, temporal=(Fr, S)), **kw)


def _with(case, **spec):
    case["spec"].update(spec)
    return case


# id -> geometry; "spec": GemmSpec fields; bias / R1 / R2: operands present; V: table rows; the smallest shapes that reach each
# path of gemm_grads / _epilogue_grads (ragged rows, N % 64 != 0, N = 4, odd images, the split-contraction plan, wrapping and
# strided row-vector index maps, every BlendGemm form at two mix factors, LoRA with one and three groups)
CASES = {
    "L-all": dict(mode=0, M=777, cin=64, N=96, bias=True, R1=True, R2=True, V=7,
                  spec=dict(s_acc=0.7, s1=0.5, s2=-0.25, vmode=1, vdiv=111, vmod=7)),
    "L-wrap": dict(mode=0, M=370, cin=128, N=64, bias=True, R1=True, V=5, spec=dict(vmode=1, vdiv=37, vmod=5)),
    "L-quirk": dict(mode=0, M=60, cin=64, N=64, bias=True, R1=True, V=2, spec=dict(vmode=2, vdiv=30, vS=10, vmod=2)),
    "L-quirk3": dict(mode=0, M=90, cin=64, N=64, bias=True, R1=True, V=3, spec=dict(vmode=2, vdiv=30, vS=10, vmod=3)),
    "L-zero": dict(mode=0, M=384, cin=64, N=64, bias=True, spec=dict(s_acc=0.8)),
    "C-s1": _with(_conv(3, 8, 12, 64, 96, bias=True, V=3), vmode=1, vdiv=96),
    "C-s2": _conv(3, 8, 12, 64, 128, stride=2, bias=True),
    "C-s2-odd": _conv(2, 9, 7, 64, 64, stride=2, bias=True),
    "C-up": _conv(2, 5, 6, 64, 64, up=1, bias=True, R1=True),
    "C-out4": _conv(2, 8, 8, 64, 4, bias=True),
    "C-long": _with(_conv(2, 5, 8, 1280, 1280, bias=True, R1=True), s1=0.5, s_acc=0.75),
    "C-long-s2": _conv(2, 10, 16, 1280, 1280, stride=2, bias=True),
    "T": _with(_temporal(2, 5, 24, 64, bias=True, V=2), vmode=1, vdiv=120),
    "T-1f": _temporal(3, 1, 24, 64, bias=True),
    "B-res-lo": _temporal(2, 3, 24, 64, bias=True, R1=True, blend="res", mix=-1.1),
    "B-res-hi": _temporal(2, 3, 24, 64, bias=True, R1=True, blend="res", mix=0.7),
    "B-tr-lo": dict(mode=0, M=333, cin=256, N=64, bias=True, R1=True, R2=True, blend="tr", mix=-1.1, spec=dict()),
    "B-tr-hi": dict(mode=0, M=333, cin=256, N=64, bias=True, R1=True, R2=True, blend="tr", mix=0.7, spec=dict()),
    "B-sw-lo": _temporal(2, 3, 24, 64, bias=True, R1=True, blend="sw", mix=-1.1),
    "B-sw-hi": _temporal(2, 3, 24, 64, bias=True, R1=True, blend="sw", mix=0.7),
    "G3": dict(mode=0, M=515, cin=320, N=960, lora=(3, 2.0), rank=4, base_frozen=True, spec=dict()),
    "G1": dict(mode=0, M=300, cin=320, N=320, bias=True, R1=True, lora=(1, 0.5), rank=16, spec=dict(s_acc=0.5)),
}
BLEND_CASES = [k for k, c in CASES.items() if c.get("blend")]


def build_case(cid):
    """Seeded CPU operands of a case: A, R1, R2 as bf16 rows, the parameters / V / mix as fp32 values, `noise` for dY."""
    c = dict(CASES[cid])
    c["id"] = cid
    gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(cid))
    rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    M, Mo, cin, N, mode = c["M"], c.get("Mo", c["M"]), c["cin"], c["N"], c["mode"]
    wshape = {0: (N, cin), 1: (N, cin, 3, 3), 2: (N, cin, 3, 1, 1)}[mode]
    c["A"] = bf(rn(M, cin))
    c["weight"] = rn(*wshape) / math.sqrt(TAPS[mode] * cin)
    c["bias"] = rn(N) if c.get("bias") else None
    blend = c.get("blend")
    # (dmix signal condition, tests/test_autograd_ref_cpu.py: xs at half the branch's scale, h2 at twice g1's)
    r1_scale = 0.5 if blend in ("res", "sw") else 1.0
    c["R1"] = bf(r1_scale * rn(Mo, N)) if c.get("R1") else None
    c["R2"] = bf((2.0 if blend == "tr" else 1.0) * rn(Mo, N)) if c.get("R2") else None
    c["V"] = rn(c["V"], N) if c.get("V") else None
    c["mix"] = torch.tensor([c["mix"]], dtype=torch.float32) if blend else None
    c["factors"] = []
    if c.get("lora"):
        g, r = c["lora"][0], c["rank"]
        for _ in range(g):
            c["factors"] += [0.3 * rn(r, cin), 0.05 * rn(N // g, r)]
    c["noise"] = rn(Mo, N)
    return c


@functools.lru_cache(maxsize=None)
def case_reference(cid):
    """(case operands, reference dict) of a case: computed once per process, shared by every test, never written to."""
    c = build_case(cid)
    ref = reference(c["A"], c["weight"], c["bias"], c["R1"], c["R2"], c["V"], noise=c["noise"], mix=c["mix"],
                    blend=c.get("blend"), lora=c.get("lora"), factors=c["factors"], **c["spec"])
    return c, ref
