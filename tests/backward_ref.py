"""fp64 references of the backward kernels that are not GEMMs (csrc/backward.hip, csrc/attention_bwd.hip): GroupNorm(+SiLU),
LayerNorm, GEGLU, the spatial and the temporal attention core -- and of the forward GELU table (csrc/common.h gelu_phi_tab).

Everything here is ordinary torch on the CPU in float64, on operands rounded exactly as the HIP side holds them (rows, upstream
gradients and skip gradients in bf16; gamma, beta, the row-vector table in fp32).  The norms and the attention cores take their
gradients from torch.autograd (F.group_norm, F.layer_norm, F.scaled_dot_product_attention); GEGLU is the closed form with erf.
The norm formulas are also written out (`gn_closed_form`, `ln_closed_form`): tests/test_backward_ref_cpu.py checks them against
autograd and plants its defects in them.  Nothing here imports ctrlv_amd or the oracle.

The seeded cases (tests/test_backward_ops_gpu.py runs them on the device) are the smallest shapes that reach each branch of the
launchers; what every case exists for is stated beside it.  A reference is computed once per process and never written to.
Upstream gradients of the norms are dy = bf16(y + 0.5 noise) with y the norm's own output: with a pure-noise dy the two group
means of the backward (mean dz gamma, mean dz gamma xhat) are ~1/sqrt(count) and a defect in them would hide in the bound.
"""
import functools
import math

import torch
import torch.nn.functional as F

TOL_DX, TOL_PARAM, TOL_ATTN = 4e-3, 2e-3, 1e-2        # the bounds of tests/test_backward_gpu.py (bf16 dx; fp32 sums; attention)


def bf(x):
    return x.to(torch.bfloat16)


def _gen(kind, cid, table):
    return torch.Generator().manual_seed(7000 + 100 * kind + sorted(table).index(cid))


# ------------------------------------------------------------------------------------------------------------ GroupNorm
# launch geometry of ctrlv_groupnorm_bwd: CV = C/8 column vectors, RPP = CV >= 256 ? 1 : 256 / CV rows per pass, CV * RPP threads;
# forward chunks of 32 / 64 / 256 rows (S < 1024 / < 4096 / above), re-chunked evenly by the backward; 16 ordered fold groups of
# the parameter gradients once n * n_chunks >= 64, one below
GN_CASES = {
    # widths: CV = 32 (RPP 8), 64 (4), 80 (3, 240 threads), 120 (2), 160 (1), 240 (1) and 320 (the CV >= 256 branch)
    "w256-ips3": dict(C=256, n=3, S=24, ips=3),
    "w512-ips3": dict(C=512, n=3, S=16, ips=3),
    "w640-add": dict(C=640, n=2, S=48, add=True),               # two chunks of 24 rows, RPP = 3
    "w960": dict(C=960, n=2, S=17),
    "w1280-add": dict(C=1280, n=3, S=16, add=True),
    "w1920": dict(C=1920, n=2, S=20),
    "w2560": dict(C=2560, n=2, S=16),
    "rows<RPP": dict(C=64, n=2, S=4),                           # RPP = 32 row lanes, 4 rows
    "last1": dict(C=320, n=2, S=33),                            # forward chunks 32 + 1 rows; the backward's own are 17 + 16
    "rechunk": dict(C=64, n=1, S=1100),                         # 18 chunks: 64 rows forward, 62 (last 46) backward
    "chunk256": dict(C=32, n=2, S=4100),                        # 17 chunks of 256 forward, 242 backward; one channel per group
    "fold16": dict(C=320, n=16, S=160, init=True),              # 80 (image, chunk) partials: the 16-group fold; += into non-zero
    "mean30": dict(C=320, n=3, S=96, mean=30.0, std=0.25),
    "mean1000-ips3": dict(C=320, n=3, S=96, ips=3, mean=1000.0, std=4.0, add=True),
}


def gn_chunks(S):
    """(n_chunks, rows per chunk of the backward) for an image of S rows (norm.hip gn_shape, ctrlv_groupnorm_bwd_add)."""
    rpc = min(S, 256 if S >= 4096 else (64 if S >= 1024 else 32))
    chunks = (S + rpc - 1) // rpc
    return chunks, (S + chunks - 1) // chunks


def gn_fold_groups(n, S):
    return 16 if n * gn_chunks(S)[0] >= 64 else 1


def _gn_5d(rows, n, S, C, ips):
    """rows [n*S, C] -> (n/ips, C, ips, S, 1): one statistics row per leading index"""
    return rows.reshape(n // ips, ips, S, C).permute(0, 3, 1, 2).unsqueeze(-1)


def _gn_rows(t5, n, S, C):
    return t5.squeeze(-1).permute(0, 2, 3, 1).reshape(n * S, C).contiguous()


@functools.lru_cache(maxsize=None)
def gn_case(cid):
    """Seeded operands of a GroupNorm case: x, dy (, add) as bf16 rows [n*S, C]; gamma, beta, and the values dgamma / dbeta start
    from (g0, b0: zeros unless `init`) in fp32."""
    c = dict(GN_CASES[cid])
    c.setdefault("ips", 1)
    gen = _gen(0, cid, GN_CASES)
    C, n, S, ips = c["C"], c["n"], c["S"], c["ips"]
    if "mean" in c:       # |mean| >> std with per-channel offsets (test_ops_gpu.py::test_groupnorm_large_mean_small_variance)
        x = torch.randn(n * S, C, generator=gen) * c["std"] + c["mean"] + torch.randn(1, C, generator=gen) * c["std"]
    else:
        x = torch.randn(n * S, C, generator=gen) * 1.5 + 0.3
    c["x"] = bf(x)
    c["gamma"], c["beta"] = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    y = _gn_rows(F.group_norm(_gn_5d(c["x"].double(), n, S, C, ips), 32, c["gamma"].double(), c["beta"].double(), 1e-5), n, S, C)
    c["dy"] = bf(y + 0.5 * torch.randn(n * S, C, generator=gen).double())
    c["add"] = bf(torch.randn(n * S, C, generator=gen)) if c.get("add") else None
    c["noise0"] = torch.randn(2, C, generator=gen)
    return c


@functools.lru_cache(maxsize=None)
def gn_reference(cid, silu):
    """fp64 autograd of F.group_norm(+SiLU) (5-D form: `ips` images share a statistics row): dx (+ add), and dgamma / dbeta as
    the buffers must read afterwards (g0 + gradient, b0 + gradient; g0 = b0 = 0 unless the case starts them non-zero, then at
    the gradient's own scale)."""
    c = gn_case(cid)
    C, n, S, ips = c["C"], c["n"], c["S"], c["ips"]
    x = c["x"].double().requires_grad_(True)
    g, b = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    y = _gn_rows(F.group_norm(_gn_5d(x, n, S, C, ips), 32, g, b, 1e-5), n, S, C)
    if silu:
        y = F.silu(y)
    dx, dg, db = torch.autograd.grad((y * c["dy"].double()).sum(), [x, g, b])
    if c["add"] is not None:
        dx = dx + c["add"].double()
    g0 = b0 = torch.zeros(C)
    if c.get("init"):
        g0 = (c["noise0"][0].double() * dg.pow(2).mean().sqrt()).float()
        b0 = (c["noise0"][1].double() * db.pow(2).mean().sqrt()).float()
    return dict(dx=dx, dgamma=g0.double() + dg, dbeta=b0.double() + db, g0=g0, b0=b0)


def _dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def gn_closed_form(cid, silu, skip_mean_rows=None, skip_param_rows=None, no_add_rows=None):
    """The backward written out as the kernels compute it (fp64): xhat, dz = dy (* silu'), dgamma = sum dz xhat, dbeta = sum dz,
    per (statistics row, group) m1 = mean dz gamma and m2 = mean dz gamma xhat, dx = rstd (dz gamma - m1 - xhat m2) (+ add).
    The three masks ([n*S] bool) plant defects: rows left out of the group means (the divisor stays), rows left out of the
    parameter sums, rows whose skip gradient is not added."""
    c = gn_case(cid)
    C, n, S, ips = c["C"], c["n"], c["S"], c["ips"]
    ns, cpg = n // ips, C // 32
    sh = (ns, ips * S, 32, cpg)
    x, dy = c["x"].double().reshape(sh), c["dy"].double().reshape(sh)
    g, b = c["gamma"].double().reshape(1, 1, 32, cpg), c["beta"].double().reshape(1, 1, 32, cpg)
    mean = x.mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(x.var((1, 3), unbiased=False, keepdim=True) + 1e-5)
    xh = (x - mean) * rstd
    dz = dy * _dsilu(xh * g + b) if silu else dy
    keep = lambda m: 1.0 if m is None else (~m).double().reshape(ns, ips * S, 1, 1)       # noqa: E731
    kp = keep(skip_param_rows)
    dg, db = (dz * xh * kp).sum((0, 1)).reshape(C), (dz * kp * torch.ones_like(xh)).sum((0, 1)).reshape(C)
    km = keep(skip_mean_rows)
    cnt = cpg * S * ips
    m1 = (dz * g * km).sum((1, 3), keepdim=True) / cnt
    m2 = (dz * g * xh * km).sum((1, 3), keepdim=True) / cnt
    dx = (rstd * (dz * g - m1 - xh * m2)).reshape(n * S, C)
    if c["add"] is not None:
        ka = 1.0 if no_add_rows is None else (~no_add_rows).double().reshape(n * S, 1)
        dx = dx + c["add"].double() * ka
    ref = gn_reference(cid, silu)
    return dict(dx=dx, dgamma=ref["g0"].double() + dg, dbeta=ref["b0"].double() + db)


def gn_chunk_rows(cid, img, chunk):
    """[n*S] bool: the rows of the backward's chunk `chunk` of image `img`"""
    c = gn_case(cid)
    _, rpc = gn_chunks(c["S"])
    m = torch.zeros(c["n"] * c["S"], dtype=torch.bool)
    m[img * c["S"] + chunk * rpc:img * c["S"] + min(c["S"], (chunk + 1) * rpc)] = True
    return m


def gn_fold_group_rows(cid, group):
    """[n*S] bool: the rows whose (image, chunk) partial k = img * n_chunks + chunk belongs to fold group `group` of
    gn_bwd_affine_kernel: (k // 4) % groups == group"""
    c = gn_case(cid)
    chunks, _ = gn_chunks(c["S"])
    groups = gn_fold_groups(c["n"], c["S"])
    m = torch.zeros(c["n"] * c["S"], dtype=torch.bool)
    for k in range(c["n"] * chunks):
        if (k // 4) % groups == group:
            m |= gn_chunk_rows(cid, k // chunks, k % chunks)
    return m


# ------------------------------------------------------------------------------------------------------------ LayerNorm
# ctrlv_layernorm_bwd: one wave per row, NV = ceil(C / 512) 8-column vectors per lane, min(ceil(M / 4), 1024) workgroups of four
# waves (grid-stride above M = 4096), per-wave partial rows folded in 16 ordered groups once there are 64 of them, in one below
LN_CASES = {
    "1x8": dict(M=1, C=8),                                       # one lane of one wave; three waves without a row
    "3x64": dict(M=3, C=64, add=True),
    "60x320": dict(M=60, C=320, V=(10, 3)),                      # 60 partial rows: the single-group fold
    "64x640": dict(M=64, C=640, add=True),                       # 64 partial rows: 16 groups; NV = 2, lanes 16..63 past C
    "333x1024": dict(M=333, C=1024, V=(37, 4)),                  # NV = 2 full; the table index wraps (rows 148.. reuse row 0..)
    "50x2048": dict(M=50, C=2048, add=True),                     # NV = 4, the limit
    "4099x64": dict(M=4099, C=64, add=True),                     # grid-stride: waves 0..2 of workgroup 0 take two rows
    "4500x640": dict(M=4500, C=640, V=(500, 5), add=True),       # grid-stride, 404 waves with two rows, ragged NV = 2
    "mean30": dict(M=37, C=320, mean=30.0, std=0.25),
}


def ln_vindex(M, V):
    vdiv, vmod = V
    return (torch.arange(M) // vdiv) % vmod


@functools.lru_cache(maxsize=None)
def ln_case(cid):
    """Seeded operands: x, dy (, add) bf16 [M, C]; gamma, beta fp32; V fp32 [vmod, C] with (vdiv, vmod) in `vmap`."""
    c = dict(LN_CASES[cid])
    gen = _gen(1, cid, LN_CASES)
    M, C = c["M"], c["C"]
    if "mean" in c:
        x = torch.randn(M, C, generator=gen) * c["std"] + c["mean"] + torch.randn(1, C, generator=gen) * c["std"]
    else:
        x = torch.randn(M, C, generator=gen) * 1.3 + 0.5
    c["x"] = bf(x)
    c["gamma"], c["beta"] = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    c["vmap"] = c.pop("V", None)
    c["V"] = torch.randn(c["vmap"][1], C, generator=gen) if c["vmap"] else None
    xin = c["x"].double() + (c["V"].double()[ln_vindex(M, c["vmap"])] if c["vmap"] else 0.0)
    y = F.layer_norm(xin, (C,), c["gamma"].double(), c["beta"].double(), 1e-5)
    c["dy"] = bf(y + 0.5 * torch.randn(M, C, generator=gen).double())
    c["add"] = bf(torch.randn(M, C, generator=gen)) if c.get("add") else None
    return c


@functools.lru_cache(maxsize=None)
def ln_reference(cid):
    """fp64 autograd of F.layer_norm(x + V[idx]): dx (+ add), dgamma, dbeta, dV (the table's gradient: without add), and
    dx_norm = dx without add (what LayerNormFn column-sums into dV)."""
    c = ln_case(cid)
    M, C = c["M"], c["C"]
    x = c["x"].double().requires_grad_(True)
    g, b = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    leaves = [x, g, b]
    xin = x
    if c["vmap"]:
        V = c["V"].double().requires_grad_(True)
        leaves.append(V)
        xin = x + V[ln_vindex(M, c["vmap"])]
    y = F.layer_norm(xin, (C,), g, b, 1e-5)
    grads = torch.autograd.grad((y * c["dy"].double()).sum(), leaves)
    dx = grads[0] + (c["add"].double() if c["add"] is not None else 0.0)
    return dict(dx=dx, dx_norm=grads[0], dgamma=grads[1], dbeta=grads[2], dV=grads[3] if c["vmap"] else None)


def ln_closed_form(cid, lanes=None):
    """The backward written out (fp64).  lanes: a defect -- the variance sum runs over `lanes` columns per row, those past C
    holding zeros (each adds mean^2), while the divisor stays C."""
    c = ln_case(cid)
    M, C = c["M"], c["C"]
    x = c["x"].double() + (c["V"].double()[ln_vindex(M, c["vmap"])] if c["vmap"] else 0.0)
    dy, g = c["dy"].double(), c["gamma"].double()
    mean = x.mean(1, keepdim=True)
    q = (x - mean).pow(2).sum(1, keepdim=True)
    if lanes is not None:
        q = q + (lanes - C) * mean.pow(2)
    rstd = 1.0 / torch.sqrt(q / C + 1e-5)
    xh = (x - mean) * rstd
    dz = dy * g
    dxn = rstd * (dz - dz.mean(1, keepdim=True) - xh * (dz * xh).mean(1, keepdim=True))
    dx = dxn + (c["add"].double() if c["add"] is not None else 0.0)
    dV = None
    if c["vmap"]:
        idx = ln_vindex(M, c["vmap"])
        dV = torch.stack([dxn[idx == j].sum(0) for j in range(c["vmap"][1])])
    return dict(dx=dx, dx_norm=dxn, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0), dV=dV)


# ------------------------------------------------------------------------------------------------------------ GEGLU
def gate_grid():
    """bf16-exact gates over [-12, 12]: every multiple of 1/16 (8 significant bits at most), and around the clamp of gelu_phi4
    (+-5) and both ends of the forward table (+-5.12 -> bf16 5.125) the value itself and its bf16 neighbours (spacing 2^-5)."""
    grid = [i / 16.0 for i in range(-192, 193)]
    for v in (5.0, 5.125):
        for d in (-1, 0, 1):
            grid += [v + d / 32.0, -(v + d / 32.0)]
    t = torch.tensor(sorted(set(grid)))
    assert torch.equal(bf(t).float(), t) and 0.0 in grid
    return t


def _grid_mixed(n, gen):
    """n gates: the grid (repeated as often as fits into three quarters) and N(0, 2) values, shuffled; bf16-exact"""
    grid = gate_grid()
    reps = max(1, (3 * n // 4) // grid.numel())
    vals = torch.cat([grid.repeat(reps), bf(2.0 * torch.randn(n - reps * grid.numel(), generator=gen)).float()])
    return vals[torch.randperm(n, generator=gen)]


# ctrlv_geglu_bwd: one thread per 8 value columns, at most 4096 workgroups of 256: the grid-stride loop needs M * I / 8 > 2^20
GEGLU_CASES = {
    "I16": dict(M=37, I=16),                    # one 32-column block per row, odd row count
    "I256": dict(M=50, I=256),
    "I1280": dict(M=9, I=1280),
    "stride": dict(M=6600, I=1280),             # 1 056 000 vectors: 7 424 threads take a second one
    "grid": dict(M=64, I=64, grid=True),        # gates on / past the clamp and the table ends
}


@functools.lru_cache(maxsize=None)
def geglu_case(cid):
    """raw [M, 2I] bf16 in the packed order (per 32 columns: 16 values | their 16 gates), du [M, I] bf16"""
    c = dict(GEGLU_CASES[cid])
    gen = _gen(2, cid, GEGLU_CASES)
    M, I = c["M"], c["I"]
    a = torch.randn(M, I, generator=gen)
    g = _grid_mixed(M * I, gen).reshape(M, I) if c.get("grid") else torch.randn(M, I, generator=gen) * 1.5
    c["raw"] = bf(geglu_pack(a, g))
    c["du"] = bf(torch.randn(M, I, generator=gen))
    return c


def geglu_pack(a, g):
    M, I = a.shape
    return torch.stack([a.reshape(M, I // 16, 16), g.reshape(M, I // 16, 16)], 2).reshape(M, 2 * I)


def geglu_unpack(raw):
    M, I = raw.shape[0], raw.shape[1] // 2
    r = raw.reshape(M, I // 16, 2, 16)
    return r[:, :, 0].reshape(M, I), r[:, :, 1].reshape(M, I)


def Phi(g):
    return 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0)))


def phi(g):
    return torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def geglu_closed_form(raw, du, g_phi_term=True):
    """draw in raw's order, fp64: da = du g Phi(g), dg = du a (Phi(g) + g phi(g))  (g_phi_term=False: a planted defect)"""
    a, g = geglu_unpack(raw.double())
    du = du.double()
    dg = du * a * (Phi(g) + (g * phi(g) if g_phi_term else 0.0))
    return geglu_pack(du * g * Phi(g), dg)


@functools.lru_cache(maxsize=None)
def geglu_reference(cid):
    c = geglu_case(cid)
    return geglu_closed_form(c["raw"], c["du"])


@functools.lru_cache(maxsize=None)
def gelu_table_case():
    """Forward GEGLU GEMM whose gates are exact: A [512, 128] carries mixed grid gates in its first 8 columns, gate row j of the
    weight [2 * 128, 128] is the unit vector of column j % 8 (so gate (m, j) = A[m, j % 8], exact in any accumulation order),
    the value rows and their bias are random, the gates have none.  Returns A (bf16), the weight (bf16-exact fp32) and the bias in
    nn.Linear order [values | gates], and the fp64 reference a * g * Phi(g) [512, 128]."""
    gen = torch.Generator().manual_seed(7999)
    M, K, I = 512, 128, 128
    A = torch.randn(M, K, generator=gen)
    A[:, :8] = _grid_mixed(M * 8, gen).reshape(M, 8)
    A = bf(A)
    W = torch.zeros(2 * I, K)
    W[:I] = bf(torch.randn(I, K, generator=gen) / math.sqrt(K)).float()
    W[I + torch.arange(I), torch.arange(I) % 8] = 1.0
    bias = torch.cat([torch.randn(I, generator=gen), torch.zeros(I)])
    a = A.double() @ W[:I].double().T + bias[:I].double()
    g = A.double()[:, torch.arange(I) % 8]
    return dict(A=A, W=W, bias=bias, ref=a * g * Phi(g), M=M, K=K, I=I)


# ------------------------------------------------------------------------------------------------------------ attention
def attn_reference(qkv, dout, n_seq, L, C):
    """fp64 autograd of F.scaled_dot_product_attention over n_seq sequences of L rows [n_seq * L, 3C] (head_dim 64):
    (out, dqkv, lse in the log2 domain [n_seq, heads, L])."""
    heads = C // 64
    x = qkv.double().clone().requires_grad_(True)
    f = x.reshape(n_seq, L, 3, heads, 64)
    q, k, v = (f[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    out = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(n_seq * L, C)
    (grad,) = torch.autograd.grad((out * dout.double()).sum(), x)
    lse = torch.logsumexp((q @ k.transpose(-1, -2)).detach() * 0.125, dim=-1) * math.log2(math.e)
    return out.detach(), grad, lse


def attn_rounding_point_reference(qkv, dout, n_seq, L, C):
    """The same formulas in fp64 with the kernels' own rounding points: the saved `out` in bf16 (D = dO . out), P and dS rounded
    to bf16 before their products (dV = P^T dO, dQ = dS K, dK = dS^T Q), every output rounded once.  Returns dqkv (fp64 values
    of bf16 numbers)."""
    heads = C // 64
    r = lambda t: bf(t).double()                                               # noqa: E731
    f = qkv.double().reshape(n_seq, L, 3, heads, 64)
    q, k, v = (f[:, :, i].permute(0, 2, 1, 3) for i in range(3))               # [n, h, L, 64]
    do = dout.double().reshape(n_seq, L, heads, 64).permute(0, 2, 1, 3)
    P = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
    out = r(P @ v)
    D = (do * out).sum(-1, keepdim=True)
    dS = r(P * (do @ v.transpose(-1, -2) - D))
    Pb = r(P)
    dq, dk, dv = r(dS @ k * 0.125), r(dS.transpose(-1, -2) @ q * 0.125), r(Pb.transpose(-1, -2) @ do)
    g = torch.stack([dq, dk, dv], 2)                                           # [n, h, 3, L, 64]
    return g.permute(0, 3, 2, 1, 4).reshape(n_seq * L, 3 * C)


def attn_with_extra_key(qkv, dout, n_seq, L, C, extra):
    """A planted defect: one more key / value row (`extra` [3C], its k and v blocks) takes part in every sequence -- the row
    just past a ragged tile left unmasked.  dqkv of the L real rows."""
    x = torch.cat([qkv.double().reshape(n_seq, L, 3 * C), extra.double().expand(n_seq, 1, 3 * C)], 1).reshape(-1, 3 * C)
    heads = C // 64
    x.requires_grad_(True)
    f = x.reshape(n_seq, L + 1, 3, heads, 64)
    q, k, v = (f[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    out = F.scaled_dot_product_attention(q[:, :, :L], k, v).permute(0, 2, 1, 3).reshape(n_seq * L, C)
    (grad,) = torch.autograd.grad((out * dout.double()).sum(), x)
    return grad.reshape(n_seq, L + 1, 3 * C)[:, :L].reshape(n_seq * L, 3 * C)


# spatial: both kernels run 128-row workgroups of four 32-row waves over 64-row tiles; a ragged last tile reads zeros past the
# image through the buffer range check.  n_img = 2 everywhere but in the large-logit case: image 1 lies behind image 0's tile.
SPATIAL_CASES = {f"S{S}": dict(S=S, C=64, n_img=2) for S in (1, 5, 31, 32, 33, 64, 65, 127, 128, 129, 191)}
# S 1, 5, 31: less than one wave; 32 / 33: one wave full / one row in the second; 64, 128: full tiles and the next image right
# behind; 65: one valid key in the masked tile; 127: one row short; 129: one valid row in the second workgroup; 191: three tiles
SPATIAL_CASES["S65-C128"] = dict(S=65, C=128, n_img=2)                    # two heads: the head stride of L, D and the columns
SPATIAL_CASES["large"] = dict(S=192, C=64, n_img=1, large=6.0)            # test_ops_gpu.py::test_attention_spatial_large_scores
SPATIAL_LEAK_CASE = "S65"                                                 # (image 1 at 1e4 in the device test)


@functools.lru_cache(maxsize=None)
def spatial_case(cid):
    c = dict(SPATIAL_CASES[cid])
    gen = _gen(3, cid, SPATIAL_CASES)
    S, C, n = c["S"], c["C"], c["n_img"]
    qkv = torch.randn(n * S, 3 * C, generator=gen)
    if c.get("large"):      # logits of several hundred, keys growing along the sequence, a run of identical keys
        ramp = torch.linspace(0.2, 1.0, S)[:, None]
        qkv[:, :64] *= c["large"]
        qkv[:, 64:128] = (qkv[:, 64:128] * ramp + 0.5 * ramp) * c["large"]
        qkv[S // 2:S // 2 + 40, 64:128] = qkv[S // 2, 64:128]
    c["qkv"], c["dout"] = bf(qkv), bf(torch.randn(n * S, C, generator=gen))
    c["extra"] = bf(torch.randn(3 * C, generator=gen))
    c["peaked"] = bool(c.get("large"))
    c["ragged"] = S % 64 != 0
    return c


@functools.lru_cache(maxsize=None)
def spatial_reference(cid):
    """(out, dqkv, lse) in fp64, rows [n_img * S, .]"""
    c = spatial_case(cid)
    return attn_reference(c["qkv"], c["dout"], c["n_img"], c["S"], c["C"])


# temporal: one wave per (clip, pixel, head), four per workgroup; frames arrive in four DMA pieces of 8 (F = 8 | 9, 16 | 17 are
# the piece boundaries); rows ordered (b, f, s)
TEMPORAL_CASES = {
    "F1": dict(B=1, F=1, S=7, C=128),           # 14 problems: the last workgroup has two idle waves; dq = dk = 0, dv = dout
    "F2": dict(B=2, F=2, S=5, C=64),            # 10 problems
    "F8": dict(B=1, F=8, S=4, C=128),
    "F9": dict(B=1, F=9, S=7, C=64),            # 7 problems
    "F16": dict(B=2, F=16, S=3, C=64),
    "F17": dict(B=1, F=17, S=5, C=128),
    "F31": dict(B=1, F=31, S=3, C=64),
    "peaked": dict(B=1, F=16, S=6, C=64, peaked=True),     # queries x 3, key 12 aligned with query 3 (x 4) at every pixel
}


def temporal_to_sequences(rows, B, Fr, S):
    """rows (b, f, s) -> (b, s, f): the frames of one pixel contiguous"""
    return rows.reshape(B, Fr, S, -1).permute(0, 2, 1, 3).reshape(B * S * Fr, -1)


def temporal_from_sequences(rows, B, Fr, S):
    return rows.reshape(B, S, Fr, -1).permute(0, 2, 1, 3).reshape(B * Fr * S, -1)


@functools.lru_cache(maxsize=None)
def temporal_case(cid):
    c = dict(TEMPORAL_CASES[cid])
    gen = _gen(4, cid, TEMPORAL_CASES)
    B, Fr, S, C = c["B"], c["F"], c["S"], c["C"]
    qkv = torch.randn(B, Fr, S, 3 * C, generator=gen)
    if c.get("peaked"):
        qkv[..., :64] *= 3.0
        qkv[:, 12, :, 64:128] = qkv[:, 3, :, :64] * 4.0
    c["qkv"] = bf(qkv.reshape(B * Fr * S, 3 * C))
    c["dout"] = bf(torch.randn(B * Fr * S, C, generator=gen))
    c["extra"] = bf(torch.randn(3 * C, generator=gen))
    c["peaked"] = bool(c.get("peaked"))
    c["ragged"] = Fr < 32
    return c


def _temporal_seq(c):
    B, Fr, S = c["B"], c["F"], c["S"]
    return temporal_to_sequences(c["qkv"], B, Fr, S), temporal_to_sequences(c["dout"], B, Fr, S), B * S, Fr, c["C"]


@functools.lru_cache(maxsize=None)
def temporal_reference(cid):
    """(out, dqkv) in fp64, rows in the kernel's (b, f, s) order"""
    c = temporal_case(cid)
    out, grad, _ = attn_reference(*_temporal_seq(c))
    return temporal_from_sequences(out, c["B"], c["F"], c["S"]), temporal_from_sequences(grad, c["B"], c["F"], c["S"])


def attn_blocks(t, C):
    """dq, dk, dv column blocks of a [rows, 3C] tensor"""
    return [t[:, i * C:(i + 1) * C] for i in range(3)]


@functools.lru_cache(maxsize=None)
def rounding_point_figure(kind, cid):
    """max over dq, dk, dv of parity_err(rounding-point reference, exact reference): what the kernel's rounding points alone
    cost on this case's data, from the reference alone."""
    from tests.parity_utils import parity_err
    if kind == "spatial":
        c = spatial_case(cid)
        exact = spatial_reference(cid)[1]
        rp = attn_rounding_point_reference(c["qkv"], c["dout"], c["n_img"], c["S"], c["C"])
    else:
        c = temporal_case(cid)
        exact = temporal_reference(cid)[1]
        rp = temporal_from_sequences(attn_rounding_point_reference(*_temporal_seq(c)), c["B"], c["F"], c["S"])
    return max(parity_err(a, b) for a, b in zip(attn_blocks(rp, c["C"]), attn_blocks(exact, c["C"])))


def attn_bound(kind, cid):
    """Bound against the exact reference: 1e-2 on plain data; on large / peaked logits twice the rounding-point reference's own
    error (the head-room test_attention_spatial_backward_peaked keeps: 1.3e-2 measured under 2e-2; it covers the fp32
    statistics and the summation order on top of the rounding points), and not below 1e-2."""
    c = spatial_case(cid) if kind == "spatial" else temporal_case(cid)
    return max(TOL_ATTN, 2.0 * rounding_point_figure(kind, cid)) if c["peaked"] else TOL_ATTN
