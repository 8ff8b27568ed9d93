"""numpy restatements of the arithmetic include/ctrlv_hip.h states for ctrlv_randn (section "Seeded clips": Philox4x32-10, the
fp32 uniforms, Box-Muller) and for ctrlv_resize_lanczos_u8 (PIL's 8-bit Lanczos resample).  A helper module, not a conftest:
tests/test_seeded_cpu.py proves the restatements (known answers, moments, PIL), tests/test_seeded_gpu.py holds the kernels
against them."""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
MAX_ABS = math.sqrt(66.0 * math.log(2.0))        # |z| <= sqrt(-2 ln 2^-33)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (values < 2^32) of one shape, key: two such values -> four uint64 arrays (Random123)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in counter)
    k0, k1 = np.uint64(key[0]) & MASK, np.uint64(key[1]) & MASK
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                    # 32 x 32 -> 64 bits: never wraps
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniforms(x):
    """(x + 0.5) / 2^32 rounded once to fp32, ties to even: 2 x + 1 (33 bits) is exact in float64, so is the power of two."""
    return ((2.0 * x.astype(np.float64) + 1.0) * 2.0 ** -33).astype(np.float32)


def randn(seed, n_clips, per_clip, clip0=0, call=0, stream_id=0):
    """(z float64 (n_clips, per_clip), r float64 of the same shape): the normals of ctrlv_randn at scale 1 -- Box-Muller in
    float64 on the fp32 uniforms -- and each one's radius sqrt(-2 ln u_a) (what the error of the fp32 kernel scales with)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nblk = (per_clip + 3) // 4
    j = np.arange(nblk, dtype=np.uint64)
    z = np.empty((n_clips, nblk * 4), dtype=np.float64)
    r = np.empty_like(z)
    for i in range(n_clips):
        clip = np.uint64((clip0 + i) & 0xFFFFFFFF)
        x = philox4x32_10((j, np.full_like(j, call), np.full_like(j, stream_id), np.full_like(j, clip)),
                          (seed & 0xFFFFFFFF, seed >> 32))
        u = [uniforms(v).astype(np.float64) for v in x]
        for a in (0, 2):
            rad = np.sqrt(-2.0 * np.log(u[a]))
            theta = 2.0 * np.pi * u[a + 1]
            z[i, a::4], z[i, a + 1::4] = rad * np.cos(theta), rad * np.sin(theta)
            r[i, a::4] = r[i, a + 1::4] = rad
    return z[:, :per_clip], r[:, :per_clip]


def _lanczos3(v):
    def sinc(t):
        t = np.where(t == 0.0, 1.0, t) * np.pi
        return np.sin(t) / t
    out = np.where(v == 0.0, 1.0, sinc(v) * sinc(v / 3.0))
    return np.where((v >= -3.0) & (v < 3.0), out, 0.0)


def lanczos_tables(n_in, n_out):
    """Per output index: (first tap, int32 weights in 22-bit fixed point), as PIL's precompute_coeffs + normalize_coeffs_8bpc."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    rows = []
    for x in range(n_out):
        center = (x + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        k = _lanczos3((np.arange(xmax - xmin, dtype=np.float64) + xmin - center + 0.5) / fs)
        total = k.sum()
        if total != 0.0:
            k = k / total
        fixed = np.where(k < 0.0, np.trunc(k * 4194304.0 - 0.5), np.trunc(k * 4194304.0 + 0.5)).astype(np.int64)
        rows.append((xmin, fixed))
    return rows


def _lanczos_pass(img, n_out, axis):
    """img (..., H, W, 3) uint8 resampled along `axis` (-3: rows, -2: columns)."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
    for x, (xmin, k) in enumerate(lanczos_tables(src.shape[0], n_out)):
        acc = (1 << 21) + np.tensordot(k, src[xmin:xmin + len(k)], axes=(0, 0))
        out[x] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_lanczos_u8(img, h, w):
    """(..., H, W, 3) uint8 -> (..., h, w, 3): the horizontal pass into a uint8 intermediate, then the vertical one."""
    return _lanczos_pass(_lanczos_pass(img, w, -2), h, -3)
