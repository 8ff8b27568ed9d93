"""numpy restatements of the arithmetic include/ctrlv_hip.h states for ctrlv_train_draws and ctrlv_train_assemble (section
"Training batches"), on top of tests/seeded_ref.py (Philox4x32-10, the fp32 uniforms, Box-Muller).  A helper module, not a
conftest: tests/test_train_batch_cpu.py proves the restatements (known answers, torch's own expressions), the GPU tests hold the
kernels against them."""
import numpy as np

from tests import seeded_ref as S

STREAM_DRAWS, STREAM_NOISE = 2, 3
F32 = np.float32


def index_of(x0, T):
    """(uint64(x0) * T) >> 32: in [0, T) for x0 < 2^32."""
    return ((np.asarray(x0, dtype=np.uint64) & S.MASK) * np.uint64(T)) >> S.S32


def thresholds(dropout_prob):
    """dp, 2 dp, 3 dp formed in double and rounded once to fp32: torch's cast of a Python scalar compared with an fp32 tensor."""
    dp = float(dropout_prob)
    return F32(dp), F32(2.0 * dp), F32(3.0 * dp)


def masks(p, dropout_prob):
    """(prompt_keep, image_mask) as fp32 0 / 1 of the fp32 uniforms p; dropout_prob None or negative: all ones."""
    p = np.asarray(p, dtype=F32)
    if dropout_prob is None or dropout_prob < 0:
        return np.ones_like(p), np.ones_like(p)
    t1, t2, t3 = thresholds(dropout_prob)
    keep = (~(p < t2)).astype(F32)
    image = F32(1) - (p >= t1).astype(F32) * (p < t3).astype(F32)
    return keep, image


def draws(seed, n_clips, sigma_table, timestep_table, clip0=0, call=0, dropout_prob=None):
    """dict of the six arrays ctrlv_train_draws writes for clips clip0 .. clip0 + n_clips - 1."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    clip = (np.arange(n_clips, dtype=np.uint64) + np.uint64(clip0)) & S.MASK
    zero = np.zeros_like(clip)
    x = S.philox4x32_10((zero, zero + np.uint64(call), zero + np.uint64(STREAM_DRAWS), clip), (seed & 0xFFFFFFFF, seed >> 32))
    idx = index_of(x[0], len(sigma_table)).astype(np.int64)
    p = S.uniforms(x[1])
    keep, image = masks(p, dropout_prob)
    return {"indices": idx.astype(np.int32), "sigmas": np.asarray(sigma_table, dtype=F32)[idx],
            "timesteps": np.asarray(timestep_table, dtype=F32)[idx], "random_p": p, "prompt_keep": keep, "image_mask": image}


def rne_el(x, el):
    """fp32 -> the element type (round to nearest even) -> fp32.  el: "bf16", "fp16" or None (fp32: unchanged)."""
    x = np.ascontiguousarray(x, dtype=F32)
    if el is None:
        return x
    if el == "fp16":
        return x.astype(np.float16).astype(F32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(F32)


def assemble(target, noise, sigmas, image_mask, cond_image, cond_frames=None, layout=0, K=0, el="bf16"):
    """(noisy fp32, sample as fp32 values already rounded to `el`) of ctrlv_train_assemble: every numpy operation below is one
    fp32 operation, rounded on its own; numpy's fp32 division and square root are correctly rounded."""
    target, noise = np.asarray(target, dtype=F32), np.asarray(noise, dtype=F32)
    n, F, L, h, w = target.shape
    s = np.asarray(sigmas, dtype=F32).reshape(n, 1, 1, 1, 1)
    noisy = target + noise * s
    inp = noisy / np.sqrt(s * s + F32(1))
    c = np.repeat(np.asarray(cond_image, dtype=F32)[:, None], F, axis=1)
    if layout == 1:
        for f in range(F):
            if f < K or f == F - 1:
                c[:, f] = np.asarray(cond_frames, dtype=F32)[:, f]
    m = np.ones(n, dtype=F32) if image_mask is None else np.asarray(image_mask, dtype=F32)
    cm = m.reshape(n, 1, 1, 1, 1) * c
    return noisy, rne_el(np.concatenate([inp, cm], axis=2), el)


def noise(seed, shape, clip0=0, call=0):
    """(z float64, r float64) of the in-kernel noise of ctrlv_train_assemble: seeded_ref.randn on stream 3, shaped (n, ...)."""
    per = int(np.prod(shape[1:]))
    z, r = S.randn(seed, shape[0], per, clip0=clip0, call=call, stream_id=STREAM_NOISE)
    return z.reshape(shape), r.reshape(shape)
