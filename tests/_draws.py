"""NumPy restatement of the training draws (csrc/draws.h; include/inerf.h, "Training draws"): the oracle of inerf_draw_fill.

Written from the definition, not from the kernel:

    Philox4x32-10 (Random123): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds
    key      {seed & 0xffffffff, seed >> 32}
    counter  {ray, block | (stream << 16), step & 0xffffffff, step >> 32},  ray = ray_base + local index (mod 2^32),
             block = sample >> 2; the four output words are samples 4 block .. 4 block + 3
    uniform  (word >> 8) * 2^-24                                    streams 0 (jitter) and 2 (u): exact in fp32
    normal   u1 = ((w_even >> 9) + 1) * 2^-23, u2 = (w_odd >> 8) * 2^-24, r = sqrt(-2 log u1), theta = fp32(2 pi) * u2,
             even sample of a pair r cos(theta), odd sample r sin(theta)      streams 1 (coarse noise) and 3 (fine noise)
"""
import numpy as np

JITTER, NOISE_COARSE, U, NOISE_FINE = 0, 1, 2, 3
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)
TWO_PI_F32 = float(np.float32(2.0 * np.pi))
MAX_NORMAL = float(np.sqrt(2.0 * 23.0 * np.log(2.0)))          # u1 >= 2^-23


def philox4x32_10(counter, key):
    """counter: four broadcastable integer arrays, key: two -> four uint64 arrays holding the 32-bit output words."""
    u = np.uint64
    c = [np.asarray(x, dtype=u) & _M32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c[0] * u(M0), c[2] * u(M1)                     # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> u(32)) ^ c[1] ^ u(k0), p1 & _M32, (p0 >> u(32)) ^ c[3] ^ u(k1), p0 & _M32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def words(seed, step, stream, n_rays, n_per_ray, ray_base=0):
    """uint64 [n_rays, n_per_ray]: the 32-bit word of every (ray, sample)."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    n_blocks = (n_per_ray + 3) // 4
    ray = ((np.arange(n_rays, dtype=np.uint64) + np.uint64(ray_base)) & _M32)[:, None]
    block = np.arange(n_blocks, dtype=np.uint64)[None, :] | np.uint64(stream << 16)
    out = philox4x32_10((ray, block, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=-1).reshape(n_rays, 4 * n_blocks)[:, :n_per_ray]


def uniform_from(w):
    return ((w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)          # exact


def normal_parts(w):
    """(u1, u2) in fp64 (both exact fp32 values) for a word array whose last axis is even: pairs (0, 1), (2, 3), ..."""
    u1 = ((w[..., 0::2] >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -23
    u2 = (w[..., 1::2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normal_from(w, dtype=np.float64):
    """Box-Muller in ``dtype`` arithmetic; w: [..., n].  fp64 is the yardstick; fp32 the formula as the device rounds it (up to libm)."""
    n = w.shape[-1]
    if n % 2:
        w = np.concatenate([w, np.zeros(w.shape[:-1] + (1,), dtype=w.dtype)], axis=-1)
    u1, u2 = normal_parts(w)
    u1, u2 = u1.astype(dtype), u2.astype(dtype)
    r = np.sqrt(dtype(-2.0) * np.log(u1))
    theta = dtype(TWO_PI_F32) * u2
    out = np.stack([r * np.cos(theta), r * np.sin(theta)], axis=-1).reshape(w.shape)
    return out[..., :n]


def uniform(seed, step, stream, n_rays, n_per_ray, ray_base=0):
    return uniform_from(words(seed, step, stream, n_rays, 4 * ((n_per_ray + 3) // 4), ray_base))[:, :n_per_ray]


def normal(seed, step, stream, n_rays, n_per_ray, ray_base=0, dtype=np.float64):
    return normal_from(words(seed, step, stream, n_rays, 4 * ((n_per_ray + 3) // 4), ray_base), dtype)[:, :n_per_ray]
