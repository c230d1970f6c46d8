"""NumPy restatement of the index draw of csrc/batch.hip (inerf_batch_assemble with INERF_BATCH_DRAW): the oracle of form (b).

Integer arithmetic only (uint32 with wrap-around, one 64-bit product for ``below``), written from the specification in
include/inerf.h and the kernel's header comment - so every function here reproduces the device's value bit for bit:

    mix32(x)            x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
    step_key(seed, s)   the 64-bit seed and the 64-bit step absorbed 32 bits at a time
    stream_key(k0, j)   mix32(k0 + 0x85ebca6b (j + 1)); streams: 0 image, 1 / 2 the offsets in the reference's draw order,
                        3 the SSR pixels, 4 .. 11 the Feistel rounds
    draw(key, ray)      mix32(key ^ mix32(ray + 0x9e3779b9))
    below(word, n)      (word * n) >> 32
    perm                eight alternating Feistel rounds on b = a + c bits, a = b // 2, cycle-walked into [0, M), at most MAX_WALK
                        applications, then the value modulo M
"""
import numpy as np

MAX_WALK = 64          # INERF_BATCH_MAX_WALK
ROUNDS = 8
_M32 = 0xFFFFFFFF


def mix32(x):
    u = np.uint64
    x = np.asarray(x, dtype=u) & u(_M32)
    x = x ^ (x >> u(16))
    x = (x * u(0x7FEB352D)) & u(_M32)
    x = x ^ (x >> u(15))
    x = (x * u(0x846CA68B)) & u(_M32)
    x = x ^ (x >> u(16))
    return x


def step_key(seed, step):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    step = int(step) & 0xFFFFFFFFFFFFFFFF                  # two's complement of a negative step, as the device reads it
    h = mix32(((seed & _M32) + 0x9E3779B9) & _M32)
    h = mix32(h ^ np.uint64(seed >> 32))
    h = mix32(h ^ np.uint64(step & _M32))
    h = mix32(h ^ np.uint64(step >> 32))
    return int(h)


def stream_key(k0, stream):
    return int(mix32((int(k0) + 0x85EBCA6B * (int(stream) + 1)) & _M32))


def draw(key, ray):
    ray = np.asarray(ray, dtype=np.uint64)
    return mix32(np.uint64(key) ^ mix32((ray + np.uint64(0x9E3779B9)) & np.uint64(_M32)))


def below(word, n):
    return (np.asarray(word, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)


def split_bits(m):
    """(a, c): left and right half widths of the smallest b = a + c with 2^b >= m."""
    b = 0
    while (1 << b) < m:
        b += 1
    return b // 2, b - b // 2


def perm_once(x, bits_l, bits_r, keys):
    x = np.asarray(x, dtype=np.uint64)
    mask_l, mask_r = np.uint64((1 << bits_l) - 1), np.uint64((1 << bits_r) - 1)
    left, right = x >> np.uint64(bits_r), x & mask_r
    for i in range(ROUNDS):
        if i % 2 == 0:
            left = left ^ ((mix32(right ^ np.uint64(keys[i])) >> np.uint64(16)) & mask_l)
        else:
            right = right ^ ((mix32(left ^ np.uint64(keys[i])) >> np.uint64(16)) & mask_r)
    return (left << np.uint64(bits_r)) | right


def perm(k, m, seed, step, return_walk=False):
    """perm(k) on [0, m) for an array of rays k; with ``return_walk`` also the number of Feistel applications per ray and whether
    the bound was reached."""
    k0 = step_key(seed, step)
    keys = [stream_key(k0, 4 + i) for i in range(ROUNDS)]
    bits_l, bits_r = split_bits(m)
    x = np.array(k, dtype=np.uint64, ndmin=1)
    walk = np.zeros(x.shape, dtype=np.int64)
    todo = np.ones(x.shape, dtype=bool)
    for _ in range(MAX_WALK):
        if not todo.any():
            break
        x[todo] = perm_once(x[todo], bits_l, bits_r, keys)
        walk[todo] += 1
        todo &= x >= m
    hit = todo.copy()
    x[hit] %= np.uint64(m)
    out = x.astype(np.int64)
    return (out, walk, hit) if return_walk else out


def image(seed, step, n_images=None, image_ids=None):
    k0 = step_key(seed, step)
    n = len(image_ids) if image_ids is not None else int(n_images)
    j = int(below(draw(stream_key(k0, 0), 0), n))
    return int(image_ids[j]) if image_ids is not None else j


def offsets(seed, step, n):
    """(first, second): the two offset arrays in the reference's draw order (object level: row then column, run_nerf.py:920-921;
    SSR: column then row, rays.py:161-162), int64 with values in {-1, 0, 1}."""
    k0 = step_key(seed, step)
    rays = np.arange(n, dtype=np.uint64)
    first = below(draw(stream_key(k0, 1), rays), 3).astype(np.int64) - 1
    second = below(draw(stream_key(k0, 2), rays), 3).astype(np.int64) - 1
    return first, second


def object_draw(seed, step, n, m, n_images=None, image_ids=None):
    """(image, pixels[n] distinct in [0, m), off_row[n], off_col[n]) of the object-level form."""
    off_row, off_col = offsets(seed, step, n)
    return image(seed, step, n_images, image_ids), perm(np.arange(n), m, seed, step), off_row, off_col


def ssr_draw(seed, step, n, hw, n_images=None, image_ids=None):
    """(image, pixels[n] in [0, hw) with replacement, off_row[n], off_col[n]) of the SSR form."""
    off_col, off_row = offsets(seed, step, n)
    k0 = step_key(seed, step)
    pixels = (draw(stream_key(k0, 3), np.arange(n, dtype=np.uint64)) % np.uint64(hw)).astype(np.int64)
    return image(seed, step, n_images, image_ids), pixels, off_row, off_col
