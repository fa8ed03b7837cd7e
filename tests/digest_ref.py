"""A NumPy restatement of the state digest (include/mk.h "checkpoints") and of the regions it is taken over:
plain uint64 wrap-around arithmetic that shares no code with the device.  tests/test_digest_ref.py pins it on the
CPU to sums worked by hand.

    D = sum_i mix(x_i + (i + 1) * 0x9E3779B97F4A7C15) mod 2^64
    mix: x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31"""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


def words_of(a):
    """An array's 8-byte words in C order, as uint64 bit patterns."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 8, a.dtype
    return a.reshape(-1).view(np.uint64)


def mix(x):
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= M1
        x ^= x >> np.uint64(27)
        x *= M2
        x ^= x >> np.uint64(31)
    return x


def digest(a):
    """The digest of an array's words, a Python int below 2^64; 0 for no words."""
    x = words_of(a)
    if x.size == 0:
        return 0
    with np.errstate(over="ignore"):
        i = np.arange(1, x.size + 1, dtype=np.uint64)
        return int(np.sum(mix(x + i * GOLDEN), dtype=np.uint64))


def region_tri(M, ns):
    """MK_DIGEST_L / MK_DIGEST_W: the lower triangle of the leading ns x ns block of M (row, column), column-major
    -- column c holds rows c .. ns - 1."""
    M = np.asarray(M, dtype=np.float64)
    return np.concatenate([M[c:ns, c] for c in range(ns)]) if ns else np.zeros(0)


def region_tiles(tiles, ns, full):
    """MK_DIGEST_WINV (full=False) / MK_DIGEST_QB (full=True): tiles[k] the k-th 128 x 128 tile (row, column); per
    tile with m_k = min(128, ns - 128 k) > 0 rows and columns below m_k, column-major: the lower triangle (Winv),
    or the two diagonal 64 x 64 quadrants, quadrant 0 then 1 (QB: no other part of a tile is ever computed)."""
    out = []
    for k, T in enumerate(tiles):
        m = min(128, ns - 128 * k)
        if m <= 0:
            break
        T = np.asarray(T, dtype=np.float64)
        if not full:
            out += [T[c:m, c] for c in range(m)]
            continue
        for r0 in (0, 64):
            out += [T[r0:min(r0 + 64, m), c] for c in range(r0, min(r0 + 64, m))]
    return np.concatenate(out) if out else np.zeros(0)
