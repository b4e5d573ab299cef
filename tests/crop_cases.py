"""The float32 numpy restatement of ops.crop_nearest and the named inputs its CPU and GPU tests share."""
import numpy as np


def sqdist_bits(points, s):
    """uint32 bit patterns of common.h's pccx_sqdist(seed, p_i) in float32: three products, two adds, each rounded on its own"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    s = np.asarray(s, dtype=np.float32)
    dx, dy, dz = s[0] - p[:, 0], s[1] - p[:, 1], s[2] - p[:, 2]
    d = dx * dx
    d = d + dy * dy
    d = d + dz * dz
    return np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)


def crop_nearest_np(points, seed, n):
    """the indices (ascending) of the n points with the smallest keys (bits of the squared distance to points[seed], index), and
    those points: -> (idx (n,) int32, crop (n, 3) float32)"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    bits = sqdist_bits(p, p[seed])
    order = np.lexsort((np.arange(len(p)), bits))            # last key is the primary one
    idx = np.sort(order[:n]).astype(np.int32)
    return idx, p[idx]


def padded(points, seed, n, N_cap):
    """crop_nearest_np as ops.crop_nearest lays a slot out: (out (N_cap, 3) with NaN behind n, idx (N_cap,) with -1 behind n)"""
    idx, crop = crop_nearest_np(points, seed, n)
    out = np.full((N_cap, 3), np.nan, dtype=np.float32)
    oi = np.full(N_cap, -1, dtype=np.int32)
    out[:n], oi[:n] = crop, idx
    return out, oi


# ---- the named inputs ---------------------------------------------------------------------------------------------------------------------
def lattice16(shuffle_seed=5):
    """the 16^3 lattice {0..15}/16 in a seeded shuffle, and the index of the point (0.5, 0.5, 0.5): distances from it come in shells
    of equal keys (6 at 1/256, 12 at 2/256, 8 at 3/256, 6 at 4/256, 24 at 5/256, 24 at 6/256, 12 at 8/256, 30 at 9/256, ...)"""
    g = np.arange(16, dtype=np.float32) / np.float32(16)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    p = p[np.random.default_rng(shuffle_seed).permutation(len(p))]
    seed = int(np.flatnonzero((p == np.float32(0.5)).all(1))[0])
    return np.ascontiguousarray(p), seed


def line_low_bits():
    """x = 1 + i * 2^-20, i < 3000, behind the origin (index 0, the seed): 3000 distinct keys that share their top 11 bits and have
    47 distinct top-22-bit values -- only the last radix pass separates them.  -> (points (3001, 3), seed index 0)"""
    x = (1.0 + np.arange(3000, dtype=np.float64) * 2.0 ** -20).astype(np.float32)
    p = np.zeros((3001, 3), dtype=np.float32)
    p[1:, 0] = x
    return p, 0


def exponents():
    """points at 2^k on the x axis for k = -60..60, the run repeated 5 times, behind the origin (index 0, the seed): squared distances
    2^(2k) differ in their exponent alone (2^-120 is still a normal float32), and every one occurs 5 times"""
    x = np.tile((2.0 ** np.arange(-60, 61, dtype=np.float64)).astype(np.float32), 5)
    p = np.zeros((1 + len(x), 3), dtype=np.float32)
    p[1:, 0] = x
    return p, 0


def duplicates():
    """5000 copies of one point"""
    return np.tile(np.array([[0.25, -1.5, 3.0]], dtype=np.float32), (5000, 1))


def uniform_cloud(seed, n):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)
