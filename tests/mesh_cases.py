"""The mesh sampler of DESIGN.md section 4.5 restated in numpy (its own Philox, uint64 weights, Python integers for the 64 x 64 product),
seeded test meshes, and an OFF writer with a switch for every liberty the grammar allows.  Shared by the CPU and GPU mesh tests."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox(key, ctr):
    """Philox4x32-10 on Python integers: key (k0, k1), counter (c0, c1, c2, c3) -> (x0, x1, x2, x3)"""
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_stream(seed, n):
    """x (n, 4) uint64 (each below 2^32): the words of samples 0 .. n - 1 of stream `seed`, vectorised"""
    seed = int(seed) & (2**64 - 1)
    k0, k1 = np.uint64(seed & MASK), np.uint64(seed >> 32)
    c = [np.arange(n, dtype=np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)]
    m = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                 # both factors below 2^32: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m]
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack(c, axis=1)


def weights(V, F):
    """-> (a (F,) float64, w (F,) uint64, I (F,) uint64 inclusive prefix, status 0 / 1)"""
    P = V.astype(np.float64)[F.astype(np.int64)]                            # (F, 3 corners, 3)
    u, v = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    cx, cy, cz = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    with np.errstate(all="ignore"):
        a = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
        amax = a.max()                                                      # a NaN area makes it NaN
        if not np.isfinite(amax) or amax == 0:
            return a, np.zeros(len(F), np.uint64), np.zeros(len(F), np.uint64), 1
        w = np.floor(a / amax * 2.0**40).astype(np.uint64)
    return a, w, np.cumsum(w, dtype=np.uint64), 0


def keys(x):
    """float32 -> uint32 keys that order as the floats do, -0 below +0"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def sample(V, F, seed, n, normalize="unit"):
    """-> (points (n, 3) float32, status, picked triangle of every sample (n,) int64)"""
    a, w, I, status = weights(V, F)
    if status:
        return np.full((n, 3), np.nan, dtype=np.float32), 1, np.full(n, -1, dtype=np.int64)
    W = int(I[-1])
    x = philox_stream(seed, n)
    target = np.array([(((int(r[1]) << 32) + int(r[0])) * W) >> 64 for r in x], dtype=np.uint64)
    t = np.searchsorted(I, target, side="right")                            # the first t with I_t > target
    assert (w[t] > 0).all()
    u, v = (x[:, 2].astype(np.float64) + 0.5) * 2.0**-32, (x[:, 3].astype(np.float64) + 0.5) * 2.0**-32
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    P = V.astype(np.float64)[F[t].astype(np.int64)]
    p = (P[:, 0] * u[:, None] + P[:, 1] * v[:, None] + P[:, 2] * (1 - (u + v))[:, None]).astype(np.float32)
    if normalize is None:
        return p, 0, t
    k = keys(p).reshape(-1)
    m, top = p.reshape(-1)[np.argmin(k)], p.reshape(-1)[np.argmax(k)]
    M = np.float32(top - m)
    q = p - m                                                               # float32 throughout
    if M == 0:
        return q, 2, t
    return q / M, 0, t


# ---- seeded meshes ------------------------------------------------------------------------------------------------------------------
def mesh(seed, nf, kind="random"):
    """A seeded triangle soup of nf faces -> (V float32, F int32).  kind: random | zero_ends (first and last face without area) |
    doubled (every face twice, nf counts both) | giant (one face 2^45 times the area of every other) | collinear (no area at all)"""
    rng = np.random.default_rng(seed)
    if kind == "doubled":
        V, F = mesh(seed, max(nf // 2, 1), "random")
        return V, np.concatenate([F, F])[:max(nf, 2)]
    nv = max(3, nf // 2 + 3)
    V = (rng.standard_normal((nv, 3)) * rng.uniform(0.1, 30)).astype(np.float32) + rng.uniform(-5, 5, 3).astype(np.float32)
    F = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int32)
    if kind == "zero_ends":
        F[0], F[-1] = (0, 0, 1), (2, 1, 1)
    elif kind == "giant":
        small = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
        V = np.concatenate([small * np.float32(2.0**-10), small * np.float32(2.0**12.5) + np.float32(3)]).astype(np.float32)
        F = np.array([[0, 1, 2]] * nf, dtype=np.int32)
        F[nf // 2] = (3, 4, 5)                                              # (2^22.5)^2 = 2^45 times the area of the others
    elif kind == "collinear":
        V = (rng.integers(-100, 100, (nv, 1)) * np.array([[1, 2, 3]])).astype(np.float32)
    return V, F


BATCH_FACES = (1, 2, 255, 256, 257, 4097)                                  # tile edges of 256 and a scan over 17 tiles


def batch(seed=7):
    """The GPU tests' batch: six random meshes of BATCH_FACES faces, then zero_ends, doubled and giant -> [(V, F, kind)]"""
    out = [mesh(seed + i, nf) + ("random",) for i, nf in enumerate(BATCH_FACES)]
    out += [mesh(seed + 10, 300, "zero_ends") + ("zero_ends",), mesh(seed + 11, 514, "doubled") + ("doubled",), mesh(seed + 12, 259, "giant") + ("giant",)]
    return out


def pack(meshes):
    """[(V, F, ...)] -> (verts, faces, v_off, f_off) numpy arrays in the packed form pccx_mesh_sample takes"""
    verts, faces = np.concatenate([m[0] for m in meshes]).astype(np.float32), np.concatenate([m[1] for m in meshes]).astype(np.int32)
    v_off = np.concatenate([[0], np.cumsum([len(m[0]) for m in meshes])]).astype(np.int64)
    f_off = np.concatenate([[0], np.cumsum([len(m[1]) for m in meshes])]).astype(np.int64)
    return verts, faces, v_off, f_off


# ---- OFF files ----------------------------------------------------------------------------------------------------------------------
def off_bytes(V, F, glued=False, comments=False, crlf=False, colours=False, blanks=False, tokens=None, final_newline=True):
    """The bytes of an OFF file of (V, F).  glued: OFF490 518 0 on one line; comments: comment lines and trailing comments; crlf: \\r\\n
    line ends; colours: r g b a behind every face; blanks: blank lines in every part; tokens: the text of every coordinate, (nv, 3)
    strings, instead of the shortest text that reads back as the float32."""
    nl = "\r\n" if crlf else "\n"
    out = []
    if comments:
        out.append("# a comment in front of everything")
    if glued:
        out.append(f"OFF{len(V)} {len(F)} 0" + (" # counts glued to the word" if comments else ""))
    else:
        out.append("OFF" + ("   # the word alone" if comments else ""))
        if blanks:
            out.append("")
        if comments:
            out.append("# nv nf ne")
        out.append(f"{len(V)} {len(F)} 0")
    for i, row in enumerate(V):
        t = tokens[i] if tokens is not None else [repr(float(x)) for x in row]
        out.append(("\t" if i % 5 == 1 else "") + " ".join(t) + ("  # v%d" % i if comments and i % 3 == 0 else ""))
        if blanks and i % 4 == 0:
            out.append("   ")
    if comments:
        out.append("#faces")
    for i, row in enumerate(F):
        out.append(f"3 {row[0]} {row[1]}  {row[2]}" + (" 255 0 128 1.0" if colours else "") + (" #f" if comments and i % 2 else ""))
        if blanks and i % 7 == 0:
            out.append("")
    text = nl.join(out) + (nl if final_newline else "")
    return text.encode("ascii")


def write_off(path, V, F, **kw):
    data = off_bytes(V, F, **kw)
    with open(path, "wb") as f:
        f.write(data)
    return data
