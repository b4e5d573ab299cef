"""GPU: the wide forms for 1024 < S <= 8192 centres -- pccx_octree_encode_wide, pccx_octree_decode above 1024 (mode 2 at any size),
pccx_patch_groups_wide -- bit for bit against the C oracle, a closed-form numpy reference and the narrow kernels.

The oracle's encode_sampled is the reference's depth search: it re-encodes the cloud up to 16 times with an O(nodes * S) walk, which
takes 9 s for 8192 uniform centres on a CPU and a minute when the uniqueness test never passes.  It is therefore the reference up to
S = 2080; `_encode_ref` below (the same stream from sorted cell codes, in numpy) is pinned against the oracle at those sizes IN THIS
FILE and is the reference at 4096, 8191 and 8192.  The oracle's decode is fast and is the reference at every size.
"""
import numpy as np
import pytest
import torch

from oracle import cport
from pccx import ops

pytestmark = pytest.mark.gpu

SIZES = [1025, 1040, 2080, 4096, 8191, 8192]
ORACLE_MAX_S = 2080
KINDS = ["uniform", "one_cell", "duplicates", "outside"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _clouds(kind, S, seed):
    rng = np.random.default_rng(seed)
    p = (0.005 + 0.99 * rng.random((S, 3))).astype(np.float32)
    if kind == "one_cell":                               # every centre inside one 2^-10 cell: sixteen levels of one chain, then a fan
        p = (np.float32(0.3125) + np.float32(2.0 ** -10) * rng.random((S, 3), dtype=np.float32)).astype(np.float32)
    elif kind == "duplicates":                           # the uniqueness test never passes: depth 17, the stream of depth 16
        p[S // 2] = p[3]
        p[S - 1] = p[S - 2]
    elif kind == "outside":                              # coordinates < 0 and >= 1 keep their identity but not their bits
        p[::7] = (-0.25 + 1.5 * rng.random((len(p[::7]), 3))).astype(np.float32)
        p[1] = [1.0, 0.5, 0.5]
        p[2] = [-0.0, 0.0, 0.999999]
    return p


def _spread(v):
    x = v.astype(np.uint64) & np.uint64(0x1fffff)
    for s, m in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(s))) & np.uint64(m)
    return x


def _encode_ref(p, N, min_bpp):
    """pn_kit.encode_sampled_np in closed form: (bits, depth).  Level-D cells are q >> (16 - D) of q = floor(p * 2^16); the reference's
    LIFO walk visits the occupied cells of a level in DESCENDING Morton order and writes one bit per child 7..0."""
    f = np.floor(p.astype(np.float32) * np.float32(65536.0))
    q = (np.clip(f, -(1 << 20), (1 << 20) - 1).astype(np.int64) + (1 << 20))
    inside = ((q >= (1 << 20)) & (q < (1 << 20) + 65536)).all(axis=1)
    key = (_spread(q[:, 0]) << np.uint64(2)) | (_spread(q[:, 1]) << np.uint64(1)) | _spread(q[:, 2])
    kin = np.sort(key[inside])
    S = p.shape[0]
    bits = [np.array([1 if kin.size else 0], dtype=np.uint8)]
    prev = np.unique(kin >> np.uint64(48))              # level 0: the root, when any centre is inside
    depth = 17
    for D in range(1, 17):
        sh = np.uint64(3 * (16 - D))
        if prev.size:
            occ = np.unique(kin >> sh)
            level = np.zeros(8 * prev.size, dtype=np.uint8)
            r = np.searchsorted(prev, occ >> np.uint64(3))
            level[8 * (prev.size - 1 - r) + (7 - (occ & np.uint64(7)).astype(np.int64))] = 1
            bits.append(level)
            prev = occ
        nb = sum(b.size for b in bits)
        if nb / N > min_bpp and np.unique(key >> sh).size == S:
            depth = D
            break
    return np.concatenate(bits), depth


def _check_encode(r, b, want, depth):
    nb = int(r["nbits"][b])
    assert nb == want.shape[0] and int(r["depth"][b]) == depth, f"{nb} vs {want.shape[0]} bits, depth {int(r['depth'][b])} vs {depth}"
    assert np.array_equal(r["bits"][b, :nb].cpu().numpy(), want)
    ny = int(r["nbytes"][b])
    assert r["bytes"][b, :ny].cpu().numpy().tobytes() == bytes(cport.pack_bits(want))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", SIZES)
def test_encode_wide(S, kind):
    N, min_bpp = 32 * S, 1.0                               # K = 64
    p = _clouds(kind, S, S + len(kind))
    want, depth = _encode_ref(p, N, min_bpp)
    if S <= ORACLE_MAX_S:
        obits, odepth = cport.encode_sampled(p, 1, N, min_bpp)
        assert odepth == depth and np.array_equal(obits, want), "the numpy closed form left the oracle"
    r = ops.octree_encode(dev(p[None]), N, min_bpp)
    _check_encode(r, 0, want, depth)
    if kind == "duplicates":
        assert depth == 17


@pytest.mark.parametrize("S", [64, 1000, 1024])
def test_encode_wide_equals_the_narrow_kernel(S):
    rng = np.random.default_rng(S)
    pcs = np.stack([_clouds(k, S, 3 * S + i) for i, k in enumerate(KINDS)])
    pcs[0, 5] = 1.5 + rng.random(3)
    a = ops.octree_encode(dev(pcs), 32 * S, 1.0)
    b = ops.octree_encode(dev(pcs), 32 * S, 1.0, wide=True)
    for k in ("nbits", "depth", "nbytes"):
        assert torch.equal(a[k], b[k]), k
    for i in range(len(KINDS)):
        assert torch.equal(a["bits"][i, :int(a["nbits"][i])], b["bits"][i, :int(a["nbits"][i])])
        assert torch.equal(a["bytes"][i, :int(a["nbytes"][i])], b["bytes"][i, :int(a["nbytes"][i])])
    want, depth = _encode_ref(pcs[0], 32 * S, 1.0)
    _check_encode(b, 0, want, depth)


@pytest.mark.parametrize("S", [64, 1025, 2080, 8191, 8192])
def test_full_decode_equals_the_oracle(S):
    pcs = np.stack([_clouds(k, S, 5 * S + i) for i, k in enumerate(["uniform", "one_cell", "outside"])])
    r = ops.octree_encode(dev(pcs), 32 * S, 1.0, wide=True)
    out, cnt = ops.octree_decode(r["bytes"], r["nbytes"], "full", S_out=S, wide=True)
    for b in range(pcs.shape[0]):
        want, d = cport.octree_decode_full(r["bits"][b, :int(r["nbits"][b])].cpu().numpy(), 1, cap=8192 + 8)
        assert d == min(int(r["depth"][b]), 16) and int(cnt[b]) == want.shape[0]   # count = the number of leaves
        got = out[b].cpu().numpy()
        assert np.array_equal(got[:want.shape[0]], want)
        assert (got[want.shape[0]:] == want[-1]).all()                             # the rest repeats the last leaf
    if S <= 1024:                                                                  # ... and the narrow kernel where it decodes at all
        narrow, ncnt = ops.octree_decode(r["bytes"], r["nbytes"], "full", S_out=S)
        assert torch.equal(narrow, out) and torch.equal(ncnt, cnt)


def test_full_decode_refuses_a_level_of_more_than_8192_cells():
    """every child set: 8, 64, 512, 4096 cells -- decoded -- and with one more level 32768, refused with count -1"""
    def stream(levels):
        nbytes = sum(8 ** l for l in range(levels))                  # 1 + 8 * nbytes bits, all ones
        return np.concatenate([np.full(nbytes, 0xFF, np.uint8), np.array([1], np.uint8)])
    ok, bad = stream(4), stream(5)
    rows = np.zeros((2, bad.size), np.uint8)
    rows[0, :ok.size], rows[1] = ok, bad
    out, cnt = ops.octree_decode(dev(rows), dev(np.array([ok.size, bad.size], np.int32)), "full", S_out=4096, wide=True)
    assert cnt.tolist() == [4096, -1]
    want, d = cport.octree_decode_full(np.ones(8 * (ok.size - 1) + 1, np.uint8), 1, cap=4096)
    assert d == 4 and np.array_equal(out[0].cpu().numpy(), want)
    _, cnt = ops.octree_decode(dev(rows), dev(np.array([ok.size, bad.size], np.int32)), "full", S_out=2048)     # S_out > 1024: wide
    assert cnt.tolist() == [4096, -1]
    _, cnt = ops.octree_decode(dev(rows), dev(np.array([ok.size, bad.size], np.int32)), "full", S_out=64)       # narrow: 2048 at the most
    assert cnt.tolist() == [-1, -1]


def _groups_ref(rows):
    """first-equal-row reference over uint32 words: rep, uniq (ascending), n_uniq -- indices across the whole batch"""
    B, S, _ = rows.shape
    rep = np.empty((B, S), np.int64)
    for b in range(B):
        _, first, inv = np.unique(rows[b], axis=0, return_index=True, return_inverse=True)
        rep[b] = first[inv.reshape(-1)] + b * S
    rep = rep.reshape(-1)
    return rep, np.flatnonzero(rep == np.arange(B * S))


@pytest.mark.parametrize("S", [64, 1025, 8192])
def test_patch_groups_wide(S):
    rng = np.random.default_rng(S)
    B = 2
    a = rng.random((B, S, 3), dtype=np.float32)
    kb = rng.integers(-2, 3, (B, S, 5)).astype(np.float32)
    src = rng.integers(0, S, (B, S // 3))
    dst = rng.integers(0, S, (B, S // 3))
    for b in range(B):                                   # planted repeats, some of them chains, in both key arrays
        a[b, dst[b]] = a[b, src[b]]
        kb[b, dst[b]] = kb[b, src[b]]
    a[0, 7], a[0, 9] = [0.0, 0.5, 0.25], [-0.0, 0.5, 0.25]       # -0 and +0 are different rows
    kb[0, 7] = kb[0, 9]
    a[1, 3] = a[1, 1] = [-0.0, -0.0, 1.0]
    kb[1, 3] = kb[1, 1]
    for with_b in (True, False):
        rows = np.concatenate([a, kb], axis=2).view(np.uint32) if with_b else a.view(np.uint32)
        rep, uniq = _groups_ref(rows)
        g = ops.patch_groups(dev(a), dev(kb) if with_b else None, wide=True)
        n = int(g.n_uniq)
        assert n == uniq.size
        assert np.array_equal(g.rep.cpu().numpy(), rep)
        assert np.array_equal(g.uniq[:n].cpu().numpy(), uniq)
        if S <= 1024:
            h = ops.patch_groups(dev(a), dev(kb) if with_b else None)
            assert torch.equal(h.rep, g.rep) and int(h.n_uniq) == n and torch.equal(h.uniq[:n], g.uniq[:n])
    if with_b is False:
        assert rep[9] == 9 and rep[S + 3] == S + 1
