"""GPU: the grid-indexed searches (csrc/grid_nn.hip, ops.GridIndex) return bit for bit what the all-pairs kernels return --
ops.nn_dist and ops.knn_points, which the rest of the suite pins to the oracle.  Every comparison is torch.equal.

Clouds come from fixed seeds.  The shapes are the smallest at which the walk can go wrong: one point, one wave's worth of points
plus and minus one, a few thousand (several rings, several workgroups), 8192 (the codec's block) and one case of 40000 reference
points, above the ball-query grid's limit.  pccx_knn itself stops at 32768 reference points, so at 40000 the all-pairs reference
is assembled from it: the K best of each half of the cloud, merged by (distance, index) with a stable sort -- the same definition.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

from pccx import _lib, codec, large, ops, synth as cloud_synth

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 1000, 8192)
KS = (1, 16, 30, 32)


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _box(B):
    """per-cloud box: extents (1, 0.7, 0.4) scaled and shifted, so that clouds of a batch get different grids"""
    scale = torch.tensor([[1.0 + 0.5 * b] for b in range(B)])
    off = torch.tensor([[-3.0 + 2.5 * b, 0.25 * b, 10.0 - b] for b in range(B)])
    return (scale * torch.tensor([1.0, 0.7, 0.4]))[:, None, :], off[:, None, :]


def uniform(B, n, *seed):
    ext, off = _box(B)
    return (torch.rand(B, n, 3, generator=_gen("uniform", B, n, *seed)) * ext + off).float()


def flat(B, n, *seed):
    p = uniform(B, n, "flat", *seed)
    p[..., 2] = 0.0
    return p


def identical(B, n, *seed):
    return uniform(B, 1, "identical").expand(B, n, 3).contiguous()


def two_cluster(B, n, *seed):
    """99 % of the points in a ball of 1 % of the box, the rest in the far corner: most cells are empty"""
    g = _gen("cluster", B, n, *seed)
    ext, off = _box(B)
    v = torch.randn(B, n, 3, generator=g)
    v = v / v.norm(dim=2, keepdim=True).clamp_min(1e-9) * torch.rand(B, n, 1, generator=g) ** (1 / 3) * 0.005
    far = torch.rand(B, n, 1, generator=g) < 0.01
    far[:, 0] = False
    far[:, -1] = n > 1                                                       # both clusters present whenever there are two points
    p = torch.where(far, 0.97 + 0.03 * torch.rand(B, n, 3, generator=g), 0.02 + v)
    return (p * ext[..., :1] + off).float()


def void_queries(B, n, *seed):
    """queries for the two-cluster cloud: everywhere in the box, so most of them sit in the void between the clusters"""
    ext, off = _box(B)
    return (torch.rand(B, n, 3, generator=_gen("void", B, n, *seed)) * ext[..., :1] + off).float()


def lattice(B, *seed):
    """integer / 8 coordinates on a 12^3 lattice, every point twice, shuffled: exactly tied distances, duplicates, points on cell faces"""
    g = _gen("lattice", B, *seed)
    r = torch.arange(12, dtype=torch.float32) / 8
    p = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1).reshape(-1, 3).repeat(2, 1)
    return torch.stack([p[torch.randperm(p.shape[0], generator=g)] + float(b) for b in range(B)]).contiguous()


def lattice_queries(B, n, *seed):
    """integer / 16 coordinates from two steps outside the lattice to two steps beyond: on points, between them, outside"""
    return torch.stack([torch.randint(-4, 27, (n, 3), generator=_gen("latq", b, n, *seed)).float() / 16 + float(b) for b in range(B)])


def outside_queries(y, n, *seed):
    """a third inside the reference box, a third well outside on every side (0.75 to 1.5 extents from the centre), a third far outside,
    at 10 times the extent (the longest side) from the centre"""
    B = y.shape[0]
    g = _gen("outside", B, n, *seed)
    lo, hi = y.amin(dim=1, keepdim=True), y.amax(dim=1, keepdim=True)
    centre, half = (lo + hi) / 2, (hi - lo).amax(dim=2, keepdim=True) / 2
    d = torch.randn(B, n, 3, generator=g)
    d = d / d.abs().amax(dim=2, keepdim=True).clamp_min(1e-9)               # on the unit cube's surface: every side is hit
    kind = (torch.arange(n) % 3).view(1, n, 1)
    scale = torch.tensor([0.5, 3.0, 20.0])[kind] * torch.where(kind == 2, 1.0, torch.rand(B, n, 1, generator=g).clamp_min(0.5))
    return (centre + d * half * scale).float()


def _p_for(q, B):
    return max(1, q // 2) if (q + B) % 2 else 2 * q + 1                      # P != Q, around Q / 2 and 2 Q


def check_nn(x, y, index=None):
    index = index or ops.GridIndex(y)
    d_g, i_g = index.nn(x, return_idx=True)
    d_b, i_b = ops.nn_dist(x, y, return_idx=True)
    assert d_g.dtype == d_b.dtype and i_g.dtype == i_b.dtype and d_g.shape == d_b.shape
    assert torch.equal(d_g, d_b), f"nn distances differ at {(d_g != d_b).sum().item()} of {d_g.numel()} queries"
    assert torch.equal(i_g, i_b), f"nn indices differ at {(i_g != i_b).sum().item()} of {i_g.numel()} queries"
    assert torch.equal(index.nn(x), d_b)
    return index


def check_knn(x, y, index, brute=ops.knn_points):
    for K in KS:
        if K > y.shape[1]:
            continue
        got, want = index.knn(x, K), brute(x, y, K)
        assert got.dists.dtype == want.dists.dtype and got.idx.dtype == want.idx.dtype and got.idx.shape == want.idx.shape
        assert torch.equal(got.dists, want.dists), f"K={K}: distances differ at {(got.dists != want.dists).sum().item()} places"
        assert torch.equal(got.idx, want.idx), f"K={K}: indices differ at {(got.idx != want.idx).sum().item()} places"


def check(x, y):
    x, y = x.cuda(), y.cuda()
    check_knn(x, y, check_nn(x, y))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q", SIZES)
def test_uniform(Q, B):
    check(uniform(B, _p_for(Q, B), "x"), uniform(B, Q, "y"))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q", SIZES)
def test_flat(Q, B):
    y = flat(B, Q, "y")
    check(flat(B, _p_for(Q, B), "x"), y)                                     # queries in the plane
    if Q == 1000:
        check(uniform(B, _p_for(Q, B), "x"), y)                              # and off it


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q", SIZES)
def test_identical_points(Q, B):
    check(uniform(B, _p_for(Q, B), "x"), identical(B, Q))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q", SIZES)
def test_two_clusters(Q, B):
    y = two_cluster(B, Q, "y")
    check(two_cluster(B, _p_for(Q, B), "x"), y)                              # queries in the clusters
    if Q <= 1000:
        check(void_queries(B, _p_for(Q, B), "x"), y)                         # queries in the void: many empty rings
    else:
        check(void_queries(B, 257, "x"), y)


@pytest.mark.parametrize("B", [1, 3])
def test_lattice_ties(B):
    y = lattice(B)
    check(lattice_queries(B, 5000), y)
    check(y[:, :1500].contiguous(), y)                                       # the points themselves: distance 0 twice, then six ties


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q", SIZES)
def test_outside_queries(Q, B):
    y = uniform(B, Q, "y")
    check(outside_queries(y, _p_for(Q, B)), y)


def _knn_by_halves(x, y, K):
    """ops.knn_points for more reference points than pccx_knn takes: the K best of each half, merged by (distance, index).  The halves'
    rows are ascending by (distance, index) and the first half's indices are the lower ones, so a stable sort by distance of the
    concatenation is the (distance, index) order."""
    h = y.shape[1] // 2
    a, b = ops.knn_points(x, y[:, :h].contiguous(), K, return_nn=False), ops.knn_points(x, y[:, h:].contiguous(), K, return_nn=False)
    d = torch.cat([a.dists, b.dists], dim=2)
    i = torch.cat([a.idx, b.idx + h], dim=2)
    order = torch.sort(d, dim=2, stable=True).indices[..., :K]
    return ops.KNN(torch.gather(d, 2, order), torch.gather(i, 2, order), None)


def test_40000_points():
    """above BQ_NMAX = 32768 and pccx_knn's own limit: a grid of about 27 cells per axis, several rings for the 30-NN"""
    x, y = uniform(1, 20000, "x40k").cuda(), uniform(1, 40000, "y40k").cuda()
    index = check_nn(x, y)
    check_knn(x, y, index, brute=_knn_by_halves)
    out = outside_queries(y.cpu(), 2000).cuda()
    check_knn(out, y, check_nn(out, y, index), brute=_knn_by_halves)


@functools.lru_cache(maxsize=None)
def _metric_clouds(kind):
    if kind == "uniform":
        y = uniform(2, 8192, "metric")
        r = (y + 0.004 * torch.randn(2, 8192, 3, generator=_gen("jitter")))[:, :8000]
    else:
        y = lattice(2, "metric")
        r = (y + torch.randint(-1, 2, tuple(y.shape), generator=_gen("latjit")).float() / 16)[:, 100:]
    return y.cuda(), r.contiguous().cuda()


@pytest.mark.parametrize("kind", ["uniform", "lattice"])
def test_normals_and_metrics_match_brute(kind):
    y, r = _metric_clouds(kind)
    assert torch.equal(ops.estimate_normals(y, 30, search="grid"), ops.estimate_normals(y, 30))
    assert torch.equal(ops.estimate_normals(y, 30, search="brute"), ops.estimate_normals(y, 30))
    n = ops.estimate_normals(y, 30)
    assert torch.equal(ops.point_plane_err(r, y, n, search="grid"), ops.point_plane_err(r, y, n))
    assert torch.equal(ops.nn_dist(r, y, search="grid"), ops.nn_dist(r, y))
    for fn in (codec.d1_psnr, codec.d2_psnr, codec.normalized_chamfer):
        assert torch.equal(fn(y, r, search="grid"), fn(y, r)), fn.__name__
        assert torch.equal(fn(y, r, search="brute"), fn(y, r)), fn.__name__


def test_evaluate_large_matches_the_batched_metrics():
    n = 3 * 8192 + 100
    room = cloud_synth.room_cloud(5, n)
    rng = np.random.default_rng(6)
    recon = (room + rng.normal(0, 0.01, size=room.shape).astype(np.float32))[rng.permutation(n)[:n - 37]]
    a, b = torch.from_numpy(room).cuda(), torch.from_numpy(np.ascontiguousarray(recon)).cuda()
    got = large.evaluate_large(a, b)
    assert set(got) == {"d1_psnr", "d2_psnr", "chamfer", "n_points_input", "n_points_output"}
    assert all(type(v) is float for v in got.values())
    assert got["n_points_input"] == n and got["n_points_output"] == n - 37
    assert got["d1_psnr"] == float(codec.d1_psnr(a[None], b[None], search="brute")[0])
    assert got["d2_psnr"] == float(codec.d2_psnr(a[None], b[None], search="brute")[0])
    assert got["chamfer"] == float(codec.normalized_chamfer(a[None], b[None], search="brute")[0])
    assert 20.0 < got["d1_psnr"] < got["d2_psnr"] < 100.0                    # a centimetre of jitter in a room of metres


def test_arguments():
    y = uniform(1, 40, "args").cuda()
    x = uniform(1, 7, "argsx").cuda()
    index = ops.GridIndex(y)
    with pytest.raises(_lib.PccxError):
        index.knn(x, 33)
    small = ops.GridIndex(y[:, :5].contiguous())
    with pytest.raises(_lib.PccxError):
        small.knn(x, 6)                                                      # K > Q
    with pytest.raises(_lib.PccxError):
        index.knn(x, 0)
    with pytest.raises(_lib.PccxError):
        ops.GridIndex(torch.empty(1, 0, 3, device="cuda"))                   # Q = 0
    with pytest.raises(_lib.PccxError):
        index.nn(torch.empty(1, 0, 3, device="cuda"))                        # no queries
    with pytest.raises(_lib.PccxError):
        index.nn(uniform(2, 7, "argsb").cuda())                              # another batch size than the index
    n = ops.estimate_normals(y, 8)
    for call in (lambda: ops.nn_dist(x, y, search="kd"), lambda: ops.estimate_normals(y, 8, search="kd"),
                 lambda: ops.point_plane_err(x, y, n, search="kd"), lambda: codec.d1_psnr(y, x, search="kd"),
                 lambda: codec.d2_psnr(y, x, knn=8, search="kd"), lambda: codec.normalized_chamfer(y, x, search="kd")):
        with pytest.raises(ValueError):
            call()
