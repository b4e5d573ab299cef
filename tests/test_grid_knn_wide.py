"""GPU: the wide-K grid search (pccx_grid_knn_wide, ops.GridIndex.knn_wide, ops.knn_points(search="grid")) returns bit for bit what
the all-pairs ops.knn_points returns -- distances, indices and the gathered (optionally centred and scaled) neighbours.  Every
comparison is torch.equal.

Shapes: M = 37 queries per cloud (one workgroup each; not a multiple of anything), B = 2 clouds with different grids, reference
clouds of 33 .. 4096 points (one cell, a few cells, a few hundred cells), K on both sides of every power of two the LDS buffer and
its sort are sized by, K == N included.  The clouds are those of tests/test_grid_nn.py, each for the way it can go wrong.
"""
import pytest
import torch

from pccx import _lib, ops
from tests.test_grid_nn import (_knn_by_halves, check_knn, check_nn, flat, identical, lattice, lattice_queries, outside_queries, two_cluster, uniform,
                                void_queries)

pytestmark = pytest.mark.gpu

B, M = 2, 37
NS = (33, 64, 65, 257, 1000, 4096)
KS = (33, 64, 65, 256, 257, 1024)
SCALE = 1.2599


def check_wide(x, y, ks=KS, index=None):
    x, y = x.cuda(), y.cuda()
    index = index or ops.GridIndex(y)
    for K in ks:
        if K > y.shape[1]:
            continue
        want = ops.knn_points(x, y, K, return_nn=True)
        got = index.knn_wide(x, K, return_nn=True)
        for name in ("dists", "idx", "knn"):
            g, w = getattr(got, name), getattr(want, name)
            assert g.dtype == w.dtype and g.shape == w.shape, (K, name)
            assert torch.equal(g, w), f"K={K}: {name} differ at {(g != w).sum().item()} of {g.numel()} places"
        only = index.knn_wide(x, K, return_nn=True, patch_scale=SCALE, return_dists=False, return_idx=False)
        assert only.dists is None and only.idx is None
        assert torch.equal(only.knn, ops.knn_points(x, y, K, patch_scale=SCALE, return_dists=False, return_idx=False).knn), f"K={K}: scaled patches"
    return index


@pytest.mark.parametrize("N", NS)
def test_uniform(N):
    check_wide(uniform(B, M, "xw"), uniform(B, N, "yw"))


@pytest.mark.parametrize("N", NS)
def test_flat(N):
    y = flat(B, N, "yw")
    index = check_wide(flat(B, M, "xw"), y)
    check_wide(uniform(B, M, "xw"), y, ks=(33, 257), index=index)          # queries off the plane


@pytest.mark.parametrize("N", NS)
def test_identical_points(N):
    check_wide(uniform(B, M, "xw"), identical(B, N))                       # one cell holds everything; every distance ties


@pytest.mark.parametrize("N", NS)
def test_two_clusters_and_the_void(N):
    y = two_cluster(B, N, "yw")
    index = check_wide(two_cluster(B, M, "xw"), y)
    check_wide(void_queries(B, M, "xw"), y, index=index)                   # long walks through empty cells


def test_lattice_ties():
    y = lattice(B)                                                         # 3456 points, each twice: ties and points on cell faces
    index = check_wide(lattice_queries(B, M), y)
    check_wide(y[:, 100:100 + M].contiguous(), y, ks=(33, 65, 1024), index=index)


@pytest.mark.parametrize("N", NS)
def test_outside_queries(N):
    y = uniform(B, N, "yw")
    check_wide(outside_queries(y, M), y)                                   # the bound is never met: the integer loop ends the walk


def test_knn_points_search_grid():
    x, y = uniform(B, M, "xs").cuda(), uniform(B, 1000, "ys").cuda()
    index = ops.GridIndex(y)
    for K, kw in ((256, {}), (256, dict(index=index, return_nn=False)), (40, dict(patch_scale=SCALE, return_dists=False)),
                  (30, dict(return_nn=False)), (30, dict(index=index)), (32, dict(patch_scale=SCALE, return_idx=False))):
        got, want = ops.knn_points(x, y, K, search="grid", **kw), ops.knn_points(x, y, K, **{k: v for k, v in kw.items() if k != "index"})
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            assert g is None or torch.equal(g, w), (K, kw)
    assert torch.equal(ops.knn_points(x, y, 64, search="brute").idx, ops.knn_points(x, y, 64).idx)
    with pytest.raises(ValueError):
        ops.knn_points(x, y, 64, search="kdtree")


def test_k_32_is_served():
    """knn_wide takes the narrow walk's K as well (it is what gives knn_points(search="grid") the points and rep at those K)"""
    check_wide(uniform(B, M, "x32"), uniform(B, 257, "y32"), ks=(1, 32))


def test_rep_skips_the_copies():
    K = 64
    y = uniform(B, 1000, "yr").cuda()
    pick = torch.randint(0, 10, (M,), generator=torch.Generator().manual_seed(5))
    x = uniform(B, 10, "xr")[:, pick].contiguous().cuda()                   # 37 queries, at most 10 distinct per cloud
    groups = ops.patch_groups(x)
    is_rep = groups.rep.cpu() == torch.arange(B * M, dtype=torch.int32)
    assert 2 <= int(is_rep.sum()) <= 2 * 10
    want = ops.knn_points(x, y, K, patch_scale=SCALE)
    index = ops.GridIndex(y)
    for got in (index.knn_wide(x, K, return_nn=True, patch_scale=SCALE, rep=groups.rep),
                ops.knn_points(x, y, K, patch_scale=SCALE, search="grid", groups=groups),
                ops.knn_points(x, y, K, patch_scale=SCALE, search="grid", index=index, rep=groups.rep)):
        for g, w in zip(got, want):
            assert torch.equal(g.view(B * M, -1)[is_rep], w.view(B * M, -1)[is_rep])
        ops.replicate_rows(groups, got.dists)
        ops.replicate_rows(groups, got.knn)
        assert torch.equal(got.dists, want.dists) and torch.equal(got.knn, want.knn)


def test_40000_points():
    """above pccx_knn's 32768 points: the all-pairs answer from the two halves of the cloud (tests/test_grid_nn.py's construction)"""
    K = 256
    x, y = uniform(1, 64, "x40kw").cuda(), uniform(1, 40000, "y40k").cuda()
    want = _knn_by_halves(x, y, K)
    got = ops.GridIndex(y).knn_wide(x, K, return_nn=True, patch_scale=SCALE)
    assert torch.equal(got.dists, want.dists) and torch.equal(got.idx, want.idx)
    assert torch.equal(got.knn, (y[0][want.idx[0]] - x[0][:, None, :]).mul(SCALE)[None])
    with pytest.raises(_lib.PccxError):
        ops.knn_points(x, y, K)


def _raw(index, x, K, qws):
    Bq, Mq = x.shape[0], x.shape[1]
    d = torch.empty(Bq, Mq, K, device="cuda")
    i = torch.empty(Bq, Mq, K, device="cuda", dtype=torch.int64)
    nn = torch.empty(Bq, Mq, K, 3, device="cuda")
    _lib.call("pccx_grid_knn_wide", x.data_ptr(), Bq, Mq, index.Q, K, index.ws.data_ptr(), qws.data_ptr(), d.data_ptr(), i.data_ptr(),
              nn.data_ptr(), 0.0, None, torch.cuda.current_stream().cuda_stream)
    return d, i, nn


@pytest.mark.parametrize("K", [65, 1024])
def test_repeatable_with_a_dirty_workspace(K):
    """the same call twice, the query workspace overwritten in between: nothing is read before it is written"""
    x, y = uniform(B, M, "xq").cuda(), uniform(B, 4096, "yq").cuda()
    index = ops.GridIndex(y)
    qws = torch.empty(_lib.load().pccx_grid_knn_wide_workspace_bytes(B, 4096), device="cuda", dtype=torch.uint8)
    qws.fill_(0xFF)
    first = _raw(index, x, K, qws)
    qws.fill_(0xFF)
    second = _raw(index, x, K, qws)
    want = ops.knn_points(x, y, K)
    for a, b, w in zip(first, second, want):
        assert torch.equal(a, b) and torch.equal(a, w)


def test_refusals():
    x, y = uniform(B, M, "xq").cuda(), uniform(B, 1000, "yq").cuda()
    index = ops.GridIndex(y)
    with pytest.raises(_lib.PccxError):
        index.knn_wide(x, 1025)                                            # K > 1024 (and > N)
    with pytest.raises(_lib.PccxError):
        index.knn_wide(x, 1001)                                            # K > N
    with pytest.raises(_lib.PccxError):
        ops.GridIndex(uniform(B, 2000, "yq").cuda()).knn_wide(x, 1025)     # K > 1024 alone
    with pytest.raises(_lib.PccxError):
        index.knn_wide(x, 64, return_dists=False, return_idx=False)        # nothing asked for
    with pytest.raises(_lib.PccxError):
        index.knn_wide(x, 64, rep=torch.zeros(B * M + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(_lib.PccxError):
        index.knn_wide(x[:1].contiguous(), 64)                             # another batch than the index's
    with pytest.raises(_lib.PccxError):
        index.knn(x, 33)                                                   # the narrow walk keeps its limit


@pytest.mark.parametrize("target", [8, 64, 5000])
def test_coarser_cells_give_the_same_answers(target):
    """GridIndex(y, target): fewer, larger cells (down to one) change the walk, never a result -- of any of the three searches"""
    x, y = uniform(B, M, "xt").cuda(), uniform(B, 4096, "yt").cuda()
    index = ops.GridIndex(y, target)
    check_wide(x, y, ks=(33, 256, 1024), index=index)
    check_knn(x, y, check_nn(x, y, index))
    with pytest.raises(_lib.PccxError):
        ops.GridIndex(y, 1)
