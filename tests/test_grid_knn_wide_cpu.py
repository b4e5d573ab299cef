"""Host-only parts of the wide-K grid search (pccx_grid_knn_wide, csrc/grid_nn.hip): its workspace size and its argument checks,
which run before anything is launched.  No GPU is touched: the pointers below are never dereferenced."""
import pytest

from pccx import _lib

PTR = 4096          # any non-null, 16-byte aligned address: a refused call does not read it


def wide(B=2, M=37, N=1000, K=64, q=PTR, index=PTR, qws=PTR, dists=PTR, idx=PTR, nn=PTR, rep=None):
    _lib.call("pccx_grid_knn_wide", q, B, M, N, K, index, qws, dists, idx, nn, 0.0, rep, None)


def test_workspace_size():
    fn = _lib.load().pccx_grid_knn_wide_workspace_bytes
    assert fn(0, 8192) == 0 and fn(4, 0) == 0 and fn(0, 0) == 0
    for B in (1, 3, 64):
        sizes = [fn(B, N) for N in (1, 33, 1000, 40000, 131072)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and all(s % 16 == 0 for s in sizes)
    assert fn(1, 131072) >= 4 * 131072                                     # one position per point of the index


@pytest.mark.parametrize("kw", [dict(K=1025, N=4096), dict(K=1001), dict(K=0), dict(dists=None, idx=None, nn=None), dict(q=None), dict(index=None),
                                dict(qws=None), dict(index=PTR + 4), dict(qws=PTR + 8), dict(B=0), dict(B=65536), dict(M=0), dict(N=0),
                                dict(B=4, N=2 ** 29, K=64), dict(B=4, M=2 ** 29)])
def test_bad_arguments_are_errors(kw):
    with pytest.raises(_lib.PccxError, match=r"\): pccx_grid_knn_wide: "):           # the entry's own check, not a failed launch
        wide(**kw)
