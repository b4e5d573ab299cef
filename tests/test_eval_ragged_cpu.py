"""CPU: the host side of the ragged evaluation -- eval_ragged_refusal against hand values, the count checks of the new ops wrappers and
of codec.evaluate_ragged (raised before anything is launched), and the C entry points' argument checks (null pointers, B == 0, a bad
shape: the error code, before any HIP call)."""
import pytest
import torch

from pccx import _lib, codec, ops

NEW_SYMBOLS = ("pccx_minmax_n", "pccx_query_rep_n", "pccx_estimate_normals_n", "pccx_point_errors_n", "pccx_mean_var_n")


def test_eval_ragged_refusal():
    assert codec.eval_ragged_refusal([30, 32768, 2048], [2, 32768, 2047]) is None
    assert codec.eval_ragged_refusal([], []) is None
    assert codec.eval_ragged_refusal([20], [20], knn=20) is None and codec.eval_ragged_refusal([5], [2], knn=5) is None
    for n, m, knn, msg in (([2048, 29], [2048, 2048], 30, "pair 1: the original holds 29 points"),
                           ([32769], [2048], 30, "pair 0: the original holds 32769 points"),
                           ([2048], [1], 30, "pair 0: the reconstruction holds 1 points"),
                           ([2048, 2048], [2048, 32769], 30, "pair 1: the reconstruction holds 32769 points"),
                           ([30], [30], 31, "knn = 31 <= n_b"),
                           ([2048, 2048], [2048], 30, "2 originals against 1 reconstructions")):
        why = codec.eval_ragged_refusal(n, m, knn)
        assert why is not None and msg in why and why.endswith(codec.EVAL_RAGGED_WAY_OUT), (n, m, why)
        if "against" not in msg:
            assert "KNN_BRUTE_MAX_N = 32768" in why
    assert "one pair per call" in codec.EVAL_RAGGED_WAY_OUT


@pytest.fixture
def calls(monkeypatch):
    made = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: made.append(name))
    return made


def test_wrappers_check_host_counts_before_any_launch(calls):
    x, y, v = torch.empty(2, 100, 3, device="meta"), torch.empty(2, 80, 3, device="meta"), torch.empty(2, 100, device="meta")
    for fn, msg in ((lambda: ops.minmax_n(x, [100, 101]), r"minmax_n.n: every length must lie in \[1, 100\].*101 for cloud 1"),
                    (lambda: ops.minmax_n(x, [0, 100]), r"minmax_n.n: every length.*0 for cloud 0"),
                    (lambda: ops.minmax_n(x, [100]), r"minmax_n.n: one int per cloud is expected"),
                    (lambda: ops.estimate_normals_n(x, [100, 29]), r"estimate_normals_n.n: every cloud needs at least knn = 30 points, got 29 for cloud 1"),
                    (lambda: ops.estimate_normals_n(x, [100, 101]), r"estimate_normals_n.n: every length must lie in \[1, 100\]"),
                    (lambda: ops.estimate_normals_n(x, [100, 100], knn=101), r"knn=101 neighbours in a slab of 100 rows"),
                    (lambda: ops.point_errors_n(x, y, [100, 100], [80, 81]), r"point_errors_n.y_lengths: every length must lie in \[1, 80\]"),
                    (lambda: ops.point_errors_n(x, y, [100, 0], [80, 80]), r"point_errors_n.x_lengths: every length.*0 for cloud 1"),
                    (lambda: ops.point_errors_n(x, y, [100, 100], [80, 80], normals_y=x), r"one normal per row of y"),
                    (lambda: ops.mean_var_n(v, [100, 200]), r"mean_var_n.n: every length must lie in \[1, 100\]"),
                    (lambda: ops.mean_var_n(x, [100, 100]), r"mean_var_n: a padded slab \(B, rows\)"),
                    (lambda: ops.minmax_n(v, [100, 100]), r"minmax_n: a padded slab \(B, rows, 3\)")):
        with pytest.raises(_lib.PccxError, match=msg):
            fn()
    # counts that pass: the next thing a wrapper wants is a tensor on the GPU -- there is no CPU path
    with pytest.raises(_lib.PccxError, match="expected a tensor on the GPU"):
        ops.minmax_n(x, [100, 1])
    assert calls == []


def test_evaluate_ragged_refuses_before_any_launch(calls):
    a, b = torch.empty(2, 2048, 3, device="meta"), torch.empty(2, 2048, 3, device="meta")
    with pytest.raises(ValueError, match=r"pair 1: the original holds 29 points.*one pair per call"):
        codec.evaluate_ragged(a, [2048, 29], b, [2048, 2048])
    with pytest.raises(ValueError, match=r"pair 0: the reconstruction holds 1 points"):
        codec.evaluate_ragged(a, [2048, 2048], b, [1, 2048])
    with pytest.raises(ValueError, match="2 originals against 1 reconstructions"):
        codec.evaluate_ragged(a, [2048, 2048], b, [2048])
    with pytest.raises(_lib.PccxError, match=r"n_orig: every length must lie in \[1, 2048\]"):
        codec.evaluate_ragged(a, [2048, 4096], b, [2048, 2048])
    with pytest.raises(_lib.PccxError, match="KNN_BRUTE_MAX_N = 32768"):
        codec.evaluate_ragged(torch.empty(1, 40000, 3, device="meta"), [2048], b[:1], [2048])
    assert calls == []


def test_abi_of_the_new_entry_points():
    """Declared, exported, and every argument check made on the host: a null pointer or a bad shape returns PCCX_ERR_ARG with a message
    naming the entry point; an empty batch returns PCCX_OK whatever the pointers."""
    lib = _lib.load()
    sig = _lib.signatures()
    for name in NEW_SYMBOLS:
        assert name in sig and hasattr(lib, name), name
    p = 4096                                                 # any non-null value: the shape checks come before a pointer is used
    cases = {
        "pccx_minmax_n": dict(empty=(None, 0, 16, None, None, None), null=(None, 1, 16, p, p, None), shape=(p, 1, 0, p, p, None)),
        "pccx_query_rep_n": dict(empty=(None, 0, 16, None, None), null=(p, 1, 16, None, None), shape=(p, 65536, 16, p, None)),
        "pccx_estimate_normals_n": dict(empty=(None, 0, 16, None, None, 3, None, None), null=(p, 1, 16, None, p, 3, p, None),
                                        shape=(p, 1, 16, p, p, 0, p, None)),
        "pccx_point_errors_n": dict(empty=(None, 0, 16, None, None, None, 16, None, None, None, None),
                                    null=(p, 1, 16, p, p, None, 16, p, None, None, None), shape=(p, 1, 16, p, p, None, 0, p, p, None, None)),
        "pccx_mean_var_n": dict(empty=(None, 0, 16, None, None, None), null=(p, 1, 16, p, None, None), shape=(p, 1, -1, p, p, None)),
    }
    for name, c in cases.items():
        fn = getattr(lib, name)
        assert fn(*c["empty"]) == 0, name
        for kind in ("null", "shape"):
            assert fn(*c[kind]) == -1 and name.encode() in lib.pccx_last_error(), (name, kind)
        assert b"null pointer" in (fn(*c["null"]), lib.pccx_last_error())[1], name
    # normals and the plane output come together
    assert lib.pccx_point_errors_n(p, 1, 16, p, p, p, 16, p, p, None, None) == -1 and b"come together" in lib.pccx_last_error()
    assert lib.pccx_query_rep_n(None, 3, 0, None, None) == 0
