"""CPU: the host side of ragged batches (Codec.compress_ragged / decompress_ragged) -- the shape arithmetic against hand values,
pad_clouds, and every refusal: raised with the limit and the way out in its message before anything is launched."""
import numpy as np
import pytest
import torch

from pccx import _lib, codec, models


def test_shape_arithmetic():
    p = codec.ragged_plan([2048, 1536, 1300, 544, 64, 1056, 2047], K=64, ALPHA=2, N0=1024, d=8)
    assert p.S == [64, 48, 40, 17, 2, 33, 63] and p.S_pad == 64
    assert p.s_stride == (1 + 8 * 64 * 16 + 7) // 8 == 1025 and p.p_cap == 2 * 64 * 8 + 16
    # the patch scales: the expressions of Codec.compress (N / N0) and Codec.decompress (S*k / N0), to the last bit of the double
    assert p.scale_compress[0] == float(2.0 ** (1 / 3)) and p.scale_decompress[0] == float(2.0 ** (1 / 3))
    assert p.scale_compress[2] == float((1300 / 1024) ** (1 / 3)) and p.scale_decompress[2] == float((40 * 32 / 1024) ** (1 / 3))
    assert p.scale_compress[2] != p.scale_decompress[2]            # 1300 points, 40 patches of 32: 1280 points come back
    assert p.scale_compress[4] == float((64 / 1024) ** (1 / 3)) == float(0.0625 ** (1 / 3))
    assert codec.ragged_plan([1300, 544, 64], 64).S_pad == 48      # S_pad != max S_b
    assert codec.ragged_plan([8193, 12000, 300], 256).S == [64, 93, 2] and codec.ragged_plan([8193, 12000, 300], 256).S_pad == 96
    q = codec.ragged_plan([32768, 32767, 128], 128, d=16)
    assert q.S == [512, 511, 2] and q.S_pad == 512 and q.p_cap == 2 * 512 * 16 + 16 and q.s_stride == 8193
    assert codec.ragged_plan([64], 64).S_pad == 16                 # never below one tile of the fused probability kernel


def test_pad_clouds():
    a, b = np.arange(15, dtype=np.float64).reshape(5, 3), torch.ones(2, 3)
    pc, n = codec.pad_clouds([a, b])
    assert n == [5, 2] and pc.shape == (2, 5, 3) and pc.dtype == torch.float32
    assert torch.equal(pc[0], torch.from_numpy(a.astype(np.float32))) and torch.equal(pc[1, :2], b)
    assert bool(torch.isnan(pc[1, 2:]).all())
    for bad in ([], [np.zeros((0, 3))], [np.zeros((4, 2))], [np.zeros(3)]):
        with pytest.raises(ValueError, match="pad_clouds"):
            codec.pad_clouds(bad)


def _codec(K=64, d=8, L=5, **kw):
    kw.setdefault("octree_mode", "full")
    return codec.Codec(models.AE(K, K // 2, d, L), models.ConditionalProbabilityModel(L, d), K=K, **kw)


REFUSALS = [
    (dict(octree_mode="reference"), [2048], r"octree_mode='full'.*'reference'"),
    (dict(p_split=4), [2048], "p_split, p_index and centres='blocks'"),
    (dict(p_index=4), [2048], "p_split, p_index and centres='blocks'"),
    (dict(centres="blocks"), [2048], "p_split, p_index and centres='blocks'"),
    (dict(knn_search="grid"), [2048], "knn_search='grid'"),
    (dict(group_duplicates=False), [2048], "group_duplicates=True"),
    (dict(d=32), [2048], r"fused probability kernel \(d <= 16, L <= 15, d\*L <= 128\), got d=32"),
    (dict(), [40000], "KNN_BRUTE_MAX_N = 32768 points, got N_max=40000"),
    (dict(), [2048, 63], r"cloud 1: 63 points.*K = 64 <= n_b"),
    (dict(K=32, d=8), [2048, 32768], r"cloud 1: S=2048 patches.*2 <= S_b <= 1024 at K=32.*OCTREE_MAX_S = 1024"),
]


def test_patch_range_is_the_one_rule_of_both_sides():
    """ragged_patch_range in patches says what ragged_refusal says in points, so that a decoder, which sees S_b alone, routes a file
    the way the encoder did.  Hand values; then every n around the limits also at a K where 32768*ALPHA // K is no multiple of 16."""
    assert _codec(K=64).ragged_patch_range() == (2, 1024)            # 1024 patches = 32768 points: both limits at once
    assert _codec(K=256, d=16, L=7).ragged_patch_range() == (2, 256)    # 32768 points; 32769..32895 share S = 256, a multiple of 16
    assert _codec(K=128, d=16, L=7).ragged_patch_range() == (2, 512)
    cd = _codec(K=80)                                                # 65536 // 80 = 819, shared by n = 32760..32799: left out
    assert cd.ragged_patch_range() == (2, 818)
    for cd in (_codec(K=80), _codec(K=64), _codec(K=256, d=16, L=7)):
        for n in list(range(1, 3 * cd.K)) + list(range(32768 - 3 * cd.K, 32768 + 3 * cd.K)):
            S = n * 2 // cd.K
            enc, dec = cd.ragged_refusal([n]) is None, cd.ragged_decode_refusal([S]) is None
            assert enc == dec or (S % 16 == 0 and S >= 16 and dec), (cd.K, n, S)   # S % 16 == 0: the same tables either way
    assert "S=1 patches" in cd.ragged_decode_refusal([64, 1]) and "one size per call" in cd.ragged_decode_refusal([300])
    assert _codec(p_split=4).ragged_decode_refusal([64]) == _codec(p_split=4).ragged_config_refusal() is not None


@pytest.mark.parametrize("kw,sizes,msg", REFUSALS)
def test_refused_before_any_launch(monkeypatch, kw, sizes, msg):
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    cd = _codec(**kw)
    pc = torch.empty(len(sizes), max(sizes), 3, device="meta")
    with pytest.raises(ValueError, match=msg) as e:
        cd.compress_ragged(pc, sizes, [0] * len(sizes))
    assert "one size per call" in str(e.value)                     # the way out: the one-cloud path
    assert calls == []


def test_decompress_refusals_before_any_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    comp = codec.Compressed.alloc(2, 1025, 2064, 0, "cpu")
    with pytest.raises(ValueError, match="octree_mode='full'"):
        _codec(octree_mode="reference").decompress_ragged(comp, [64, 64])
    with pytest.raises(ValueError, match=r"cloud 1: S=1025 patches.*2 <= S_b <= 1024"):
        _codec().decompress_ragged(comp, [64, 1025])
    with pytest.raises(_lib.PccxError, match=r"clouds \[0\] have S=\[0\]"):
        _codec().decompress_ragged(comp, [0, 64])
    with pytest.raises(ValueError, match="3 patch counts for 2 clouds"):
        _codec().decompress_ragged(comp, [64, 64, 64])
    with pytest.raises(ValueError, match="1 point counts for 2 clouds"):
        _codec().compress_ragged(torch.empty(2, 64, 3, device="meta"), [64], [0, 0])
    assert calls == []
