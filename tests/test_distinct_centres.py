"""The duplicate-centre saving in the probability model, the kNN patching and the decoder head (csrc/prob.hip
pccx_prob_forward_distinct, csrc/knn.hip pccx_knn_uniq, csrc/decoder.hip dec_head_kernel<true>): every result torch.equal to the
untouched entry point on the same seeded inputs.  Outputs are pre-filled with a sentinel, so a row nobody wrote fails (NaN is not
equal to itself) and a row that must stay unwritten is seen to."""
import numpy as np
import pytest
import torch

from oracle import ref_model
from pccx import _lib, codec, models, ops, synth as cloud_synth
from tests import synth

K, k, d, L = synth.MODEL_CFG


def cloud_of(rng, S, n, rows=None):
    """(S, 3) centres with exactly n distinct rows, every one of them used, in an order unrelated to the rows' own."""
    rows = rng.random((n, 3), dtype=np.float32) if rows is None else rows
    pick = np.concatenate([rng.permutation(n), rng.integers(0, n, size=S - n)])
    return rows[rng.permutation(pick)]


def reference_like(rng, S):
    """What the reference decode produces: rows from {0.25, 0.75}^3, all eight of them, the tail repeating the last row."""
    corners = np.array([[x, y, z] for x in (0.25, 0.75) for y in (0.25, 0.75) for z in (0.25, 0.75)], np.float32)
    head = cloud_of(rng, S - S // 4, 8, corners)
    return np.concatenate([head, np.tile(head[-1], (S // 4, 1))])


def signed_zero(rng, S):
    """Eight distinct rows, two of which differ in the sign of a zero only: different keys, as patch_groups compares them."""
    rows = rng.random((8, 3), dtype=np.float32)
    rows[3] = rows[5]
    rows[3, 1], rows[5, 1] = 0.0, -0.0
    return cloud_of(rng, S, 8, rows)


def prob_clouds(S, counts):
    rng = np.random.default_rng(100 + S)
    out = []
    for n in counts:
        out.append(reference_like(rng, S) if n == "ref8" else signed_zero(rng, S) if n == "zero8" else cloud_of(rng, S, n))
    return torch.from_numpy(np.stack(out))


@pytest.fixture(scope="module")
def prob():
    m = models.ConditionalProbabilityModel(7, 16)
    m.load_state_dict(ref_model.seeded_state_dict(m, synth.PROB_SEED, gain=synth.PROB_GAIN))
    return m.pack("cuda")


def _prob_call(fn, prob, x):
    B, S, _ = x.shape
    out = (torch.full((B, S, prob.d, prob.L), float("nan"), device="cuda"),
           torch.full((B, S, prob.d, prob.L + 1), float("nan"), device="cuda"),
           torch.full((B, S, prob.d, prob.L + 1), -1, device="cuda", dtype=torch.int32))
    _lib.call(fn, x.data_ptr(), B, S, prob.d, prob.L, prob._blob.data_ptr(), *(t.data_ptr() for t in out), ops._stream())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("S,counts", [(64, [1, "ref8", 16, 17, 64, "zero8"]),      # B % 4 = 2: a partly filled workgroup; 17 = two tiles
                                      (16, [1, 8, 16, 5, 16]),                      # in one wave beside one-tile waves
                                      (32, [1, 8, 17, 32, 16])])
def test_prob_distinct_equals_prob_forward(prob, S, counts):
    x = prob_clouds(S, counts).cuda()
    want = _prob_call("pccx_prob_forward", prob, x)
    got = _prob_call("pccx_prob_forward_distinct", prob, x)
    again = _prob_call("pccx_prob_forward_distinct", prob, x)
    for name, w, g, a in zip(("pmf", "cdf", "cdf_int"), want, got, again):
        assert not torch.isnan(w.float()).any() and (name != "cdf_int" or (w >= 0).all())
        assert torch.equal(w, g), name
        assert torch.equal(g, a), name
    # each output alone (all three are optional), through the host layer's switch
    for name, w in zip(("pmf", "cdf", "cdf_int"), want):
        assert torch.equal(prob.run(x, (name,), distinct=True)[name], w), name


def test_prob_distinct_falls_back(monkeypatch):
    """CPU: distinct=True outside the kernel's shapes takes the usual paths -- S > 64 the plain fused kernel, shapes the fused kernel
    does not cover the generic layers."""
    calls = []
    monkeypatch.setattr(models, "_f32c", lambda t, name: t)
    monkeypatch.setattr(models, "_stream", lambda: 0)
    monkeypatch.setattr(models._lib, "call", lambda name, *a: calls.append(name))
    m = models.ConditionalProbabilityModel(7, 16)
    m._blob = torch.zeros(1)
    m.run(torch.zeros(2, 128, 3), ("cdf_int",), distinct=True)
    m.run(torch.zeros(2, 64, 3), ("cdf_int",), distinct=True)
    m.run(torch.zeros(2, 64, 3), ("cdf_int",))
    assert calls == ["pccx_prob_forward", "pccx_prob_forward_distinct", "pccx_prob_forward"]
    wide = models.ConditionalProbabilityModel(20, 16)                         # L > 15: not fused
    assert not wide.fused_ok(64)
    monkeypatch.setattr(wide, "_run_generic", lambda x, want: "generic")
    assert wide.run(torch.zeros(2, 64, 3), ("cdf_int",), distinct=True) == "generic"
    monkeypatch.setattr(m, "_run_generic", lambda x, want: "generic")
    assert m.run(torch.zeros(2, 40, 3), ("cdf_int",), distinct=True) == "generic"      # S % 16 != 0


def _knn_call(fn, q, ref, K_, lists):
    B, M, _ = q.shape
    out = (torch.full((B, M, K_), float("nan"), device="cuda"), torch.full((B, M, K_), -7, device="cuda", dtype=torch.int64),
           torch.full((B, M, K_, 3), float("nan"), device="cuda"))
    _lib.call(fn, q.data_ptr(), B, M, ref.data_ptr(), ref.shape[1], K_, *(t.data_ptr() for t in out), 1.5, *lists, ops._stream())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("B,M,N,K_,distinct", [(3, 64, 8192, 256, 8), (3, 64, 300, 100, 8),     # N = 300: the i < N mask
                                               (64, 64, 1024, 16, 64)])                          # 4096 entries: every workgroup loops
def test_knn_uniq_equals_knn(B, M, N, K_, distinct):
    rng = np.random.default_rng(N + K_)
    ref = torch.from_numpy(rng.random((B, N, 3), dtype=np.float32)).cuda()
    q = torch.from_numpy(np.stack([cloud_of(rng, M, distinct) for _ in range(B)])).cuda()
    g = ops.patch_groups(q)
    is_rep = (g.rep.long() == torch.arange(B * M, device="cuda")).view(B, M)
    assert int(g.n_uniq.item()) == B * distinct
    want = _knn_call("pccx_knn", q, ref, K_, ())
    got = _knn_call("pccx_knn_uniq", q, ref, K_, (g.uniq.data_ptr(), g.n_uniq.data_ptr()))
    fresh = _knn_call("pccx_knn_uniq", q, ref, K_, (None, None))              # null lists: launched as pccx_knn is
    for name, w, x, f in zip(("dists", "idx", "nn"), want, got, fresh):
        assert torch.equal(w, f), name
        assert torch.equal(x[is_rep], w[is_rep]), name
        rest = x[~is_rep]
        assert bool(torch.isnan(rest).all() if rest.is_floating_point() else (rest == -7).all()), name + ": a duplicate's row was written"
    via_ops = ops.knn_points(q, ref, K_, patch_scale=1.5, groups=g)
    for w, x in zip(want, via_ops):
        assert torch.equal(x[is_rep], w[is_rep])


@pytest.fixture(scope="module")
def ae():
    m = models.AE(K, k, d, L)
    m.load_state_dict(ref_model.seeded_state_dict(m, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    return m.pack("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("matmul", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("n_uniq", [1, 15, 16, 17, 100])
def test_decoder_head_grouped_equals_ungrouped(ae, matmul, n_uniq):
    """One cloud of P = 128 patches with n_uniq distinct (centre, latent) pairs: less than a tile, a tile, a tile and one, seven tiles."""
    P = 128
    rng = np.random.default_rng(n_uniq)
    rows = np.concatenate([rng.random((n_uniq, 3), dtype=np.float32),
                           rng.integers(-(L // 2), L // 2 + 1, size=(n_uniq, d)).astype(np.float32)], axis=1)
    rows = cloud_of(rng, P, n_uniq, rows)
    centres, q = torch.from_numpy(rows[:, :3].copy()).cuda(), torch.from_numpy(rows[:, 3:].copy()).cuda()
    assert int(ops.patch_groups(centres.view(1, P, 3), q.view(1, P, d)).n_uniq.item()) == n_uniq
    center, longest = torch.tensor([[0.1, 0.2, 0.3]], device="cuda"), torch.tensor([1.3], device="cuda")
    kw = dict(S=P, scale=2.0, margin=0.01, matmul=matmul)
    plain = ae.decode(q, centres, center, longest, **kw)
    grouped = ae.decode(q, centres, center, longest, group=True, **kw)
    assert torch.equal(plain, grouped)
    per_tile = ae.decode(q, centres, center, longest, group=True, short_list=True, **kw)      # the head's one-tile-per-workgroup form
    assert torch.equal(plain, per_tile)


@pytest.mark.gpu
def test_codec_reference_mode_grouped_equals_ungrouped(ae, prob):
    """The three paths together: Codec in reference mode, three clouds of 8192 points, grouped against ungrouped.  The packed buffer is
    allocated uninitialised and the coders write only the bytes they count, so it is compared section by section with the stream
    bytes past each cloud's count masked out -- every byte that is defined."""
    B = 3
    clouds = torch.from_numpy(cloud_synth.cad_batch(41, B, 8192)).cuda()
    starts = np.array([5, 4000, 8191])
    res = {}
    for grp in (False, True):
        cd = codec.Codec(ae, prob, K=K, octree_mode="reference", matmul="f16x2", group_duplicates=grp)
        comp = cd.compress(clouds, starts)
        res[grp] = (comp, cd.decompress(comp))
    (ca, ra), (cb, rb) = res[False], res[True]
    assert torch.equal(ra, rb)
    assert torch.equal(ca.s_nbytes, cb.s_nbytes) and torch.equal(ca.p_nbytes, cb.p_nbytes) and torch.equal(ca.c, cb.c)
    assert (ca.p_nbytes > 0).all()
    for xa, xb, nb in ((ca.s_bytes, cb.s_bytes, ca.s_nbytes), (ca.p_bytes, cb.p_bytes, ca.p_nbytes)):
        live = torch.arange(xa.shape[1], device="cuda")[None, :] < nb[:, None]
        assert torch.equal(xa * live, xb * live)
