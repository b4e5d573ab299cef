"""Duplicate patches (csrc/patch_groups.hip): the grouping itself against a numpy restatement, and every consumer of the lists --
kNN patching, the in-patch neighbour tables + fused f16x2 encoder, the f16x2 decoder, Codec.compress / decompress -- bit-identical
(torch.equal) to the ungrouped computation.  A patch's result must not depend on which workgroup or tile slot computed it."""
import numpy as np
import pytest
import torch

from oracle import ref_model
from pccx import codec, models, ops, synth as cloud_synth
from tests import synth

K, k, d, L = synth.MODEL_CFG


def groups_numpy(keys, B, S):
    """rep / uniq as the header states them: rows compared as uint32 words, inside one cloud only."""
    u = np.ascontiguousarray(keys, dtype=np.float32).view(np.uint32).reshape(B * S, -1)
    rep = np.empty(B * S, np.int32)
    for b in range(B):
        first = {}
        for i in range(S):
            p = b * S + i
            rep[p] = first.setdefault(u[p].tobytes(), p)
    return rep, np.nonzero(rep == np.arange(B * S))[0].astype(np.int32)


def planted_keys(rng, B, S, f):
    """Random rows, each replaced with probability 1/2 by a copy of a random EARLIER-OR-LATER row of any cloud (so equal rows occur inside
    a cloud and across clouds), some entries +0 / -0."""
    keys = rng.standard_normal((B * S, f)).astype(np.float32)
    keys[rng.random((B * S, f)) < 0.2] = 0.0
    keys[rng.random((B * S, f)) < 0.1] = -0.0
    pool = keys[rng.integers(0, B * S, size=max(1, min(8, B * S)))].copy()       # a few rows that many patches of every cloud share
    take = rng.random(B * S) < 0.5
    keys[take] = pool[rng.integers(0, len(pool), size=int(take.sum()))]
    return keys.reshape(B, S, f)


def test_numpy_restatement_semantics():
    """CPU: the restatement the GPU test compares against does what the header says (smallest equal row of the SAME cloud; -0 != +0)."""
    keys = np.array([[[1, 2], [0.0, 5], [1, 2], [-0.0, 5], [0.0, 5]],
                     [[1, 2], [1, 2], [3, 4], [0.0, 5], [3, 4]]], np.float32)
    rep, uniq = groups_numpy(keys, 2, 5)
    assert rep.tolist() == [0, 1, 0, 3, 1, 5, 5, 7, 8, 7]
    assert uniq.tolist() == [0, 1, 3, 5, 7, 8]


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 8, 64, 100, 1024])
@pytest.mark.parametrize("fa,fb", [(3, 0), (3, 16), (1, 0)])
def test_groups_match_numpy(S, fa, fb):
    rng = np.random.default_rng(1000 * S + 10 * fa + fb)
    for B in (1, 5, 37):
        keys = planted_keys(rng, B, S, fa + fb)
        if B > 1 and S > 1:
            keys[1, 0] = keys[0, 0]                                                # equal rows in different clouds must not merge
            keys[1, S - 1] = keys[0, 0]
        a = torch.from_numpy(np.ascontiguousarray(keys[..., :fa])).cuda()
        b_ = torch.from_numpy(np.ascontiguousarray(keys[..., fa:])).cuda() if fb else None
        g = ops.patch_groups(a, b_)
        rep, uniq = groups_numpy(keys, B, S)
        n = int(g.n_uniq.item())
        assert n == len(uniq)
        assert np.array_equal(g.rep.cpu().numpy(), rep)
        assert np.array_equal(g.uniq[:n].cpu().numpy(), uniq)
        if B > 1 and S > 1:
            assert rep[S] == S and rep[2 * S - 1] == S


@pytest.fixture(scope="module")
def nets():
    ae = models.AE(K, k, d, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    prob = models.ConditionalProbabilityModel(L, d)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    return ae.pack("cuda"), prob.pack("cuda")


def _centres(kind, B, S, pcn, ae, prob):
    rng = np.random.default_rng(7)
    if kind == "reference":                    # what Codec.compress really feeds the transforms: the bug-compatible octree decode
        cd = codec.Codec(ae, prob, K=K, octree_mode="reference", matmul="f16x2")
        comp = cd.compress(pcn, np.arange(B) * 17 % pcn.shape[1], keep_extras=True)
        return comp.extras["rec_sampled"].contiguous()
    if kind == "distinct":
        return torch.from_numpy(rng.random((B, S, 3), dtype=np.float32)).cuda()
    if kind == "equal":
        return torch.from_numpy(np.tile(rng.random((B, 1, 3), dtype=np.float32), (1, S, 1))).cuda()
    raise ValueError(kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["reference", "distinct", "equal"])
@pytest.mark.parametrize("B", [3, 37])
def test_consumers_grouped_equal_ungrouped(nets, kind, B):
    """kNN patches of the representatives, all P rows of latent_raw / latent / latent_q, and the decoder's (B, S*k, 3) output: grouped ==
    ungrouped, on reference-mode centres of real compress runs, all-distinct and all-equal centres; P = 192 and 2368 patches are multiples
    of neither the encoder's grid nor the decoder's 256-patch blocks."""
    ae, prob = nets
    S, N = 64, 8192
    pcn, center, longest = ops.normalize(torch.from_numpy(cloud_synth.cad_batch(21, B, N)).cuda())
    rec = _centres(kind, B, S, pcn, ae, prob)
    g = ops.patch_groups(rec)
    rep = g.rep.long()
    is_rep = rep == torch.arange(B * S, device="cuda")
    n = int(g.n_uniq.item())
    assert n == int(is_rep.sum())
    if kind == "reference":
        assert n <= 8 * B
    elif kind == "distinct":
        assert n == B * S
    else:
        assert n == B

    full = ops.knn_points(rec, pcn, K, patch_scale=2.0, return_dists=False, return_idx=False).knn.view(B * S, K, 3)
    part = ops.knn_points(rec, pcn, K, patch_scale=2.0, return_dists=False, return_idx=False, rep=g.rep).knn.view(B * S, K, 3)
    assert torch.equal(part[is_rep], full[is_rep])
    assert torch.equal(full[rep], full)                       # the premise: a duplicate's patch IS its representative's patch

    want = ae.encode(full, sa_matmul="f16x2", pn_matmul="f16x2")
    # the grouped run reads the representatives' rows only: poison the others
    poisoned = torch.where(is_rep[:, None, None], part, torch.full_like(part, float("nan")))
    got = ae.encode(poisoned, sa_matmul="f16x2", pn_matmul="f16x2", groups=g)
    for w, x in zip(want, got):
        assert torch.equal(w, x)
    # a mode that does not take the list computes everything and is completed by the copy all the same
    want_b3 = ae.encode(full, sa_matmul="bf16x3", pn_matmul="bf16x3")
    got_b3 = ae.encode(full, sa_matmul="bf16x3", pn_matmul="bf16x3", groups=g)
    for w, x in zip(want_b3, got_b3):
        assert torch.equal(w, x)

    q = want[2]
    kw = dict(S=S, scale=2.0, margin=0.01)
    for matmul in ("f16x2", "bf16x3"):
        plain = ae.decode(q, rec.view(-1, 3), center, longest, matmul=matmul, **kw)
        grouped = ae.decode(q, rec.view(-1, 3), center, longest, matmul=matmul, group=True, **kw)
        assert torch.equal(plain, grouped)
    # equal centres, different latents: those patches are NOT duplicates for the decoder
    q2 = q.clone()
    q2[::3] += 1.0
    assert torch.equal(ae.decode(q2, rec.view(-1, 3), center, longest, matmul="f16x2", **kw),
                       ae.decode(q2, rec.view(-1, 3), center, longest, matmul="f16x2", group=True, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["reference", "full"])
@pytest.mark.parametrize("matmul", ["f16x2", "bf16x3"])
def test_codec_grouped_equal_ungrouped(nets, mode, matmul):
    """Codec.compress + decompress with and without grouping: the packed stream buffer, the reconstruction and every array of extras."""
    ae, prob = nets
    B = 5
    clouds = torch.from_numpy(cloud_synth.cad_batch(31, B, 8192) * np.float32(1.7) + np.float32(0.3)).cuda()
    starts = np.array([0, 11, 4000, 8191, 77])
    res = {}
    for grp in (False, True):
        cd = codec.Codec(ae, prob, K=K, octree_mode=mode, matmul=matmul, group_duplicates=grp)
        comp = cd.compress(clouds, starts)
        compx = cd.compress(clouds, starts, keep_extras=True)
        res[grp] = (comp, cd.decompress(comp), compx, compx.extras, cd.decompress(compx))
    a, b = res[False], res[True]
    for i in (0, 2):                                          # the three files of every cloud, byte for byte
        ca, cb = a[i], b[i]
        assert torch.equal(ca.s_nbytes, cb.s_nbytes) and torch.equal(ca.p_nbytes, cb.p_nbytes) and torch.equal(ca.c, cb.c)
        assert all(ca.files(j) == cb.files(j) for j in range(B))
    assert all(a[0].files(j) == a[2].files(j) for j in range(B))
    assert torch.equal(a[1], b[1]) and torch.equal(a[4], b[4]) and torch.equal(a[1], a[4])
    for name in ("pcn", "fps_idx", "sampled", "rec_sampled", "patches", "latent_raw", "latent", "latent_q", "cdf_int", "knn_idx"):
        assert torch.equal(a[3][name], b[3][name]), name
    for name in ("nbits", "depth", "nbytes"):
        assert torch.equal(a[3]["octree"][name], b[3]["octree"][name]), name
