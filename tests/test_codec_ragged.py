"""GPU: ragged batches -- Codec.compress_ragged / decompress_ragged take clouds of different sizes in one launch sequence
(octree_mode "full"; csrc: pccx_normalize_n, pccx_fps_n, pccx_octree_encode_n, pccx_knn_list_n, pccx_range_encode_n /
pccx_range_decode_n, pccx_reassemble_n).

The contract: a cloud's streams and points do not depend on the batch it travels in; they are the one-cloud
path's wherever that path runs the fused probability kernel (S_b a multiple of 16); for every other S_b everything but the
probability table is the one-cloud path's, and the table is rows [0, S_b) of the fused kernel's table on the centres padded to a
multiple of 16 with repeats of the last one.  Every comparison is torch.equal or byte equality; padding rows are NaN throughout.

| batch | K   | what it hits                                                        |
| A     | 64  | S a multiple of 16 and not, S < 16, n_b = K                          |
| A'    | 64  | S_pad != max S_b                                                     |
| B     | 256 | the fast kNN kernel's last N (8192)                                  |
| C     | 256 | the radix-select kNN kernel                                          |
| D     | 128 | the largest N (32768: FPS from global memory, the one-lane coders)   |
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cport, ref_model
from pccx import _lib, codec, models, ops, synth as cloud_synth

pytestmark = pytest.mark.gpu

BATCHES = {
    "A": (64, [2048, 1536, 1300, 544, 64, 1056, 2047]),
    "A'": (64, [1300, 544, 64]),
    "B": (256, [8192, 5000, 8191, 256]),
    "C": (256, [8193, 12000, 300]),
    "D": (128, [32768, 32767, 128]),
}
EXPECT_S = {"A": ([64, 48, 40, 17, 2, 33, 63], 64), "A'": ([40, 17, 2], 48), "B": ([64, 39, 63, 2], 64), "C": ([64, 93, 2], 96),
            "D": ([512, 511, 2], 512)}
DL = {64: (8, 5), 256: (16, 7), 128: (16, 7)}


@functools.lru_cache(maxsize=None)
def _nets(K):
    d, L = DL[K]
    ae = models.AE(K, K // 2, d, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, 3, last_gain={"pn.mlp_Modules.3.0": 40.0}))
    prob = models.ConditionalProbabilityModel(L, d)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, 4, gain=2.0))
    return ae.pack("cuda"), prob.pack("cuda")


@functools.lru_cache(maxsize=None)
def _cloud(n):
    """One seeded cloud per size: the same cloud wherever that size appears, so A, A' and the lone batches share their references."""
    return cloud_synth.cad_cloud(7000 + n, n)


def _start(n):
    return n // 3


def _codec(K, matmul="f16x2", **kw):
    return codec.Codec(*_nets(K), K=K, octree_mode="full", matmul=matmul, **kw)


@functools.lru_cache(maxsize=None)
def _solo(K, n, matmul="f16x2"):
    """The one-cloud path on the unpadded cloud: (Compressed with extras, its files, its decompressed points).  Computed once."""
    cd = _codec(K, matmul)
    comp = cd.compress(torch.from_numpy(_cloud(n)[None]).cuda(), [_start(n)], keep_extras=True)
    return comp, comp.files(0), cd.decompress(comp, S=n * 2 // K)[0]


@functools.lru_cache(maxsize=None)
def _ragged(name, matmul="f16x2", order=None):
    """A batch through the ragged path: (sizes, Compressed with extras, list of decompressed clouds).  Computed once."""
    K, sizes = BATCHES[name]
    sizes = list(sizes) if order is None else [sizes[i] for i in order]
    pc, n = codec.pad_clouds([_cloud(v) for v in sizes], device="cuda")
    assert n == sizes and bool(torch.isnan(pc).any()) == (len(set(sizes)) > 1)
    cd = _codec(K, matmul)
    comp = cd.compress_ragged(pc, n, [_start(v) for v in sizes], keep_extras=True)
    return sizes, comp, cd.decompress_ragged(comp, comp.extras["S"])


def test_shapes_of_the_batches():
    for name, (K, sizes) in BATCHES.items():
        plan = codec.ragged_plan(sizes, K, 2, 1024, DL[K][0])
        assert (plan.S, plan.S_pad) == EXPECT_S[name]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_stage_pins(name):
    K, _ = BATCHES[name]
    d = DL[K][0]
    sizes, comp, _ = _ragged(name)
    ex, S_pad = comp.extras, EXPECT_S[name][1]
    for key in ("pcn", "sampled", "rec_sampled", "patches", "latent_q", "latent"):
        assert not bool(torch.isnan(ex[key]).any()), f"padding reached {key}"
    for b, n in enumerate(sizes):
        S = n * 2 // K
        one = _solo(K, n)[0]
        so = one.extras
        assert torch.equal(ex["pcn"][b, :n], so["pcn"][0]) and not bool(ex["pcn"][b, n:].any())
        assert torch.equal(comp.c[b], one.c[0])
        assert torch.equal(ex["fps_idx"][b, :S], so["fps_idx"][0])
        assert np.array_equal(ex["fps_idx"][b, :S].cpu().numpy(), cport.fps(so["pcn"][0].cpu().numpy(), S, _start(n)))
        assert bool((ex["fps_idx"][b, S:] == ex["fps_idx"][b, S - 1]).all())
        nb = int(ex["octree"]["nbytes"][b])
        assert nb == int(so["octree"]["nbytes"][0]) and int(ex["octree"]["depth"][b]) == int(so["octree"]["depth"][0])
        got = ex["octree"]["bytes"][b, :nb].cpu().numpy().tobytes()
        assert got == so["octree"]["bytes"][0, :nb].cpu().numpy().tobytes()
        want, wd = cport.encode_sampled(ex["sampled"][b, :S].cpu().numpy(), 1, n, ops.OCTREE_BPP_DICT[K])
        assert got == bytes(cport.pack_bits(want)) and wd == int(ex["octree"]["depth"][b])
        assert torch.equal(ex["rec_sampled"][b, :S], so["rec_sampled"][0])
        assert torch.equal(ex["patches"].view(len(sizes), S_pad, K, 3)[b, :S], so["patches"])
        assert torch.equal(ex["latent_q"].view(len(sizes), S_pad, d)[b, :S], so["latent_q"])


def _padded_table(K, s_bytes, s_nbytes, S):
    """The definition: rows [0, S) of the fused kernel's table on the cloud's own decoded centres padded to a multiple of 16."""
    rec, _ = ops.octree_decode(s_bytes, s_nbytes, "full", 16 * -(-S // 16))
    return _nets(K)[1].run(rec, ("cdf_int",))["cdf_int"][0, :S]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_streams(name):
    K, _ = BATCHES[name]
    d, L = DL[K]
    sizes, comp, _ = _ragged(name)
    ex, S_pad = comp.extras, EXPECT_S[name][1]
    for b, n in enumerate(sizes):
        S = n * 2 // K
        one, files, _ = _solo(K, n)
        s, p, c = comp.files(b)
        assert s == files[0] and c == files[2]
        if S % 16 == 0 and S >= 16:
            assert p == files[1]
            continue
        table = _padded_table(K, one.s_bytes, one.s_nbytes, S)
        assert torch.equal(ex["cdf_int"][b, :S], table)
        q = ex["latent_q"].view(len(sizes), S_pad * d)[b:b + 1, :S * d]
        out, nb = models.range_encode(table[None].contiguous(), q.contiguous(), L)
        assert p == out[0, :int(nb[0])].cpu().numpy().tobytes()


def test_batch_independence():
    K, _ = BATCHES["A"]
    sizes, comp, outs = _ragged("A")
    small_sizes, small, small_outs = _ragged("A'")
    order = tuple(reversed(range(len(sizes))))
    rev_sizes, rev, rev_outs = _ragged("A", order=order)
    assert small.s_bytes.shape[1] != comp.s_bytes.shape[1]              # another S_pad: other strides, the same bytes
    for j, n in enumerate(small_sizes):
        b = sizes.index(n)
        assert small.files(j) == comp.files(b) and torch.equal(small_outs[j], outs[b])
    for j, n in enumerate(rev_sizes):
        b = sizes.index(n)
        assert rev.files(j) == comp.files(b) and torch.equal(rev_outs[j], outs[b])
    cd = _codec(K)
    for n in small_sizes:                                               # alone, N_max = n_b: no padding row at all
        b = sizes.index(n)
        pc = torch.from_numpy(_cloud(n)[None]).cuda()
        lone = cd.compress_ragged(pc, [n], [_start(n)])
        assert lone.files(0) == comp.files(b)
        assert torch.equal(cd.decompress_ragged(lone, [n * 2 // K])[0], outs[b])


@pytest.mark.parametrize("name,matmul", [("A", "f16x2"), ("A'", "f16x2"), ("B", "f16x2"), ("C", "f16x2"), ("D", "f16x2"), ("A", "f32")])
def test_round_trip(name, matmul):
    """Both coders are lossless and the points are a function of (latent_q, centres, c, scale) only: every cloud comes back as the
    one-cloud path's reconstruction, for all S_b."""
    K, _ = BATCHES[name]
    d, L = DL[K]
    sizes, comp, outs = _ragged(name, matmul)
    ex, S_pad, B = comp.extras, EXPECT_S[name][1], len(sizes)
    q = models.range_decode_n(ex["cdf_int"], comp.p_bytes, comp.p_nbytes, [s * d for s in ex["S"]], L).view(B, S_pad, d)
    for b, n in enumerate(sizes):
        S = n * 2 // K
        assert torch.equal(q[b, :S], ex["latent_q"].view(B, S_pad, d)[b, :S]) and not bool(q[b, S:].any())
        assert outs[b].shape == (S * (K // 2), 3)
        assert torch.equal(outs[b], _solo(K, n, matmul)[2]), f"cloud {b} (n={n}, S={S})"
    assert outs[0].untyped_storage().data_ptr() == outs[-1].untyped_storage().data_ptr()       # views of one allocation
    assert torch.equal(comp.bpp().cpu(), (comp.bits().double() / torch.tensor(sizes, device="cuda")).cpu())


def test_from_files(tmp_path):
    K, _ = BATCHES["A"]
    sizes, comp, outs = _ragged("A")
    names = [f"cloud{n}" for n in sizes]
    total = comp.write_files(str(tmp_path), names)
    sn, pn = comp.s_nbytes.cpu().tolist(), comp.p_nbytes.cpu().tolist()
    assert total == sum(sn) + sum(pn) + 16 * len(sizes)
    for name, a, b_ in zip(names, sn, pn):
        assert (tmp_path / (name + ".s.bin")).stat().st_size == a and (tmp_path / (name + ".p.bin")).stat().st_size == b_
        assert (tmp_path / (name + ".c.bin")).stat().st_size == 16
    back = codec.Compressed.read_files(str(tmp_path), names, device="cuda")
    got = _codec(K).decompress_ragged(back, comp.extras["S"])
    for a, b_ in zip(got, outs):
        assert torch.equal(a, b_)


def test_wrong_S_names_the_cloud():
    K, _ = BATCHES["A'"]
    _, comp, _ = _ragged("A'")
    cd = _codec(K)
    S = list(comp.extras["S"])
    S[1] += 1
    with pytest.raises(_lib.PccxError, match=r"cloud 1: S=18 given but its \.s\.bin holds 17"):
        cd.decompress_ragged(comp, S)
    for bad in (0, -3):
        with pytest.raises(_lib.PccxError, match="clouds \\[2\\]"):
            cd.decompress_ragged(comp, S[:1] + [17, bad])


def test_truncated_stream_decodes_inside_its_row():
    """pccx_range_decode_n on foreign bytes is pccx_range_decode on the same row: nbytes cut to the row, bits past the stream zero."""
    K, _ = BATCHES["A"]
    d, L = DL[K]
    sizes, comp, _ = _ragged("A")
    ex, B = comp.extras, len(sizes)
    for nbytes in (comp.p_nbytes // 2, torch.zeros_like(comp.p_nbytes), torch.full_like(comp.p_nbytes, 1 << 30), -comp.p_nbytes):
        q = models.range_decode_n(ex["cdf_int"], comp.p_bytes, nbytes, [s * d for s in ex["S"]], L)
        for b, S in enumerate(ex["S"]):
            want = models.range_decode(ex["cdf_int"][b:b + 1, :S].contiguous(), comp.p_bytes[b:b + 1], nbytes[b:b + 1], L)
            assert torch.equal(q[b, :S * d], want[0]) and not bool(q[b, S * d:].any())
    cut = codec.Compressed(comp.s_bytes, comp.s_nbytes, comp.p_bytes, comp.p_nbytes // 2, comp.c, comp.n_points)
    for pts in _codec(K).decompress_ragged(cut, ex["S"]):
        assert bool(torch.isfinite(pts).all())


def test_padded_table_against_the_generic_layers(capsys):
    """A measurement, not a gate: where S_b is no multiple of 16 the one-cloud path evaluates the generic layers; how many entries of
    its table differ from the padded definition, and by how much, is printed (the figure is in DESIGN.md section 4.5).  Asserted: both
    tables are valid -- strictly increasing rows from 0, ending at 2^16."""
    total = differ = worst = 0
    for name in ("A", "B", "C"):
        K, _ = BATCHES[name]
        sizes, comp, _ = _ragged(name)
        for b, n in enumerate(sizes):
            S = n * 2 // K
            if S % 16 == 0:
                continue
            padded = comp.extras["cdf_int"][b, :S]
            generic = _solo(K, n)[0].extras["cdf_int"][0]
            for t in (padded, generic):
                # the tables hold 16-bit words as torchac's do: the closing 2^16 is stored as 65536 & 0xFFFF = 0 and read back as 2^16
                # by the coders, so "ending at 2^16" is a last word of 0 behind L strictly increasing ones that start at 0
                assert bool((t[..., 0] == 0).all()) and bool((t[..., -1] == 0).all())
                assert bool((t[..., 1:-1] > t[..., :-2]).all()) and bool((t[..., -2] < 65536).all())
            diff = (padded - generic).abs()
            total, differ, worst = total + diff.numel(), differ + int((diff != 0).sum()), max(worst, int(diff.max()))
    with capsys.disabled():
        print(f"\npadded fused table vs generic layers: {differ} of {total} entries differ, largest difference {worst}")
