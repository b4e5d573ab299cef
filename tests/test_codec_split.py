"""GPU: Codec(p_split=G) -- the split form of .p.bin (segments of G patches, include/pccx.h) through compress / decompress / the
file layer, against Codec(p_split=None) on the same clouds and against the oracle's coder segment by segment."""
import struct

import numpy as np
import pytest
import torch

from oracle import cport, ref_model
from pccx import codec, models, synth as cloud_synth
from tests import synth

pytestmark = pytest.mark.gpu

K, _k, D, L = synth.MODEL_CFG            # 256, 128, 16, 7
B, N = 2, 2048                           # S = 16 patches, 256 symbols per cloud
S = N * 2 // K
STARTS = np.array([5, 1234])


@pytest.fixture(scope="module")
def nets():
    ae = models.AE(K, K // 2, D, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    prob = models.ConditionalProbabilityModel(L, D)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    return ae.pack("cuda"), prob.pack("cuda")


@pytest.fixture(scope="module")
def plain(nets):
    """The unsplit codec on the small batch: (clouds, Compressed with extras, reconstruction)."""
    pc = torch.from_numpy(cloud_synth.cad_batch(41, B, N)).cuda()
    cd = codec.Codec(*nets, K=K, octree_mode="full")
    comp = cd.compress(pc, STARTS, keep_extras=True)
    return pc, comp, cd.decompress(comp, S=S)


def _want_p(cdf, q, seg_sym):
    sym = (q.astype(np.int64) + L // 2).astype(np.int16)
    segs = [cport.range_encode(np.ascontiguousarray(cdf[i:i + seg_sym]), sym[i:i + seg_sym]) for i in range(0, len(sym), seg_sym)]
    return b"PXS1" + struct.pack("<IHH", len(sym), seg_sym, 0) + np.array([len(s) for s in segs], dtype="<u2").tobytes() + b"".join(segs)


@pytest.mark.parametrize("G", [4, 5])
def test_small_batch_against_the_unsplit_codec_and_the_oracle_segments(nets, plain, tmp_path, G):
    pc, comp0, out0 = plain
    assert S == 16 and -(-S // G) == 4
    cd = codec.Codec(*nets, K=K, octree_mode="full", p_split=G)
    comp = cd.compress(pc, STARTS, keep_extras=True)
    assert comp.p_bytes.shape[1] == models.split_cap(S * D, G * D)
    assert torch.equal(comp.extras["latent_q"], comp0.extras["latent_q"]) and torch.equal(comp.extras["cdf_int"], comp0.extras["cdf_int"])
    cdf = comp.extras["cdf_int"].cpu().numpy().reshape(B, S * D, L + 1)
    q = comp.extras["latent_q"].cpu().numpy().reshape(B, S * D)
    for b in range(B):
        s, p, c = comp.files(b)
        s0, p0, c0 = comp0.files(b)
        assert s == s0 and c == c0
        assert p == _want_p(cdf[b], q[b], G * D), f"cloud {b}: .p.bin is not header + the oracle's segments"
        assert p0 == cport.range_encode(cdf[b], (q[b].astype(np.int64) + L // 2).astype(np.int16))       # and the default stays one stream
        # bits() / bpp() count the header with the file
        assert int(comp.bits()[b]) == 8 * (len(s) + len(p) + 16)
        assert float(comp.bpp()[b]) - float(comp0.bpp()[b]) == pytest.approx(8 * (len(p) - len(p0)) / N, abs=1e-12)
        assert len(p) >= 12 + 2 * 4
    assert torch.equal(cd.decompress(comp, S=S), out0)
    assert torch.equal(cd.decompress(comp, S=S, reuse_cdf=True), out0)
    # files: write -> read -> decompress
    names = [f"c{b}.ply" for b in range(B)]
    comp.write_files(str(tmp_path), names)
    for b, n in enumerate(names):
        assert open(tmp_path / (n + ".p.bin"), "rb").read() == comp.files(b)[1]
    back = codec.Compressed.read_files(str(tmp_path), names, n_points=N, device="cuda")
    assert torch.equal(cd.decompress(back, S=S), out0)
    # the other side must agree on p_split: another G, and the unsplit stream, are refused by the header check
    with pytest.raises(models._lib.PccxError, match="clouds"):
        codec.Codec(*nets, K=K, octree_mode="full", p_split=G + 2).decompress(back, S=S)
    with pytest.raises(models._lib.PccxError, match="clouds"):
        cd.decompress(comp0, S=S)


def test_wide_path_139264_points_17_segments(nets):
    n = 139264
    s_ = n * 2 // K
    assert s_ == 1088 > codec.OCTREE_MAX_S and -(-s_ // 64) == 17
    pc = torch.from_numpy(cloud_synth.cad_batch(43, 1, n)).cuda()
    start = np.array([7])
    cd0 = codec.Codec(*nets, K=K, octree_mode="full", max_centres=8192)
    cd = codec.Codec(*nets, K=K, octree_mode="full", max_centres=8192, p_split=64)
    comp0, comp = cd0.compress(pc, start), cd.compress(pc, start)
    out0 = cd0.decompress(comp0, S=s_)
    assert torch.equal(cd.decompress(comp, S=s_), out0)
    s, p, c = comp.files(0)
    assert (s, c) == (comp0.files(0)[0], comp0.files(0)[2]) and p[:12] == b"PXS1" + struct.pack("<IHH", s_ * D, 64 * D, 0)
    assert models.split_stream_status(p, s_ * D, 64 * D) == 0


def test_p_split_is_validated_in_the_constructor():
    ae = models.AE(K, K // 2, D, L)                     # unpacked: nothing here may reach a kernel
    prob = models.ConditionalProbabilityModel(L, D)
    g_max = models.split_max_seg_sym(L) // D
    assert g_max >= 128
    assert codec.Codec(ae, prob, K=K).p_split is None
    assert codec.Codec(ae, prob, K=K, p_split=g_max).p_split == g_max
    for bad in (0, True, g_max + 1, -1, 4.0, "4"):
        with pytest.raises(ValueError, match=rf"p_split must be None or an int in 1\.\.{g_max} "):
            codec.Codec(ae, prob, K=K, p_split=bad)
