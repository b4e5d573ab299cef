"""GPU: the tiled probability model (ConditionalProbabilityModel.run(tiles=True), pccx_prob_forward_tiled)
against the one-workgroup kernel of run(), which the reference's fixtures pin elsewhere: every output bit for bit, at every shape at
which the three launches take another path."""
import pytest
import torch

from oracle import ref_model
from pccx import _lib, models, ops, synth as cloud_synth
from tests import synth

pytestmark = pytest.mark.gpu

K, _k, D, L = synth.MODEL_CFG            # 256, 128, 16, 7
WANTS = [("pmf",), ("cdf",), ("cdf_int",), ("pmf", "cdf", "cdf_int")]


def _prob(d=D, l=L):
    prob = models.ConditionalProbabilityModel(l, d)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    return prob.pack("cuda")


@pytest.fixture(scope="module")
def prob():
    return _prob()


_CENTRES = {}


def centres(B, S):
    """(B,S,3) decoded patch centres of B different seeded clouds of S*K/2 points: normalise, FPS, octree coder, full-mode decode, as
    Codec.compress produces them.  Computed once per shape and left unchanged."""
    if (B, S) not in _CENTRES:
        N = S * K // 2
        pcn, _, _ = ops.normalize(torch.from_numpy(cloud_synth.cad_batch(50 + S % 37, B, N)).cuda())
        idx = ops.farthest_point_sample_batch(pcn, S, [3 + 11 * b for b in range(B)], workgroups="auto" if S > 1024 else None)
        oc = ops.octree_encode(ops.index_points(pcn, idx), N, ops.OCTREE_BPP_DICT[K])
        rec, _ = ops.octree_decode(oc["bytes"], oc["nbytes"], "full", S)
        if B > 1:
            assert not torch.equal(rec[0], rec[1]) and not torch.equal(rec[0], rec[B - 1])
        _CENTRES[B, S] = rec
    return _CENTRES[B, S]


def _bits(t):
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def _same(got, want, names, shape):
    assert sorted(got) == sorted(want) == sorted(names)
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape
        assert got[name].shape[:2] == shape
        assert torch.equal(_bits(got[name]), _bits(want[name])), name


# S = 16: one tile (three waves idle in pass 1, three clamped waves in pass 2); 48: three tiles; 80: two workgroups, the second with one
# tile; 1088: 68 tiles on 17 workgroups, nothing ragged; 4112: 257 tiles = 65 rounds over the cap of 64 workgroups
@pytest.mark.parametrize("S,B", [(16, 1), (16, 3), (48, 1), (80, 3), (1088, 1), (4112, 1)])
def test_tiles_equal_the_one_workgroup_kernel(prob, S, B):
    x = centres(B, S)
    for want in WANTS:
        _same(prob.run(x, want, tiles=True), prob.run(x, want), want, (B, S))
    # distinct is ignored under tiles: the outputs are the same by definition
    _same(prob.run(x, ("cdf_int",), distinct=True, tiles=True), prob.run(x, ("cdf_int",)), ("cdf_int",), (B, S))


@pytest.mark.parametrize("d,l", [(8, 15), (4, 5), (16, 8)])       # d*L = 120; a small d in the table stage's e / d; d*L = 128 exactly
def test_other_d_and_L(d, l):
    p, x = _prob(d, l), centres(1, 48)
    assert p.fused_ok(48)
    for want in WANTS:
        got = p.run(x, want, tiles=True)
        _same(got, p.run(x, want), want, (1, 48))
        assert all(got[n].shape[2:] == (d, l + (n != "pmf")) for n in want)


def test_shapes_outside_the_fused_kernel_take_the_generic_layers(prob):
    x = centres(1, 24)                                            # S % 16 != 0
    assert not prob.fused_ok(24)
    _same(prob.run(x, WANTS[3], tiles=True), prob.run(x, WANTS[3]), WANTS[3], (1, 24))
    p17, x = _prob(4, 17), centres(1, 48)                         # L above 15
    assert not p17.fused_ok(48)
    _same(p17.run(x, WANTS[3], tiles=True), p17.run(x, WANTS[3]), WANTS[3], (1, 48))


def test_two_calls_back_to_back_share_the_workspace(prob):
    a, b = centres(3, 80), centres(1, 16)
    want_a, want_b = prob.run(a, WANTS[3]), prob.run(b, WANTS[3])
    torch.cuda.synchronize()
    got_a = prob.run(a, WANTS[3], tiles=True)                     # the second call's launches reuse the first one's workspace
    got_b = prob.run(b, WANTS[3], tiles=True)
    got_a2 = prob.run(a, ("cdf_int",), tiles=True)
    _same(got_a, want_a, WANTS[3], (3, 80))
    _same(got_b, want_b, WANTS[3], (1, 16))
    _same(got_a2, {"cdf_int": want_a["cdf_int"]}, ("cdf_int",), (3, 80))


def _call(prob, x, S, d, l, ws_ptr):
    out = torch.empty(x.shape[0] * x.shape[1] * 16 * 16, device="cuda", dtype=torch.int32)
    _lib.call("pccx_prob_forward_tiled", x.data_ptr(), x.shape[0], S, d, l, prob._blob.data_ptr(), None, None, out.data_ptr(), ws_ptr,
              torch.cuda.current_stream().cuda_stream)


def test_abi_refusals_launch_nothing(prob):
    x = centres(1, 48)
    ws = torch.empty(int(_lib.load().pccx_prob_forward_tiled_workspace_floats(1, 48)) + 4, device="cuda", dtype=torch.float32)
    with pytest.raises(_lib.PccxError, match="S=20"):
        _call(prob, x, 20, D, L, ws.data_ptr())
    for d, l in ((3, 43), (13, 10)):                              # d*L = 129 (only with L above 15), and d*L = 130 inside the d / L limits
        with pytest.raises(_lib.PccxError, match="unsupported"):
            _call(prob, x, 48, d, l, ws.data_ptr())
    with pytest.raises(_lib.PccxError, match="aligned"):
        _call(prob, x, 48, D, L, ws.data_ptr() + 4)
    with pytest.raises(_lib.PccxError, match="B="):
        _lib.call("pccx_prob_forward_tiled", x.data_ptr(), 65536, 48, D, L, prob._blob.data_ptr(), None, None, x.data_ptr(), ws.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    _call(prob, x, 48, D, L, ws.data_ptr())                       # and the same arguments put right are taken
    torch.cuda.synchronize()


def test_workspace_size_function():
    f = _lib.load().pccx_prob_forward_tiled_workspace_floats
    assert f(1, 16) == 256 + 512 and f(3, 80) == 3 * (2 * 256 + 512)
    assert f(1, 4096) == 64 * 256 + 512 == f(1, 8192)             # the cap of 64 workgroups
    assert f(0, 64) == 0 and f(2, 0) == 0


def test_an_empty_batch_returns_empty_outputs(prob):
    got = prob.run(torch.empty(0, 16, 3, device="cuda"), WANTS[3], tiles=True)
    assert got["pmf"].shape == (0, 16, D, L) and got["cdf"].shape == (0, 16, D, L + 1) and got["cdf_int"].shape == (0, 16, D, L + 1)
    assert got["cdf_int"].dtype == torch.int32
