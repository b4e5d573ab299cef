"""Codec(prob_path="tiles") against Codec(prob_path="cloud"): the integer CDF is the same function of the same
centres, so compress writes the same bytes, decompress decodes the same points whichever side used which path, and build_index
makes the same sidecar."""
import numpy as np
import pytest
import torch

from oracle import ref_model
from pccx import codec, models, synth as cloud_synth
from tests import synth

K, _k, D, L = synth.MODEL_CFG            # 256, 128, 16, 7


def _nets(device=None):
    ae = models.AE(K, K // 2, D, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    prob = models.ConditionalProbabilityModel(L, D)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    return (ae.pack(device), prob.pack(device)) if device else (ae, prob)


@pytest.fixture(scope="module")
def nets():
    return _nets("cuda")


def _pair(nets, **kw):
    kw = dict(dict(K=K, octree_mode="full", max_centres=codec.OCTREE_WIDE_MAX_S), **kw)
    return {path: codec.Codec(*nets, prob_path=path, **kw) for path in ("cloud", "tiles")}


def _same_streams(a, b):
    """s_bytes / p_bytes are rows of capacity whose tail past s_nbytes / p_nbytes no kernel writes: the streams are the prefixes."""
    for f in ("s_nbytes", "p_nbytes", "c"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.s_bytes.shape == b.s_bytes.shape and a.p_bytes.shape == b.p_bytes.shape
    for i, (sn, pn) in enumerate(zip(a.s_nbytes.tolist(), a.p_nbytes.tolist())):
        assert sn > 0 and pn > 0
        assert torch.equal(a.s_bytes[i, :sn], b.s_bytes[i, :sn]) and torch.equal(a.p_bytes[i, :pn], b.p_bytes[i, :pn])
        assert a.files(i) == b.files(i)
    assert torch.equal(a.extras["cdf_int"], b.extras["cdf_int"])


def _fresh(comp, N):
    """The streams alone, as read from files: nothing of compress's own state (the kept integer CDF, the extras) travels."""
    return codec.Compressed(comp.s_bytes, comp.s_nbytes, comp.p_bytes, comp.p_nbytes, comp.c, N)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,kw", [(2, 2048, {}), (1, 6144, {}), (1, 139264, {"p_split": 60})])
def test_same_files_and_same_decode_in_all_four_pairings(nets, B, N, kw):
    cds = _pair(nets, **kw)
    pc = torch.from_numpy(cloud_synth.cad_batch(61, B, N)).cuda()
    starts = np.array([5, 1234][:B])
    comp = {path: cd.compress(pc, starts, keep_extras=True) for path, cd in cds.items()}
    _same_streams(comp["tiles"], comp["cloud"])
    S = N * 2 // K
    want = cds["cloud"].decompress(_fresh(comp["cloud"], N), S=S)
    assert want.shape == (B, S * (K // 2), 3)
    for wrote in ("cloud", "tiles"):
        for reads in ("cloud", "tiles"):
            assert torch.equal(cds[reads].decompress(_fresh(comp[wrote], N), S=S), want), (wrote, reads)


@pytest.mark.gpu
def test_entry_point_index_from_compress_and_from_build_index(nets):
    N, S = 6144, 48
    cds = _pair(nets, p_index=16)
    pc = torch.from_numpy(cloud_synth.cad_batch(62, 1, N)).cuda()
    comp = {path: cd.compress(pc, np.array([9]), keep_extras=True) for path, cd in cds.items()}
    _same_streams(comp["tiles"], comp["cloud"])
    assert comp["cloud"].p_index is not None and torch.equal(comp["tiles"].p_index, comp["cloud"].p_index)
    for path, cd in cds.items():
        bare = _fresh(comp["cloud"], N)                                                      # a copy with the index dropped
        assert bare.p_index is None
        built = cd.build_index(bare, S=S)
        assert torch.equal(built, comp["cloud"].p_index) and bare.p_index is built, path
        assert torch.equal(cd.decompress(bare, S=S), cds["cloud"].decompress(comp["cloud"], S=S))


@pytest.mark.gpu
def test_reference_mode_where_the_distinct_centre_kernel_ran(nets):
    """octree_mode "reference": _distinct() is true and "cloud" runs pccx_prob_forward_distinct; "tiles" replaces it, same files."""
    B, N = 2, 8192
    cds = _pair(nets, octree_mode="reference", max_centres=codec.OCTREE_MAX_S)
    assert cds["cloud"]._distinct() and cds["tiles"]._distinct()
    pc = torch.from_numpy(cloud_synth.cad_batch(63, B, N)).cuda()
    comp = {path: cd.compress(pc, np.array([3, 4567]), keep_extras=True) for path, cd in cds.items()}
    _same_streams(comp["tiles"], comp["cloud"])
    want = cds["cloud"].decompress(_fresh(comp["cloud"], N))
    assert torch.equal(cds["tiles"].decompress(_fresh(comp["tiles"], N)), want)
    assert torch.equal(cds["tiles"].decompress(_fresh(comp["cloud"], N)), want)


@pytest.mark.gpu
def test_region_decode_is_untouched(nets):
    N, S = 6144, 48
    cd = _pair(nets, p_split=5)["tiles"]
    pc = torch.from_numpy(cloud_synth.cad_batch(64, 1, N)).cuda()
    comp = cd.compress(pc, np.array([9]))
    full = cd.decompress(_fresh(comp, N), S=S)[0].view(S, K // 2, 3)
    c = comp.c[0].tolist()
    for box in ((c[:3], [v + c[3] for v in c[:3]]),                                      # the upper octant: a prefix of the patches
                ([v - c[3] for v in c[:3]], [v + c[3] for v in c[:3]])):                 # everything
        reg = cd.decompress_region(_fresh(comp, N), S, box)
        assert torch.equal(reg.points, full[reg.patch_idx].reshape(-1, 3))
    assert reg.patch_idx.numel() == S


def test_an_unknown_prob_path_is_refused_before_any_gpu_call():
    ae, prob = _nets()                                                                    # on the host, not packed: nothing touches a device
    with pytest.raises(ValueError, match="'cloud' or 'tiles'"):
        codec.Codec(ae, prob, K=K, prob_path="rows")
    assert codec.Codec(ae, prob, K=K).prob_path == "cloud"
    assert codec.Codec(ae, prob, K=K, prob_path="tiles").prob_path == "tiles"
