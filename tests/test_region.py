"""GPU: the region decode (Codec.decompress_region) layer by layer against its definition -- the selection
against torch comparisons on ops.denormalize, the listed probability rows and the listed range decoder against the same rows of the
whole-cloud entry points, and the decoded points against the rows of Codec.decompress, all with torch.equal."""
import numpy as np
import pytest
import torch

from oracle import ref_model
from pccx import codec, models, ops, synth as cloud_synth
from tests import synth

pytestmark = pytest.mark.gpu

K, _k, D, L = synth.MODEL_CFG            # 256, 128, 16, 7
MARGIN = 0.01


@pytest.fixture(scope="module")
def nets():
    ae = models.AE(K, K // 2, D, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    prob = models.ConditionalProbabilityModel(L, D)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    return ae.pack("cuda"), prob.pack("cuda")


class Case:
    """One compressed batch with everything the tests compare against, computed once and left unchanged."""

    def __init__(self, nets, seed, B, N, G, starts, matmul=None):
        self.S, self.G, self.B, self.N = N * 2 // K, G, B, N
        self.cd = codec.Codec(*nets, K=K, octree_mode="full", max_centres=codec.OCTREE_WIDE_MAX_S, p_split=G, matmul=matmul)
        pc = torch.from_numpy(cloud_synth.cad_batch(seed, B, N)).cuda()
        self.comp = self.cd.compress(pc, np.array(starts), keep_extras=True)
        self.rec = self.comp.extras["rec_sampled"]                                           # (B,S,3)
        self.cdf = self.comp.extras["cdf_int"]                                               # (B,S,d,L+1)
        self.w = ops.denormalize(self.rec, self.comp.c[:, :3].contiguous(), self.comp.c[:, 3].contiguous(), MARGIN)
        self.full = self.cd.decompress(self.comp, S=self.S).view(B, self.S, K // 2, 3)
        torch.cuda.synchronize()

    def one(self, b, comp=None):
        c = comp or self.comp
        return codec.Compressed(c.s_bytes[b:b + 1], c.s_nbytes[b:b + 1], c.p_bytes[b:b + 1], c.p_nbytes[b:b + 1], c.c[b:b + 1], self.N)

    def want(self, b, box, halo=0.0):
        """The definition: (mask of the selected patches, their ascending indices, the touched segments), by torch on fp32."""
        lo, hi = (torch.tensor(v, dtype=torch.float32, device="cuda") for v in box)
        h = torch.tensor(halo, dtype=torch.float32, device="cuda")
        m = ((self.w[b] >= lo - h) & (self.w[b] <= hi + h)).all(dim=1)
        idx = m.nonzero().flatten()
        return m, idx, torch.unique(idx // self.G)

    def mid_box(self, b, span=0.25, p0=None):
        """A box around patch p0's centre that reaches ``span`` of the distinct centre coordinates to either side on every axis, its
        faces at midpoints between neighbouring sorted coordinates (or beyond the outermost one): no face lies on a centre."""
        p0 = self.S // 3 if p0 is None else p0
        lo, hi = [], []
        for ax in range(3):
            u = torch.unique(self.w[b, :, ax]).double().cpu().numpy()
            r = int(np.searchsorted(u, float(self.w[b, p0, ax])))
            i, j = max(r - int(np.ceil(span * len(u))), 0), min(r + int(np.ceil(span * len(u))), len(u) - 1)
            pad = float(self.comp.c[b, 3]) / 128
            lo.append(float(np.float32((u[i - 1] + u[i]) / 2 if i > 0 else u[0] - pad)))
            hi.append(float(np.float32((u[j] + u[j + 1]) / 2 if j + 1 < len(u) else u[-1] + pad)))
        assert not any(np.float32(f) in self.w[b, :, ax % 3].cpu().numpy() for ax, f in enumerate(lo + hi))
        return lo, hi

    def bbox(self, b):
        return self.w[b].amin(dim=0).tolist(), self.w[b].amax(dim=0).tolist()

    def octant(self, b):
        c = self.comp.c[b].tolist()
        return c[:3], [v + c[3] for v in c[:3]]


@pytest.fixture(scope="module")
def c16(nets):
    return Case(nets, 41, 2, 2048, 4, [5, 1234])


@pytest.fixture(scope="module")
def c48(nets):
    return Case(nets, 45, 1, 6144, 5, [9])


@pytest.fixture(scope="module")
def c1088(nets):
    return Case(nets, 43, 1, 139264, 60, [7])


def _case(request, name):
    return request.getfixturevalue(name)


def _select(case, b, box, halo=0.0):
    sel = ops.region_select(case.rec[b], case.comp.c[b], box, case.G, halo, MARGIN)
    n_sel, n_seg = sel.counts.tolist()
    return sel, n_sel, n_seg


def _check_select(case, b, box, halo=0.0):
    sel, n_sel, n_seg = _select(case, b, box, halo)
    m, idx, segs = case.want(b, box, halo)
    assert (n_sel, n_seg) == (idx.numel(), segs.numel())
    assert sel.patch_idx.dtype == torch.int64 and sel.seg_idx.dtype == torch.int32
    assert torch.equal(sel.patch_idx[:n_sel], idx) and torch.equal(sel.seg_idx[:n_seg].long(), segs)
    rows = torch.searchsorted(segs, idx // case.G) * case.G + idx % case.G
    assert torch.equal(sel.rows[:n_sel], rows)
    again, n2, s2 = _select(case, b, box, halo)                                          # no atomics: the same lists on every run
    assert (n2, s2) == (n_sel, n_seg) and torch.equal(again.patch_idx[:n_sel], idx) and torch.equal(again.seg_idx[:n_seg].long(), segs)
    assert torch.equal(again.rows[:n_sel], rows)
    return n_sel, n_seg


@pytest.mark.parametrize("name,S,G", [("c16", 16, 4), ("c48", 48, 5), ("c1088", 1088, 60)])
def test_select_against_torch_on_the_denormalised_centres(request, name, S, G):
    case = _case(request, name)
    assert (case.S, case.G) == (S, G)
    for b in range(case.B):
        n_sel, n_seg = _check_select(case, b, case.mid_box(b))
        assert 0 < n_sel < S
        _check_select(case, b, case.mid_box(b, 0.1, p0=case.S - 1))
        assert _check_select(case, b, case.bbox(b)) == (S, -(-S // G))                   # a box holding everything
        lo, hi = case.bbox(b)
        step = float(case.comp.c[b, 3]) / 64
        empty = ([hi[0] + step, lo[1], lo[2]], [hi[0] + 2 * step, hi[1], hi[2]])       # a slab beyond the cloud's +x face
        assert _check_select(case, b, empty) == (0, 0)
        assert _check_select(case, b, empty, halo=2 * step)[0] > 0                       # the halo reaches back into the cloud
        assert _check_select(case, b, empty, halo=step / 2) == (0, 0)


@pytest.mark.parametrize("name", ["c16", "c1088"])
def test_the_upper_octant_is_a_prefix_of_the_patch_order(request, name):
    """The decoded centres come in descending Morton order, so [center, center + longest] is the first n_sel patches and the first
    ceil(n_sel / G) segments: why a box meets few segments."""
    case = _case(request, name)
    for b in range(case.B):
        sel, n_sel, n_seg = _select(case, b, case.octant(b))
        assert 0 < n_sel < case.S
        assert torch.equal(sel.patch_idx[:n_sel], torch.arange(n_sel, device="cuda"))
        assert n_seg == -(-n_sel // case.G) and torch.equal(sel.seg_idx[:n_seg].long(), torch.arange(n_seg, device="cuda"))


def _orig_rows(segs, S, G):
    r = torch.arange(len(segs) * G, device="cuda")
    orig = torch.tensor(segs, device="cuda")[r // G] * G + r % G
    return orig, orig < S


@pytest.mark.parametrize("name,segs", [("c16", [0, 1, 2, 3]), ("c16", [2]), ("c48", [0, 3, 9]), ("c48", [0, 1, 3, 5, 9]),
                                       ("c1088", [0, 5, 6, 17, 18]), ("c1088", list(range(19)))])
def test_probability_rows_of_listed_segments(request, nets, name, segs):
    case = _case(request, name)
    S, G = case.S, case.G
    prob = nets[1]
    full = prob.run(case.rec[:1], ("cdf_int",))["cdf_int"][0]
    assert torch.equal(full, case.cdf[0])
    seg_idx = torch.tensor(segs + [0, 0], device="cuda", dtype=torch.int32)              # entries past n_seg are not read
    got = prob.run_segments(case.rec[0], seg_idx, len(segs), G)
    assert got.shape == (len(segs) * G, D, L + 1) and got.dtype == torch.int32
    orig, valid = _orig_rows(segs, S, G)
    assert bool(valid.all()) == (segs[-1] * G + G <= S)
    assert torch.equal(got[valid], full[orig[valid]])
    assert torch.equal(prob.run_segments(case.rec[0], seg_idx, len(segs), G), got)
    assert prob.run_segments(case.rec[0], seg_idx, 0, G).shape == (0, D, L + 1)
    # the listed and the whole-cloud tiled entry points share their kernels: every segment listed gives the tiled path's rows
    P = -(-S // G)
    every = prob.run_segments(case.rec[0], torch.arange(P, device="cuda", dtype=torch.int32), P, G)
    assert torch.equal(every[:S], prob.run(case.rec[:1], ("cdf_int",), tiles=True)["cdf_int"][0])


def _flip_unlisted(p_bytes, nbytes, P, listed):
    """XOR 0xFF into the payload bytes of every unlisted segment; header and directory stay."""
    raw = p_bytes.cpu().numpy().copy()
    lens = raw[12:12 + 2 * P].view("<u2").astype(np.int64)
    off = 12 + 2 * P + np.concatenate([[0], np.cumsum(lens)])
    assert off[-1] == nbytes
    flipped = 0
    for p in range(P):
        if p not in listed:
            raw[off[p]:off[p + 1]] ^= 0xFF
            flipped += int(lens[p])
    assert flipped > 0
    return torch.from_numpy(raw).cuda()


@pytest.mark.parametrize("name,segs", [("c16", [1, 2]), ("c48", [0, 9]), ("c1088", [0, 18]), ("c1088", [3, 4, 11])])
def test_listed_range_decode_reads_only_the_listed_segments(request, name, segs):
    case = _case(request, name)
    S, G = case.S, case.G
    P = -(-S // G)
    comp = case.one(0)
    q_full = models.range_decode_split(case.cdf[:1], comp.p_bytes, comp.p_nbytes, L, G * D).view(S, D)
    orig, valid = _orig_rows(segs, S, G)
    cdf = case.cdf[0][orig.clamp(max=S - 1)].contiguous()
    seg_idx = torch.tensor(segs, device="cuda", dtype=torch.int32)
    q, status = models.range_decode_split_list(cdf, comp.p_bytes[0], comp.p_nbytes, L, G * D, S * D, seg_idx, len(segs))
    assert int(status) == 0 and q.shape == (len(segs) * G * D,)
    assert torch.equal(q.view(-1, D)[valid], q_full[orig[valid]])
    foreign = _flip_unlisted(comp.p_bytes[0], int(comp.p_nbytes[0]), P, segs)
    q2, status2 = models.range_decode_split_list(cdf, foreign, comp.p_nbytes, L, G * D, S * D, seg_idx, len(segs))
    assert int(status2) == 0 and torch.equal(q2.view(-1, D)[valid], q_full[orig[valid]])
    _, st = models.range_decode_split_list(None, comp.p_bytes[0], comp.p_nbytes, L, (G + 1) * D, S * D, None, 0)   # the check alone
    assert int(st) == 2


def _check_region(case, cd, b, comp, full, box, halo=0.0):
    reg = cd.decompress_region(case.one(b, comp), case.S, box, halo)
    _, idx, segs = case.want(b, box, halo)
    assert torch.equal(reg.patch_idx, idx) and torch.equal(reg.segments, segs) and reg.n_segments_total == -(-case.S // case.G)
    assert reg.points.dtype == torch.float32 and reg.points.shape == (idx.numel() * (K // 2), 3)
    assert torch.equal(reg.points, full[b][idx].reshape(-1, 3))
    return reg


@pytest.mark.parametrize("matmul", ["f16x2", "f32", "bf16x3"])
def test_small_clouds_end_to_end_in_every_decoder_mode(nets, c16, tmp_path, matmul):
    case = c16 if c16.cd.decoder_matmul == matmul else Case(nets, 41, 2, 2048, 4, [5, 1234], matmul=matmul)
    assert case.cd.decoder_matmul == matmul
    names = [f"c{b}.ply" for b in range(case.B)]
    case.comp.write_files(str(tmp_path), names)
    back = codec.Compressed.read_files(str(tmp_path), names, n_points=case.N, device="cuda")
    for b in range(case.B):
        lo, hi = case.bbox(b)
        far = ([v + 10.0 for v in hi], [v + 11.0 for v in hi])
        for comp in (case.comp, back):
            reg = _check_region(case, case.cd, b, comp, case.full, case.mid_box(b))
            assert 0 < reg.patch_idx.numel() < case.S
            _check_region(case, case.cd, b, comp, case.full, case.mid_box(b, 0.4, p0=0), halo=float(case.comp.c[b, 3]) / 50)
            _check_region(case, case.cd, b, comp, case.full, case.octant(b))
            whole = _check_region(case, case.cd, b, comp, case.full, (lo, hi))
            assert torch.equal(whole.points, case.full[b].reshape(-1, 3))                # the box holding everything = the full decode
            none = _check_region(case, case.cd, b, comp, case.full, far)
            assert none.points.shape == (0, 3) and none.patch_idx.numel() == 0 and none.segments.numel() == 0


def test_wide_cloud_end_to_end_octant_and_last_segment(c1088, tmp_path):
    case = c1088
    S, G = case.S, case.G
    assert (S, G, -(-S // G), S - 18 * G) == (1088, 60, 19, 8)
    case.comp.write_files(str(tmp_path), ["room.ply"])
    back = codec.Compressed.read_files(str(tmp_path), ["room.ply"], n_points=case.N, device="cuda")
    last = case.w[0, S - 1].tolist()                                                     # the lowest Morton key: the last segment's
    for comp in (case.comp, back):
        reg = _check_region(case, case.cd, 0, comp, case.full, case.octant(0))
        assert 0 < reg.patch_idx.numel() < S and reg.segments.numel() < 19
        reg = _check_region(case, case.cd, 0, comp, case.full, (last, last))              # a closed box of one point: that patch
        assert reg.patch_idx.tolist() == [S - 1] and reg.segments.tolist() == [18]
    _check_region(case, case.cd, 0, case.comp, case.full, case.mid_box(0, 0.15, p0=S // 2))


def test_a_stream_written_without_the_split_is_refused(nets, c16):
    plain = codec.Codec(*nets, K=K, octree_mode="full")
    pc = torch.from_numpy(cloud_synth.cad_batch(41, 2, 2048)).cuda()
    comp0 = plain.compress(pc, np.array([5, 1234]))
    with pytest.raises(models._lib.PccxError, match="clouds"):
        c16.cd.decompress_region(c16.one(0, comp0), c16.S, c16.bbox(0))
    with pytest.raises(models._lib.PccxError, match="clouds"):
        codec.Codec(*nets, K=K, octree_mode="full", p_split=5).decompress_region(c16.one(0), c16.S, c16.bbox(0))


def test_shapes_outside_the_fused_probability_kernel_take_the_full_decode(nets):
    """S = 17 is no multiple of 16 (prob.fused_ok false): decompress_region decodes the cloud and takes the rows, the same result."""
    case = Case(nets, 41, 1, 2176, 4, [5])
    assert case.S == 17 and not nets[1].fused_ok(17)
    reg = _check_region(case, case.cd, 0, case.comp, case.full, case.mid_box(0))
    assert 0 < reg.patch_idx.numel() < 17
    _check_region(case, case.cd, 0, case.comp, case.full, case.bbox(0))
