"""GPU: Codec(p_index=G) -- the three files stay Codec()'s bytes, decompress with the index equals decompress without it, region
decode through the index equals the rows of the full decode and selects what the p_split codec selects, and files written with and
without the index go through both command-line tools.  Random weights as tests/test_region.py; everything with torch.equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model
from pccx import codec, models, plyio, synth as cloud_synth
from tests import index_cases as ic
from tests import synth

pytestmark = pytest.mark.gpu

K, _k, D, L = synth.MODEL_CFG            # 256, 128, 16, 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "point-cloud-compression_amd", "cli")


@pytest.fixture(scope="module")
def nets():
    ae = models.AE(K, K // 2, D, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    prob = models.ConditionalProbabilityModel(L, D)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    return ae.pack("cuda"), prob.pack("cuda")


class Room:
    """N = 16384 points, S = 128 patches, an entry every G = 16: one cloud through the plain, the indexed and the split codec,
    computed once and left unchanged."""
    N, S, G = 16384, 128, 16

    def __init__(self, nets):
        kw = dict(K=K, octree_mode="full", max_centres=codec.OCTREE_WIDE_MAX_S)
        self.plain, self.indexed, self.split = codec.Codec(*nets, **kw), codec.Codec(*nets, p_index=self.G, **kw), codec.Codec(*nets, p_split=self.G, **kw)
        self.pc = torch.from_numpy(cloud_synth.cad_batch(47, 1, self.N)).cuda()
        start = np.array([11])
        self.c_plain, self.c_indexed, self.c_split = (cd.compress(self.pc, start) for cd in (self.plain, self.indexed, self.split))
        self.full = self.plain.decompress(self.c_plain, S=self.S)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def room(nets):
    return Room(nets)


def test_the_three_files_are_those_of_the_codec_without_the_index(room):
    assert room.c_plain.p_index is None and int(room.c_plain.index_bits()[0]) == 0
    assert room.c_plain.files(0) == room.c_indexed.files(0)
    assert torch.equal(room.c_plain.bits(), room.c_indexed.bits()) and torch.equal(room.c_plain.bpp(), room.c_indexed.bpp())
    P = room.S // room.G
    assert room.c_indexed.p_index.shape == (1, 16 + 12 * P) and int(room.c_indexed.index_bits()[0]) == 8 * (16 + 12 * P)
    side = bytes(room.c_indexed.p_index[0].cpu().numpy())
    e = ic.parse(side, room.S * D, room.G * D)
    assert tuple(e[0]) == ic.INITIAL and (np.diff(e[:, 2] & 0x7FFFFFFF) >= 0).all()
    assert models.index_status(side, len(room.c_plain.files(0)[1]), room.S * D, room.G * D) == 0


def test_decompress_with_the_index_equals_decompress_without_it(room):
    assert torch.equal(room.indexed.decompress(room.c_indexed, S=room.S), room.full)
    # the index absent: the same codec falls back to the sequential decoder
    assert torch.equal(room.indexed.decompress(room.c_plain, S=room.S), room.full)
    # the index of a stream written without one, bit for bit the encoder's
    bare = codec.Compressed(room.c_plain.s_bytes, room.c_plain.s_nbytes, room.c_plain.p_bytes, room.c_plain.p_nbytes, room.c_plain.c, room.N)
    built = room.indexed.build_index(bare, room.S)
    assert torch.equal(built, room.c_indexed.p_index) and bare.p_index is built
    assert torch.equal(room.indexed.decompress(bare, S=room.S), room.full)
    # an index of another G is refused by name
    other = codec.Codec(room.indexed.ae, room.indexed.prob, K=K, octree_mode="full", max_centres=codec.OCTREE_WIDE_MAX_S, p_index=8)
    with pytest.raises(models._lib.PccxError, match=r"clouds \[0\].*disagree"):
        other.decompress(room.c_indexed, S=room.S)


def test_reference_octree_mode(nets):
    N, S, G = 8192, 64, 16
    pc = torch.from_numpy(cloud_synth.cad_batch(48, 2, N)).cuda()
    starts = np.array([3, 4567])
    plain, indexed = codec.Codec(*nets, K=K), codec.Codec(*nets, K=K, p_index=G)
    c0, c1 = plain.compress(pc, starts), indexed.compress(pc, starts)
    assert [c0.files(b) for b in range(2)] == [c1.files(b) for b in range(2)]
    assert c1.p_index.shape == (2, 16 + 12 * (S // G))
    want = plain.decompress(c0)
    assert torch.equal(indexed.decompress(c1), want)
    bare = codec.Compressed(c0.s_bytes, c0.s_nbytes, c0.p_bytes, c0.p_nbytes, c0.c, N)
    assert torch.equal(indexed.build_index(bare), c1.p_index) and torch.equal(indexed.decompress(bare), want)
    with pytest.raises(ValueError, match="octree_mode"):
        indexed.decompress_region(codec.Compressed(c1.s_bytes[:1], c1.s_nbytes[:1], c1.p_bytes[:1], c1.p_nbytes[:1], c1.c[:1], N, p_index=c1.p_index[:1]),
                                  S, ((0, 0, 0), (1, 1, 1)))


def _boxes(room):
    c = room.c_plain.c[0].tolist()
    centre, longest = c[:3], c[3]
    lo, hi = room.full[0].amin(dim=0).tolist(), room.full[0].amax(dim=0).tolist()      # the decoded cloud's own bounding box
    yield "octant", (lo, [(a + b) / 2 for a, b in zip(lo, hi)])
    yield "middle", ([v - longest / 7 for v in centre], [v + longest / 5 for v in centre])
    yield "everything", ([v - longest for v in centre], [v + longest for v in centre])
    yield "nothing", ([v + 10 * longest for v in centre], [v + 11 * longest for v in centre])


def test_region_through_the_index_equals_the_rows_of_the_full_decode(room):
    full = room.full[0].view(room.S, K // 2, 3)
    counts = {}
    for name, box in _boxes(room):
        for halo in (0.0, room.c_plain.c[0, 3].item() / 40):
            reg = room.indexed.decompress_region(room.c_indexed, room.S, box, halo)
            ref = room.split.decompress_region(room.c_split, room.S, box, halo)
            assert torch.equal(reg.patch_idx, ref.patch_idx) and torch.equal(reg.segments, ref.segments)
            assert reg.n_segments_total == ref.n_segments_total == room.S // room.G
            assert torch.equal(reg.points, full[reg.patch_idx].reshape(-1, 3)) and torch.equal(reg.points, ref.points)
        counts[name] = (reg.patch_idx.numel(), reg.segments.numel())
    assert counts["everything"] == (room.S, room.S // room.G) and counts["nothing"] == (0, 0)
    assert 0 < counts["octant"][0] < room.S and 0 < counts["octant"][1] < room.S // room.G
    # without the index on the Compressed, and with the index of another stream: refused, by name
    bare = codec.Compressed(room.c_plain.s_bytes, room.c_plain.s_nbytes, room.c_plain.p_bytes, room.c_plain.p_nbytes, room.c_plain.c, room.N)
    with pytest.raises(ValueError, match="comp.p_index"):
        room.indexed.decompress_region(bare, room.S, dict(_boxes(room))["octant"])
    bare.p_index = room.c_indexed.p_index.clone()
    bare.p_index[0, 16 + 12 + 8:16 + 12 + 12] = torch.tensor([0xFF, 0xFF, 0xFF, 0x7F], dtype=torch.uint8)   # entry 1: position 2^31 - 1
    with pytest.raises(models._lib.PccxError, match="clouds"):
        room.indexed.decompress_region(bare, room.S, dict(_boxes(room))["octant"])


def test_files_and_both_command_line_tools(room, nets, tmp_path):
    """write_files / read_files with the sidecar, then compress.py --p-index, decompress.py --p-index, --build-index on a directory
    written without --p-index, and --region through the index: each tool a fresh child process."""
    names = ["room.ply"]
    lib_dir = tmp_path / "lib"
    room.c_indexed.write_files(str(lib_dir.mkdir() or lib_dir), names)
    assert sorted(os.listdir(lib_dir)) == ["room.ply.c.bin", "room.ply.p.bin", "room.ply.p.idx", "room.ply.s.bin"]
    assert (lib_dir / "room.ply.p.idx").read_bytes() == bytes(room.c_indexed.p_index[0].cpu().numpy())
    back = codec.Compressed.read_files(str(lib_dir), names, n_points=room.N, device="cuda", p_index=(room.S * D, room.G * D))
    assert torch.equal(back.p_index, room.c_indexed.p_index) and back.p_index_nbytes.tolist() == [16 + 12 * room.S // room.G]
    assert torch.equal(room.indexed.decompress(back, S=room.S), room.full)
    box = dict(_boxes(room))["octant"]
    want = room.indexed.decompress_region(room.c_indexed, room.S, box)
    assert torch.equal(room.indexed.decompress_region(back, room.S, box).points, want.points)

    data, mdl, with_idx, without, dec1, dec2, dec3 = (tmp_path / n for n in ("data", "model", "with", "without", "dec1", "dec2", "dec3"))
    data.mkdir(), mdl.mkdir()
    plyio.save_point_cloud(room.pc[0].cpu().numpy(), str(data / names[0]))
    ae = models.AE(K, K // 2, D, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    prob = models.ConditionalProbabilityModel(L, D)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    torch.save(ae.state_dict(), str(mdl / "ae.pkl"))
    torch.save(prob.state_dict(), str(mdl / "prob.pkl"))
    run = lambda *a: subprocess.run([sys.executable, *a], capture_output=True, text=True, timeout=600)
    flags = ["--octree-mode", "full", "--p-index", str(room.G)]
    r = run(os.path.join(CLI, "compress.py"), str(data / "*.ply"), str(with_idx), str(mdl), *flags)
    assert r.returncode == 0 and "Execution time" in r.stdout and "index 0.0" in r.stdout, r.stderr[-2000:]
    r = run(os.path.join(CLI, "compress.py"), str(data / "*.ply"), str(without), str(mdl), "--octree-mode", "full")
    assert r.returncode == 0, r.stderr[-2000:]
    assert not os.path.exists(without / "room.ply.p.idx") and os.path.exists(with_idx / "room.ply.p.idx")
    for ext in (".p.bin", ".s.bin", ".c.bin"):
        assert (with_idx / ("room.ply" + ext)).read_bytes() == (without / ("room.ply" + ext)).read_bytes(), ext

    r = run(os.path.join(CLI, "decompress.py"), str(with_idx), str(dec1), str(mdl), *flags)
    assert r.returncode == 0 and "Index 0.0" in r.stdout, r.stderr[-2000:]
    r = run(os.path.join(CLI, "decompress.py"), str(without), str(dec2), str(mdl), *flags)
    assert r.returncode != 0 and "--build-index" in r.stderr and not os.path.exists(without / "room.ply.p.idx")
    r = run(os.path.join(CLI, "decompress.py"), str(without), str(dec2), str(mdl), *flags, "--build-index")
    assert r.returncode == 0 and "built room.ply.p.idx" in r.stdout, r.stderr[-2000:]
    assert (without / "room.ply.p.idx").read_bytes() == (with_idx / "room.ply.p.idx").read_bytes()
    a, b = plyio.read_point_cloud(str(dec1 / names[0])), plyio.read_point_cloud(str(dec2 / names[0]))
    assert np.array_equal(a, b) and a.shape == (room.S * K // 2, 3)
    # the CLI's own compress chose its FPS start, so its full decode is the definition here
    cli_back = codec.Compressed.read_files(str(with_idx), names, n_points=room.N, device="cuda", p_index=(room.S * D, room.G * D))
    assert np.array_equal(a, room.plain.decompress(cli_back, S=room.S)[0].cpu().numpy())
    lo, hi = a.min(axis=0).tolist(), ((a.min(axis=0) + a.max(axis=0)) / 2).tolist()    # the lower octant of the decoded cloud's box
    reg = room.indexed.decompress_region(cli_back, room.S, (lo, hi))
    r = run(os.path.join(CLI, "decompress.py"), str(with_idx), str(dec3), str(mdl), *flags, "--region", *[repr(float(np.float32(v))) for v in lo + hi])
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(plyio.read_point_cloud(str(dec3 / names[0])), reg.points.cpu().numpy()) and 0 < reg.patch_idx.numel() < room.S
