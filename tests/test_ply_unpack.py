"""GPU: plyio.read_point_clouds (host threads + pccx_ply_unpack, csrc/plyio.hip) against plyio.read_point_cloud on the same files,
compared as int32 bit patterns: the NaN fill behind a cloud and the payload of a float32 NaN are pinned."""
import os

import numpy as np
import pytest
import torch

from pccx import codec, ops, plyio
from tests import ply_cases as pc
from tests.test_no_memset_nodes import CSRC, _calls

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, 0x5A5A5A5A
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]        # the wave edge, the tile edge, a tile with a single record


def _node_kinds(graph):
    """hipGraphNodeType -> count over the nodes of a hipGraph captured with keep_graph=True (0 kernel, 1 memcpy, 2 memset)"""
    import ctypes as C
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    raw, n = C.c_void_p(graph.raw_cuda_graph()), C.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, C.byref(n)) == 0 and n.value > 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, C.byref(n)) == 0
    kinds = {}
    for node in nodes:
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)) == 0
        kinds[t.value] = kinds.get(t.value, 0) + 1
    return kinds


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


@pytest.fixture(scope="module")
def ragged_files(tmp_path_factory):
    """sixteen binary files: every size twice, the seven layouts (strides 7 9 12 15 24 27 300) in turn, each in both byte orders; and
    two ASCII files.  -> (paths, the clouds plyio.read_point_cloud gives)"""
    d = tmp_path_factory.mktemp("ragged")
    strides, paths = list(pc.LAYOUTS), []
    for i, n in enumerate(SIZES + SIZES):
        paths.append(str(d / f"c{i:02d}.ply"))
        pc.write_ply(paths[-1], pc.LAYOUTS[strides[i % 7]], n, pc.LE if i % 2 == 0 else pc.BE, 100 + i, upper=i % 3 == 0, comments=i % 4 == 1,
                     faces=i % 5 == 2, crlf=i % 6 == 3)
    for j, n in enumerate((5, 300)):
        paths.append(str(d / f"a{j}.ply"))
        pc.write_ply(paths[-1], pc.LAYOUTS[15 if j else 27], n, pc.ASCII, 200 + j, crlf=bool(j))
    return paths, [plyio.read_point_cloud(p) for p in paths]


def test_ragged_batch_equals_pad_clouds_bit_for_bit(ragged_files):
    paths, clouds = ragged_files
    want, n_want = codec.pad_clouds(clouds)
    got, n = plyio.read_point_clouds(paths, "cuda", layout="padded")
    assert n == n_want and got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(bits(got), want.view(torch.int32))
    # consecutive 16-byte-aligned vertex blocks, most of them starting at an odd place inside their 16 bytes' neighbours
    table = plyio.scan_point_clouds(paths)
    off, _ = plyio.staging_offsets(table)
    assert (off % 16 == 0).all() and (np.diff(off) == (plyio.block_bytes(table)[:-1] + 15) // 16 * 16).all()
    # the float32 files hold NaN payloads, and the comparison above saw them
    assert any(np.isnan(c).any() and (c.view(np.uint32)[np.isnan(c)] != 0x7FC00000).any() for c in clouds)
    for threads in (1, 3):
        again, _ = plyio.read_point_clouds(paths, "cuda", threads=threads)
        assert torch.equal(bits(again), want.view(torch.int32))


def test_packed_layout_inside_guard_bands(ragged_files):
    paths, clouds = ragged_files
    points, offsets, sizes = codec.pack_clouds(clouds)
    arena = torch.full((3 * sum(sizes) + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    out = arena[GUARD:GUARD + 3 * sum(sizes)].view(torch.float32).view(-1, 3)
    got, got_off, got_sizes = plyio.read_point_clouds(paths, "cuda", layout="packed", out=out)
    assert got_sizes == sizes and got_off.dtype == torch.int64 and torch.equal(got_off.cpu(), offsets)
    assert got.data_ptr() == out.data_ptr() and torch.equal(bits(got), points.view(torch.int32))
    assert bool((arena[:GUARD] == SENTINEL).all()) and bool((arena[-GUARD:] == SENTINEL).all())


@pytest.mark.filterwarnings("ignore:overflow encountered in cast")      # the oracle's astype on values beyond FLT_MAX
def test_conversion_edge_values(tmp_path):
    """float64 and uint32 as numpy's astype(float32) converts them: ties to even, beyond FLT_MAX, into the subnormals, signed zeros and
    infinities, integers above 2^24"""
    fmax = float(np.finfo(np.float32).max)
    f8 = [1 + 2.0**-24, 1 + 3 * 2.0**-24, 1 + 2.0**-24 + 2.0**-50, -(1 + 2.0**-24), 3.5e38, -3.5e38, 1e300, -1e300, fmax, fmax + 2.0**103,
          np.nextafter(fmax + 2.0**103, 0), -(fmax + 2.0**103), 1e-40, -1e-40, 2.0**-149, 2.0**-150, np.nextafter(2.0**-150, 1), 1.5 * 2.0**-149,
          2.5 * 2.0**-149, 2.0**-126, np.nextafter(2.0**-126, 0), 1e-320, 5e-324, 0.0, -0.0, np.inf, -np.inf, 0.1, 1 / 3, np.nan]
    u4 = [0, 1, 2**24, 2**24 + 1, 2**24 + 2, 2**24 + 3, 2**25 + 2, 2**25 + 6, 2**31, 2**31 + 128, 2**31 + 129, 2**31 + 384, 2**32 - 1,
          2**32 - 128, 2**32 - 129, 2**32 - 384, 0xFFFFFF7F, 0xFFFFFF80, 123456789, 4000000001, 16777217]
    files = []
    for name, t, vals in (("f8", "f8", f8), ("u4", "u4", u4)):
        vals = vals + [vals[0]] * (-len(vals) % 3)
        a = np.array(vals, dtype=t).reshape(-1, 3)
        rec = np.zeros(a.shape[0], dtype=[("x", t), ("y", t), ("z", t)])
        rec["x"], rec["y"], rec["z"] = a[:, 0], a[:, 1], a[:, 2]
        for fmt in (pc.LE, pc.BE):
            files.append(str(tmp_path / f"{name}_{fmt}.ply"))
            pc.write_ply(files[-1], [("x", t), ("y", t), ("z", t)], a.shape[0], fmt, 0, rec=rec)
    want = [plyio.read_point_cloud(f) for f in files]
    with np.errstate(over="ignore"):
        assert want[0].tobytes() == np.array(f8, dtype=np.float64).astype(np.float32).reshape(-1, 3).tobytes()        # the oracle is astype
    got, n = plyio.read_point_clouds(files, "cuda")
    for b, w in enumerate(want):
        g, w = got[b, :n[b]].cpu().numpy().reshape(-1), w.reshape(-1)
        nan = np.isnan(w)
        assert nan.sum() == (1 if b < 2 else 0) and np.isnan(g[nan]).all()
        assert g[~nan].tobytes() == w[~nan].tobytes(), (files[b], g.view(np.uint32)[g.view(np.uint32) != w.view(np.uint32)][:4])


@pytest.mark.parametrize("case", ["one", "many-small", "large-beside-small"])
def test_batch_shapes(tmp_path, case):
    """B = 1; 300 clouds of 1 .. 5 points, where most tiles hold one cloud's few records; 70 000 points beside 3"""
    if case == "one":
        spec = [(12, 77)]
    elif case == "many-small":
        spec = [((7, 9, 12, 15, 24, 27, 300)[i % 7], 1 + i % 5) for i in range(300)]
    else:
        spec = [(15, 70000), (27, 3)]
    paths = []
    for i, (stride, n) in enumerate(spec):
        paths.append(str(tmp_path / f"{i}.ply"))
        pc.write_ply(paths[-1], pc.LAYOUTS[stride], n, pc.BE if i % 3 == 1 else pc.LE, 300 + i)
    clouds = [plyio.read_point_cloud(p) for p in paths]
    want, n_want = codec.pad_clouds(clouds)
    got, n = plyio.read_point_clouds(paths, "cuda")
    assert n == n_want and torch.equal(bits(got), want.view(torch.int32))
    points, offsets, sizes = codec.pack_clouds(clouds)
    got, got_off, got_sizes = plyio.read_point_clouds(paths, "cuda", layout="packed")
    assert got_sizes == sizes and torch.equal(got_off.cpu(), offsets) and torch.equal(bits(got), points.view(torch.int32))


def test_captured_call_is_one_kernel_node(ragged_files):
    """pccx_ply_unpack enqueues kernels only: captured, its graph holds no memcpy and no memset node (read from the hipGraph itself),
    and csrc/plyio.hip calls neither (the lint of tests/test_no_memset_nodes.py)"""
    paths, clouds = ragged_files
    table = plyio.scan_point_clouds(paths)
    off, nbytes = plyio.staging_offsets(table)
    host = torch.zeros(nbytes, dtype=torch.uint8)
    plyio.load_point_clouds(paths, table, host, off)
    n = table[:, plyio.N_VERTEX]
    dev, prefix = plyio.device_tables(table, off, np.cumsum(n) - n, n)
    args = [host.cuda(), torch.from_numpy(dev).cuda(), torch.from_numpy(prefix).cuda(), torch.zeros(int(n.sum()), 3, device="cuda")]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ply_unpack(*args, total_tiles=int(prefix[-1]))
    torch.cuda.current_stream().wait_stream(side)
    args[3].zero_()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        ops.ply_unpack(*args, total_tiles=int(prefix[-1]))
    kinds = _node_kinds(graph)
    print("node kinds (0 kernel, 1 memcpy, 2 memset):", kinds)
    assert kinds == {0: 1}, kinds
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(args[3]), codec.pack_clouds(clouds)[0].view(torch.int32))
    for what in ("hipMemsetAsync", "hipMemset", "hipMemcpyAsync", "hipMemcpy"):
        assert _calls(os.path.join(CSRC, "plyio.hip"), what) == []


def test_bad_tables_and_files_are_refused_before_any_launch(tmp_path, ragged_files):
    paths, _ = ragged_files
    bad = str(tmp_path / "bad.ply")
    open(bad, "wb").write(b"ply\nformat binary_little_endian 1.0\nelement vertex 9\nproperty float x\nproperty float y\nproperty float z\nend_header\n" + bytes(50))
    with pytest.raises(ValueError, match="bad.ply.*too short"):
        plyio.read_point_clouds(paths[:2] + [bad], "cuda")
    stage = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(ops._lib.PccxError, match="multiple of 16"):
        ops.ply_unpack(stage[1:33], torch.zeros(1, 12, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
                       torch.zeros(4, 3, device="cuda"), 1)
