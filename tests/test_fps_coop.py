"""GPU: pccx_fps_coop -- one cloud's farthest point sampling on G workgroups (csrc/geometry.hip, fps_coop_kernel).

The keys of distinct points are distinct and max is associative, so the merged winner of a round does not depend on the partition or
on the order in which the workgroups arrive: the indices must equal pccx_fps's (one workgroup per cloud; above 16384 points its
global-memory form) for every G.  That identity is what these tests pin, with torch.equal.
"""
import numpy as np
import pytest
import torch

from oracle import cport
from pccx import _lib, ops

pytestmark = pytest.mark.gpu


def _cloud(seed, B, N):
    return torch.from_numpy(np.random.default_rng(seed).random((B, N, 3), dtype=np.float32)).cuda()


def _same(xyz, npoint, start, G, **kw):
    want = ops.farthest_point_sample_batch(xyz, npoint, start)
    got = ops.farthest_point_sample_batch(xyz, npoint, start, workgroups=G, **kw)
    assert got.dtype == torch.int64 and got.shape == want.shape
    assert torch.equal(got, want), f"G={G}: first difference at {torch.nonzero(got != want)[:1].tolist()}"
    return got


@pytest.mark.parametrize("N,G", [(1000, 2),        # partial lanes, a workgroup with no point at all
                                 (4099, 3),        # uneven split
                                 (16385, 2),       # the smallest G allowed; the reference side is the global-memory kernel
                                 (40000, 3), (40000, 8)])
def test_equals_the_single_workgroup_kernels(N, G):
    _same(_cloud(N + G, 1, N), 128, np.array([N // 3]), G)


def test_batch_with_three_starts_one_out_of_range():
    N = 4099
    xyz = _cloud(7, 3, N)
    got = _same(xyz, 64, np.array([5, N + 10, N - 1]), 3)
    assert got[:, 0].tolist() == [5, 0, N - 1]                   # an out-of-range start is point 0


@pytest.mark.parametrize("npoint", [1, 2, 64, 300])
def test_npoint(npoint):
    _same(_cloud(11, 2, 5000), npoint, np.array([1, 4999]), 2)


def test_lattice_with_exact_distance_ties():
    g = np.arange(16, dtype=np.float32) / np.float32(16)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(1, 4096, 3)
    for G in (2, 3):
        _same(torch.from_numpy(pts).cuda(), 200, np.array([77]), G)


def test_every_point_stored_twice():
    """npoint above the number of distinct points: the distances reach zero and the lowest index wins from then on"""
    half = np.random.default_rng(5).random((1, 600, 3), dtype=np.float32)
    xyz = torch.from_numpy(np.concatenate([half, half], axis=1)).cuda()
    got = _same(xyz, 700, np.array([3]), 2)
    assert got[0, 600:].eq(got[0, 600]).all() and int(got[0, 600]) == 0


def test_against_the_c_oracle():
    N, S = 20000, 256
    xyz = _cloud(21, 1, N)
    got = ops.farthest_point_sample_batch(xyz, S, np.array([17]), workgroups=4)
    assert np.array_equal(got[0].cpu().numpy(), cport.fps(xyz[0].cpu().numpy(), S, 17))


def test_a_poisoned_workspace_is_cleared_by_the_entry():
    N, S, B = 9000, 96, 2
    xyz = _cloud(31, B, N)
    ws = torch.empty(int(_lib.load().pccx_fps_coop_workspace_bytes(B, S)), device="cuda", dtype=torch.uint8)
    ws.fill_(0xFF)
    a = _same(xyz, S, np.array([0, 8999]), 2, workspace=ws)
    ws.fill_(0xFF)
    b = _same(xyz, S, np.array([0, 8999]), 2, workspace=ws)
    assert torch.equal(a, b)


def test_beside_a_stream_of_ordinary_kernels():
    """The launch shares the device with other work: a side stream keeps the compute units busy while the cooperative launch runs."""
    N, S = 40000, 200
    xyz = _cloud(41, 1, N)
    want = ops.farthest_point_sample_batch(xyz, S, np.array([9]))
    side = torch.cuda.Stream()
    a = torch.randn(1024, 1024, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(50):
            a = torch.tanh(a @ a * 1e-3)
    got = ops.farthest_point_sample_batch(xyz, S, np.array([9]), workgroups=4)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.isfinite(a).all()


def test_auto_gives_the_same_indices_whichever_form_it_takes():
    xyz = _cloud(51, 1, 20000)
    start = np.array([2])
    small = _cloud(52, 2, 3000)                            # up to 16384 points: pccx_fps itself
    assert torch.equal(ops.farthest_point_sample_batch(small, 64, [0, 1], workgroups="auto"), ops.farthest_point_sample_batch(small, 64, [0, 1]))
    assert torch.equal(ops.farthest_point_sample_batch(xyz, 64, start, workgroups="auto"), ops.farthest_point_sample_batch(xyz, 64, start))
    assert torch.equal(ops.farthest_point_sample_batch(xyz, 1100, start, workgroups="auto"), ops.farthest_point_sample_batch(xyz, 1100, start))
    with pytest.raises(ValueError):
        ops.farthest_point_sample_batch(xyz, 64, start, workgroups="many")


def test_a_batch_above_the_compute_units_runs_in_sub_batches():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = cus // 2 + 3                                   # B * 2 workgroups do not fit: two launches
    _same(_cloud(61, B, 700), 16, np.arange(B), 2)


def test_the_host_check_refuses_before_launching():
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    xyz = _cloud(71, 1, 16385)
    with pytest.raises(_lib.PccxError, match="need 2 <= G"):            # G below ceil(N / 16384)
        ops.farthest_point_sample_batch(xyz, 8, np.array([0]), workgroups=1)
    with pytest.raises(_lib.PccxError, match="G"):                      # G above the 64 the barrier is sized for
        ops.farthest_point_sample_batch(xyz, 8, np.array([0]), workgroups=65)
    B = cus + 1                                                         # B * G above the compute units, straight at the entry
    small = _cloud(72, B, 64)
    out = torch.empty(B, 4, device="cuda", dtype=torch.int64)
    ws = torch.empty(int(lib.pccx_fps_coop_workspace_bytes(B, 4)), device="cuda", dtype=torch.uint8)
    with pytest.raises(_lib.PccxError, match="resident"):
        _lib.call("pccx_fps_coop", small.data_ptr(), B, 64, 4, None, out.data_ptr(), 1, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
