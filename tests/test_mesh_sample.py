"""GPU: pccx_mesh_sample (csrc/mesh_sample.hip) bit for bit against the numpy restatement of the sampler's definition
(tests/mesh_cases.py): weights and prefix, samples raw and normalised, independence of the batch, statuses, no write outside."""
import numpy as np
import pytest
import torch

from pccx import meshes, ops
from tests import mesh_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 255, 257, 8192)
SEEDS = [11, 2**63 + 5, 0, 2**64 - 1, 0x299f31d0a4093822, 77, 78, 79, 80]          # one 64-bit stream per mesh of the batch


def to_dev(ms):
    return [torch.from_numpy(a).to(DEV) for a in mc.pack(ms)]


def u32(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t, dtype=np.float32)).view(np.uint32)


@pytest.fixture(scope="module")
def batch():
    return mc.batch()


@pytest.fixture(scope="module")
def want(batch):
    """the restatement's clouds: {(n, normalize): [(points, status, picked), ...]}, computed once"""
    return {(n, norm): [mc.sample(V, F, s, n, norm) for (V, F, _), s in zip(batch, SEEDS)] for n in NS for norm in (None, "unit")}


def test_w1_weights_and_prefix(batch):
    verts, faces, v_off, f_off = to_dev(batch)
    Ft = faces.shape[0]
    ws = torch.empty(ops.mesh_sample_workspace_bytes(len(batch), Ft, 1), dtype=torch.uint8, device=DEV)
    meshes.sample_meshes(verts, faces, v_off, f_off, 1, SEEDS, workspace=ws)
    host = ws.cpu().numpy()
    a, w, I = host[:8 * Ft].view(np.float64), host[8 * Ft:16 * Ft].view(np.uint64), host[16 * Ft:24 * Ft].view(np.uint64)
    at = 0
    for V, F, kind in batch:
        ra, rw, rI, status = mc.weights(V, F)
        assert status == 0
        sl = slice(at, at + len(F))
        bad = np.flatnonzero(a[sl].view(np.uint64) != ra.view(np.uint64))
        print(kind, len(F), "areas differing:", len(bad), "weights differing:", int((w[sl] != rw).sum()))
        assert len(bad) == 0, (kind, len(F), bad[:5], a[sl][bad[:5]], ra[bad[:5]])
        assert (w[sl] == rw).all() and (I[sl] == rI).all(), (kind, len(F))
        if kind == "giant":
            assert int((rw > 0).sum()) == 1 and int(rI[-1]) == 2**40
        if kind == "zero_ends":
            assert rw[0] == 0 and rw[-1] == 0
        at += len(F)


@pytest.mark.parametrize("n", NS)
def test_w2_samples_equal_the_restatement(batch, want, n):
    verts, faces, v_off, f_off = to_dev(batch)
    for norm in (None, "unit"):
        pts, status = meshes.sample_meshes(verts, faces, v_off, f_off, n, SEEDS, normalize=norm)
        assert pts.shape == (len(batch), n, 3) and status.tolist() == [0] * len(batch)
        got = u32(pts)
        for b, (V, F, kind) in enumerate(batch):
            p, s, t = want[(n, norm)][b]
            diff = int((got[b] != u32(p)).sum())
            print(kind, len(F), n, norm, "words differing:", diff)
            assert diff == 0, (kind, len(F), n, norm)
            if norm == "unit" and n > 1:
                assert got[b].view(np.float32).min() == 0 and got[b].view(np.float32).max() == 1
    # the picks, recovered by the restatement's own pick: only faces with area, both copies of a doubled face, the giant alone
    if n == 8192:
        for b, (V, F, kind) in enumerate(batch):
            t = want[(n, None)][b][2]
            assert (mc.weights(V, F)[1][t] > 0).all()
            if kind == "zero_ends":
                assert 0 not in t and len(F) - 1 not in t
            if kind == "giant":
                assert (t == len(F) // 2).all()
            if kind == "doubled":
                half = len(F) // 2
                assert (t < half).any() and (t >= half).any()


def test_w3_a_sample_depends_on_mesh_seed_and_index_alone(batch, want):
    k = 4                                                                        # the 257-face mesh
    six = batch[:6]
    alone, _ = meshes.sample_meshes(*to_dev([batch[k]]), 255, [SEEDS[k]], normalize=None)
    first, _ = meshes.sample_meshes(*to_dev([batch[k]] + six[:5]), 255, [SEEDS[k]] + SEEDS[:5], normalize=None)
    last, _ = meshes.sample_meshes(*to_dev(six[:5] + [batch[k]]), 255, SEEDS[:5] + [SEEDS[k]], normalize=None)
    long, _ = meshes.sample_meshes(*to_dev([batch[k]]), 8192, [SEEDS[k]], normalize=None)
    assert (u32(alone[0]) == u32(first[0])).all() and (u32(alone[0]) == u32(last[5])).all()
    assert (u32(alone[0]) == u32(long[0, :255])).all()
    assert (u32(long[0]) == u32(want[(8192, None)][k][0])).all()


def test_w4_statuses(batch):
    line = mc.mesh(5, 40, "collinear")
    assert mc.weights(*line)[3] == 1
    # status 2 is reachable: a triangle one ulp wide beside the diagonal, one sample that rounds onto (1, 1, 1)
    e = np.float32(1) + np.finfo(np.float32).eps
    tiny = (np.array([[1, 1, 1], [e, 1, 1], [1, e, 1]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32))
    seed2 = next(s for s in range(64) if mc.sample(*tiny, s, 1)[1] == 2)
    seed0 = next(s for s in range(64) if mc.sample(*tiny, s, 1)[1] == 0)
    ms = [batch[2], line + ("collinear",), batch[3], tiny + ("tiny",), tiny + ("tiny",), batch[1]]
    seeds = [SEEDS[2], 5, SEEDS[3], seed2, seed0, SEEDS[1]]
    for n in (1, 257):
        pts, status = meshes.sample_meshes(*to_dev(ms), n, seeds)
        refs = [mc.sample(V, F, s, n) for (V, F, _), s in zip(ms, seeds)]
        assert status.tolist() == [r[1] for r in refs]
        assert status.tolist()[:3] == [0, 1, 0] and (n != 1 or status.tolist()[3:5] == [2, 0])
        got = u32(pts)
        assert (got[1] == 0x7FC00000).all()                                      # NaN rows, the quiet NaN of codec.pad_clouds
        for b, r in enumerate(refs):
            assert (got[b] == u32(r[0])).all(), (n, b)


def test_w5_nothing_is_written_outside_output_and_workspace(batch):
    verts, faces, v_off, f_off = to_dev(batch)
    B, n, guard = len(batch), 257, 3 * 64
    need = ops.mesh_sample_workspace_bytes(B, faces.shape[0], n)
    big = torch.full((B * n * 3 + 2 * guard,), -7.5, dtype=torch.float32, device=DEV)
    ws = torch.full((need + 2 * 256,), 0xA5, dtype=torch.uint8, device=DEV)
    seeds = torch.from_numpy(np.array(SEEDS, dtype=np.uint64).view(np.int64)).to(DEV)
    out = big[guard:guard + B * n * 3].view(B, n, 3)
    for norm in (False, True):
        pts, status = ops.mesh_sample(verts, faces, v_off, f_off, seeds, n, norm, out=out, workspace=ws[256:256 + need])
        assert pts.data_ptr() == out.data_ptr() and status.tolist() == [0] * B
        assert (big[:guard] == -7.5).all() and (big[-guard:] == -7.5).all()
        assert (ws[:256] == 0xA5).all() and (ws[256 + need:] == 0xA5).all()
    assert (u32(out[4]) == u32(mc.sample(batch[4][0], batch[4][1], SEEDS[4], n)[0])).all()
    with pytest.raises(Exception, match="workspace"):
        ops.mesh_sample(verts, faces, v_off, f_off, seeds, n, True, workspace=ws[256:256 + need - 8])
