"""GPU: pccx_fps_blocks (csrc/geometry.hip, fps_blocks_kernel) -- an independent farthest point sampling in every run of a cloud's
Morton order, all runs in one launch -- and what stands on it: ops.farthest_point_sample_blocks, Codec(centres="blocks") and
compress.py --centres blocks.

The kernel's definition is restated below in numpy float32 (elementwise operations, so nothing is contracted; np.minimum; np.argmax
returns the FIRST maximum = the lower local index).  The permutation comes from large.morton_order, which has its own tests
(tests/test_gpu_geometry.py).  Indices are compared exactly.  Downstream of the centres the codec is unchanged, so the files are
checked the way tests/test_codec_whole_cloud.py checks them: .s.bin against the oracle's octree coder on the chosen centres, the
reconstruction against the oracle's decoder at 2e-5 of the longest side, and a default Codec reads what centres="blocks" wrote."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cport, ref_model, ref_pipeline
from pccx import _lib, codec, dist, large, models, ops, plyio, synth as cloud_synth
from pccx import torch_ops  # noqa: F401  (registers torch.ops.pccx.*)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "point-cloud-compression_amd", "cli")
MODES = ["f32", "bf16x3", "f16x2"]
K, D, L = 256, 16, 7


def blocks_definition(xyz, order, P, npoint, start):
    """include/pccx.h, pccx_fps_blocks, for one cloud: xyz (N,3) f32, order (N,) i64 -> (npoint,) i64."""
    N = xyz.shape[0]
    out = np.full(npoint, -1, dtype=np.int64)
    for j in range(P):
        lo, hi, o0, o1 = j * N // P, (j + 1) * N // P, j * npoint // P, (j + 1) * npoint // P
        pts = xyz[order[lo:hi]]
        n = hi - lo
        far = (start if 0 <= start < N else 0) % n
        md = np.full(n, np.float32(1e10), dtype=np.float32)
        for t in range(o1 - o0):
            out[o0 + t] = order[lo + far]
            dx, dy, dz = pts[:, 0] - pts[far, 0], pts[:, 1] - pts[far, 1], pts[:, 2] - pts[far, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            md = np.minimum(md, d)
            far = int(np.argmax(md))
    return out


def _orders(x):
    return torch.stack([large.morton_order(c) for c in x])


def _check(clouds, npoint, starts, block):
    x = torch.from_numpy(np.ascontiguousarray(clouds, dtype=np.float32)).cuda()
    B, N, _ = x.shape
    P = ops.fps_block_plan(N, npoint, block)[0]
    order = _orders(x)
    assert all(torch.equal(torch.sort(order[b]).values, torch.arange(N, device="cuda")) for b in range(B))
    got = ops.farthest_point_sample_blocks(x, npoint, np.array(starts), block=block, order=order)
    assert got.shape == (B, npoint) and got.dtype == torch.int64
    want = np.stack([blocks_definition(clouds[b], order[b].cpu().numpy(), P, npoint, int(starts[b])) for b in range(B)])
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(ops.farthest_point_sample_blocks(x, npoint, np.array(starts), block=block), got)     # the default permutation
    assert torch.equal(torch.ops.pccx.fps_blocks(x, npoint, torch.as_tensor(starts).cuda(), block), got)    # ... and the registered op
    return got, P


def _lattice(seed, n, side):
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return g[np.random.default_rng(seed).permutation(side ** 3)[:n]].astype(np.float32)


def _duplicated(seed, n):
    base = cloud_synth.cad_cloud(seed, n // 2)
    pts = np.concatenate([base, base, base[:n - 2 * (n // 2)]])
    return pts[np.random.default_rng(seed).permutation(n)]


def test_ragged_blocks_smallest_template_ties_and_duplicates():
    N, S = 4099, 37
    clouds = np.stack([cloud_synth.cad_cloud(31, N), _lattice(32, N, 17), _duplicated(33, N)])
    got, P = _check(clouds, S, [0, N - 1, 2500], 1024)
    assert P == 5
    for b in range(2):                                          # distinct points: distinct centres (cloud 2 holds every point twice)
        assert got[b].unique().numel() == S
    assert np.unique(clouds[2][got[2].cpu().numpy()], axis=0).shape[0] == S


def test_largest_template_sixteen_points_per_thread():
    N, S = 32763, 33                                            # blocks of 16381 and 16382 points: 16 per thread in the last row of the second
    got, P = _check(cloud_synth.cad_batch(34, 1, N), S, [N - 1], 16384)
    assert P == 2 and got.unique().numel() == S


def test_whole_room_shape():
    N, S = 132096, 1032                                         # 17 blocks of 7770 / 7771 points, 60 / 61 centres each
    got, P = _check(cloud_synth.cad_batch(35, 1, N), S, [70001], 8192)
    assert P == 17 and got.unique().numel() == S


def test_start_index_out_of_range_and_none_start_from_zero():
    N, S = 4099, 37
    clouds = cloud_synth.cad_batch(36, 2, N)
    x = torch.from_numpy(clouds).cuda()
    zero = ops.farthest_point_sample_blocks(x, S, np.array([0, 0]), block=1024)
    assert torch.equal(ops.farthest_point_sample_blocks(x, S, np.array([N, -3]), block=1024), zero)
    assert torch.equal(ops.farthest_point_sample_blocks(x, S, "zero", block=1024), zero)


def test_against_the_existing_kernel_block_by_block():
    N, S, block, start = 4 * 2048, 4 * 16, 2048, 5000
    x = torch.from_numpy(cloud_synth.cad_batch(37, 1, N)).cuda()
    order = large.morton_order(x[0])
    sorted_blocks = x[0][order].view(4, 2048, 3).contiguous()
    local = ops.farthest_point_sample_batch(sorted_blocks, 16, np.array([start % 2048] * 4))
    want = order.view(4, 2048).gather(1, local).view(1, S)
    assert torch.equal(ops.farthest_point_sample_blocks(x, S, np.array([start]), block=block), want)


def _nets():
    ae = models.AE(K, K // 2, D, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, 3, last_gain={"pn.mlp_Modules.3.0": 40.0}))
    prob = models.ConditionalProbabilityModel(L, D)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, 4, gain=2.0))
    return ae, prob


@pytest.fixture(scope="module")
def nets():
    ae, prob = _nets()
    oae = ref_model.AE(K, K // 2, D, L).eval()
    oae.load_state_dict(ae.state_dict())
    oprob = ref_model.ConditionalProbabilityModel(L, D).eval()
    oprob.load_state_dict(prob.state_dict())
    return dict(ae=ae.pack("cuda"), prob=prob.pack("cuda"), oae=oae, oprob=oprob)


def test_one_block_is_the_exact_sampling(nets):
    N, S = 2048, 16
    pc = torch.from_numpy(cloud_synth.cad_batch(38, 2, N)).cuda()
    starts = np.array([7, N - 1])
    assert torch.equal(ops.farthest_point_sample_blocks(pc, S, starts, block=2048), ops.farthest_point_sample_batch(pc, S, starts))
    a = codec.Codec(nets["ae"], nets["prob"], K=K, octree_mode="full", centres="blocks", fps_block=2048).compress(pc, starts)
    b = codec.Codec(nets["ae"], nets["prob"], K=K, octree_mode="full", centres="fps").compress(pc, starts)
    for i in range(2):
        assert a.files(i) == b.files(i)


def test_abi_refusals_leave_the_output_untouched():
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(cloud_synth.cad_batch(39, 1, 16385)).cuda()
    order = torch.arange(16385, device="cuda").view(1, -1)
    out = torch.full((1, 4096), -1, device="cuda", dtype=torch.int64)
    for N, P, npoint, word in ((16385, 1, 64, b"16384"),        # a block over 16384 points
                               (4096, 4, 3, b"without a centre"),   # a quota of 0
                               (2050, 3, 2050, b"cannot give"),     # a quota of 684 in a block of 683 points
                               (4096, 0, 32, b"P >= 1")):
        rc = lib.pccx_fps_blocks(x.data_ptr(), 1, N, order.data_ptr(), P, npoint, None, out.data_ptr(), st)
        assert rc == -1 and word in lib.pccx_last_error(), (N, P, npoint, lib.pccx_last_error())
    torch.cuda.synchronize()
    assert bool((out == -1).all())


def test_an_order_entry_out_of_range_is_clamped():
    N, S = 4099, 37
    x = torch.from_numpy(cloud_synth.cad_batch(40, 1, N)).cuda()
    order = _orders(x)
    bad = order.clone()
    at_last, at_first = (order[0] == N - 1).nonzero().item(), (order[0] == 0).nonzero().item()
    bad[0, at_last], bad[0, at_first] = 2 ** 40, -5                      # clamped to N - 1 and to 0: the permutation itself
    assert torch.equal(ops.farthest_point_sample_blocks(x, S, np.array([1]), block=1024, order=bad),
                       ops.farthest_point_sample_blocks(x, S, np.array([1]), block=1024, order=order))


@pytest.mark.parametrize("matmul", MODES)
def test_codec_end_to_end(nets, matmul):
    N, S, B = 4096, 32, 2
    clouds = cloud_synth.cad_batch(41, B, N) * np.float32(2.5)
    pc = torch.from_numpy(clouds).cuda()
    starts = np.array([3, N - 2])
    cd = codec.Codec(nets["ae"], nets["prob"], K=K, octree_mode="full", matmul=matmul, centres="blocks", fps_block=1024)
    comp = cd.compress(pc, starts, keep_extras=True)
    ex = comp.extras
    assert torch.equal(ex["fps_idx"], ops.farthest_point_sample_blocks(ex["pcn"], S, starts, block=1024))
    assert not torch.equal(ex["fps_idx"], ops.farthest_point_sample_batch(ex["pcn"], S, starts))     # four blocks: other centres
    plain = cd.compress(pc, starts)
    reader = codec.Codec(nets["ae"], nets["prob"], K=K, octree_mode="full", matmul=matmul)           # no `centres`: the decoder needs none
    out = reader.decompress(codec.Compressed.from_packed(comp.packed.clone(), B, comp.s_bytes.shape[1], comp.p_bytes.shape[1], N), S=S)
    assert torch.equal(out, cd.decompress(comp, S=S))
    pcn, idx = ex["pcn"].cpu().numpy(), ex["fps_idx"].cpu().numpy()
    codes, _ = cport.encode_sampled_np(np.stack([pcn[b][idx[b]] for b in range(B)]), 1, N, ref_model.OCTREE_BPP_DICT[K])
    for b in range(B):
        s, p, c = comp.files(b)
        assert (s, p, c) == plain.files(b)
        assert s == bytes(cport.pack_bits(codes[b]))
        q = ex["latent_q"].view(B, S, D)[b].cpu().numpy()
        want, _ = ref_pipeline.decompress_one(s, p, c, nets["oae"], nets["oprob"], octree_mode="full", latent_q_override=q.copy())
        got = out[b].cpu().numpy()
        assert got.shape == want.shape == (S * K // 2, 3)
        print(f"{matmul} cloud {b}: max |recon - oracle| / longest =", float(np.abs(got - want).max()) / float(comp.c[b, 3]))
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5 * float(comp.c[b, 3]))


def test_above_1024_centres_with_the_split_stream_and_region_decode(nets):
    N, S = 132096, 1032
    pc = torch.from_numpy(cloud_synth.cad_batch(42, 1, N)).cuda()
    cd = codec.Codec(nets["ae"], nets["prob"], K=K, octree_mode="full", max_centres=8192, p_split=64, centres="blocks")
    comp = cd.compress(pc, np.array([9]), keep_extras=True)
    idx = comp.extras["fps_idx"]
    assert idx.shape == (1, S) and idx.unique().numel() == S and int(idx.min()) >= 0 and int(idx.max()) < N
    assert torch.equal(idx, ops.farthest_point_sample_blocks(comp.extras["pcn"], S, np.array([9]), block=8192))
    out = cd.decompress(comp, S=S)
    assert out.shape == (1, S * K // 2, 3) and bool(torch.isfinite(out).all())
    w = ops.denormalize(comp.extras["rec_sampled"], comp.c[:, :3].contiguous(), comp.c[:, 3].contiguous(), cd.margin)
    reg = cd.decompress_region(comp, S, (w[0].amin(dim=0).tolist(), w[0].amax(dim=0).tolist()))
    assert torch.equal(reg.patch_idx, torch.arange(S, device="cuda")) and torch.equal(reg.points, out[0])


def test_cli_centres_blocks_round_trip(nets, tmp_path):
    N, S = 4096, 32
    data, mdl, comp, dec = (tmp_path / n for n in ("data", "model", "comp", "dec"))
    data.mkdir(), mdl.mkdir()
    names = ["a.ply", "b.ply"]
    for i, n in enumerate(names):
        plyio.save_point_cloud(cloud_synth.cad_cloud(80 + i, N) * np.float32(2.0), str(data / n))
    ae, prob = _nets()
    torch.save(ae.state_dict(), str(mdl / "ae.pkl"))
    torch.save(prob.state_dict(), str(mdl / "prob.pkl"))
    run = lambda *a: subprocess.run([sys.executable, *a], capture_output=True, text=True, timeout=600)
    r = run(os.path.join(CLI, "compress.py"), str(data / "*.ply"), str(comp), str(mdl), "--octree-mode", "full", "--centres", "blocks", "--fps-block", "1024")
    assert r.returncode == 0 and "Execution time" in r.stdout, r.stderr[-2000:]
    r = run(os.path.join(CLI, "decompress.py"), str(comp), str(dec), str(mdl), "--octree-mode", "full")       # no new flag on this side
    assert r.returncode == 0 and "Execution time" in r.stdout, r.stderr[-2000:]
    cd = codec.Codec(nets["ae"], nets["prob"], K=K, octree_mode="full", max_centres=codec.OCTREE_WIDE_MAX_S, centres="blocks", fps_block=1024)
    pc = torch.from_numpy(np.stack([plyio.read_point_cloud(str(data / n)) for n in names])).cuda()
    c = cd.compress(pc, [dist.fps_start_index(11, i, N) for i in range(2)])
    out = cd.decompress(c, S=S).cpu().numpy()
    for b, n in enumerate(names):
        s, p, cc = c.files(b)
        assert [open(comp / (n + e), "rb").read() for e in (".s.bin", ".p.bin", ".c.bin")] == [s, p, cc]
        back = plyio.read_point_cloud(str(dec / n))
        assert back.shape == (S * K // 2, 3) and np.array_equal(back, out[b])
