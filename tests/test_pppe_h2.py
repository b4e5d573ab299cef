"""The pppe PointCloudAE forward on f16x2 planes stacks (families.PointCloudAE._forward_h2) against the float64 oracle: the centred
operand kernel (pccx_group_planes_centred / _h2) with one layer, the forward at the smallest shapes that take every branch, its
dynamic range, its reproducibility on dirtied memory, and the other arithmetic modes left as they were."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import ref_families as rf
from tests import synth

pytestmark = pytest.mark.gpu

# Seeds of the two forward cases (weights, cloud, FPS starts).  Checked on the CPU with the float64 oracle alone: the share of latents
# within 1e-3 of a rounding boundary is 0 / 64 for (N=512, B=1) and 0 / 192 for (N=640, B=3) -- under the 2 % the symbols test excuses.
CASES = {512: dict(B=1, seed=41), 640: dict(B=3, seed=42)}


@contextlib.contextmanager
def matmul(mode):
    import pccx
    old = pccx.DEFAULT_MATMUL
    pccx.DEFAULT_MATMUL = mode
    try:
        yield
    finally:
        pccx.DEFAULT_MATMUL = old


@contextlib.contextmanager
def h2_stacks(on):
    from pccx import families
    old = families.PointCloudAE.h2_stacks
    families.PointCloudAE.h2_stacks = on
    try:
        yield
    finally:
        families.PointCloudAE.h2_stacks = old


def _case(N):
    """oracle module (float32 weights), cloud (B, N, 3) float32 and FPS starts of one forward case"""
    B, seed = CASES[N]["B"], CASES[N]["seed"]
    p = rf.PointCloudAE(64, 16, N).eval()
    p.load_state_dict(synth.family_tweak(rf.seeded_with_bn(p, seed), "pppe"))
    x = np.stack([synth.cloud_synth.cad_cloud(seed + 100 + b, N) for b in range(B)]).astype(np.float32)
    rng = np.random.default_rng(seed)
    starts = [[rng.integers(0, N, B), rng.integers(0, N, B)], rng.integers(0, 512, B), rng.integers(0, 128, B)]
    return p, x, starts


def _oracle64(p, x, starts):
    """the oracle in float64 on the float32 cloud x: (coarse, fine, cond, y_q, latent) as numpy float64"""
    import copy
    q = copy.deepcopy(p).double()
    with torch.no_grad():
        return [t.numpy() for t in q(torch.from_numpy(x).double(), starts)]


_CACHE = {}


def _setup(N):
    """(our model with the oracle's weights, cloud on the GPU, starts, float64 oracle outputs), built once per case"""
    if N not in _CACHE:
        from pccx import families
        p, x, starts = _case(N)
        g = families.PointCloudAE(64, 16, N)
        g.load_state_dict(p.state_dict())
        _CACHE[N] = (g, p, x, starts, _oracle64(p, x, starts))
    return _CACHE[N]


def _near_boundary(pre, tol):
    return np.abs(pre - np.floor(pre) - 0.5) < tol


@pytest.mark.parametrize("B,Nsrc,S,K,C", [(2, 40, 5, 3, 0), (2, 40, 5, 3, 5), (2, 40, 5, 3, 192),
                                          (3, 40, 9, 5, 5),          # 135 rows: not a multiple of 128
                                          (1, 40, 1, 1, 5)])         # a single row
def test_centred_operand_planes_and_one_layer_against_float64(B, Nsrc, S, K, C):
    """[xyz[idx] - centre | feats[idx]] (pppe_pcd_ae.py:599-606) -> planes -> one layer -> rows, in bf16x3 and f16x2, against
    W [centred | feats] + b in float64 at the tolerances of test_generic_linear_ragged_shapes; the folded |offset| maximum is exact."""
    from pccx import families, ops
    rng = np.random.default_rng(1000 + 7 * C + S)
    xyz = rng.uniform(-1, 1, (B, Nsrc, 3)).astype(np.float32)
    feats = rng.uniform(0, 1, (B, Nsrc, C)).astype(np.float32) if C else None
    centres = xyz[:, :S].copy()
    xg, cg = torch.from_numpy(xyz).cuda(), torch.from_numpy(centres).cuda()
    fg = torch.from_numpy(feats).cuda() if C else None
    nn_ = ops.knn_points(cg, xg, K, patch_scale=1.0)
    idx, off = nn_.idx.cpu().numpy(), nn_.knn.cpu().numpy()
    bi = np.arange(B)[:, None, None]
    assert np.array_equal(off, xyz[bi, idx] - centres[:, :, None, :])                # the one fp32 subtraction of the rows path
    rows64 = np.concatenate([off] + ([feats[bi, idx]] if C else []), axis=-1).astype(np.float64).reshape(B * S * K, 3 + C)
    N_out = 70
    W = (rng.standard_normal((N_out, 3 + C)) / np.sqrt(3 + C)).astype(np.float32)   # columns in the reference's order: xyz first
    b = rng.standard_normal(N_out).astype(np.float32)
    want = np.maximum(rows64 @ W.T.astype(np.float64) + b, 0)
    Wp = np.concatenate([W[:, 3:], W[:, :3]], axis=1)                                # the planes are features first
    for ar in ("bf16x3", "f16x2"):
        lyr = families.FoldedLinear(torch.from_numpy(Wp), torch.from_numpy(b), True, matmul=ar)
        sig = None
        if ar == "f16x2":                                                            # offsets of points in [-1, 1]^3 lie within [-2, 2]
            families.h2_prepare_stack([lyr], np.concatenate([np.zeros(C), -2 * np.ones(3)]), np.concatenate([np.ones(C), 2 * np.ones(3)]))
            sig = lyr.h2["sig"]
        amax = torch.zeros(8, device="cuda")
        pl, rows = families.group_planes_centred(nn_.knn, fg, nn_.idx, ar, sig=sig, amax=amax)
        assert rows == B * S * K
        got = lyr.planes(pl, rows, 1, ar=ar).cpu().numpy()
        np.testing.assert_allclose(got, want, atol=2e-5, rtol=1e-5, err_msg=ar)
        assert float(amax.max()) == float(np.abs(off).max())


@pytest.mark.parametrize("N", [512, 640])
def test_forward_f16x2_matches_the_float64_oracle(N):
    """N = 512, B = 1: level 0 keeps every point (S == N, no FPS).  N = 640, B = 3: the FPS branch at every level, and dense stacks on three
    rows.  (The set-abstraction stacks' row counts B * S * K are multiples of the GEMM's 128-row tile for every B -- S * K is 8192, 16384,
    4096 and 1024 by construction; the ragged row counts are the operand test's.)"""
    g, p, x, starts, (oc, of, ocond, oyq, olat) = _setup(N)
    with matmul("f16x2"), h2_stacks(True):
        coarse, fine, cond, yq, latent = [t.cpu().numpy() for t in g(torch.from_numpy(x).cuda(), starts)]
    assert "h2" in g._packed
    np.testing.assert_allclose(cond, ocond, atol=2e-5, rtol=1e-4)
    np.testing.assert_allclose(latent, olat, atol=2e-4, rtol=1e-4)
    near = _near_boundary(np.clip(olat, 0, 15), 1e-3)
    assert near.mean() <= 0.02
    assert near[yq != oyq].all()                            # with the seeds above no latent is near a boundary: every symbol is equal
    np.testing.assert_allclose(coarse, oc, atol=5e-5, rtol=1e-4)
    np.testing.assert_allclose(fine, of, atol=5e-5, rtol=1e-4)


@pytest.mark.parametrize("scale", [2.0 ** 10, 2.0 ** -10])
def test_forward_f16x2_dynamic_range(scale):
    """The N = 640 cloud times 2^10 and 2^-10 (the selection is unchanged by a power of two): cond stays within rtol 1e-4 of the float64
    oracle of THAT input -- the per-stack normalisation comes from the data."""
    g, p, x, starts, _ = _setup(640)
    xs = (x * np.float32(scale)).astype(np.float32)
    ocond = _oracle64(p, xs, starts)[2]
    with matmul("f16x2"), h2_stacks(True):
        cond = g(torch.from_numpy(xs).cuda(), starts)[2].cpu().numpy()
    np.testing.assert_allclose(cond, ocond, atol=2e-5 * float(np.abs(ocond).max()), rtol=1e-4)


def test_forward_f16x2_reproducible_on_dirtied_memory():
    """The same forward twice with the allocator's free memory filled with 0xFF bytes in between: identical outputs (nothing reads a
    plane, a pad channel or a slot it did not write)."""
    g, p, x, starts, _ = _setup(640)
    xg = torch.from_numpy(x).cuda()
    with matmul("f16x2"), h2_stacks(True):
        a = [t.clone() for t in g(xg, starts)]
        torch.cuda.synchronize()
        dirt = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")          # larger than every activation of the call (< 40 MB)
        dirt.fill_(0xFF)
        del dirt
        torch.cuda.synchronize()
        b = g(xg, starts)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_other_modes_are_untouched():
    """f32 and bf16x3: the switch changes nothing.  f16x2 with the switch off: the bf16x3 rows path, bit for bit."""
    g, p, x, starts, _ = _setup(640)
    xg = torch.from_numpy(x).cuda()
    res = {}
    for mode in ("f32", "bf16x3"):
        with matmul(mode):
            with h2_stacks(True):
                on = g(xg, starts)
            with h2_stacks(False):
                off = g(xg, starts)
        for u, v in zip(on, off):
            assert torch.equal(u, v)
        res[mode] = off
    with matmul("f16x2"), h2_stacks(False):
        off = g(xg, starts)
    for u, v in zip(off, res["bf16x3"]):
        assert torch.equal(u, v)


def test_auto_switch_picks_the_path_by_the_number_of_input_points():
    """h2_stacks = "auto" (the default): below h2_min_points input points the rows path, from there on the planes path -- each bit for
    bit what the forced switch gives."""
    from pccx import families
    assert families.PointCloudAE.h2_stacks == "auto"
    g, p, x, starts, _ = _setup(640)
    xg = torch.from_numpy(x).cuda()
    with matmul("f16x2"):
        with h2_stacks(True):
            on = g(xg, starts)
        with h2_stacks(False):
            off = g(xg, starts)
        assert not torch.equal(on[4], off[4])               # two arithmetics: the latents differ in their last bits
        assert x.shape[0] * x.shape[1] < families.PointCloudAE.h2_min_points
        small = g(xg, starts)
        old = families.PointCloudAE.h2_min_points
        families.PointCloudAE.h2_min_points = x.shape[0] * x.shape[1]
        try:
            large = g(xg, starts)
        finally:
            families.PointCloudAE.h2_min_points = old
    for u, v, w, z in zip(small, off, large, on):
        assert torch.equal(u, v) and torch.equal(w, z)
