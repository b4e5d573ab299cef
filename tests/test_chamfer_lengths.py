"""GPU: nearest-neighbour distance and chamfer_distance over ragged batches (pytorch3d's x_lengths / y_lengths).

Cloud b is the first lengths[b] rows of its slab; everything behind them is NaN here (codec.pad_clouds), so a kernel that lets a
padded row reach a minimum, a mean or a gradient shows it.  Bars are the dense tests' own (tests/test_gpu_geometry.py): bit-exact
against the oracle for the search, 1e-6 relative for the value (fp64 means of identical fp32 terms), rtol 1e-4 / atol 1e-9 for the
gradients (fp32 atomics against an fp64 sum)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cport
from pccx import _lib, ops
from pccx.codec import pad_clouds

pytestmark = pytest.mark.gpu
COMPAT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "point-cloud-compression_amd", "compat")


def _ragged(rng, lens, cap, lattice=None):
    """clouds of `lens` points in [0,1)^3 (cloud `lattice` snapped to multiples of 1/4) -> (list of arrays, the (B, cap, 3) device
    tensor of pad_clouds: NaN behind each cloud)"""
    clouds = [rng.random((n, 3)).astype(np.float32) for n in lens]
    if lattice is not None:
        clouds[lattice] = np.round(clouds[lattice] * 4) / 4
    pc, n = pad_clouds(clouds, device="cuda")
    assert pc.shape[1] == cap and n == list(lens) and bool(torch.isnan(pc).any())
    return clouds, pc


def test_nn_dist_n_is_nn_dist_on_the_unpadded_clouds_bit_for_bit():
    """Capacities one past two tiles of queries and of references; lengths of 1, of the capacity, at and around the 1024 tile; one
    cloud on a 1/4 lattice so that equal distances occur and the first minimum has to win.  One query per thread (B = 5)."""
    lens = [(1, 5), (2049, 1), (1024, 1025), (1023, 2050), (257, 1024)]
    rng = np.random.default_rng(2049)
    xs, x = _ragged(rng, [p for p, _ in lens], 2049)
    ys, y = _ragged(rng, [q for _, q in lens], 2050, lattice=3)
    p, q = [p for p, _ in lens], [q for _, q in lens]
    d2, nn = ops.nn_dist_n(x, y, p, q, return_idx=True)
    only = ops.nn_dist_n(x, y, torch.tensor(p, dtype=torch.int32).cuda(), torch.tensor(q).cuda())     # no argmin; device lengths
    ties = 0
    for b, (pb, qb) in enumerate(lens):
        d, i = cport.nn_dist(xs[b], ys[b])
        assert np.array_equal(d2[b, :pb].cpu().numpy(), d), b
        assert np.array_equal(nn[b, :pb].cpu().numpy(), i), b
        assert np.array_equal(only[b, :pb].cpu().numpy(), d), b
        dd = ((xs[b][:64, None, :] - ys[b][None, :, :]) ** 2).sum(-1)
        ties += int(((dd == dd.min(1, keepdims=True)).sum(1) > 1).sum())
    assert ties > 0                                                 # the lattice cloud really has equal minima


def test_nn_dist_n_four_queries_per_thread_equals_nn_dist_per_cloud():
    """B = 520 clouds of capacity 1000 x 300: the launch that keeps four queries per thread.  Random lengths, the extremes included."""
    rng = np.random.default_rng(520)
    B, P, Q = 520, 1000, 300
    p, q = rng.integers(1, P + 1, B), rng.integers(1, Q + 1, B)
    p[:4], q[:4] = (1, P, 256, 257), (Q, 1, 2, Q)
    x = torch.full((B, P, 3), float("nan"))
    y = torch.full((B, Q, 3), float("nan"))
    for b in range(B):
        x[b, :p[b]] = torch.from_numpy(rng.random((p[b], 3)).astype(np.float32))
        y[b, :q[b]] = torch.from_numpy(rng.random((q[b], 3)).astype(np.float32))
    x, y = x.cuda(), y.cuda()
    d2, nn = ops.nn_dist_n(x, y, p.tolist(), q.tolist(), return_idx=True)
    for b in list(range(8)) + list(range(8, B, 37)) + [B - 1]:
        d, i = ops.nn_dist(x[b:b + 1, :p[b]], y[b:b + 1, :q[b]], return_idx=True)
        assert torch.equal(d2[b, :p[b]], d[0]) and torch.equal(nn[b, :p[b]], i[0]), b
    assert bool(torch.isfinite(torch.cat([d2[b, :p[b]] for b in range(B)])).all())


def _definition(xs, ys, scale=3.0):
    """float64 autograd of the definition over the unpadded clouds: (value, per-cloud values, grads of x, grads of y)"""
    xr = [torch.from_numpy(c).double().requires_grad_(True) for c in xs]
    yr = [torch.from_numpy(c).double().requires_grad_(True) for c in ys]
    per = []
    for a, b in zip(xr, yr):
        d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        per.append(d.min(1).values.mean() + d.min(0).values.mean())
    ref = torch.stack(per).mean()
    (ref * scale).backward()
    return float(ref.detach()), [float(v.detach()) for v in per], [a.grad.numpy() for a in xr], [b.grad.numpy() for b in yr]


@pytest.mark.parametrize("lens,cap", [(((300, 500), (1, 7), (2048, 2048)), (2048, 2048)),
                                      (((2050, 3), (1025, 1024)), (2050, 1024))])
def test_chamfer_by_length_matches_autograd_of_the_definition(lens, cap):
    rng = np.random.default_rng(sum(p * 7 + q for p, q in lens))
    xs, x = _ragged(rng, [p for p, _ in lens], cap[0])
    ys, y = _ragged(rng, [q for _, q in lens], cap[1])
    p, q = [p for p, _ in lens], [q for _, q in lens]
    want, want_per, gxr, gyr = _definition(xs, ys)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    loss, none = ops.chamfer_distance(xg, yg, x_lengths=p, y_lengths=q)
    (loss * 3.0).backward()
    assert none is None and abs(float(loss.detach()) - want) <= 1e-6 * want
    gx, gy = xg.grad.cpu().numpy(), yg.grad.cpu().numpy()
    assert np.isfinite(gx).all() and np.isfinite(gy).all()
    for b, (pb, qb) in enumerate(lens):
        np.testing.assert_allclose(gx[b, :pb], gxr[b], rtol=1e-4, atol=1e-9)
        np.testing.assert_allclose(gy[b, :qb], gyr[b], rtol=1e-4, atol=1e-9)
        assert not gx[b, pb:].any() and not gy[b, qb:].any()       # behind the lengths: exact zeros
    # the other reductions, without a graph; lengths as device tensors
    pd, qd = torch.tensor(p, dtype=torch.int32).cuda(), torch.tensor(q, dtype=torch.int64).cuda()
    per, _ = ops.chamfer_distance(x, y, x_lengths=pd, y_lengths=qd, batch_reduction=None)
    assert per.shape == (len(lens),)
    np.testing.assert_allclose(per.cpu().numpy(), want_per, rtol=1e-6)
    tot, _ = ops.chamfer_distance(x, y, x_lengths=pd, y_lengths=qd, batch_reduction="sum")
    assert abs(float(tot) - sum(want_per)) <= 1e-6 * sum(want_per)
    val, _ = ops.chamfer_distance(x, y, x_lengths=p, y_lengths=q)
    assert float(val) == float(loss.detach())
    # the drop-in surface: pytorch3d's own keyword names
    if COMPAT not in sys.path:
        sys.path.insert(0, COMPAT)
    from pytorch3d.loss import chamfer_distance
    xc, yc = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    l2, _ = chamfer_distance(xc, yc, x_lengths=pd, y_lengths=qd)
    (l2 * 3.0).backward()
    assert float(l2.detach()) == float(loss.detach())
    for b, (pb, qb) in enumerate(lens):
        np.testing.assert_allclose(xc.grad[b, :pb].cpu().numpy(), gxr[b], rtol=1e-4, atol=1e-9)
        assert not xc.grad[b, pb:].any() and not yc.grad[b, qb:].any()


@pytest.mark.parametrize("P,Q", [(300, 500), (2050, 1024)])
def test_chamfer_with_every_length_at_capacity_is_the_dense_chamfer(P, Q):
    """Against ops.chamfer_distance(x, y): the value within 1e-6 relative, the gradients within rtol 1e-4 / atol 1e-9 (both sum
    the same fp32 terms, by atomics in an order of their own)."""
    rng = np.random.default_rng(P + Q)
    x = torch.from_numpy(rng.random((3, P, 3)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.random((3, Q, 3)).astype(np.float32)).cuda()
    xa, ya = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    la, _ = ops.chamfer_distance(xa, ya)
    (la * 3.0).backward()
    xb, yb = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    lb, _ = ops.chamfer_distance(xb, yb, x_lengths=[P] * 3, y_lengths=[Q] * 3)
    (lb * 3.0).backward()
    assert abs(float(lb.detach()) - float(la.detach())) <= 1e-6 * float(la.detach())
    np.testing.assert_allclose(xb.grad.cpu().numpy(), xa.grad.cpu().numpy(), rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(yb.grad.cpu().numpy(), ya.grad.cpu().numpy(), rtol=1e-4, atol=1e-9)
    # one of the two alone: the other cloud is full
    lc, _ = ops.chamfer_distance(x, y, x_lengths=[P] * 3)
    assert float(lc) == float(lb.detach())


def test_chamfer_by_length_with_thousands_of_points_sharing_a_neighbour():
    """test_chamfer_backward_with_thousands_of_points_sharing_a_neighbour (tests/test_gpu_geometry.py) with lengths (4096, 3000) in
    capacities (4096, 4096): the reconstruction is a blob, so the per-wave combining rounds of the scatter carry almost all of the
    sum.  Expected: the definition's gradient with wx = 1 / (B p_b), wy = 1 / (B q_b), summed in float64 over the assignment the GPU's
    own search made."""
    rng = np.random.default_rng(77)
    cap, lens = 4096, (4096, 3000)
    x = np.stack([0.5 + 1e-3 * rng.random((cap, 3)), rng.random((cap, 3))]).astype(np.float32)
    x[0, :5] = rng.random((5, 3))
    y = rng.random((2, cap, 3)).astype(np.float32)
    x[1, lens[1]:] = np.nan
    y[1, lens[1]:] = np.nan
    xg, yg = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(y).cuda().requires_grad_(True)
    loss, _ = ops.chamfer_distance(xg, yg, x_lengths=lens, y_lengths=lens)
    loss.backward()
    nxy = ops.nn_dist_n(xg.detach(), yg.detach(), lens, lens, return_idx=True)[1].cpu().numpy()
    nyx = ops.nn_dist_n(yg.detach(), xg.detach(), lens, lens, return_idx=True)[1].cpu().numpy()
    assert np.unique(nyx[0]).size < 64
    gx, gy = np.zeros((2, cap, 3)), np.zeros((2, cap, 3))
    for b, n in enumerate(lens):
        xb, yb = x[b, :n].astype(np.float64), y[b, :n].astype(np.float64)
        dx = 2.0 * (xb - yb[nxy[b, :n]]) / (2 * n)
        dy = 2.0 * (yb - xb[nyx[b, :n]]) / (2 * n)
        gx[b, :n] += dx
        np.add.at(gy[b], nxy[b, :n], -dx)
        gy[b, :n] += dy
        np.add.at(gx[b], nyx[b, :n], -dy)
    scale = float(np.abs(gx).max())
    assert scale > 100 * float(np.abs(gx[1]).max())
    np.testing.assert_allclose(xg.grad.cpu().numpy(), gx, rtol=1e-4, atol=2e-6 * scale)
    np.testing.assert_allclose(yg.grad.cpu().numpy(), gy, rtol=1e-4, atol=2e-6 * scale)
    assert not xg.grad[1, lens[1]:].any() and not yg.grad[1, lens[1]:].any()


def test_lengths_and_the_deterministic_mode_are_refused_before_any_launch(monkeypatch):
    x = torch.rand(2, 16, 3).cuda()
    for bad in ([0, 16], [16, 17], [-1, 3]):
        with pytest.raises(_lib.PccxError, match=r"\[1, 16\]"):
            ops.chamfer_distance(x, x, x_lengths=bad)
    with pytest.raises(_lib.PccxError, match="one int per cloud"):
        ops.nn_dist_n(x, x, [16], [16, 16])
    monkeypatch.setattr(ops, "deterministic_hook", lambda: True)
    with pytest.raises(_lib.PccxError, match="deterministic"):
        ops.chamfer_distance(x, x, x_lengths=[16, 16], y_lengths=[16, 16])
    assert ops.chamfer_distance(x, x)[0].shape == ()               # without lengths the mode is served as before
