"""The deterministic training mode (train.step_scope(deterministic=True)): every kernel family alone, then both trainers end
to end.  Every bitwise check hands the entry an output and a workspace filled with 0xFF bytes (NaN as float / double, -1 as int), so it
also proves "written, not accumulated", and calls twice: the second call runs on recycled memory that the first one dirtied."""
import os

import numpy as np
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu


def _dirty(n, dtype):
    """n elements of 0xFF bytes on the GPU"""
    size = torch.empty(0, dtype=dtype).element_size()
    return torch.full((max(int(n), 1) * size,), 0xFF, dtype=torch.uint8, device="cuda").view(dtype)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- 1. dW / dX fold ---------------------------------------------------------------------------------------------------------------
def _dw_det(lib, dz, x, M, N, K, flags):
    from pccx import _lib
    out = _dirty(N * K, torch.float32).view(N, K)
    ws = _dirty(lib.pccx_linear_dw_det_workspace_floats(M, N, K), torch.float32)
    _lib.call("pccx_linear_dw_det", dz.data_ptr(), x.data_ptr(), M, N, K, dz.stride(0), x.stride(0), out.data_ptr(), flags, ws.data_ptr(), _st())
    return out


def _dw_atomic(dz, x, M, N, K, flags):
    from pccx import _lib
    out = torch.zeros(N, K, device="cuda")
    _lib.call("pccx_linear_dw", dz.data_ptr(), x.data_ptr(), M, N, K, dz.stride(0), x.stride(0), out.data_ptr(), flags, _st())
    return out


@pytest.mark.parametrize("flags", [0, 2], ids=["fp32", "autocast"])
def test_dw_and_dx_fold_is_written_reproducible_and_pinned(flags):
    """The issue's shapes read as (rows, the layer's two widths): dW of 3000 rows into a 70 x 35 weight (several row slices, ragged tiles);
    64 rows through a 1030 x 300 weight with the ROLES SWAPPED as train._is_wide does it (dX^T = the dW entry over the weight's 1030 rows);
    4 rows through the same weight as the split-K skinny dX (K = 300 is the width a float4 load needs a multiple of four of).
    Tolerance: the per-layer pin of tests/test_train_step.py for the atomic path (rtol 1e-4, atol 1e-4 of the largest entry) against a
    float64 product -- of the bf16-rounded operands under the autocast flag, whose products are exact -- and against the atomic entry."""
    from pccx import _lib
    lib = _lib.load()
    rng = np.random.default_rng(21)
    r = (lambda t: t.bfloat16().double()) if flags else (lambda t: t.double())
    tol = lambda got, want: np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(want.abs().max()))
    # dW: (M, N, K) = (3000, 70, 35)
    M, N, K = 3000, 70, 35
    assert lib.pccx_linear_dw_det_workspace_floats(M, N, K) >= 2 * N * K                       # more than one slice
    dz = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).cuda()
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).cuda()
    a, b = _dw_det(lib, dz, x, M, N, K, flags), _dw_det(lib, dz, x, M, N, K, flags)
    assert _same(a, b) and bool(torch.isfinite(a).all())
    tol(a, (r(dz).T @ r(x)).float())
    tol(a, _dw_atomic(dz, x, M, N, K, flags))
    # role-swapped dX of a wide layer: 64 rows, W (1030, 300): dX^T (300, 64) = W^T dZ^T
    Ml, Nl, Kl = 64, 1030, 300
    W = torch.from_numpy((rng.standard_normal((Nl, Kl)) / np.sqrt(Kl)).astype(np.float32)).cuda()
    dzl = torch.from_numpy(rng.standard_normal((Ml, Nl)).astype(np.float32)).cuda()
    dzT = dzl.t().contiguous()
    a, b = _dw_det(lib, W, dzT, Nl, Kl, Ml, flags), _dw_det(lib, W, dzT, Nl, Kl, Ml, flags)
    assert _same(a, b)
    tol(a, (r(W).T @ r(dzT)).float())
    tol(a, _dw_atomic(W, dzT, Nl, Kl, Ml, flags))
    # skinny split-K dX: 4 rows
    Ms = 4
    dzs = torch.from_numpy(rng.standard_normal((Ms, Nl)).astype(np.float32)).cuda()

    def skinny():
        out = _dirty(Ms * Kl, torch.float32).view(Ms, Kl)
        ws = _dirty(lib.pccx_linear_skinny_dx_det_workspace_floats(Ms, Nl, Kl), torch.float32)
        _lib.call("pccx_linear_skinny_dx_det", dzs.data_ptr(), Ms, Nl, Nl, W.data_ptr(), Kl, flags, out.data_ptr(), Kl, ws.data_ptr(), _st())
        return out
    a, b = skinny(), skinny()
    assert _same(a, b)
    tol(a, (r(dzs) @ r(W)).float())
    at = torch.zeros(Ms, Kl, device="cuda")
    _lib.call("pccx_linear_skinny_dx", dzs.data_ptr(), Ms, Nl, Nl, W.data_ptr(), Kl, flags, at.data_ptr(), Kl, _st())
    tol(a, at)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_linear_fn_takes_the_wide_and_skinny_branches_deterministically(autocast):
    """LinearFn itself under step_scope(deterministic=True): 12 rows through a 2048 x 1024 weight really is train._is_wide (the role-swapped
    dX through pccx_linear_dw_det), 4 rows through it the skinny split-K dX; gradients of two runs are bit-equal and agree with float64 at
    the per-layer pin (1e-4; under autocast the generic pin of one bf16 ulp, 2^-7, as the operands and dX's product are bf16 values)."""
    from pccx import train
    rng = np.random.default_rng(27)
    N, K = 2048, 1024
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    for M in (12, 4):
        assert train._is_wide(M, N, K) == (M == 12)
        x = rng.standard_normal((M, K)).astype(np.float32)
        gz = rng.standard_normal((M, N)).astype(np.float32)
        runs = []
        for _ in range(2):
            xg, Wg, bg = (torch.from_numpy(t).cuda().requires_grad_(True) for t in (x, W, b))
            with train.step_scope("cuda", autocast=autocast, deterministic=True) as forward_done:
                z = train.LinearFn.apply(xg, Wg, bg)
                forward_done()
                z.backward(torch.from_numpy(gz).cuda())
            runs.append((xg.grad.clone(), Wg.grad.clone(), bg.grad.clone()))
            _dirty(1 << 20, torch.float32)                                             # dirty what the caching allocator hands out next
        assert all(_same(p, q) for p, q in zip(*runs))
        r = (lambda t: torch.from_numpy(t).bfloat16().double()) if autocast else (lambda t: torch.from_numpy(t).double())
        want = (r(gz) @ r(W), r(gz).T @ r(x), torch.from_numpy(gz).double().sum(0))
        rt = 2.0 ** -7 if autocast else 1e-4
        for got, w in zip(runs[0], want):
            np.testing.assert_allclose(got.cpu().numpy(), w.numpy(), rtol=rt, atol=rt * float(w.abs().max()))


# ---- 2. column / scalar sums -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [67, 4])
def test_ordered_column_sums_three_modes(C):
    from pccx import _lib
    lib = _lib.load()
    rng = np.random.default_rng(22 + C)
    M = 5000
    z = torch.from_numpy((rng.standard_normal((M, C)) * 2 + 0.3).astype(np.float32)).cuda()
    dy = torch.from_numpy((rng.standard_normal((M, C)) + 0.5).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.standard_normal((M, C)).astype(np.float32)).cuda()
    mean = z.mean(0).contiguous()
    rstd = (1.0 / (z.var(0, unbiased=False) + 1e-5).sqrt()).contiguous()
    d = torch.where(y > 0, dy, torch.zeros_like(dy))
    xhat = (z - mean) * rstd                                                          # float32, as the kernel forms it
    want = {0: (z.double().sum(0), (z.double() ** 2).sum(0)), 1: ((d.double() * xhat.double()).sum(0), d.double().sum(0)), 2: (dy.double().sum(0), None)}
    nsum = int(lib.pccx_train_sums_doubles(C))

    def run(mode):
        part = _dirty(lib.pccx_col_reduce_det_doubles(M, C), torch.float64)
        sums = _dirty(nsum, torch.float64)
        f32 = _dirty(C, torch.float32)
        a = dy if mode else z
        _lib.call("pccx_col_reduce_det", mode, a.data_ptr(), y.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, C, part.data_ptr(),
                  sums.data_ptr(), f32.data_ptr(), _st())
        return sums, f32
    for mode in (0, 1, 2):
        (s1, f1), (s2, f2) = run(mode), run(mode)
        used = C if mode == 2 else nsum
        assert _same(s1[:used], s2[:used]) and _same(f1, f2)
        w0, w1 = want[mode]
        rel = lambda got, w: float(((got - w).abs() / w.abs()).max())
        print(f"mode {mode} C {C}: rel err sum0 {rel(s1[:C], w0):.3e}" + (f" sum1 {rel(s1[C:2 * C], w1):.3e}" if w1 is not None else ""))
        assert rel(s1[:C], w0) <= 1e-12
        assert torch.equal(f1, s1[:C].float())
        if w1 is not None:
            assert rel(s1[C:2 * C], w1) <= 1e-12
            assert bool((s1[2 * C:] == 0).all()) and not bool(torch.signbit(s1[2 * C:]).any())       # the other replicas: +0, written


def test_ordered_scalar_sums():
    from pccx import _lib
    lib = _lib.load()
    rng = np.random.default_rng(23)
    n = 70001
    a = torch.from_numpy((rng.standard_normal(n) * 2).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()

    def l1():
        part, val, grad = _dirty(lib.pccx_smooth_l1_det_doubles(n), torch.float64), _dirty(1, torch.float64), _dirty(n, torch.float32)
        _lib.call("pccx_smooth_l1_det", a.data_ptr(), b.data_ptr(), n, 0.25, part.data_ptr(), val.data_ptr(), grad.data_ptr(), _st())
        return val, grad
    (v1, g1), (v2, g2) = l1(), l1()
    assert _same(v1, v2) and _same(g1, g2)
    dd = a - b
    want = torch.where(dd.abs() < 1, 0.5 * dd.double() * dd.double(), dd.abs().double() - 0.5).sum()
    print("smooth_l1 rel err", float((v1[0] - want).abs() / want))
    assert float((v1[0] - want).abs() / want) <= 1e-12
    gref = torch.empty_like(a)
    vref = torch.empty(1, device="cuda", dtype=torch.float64)
    _lib.call("pccx_smooth_l1", a.data_ptr(), b.data_ptr(), n, 0.25, vref.data_ptr(), gref.data_ptr(), _st())
    assert torch.equal(g1, gref)
    # sum of squares over five tensors of unequal size (the table of train.Adam.step)
    gs = [torch.from_numpy(rng.standard_normal(k).astype(np.float32)).cuda() for k in (5, 1024, 1025, 40000, 333)]
    rows, first = np.zeros((len(gs), 6), dtype=np.int64), 0
    for i, g in enumerate(gs):
        rows[i] = (g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), g.numel(), first)
        first += (g.numel() + 1023) // 1024
    table = torch.from_numpy(rows).cuda()

    def ss():
        part, acc = _dirty(lib.pccx_sumsq_multi_det_doubles(first), torch.float64), _dirty(1, torch.float64)
        _lib.call("pccx_sumsq_multi_det", table.data_ptr(), len(gs), first, part.data_ptr(), acc.data_ptr(), _st())
        return acc
    s1, s2 = ss(), ss()
    want = sum((g.double() ** 2).sum() for g in gs)
    print("sumsq rel err", float((s1[0] - want).abs() / want))
    assert _same(s1, s2) and float((s1[0] - want).abs() / want) <= 1e-12


# ---- 3. segmented scatter -----------------------------------------------------------------------------------------------------------
def _scatter(vals, ldv, idx, B, M, N, C):
    from pccx import _lib
    out = _dirty(B * N * C, torch.float32).view(B, N, C)
    ws = _dirty(_lib.load().pccx_scatter_add_ordered_workspace_ints(B, M, N), torch.int32)
    _lib.call("pccx_scatter_add_ordered", vals.data_ptr(), ldv, idx.data_ptr(), 0, B, M, N, C, out.data_ptr(), ws.data_ptr(), _st())
    return out


def _scatter_host(vals, idx, B, N, C):
    want = np.zeros((B, N, C), dtype=np.float32)
    for b in range(B):
        np.add.at(want[b], idx[b], vals[b, :, :C])                                    # unbuffered: adds in ascending source position
    return want


@pytest.mark.parametrize("C,ld", [(3, 4), (5, 5), (131, 131)])
def test_ordered_scatter_is_np_add_at_bit_for_bit(C, ld):
    rng = np.random.default_rng(24 + C)
    B, N, M = 2, 257, 33 * 16
    tables = {"random": rng.integers(0, N, (B, M)), "one row": np.full((B, M), 101), "half untouched": rng.integers(0, N // 2, (B, M)) * 2}
    for name, idx in tables.items():
        vals = (rng.standard_normal((B, M, ld)) * 10.0 ** rng.integers(-3, 4, (B, M, 1))).astype(np.float32)
        v, i = torch.from_numpy(vals).cuda(), torch.from_numpy(idx.astype(np.int64)).cuda()
        a, b = _scatter(v, ld, i, B, M, N, C), _scatter(v, ld, i, B, M, N, C)
        want = _scatter_host(vals, idx, B, N, C)
        assert _same(a, b), name
        assert np.array_equal(a.cpu().numpy().view(np.uint32), want.view(np.uint32)), name   # bit for bit: untouched rows are +0, not -0
        untouched = np.setdiff1d(np.arange(N), idx[0])
        assert untouched.size and not a[0, untouched].cpu().numpy().view(np.uint32).any(), name


def test_ordered_scatter_of_4096_sources_onto_one_row():
    rng = np.random.default_rng(25)
    B, N, M, C = 1, 257, 4096, 5
    idx = np.full((B, M), 200)
    vals = (rng.standard_normal((B, M, C)) * 10.0 ** rng.integers(-3, 4, (B, M, 1))).astype(np.float32)
    v, i = torch.from_numpy(vals).cuda(), torch.from_numpy(idx.astype(np.int64)).cuda()
    a, b = _scatter(v, C, i, B, M, N, C), _scatter(v, C, i, B, M, N, C)
    assert _same(a, b)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), _scatter_host(vals, idx, B, N, C).view(np.uint32))


# ---- 4. Chamfer gradient ------------------------------------------------------------------------------------------------------------
def test_chamfer_gradient_is_reproducible_and_close_to_the_atomic_one():
    from pccx import _lib, ops, train
    lib = _lib.load()
    rng = np.random.default_rng(26)
    B, P, Q = 2, 300, 517
    x = rng.random((B, P, 3)).astype(np.float32)
    y = rng.random((B, Q, 3)).astype(np.float32)
    y[0, :400] = x[0, 7] + 1e-3 * rng.standard_normal((400, 3)).astype(np.float32)      # hundreds of y share one nearest x
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    _, nxy = ops.nn_dist(xg, yg, return_idx=True)
    _, nyx = ops.nn_dist(yg, xg, return_idx=True)
    assert int((nyx[0] == 7).sum()) >= 300
    gd = torch.full((1,), 1.7, device="cuda")

    def det():
        gx, gy = _dirty(B * P * 3, torch.float32).view(B, P, 3), _dirty(B * Q * 3, torch.float32).view(B, Q, 3)
        wf = _dirty(lib.pccx_chamfer_grad_det_workspace_floats(B, P, Q), torch.float32)
        wi = _dirty(lib.pccx_chamfer_grad_det_workspace_ints(B, P, Q), torch.int32)
        _lib.call("pccx_chamfer_grad_det", xg.data_ptr(), B, P, yg.data_ptr(), Q, nxy.data_ptr(), nyx.data_ptr(), gd.data_ptr(), gx.data_ptr(),
                  gy.data_ptr(), wf.data_ptr(), wi.data_ptr(), _st())
        return gx, gy
    (ax, ay), (bx, by) = det(), det()
    assert _same(ax, bx) and _same(ay, by)
    rx, ry = torch.empty_like(xg), torch.empty_like(yg)
    _lib.call("pccx_chamfer_grad_dev", xg.data_ptr(), B, P, yg.data_ptr(), Q, nxy.data_ptr(), nyx.data_ptr(), gd.data_ptr(), rx.data_ptr(),
              ry.data_ptr(), _st())
    for got, ref in ((ax, rx), (ay, ry)):
        print("chamfer det vs atomic, max diff / max entry:", float((got - ref).abs().max() / ref.abs().max()))
        assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    # the autograd path takes the ordered form inside a deterministic step, and the atomic one outside it
    outs = []
    for flag in (True, True, False):
        xa = xg.clone().requires_grad_(True)
        with train.step_scope("cuda", deterministic=flag) as forward_done:
            loss, _ = ops.chamfer_distance(xa, yg)
            forward_done()
            (loss * 1.7).backward()
        outs.append(xa.grad.clone())
    assert _same(outs[0], outs[1]) and _same(outs[0], ax)
    assert float((outs[2] - ax).abs().max()) <= 1e-6 * float(ax.abs().max())
    # the registered op (torch.ops.pccx.chamfer_distance) routes its backward the same way
    from pccx import torch_ops  # noqa: F401
    tout = []
    for flag in (True, True):
        xa, ya = xg.clone().requires_grad_(True), yg.clone().requires_grad_(True)
        with train.step_scope("cuda", deterministic=flag) as forward_done:
            loss, _, _ = torch.ops.pccx.chamfer_distance(xa, ya)
            forward_done()
            (loss * 1.7).backward()
        tout.append((xa.grad.clone(), ya.grad.clone()))
    assert _same(tout[0][0], tout[1][0]) and _same(tout[0][1], tout[1][1])
    assert _same(tout[0][0], ax) and _same(tout[0][1], ay)


# ---- 5. IPDAE end to end ------------------------------------------------------------------------------------------------------------
def _ipdae_trainer(autocast):
    from pccx import train_ipdae
    from tests.test_train_ipdae import CFG as c, _models
    ae, prob = _models()
    return train_ipdae.IpdaeTrainer(ae.cuda(), prob.cuda(), N=c["N"], N0=c["N0"], ALPHA=c["ALPHA"], K=c["K"], lr=c["lr"], lamda=c["lamda"],
                                    rate_loss_enable_step=c["rate_loss_enable_step"], lr_decay=c["lr_decay"], lr_decay_steps=c["lr_decay_steps"],
                                    autocast=autocast, deterministic=True)


def _ipdae_state(tr):
    return [t.detach().clone() for t in list(tr.opt.params) + tr.opt.m + tr.opt.v]


def _ipdae_run(autocast, graphed, check=None):
    """three iterations on the fixture's batch -> (the three returned dicts, parameters + Adam moments)"""
    from tests.test_train_ipdae import CFG as c, GOLD
    gold = np.load(GOLD)
    x = torch.from_numpy(synth.train_input(c["B"], c["N"])).cuda()
    starts = [gold["starts"][0], gold["starts"][1], gold["starts"][0]]
    tr = _ipdae_trainer(autocast)
    outs = []
    if graphed:
        g = tr.graphed(x, starts[0], warmup=1)                                          # the warm-up iteration IS step 0
        outs.append({k: float(v) for k, v in zip(("loss", "fbpp", "bpp"), g.warm_out)})
        outs += [g(x, starts[1]), g(x, starts[2])]
    else:
        for it in range(3):
            outs.append(tr.step(x, starts[it]))
            if check is not None and it < 2:
                check(tr, it, outs[-1], gold)
    torch.cuda.synchronize()
    return outs, _ipdae_state(tr)


def _ipdae_fixture_check(tr, it, out, gold):
    """the assertions of tests/test_train_ipdae.py::test_ipdae_training_step_matches_the_reference_run, tolerance for tolerance"""
    from tests.test_train_ipdae import CFG as c
    names, lr = list(gold["param_names"]), c["lr"]
    sd = dict([("ae." + k, v) for k, v in tr.ae.named_parameters()] + [("prob." + k, v) for k, v in tr.prob.named_parameters()])
    want_loss, want_fbpp, _, _ = gold["scalars"][it]
    tol = 2e-5 if it == 0 else 1e-2
    assert abs(out["fbpp"] - want_fbpp) <= (1e-5 if it == 0 else 1e-2) * want_fbpp, (it, out, want_fbpp)
    assert abs(out["loss"] - want_loss) <= tol * abs(want_loss) + 1e-7, (it, out, want_loss)
    got_g = np.concatenate([synth.sample64(sd[k].grad.cpu().numpy()) for k in names])
    wg, wn = gold[f"grads_{it}"], gold[f"grad_norms_{it}"]
    gn = np.array([float(sd[k].grad.double().norm()) for k in names])
    pz = np.array([k.startswith("prob.") for k in names])
    if it == 0:
        assert (wn[pz] == 0).all() and (gn[pz] == 0).all()
        assert np.abs(gn - wn).max() <= 1e-2 * wn.max(), np.abs(gn - wn).max() / wn.max()
        off = 0
        for k in names:
            n = synth.sample64(sd[k].detach().cpu().numpy()).size
            a, b = got_g[off:off + n], wg[off:off + n]
            assert np.abs(a - b).max() <= 1e-2 * max(float(sd[k].grad.abs().max()), 1e-12) + 1e-9, (k, np.abs(a - b).max())
            off += n
    else:
        assert (gn[pz] > 0).all()
        assert np.abs(gn - wn).max() <= 5e-2 * wn.max()
    got_p = np.concatenate([synth.sample64(sd[k].detach().cpu().numpy()) for k in names])
    d = np.abs(got_p - gold[f"params_{it}"])
    assert d.max() <= 2.2 * lr * (it + 1), (it, d.max())
    if it == 0:
        assert np.median(d) <= 0.05 * lr and (d > 0.1 * lr).mean() < 0.25, (np.median(d), (d > 0.1 * lr).mean())
    assert abs(tr.opt.lr - float(gold[f"lr_{it}"])) < 1e-12


def _equal_runs(a, b):
    (oa, sa), (ob, sb) = a, b
    assert oa == ob, (oa, ob)                                                           # the three returned scalars of every iteration
    assert len(sa) == len(sb) and all(_same(p, q) for p, q in zip(sa, sb))


def test_ipdae_deterministic_steps_are_bit_identical_eager_graphed_and_match_the_fixture():
    e1 = _ipdae_run(False, False, check=_ipdae_fixture_check)
    e2 = _ipdae_run(False, False)
    _equal_runs(e1, e2)
    g1, g2 = _ipdae_run(False, True), _ipdae_run(False, True)
    _equal_runs(g1, g2)
    _equal_runs(e1, g1)                                                                 # fp32: the replayed step IS the eager one


def test_ipdae_deterministic_autocast_steps_are_bit_identical():
    _equal_runs(_ipdae_run(True, False), _ipdae_run(True, False))
    _equal_runs(_ipdae_run(True, True), _ipdae_run(True, True))


# ---- 6. pppe end to end --------------------------------------------------------------------------------------------------------------
def _pppe():
    from pccx import families, train
    from tests.test_train_step import _models
    g = families.PointCloudAE(64, 16, 2048)
    g.load_state_dict(_models(2048).state_dict())
    g = g.cuda()
    return g, train.Adam(g.parameters(), lr=1e-3)


def _pppe_state(g, opt):
    return [t.detach().clone() for t in list(g.parameters()) + list(g.buffers()) + opt.m + opt.v]


def _pppe_starts(gold, it):
    st = gold["starts"][it]
    return [[st[0], st[1]], st[2], st[3]]


def _pppe_gold():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "train_step.npz"))


def _pppe_eager(check):
    """three deterministic eager iterations as tests/test_train_step.py::test_training_step_matches_reference_run runs its two"""
    from pccx import train
    gold = _pppe_gold()
    names = list(gold["param_names"])
    g, opt = _pppe()
    x = torch.from_numpy(synth.train_input(2, 2048)).cuda()
    outs = []
    for it in range(3):
        if it == 1:
            opt.lr = float(gold["lr_0"])
        k = it % 2
        out = train.train_step(g, opt, x, _pppe_starts(gold, k), lam=float(gold["scalars"][k, 3]), loss_type="chamfer", deterministic=True)
        outs.append(out)
        if not check or it == 2:
            continue
        loss, dist, rate = out
        want = gold["scalars"][it]
        lam = float(want[3])
        tol = 2e-5 if it == 0 else 1e-2
        assert abs(dist - want[1]) <= tol * abs(want[1]) + 1e-7, (it, dist, want)
        assert abs(rate - want[2]) <= (1e-4 if it == 0 else 5e-2) * abs(want[2]) + 1e-6, (it, rate, want)
        assert abs(loss - (dist + lam * rate)) <= 1e-5 * abs(loss), (it, loss, dist, rate)
        if it == 0:
            assert abs(loss - want[0]) <= tol * abs(want[0]) + 1e-7, (it, loss, want)
        sd = dict(g.named_parameters())
        got_p = np.concatenate([synth.sample64(sd[n].detach().cpu().numpy()) for n in names])
        wp, wg = gold[f"params_{it}"], gold[f"grads_{it}"]
        if it == 0:
            gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in sd.values() if p.grad is not None)))
            coef = min(1.0, 1.0 / (gn + 1e-6))
            got_g = np.concatenate([synth.sample64(sd[n].grad.cpu().numpy()) * coef if sd[n].grad is not None
                                    else np.full(synth.sample64(sd[n].detach().cpu().numpy()).shape, np.nan, np.float32) for n in names])
            assert np.array_equal(np.isnan(got_g), np.isnan(wg))
            m = ~np.isnan(wg)
            assert np.abs(got_g[m] - wg[m]).max() <= 1e-2 * np.abs(wg[m]).max()
        d = np.abs(got_p - wp)
        assert d.max() <= 2.2e-3 * (it + 1), (it, d.max())
        if it == 0:
            assert np.median(d) <= 0.05 * 1e-3 and (d > 1e-4).mean() < 0.25, (np.median(d), (d > 1e-4).mean())
    torch.cuda.synchronize()
    return outs, _pppe_state(g, opt)


def _pppe_graphed(prefetch, debug_dot=None):
    from pccx import train
    gold = _pppe_gold()
    g, opt = _pppe()
    x = torch.from_numpy(synth.train_input(2, 2048)).cuda()
    step = train.GraphedTrainStep(g, opt, x, _pppe_starts(gold, 0), lam=float(gold["scalars"][0, 3]), warmup=1, prefetch=prefetch,
                                  deterministic=True, debug_dot=debug_dot)             # the warm-up iteration is step 0
    outs = [step(x, _pppe_starts(gold, 1)), step(x, _pppe_starts(gold, 0))]
    torch.cuda.synchronize()
    return outs, _pppe_state(g, opt)


def test_pppe_deterministic_eager_steps_are_bit_identical_and_match_the_fixture():
    _equal_runs(_pppe_eager(True), _pppe_eager(False))


@pytest.mark.parametrize("prefetch", [False, True])
def test_pppe_deterministic_graphed_steps_are_bit_identical(prefetch):
    _equal_runs(_pppe_graphed(prefetch), _pppe_graphed(prefetch))


def test_deterministic_data_parallel_is_refused():
    from pccx import _lib, train
    g, opt = _pppe()
    x = torch.from_numpy(synth.train_input(2, 2048)).cuda()
    st = _pppe_starts(_pppe_gold(), 0)
    with pytest.raises(_lib.PccxError, match="RCCL"):
        train.train_step(g, opt, x, st, data_parallel=True, deterministic=True)
    with pytest.raises(_lib.PccxError, match="RCCL"):
        train.GraphedTrainStep(g, opt, x, st, data_parallel=True, deterministic=True)
    assert train._DETERMINISTIC is False


# ---- 7. graph contents ---------------------------------------------------------------------------------------------------------------
def _node_kinds(graph):
    """hipGraphNodeType -> count over the nodes of the hipGraph a step REPLAYS (capture with keep_graph=True)"""
    import ctypes as C
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    raw = C.c_void_p(graph.raw_cuda_graph())
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, C.byref(n)) == 0 and n.value > 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, C.byref(n)) == 0
    kinds = {}
    for node in nodes:
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)) == 0
        kinds[t.value] = kinds.get(t.value, 0) + 1
    return kinds


@pytest.mark.parametrize("which", ["ipdae", "pppe", "pppe-prefetch"])
def test_deterministic_replay_has_no_memset_or_fill_node(which):
    """The three captured deterministic steps -- GraphedIpdaeStep, GraphedTrainStep with and without prefetch -- each read back node by
    node from the very hipGraph it replays (hipGraphGetNodes / hipGraphNodeGetType): hundreds of kernel nodes and no memset (fill) node;
    and the step's arena was never allocated, because nothing in the step accumulates into cleared memory.
    tests/test_no_memset_nodes.py keeps such calls out of the sources; this looks at what the capture recorded."""
    from pccx import train
    if which == "ipdae":
        from tests.test_train_ipdae import CFG as c, GOLD
        gold = np.load(GOLD)
        x = torch.from_numpy(synth.train_input(c["B"], c["N"])).cuda()
        step = _ipdae_trainer(False).graphed(x, gold["starts"][0], warmup=1, keep_graph=True)
        out = step(x, gold["starts"][1])
        assert all(np.isfinite(v) for v in out.values())
    else:
        gold = _pppe_gold()
        g, opt = _pppe()
        x = torch.from_numpy(synth.train_input(2, 2048)).cuda()
        step = train.GraphedTrainStep(g, opt, x, _pppe_starts(gold, 0), lam=float(gold["scalars"][0, 3]), warmup=1, deterministic=True,
                                      prefetch=which == "pppe-prefetch", keep_graph=True)
        out = step(x, _pppe_starts(gold, 1))
        assert all(np.isfinite(v) for v in out)
    torch.cuda.synchronize()
    assert step.arena.buf is None
    kinds = _node_kinds(step.graph)
    print(which, "node kinds (0 kernel, 1 memcpy, 2 memset, 5 empty):", kinds)
    assert kinds.get(2, 0) == 0, kinds                                                 # no memset (fill) node
    assert kinds.get(0, 0) > 100, kinds
