"""The run-time arithmetic choices of the training layers (pccx/train.py) against float64 on the CPU: every kernel path of LinearFn
(skinny, wide, generic vector / scalar) with and without bias, fp32 and autocast, under every state of the step arena (none, measuring,
live, undersized); the folded Conv -> BatchNorm -> Linear chains (pccx_linear_moments, pccx_linear_bnback) against an independent
reference; BatchNorm outputs with two consumers and parked sums outside forward_train; one whole step at a shape whose global Linear is
512 -> 512 with bias behind a BatchNorm at batch 12.  Autocast references: operands rounded to bf16, exact products, the float64 sum plus
the bias, ONE rounding to bf16.  Every test leaves the module state of pccx.train as it found it."""
import contextlib
import copy

import numpy as np
import pytest
import torch

from oracle import ref_families as rf, ref_train
from tests import synth


def _bf(a):
    """round to bf16 (nearest even), as float64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().double().numpy()


def _ulp(v):
    """one bf16 ulp at |v| (8 significant bits); the smallest normal's ulp at 0"""
    a = np.maximum(np.abs(v), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def _acc_floor(xr, Wr, b):
    """what fp32 accumulation of the K products may leave behind, below which a bf16 ulp of the result is no bar (an output that cancels to
    1e-6 has a bf16 ulp of 1e-8): 2^-19 of the sum of the magnitudes of its terms (measured: under 2^-21 at K = 1024)"""
    return 2.0 ** -19 * (np.abs(xr) @ np.abs(Wr).T + (np.abs(b.astype(np.float64)) if b is not None else 0.0))


@contextlib.contextmanager
def _train_state():
    """save and restore everything of pccx.train a layer call can change"""
    from pccx import train
    saved = (train._AUTOCAST, train._ARENA, train._EAGER_ARENA, train._FOLD_MOMENTS)
    maps = [dict(m) for m in (train._MOMENTS, train._BN_OF, train._BWD_SUMS)]
    try:
        yield train
    finally:
        train._AUTOCAST, train._ARENA, train._EAGER_ARENA, train._FOLD_MOMENTS = saved
        for m, s in zip((train._MOMENTS, train._BN_OF, train._BWD_SUMS), maps):
            m.clear()
            m.update(s)


ARENAS = ("none", "measuring", "live", "undersized")


def _in_arena(train, state, run):
    """run() (forward AND backward: the arena must be in place for both, as in train_step) under one state of the step arena.
    measuring: the first step through a fresh StepArena (every request falls back).  live: the step after it.  undersized: a live arena
    that holds only half of what the step asks for, as after an earlier, smaller step -- the later requests fall back."""
    dev = torch.device("cuda", torch.cuda.current_device())
    if state == "none":
        train._ARENA = None
        try:
            return run()
        finally:
            train._ARENA = None
    a = train.StepArena()
    if state in ("live", "undersized"):
        a.begin(dev)
        train._ARENA = a
        try:
            run()
        finally:
            train._ARENA = None
            a.end(dev)
        if state == "undersized":
            half = a.need // 2 // 16 * 16
            assert half > 0
            a.buf = a.buf[:half]
        assert a.buf is not None
    a.begin(dev)
    train._ARENA = a
    held = a.buf.numel() if a.buf is not None else 0
    try:
        out = run()
    finally:
        train._ARENA = None
        a.end(dev)
    if state == "measuring":
        assert a.need > 0 and held == 0                         # the step asked for arena memory and got none
    elif state == "undersized":
        assert a.need > held, "nothing fell back"
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# 1a. LinearFn: path x bias x arithmetic x arena

# (name, M, K, N, storage-offset view, expected path)
LINEAR_CASES = [
    ("m1", 1, 256, 96, False, "skinny"),
    ("m8", 8, 256, 96, False, "skinny"),
    ("m9", 9, 256, 96, False, "generic"),
    ("m4k3", 4, 3, 32, False, "generic"),
    ("wide12", 12, 1024, 2048, False, "wide"),
    ("wide256", 256, 1024, 2048, False, "wide"),
    ("m260", 260, 1024, 2048, False, "generic"),
    ("offset6", 6, 64, 96, True, "generic"),              # dword-aligned rows: the generic layer's scalar variant
    ("offset_wide12", 12, 1024, 2048, True, "wide"),      # pccx_pack_linear_device / pccx_linear_dw load x one float at a time
]


def test_linear_path_dispatch_without_a_gpu():
    """_linear_path is the dispatch of LinearFn.forward; on the CPU the wide form (a GPU pack) is never chosen."""
    from pccx import train
    W = torch.zeros(2048, 1024)
    assert train._linear_path(torch.zeros(8, 1024), W) == "skinny"
    assert train._linear_path(torch.zeros(12, 1024), W) == "generic"
    assert train._linear_path(torch.zeros(1 + 8 * 1024)[1:].view(8, 1024), W) == "generic"
    assert train._linear_path(torch.zeros(4, 3), torch.zeros(32, 3)) == "generic"
    assert train._is_wide(12, 2048, 1024) and train._is_wide(256, 2048, 1024) and not train._is_wide(260, 2048, 1024)


def test_step_scope_restores_the_module_state_when_the_step_raises():
    """Whatever happens inside a step, pccx.train is left as outside one: no arena installed, the arena ended, autocast off, also for
    the first half of a step cut in two (end=False), whose arena would otherwise stay open for a second half that never comes."""
    with _train_state() as train:
        for end in (True, False):
            arena, p = train.StepArena(), torch.nn.Parameter(torch.zeros(2))
            p.grad = torch.ones(2)
            with pytest.raises(ZeroDivisionError):
                with train.step_scope("cpu", arena, autocast=True, params=[p], end=end) as forward_done:
                    assert train._ARENA is arena and train._AUTOCAST is True and arena.active and p.grad is None
                    forward_done()
                    assert train._AUTOCAST is False and train._ARENA is arena
                    1 / 0
            assert train._ARENA is None and train._AUTOCAST is False and arena.active is False
        with train.step_scope("cpu", arena, autocast=True, end=False):              # no exception: the first half leaves the arena open ...
            pass
        assert train._ARENA is None and train._AUTOCAST is False and arena.active is True
        with train.step_scope("cpu", arena, params=[p], begin=False):                # ... and the second half ends it
            assert train._ARENA is arena and arena.active
        assert train._ARENA is None and arena.active is False
        with train.step_scope("cpu"):                                                # an eager step on the CPU runs without an arena
            assert train._ARENA is None


def _linear_ref(x, W, b, gz, autocast):
    """float64 forward / dX / dW / db of z = x W^T + b; autocast: the bf16 form, the forward rounded once after the bias"""
    r = _bf if autocast else (lambda a: a.astype(np.float64))
    z = r(x) @ r(W).T + (b.astype(np.float64) if b is not None else 0.0)
    return dict(z=z, dx=r(gz) @ r(W), dW=r(gz).T @ r(x), db=gz.astype(np.float64).sum(0) if b is not None else None,
                floor=_acc_floor(r(x), r(W), b))


def _check_linear(got, want, autocast, what):
    z = got["z"].astype(np.float64)
    if autocast:
        zr = _bf(want["z"])
        assert np.array_equal(z, _bf(z)), f"{what}: the autocast forward is not a bf16 value"
        bad = np.abs(z - zr) > _ulp(zr) + want["floor"]
        assert not bad.any(), (what, "forward", int(bad.sum()), float(np.abs(z - zr).max()))
        dx = want["dx"]
        tol = np.maximum(np.abs(dx), 1e-3 * np.abs(dx).max()) * 2.0 ** -7          # one bf16 ulp (the generic dX rounds, the others not)
        assert (np.abs(got["dx"] - dx) <= tol).all(), (what, "dX", float(np.abs(got["dx"] - dx).max()))
        for k in ("dW", "db"):
            if want[k] is not None:
                np.testing.assert_allclose(got[k], want[k], rtol=1e-4, atol=1e-4 * np.abs(want[k]).max(), err_msg=f"{what} {k}")
    else:
        np.testing.assert_allclose(z, want["z"], rtol=1e-5, atol=1e-5 * np.abs(want["z"]).max(), err_msg=f"{what} forward")
        for k in ("dx", "dW", "db"):
            if want[k] is not None:
                assert np.abs(got[k] - want[k]).max() <= 1e-4 * np.abs(want[k]).max(), (what, k, float(np.abs(got[k] - want[k]).max()))
    if want["db"] is None:
        assert got["db"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("case", LINEAR_CASES, ids=[c[0] for c in LINEAR_CASES])
def test_linear_paths_against_float64(case):
    name, M, K, N, offset, path = case
    rng = np.random.default_rng(M * 7919 + K + N)
    x = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    gz = rng.standard_normal((M, N)).astype(np.float32)
    with _train_state() as train:
        for with_bias in (True, False):
            b = bias if with_bias else None
            for autocast in (False, True):
                want = _linear_ref(x, W, b, gz, autocast)

                def run():
                    if offset:
                        buf = torch.zeros(1 + M * K, device="cuda")
                        xg = buf[1:].view(M, K)
                        xg.copy_(torch.from_numpy(x))
                        xg.requires_grad_(True)
                    else:
                        xg = torch.from_numpy(x).cuda().requires_grad_(True)
                    Wg = torch.from_numpy(W).cuda().requires_grad_(True)
                    bg = torch.from_numpy(b).cuda().requires_grad_(True) if b is not None else None
                    assert train._linear_path(xg.detach().contiguous(), Wg.detach()) == path
                    if offset:
                        assert xg.data_ptr() % 16 == 4                         # the scalar loads of the generic layer
                    train._AUTOCAST = autocast
                    try:
                        z = train.LinearFn.apply(xg, Wg, bg)
                    finally:
                        train._AUTOCAST = False
                    z.backward(torch.from_numpy(gz).cuda())
                    return dict(z=z.detach().cpu().numpy(), dx=xg.grad.cpu().numpy().astype(np.float64),
                                dW=Wg.grad.cpu().numpy().astype(np.float64),
                                db=bg.grad.cpu().numpy().astype(np.float64) if bg is not None else None)

                for state in ARENAS:
                    got = _in_arena(train, state, run)
                    _check_linear(got, want, autocast, (name, "bias" if with_bias else "no bias", "autocast" if autocast else "fp32", state))


@pytest.mark.gpu
def test_autocast_rounds_once_after_the_bias_whatever_the_batch():
    """A bias that cancels 95 % of row r0's product: the layer's one rounding must come after the bias (a rounding of the product first is
    off by up to half a bf16 ulp of the PRODUCT, many ulps of the result).  The same 8 rows inside batches of 8 (skinny), 12 (wide) and
    300 (generic): equal to one bf16 ulp among themselves and to the round-once value."""
    K, N = 1024, 2048
    rng = np.random.default_rng(17)
    rows = rng.standard_normal((8, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    r0 = 3
    b = (-0.95 * (_bf(rows[r0:r0 + 1]) @ _bf(W).T)[0]).astype(np.float32)
    want = _bf(_bf(rows) @ _bf(W).T + b.astype(np.float64))
    tol = _ulp(want) + _acc_floor(_bf(rows), _bf(W), b)
    outs = {}
    with _train_state() as train:
        for M, path in ((8, "skinny"), (12, "wide"), (300, "generic")):
            x = np.concatenate([rows, rng.standard_normal((M - 8, K)).astype(np.float32)])
            xg, Wg, bg = (torch.from_numpy(t).cuda() for t in (x, W, b))
            assert train._linear_path(xg, Wg) == path
            train._ARENA, train._AUTOCAST = None, True
            try:
                z = train.LinearFn.apply(xg, Wg, bg)
            finally:
                train._AUTOCAST = False
            outs[path] = z[:8].cpu().numpy().astype(np.float64)
            err = np.abs(outs[path] - want)
            assert (err <= tol).all(), (path, int((err > tol).sum()), float((err / tol).max()))
    for a, c in (("skinny", "wide"), ("skinny", "generic"), ("wide", "generic")):
        d = np.abs(outs[a] - outs[c])
        assert (d <= _ulp(np.maximum(np.abs(outs[a]), np.abs(outs[c]))) + 2 * (tol - _ulp(want))).all(), (a, c, float(d.max()))


# ------------------------------------------------------------------------------------------------------------------------------------
# 1b. Conv (no bias, column moments in its epilogue) -> BatchNorm-ReLU -> Linear (dY and the BatchNorm's sums from one GEMM)

def _chain_ref(x, W1, gamma, beta, W2, b2, wgt, autocast, eps=1e-5, momentum=0.1):
    """float64 forward and hand-written backward of sum(wgt * (relu(bn(x W1^T)) W2^T + b2)), with the roundings of the autocast layers:
    every GEMM operand rounded to bf16, the forward GEMMs' and the dX GEMMs' results rounded once (after the bias), dW in full precision"""
    r = _bf if autocast else (lambda a: np.asarray(a, dtype=np.float64))
    rr = _bf if autocast else (lambda a: a)
    M = x.shape[0]
    z1 = rr(r(x) @ r(W1).T)
    mean, var = z1.mean(0), z1.var(0)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (z1 - mean) * rstd
    y = np.maximum(gamma * xhat + beta, 0.0)
    g = wgt.astype(np.float64)
    out = dict(db2=g.sum(0) if b2 is not None else None, dW2=r(g).T @ r(y))
    dy = rr(r(g) @ r(W2))
    d = dy * (y > 0)
    out["dgamma"], out["dbeta"] = (d * xhat).sum(0), d.sum(0)
    dz1 = gamma * rstd * (d - out["dbeta"] / M - xhat * out["dgamma"] / M)
    out["dW1"], out["dx"] = r(dz1).T @ r(x), rr(r(dz1) @ r(W1))
    out["running_mean"] = momentum * mean
    out["running_var"] = (1 - momentum) + momentum * var * M / (M - 1)
    return out


def test_chain_reference_matches_torch_autograd():
    """the hand-written float64 chain above against torch autograd over nn.BatchNorm1d (train mode), fp32 form"""
    rng = np.random.default_rng(2)
    M, Ci, C, N = 40, 12, 16, 16
    x, W1, W2 = rng.standard_normal((M, Ci)), rng.standard_normal((C, Ci)) / 3, rng.standard_normal((N, C)) / 4
    gamma, beta, b2, wgt = rng.random(C) + 0.5, rng.standard_normal(C) * 0.1, rng.standard_normal(N), rng.standard_normal((M, N))
    want = _chain_ref(x, W1, gamma, beta, W2, b2, wgt, False)
    t = {k: torch.from_numpy(v).requires_grad_(True) for k, v in dict(x=x, W1=W1, W2=W2, b2=b2).items()}
    bn = torch.nn.BatchNorm1d(C).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)), bn.bias.copy_(torch.from_numpy(beta))
    z2 = torch.relu(bn(t["x"] @ t["W1"].T)) @ t["W2"].T + t["b2"]
    (z2 * torch.from_numpy(wgt)).sum().backward()
    for k, v in (("dx", t["x"].grad), ("dW1", t["W1"].grad), ("dW2", t["W2"].grad), ("db2", t["b2"].grad), ("dgamma", bn.weight.grad),
                 ("dbeta", bn.bias.grad), ("running_mean", bn.running_mean), ("running_var", bn.running_var)):
        np.testing.assert_allclose(want[k], v.detach().numpy(), rtol=1e-10, atol=1e-12, err_msg=k)


def _chain_gpu(train, x, W1, gamma, beta, W2, b2, wgt, autocast):
    dev = "cuda"
    C = W1.shape[0]
    xg = torch.from_numpy(x).to(dev).requires_grad_(True)
    W1g = torch.from_numpy(W1.reshape(C, -1, 1, 1)).to(dev).requires_grad_(True)        # a 1x1 Conv's weight
    W2g = torch.from_numpy(W2).to(dev).requires_grad_(True)
    b2g = torch.from_numpy(b2).to(dev).requires_grad_(True) if b2 is not None else None
    bn = torch.nn.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)), bn.bias.copy_(torch.from_numpy(beta))
    reductions = []                                  # column sums asked for by a Function that reduces on its own (not parked)
    sums = train._sums

    def counted(C_, device, private=False):
        if not private:
            reductions.append(C_)
        return sums(C_, device, private)

    train._sums = counted
    try:
        train._AUTOCAST = autocast
        try:
            z1 = train.LinearFn.apply(xg, W1g, None, True)
            assert train._MOMENTS and train._linear_path(xg.detach(), W1g.detach().view(C, -1)) == "generic"
            y = train.BnReluFn.apply(z1, bn.weight, bn.bias, bn)
            assert not train._MOMENTS, "the BatchNorm did not take the GEMM's moments"
            assert train._linear_path(y.detach(), W2g.detach()) == "generic" and y.data_ptr() in train._BN_OF
            z2 = train.LinearFn.apply(y, W2g, b2g)
        finally:
            train._AUTOCAST = False
        params = [xg, W1g, W2g, bn.weight, bn.bias] + ([b2g] if b2g is not None else [])
        grads = torch.autograd.grad((z2 * torch.from_numpy(wgt).to(dev)).sum(), params)
    finally:
        train._sums = sums
    assert not train._BWD_SUMS, "the BatchNorm backward did not take the sums of the GEMM that produced its dY"
    # both folds taken: the BatchNorm reduced neither its input nor its dY; the one reduction is the bias gradient's
    assert reductions == ([W2.shape[0]] if b2 is not None else []), reductions
    out = dict(zip(["dx", "dW1", "dW2", "dgamma", "dbeta", "db2"], [g.detach().cpu().double().numpy() for g in grads]))
    out["dW1"] = out["dW1"].reshape(C, -1)
    out.setdefault("db2", None)
    out["running_mean"], out["running_var"] = bn.running_mean.cpu().double().numpy(), bn.running_var.cpu().double().numpy()
    return out


CHAIN_CASES = [("n_eq_k_bias", 64, True), ("n_ne_k_bias", 96, True), ("no_bias", 64, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("M", [12, 300, 5000])
@pytest.mark.parametrize("second", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_folded_batchnorm_chain_against_float64(second, M):
    name, N, with_bias = second
    Ci, C = 32, 64
    rng = np.random.default_rng(M + N)
    x = rng.standard_normal((M, Ci)).astype(np.float32)
    W1 = (rng.standard_normal((C, Ci)) / 6).astype(np.float32)
    W2 = (rng.standard_normal((N, C)) / 8).astype(np.float32)
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    beta = (rng.standard_normal(C) * 0.3).astype(np.float32)
    b2 = rng.standard_normal(N).astype(np.float32) if with_bias else None
    wgt = rng.standard_normal((M, N)).astype(np.float32)
    with _train_state() as train:
        train._FOLD_MOMENTS = True
        for autocast in (False, True):
            want = _chain_ref(x, W1, gamma.astype(np.float64), beta.astype(np.float64), W2, b2, wgt, autocast)
            for state in ARENAS:
                got = _in_arena(train, state, lambda: _chain_gpu(train, x, W1, gamma, beta, W2, b2, wgt, autocast))
                # fp32: 1e-4 of each tensor's largest entry.  autocast: the GPU's fp32 sums and the reference's float64 ones round a few
                # elements to neighbouring bf16 values; the BatchNorm carries such a flip into every gradient at ~2^-8 of its scale
                tol = 2.0 ** -7 if autocast else 1e-4
                for k, w in want.items():
                    if w is None:
                        assert got[k] is None, k
                        continue
                    err = float(np.abs(got[k] - w).max())
                    assert err <= tol * float(np.abs(w).max()) + 1e-7, (name, M, "autocast" if autocast else "fp32", state, k, err,
                                                                        float(np.abs(w).max()))


# ------------------------------------------------------------------------------------------------------------------------------------
# 1c. BatchNorm outputs with two consumers, parked moments outside forward_train

def _bn_layer(rng, M, Ci, C):
    x = rng.standard_normal((M, Ci)).astype(np.float32)
    W1 = (rng.standard_normal((C, Ci)) / 6).astype(np.float32)
    gamma, beta = (rng.random(C) + 0.5).astype(np.float32), (rng.standard_normal(C) * 0.3).astype(np.float32)
    return x, W1, gamma, beta


def _cpu_bn(x, W1, gamma, beta):
    """float64 torch autograd: relu(BatchNorm1d(x W1^T)) -> (y, leaves, bn)"""
    t = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in dict(x=x, W1=W1).items()}
    bn = torch.nn.BatchNorm1d(W1.shape[0]).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)), bn.bias.copy_(torch.from_numpy(beta))
    return torch.relu(bn(t["x"] @ t["W1"].T)), [t["x"], t["W1"], bn.weight, bn.bias], bn


def _gpu_bn(train, x, W1, gamma, beta):
    xg, W1g = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(W1).cuda().requires_grad_(True)
    bn = torch.nn.BatchNorm2d(W1.shape[0]).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)), bn.bias.copy_(torch.from_numpy(beta))
    y = train.BnReluFn.apply(train.LinearFn.apply(xg, W1g, None, True), bn.weight, bn.bias, bn)
    return y, [xg, W1g, bn.weight, bn.bias], bn


def _compare(got, want, what, tol=1e-4):
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = a.detach().cpu().double().numpy(), b.detach().double().numpy()
        err = float(np.abs(a - b).max())
        assert err <= tol * float(np.abs(b).max()) + 1e-7, (what, i, err, float(np.abs(b).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("second", ["linear", "group_max"])
def test_batchnorm_output_with_two_consumers(second):
    """y = relu(bn(x W1^T)) read by a Linear (bnback: dY and the BatchNorm's sums from one GEMM) AND by a second consumer -- another
    Linear, or the max over neighbours of a set-abstraction layer.  Autograd sums the two dY, possibly in place into one of them; the
    BatchNorm's backward must see the sum, not the sums of one consumer."""
    M, Ci, C, N = 512, 32, 64, 48
    G = M // 16
    rng = np.random.default_rng(21)
    x, W1, gamma, beta = _bn_layer(rng, M, Ci, C)
    Wa, ba = (rng.standard_normal((N, C)) / 8).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    Wb = (rng.standard_normal((C, C)) / 8).astype(np.float32)
    wa = rng.standard_normal((M, N)).astype(np.float32)
    wb = rng.standard_normal((M, C) if second == "linear" else (G, C)).astype(np.float32)
    y_r, leaves_r, bn_r = _cpu_bn(x, W1, gamma, beta)
    Wa_r, ba_r, Wb_r = (torch.from_numpy(t).double().requires_grad_(True) for t in (Wa, ba, Wb))
    lr = ((y_r @ Wa_r.T + ba_r) * torch.from_numpy(wa).double()).sum()
    if second == "linear":
        lr = lr + ((y_r @ Wb_r.T) * torch.from_numpy(wb).double()).sum()
        extra_r = [Wa_r, ba_r, Wb_r]
    else:
        lr = lr + (y_r.view(G, 16, C).max(1).values * torch.from_numpy(wb).double()).sum()
        extra_r = [Wa_r, ba_r]
    want = torch.autograd.grad(lr, leaves_r + extra_r)
    with _train_state() as train:
        train._FOLD_MOMENTS = True
        for state in ARENAS:
            def run():
                y, leaves, bn = _gpu_bn(train, x, W1, gamma, beta)
                Wa_g, ba_g, Wb_g = (torch.from_numpy(t).cuda().requires_grad_(True) for t in (Wa, ba, Wb))
                loss = (train.LinearFn.apply(y, Wa_g, ba_g) * torch.from_numpy(wa).cuda()).sum()
                if second == "linear":
                    loss = loss + (train.LinearFn.apply(y, Wb_g, None) * torch.from_numpy(wb).cuda()).sum()
                    extra = [Wa_g, ba_g, Wb_g]
                else:
                    loss = loss + (train.GroupMaxFn.apply(y.view(G, 16, C)) * torch.from_numpy(wb).cuda()).sum()
                    extra = [Wa_g, ba_g]
                return [g.clone() for g in torch.autograd.grad(loss, leaves + extra)], bn

            got, bn = _in_arena(train, state, run)
            _compare(got, want, (second, state))
            _compare([bn.running_mean, bn.running_var], [bn_r.running_mean, bn_r.running_var], (second, state, "running"), 1e-5)


@pytest.mark.gpu
def test_parked_moments_of_a_dropped_output_do_not_reach_another_tensor():
    """Outside forward_train nothing clears the maps: a LinearFn(want_moments=True) output that is dropped before any BatchNorm reads it
    leaves its moments parked, and the caching allocator hands its address to the next tensor of the same size.  A BatchNorm over THAT
    tensor must reduce it, not take the dropped one's moments."""
    M, Ci, C = 1000, 32, 64
    rng = np.random.default_rng(23)
    x, W1, gamma, beta = _bn_layer(rng, M, Ci, C)
    x2, W2, _, _ = _bn_layer(rng, M, Ci, C)
    with _train_state() as train:
        train._FOLD_MOMENTS = True
        train._MOMENTS.clear(), train._BN_OF.clear(), train._BWD_SUMS.clear()
        for state in ARENAS:
            def run():
                dropped = train.LinearFn.apply(torch.from_numpy(x).cuda(), torch.from_numpy(W1).cuda(), None, True)
                del dropped
                y, leaves, bn = _gpu_bn(train, x2, W2, gamma, beta)       # its own Conv: a fresh (M, C) output, then its BatchNorm
                gy = torch.from_numpy(np.cos(np.arange(M * C, dtype=np.float32)).reshape(M, C)).cuda()
                # and a BatchNorm over a plain tensor of the same size, made after another dropped moments output
                dropped = train.LinearFn.apply(torch.from_numpy(x).cuda(), torch.from_numpy(W1).cuda(), None, True)
                del dropped
                zt = torch.from_numpy(x2 @ W2.T).cuda().requires_grad_(True)
                bn2 = torch.nn.BatchNorm2d(C).cuda()
                with torch.no_grad():
                    bn2.weight.copy_(torch.from_numpy(gamma)), bn2.bias.copy_(torch.from_numpy(beta))
                y2 = train.BnReluFn.apply(zt, bn2.weight, bn2.bias, bn2)
                g = torch.autograd.grad((y * gy).sum() + (y2 * gy).sum(), leaves + [zt, bn2.weight, bn2.bias])
                return y.detach().clone(), y2.detach().clone(), [t.clone() for t in g], bn, bn2

            y, y2, got, bn, bn2 = _in_arena(train, state, run)
            y_r, leaves_r, bn_r = _cpu_bn(x2, W2, gamma, beta)
            gy = torch.from_numpy(np.cos(np.arange(M * C, dtype=np.float32)).reshape(M, C)).double()
            zt_r = torch.from_numpy(x2 @ W2.T).double().requires_grad_(True)
            bn2_r = torch.nn.BatchNorm1d(C).double()
            with torch.no_grad():
                bn2_r.weight.copy_(torch.from_numpy(gamma)), bn2_r.bias.copy_(torch.from_numpy(beta))
            y2_r = torch.relu(bn2_r(zt_r))
            want = torch.autograd.grad((y_r * gy).sum() + (y2_r * gy).sum(), leaves_r + [zt_r, bn2_r.weight, bn2_r.bias])
            _compare([y, y2], [y_r, y2_r], (state, "forward"), 1e-5)
            _compare(got, want, (state, "gradients"))
            _compare([bn.running_mean, bn.running_var, bn2.running_mean, bn2.running_var],
                     [bn_r.running_mean, bn_r.running_var, bn2_r.running_mean, bn2_r.running_var], (state, "running"), 1e-5)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1d. The whole step where the global Linear is 512 -> 512 with bias behind a BatchNorm and the batch is above 8

@pytest.mark.gpu
def test_step_with_a_square_global_linear_behind_batchnorm_at_batch_12():
    """PointCloudAE(latent 512) at batch 12: encoder.global_conv[3] is a 512 -> 512 Linear with bias fed by a BatchNorm, evaluated by the
    generic layer (12 rows), so its backward takes the bnback fold AND a bias reduction over the same channel count.  The first eager step
    through a fresh arena only measures it (every column sum falls back), as does the warm-up of a GraphedTrainStep.  One train_step
    against the CPU oracle at the bars of test_training_step_matches_autograd_and_adam's first step; then the parameters a
    GraphedTrainStep(warmup=1) leaves after its construction (the warm-up is a real step; the capture only records) against the same
    oracle step."""
    from pccx import families
    from pccx import synth as cloud_synth
    N, B, lr = 2048, 12, 1e-3
    x = np.stack([cloud_synth.cad_cloud(700 + b, N) for b in range(B)]).astype(np.float32)
    rng = np.random.default_rng(5)
    starts = [[rng.integers(0, N, B), rng.integers(0, N, B)], rng.integers(0, 512, B), rng.integers(0, 128, B)]
    o = rf.PointCloudAE(512, 16, N)
    o.load_state_dict(synth.family_tweak(rf.seeded_with_bn(o, synth.PPPE_SEED), "pppe"))
    init = copy.deepcopy(o.state_dict())
    torch.set_num_threads(8)
    ol = ref_train.train_step(o, torch.optim.Adam(o.parameters(), lr=lr), torch.from_numpy(x), starts, lam=0.5)
    osd, ob = dict(o.named_parameters()), dict(o.named_buffers())
    with _train_state() as train:
        train._EAGER_ARENA = train.StepArena()                     # step 0 is the measuring step
        g = families.PointCloudAE(512, 16, N)
        g.load_state_dict(init)
        g = g.cuda()
        w3 = g.encoder.global_conv[3].weight.detach()
        assert tuple(w3.shape[:2]) == (512, 512) and g.encoder.global_conv[3].bias is not None
        assert train._linear_path(torch.zeros(B, 512, device="cuda"), w3.reshape(512, -1)) == "generic"
        gl = train.train_step(g, train.Adam(g.parameters(), lr=lr), torch.from_numpy(x).cuda(), starts, lam=0.5)
        assert abs(gl[2] - ol[2]) <= 1e-4 * abs(ol[2]) + 1e-6, (gl, ol)
        assert abs(gl[0] - ol[0]) <= 2e-5 * abs(ol[0]) + 1e-7, (gl, ol)
        gsd = dict(g.named_parameters())
        gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in gsd.values() if p.grad is not None)))
        coef = min(1.0, 1.0 / (gn + 1e-6))
        gmax = max(float(p.grad.abs().max()) for p in osd.values() if p.grad is not None)
        noise = {k for k, p in osd.items() if p.grad is not None and float(p.grad.abs().max()) < 1e-5 * gmax}
        for k, p in osd.items():
            if p.grad is None:
                assert gsd[k].grad is None, k
                continue
            a, b = gsd[k].grad.cpu().numpy() * coef, p.grad.numpy()
            assert np.abs(a - b).max() <= 1e-2 * np.abs(b).max() + 1e-5 * gmax, (k, np.abs(a - b).max(), np.abs(b).max())

        def check_state(model, what):
            for k, p in osd.items():
                d = np.abs(dict(model.named_parameters())[k].detach().cpu().numpy() - p.detach().numpy())
                assert d.max() <= 2.2 * lr, (what, k, d.max())
                if k not in noise:
                    assert np.median(d) < 0.05 * lr and (d > 0.1 * lr).mean() < 0.25, (what, k, np.median(d), (d > 0.1 * lr).mean())
            mb = dict(model.named_buffers())
            for k, v in ob.items():
                np.testing.assert_allclose(mb[k].cpu().numpy(), v.numpy(), rtol=1e-4, atol=1e-5, err_msg=f"{what} {k}")

        check_state(g, "eager step")
        g2 = families.PointCloudAE(512, 16, N)
        g2.load_state_dict(init)
        g2 = g2.cuda()
        opt2 = train.Adam(g2.parameters(), lr=lr)
        train.GraphedTrainStep(g2, opt2, torch.from_numpy(x).cuda(), starts, lam=0.5, warmup=1)
        torch.cuda.synchronize()
        assert opt2.t == 1
        check_state(g2, "graphed warm-up")
