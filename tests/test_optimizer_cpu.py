"""Reference side of the optimiser pins (tests/test_optimizer.py): one clipped Adam step restated in float64 numpy, the three error
statistics in units of u = 2^-24, torch's own float32 Adam on the same inputs (the arithmetic the reference project trains with, and
the yardstick every GPU bar is a multiple of), and the input distributions.  The tests here check the helpers on the CPU: the
restatement against clip_grad_norm_ + torch.optim.Adam in float64, the statistics on planted errors, and -- with the kernels' fp32
arithmetic emulated in numpy -- that the bar of 4 x torch-float32 separates the right update from every near miss it is meant to catch."""
import numpy as np
import pytest
import torch

U = 2.0 ** -24
STEPS = (1, 2, 7, 1000, 100000)
DEFAULT = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
OTHER = dict(lr=0.25, b1=0.5, b2=0.9, eps=1e-3)                    # no constant is hard-wired


# ---- the float64 restatement ----------------------------------------------------------------------------------------------------------
def sumsq64(grads):
    """sum of the squares of float32 gradients, in float64 (every product is exact in double)"""
    return float(sum(np.square(np.asarray(g, dtype=np.float64)).sum() for g in grads))


def clip_factor(gnorm_sq, max_norm):
    """clip_grad_norm_'s factor from the squared norm; max_norm None = no clipping"""
    if max_norm is None:
        return 1.0
    return min(1.0, float(max_norm) / (np.sqrt(gnorm_sq) + 1e-6))


def adam_step64(p0, g, m0, v0, t, lr, b1, b2, eps, clip=1.0):
    """-> (P, M, V): step t (1-based) of torch.optim.Adam on the gradient g * clip, all in float64"""
    p0, g, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (p0, g, m0, v0))
    gc = g * clip
    M = b1 * m0 + (1.0 - b1) * gc
    V = b2 * v0 + (1.0 - b2) * gc * gc
    P = p0 - lr / (1.0 - b1 ** t) * M / (np.sqrt(V) / np.sqrt(1.0 - b2 ** t) + eps)
    return P, M, V


# ---- the error statistics -------------------------------------------------------------------------------------------------------------
def ulp32(x):
    """the spacing of float32 at |x|, as float64"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _worst(err, scale):
    """max err / scale; where the scale is 0 the result is exact in any arithmetic, so an error there is infinite"""
    err, scale = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(scale, dtype=np.float64))
    if err.size == 0:
        return 0.0
    pos = scale > 0
    r = np.where(pos, err / np.where(pos, scale, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(max(r.max(), 0.0))


def uncancelled(g, m0, V, t, lr, b1, b2, eps, clip=1.0):
    """-> (a, Ubar): |b1 m0| + |(1-b1) g clip|, and the update that size of first moment would make.  Errors are measured against these
    and not against M or P - p0, which cancel: dividing by them gives outliers in the thousands for any float32 Adam."""
    g, m0, V = (np.asarray(x, dtype=np.float64) for x in (g, m0, V))
    a = np.abs(b1 * m0) + np.abs((1.0 - b1) * g * clip)
    return a, lr / (1.0 - b1 ** t) * a / (np.sqrt(V) / np.sqrt(1.0 - b2 ** t) + eps)


def error_stats(got, want, p0, g, m0, t, lr, b1, b2, eps, clip=1.0):
    """got = (p, m, v) of a float32 implementation, want = (P, M, V) of adam_step64 -> (cm, cv, cp) in units of u = 2^-24:
        cm = max |m - M| / (u a),  cv = max |v - V| / (u V),  cp = max (|p - P| - ulp32(max(|p0|, |P|)) / 2) / (u Ubar)
    The half ulp is what storing p in float32 costs whatever the update was."""
    (p, m, v), (P, M, V) = (tuple(np.asarray(x, dtype=np.float64) for x in s) for s in (got, want))
    a, ubar = uncancelled(g, m0, V, t, lr, b1, b2, eps, clip)
    cm = _worst(np.abs(m - M), U * a)
    cv = _worst(np.abs(v - V), U * V)
    cp = _worst(np.abs(p - P) - 0.5 * ulp32(np.maximum(np.abs(np.asarray(p0, dtype=np.float64)), np.abs(P))), U * ubar)
    return cm, cv, cp


# ---- torch's own Adam on the same inputs ----------------------------------------------------------------------------------------------
def fresh(a, dtype):
    """a torch tensor that owns its memory: torch.from_numpy aliases the array (and .to() of the same dtype still does), and
    clip_grad_norm_ / Adam.step write in place -- the caller's inputs would change under it"""
    return torch.from_numpy(np.array(a, dtype=dtype, copy=True))


def torch_adam(ps, gs, ms, vs, t, lr, b1, b2, eps, max_norm=None, clip=None, dtype=np.float32):
    """clip_grad_norm_(max_norm) + torch.optim.Adam.step() as step t on the CPU in `dtype`; the state (step t - 1, exp_avg, exp_avg_sq)
    goes in through load_state_dict.  gs[i] None = a parameter without gradient.  clip: the factor is GIVEN and applied the way
    clip_grad_norm_ applies its own (one in-place multiplication of every gradient by the factor rounded to `dtype`).
    -> lists (p, m, v) of numpy arrays"""
    params = [torch.nn.Parameter(fresh(p, dtype)) for p in ps]
    for q, g in zip(params, gs):
        q.grad = None if g is None else fresh(g, dtype)
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps)
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(float(t - 1)), "exp_avg": fresh(m, dtype), "exp_avg_sq": fresh(v, dtype)}
                   for i, (m, v) in enumerate(zip(ms, vs))}
    opt.load_state_dict(sd)
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(params, max_norm)
    if clip is not None:
        for q in params:
            if q.grad is not None:
                q.grad.mul_(torch.tensor(clip, dtype=q.dtype))
    opt.step()
    return ([q.detach().numpy().copy() for q in params], [opt.state[q]["exp_avg"].numpy().copy() for q in params],
            [opt.state[q]["exp_avg_sq"].numpy().copy() for q in params])


def cat(arrays):
    return np.concatenate([np.asarray(a).reshape(-1) for a in arrays]) if len(arrays) else np.zeros(0)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def draw_grad(rng, n):
    """N(0,1) * 10^U(-6,1) per element"""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-6.0, 1.0, n)).astype(np.float32)


def draw_case(seed, sizes, t, b1, b2):
    """-> lists (p0, g, m0, v0) of float32 arrays, one per size.  The moments are min(t - 1, 30) steps of the float64 recurrences on
    gradients of the same distribution, cast to float32: realistic state, v of the order of m^2 or above; zero state at t = 1."""
    rng = np.random.default_rng(seed)
    ps, gs, ms, vs = [], [], [], []
    for n in sizes:
        m, v = np.zeros(n), np.zeros(n)
        for _ in range(min(t - 1, 30)):
            h = draw_grad(rng, n).astype(np.float64)
            m, v = b1 * m + (1.0 - b1) * h, b2 * v + (1.0 - b2) * h * h
        ps.append((rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 1.0, n)).astype(np.float32))
        gs.append(draw_grad(rng, n))
        ms.append(m.astype(np.float32))
        vs.append(v.astype(np.float32))
    return ps, gs, ms, vs


def reference_and_torch32(ps, gs, ms, vs, t, hp, max_norm):
    """One case both ways: -> (clip, (P, M, V) float64 on the concatenated tensors, (cm, cv, cp) of torch's float32 CPU Adam).
    The float32 Adam gets the clip factor of the float64 norm, rounded to float32: left to clip_grad_norm_ in float32 it sums 10^5
    squares in float32, its factor comes out some 20 u off and cm / cv of the yardstick read 20 / 40 instead of 2 / 2.5 -- a bar of four
    times that would measure torch's norm, not Adam's arithmetic, and let the kernels be an order of magnitude worse than they may be."""
    clip = clip_factor(sumsq64(gs), max_norm)
    p0, g, m0 = cat(ps), cat(gs), cat(ms)
    want = adam_step64(p0, g, m0, cat(vs), t, clip=clip, **hp)
    tp, tm, tv = torch_adam(ps, gs, ms, vs, t, clip=None if max_norm is None else clip, **hp)
    return clip, want, error_stats((cat(tp), cat(tm), cat(tv)), want, p0, g, m0, t, clip=clip, **hp)


# ---- the kernels' arithmetic in numpy float32 (the library is built with -ffp-contract=off: no fused multiply-add) --------------------
def kernel32(p0, g, m0, v0, t, lr, b1, b2, eps, clip=1.0, constants="double", eps_inside=False, bc2_plain=False):
    """adam_kernel's expression tree in float32.  constants="double": 1 - beta and 1 - beta^t formed in double and rounded once, as
    torch does; "float": 1.f - (float)beta and 1.f - powf(beta, t), every operand already rounded.  eps_inside / bc2_plain are the two
    misplacements the eps-regime and bias-correction checks are there for."""
    f = np.float32
    p0, g, m0, v0 = (np.asarray(a, dtype=f) for a in (p0, g, m0, v0))
    if constants == "double":
        om1, om2, bc1, bc2 = f(1.0 - b1), f(1.0 - b2), f(1.0 - b1 ** t), f(1.0 - b2 ** t)
    else:
        om1, om2 = f(1) - f(b1), f(1) - f(b2)
        bc1, bc2 = f(1) - np.power(f(b1), f(t)), f(1) - np.power(f(b2), f(t))
    gi = g * f(clip)
    mi = f(b1) * m0 + om1 * gi
    vi = f(b2) * v0 + om2 * gi * gi
    root = bc2 if bc2_plain else np.sqrt(bc2)
    denom = np.sqrt(vi / bc2 + f(eps)) if eps_inside else np.sqrt(vi) / root + f(eps)
    return p0 - (f(lr) / bc1) * (mi / denom), mi, vi


# ---- the helpers' own tests -----------------------------------------------------------------------------------------------------------
SIZES_CPU = (1, 3, 257, 0, 4099)


@pytest.mark.parametrize("hp", [DEFAULT, OTHER], ids=["default", "other"])
@pytest.mark.parametrize("t", STEPS)
def test_float64_restatement_is_clip_grad_norm_and_torch_adam(t, hp):
    """adam_step64 against clip_grad_norm_ + torch.optim.Adam on float64 tensors with the state loaded through load_state_dict, to
    1e-14 relative -- of the un-cancelled sizes the statistics divide by: a for m, V for v, max(|p0|, |P|) + Ubar for p (torch forms m
    as a lerp, so the two first moments differ by an ulp of a, which the update carries at the size of Ubar however small p is)."""
    ps, gs, ms, vs = draw_case(100 + t, SIZES_CPU, t, hp["b1"], hp["b2"])
    ss = sumsq64(gs)
    for max_norm in (None, 1.0, 2.0 * np.sqrt(ss)):
        clip = clip_factor(ss, max_norm)
        assert (clip < 1e-1) if max_norm == 1.0 else clip == 1.0
        keep = [a.copy() for a in ps + gs + ms + vs]
        tp, tm, tv = torch_adam(ps, gs, ms, vs, t, max_norm=max_norm, dtype=np.float64, **hp)
        assert all(np.array_equal(a, b) for a, b in zip(keep, ps + gs + ms + vs)), "torch wrote into the inputs"
        P, M, V = adam_step64(cat(ps), cat(gs), cat(ms), cat(vs), t, clip=clip, **hp)
        a, ubar = uncancelled(cat(gs), cat(ms), V, t, clip=clip, **hp)
        assert _worst(np.abs(cat(tm) - M), a) <= 1e-14
        assert _worst(np.abs(cat(tv) - V), V) <= 1e-14
        assert _worst(np.abs(cat(tp) - P), np.maximum(np.abs(cat(ps)), np.abs(P)) + ubar) <= 1e-14


def test_statistics_read_planted_errors_in_units_of_u():
    hp, t = DEFAULT, 7
    ps, gs, ms, vs = draw_case(5, (300,), t, hp["b1"], hp["b2"])
    p0, g, m0, v0 = ps[0], gs[0], ms[0], vs[0]
    P, M, V = adam_step64(p0, g, m0, v0, t, **hp)
    a, ubar = uncancelled(g, m0, V, t, **hp)
    assert error_stats((P, M, V), (P, M, V), p0, g, m0, t, **hp) == (0.0, 0.0, 0.0)
    m, v, p = M.copy(), V.copy(), P.copy()
    m[17] += 3 * U * a[17]
    v[101] -= 5 * U * V[101]
    p[250] += 7 * U * ubar[250] + 0.5 * ulp32(max(abs(p0[250]), abs(P[250])))
    cm, cv, cp = error_stats((p, m, v), (P, M, V), p0, g, m0, t, **hp)
    assert abs(cm - 3) < 1e-6 and abs(cv - 5) < 1e-6 and abs(cp - 7) < 1e-6
    # a zero scale is an exact result: any error there is infinite, none is nothing
    z = np.zeros(4)
    assert error_stats((z, z, z), (z, z, z), z, z, z, 1, **hp) == (0.0, 0.0, 0.0)
    assert error_stats((z, z + 1e-30, z), (z, z, z), z, z, z, 1, **hp)[0] == np.inf
    assert error_stats(tuple(np.zeros(0) for _ in range(3)), tuple(np.zeros(0) for _ in range(3)), *(np.zeros(0),) * 3, 1, **hp) == (0, 0, 0)


def test_fresh_does_not_alias_its_source():
    a = np.arange(4, dtype=np.float32)
    fresh(a, np.float32).mul_(2.0)
    assert a.tolist() == [0.0, 1.0, 2.0, 3.0]
    assert torch.from_numpy(a).to(torch.float32).data_ptr() == a.ctypes.data        # the trap fresh() is there for


@pytest.mark.parametrize("hp", [DEFAULT, OTHER], ids=["default", "other"])
@pytest.mark.parametrize("t", STEPS)
def test_the_bar_separates_the_right_update_from_its_near_misses(t, hp):
    """The GPU bar (each statistic <= 4 x torch-float32's on the same case) applied to the kernels' arithmetic emulated in numpy, without
    clipping and clipped to norm 1: constants rounded once from double pass; eps inside the square root or bc2 without its root fail cp
    wherever they change the update (bc2 is 1 at t = 100000, where the root changes nothing); 1.f - beta formed from the float betas fails
    cv for the default betas on unclipped gradients (1 - 0.999f is off by 1.3e-5, about 200 u of the second moment's increment; a
    gradient clipped by 1/400 adds next to nothing to a second moment built from unclipped ones) -- the deviation the double constants
    remove."""
    ps, gs, ms, vs = draw_case(200 + t, (1025, 40000), t, hp["b1"], hp["b2"])
    p0, g, m0, v0 = cat(ps), cat(gs), cat(ms), cat(vs)
    for max_norm in (None, 1.0):
        clip, want, tstat = reference_and_torch32(ps, gs, ms, vs, t, hp, max_norm)
        stat = lambda **kw: error_stats(kernel32(p0, g, m0, v0, t, clip=clip, **hp, **kw), want, p0, g, m0, t, clip=clip, **hp)
        good, floats, inside, plain = stat(), stat(constants="float"), stat(eps_inside=True), stat(bc2_plain=True)
        print(f"t={t} max_norm={max_norm} torch32 {tstat}\n  double constants {good}\n  float constants {floats}\n  eps inside {inside}\n"
              f"  bc2 plain {plain}")
        assert all(0 <= s < 16 for s in tstat)                 # a handful of roundings of at most u each (none: 0.5 g from zero state)
        assert all(a <= 4 * b for a, b in zip(good, tstat))
        assert inside[2] > 4 * tstat[2]
        if 1.0 - hp["b2"] ** t < 1.0 - 2 * U:
            assert plain[2] > 4 * tstat[2]
        if hp is DEFAULT and max_norm is None:
            assert floats[1] > 4 * tstat[1]


def test_adam_refuses_a_parameter_that_is_not_contiguous():
    """m and v would keep the parameter's strides while the kernels walk the parameter by flat index against a contiguous gradient"""
    from pccx import _lib, train
    ok = torch.nn.Parameter(torch.randn(5, 8))
    with pytest.raises(_lib.PccxError, match="parameter 1 .*not contiguous"):
        train.Adam([ok, torch.nn.Parameter(torch.randn(8, 5).t())])
    assert len(train.Adam([ok, torch.nn.Parameter(torch.randn(0)), torch.nn.Parameter(torch.randn(8, 5).t().contiguous())]).params) == 3
