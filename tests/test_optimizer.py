"""clip_grad_norm_ + Adam as HIP kernels (csrc/train.hip: sumsq_kernel, sumsq_multi_kernel, sumsq_multi_det_kernel, adam_kernel,
adam_dev_kernel, adam_multi_kernel, adam_advance_kernel; driven by pccx.train.Adam), pinned element for element against the float64
restatement of tests/test_optimizer_cpu.py:

  1. the sums of squares against a float64 sum, 1e-12 relative (the bar of test_ordered_scalar_sums);
  2. one Adam step from given state through every entry point: the statistics cm / cv / cp (units of 2^-24 of the un-cancelled sizes)
     at most FOUR TIMES what torch's float32 CPU Adam -- the arithmetic the reference trains with -- shows on the same case;
  3. pccx.train.Adam over twelve steps in every mode it has, per tensor at most four times the float32 torch run's deviation from the
     float64 torch run plus one float32 ulp of the largest parameter.

No bar is a constant read off the GPU: each is computed in the test from torch's float32 Adam on the test's own inputs, printed beside
the GPU's figure (pytest -s) and recorded in the docstrings below and in DESIGN.md 4.4d as measured on one MI355X."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import test_optimizer_cpu as ref

pytestmark = pytest.mark.gpu

# 101 blocks of 1024 elements: the 16-block spans of sumsq_multi_kernel straddle tensor boundaries, the last span is ragged (5 blocks),
# an empty tensor sits in the middle and at the end
SIZES = (1, 3, 255, 256, 257, 1023, 1024, 1025, 2048, 0, 16383, 16384, 16385, 40000, 7, 0)
GUARD = 64
SENTINEL = np.int32(0x7FC5A5A5)                                     # a NaN as float: a guard read as data poisons the result as well
KINDS = ("step", "step_dev", "multi", "multi_hyper")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _blocks(n):
    return (n + 1023) // 1024


def _dirty(n, dtype):
    size = torch.empty(0, dtype=dtype).element_size()
    return torch.full((max(int(n), 1) * size,), 0xFF, dtype=torch.uint8, device="cuda").view(dtype)


def _rel(a, b):
    return abs(a - b) / abs(b)


# ---- 1. sums of squares ---------------------------------------------------------------------------------------------------------------
def _graded_grads(seed, sizes):
    """Every tensor's gradient at a magnitude of its own in 10^(-3 .. +2), entries +-U(0.5, 1.5) of it: the smaller the tensor the
    larger, and no entry near zero, so that no tensor's last partial block hides below the bar (asserted by the caller)"""
    rng = np.random.default_rng(seed)
    order = np.argsort(np.argsort(sizes, kind="stable"), kind="stable")
    mags = 10.0 ** (2.0 - 5.0 * order / max(len(sizes) - 1, 1))
    return [(rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.5, n) * s).astype(np.float32) for n, s in zip(sizes, mags)]


def _grad_table(gs):
    """the optimiser's table over gradients alone (the sums of squares read column 1 only) -> (device tensors, table, total blocks)"""
    dev = [torch.from_numpy(g.copy()).cuda() for g in gs]
    rows, first = np.zeros((len(dev), 6), dtype=np.int64), 0
    for i, g in enumerate(dev):
        rows[i] = (0, g.data_ptr(), 0, 0, g.numel(), first)
        first += _blocks(g.numel())
    return dev, torch.from_numpy(rows).cuda(), first


@pytest.mark.parametrize("sizes", [SIZES, (1,), (700,) * 15, (1024, 1, 513) * 5 + (77,), (1000,) * 17], ids=["table", "one", "15", "16", "17"])
def test_sums_of_squares_over_a_table(sizes):
    """pccx_sumsq_multi (atomic: accumulates, two calls give twice the sum) and pccx_sumsq_multi_det (writes: dirty accumulator and
    partials, two runs bit-identical) against the float64 sum of the float32 squares, 1e-12 relative.  Measured: at most 2.3e-16."""
    from pccx import _lib
    lib = _lib.load()
    gs = _graded_grads(31, sizes)
    want = ref.sumsq64(gs)
    for n, g in zip(sizes, gs):                                     # the table can see what it is there to see
        tail = g[(n - 1) // 1024 * 1024:] if n else g
        assert n == 0 or ref.sumsq64([tail]) > 50 * 1e-12 * want, "a dropped last block of this tensor would pass the bar"
    dev, table, total = _grad_table(gs)
    assert total == sum(_blocks(n) for n in sizes) and (sizes is not SIZES or total == 101)
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    _lib.call("pccx_sumsq_multi", table.data_ptr(), len(gs), total, acc.data_ptr(), _st())
    once = float(acc[0])
    _lib.call("pccx_sumsq_multi", table.data_ptr(), len(gs), total, acc.data_ptr(), _st())
    twice = float(acc[0])

    def det():
        part, out = _dirty(lib.pccx_sumsq_multi_det_doubles(total), torch.float64), _dirty(1, torch.float64)
        _lib.call("pccx_sumsq_multi_det", table.data_ptr(), len(gs), total, part.data_ptr(), out.data_ptr(), _st())
        return out
    d1, d2 = det(), det()
    print(f"sumsq T={len(sizes)} blocks={total}: atomic {_rel(once, want):.2e}, twice {_rel(twice, 2 * want):.2e}, det {_rel(float(d1[0]), want):.2e}")
    assert lib.pccx_sumsq_multi_det_doubles(total) == (total + 15) // 16
    assert _rel(once, want) <= 1e-12 and _rel(twice, 2 * want) <= 1e-12
    assert torch.equal(d1.view(torch.int64), d2.view(torch.int64)) and _rel(float(d1[0]), want) <= 1e-12


def test_sum_of_squares_of_one_tensor():
    """pccx_sumsq_accumulate at n = 1, 255, 262144 + 77 (past its 1024-block grid: the grid-stride loop) and 0 (the accumulator
    stays as it was), accumulating.  Measured: exact at 1 and 255, 1.4e-15 (one call) and 3.1e-15 (two) at 262221."""
    from pccx import _lib
    rng = np.random.default_rng(32)
    for n in (1, 255, 262144 + 77, 0):
        g = (rng.standard_normal(n) * 3.0).astype(np.float32)
        d = torch.from_numpy(g.copy()).cuda()
        acc = torch.full((1,), 3.5 if n == 0 else 0.0, dtype=torch.float64, device="cuda")
        _lib.call("pccx_sumsq_accumulate", d.data_ptr(), n, acc.data_ptr(), _st())
        once = float(acc[0])
        _lib.call("pccx_sumsq_accumulate", d.data_ptr(), n, acc.data_ptr(), _st())
        twice = float(acc[0])
        if n == 0:
            assert once == 3.5 and twice == 3.5
            continue
        want = ref.sumsq64([g])
        print(f"sumsq_accumulate n={n}: {_rel(once, want):.2e}, twice {_rel(twice, 2 * want):.2e}")
        assert _rel(once, want) <= 1e-12 and _rel(twice, 2 * want) <= 1e-12


# ---- 2. one Adam step from given state ------------------------------------------------------------------------------------------------
class Arena:
    """All tensors of one kind (p, g, m or v) carved from ONE buffer with GUARD sentinel words in front of, between and behind them;
    the odd sizes put most tensors at addresses that are no multiple of 16 bytes."""

    def __init__(self, arrays):
        self.sizes, self.off, o = [a.size for a in arrays], [], GUARD
        for a in arrays:
            self.off.append(o)
            o += a.size + GUARD
        self.host = np.full(o, SENTINEL, dtype=np.int32)
        for a, at in zip(arrays, self.off):
            self.host[at:at + a.size] = np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
        self.dev = torch.from_numpy(self.host.copy()).cuda()

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.off[i]

    def read(self):
        return self.dev.cpu().numpy()

    def tensors(self, buf):
        return [buf[at:at + n].view(np.float32) for at, n in zip(self.off, self.sizes)]

    def guards_intact(self, buf):
        keep = np.ones(buf.size, dtype=bool)
        for at, n in zip(self.off, self.sizes):
            keep[at:at + n] = False
        return bool((buf[keep] == SENTINEL).all())


def _hyper(t, lr, b1, b2, **_):
    """the 32-byte device state of pccx.h as the host path's own scalars: float lr | 1-b1^t | 1-b2^t | int32 t | double b1^t | b2^t"""
    h = np.zeros(8, dtype=np.float32)
    h[0], h[1], h[2] = lr, 1.0 - b1 ** t, 1.0 - b2 ** t
    h.view(np.int32)[3] = t
    h.view(np.float64)[2:4] = (b1 ** t, b2 ** t)
    return torch.from_numpy(h).cuda()


def _step(kind, case, t, hp, gnorm_sq=None, max_norm=0.0, rows=None):
    """One step through one entry point on fresh arenas -> {kind of tensor: the arena read back}, the arenas.  rows: the tensors that
    are in the table (the others are parameters without gradient).  Every call checks every guard word and every gradient bit."""
    from pccx import _lib
    ar = {k: Arena(a) for k, a in zip("pgmv", case)}
    rows = list(range(len(case[0]))) if rows is None else list(rows)
    acc = None if gnorm_sq is None else torch.tensor([gnorm_sq], dtype=torch.float64, device="cuda")
    accp = None if acc is None else acc.data_ptr()
    hyper = _hyper(t, **hp) if kind in ("step_dev", "multi_hyper") else None
    lr, b1, b2, eps = hp["lr"], hp["b1"], hp["b2"], hp["eps"]
    if kind in ("step", "step_dev"):
        for i in rows:
            ptrs = [ar[k].ptr(i) for k in "pgmv"] + [ar["p"].sizes[i], accp, max_norm]
            if kind == "step":
                _lib.call("pccx_adam_step", *ptrs, lr, b1, b2, eps, t, _st())
            else:
                _lib.call("pccx_adam_step_dev", *ptrs, hyper.data_ptr(), b1, b2, eps, _st())
    else:
        tab, first = np.zeros((len(rows), 6), dtype=np.int64), 0
        for r, i in enumerate(rows):
            tab[r] = tuple(ar[k].ptr(i) for k in "pgmv") + (ar["p"].sizes[i], first)
            first += _blocks(ar["p"].sizes[i])
        table = torch.from_numpy(tab).cuda()
        _lib.call("pccx_adam_multi", table.data_ptr(), len(rows), first, accp, max_norm, None if hyper is None else hyper.data_ptr(),
                  lr, t, b1, b2, eps, _st())
    torch.cuda.synchronize()
    out = {k: ar[k].read() for k in "pgmv"}
    for k in "pgmv":
        assert ar[k].guards_intact(out[k]), f"{kind}: a guard word of the {k} arena was written"
    assert np.array_equal(out["g"], ar["g"].host), f"{kind}: the gradients were written (the kernels scale on the fly)"
    for i in set(range(len(case[0]))) - set(rows):
        for k in "pmv":
            assert np.array_equal(ar[k].tensors(out[k])[i].view(np.int32), ar[k].tensors(ar[k].host)[i].view(np.int32)), \
                f"{kind}: tensor {i} is not in the table and its {k} changed"
    return out, ar


def _stats(out, ar, want, case, t, hp, clip):
    got = tuple(ref.cat(ar[k].tensors(out[k])) for k in "pmv")
    return ref.error_stats(got, want, ref.cat(case[0]), ref.cat(case[1]), ref.cat(case[2]), t, clip=clip, **hp)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in "pmv")


def _check_case(label, case, t, hp, max_norm, kinds=KINDS, gnorm_sq="float64"):
    """Every entry point in `kinds` on one case: statistics printed, p / m / v bit-identical between the entry points, each statistic
    at most 4 x torch-float32's.  gnorm_sq: the squared norm handed to the kernels (default: the float64 sum of squares)."""
    ss = ref.sumsq64(case[1])
    clip, want, tstat = ref.reference_and_torch32(*case, t, hp, max_norm)
    given = None if max_norm is None else (ss if gnorm_sq == "float64" else gnorm_sq)
    outs = {k: _step(k, case, t, hp, given, 0.0 if max_norm is None else max_norm) for k in kinds}
    stats = {k: _stats(o, ar, want, case, t, hp, clip) for k, (o, ar) in outs.items()}
    fmt = lambda s: "cm %.2f cv %.2f cp %.2f" % s
    print(f"{label} t={t} max_norm={max_norm} clip={clip:.3g}: torch-f32 {fmt(tstat)}")
    for k in kinds:
        print(f"    {k:12s} {fmt(stats[k])}")
    for k in kinds[1:]:
        assert _same(outs[kinds[0]][0], outs[k][0]), f"{k} and {kinds[0]} differ in bits ({label}, t={t}, max_norm={max_norm})"
    for k in kinds:
        for name, got, bar in zip(("cm", "cv", "cp"), stats[k], tstat):
            assert got <= 4 * bar, f"{k}: {name} = {got:.2f} u, torch-float32 {bar:.2f} u ({label}, t={t}, max_norm={max_norm})"
    return outs


CASES = [(t, ref.DEFAULT) for t in ref.STEPS] + [(7, ref.OTHER)]


@pytest.mark.parametrize("t,hp", CASES, ids=[f"t{t}" for t in ref.STEPS] + ["other"])
def test_one_adam_step_through_every_entry_point(t, hp):
    """The table of 16 tensors from realistic state at t = 1, 2, 7, 1000, 100000 (lr 1e-3, betas 0.9 / 0.999, eps 1e-8) and once with
    lr 0.25, betas 0.5 / 0.9, eps 1e-3; unclipped (gnorm_sq NULL) and clipped to norm 1 (a factor of about 1/540).  pccx_adam_step,
    pccx_adam_step_dev, pccx_adam_multi with host scalars and with a hand-built device state: bit-identical, and cm / cv / cp within
    4 x torch-float32's.

    Measured on one MI355X (cm / cv / cp; the four entry points agree in every bit, so one line each), unclipped:
        t        torch-float32       GPU                 GPU with 1.f - beta, 1.f - powf(beta, t) formed in float (before this test)
        1        1.20  2.71  5.24    1.20  2.71  5.91    4.95  217.9    5.0   (device-state entries: cp 117.8, not bit-identical)
        2        1.99  2.68  4.02    2.38  3.49  4.12    5.86  218.5  171.8   (116.9)
        7        1.84  2.54  4.01    2.37  3.45  4.54    5.70  218.3  132.6   (114.4)
        1000     1.88  2.42  3.70    2.37  2.85  4.28    5.52  217.6   66.7   (113.9)
        100000   1.95  2.26  4.84    2.38  3.02  4.04    5.67  216.9  113.9
        other    1.50  2.38  4.83    1.00  2.60  4.70    1.00    6.3    4.7
    clipped to norm 1 the GPU reads at most 3.45 / 6.33 / 5.90 (t = 2, 2, 1) where torch-float32 reads 2.45 / 3.46 / 5.11."""
    case = ref.draw_case(1000 + t, SIZES, t, hp["b1"], hp["b2"])
    for max_norm in (None, 1.0):
        _check_case("table", case, t, hp, max_norm)


def test_grid_stride_loop_of_the_single_tensor_kernels():
    """One tensor of 524288 + 257 elements: adam_kernel / adam_dev_kernel run 2048 workgroups, so every thread takes a second trip
    and the first 257 a third; the multi-tensor kernel covers the same tensor with 513 workgroups.  Same bar, bit-identical.
    Measured: GPU 2.85 / 5.28 / 4.83, torch-float32 2.56 / 4.19 / 4.28 (float constants: 6.25 / 217.3 / 133.1)."""
    t, hp = 7, ref.DEFAULT
    case = ref.draw_case(77, (524288 + 257,), t, hp["b1"], hp["b2"])
    _check_case("grid-stride", case, t, hp, 1.0)


def test_clip_factor_of_one_changes_no_bit_and_37_is_taken_from_the_norm():
    """norm < max_norm: clip = 1 and the step is bit for bit the gnorm_sq = NULL step.  norm = 37 max_norm: the reference clips by the
    float64 norm, same bar as everywhere.  Measured: GPU 2.66 / 4.70 / 4.36, torch-float32 2.87 / 4.61 / 3.83."""
    t, hp = 7, ref.DEFAULT
    case = ref.draw_case(78, SIZES, t, hp["b1"], hp["b2"])
    norm = math.sqrt(ref.sumsq64(case[1]))
    for kind in ("multi", "step"):
        free, _ = _step(kind, case, t, hp, None, 0.0)
        loose, _ = _step(kind, case, t, hp, norm * norm, 2.0 * norm)
        assert _same(free, loose), kind
    outs = _check_case("37x", case, t, hp, norm / 37.0, kinds=("multi", "step_dev"))
    assert not _same(outs["multi"][0], free)


def test_all_zero_gradients():
    """Zero gradients on zero moments: p bit-unchanged, m = v = 0, nothing NaN (0 / (0 + eps)).  On non-zero moments: the moments
    decay and p moves, as the reference has it.  Measured: GPU 1.40 / 1.21 / 3.99, torch-float32 1.00 / 1.21 / 3.71."""
    t, hp = 7, ref.DEFAULT
    ps, gs, ms, vs = ref.draw_case(79, SIZES, t, hp["b1"], hp["b2"])
    zeros = [np.zeros_like(g) for g in gs]
    for kind in ("multi", "step"):
        for given in (None, 0.0):
            out, ar = _step(kind, (ps, zeros, zeros, zeros), t, hp, given, 1.0)
            assert np.array_equal(out["p"], ar["p"].host), f"{kind}: p moved on zero gradients and zero moments"
            assert all(not a.any() for k in "mv" for a in ar[k].tensors(out[k]))
    _check_case("zero-grad", (ps, zeros, ms, vs), t, hp, 1.0, kinds=("multi", "step"), gnorm_sq=0.0)


def test_eps_decides_the_update_of_tiny_gradients():
    """|g| in 1e-10 .. 1e-7 on zero state at t = 1: the update is lr g / (|g| + eps), eps = 1e-8 in the middle of the range.  Absolute
    bound per element: half an ulp of p plus four times the largest error of torch's float32 Adam on the same tensor; eps inside the
    square root (denominator 1e-4) misses it by orders of magnitude.  Tensor 0 starts at p = 0, so the stored update is all there is.
    Measured (updates 9.9e-6 .. 9.1e-4): GPU worst 2.2e-10 and 2.5e-10, torch-float32 worst 1.8e-10 and 2.8e-10."""
    t, hp, n = 1, ref.DEFAULT, 2048
    rng = np.random.default_rng(80)
    gs = [(rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-10.0, -7.0, n)).astype(np.float32) for _ in range(2)]
    ps = [np.zeros(n, dtype=np.float32), (rng.standard_normal(n) * 1e-3).astype(np.float32)]
    zeros = [np.zeros(n, dtype=np.float32)] * 2
    case = (ps, gs, zeros, zeros)
    tp, _, _ = ref.torch_adam(*case, t, **hp)
    for kind in ("multi", "step"):
        out, ar = _step(kind, case, t, hp, None, 0.0)
        for i in range(2):
            P, _, _ = ref.adam_step64(ps[i], gs[i], zeros[i], zeros[i], t, **hp)
            err, terr = np.abs(ar["p"].tensors(out["p"])[i] - P), np.abs(tp[i] - P)
            allow = 0.5 * ref.ulp32(np.maximum(np.abs(ps[i]), np.abs(P))) + 4.0 * terr.max()
            print(f"eps regime {kind} tensor {i}: worst {err.max():.3e}, torch-f32 worst {terr.max():.3e}, update {np.abs(P - ps[i]).min():.2e} .. "
                  f"{np.abs(P - ps[i]).max():.2e}")
            assert terr.max() > 0 and bool((err <= allow).all())


def test_rows_left_out_of_the_table_are_untouched():
    """A parameter with grad None has no row: tensors 0, 7, 9 and the last are left out.  _step checks their p / m / v bit for bit, as
    it checks every guard word and every gradient in every test of this file; here the rows that ARE in the table are seen to move."""
    t, hp = 2, ref.DEFAULT
    case = ref.draw_case(81, SIZES, t, hp["b1"], hp["b2"])
    rows = [i for i in range(len(SIZES)) if i not in (0, 7, 9, len(SIZES) - 1)]
    norm2 = ref.sumsq64([case[1][i] for i in rows])
    outs = {k: _step(k, case, t, hp, norm2, 1.0, rows=rows) for k in KINDS}
    for k in KINDS[1:]:
        assert _same(outs["step"][0], outs[k][0]), k
    out, ar = outs["multi"]
    for i in rows:
        if SIZES[i]:
            assert all(not np.array_equal(ar[k].tensors(out[k])[i], ar[k].tensors(ar[k].host)[i]) for k in "pmv"), i


def test_device_step_counter_and_bias_corrections():
    """pccx_adam_advance_dev from t = 0, advanced 1, 2, 10 and 1000 times: the int32 counter exact, the two doubles within 1e-13
    relative of beta^t, the two floats within one ulp of float32(1 - beta^t), lr untouched."""
    from pccx import _lib
    for hp in (ref.DEFAULT, ref.OTHER):
        b1, b2 = hp["b1"], hp["b2"]
        for steps in (1, 2, 10, 1000):
            h = np.zeros(8, dtype=np.float32)
            h[0] = hp["lr"]
            h.view(np.float64)[2:4] = 1.0
            d = torch.from_numpy(h.copy()).cuda()
            for _ in range(steps):
                _lib.call("pccx_adam_advance_dev", d.data_ptr(), b1, b2, _st())
            got = d.cpu().numpy()
            assert got[0] == np.float32(hp["lr"]) and int(got.view(np.int32)[3]) == steps
            for k, b in enumerate((b1, b2)):
                pw, bc = float(got.view(np.float64)[2 + k]), got[1 + k]
                assert pw == b ** steps == 0.0 or abs(pw - b ** steps) <= 1e-13 * b ** steps, (steps, b, pw)
                want = np.float32(1.0 - b ** steps)
                assert abs(float(bc) - float(want)) <= float(np.spacing(want)), (steps, b, bc, want)


# ---- 3. pccx.train.Adam over a run ----------------------------------------------------------------------------------------------------
SHAPES = ((64, 3), (64,), (128, 64), (0,), (1025,), (16385,), (7,))
NO_GRAD, TRANSPOSED, NSTEPS, LR = 1, 2, 12, 1e-3


@functools.lru_cache(maxsize=None)
def _run_inputs():
    """-> (initial parameters, base gradients).  Parameter 1 never has a gradient; the gradient of parameter 2 is the transpose of a
    (64, 128) tensor.  Every non-empty base gradient has the same norm (a tensor or a row the norm kernel lost would move the clip
    factor by a tenth) and together they have norm 1, so the norm of step t is 1 + 0.3 sin t: above max_norm = 1 on steps 1-3 and
    7-9, below on 4-6 and 10-12."""
    rng = np.random.default_rng(90)
    p0 = [(rng.standard_normal(s) * 0.1).astype(np.float32) for s in SHAPES]
    base = [None if i == NO_GRAD else rng.standard_normal(s[::-1] if i == TRANSPOSED else s) for i, s in enumerate(SHAPES)]
    live = sum(1 for b in base if b is not None and b.size)
    return p0, [None if b is None else b / (math.sqrt(float((b * b).sum()) * live) if b.size else 1.0) for b in base]


@functools.lru_cache(maxsize=None)
def _grads(t):
    """the float32 gradients of step t (1-based), a function of t alone -- the runs are trajectories, not chaotic systems.  Parameter
    2's is stored as (64, 128): every run hands its transpose to the optimiser."""
    return [None if b is None else (b * (1.0 + 0.3 * math.sin(t))).astype(np.float32) for b in _run_inputs()[1]]


def _as_grad(i, g):
    return g.t() if i == TRANSPOSED else g


def _torch_run(dtype, params, first, lr_change=None, state=None, zero_norm_at=None, last=NSTEPS):
    """clip_grad_norm_(1.0) + torch.optim.Adam on the CPU in `dtype` over steps first .. last -> (parameters after the run, the
    optimiser).  lr_change: step before which the rate becomes 2.5e-4."""
    ps = [torch.nn.Parameter(ref.fresh(p, dtype)) for p in params]
    opt = torch.optim.Adam(ps, lr=LR)
    if state is not None:
        opt.load_state_dict(state)
    for t in range(first, last + 1):
        if t == lr_change:
            opt.param_groups[0]["lr"] = 2.5e-4
        for i, (q, g) in enumerate(zip(ps, _grads(t))):
            q.grad = None if g is None else _as_grad(i, ref.fresh(g, dtype))
        torch.nn.utils.clip_grad_norm_(ps, 0.0 if t == zero_norm_at else 1.0)
        opt.step()
    return [q.detach().numpy().copy() for q in ps], opt


@functools.lru_cache(maxsize=None)
def _reference(lr_change=None, zero_norm_at=None, last=NSTEPS):
    """the float64 and the float32 torch run from the initial parameters, computed once per variant and read-only afterwards"""
    p0 = _run_inputs()[0]
    return tuple(_torch_run(dt, p0, 1, lr_change, None, zero_norm_at, last)[0] for dt in (np.float64, np.float32))


def _state_copy(sd, dtype):
    """a deep copy of an optimiser state_dict on the CPU with the moments in `dtype`.  load_state_dict keeps the "step" tensors it is
    given and Adam.step increments them in place: a state handed to two optimisers un-copied would count both their steps."""
    return {"state": {i: {k: (v.detach().cpu().clone() if k == "step" else v.detach().cpu().to(dtype, copy=True)) for k, v in st.items()}
                      for i, st in sd["state"].items()},
            "param_groups": [dict(g) for g in sd["param_groups"]]}


def _gpu_params(params):
    return [torch.nn.Parameter(torch.from_numpy(np.array(p, dtype=np.float32, copy=True)).cuda()) for p in params]


def _gpu_grads(first, last):
    return {t: [None if g is None else torch.from_numpy(g.copy()).cuda() for g in _grads(t)] for t in range(first, last + 1)}


def _gpu_run(opt, first, last=NSTEPS, lr_change=None, deterministic=False, zero_norm_at=None):
    from pccx import train
    grads = _gpu_grads(first, last)
    for t in range(first, last + 1):
        if t == lr_change:
            opt.set_lr(2.5e-4)
        for i, (q, g) in enumerate(zip(opt.params, grads[t])):
            q.grad = None if g is None else _as_grad(i, g)
        max_norm = 0.0 if t == zero_norm_at else 1.0
        if deterministic:
            with train.step_scope("cuda", deterministic=True):
                opt.step(max_norm=max_norm)
        else:
            opt.step(max_norm=max_norm)
    return [q.detach().cpu().numpy() for q in opt.params]


def _gpu_graph_run(opt, first, last=NSTEPS, lr_change=None):
    """opt.step(max_norm=1.0) ALONE captured once on static gradient tensors, replayed last - first + 1 times; the next gradients are
    copied into the static tensors on the replays' stream (device to device), the host never waits in between"""
    from pccx import train
    grads = _gpu_grads(first, last)
    warm = train.Adam(_gpu_params(_run_inputs()[0]), lr=LR).make_capturable("cuda")       # loads the kernels outside the capture
    for i, (q, g) in enumerate(zip(warm.params, grads[first])):
        q.grad = None if g is None else _as_grad(i, g.clone())
    warm.step(max_norm=1.0)
    static = [None if g is None else torch.zeros_like(g) for g in grads[first]]
    for i, (q, s) in enumerate(zip(opt.params, static)):
        q.grad = None if s is None else _as_grad(i, s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(max_norm=1.0)
    opt.flush_table()
    for t in range(first, last + 1):
        if t == lr_change:
            opt.set_lr(2.5e-4)
        for s, g in zip(static, grads[t]):
            if s is not None:
                s.copy_(g)
        graph.replay()
        opt.t += 1                                                  # the host mirror, as GraphedTrainStep.step keeps it
    torch.cuda.synchronize()
    return [q.detach().cpu().numpy() for q in opt.params]


def _counter(opt):
    return int(opt.hyper.view(torch.int32)[3])


def _check_run(label, got, r64, r32):
    """per tensor: max |gpu - float64| <= 4 max |float32 torch - float64| + one float32 ulp of the largest parameter"""
    for i, (g, a, b) in enumerate(zip(got, r64, r32)):
        if a.size == 0:
            assert g.size == 0
            continue
        dev, tdev = float(np.abs(g - a).max()), float(np.abs(b - a).max())
        allow = 4.0 * tdev + float(ref.ulp32(np.abs(a).max()))
        print(f"{label} tensor {i} {SHAPES[i]}: gpu {dev:.3e}, torch-f32 {tdev:.3e}, bar {allow:.3e}")
        assert np.isfinite(g).all() and dev <= allow, (label, i, dev, allow)
    assert np.array_equal(got[NO_GRAD], _run_inputs()[0][NO_GRAD])       # no gradient: never in the table


def _make(capturable):
    from pccx import train
    opt = train.Adam(_gpu_params(_run_inputs()[0]), lr=LR)
    return opt.make_capturable("cuda") if capturable else opt


@pytest.mark.parametrize("mode", ["eager", "capturable", "graph"])
@pytest.mark.parametrize("lr_change", [None, 6], ids=["lr-fixed", "lr-changes"])
def test_twelve_steps_follow_the_float64_run(mode, lr_change):
    """(a) eager with host scalars, (b) make_capturable() eager, (c) one captured opt.step replayed twelve times, each with a fixed
    rate and (d) with set_lr(2.5e-4) before step 6.  opt.t and the device counter read 12 afterwards.
    Measured on one MI355X, max |p - float64| after step 12: (64, 3) 4.46e-8, (128, 64) 7.93e-8, (1025,) 4.26e-8, (16385,) 7.51e-8,
    (7,) 6.9e-9 -- in all three modes; the float32 torch run reads the same to three digits (what is left is the rounding of p
    itself) except 5.6e-9 on the last.  With the rate change: 4.17e-8 and 6.97e-8 for the first and the largest.  Bars 3.7e-8 (the
    seven elements) and 2.0e-7 .. 3.5e-7."""
    r64, r32 = _reference(lr_change)
    opt = _make(mode != "eager")
    got = _gpu_graph_run(opt, 1, NSTEPS, lr_change) if mode == "graph" else _gpu_run(opt, 1, NSTEPS, lr_change)
    _check_run(f"{mode} lr_change={lr_change}", got, r64, r32)
    assert opt.t == NSTEPS and (opt.hyper is None or _counter(opt) == NSTEPS)
    assert opt.lr == (LR if lr_change is None else 2.5e-4)


@pytest.mark.parametrize("capturable", [False, True], ids=["host-scalars", "capturable"])
def test_deterministic_switch_is_bit_identical_and_within_the_bar(capturable):
    """(e) every step inside train.step_scope(deterministic=True): the norm through pccx_sumsq_multi_det.  Two runs agree in every bit
    of the parameters and both moments."""
    r64, r32 = _reference()
    runs = []
    for _ in range(2):
        opt = _make(capturable)
        got = _gpu_run(opt, 1, deterministic=True)
        runs.append(got + [m.cpu().numpy() for m in opt.m] + [v.cpu().numpy() for v in opt.v])
        assert opt.t == NSTEPS and (opt.hyper is None or _counter(opt) == NSTEPS)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(*runs))
    _check_run("deterministic", runs[0][:len(SHAPES)], r64, r32)


def test_max_norm_zero_clips_to_nothing():
    """Adam.step(max_norm=0.0) on the fourth step: clip = 0 as clip_grad_norm_(params, 0.0) gives -- not "no clipping"; the moments
    decay and the parameters follow them."""
    r64, r32 = _reference(None, 4, 4)
    unclipped = _reference(None, None, 4)[0]
    assert max(float(np.abs(a - b).max()) for a, b in zip(r64, unclipped) if a.size) > 1e-5       # the references tell the two apart
    for capturable in (False, True):
        opt = _make(capturable)
        _check_run(f"max_norm=0 capturable={capturable}", _gpu_run(opt, 1, 4, zero_norm_at=4), r64, r32)
        assert opt.t == 4


def test_checkpoint_goes_to_torch_and_back_at_step_six():
    """(f) state_dict() after six steps loads into torch.optim.Adam over float64 copies of the parameters; both continue to step 12
    and the GPU stays within the bar of a float32 torch run continued from the same checkpoint.  The other way: a torch state at
    step 6 loads into train.Adam, host-scalar and capturable, the device counter reads 6, and steps 7-12 follow."""
    opt = _make(False)
    p6 = _gpu_run(opt, 1, 6)
    sd = opt.state_dict()
    assert opt.t == 6 and all(float(st["step"]) == 6.0 for st in sd["state"].values())
    r64, _ = _torch_run(np.float64, p6, 7, state=_state_copy(sd, torch.float64))
    r32, _ = _torch_run(np.float32, p6, 7, state=_state_copy(sd, torch.float32))
    _check_run("handover to torch", _gpu_run(opt, 7), r64, r32)
    assert opt.t == NSTEPS
    # the other way: six float64 torch steps, rounded to float32 as a checkpoint file of the reference holds them
    q6, topt = _torch_run(np.float64, _run_inputs()[0], 1, last=6)
    q6 = [q.astype(np.float32) for q in q6]
    tsd = _state_copy(topt.state_dict(), torch.float32)
    assert NO_GRAD not in tsd["state"]                              # torch keeps no state for a parameter that never had a gradient
    r64, _ = _torch_run(np.float64, q6, 7, state=_state_copy(tsd, torch.float64))
    r32, _ = _torch_run(np.float32, q6, 7, state=_state_copy(tsd, torch.float32))
    from pccx import train
    for capturable in (False, True):
        opt = train.Adam(_gpu_params(q6), lr=5.0)                   # lr, betas, eps and t come from the checkpoint
        if capturable:
            opt.make_capturable("cuda")
        opt.load_state_dict(_state_copy(tsd, torch.float32))
        assert opt.t == 6 and opt.lr == LR and (not capturable or _counter(opt) == 6)
        _check_run(f"handover from torch capturable={capturable}", _gpu_run(opt, 7), r64, r32)
        assert opt.t == NSTEPS and (not capturable or _counter(opt) == NSTEPS)
