"""The f16x2 planes kernels of csrc/planes.hip (the P = 2 instantiations: pccx_*_h2, pccx_absmax, pccx_dyn_scale) pinned layer by layer
against float64 matmuls of the same fp32 inputs and weights, at ragged shapes, plus the host rules that choose their power-of-two scales
(pccx/families.py: _pow2_floor, h2_act_scale, h2_w_scale, ibp_layer, Stack.chain4).

Bars.  A single layer is held to the bar of its bf16x3 twin (tests/test_families.py: test_planes_layers_ragged_shapes), atol 2e-5,
rtol 1e-5; a four-layer chain to that of test_planes_chain4_matches_layer_by_layer_and_float64, atol 3e-5, rtol 2e-5.  Every scale in these
kernels is a power of two, so where two forms differ only in where an activation lives, or in a power-of-two factor, the results are
compared bit for bit.  Inputs are drawn inside the bounds h2_prepare_stack is given ([-1, 1] per channel): the kernels are specified for
normalised inputs only.  Every float64 comparison prints the largest error it saw (pytest -s / -rP shows them).
"""
import copy
import math

import numpy as np
import pytest
import torch

ATOL, RTOL = 2e-5, 1e-5               # one layer (the bf16x3 twin's bar)
CH_ATOL, CH_RTOL = 3e-5, 2e-5         # a chain of four (the bf16x3 chain test's bar)
AR = "f16x2"
LAYER_CASES = [(1, 3, 3, True), (130, 3, 64, True), (257, 131, 128, False), (33, 1027, 128, True), (200, 64, 1024, False),
               (1000, 259, 7, True), (300, 512, 512, True)]
CHAIN_CASES = [(3, (3, 64, 64, 128), 32, 37), (131, (128, 128, 128, 256), 64, 21), (7, (20, 40, 64, 100), 32, 5),
               (70, (100, 128, 97, 200), 128, 3)]


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def _st():
    return torch.cuda.current_stream().cuda_stream


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, want, atol, rtol, tag):
    """assert_allclose that first prints the largest |error| and the largest error as a fraction of its bar"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    err = np.abs(got.astype(np.float64) - want)
    frac = err / (atol + rtol * np.abs(want))
    print(f"f64 {tag}: max|err| {err.max():.3e} = {frac.max():.3f} of the bar (atol {atol:g}, rtol {rtol:g})")
    np.testing.assert_allclose(got, want, atol=atol, rtol=rtol, err_msg=tag)


def _layer(rng, N, K, relu, bscale=1.0):
    """a FoldedLinear of the bf16x3 tests' distribution and its float64 (W, b)"""
    from pccx import families
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = (rng.standard_normal(N) * bscale).astype(np.float32)
    return families.FoldedLinear(torch.from_numpy(W), torch.from_numpy(b), relu, matmul=AR), W.astype(np.float64), b.astype(np.float64)


def _prepared(layers, lo=-1.0):
    from pccx import families
    stack = families.Stack(layers)
    families.h2_prepare_stack(stack, np.full(stack[0].K, lo), np.ones(stack[0].K))
    return stack


def _chain(rng, K0, widths, wmul=1.0, bmul=1.0):
    """the four-layer ReLU stack of the bf16x3 chain test (biases x 0.1), prepared, with its float64 [(W, b)]; wmul scales the first
    layer's weights and bmul every bias (exactly, for powers of two)"""
    from pccx import families
    layers, Ws, k = [], [], K0
    for i, nw in enumerate(widths):
        W = (rng.standard_normal((nw, k)) / np.sqrt(k)).astype(np.float32) * np.float32(wmul if i == 0 else 1.0)
        b = (rng.standard_normal(nw) * 0.1).astype(np.float32) * np.float32(bmul)
        layers.append(families.FoldedLinear(torch.from_numpy(W), torch.from_numpy(b), True, matmul=AR))
        Ws.append((W.astype(np.float64), b.astype(np.float64)))
        k = nw
    return _prepared(layers), Ws


def _f64(x, Ws, relus):
    h = x.astype(np.float64)
    for (W, b), relu in zip(Ws, relus):
        h = h @ W.T + b
        if relu:
            h = np.maximum(h, 0)
    return h


def _unit(rng, shape):
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


def _planes(x, layer, dyn=None):
    """fp32 rows (a cuda tensor) -> the operand planes of `layer` (times its sigma, times dyn[0])"""
    from pccx import families
    return families.group_planes(x, ar=AR, sig=layer.h2["sig"], dyn=dyn)[0]


def _with_bias(layers, biases):
    """the same prepared layers (same sigma, tau and weight stream) with other fp32 biases: the kernels' bias argument is sigma tau b"""
    out = []
    for l, b in zip(layers, biases):
        l2 = copy.copy(l)
        b = torch.from_numpy(np.asarray(b, np.float32)).to(l.b.device)
        l2.b, l2.h2 = b, dict(l.h2, b=(b * float(l.h2["sig"] * l.h2["tau"])).contiguous())
        out.append(l2)
    return out


def _restack(layers):
    """a Stack of layers that carry their f16x2 operands already"""
    from pccx import families
    st = families.Stack(layers)
    st.derived["h2"] = True
    return st


def _dyn_of(x):
    """{s, 1 / s} of a cuda tensor through pccx_absmax + pccx_dyn_scale"""
    from pccx import _lib
    am = torch.zeros(8, device="cuda")
    dyn = torch.full((2,), float("nan"), device="cuda")
    _lib.call("pccx_absmax", x.data_ptr(), x.numel(), am.data_ptr(), _st())
    _lib.call("pccx_dyn_scale", am.data_ptr(), 1.0, None, 0.0, 0.0, 1, dyn.data_ptr(), _st())
    return dyn


def _is_pow2(v):
    return v > 0 and math.frexp(v)[0] == 0.5


def _amax_checks(run, rows):
    """`run(amax)` writes `rows` again: the fold is bit-exact, leaves a larger value alone and raises a smaller one"""
    top = rows.abs().max()
    big = torch.full((8,), 2.0 * float(top) + 1.0, device="cuda")
    keep = big.clone()
    assert torch.equal(run(big), rows) and torch.equal(big, keep), "a larger value in the slot must survive"
    small = torch.full((8,), float(top) * 0.25, device="cuda")
    run(small)
    assert torch.equal(small.max(), top) and bool((small >= float(top) * 0.25).all())


# ---- 1, 2: one layer, row epilogue, amax8 -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N,relu", LAYER_CASES)
def test_single_layer_rows_and_amax(M, K, N, relu):
    """rows -> planes -> pccx_planes_gemm_h2 (row epilogue) against float64 at the bf16x3 twin's bar (MB = 4 and 8, MBS > 1, half a K
    block, part of an m-tile, one row, M no multiple of 16 / 128), and the amax8 side output: bit-equal to the largest |value| written --
    padded rows and channels past N add nothing -- and folded into, not written over."""
    rng = np.random.default_rng(100 + M + K + N)
    lyr, W, b = _layer(rng, N, K, relu)
    _prepared([lyr])
    x = _unit(rng, (M, K))
    pl = _planes(_cu(x), lyr)
    amax = torch.zeros(8, device="cuda")
    rows = lyr.planes(pl, M, 1, ar=AR, amax=amax)
    assert rows.shape == (M, N)
    _close(rows, _f64(x, [(W, b)], [relu]), ATOL, RTOL, f"layer {(M, K, N, relu)}")
    assert torch.equal(amax.max(), rows.abs().max())
    _amax_checks(lambda am: lyr.planes(pl, M, 1, ar=AR, amax=am), rows)


@pytest.mark.gpu
@pytest.mark.parametrize("ldo", [76, 75])
def test_rows_into_a_wider_buffer_leave_the_columns_past_N_alone(ldo):
    """ldo > N: the vector store path (ldo a multiple of 4; the last, partial quad of N = 70 still goes out in scalars) and the scalar
    one write the same values and nothing past column N."""
    from pccx import _lib
    M, K, N = 130, 35, 70
    rng = np.random.default_rng(7)
    lyr, W, b = _layer(rng, N, K, False)
    _prepared([lyr])
    x = _unit(rng, (M, K))
    pl = _planes(_cu(x), lyr)
    h = lyr.h2
    out = torch.full((M, ldo), float("nan"), device="cuda")
    _lib.call("pccx_planes_gemm_h2", pl.data_ptr(), M, K, h["ws"].data_ptr(), h["b"].data_ptr(), N, 0, 1, 0, 1.0 / (h["sig"] * h["tau"]), None, None,
              out.data_ptr(), ldo, _st())
    assert bool(torch.isnan(out[:, N:]).all()) and not bool(torch.isnan(out[:, :N]).any())
    assert torch.equal(out[:, :N], lyr.planes(pl, M, 1, ar=AR))
    _close(out[:, :N], _f64(x, [(W, b)], [False]), ATOL, RTOL, f"ldo {ldo}")


@pytest.mark.gpu
def test_amax_is_refused_where_the_header_forbids_it():
    from pccx import _lib, families
    rng = np.random.default_rng(8)
    lyr, _, _ = _layer(rng, 40, 35, True)
    _prepared([lyr])
    M = 128
    pl = _planes(_cu(_unit(rng, (M, 35))), lyr)
    amax = torch.zeros(8, device="cuda")
    for epilogue in (0, 2):
        with pytest.raises(_lib.PccxError, match=r"pccx_planes_gemm_h2 failed \(-1\).*row epilogue only"):
            lyr.planes(pl, M, epilogue, 32, ar=AR, sig_next=1.0, amax=amax)
    src = torch.zeros(1, M, 64, device="cuda")
    idx = families.identity_index(1, M, "cuda").view(1, M, 1)
    for epilogue in (0, 2):
        with pytest.raises(_lib.PccxError, match=r"pccx_planes_gemm_gather_h2 failed \(-1\).*row epilogue only"):
            lyr.planes(src, M, epilogue, 32, idx=idx, ar=AR, sig_next=1.0, amax=amax)
    stack, _ = _chain(rng, 7, (20, 40, 64, 100))
    pl = _planes(_cu(_unit(rng, (M, 7))), stack[0])
    with pytest.raises(_lib.PccxError, match=r"pccx_planes_chain4_h2 failed \(-1\).*group == 1"):
        families.run_planes(stack, pl, M, "max", 32, ar=AR, amax=amax)
    with pytest.raises(_lib.PccxError, match=r"pccx_planes_chain4_gather_h2 failed \(-1\).*group == 1"):
        families.run_planes(stack, torch.zeros(1, M, 32, device="cuda"), M, "max", 32, idx=idx, ar=AR, amax=amax)
    assert not bool(amax.any())


@pytest.mark.gpu
@pytest.mark.parametrize("M,Mfull", [(1, 16), (257, 272)])
def test_amax_ignores_the_padded_rows_of_the_last_tile(M, Mfull):
    """Planes made by group_planes repeat row M - 1 in the padded rows of the last tile, so there a fold without the row < M mask
    would go unnoticed.  Here the planes hold Mfull = 16 * ntiles rows whose tail rows are LARGER than the M real ones (inputs and
    biases of the real rows are 2^-6 of full size), and the kernels run on the first M: the rows written equal the first M of the full
    run, and amax8 is their maximum, not the tail's -- pccx_planes_gemm_h2 (MB = 4 and 8) and pccx_planes_chain4_h2.  The gathering
    forms compute the rows of the last tile themselves, from idx[min(r, M - 1)], so their padded rows cannot differ from row M - 1;
    their amax8 is checked at the same ragged M against the planes forms."""
    from pccx import families
    rng = np.random.default_rng(20 + M)
    small = np.float32(2.0 ** -6)

    def tail_heavy(K):
        x = _unit(rng, (Mfull, K))
        x[:M] *= small
        return x

    def check(run, pl):
        am_full, am = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
        full, rows = run(pl, Mfull, am_full), run(pl, M, am)
        assert rows.shape[0] == M and torch.equal(rows, full[:M])
        assert float(full[M:].abs().max()) > 4 * float(rows.abs().max()), "the tail rows must be the larger ones"
        assert torch.equal(am_full.max(), full.abs().max())
        assert torch.equal(am.max(), rows.abs().max()), "amax8 took a padded row"
        return rows

    for N in (40, 70):
        lyr, _, _ = _layer(rng, N, 35, False, bscale=float(small))
        _prepared([lyr])
        check(lambda pl, m, am: lyr.planes(pl, m, 1, ar=AR, amax=am), _planes(_cu(tail_heavy(35)), lyr))
    stack, _ = _chain(rng, 7, (20, 40, 64, 100), bmul=float(small))
    check(lambda pl, m, am: families.run_planes(stack, pl, m, "rows", ar=AR, amax=am), _planes(_cu(tail_heavy(7)), stack[0]))
    # gathering forms at the same M: equal to the planes forms, amax8 included
    if M > 1:
        Nsrc = 50
        feats, xyz = _cu(_unit(rng, (1, Nsrc, 4))), _cu(_unit(rng, (1, Nsrc, 3)))
        idx = _cu(rng.integers(-1, Nsrc, (1, M, 1)))
        src = families.padded_rows(feats, xyz)[0]
        pl = families.group_planes(feats, xyz, idx, ar=AR, sig=stack[0].h2["sig"])[0]
        lyr7, _, _ = _layer(rng, 70, 7, True)
        _prepared([lyr7])
        for run in (lambda x, i, am: lyr7.planes(x, M, 1, idx=i, ar=AR, amax=am),
                    lambda x, i, am: families.run_planes(stack, x, M, "rows", idx=i, ar=AR, amax=am)):
            am_g, am_p = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
            got = run(src, idx, am_g)
            assert torch.equal(got, run(pl, None, am_p))
            assert torch.equal(am_g.max(), got.abs().max()) and torch.equal(am_p.max(), am_g.max())


# ---- 3: planes epilogue, a chain kept in planes --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_layers_kept_in_planes():
    """35 -> 48 -> 40: epilogue 0 writes sigma_next * output as the next layer's planes.  The 48-channel middle has an odd number of
    16-channel tiles: its missing half block reads as zeros whatever the allocator left there (the same result on recycled, NaN-filled
    memory)."""
    from pccx import _lib, families
    rng = np.random.default_rng(5)
    l0, W0, b0 = _layer(rng, 48, 35, True)
    l1, W1, b1 = _layer(rng, 40, 48, False)
    stack = _prepared([l0, l1])
    M = 300
    x = _unit(rng, (M, 35))
    xc = _cu(x)

    def run():
        p1 = l0.planes(_planes(xc, l0), M, 0, ar=AR, sig_next=l1.h2["sig"])
        return l1.planes(p1, M, 1, ar=AR)

    first = run().clone()
    _close(first, _f64(x, [(W0, b0), (W1, b1)], [True, False]), ATOL, RTOL, "35->48->40")
    # dirty the allocator's free blocks: 64 MiB for its pool of large blocks, and, because the buffers of run() are small (planes of
    # 77 and 38 KB, rows of 48 KB, served from a pool of their own), NaN-filled tensors of exactly those sizes, which first take the
    # blocks run() has just freed
    lib = _lib.load()
    sizes = [lib.pccx_planes_floats_h2(M, 35), lib.pccx_planes_floats_h2(M, 48), M * 40]
    junk = [torch.full((16 << 20,), float("nan"), device="cuda")] + [torch.full((n,), float("nan"), device="cuda") for n in sizes for _ in range(8)]
    del junk
    assert torch.equal(run(), first)
    assert torch.equal(families.run_planes(stack, _planes(xc, l0), M, ar=AR), first)


# ---- 4: gather forms, max epilogue, members ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("ns,C", [(32, 0), (64, 5), (128, 128)])
def test_gather_max_and_member_forms(ns, C, relu):
    """gather + concat (-1 -> row 0) -> layer -> max over nsample against float64, and the identities between the forms, bit for bit:
    the gathering GEMM == group_planes + GEMM; the max epilogue == the row epilogue reduced by torch; member_max with every row a member
    == the max epilogue, with a random table == the masked maximum, with no member == 0 (ReLU) or -inf (none)."""
    from pccx import families
    rng = np.random.default_rng(40 + ns + C)
    B, Nsrc, Mq, N = 3, 50, 7, 70
    xyz = _unit(rng, (B, Nsrc, 3))
    feats = _unit(rng, (B, Nsrc, C)) if C else None
    idx = rng.integers(-1, Nsrc, (B, Mq, ns))
    lyr, W, b = _layer(rng, N, C + 3, relu)
    _prepared([lyr])
    f_, z_, i_ = _cu(feats) if C else None, _cu(xyz), _cu(idx)
    pl, rows = families.group_planes(f_, z_, i_, ar=AR, sig=lyr.h2["sig"])
    assert rows == B * Mq * ns
    got = lyr.planes(pl, rows, 2, ns, ar=AR)                                                    # (a)
    j = np.where(idx < 0, 0, idx)
    bi = np.arange(B)[:, None, None]
    g = np.concatenate(([feats[bi, j]] if C else []) + [xyz[bi, j]], axis=-1)                   # (B, Mq, ns, C + 3)
    want = _f64(g, [(W, b)], [relu]).max(axis=2).reshape(B * Mq, N)
    _close(got, want, ATOL, RTOL, f"gather max {(ns, C, relu)}")
    src, Cs = families.padded_rows(f_, z_)
    assert Cs == C + 3
    assert torch.equal(lyr.planes(src, rows, 2, ns, idx=i_, ar=AR), got)                        # (b)
    full = lyr.planes(pl, rows, 1, ar=AR)
    assert torch.equal(lyr.planes(src, rows, 1, idx=i_, ar=AR), full)
    assert torch.equal(got, full.view(-1, ns, N).amax(1))                                       # (c)
    member = _cu((rng.random(rows) < 0.3).astype(np.uint8))                                     # (d)
    member[:ns] = 0                                                                             # a group without a member
    got_m = lyr.planes(pl, rows, 2, ns, member=member, ar=AR)
    ref = torch.where(member.view(-1, ns, 1).bool(), full.view(-1, ns, N), torch.full_like(full.view(-1, ns, N), float("-inf"))).amax(1)
    empty = 0.0 if relu else float("-inf")
    assert torch.equal(got_m, ref.clamp(min=0) if relu else ref) and bool((got_m[0] == empty).all())
    assert torch.equal(lyr.planes(pl, rows, 2, ns, member=torch.ones_like(member), ar=AR), got)
    none = lyr.planes(pl, rows, 2, ns, member=torch.zeros_like(member), ar=AR)
    assert torch.equal(none, torch.full_like(none, empty))


# ---- 5: the four-layer chain ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K0,widths,ns,groups", CHAIN_CASES)
def test_chain4_matches_layer_by_layer_and_float64(K0, widths, ns, groups):
    """pccx_planes_chain4_h2 / _gather_h2 on both width patterns, full and ragged: against the float64 stack at the bf16x3 chain test's
    bar, BIT-identical to the same stack layer by layer (epilogue 0 with sigma_next, then the max / row epilogue: the same products in the
    same order, every scale a power of two, only where the activation lives differs) and to its gathering form; the row form's amax8;
    and the five scales Stack.chain4 hands the kernel."""
    from pccx import families
    rng = np.random.default_rng(900 + K0)
    stack, Ws = _chain(rng, K0, widths)
    assert families.chain4_fits(stack)
    _, sc, _ = stack.chain4(AR)
    h = [l.h2 for l in stack]
    assert sc.dtype == np.float32 and all(_is_pow2(float(v)) for v in sc)
    # the ratios telescope: the gathered rows take sigma_0 (= 2^15 for inputs within [-1, 1]), the planes in front of layer 3 carry
    # sigma_3, and the output rows no scale at all (each single ratio is pinned by the bit equality with layer by layer below)
    tau = [x["tau"] for x in h]
    assert float(sc[0]) == h[0]["sig"] == 2.0 ** 15
    assert float(np.prod(sc[:4].astype(np.float64))) * tau[0] * tau[1] * tau[2] == h[3]["sig"]
    assert float(np.prod(sc.astype(np.float64))) * float(np.prod(tau)) == 1.0
    rows = groups * ns
    x = _unit(rng, (rows, K0))
    pl = _planes(_cu(x), stack[0])
    got_max = families.run_planes(stack, pl, rows, "max", ns, ar=AR)
    amax = torch.zeros(8, device="cuda")
    got_rows = families.run_planes(stack, pl, rows, "rows", ar=AR, amax=amax)
    p = pl
    for i in range(3):
        p = stack[i].planes(p, rows, 0, ar=AR, sig_next=stack[i + 1].h2["sig"])
    assert torch.equal(got_max, stack[3].planes(p, rows, 2, ns, ar=AR)), "chain (max) != layer by layer"
    assert torch.equal(got_rows, stack[3].planes(p, rows, 1, ar=AR)), "chain (rows) != layer by layer"
    want = _f64(x, Ws, [True] * 4)
    _close(got_rows, want, CH_ATOL, CH_RTOL, f"chain rows {(K0, widths)}")
    _close(got_max, want.reshape(groups, ns, -1).max(1), CH_ATOL, CH_RTOL, f"chain max {(K0, widths)}")
    assert torch.equal(amax.max(), got_rows.abs().max())
    _amax_checks(lambda am: families.run_planes(stack, pl, rows, "rows", ar=AR, amax=am), got_rows)
    if K0 >= 4:
        Bq, Nsrc = 3, 40
        Mq = groups // Bq
        feats, xyz = _unit(rng, (Bq, Nsrc, K0 - 3)), _unit(rng, (Bq, Nsrc, 3))
        idx = rng.integers(-1, Nsrc, (Bq, Mq, ns))
        f_, z_, i_ = _cu(feats), _cu(xyz), _cu(idx)
        pl2, rows2 = families.group_planes(f_, z_, i_, ar=AR, sig=stack[0].h2["sig"])
        src = families.padded_rows(f_, z_)[0]
        g_max = families.run_planes(stack, src, rows2, "max", ns, idx=i_, ar=AR)
        assert torch.equal(g_max, families.run_planes(stack, pl2, rows2, "max", ns, ar=AR)), "gather (max) != planes"
        assert torch.equal(families.run_planes(stack, src, rows2, "rows", idx=i_, ar=AR), families.run_planes(stack, pl2, rows2, "rows", ar=AR))
        j = np.where(idx < 0, 0, idx)
        bi = np.arange(Bq)[:, None, None]
        g = np.concatenate([feats[bi, j], xyz[bi, j]], axis=-1)
        _close(g_max, _f64(g, Ws, [True] * 4).max(axis=2).reshape(Bq * Mq, -1), CH_ATOL, CH_RTOL, f"chain gather {(K0, widths)}")


@pytest.mark.gpu
def test_chain4_refuses_widths_outside_both_patterns():
    from pccx import _lib, families
    rng = np.random.default_rng(3)
    stack, _ = _chain(rng, 3, (64, 64, 64, 128))
    assert not families.chain4_fits(stack)
    M = 64
    ws, sc, a = stack.chain4(AR)
    pl = _planes(_cu(_unit(rng, (M, 3))), stack[0])
    out = torch.zeros(M, 128, device="cuda")
    idx = families.identity_index(1, M, "cuda")
    src = torch.zeros(1, M, 32, device="cuda")
    for group in (1, 32):
        with pytest.raises(_lib.PccxError, match=r"\(-1\).*unsupported widths"):
            _lib.call("pccx_planes_chain4_h2", pl.data_ptr(), M, 3, ws.data_ptr(), *a, group, sc.ctypes.data, None, None, out.data_ptr(), 128, _st())
        with pytest.raises(_lib.PccxError, match=r"\(-1\).*unsupported widths"):
            _lib.call("pccx_planes_chain4_gather_h2", src.data_ptr(), 32, idx.data_ptr(), M, M, M, 3, ws.data_ptr(), *a, group, sc.ctypes.data, None,
                      None, out.data_ptr(), 128, _st())
    assert not bool(out.any())


# ---- 6: exact scale equivariance -----------------------------------------------------------------------------------------------------
def _equivariance(build, K, rows_of, atol, rtol):
    """build(wmul, bmul) -> (prepared stack, [(W, b)] float64, relus); rows_of(stack, planes, dyn) -> fp32 rows; (atol, rtol) the form's own
    float64 bar.  See the two tests below."""
    rng = np.random.default_rng(61)
    M = 257 if K == 131 else 160
    x = _unit(rng, (M, K))
    xc = _cu(x)
    stack, Ws, relus = build(1.0, 1.0)
    pl = _planes(xc, stack[0])
    base = rows_of(stack, pl, None)
    _close(base, _f64(x, Ws, relus), atol, rtol, f"equivariance base K={K}")
    # weights: 2^e on the first layer's weights and every bias scales every activation by 2^e; tau_0 and sigma_1.. absorb the factor,
    # so every plane and every accumulator is the same and only the final un-scaling differs
    for e in (-10, 7):
        s2, _, _ = build(2.0 ** e, 2.0 ** e)
        assert all(torch.equal(a.h2["ws"], b.h2["ws"]) for a, b in zip(s2, stack)) and s2[0].h2["tau"] == stack[0].h2["tau"] * 2.0 ** -e
        assert torch.equal(rows_of(s2, _planes(xc, s2[0]), None), base * 2.0 ** e), f"weights x 2^{e}"
    # inputs: m x with the dyn of the data and biases m b
    biases = [b for _, b in Ws]
    for m in (64.0, 1.0 / 64.0):
        xm = xc * m
        dyn = _dyn_of(xm)
        sm = _restack(_with_bias(stack, [b * m for b in biases]))
        got = rows_of(sm, _planes(xm, sm[0], dyn), dyn)
        if m > 1:
            assert dyn.tolist() == [1.0 / m, m]
            assert torch.equal(_planes(xm, sm[0], dyn), pl)
            assert torch.equal(got, base * m), "dyn: the result for (m x, m b) is m times the result for (x, b)"
        else:
            assert dyn.tolist() == [1.0, 1.0], "s <= 1: small inputs are not blown up"
            _close(got, _f64(x * np.float32(m), [(W, b * m) for W, b in Ws], relus), ATOL, RTOL, f"dyn m=2^-6 K={K}")
    b37 = [(b * 37.0).astype(np.float32) for b in biases]
    x37 = (x * np.float32(37.0)).astype(np.float32)
    dyn = _dyn_of(_cu(x37))
    assert dyn.tolist() == [2.0 ** -6, 2.0 ** 6]
    sm = _restack(_with_bias(stack, b37))
    got = rows_of(sm, _planes(_cu(x37), sm[0], dyn), dyn)
    _close(got, _f64(x37, [(W, b.astype(np.float64)) for (W, _), b in zip(Ws, b37)], relus), ATOL * 37, RTOL, f"x37 K={K}")


@pytest.mark.gpu
def test_scale_equivariance_single_layer():
    """Powers of two commute with every rounding of these kernels while nothing under- or overflows, so: 2^e (W, b) gives bit-exactly
    2^e times the rows (e = -10, 7); (64 x, 64 b) under the dyn of the data gives bit-exactly 64 times the rows of (x, b) without dyn;
    (x / 64, b / 64) keeps s = 1 and still meets the float64 bar with atol unchanged; a factor of 37 meets the bar scaled by 37."""
    from pccx import families

    def build(wmul, bmul):
        rng = np.random.default_rng(62)
        W = (rng.standard_normal((128, 131)) / np.sqrt(131)).astype(np.float32) * np.float32(wmul)
        b = rng.standard_normal(128).astype(np.float32) * np.float32(bmul)
        lyr = families.FoldedLinear(torch.from_numpy(W), torch.from_numpy(b), False, matmul=AR)
        return _prepared([lyr]), [(W.astype(np.float64), b.astype(np.float64))], [False]

    _equivariance(build, 131, lambda st, pl, dyn: st[0].planes(pl, 257, 1, ar=AR, dyn=dyn), ATOL, RTOL)


@pytest.mark.gpu
def test_scale_equivariance_chain4():
    """the same identities through pccx_planes_chain4_h2 (rows) on the ragged stack 7 -> (20, 40, 64, 100): the biases of all four
    layers take dyn[0], the rows dyn[1]"""
    from pccx import families

    def build(wmul, bmul):
        stack, Ws = _chain(np.random.default_rng(63), 7, (20, 40, 64, 100), wmul, bmul)
        return stack, Ws, [True] * 4

    _equivariance(build, 7, lambda st, pl, dyn: families.run_planes(st, pl, 160, "rows", ar=AR, dyn=dyn), CH_ATOL, CH_RTOL)


# ---- 7: rows_affine_planes_h2, fold_planes_h2 ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C", [128, 512])
@pytest.mark.parametrize("Ks", [2, 3])
def test_rows_affine_planes_equal_the_planes_of_the_rows(C, Ks):
    """pccx_rows_affine_planes_h2 == group_planes of the fp32 rows pccx_rows_affine_small writes (the same fmaf chain), for the grid
    form (mod = P) and the per-row form (mod = 0), M = 3 * 45 * 45 (no multiple of 16), with and without dyn and ReLU"""
    from pccx import _lib, families
    rng = np.random.default_rng(70 + C + Ks)
    B, P = 3, 45 * 45
    M, rho = B * P, 2.0 ** 12                                                       # |value| <= 1 + Ks: rho |value| within fp16's range
    base, w = _cu(_unit(rng, (B, C))), _cu(_unit(rng, (C, Ks)))
    dyn2 = torch.tensor([0.5, 2.0], device="cuda")
    for mod in (P, 0):
        x = _cu(_unit(rng, (P if mod else M, Ks)))
        for relu, dyn in ((True, None), (False, dyn2)):
            rows = families.rows_affine_small(base, P, x, mod, w, relu, M)
            got = families.rows_affine_small(base, P, x, mod, w, relu, M, planes=AR, rho=rho, dyn=dyn)
            assert torch.equal(got, families.group_planes(rows, ar=AR, sig=rho, dyn=dyn)[0]), (mod, relu)
    out = torch.empty(_lib.load().pccx_planes_floats_h2(M, C), device="cuda")
    for bad in (0.0, -1.0):
        with pytest.raises(_lib.PccxError, match=r"\(-1\).*pccx_rows_affine_planes_h2: rho must be"):
            _lib.call("pccx_rows_affine_planes_h2", base.data_ptr(), C, P, x.data_ptr(), Ks, Ks, 0, w.data_ptr(), 1, M, bad, None, out.data_ptr(), _st())


@pytest.mark.gpu
def test_fold_planes_h2_equal_the_planes_of_the_concatenated_rows():
    """pccx_fold_planes_h2 (no Python wrapper, no caller): [a tiled | b repeated] and [a | b repeated] straight to f16x2 planes == the
    concatenated rows converted (the two cases of the bf16x3 test)"""
    from pccx import _lib, families
    rng = np.random.default_rng(71)
    rho, M = 2.0 ** 13, 70
    dyn2 = torch.tensor([0.25, 4.0], device="cuda")
    b2 = _unit(rng, (7, 37))
    for a, mod0 in ((_unit(rng, (10, 2)), 10), (_unit(rng, (70, 3)), 0)):
        cat = np.concatenate([np.tile(a, (7, 1)) if mod0 else a, np.repeat(b2, 10, axis=0)], axis=1)
        C0 = a.shape[1]
        at, bt = _cu(a), _cu(b2)
        for dyn in (None, dyn2):
            out = torch.full((_lib.load().pccx_planes_floats_h2(M, C0 + 37),), float("nan"), device="cuda")
            _lib.call("pccx_fold_planes_h2", at.data_ptr(), C0, C0, mod0, bt.data_ptr(), 37, 37, 10, M, rho, dyn.data_ptr() if dyn is not None else None,
                      out.data_ptr(), _st())
            assert torch.equal(out, families.group_planes(_cu(cat), ar=AR, sig=rho, dyn=dyn)[0]), mod0
    for bad in (0.0, -2.0):
        with pytest.raises(_lib.PccxError, match=r"\(-1\).*pccx_fold_planes_h2: rho must be"):
            _lib.call("pccx_fold_planes_h2", at.data_ptr(), C0, C0, 0, bt.data_ptr(), 37, 37, 10, M, bad, None, out.data_ptr(), _st())


# ---- 8: absmax, dyn_scale ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 16385, 5_000_000])
def test_absmax(n):
    """max |x| bit for bit (one block, a partial wave, two blocks, the grid at its 256-block cap), the maximum in the last and in the
    first element and negative, all zeros, folded into a slot that holds something, n == 0 a no-op"""
    from pccx import _lib
    rng = np.random.default_rng(n)
    x = _unit(rng, n)
    for at, v in ((n - 1, -3.5), (0, 3.25), (None, 0.0)):
        xs = np.zeros_like(x) if at is None else x.copy()
        if at is not None:
            xs[at] = v
        xt = _cu(xs)
        am = torch.zeros(8, device="cuda")
        _lib.call("pccx_absmax", xt.data_ptr(), n, am.data_ptr(), _st())
        assert torch.equal(am.max(), xt.abs().max()) and float(am.max()) == abs(v) and bool((am >= 0).all())
        hi, lo = torch.full((8,), 10.0, device="cuda"), torch.full((8,), 1.0, device="cuda")
        _lib.call("pccx_absmax", xt.data_ptr(), n, hi.data_ptr(), _st())
        _lib.call("pccx_absmax", xt.data_ptr(), n, lo.data_ptr(), _st())
        assert bool((hi == 10.0).all()) and float(lo.max()) == max(abs(v), 1.0) and bool((lo >= 1.0).all())
        _lib.call("pccx_absmax", None, 0, lo.data_ptr(), _st())
        assert float(lo.max()) == max(abs(v), 1.0)


def _dyn_rule(v1, a1, v2, a2, add, combine):
    """include/pccx.h: s = the largest power of two <= 1 (and >= 2^-60) with bound s <= 1, bound = (max or sum of a1 m1, a2 m2) + add in
    fp32, inflated by (1 + 2^-20) (csrc/planes.hip) -- so a bound of exactly 2^k gives 2^-(k+1)"""
    f = np.float32
    bound = float(((max(f(a1) * f(v1), f(a2) * f(v2)) if combine else f(a1) * f(v1) + f(a2) * f(v2)) + f(add)) * f(1 + 2.0 ** -20))
    s = 1.0 if bound <= 1.0 else max(2.0 ** -math.ceil(math.log2(bound)), 2.0 ** -60)
    return s, bound


@pytest.mark.gpu
def test_dyn_scale():
    from pccx import _lib
    cases = [  # m1, a1, m2, a2, add, combine -> s          (products and sums exact in fp32)
        (0.0, 1.0, None, 0.0, 0.0, 1, 1.0), (0.0, 1.0, 0.0, 1.0, 0.0, 0, 1.0), (0.3, 1.0, None, 0.0, 0.0, 1, 1.0),
        (1.0, 1.0, None, 0.0, 0.0, 1, 0.5), (1.5, 1.0, None, 0.0, 0.0, 0, 0.5), (64.0, 1.0, None, 0.0, 0.0, 1, 2.0 ** -7),
        (2.0 ** 61, 1.0, None, 0.0, 0.0, 1, 2.0 ** -60), (0.75, 2.0, 0.5, 3.0, 0.25, 0, 0.25), (0.75, 2.0, 0.5, 3.0, 0.25, 1, 0.5),
        (0.75, 2.0, 0.5, 5.0, 0.25, 1, 0.25), (0.25, 1.0, 3.0, 1.0, 0.0, 1, 0.25), (0.25, 1.0, None, 7.0, 0.5, 0, 1.0),
        (0.25, 1.0, None, 7.0, 0.75, 0, 0.5), (0.0, 1.0, None, 0.0, 5.0, 1, 0.125)]
    for i, (v1, a1, v2, a2, add, comb, want) in enumerate(cases):
        m1 = torch.zeros(8, device="cuda")
        m1[i % 8] = v1                                                             # the maximum of the eight replicas, wherever it sits
        m2 = None
        if v2 is not None:
            m2 = torch.zeros(8, device="cuda")
            m2[(3 * i) % 8] = v2
        dyn = torch.full((2,), float("nan"), device="cuda")
        _lib.call("pccx_dyn_scale", m1.data_ptr(), a1, m2.data_ptr() if m2 is not None else None, a2, add, comb, dyn.data_ptr(), _st())
        s, inv = dyn.tolist()
        rule, bound = _dyn_rule(v1, a1, v2 or 0.0, a2 if v2 is not None else 0.0, add, comb)
        assert s == want == rule, (i, s, want, rule)
        assert inv == 1.0 / s and _is_pow2(s) and s <= 1.0 and (bound * s <= 1.0 or s == 2.0 ** -60) and (s == 1.0 or 2 * s * bound > 1.0), i
    with pytest.raises(_lib.PccxError, match=r"\(-1\).*pccx_dyn_scale: bad arguments"):
        _lib.call("pccx_dyn_scale", m1.data_ptr(), 1.0, None, 0.0, 0.0, 2, dyn.data_ptr(), _st())


# ---- 9: the host's scale rules (no GPU) ----------------------------------------------------------------------------------------------
def test_pow2_floor_act_scale_and_w_scale():
    from pccx.families import _pow2_floor, h2_act_scale, h2_w_scale
    up, dn = 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53
    for e in (-1074, -1022, -40, -1, 0, 1, 15, 100, 1023):
        p = math.ldexp(1.0, e)
        assert _pow2_floor(p) == p
        if e > -1022:
            assert _pow2_floor(p * up) == p and _pow2_floor(p * dn) == p / 2
    assert _pow2_floor(3.0) == 2.0 and _pow2_floor(0.75) == 0.5 and _pow2_floor(5e-324) == 5e-324
    for bound in (1.0, up, dn, 2.0, 0.5, 3.7, 1e-3, 123456.0, 2.0 ** 15, 2.0 ** 15 * up, 2.0 ** 15 * dn, 2.0 ** -40, 2.0 ** -40 * up, np.float32(0.3)):
        sig = h2_act_scale(bound)
        assert _is_pow2(sig) and sig * bound <= 2.0 ** 15 < 2 * sig * bound, bound
    assert h2_act_scale(1.0) == 2.0 ** 15 and h2_act_scale(up) == 2.0 ** 14 and h2_act_scale(dn) == 2.0 ** 15
    # 0 and tiny bounds stop at the floor of 2^-40: sigma = 2^55, still within fp32 and sigma * bound <= 2^15
    assert h2_act_scale(0.0) == h2_act_scale(1e-30) == h2_act_scale(2.0 ** -41) == 2.0 ** 55
    for m in (1.0, float(np.float32(up)), dn, 0.37, 16384.0, 16384.0 * up, 16384.0 * dn, 2.0 ** -100, 3e4):
        W = np.array([[0.0, -m], [m / 3, m / 2]])
        tau = h2_w_scale(W)
        assert _is_pow2(tau) and tau * m <= 2.0 ** 14 < 2 * tau * m, m
        assert h2_w_scale(-W) == tau and h2_w_scale(W.astype(np.float32)) == h2_w_scale(W.astype(np.float32).astype(np.float64))
    assert h2_w_scale(np.ones((2, 2))) == 2.0 ** 14 and h2_w_scale(np.full((1, 3), up)) == 2.0 ** 13
    assert h2_w_scale(np.zeros((3, 4))) == 1.0 and h2_w_scale(np.zeros((0, 4))) == 1.0


@pytest.mark.parametrize("seed", range(6))
def test_ibp_layer_bounds_contain_every_activation(seed):
    """the interval bounds that choose sigma are sound: through three layers the float64 activations of every corner input (the input
    that maximises one output of the first layer, and its mirror), of 1000 random inputs and for every bias multiplier s <= 1 stay inside
    the propagated [lo, hi]"""
    from pccx.families import ibp_layer
    rng = np.random.default_rng(seed)
    K = int(rng.integers(3, 65))
    lo0, hi0 = -(rng.random(K) < 0.5).astype(np.float64), np.ones(K)               # post-ReLU channels in [0, 1], the others in [-1, 1]
    layers = []
    for _ in range(3):
        N = int(rng.integers(3, 65))
        layers.append((rng.standard_normal((N, K)) / np.sqrt(K), rng.standard_normal(N), bool(rng.integers(0, 2))))
        K = N
    bounds, lo, hi = [], lo0, hi0
    for W, b, relu in layers:
        lo, hi = ibp_layer(W, b, lo, hi, relu)
        assert lo.shape == hi.shape == b.shape and bool((lo <= hi).all())
        bounds.append((lo, hi))
    W0 = layers[0][0]
    corners = np.where(W0 > 0, hi0, lo0)
    xs = np.concatenate([corners, np.where(W0 > 0, lo0, hi0), lo0 + (hi0 - lo0) * rng.random((1000, len(lo0))), lo0[None], hi0[None]])
    for s in (1.0, 2.0 ** -3, 2.0 ** -20):
        h = xs
        for (W, b, relu), (lo, hi) in zip(layers, bounds):
            h = h @ W.T + b * s
            if relu:
                h = np.maximum(h, 0)
            assert bool((h >= lo).all()) and bool((h <= hi).all()), (seed, s)


def test_chain4_scales_are_the_ratios_of_the_layer_scales():
    """Stack.chain4("f16x2"): {sigma_0, sigma_l / (sigma_{l-1} tau_{l-1}) for l = 1..3, 1 / (sigma_3 tau_3)}, all powers of two, from layers
    packed on the host with the scales h2_prepare_stack's rules give them (the GPU chain test checks the prepared stacks themselves)"""
    from pccx import families
    rng = np.random.default_rng(4)
    layers, K = [], 7
    lo, hi = -np.ones(K), np.ones(K)
    for N in (20, 40, 64, 100):
        W = (rng.standard_normal((N, K)) / np.sqrt(K) * rng.choice([0.01, 1.0, 50.0])).astype(np.float32)
        b = rng.standard_normal(N).astype(np.float32)
        l = families.FoldedLinear(torch.from_numpy(W), torch.from_numpy(b), True, device="cpu", matmul=AR)
        sig, tau = families.h2_act_scale(max(np.abs(lo).max(), np.abs(hi).max())), families.h2_w_scale(l.W_host)
        l.h2 = dict(sig=sig, tau=tau, ws=torch.zeros(4), b=l.b * float(sig * tau))
        lo, hi = families.ibp_layer(l.W_host, l.b_host, lo, hi, True)
        layers.append(l)
        K = N
    ws, sc, a = families.Stack(layers).chain4(AR)
    sig, tau = [l.h2["sig"] for l in layers], [l.h2["tau"] for l in layers]
    assert sc.dtype == np.float32 and sc.shape == (5,) and ws.numel() == 16 and len(a) == 8 and a[1::2] == [20, 40, 64, 100]
    assert sig[0] == 2.0 ** 15 and len(set(sig)) > 1
    assert [float(v) for v in sc] == [sig[0], sig[1] / (sig[0] * tau[0]), sig[2] / (sig[1] * tau[1]), sig[3] / (sig[2] * tau[2]), 1.0 / (sig[3] * tau[3])]
    assert all(_is_pow2(float(v)) for v in sc)
    # the ratios telescope: the planes in front of layer 3 carry sigma_3, and the output rows carry no scale at all
    assert float(sc[0]) * float(sc[1]) * float(sc[2]) * float(sc[3]) * tau[0] * tau[1] * tau[2] == sig[3]
    assert float(np.prod(sc.astype(np.float64))) * np.prod(tau) == 1.0
