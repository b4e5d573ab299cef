"""Cases and plain references for the probability model's tables (tests/test_prob_cases_cpu.py, tests/test_prob_float64.py).  No GPU.

The table stage -- softmax over the L levels, pn_kit.pmf_to_cdf, torchac's 16-bit conversion -- exists in five copies on the device
(csrc/prob.hip, softmax_cdf_kernel in csrc/linear.hip).  Two restatements of it live here:

    tables32(logits)   numpy float32, the reference's statements in their order: max, sequential sum of exp, division, sequential
                       cumsum, min(., 1), rint(cv * (65536 - L)) + l, kept to 16 bits
    tables64(logits)   the same in float64: pmf, clamped cdf, and the UNROUNDED x64 = cdf * (65536 - L)

and the assertions that both test files share.  Every margin is derived from tables32's own distance to tables64 on the same
logits (e_ref), never from the code under test.

exact_logit_state_dict() gives weights whose logits are exact in fp32 under any summation order: model_pn's output meets zero
weights, the two hidden layers pass xyz through a 3x3 identity (xyz > 0, so the ReLUs keep it), and the last layer holds small
integers and a bias in eighths.  With centres on the grid (q + 0.5) / 128 every product and partial sum is a multiple of 1/256 far
below 2^24 of them, so the fused kernels, the generic layers, the fp32 oracle and float64 all see the same logits, and the table
stage can be compared with float64 on its own.
"""
import numpy as np
import torch

from oracle import ref_model

# (d, L) of the exact-logit cases; d * L <= 128, d <= 16, L <= 15: the fused kernels' shapes
#   (5, 7):  d*L = 35, d*(L+1) = 40 -> the distinct kernel's prob_store_pmf<1> with prob_store_cdf<4>
#   (3, 4):  d*L = 12, d*(L+1) = 15 -> prob_store_pmf<4> with prob_store_cdf<1>
#   (1, 15): 15, 16 -> <1> with <4> again; (9, 14): 126, 135 -> both <1>; (16, 1): one level, every table is [0, 65536 -> 0]
DL_CASES = [(16, 7), (5, 7), (3, 4), (1, 15), (9, 14), (16, 8), (8, 15), (16, 1)]
AMPS = [1, 8, 64]
S_FUSED = [16, 48, 64, 80]
GENERIC_CASES = [(16, 7, 24), (5, 7, 24), (4, 17, 48)]         # (d, L, S): S % 16 != 0 twice, L above 15
SHARE_CAP = {False: 0.005, True: 0.01}                         # key: L >= 64
FACTOR = 4.0                                                   # device expf and division may each sit an ulp or two from numpy's


def store_widths(d, L):
    """(W of prob_store_pmf, W of prob_store_cdf) that prob_forward_distinct_kernel takes on 16-byte-aligned outputs."""
    return (4 if d * L % 4 == 0 else 1, 4 if d * (L + 1) % 4 == 0 else 1)


def grid_centres(B, S, seed):
    """(B, S, 3) fp32 centres (q + 0.5) / 128, q uniform in 0..127: eight significant bits, exact in every operand split."""
    q = np.random.default_rng(seed).integers(0, 128, size=(B, S, 3))
    return ((q + 0.5) / 128.0).astype(np.float32)


def fused_centres(S):
    """The three clouds that run() sees at S centres, on the CPU and on the GPU alike."""
    return grid_centres(3, S, 400 + S)


def exact_case(d, L, amp):
    return exact_logit_state_dict(d, L, 300 + d * L, amp)


def repeated_centres(S, counts, seed):
    """(len(counts), S, 3) grid centres, cloud b with exactly counts[b] distinct rows, every one used, in an unrelated order."""
    rng = np.random.default_rng(seed)
    out = []
    for n in counts:
        while True:
            rows = grid_centres(1, n, int(rng.integers(1 << 30)))[0]
            if len(np.unique(rows, axis=0)) == n:
                break
        pick = np.concatenate([rng.permutation(n), rng.integers(0, n, size=S - n)])
        out.append(rows[rng.permutation(pick)])
    return np.stack(out)


def exact_logit_state_dict(d, L, seed, amp):
    """State dict of a ConditionalProbabilityModel(L, d) whose logits are A . xyz + b exactly (module docstring)."""
    m = ref_model.ConditionalProbabilityModel(L, d)
    sd = ref_model.seeded_state_dict(m, seed)                  # model_pn as usual: its output is multiplied by zeros
    rng = np.random.default_rng(seed + 1000 * amp + 7)
    for key in ("model_mlp.0", "model_mlp.2"):
        w = torch.zeros_like(sd[key + ".weight"])
        w[0, 0], w[1, 1], w[2, 2] = 1.0, 1.0, 1.0              # xyz are the first three inputs (AE.py:115) and stay channels 0..2
        sd[key + ".weight"], sd[key + ".bias"] = w, torch.zeros_like(sd[key + ".bias"])
    w = torch.zeros_like(sd["model_mlp.4.weight"])
    w[:, :3, 0, 0] = torch.from_numpy(rng.integers(-amp, amp + 1, size=(d * L, 3)).astype(np.float32))
    sd["model_mlp.4.weight"] = w
    sd["model_mlp.4.bias"] = torch.from_numpy((rng.integers(-8 * amp, 8 * amp + 1, size=d * L) / 8.0).astype(np.float32))
    return sd


def intended_logits(sd, x, d, L):
    """float64 (B, S, d, L): A . xyz + b of an exact-logit state dict on centres x (B, S, 3)."""
    A = sd["model_mlp.4.weight"][:, :3, 0, 0].numpy().astype(np.float64)
    b = sd["model_mlp.4.bias"].numpy().astype(np.float64)
    lg = np.asarray(x, np.float64) @ A.T + b
    return lg.reshape(x.shape[0], x.shape[1], d, L)


# --------------------------------------------------------------------------- the table stage, restated
def softmax32(logits):
    lg = np.asarray(logits, np.float32)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    s = np.zeros(lg.shape[:-1], np.float32)
    for l in range(lg.shape[-1]):
        s = s + e[..., l]
    return e / s[..., None]


def cdf32(pmf):
    """pmf fp32 (..., L) -> (cdf fp32 (..., L+1), x32 = fp32(cv * (65536 - L)), cdf_int int32): pmf_to_cdf + torchac's conversion."""
    pmf = np.asarray(pmf, np.float32)
    L = pmf.shape[-1]
    cdf = np.zeros(pmf.shape[:-1] + (L + 1,), np.float32)
    run = np.zeros(pmf.shape[:-1], np.float32)
    for l in range(L):
        run = run + pmf[..., l]
        cdf[..., l + 1] = np.minimum(run, np.float32(1.0))
    x32 = cdf * np.float32(65536 - L)
    return cdf, x32, int_from_float_cdf(cdf)


def int_from_float_cdf(cdf):
    """torchac: round-half-even(cdf * (2^16 - L)) + arange(L + 1), kept to 16 bits -- the integer conversion alone, in fp32."""
    cdf = np.asarray(cdf, np.float32)
    L = cdf.shape[-1] - 1
    x32 = cdf * np.float32(65536 - L)
    assert x32.dtype == np.float32
    return ((np.rint(x32).astype(np.int64) + np.arange(L + 1)) & 0xFFFF).astype(np.int32)


def tables32(logits):
    pmf = softmax32(logits)
    cdf, x32, ci = cdf32(pmf)
    return {"pmf": pmf, "cdf": cdf, "x32": x32, "cdf_int": ci}


def tables64(logits):
    lg = np.asarray(logits).astype(np.float64)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    s = np.zeros(lg.shape[:-1])
    for l in range(lg.shape[-1]):
        s = s + e[..., l]
    pmf = e / s[..., None]
    return from_pmf64(pmf)


def from_pmf64(pmf):
    """float64 pmf -> the float64 tables (also for a pmf that a float64 network produced)."""
    L = pmf.shape[-1]
    cdf = np.zeros(pmf.shape[:-1] + (L + 1,))
    run = np.zeros(pmf.shape[:-1])
    for l in range(L):
        run = run + pmf[..., l]
        cdf[..., l + 1] = np.minimum(run, 1.0)
    x64 = cdf * float(65536 - L)
    want = ((np.rint(x64).astype(np.int64) + np.arange(L + 1)) & 0xFFFF).astype(np.int32)
    return {"pmf": pmf, "cdf": cdf, "x64": x64, "cdf_int": want}


# --------------------------------------------------------------------------- logits classes for pccx_softmax_cdf
CLASS_LS = [1, 2, 7, 15, 64, 257]
CLASS_ROWS = 4096


def logit_classes(L, rows=CLASS_ROWS, seed=77):
    """name -> (rows, L) fp32 finite logits."""
    rng = np.random.default_rng(seed + L)
    z = rng.standard_normal((rows, L))
    out = {f"normal_x{s}": z * s for s in (0.1, 1, 10, 100)}
    out["all_equal"] = np.repeat(rng.uniform(-50, 50, size=(rows, 1)), L, axis=1)
    hot = np.zeros((rows, L))
    hot[np.arange(rows), rng.integers(0, L, size=rows)] = np.where(rng.random(rows) < 0.5, 100.0, -100.0)
    out["one_hot_pm100"] = hot
    # equal +- k * 2^-20, |k| <= 1024 (the logits of a row agree to 1e-3).  With a handful of k the cumsum of a long row is the all-equal
    # row's plus a perturbation far below one count, and at L = 257 its x64 = 254.004 l sits within 0.04 of a rounding boundary for
    # every l in 118..138 of EVERY row: the share of entries near a boundary is then a property of the class, not of the arithmetic.
    # 1024 spreads x64 by about a count in mid-row (65279 / 257 * sqrt(128) * 1024 * 2^-20 / sqrt(3)), so the boundaries are met as
    # often as anywhere else.
    out["near_ties"] = 0.5 + rng.integers(-1024, 1025, size=(rows, L)) * 2.0 ** -20
    # slopes of either sign from 1/64 to 4 per level, every row its own (a handful of slopes would make the class a handful of
    # distinct rows, and a share over them no statistic), from a start in -8..8
    slope = rng.choice([-1.0, 1.0], size=(rows, 1)) * 2.0 ** rng.uniform(-6, 2, size=(rows, 1))
    out["ramps"] = rng.uniform(-8, 8, size=(rows, 1)) + slope * np.arange(L)[None, :]
    # fp32 resolves 1/16 at 1e6, so a row of unit spread would be drawn from ~100 values, and equal logits share one exp error, which
    # then adds up coherently along the cumsum (tables32 itself: 0.95 % at L = 257, against 0.44 % here).  Ten times the spread keeps
    # the class about the offset -- the subtraction lg - mx at a large magnitude -- and not about repeated values.
    out["offset_1e6"] = 10.0 * z + 1e6
    return {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in out.items()}


def narrow_logit_classes(L, rows=CLASS_ROWS, seed=78):
    """The three classes above in their narrow form, whose share of entries near a rounding boundary belongs to the class and not
    to the arithmetic (see there): held to the exact invariants and to one count of float64, not to the share caps.  Truly near-tied
    rows (|k| <= 4), rows of repeated values at 1e6 (unit spread on a grid of 1/16), ramps of eighteen slopes in powers of two."""
    rng = np.random.default_rng(seed + L)
    out = {"near_ties_k4": 0.5 + rng.integers(-4, 5, size=(rows, L)) * 2.0 ** -20,
           "offset_1e6_unit": rng.standard_normal((rows, L)) + 1e6,
           "ramps_pow2": rng.choice([-1.0, 1.0], size=(rows, 1)) * 2.0 ** rng.integers(-6, 3, size=(rows, 1)) * np.arange(L)[None, :]}
    return {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in out.items()}


# --------------------------------------------------------------------------- assertions shared by the CPU and the GPU tests
def check_exact_invariants(cdf_int, L, cdf=None, who=""):
    """What holds for every table without any tolerance.  cdf_int (..., L+1) int32, cdf (..., L+1) fp32 or None."""
    ci = np.asarray(cdf_int).astype(np.int64)
    assert ci.shape[-1] == L + 1
    assert ((ci >= 0) & (ci < 65536)).all(), who + ": an entry outside 16 bits"
    assert (ci[..., 0] == 0).all(), who + ": cdf_int[..., 0]"
    assert (ci[..., L] == 0).all(), who + ": cdf_int[..., L] is not the wrapped 65536"
    # the steps (cdf_int[l+1] - cdf_int[l]) mod 65536, the last entry standing for the 65536 it wraps from (with L = 1 the one step is
    # 65536 itself, which mod 65536 would read 0): every symbol's frequency >= 1, and they add up to 65536
    un = ci.copy()
    un[..., L] = 65536
    steps = np.diff(un, axis=-1)
    assert (steps >= 1).all(), who + f": a step below 1 (min {steps.min()})"
    assert (steps.sum(-1) == 65536).all(), who
    if cdf is not None:
        cdf = np.asarray(cdf)
        assert cdf.dtype == np.float32 and (cdf[..., 0] == 0).all(), who + ": cdf[..., 0]"
        assert (cdf <= 1.0).all() and (cdf >= 0).all(), who + ": cdf outside [0, 1]"
        assert (np.diff(cdf, axis=-1) >= 0).all(), who + ": cdf not monotone"
        # the integer conversion alone, recomputed from the same float cdf: no tolerance
        again = int_from_float_cdf(cdf)
        bad = int((again != np.asarray(cdf_int)).sum())
        assert bad == 0, who + f": {bad} entries of cdf_int are not rint(cdf * (65536 - L)) + l of the float cdf beside them"


def e_ref_counts(t32, t64):
    """tables32's own distance to float64 in counts, on the quantity that rint() sees."""
    return float(np.abs(t32["x32"].astype(np.float64) - t64["x64"]).max())


def check_against64(cdf_int, t64, e_ref, L, who="", cap=None):
    """cdf_int against rint(x64) + l: every differing entry is +-1 (mod 65536) and sits where x64 is within FACTOR * e_ref of a
    rounding boundary.  Returns (share of differing entries, their number, the number of entries left out of the share); with cap,
    asserts share <= cap.
    An entry whose x64 lies closer to a boundary than float64's own error on it, 65536 * (L + 3) * 2^-52 counts (L + 3 roundings of
    values below 1, scaled), is one the reference itself does not decide -- 65529 / 6 = 10921.5 exactly, so six equal levels at
    L = 7 put every interior entry there.  Such entries must still be within one count; they are left out of the share."""
    got, want = np.asarray(cdf_int).astype(np.int64), t64["cdf_int"].astype(np.int64)
    assert got.shape == want.shape, who
    delta = (got - want) & 0xFFFF
    differ = delta != 0
    assert np.isin(delta[differ], (1, 65535)).all(), who + f": an entry off by more than one count ({np.unique(delta[differ])[:8]})"
    x64 = t64["x64"]
    dist = np.abs((x64 - np.floor(x64)) - 0.5)
    assert (dist[differ] < FACTOR * e_ref).all(), \
        who + f": a differing entry {dist[differ].max():.4f} counts from a rounding boundary, e_ref = {e_ref:.4f}"
    decided = dist >= 65536.0 * (L + 3) * 2.0 ** -52
    left_out = int(decided.size - decided.sum())
    # the statistic must keep its population: one-hot -100 at L = 7 leaves out 22 % of a class's entries, nothing else above 7 %
    assert 2 * left_out <= decided.size, who + f": {left_out} of {decided.size} entries sit on a rounding boundary of float64"
    share = float((differ & decided).sum() / max(int(decided.sum()), 1))
    if cap is not None:
        assert share <= cap, who + f": {100 * share:.3f} % of the entries differ from float64 (cap {100 * cap} %)"
    return share, int(differ.sum()), left_out


def float_errors(t, t64):
    """(max |pmf - pmf64|, max |cdf - cdf64|) of fp32 tables t (dict with pmf, cdf) against float64."""
    return (float(np.abs(np.asarray(t["pmf"]).astype(np.float64) - t64["pmf"]).max()),
            float(np.abs(np.asarray(t["cdf"]).astype(np.float64) - t64["cdf"]).max()))
