"""CPU: the cases and references of tests/prob_cases.py, proved on the oracle alone before tests/test_prob_float64.py holds the HIP
kernels to them -- the exact-logit weights are exact, tables32 is the reference's table stage, and every cap the GPU test asserts
holds for tables32 itself on the same cases (a cap the plain fp32 statement missed would be no statement about the kernels)."""
import numpy as np
import pytest
import torch

from oracle import ref_model
from tests import prob_cases as pc

CPU_S = {(16, 7): 64, (5, 7): 48, (3, 4): 48, (1, 15): 32, (9, 14): 48, (16, 8): 80, (8, 15): 48, (16, 1): 16}


def _oracle(d, L, sd, double=False):
    m = ref_model.ConditionalProbabilityModel(L, d).eval()
    m.load_state_dict(sd)
    return m.double() if double else m


def _oracle_logits(m, x):
    """The logits in front of ref_model's softmax (AE.py:107-119), fp32."""
    B, S, _ = x.shape
    with torch.no_grad():
        feature = m.model_pn(x.transpose(1, 2))
        mlp_input = torch.cat((x, feature.repeat((1, S)).view(B, S, -1)), dim=2)
        out = m.model_mlp(mlp_input.unsqueeze(-1).transpose(1, 2))
        return out.transpose(1, 2).reshape(B, S, m.d, m.L)


@pytest.mark.parametrize("amp", pc.AMPS)
@pytest.mark.parametrize("d,L", pc.DL_CASES)
def test_exact_logit_weights_are_exact_and_tables32_is_the_oracles_table_stage(d, L, amp):
    torch.set_num_threads(8)
    S = CPU_S[d, L]
    sd = pc.exact_case(d, L, amp)
    x = pc.grid_centres(2, S, 400 + S)
    want = pc.intended_logits(sd, x, d, L)
    assert (want == want.astype(np.float32)).all()                   # representable: float64 and fp32 hold the same numbers
    m = _oracle(d, L, sd)
    got = _oracle_logits(m, torch.from_numpy(x)).numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    if L > 1:
        assert len(np.unique(got)) > 8 and np.abs(got).max() > amp / 2      # not a degenerate case

    # tables32 against pn_kit's / torchac's statements on the oracle's own pmf: the cumsum, the clamp and the integer
    # conversion are the oracle's bit for bit; the softmax differs only where torch's exp and numpy's do
    with torch.no_grad():
        opmf = m(torch.from_numpy(x))
    ocdf = ref_model.pmf_to_cdf(opmf)
    oint = ref_model.cdf_float_to_int(ocdf)
    assert np.array_equal(pc.int_from_float_cdf(ocdf.numpy()), oint)             # the integer conversion: the same statement
    # torch's CPU cumsum keeps its running sum in double and rounds every output once, where the device (and torch on a GPU) adds in
    # fp32: the oracle's cdf is that, exactly, and the sequential fp32 cumsum sits within its L half-ulps of it
    wide = np.minimum(np.cumsum(opmf.numpy().astype(np.float64), -1), 1.0).astype(np.float32)
    assert np.array_equal(wide, ocdf.numpy()[..., 1:])
    cdf, _, ci = pc.cdf32(opmf.numpy())
    assert np.abs(cdf.astype(np.float64) - ocdf.numpy()).max() <= (L + 1) * 2.0 ** -25
    t32 = pc.tables32(got)
    assert np.abs(t32["pmf"] - opmf.numpy()).max() <= 2.0 ** -22                 # torch's exp against numpy's: a few ulp below 1
    assert np.abs(t32["cdf"].astype(np.float64) - ocdf.numpy()).max() <= (L + 1) * 2.0 ** -25 + L * 2.0 ** -22
    for mine in (ci, t32["cdf_int"]):
        d_int = (mine.astype(np.int64) - oint + 32768) % 65536 - 32768
        assert np.abs(d_int).max() <= 1 and (d_int != 0).mean() <= 0.005


def _caps_hold(t32, t64, L, who):
    e_ref = pc.e_ref_counts(t32, t64)
    pc.check_exact_invariants(t32["cdf_int"], L, t32["cdf"], who)
    share, _, _ = pc.check_against64(t32["cdf_int"], t64, e_ref, L, who, cap=pc.SHARE_CAP[L >= 64])
    return e_ref, share


@pytest.mark.parametrize("amp", pc.AMPS)
@pytest.mark.parametrize("d,L", pc.DL_CASES)
def test_caps_hold_for_tables32_on_the_exact_logit_cases(d, L, amp):
    """The pooled centres of every S the GPU test runs, as it pools them."""
    sd = pc.exact_case(d, L, amp)
    x = np.concatenate([pc.fused_centres(S) for S in pc.S_FUSED], axis=1)
    lg = pc.intended_logits(sd, x, d, L).astype(np.float32)
    t32, t64 = pc.tables32(lg), pc.tables64(lg)
    e_ref, share = _caps_hold(t32, t64, L, f"d={d} L={L} amp={amp}")
    print(f"d={d} L={L} amp={amp}: e_ref {e_ref:.4f} counts, tables32 differs on {100 * share:.3f} %")
    if amp == 8 and L >= 7:
        un = t32["cdf_int"].astype(np.int64)
        un[..., L] = 65536
        assert (np.diff(un, axis=-1) == 1).mean() > 0.2                          # the flat stretches are there: frequency 1
    if amp == 64 and L >= 7:
        assert (t32["pmf"] == 0).mean() > 0.15                                   # and the underflown entries


@pytest.mark.parametrize("d,L,S", pc.GENERIC_CASES)
def test_caps_hold_for_tables32_on_the_generic_cases(d, L, S):
    for amp in pc.AMPS:
        sd = pc.exact_case(d, L, amp)
        lg = pc.intended_logits(sd, pc.grid_centres(2, S, 400 + S), d, L).astype(np.float32)
        _caps_hold(pc.tables32(lg), pc.tables64(lg), L, f"generic d={d} L={L} S={S} amp={amp}")


@pytest.mark.parametrize("L", pc.CLASS_LS)
def test_caps_hold_for_tables32_on_the_logit_classes(L):
    for name, lg in pc.logit_classes(L).items():
        assert np.isfinite(lg).all() and lg.shape == (pc.CLASS_ROWS, L)
        t32, t64 = pc.tables32(lg), pc.tables64(lg)
        e_ref, share = _caps_hold(t32, t64, L, f"{name} L={L}")
        print(f"{name} L={L}: e_ref {e_ref:.4f} counts, tables32 differs on {100 * share:.3f} %")


@pytest.mark.parametrize("L", pc.CLASS_LS)
def test_exact_invariants_hold_for_tables32_on_the_narrow_classes(L):
    """The narrow forms of three classes: every exact invariant and the per-entry conditions, no share."""
    for name, lg in pc.narrow_logit_classes(L).items():
        assert np.isfinite(lg).all() and lg.shape == (pc.CLASS_ROWS, L)
        t32, t64 = pc.tables32(lg), pc.tables64(lg)
        pc.check_exact_invariants(t32["cdf_int"], L, t32["cdf"], f"{name} L={L}")
        share, _, left_out = pc.check_against64(t32["cdf_int"], t64, pc.e_ref_counts(t32, t64), L, f"{name} L={L}")
        print(f"{name} L={L}: tables32 differs on {100 * share:.3f} %, {left_out} entries on a boundary")
    if L > 1:
        assert len(np.unique(pc.narrow_logit_classes(L)["ramps_pow2"], axis=0)) <= 18


def test_store_widths_of_the_distinct_kernel_are_all_reached():
    assert {pc.store_widths(d, L) for d, L in pc.DL_CASES} == {(4, 4), (1, 4), (4, 1), (1, 1)}
    assert pc.store_widths(5, 7) == (1, 4) and pc.store_widths(3, 4) == (4, 1)


def test_the_checks_see_the_mutations_they_are_for():
    """Truncation, a wrong arange and a dropped clamp, applied to tables32's own statements: each trips an exact assertion."""
    lg = pc.logit_classes(7)["normal_x10"]
    t32 = pc.tables32(lg)
    x32, ar = t32["x32"], np.arange(8)
    trunc = ((np.floor(x32).astype(np.int64) + ar) & 0xFFFF).astype(np.int32)
    assert (pc.int_from_float_cdf(t32["cdf"]) != trunc).mean() > 0.25            # half the interior entries, none of the first
    with pytest.raises(AssertionError):
        pc.check_exact_invariants(trunc, 7, t32["cdf"])
    shifted = ((np.rint(x32).astype(np.int64) + np.maximum(ar - 1, 0)) & 0xFFFF).astype(np.int32)
    with pytest.raises(AssertionError):
        pc.check_exact_invariants(shifted, 7, t32["cdf"])
    run, unclamped = np.zeros(lg.shape[0], np.float32), np.zeros_like(t32["cdf"])
    for l in range(7):
        run = run + t32["pmf"][:, l]
        unclamped[:, l + 1] = run
    assert (unclamped > 1).any()                                                 # the fp32 cumsum does pass 1 on these rows
    with pytest.raises(AssertionError, match="outside"):
        pc.check_exact_invariants(pc.int_from_float_cdf(unclamped), 7, unclamped)
