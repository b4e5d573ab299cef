"""GPU: the probability model's tables against float64 (csrc/prob.hip in its four fused forms, the generic path, softmax_cdf_kernel of
csrc/linear.hip).  DESIGN.md section 4.5b holds the figures this file prints.

Part A -- the table stage alone.  tests/prob_cases.py builds weights whose logits are exact in fp32 (tests/test_prob_cases_cpu.py
proves it on the oracle), so everything between the logits and the 16-bit CDF is compared with tables64 on the same numbers, at
amplitudes that reach the clamp, the frequency-1 stretches and pmf == 0.  Exact assertions carry the weight: first and last entry,
steps >= 1 summing to 65536, cdf <= 1, cdf_int == rint(cdf * (65536 - L)) + l recomputed from the device's own float cdf, and every
fused form bit for bit run()'s.  Against float64 every margin comes from tables32's own distance to it (e_ref) -- prob_cases.

Part B -- the network in front of the tables, seeded weights, against oracle/ref_model in double on the same fp32 weights and
inputs; the yardstick is the fp32 oracle's own distance to that, per case.

The share of entries that differ from float64 is a statistic: it is taken per model over the pooled centres of all S (a model with
d = 1 at S = 16 alone has 256 entries, one of which is already 0.4 %; with exact logits a row's table does not depend on S, and
every form at every S is bit for bit run()'s); in part B per shape, in whole entries below 1000 of them, and per gain over all
shapes.  Every other assertion is per entry.
"""
import numpy as np
import pytest
import torch

from oracle import ref_model
from pccx import _lib, models, ops
from tests import prob_cases as pc
from tests import synth

pytestmark = pytest.mark.gpu

WANTS = ("pmf", "cdf", "cdf_int")
FILL = {"pmf": float("nan"), "cdf": float("nan"), "cdf_int": -1}


def _model(d, L, sd):
    m = models.ConditionalProbabilityModel(L, d)
    m.load_state_dict(sd)
    return m.pack("cuda")


def _bits(t):
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def _same(got, want, who):
    for name in got:
        assert got[name].shape == want[name].shape and torch.equal(_bits(got[name]), _bits(want[name])), f"{who}: {name}"


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _singles(fn, full, who):
    """Each output requested alone is the one of the three requested together."""
    for name in WANTS:
        _same(fn((name,)), {name: full[name]}, f"{who}, {name} alone")


def _distinct_prefilled(p, x):
    """pccx_prob_forward_distinct into sentinel-filled outputs: a row nobody wrote is seen (NaN is not equal to itself)."""
    B, S, _ = x.shape
    out = {"pmf": torch.full((B, S, p.d, p.L), FILL["pmf"], device="cuda"),
           "cdf": torch.full((B, S, p.d, p.L + 1), FILL["cdf"], device="cuda"),
           "cdf_int": torch.full((B, S, p.d, p.L + 1), FILL["cdf_int"], device="cuda", dtype=torch.int32)}
    _lib.call("pccx_prob_forward_distinct", x.data_ptr(), B, S, p.d, p.L, p._blob.data_ptr(), *(out[n].data_ptr() for n in WANTS),
              ops._stream())
    return out


def _segments(p, x, G):
    """run_segments with every segment listed, cloud by cloud -> (B, S, d, L+1)."""
    B, S, _ = x.shape
    n_seg = -(-S // G)
    seg = torch.arange(n_seg, device="cuda", dtype=torch.int32)
    return torch.stack([p.run_segments(x[b], seg, n_seg, G)[:S] for b in range(B)])


def _softmax_cdf(lg, rows, L, want=WANTS):
    """pccx_softmax_cdf on the first `rows` rows of lg (N, L) into sentinel-filled outputs of all N rows."""
    N = lg.shape[0]
    out = {"pmf": torch.full((N, L), FILL["pmf"], device="cuda"), "cdf": torch.full((N, L + 1), FILL["cdf"], device="cuda"),
           "cdf_int": torch.full((N, L + 1), FILL["cdf_int"], device="cuda", dtype=torch.int32)}
    _lib.call("pccx_softmax_cdf", lg.data_ptr(), rows, L, *(out[n].data_ptr() if n in want else None for n in WANTS), ops._stream())
    return out


def _report(who, got, lg32, L, cap):
    """The float64 comparison of one case: got = numpy pmf / cdf / cdf_int over rows (..., L), lg32 the exact fp32 logits.  cap None:
    the per-entry conditions and the float bounds alone, for rows that are no sample (repeated centres, the narrow classes)."""
    t32, t64 = pc.tables32(lg32), pc.tables64(lg32)
    e_ref = pc.e_ref_counts(t32, t64)
    ref_pmf, ref_cdf = pc.float_errors(t32, t64)
    gpu_pmf, gpu_cdf = pc.float_errors(got, t64)
    share32, _, _ = pc.check_against64(t32["cdf_int"], t64, e_ref, L, who + " (tables32)")
    share, n, left_out = pc.check_against64(got["cdf_int"], t64, e_ref, L, who)
    vs32 = float((got["cdf_int"] != t32["cdf_int"]).mean())
    print(f"{who}: e_ref {e_ref:.4f} counts; pmf err {gpu_pmf:.3g} (tables32 {ref_pmf:.3g}, ratio {gpu_pmf / max(ref_pmf, 1e-30):.2f}); "
          f"cdf err {gpu_cdf:.3g} (tables32 {ref_cdf:.3g}, ratio {gpu_cdf / max(ref_cdf, 1e-30):.2f}); differs from float64 on "
          f"{100 * share:.3f} % = {n} entries (tables32 {100 * share32:.3f} %), from tables32 on {100 * vs32:.3f} %; {left_out} of "
          f"{got['cdf_int'].size} entries on a rounding boundary of float64, left out of the share")
    assert gpu_pmf <= pc.FACTOR * ref_pmf + 1e-9, who
    assert gpu_cdf <= pc.FACTOR * ref_cdf + 1e-9, who
    assert cap is None or share <= cap, f"{who}: {100 * share:.3f} % of the entries differ from float64 (cap {cap})"


# ------------------------------------------------------------------------------------------ part A
@pytest.mark.parametrize("amp", pc.AMPS)
@pytest.mark.parametrize("d,L", pc.DL_CASES)
def test_table_stage_of_every_fused_form_on_exact_logits(d, L, amp):
    sd = pc.exact_case(d, L, amp)
    p = _model(d, L, sd)
    assert p.fused_ok(16)
    pooled = {n: [] for n in WANTS}
    logits = []
    for S in pc.S_FUSED:
        who = f"d={d} L={L} amp={amp} S={S}"
        xn = pc.fused_centres(S)
        x = torch.from_numpy(xn).cuda()
        full = p.run(x, WANTS)
        _singles(lambda w: p.run(x, w), full, who + " run")
        got = _np(full)
        pc.check_exact_invariants(got["cdf_int"], L, got["cdf"], who)
        # the tiled trio
        tiled = p.run(x, WANTS, tiles=True)
        _same(tiled, full, who + " tiles")
        _singles(lambda w: p.run(x, w, tiles=True), full, who + " tiles")
        # pccx_prob_feature + pccx_prob_rows: G = 4 (never ragged: S % 16 == 0), and at S = 48 G = 5, whose tenth segment has three
        # rows inside the cloud
        assert torch.equal(_segments(p, x, 4), full["cdf_int"]), who + " segments"
        if S == 48:
            assert torch.equal(_segments(p, x, 5), full["cdf_int"]), who + " segments, G = 5"
        # the distinct kernel: the clouds as they are (every row its own slot), then clouds of at most eight distinct rows, one of a
        # single row; B = 1 and B = 5 leave three of a workgroup's four waves without a cloud
        if S <= 64:
            _same(_distinct_prefilled(p, x), full, who + " distinct")
            for counts in ([6], [1, 8, 3, 5, 8]):
                xr = torch.from_numpy(pc.repeated_centres(S, counts, 500 + S + len(counts))).cuda()
                want = p.run(xr, WANTS)
                _same(_distinct_prefilled(p, xr), want, who + f" distinct {counts}")
                _singles(lambda w: p.run(xr, w, distinct=True), want, who + f" distinct {counts}")
                w = _np(want)
                pc.check_exact_invariants(w["cdf_int"], L, w["cdf"], who + f" repeated {counts}")
                # a handful of distinct rows, each many times: no sample for a share, every entry still held to float64
                _report(who + f" repeated {counts}", w, pc.intended_logits(sd, xr.cpu().numpy(), d, L).astype(np.float32), L, None)
        for n in WANTS:
            pooled[n].append(got[n].reshape(-1, d, got[n].shape[-1]))
        logits.append(pc.intended_logits(sd, xn, d, L).astype(np.float32).reshape(-1, d, L))
    got = {n: np.concatenate(pooled[n]) for n in WANTS}
    _report(f"exact d={d} L={L} amp={amp} store<{pc.store_widths(d, L)}>", got, np.concatenate(logits), L, pc.SHARE_CAP[L >= 64])


@pytest.mark.parametrize("d,L,S", pc.GENERIC_CASES)
def test_generic_path_on_exact_logits(d, L, S):
    for amp in pc.AMPS:
        who = f"generic d={d} L={L} S={S} amp={amp}"
        sd = pc.exact_case(d, L, amp)
        p = _model(d, L, sd)
        assert not p.fused_ok(S)
        xn = pc.grid_centres(2, S, 400 + S)
        x = torch.from_numpy(xn).cuda()
        full = p.run(x, WANTS)
        _singles(lambda w: p.run(x, w), full, who)
        _same(p.run(x, WANTS, tiles=True, distinct=True), full, who + " with the switches of the fused forms")
        lg32 = pc.intended_logits(sd, xn, d, L).astype(np.float32)
        direct = _softmax_cdf(torch.from_numpy(lg32.reshape(-1, L)).cuda(), 2 * S * d, L)
        _same({n: direct[n].view(full[n].shape) for n in WANTS}, full, who + ": the layers' logits are not the exact ones")
        got = _np(full)
        pc.check_exact_invariants(got["cdf_int"], L, got["cdf"], who)
        _report(who, got, lg32, L, pc.SHARE_CAP[L >= 64])


@pytest.mark.parametrize("L", pc.CLASS_LS)
def test_softmax_cdf_kernel_on_logit_classes(L):
    N = pc.CLASS_ROWS
    for name, lg32 in pc.logit_classes(L).items():
        who = f"softmax_cdf {name} L={L}"
        lg = torch.from_numpy(lg32).cuda()
        full = _softmax_cdf(lg, N, L)
        for n in WANTS:                                               # each output alone: the same bits, the other two untouched
            one = _softmax_cdf(lg, N, L, (n,))
            for m in WANTS:
                if m == n:
                    assert torch.equal(_bits(one[m]), _bits(full[m])), f"{who}: {n} alone"
                else:
                    assert bool(torch.isnan(one[m]).all() if one[m].is_floating_point() else (one[m] == FILL[m]).all()), who
        for rows in (1, 255, 257):                                    # around the 256-thread block: rows written, the rest not
            part = _softmax_cdf(lg, rows, L)
            for n in WANTS:
                assert torch.equal(_bits(part[n][:rows]), _bits(full[n][:rows])), f"{who}: rows={rows} {n}"
                rest = part[n][rows:]
                assert bool(torch.isnan(rest).all() if rest.is_floating_point() else (rest == FILL[n]).all()), f"{who}: rows={rows} {n}"
        got = _np(full)
        pc.check_exact_invariants(got["cdf_int"], L, got["cdf"], who)
        _report(who, got, lg32, L, pc.SHARE_CAP[L >= 64])
    # the narrow forms of three classes (truly near-tied rows, repeated values at 1e6, ramps of a few slopes): the share of their
    # entries near a rounding boundary belongs to the class, so the exact invariants and the per-entry conditions alone
    for name, lg32 in pc.narrow_logit_classes(L).items():
        got = _np(_softmax_cdf(torch.from_numpy(lg32).cuda(), N, L))
        pc.check_exact_invariants(got["cdf_int"], L, got["cdf"], f"softmax_cdf {name} L={L}")
        _report(f"softmax_cdf {name} L={L}", got, lg32, L, None)


# ------------------------------------------------------------------------------------------ part B
B_SHAPES = [(16, 7, 64, 3), (16, 7, 16, 1), (16, 7, 80, 2), (16, 7, 1088, 1), (8, 15, 48, 1), (5, 7, 48, 2), (3, 4, 32, 1), (1, 15, 16, 1),
            (9, 14, 48, 1), (16, 8, 48, 1)]


def _seeded(d, L, g):
    m = models.ConditionalProbabilityModel(L, d)
    sd = ref_model.seeded_state_dict(m, synth.PROB_SEED, gain=synth.PROB_GAIN, last_gain={"model_mlp.4": float(g)})
    m.load_state_dict(sd)
    o32, o64 = ref_model.ConditionalProbabilityModel(L, d).eval(), ref_model.ConditionalProbabilityModel(L, d).eval()
    o32.load_state_dict(sd)
    o64.load_state_dict(sd)
    return m.pack("cuda"), o32, o64.double(), sd


def _evaluate(d, L, S, B, g):
    """One shape at one gain: the float64 oracle, the fp32 oracle's own distance to it, run() and run_segments on the device."""
    torch.set_num_threads(8)
    c = {"who": f"seeded d={d} L={L} S={S} B={B} g={g}"}
    p, o32, o64, _ = _seeded(d, L, g)
    xn = pc.grid_centres(B, S, 600 + S + B)
    with torch.no_grad():
        pmf32 = o32(torch.from_numpy(xn))
        pmf64 = o64(torch.from_numpy(xn).double())
    t64 = c["t64"] = pc.from_pmf64(pmf64.numpy())
    cdf32 = ref_model.pmf_to_cdf(pmf32)
    c["ref_pmf"], c["ref_cdf"] = pc.float_errors({"pmf": pmf32.numpy(), "cdf": cdf32.numpy()}, t64)
    c["ref_differ"] = int((ref_model.cdf_float_to_int(cdf32) != t64["cdf_int"]).sum())
    # the oracle's distance to float64 on the quantity its round() sees: the fp32 product of cdf_float_to_int
    c["ref_counts"] = float(np.abs((cdf32.numpy() * np.float32(65536 - L)).astype(np.float64) - t64["x64"]).max())
    c["peak"] = float(pmf64.max(-1)[0].mean())
    x = torch.from_numpy(xn).cuda()
    full = p.run(x, WANTS)
    c["segments_equal"] = torch.equal(_segments(p, x, 4), full["cdf_int"]) and (S % 5 == 0 or torch.equal(_segments(p, x, 5), full["cdf_int"]))
    got = c["got"] = _np(full)
    c["gpu_pmf"], c["gpu_cdf"] = pc.float_errors(got, t64)
    c["delta"] = (got["cdf_int"].astype(np.int64) - t64["cdf_int"]) & 0xFFFF
    c["differ"], c["entries"] = int((c["delta"] != 0).sum()), c["delta"].size
    return c


@pytest.fixture(scope="module")
def seeded_case():
    """(d, L, S, B, g) -> its evaluation, computed once for the module and left unchanged."""
    cache = {}

    def get(*key):
        if key not in cache:
            cache[key] = _evaluate(*key)
        return cache[key]
    return get


@pytest.mark.parametrize("g", [1, 8])
@pytest.mark.parametrize("d,L,S,B", B_SHAPES)
def test_network_and_tables_against_the_float64_oracle(seeded_case, d, L, S, B, g):
    """Per shape: the exact invariants; run_segments == run() at G = 4 and, where 5 does not divide S, at G = 5 (a ragged last
    segment); every entry within one count of float64, a differing one within four times the fp32 oracle's own error of a rounding
    boundary of x64; the float outputs within four times the oracle's error; and the number of differing entries at most four times
    the oracle's plus 0.1 % of the entries.  That allowance is taken in whole entries and is at least one: (3, 4, 32, 1) has 480
    entries and (1, 15, 16, 1) 256, of which 0.1 % is half an entry and a quarter, so that one entry 0.05 counts from a boundary
    would decide the outcome whenever the oracle happens to have none (measured: one of 480 at g = 8 against none).  From 1000
    entries on the bound is the share's as stated, without rounding up."""
    c = seeded_case(d, L, S, B, g)
    who = c["who"]
    pc.check_exact_invariants(c["got"]["cdf_int"], L, c["got"]["cdf"], who)
    assert c["segments_equal"], who + ": run_segments over all rows"
    share, ref_share = c["differ"] / c["entries"], c["ref_differ"] / c["entries"]
    differ = c["delta"] != 0
    x64 = c["t64"]["x64"]
    dist = np.abs((x64 - np.floor(x64)) - 0.5)
    far = float(dist[differ].max()) if differ.any() else 0.0
    print(f"{who}: peak {c['peak']:.2f}; fp32 oracle {c['ref_counts']:.3f} counts from float64; pmf err {c['gpu_pmf']:.3g} (oracle "
          f"{c['ref_pmf']:.3g}, ratio {c['gpu_pmf'] / c['ref_pmf']:.2f}); cdf err {c['gpu_cdf']:.3g} (oracle {c['ref_cdf']:.3g}, ratio "
          f"{c['gpu_cdf'] / c['ref_cdf']:.2f}); cdf_int differs on {c['differ']} = {100 * share:.3f} % of {c['entries']} (oracle "
          f"{c['ref_differ']} = {100 * ref_share:.3f} %), at most {far:.4f} counts from a rounding boundary")
    assert np.isin(c["delta"], (0, 1, 65535)).all(), who + ": an entry more than one count from float64"
    assert (dist[differ] < 4 * c["ref_counts"]).all(), who + f": a differing entry {far:.4f} counts from a rounding boundary"
    assert c["gpu_pmf"] <= 4 * c["ref_pmf"] and c["gpu_cdf"] <= 4 * c["ref_cdf"], who
    if c["entries"] >= 1000:
        assert share <= 4 * ref_share + 0.001, who
    else:
        assert c["differ"] <= 4 * c["ref_differ"] + max(1, int(np.ceil(0.001 * c["entries"]))), who


@pytest.mark.parametrize("g", [1, 8])
def test_share_of_entries_differing_from_float64_per_gain(seeded_case, g):
    """The share condition over every shape's entries together, as the one oracle figure per gain is taken."""
    cases = [seeded_case(*shape, g) for shape in B_SHAPES]
    entries = sum(c["entries"] for c in cases)
    share, ref_share = sum(c["differ"] for c in cases) / entries, sum(c["ref_differ"] for c in cases) / entries
    print(f"seeded g={g}, all shapes: cdf_int differs on {100 * share:.3f} % of {entries} (oracle {100 * ref_share:.3f} %)")
    assert share <= 4 * ref_share + 0.001


@pytest.mark.parametrize("S", [16, 80, 1088, 4112])
def test_feature_stage_against_float64(S):
    """pccx_prob_feature: pass 1 + 1b, the 512 numbers b0 + W0[:, 3:] . max_S relu(model_pn(centres))."""
    torch.set_num_threads(8)
    p, o32, o64, sd = _seeded(16, 7, 1)
    xn = pc.grid_centres(1, S, 700 + S)
    W0, b0 = sd["model_mlp.0.weight"][:, 3:, 0, 0], sd["model_mlp.0.bias"]
    with torch.no_grad():
        u32 = torch.nn.functional.linear(o32.model_pn(torch.from_numpy(xn).transpose(1, 2)), W0, b0)[0].numpy()
        u64 = torch.nn.functional.linear(o64.model_pn(torch.from_numpy(xn).double().transpose(1, 2)), W0.double(), b0.double())[0].numpy()
    ref = float(np.abs(u32.astype(np.float64) - u64).max())
    x = torch.from_numpy(xn).cuda()
    ws = torch.full((int(_lib.load().pccx_prob_feature_workspace_floats(S)) + 512,), float("nan"), device="cuda")
    _lib.call("pccx_prob_feature", x.data_ptr(), S, p._blob.data_ptr(), ws[512:].data_ptr(), ws[:512].data_ptr(), ops._stream())
    u = ws[:512].cpu().numpy()
    err = float(np.abs(u.astype(np.float64) - u64).max())
    print(f"feature S={S}: max |u| {np.abs(u64).max():.3f}; err {err:.3g} (fp32 oracle {ref:.3g}, ratio {err / ref:.2f})")
    assert np.isfinite(u).all() and err <= 4 * ref
