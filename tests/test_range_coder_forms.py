"""GPU: both kernels of each direction of the range coder (csrc/rangecoder.hip) against the oracle's literal bit-at-a-time coder
(oracle.cport.range_encode / range_decode), byte for byte and symbol for symbol -- integers, so there is no tolerance.

Form 0 is one wave per cloud staged in LDS, form 1 one lane per cloud from global memory; the launchers choose by an LDS budget
that pccx_range_coder_form states.  Every launch here goes through tests/coder_cases.py, which asserts through that query which
kernel the launch runs, so that a later change of the budget fails these tests and does not quietly turn them into tests of the
other kernel.  Small shapes reach form 1 by padding the caller's `cap` (encode) or the byte tensor's `stride` (decode) to 60 KiB,
not by a large nsym: the one-lane kernels are serial per cloud.

Decode inputs carry 0xFF after every stream's last byte: bytes past nbytes must read as zero, as the oracle reads them."""
import numpy as np
import pytest
import torch

from oracle import cport, ref_model
from pccx import models
from tests import coder_cases as cc
from tests import synth

pytestmark = pytest.mark.gpu
PAD = cc.FORM1_PAD


def _oracle_streams(cdf, sym):
    return [cport.range_encode(cdf[b], sym[b].astype(np.int16)) for b in range(cdf.shape[0])]


def _check_encode(cdf, sym, L, cap, want_form, want, q=None):
    """One encode launch: nbytes, the stream bytes, and the sentinel everywhere else (row tails and the spare row)."""
    B = cdf.shape[0]
    out, nb = cc.encode(cdf, (sym - L // 2) if q is None else q, L, cap, want_form)
    for b in range(B):
        assert nb[b] == len(want[b]), f"form {want_form} cloud {b}: nbytes {nb[b]} vs oracle {len(want[b])}"
        assert bytes(out[b, :nb[b]]) == want[b], f"form {want_form} cloud {b}: bytes differ from the oracle"
        assert (out[b, nb[b]:] == cc.SENTINEL).all(), f"form {want_form} cloud {b}: wrote at or after nbytes"
    assert (out[B] == cc.SENTINEL).all(), f"form {want_form}: wrote past the last row"
    return out, nb


def _check_decode(cdf, streams, L, want_sym, nbytes=None, only_form=None):
    """Decode in every form the launcher can reach for this shape; returns the forms that ran."""
    nsym = cdf.shape[1]
    ran = []
    for stride, f in cc.decode_forms(nsym, L, max(len(s) for s in streams)):
        if only_form is not None and f != only_form:
            continue
        by, nb = cc.rows(streams, stride, 0xFF)
        got = cc.decode(cdf, by, nb if nbytes is None else nbytes, L, f)
        assert np.array_equal(got, want_sym), f"decode form {f} stride {stride}: symbols differ from the oracle"
        ran.append(f)
    return ran


@pytest.mark.parametrize("L", [2, 7, 15, 63])
@pytest.mark.parametrize("nsym", [1, 77, 1024])
def test_same_input_both_forms_equal_each_other_and_the_oracle(nsym, L):
    """Each input is encoded with the default cap (form 0) and with cap = 60 KiB (form 1): equal nbytes, equal bytes, equal to the
    oracle, and nothing written at or after nbytes.  Then the oracle's streams are decoded in both forms (tight stride / stride
    padded to 60 KiB); at (1024, 63) the tables alone are 128 KiB, no stride reaches the wave decoder, and form 1 is the only one."""
    B = 10
    cdf, sym = cc.batch(nsym, L, B, 1000 * L + nsym)
    want = _oracle_streams(cdf, sym)
    cap0 = models.range_cap(nsym)
    assert max(len(w) for w in want) <= cap0                       # input condition: the default cap holds every stream
    o0, n0 = _check_encode(cdf, sym, L, cap0, 0, want)
    o1, n1 = _check_encode(cdf, sym, L, PAD, 1, want)
    assert np.array_equal(n0, n1)
    for b in range(B):
        assert np.array_equal(o0[b, :n0[b]], o1[b, :n1[b]])
        assert np.array_equal(cport.range_decode(cdf[b], want[b]), sym[b])
    ran = _check_decode(cdf, want, L, sym)
    assert ran == ([1] if (nsym, L) == (1024, 63) else [0, 1])


def test_the_lds_threshold_itself():
    """nsym*8 + round4(cap) (encode) and round4(nsym*(L+1)*2) + round4(stride) + nsym (decode) equal to 60 KiB, 4 below and 4
    above: the first two run the wave kernel with its largest LDS image, the third the one-lane kernel."""
    nsym, L, B = 1024, 7, 5
    cdf, sym = cc.batch(nsym, L, B, 77)
    want = _oracle_streams(cdf, sym)
    for delta, f in ((0, 0), (-4, 0), (4, 1)):
        cap = 61440 - nsym * 8 + delta
        assert nsym * 8 + cc.round4(cap) == 61440 + delta
        _check_encode(cdf, sym, L, cap, f, want)
        stride = 61440 - nsym * (L + 1) * 2 - nsym + delta
        assert cc.round4(nsym * (L + 1) * 2) + cc.round4(stride) + nsym == 61440 + delta
        by, nb = cc.rows(want, stride, 0xFF)
        assert np.array_equal(cc.decode(cdf, by, nb, L, f), sym)
    # a cap / stride that is no multiple of 4 rounds up before it is compared
    assert cc.form(0, nsym, L, 61440 - nsym * 8 - 3) == 0 and cc.form(0, nsym, L, 61440 - nsym * 8 + 1) == 1
    assert cc.form(1, nsym, L, 44032 - 3) == 0 and cc.form(1, nsym, L, 44032 + 1) == 1


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_one_lane_kernels_across_workgroups(B):
    """Grid (B+63)/64 of the one-lane kernels: one lane, a workgroup short of one lane, a full one, a ragged second, three."""
    nsym, L = 77, 7
    cdf, sym = cc.batch(nsym, L, B, 500 + B)
    want = _oracle_streams(cdf, sym)
    _check_encode(cdf, sym, L, PAD, 1, want)
    assert _check_decode(cdf, want, L, sym, only_form=1) == [1]


@pytest.mark.parametrize("want_form,nsym", [(0, 1024), (1, 7680)])
def test_capacity_exceeded_is_marked_and_confined(want_form, nsym):
    """cap about half of what the stream needs: nbytes = -(bytes needed), the cap bytes written are the oracle's prefix, and the row
    placed after the cloud's row is untouched (one cloud per launch, so that row is not another cloud's).  With a cap that small
    the one-lane encoder is reached only through nsym: nsym*8 alone must exceed 60 KiB.  The mirror: the marked count decodes as an
    empty stream, and the prefix decodes as the oracle decodes it, a truncated stream."""
    L = 7
    rng = np.random.default_rng(31 + nsym)
    for kind in ("uniform", "random", "one_count"):
        c, s = cc.tables(kind, nsym, L, rng)
        cdf, sym = c[None], s[None]
        want = _oracle_streams(cdf, sym)[0]
        cap = cc.round4(len(want) // 2) + 1                         # odd on purpose: the wave form rounds its word count up
        assert 8 <= cap < len(want)
        out, nb = cc.encode(cdf, sym - L // 2, L, cap, want_form)
        assert nb[0] == -len(want)
        assert bytes(out[0]) == want[:cap]
        assert (out[1] == cc.SENTINEL).all(), "overflow ran into the next row"
        for f_stride, f in cc.decode_forms(nsym, L, cap):
            by, _ = cc.rows([want[:cap]], f_stride, 0xFF)
            assert np.array_equal(cc.decode(cdf, by, nb, L, f)[0], cport.range_decode(c, b""))
            assert np.array_equal(cc.decode(cdf, by, np.array([cap]), L, f)[0], cport.range_decode(c, want[:cap]))


@pytest.mark.parametrize("L", [2, 7, 63])
def test_symbol_clamp_in_both_forms(L):
    """latent_q outside [-(L//2), L - 1 - L//2] codes as the nearest symbol of the alphabet."""
    nsym, B = 77, 5
    cdf, sym = cc.batch(nsym, L, B, 900 + L)
    q = (sym - L // 2).astype(np.float32)
    far = np.array([L // 2 + 5, -(L // 2 + 5), 1000, -1000], dtype=np.float32)
    q[:, ::3] = far[np.arange(q[:, ::3].shape[1]) % 4]
    clamped = np.clip(q.astype(np.int64) + L // 2, 0, L - 1)
    assert (clamped != q.astype(np.int64) + L // 2).any()
    want = _oracle_streams(cdf, clamped)
    _check_encode(cdf, clamped, L, models.range_cap(nsym), 0, want, q=q)
    _check_encode(cdf, clamped, L, PAD, 1, want, q=q)


@pytest.mark.parametrize("L", [1, 64, 200])
def test_alphabets_only_the_one_lane_decoder_takes(L):
    """L = 1 (an empty search mask) and L + 1 > 64 (a symbol's table does not fit the 64 lanes) decode in form 1 at any stride;
    the encoder has no such condition, so its two forms are both run."""
    nsym, B = 77, 5
    cdf, sym = cc.batch(nsym, L, B, 40 + L)
    want = _oracle_streams(cdf, sym)
    _check_encode(cdf, sym, L, 4 * nsym + 16, 0, want)
    _check_encode(cdf, sym, L, PAD, 1, want)
    assert cc.form(1, nsym, L, 8) == 1
    assert _check_decode(cdf, want, L, sym) == [1]


def test_nbytes_beyond_the_row_and_negative():
    """nbytes > stride decodes the stride bytes of the row and no byte of the next row (rows are tight: the next row starts right
    there, and a stream shorter than the row is followed by 0xFF, which then belongs to what is decoded); nbytes <= 0 decodes
    the empty stream.  Expected: the oracle on the row cut at nbytes clamped to [0, stride]."""
    L = 7
    # form 0, form 1 by a padded stride, and form 1 with a tight row, which only a large nsym gives the one-lane decoder
    for nsym, B, stride, row, f in ((77, 6, 16, 16, 0), (77, 6, 16, PAD, 1), (4096, 6, 200, 200, 1)):
        cdf, sym = cc.batch(nsym, L, B, 61 + nsym)
        cut = [s[:stride] for s in _oracle_streams(cdf, sym)]
        assert any(len(s) == stride for s in cut)
        by, _ = cc.rows(cut, row, 0xFF)
        nbytes = np.array([row + 1, 1 << 30, -1, -(1 << 30), 0, row], dtype=np.int32)
        want = np.stack([cport.range_decode(cdf[b], bytes(by[b, :min(max(int(nbytes[b]), 0), row)])) for b in range(B)])
        assert np.array_equal(cc.decode(cdf, by, nbytes, L, f), want), f"nsym {nsym} row {row} form {f}"


def test_production_shape_of_the_whole_cloud_codec():
    """B = 2, nsym = 16384 (S = 1024 patches, d = 16), L = 7, tables from the seeded probability model: form 1 in both directions,
    bytes equal to the oracle's, lossless round trip."""
    K, k, d, L = synth.MODEL_CFG
    assert (d, L) == (16, 7)
    prob = models.ConditionalProbabilityModel(L, d)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    prob = prob.pack("cuda")
    rng = np.random.default_rng(16384)
    B, S = 2, 1024
    nsym = S * d
    centres = ((rng.integers(0, 128, size=(B, S, 3)) + 0.5) / 128).astype(np.float32)
    r = prob.run(torch.from_numpy(centres).cuda(), ("pmf", "cdf_int"))
    pmf = r["pmf"].cpu().numpy().reshape(B, nsym, L).astype(np.float64)
    cdf = np.ascontiguousarray(r["cdf_int"].cpu().numpy().reshape(B, nsym, L + 1))
    cc.assert_widths(cdf)
    u = rng.random((B, nsym, 1)) * pmf.sum(-1, keepdims=True)
    sym = np.minimum((np.cumsum(pmf, -1) <= u).sum(-1), L - 1)
    want = _oracle_streams(cdf, sym)
    cap = models.range_cap(nsym)
    _check_encode(cdf, sym, L, cap, 1, want)
    by, nb = cc.rows(want, cap, 0xFF)
    assert np.array_equal(cc.decode(cdf, by, nb, L, 1), sym)
    # and through the calls the codec makes
    q = torch.from_numpy((sym - L // 2).astype(np.float32)).cuda()
    dby, dnb = models.range_encode(r["cdf_int"], q, L)
    assert np.array_equal(models.range_decode(r["cdf_int"], dby, dnb, L).cpu().numpy(), q.cpu().numpy())
