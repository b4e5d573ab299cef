"""GPU: the split form of the range-coded latent stream (pccx_range_encode_split / pccx_range_decode_split, csrc/rangecoder.hip)
against the oracle's literal coder, byte for byte and symbol for symbol -- integers, so there is no tolerance.

    "PXS1" | nsym u32 | seg_sym u16 | reserved u16 = 0 | len[P] u16 | segments,  P = ceil(nsym / seg_sym)      (little-endian)

Segment p must be oracle.cport.range_encode of symbols [p*seg_sym, (p+1)*seg_sym) with their tables; the expected file is put
together here from that and the header.  Tables and symbols come from tests/coder_cases.py (the five table kinds, sentinel rows,
a spare row after the batch)."""
import functools
import struct

import numpy as np
import pytest
import torch

from oracle import cport
from pccx import _lib, models
from pccx.ops import _stream
from tests import coder_cases as cc

pytestmark = pytest.mark.gpu

#        name                       B  nsym  seg_sym  L
CASES = {"four_even_segments":     (3, 1024, 256, 7),
         "ragged_last_segment":    (2, 1000, 256, 7),
         "one_segment":            (2, 100, 256, 7),
         "one_symbol_per_segment": (1, 5, 1, 7),
         "empty_stream":           (1, 0, 16, 7),
         "L_2":                    (2, 300, 128, 2),
         "L_63":                   (2, 300, 128, 63),
         "headline_segment_shape": (1, 2048, 1024, 7)}


def want_file(cdf, sym, seg_sym):
    """One cloud's split stream from the oracle: cdf (nsym, L+1), sym (nsym,)."""
    nsym = sym.shape[0]
    segs = [cport.range_encode(np.ascontiguousarray(cdf[i:i + seg_sym]), sym[i:i + seg_sym].astype(np.int16)) for i in range(0, nsym, seg_sym)]
    assert len(segs) == models.split_segments(nsym, seg_sym) and all(len(s) <= models.range_cap(seg_sym) for s in segs)
    return b"PXS1" + struct.pack("<IHH", nsym, seg_sym, 0) + np.array([len(s) for s in segs], dtype="<u2").tobytes() + b"".join(segs)


@functools.lru_cache(maxsize=None)
def case(name):
    """(cdf (B,nsym,L+1), sym (B,nsym), the B expected files): computed once, shared and not modified."""
    B, nsym, seg_sym, L = CASES[name]
    if nsym:
        cdf, sym = cc.batch(nsym, L, B, 7000 + 13 * nsym + L)
    else:
        cdf, sym = np.zeros((B, 0, L + 1), dtype=np.int32), np.zeros((B, 0), dtype=np.int64)
    files = [want_file(cdf[b], sym[b], seg_sym) for b in range(B)]
    return cdf, sym, files


def encode(cdf, sym, L, seg_sym, cap):
    """-> (out (B+1,cap) with the spare row, nbytes (B,)): rows pre-filled with the sentinel."""
    B = cdf.shape[0]
    buf = torch.full((B + 1, cap), cc.SENTINEL, dtype=torch.uint8, device="cuda")
    q = torch.from_numpy((sym - L // 2).astype(np.float32)).cuda()
    _, nb = models.range_encode_split(torch.from_numpy(np.ascontiguousarray(cdf)).cuda(), q, L, seg_sym, out=buf[:B])
    return buf.cpu().numpy(), nb.cpu().numpy()


def decode(cdf, by, nbytes, L, seg_sym):
    """The raw call on rows `by` (B,stride), outputs pre-filled with a sentinel and followed by a spare row that must come back
    untouched.  -> (symbols (B,nsym) int64, status (B,))."""
    B, nsym = cdf.shape[0], cdf.shape[1]
    ci = torch.from_numpy(np.ascontiguousarray(cdf)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(by)).cuda()
    nt = torch.from_numpy(np.asarray(nbytes, dtype=np.int32)).cuda()
    q = torch.full((B + 1, nsym), -7777.0, dtype=torch.float32, device="cuda")
    st = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    ws = models._split_workspace(B, nsym, seg_sym, "cuda")
    _lib.call("pccx_range_decode_split", ci.data_ptr(), bt.data_ptr(), by.shape[1], nt.data_ptr(), B, nsym, seg_sym, int(L), q.data_ptr(),
              st.data_ptr(), ws.data_ptr(), _stream())
    q, st = q.cpu().numpy(), st.cpu().numpy()
    assert (q[B] == -7777.0).all() and st[B] == -7, "the decoder wrote past its last output row"
    s = q[:B] + L // 2
    assert (s == np.round(s)).all()
    return s.astype(np.int64), st[:B]


@pytest.mark.parametrize("name", list(CASES))
def test_encode_equals_header_plus_oracle_segments(name):
    B, nsym, seg_sym, L = CASES[name]
    cdf, sym, files = case(name)
    cap = models.split_cap(nsym, seg_sym)
    out, nb = encode(cdf, sym, L, seg_sym, cap)
    for b in range(B):
        assert nb[b] == len(files[b]), f"cloud {b}: nbytes {nb[b]} vs {len(files[b])}"
        assert bytes(out[b, :nb[b]]) == files[b], f"cloud {b}: bytes differ from header + oracle segments"
        assert (out[b, nb[b]:] == cc.SENTINEL).all(), f"cloud {b}: wrote at or after nbytes"
    assert (out[B] == cc.SENTINEL).all(), "wrote past the last row"
    if nsym == 0:
        assert files[0] == b"PXS1" + struct.pack("<IHH", 0, seg_sym, 0) and len(files[0]) == 12 and nb[0] == 12


@pytest.mark.parametrize("name", list(CASES))
def test_decode_returns_the_symbols_and_agrees_with_the_single_stream_decoder(name):
    B, nsym, seg_sym, L = CASES[name]
    cdf, sym, files = case(name)
    by, nb = cc.rows(files, max(len(f) for f in files), 0xFF)        # tight stride, 0xFF after every file's last byte
    got, st = decode(cdf, by, nb, L, seg_sym)
    assert (st == 0).all() and np.array_equal(got, sym)
    ci = torch.from_numpy(np.ascontiguousarray(cdf)).cuda()
    q = models.range_decode_split(ci, torch.from_numpy(by).cuda(), torch.from_numpy(nb).cuda(), L, seg_sym)
    assert np.array_equal(q.cpu().numpy() + L // 2, sym)
    if nsym:                                                         # the same input as ONE stream through pccx_range_encode / _decode
        q1 = torch.from_numpy((sym - L // 2).astype(np.float32)).cuda()
        sb, sn = models.range_encode(ci, q1, L)
        assert torch.equal(models.range_decode(ci, sb, sn, L), q)


def test_capacity_exceeded_is_marked_and_confined():
    B, nsym, seg_sym, L = CASES["four_even_segments"]
    cdf, sym, files = case("four_even_segments")
    want = files[1]
    cap = cc.round4(len(want) // 2) + 1
    assert 8 <= cap < len(want)
    out, nb = encode(cdf[1:2], sym[1:2], L, seg_sym, cap)
    assert nb[0] == -len(want)
    assert bytes(out[0]) == want[:cap]
    assert (out[1] == cc.SENTINEL).all(), "overflow ran into the next row"
    cap = 16                                                         # inside the directory: the header itself is cut
    out, nb = encode(cdf[1:2], sym[1:2], L, seg_sym, cap)
    assert nb[0] == -len(want) and bytes(out[0]) == want[:cap] and (out[1] == cc.SENTINEL).all()


def _mutations(f, nsym, seg_sym):
    """(label, bytes, nbytes or None = len, status) for one valid file f of a cloud with P >= 2 segments."""
    P, segcap = models.split_segments(nsym, seg_sym), models.range_cap(seg_sym)
    lens = np.frombuffer(f[12:12 + 2 * P], dtype="<u2").astype(np.int64)

    def with_len(p, v):
        return f[:12 + 2 * p] + struct.pack("<H", v) + f[14 + 2 * p:]
    return [("wrong magic", b"PXS2" + f[4:], None, 1),
            ("magic of another case", b"pxs1" + f[4:], None, 1),
            ("nbytes 0", f, 0, 1), ("nbytes 3", f, 3, 1), ("nbytes 11", f, 11, 1),
            ("nbytes inside the directory", f, 12 + 2 * P - 1, 1),
            ("seg_sym of the file differs", f[:8] + struct.pack("<H", seg_sym - 1) + f[10:], None, 2),
            ("nsym of the file differs", f[:4] + struct.pack("<I", nsym + 1) + f[8:], None, 2),
            ("reserved field set", f[:10] + b"\x01\x00" + f[12:], None, 2),
            ("one length raised by 1", with_len(1, int(lens[1]) + 1), None, 3),
            ("one length above segcap", with_len(P - 1, segcap + 1), None, 3),
            ("every length 65535", f[:12] + b"\xff" * (2 * P) + f[12 + 2 * P:], None, 3),
            ("nbytes one less", f, len(f) - 1, 3),
            ("nbytes one more", f, len(f) + 1, 3)]


def test_refused_headers_status_error_and_the_good_clouds_of_the_batch():
    """Every refusal sits in cloud 1 of a batch of three: its status is the expected code (device and host check alike), check=True
    raises naming cloud 1 and the reason, clouds 0 and 2 still decode exactly, and cloud 1 decodes every segment as the oracle
    decodes an empty stream."""
    B, nsym, seg_sym, L = CASES["four_even_segments"]
    cdf, sym, files = case("four_even_segments")
    empty = np.concatenate([cport.range_decode(np.ascontiguousarray(cdf[1, i:i + seg_sym]), b"") for i in range(0, nsym, seg_sym)])
    want = np.stack([sym[0], empty, sym[2]])
    stride = max(len(f) for f in files) + 8
    ci = torch.from_numpy(np.ascontiguousarray(cdf)).cuda()
    for label, data, n, code in _mutations(files[1], nsym, seg_sym):
        by, nb = cc.rows([files[0], data, files[2]], stride, 0xFF)
        if n is not None:
            nb[1] = n
        got, st = decode(cdf, by, nb, L, seg_sym)
        assert st.tolist() == [0, code, 0], f"{label}: status {st.tolist()}"
        assert np.array_equal(got, want), f"{label}: symbols"
        assert models.split_stream_status(bytes(by[1, :nb[1]]), nsym, seg_sym) == code, f"{label}: host check"
        q, dst = models.range_decode_split(ci, torch.from_numpy(by).cuda(), torch.from_numpy(nb).cuda(), L, seg_sym, check=False)
        assert dst.cpu().tolist() == [0, code, 0] and np.array_equal(q.cpu().numpy() + L // 2, want)
        with pytest.raises(_lib.PccxError, match=r"clouds \[1\]") as e:
            models.range_decode_split(ci, torch.from_numpy(by).cuda(), torch.from_numpy(nb).cuda(), L, seg_sym)
        assert models.SPLIT_STATUS[code] in str(e.value), label
    # nbytes beyond the row is cut to the row, whose bytes then fail their own length sum; a negative count is an empty file
    by, nb = cc.rows(files, max(len(f) for f in files), 0xFF)
    short = int(np.argmin([len(f) for f in files]))
    assert len(files[short]) < by.shape[1]
    nb2 = nb.copy()
    nb2[short] = 1 << 30
    assert decode(cdf, by, nb2, L, seg_sym)[1][short] == 3
    nb2[short] = -5
    assert decode(cdf, by, nb2, L, seg_sym)[1][short] == 1


def test_argument_limits_are_refused_before_any_launch():
    L = 7
    seg_max = models.split_max_seg_sym(L)
    # the limit is the wave kernels' own LDS budget at segcap bytes per segment (at L = 7 the decoder's image is the larger one)
    assert cc.form(1, seg_max, L, models.range_cap(seg_max)) == 0 and cc.form(0, seg_max, L, models.range_cap(seg_max)) == 0
    assert cc.form(1, seg_max + 1, L, models.range_cap(seg_max + 1)) == 1
    assert models.split_max_seg_sym(1) == 0 == models.split_max_seg_sym(64)
    for what, nsym, seg_sym, Lc in (("seg_sym beyond the LDS budget", seg_max + 1, seg_max + 1, L), ("L = 1", 64, 16, 1), ("L = 64", 64, 16, 64),
                                    ("P above 8192", 8193, 1, L), ("seg_sym = 0", 64, 0, L)):
        cdf = torch.zeros(1, nsym, Lc + 1, dtype=torch.int32, device="cuda")
        q = torch.zeros(1, nsym, device="cuda")
        out = torch.full((2, models.split_cap(nsym, max(seg_sym, 1))), cc.SENTINEL, dtype=torch.uint8, device="cuda")
        nb = torch.full((1,), -99, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.PccxError, match=r"pccx_range_encode_split failed \(-1\)") as e:
            models.range_encode_split(cdf, q, Lc, seg_sym, out=out[:1], nb=nb)
        if what.startswith("seg_sym beyond"):
            assert f"largest seg_sym at L={L} is {seg_max}" in str(e.value)
        with pytest.raises(_lib.PccxError, match=r"pccx_range_decode_split failed \(-1\)"):
            models.range_decode_split(cdf, out[:1], nb, Lc, seg_sym)
        torch.cuda.synchronize()
        assert (out == cc.SENTINEL).all() and int(nb[0]) == -99, f"{what}: something ran"
    # the largest seg_sym that fits runs, in both directions
    cdf, sym = cc.batch(seg_max, L, 1, 5)
    f = want_file(cdf[0], sym[0], seg_max)
    out, nb = encode(cdf, sym, L, seg_max, models.split_cap(seg_max, seg_max))
    assert nb[0] == len(f) and bytes(out[0, :nb[0]]) == f
    by, n = cc.rows([f], len(f), 0xFF)
    got, st = decode(cdf, by, n, L, seg_max)
    assert st[0] == 0 and np.array_equal(got, sym)
