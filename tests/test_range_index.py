"""GPU: the entry-point index of the single range-coded stream (pccx_range_encode_indexed / pccx_range_index_build /
pccx_range_decode_indexed / pccx_range_decode_indexed_list, csrc/rangecoder.hip, format in csrc/entry_index.h) -- integers, so there
is no tolerance anywhere.

    "PXI1" | nsym u32 | seg_sym u32 | P u32 | P entries {low u32, high u32, pos u32 (bit 31: underflow pending)}     (little-endian)

The stream must stay pccx_range_encode's bytes, the entries must be the states a bit-at-a-time decoder passes through
(tests/index_cases.py restates it in Python and is itself held against the oracle's coder), and one wave per segment entering the
stream at its entry must give the sequential decoder's symbols.  B = 3 clouds of different table kinds, so the streams differ in
length."""
import functools
import struct

import numpy as np
import pytest
import torch

from oracle import cport
from pccx import _lib, models
from tests import coder_cases as cc
from tests import index_cases as ic

pytestmark = pytest.mark.gpu

L7 = 7


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()          # a copy: frombuffer arrays are read-only


def encode_indexed(cdf, sym, L, seg_sym):
    """-> (streams list of bytes, sidecars list of bytes) from pccx_range_encode_indexed."""
    q = dev((sym - L // 2).astype(np.float32))
    out, nb, index = models.range_encode_indexed(dev(cdf), q, L, seg_sym)
    out, nb, index = out.cpu().numpy(), nb.cpu().numpy(), index.cpu().numpy()
    assert (nb > 0).all()
    return [bytes(out[b, :nb[b]]) for b in range(len(nb))], [bytes(index[b]) for b in range(len(nb))]


def decode_indexed(cdf, streams, sidecars, L, seg_sym, fill=0xFF, idx_nbytes=None):
    """The raw call, outputs pre-filled with a sentinel and followed by a spare row that must come back untouched.
    -> (symbols (B,nsym) int64, status (B,))."""
    B, nsym = cdf.shape[0], cdf.shape[1]
    by, nb = cc.rows(streams, max(len(s) for s in streams), fill)
    ix, ni = cc.rows(sidecars, models.index_bytes(nsym, seg_sym), 0xEE)
    q = torch.full((B + 1, nsym), -7777.0, dtype=torch.float32, device="cuda")
    st = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    ws = models._index_workspace(B, nsym, seg_sym, "cuda")
    from pccx.ops import _stream
    ci, bt, nt, it, nit = dev(cdf), dev(by), dev(nb), dev(ix), dev(ni if idx_nbytes is None else idx_nbytes, np.int32)
    _lib.call("pccx_range_decode_indexed", ci.data_ptr(), bt.data_ptr(), by.shape[1], nt.data_ptr(), it.data_ptr(), ix.shape[1],
              nit.data_ptr(), B, nsym, seg_sym, int(L), q.data_ptr(), st.data_ptr(), ws.data_ptr(), _stream())
    q, st = q.cpu().numpy(), st.cpu().numpy()
    assert (q[B] == -7777.0).all() and st[B] == -7, "the decoder wrote past its last output row"
    s = q[:B] + L // 2
    assert (s == np.round(s)).all()
    return s.astype(np.int64), st[:B]


@functools.lru_cache(maxsize=None)
def basic():
    """nsym = 1152 in segments of 256: P = 5, the last of 128 symbols.  (cdf, sym, the oracle's streams): computed once, not modified."""
    cdf, sym = cc.batch(1152, L7, 3, 4242)
    streams = [cport.range_encode(cdf[b], sym[b].astype(np.int16)) for b in range(3)]
    assert len({len(s) for s in streams}) == 3, "the streams of the three clouds should differ in length"
    return cdf, sym, streams


def test_stream_bytes_symbols_and_the_built_index_equal_the_sequential_coder():
    cdf, sym, want = basic()
    nsym, seg = 1152, 256
    q = dev((sym - L7 // 2).astype(np.float32))
    ref_bytes, ref_nb = models.range_encode(dev(cdf), q, L7)
    out, nb, index = models.range_encode_indexed(dev(cdf), q, L7, seg)
    assert torch.equal(nb, ref_nb)
    streams, sidecars = encode_indexed(cdf, sym, L7, seg)
    for b in range(3):
        assert streams[b] == want[b] == bytes(ref_bytes[b, :int(ref_nb[b])].cpu().numpy()), f"cloud {b}: the stream is not range_encode's"
        e = ic.parse(sidecars[b], nsym, seg)
        assert e.shape == (5, 3) and tuple(e[0]) == ic.INITIAL
        _, rec = ic.decode_from(cdf[b], want[b], ic.INITIAL, 0, nsym, seg)
        assert [tuple(r) for r in e.tolist()] == rec, f"cloud {b}: entries differ from the bit-at-a-time decoder's states"
        assert models.index_status(sidecars[b], len(want[b]), nsym, seg) == 0
    assert index.shape == (3, models.index_bytes(nsym, seg)) == (3, 16 + 12 * 5)
    # the symbols: indexed decode == sequential decode == what was coded
    seq = models.range_decode(dev(cdf), ref_bytes, ref_nb, L7)
    par = models.range_decode_indexed(dev(cdf), ref_bytes, ref_nb, index, L7, seg)
    assert torch.equal(seq, par) and np.array_equal(par.cpu().numpy() + L7 // 2, sym)
    got, st = decode_indexed(cdf, want, sidecars, L7, seg)             # tight rows, 0xFF after every stream's last byte
    assert (st == 0).all() and np.array_equal(got, sym)
    # the index of an existing stream, bit for bit the encoder's; and the symbols it decodes on the way
    built, bq = models.range_index_build(dev(cdf), ref_bytes, ref_nb, L7, seg, return_latent=True)
    assert torch.equal(built, index) and torch.equal(bq, seq)
    assert torch.equal(models.range_index_build(dev(cdf), ref_bytes, ref_nb, L7, seg), index)


def test_one_segment_gives_the_single_initial_entry():
    cdf, sym, want = basic()
    for seg in (1152, 2000):
        streams, sidecars = encode_indexed(cdf, sym, L7, seg)
        for b in range(3):
            assert streams[b] == want[b]
            assert sidecars[b] == b"PXI1" + struct.pack("<III", 1152, seg, 1) + struct.pack("<III", *ic.INITIAL)
        got, st = decode_indexed(cdf, want, sidecars, L7, seg)
        assert (st == 0).all() and np.array_equal(got, sym)


def test_one_lane_kernels_write_the_same_index():
    """A cap / stride beyond the wave kernels' LDS budget takes the one-lane encoder and the one-lane decoder (the forms whole rooms
    run): the same bytes and the same entries."""
    cdf, sym, want = basic()
    nsym, seg = 1152, 256
    assert cc.form(0, nsym, L7, cc.FORM1_PAD) == 1 and cc.form(1, nsym, L7, cc.FORM1_PAD) == 1
    q = dev((sym - L7 // 2).astype(np.float32))
    out, nb, index = models.range_encode_indexed(dev(cdf), q, L7, seg, cap=cc.FORM1_PAD)
    _, _, wave_index = models.range_encode_indexed(dev(cdf), q, L7, seg)
    assert torch.equal(index, wave_index)
    for b in range(3):
        assert bytes(out[b, :int(nb[b])].cpu().numpy()) == want[b]
    assert torch.equal(models.range_index_build(dev(cdf), out, nb, L7, seg), index)
    assert np.array_equal(models.range_decode_indexed(dev(cdf), out, nb, index, L7, seg).cpu().numpy() + L7 // 2, sym)


def test_underflow_pending_at_every_boundary():
    """L = 3, table [0, 21845, 43690, 65536], every symbol the middle one.  The table is not exact thirds (3 * 21845 = 65535), so the
    interval's asymmetry about the midpoint triples with every symbol and the straddle ends after about ten symbols, then starts
    again: it is not pending for ever.  The bit-at-a-time decoder shows an underflow pending at every multiple of 13 up to 78, which
    is what this case cuts at (nsym = 91, P = 7); a second run at seg_sym = 16 over 1200 symbols has both kinds of boundary."""
    for nsym, seg, all_pending in ((91, 13, True), (1200, 16, False)):
        cdf1, sym1 = ic.underflow_case(nsym)
        cdf, sym = np.stack([cdf1] * 3), np.stack([sym1] * 3)
        stream = cport.range_encode(cdf1, sym1.astype(np.int16))
        _, rec = ic.decode_from(cdf1, stream, ic.INITIAL, 0, nsym, seg)
        streams, sidecars = encode_indexed(cdf, sym, 3, seg)
        e = ic.parse(sidecars[1], nsym, seg)
        assert streams[1] == stream and [tuple(r) for r in e.tolist()] == rec
        flags = e[1:, 2] >> 31
        if all_pending:
            assert len(flags) == 6 and flags.all(), "every entry after the first carries the pending flag"
        else:
            assert flags.any() and not flags.all()
        got, st = decode_indexed(cdf, streams, sidecars, 3, seg)
        assert (st == 0).all() and np.array_equal(got, sym), "symbols entered under a pending underflow"
        by, nb = cc.rows(streams, len(stream), 0)
        assert torch.equal(models.range_index_build(dev(cdf), dev(by), dev(nb), 3, seg).cpu(), torch.from_numpy(cc.rows(sidecars, len(sidecars[0]), 0)[0]))


def test_equal_positions_at_consecutive_boundaries():
    """L = 7, symbol 0 with cdf[1] = 65530, every symbol 0, seg_sym = 16: no bit is shifted for many symbols, so consecutive entries
    share their position and differ in `high` alone; a wave then stages nothing but the 32-bit window."""
    nsym, seg = 400, 16
    cdf1, sym1 = ic.equal_positions_case(nsym)
    cdf, sym = np.stack([cdf1] * 3), np.stack([sym1] * 3)
    streams, sidecars = encode_indexed(cdf, sym, L7, seg)
    assert streams[0] == cport.range_encode(cdf1, sym1.astype(np.int16))
    e = ic.parse(sidecars[0], nsym, seg)
    pos = e[:, 2] & 0x7FFFFFFF
    same = (pos[1:] == pos[:-1]) & (e[1:, 1] != e[:-1, 1])
    assert same.sum() >= 2, "at least two consecutive entries with equal positions and differing high"
    assert [tuple(r) for r in e.tolist()] == ic.decode_from(cdf1, streams[0], ic.INITIAL, 0, nsym, seg)[1]
    got, st = decode_indexed(cdf, streams, sidecars, L7, seg)
    assert (st == 0).all() and np.array_equal(got, sym)


@pytest.mark.parametrize("L,nsym,seg", [(7, 300, 64), (2, 257, 32), (63, 150, 50), (12, 333, 1)])
def test_random_tables_python_decoder_started_at_each_entry(L, nsym, seg):
    """The Python restatement of the decoder, started at each entry the DEVICE wrote, reproduces the oracle coder's symbols of that
    segment; the device's indexed decode gives the same."""
    cdf, sym = cc.batch(nsym, L, 3, 500 + L)
    streams, sidecars = encode_indexed(cdf, sym, L, seg)
    for b in range(3):
        assert streams[b] == cport.range_encode(cdf[b], sym[b].astype(np.int16))
        want = cport.range_decode(cdf[b], streams[b]).astype(np.int64)
        assert np.array_equal(want, sym[b])
        for p, entry in enumerate(ic.parse(sidecars[b], nsym, seg).tolist()):
            n = min(seg, nsym - p * seg)
            got, _ = ic.decode_from(cdf[b], streams[b], entry, p * seg, n)
            assert got == want[p * seg:p * seg + n].tolist(), f"cloud {b}, entry {p}"
    got, st = decode_indexed(cdf, streams, sidecars, L, seg)
    assert (st == 0).all() and np.array_equal(got, sym)


def _foreign(side, nsym, seg, stream_bytes):
    """label -> (sidecar bytes, its byte count or None = all, status) from one valid sidecar of P >= 3 entries."""
    e = [tuple(r) for r in ic.parse(side, nsym, seg).tolist()]
    maxspan = 8 * models.range_cap(seg)

    def with_entry(p, v):
        return ic.sidecar(nsym, seg, e[:p] + [v] + e[p + 1:])
    far = (e[1][2] & 0x7FFFFFFF) + maxspan + 1
    assert far <= 8 * stream_bytes, "the oversized span must stay inside the stream to be refused as a span"
    return {"truncated": (side, len(side) - 5, 1),
            "wrong_magic": (b"PXI2" + side[4:], None, 1),
            "decreasing_positions": (with_entry(2, (e[2][0], e[2][1], (e[1][2] & 0x7FFFFFFF) - 1)), None, 3),
            "position_past_the_stream": (with_entry(len(e) - 1, (e[-1][0], e[-1][1], 8 * stream_bytes + 1)), None, 4),
            "oversized_span": (with_entry(2, (e[2][0], e[2][1], far)), None, 5),
            "broken_invariant": (with_entry(1, (0x50000000, 0xB0000000, e[1][2])), None, 6)}


@pytest.mark.parametrize("label", ["truncated", "wrong_magic", "decreasing_positions", "position_past_the_stream", "oversized_span",
                                   "broken_invariant"])
def test_foreign_sidecar_is_refused_with_its_status_and_an_all_empty_decode(label):
    """The refused sidecar sits in cloud 1 of three: its status is the expected code (device and host check alike), check=True raises
    naming cloud 1, clouds 0 and 2 still decode exactly, and cloud 1 decodes every segment as the oracle decodes an empty stream.
    Nothing of cloud 1's stream is read: the check makes every segment empty before any address is formed."""
    nsym, seg, L = 1152, 32, L7                                        # P = 36; a segment may take 8 * (2*32 + 16) = 640 bits
    cdf, sym, want = basic()
    streams, sidecars = encode_indexed(cdf, sym, L, seg)
    data, n, code = _foreign(sidecars[1], nsym, seg, len(want[1]))[label]
    empty = np.concatenate([cport.range_decode(np.ascontiguousarray(cdf[1, i:i + seg]), b"") for i in range(0, nsym, seg)])
    expect = np.stack([sym[0], empty, sym[2]])
    assert models.index_status(data[:n], len(want[1]), nsym, seg) == code, "host check"
    full = len(sidecars[1])
    ni = np.array([full, full if n is None else n, full], dtype=np.int32)
    got, st = decode_indexed(cdf, want, [sidecars[0], data, sidecars[2]], L, seg, idx_nbytes=ni)
    assert st.tolist() == [0, code, 0] and np.array_equal(got, expect)
    by, nb = cc.rows(want, max(len(s) for s in want), 0xFF)
    ix, _ = cc.rows([sidecars[0], data, sidecars[2]], full, 0)
    with pytest.raises(_lib.PccxError, match=r"clouds \[1\]") as err:
        models.range_decode_indexed(dev(cdf), dev(by), dev(nb), dev(ix), L, seg, index_nbytes=dev(ni))
    assert models.INDEX_STATUS[code] in str(err.value)
    # the list form: the same status, and the check alone (n_list = 0) gives it too
    q, s1 = models.range_decode_indexed_list(None, dev(by[1]), dev(nb[1:2]), dev(np.frombuffer(data[:n], dtype=np.uint8)), L, seg, nsym, None, 0)
    assert int(s1) == code and q.numel() == 0


def test_list_form_reads_no_byte_outside_the_listed_spans():
    """Segments 3, 17 and the ragged last one of one cloud, with every stream byte that lies outside their spans (position to next
    position + the 32-bit window) poisoned: the listed symbols are still exact."""
    nsym, seg, L = 1152 - 20, 32, L7                                   # P = 36, the last segment of 12 symbols
    cdf3, sym3, _ = basic()
    cdf, sym = cdf3[2:3, :nsym], sym3[2:3, :nsym]
    (stream,), (side,) = encode_indexed(cdf, sym, L, seg)
    e = ic.parse(side, nsym, seg)
    pos = (e[:, 2] & 0x7FFFFFFF).tolist() + [8 * len(stream)]
    listed = [3, 17, 35]
    keep = np.zeros(len(stream), dtype=bool)
    for p in listed:
        keep[pos[p] // 8:min(len(stream), (pos[p + 1] + 32 + 7) // 8)] = True
    assert 0 < keep.sum() < len(stream) // 2
    poisoned = np.where(keep, np.frombuffer(stream, dtype=np.uint8), np.uint8(0x5A))
    rows = np.zeros((3, seg, L + 1), dtype=np.int32)
    for j, p in enumerate(listed):
        n = min(seg, nsym - p * seg)
        rows[j, :n] = cdf[0, p * seg:p * seg + n]
    q, st = models.range_decode_indexed_list(dev(rows.reshape(-1, L + 1)), dev(poisoned), dev(np.array([len(stream)], dtype=np.int32)),
                                             dev(np.frombuffer(side, dtype=np.uint8)), L, seg, nsym, dev(np.array(listed, dtype=np.int32)), 3)
    assert int(st) == 0
    got = q.cpu().numpy().reshape(3, seg) + L // 2
    for j, p in enumerate(listed):
        n = min(seg, nsym - p * seg)
        assert np.array_equal(got[j, :n], sym[0, p * seg:p * seg + n]), f"segment {p}"


def test_argument_limits_are_refused_before_any_launch():
    L = L7
    seg_max = models.split_max_seg_sym(L)
    for what, nsym, seg, Lc in (("seg_sym beyond the LDS budget", seg_max + 1, seg_max + 1, L), ("L = 1", 64, 16, 1), ("L = 64", 64, 16, 64),
                                ("P above 8192", 8193, 1, L), ("seg_sym = 0", 64, 0, L)):
        cdf = torch.zeros(1, nsym, Lc + 1, dtype=torch.int32, device="cuda")
        q = torch.zeros(1, nsym, device="cuda")
        out = torch.full((2, models.range_cap(nsym)), cc.SENTINEL, dtype=torch.uint8, device="cuda")
        nb = torch.full((1,), -99, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.PccxError, match=r"pccx_range_encode_indexed failed \(-1\)"):
            models.range_encode_indexed(cdf, q, Lc, seg, out=out[:1], nb=nb)
        index = torch.zeros(1, models.index_bytes(nsym, max(seg, 1)), dtype=torch.uint8, device="cuda")
        with pytest.raises(_lib.PccxError, match=r"pccx_range_decode_indexed failed \(-1\)"):
            models.range_decode_indexed(cdf, out[:1], nb, index, Lc, seg)
        with pytest.raises(_lib.PccxError, match=r"pccx_range_index_build failed \(-1\)"):
            models.range_index_build(cdf, out[:1], nb, Lc, seg)
        torch.cuda.synchronize()
        assert (out == cc.SENTINEL).all() and int(nb[0]) == -99, f"{what}: something ran"
    # the largest seg_sym that fits runs, with a ragged second segment
    cdf, sym = cc.batch(seg_max + 100, L, 1, 5)
    streams, sidecars = encode_indexed(cdf, sym, L, seg_max)
    assert streams[0] == cport.range_encode(cdf[0], sym[0].astype(np.int16))
    got, st = decode_indexed(cdf, streams, sidecars, L, seg_max)
    assert st[0] == 0 and np.array_equal(got, sym)
