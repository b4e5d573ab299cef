"""Shared by the entry-point index tests (tests/test_range_index.py, tests/test_entry_index_cpu.py): a Python restatement of the
bit-at-a-time range decoder that can be started at an entry, the sidecar's byte layout, and the fixed tables of the boundary cases.
Nothing here needs a GPU to import.

The state identity under test: a decoder that reaches symbol i has shifted `pos` bits in beyond its first 32, and its `value` is the
32 stream bits from bit pos on (bits past the stream are zero), bit 31 inverted when the last renormalisation step taken was an
underflow step -- each of those subtracts 2^30 before doubling, and a run of them sums to 2^31 mod 2^32."""
import struct

import numpy as np

FLAG = 1 << 31
INITIAL = (0, 0xFFFFFFFF, 0)


def window(stream, pos):
    """The 32 stream bits from bit `pos` on, MSB first, zeros past the end."""
    first = pos >> 3
    chunk = bytes(stream[first:first + 5]).ljust(5, b"\0")
    return (int.from_bytes(chunk, "big") >> (8 - (pos & 7))) & 0xFFFFFFFF


def decode_from(cdf, stream, entry, first, n, seg_sym=None):
    """Symbols first .. first+n-1 of `stream` by the reference's decoder loop, started from entry = (low, high, pos | flag).
    cdf (nsym, L+1) holding 16-bit values.  -> (symbols list, entries recorded at every multiple of seg_sym met, when given)."""
    low, high, pf = (int(v) for v in entry)
    pos, under = pf & (FLAG - 1), bool(pf & FLAG)
    value = window(stream, pos) ^ (FLAG if under else 0)
    max_symbol = cdf.shape[1] - 2
    out, rec = [], []
    for i in range(first, first + n):
        if seg_sym and i % seg_sym == 0:
            rec.append((low, high, pos | (FLAG if under else 0)))
        c = [int(v) & 0xFFFF for v in cdf[i]]
        span = high - low + 1
        count = (((value - low + 1) << 16) - 1) // span & 0xFFFF
        s = max(j for j in range(max_symbol + 1) if c[j] <= count or j == 0)
        out.append(s)
        c_high = 0x10000 if s == max_symbol else c[s + 1]
        high = (low - 1 + ((span * c_high) >> 16)) & 0xFFFFFFFF
        low = (low + ((span * c[s]) >> 16)) & 0xFFFFFFFF
        while True:
            if low >= 0x80000000 or high < 0x80000000:
                under = False
            elif low >= 0x40000000 and high < 0xC0000000:
                low &= 0x3FFFFFFF                                   # (low << 1) & 0x7FFFFFFF below
                high |= 0x40000000                                  # (high << 1) | 0x80000001 below
                under = True
            else:
                break
            low, high = (low << 1) & 0xFFFFFFFF, ((high << 1) | 1) & 0xFFFFFFFF
            pos += 1
            value = window(stream, pos) ^ (FLAG if under else 0)    # the identity, instead of carrying value along
    return out, rec


def sidecar(nsym, seg_sym, entries):
    """The .p.idx bytes of `entries` = [(low, high, pos | flag), ...]."""
    return b"PXI1" + struct.pack("<III", nsym, seg_sym, len(entries)) + b"".join(struct.pack("<III", *e) for e in entries)


def parse(data, nsym=None, seg_sym=None):
    """The entries of well-formed sidecar bytes as an (P, 3) int64 array (fields checked when given)."""
    data = bytes(data)
    assert data[:4] == b"PXI1"
    n, g, P = struct.unpack("<III", data[4:16])
    assert len(data) == 16 + 12 * P and (nsym is None or n == nsym) and (seg_sym is None or g == seg_sym) and P == -(-n // g)
    return np.frombuffer(data[16:], dtype="<u4").reshape(P, 3).astype(np.int64)


def underflow_case(nsym):
    """L = 3, thirds, every symbol the middle one: the interval straddles the midpoint for ever and no bit is ever certain."""
    cdf = np.tile(np.array([0, 21845, 43690, 0], dtype=np.int32), (nsym, 1))
    return cdf, np.full(nsym, 1, dtype=np.int64)


def equal_positions_case(nsym):
    """L = 7, symbol 0 holds 65530 of the 65536 counts and every symbol is 0: many symbols pass without a bit being shifted."""
    cdf = np.tile(np.array([0, 65530, 65531, 65532, 65533, 65534, 65535, 0], dtype=np.int32), (nsym, 1))
    return cdf, np.zeros(nsym, dtype=np.int64)
