"""CPU: the entry-point index without a GPU -- csrc/entry_index.h compiles alone with the host compiler, the check function and the
sidecar host I/O through ctypes, the state identity on the oracle's coder (the Python decoder of tests/index_cases.py started at
every state it passed through), and the argument refusals of Codec(p_index=...)."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from oracle import cport, ref_model
from pccx import _lib, codec, models
from tests import coder_cases as cc
from tests import index_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-compression_amd", "csrc")


def _stream_and_entries(L, nsym, seg, seed, kind=None):
    cdf, sym = cc.batch(nsym, L, 5, seed)
    b = 4 if kind is None else cc.KINDS.index(kind)
    stream = cport.range_encode(cdf[b], sym[b].astype(np.int16))
    out, rec = ic.decode_from(cdf[b], stream, ic.INITIAL, 0, nsym, seg)
    assert out == sym[b].tolist() == cport.range_decode(cdf[b], stream).tolist()
    return cdf[b], sym[b], stream, rec


@pytest.mark.parametrize("L,nsym,seg", [(7, 300, 64), (3, 200, 16), (63, 150, 50)])
def test_state_identity_on_the_oracle_coder(L, nsym, seg):
    """value is the 32 stream bits at the position, bit 31 inverted under a pending underflow: started from (low, high, pos, flag)
    alone at any boundary, the decoder reproduces the oracle's symbols from there on.  All five table kinds."""
    for kind in cc.KINDS:
        cdf, sym, stream, rec = _stream_and_entries(L, nsym, seg, 99 + L, kind)
        assert len(rec) == -(-nsym // seg) and rec[0] == ic.INITIAL
        for p, entry in enumerate(rec):
            n = min(seg, nsym - p * seg)
            got, _ = ic.decode_from(cdf, stream, entry, p * seg, n)
            assert got == sym[p * seg:p * seg + n].tolist(), f"{kind}: entry {p}"
            low, high, pf = entry
            assert low < 2**31 <= high and not (low >= 2**30 and high < 3 * 2**30), "the post-renormalisation invariant"
            assert (pf & 0x7FFFFFFF) <= 8 * len(stream)
        assert models.index_status(ic.sidecar(nsym, seg, rec), len(stream), nsym, seg) == 0


def test_boundary_cases_of_the_fixed_tables():
    cdf, sym = ic.underflow_case(91)
    stream = cport.range_encode(cdf, sym.astype(np.int16))
    _, rec = ic.decode_from(cdf, stream, ic.INITIAL, 0, 91, 13)
    assert len(rec) == 7 and all(e[2] >> 31 for e in rec[1:]), "an underflow is pending at every multiple of 13 up to 78"
    cdf, sym = ic.equal_positions_case(400)
    stream = cport.range_encode(cdf, sym.astype(np.int16))
    _, rec = ic.decode_from(cdf, stream, ic.INITIAL, 0, 400, 16)
    assert sum(a[2] == b[2] and a[1] != b[1] for a, b in zip(rec, rec[1:])) >= 2
    assert models.index_status(ic.sidecar(400, 16, rec), len(stream), 400, 16) == 0


def test_check_function_on_host_bytes():
    nsym, seg = 300, 64
    _, _, stream, rec = _stream_and_entries(7, nsym, seg, 106)
    good = ic.sidecar(nsym, seg, rec)
    nb = len(stream)
    maxspan = 8 * models.range_cap(seg)
    st = lambda data, nbytes=nb, n=nsym, g=seg: models.index_status(data, nbytes, n, g)
    assert st(good) == 0 and len(good) == models.index_bytes(nsym, seg) == 16 + 12 * 5
    pos = [e[2] & 0x7FFFFFFF for e in rec]
    assert 0 < pos[1] < pos[2] and max(np.diff(pos)) <= maxspan

    def with_entry(p, v):
        return ic.sidecar(nsym, seg, rec[:p] + [v] + rec[p + 1:])
    for cut in (0, 3, 15, 16, 27, len(good) - 1):
        assert st(good[:cut]) == 1, cut                                                # inside the header, or fewer entries than it announces
    assert st(good + b"\0") == 1
    assert st(b"PXS1" + good[4:]) == 1 and st(b"pxi1" + good[4:]) == 1
    assert st(good, n=nsym + 1) == 2 and st(good, g=seg + 1) == 2
    assert st(good[:12] + struct.pack("<I", 4) + good[16:]) == 2                      # P of the file differs
    assert st(with_entry(2, (rec[2][0], rec[2][1], pos[1] - 1))) == 3
    assert st(with_entry(4, (rec[4][0], rec[4][1], 8 * nb + 1))) == 4
    assert st(with_entry(4, (rec[4][0], rec[4][1], 8 * nb))) == 0                       # the last bit's end is still a position
    assert st(good, nbytes=pos[4] // 8) == 4                                          # the index of a longer stream
    long_nsym = 4000                                                                   # a stream long enough to hold an oversized span
    _, _, lstream, lrec = _stream_and_entries(7, long_nsym, seg, 107, "one_count")
    far = (lrec[1][2] & 0x7FFFFFFF) + maxspan + 1
    assert far < 8 * len(lstream)
    bad = ic.sidecar(long_nsym, seg, lrec[:2] + [(lrec[2][0], lrec[2][1], far)] + lrec[3:])
    assert models.index_status(bad, len(lstream), long_nsym, seg) == 5
    for low, high in ((0x80000000, 0xFFFFFFFF), (0, 0x7FFFFFFF), (0x40000000, 0xBFFFFFFF), (0x90000000, 0x10000000)):
        assert st(with_entry(1, (low, high, rec[1][2]))) == 6, (low, high)
    assert st(with_entry(0, (0, 0xFFFFFFFF, 1 << 31))) == 6 and st(with_entry(0, (1, 0xFFFFFFFF, 0))) == 6   # entry 0 is the initial state
    # calls no file agrees with
    assert st(good, n=-1) == 2 and st(good, g=0) == 2 and st(good, nbytes=-1) == 2
    # nsym = 0: the 16 fixed bytes
    assert st(ic.sidecar(0, 16, []), nbytes=2, n=0, g=16) == 0


def test_sidecar_host_io(tmp_path):
    names = ["a.ply", "b", "c.bin"]
    rows = torch.arange(3 * 40, dtype=torch.int32).to(torch.uint8).view(3, 40).contiguous()
    codec.write_index(rows, str(tmp_path), names, threads=2)
    for b, n in enumerate(names):
        assert (tmp_path / (n + ".p.idx")).read_bytes() == bytes(rows[b].numpy())
    idx, cnt = codec.read_index(str(tmp_path), names, 40, threads=3)
    assert torch.equal(idx, rows) and cnt.tolist() == [40, 40, 40]
    (tmp_path / "b.p.idx").write_bytes(b"PXI1abc")                                     # a shorter file: its length, zeros behind it
    idx, cnt = codec.read_index(str(tmp_path), names, 40)
    assert cnt.tolist() == [40, 7, 40] and bytes(idx[1].numpy()) == b"PXI1abc" + b"\0" * 33 and torch.equal(idx[0], rows[0])
    with pytest.raises(_lib.PccxError, match=r"a\.ply\.p\.idx.*longer"):
        codec.read_index(str(tmp_path), names, 39)
    os.remove(tmp_path / "c.bin.p.idx")
    with pytest.raises(_lib.PccxError, match=r"c\.bin\.p\.idx"):
        codec.read_index(str(tmp_path), names, 40)
    with pytest.raises(ValueError, match="directory"):
        codec.write_index(rows, str(tmp_path), ["x/y", "b", "c"])
    with pytest.raises(ValueError, match="host uint8"):
        codec.write_index(rows[:2], str(tmp_path), names)
    # Compressed.write_files / read_files carry the sidecar when the field is present / requested, and leave the rest alone
    comp = codec.Compressed.alloc(2, 8, 12, 100, "cpu")
    comp.packed.zero_()
    comp.s_nbytes[:] = torch.tensor([3, 8], dtype=torch.int32)
    comp.p_nbytes[:] = torch.tensor([12, 5], dtype=torch.int32)
    out = tmp_path / "out"
    out.mkdir()
    comp.write_files(str(out), ["u", "v"])
    assert sorted(os.listdir(out)) == ["u.c.bin", "u.p.bin", "u.s.bin", "v.c.bin", "v.p.bin", "v.s.bin"]
    comp.p_index = rows[:2, :28].contiguous()
    assert comp.index_bits().tolist() == [224, 224] and comp.bits().tolist() == [8 * (3 + 12 + 16), 8 * (8 + 5 + 16)]
    comp.write_files(str(out), ["u", "v"])
    assert (out / "v.p.idx").read_bytes() == bytes(rows[1, :28].numpy())
    back = codec.Compressed.read_files(str(out), ["u", "v"], p_index=(16, 16))        # 16 symbols in one segment: 28 bytes
    assert torch.equal(back.p_index, comp.p_index) and back.p_index_nbytes.tolist() == [28, 28]
    assert codec.Compressed.read_files(str(out), ["u", "v"]).p_index is None


def test_argument_refusals():
    ae = models.AE(64, 32, 16, 7)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, 3))
    prob = models.ConditionalProbabilityModel(7, 16)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, 4))
    g_max = models.split_max_seg_sym(7) // 16
    assert g_max >= 64
    with pytest.raises(ValueError, match="p_index and p_split exclude each other"):
        codec.Codec(ae, prob, K=64, p_index=4, p_split=4)
    for bad in (0, -1, g_max + 1, 2.0, True, "4"):
        with pytest.raises(ValueError, match=rf"p_index must be None or an int in 1\.\.{g_max}"):
            codec.Codec(ae, prob, K=64, p_index=bad)
    assert codec.Codec(ae, prob, K=64, p_index=g_max).p_index == g_max and codec.Codec(ae, prob, K=64).p_index is None
    for badL in (1, 64):                                                              # a bad L: no entry count fits
        ae2 = models.AE(64, 32, 16, badL)
        prob2 = models.ConditionalProbabilityModel(badL, 16)
        with pytest.raises(ValueError, match=r"L must be in 2\.\.63"):
            codec.Codec(ae2, prob2, K=64, p_index=4)
    comp = codec.Compressed.alloc(1, 8, 8, 0, "meta")
    with pytest.raises(ValueError, match="build_index needs p_index"):
        codec.Codec(ae, prob, K=64).build_index(comp)
    with pytest.raises(ValueError, match="comp.p_index"):
        codec.Codec(ae, prob, K=64, octree_mode="full", p_index=4).decompress_region(comp, 16, ((0, 0, 0), (1, 1, 1)))
    with pytest.raises(ValueError, match="p_index"):
        codec.Codec(ae, prob, K=64, octree_mode="full").decompress_region(comp, 16, ((0, 0, 0), (1, 1, 1)))


MAIN = r"""
#include "entry_index.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
// Random and mutated sidecars, each in a heap block of exactly its length (the sanitizer sees any byte read past it), checked for
// what the decoder relies on: pos <= end <= 8 * stream_bytes, end - pos <= maxspan + 32, and all-empty segments on any refusal.
static unsigned long long state = 88172645463325252ull;
static unsigned rnd(unsigned n) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (unsigned)(state % n); }
static void put(uint8_t *p, uint32_t v) { p[0] = v & 255; p[1] = (v >> 8) & 255; p[2] = (v >> 16) & 255; p[3] = v >> 24; }
int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 1000;
    int ok = 0, refused = 0;
    for (int r = 0; r < rounds; ++r) {
        const int64_t seg = 1 + rnd(6), nsym = rnd(40), P = pccx_index_segments(nsym, seg), maxspan = 8 * (2 * seg + 16);
        const int64_t stream_bytes = rnd(200);
        const int64_t full = pccx_index_bytes(nsym, seg);
        uint8_t *good = (uint8_t *)malloc(full);
        memcpy(good, "PXI1", 4), put(good + 4, (uint32_t)nsym), put(good + 8, (uint32_t)seg), put(good + 12, (uint32_t)P);
        uint32_t pos = 0;
        for (int64_t p = 0; p < P; ++p) {
            uint8_t *e = good + 16 + 12 * p;
            if (p > 0) pos += rnd((unsigned)maxspan + 1);
            put(e, p ? rnd(0x80000000u) & 0x3FFFFFFFu : 0u), put(e + 4, p ? 0xC0000000u | rnd(0x40000000u) : 0xFFFFFFFFu);
            put(e + 8, pos | (p && rnd(2) ? 0x80000000u : 0u));
        }
        const int mode = rnd(4);
        int64_t n = full;
        if (mode == 1) n = rnd((unsigned)full + 1);                                 // truncated anywhere
        if (mode == 2 && full > 0) good[rnd((unsigned)full)] ^= (uint8_t)(1u << rnd(8));   // one bit flipped
        if (mode == 3) for (int64_t i = 0; i < full; ++i) good[i] = (uint8_t)rnd(256);      // noise
        uint8_t *arg = (uint8_t *)malloc(n ? n : 1);
        memcpy(arg, good, n);
        uint32_t *out = (uint32_t *)malloc(sizeof(uint32_t) * (4 * P + 1));
        for (int64_t i = 0; i <= 4 * P; ++i) out[i] = 0xDEADBEEFu;
        const int st = pccx_entry_index_check(arg, n, stream_bytes, nsym, seg, maxspan, out);
        if (st != pccx_entry_index_check(arg, n, stream_bytes, nsym, seg, maxspan, NULL)) return 2;
        if (out[4 * P] != 0xDEADBEEFu) return 3;
        for (int64_t p = 0; p < P; ++p) {
            const uint32_t lo = out[4 * p], hi = out[4 * p + 1], pf = out[4 * p + 2], end = out[4 * p + 3], at = pf & 0x7FFFFFFFu;
            if (st != PCCX_INDEX_OK) {
                if (lo != 0u || hi != 0xFFFFFFFFu || pf != 0u || end != 0u) return 4;
                continue;
            }
            if (!(at <= end && (int64_t)end <= 8 * stream_bytes && (int64_t)end - at <= maxspan + 32)) return 5;
            if (!pccx_index_state_ok(lo, hi)) return 6;
        }
        st == PCCX_INDEX_OK ? ++ok : ++refused;
        free(out), free(arg), free(good);
    }
    printf("ok %d refused %d\n", ok, refused);
    return ok > 0 && refused > 0 ? 0 : 7;
}
"""


def test_entry_index_header_compiles_alone_and_bounds_what_it_yields(tmp_path):
    """entry_index.h is plain C++ with no dependency: a stand-alone host program that includes nothing else of the project, built
    with the address and undefined-behaviour sanitizers, runs the check over random, truncated, bit-flipped and noise sidecars."""
    src, exe = tmp_path / "entry_index_main.cc", tmp_path / "entry_index_main"
    src.write_text(MAIN)
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ")
