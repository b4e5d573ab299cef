"""CPU: the header rules of the split latent stream (csrc/split_stream.h, one function for the host and the device), through
pccx_split_stream_check_host -- loaded as tests/test_hostio.py loads the host entries, no GPU call -- and as a stand-alone program
built from the same header with the address and undefined-behaviour sanitizers.

    "PXS1" | nsym u32 | seg_sym u16 | reserved u16 = 0 | len[P] u16, P = ceil(nsym / seg_sym) | segments      (little-endian)

Status: 0 ok; 1 shorter than its header, or wrong magic; 2 nsym / seg_sym / reserved disagree with the call; 3 a length above
segcap, or header + sum of the lengths != nbytes."""
import os
import struct
import subprocess

import numpy as np

from pccx import models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-compression_amd", "csrc")


def _status(data, nsym, seg_sym, segcap=None):
    import ctypes
    from pccx import _lib
    data = bytes(data)
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    return int(_lib.load().pccx_split_stream_check_host(ctypes.addressof(buf), len(data), nsym, seg_sym,
                                                        models.range_cap(seg_sym) if segcap is None else segcap))


def _file(nsym, seg_sym, lens, payload=None, magic=b"PXS1", reserved=0):
    body = bytes(sum(lens)) if payload is None else payload
    return magic + struct.pack("<IHH", nsym, seg_sym, reserved) + np.asarray(lens, dtype="<u2").tobytes() + body


def _restated(data, nsym, seg_sym, segcap):
    """The rules of the module docstring, in numpy."""
    P, n = -(-nsym // seg_sym), len(data)
    if n < 12 or data[:4] != b"PXS1":
        return 1
    if struct.unpack("<IHH", data[4:12]) != (nsym, seg_sym, 0):
        return 2
    if 12 + 2 * P > n:
        return 1
    lens = np.frombuffer(data[12:12 + 2 * P], dtype="<u2").astype(np.int64)
    return 3 if (lens > segcap).any() or 12 + 2 * P + int(lens.sum()) != n else 0


def test_status_table_on_hand_built_headers():
    nsym, seg = 1000, 256                                           # P = 4, segcap = 528
    lens = [5, 0, 528, 17]
    good = _file(nsym, seg, lens)
    assert len(good) == 12 + 8 + 550 and _status(good, nsym, seg) == 0
    assert _status(_file(0, 16, []), 0, 16) == 0 and len(_file(0, 16, [])) == 12       # nsym = 0: the 12 fixed bytes
    assert _status(_file(5, 1, [1] * 5), 5, 1) == 0
    # 1: shorter than its header, or the magic is wrong
    for n in (0, 3, 11):
        assert _status(good[:n], nsym, seg) == 1
    assert _status(good[:12], nsym, seg) == 1 and _status(good[:19], nsym, seg) == 1   # inside the directory
    for magic in (b"PXS2", b"pXS1", b"\0\0\0\0", b"1SXP"):
        assert _status(_file(nsym, seg, lens, magic=magic), nsym, seg) == 1
    # 2: the fields disagree with the call
    assert _status(good, nsym + 1, seg) == 2 and _status(good, nsym, seg - 1) == 2 and _status(good, 999, 255) == 2
    assert _status(_file(nsym, seg, lens, reserved=1), nsym, seg) == 2
    assert _status(_file(nsym, seg, lens, reserved=0x100), nsym, seg) == 2
    assert _status(_file(nsym & 0xFFFF, seg, lens), nsym + 0x10000, seg) == 2          # all 32 bits of nsym count
    # 3: the lengths
    assert _status(_file(nsym, seg, [5, 0, 529, 17]), nsym, seg) == 3                   # above segcap, sum consistent
    assert _status(_file(nsym, seg, lens, payload=bytes(551)), nsym, seg) == 3          # one byte more than the header says
    assert _status(good[:-1], nsym, seg) == 3                                           # one byte less
    assert _status(_file(nsym, seg, [6, 0, 528, 17], payload=bytes(550)), nsym, seg) == 3   # one length raised by 1
    assert _status(_file(nsym, seg, [0xFFFF] * 4, payload=b""), nsym, seg) == 3
    assert _status(good[:20], nsym, seg) == 3                                           # the directory alone
    assert _status(good, nsym, seg, segcap=527) == 3 and _status(good, nsym, seg, segcap=528) == 0
    # the first failing rule names the status: magic before fields before lengths
    assert _status(_file(nsym + 1, seg, [0xFFFF] * 4, magic=b"XXXX"), nsym, seg) == 1
    assert _status(_file(nsym + 1, seg, [0xFFFF] * 4), nsym, seg) == 2
    assert models.split_stream_status(good, nsym, seg) == 0 and models.split_stream_status(good[:-1], nsym, seg) == 3
    assert models.split_cap(nsym, seg) == 12 + 2 * 4 + 4 * (2 * 256 + 16)


def test_agrees_with_the_numpy_restatement_on_random_strings():
    rng = np.random.default_rng(20260)
    seen = set()
    for _ in range(2000):
        n = int(rng.integers(0, 65))
        data = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        seg = int(rng.integers(1, 9))
        nsym = int(rng.integers(0, 41))
        segcap = int(rng.integers(0, 20))
        kind = int(rng.integers(0, 4))
        if kind >= 1:                                               # a valid magic, so that the later rules are reached
            data[:4] = b"PXS1"[:n]
        if kind >= 2 and n >= 12:                                   # ... and fields that agree with the call
            data[4:12] = struct.pack("<IHH", nsym, seg, 0)
        P = -(-nsym // seg)
        if kind == 3 and n >= 12 + 2 * P:                           # ... and lengths that add up (some still above segcap)
            left, lens = n - 12 - 2 * P, []
            for p in range(P):
                lens.append(left if p == P - 1 else int(rng.integers(0, min(left, 2 * segcap) + 1)))
                left -= lens[-1]
            if P:
                data[12:12 + 2 * P] = np.asarray(lens, dtype="<u2").tobytes()
        want = _restated(bytes(data), nsym, seg, segcap)
        assert _status(data, nsym, seg, segcap) == want, (bytes(data), nsym, seg, segcap)
        seen.add(want)
    assert seen == {0, 1, 2, 3}                                     # the draw reaches every status


_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "split_stream.h"

static uint64_t state;
static uint32_t rnd(uint32_t n) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (uint32_t)((state >> 11) % n); }

// every byte string lives in a heap block of exactly its length and the offsets in one of exactly P + 1 entries: a read at or
// after nbytes, or an offset written outside, is an error the address sanitizer reports
static int one(const uint8_t *src, int64_t n, int64_t nsym, int64_t seg, int64_t segcap, int want_ok)
{
    const int64_t P = pccx_split_segments(nsym, seg);
    uint8_t *b = (uint8_t *)malloc(n ? n : 1);
    int32_t *off = (int32_t *)malloc((P + 1) * sizeof(int32_t));
    if (n) memcpy(b, src, n);
    uint8_t *arg = n ? b : NULL;                                   // nbytes = 0: not even the pointer is needed
    const int st = pccx_split_stream_check(arg, n, nsym, seg, segcap, off);
    const int st2 = pccx_split_stream_check(arg, n, nsym, seg, segcap, NULL);
    int bad = st != st2 || st < 0 || st > 3 || (want_ok >= 0 && (st == 0) != want_ok);
    for (int64_t p = 0; p <= P; ++p) bad |= off[p] < 0 || off[p] > n || (p && off[p] < off[p - 1]);
    for (int64_t p = 0; p < P; ++p) bad |= st == 0 ? off[p + 1] - off[p] > segcap : off[p] != 0;
    if (st == 0) bad |= off[0] != 12 + 2 * P || off[P] != n;
    free(off);
    free(b);
    if (bad) fprintf(stderr, "violation: n=%lld nsym=%lld seg=%lld segcap=%lld status=%d\n", (long long)n, (long long)nsym, (long long)seg, (long long)segcap, st);
    return bad;
}

int main(int argc, char **argv)
{
    state = argc > 1 ? strtoull(argv[1], NULL, 10) * 2654435761u + 1 : 1;
    int bad = 0;
    uint8_t buf[4096];
    for (int it = 0; it < 2000; ++it) {
        const int64_t n = rnd(65), seg = 1 + rnd(8), nsym = rnd(41), segcap = rnd(20), P = pccx_split_segments(nsym, seg);
        for (int i = 0; i < n; ++i) buf[i] = (uint8_t)rnd(256);
        const uint32_t kind = rnd(4);
        if (kind >= 1) memcpy(buf, "PXS1", n < 4 ? n : 4);
        if (kind >= 2 && n >= 12) {
            for (int i = 0; i < 4; ++i) buf[4 + i] = (uint8_t)(nsym >> (8 * i));
            buf[8] = (uint8_t)seg; buf[9] = buf[10] = buf[11] = 0;
        }
        if (kind == 3 && n >= 12 + 2 * P) {
            int64_t left = n - 12 - 2 * P;
            for (int64_t p = 0; p < P; ++p) {
                const int64_t cap2 = left < 2 * segcap ? left : 2 * segcap, len = p == P - 1 ? left : rnd((uint32_t)cap2 + 1);
                buf[12 + 2 * p] = (uint8_t)len; buf[13 + 2 * p] = (uint8_t)(len >> 8);
                left -= len;
            }
        }
        bad |= one(buf, n, nsym, seg, segcap, -1);
    }
    // one valid file (nsym = 1000, seg_sym = 256: P = 4, segcap = 528) and every truncation of it
    const int64_t lens[4] = {5, 0, 528, 17};
    memset(buf, 0, sizeof buf);
    memcpy(buf, "PXS1", 4);
    buf[4] = 1000 & 255; buf[5] = 1000 >> 8; buf[8] = 0; buf[9] = 1;
    for (int p = 0; p < 4; ++p) { buf[12 + 2 * p] = (uint8_t)lens[p]; buf[13 + 2 * p] = (uint8_t)(lens[p] >> 8); }
    const int64_t full = 12 + 8 + 550;
    for (int64_t n = 0; n <= full; ++n) bad |= one(buf, n, 1000, 256, 528, n == full);
    // lengths that say 65535 each while the file ends right after the directory: the offsets stay inside the 20 bytes
    for (int p = 0; p < 4; ++p) buf[12 + 2 * p] = buf[13 + 2 * p] = 0xFF;
    bad |= one(buf, 20, 1000, 256, 65535, 0);
    return bad ? 1 : 0;
}
"""


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/split_stream.h compiled by the host compiler alone, with a main of its own, -fsanitize=address,undefined (runtimes linked
    statically, so the program needs nothing from its environment): random strings as above, every truncation of one valid file,
    each in a heap block of exactly its size, plus the offsets' invariants (inside the file, non-decreasing, all zero on refusal)."""
    src, exe = tmp_path / "split_header_main.cc", tmp_path / "split_header_main"
    src.write_text(_MAIN)
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), "20260"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
