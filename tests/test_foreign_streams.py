"""GPU: the decoders on streams no encoder of ours wrote -- they are what reads files from disk.  include/pccx.h states what each
does with arbitrary bytes (next to pccx_range_decode and pccx_octree_decode); this module pins it against the oracle.

Range decode.  With every symbol width >= 1 (tests/coder_cases.py), low <= value <= high holds after every symbol, so every byte
string decodes to some symbol sequence and the wave decoder (all candidates scaled and compared at once, bulk renormalisation)
must agree with the literal bit-at-a-time form symbol for symbol.

Octree, reference mode.  Exactly byte 0 is read; all 256 values, against octree_np.decode as the oracle restates it on
unpack_bits(bytes).  (tests/test_gpu_geometry.py's remark still holds: a stream of fewer than 8 bits packs right-aligned into its one
byte and therefore unpacks to different bits than were packed, in the reference itself.  That is why the comparison here is on
what decompress.py sees, the unpacked bytes, and not on bits before packing.)

Octree, full mode.  The stream of nbytes bytes is 8*(nbytes-1) + 1 bits: whole bytes MSB first, then ONE bit right-aligned in the last
byte (pn_kit.py:465-466), which is what makes the encoder's streams decode losslessly.  unpack_bits() (f'{b:08b}' per byte) puts
that last bit at position 8*(nbytes-1) + 7 and a 0 at 8*(nbytes-1), so on a byte string whose last byte's top and bottom bits
differ it describes another stream; the level structure is the same either way (a level ends at a position 1 + 8k, and
1 + 8k <= 8*nbytes <=> 1 + 8k <= 8*(nbytes-1) + 1).  The oracle is therefore handed `_stream_bits`: unpack_bits(bytes) cut to
8*(nbytes-1) + 1 entries with the last one replaced by the last byte's lowest bit.  Where the last byte's top and bottom bits are
equal the two readings are the same stream, and the test asserts that the oracle returns the same for both.
Equal or refused: where the oracle's depth is at most 16 and no level holds more than 2048 occupied cells, points, count and depth
are the oracle's; beyond either limit count must be -1.  The kernel does not return the depth, but a leaf coordinate
(k + 0.5) * 2^-depth = (2k + 1) * 2^-(depth+1) has an odd numerator, so it determines the depth, and `_depth_of` reads it back."""
import numpy as np
import pytest
import torch

from oracle import cport
from pccx import models, ops
from tests import coder_cases as cc

pytestmark = pytest.mark.gpu

OCT_MAX_DEPTH, OCT_MAX_NODES = 16, 2048


# ---- range decode ------------------------------------------------------------------------------------------------------------------

def range_corpus(nsym, L, seed):
    """(cdf (B,nsym,L+1), list of B byte strings): per table kind, two random strings, all 0x00, all 0xFF, the empty string, and a
    valid stream cut at each of its first 16 bytes and at half its length."""
    rng = np.random.default_rng(seed)
    cdfs, streams = [], []
    for kind in cc.KINDS:
        c, s = cc.tables(kind, nsym, L, rng)
        valid = cport.range_encode(c, s.astype(np.int16))
        n = max(len(valid), 8)
        mine = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes(), rng.integers(0, 256, size=3, dtype=np.uint8).tobytes(),
                b"\x00" * n, b"\xff" * n, b""]
        mine += [valid[:i] for i in range(1, 17) if i <= len(valid)] + [valid[:len(valid) // 2]]
        streams += mine
        cdfs += [c] * len(mine)
    return np.stack(cdfs), streams


@pytest.mark.parametrize("L", [2, 7, 63])
@pytest.mark.parametrize("nsym", [64, 1024])
def test_range_decode_of_arbitrary_bytes_in_both_forms(nsym, L):
    cdf, streams = range_corpus(nsym, L, 7000 + 10 * nsym + L)
    B = len(streams)
    want = np.stack([cport.range_decode(cdf[b], streams[b]) for b in range(B)]).astype(np.int64)
    assert want.min() >= 0 and want.max() <= L - 1
    forms = cc.decode_forms(nsym, L, max(len(s) for s in streams))
    assert [f for _, f in forms] == ([1] if (nsym, L) == (1024, 63) else [0, 1])      # 128 KiB of tables: no stride reaches the wave form
    got = {}
    for stride, f in forms:
        by, nb = cc.rows(streams, stride, 0xFF)                     # 0xFF after each stream: bytes past nbytes read as zero
        got[f] = cc.decode(cdf, by, nb, L, f)
        assert np.array_equal(got[f], want), f"form {f}: symbols differ from the oracle's on the same bytes"
    if 0 in got:
        assert np.array_equal(got[0], got[1])
    # what came out is a symbol sequence like any other: encoded again, it decodes to itself
    ci = torch.from_numpy(cdf).cuda()
    q = torch.from_numpy((want - L // 2).astype(np.float32)).cuda()
    by, nb = models.range_encode(ci, q, L, cap=4 * nsym + 16)
    assert (nb > 0).all()
    assert np.array_equal(models.range_decode(ci, by, nb, L).cpu().numpy(), q.cpu().numpy())
    for b in range(0, B, 7):
        assert bytes(by[b, :int(nb[b])].cpu().numpy()) == cport.range_encode(cdf[b], want[b].astype(np.int16))


# ---- octree ------------------------------------------------------------------------------------------------------------------------

SENT = -7777.0


def _chain(levels, rng):
    """Bits of a stream whose every level holds one occupied cell: 1 + 8*levels bits."""
    bits = [1]
    for _ in range(levels):
        g = [0] * 8
        g[int(rng.integers(0, 8))] = 1
        bits += g
    return np.array(bits, dtype=np.uint8)


def _pack(bits):
    return bytes(cport.pack_bits(np.asarray(bits, dtype=np.uint8)))


def _refused_filler():
    return _pack(_chain(OCT_MAX_DEPTH + 1, np.random.default_rng(0)))             # 17 levels, 18 bytes


def octree_full_corpus():
    """List of (tag, bytes).  Built on the CPU alone (oracle encoder, numpy)."""
    rng = np.random.default_rng(2024)
    out = []
    for S in (1, 7, 64, 500):
        pc = (0.005 + 0.99 * rng.random((S, 3))).astype(np.float32)
        bits, _ = cport.encode_sampled(pc, 1, 8192, 0.25 if S == 64 else 0.1)
        by = _pack(bits)
        assert len(by) * 8 - 7 == bits.shape[0]
        out += [(f"S{S}/cut{i}", by[:i]) for i in range(1, len(by) + 1)]                 # cut after every byte; the last is whole
        for _ in range(24):                                                              # one random bit flipped
            pos = int(rng.integers(0, bits.shape[0]))
            fl = bits.copy()
            fl[pos] ^= 1
            out.append((f"S{S}/flip{pos}", _pack(fl)))
        top = bytearray(by)
        top[-1] ^= 0x80                                                                  # a bit of the last byte the format does not read
        out.append((f"S{S}/fliptop", bytes(top)))
    for n in range(1, 65):                                                               # random bytes
        out.append((f"random{n}", rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()))
        out.append((f"random{n}/root", bytes([255]) + rng.integers(0, 256, size=n - 1, dtype=np.uint8).tobytes() if n > 1 else b"\x01"))
    # sparse random bytes walk deeper than dense ones before a level runs past the end
    for n in (8, 16, 32, 64):
        a = rng.integers(0, 256, size=n, dtype=np.uint8) & rng.integers(0, 256, size=n, dtype=np.uint8) & rng.integers(0, 256, size=n, dtype=np.uint8)
        a[0] |= 0x80
        out.append((f"sparse{n}", a.tobytes()))
    out += [("empty", b""), ("zero", b"\x00"), ("root_only", b"\x01"), ("root_top_bit", b"\x80")]
    # depth: 16 levels is the deepest stream the encoder writes, 17 is refused; trailing bytes that do not fill a level are ignored
    c16 = _chain(16, rng)
    out += [("chain16", _pack(c16)), ("chain17", _pack(_chain(17, rng))), ("chain20", _pack(_chain(20, rng)))]
    two = c16.copy()
    two[-8:] = [1, 0, 0, 0, 0, 0, 0, 1]                                                   # two leaves at level 16: a level 17 needs 16 bits
    out.append(("chain16+8bits", _pack(np.concatenate([two, rng.integers(0, 2, size=8).astype(np.uint8)]))))
    out.append(("chain16+16bits", _pack(np.concatenate([two, rng.integers(0, 2, size=16).astype(np.uint8)]))))
    # width: 1, 8, 64, 512 cells all occupied, then a last level of 4096 cells
    full = np.ones(1 + 8 + 64 + 512, dtype=np.uint8)
    for tag, k in (("2048", 2048), ("2049", 2049), ("4096", 4096)):
        last = np.zeros(4096, dtype=np.uint8)
        last[rng.permutation(4096)[:k]] = 1
        out.append((f"last_level_{tag}", _pack(np.concatenate([full, last]))))
    wide = np.concatenate([full, np.ones(4096, dtype=np.uint8), np.zeros(8 * 4096, dtype=np.uint8)])
    wide[-3] = 1
    out.append(("inner_level_4096", _pack(wide)))                                         # too wide in the middle, one leaf at the end
    return out


def _stream_bits(by):
    """The bits of a full-mode stream as the format defines them (module docstring)."""
    if len(by) == 0:
        return np.zeros(0, dtype=np.uint8)
    bits = cport.unpack_bits(by).astype(np.uint8)[:8 * (len(by) - 1) + 1]
    bits[-1] = by[-1] & 1
    return bits


def _level_counts(bits):
    """Occupied cells per level, walked as the oracle walks them (whole levels only, at most 30)."""
    if bits.shape[0] < 1 or bits[0] != 1:
        return [0]
    pops, pos = [1], 1
    while pos < bits.shape[0] and pops[-1] > 0 and len(pops) - 1 < 30 and pos + 8 * pops[-1] <= bits.shape[0]:
        pops.append(int(bits[pos:pos + 8 * pops[-1]].sum()))
        pos += 8 * (pops[-2])
    return pops


def octree_full_expected(corpus):
    """Per stream: dict(points, count, depth, refused) from the oracle on the CPU."""
    exp = []
    for tag, by in corpus:
        bits = _stream_bits(by)
        pts, depth = cport.octree_decode_full(bits, 1, cap=max(1, int(bits.sum())))
        pops = _level_counts(bits)
        assert len(pops) - 1 == depth and (pops[-1] == pts.shape[0] or pops == [0]), tag      # the walk above is the oracle's
        if len(by) and (by[-1] >> 7) == (by[-1] & 1):                                     # then unpack_bits(bytes) is the same stream
            p2, d2 = cport.octree_decode_full(cport.unpack_bits(by).astype(np.uint8), 1, cap=max(1, int(bits.sum()) + 8))
            assert d2 == depth and np.array_equal(p2, pts), tag
        exp.append(dict(tag=tag, points=pts, count=pts.shape[0], depth=depth,
                        refused=depth > OCT_MAX_DEPTH or max(pops) > OCT_MAX_NODES))
    return exp


def _depth_of(x):
    for k in range(1, 40):
        if float(x) * 2.0 ** k % 1.0 == 0.0:
            return k - 1
    raise AssertionError(f"{x} is no cell centre")


def _octree_raw(by, nbytes, mode, S_out):
    """One launch; out and count carry a spare row / entry after the batch that must come back untouched."""
    from pccx import _lib
    B, stride = by.shape
    out = torch.full((B + 1, S_out, 3), SENT, dtype=torch.float32, device="cuda")
    count = torch.full((B + 1,), -7777, dtype=torch.int32, device="cuda")
    _lib.call("pccx_octree_decode", by.data_ptr(), stride, nbytes.data_ptr(), B, {"reference": 0, "full": 1}[mode], int(S_out),
              out.data_ptr(), count.data_ptr(), ops._stream())
    out, count = out.cpu().numpy(), count.cpu().numpy()
    assert (out[B] == SENT).all() and count[B] == -7777, "the decoder wrote past its last row"
    return out[:B], count[:B]


def test_octree_reference_mode_all_256_first_bytes():
    """All 256 values of byte 0 with nbytes in {1, 2, 5} (what follows byte 0 is random and must not matter), 768 clouds in one
    launch; the kernel decodes four clouds per workgroup, so the first 767 are launched as well for a ragged last workgroup."""
    rng = np.random.default_rng(256)
    streams = [bytes([v]) + rng.integers(0, 256, size=n - 1, dtype=np.uint8).tobytes() for n in (1, 2, 5) for v in range(256)]
    by, nb = cc.rows(streams, 5, 0xFF)
    want = [cport.octree_decode_reference(cport.unpack_bits(s).astype(np.uint8), 1) for s in streams]
    for B in (768, 767):
        out, count = _octree_raw(torch.from_numpy(by[:B].copy()).cuda(), torch.from_numpy(nb[:B].copy()).cuda(), "reference", 64)
        for b in range(B):
            assert count[b] == want[b][1] == bin(streams[b][0]).count("1"), f"byte {streams[b][0]:#04x} nbytes {nb[b]}"
            assert np.array_equal(out[b], want[b][0]), f"byte {streams[b][0]:#04x} nbytes {nb[b]}"


def test_octree_full_mode_equal_or_refused():
    corpus = octree_full_corpus()
    exp = octree_full_expected(corpus)
    assert any(e["refused"] and e["depth"] > OCT_MAX_DEPTH for e in exp) and any(e["refused"] and e["depth"] <= 5 for e in exp)
    assert any(e["depth"] == OCT_MAX_DEPTH and not e["refused"] for e in exp) and any(e["count"] == OCT_MAX_NODES for e in exp)
    # every stream is followed by a stream that is refused: a refused cloud's output row is left untouched, so each real cloud
    # has a sentinel row right after its own
    streams = [s for _, by in corpus for s in (by, _refused_filler())]
    stride = max(len(s) for s in streams)
    by_np, nb_np = cc.rows(streams, stride, 0xFF)
    by_all, nb_all = torch.from_numpy(by_np).cuda(), torch.from_numpy(nb_np).cuda()
    n = len(corpus)

    def run(which, S_out):
        idx = torch.tensor([j for i in which for j in (2 * i, 2 * i + 1)], device="cuda")
        out, count = _octree_raw(by_all[idx].contiguous(), nb_all[idx].contiguous(), "full", S_out)
        assert (count[1::2] == -1).all() and (out[1::2] == SENT).all(), f"S_out={S_out}: a row after a cloud's row was written"
        for i, o, c in zip(which, out[0::2], count[0::2]):
            e = exp[i]
            if e["refused"]:
                assert c == -1, f"{e['tag']}: depth {e['depth']} must be refused, count {c}"
                continue
            assert c == e["count"], f"{e['tag']}: count {c} vs oracle {e['count']}"
            if c == 0:
                assert (o == 0).all(), e["tag"]
                continue
            m = min(int(c), S_out)
            assert np.array_equal(o[:m], e["points"][:m]), f"{e['tag']} S_out={S_out}: leaves differ"
            assert (o[m:] == e["points"][c - 1]).all(), f"{e['tag']} S_out={S_out}: padding is not the last leaf"
            assert _depth_of(o[0, 0]) == e["depth"], e["tag"]

    everything = list(range(n))
    run(everything, 1)
    run(everything, 64)
    by_count = {}
    for i, e in enumerate(exp):
        if not e["refused"] and e["count"] > 0:
            by_count.setdefault(e["count"], []).append(i)
    for c, which in sorted(by_count.items()):                       # S_out = the decoded count itself
        run(which, c)
