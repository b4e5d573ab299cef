"""Inputs shared by tests/test_range_coder_forms.py and tests/test_foreign_streams.py: the CDF table family, symbol draws, raw
launches with sentinels, and the oracle side of each comparison.  Everything is seeded; nothing here needs a GPU to import.

Table family.  A table row holds L+1 entries: entry 0 is 0, entries 1..L-1 increase strictly, entry L stands for 2^16 and is stored
as 0 (2^16 wrapped to 16 bits, as torchac stores it).  Every one of the L symbol widths, the last symbol's 2^16 - c[L-1] included,
is at least 1: a zero width lets `span` reach 0, where the oracle's division traps, so this is a condition on the inputs and
`assert_widths` is called on every table that is generated.  The kinds are those of
test_range_coder_adversarial_tables_match_oracle_bit_for_bit, stated for any L."""
import numpy as np

KINDS = ("sliver", "one_count", "near_certain", "uniform", "random")
FORM1_PAD = 61440          # a cap / stride that by itself exceeds the wave kernels' LDS budget of 60 KiB
SENTINEL = 0xA5


def round4(v):
    return (int(v) + 3) // 4 * 4


def tables(kind, nsym, L, rng):
    """(cdf (nsym, L+1) int32, sym (nsym,) int64): one cloud's tables of one kind and symbols drawn to exercise it."""
    c = np.zeros((nsym, L + 1), dtype=np.int64)
    sym = rng.integers(0, L, size=nsym)
    j = np.arange(L)
    if L == 1:
        pass                                                       # the only table: one symbol of width 2^16
    elif kind == "sliver":                                         # symbol L//2 straddles 0x8000 two counts wide: long E3 runs
        m = L // 2
        row = np.where(j < m, j, 0x10000 - (L - j))
        row[m] = 0x7FFF
        if m + 1 < L:
            row[m + 1] = 0x8001
        c[:, :L] = row
        sym = np.where(rng.random(nsym) < 0.9, m, sym)
    elif kind == "one_count":                                      # every symbol one count wide but one per row: 16-bit symbols
        k = rng.integers(0, L, size=nsym)
        w = np.ones((nsym, L), dtype=np.int64)
        w[np.arange(nsym), k] = 0x10000 - (L - 1)
        c[:, 1:L] = np.cumsum(w, axis=1)[:, :-1]
        sym = np.where(rng.random(nsym) < 0.5, k, sym)
    elif kind == "near_certain":                                   # symbol L-2 holds all but L-1 counts: long E1/E2-free stretches
        row = j.copy()
        row[L - 1] = 0xFFFF
        c[:, :L] = row
        sym = np.where(rng.random(nsym) < 0.97, max(L - 2, 0), sym)
    elif kind == "uniform":
        c[:, :L] = (j * 0x10000) // L
    elif kind == "random":                                         # random strictly increasing
        e = rng.exponential(size=(nsym, L))
        w = 1 + np.floor(e / e.sum(axis=1, keepdims=True) * (0x10000 - 2 * L)).astype(np.int64)
        c[:, 1:L] = np.cumsum(w, axis=1)[:, :-1]
    else:
        raise ValueError(kind)
    c = c.astype(np.int32)
    assert_widths(c)
    return c, sym


def assert_widths(cdf):
    """The input condition of the whole family: entry 0 is 0 and all L widths are >= 1 (the last against 2^16)."""
    c = np.asarray(cdf).astype(np.int64) & 0xFFFF
    L = c.shape[-1] - 1
    edges = np.concatenate([c[..., :L], np.full(c.shape[:-1] + (1,), 0x10000, dtype=np.int64)], axis=-1)
    assert (c[..., 0] == 0).all() and (np.diff(edges, axis=-1) >= 1).all(), "a table gives some symbol a zero width"


def batch(nsym, L, B, seed):
    """B clouds cycling through the five kinds: (cdf (B,nsym,L+1) int32, sym (B,nsym) int64)."""
    rng = np.random.default_rng(seed)
    cs, ss = zip(*(tables(KINDS[b % len(KINDS)], nsym, L, rng) for b in range(B)))
    return np.stack(cs), np.stack(ss)


def rows(streams, stride, fill):
    """Byte strings -> ((B,stride) uint8 with everything past each stream set to `fill`, lengths (B,) int32)."""
    out = np.full((len(streams), stride), fill, dtype=np.uint8)
    for b, s in enumerate(streams):
        out[b, :len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    return out, np.array([len(s) for s in streams], dtype=np.int32)


# ---- the device side (imports torch / pccx lazily so that the CPU pass can use the generators alone) ----------------------------

def form(decode, nsym, L, cap_or_stride):
    from pccx import _lib
    return int(_lib.load().pccx_range_coder_form(int(decode), int(nsym), int(L), int(cap_or_stride)))


def encode(cdf, q, L, cap, want_form):
    """Encode on the device into rows pre-filled with SENTINEL, one spare row after the batch.  Asserts through the query that the call
    runs the kernel `want_form` names.  -> (out (B+1,cap) uint8 numpy, nbytes (B,) numpy)."""
    import torch
    from pccx import models
    B, nsym = q.shape
    assert form(0, nsym, L, cap) == want_form, f"encode nsym={nsym} L={L} cap={cap} is not form {want_form}"
    buf = torch.full((B + 1, cap), SENTINEL, dtype=torch.uint8, device="cuda")
    _, nb = models.range_encode(torch.from_numpy(cdf).cuda(), torch.from_numpy(np.asarray(q, dtype=np.float32)).cuda(), L, out=buf[:B])
    return buf.cpu().numpy(), nb.cpu().numpy()


def decode(cdf, by, nbytes, L, want_form):
    """Decode rows `by` (B,stride) on the device into rows pre-filled with a sentinel, one spare row after the batch, which must
    come back untouched.  -> symbols (B,nsym) int64 (latent + L//2)."""
    import torch
    from pccx import _lib
    from pccx.ops import _stream
    B, nsym = cdf.shape[0], cdf.shape[1]
    stride = by.shape[1]
    assert form(1, nsym, L, stride) == want_form, f"decode nsym={nsym} L={L} stride={stride} is not form {want_form}"
    ci = torch.from_numpy(np.ascontiguousarray(cdf)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(by)).cuda()
    nt = torch.from_numpy(np.asarray(nbytes, dtype=np.int32)).cuda()
    q = torch.full((B + 1, nsym), -7777.0, dtype=torch.float32, device="cuda")
    _lib.call("pccx_range_decode", ci.data_ptr(), bt.data_ptr(), stride, nt.data_ptr(), B, nsym, int(L), q.data_ptr(), _stream())
    q = q.cpu().numpy()
    assert (q[B] == -7777.0).all(), "the decoder wrote past its last output row"
    s = q[:B] + L // 2
    assert (s == np.round(s)).all()
    return s.astype(np.int64)


def decode_forms(nsym, L, nbmax):
    """(stride, form) pairs that decode streams of up to nbmax bytes in each form the launcher can reach at (nsym, L): form 1 by
    padding the stride, form 0 with the tight stride -- unless the tables alone exceed the LDS budget or L is outside 2..63,
    where no stride reaches the wave kernel and the only pair is the tight one, form 1."""
    tight = max(int(nbmax), 1)
    fixed = round4(nsym * (L + 1) * 2) + nsym
    wave_reachable = 2 <= L <= 63 and fixed + round4(tight) <= FORM1_PAD
    assert form(1, nsym, L, tight) == (0 if wave_reachable else 1)
    return [(tight, 0), (max(FORM1_PAD, tight), 1)] if wave_reachable else [(tight, 1)]
