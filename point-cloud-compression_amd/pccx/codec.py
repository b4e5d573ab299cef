"""Batched compress / decompress pipeline: the loop bodies of compress.py:90-152 and
decompress.py:80-116 for B clouds per launch sequence, everything resident in HBM.

The reference processes one cloud at a time (B = 1, compress.py:48) with 128 per-patch module
calls and several host round trips per cloud; here each stage is one kernel launch over the whole
batch and nothing returns to the host until the caller asks for the byte streams.

Stream formats are the reference's: ``.s.bin`` = packed octree bits (tail byte
right-aligned), ``.p.bin`` = range-coder bytes of the S*d latent symbols, ``.c.bin`` = 4 x fp32
[cx, cy, cz, longest].
"""
import collections
import dataclasses
import functools
import os

import numpy as np
import torch

from . import models, ops
from .ops import stage


def packed_layout(B, s_stride, p_cap):
    """Byte offsets of the five sections of one batch's packed stream buffer (SoA, so that every section is a dense
    tensor the kernels write in place): s_nbytes (B) i32 | p_nbytes (B) i32 | c (B,4) f32 | s_bytes (B,s_stride) u8 |
    p_bytes (B,p_cap) u8.  Everything the three files of compress.py:139-152 need, in ONE device->host copy."""
    o_sn, o_pn, o_c = 0, 4 * B, 8 * B
    o_sb = o_c + 16 * B
    o_pb = o_sb + B * s_stride
    return o_sn, o_pn, o_c, o_sb, o_pb, o_pb + B * p_cap


@dataclasses.dataclass
class Compressed:
    s_bytes: torch.Tensor     # (B, stride) u8  packed octree streams
    s_nbytes: torch.Tensor    # (B) i32
    p_bytes: torch.Tensor     # (B, cap) u8     range-coded latents
    p_nbytes: torch.Tensor    # (B) i32
    c: torch.Tensor           # (B, 4) f32      centre xyz + longest side
    n_points: int             # points per cloud; a (B,) int64 device tensor for a ragged batch (Codec.compress_ragged)
    extras: dict = None       # intermediates for tests / diagnostics
    packed: torch.Tensor = None   # the u8 buffer the five fields above are views of (packed_layout), when built by Codec
    p_index: torch.Tensor = None  # (B, 16 + 12*P) u8  entry-point index of p_bytes (<name>.p.idx), or None: no index
    p_index_nbytes: torch.Tensor = None   # (B) i32 byte counts of the sidecars when they came from files, or None: whole rows

    @classmethod
    def alloc(cls, B, s_stride, p_cap, n_points, device):
        return cls.from_packed(torch.empty(packed_layout(B, s_stride, p_cap)[-1], device=device, dtype=torch.uint8),
                               B, s_stride, p_cap, n_points)

    @classmethod
    def from_packed(cls, packed, B, s_stride, p_cap, n_points):
        """Views over a packed buffer (device: as produced by Codec.compress; or the same bytes uploaded from the host)."""
        o_sn, o_pn, o_c, o_sb, o_pb, end = packed_layout(B, s_stride, p_cap)
        if packed.numel() != end or packed.dtype != torch.uint8:
            raise ValueError(f"packed stream buffer: expected {end} bytes of uint8, got {packed.numel()} of {packed.dtype}")
        return cls(packed[o_sb:o_pb].view(B, s_stride), packed[o_sn:o_pn].view(torch.int32),
                   packed[o_pb:end].view(B, p_cap), packed[o_pn:o_c].view(torch.int32),
                   packed[o_c:o_sb].view(torch.float32).view(B, 4), n_points, None, packed)

    def bits(self):
        """Total bits per cloud of the three files (eval.py:189 numerator)."""
        return 8 * (self.s_nbytes.long() + self.p_nbytes.long() + 16)

    def bpp(self):
        return self.bits().double() / self.n_points

    def index_bits(self):
        """Bits per cloud of the entry-point index (<name>.p.idx), 0 without one.  Not part of bits() / bpp(), which stay the
        reference's three files.  Derived from the shape alone: 96 per segment of G patches and 128 of header, that is
        96 / (G*K/ALPHA) bits per input point plus 128 / N."""
        B = self.s_bytes.shape[0]
        return torch.full((B,), 0 if self.p_index is None else 8 * self.p_index.shape[1], dtype=torch.int64, device=self.s_bytes.device)

    def to_host(self):
        """ONE device->host transfer of everything the three files need (cached).  Raises PccxError when a range-coder
        output buffer was too small (the kernel reports that as a negative byte count)."""
        if getattr(self, "_host", None) is None:
            B = self.s_bytes.shape[0]
            if self.packed is None:       # assembled by hand (e.g. from files): gather the five pieces first
                comp = Compressed.alloc(B, self.s_bytes.shape[1], self.p_bytes.shape[1], self.n_points, self.s_bytes.device)
                for dst, src in ((comp.s_bytes, self.s_bytes), (comp.s_nbytes, self.s_nbytes), (comp.p_bytes, self.p_bytes),
                                 (comp.p_nbytes, self.p_nbytes), (comp.c, self.c)):
                    dst.copy_(src)
                packed = comp.packed
            else:
                packed = self.packed
            self._host_packed = packed if not packed.is_cuda else packed.cpu()
            h = Compressed.from_packed(self._host_packed, B, self.s_bytes.shape[1], self.p_bytes.shape[1], self.n_points)
            sn, pn = h.s_nbytes.numpy(), h.p_nbytes.numpy()
            if (pn < 0).any() or (sn < 0).any():
                from ._lib import PccxError
                raise PccxError("range coder / octree output buffer too small for clouds %s (negative byte count): "
                                "raise `cap`" % np.nonzero((pn < 0) | (sn < 0))[0].tolist())
            self._host = (h.s_bytes.numpy(), sn, h.p_bytes.numpy(), pn, h.c.numpy())
        return self._host

    def files(self, b):
        """The three byte strings compress.py:139-152 writes for cloud b."""
        sb, sn, pb, pn, c = self.to_host()
        return bytes(sb[b, :sn[b]]), bytes(pb[b, :pn[b]]), c[b].tobytes()

    def write_files(self, directory, names, threads=0):
        """<directory>/<names[b]>.p.bin / .s.bin / .c.bin for every cloud (compress.py:139-152), cut from ONE host copy of the packed
        buffer by the library's host threads (pccx_write_streams_host).  Returns the total number of bytes of the three files.
        With p_index present also <names[b]>.p.idx (pccx_write_index_host; not counted in the total)."""
        B = self.s_bytes.shape[0]
        if len(names) != B:
            raise ValueError(f"write_files: {len(names)} names for {B} clouds")
        self.to_host()                                         # ONE D2H (cached); raises on a negative byte count
        host = self._host_packed
        write_streams(host, B, self.s_bytes.shape[1], self.p_bytes.shape[1], directory, names, threads)
        if self.p_index is not None:
            write_index(self.p_index.cpu().contiguous(), directory, names, threads)
        return int(self._host[1].sum()) + int(self._host[3].sum()) + 16 * B

    @classmethod
    def read_files(cls, directory, names, n_points=0, s_stride=None, p_cap=None, device=None, threads=0, out=None, p_index=None):
        """The inverse (decompress.py:80-91,113): the three files of every name into one packed host buffer (rows sized from the largest
        file unless s_stride / p_cap are given; `out` = a host uint8 tensor to fill, e.g. pinned), then -- with `device` -- ONE upload.
        p_index = (nsym, seg_sym): also read <name>.p.idx of every name into p_index / p_index_nbytes (rows of the 16 + 12*P bytes
        that shape gives; a missing or longer file raises PccxError, a shorter one is refused by the decoder's check)."""
        B = len(names)
        if s_stride is None or p_cap is None:
            ss, ps = stream_sizes(directory, names, threads)
            if B and (ss.min() < 0 or ps.min() < 0):
                from ._lib import PccxError
                raise PccxError("missing .s.bin / .p.bin for: " + ", ".join(n for n, a, b_ in zip(names, ss, ps) if a < 0 or b_ < 0))
            s_stride = int(max(1, ss.max() if B else 1)) if s_stride is None else s_stride
            p_cap = int(max(1, ps.max() if B else 1)) if p_cap is None else p_cap
        need = packed_layout(B, s_stride, p_cap)[-1]
        host = out if out is not None else torch.empty(need, dtype=torch.uint8)
        if host.numel() != need or host.dtype != torch.uint8 or host.is_cuda:
            raise ValueError(f"read_files: `out` must be a host uint8 tensor of {need} bytes")
        read_streams(host, B, s_stride, p_cap, directory, names, threads)
        packed = host.to(device, non_blocking=True) if device is not None else host
        comp = cls.from_packed(packed, B, s_stride, p_cap, n_points)
        if p_index is not None:
            idx, n = read_index(directory, names, models.index_bytes(*p_index), threads)
            comp.p_index = idx.to(device) if device is not None else idx
            comp.p_index_nbytes = n.to(device) if device is not None else n
            comp._p_index_nbytes_host = n.tolist()
        return comp


def _name_table(names):
    blob, off, o = bytearray(), np.zeros(max(len(names), 1), dtype=np.int64), 0
    for i, n in enumerate(names):
        e = os.fsencode(n)
        if b"\0" in e or b"/" in e:
            raise ValueError(f"stream name {n!r}: a file name without directory part is expected")
        off[i] = o
        blob += e + b"\0"
        o += len(e) + 1
    return bytes(blob) or b"\0", off


def _host_u8(t, need, who):
    if not isinstance(t, torch.Tensor) or t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != need:
        raise ValueError(f"{who}: a contiguous host uint8 tensor of {need} bytes is expected (codec.packed_layout)")
    return t


def write_streams(packed_host, B, s_stride, p_cap, directory, names, threads=0):
    """pccx_write_streams_host: the files of B clouds from the host copy of a packed buffer (no GPU call)."""
    from . import _lib
    blob, off = _name_table(names)
    _host_u8(packed_host, packed_layout(B, s_stride, p_cap)[-1], "write_streams")
    _lib.call("pccx_write_streams_host", packed_host.data_ptr(), B, s_stride, p_cap, os.fsencode(directory), blob, off.ctypes.data, int(threads))


def read_streams(packed_host, B, s_stride, p_cap, directory, names, threads=0):
    """pccx_read_streams_host: the files of B clouds into a packed host buffer (counts, centres, rows; row tails cleared)."""
    from . import _lib
    blob, off = _name_table(names)
    _host_u8(packed_host, packed_layout(B, s_stride, p_cap)[-1], "read_streams")
    _lib.call("pccx_read_streams_host", packed_host.data_ptr(), B, s_stride, p_cap, os.fsencode(directory), blob, off.ctypes.data, int(threads))


def write_index(index_host, directory, names, threads=0):
    """pccx_write_index_host: <directory>/<names[b]>.p.idx = row b of a host (B, bytes) u8 tensor (no GPU call)."""
    from . import _lib
    blob, off = _name_table(names)
    if index_host.is_cuda or index_host.dtype != torch.uint8 or index_host.dim() != 2 or index_host.shape[0] != len(names) or not index_host.is_contiguous():
        raise ValueError(f"write_index: a contiguous host uint8 tensor of ({len(names)}, bytes) is expected")
    _lib.call("pccx_write_index_host", index_host.data_ptr(), len(names), index_host.shape[1], os.fsencode(directory), blob, off.ctypes.data, int(threads))


def read_index(directory, names, idx_bytes, threads=0):
    """pccx_read_index_host: the sidecars of every name -> (host (B, idx_bytes) u8 rows, host (B,) i32 byte counts)."""
    from . import _lib
    blob, off = _name_table(names)
    idx = torch.zeros(len(names), int(idx_bytes), dtype=torch.uint8)
    n = torch.zeros(max(len(names), 1), dtype=torch.int32)
    _lib.call("pccx_read_index_host", idx.data_ptr() if idx.numel() else n.data_ptr(), len(names), int(idx_bytes), n.data_ptr(), os.fsencode(directory), blob, off.ctypes.data, int(threads))
    return idx, n[:len(names)]


def stream_sizes(directory, names, threads=0):
    """(sizes of <name>.s.bin, sizes of <name>.p.bin) as int64 arrays, -1 where the file does not exist."""
    from . import _lib
    blob, off = _name_table(names)
    ss, ps = np.zeros(max(len(names), 1), np.int64), np.zeros(max(len(names), 1), np.int64)
    _lib.call("pccx_stream_sizes_host", len(names), os.fsencode(directory), blob, off.ctypes.data, ss.ctypes.data, ps.ctypes.data, int(threads))
    return ss[:len(names)], ps[:len(names)]


KNN_BRUTE_MAX_N = 32768        # pccx_knn / pccx_knn_list / pccx_knn_uniq keep a cloud's keys in LDS (csrc/knn.hip)
OCTREE_MAX_S = 1024            # centres per cloud pccx_octree_encode, pccx_patch_groups and the narrow full decode take
OCTREE_WIDE_MAX_S = 8192       # ... and their wide forms (pccx_octree_encode_wide, pccx_octree_decode above 1024, pccx_patch_groups_wide)


RaggedPlan = collections.namedtuple("RaggedPlan", ["S", "S_pad", "scale_compress", "scale_decompress", "s_stride", "p_cap"])


def ragged_plan(n_points, K=256, ALPHA=2, N0=1024, d=16):
    """The shape arithmetic of a ragged batch (host only): per cloud S_b = n_b*ALPHA // K patches, the patch scale of compress
    float((n_b / N0) ** (1/3)) and of decompress float((S_b*k / N0) ** (1/3)) with k = K // ALPHA -- each the very expression
    Codec.compress / Codec.decompress evaluate for a dense batch of that size -- and for the batch S_pad = 16*ceil(max S_b / 16), the
    row of the octree streams in bytes and the capacity of the range-coded rows, both those of S_pad."""
    n = [int(v) for v in n_points]
    S = [v * ALPHA // K for v in n]
    S_pad = 16 * -(-max(S + [1]) // 16)
    k = K // ALPHA
    return RaggedPlan(S, S_pad, [float((v / N0) ** (1 / 3)) for v in n], [float((s * k / N0) ** (1 / 3)) for s in S],
                      (1 + 8 * S_pad * 16 + 7) // 8, models.range_cap(S_pad * d))


RAGGED_WAY_OUT = " Such clouds go through compress / decompress, one size per call."


def ragged_patch_range(K, ALPHA):
    """(lo, hi): the patch counts S_b a cloud of a ragged batch may have, the ONE rule both sides route by.  lo = ALPHA is n_b = K;
    hi is OCTREE_MAX_S or, where that comes first, the S of KNN_BRUTE_MAX_N points.  A decoder sees S_b only, so where clouds above
    and below KNN_BRUTE_MAX_N points share that last S, and it is no multiple of 16 (the tables of the two paths differ there),
    it is left to the one-cloud path on both sides.  No K that is a power of two is affected."""
    s_lim = KNN_BRUTE_MAX_N * ALPHA // K
    hi = min(OCTREE_MAX_S, s_lim)
    if hi == s_lim and hi % 16 and ((hi + 1) * K - 1) // ALPHA > KNN_BRUTE_MAX_N:
        hi -= 1
    return ALPHA, hi


def ragged_patch_refusal(S, K, ALPHA):
    lo, hi = ragged_patch_range(K, ALPHA)
    for b, v in enumerate(S):
        if not lo <= int(v) <= hi:
            return (f"cloud {b}: S={int(v)} patches; a ragged batch takes {lo} <= S_b <= {hi} at K={K}, ALPHA={ALPHA} "
                    f"(n_b >= K points; OCTREE_MAX_S = {OCTREE_MAX_S} patches; KNN_BRUTE_MAX_N = {KNN_BRUTE_MAX_N} points)." + RAGGED_WAY_OUT)
    return None


def ragged_shape_refusal(n_points, K, ALPHA, N_max=None):
    """The shape rule of a ragged batch, stated once for the codec (Codec.ragged_refusal) and the trainer (IpdaeTrainer.step_ragged):
    why clouds of these point counts cannot share a slab of N_max rows (default: the largest count) -- a message naming the limit
    and the way out, or None.  Host only."""
    n = [int(v) for v in n_points]
    N_max = max(n) if N_max is None else int(N_max)
    if N_max > KNN_BRUTE_MAX_N:
        return f"a ragged batch holds clouds of at most KNN_BRUTE_MAX_N = {KNN_BRUTE_MAX_N} points, got N_max={N_max}." + RAGGED_WAY_OUT
    for b, v in enumerate(n):
        if v < K or v > N_max:
            return f"cloud {b}: {v} points; a ragged batch needs K = {K} <= n_b <= N_max = {N_max}." + RAGGED_WAY_OUT
    return ragged_patch_refusal([v * ALPHA // K for v in n], K, ALPHA)


def pad_clouds(clouds, device=None):
    """A list of (n_b, 3) arrays or tensors -> (pc (B, N_max, 3) f32, n_points list): every cloud in the first rows of its slab, the
    rows behind it NaN -- no kernel of the ragged path lets them reach a result, and a NaN would show it.  device: where pc goes
    (default: the first cloud's device for tensors, the host for arrays)."""
    if not len(clouds):
        raise ValueError("pad_clouds: at least one cloud is expected")
    ts = [c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)) for c in clouds]
    for b, t in enumerate(ts):
        if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError(f"pad_clouds: cloud {b} must be (n, 3) with n >= 1, got {tuple(t.shape)}")
    n = [int(t.shape[0]) for t in ts]
    device = device if device is not None else ts[0].device
    pc = torch.full((len(ts), max(n), 3), float("nan"), dtype=torch.float32, device=device)
    for b, t in enumerate(ts):
        pc[b, :n[b]] = t.to(device=device, dtype=torch.float32)
    return pc, n


def pack_clouds(clouds, device=None):
    """pad_clouds' sibling for a training set that does not fit a padded slab: a list of (n_b, 3) arrays or tensors -> (points
    (M_total, 3) f32 = the clouds one behind the other, offsets (F+1,) int64 on the same device with cloud c in rows
    offsets[c]..offsets[c+1], sizes = the host list of the n_b): the store ops.crop_nearest / train_ipdae.CropSampler cut from."""
    if not len(clouds):
        raise ValueError("pack_clouds: at least one cloud is expected")
    ts = [c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)) for c in clouds]
    for b, t in enumerate(ts):
        if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError(f"pack_clouds: cloud {b} must be (n, 3) with n >= 1, got {tuple(t.shape)}")
    sizes = [int(t.shape[0]) for t in ts]
    device = device if device is not None else ts[0].device
    points = torch.cat([t.to(device=device, dtype=torch.float32) for t in ts]).contiguous()
    offsets = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64).to(device)
    return points, offsets, sizes


def _check_patches(ae, name, G, unit):
    if G is None:
        return
    g_max = models.split_max_seg_sym(ae.L) // ae.d
    if isinstance(G, bool) or not isinstance(G, int) or not 1 <= G <= g_max:
        raise ValueError(f"{name} must be None or an int in 1..{g_max} patches per {unit} (a segment of {name}*d symbols is staged in "
                         f"LDS by one wave, d={ae.d}, L={ae.L}; L must be in 2..63), got {G!r}")


class Codec:
    def __init__(self, ae, prob, K=256, ALPHA=2, N0=1024, octree_mode="reference", margin=0.01, matmul=None,
                 decoder_matmul=None, sa_matmul=None, pn_matmul=None, group_duplicates=True, knn_search="auto",
                 max_centres=OCTREE_MAX_S, p_split=None, p_index=None, centres="fps", fps_block=8192, prob_path="cloud"):
        """matmul: how the three transforms (SetAbstraction, PointNet, decoder) form their fp32 products --
        "f32" = v_mfma_f32_16x16x4_f32 (bit-for-bit a k-ordered fmaf chain), "bf16x3" = each fp32 operand split exactly into
        three bf16 pieces, six products per pair on the bf16 matrix cores, fp32 accumulate (fp32-level error, 2.6x the
        rate).  None = pccx.DEFAULT_MATMUL.  The per-stage arguments override it.
        group_duplicates: transform each distinct patch of a cloud once and copy the result to its duplicates (ops.patch_groups; in
        octree_mode "reference" a cloud has at most 8 distinct centres among its 64).  Same bytes, same
        reconstruction either way; False computes every patch.
        knn_search: how compress finds the K points of a patch (compress.py:105-108) -- "brute" = the all-pairs kernels, which keep a
        cloud's keys in LDS and stop at KNN_BRUTE_MAX_N = 32768 points; "grid" = ops.GridIndex.knn_wide, the same patches bit for bit at any
        size; "auto" = brute wherever it can run and the grid above (the hard limit, not a tuned crossover: DESIGN.md section 4.5).
        max_centres: the most patch centres S = N*ALPHA/K a cloud may have, 1 .. OCTREE_WIDE_MAX_S = 8192.  Up to OCTREE_MAX_S = 1024 (the
        default) everything runs as before; above it the octree coder, the full decode and the patch grouping take their wide forms and
        the farthest point sampling its cooperative form (ops.farthest_point_sample_batch(workgroups="auto")) -- 1048576 points at K = 256.
        p_split: None (the default) writes ``.p.bin`` as the reference does, one range-coded stream per cloud, launch for launch as
        before.  An int G >= 1 writes the split form (include/pccx.h): the S patches are cut into segments of G patches (G*d symbols),
        each coded from a fresh coder state by its own wave behind a directory of segment lengths, so that a whole room's latents are
        coded and decoded side by side and not by one lane.  Both sides must agree on p_split, as they must
        on octree_mode: it is not recorded outside the stream's own header, which decompress checks.  A split ``.p.bin`` is NOT a file
        the reference's decompress.py reads.
        p_index: None (the default) changes nothing.  An int G >= 1 keeps ``.p.bin`` the reference's single stream, byte for byte, and
        makes compress also write an entry-point index (Compressed.p_index, the file ``.p.idx``): the coder's state every G patches,
        12 bytes each.  decompress then enters the one stream with one wave per G patches when comp.p_index is present (and decodes
        sequentially when it is absent), decompress_region takes it in place of p_split, and build_index makes the index of a file
        written without one, the reference's own included.  The same limits as p_split; the two exclude each other.
        centres: how compress picks the S patch centres of a cloud.  "fps" (the default) is the reference's farthest point sampling over
        the whole cloud, launch for launch as before.  "blocks" cuts the normalised cloud into ceil(N / fps_block) runs of its Morton
        order and samples every run on its own, all side by side (ops.farthest_point_sample_blocks; fps_block an int in 1024..16384
        points) -- a whole room's centres in a few launches instead of S dependent rounds.  The normalisation, the whole-cloud kNN
        patches and everything downstream stay as they are, and the decoder never learns how the centres were chosen (``.s.bin`` is the
        octree of whatever S points it was given): the three files are ones any decoder of this codec reads -- decompress,
        build_index, decompress_region and the reference's decompress.py, none of which takes this argument.  The choice does change
        the centres, hence the bytes and the quality (DESIGN.md section 4.5 has the measured cost).  A cloud of one block
        (N <= fps_block) gets the exact indices and the same files as "fps".
        prob_path: how compress, decompress and build_index evaluate the probability model.  "cloud" (the default) is the kernel that
        gives each cloud to one workgroup, call for call as before: right for many clouds of 64 centres.  "tiles" deals the 16-centre
        tiles of every cloud over the chip (ConditionalProbabilityModel.run(tiles=True)): for a whole room's 8192 centres, where one
        workgroup would walk 512 tiles alone.  The integer CDF is the same function of the same centres bit
        for bit, so the files are the same bytes and the two sides need NOT agree on it.  decompress(reuse_cdf=True) evaluates
        nothing, and decompress_region's own path is tiled already: neither reads this argument."""
        if prob_path not in ("cloud", "tiles"):
            raise ValueError(f"prob_path must be 'cloud' or 'tiles', got {prob_path!r}")
        self.prob_path = prob_path
        self._prob_kw = {"tiles": True} if prob_path == "tiles" else {}      # "cloud": the former call, argument for argument
        from . import DEFAULT_MATMUL
        matmul = matmul or DEFAULT_MATMUL
        self.ae, self.prob = ae, prob
        self.decoder_matmul = decoder_matmul or matmul
        self.sa_matmul, self.pn_matmul = sa_matmul or matmul, pn_matmul or matmul
        for m in (self.decoder_matmul, self.sa_matmul, self.pn_matmul):
            models.check_matmul("matmul", m)
        self.K, self.ALPHA, self.N0 = K, ALPHA, N0
        self.k = K // ALPHA                                  # compress.py:46
        self.octree_mode = octree_mode
        self.group_duplicates = bool(group_duplicates)
        self.margin = margin
        if knn_search not in ("auto", "brute", "grid"):
            raise ValueError(f"knn_search must be 'auto', 'brute' or 'grid', got {knn_search!r}")
        self.knn_search = knn_search
        if isinstance(max_centres, bool) or not isinstance(max_centres, int) or not 1 <= max_centres <= OCTREE_WIDE_MAX_S:
            raise ValueError(f"max_centres must be an int in 1..{OCTREE_WIDE_MAX_S} (the wide octree coder's limit), got {max_centres!r}")
        self.max_centres = max_centres
        _check_patches(ae, "p_split", p_split, "segment")
        if p_index is not None and p_split is not None:
            raise ValueError("p_index and p_split exclude each other: the index enters the single stream, the split form has no single stream")
        _check_patches(ae, "p_index", p_index, "entry")
        self.p_split, self.p_index = p_split, p_index
        if centres not in ("fps", "blocks"):
            raise ValueError(f"centres must be 'fps' or 'blocks', got {centres!r}")
        self.centres, self.fps_block = centres, ops.check_fps_block(fps_block)
        if ae.K != K or ae.k != self.k:
            raise ValueError("AE was built for a different K / k")

    def _distinct(self):
        """Whether the centres of a cloud repeat (at most 8 distinct among 64): then the probability model runs its distinct-centre form,
        the kNN patching walks the list and the decoder head takes one listed tile per workgroup.  In "full" mode the lists hold nearly every
        patch, where those forms cost more than they save, and the kernels take the lists as before."""
        return self.octree_mode == "reference" and self.group_duplicates

    def _check_centres(self, S, what):
        """S above max_centres: refused on the host, before anything is launched, with the limit in points and the way out."""
        m = self.max_centres
        if S > m:
            raise ValueError(f"{what}; the octree coder takes at most {m}, which is "
                             f"{m}*K/ALPHA = {m * self.K // self.ALPHA} points at K={self.K}, ALPHA={self.ALPHA}. "
                             f"Larger clouds go through pccx.large.compress_large (blocks of points).")

    def compress(self, pc, start_idx, keep_extras=False):
        """pc (B,N,3) f32 on the GPU; start_idx (B,) FPS start per cloud (the reference draws it
        from torch.randint, pn_kit.py:321)."""
        B, N, _ = pc.shape
        d, L = self.ae.d, self.ae.L
        S = int(N * self.ALPHA // self.K)                                            # compress.py:93
        self._check_centres(S, f"a cloud of {N} points gives S={S} patches")
        with stage("normalize"):
            pcn, center, longest = ops.normalize(pc, self.margin)                    # compress.py:90
        if self.octree_mode == "reference" and S != 64:
            raise ValueError(f"octree_mode='reference' reproduces octree_np.decode's hard-coded S=64 "
                             f"(octree_np.py:100; compress.py:102 asserts); got S={S}. Use octree_mode='full'.")
        with stage("fps"):
            if self.centres == "blocks":
                fps_idx = ops.farthest_point_sample_blocks(pcn, S, start_idx, block=self.fps_block)
            else:
                fps_idx = ops.farthest_point_sample_batch(pcn, S, start_idx,         # compress.py:96
                                                          workgroups="auto" if self.max_centres > OCTREE_MAX_S else None)
        with stage("gather"):
            sampled = ops.index_points(pcn, fps_idx)
        p_cap = models.range_cap(S * d) if self.p_split is None else models.split_cap(S * d, self.p_split * d)
        comp = Compressed.alloc(B, (ops.octree_bits_capacity(S) + 7) // 8, p_cap, N, pc.device)
        with stage("octree_encode"):
            oc = ops.octree_encode(sampled, N, ops.OCTREE_BPP_DICT[self.K],          # compress.py:98
                                   out_bytes=comp.s_bytes, out_nbytes=comp.s_nbytes)
        with stage("octree_decode"):
            rec, _ = ops.octree_decode(oc["bytes"], oc["nbytes"], self.octree_mode, S)   # compress.py:100
        scale = float((N / self.N0) ** (1 / 3))
        # equal centres of one cloud select the same patch and encode to the same latent rows: one transform per distinct centre.
        # With keep_extras the search still runs for every centre, so that extras["patches"] / ["knn_idx"] are complete arrays.
        groups = ops.patch_groups(rec) if self.group_duplicates else None
        with stage("knn_patches"):
            nn = ops.knn_points(rec, pcn, self.K, patch_scale=scale,                 # compress.py:105-108 (KNN_Patching keeps the
                                return_dists=False, return_idx=keep_extras,          # patches; the indices only for diagnostics)
                                search="grid" if self.knn_search == "grid" or (self.knn_search == "auto" and N > KNN_BRUTE_MAX_N) else None,
                                **({} if keep_extras or groups is None else {"groups": groups} if self._distinct() else {"rep": groups.rep}))
        patches = nn.knn.view(B * S, self.K, 3)
        raw, latent, q = self.ae.encode(patches, sa_matmul=self.sa_matmul, pn_matmul=self.pn_matmul, groups=groups)                      # compress.py:113-127
        with stage("prob"):
            cdf_int = self.prob.run(rec, ("cdf_int",), distinct=self._distinct(), **self._prob_kw)["cdf_int"]                    # compress.py:131-134
        with stage("range_encode"):
            if self.p_index is not None:
                comp.p_index = models.range_encode_indexed(cdf_int, q.view(B, S * d), L, self.p_index * d, out=comp.p_bytes, nb=comp.p_nbytes)[2]
            elif self.p_split is None:
                models.range_encode(cdf_int, q.view(B, S * d), L, out=comp.p_bytes, nb=comp.p_nbytes)   # compress.py:135-136
            else:
                models.range_encode_split(cdf_int, q.view(B, S * d), L, self.p_split * d, out=comp.p_bytes, nb=comp.p_nbytes)
        comp.c[:, :3].copy_(center)                                                  # compress.py:149-152
        comp.c[:, 3].copy_(longest)
        comp._cdf_int = cdf_int               # kept for decompress(reuse_cdf=True): the resident pipeline's shortcut, never part of the streams
        if keep_extras:
            comp.extras = dict(pcn=pcn, fps_idx=fps_idx, sampled=sampled, octree=oc, rec_sampled=rec, patches=patches,
                          latent_raw=raw, latent=latent, latent_q=q, cdf_int=cdf_int, knn_idx=nn.idx)
        return comp

    def decompress(self, comp, S=64, reuse_cdf=False):
        """Inverse pipeline (decompress.py:80-116) -> (B, S*k, 3) f32.
        reuse_cdf=True (resident pipelines only): when `comp` is the very object compress() returned, the integer CDF it coded with is
        still in HBM and the probability model is not evaluated a second time -- both sides evaluate the SAME function of the SAME
        decoded centres (compress.py:131, decompress.py:88), so the table is identical by construction.  From bytes (files, a
        Compressed built by from_packed / read_files) the table is always recomputed, as decompress.py does."""
        B = comp.s_bytes.shape[0]
        d, L = self.ae.d, self.ae.L
        self._check_centres(int(S), f"decompress(S={S})")
        with stage("octree_decode"):
            rec, cnt = ops.octree_decode(comp.s_bytes, comp.s_nbytes, self.octree_mode, S)    # decompress.py:80-85
        cdf_int = getattr(comp, "_cdf_int", None) if reuse_cdf else None
        if cdf_int is None or cdf_int.shape[0] != B or cdf_int.shape[1] != S:
            with stage("prob"):
                cdf_int = self.prob.run(rec, ("cdf_int",), distinct=self._distinct(), **self._prob_kw)["cdf_int"]                     # decompress.py:88-92
        with stage("range_decode"):
            if self.p_index is not None and comp.p_index is not None:
                q = models.range_decode_indexed(cdf_int, comp.p_bytes, comp.p_nbytes, comp.p_index, L, self.p_index * d,
                                                index_nbytes=comp.p_index_nbytes)
            elif self.p_split is None:
                q = models.range_decode(cdf_int, comp.p_bytes, comp.p_nbytes, L)          # decompress.py:93
            else:
                q = models.range_decode_split(cdf_int, comp.p_bytes, comp.p_nbytes, L, self.p_split * d)
        N = S * self.k                                                                    # decompress.py:106
        scale = float((N / self.N0) ** (1 / 3))
        with stage("ae_decode"):
            return self.ae.decode(q.view(B * S, d), rec.view(B * S, 3), comp.c[:, :3].contiguous(),
                                  comp.c[:, 3].contiguous(), S=S, scale=scale, margin=self.margin,
                                  matmul=self.decoder_matmul, group=self.group_duplicates, short_list=self._distinct())

    _RAGGED_WAY_OUT = RAGGED_WAY_OUT

    def ragged_config_refusal(self):
        """Why this Codec's configuration cannot run ragged batches at all, whatever the clouds: a message naming the setting and the
        way out, or None.  Host only."""
        out = self._RAGGED_WAY_OUT
        if self.octree_mode != "full":
            return f"ragged batches need octree_mode='full' (octree_mode='reference' is S = 64 by definition), got {self.octree_mode!r}." + out
        if self.p_split is not None or self.p_index is not None or self.centres != "fps":
            return ("ragged batches take the single .p.bin stream and whole-cloud FPS centres: p_split, p_index and centres='blocks' "
                    "are not covered." + out)
        if self.knn_search == "grid":
            return "ragged batches use the all-pairs patch search: knn_search='grid' is not covered." + out
        if not self.group_duplicates:
            return "ragged batches need group_duplicates=True: the padded centres of a cloud are skipped as its duplicates." + out
        if not self.prob.fused_ok(16):
            return (f"ragged batches need the fused probability kernel (d <= 16, L <= 15, d*L <= 128), got d={self.prob.d}, "
                    f"L={self.prob.L}." + out)
        return None

    def ragged_patch_range(self):
        """ragged_patch_range(K, ALPHA) of this Codec: the patch counts S_b a cloud of a ragged batch may have."""
        return ragged_patch_range(self.K, self.ALPHA)

    def _ragged_patch_refusal(self, S):
        return ragged_patch_refusal(S, self.K, self.ALPHA)

    def ragged_refusal(self, n_points, N_max=None):
        """Why compress_ragged cannot take a batch of these point counts (N_max: the rows of its slab, default the largest count): a
        message naming the limit and the way out, or None.  Host only; compress_ragged raises it as ValueError before anything is
        launched, and compress.py --ragged sends a refused file the existing way."""
        return self.ragged_config_refusal() or ragged_shape_refusal(n_points, self.K, self.ALPHA, N_max)

    def ragged_decode_refusal(self, S):
        """Why decompress_ragged cannot take clouds of these patch counts: the same rule seen from the decoder, which knows S_b alone
        (ragged_patch_range) -- a file compress.py --ragged sent the existing way is sent the existing way by decompress.py --ragged
        too, and a file it wrote through compress_ragged comes back through decompress_ragged.  A message or None; host only."""
        return self.ragged_config_refusal() or self._ragged_patch_refusal(S)

    def compress_ragged(self, pc, n_points, start_idx, keep_extras=False):
        """compress for clouds of different sizes in ONE launch sequence (opt-in; octree_mode "full").  pc (B,N_max,3) f32 on the
        GPU, cloud b in its first n_points[b] rows (a host sequence, K <= n_b <= N_max <= 32768); the rows behind them are padding
        that reaches no result (pad_clouds fills them with NaN).  start_idx (B,) as compress.  -> Compressed with n_points a (B,)
        tensor, its rows sized for S_pad = 16*ceil(max S_b / 16) patches (ragged_plan).

        A cloud's three streams do not depend on the batch it travels in, on N_max, S_pad or its position.  Where S_b is a multiple
        of 16 they are byte for byte those of compress(cloud[None], [start]).  For every other S_b, .s.bin and .c.bin (and the FPS
        indices, patches and latent_q) still are, but the integer CDF is DEFINED as rows [0, S_b) of the fused probability kernel's
        table on the decoded centres padded to a multiple of 16 with repeats of the last one, where compress evaluates the generic
        layers at such S (ConditionalProbabilityModel.fused_ok) and may differ in the last unit of a table entry: as with p_split,
        BOTH sides must then use the ragged path (decompress_ragged) for such a cloud.  DESIGN.md section 4.5 has the measured count.
        Refused with ValueError before any launch: what ragged_refusal names.  extras: (B, ..._max) arrays plus S and n_points."""
        B, N_max, _ = pc.shape
        n = [int(v) for v in n_points]
        if len(n) != B:
            raise ValueError(f"compress_ragged: {len(n)} point counts for {B} clouds")
        why = self.ragged_refusal(n, N_max)
        if why:
            raise ValueError("compress_ragged: " + why)
        d, L = self.ae.d, self.ae.L
        plan = ragged_plan(n, self.K, self.ALPHA, self.N0, d)
        S_pad, dev = plan.S_pad, pc.device
        n_dev, S_dev = ops.counts(n, B, dev, "n_points"), ops.counts(plan.S, B, dev, "S")
        scale = torch.tensor(plan.scale_compress, dtype=torch.float32).to(dev)
        with stage("normalize"):
            pcn, center, longest = ops.normalize_n(pc, n_dev, self.margin)
        with stage("fps"):
            fps_idx = ops.farthest_point_sample_n(pcn, n_dev, S_pad, S_dev, start_idx)
        with stage("gather"):
            sampled = ops.index_points(pcn, fps_idx)
        comp = Compressed.alloc(B, plan.s_stride, plan.p_cap, n_dev.to(torch.int64), dev)
        with stage("octree_encode"):
            oc = ops.octree_encode_n(sampled, S_dev, n_dev, ops.OCTREE_BPP_DICT[self.K], out_bytes=comp.s_bytes, out_nbytes=comp.s_nbytes)
        with stage("octree_decode"):
            rec, _ = ops.octree_decode(oc["bytes"], oc["nbytes"], "full", S_pad)      # the centres past S_b repeat the last one ...
        groups = ops.patch_groups(rec)                                                # ... and so are its duplicates: never transformed
        with stage("knn_patches"):
            nn = ops.knn_points_n(rec, pcn, n_dev, self.K, scale, rep=groups.rep)
        patches = nn.knn.view(B * S_pad, self.K, 3)
        ops.replicate_rows(groups, patches)               # only the f16x2 kernels walk the list; the others read every patch's rows
        raw, latent, q = self.ae.encode(patches, sa_matmul=self.sa_matmul, pn_matmul=self.pn_matmul, groups=groups)
        with stage("prob"):
            cdf_int = self.prob.run(rec, ("cdf_int",), **self._prob_kw)["cdf_int"]
        with stage("range_encode"):
            models.range_encode_n(cdf_int, q.view(B, S_pad * d), [s * d for s in plan.S], L, out=comp.p_bytes, nb=comp.p_nbytes)
        comp.c[:, :3].copy_(center)
        comp.c[:, 3].copy_(longest)
        if keep_extras:
            comp.extras = dict(pcn=pcn, fps_idx=fps_idx, sampled=sampled, octree=oc, rec_sampled=rec, patches=patches, latent_raw=raw,
                               latent=latent, latent_q=q, cdf_int=cdf_int, S=list(plan.S), n_points=n)
        return comp

    def decompress_ragged(self, comp, S):
        """The inverse of compress_ragged -> a list of B tensors (S_b*k, 3) f32, views of one allocation.  S: a host sequence, the
        patches of every cloud (n_b*ALPHA // K); each must equal the number of centres its .s.bin holds, else PccxError names the
        cloud (one read-back of the B counts, the only synchronisation).  The probability tables are those compress_ragged coded
        with (see there), so a cloud whose S_b is no multiple of 16 must have been written by compress_ragged."""
        B = comp.s_bytes.shape[0]
        S = [int(v) for v in S]
        if len(S) != B:
            raise ValueError(f"decompress_ragged: {len(S)} patch counts for {B} clouds")
        from ._lib import PccxError
        bad = [b for b, v in enumerate(S) if v < 1]
        if bad:
            raise PccxError(f"decompress_ragged: clouds {bad} have S={[S[b] for b in bad]}: every cloud needs at least one patch")
        why = self.ragged_decode_refusal(S)
        if why:
            raise ValueError("decompress_ragged: " + why)
        d, L, dev = self.ae.d, self.ae.L, comp.s_bytes.device
        S_pad = 16 * -(-max(S) // 16)
        with stage("octree_decode"):
            rec, cnt = ops.octree_decode(comp.s_bytes, comp.s_nbytes, "full", S_pad)
            cnt = cnt.cpu().tolist()
        bad = [b for b in range(B) if cnt[b] != S[b]]
        if bad:
            raise PccxError("decompress_ragged: " + "; ".join(f"cloud {b}: S={S[b]} given but its .s.bin holds {cnt[b]} centres" for b in bad))
        with stage("prob"):
            cdf_int = self.prob.run(rec, ("cdf_int",), **self._prob_kw)["cdf_int"]
        with stage("range_decode"):
            q = models.range_decode_n(cdf_int, comp.p_bytes, comp.p_nbytes, [s * d for s in S], L)
        scale = torch.tensor([float((s * self.k / self.N0) ** (1 / 3)) for s in S], dtype=torch.float32).to(dev)
        with stage("ae_decode"):
            # the padded patches of a cloud share their key (last centre, zero latents): one of them is decoded, none is reassembled
            groups = ops.patch_groups(rec, q.view(B, S_pad, d)) if self.decoder_matmul == "f16x2" and self.ae.fused_d else None
            raw = self.ae.decode(q.view(B * S_pad, d), matmul=self.decoder_matmul, groups=groups)
        with stage("reassemble"):
            out = ops.reassemble_n(raw, S, self.k, scale, rec, comp.c[:, :3].contiguous(), comp.c[:, 3].contiguous(), self.margin)
        return [out[b, :S[b] * self.k] for b in range(B)]

    def build_index(self, comp, S=64):
        """The entry-point index of a Compressed that has none (files written without p_index, the reference's own included): the
        probability model and the sequential decoder run once, and comp.p_index is set (and returned) -- bit for bit what compress
        with this p_index writes.  The three streams are not touched."""
        if self.p_index is None:
            raise ValueError("build_index needs p_index (patches per entry); this Codec has p_index=None")
        self._check_centres(int(S), f"build_index(S={S})")
        with stage("octree_decode"):
            rec, _ = ops.octree_decode(comp.s_bytes, comp.s_nbytes, self.octree_mode, S)
        with stage("prob"):
            cdf_int = self.prob.run(rec, ("cdf_int",), distinct=self._distinct(), **self._prob_kw)["cdf_int"]
        with stage("build_index"):
            comp.p_index = models.range_index_build(cdf_int, comp.p_bytes, comp.p_nbytes, self.ae.L, self.p_index * self.ae.d)
        comp.p_index_nbytes = None
        return comp.p_index

    def decompress_region(self, comp, S, box, halo=0.0):
        """The decoded patches of ONE cloud whose centre lies in a box, without decoding the rest -> Region.

        comp: a Compressed of one cloud (B == 1) written by a Codec with this p_split = G and octree_mode="full".  box = (lo, hi), six
        finite floats with lo <= hi in the cloud's original coordinates; halo >= 0 grows it on every side.  With rec the S decoded
        centres and w = ops.denormalize(rec, center, longest, margin), patch p is selected iff lo[a] - halo <= w[p][a] <= hi[a] + halo
        on the three axes in fp32; a touched segment is one that holds a selected patch.  Region.points is bit for bit
        ``decompress(comp, S)[0].view(S, k, 3)[patch_idx].reshape(-1, 3)``: the probability model's per-centre part, the range
        decoder and the AE decoder run for the touched segments / selected patches only.  The decoded
        centres come out in descending Morton order, so a box meets few segments.

        ONE read-back sizes the launches that follow: the two counts of the selection, together with the status word of the split
        stream's header check.  That read-back is the only synchronisation.  An empty selection returns points of shape (0, 3) and
        launches nothing after it.  Where the fused probability kernel does not cover the shape (prob.fused_ok(S) false) or the AE
        is not fused, the whole cloud is decoded by decompress() and the selected rows are taken: the same result by definition.
        Refused with ValueError before any launch: p_split None, octree_mode other than "full", a batch, a bad box or halo, S above
        max_centres.  A stream written without this split raises PccxError as decompress() does."""
        if self.p_split is None and self.p_index is None:
            raise ValueError("decompress_region needs p_split or p_index (a stream is entered at a segment through the split .p.bin's "
                             "directory or the single stream's entry-point index); this Codec has p_split=None and p_index=None")
        indexed = self.p_index is not None
        if indexed and comp.p_index is None:
            raise ValueError("decompress_region with p_index needs comp.p_index (read_files(p_index=...) or Codec.build_index first)")
        if self.octree_mode != "full":
            raise ValueError(f"decompress_region needs octree_mode='full', got octree_mode={self.octree_mode!r}")
        B = comp.s_bytes.shape[0]
        if B != 1:
            raise ValueError(f"decompress_region takes comp holding ONE cloud, got B={B}")
        ops.check_box(box, halo)
        S = int(S)
        self._check_centres(S, f"decompress_region(S={S})")
        d, L, G = self.ae.d, self.ae.L, self.p_index if indexed else self.p_split
        if indexed:
            side = comp.p_index[0]
            if comp.p_index_nbytes is not None:              # from a file: the sidecar is as long as the file was (read_files keeps the
                host_n = getattr(comp, "_p_index_nbytes_host", None)     # counts on the host too, so this is no synchronisation)
                side = side[:max(int(host_n[0] if host_n is not None else comp.p_index_nbytes[0]), 1)]
        # the listed decoder of this stream form and the cloud's stream as it takes it; an empty list runs the stream's check alone
        decode_list = functools.partial(models.range_decode_indexed_list, index=side) if indexed else models.range_decode_split_list
        stream = dict(bytes_=comp.p_bytes[0], nbytes=comp.p_nbytes, L=L, seg_sym=G * d, nsym=S * d)
        fast = self.prob.fused_ok(S) and self.ae.fused_d
        with stage("octree_decode"):
            rec, _ = ops.octree_decode(comp.s_bytes, comp.s_nbytes, self.octree_mode, S)
        head = torch.zeros(3, device=rec.device, dtype=torch.int32)           # n_sel, n_seg, status of the stream's header
        with stage("region_select"):
            sel = ops.region_select(rec[0], comp.c[0], box, G, halo, self.margin, counts=head[:2])
            if fast:
                decode_list(None, seg_idx=None, n_list=0, status=head[2:], **stream)
            n_sel, n_seg, status = (int(v) for v in head.cpu())               # THE synchronisation
        err = (models.index_status_error if indexed else models.split_status_error)("decompress_region", [status])
        if err is not None:
            raise err
        patch_idx, segments = sel.patch_idx[:n_sel], sel.seg_idx[:n_seg].to(torch.int64)
        region = lambda pts: Region(pts, patch_idx, segments, -(-S // G))
        if n_sel == 0:
            return region(torch.empty(0, 3, device=rec.device, dtype=torch.float32))
        if not fast:
            return region(self.decompress(comp, S)[0].view(S, self.k, 3)[patch_idx].reshape(-1, 3))
        with stage("prob"):
            cdf_int = self.prob.run_segments(rec[0], sel.seg_idx, n_seg, G)
        with stage("range_decode"):
            q, _ = decode_list(cdf_int, seg_idx=sel.seg_idx, n_list=n_seg, **stream)
        with stage("gather"):
            q_sel = ops.index_points(q.view(1, n_seg * G, d), sel.rows[:n_sel].view(1, n_sel))
            c_sel = ops.index_points(rec, patch_idx.view(1, n_sel))
        scale = float((S * self.k / self.N0) ** (1 / 3))                      # of the WHOLE cloud, as decompress
        with stage("ae_decode"):
            pts = self.ae.decode(q_sel.view(n_sel, d), c_sel.view(n_sel, 3), comp.c[:, :3].contiguous(), comp.c[:, 3].contiguous(),
                                 S=n_sel, scale=scale, margin=self.margin, matmul=self.decoder_matmul)
        return region(pts.view(-1, 3))


@dataclasses.dataclass
class Region:
    """What Codec.decompress_region returns.  All tensors on the device."""
    points: torch.Tensor          # (n_sel*k, 3) f32  the selected patches' points, in patch order
    patch_idx: torch.Tensor       # (n_sel,) i64      ascending
    segments: torch.Tensor        # (n_seg,) i64      the touched segments of the split stream, ascending
    n_segments_total: int         # ceil(S / G)


def d1_psnr(orig, recon, search=None, index=None):
    """eval.py:43-98 D1 (point-to-point) PSNR, batched: 10*log10(diag^2 / mean_recon min_orig |.|^2),
    diag = bounding-box diagonal of the original.  (B,N,3),(B,M,3) -> (B,) f64.  search="grid": the nearest original through an
    ops.GridIndex of the original (``index``: one the caller already built), same value."""
    d2 = ops.nn_dist(recon, index if search == "grid" and index is not None else orig, search=search).double()
    mse = d2.mean(dim=1)
    rng = orig.amax(dim=1).double() - orig.amin(dim=1).double()
    diag2 = (rng * rng).sum(dim=1)
    return 10 * torch.log10(diag2 / mse)


def d2_psnr(orig, recon, knn=30, search=None, index=None):
    """eval.py:43-98 D2 (point-to-plane) PSNR: normals of the ORIGINAL by 30-NN PCA, error = squared
    projection of (recon - nearest original) on that normal.  (B,) f64.  search="grid": ONE ops.GridIndex of the original
    (``index``, or built here) serves the normals' 30-NN and the nearest-original lookup, same value."""
    if search == "grid" and index is None:
        index = ops.GridIndex(orig)
    normals = ops.estimate_normals(orig, knn, search=search, index=index)
    mse = ops.point_plane_err(recon, orig, normals, search=search, index=index).double().mean(dim=1)
    rng = orig.amax(dim=1).double() - orig.amin(dim=1).double()
    return 10 * torch.log10((rng * rng).sum(dim=1) / mse)


def normalized_chamfer(orig, recon, search=None):
    """eval.py:198-205: both clouds min-max normalised by the ORIGINAL's global min/max, then
    pytorch3d chamfer_distance.  Returns (B,) f64.  search="grid": both directions through an ops.GridIndex of the normalised
    clouds, same value."""
    lo = orig.amin(dim=(1, 2), keepdim=True)
    hi = orig.amax(dim=(1, 2), keepdim=True)
    a = ((orig - lo) / (hi - lo)).contiguous()
    b = ((recon - lo) / (hi - lo)).contiguous()
    return ops.nn_dist(b, a, search=search).double().mean(dim=1) + ops.nn_dist(a, b, search=search).double().mean(dim=1)


EVAL_RAGGED_WAY_OUT = " Such pairs go through d1_psnr / d2_psnr / normalized_chamfer, one pair per call."


def eval_ragged_refusal(n_orig, n_recon, knn=30):
    """Why these pairs cannot be scored by evaluate_ragged -- a message naming the limit and the way out, or None.  Host only.  Every
    original needs knn <= n <= KNN_BRUTE_MAX_N points (each point's knn nearest, the all-pairs kernels' limit); every reconstruction
    2 <= m <= KNN_BRUTE_MAX_N (the uniformity coefficient takes a 2-NN distance)."""
    way_out = EVAL_RAGGED_WAY_OUT
    n, m = [int(v) for v in n_orig], [int(v) for v in n_recon]
    if len(n) != len(m):
        return f"{len(n)} originals against {len(m)} reconstructions; a ragged evaluation scores pairs." + way_out
    for b, (v, w) in enumerate(zip(n, m)):
        if not knn <= v <= KNN_BRUTE_MAX_N:
            return (f"pair {b}: the original holds {v} points; a ragged evaluation needs knn = {knn} <= n_b <= KNN_BRUTE_MAX_N = "
                    f"{KNN_BRUTE_MAX_N}." + way_out)
        if not 2 <= w <= KNN_BRUTE_MAX_N:
            return (f"pair {b}: the reconstruction holds {w} points; a ragged evaluation needs 2 <= m_b <= KNN_BRUTE_MAX_N = "
                    f"{KNN_BRUTE_MAX_N}." + way_out)
    return None


def _mask_rows(pc, n):
    """pc (B,N_max,3) with every row behind n[b] (device int32) set to NaN, whatever it held: an elementwise select, no read-back."""
    rows = torch.arange(pc.shape[1], device=pc.device, dtype=torch.int32)
    return torch.where((rows[None, :] < n[:, None])[..., None], pc, torch.full((), float("nan"), device=pc.device, dtype=pc.dtype))


def _nn_distance_var(pc, n, region):
    """calc_uc's inner value for every cloud of a slab: population variance of the distance to the nearest other point inside the
    min(region, n_b) points nearest to point 0 -> (B,) f64.  The region is ops.crop_nearest's: its key (bits of pccx_sqdist to the
    seed, index) picks the SET pccx_knn picks; it comes in ascending index, not nearest first, which a variance does not see.  The
    slab is the store (every cloud N_max rows long), so the rows behind n[b] must be NaN -- the largest keys -- and _mask_rows makes
    them so, whatever the caller left there."""
    B, N, _ = pc.shape
    dev = pc.device
    R = min(int(region), N)
    r = torch.clamp(n, max=R)
    masked = _mask_rows(pc, n)
    out = []
    for b0 in range(0, B, ops.CROP_MAX_B):                                           # pccx_crop_nearest cuts 1024 crops per call
        b1 = min(b0 + ops.CROP_MAX_B, B)
        nb = b1 - b0
        offsets = torch.arange(nb + 1, device=dev, dtype=torch.int64) * N
        crop = ops.crop_nearest(masked[b0:b1].reshape(-1, 3), offsets, torch.arange(nb, device=dev, dtype=torch.int32),
                                torch.zeros(nb, device=dev, dtype=torch.int32), r[b0:b1], R, sizes=[N] * nb)
        reg = crop - pc[b0:b1, :1]                                                   # centred on point 0 in fp32, as knn_points' patch form
        d2 = ops.knn_points_n(reg, reg, r[b0:b1], 2, torch.zeros(nb, device=dev, dtype=torch.float32),
                              rep=ops.query_rep_n(r[b0:b1], nb, R, dev), return_dists=True, return_nn=False).dists[..., 1]
        out.append(ops.mean_var_n(torch.sqrt(d2), r[b0:b1])[:, 1])
    return out[0] if len(out) == 1 else torch.cat(out)


def evaluate_ragged(orig, n_orig, recon, n_recon, knn=30, region=1024):
    """eval.py's four metrics for B pairs of clouds of different sizes in one launch sequence: orig (B,N_max,3) and recon (B,M_max,3)
    are padded slabs as pad_clouds makes them, pair b in the first n_orig[b] / n_recon[b] rows.  -> dict of (B,) f64 device tensors
    d1_psnr, d2_psnr, chamfer, uc, pair b's values those of d1_psnr / d2_psnr / normalized_chamfer / eval.py's calc_uc on the unpadded
    pair: every per-point intermediate is bit-identical (bounding box, normals, the squared distances and plane errors, the normalised
    clouds and their two scans, the 2-NN distances of the regions), only the order of the fp64 sums differs (ops.mean_var_n's fixed
    order), so a result is inf or NaN exactly where the per-file one is (mse == 0).  A pair's four values do not depend on the batch,
    its position in it or the slabs' sizes.

    The call only enqueues work on the current stream -- no read-back, no float(): the caller reads the four vectors once.  Counts
    follow ops.checked_counts: host sequences are checked (eval_ragged_refusal) before any launch, device int32 tensors are taken as
    they are.  Padding: no row behind a count reaches a result and it need not be pad_clouds' NaN -- the one step that would need it,
    the region cut of uc (ops.crop_nearest over the slab as its store), works on a copy whose padding is overwritten with NaN here."""
    from ._lib import PccxError
    (B, N), (Br, M) = ops._slab_shape(orig, "evaluate_ragged.orig"), ops._slab_shape(recon, "evaluate_ragged.recon")
    if Br != B:
        raise PccxError(f"evaluate_ragged: {B} originals against {Br} reconstructions")
    host = [None if isinstance(v, torch.Tensor) and v.is_cuda else [int(c) for c in (v.tolist() if isinstance(v, torch.Tensor) else v)]
            for v in (n_orig, n_recon)]
    if host[0] is not None and host[1] is not None:
        why = eval_ragged_refusal(host[0], host[1], knn)
        if why:
            raise ValueError("evaluate_ragged: " + why)
    if max(N, M) > KNN_BRUTE_MAX_N or N < knn or M < 2:
        raise PccxError(f"evaluate_ragged: slabs of {N} and {M} rows; a ragged evaluation needs knn = {knn} <= N_max and 2 <= M_max, both "
                        f"at most KNN_BRUTE_MAX_N = {KNN_BRUTE_MAX_N}")
    n = ops.checked_counts(n_orig if host[0] is None else host[0], B, N, orig.device, "evaluate_ragged.n_orig")
    m = ops.checked_counts(n_recon if host[1] is None else host[1], B, M, orig.device, "evaluate_ragged.n_recon")
    orig, recon = ops._f32c(orig, "evaluate_ragged.orig"), ops._f32c(recon, "evaluate_ragged.recon")
    box = ops.minmax_n(orig, n)                                                      # (B,2,3)
    rng = box[:, 1].double() - box[:, 0].double()
    diag2 = rng[:, 0] * rng[:, 0] + rng[:, 1] * rng[:, 1] + rng[:, 2] * rng[:, 2]
    with ops.stage("eval_normals"):
        normals = ops.estimate_normals_n(orig, n, knn)
    with ops.stage("eval_scans"):
        d2, plane = ops.point_errors_n(recon, orig, m, n, normals)                   # D1 and D2 from one scan
        lo, hi = box[:, 0].amin(dim=1)[:, None, None], box[:, 1].amax(dim=1)[:, None, None]
        a, b = ((orig - lo) / (hi - lo)).contiguous(), ((recon - lo) / (hi - lo)).contiguous()
        cd = ops.mean_var_n(ops.nn_dist_n(b, a, m, n), m)[:, 0] + ops.mean_var_n(ops.nn_dist_n(a, b, n, m), n)[:, 0]
    with ops.stage("eval_regions"):
        uc = _nn_distance_var(recon, m, region) / _nn_distance_var(orig, n, region)
    return dict(d1_psnr=10 * torch.log10(diag2 / ops.mean_var_n(d2, m)[:, 0]), d2_psnr=10 * torch.log10(diag2 / ops.mean_var_n(plane, m)[:, 0]),
                chamfer=cd, uc=uc)
