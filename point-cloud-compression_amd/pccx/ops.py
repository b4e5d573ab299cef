"""Tensor-level operators over libpccx.so, named after the reference callables they replace.

PyTorch is used for device memory and streams only; every computation is a HIP kernel behind
the C ABI (include/pccx.h).  Inputs must live on a ROCm device: there is no CPU path.
"""
import collections

import torch

from . import _lib

KNN = collections.namedtuple("KNN", ["dists", "idx", "knn"])      # pytorch3d's _KNN result shape
# duplicate patches of a batch (patch_groups): rep (B*S) i32 = first patch of the same cloud with an equal key row, uniq (B*S) i32 = the
# patches with rep[p] == p, n_uniq (1) i32 = how many -- all on the device, never read back
Groups = collections.namedtuple("Groups", ["rep", "uniq", "n_uniq"])
OCTREE_BPP_DICT = {1024: 0.07, 512: 0.125, 256: 0.25, 128: 0.5, 64: 1.0}   # pn_kit.py:17-23


def _stream():
    return torch.cuda.current_stream().cuda_stream


class StageTimer:
    """Optional per-stage HIP-event timing (bench.py).  Events are recorded on torch's current
    stream, the stream every pccx kernel is launched on."""

    def __init__(self):
        self.records = []

    def totals_ms(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.records:
            t, n = out.get(name, (0.0, 0))
            out[name] = (t + a.elapsed_time(b), n + 1)
        return out


_timer = None


def set_timer(t):
    global _timer
    _timer = t


class stage:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if _timer is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if _timer is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _timer.records.append((self.name, self.a, b))
        return False


def _dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.PccxError(f"{name}: expected a tensor on the GPU (pccx has no CPU fallback)")
    return t


def _f32c(t, name):
    _dev(t, name)
    if t.dtype != torch.float32:
        raise _lib.PccxError(f"{name}: expected float32, got {t.dtype}")
    return t.contiguous()


def normalize(pc, margin=0.01):
    """pn_kit.normalize (pn_kit.py:47-60), batched over B: returns (pc, center (B,3), longest (B))."""
    pc = _f32c(pc, "normalize")
    B, N, _ = pc.shape
    out = torch.empty_like(pc)
    center = torch.empty(B, 3, device=pc.device, dtype=torch.float32)
    longest = torch.empty(B, device=pc.device, dtype=torch.float32)
    _lib.call("pccx_normalize", pc.data_ptr(), B, N, float(margin), out.data_ptr(), center.data_ptr(),
              longest.data_ptr(), _stream())
    return out, center, longest


def counts(v, B, device, name):
    """A per-cloud count table of a ragged batch as the kernels take it: (B,) int32 on the device, from a host sequence or a tensor."""
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor([int(x) for x in v], dtype=torch.int32)
    t = t.to(device=device, dtype=torch.int32).contiguous()
    if tuple(t.shape) != (B,):
        raise _lib.PccxError(f"{name}: one int per cloud is expected, got {tuple(t.shape)} for {B} clouds")
    return t


def normalize_n(pc, n, margin=0.01):
    """normalize for a ragged batch (pccx_normalize_n): pc (B,N_max,3), cloud b in its first n[b] rows.  The box is taken over those
    rows only -- cloud b's results are normalize's on the unpadded cloud, bit for bit -- and the rows behind them come out as zeros."""
    pc = _f32c(pc, "normalize_n")
    B, N, _ = pc.shape
    n = counts(n, B, pc.device, "normalize_n.n")
    out = torch.empty_like(pc)
    center = torch.empty(B, 3, device=pc.device, dtype=torch.float32)
    longest = torch.empty(B, device=pc.device, dtype=torch.float32)
    _lib.call("pccx_normalize_n", pc.data_ptr(), B, N, n.data_ptr(), float(margin), out.data_ptr(), center.data_ptr(), longest.data_ptr(),
              _stream())
    return out, center, longest


def denormalize(pc, center, longest, margin=0.01):
    """pn_kit.denormalize (pn_kit.py:62-66), batched."""
    pc = _f32c(pc, "denormalize")
    B, N, _ = pc.shape
    center = _f32c(center.reshape(B, 3), "denormalize.center")
    longest = _f32c(longest.reshape(B), "denormalize.longest")
    out = torch.empty_like(pc)
    _lib.call("pccx_denormalize", pc.data_ptr(), B, N, float(margin), center.data_ptr(), longest.data_ptr(),
              out.data_ptr(), _stream())
    return out


REGION_MAX_S = 8192                       # pccx_region_select: one workgroup scans a cloud's centres (csrc/region.hip)
RegionSelection = collections.namedtuple("RegionSelection", ["patch_idx", "seg_idx", "rows", "counts"])


def check_box(box, halo=0.0):
    """(six floats lo xyz + hi xyz, halo) of a region box ``(lo, hi)``: ValueError naming the argument unless the box is six finite
    floats with lo <= hi on every axis and halo is finite and not negative.  Host only."""
    import math
    try:
        lo, hi = (list(side) for side in box)
        vals = [float(v) for v in lo] + [float(v) for v in hi]
    except (TypeError, ValueError):
        raise ValueError(f"box must be (lo, hi), two triples of floats, got {box!r}") from None
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(v) for v in vals) or any(vals[a] > vals[3 + a] for a in range(3)):
        raise ValueError(f"box must be six finite floats with lo <= hi on every axis, got {box!r}")
    try:
        h = float(halo)
    except (TypeError, ValueError):
        raise ValueError(f"halo must be a finite float >= 0, got {halo!r}") from None
    if not math.isfinite(h) or h < 0:
        raise ValueError(f"halo must be a finite float >= 0, got {halo!r}")
    return vals, h


def region_select(centres, c4, box, G, halo=0.0, margin=0.01, counts=None):
    """pccx_region_select: the patches of ONE cloud whose denormalised centre (ops.denormalize's float) lies in the closed box
    ``(lo, hi)`` grown by ``halo``, and the segments of G patches that hold one.  centres (S,3) decoded centres, c4 (4,) the cloud's
    centre xyz + longest side.  -> RegionSelection of device tensors, never read back here: patch_idx (S) i64 and seg_idx
    (ceil(S/G)) i32, ascending, of which the first counts[0] / counts[1] are valid; rows (S) i64, each selected patch's row among
    the touched segments' patches; counts (2) i32 (``counts``: a dense int32 device tensor of two entries to write instead)."""
    import ctypes
    vals, h = check_box(box, halo)
    x = _f32c(centres, "region_select")
    S = x.shape[0]
    if x.dim() != 2 or x.shape[1] != 3 or not 1 <= S <= REGION_MAX_S:
        raise ValueError(f"region_select: centres must be (S,3) with 1 <= S <= {REGION_MAX_S}, got {tuple(x.shape)}")
    G = int(G)
    if G < 1:
        raise ValueError(f"region_select: G must be >= 1, got {G}")
    c4 = _f32c(c4.reshape(4), "region_select.c4")
    if counts is None:
        counts = torch.empty(2, device=x.device, dtype=torch.int32)
    if counts.dtype != torch.int32 or tuple(counts.shape) != (2,) or not counts.is_contiguous() or counts.device != x.device:
        raise ValueError("region_select: counts must be a dense (2,) int32 tensor on the centres' device")
    sel = RegionSelection(torch.empty(S, device=x.device, dtype=torch.int64), torch.empty(-(-S // G), device=x.device, dtype=torch.int32),
                          torch.empty(S, device=x.device, dtype=torch.int64), counts)
    box_c = (ctypes.c_float * 6)(*vals)
    _lib.call("pccx_region_select", x.data_ptr(), S, c4.data_ptr(), float(margin), ctypes.addressof(box_c), h, G,
              sel.patch_idx.data_ptr(), sel.seg_idx.data_ptr(), sel.rows.data_ptr(), sel.counts.data_ptr(), _stream())
    return sel


FPS_COOP_POINTS_PER_WORKGROUP = 16384    # 1024 threads x 16 points in registers (csrc/geometry.hip, fps_coop_kernel)
FPS_COOP_MAX_WORKGROUPS = 64              # per cloud: the flat barrier of pccx_fps_coop is sized for that many arrivals
FPS_COOP_SPREAD = 2                       # "auto" aims at this many times the least G, i.e. 8 points per thread


def fps_coop_workgroups(N, B, n_cus):
    """Workgroups per cloud G that "auto" hands to pccx_fps_coop for B clouds of N points on a device of n_cus compute units.
    Never below ceil(N / 16384) (a thread holds at most 16 points) nor above 64 or n_cus; FPS_COOP_SPREAD times the least G
    where the whole batch is then resident at once (B * G <= n_cus), less -- down to the least G -- where that keeps it resident.
    A batch that does not fit even at the least G is run in sub-batches of n_cus // G clouds by the caller."""
    N, B, n_cus = int(N), int(B), int(n_cus)
    if N < 1 or B < 0 or n_cus < 1:
        raise ValueError(f"fps_coop_workgroups: need N >= 1, B >= 0, n_cus >= 1, got N={N} B={B} n_cus={n_cus}")
    least = -(-N // FPS_COOP_POINTS_PER_WORKGROUP)
    most = min(FPS_COOP_MAX_WORKGROUPS, n_cus)
    if least > most:
        raise ValueError(f"fps_coop_workgroups: a cloud of {N} points needs {least} workgroups of {FPS_COOP_POINTS_PER_WORKGROUP} points; "
                         f"at most {most} can share a cloud on {n_cus} compute units")
    G = min(FPS_COOP_SPREAD * least, most)
    if B * G > n_cus:
        G = max(least, min(G, n_cus // max(B, 1)))
    return G


def fps_auto_workgroups(N, npoint, B, n_cus):
    """What workgroups="auto" does: G for pccx_fps_coop, or None for pccx_fps.  Cooperative wherever npoint > 1024 (a whole room: the
    single workgroup would take seconds), and for N > 16384 -- where pccx_fps keeps its running minima in global memory -- when the whole
    batch is resident in one launch: measured 4.3x to 8.3x faster at 65536 and 131072 points, B = 1, in each of three alternating rounds
    (DESIGN.md 4.5).  Up to 16384 points pccx_fps holds the cloud in registers on one CU and stays."""
    if B < 1 or npoint < 1:
        return None
    if npoint > 1024:
        return fps_coop_workgroups(N, B, n_cus)
    if N > FPS_COOP_POINTS_PER_WORKGROUP and -(-N // FPS_COOP_POINTS_PER_WORKGROUP) <= min(FPS_COOP_MAX_WORKGROUPS, n_cus):
        G = fps_coop_workgroups(N, B, n_cus)
        return G if B * G <= n_cus else None
    return None


def _n_cus(device):
    return int(torch.cuda.get_device_properties(device).multi_processor_count)


def _fps_coop(xyz, npoint, start, out, G, workspace):
    """pccx_fps_coop over sub-batches of n_cus // G clouds; raises when a cloud's status word reports an expired barrier wait."""
    B, N, _ = xyz.shape
    lib = _lib.load()
    G = int(G)
    per = max(1, _n_cus(xyz.device) // max(G, 1))            # clouds per launch: B * G workgroups must all be resident (the entry checks G itself)
    need = int(lib.pccx_fps_coop_workspace_bytes(B, int(npoint)))
    if workspace is None:
        workspace = torch.empty(max(need, 16), device=xyz.device, dtype=torch.uint8)
    elif (not isinstance(workspace, torch.Tensor) or workspace.device != xyz.device or workspace.dtype != torch.uint8 or not workspace.is_contiguous()
          or workspace.numel() < need or workspace.data_ptr() % 16):
        raise _lib.PccxError(f"farthest_point_sample_batch: workspace must be a dense 16-byte aligned uint8 tensor of at least {need} bytes on {xyz.device}")
    row = (int(npoint) + 2) * 8
    for b0 in range(0, B, per):
        nb = min(per, B - b0)
        _lib.call("pccx_fps_coop", xyz[b0:].data_ptr(), nb, N, int(npoint), start[b0:].data_ptr() if start is not None else None,
                  out[b0:].data_ptr(), G, workspace[b0 * row:].data_ptr(), _stream())
    if B and npoint:
        status = workspace[:B * row].view(torch.int64).view(B, int(npoint) + 2)[:, 1]
        bad = torch.nonzero(status).flatten().tolist()            # the one read-back of this path (it is eager, never captured)
        if bad:
            raise _lib.PccxError(f"pccx_fps_coop: the workgroups of clouds {bad} gave up a barrier wait that outlasted its bound; their indices are incomplete")
    return out


def farthest_point_sample_batch(xyz, npoint, start_idx=None, workgroups=None, workspace=None):
    """pn_kit.farthest_point_sample_batch (pn_kit.py:309-330).  ``start_idx`` (B,) replaces the
    reference's torch.randint draw (:321); None draws it the same way the reference does.
    workgroups: None = pccx_fps, one workgroup per cloud; an int G = pccx_fps_coop with G workgroups per cloud (the same indices, bit
    for bit; ceil(N / 16384) <= G <= 64; a batch with B * G above the device's compute units runs in sub-batches); "auto" =
    fps_auto_workgroups' choice: the cooperative form where npoint > 1024 and for resident batches above 16384 points.  workspace: for the cooperative
    form, a uint8 tensor of pccx_fps_coop_workspace_bytes(B, npoint) to use instead of a fresh one (the entry clears it itself)."""
    xyz = _f32c(xyz, "farthest_point_sample_batch")
    B, N, _ = xyz.shape
    if isinstance(workgroups, str):
        if workgroups != "auto":
            raise ValueError(f"farthest_point_sample_batch: workgroups must be None, 'auto' or an int, got {workgroups!r}")
        workgroups = fps_auto_workgroups(N, int(npoint), B, _n_cus(xyz.device))
    if start_idx is None:
        start_idx = torch.randint(0, N, (B,), dtype=torch.long)
    # start_idx == "zero": every cloud starts from its point 0 (pytorch3d's sample_farthest_points); the kernel takes a null table for
    # that, so nothing is uploaded (a pageable upload blocks the calling thread behind everything queued on its stream)
    start = None if isinstance(start_idx, str) and start_idx == "zero" else torch.as_tensor(start_idx).to(device=xyz.device, dtype=torch.int32).contiguous()
    out = torch.empty(B, npoint, device=xyz.device, dtype=torch.int64)
    if workgroups is not None:
        return _fps_coop(xyz, npoint, start, out, workgroups, workspace)
    work = torch.empty(B * N, device=xyz.device, dtype=torch.float32) if N > 16384 else None
    _lib.call("pccx_fps", xyz.data_ptr(), B, N, int(npoint), start.data_ptr() if start is not None else None, out.data_ptr(),
              work.data_ptr() if work is not None else None, _stream())
    return out


def farthest_point_sample_n(xyz, n, npoint_max, npoint, start_idx=None):
    """farthest_point_sample_batch for a ragged batch (pccx_fps_n): cloud b samples npoint[b] <= npoint_max of its first n[b] points
    -> (B, npoint_max) int64, the indices of farthest_point_sample_batch on the unpadded cloud and then the last of them repeated
    (a gather over the whole row reads real points).  N_max <= KNN_BRUTE_MAX_N = 32768.  start_idx: (B,) or "zero"."""
    xyz = _f32c(xyz, "farthest_point_sample_n")
    B, N, _ = xyz.shape
    n, npoint = counts(n, B, xyz.device, "farthest_point_sample_n.n"), counts(npoint, B, xyz.device, "farthest_point_sample_n.npoint")
    start = None if start_idx is None or (isinstance(start_idx, str) and start_idx == "zero") else counts(start_idx, B, xyz.device, "farthest_point_sample_n.start_idx")
    out = torch.empty(B, int(npoint_max), device=xyz.device, dtype=torch.int64)
    work = torch.empty(B * N, device=xyz.device, dtype=torch.float32) if N > 16384 else None
    _lib.call("pccx_fps_n", xyz.data_ptr(), B, N, n.data_ptr(), int(npoint_max), npoint.data_ptr(), start.data_ptr() if start is not None else None,
              out.data_ptr(), work.data_ptr() if work is not None else None, _stream())
    return out


FPS_BLOCK_MIN, FPS_BLOCK_MAX = 1024, 16384   # points per block of pccx_fps_blocks: one workgroup's registers hold at most 1024 x 16


def check_fps_block(block):
    """``block`` as an int in 1024..16384 points per block, or a ValueError naming fps_block.  Host only."""
    if isinstance(block, bool) or not isinstance(block, int) or not FPS_BLOCK_MIN <= block <= FPS_BLOCK_MAX:
        raise ValueError(f"fps_block must be an int in {FPS_BLOCK_MIN}..{FPS_BLOCK_MAX} points per block, got {block!r}")
    return block


def fps_block_plan(N, npoint, block):
    """How farthest_point_sample_blocks cuts a cloud of N points with npoint centres: (P, lo, o) with P = ceil(N / block) blocks,
    lo[j] = floor(j*N/P) the first sorted position of block j and o[j] = floor(j*npoint/P) its first output slot (P + 1 entries each,
    ending at N and npoint), the arithmetic of pccx_fps_blocks.  Host only.  ``block`` is an int in 1024..16384; anything else, or a
    shape the kernel refuses (a block without a centre, or asked for more centres than it has points), is a ValueError."""
    check_fps_block(block)
    N, npoint = int(N), int(npoint)
    if N < 1 or npoint < 0:
        raise ValueError(f"fps_block_plan: need N >= 1 and npoint >= 0, got N={N} npoint={npoint}")
    P = -(-N // block)
    if P > 1 and (npoint // P < 1 or -(-npoint // P) > N // P):
        raise ValueError(f"fps_block_plan: {npoint} centres over {P} blocks of {N // P} points: every block needs at least one centre "
                         f"and at most as many as it has points")
    return P, [j * N // P for j in range(P + 1)], [j * npoint // P for j in range(P + 1)]


def farthest_point_sample_blocks(xyz, npoint, start_idx=None, block=8192, order=None):
    """Block-parallel centre selection (pccx_fps_blocks): the cloud is cut into P = ceil(N / block) runs of its Morton order
    (fps_block_plan) and every run picks its share of the npoint centres by a farthest point sampling of its own, all runs side by
    side in one launch -> (B, npoint) int64 indices into xyz.  These are NOT farthest_point_sample_batch's indices unless P == 1,
    where that function is called and nothing is sorted.  A run starts at its local point start_idx[b] mod (points of the run).
    order: (B,N) int64, each row a permutation of 0..N-1, instead of large.morton_orders of the clouds."""
    xyz = _f32c(xyz, "farthest_point_sample_blocks")
    B, N, _ = xyz.shape
    P = fps_block_plan(N, npoint, block)[0]
    if P == 1:
        return farthest_point_sample_batch(xyz, npoint, start_idx)
    if start_idx is None:
        start_idx = torch.randint(0, N, (B,), dtype=torch.long)
    start = None if isinstance(start_idx, str) and start_idx == "zero" else torch.as_tensor(start_idx).to(device=xyz.device, dtype=torch.int32).contiguous()
    if order is None:
        from . import large
        rows = large.morton_orders(list(xyz.unbind(0)))
        order = rows[0].view(1, N) if B == 1 else torch.stack(rows)
    order = _dev(order, "farthest_point_sample_blocks.order")
    if order.dtype != torch.int64 or tuple(order.shape) != (B, N) or order.device != xyz.device:
        raise ValueError(f"farthest_point_sample_blocks: order must be a ({B}, {N}) int64 tensor on {xyz.device}, got {tuple(order.shape)} {order.dtype}")
    order = order.contiguous()
    out = torch.empty(B, npoint, device=xyz.device, dtype=torch.int64)
    _lib.call("pccx_fps_blocks", xyz.data_ptr(), B, N, order.data_ptr(), P, int(npoint), start.data_ptr() if start is not None else None,
              out.data_ptr(), _stream())
    return out


def sample_farthest_points(xyz, K):
    """pytorch3d.ops.sample_farthest_points as pointnet_sa_module.py:12 uses it: start index 0,
    returns (points, idx)."""
    idx = farthest_point_sample_batch(xyz, K, start_idx="zero")
    return index_points(xyz, idx), idx


def index_points(points, idx):
    """pn_kit.index_points (pn_kit.py:332-360): idx (B,S) or (B,S,K)."""
    points = _f32c(points, "index_points")
    B, N, Cc = points.shape
    idx = _dev(idx, "index_points.idx").to(torch.int64).contiguous()
    M = idx[0].numel()
    out = torch.empty(B, M, Cc, device=points.device, dtype=torch.float32)
    _lib.call("pccx_gather", points.data_ptr(), B, N, Cc, idx.data_ptr(), M, out.data_ptr(), _stream())
    return out.view(*idx.shape, Cc)


def knn_gather(x, idx):
    """pytorch3d.ops.knn_gather(x (B,N,C), idx (B,M,K)) -> (B,M,K,C)."""
    return index_points(x, idx)


PATCH_GROUPS_MAX_S = 1024          # pccx_patch_groups, pccx_octree_encode and the narrow full decode; above it the *_wide forms, to 8192
WIDE_MAX_S = 8192


def patch_groups(keys_a, keys_b=None, wide=False):
    """Which patches of a batch repeat an earlier patch of their own cloud (csrc/patch_groups.hip).  keys_a (B,S,fa) f32 and optionally
    keys_b (B,S,fb) f32: the key row of patch (b, i) is the fa + fb words of the two rows, compared bit for bit.  In octree_mode
    "reference" the decoded centres take at most 8 distinct values per cloud (octree_np.py:47-112 consumes one byte of the stream), so
    the transforms run on about an eighth of the patches and the results are copied (replicate_rows).  Returns Groups, all on the device.
    S > 1024 (to 8192), or wide=True at any S, takes pccx_patch_groups_wide: the same tables through a hash table in LDS."""
    a = _f32c(keys_a, "patch_groups.keys_a")
    B, S, fa = a.shape
    b = _f32c(keys_b.reshape(B, S, -1), "patch_groups.keys_b") if keys_b is not None else None
    buf = torch.empty(2 * B * S + 1 + _lib.load().pccx_patch_groups_workspace_ints(B), device=a.device, dtype=torch.int32)
    g = Groups(buf[:B * S], buf[B * S:2 * B * S], buf[2 * B * S:2 * B * S + 1])
    with stage("patch_groups"):
        _lib.call("pccx_patch_groups_wide" if wide or S > PATCH_GROUPS_MAX_S else "pccx_patch_groups", a.data_ptr(), fa, b.data_ptr() if b is not None else None, b.shape[2] if b is not None else 0, B, S,
                  g.rep.data_ptr(), g.uniq.data_ptr(), g.n_uniq.data_ptr(), buf[2 * B * S + 1:].data_ptr(), _stream())
    return g


def replicate_rows(groups, *arrays):
    """Rows of the duplicates := rows of their representatives, in place, in up to three dense f32 arrays of P rows each (same row width)."""
    P = groups.rep.numel()
    if not arrays or len(arrays) > 3 or any(t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != arrays[0].numel() or t.numel() % max(P, 1)
                                            for t in arrays):
        raise _lib.PccxError("replicate_rows: one to three dense float32 arrays of P rows each, all of one row width, are expected")
    ptrs = [t.data_ptr() for t in arrays] + [None] * (3 - len(arrays))
    with stage("replicate"):
        _lib.call("pccx_replicate_rows", groups.rep.data_ptr(), P, arrays[0].numel() // max(P, 1), *ptrs, _stream())


def knn_points(p1, p2, K, return_nn=True, patch_scale=0.0, return_dists=True, return_idx=True, rep=None, groups=None, search=None, index=None):
    """pytorch3d.ops.knn_points (compress.py:71, pn_kit.py:190).  With patch_scale != 0 the third
    field holds (nn - p1) * patch_scale, i.e. compress.py:72 and :108 fused.  return_dists / return_idx = False leave that field None
    and its bytes unwritten (KNN_Patching, compress.py:70-74, keeps the gathered points only).
    rep: Groups.rep over the (B, M) queries -- only the representatives are searched, the rows of the other queries stay unwritten.
    groups: the Groups themselves -- the same, with the workgroups walking groups.uniq instead of one being launched per query.
    search="grid": the same results through a GridIndex of p2 (``index``: one the caller already built over p2), which has no limit
    on p2's size where the all-pairs kernels stop at 32768 points; groups= then counts as its rep table."""
    if _search(search, "knn_points"):
        return _knn_points_grid(p1, p2, int(K), return_nn, patch_scale, return_dists, return_idx, rep, groups, index)
    p1, p2 = _f32c(p1, "knn_points.p1"), _f32c(p2, "knn_points.p2")
    B, M, _ = p1.shape
    N = p2.shape[1]
    dists = torch.empty(B, M, K, device=p1.device, dtype=torch.float32) if return_dists else None
    idx = torch.empty(B, M, K, device=p1.device, dtype=torch.int64) if return_idx else None
    nn = torch.empty(B, M, K, 3, device=p1.device, dtype=torch.float32) if return_nn else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    if rep is not None and (rep.dtype != torch.int32 or rep.numel() != B * M or not rep.is_cuda or not rep.is_contiguous()):
        raise _lib.PccxError("knn_points: rep must be the dense int32 (B*M) table of patch_groups over the queries")
    if groups is not None:
        if rep is not None or groups.rep.numel() != B * M:
            raise _lib.PccxError("knn_points: groups must be the patch_groups of the (B, M) queries, given without rep")
        if _lib.load().pccx_knn_uniq_ok(N, int(K)):
            _lib.call("pccx_knn_uniq", p1.data_ptr(), B, M, p2.data_ptr(), N, int(K), ptr(dists), ptr(idx), ptr(nn), float(patch_scale),
                      groups.uniq.data_ptr(), groups.n_uniq.data_ptr(), _stream())
            return KNN(dists, idx, nn)
        rep = groups.rep                       # the radix-select kernel of the larger shapes skips by the table
    _lib.call("pccx_knn_list", p1.data_ptr(), B, M, p2.data_ptr(), N, int(K), ptr(dists), ptr(idx), ptr(nn), float(patch_scale), ptr(rep), _stream())
    return KNN(dists, idx, nn)


def knn_points_n(p1, p2, n, K, scale, rep=None, return_dists=False, return_idx=False, return_nn=True):
    """knn_points for a ragged batch (pccx_knn_list_n), the all-pairs search: the keys of cloud b are the first n[b] >= K rows of
    p2 (B,N_max,3), and its third field holds (nn - p1) * scale[b] (scale: (B,) f32 on the device, none of them 0 unless the points
    themselves are wanted).  rep as knn_points.  Cloud b's rows are knn_points' on the unpadded cloud, bit for bit."""
    p1, p2 = _f32c(p1, "knn_points_n.p1"), _f32c(p2, "knn_points_n.p2")
    B, M, _ = p1.shape
    N = p2.shape[1]
    n = counts(n, B, p1.device, "knn_points_n.n")
    scale = _f32c(scale, "knn_points_n.scale")
    if tuple(scale.shape) != (B,):
        raise _lib.PccxError(f"knn_points_n: scale must be (B,) float32, got {tuple(scale.shape)}")
    if rep is not None and (rep.dtype != torch.int32 or rep.numel() != B * M or not rep.is_cuda or not rep.is_contiguous()):
        raise _lib.PccxError("knn_points_n: rep must be the dense int32 (B*M) table of patch_groups over the queries")
    dists = torch.empty(B, M, K, device=p1.device, dtype=torch.float32) if return_dists else None
    idx = torch.empty(B, M, K, device=p1.device, dtype=torch.int64) if return_idx else None
    nn = torch.empty(B, M, K, 3, device=p1.device, dtype=torch.float32) if return_nn else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.call("pccx_knn_list_n", p1.data_ptr(), B, M, p2.data_ptr(), N, n.data_ptr(), int(K), ptr(dists), ptr(idx), ptr(nn), scale.data_ptr(),
              ptr(rep), _stream())
    return KNN(dists, idx, nn)


def ball_query(p1, p2, K, radius, method="auto", extent=1.0):
    """pytorch3d.ops.ball_query (pointnet_sa_module.py:18): the first K candidates in index order with d2 < radius2, idx padded
    with -1.  method: "scan" = one wave per query walks the candidates in order and stops at the K-th hit; "grid" = uniform grid
    hash of the candidates (cells of side >= radius), 27-cell walk, index order restored by a bitmap; "auto" takes the grid for
    4096 <= N <= 32768 candidates when the clouds are at least four cells wide, extent / radius >= 4 (``extent`` = the callers'
    bound on a cloud's longest side: 1.0 for this codec's normalised clouds; narrower boxes put most of the cloud in the 27-cell
    walk and the ordered scan with its early exit at the K-th hit is faster -- as on the few-hundred-point sets of PPPF_AE).
    Same results either way."""
    p1, p2 = _f32c(p1, "ball_query.p1"), _f32c(p2, "ball_query.p2")
    B, M, _ = p1.shape
    N = p2.shape[1]
    dists = torch.empty(B, M, K, device=p1.device, dtype=torch.float32)
    idx = torch.empty(B, M, K, device=p1.device, dtype=torch.int64)
    if method == "grid" or (method == "auto" and 4096 <= N <= 32768 and float(extent) >= 4.0 * float(radius)):
        ws = torch.empty(_lib.load().pccx_ball_query_grid_workspace_ints(B, N), device=p1.device, dtype=torch.int32)
        _lib.call("pccx_ball_query_grid", p1.data_ptr(), B, M, p2.data_ptr(), N, int(K), float(radius), ws.data_ptr(),
                  dists.data_ptr(), idx.data_ptr(), _stream())
    else:
        _lib.call("pccx_ball_query", p1.data_ptr(), B, M, p2.data_ptr(), N, int(K), float(radius),
                  dists.data_ptr(), idx.data_ptr(), _stream())
    return KNN(dists, idx, None)


GRID_WIDE_TARGET = None      # points per cell of the index knn_points(search="grid") builds for knn_wide; None = the library's 2


def _search(search, who):
    """search=None / "brute": the all-pairs kernels; "grid": through a GridIndex.  Anything else is an error."""
    if search is None or search == "brute":
        return False
    if search == "grid":
        return True
    raise ValueError(f"{who}: search must be None, 'brute' or 'grid', got {search!r}")


class GridIndex:
    """Exact grid index over the reference clouds y (B,Q,3) (csrc/grid_nn.hip): built once, queried any number of times.  .nn,
    .knn and .knn_wide return what nn_dist and knn_points return for the same clouds, bit for bit (same fp32 distances, ties to the lower index);
    they stand in for open3d's KDTreeFlann.search_knn_vector_3d (eval.py:55-81) at sizes where the all-pairs scans cost P * Q pairs.
    The index keeps its own copy of the points in cell order, so y need not stay alive."""

    def __init__(self, y, target=None):
        """target: points per cell aimed at (>= 2); None = the library's 2, chosen for K <= 32 (pccx_grid_index_build_target)."""
        y = _f32c(y, "GridIndex.y")
        if y.dim() != 3 or y.shape[2] != 3:
            raise _lib.PccxError(f"GridIndex: expected (B,Q,3), got {tuple(y.shape)}")
        self.B, self.Q = int(y.shape[0]), int(y.shape[1])
        self.device = y.device
        self.ws = torch.empty(max(int(_lib.load().pccx_grid_index_workspace_bytes(self.B, self.Q)), 16), device=y.device, dtype=torch.uint8)
        with stage("grid_index"):
            if target is None:
                _lib.call("pccx_grid_index_build", y.data_ptr(), self.B, self.Q, self.ws.data_ptr(), _stream())
            else:
                _lib.call("pccx_grid_index_build_target", y.data_ptr(), self.B, self.Q, int(target), self.ws.data_ptr(), _stream())

    def _queries(self, x, who, workspace=True):
        x = _f32c(x, who)
        if x.dim() != 3 or x.shape[2] != 3 or x.shape[0] != self.B or x.device != self.device:
            raise _lib.PccxError(f"{who}: expected ({self.B},P,3) on {self.device}, got {tuple(x.shape)} on {x.device}")
        if not workspace:
            return x, None
        qws = torch.empty(max(int(_lib.load().pccx_grid_query_workspace_bytes(self.B, int(x.shape[1]))), 16), device=x.device, dtype=torch.uint8)
        return x, qws

    def nn(self, x, return_idx=False):
        """nn_dist(x, y, return_idx) through the index."""
        x, qws = self._queries(x, "GridIndex.nn")
        P = int(x.shape[1])
        d2 = torch.empty(self.B, P, device=x.device, dtype=torch.float32)
        nn = torch.empty(self.B, P, device=x.device, dtype=torch.int32) if return_idx else None
        with stage("grid_nn"):
            _lib.call("pccx_grid_nn", x.data_ptr(), self.B, P, self.Q, self.ws.data_ptr(), qws.data_ptr(), d2.data_ptr(),
                      nn.data_ptr() if nn is not None else None, _stream())
        return (d2, nn) if return_idx else d2

    def knn(self, x, K):
        """knn_points(x, y, K, return_nn=False) through the index, 1 <= K <= min(Q, 32): KNN(dists, idx, None)."""
        x, qws = self._queries(x, "GridIndex.knn")
        M = int(x.shape[1])
        dists = torch.empty(self.B, M, int(K), device=x.device, dtype=torch.float32)
        idx = torch.empty(self.B, M, int(K), device=x.device, dtype=torch.int64)
        with stage("grid_knn"):
            _lib.call("pccx_grid_knn", x.data_ptr(), self.B, M, self.Q, int(K), self.ws.data_ptr(), qws.data_ptr(), dists.data_ptr(),
                      idx.data_ptr(), _stream())
        return KNN(dists, idx, None)

    def knn_wide(self, x, K, return_nn=False, patch_scale=0.0, return_dists=True, return_idx=True, rep=None):
        """knn_points(x, y, K, ...) through the index for K <= min(Q, 1024), the codec's patch search (compress.py:70-74,105-108; K <= 32
        is served too, where .knn is the faster kernel but returns neither the points nor takes rep):
        KNN(dists, idx, knn), each field None unless asked for; with patch_scale != 0 knn holds (y[idx] - x) * patch_scale.  rep:
        Groups.rep over the (B, M) queries -- only the representatives are searched, the rows of the others stay unwritten."""
        x, _ = self._queries(x, "GridIndex.knn_wide", workspace=False)
        M, K = int(x.shape[1]), int(K)
        if rep is not None and (rep.dtype != torch.int32 or rep.numel() != self.B * M or not rep.is_cuda or not rep.is_contiguous()):
            raise _lib.PccxError("GridIndex.knn_wide: rep must be the dense int32 (B*M) table of patch_groups over the queries")
        if not (return_dists or return_idx or return_nn):
            raise _lib.PccxError("GridIndex.knn_wide: at least one of dists / idx / nn must be asked for")
        if not 1 <= K <= min(self.Q, 1024):
            raise _lib.PccxError(f"GridIndex.knn_wide: need 1 <= K <= min(Q,1024), got K={K} Q={self.Q}")
        qws = torch.empty(max(int(_lib.load().pccx_grid_knn_wide_workspace_bytes(self.B, self.Q)), 16), device=x.device, dtype=torch.uint8)
        dists = torch.empty(self.B, M, K, device=x.device, dtype=torch.float32) if return_dists else None
        idx = torch.empty(self.B, M, K, device=x.device, dtype=torch.int64) if return_idx else None
        nn = torch.empty(self.B, M, K, 3, device=x.device, dtype=torch.float32) if return_nn else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        with stage("grid_knn_wide"):
            _lib.call("pccx_grid_knn_wide", x.data_ptr(), self.B, M, self.Q, K, self.ws.data_ptr(), qws.data_ptr(), ptr(dists), ptr(idx),
                      ptr(nn), float(patch_scale), ptr(rep), _stream())
        return KNN(dists, idx, nn)


def _knn_points_grid(p1, p2, K, return_nn, patch_scale, return_dists, return_idx, rep, groups, index):
    """knn_points(search="grid"): GridIndex.knn where it serves the request (K <= 32, dists and idx only, every query), knn_wide otherwise."""
    if groups is not None:
        if rep is not None:
            raise _lib.PccxError("knn_points: groups must be given without rep")
        rep = groups.rep
    narrow = K <= 32 and not return_nn and rep is None
    if index is None:
        index = GridIndex(p2, None if narrow else GRID_WIDE_TARGET)
    if narrow:
        r = index.knn(p1, K)
        return KNN(r.dists if return_dists else None, r.idx if return_idx else None, None)
    return index.knn_wide(p1, K, return_nn=return_nn, patch_scale=patch_scale, return_dists=return_dists, return_idx=return_idx, rep=rep)


def nn_dist(x, y, return_idx=False, search=None):
    """min_j |x_i - y_j|^2 for every i: (B,P,3),(B,Q,3) -> (B,P) [, idx (B,P) int32].  search="grid": through a GridIndex of y
    (y may be that index itself), same results."""
    if _search(search, "nn_dist"):
        return (y if isinstance(y, GridIndex) else GridIndex(y)).nn(x, return_idx)
    x, y = _f32c(x, "nn_dist.x"), _f32c(y, "nn_dist.y")
    B, P, _ = x.shape
    d2 = torch.empty(B, P, device=x.device, dtype=torch.float32)
    nn = torch.empty(B, P, device=x.device, dtype=torch.int32) if return_idx else None
    split = _lib.load().pccx_nn_dist_split_count(B, P, int(y.shape[1])) if B > 0 else 1
    if split > 1:
        # a batch too small to fill the chip (the training step's 4 clouds): the reference cloud in `split` chunks over more workgroups
        sd = torch.empty(split, B, P, device=x.device, dtype=torch.float32)
        sn = torch.empty(split, B, P, device=x.device, dtype=torch.int32) if return_idx else None
        _lib.call("pccx_nn_dist_split", x.data_ptr(), B, P, y.data_ptr(), y.shape[1], split, sd.data_ptr(),
                  sn.data_ptr() if sn is not None else None, d2.data_ptr(), nn.data_ptr() if nn is not None else None, _stream())
        return (d2, nn) if return_idx else d2
    _lib.call("pccx_nn_dist", x.data_ptr(), B, P, y.data_ptr(), y.shape[1], d2.data_ptr(),
              nn.data_ptr() if nn is not None else None, _stream())
    return (d2, nn) if return_idx else d2


def checked_counts(v, B, cap, device, name):
    """pytorch3d's x_lengths / y_lengths as the kernels take them (``counts``).  A host sequence is checked against [1, cap] here,
    before any launch; a device tensor is not read back -- the kernels clamp it into [0, cap] where they read it."""
    if not isinstance(v, torch.Tensor) or not v.is_cuda:
        host = [int(c) for c in (v.tolist() if isinstance(v, torch.Tensor) else v)]
        bad = [(b, c) for b, c in enumerate(host) if not 1 <= c <= cap]
        if bad:
            raise _lib.PccxError(f"{name}: every length must lie in [1, {cap}] (the padded size), got " +
                                 ", ".join(f"{c} for cloud {b}" for b, c in bad[:4]))
        v = host
    return counts(v, B, device, name)


CROP_MAX_M, CROP_MAX_NCAP, CROP_MAX_B = 1 << 24, 131072, 1024       # csrc/crop.hip: points per cloud, points per crop, crops per call


def crop_sizes(offsets, name="crop_nearest.offsets"):
    """The point count of every cloud of a store from its (F+1,) int64 offset table (codec.pack_clouds), on the host -- ONE read-back
    when the table lives on the device: callers that crop every step keep the list (CropSampler does)."""
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2:
        got = f"{tuple(offsets.shape)} {offsets.dtype}" if isinstance(offsets, torch.Tensor) else type(offsets).__name__
        raise _lib.PccxError(f"{name}: an (F+1,) int64 tensor with F >= 1 is expected (codec.pack_clouds), got {got}")
    o = offsets.tolist()
    return [b - a for a, b in zip(o[:-1], o[1:])]


def crop_nearest(points, offsets, cloud, seed, n, N_cap, return_idx=False, workspace=None, sizes=None, out=None, out_idx=None):
    """Nearest-n crops of a store of clouds (pccx_crop_nearest, csrc/crop.hip): points (M_total,3) f32 and offsets (F+1,) int64 as
    codec.pack_clouds makes them; slot b keeps, of cloud cloud[b], the n[b] points with the smallest keys (bits of the squared distance
    to that cloud's point seed[b], index) in ascending index.  -> out (B,N_cap,3), rows behind n[b] NaN [, idx (B,N_cap) int32, -1
    behind n[b]].  cloud / seed / n: host sequences, range-checked here before any launch, or device int32 tensors, taken as they are
    and clamped where the kernels read them (never read back).  sizes: the host list of point counts (pack_clouds' third result); None
    reads it from offsets, one read-back.  workspace: a uint8 device tensor of at least pccx_crop_nearest_workspace_bytes(B,
    max(sizes)) bytes whose content does not matter (default: allocated here).  out / out_idx: buffers of the result's shapes to write
    into (default: allocated here).  With sizes given the call only enqueues kernels on the current stream: it can be captured, and a
    captured call replays on other table contents."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise _lib.PccxError(f"crop_nearest.points: (M_total, 3) with M_total >= 1 is expected, got "
                             f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
    if points.dtype != torch.float32:
        raise _lib.PccxError(f"crop_nearest.points: expected float32, got {points.dtype}")
    sizes = crop_sizes(offsets) if sizes is None else [int(v) for v in sizes]
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or tuple(offsets.shape) != (len(sizes) + 1,):
        raise _lib.PccxError(f"crop_nearest.offsets: an ({len(sizes) + 1},) int64 tensor is expected for {len(sizes)} clouds")
    F, M_total, M_max = len(sizes), int(points.shape[0]), max(sizes)
    if min(sizes) < 1 or sum(sizes) != M_total:
        raise _lib.PccxError(f"crop_nearest: the store holds {M_total} points, its {F} clouds {sum(sizes)} (every cloud needs at least one)")
    if M_max > CROP_MAX_M:
        raise _lib.PccxError(f"crop_nearest: a cloud of {M_max} points; a crop is cut from at most CROP_MAX_M = {CROP_MAX_M} points per cloud")
    N_cap = int(N_cap)
    if not 1 <= N_cap <= CROP_MAX_NCAP:
        raise _lib.PccxError(f"crop_nearest: N_cap={N_cap}; a crop holds 1..CROP_MAX_NCAP = {CROP_MAX_NCAP} points")
    B = int(cloud.shape[0]) if isinstance(cloud, torch.Tensor) and cloud.dim() == 1 else len(cloud)
    if not 1 <= B <= CROP_MAX_B:
        raise _lib.PccxError(f"crop_nearest: {B} crops; one call cuts 1..CROP_MAX_B = {CROP_MAX_B}")
    host = [None if isinstance(v, torch.Tensor) and v.is_cuda else [int(x) for x in (v.tolist() if isinstance(v, torch.Tensor) else v)]
            for v in (cloud, seed, n)]
    for name, v in zip(("cloud", "seed", "n"), host):
        if v is not None and len(v) != B:
            raise _lib.PccxError(f"crop_nearest.{name}: one int per crop is expected, got {len(v)} for {B} crops")
    if host[0] is not None:
        bad = [(b, c) for b, c in enumerate(host[0]) if not 0 <= c < F]
        if bad:
            raise _lib.PccxError(f"crop_nearest.cloud: every cloud index must lie in [0, {F - 1}], got " + ", ".join(f"{c} for crop {b}" for b, c in bad[:4]))
    m_of = [sizes[c] for c in host[0]] if host[0] is not None else [M_max] * B        # device cloud table: the loosest bound
    if host[1] is not None:
        bad = [(b, s) for b, s in enumerate(host[1]) if not 0 <= s < m_of[b]]
        if bad:
            raise _lib.PccxError("crop_nearest.seed: a seed index must lie inside its cloud, got " +
                                 ", ".join(f"{s} for crop {b} (cloud of {m_of[b]} points)" for b, s in bad[:4]))
    if host[2] is not None:
        bad = [(b, v) for b, v in enumerate(host[2]) if not 1 <= v <= min(N_cap, m_of[b])]
        if bad:
            raise _lib.PccxError("crop_nearest.n: every count must lie in [1, min(N_cap, its cloud's size)], got " +
                                 ", ".join(f"{v} for crop {b} (N_cap={N_cap}, cloud of {m_of[b]} points)" for b, v in bad[:4]))
    points = _f32c(points, "crop_nearest.points")
    dev = points.device
    if not offsets.is_cuda:
        raise _lib.PccxError("crop_nearest.offsets: expected a tensor on the GPU (pccx has no CPU fallback)")
    offsets = offsets.contiguous()
    cloud_t = counts(cloud if host[0] is None else host[0], B, dev, "crop_nearest.cloud")
    seed_t = counts(seed if host[1] is None else host[1], B, dev, "crop_nearest.seed")
    n_t = counts(n, B, dev, "crop_nearest.n") if host[2] is None else checked_counts(host[2], B, N_cap, dev, "crop_nearest.n")
    need = int(_lib.load().pccx_crop_nearest_workspace_bytes(B, M_max))
    if workspace is None:
        workspace = torch.empty(need, device=dev, dtype=torch.uint8)
    elif (not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous()
          or workspace.numel() < need or workspace.data_ptr() % 8):
        raise _lib.PccxError(f"crop_nearest.workspace: a contiguous, 8-byte aligned uint8 device tensor of at least {need} bytes is expected")
    for name, t, shape, dtype in (("out", out, (B, N_cap, 3), torch.float32), ("out_idx", out_idx, (B, N_cap), torch.int32)):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
            raise _lib.PccxError(f"crop_nearest.{name}: a contiguous {shape} {dtype} device tensor is expected")
    out = torch.empty(B, N_cap, 3, device=dev, dtype=torch.float32) if out is None else out
    idx = out_idx if out_idx is not None else torch.empty(B, N_cap, device=dev, dtype=torch.int32) if return_idx else None
    _lib.call("pccx_crop_nearest", points.data_ptr(), M_total, offsets.data_ptr(), F, cloud_t.data_ptr(), seed_t.data_ptr(), n_t.data_ptr(),
              B, N_cap, M_max, out.data_ptr(), idx.data_ptr() if idx is not None else None, workspace.data_ptr(), _stream())
    return (out, idx) if return_idx or out_idx is not None else out


def nn_dist_n(x, y, x_lengths, y_lengths, return_idx=False):
    """nn_dist over a ragged batch (pccx_nn_dist_n): x (B,P_max,3), y (B,Q_max,3), cloud b in its first x_lengths[b] / y_lengths[b]
    rows; what lies behind them is never read (pad_clouds' NaN).  d2 (B,P_max) [, idx (B,P_max) int32]: the first x_lengths[b] entries
    of cloud b are nn_dist's on the unpadded pair, bit for bit; the entries behind them are left unwritten."""
    x, y = _f32c(x, "nn_dist_n.x"), _f32c(y, "nn_dist_n.y")
    B, P, _ = x.shape
    Q = int(y.shape[1])
    p, q = checked_counts(x_lengths, B, P, x.device, "nn_dist_n.x_lengths"), checked_counts(y_lengths, B, Q, x.device, "nn_dist_n.y_lengths")
    d2 = torch.empty(B, P, device=x.device, dtype=torch.float32)
    nn = torch.empty(B, P, device=x.device, dtype=torch.int32) if return_idx else None
    _lib.call("pccx_nn_dist_n", x.data_ptr(), B, P, p.data_ptr(), y.data_ptr(), Q, q.data_ptr(), d2.data_ptr(),
              nn.data_ptr() if nn is not None else None, _stream())
    return (d2, nn) if return_idx else d2


def estimate_normals(xyz, knn=30, search=None, index=None):
    """open3d estimate_normals(KDTreeSearchParamKNN(knn)) (eval.py:59-60): unoriented PCA normals (B,N,3).  search="grid": the
    neighbours come from a GridIndex of xyz (``index``: one the caller already built over xyz), same normals."""
    grid = _search(search, "estimate_normals")
    xyz = _f32c(xyz, "estimate_normals")
    B, N, _ = xyz.shape
    if grid:
        idx = (index if index is not None else GridIndex(xyz)).knn(xyz, min(knn, N)).idx
    else:
        idx = knn_points(xyz, xyz, min(knn, N), return_nn=False).idx
    out = torch.empty(B, N, 3, device=xyz.device, dtype=torch.float32)
    _lib.call("pccx_estimate_normals", xyz.data_ptr(), B, N, idx.data_ptr(), idx.shape[2], out.data_ptr(), _stream())
    return out


def point_plane_err(x, y, normals_y, search=None, index=None):
    """Squared projection of (x - nearest y) on that y's normal, eval.py:79-81: (B,P).  search="grid": the nearest y through a
    GridIndex of y (``index``: one already built), same values."""
    grid = _search(search, "point_plane_err")
    x, y, normals_y = _f32c(x, "point_plane_err.x"), _f32c(y, "point_plane_err.y"), _f32c(normals_y, "point_plane_err.n")
    B, P, _ = x.shape
    _, nn = (index if index is not None else GridIndex(y)).nn(x, return_idx=True) if grid else nn_dist(x, y, return_idx=True)
    err = torch.empty(B, P, device=x.device, dtype=torch.float32)
    _lib.call("pccx_point_plane_err", x.data_ptr(), B, P, y.data_ptr(), normals_y.data_ptr(), y.shape[1], nn.data_ptr(),
              err.data_ptr(), _stream())
    return err


def _slab_shape(t, name, last=3):
    """(B, rows) of a padded slab (B,rows,3) -- or (B,rows) with last=None -- read before anything else, so that a wrapper can check its
    host counts first and touch the device after."""
    want = 3 if last else 2
    if not isinstance(t, torch.Tensor) or t.dim() != want or (last and t.shape[2] != last) or t.shape[1] < 1:
        raise _lib.PccxError(f"{name}: a padded slab (B, rows{', 3' if last else ''}) with at least one row is expected, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    return int(t.shape[0]), int(t.shape[1])


def minmax_n(x, n):
    """Per-axis bounding box of a ragged batch (pccx_minmax_n): x (B,P_max,3), cloud b in its first n[b] rows -> (B,2,3) f32, row 0 the
    minima and row 1 the maxima: amin / amax of the unpadded cloud, bit for bit.  n as checked_counts takes it."""
    B, P = _slab_shape(x, "minmax_n")
    n = checked_counts(n, B, P, x.device, "minmax_n.n")
    x = _f32c(x, "minmax_n")
    out = torch.empty(B, 2, 3, device=x.device, dtype=torch.float32)
    _lib.call("pccx_minmax_n", x.data_ptr(), B, P, n.data_ptr(), out.data_ptr(), _stream())
    return out


def query_rep_n(n, B, M, device):
    """The rep table that makes knn_points_n skip the padded queries of a slab (pccx_query_rep_n): (B*M,) int32, rep[b*M+i] = b*M+i for
    i < n[b], else b*M.  n: (B,) int32 on the device."""
    n = counts(n, B, device, "query_rep_n.n")
    rep = torch.empty(B * M, device=device, dtype=torch.int32)
    _lib.call("pccx_query_rep_n", n.data_ptr(), B, M, rep.data_ptr(), _stream())
    return rep


def estimate_normals_n(xyz, n, knn=30):
    """estimate_normals over a ragged batch: xyz (B,N_max,3), cloud b in its first n[b] >= knn rows -> normals (B,N_max,3) whose first
    n[b] rows are estimate_normals' on the unpadded cloud, bit for bit; the rows behind them are left unwritten.  The 30-NN comes from
    knn_points_n with the padded queries skipped (query_rep_n), the PCA from pccx_estimate_normals_n.  A host n is checked against
    [knn, N_max] before any launch; a device tensor is taken as it is."""
    B, N = _slab_shape(xyz, "estimate_normals_n")
    knn = int(knn)
    if not 1 <= knn <= N:
        raise _lib.PccxError(f"estimate_normals_n: knn={knn} neighbours in a slab of {N} rows")
    if not isinstance(n, torch.Tensor) or not n.is_cuda:
        host = [int(c) for c in (n.tolist() if isinstance(n, torch.Tensor) else n)]
        bad = [(b, c) for b, c in enumerate(host) if c < knn]
        if bad:
            raise _lib.PccxError(f"estimate_normals_n.n: every cloud needs at least knn = {knn} points, got " +
                                 ", ".join(f"{c} for cloud {b}" for b, c in bad[:4]))
        n = host
    n = checked_counts(n, B, N, xyz.device, "estimate_normals_n.n")
    xyz = _f32c(xyz, "estimate_normals_n")
    idx = knn_points_n(xyz, xyz, n, knn, torch.zeros(B, device=xyz.device, dtype=torch.float32), rep=query_rep_n(n, B, N, xyz.device),
                       return_idx=True, return_nn=False).idx
    out = torch.empty(B, N, 3, device=xyz.device, dtype=torch.float32)
    _lib.call("pccx_estimate_normals_n", xyz.data_ptr(), B, N, n.data_ptr(), idx.data_ptr(), knn, out.data_ptr(), _stream())
    return out


def point_errors_n(x, y, x_lengths, y_lengths, normals_y=None):
    """D1 and D2 errors of a ragged batch from ONE all-pairs scan (pccx_point_errors_n): x (B,P_max,3), y (B,Q_max,3), normals_y
    (B,Q_max,3) or None -> d2 (B,P_max) = nn_dist_n's values [, plane (B,P_max) = point_plane_err's values for the same nearest
    neighbour].  The first x_lengths[b] entries of cloud b are those of nn_dist / point_plane_err on the unpadded pair, bit for bit; the
    entries behind them are left unwritten.  Without normals_y only d2 is returned."""
    (B, P), (By, Q) = _slab_shape(x, "point_errors_n.x"), _slab_shape(y, "point_errors_n.y")
    if By != B or (normals_y is not None and (not isinstance(normals_y, torch.Tensor) or tuple(normals_y.shape) != tuple(y.shape))):
        raise _lib.PccxError(f"point_errors_n: y (and normals_y, one normal per row of y) must hold {B} clouds, got {tuple(y.shape)}" +
                             (f" and {tuple(normals_y.shape)}" if isinstance(normals_y, torch.Tensor) else ""))
    p, q = checked_counts(x_lengths, B, P, x.device, "point_errors_n.x_lengths"), checked_counts(y_lengths, B, Q, x.device, "point_errors_n.y_lengths")
    x, y = _f32c(x, "point_errors_n.x"), _f32c(y, "point_errors_n.y")
    normals_y = _f32c(normals_y, "point_errors_n.normals_y") if normals_y is not None else None
    d2 = torch.empty(B, P, device=x.device, dtype=torch.float32)
    plane = torch.empty(B, P, device=x.device, dtype=torch.float32) if normals_y is not None else None
    _lib.call("pccx_point_errors_n", x.data_ptr(), B, P, p.data_ptr(), y.data_ptr(), normals_y.data_ptr() if normals_y is not None else None,
              Q, q.data_ptr(), d2.data_ptr(), plane.data_ptr() if plane is not None else None, _stream())
    return (d2, plane) if plane is not None else d2


def mean_var_n(v, n):
    """Mean and population variance of the first n[b] entries of every row of v (B,P_max) f32 (pccx_mean_var_n) -> (B,2) f64.  Two
    passes in double in an order fixed by n[b] alone: a cloud's two numbers do not depend on the batch around it."""
    B, P = _slab_shape(v, "mean_var_n", last=None)
    n = checked_counts(n, B, P, v.device, "mean_var_n.n")
    v = _f32c(v, "mean_var_n")
    out = torch.empty(B, 2, device=v.device, dtype=torch.float64)
    _lib.call("pccx_mean_var_n", v.data_ptr(), B, P, n.data_ptr(), out.data_ptr(), _stream())
    return out


zeros_hook = None       # pccx.train installs its arena's allocator here: (shape, dtype, device) -> (zero tensor, from-arena?)
deterministic_hook = None    # pccx.train: () -> True while a deterministic step runs (train.step_scope(deterministic=True))


def chamfer_grad_det(x, y, nxy, nyx, gd):
    """The Chamfer gradient with its nearest-neighbour scatter in ascending source order (pccx_chamfer_grad_det): gx, gy WRITTEN into
    plain memory; gd = the upstream gradient, one float32 on the device."""
    lib = _lib.load()
    B, P, Q = x.shape[0], x.shape[1], y.shape[1]
    gx, gy = torch.empty_like(x), torch.empty_like(y)
    wf = torch.empty(max(int(lib.pccx_chamfer_grad_det_workspace_floats(B, P, Q)), 1), device=x.device, dtype=torch.float32)
    wi = torch.empty(max(int(lib.pccx_chamfer_grad_det_workspace_ints(B, P, Q)), 1), device=x.device, dtype=torch.int32)
    _lib.call("pccx_chamfer_grad_det", x.data_ptr(), B, P, y.data_ptr(), Q, nxy.data_ptr(), nyx.data_ptr(), gd.data_ptr(), gx.data_ptr(),
              gy.data_ptr(), wf.data_ptr(), wi.data_ptr(), _stream())
    return gx, gy


class _ChamferFn(torch.autograd.Function):
    """Differentiable chamfer_distance (batch mean): forward = two nn_dist launches, backward =
    pccx_chamfer_grad with the argmins saved from the forward."""

    @staticmethod
    def forward(ctx, x, y):
        dxy, nxy = nn_dist(x, y, return_idx=True)
        dyx, nyx = nn_dist(y, x, return_idx=True)
        ctx.save_for_backward(x, y, nxy, nyx)
        ctx.det = bool(deterministic_hook()) if deterministic_hook is not None else False
        out = torch.empty((), device=x.device, dtype=torch.float32)
        _lib.call("pccx_chamfer_mean", dxy.data_ptr(), dyx.data_ptr(), x.shape[0], x.shape[1], y.shape[1], out.data_ptr(), _stream())
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, nxy, nyx = ctx.saved_tensors
        gd = g.detach().to(torch.float32).reshape(1).contiguous()        # stays on the device: no sync inside backward
        if ctx.det:
            return chamfer_grad_det(x, y, nxy, nyx, gd)
        if zeros_hook is not None:          # inside a training step: the two gradients come cleared from the step's arena (train.StepArena)
            gx, gy = zeros_hook(tuple(x.shape), torch.float32, x.device)[0], zeros_hook(tuple(y.shape), torch.float32, y.device)[0]
            _lib.call("pccx_chamfer_grad_dev_acc", x.data_ptr(), x.shape[0], x.shape[1], y.data_ptr(), y.shape[1], nxy.data_ptr(),
                      nyx.data_ptr(), gd.data_ptr(), gx.data_ptr(), gy.data_ptr(), 4, _stream())
            return gx, gy
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        _lib.call("pccx_chamfer_grad_dev", x.data_ptr(), x.shape[0], x.shape[1], y.data_ptr(), y.shape[1], nxy.data_ptr(),
                  nyx.data_ptr(), gd.data_ptr(), gx.data_ptr(), gy.data_ptr(), _stream())
        return gx, gy


def _chamfer_n(x, y, p, q, per_cloud):
    """Both nn_dist_n passes and pccx_chamfer_mean_n: (value (), per-cloud brackets (B,) or None, nxy, nyx)."""
    B, P, Q = x.shape[0], x.shape[1], y.shape[1]
    dxy, nxy = nn_dist_n(x, y, p, q, return_idx=True)
    dyx, nyx = nn_dist_n(y, x, q, p, return_idx=True)
    out = torch.empty((), device=x.device, dtype=torch.float32)
    per = torch.empty(B, device=x.device, dtype=torch.float32) if per_cloud else None
    _lib.call("pccx_chamfer_mean_n", dxy.data_ptr(), dyx.data_ptr(), B, P, p.data_ptr(), Q, q.data_ptr(), out.data_ptr(),
              per.data_ptr() if per is not None else None, _stream())
    return out, per, nxy, nyx


class _ChamferNFn(torch.autograd.Function):
    """_ChamferFn for ragged batches: p, q (B,) int32 on the device are pytorch3d's x_lengths / y_lengths.  forward = two nn_dist_n
    launches and pccx_chamfer_mean_n, backward = pccx_chamfer_grad_n with the argmins saved from the forward; the rows of the
    gradients behind the lengths are exact zeros."""

    @staticmethod
    def forward(ctx, x, y, p, q):
        out, _, nxy, nyx = _chamfer_n(x, y, p, q, False)
        ctx.save_for_backward(x, y, p, q, nxy, nyx)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, p, q, nxy, nyx = ctx.saved_tensors
        gd = g.detach().to(torch.float32).reshape(1).contiguous()        # stays on the device: no sync inside backward
        if zeros_hook is not None:          # inside a training step: cleared by the step's arena, accumulated into (flags & 4)
            gx, gy = zeros_hook(tuple(x.shape), torch.float32, x.device)[0], zeros_hook(tuple(y.shape), torch.float32, y.device)[0]
            flags = 4
        else:
            gx, gy, flags = torch.empty_like(x), torch.empty_like(y), 0
        _lib.call("pccx_chamfer_grad_n", x.data_ptr(), x.shape[0], x.shape[1], p.data_ptr(), y.data_ptr(), y.shape[1], q.data_ptr(),
                  nxy.data_ptr(), nyx.data_ptr(), gd.data_ptr(), gx.data_ptr(), gy.data_ptr(), flags, _stream())
        return gx, gy, None, None


class _STERound(torch.autograd.Function):
    """AE.STEQuantize (AE.py:72-85): forward x.round() (pccx_round: round half to even, as torch.round), backward the
    incoming gradient unchanged (straight-through estimator)."""

    @staticmethod
    def forward(ctx, x):
        xc = _f32c(x, "STEQuantize")
        y = torch.empty_like(xc)
        _lib.call("pccx_round", xc.data_ptr(), xc.numel(), y.data_ptr(), _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        return g


def ste_round(x):
    """AE.STEQuantize.apply.  compress.py:127 hands over a HOST tensor (the script moved the latents to the CPU at :121):
    such an input is uploaded, rounded by the kernel and returned on the caller's device -- there is no CPU compute path."""
    if isinstance(x, torch.Tensor) and not x.is_cuda:
        return _STERound.apply(x.cuda()).to(x.device)
    return _STERound.apply(x)


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, batch_reduction="mean"):
    """pytorch3d.loss.chamfer_distance defaults (AE.py:67, eval.py:204): squared distances,
    point mean, both directions summed; returns (value, None).  Differentiable w.r.t. x and y for
    batch_reduction="mean" (the loss of AE.py:57-70 / pppe_pcd_ae.py:817-838).

    x_lengths / y_lengths (pytorch3d's names and pytorch3d's positions, third and fourth: batch_reduction is passed by keyword, as
    every caller in the tree does; either alone means the other cloud is full): cloud b is the first x_lengths[b] rows of
    x (B,P_max,3) and the first y_lengths[b] of y, each point mean is over those rows, and what lies behind them is never read.  Host
    sequences are checked against [1, P_max] before any launch; device tensors are read by the kernels only.  Differentiable for
    "mean" (gradient rows behind the lengths are exact zeros); batch_reduction=None returns the (B,) per-cloud values.  The
    deterministic mode has no ragged form (pccx_chamfer_grad_det is dense): inside a deterministic step this raises."""
    if x_lengths is not None or y_lengths is not None:
        if deterministic_hook is not None and deterministic_hook():
            raise _lib.PccxError("chamfer_distance: x_lengths / y_lengths cannot be combined with the deterministic mode -- the ordered "
                                 "scatter of pccx_chamfer_grad_det is dense only; run the step with deterministic=False, or pad to one size")
        if batch_reduction not in ("mean", "sum", None):
            raise _lib.PccxError(f"chamfer_distance: batch_reduction must be 'mean', 'sum' or None, got {batch_reduction!r}")
        x, y = _f32c(x, "chamfer.x"), _f32c(y, "chamfer.y")
        B, P, Q = x.shape[0], x.shape[1], y.shape[1]
        p = checked_counts(x_lengths if x_lengths is not None else [P] * B, B, P, x.device, "chamfer.x_lengths")
        q = checked_counts(y_lengths if y_lengths is not None else [Q] * B, B, Q, x.device, "chamfer.y_lengths")
        if batch_reduction == "mean" and (x.requires_grad or y.requires_grad):
            return _ChamferNFn.apply(x, y, p, q), None
        out, per, _, _ = _chamfer_n(x.detach(), y.detach(), p, q, batch_reduction != "mean")
        return (out if batch_reduction == "mean" else per.double().sum().float() if batch_reduction == "sum" else per), None
    if batch_reduction == "mean" and (x.requires_grad or y.requires_grad):
        return _ChamferFn.apply(_f32c(x, "chamfer.x"), _f32c(y, "chamfer.y")), None
    dxy, dyx = nn_dist(x, y), nn_dist(y, x)
    per = dxy.double().mean(dim=1) + dyx.double().mean(dim=1)
    if batch_reduction == "mean":
        per = per.mean()
    elif batch_reduction == "sum":
        per = per.sum()
    return per.float(), None


def octree_bits_capacity(S):
    """Longest possible stream of S centres in bits (1 + 8*S*16); the packed rows are (cap + 7) // 8 bytes."""
    return int(_lib.load().pccx_octree_bits_capacity(int(S)))


def octree_encode(centres, N, min_bpp, out_bytes=None, out_nbytes=None, wide=False):
    """pn_kit.encode_sampled_np (pn_kit.py:380-401) + binary_array_to_byte_array (:463-467),
    batched on the GPU.  centres (B,S,3).  Returns dict of device tensors:
    bits (B,cap) u8 one byte per bit, nbits (B), depth (B), bytes (B,stride) u8, nbytes (B).
    out_bytes / out_nbytes: caller-provided dense destinations of that shape (codec.Compressed's packed buffer).
    S > 1024 (to 8192), or wide=True at any S, takes pccx_octree_encode_wide: the same outputs."""
    centres = _f32c(centres, "octree_encode")
    B, S, _ = centres.shape
    cap = octree_bits_capacity(S)
    dev = centres.device
    if out_bytes is None:
        out_bytes = torch.empty(B, (cap + 7) // 8, device=dev, dtype=torch.uint8)
    if out_nbytes is None:
        out_nbytes = torch.empty(B, device=dev, dtype=torch.int32)
    if (tuple(out_bytes.shape) != (B, (cap + 7) // 8) or out_bytes.dtype != torch.uint8 or not out_bytes.is_contiguous()
            or tuple(out_nbytes.shape) != (B,) or out_nbytes.dtype != torch.int32 or not out_nbytes.is_contiguous()):
        raise _lib.PccxError("octree_encode: out_bytes must be dense (B, (cap+7)//8) u8 and out_nbytes dense (B,) i32")
    r = dict(bits=torch.empty(B, cap, device=dev, dtype=torch.uint8),
             nbits=torch.empty(B, device=dev, dtype=torch.int32),
             depth=torch.empty(B, device=dev, dtype=torch.int32),
             bytes=out_bytes, nbytes=out_nbytes)
    _lib.call("pccx_octree_encode_wide" if wide or S > PATCH_GROUPS_MAX_S else "pccx_octree_encode", centres.data_ptr(), B, S, int(N), float(min_bpp), r["bits"].data_ptr(),
              r["nbits"].data_ptr(), r["depth"].data_ptr(), r["bytes"].data_ptr(), r["nbytes"].data_ptr(), _stream())
    return r


def octree_encode_n(centres, S, N, min_bpp, out_bytes=None, out_nbytes=None):
    """octree_encode for a ragged batch (pccx_octree_encode_n): centres (B,S_max,3), S_max <= 1024, of which cloud b codes its first
    S[b] with its own point count N[b] in the depth search.  The same dict; the strides are those of S_max, and cloud b's
    bytes[:nbytes] / depth are octree_encode's on its own S[b] centres."""
    centres = _f32c(centres, "octree_encode_n")
    B, S_max, _ = centres.shape
    cap = octree_bits_capacity(S_max)
    dev = centres.device
    S, N = counts(S, B, dev, "octree_encode_n.S"), counts(N, B, dev, "octree_encode_n.N")
    if out_bytes is None:
        out_bytes = torch.empty(B, (cap + 7) // 8, device=dev, dtype=torch.uint8)
    if out_nbytes is None:
        out_nbytes = torch.empty(B, device=dev, dtype=torch.int32)
    if (tuple(out_bytes.shape) != (B, (cap + 7) // 8) or out_bytes.dtype != torch.uint8 or not out_bytes.is_contiguous()
            or tuple(out_nbytes.shape) != (B,) or out_nbytes.dtype != torch.int32 or not out_nbytes.is_contiguous()):
        raise _lib.PccxError("octree_encode_n: out_bytes must be dense (B, (cap+7)//8) u8 and out_nbytes dense (B,) i32")
    r = dict(bits=torch.empty(B, cap, device=dev, dtype=torch.uint8),
             nbits=torch.empty(B, device=dev, dtype=torch.int32),
             depth=torch.empty(B, device=dev, dtype=torch.int32),
             bytes=out_bytes, nbytes=out_nbytes)
    _lib.call("pccx_octree_encode_n", centres.data_ptr(), B, S_max, S.data_ptr(), N.data_ptr(), float(min_bpp), r["bits"].data_ptr(),
              r["nbits"].data_ptr(), r["depth"].data_ptr(), r["bytes"].data_ptr(), r["nbytes"].data_ptr(), _stream())
    return r


def reassemble_n(patches, S, k, scale, centres, center, longest, margin=0.01):
    """The reassembly step of decompress.py:104-116 for a ragged batch (pccx_reassemble_n): patches (B*S_max,k,3) raw decoder output,
    centres (B,S_max,3), S (B,) patches per cloud, scale (B,) f32 on the device -> (B, S_max*k, 3), cloud b's first S[b]*k rows
    filled, the rest left unwritten."""
    centres = _f32c(centres, "reassemble_n.centres")
    B, S_max, _ = centres.shape
    patches = _f32c(patches, "reassemble_n.patches")
    if patches.numel() != B * S_max * int(k) * 3:
        raise _lib.PccxError(f"reassemble_n: patches of {tuple(patches.shape)} for {B} clouds of {S_max} patches of {k} points")
    S = counts(S, B, centres.device, "reassemble_n.S")
    scale, center, longest = _f32c(scale, "reassemble_n.scale"), _f32c(center.reshape(B, 3), "reassemble_n.center"), _f32c(longest.reshape(B), "reassemble_n.longest")
    out = torch.empty(B, S_max * int(k), 3, device=centres.device, dtype=torch.float32)
    _lib.call("pccx_reassemble_n", patches.data_ptr(), B, S_max, S.data_ptr(), int(k), scale.data_ptr(), centres.data_ptr(), center.data_ptr(),
              longest.data_ptr(), float(margin), out.data_ptr(), _stream())
    return out


def octree_decode(bytes_, nbytes, mode="reference", S_out=64, wide=False):
    """pn_kit.decode_sampled_np (pn_kit.py:424-431) from packed streams.  mode 'reference' is
    bug-compatible with octree_np.decode as written; 'full' is the level-by-level decode.
    bytes_ (B,stride) u8, nbytes (B) i32 -> (points (B,S_out,3), count (B)).
    'full' with S_out > 1024, or wide=True, decodes with the wide kernel: up to 8192 cells per level where the narrow one stops at 2048."""
    _dev(bytes_, "octree_decode")
    bytes_ = bytes_.contiguous()
    B, stride = bytes_.shape
    nbytes = _dev(nbytes, "octree_decode.nbytes").to(torch.int32).contiguous()
    out = torch.empty(B, S_out, 3, device=bytes_.device, dtype=torch.float32)
    count = torch.empty(B, device=bytes_.device, dtype=torch.int32)
    _lib.call("pccx_octree_decode", bytes_.data_ptr(), stride, nbytes.data_ptr(), B,
              {"reference": 0, "full": 2 if wide else 1}[mode], int(S_out), out.data_ptr(), count.data_ptr(), _stream())
    return out, count


def ply_unpack(staging, table, tile_prefix, out, total_tiles):
    """pccx_ply_unpack (csrc/plyio.hip): raw PLY vertex records -> float32 x y z rows.  staging: device uint8, its memory 16-byte
    aligned and a multiple of 16 bytes long; table (B, 12) int64 and tile_prefix (B + 1,) int32 on the device, as
    plyio.device_tables lays them out, total_tiles the prefix's last entry (the grid); out (rows, 3) f32, written
    in place and returned.  One kernel on the current stream."""
    for t, name, dtype in ((staging, "staging", torch.uint8), (table, "table", torch.int64), (tile_prefix, "tile_prefix", torch.int32),
                           (out, "out", torch.float32)):
        if _dev(t, "ply_unpack." + name).dtype != dtype or not t.is_contiguous():
            raise _lib.PccxError(f"ply_unpack.{name}: a contiguous {dtype} tensor is expected")
    B = int(table.shape[0])
    if table.dim() != 2 or table.shape[1] != 12 or tuple(tile_prefix.shape) != (B + 1,) or out.dim() != 2 or out.shape[1] != 3:
        raise _lib.PccxError("ply_unpack: table (B, 12), tile_prefix (B + 1,) and out (rows, 3) are expected")
    if staging.numel() % 16 or staging.data_ptr() % 16:
        raise _lib.PccxError("ply_unpack.staging: must start at a multiple of 16 bytes and be a multiple of 16 bytes long")
    _lib.call("pccx_ply_unpack", staging.data_ptr(), staging.numel(), table.data_ptr(), tile_prefix.data_ptr(), B, int(total_tiles),
              out.data_ptr(), int(out.shape[0]), _stream())
    return out


MESH_MAX_B, MESH_MAX_N, MESH_MAX_F = 1024, 1 << 20, 1 << 22         # csrc/mesh_sample.hip: meshes per call, samples per mesh, faces per mesh


def mesh_sample_workspace_bytes(B, F_total, n):
    return int(_lib.load().pccx_mesh_sample_workspace_bytes(int(B), int(F_total), int(n)))


def mesh_sample(verts, faces, v_off, f_off, seeds, n, normalize=True, out=None, workspace=None):
    """pccx_mesh_sample (csrc/mesh_sample.hip): n points on each of B triangle meshes.  verts (V_total, 3) f32 and faces (F_total, 3)
    int32 (indices local to their mesh) hold mesh after mesh; v_off / f_off (B + 1,) int64 and seeds (B,) int64 on the device.
    -> (out (B, n, 3) f32, status (B,) int32: 0 good, 1 no area -- NaN rows --, 2 nothing to scale by).  normalize: the unit-cube
    normalisation of sample_modelnet.py, else the raw samples.  workspace: a uint8 device tensor of at least
    mesh_sample_workspace_bytes(B, F_total, n) bytes whose content does not matter (default: allocated here); afterwards it begins with
    a_t float64, w_t uint64 and the inclusive prefix I_t uint64, F_total each.  Only enqueues kernels on the current stream."""
    for t, name, dtype, cols in ((verts, "verts", torch.float32, 3), (faces, "faces", torch.int32, 3), (v_off, "v_off", torch.int64, None),
                                 (f_off, "f_off", torch.int64, None), (seeds, "seeds", torch.int64, None)):
        if _dev(t, "mesh_sample." + name).dtype != dtype or not t.is_contiguous() or t.dim() != (2 if cols else 1) or (cols and t.shape[1] != cols):
            raise _lib.PccxError(f"mesh_sample.{name}: a contiguous {dtype} tensor of shape {'(rows, 3)' if cols else '(len,)'} is expected")
    B, n = int(seeds.shape[0]), int(n)
    if tuple(v_off.shape) != (B + 1,) or tuple(f_off.shape) != (B + 1,):
        raise _lib.PccxError(f"mesh_sample: {B} seeds need v_off and f_off of ({B + 1},)")
    if not 1 <= B <= MESH_MAX_B or not 1 <= n <= MESH_MAX_N:
        raise _lib.PccxError(f"mesh_sample: B={B}, n={n}; one call takes 1..{MESH_MAX_B} meshes and 1..{MESH_MAX_N} samples of each")
    V_total, F_total = int(verts.shape[0]), int(faces.shape[0])
    if V_total < 1 or F_total < 1:
        raise _lib.PccxError("mesh_sample: empty verts or faces")
    need = mesh_sample_workspace_bytes(B, F_total, n)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=verts.device)
    elif _dev(workspace, "mesh_sample.workspace").dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need or workspace.data_ptr() % 8:
        raise _lib.PccxError(f"mesh_sample.workspace: a contiguous 8-byte-aligned uint8 tensor of at least {need} bytes is expected")
    if out is None:
        out = torch.empty(B, n, 3, dtype=torch.float32, device=verts.device)
    elif _dev(out, "mesh_sample.out").dtype != torch.float32 or tuple(out.shape) != (B, n, 3) or not out.is_contiguous():
        raise _lib.PccxError(f"mesh_sample.out: a contiguous float32 tensor of ({B}, {n}, 3) is expected")
    status = torch.empty(B, dtype=torch.int32, device=verts.device)
    with torch.cuda.device(verts.device):
        _lib.call("pccx_mesh_sample", verts.data_ptr(), V_total, faces.data_ptr(), F_total, v_off.data_ptr(), f_off.data_ptr(), seeds.data_ptr(), B, n,
                  1 if normalize else 0, out.data_ptr(), status.data_ptr(), workspace.data_ptr(), _stream())
    return out, status
