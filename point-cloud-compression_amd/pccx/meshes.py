"""Triangle meshes in, point clouds out: what sample_modelnet.py does with pyntcloud, for a batch of OFF files at a time.

read_off is the file-at-a-time Python reader and the yardstick of the host threads (pccx_off_scan_host / pccx_off_load_host,
csrc/off_host.h); read_meshes reads a batch with them into one pinned buffer and makes one copy to the device; sample_meshes draws the
clouds there (pccx_mesh_sample, csrc/mesh_sample.hip).  The sampler's definition is DESIGN.md section 4.5 ("meshes")."""
import hashlib
import re

import numpy as np

from .plyio import _MSG, _Pinned, _path_table

ROW = 8                        # int64 per file of the scan table (include/pccx.h: PCCX_OFF_ROW)
STATUS, NV, NF, BODY_OFFSET, FILE_SIZE, NE = 0, 1, 2, 3, 4, 5
# csrc/off_host.h OffStatus
OK, NOT_OFF, TRUNCATED, BAD_NV, BAD_NF, NOT_TRIANGLE, BAD_INDEX, BAD_COORD, MALFORMED, IO, ARG = range(11)
MAX_VERTICES, MAX_FACES = 2**31 - 1, 2**22

_COUNT = re.compile(r"\+?[0-9]+\Z")
# what std::from_chars reads behind an optional sign (inf and nan parse, and are refused afterwards as not finite)
_NUMBER = re.compile(r"[+-]?(([0-9]+\.?[0-9]*|\.[0-9]+)(e[+-]?[0-9]+)?|inf|infinity|nan)\Z", re.IGNORECASE)


class OffError(ValueError):
    """A refused OFF file: .status is csrc/off_host.h's OffStatus, the message names the cause."""

    def __init__(self, status, text):
        super().__init__(text)
        self.status = status


def _lines(data, pos):
    """the lines of data[pos:] that hold a token outside their comment, as token lists"""
    for line in data[pos:].split(b"\n"):
        tok = line.split(b"#", 1)[0].decode("ascii", "replace").split()
        if tok:
            yield tok


def _count(tok):
    return int(tok) if _COUNT.match(tok) else -1


def parse_off(data):
    """The bytes of one OFF file -> (V (nv, 3) float32, F (nf, 3) int32), or OffError: the grammar and the refusals of csrc/off_host.h."""
    pos, head = 0, []
    while len(head) < 2:                                       # the OFF line and, if it holds no count, the line of the counts
        if pos >= len(data):
            raise OffError(TRUNCATED, "truncated: the file ends before its " + ("three counts" if head else "OFF line"))
        end = data.find(b"\n", pos)
        end = len(data) if end < 0 else end
        tok = data[pos:end].split(b"#", 1)[0].decode("ascii", "replace").split()
        pos = min(end + 1, len(data))
        if not tok:
            continue
        if not head:
            if not tok[0].startswith("OFF"):
                raise OffError(NOT_OFF, "not an OFF file")
            counts = ([tok[0][3:]] if len(tok[0]) > 3 else []) + tok[1:]
            if len(counts) > 3:
                raise OffError(MALFORMED, "the OFF line holds more than three counts")
            head.append(tok)
            if counts:
                if len(counts) != 3:
                    raise OffError(MALFORMED, "the OFF line does not hold three counts (nv nf ne)")
                head.append(counts)
        else:
            if len(tok) != 3:
                raise OffError(MALFORMED, "the line of the counts does not hold three counts (nv nf ne)")
            head.append(tok)
    nv, nf, ne = (_count(t) for t in head[1])
    if nv == -1 or nf == -1 or ne == -1:
        raise OffError(MALFORMED, "a count (nv nf ne) is no number")
    if not 3 <= nv <= MAX_VERTICES:
        raise OffError(BAD_NV, "vertex count nv must be 3 .. 2147483647")
    if not 1 <= nf <= MAX_FACES:
        raise OffError(BAD_NF, "face count nf must be 1 .. 4194304")
    if nv * 6 + nf * 8 - 1 > len(data) - pos:
        raise OffError(TRUNCATED, "truncated: the file is too short for its counts")
    lines = _lines(data, pos)
    V, F = np.empty((nv, 3), dtype=np.float32), np.empty((nf, 3), dtype=np.int32)
    for i in range(nv):
        tok = next(lines, None)
        if tok is None:
            raise OffError(TRUNCATED, "truncated: fewer vertex lines than nv")
        if len(tok) != 3:
            raise OffError(BAD_COORD, "a vertex line does not hold three numbers")
        for c in range(3):
            if not _NUMBER.match(tok[c]):
                raise OffError(BAD_COORD, "a vertex line holds a token that is no number")
            with np.errstate(over="ignore"):
                V[i, c] = np.float32(float(tok[c]))            # to double, then to float32: two roundings, as the threads make
            if not np.isfinite(V[i, c]):
                raise OffError(BAD_COORD, "a vertex coordinate is not finite as float32")
    for i in range(nf):
        tok = next(lines, None)
        if tok is None:
            raise OffError(TRUNCATED, "truncated: fewer face lines than nf")
        corners = _count(tok[0])
        if corners == -1:
            raise OffError(BAD_INDEX, "a face line does not begin with a count")
        if corners != 3:
            raise OffError(NOT_TRIANGLE, "a face is not a triangle (polygons are not triangulated)")
        if len(tok) < 4:
            raise OffError(BAD_INDEX, "a face line holds fewer than three indices")
        for c in range(3):
            v = _count(tok[1 + c])
            if not 0 <= v < nv:
                raise OffError(BAD_INDEX, "a face index is no number or lies outside 0 .. nv - 1")
            F[i, c] = v
    return V, F


def read_off(path):
    """-> (V (nv, 3) float32, F (nf, 3) int32) of one OFF triangle mesh; ValueError naming the path and the cause for a file that is
    refused (not OFF, truncated, nv outside 3..2^31-1, nf outside 1..2^22, a polygon, an index outside 0..nv-1, a coordinate that is
    no finite number).  One file at a time, in Python: the yardstick for read_meshes."""
    with open(path, "rb") as f:
        data = f.read()
    try:
        return parse_off(data)
    except OffError as e:
        raise OffError(e.status, f"{path}: {e}") from None


def _text(msg):
    return bytes(msg).split(bytes(1))[0].decode("utf-8", "replace")


def _raise_refused(paths, refused, who):
    """refused: [(index, cause)]"""
    if refused:
        raise ValueError(f"{who}: {len(refused)} of {len(paths)} OFF files refused:\n  " + "\n  ".join(f"{paths[b]}: {why}" for b, why in refused))


def _raise_bad(paths, table, msgs, who):
    _raise_refused(paths, [(b, _text(msgs[b])) for b in np.flatnonzero(table[:, STATUS] != 0).tolist()], who)


def scan_meshes(paths, threads=0, check=True):
    """pccx_off_scan_host: the headers of every file -> table (B, ROW) int64, one row per file (status, nv, nf, body offset, file size,
    ne).  check: raise ValueError naming every refused file and its cause; check=False returns (table, msgs) instead.  No GPU call."""
    from . import _lib
    paths = [str(p) for p in paths]
    blob, off = _path_table(paths)
    table = np.zeros((len(paths), ROW), dtype=np.int64)
    msgs = np.zeros((len(paths), _MSG), dtype=np.uint8)
    if paths:
        _lib.call("pccx_off_scan_host", len(paths), blob, off.ctypes.data, table.ctypes.data, msgs.ctypes.data, _MSG, int(threads))
    if not check:
        return table, msgs
    _raise_bad(paths, table, msgs, "scan_meshes")
    return table


def staging_offsets(table):
    """(v_dst (B,), f_dst (B,), total): byte offsets of the packed form -- every good file's vertices one behind the other, then every
    good file's faces -- in one staging buffer of `total` bytes.  A refused file takes no room."""
    good = table[:, STATUS] == 0
    vb, fb = np.where(good, 12 * table[:, NV], 0), np.where(good, 12 * table[:, NF], 0)
    v_end, f_end = np.cumsum(vb), np.cumsum(fb)
    v_total = int(v_end[-1]) if len(v_end) else 0
    return (v_end - vb).astype(np.int64), (v_total + f_end - fb).astype(np.int64), v_total + (int(f_end[-1]) if len(f_end) else 0)


def load_meshes(paths, table, staging, v_dst, f_dst, threads=0, check=True):
    """pccx_off_load_host: every good file's body parsed by the threads, nv * 3 float32 to staging[v_dst[b]:] and nf * 3 int32 (indices
    local to the mesh) to staging[f_dst[b]:] (a contiguous host uint8 tensor or array at a multiple of 4).  A file refused here gets
    its status into `table`; check as in scan_meshes.  No GPU call."""
    from . import _lib
    paths = [str(p) for p in paths]
    blob, off = _path_table(paths)
    v_dst, f_dst = np.ascontiguousarray(v_dst, dtype=np.int64), np.ascontiguousarray(f_dst, dtype=np.int64)
    if table.dtype != np.int64 or table.shape != (len(paths), ROW) or not table.flags.c_contiguous or v_dst.shape != (len(paths),) or f_dst.shape != v_dst.shape:
        raise ValueError(f"load_meshes: a contiguous ({len(paths)}, {ROW}) int64 table and two offsets per file are expected")
    ptr, nbytes = (staging.ctypes.data, staging.nbytes) if isinstance(staging, np.ndarray) else (staging.data_ptr(), staging.numel() * staging.element_size())
    msgs = np.zeros((len(paths), _MSG), dtype=np.uint8)
    if paths:
        _lib.call("pccx_off_load_host", len(paths), blob, off.ctypes.data, table.ctypes.data, ptr, nbytes, v_dst.ctypes.data, f_dst.ctypes.data,
                  msgs.ctypes.data, _MSG, int(threads))
    if not check:
        return msgs
    _raise_bad(paths, table, msgs, "load_meshes")


def check_meshes(paths, threads=0, scanned=None):
    """Every file of `paths` read once on the host (headers and bodies), nothing kept: -> [(index, cause)] of the refused ones.
    scanned: the (table, msgs) of scan_meshes(paths, check=False), when the caller has them."""
    paths = [str(p) for p in paths]
    table, msgs = scan_meshes(paths, threads, check=False) if scanned is None else scanned
    v_dst, f_dst, total = staging_offsets(table)
    msgs2 = load_meshes(paths, table, np.empty(max(total, 4), dtype=np.uint8), v_dst, f_dst, threads, check=False)
    return [(b, _text(msgs[b]) or _text(msgs2[b])) for b in np.flatnonzero(table[:, STATUS] != 0).tolist()]


_staging = _Pinned()


def release_pinned():
    """Give back the pinned buffer read_meshes keeps between calls (it only grows).  Waits for the copy that last used it."""
    _staging.drop()


def read_meshes(paths, device, threads=0):
    """The OFF files of `paths` on `device` in the packed form pccx_mesh_sample takes -> (verts (V_total, 3) f32, faces (F_total, 3)
    int32, v_off (B + 1,) int64, f_off (B + 1,) int64): scan, one pinned staging buffer filled by the host threads (the two offset
    tables travel in its tail), ONE host-to-device copy.  Any file that cannot be read raises ValueError naming every such path and its
    cause, before any GPU work."""
    import torch
    paths = [str(p) for p in paths]
    if not paths:
        raise ValueError("read_meshes: at least one file is expected")
    B = len(paths)
    table, msgs = scan_meshes(paths, threads, check=False)
    if (table[:, STATUS] != 0).any():                          # the bodies of the others are read too, so that ONE error names every bad file
        _raise_refused(paths, check_meshes(paths, threads, (table, msgs)), "read_meshes")
    v_dst, f_dst, data_bytes = staging_offsets(table)
    t0 = (data_bytes + 7) // 8 * 8
    t1 = t0 + 8 * (B + 1)
    total = t1 + 8 * (B + 1)
    host = _staging.take(total)
    load_meshes(paths, table, host[:data_bytes], v_dst, f_dst, threads)
    view = host.numpy()
    view[data_bytes:t0] = 0
    view[t0:t1] = np.concatenate([[0], np.cumsum(table[:, NV])]).astype(np.int64).view(np.uint8)
    view[t1:total] = np.concatenate([[0], np.cumsum(table[:, NF])]).astype(np.int64).view(np.uint8)
    on_dev = torch.empty(total, dtype=torch.uint8, device=device)
    with torch.cuda.device(on_dev.device):
        on_dev.copy_(host, non_blocking=True)
        _staging.mark()
    v_bytes = 12 * int(table[:, NV].sum())
    return (on_dev[:v_bytes].view(torch.float32).view(-1, 3), on_dev[v_bytes:data_bytes].view(torch.int32).view(-1, 3),
            on_dev[t0:t1].view(torch.int64), on_dev[t1:total].view(torch.int64))


def stream_seed(seed, relpath):
    """The 64-bit stream of one file: the first 8 bytes (little endian) of blake2b(seed as 8 little-endian bytes + relpath in utf-8).
    A file's cloud depends on the run's seed and on its own relative path, not on the glob's order or the chunking."""
    h = hashlib.blake2b((int(seed) & (2**64 - 1)).to_bytes(8, "little") + str(relpath).encode("utf-8")).digest()
    return int.from_bytes(h[:8], "little")


def sample_meshes(verts, faces, v_off, f_off, n, seeds, normalize="unit", out=None, workspace=None):
    """n points on each mesh of a packed batch (read_meshes) -> (points (B, n, 3) f32, status (B,) int32).  seeds: B integers (any 64
    bits each; a host sequence, or an int64 device tensor taken as it is): sample i of mesh b is a function of (mesh b, seeds[b], i)
    alone.  normalize: "unit" = sample_modelnet.py's (p - min) / max(p - min) per mesh, None = the raw samples.  status: 0 good, 1 the
    mesh has no area (its rows are NaN), 2 every sampled value is the same (rows shifted, not scaled)."""
    import torch
    from . import ops
    if normalize not in ("unit", None):
        raise ValueError(f"sample_meshes: normalize must be 'unit' or None, got {normalize!r}")
    if not isinstance(seeds, torch.Tensor):
        s = np.array([int(v) & (2**64 - 1) for v in seeds], dtype=np.uint64).view(np.int64)
        seeds = torch.from_numpy(s).to(verts.device)
    return ops.mesh_sample(verts, faces, v_off, f_off, seeds, n, normalize == "unit", out=out, workspace=workspace)
