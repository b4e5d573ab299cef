"""Minimal PLY point-cloud I/O (x,y,z vertices), replacing the reference's plyfile / pyntcloud use
(pn_kit.py:25-42: read_point_cloud, save_point_cloud).  Reads ASCII and binary_little_endian files
with arbitrary extra vertex properties; writes binary_little_endian float32 x,y,z."""
import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
          "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
          "double": "f8", "float64": "f8"}


def read_point_cloud(path):
    """-> (N,3) float32, columns x,y,z (or X,Y,Z, as pn_kit.py:27-30 accepts)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, n_vertex, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated header")
            tok = line.decode("ascii", "replace").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    n_vertex = int(tok[2])
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError(f"{path}: list property on vertex element unsupported")
                props.append((tok[2], _TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        names = [p[0] for p in props]
        cols = [names.index(c) if c in names else names.index(c.upper()) for c in ("x", "y", "z")]
        if fmt == "ascii":
            data = np.loadtxt(f, max_rows=n_vertex, ndmin=2)
            return np.ascontiguousarray(data[:, cols], dtype=np.float32)
        if fmt not in ("binary_little_endian", "binary_big_endian"):
            raise ValueError(f"{path}: unsupported PLY format {fmt}")
        end = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(n, end + t) for n, t in props])
        raw = np.frombuffer(f.read(n_vertex * dt.itemsize), dtype=dt, count=n_vertex)
        return np.stack([raw[names[c]].astype(np.float32) for c in cols], axis=1)


def save_point_cloud(pc, path):
    pc = np.ascontiguousarray(pc, dtype="<f4").reshape(-1, 3)
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % pc.shape[0])
        f.write(b"property float x\nproperty float y\nproperty float z\nend_header\n")
        f.write(pc.tobytes())


# ---- a batch of files at once: headers and raw vertex blocks on the library's host threads (csrc/hostio.hip), conversion to float32
# on the GPU (pccx_ply_unpack, csrc/plyio.hip).  The same arrays and the same files as the two functions above, bit for bit.
ROW = 16                       # int64 per file of the scan table (include/pccx.h: PCCX_PLY_ROW)
STATUS, FORMAT, N_VERTEX, STRIDE, DATA_OFFSET, FILE_SIZE, OFF_X, TYPE_X, N_PROPS, COL_X = 0, 1, 2, 3, 4, 5, 6, 9, 12, 13
ASCII, LITTLE, BIG = 0, 1, 2
TILE = 256                     # rows per workgroup of pccx_ply_unpack
_MSG = 256


def _path_table(paths):
    import os
    blob, off, o = bytearray(), np.zeros(max(len(paths), 1), dtype=np.int64), 0
    for i, p in enumerate(paths):
        e = os.fsencode(p)
        if b"\0" in e:
            raise ValueError(f"path {p!r} holds a zero byte")
        off[i] = o
        blob += e + b"\0"
        o += len(e) + 1
    return bytes(blob) or b"\0", off


def _raise_bad(paths, table, msgs, who):
    bad = np.flatnonzero(table[:, STATUS] != 0)
    if len(bad):
        why = [f"{paths[b]}: {bytes(msgs[b]).split(bytes(1))[0].decode('utf-8', 'replace')}" for b in bad.tolist()]
        raise ValueError(f"{who}: {len(bad)} of {len(paths)} PLY files refused:\n  " + "\n  ".join(why))


def scan_point_clouds(paths, threads=0, check=True):
    """pccx_ply_scan_host: the headers of every file -> table (B, ROW) int64, one row per file (include/pccx.h names the columns;
    table[:, N_VERTEX] are the point counts).  check: raise ValueError naming every refused file and its cause; check=False returns
    (table, msgs) with the statuses in column 0 instead.  No GPU call."""
    from . import _lib
    paths = [str(p) for p in paths]
    blob, off = _path_table(paths)
    table = np.zeros((len(paths), ROW), dtype=np.int64)
    msgs = np.zeros((len(paths), _MSG), dtype=np.uint8)
    if paths:
        _lib.call("pccx_ply_scan_host", len(paths), blob, off.ctypes.data, table.ctypes.data, msgs.ctypes.data, _MSG, int(threads))
    if not check:
        return table, msgs
    _raise_bad(paths, table, msgs, "scan_point_clouds")
    return table


def block_bytes(table):
    """Bytes of every file's vertex block in the staging buffer: n * stride, n * 12 for an ASCII file (parsed to float32 x y z)."""
    return table[:, N_VERTEX] * np.where(table[:, FORMAT] == ASCII, 12, table[:, STRIDE])


def staging_offsets(table):
    """(dst_off (B,) int64, total): consecutive 16-byte-aligned places of the files' vertex blocks in one staging buffer."""
    size = (block_bytes(table) + 15) // 16 * 16
    end = np.cumsum(size)
    return (end - size).astype(np.int64), int(end[-1]) if len(end) else 0


def load_point_clouds(paths, table, staging, dst_off, threads=0, check=True):
    """pccx_ply_load_host: every file's vertex block, as it is in the file, to staging[dst_off[b]:] (a contiguous host uint8 tensor or
    array whose memory starts at a multiple of 16); ASCII files are parsed to float32 x y z records and their rows of `table` rewritten
    to say so.  check as in scan_point_clouds.  No GPU call."""
    from . import _lib
    paths = [str(p) for p in paths]
    blob, off = _path_table(paths)
    dst_off = np.ascontiguousarray(dst_off, dtype=np.int64)
    if table.dtype != np.int64 or table.shape != (len(paths), ROW) or not table.flags.c_contiguous or dst_off.shape != (len(paths),):
        raise ValueError(f"load_point_clouds: a contiguous ({len(paths)}, {ROW}) int64 table and one offset per file are expected")
    ptr, nbytes = (staging.ctypes.data, staging.nbytes) if isinstance(staging, np.ndarray) else (staging.data_ptr(), staging.numel() * staging.element_size())
    msgs = np.zeros((len(paths), _MSG), dtype=np.uint8)
    if paths:
        _lib.call("pccx_ply_load_host", len(paths), blob, off.ctypes.data, table.ctypes.data, ptr, nbytes, dst_off.ctypes.data, msgs.ctypes.data, _MSG, int(threads))
    if not check:
        return msgs
    _raise_bad(paths, table, msgs, "load_point_clouds")


class _Pinned:
    """One pinned host buffer, kept and grown (never shrunk): `take(n)` hands out its first n bytes once the copy that last read or
    wrote it has finished."""

    def __init__(self):
        self.buf, self.busy = None, None

    def take(self, nbytes):
        import torch
        if self.busy is not None:
            self.busy.synchronize()
            self.busy = None
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = None
            self.buf = torch.empty(max(nbytes, 1 << 20) * 5 // 4 // 16 * 16 + 16, dtype=torch.uint8, pin_memory=True)
        return self.buf[:nbytes]

    def mark(self):
        import torch
        self.busy = torch.cuda.Event()
        self.busy.record()

    def drop(self):
        if self.busy is not None:
            self.busy.synchronize()
        self.buf, self.busy = None, None


_staging, _writeback = _Pinned(), _Pinned()


def release_pinned():
    """Give back the two pinned buffers read_point_clouds / save_point_clouds keep between calls (they only grow): for a caller that
    has read a whole set in one call and will not read again, such as a trainer.  Waits for the copy that last used them."""
    _staging.drop()
    _writeback.drop()


def device_tables(table, dst_off, dst_row, cap):
    """The kernel's side of a scan table (host arrays): dev (B, 12) int64 = source byte offset, stride, byte offset of x y z, type
    code of x y z, big endian, n, dst_row, cap; prefix (B + 1,) int32 = exclusive prefix of the clouds' 256-row tiles."""
    B = table.shape[0]
    dev = np.zeros((B, 12), dtype=np.int64)
    dev[:, 0], dev[:, 1] = dst_off, table[:, STRIDE]
    dev[:, 2:5], dev[:, 5:8] = table[:, OFF_X:OFF_X + 3], table[:, TYPE_X:TYPE_X + 3]
    dev[:, 8], dev[:, 9], dev[:, 10], dev[:, 11] = table[:, FORMAT] == BIG, table[:, N_VERTEX], dst_row, cap
    tiles = np.concatenate([[0], np.cumsum((np.asarray(cap, dtype=np.int64) + TILE - 1) // TILE)])
    if tiles[-1] > 2**31 - 1:
        raise ValueError(f"read_point_clouds: {int(tiles[-1])} tiles of {TILE} rows; one call takes 2^31 - 1")
    return dev, tiles.astype(np.int32)


def read_point_clouds(paths, device, layout="padded", threads=0, table=None, out=None):
    """The files of `paths` on `device`, read by host threads and unpacked by one kernel: scan (skipped when `table`, the rows of
    scan_point_clouds for these paths, is given), one pinned staging buffer filled with the raw vertex blocks, ONE host-to-device
    copy (the kernel's tables travel in its tail), pccx_ply_unpack.
      layout="padded" -> (pc (B, N_max, 3) f32, n list): codec.pad_clouds of the clouds read_point_cloud returns, bit for bit;
      layout="packed" -> (points (M_total, 3), offsets (B + 1,) int64, sizes list): codec.pack_clouds of them.
    out: a contiguous float32 device tensor of the result's (rows, 3) to write into (default: allocated here).
    Any file that cannot be read raises ValueError naming every such path and its cause, before any GPU work."""
    import torch
    from . import ops
    if layout not in ("padded", "packed"):
        raise ValueError(f"read_point_clouds: layout must be 'padded' or 'packed', got {layout!r}")
    paths = [str(p) for p in paths]
    if not paths:
        raise ValueError("read_point_clouds: at least one file is expected")
    table = scan_point_clouds(paths, threads) if table is None else np.array(table, dtype=np.int64, order="C")
    if table.shape != (len(paths), ROW) or (table[:, STATUS] != 0).any():
        raise ValueError("read_point_clouds: table must hold one good row of scan_point_clouds per path")
    B = len(paths)
    n = table[:, N_VERTEX].copy()
    dst_off, data_bytes = staging_offsets(table)
    if layout == "padded":
        n_max = int(n.max())
        dst_row, cap, rows = np.arange(B, dtype=np.int64) * n_max, np.full(B, n_max, dtype=np.int64), B * n_max
    else:
        end = np.cumsum(n)
        dst_row, cap, rows = end - n, n, int(end[-1])
    # tail of the staging buffer: the kernel's table, the packed layout's offsets, the tile prefix
    t0 = data_bytes
    t1 = t0 + 8 * 12 * B
    t2 = t1 + 8 * (B + 1)
    total = (t2 + 4 * (B + 1) + 15) // 16 * 16
    host = _staging.take(total)
    load_point_clouds(paths, table, host[:data_bytes], dst_off, threads)          # may rewrite the rows of ASCII files
    dev, prefix = device_tables(table, dst_off, dst_row, cap)
    view = host.numpy()
    view[t0:t1] = dev.view(np.uint8).reshape(-1)
    view[t1:t2] = np.concatenate([[0], np.cumsum(n)]).astype(np.int64).view(np.uint8)
    view[t2:t2 + 4 * (B + 1)] = prefix.view(np.uint8)
    on_dev = torch.empty(total, dtype=torch.uint8, device=device)
    with torch.cuda.device(on_dev.device):
        on_dev.copy_(host, non_blocking=True)
        _staging.mark()
        if out is None:
            out = torch.empty(rows, 3, dtype=torch.float32, device=device)
        elif tuple(out.shape) != (rows, 3) or out.dtype != torch.float32 or out.device != on_dev.device:
            raise ValueError(f"read_point_clouds: out must be a float32 tensor of ({rows}, 3) on {on_dev.device}")
        ops.ply_unpack(on_dev[:data_bytes], on_dev[t0:t1].view(torch.int64).view(B, 12), on_dev[t2:t2 + 4 * (B + 1)].view(torch.int32), out,
                       total_tiles=int(prefix[-1]))
        if layout == "padded":
            return out.view(B, -1, 3), [int(v) for v in n]
        return out, on_dev[t1:t2].view(torch.int64).clone(), [int(v) for v in n]


def save_point_clouds(rows, counts, directory, names, suffix=".ply", threads=0, first_rows=None):
    """save_point_cloud for a batch: rows = the device tensor a decoder produced, (B, N, 3) with cloud b in the first counts[b] rows of
    slab b, or (M, 3) with the clouds one behind the other (first_rows: where each begins, for any other arrangement).  ONE
    device-to-host copy into pinned memory, then <directory>/<names[b]><suffix> written by the library's host threads
    (pccx_ply_write_host): the bytes of save_point_cloud.
    rows may also be a list of B contiguous (n_b, 3) tensors, as decompress_ragged returns them and as the rows of decompress's slab
    are (counts may then be None): tensors that are views of one allocation are copied together, the span they cover once and as it
    lies -- no gathering copy on the device -- so the call makes one device-to-host copy per allocation."""
    import os
    import torch
    from . import _lib
    from .codec import _name_table
    if isinstance(rows, (list, tuple)):
        if len(rows) != len(names) or any(not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3
                                          or not t.is_contiguous() or t.storage_offset() % 3 for t in rows):
            raise ValueError(f"save_point_clouds: a list of {len(names)} contiguous float32 (n, 3) tensors is expected")
        groups = {}
        for b, t in enumerate(rows):
            groups.setdefault((t.device, t.untyped_storage().data_ptr()), []).append(b)
        for bs in groups.values():
            lo = min(rows[b].storage_offset() for b in bs)
            hi = max(rows[b].storage_offset() + rows[b].numel() for b in bs)
            span = torch.as_strided(rows[bs[0]], ((hi - lo) // 3, 3), (3, 1), lo)
            save_point_clouds(span, [rows[b].shape[0] for b in bs], directory, [names[b] for b in bs], suffix, threads,
                              [(rows[b].storage_offset() - lo) // 3 for b in bs])
        return
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.dim() not in (2, 3) or rows.shape[-1] != 3:
        raise ValueError("save_point_clouds: rows must be a float32 tensor of shape (B, N, 3) or (M, 3)")
    counts = np.asarray([int(c) for c in counts], dtype=np.int64)
    B = len(names)
    if counts.shape != (B,):
        raise ValueError(f"save_point_clouds: {B} names but {counts.shape[0]} counts")
    if first_rows is None:
        first_rows = np.arange(B, dtype=np.int64) * rows.shape[1] if rows.dim() == 3 else np.cumsum(counts) - counts
        if rows.dim() == 3 and rows.shape[0] != B:
            raise ValueError(f"save_point_clouds: {B} names but a slab of {rows.shape[0]} clouds")
    first_rows = np.ascontiguousarray(first_rows, dtype=np.int64)
    total = rows.numel() // 3
    if first_rows.shape != (B,) or (counts < 0).any() or (first_rows < 0).any() or (first_rows + counts > total).any():
        raise ValueError(f"save_point_clouds: the clouds' rows do not lie inside the {total} rows given")
    blob, off = _name_table(names)
    flat = rows.contiguous().view(-1)
    if flat.is_cuda:
        host = _writeback.take(4 * flat.numel()).view(torch.float32)
        with torch.cuda.device(flat.device):
            host.copy_(flat, non_blocking=True)
            torch.cuda.current_stream().synchronize()
    else:
        host = flat
    if B:
        _lib.call("pccx_ply_write_host", host.data_ptr(), total, first_rows.ctypes.data, counts.ctypes.data, B, os.fsencode(directory), blob,
                  off.ctypes.data, os.fsencode(suffix), int(threads))
