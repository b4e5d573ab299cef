"""PLY files for the tests of the batch reader (tests/test_ply_host_cpu.py, tests/test_ply_unpack.py, tests/test_cli_ply_io.py), written
with numpy alone; the oracle of every test is plyio.read_point_cloud / plyio.save_point_cloud on the same files."""
import numpy as np

LE, BE, ASCII = "binary_little_endian", "binary_big_endian", "ascii"

# vertex layouts by record stride: extra properties in front of, between and behind the coordinates, x y z in any order, and between
# them every one of the eight scalar types as a coordinate
LAYOUTS = {
    7: [("x", "i2"), ("y", "u1"), ("z", "f4")],
    9: [("q", "u1"), ("x", "i1"), ("y", "i2"), ("z", "i4"), ("w", "u1")],
    12: [("x", "f4"), ("y", "f4"), ("z", "f4")],
    15: [("x", "f4"), ("red", "u1"), ("y", "f4"), ("green", "u1"), ("z", "f4"), ("blue", "u1")],
    24: [("x", "f8"), ("y", "f8"), ("z", "f8")],
    27: [("x", "f8"), ("y", "f8"), ("z", "f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1")],
    300: [(f"pad{i}", "f8") for i in range(36)] + [("z", "i4"), ("s", "i1"), ("y", "u4"), ("x", "u2"), ("t", "i1")],
}
PLY_NAME = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float", "f8": "double"}
ALT_NAME = {"i1": "int8", "u1": "uint8", "i2": "int16", "u2": "uint16", "i4": "int32", "u4": "uint32", "f4": "float32", "f8": "float64"}
CODE = {"i1": 0, "u1": 1, "i2": 2, "u2": 3, "i4": 4, "u4": 5, "f4": 6, "f8": 7}


def stride_of(layout):
    return sum(np.dtype(t).itemsize for _, t in layout)


def values(t, n, rng, text):
    """n values of type t: integers over their whole range; float32 as random BIT PATTERNS in a binary file (NaN payloads, infinities
    and subnormals among them), decimal-friendly numbers in a text file; float64 finite and inside float32's range."""
    if t[0] in "iu":
        info = np.iinfo(t)
        return rng.integers(info.min, info.max, n, dtype=np.int64 if t != "u4" else np.uint64, endpoint=True).astype(t)
    if t == "f4" and not text:
        return rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(t)


def header(fmt, n, layout, upper=False, crlf=False, comments=False, faces=False, alt_names=False):
    names = ALT_NAME if alt_names else PLY_NAME
    lines = ["ply", f"format {fmt} 1.0"]
    if comments:
        lines += ["comment written by the test suite", "obj_info  anything", ""]
    lines += [f"element vertex {n}"]
    lines += [f"property {names[t]} {nm.upper() if upper and nm in 'xyz' else nm}" for nm, t in layout]
    if comments:
        lines += ["comment between the elements"]
    if faces:
        lines += ["element face 1", "property list uchar int vertex_indices"]
    lines += ["end_header"]
    return ("\r\n" if crlf else "\n").join(lines).encode() + (b"\r\n" if crlf else b"\n")


def write_ply(path, layout, n, fmt, seed, rec=None, **how):
    """One file; returns (header bytes, vertex block bytes).  rec: a structured array of the layout's fields to write instead of random
    values (native byte order)."""
    rng = np.random.default_rng(seed)
    if rec is None:
        rec = np.zeros(n, dtype=np.dtype([(nm, t) for nm, t in layout]))
        for nm, t in layout:
            rec[nm] = values(t, n, rng, fmt == ASCII)
    head = header(fmt, n, layout, **how)
    if fmt == ASCII:
        eol = "\r\n" if how.get("crlf") else "\n"
        body = "".join(" ".join(repr(float(r[nm])) if t[0] == "f" else str(int(r[nm])) for nm, t in layout) + eol for r in rec).encode()
        tail = b"3 0 0 0\n" if how.get("faces") else b""
    else:
        end = "<" if fmt == LE else ">"
        body = rec.astype(np.dtype([(nm, end + t) for nm, t in layout])).tobytes()
        tail = b"\x03" + bytes(12) if how.get("faces") else b""
    with open(path, "wb") as f:
        f.write(head + body + tail)
    return head, body


def expected_row(fmt, n, layout, head, size):
    """The scan's table row of a file written by write_ply"""
    off, o = {}, 0
    for nm, t in layout:
        off[nm] = (o, CODE[t])
        o += np.dtype(t).itemsize
    names = [nm for nm, _ in layout]
    return ([0, {ASCII: 0, LE: 1, BE: 2}[fmt], n, o, len(head), size] + [off[c][0] for c in "xyz"] + [off[c][1] for c in "xyz"] +
            [len(layout)] + [names.index(c) for c in "xyz"])
