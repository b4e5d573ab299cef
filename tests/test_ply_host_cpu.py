"""CPU: the PLY header parser (csrc/ply_host.h) and the host threads that scan, load and write PLY files (pccx_ply_scan_host /
pccx_ply_load_host / pccx_ply_write_host, csrc/hostio.hip; no GPU call) against plyio.read_point_cloud / plyio.save_point_cloud on
files written with numpy."""
import os
import subprocess
from decimal import Decimal

import numpy as np
import pytest
import torch

from pccx import _lib, plyio
from tests import ply_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-compression_amd", "csrc")
GAP = 48                                  # guard bytes in front of, between and behind the files' ranges of a staging buffer


@pytest.fixture(scope="module")
def pool(tmp_path_factory):
    """3 formats x 7 layouts x n = 1, 2, 257, with upper-case names, comments and a blank line, \\r\\n line ends, a face element and the
    second set of type names in turn -> list of (path, format, n, layout, header bytes, vertex block bytes)"""
    d = tmp_path_factory.mktemp("pool")
    out, i = [], 0
    for fmt in (pc.ASCII, pc.LE, pc.BE):
        for stride, layout in pc.LAYOUTS.items():
            for n in (1, 2, 257):
                path = str(d / f"{fmt}_{stride}_{n}.ply")
                head, body = pc.write_ply(path, layout, n, fmt, 1000 + i, upper=i % 2 == 1, comments=i % 3 == 1, crlf=i % 4 == 2, faces=i % 5 == 3,
                                          alt_names=i % 7 == 4)
                out.append((path, fmt, n, layout, head, body))
                i += 1
    assert {pc.stride_of(f[3]) for f in out} == {7, 9, 12, 15, 24, 27, 300}
    return out


def guarded(table, gap=GAP):
    """(staging (uint8 array at a multiple of 16, filled with 0xA5), dst_off): every file's range with `gap` guard bytes around it"""
    size = (plyio.block_bytes(table) + 15) // 16 * 16
    off = np.cumsum(size + gap) - size
    raw = np.full(int(off[-1] + size[-1]) + gap + 16, 0xA5, dtype=np.uint8)
    return raw[(-raw.ctypes.data) % 16:][:int(off[-1] + size[-1]) + gap], off.astype(np.int64)


def guards_intact(staging, table, off, written):
    """no byte outside the files' own ranges changed; written[b]: how many bytes of file b's range may differ from the fill"""
    mask = np.ones(staging.shape[0], dtype=bool)
    for o, w in zip(off.tolist(), written):
        mask[o:o + int(w)] = False
    return bool((staging[mask] == 0xA5).all())


@pytest.mark.parametrize("B,threads", [(1, 1), (37, 3), (300, 0), (63, 1), (63, 3), (63, 0)])
def test_scan_and_load_equal_the_files_and_the_python_reader(pool, B, threads):
    files = [pool[(5 * i) % len(pool)] for i in range(B)] if B != 63 else pool
    paths = [f[0] for f in files]
    table = plyio.scan_point_clouds(paths, threads)
    for row, (path, fmt, n, layout, head, body) in zip(table.tolist(), files):
        assert row == pc.expected_row(fmt, n, layout, head, os.path.getsize(path)), path
    staging, off = guarded(table)
    want_bytes = plyio.block_bytes(table).copy()
    plyio.load_point_clouds(paths, table, staging, off, threads)
    for b, (path, fmt, n, layout, head, body) in enumerate(files):
        got = staging[off[b]:off[b] + want_bytes[b]].tobytes()
        if fmt == pc.ASCII:
            assert got == plyio.read_point_cloud(path).tobytes(), path
            assert table[b].tolist()[:12] == [0, plyio.LITTLE, n, 12, len(head), os.path.getsize(path), 0, 4, 8, 6, 6, 6], path
        else:
            assert got == body, path
    assert guards_intact(staging, table, off, want_bytes)


def double_rounding_tokens():
    """Decimal strings just above the middle of two neighbouring float32 whose lower one is even: to double they round onto the middle,
    from there to the even neighbour BELOW, while one rounding from the text gives the neighbour ABOVE.  -> [(token, two-step, direct)]"""
    out = []
    for a in (np.float32(1.0), np.float32(0.1), np.float32(123456.0), np.float32(3.0e-5), np.float32(-7.25)):
        a = a if int(a.view(np.uint32)) % 2 == 0 else np.nextafter(a, np.float32(np.inf) * np.sign(a))
        b = np.nextafter(a, np.float32(np.inf) * np.sign(a))                     # away from zero
        mid = (Decimal(float(a)) + Decimal(float(b))) / 2
        tok = format(mid * (1 + Decimal(10) ** -25), "f")
        direct = b if abs(Decimal(tok) - Decimal(float(b))) < abs(Decimal(tok) - Decimal(float(a))) else a
        out.append((tok, np.float32(np.float64(tok)), direct))
    return out


@pytest.mark.filterwarnings("ignore")              # loadtxt on the blank line, astype on 1e39
def test_ascii_tokens_round_twice_as_loadtxt_does(tmp_path):
    tokens = double_rounding_tokens()
    for tok, two_step, direct in tokens:                                       # the case is real: the two rules differ on these strings
        assert two_step.view(np.uint32) != direct.view(np.uint32), tok
    special = ["1e3", "-2.5E-3", "+4.75", "+1e+2", "inf", "-inf", "nan", "+inf", "Infinity", "1e-50", "1e39", "-1e39", "1e-400", "1e400", ".5", "5.",
               "0.000000000000000000000000000000000000000000001", "16777217", "-0"]
    toks = [t for t, _, _ in tokens] + special
    toks += ["0"] * (-len(toks) % 3)
    rows = [toks[i:i + 3] for i in range(0, len(toks), 3)]
    path = str(tmp_path / "tokens.ply")
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(rows)}\nproperty double x\nproperty uchar r\nproperty double y\nproperty double z\nend_header\n")
        for i, r in enumerate(rows):
            f.write(f"{r[0]} {i}\t{r[1]}   {r[2]}\n" + ("\n" if i == 1 else "") + ("# a comment line\n" if i == 2 else ""))
    want = plyio.read_point_cloud(path)
    flat = want.reshape(-1)
    for i, (tok, two_step, direct) in enumerate(tokens):
        assert flat[i].view(np.uint32) == two_step.view(np.uint32)
    table = plyio.scan_point_clouds([path])
    staging, off = guarded(table)
    plyio.load_point_clouds([path], table, staging, off)
    got = staging[off[0]:off[0] + 12 * len(rows)]
    w = want.view(np.uint32).reshape(-1)
    g = got.view(np.uint32)
    nan = np.isnan(flat)
    assert nan.sum() == 1 and np.isnan(got.view(np.float32)[nan]).all() and (g[~nan] == w[~nan]).all(), (g, w)
    assert guards_intact(staging, table, off, [12 * len(rows)])


@pytest.mark.parametrize("lines,least", [(400, 4096), (900, 16384)])
def test_headers_longer_than_the_scan_first_reads(tmp_path, lines, least):
    """The scan reads 4 KiB of a file, then 16 KiB, then more: headers above both sizes, shifted byte by byte by a comment so that the
    cut sweeps a whole property line (through `property`, the type and the name), read as read_point_cloud reads them"""
    layout = [(f"p{i}", "u1") for i in range(lines)]
    layout[lines // 2:lines // 2] = [("x", "f4"), ("y", "f8"), ("z", "i2")]
    paths, want = [], []
    for shift in range(0, 26):
        rng = np.random.default_rng(shift)
        rec = np.zeros(3, dtype=np.dtype(layout))
        for nm, t in layout:
            rec[nm] = pc.values(t, 3, rng, False)
        head = pc.header(pc.LE, 3, layout).replace(b"element vertex", b"comment " + b"c" * shift + b"\nelement vertex")
        assert len(head) > least + 64
        paths.append(str(tmp_path / f"long_{shift}.ply"))
        open(paths[-1], "wb").write(head + rec.tobytes())
        want.append((len(head), rec.tobytes()))
    table = plyio.scan_point_clouds(paths, 3)
    assert table[:, plyio.STRIDE].tolist() == [lines + 14] * len(paths) and table[:, plyio.DATA_OFFSET].tolist() == [w[0] for w in want]
    staging, off = guarded(table)
    plyio.load_point_clouds(paths, table, staging, off)
    for b, path in enumerate(paths):
        assert staging[off[b]:off[b] + 3 * (lines + 14)].tobytes() == want[b][1]
        cloud = plyio.read_point_cloud(path)
        mid = lines // 2
        got = np.frombuffer(want[b][1], dtype=np.dtype(layout))
        assert np.array_equal(cloud.view(np.uint32), np.stack([got["x"], got["y"].astype(np.float32), got["z"].astype(np.float32)], axis=1).view(np.uint32)), mid


HEAD = "ply\nformat binary_little_endian 1.0\n"
XYZ = "property float x\nproperty float y\nproperty float z\n"
REFUSALS = {
    "not_ply": (b"plx\nformat ascii 1.0\nelement vertex 1\n" + XYZ.encode() + b"end_header\n0 0 0\n", "not a PLY"),
    "truncated": ((HEAD + "element vertex 1\n" + XYZ).encode(), "truncated header"),
    "format": (("ply\nformat binary_middle_endian 1.0\nelement vertex 1\n" + XYZ + "end_header\n").encode() + bytes(12), "format"),
    "type": ((HEAD + "element vertex 1\nproperty half x\nproperty float y\nproperty float z\nend_header\n").encode() + bytes(12), "type"),
    "list": ((HEAD + "element vertex 1\n" + XYZ + "property list uchar int k\nend_header\n").encode() + bytes(32), "list property"),
    "coordinate": ((HEAD + "element vertex 1\nproperty float x\nproperty float y\nend_header\n").encode() + bytes(12), "no x, y and z"),
    "no_vertex": ((HEAD + "element face 1\nproperty list uchar int vertex_indices\nend_header\n").encode() + bytes(13), "no vertex element"),
    "order": ((HEAD + "element face 1\nproperty list uchar int vertex_indices\nelement vertex 1\n" + XYZ + "end_header\n").encode() + bytes(25), "in front of vertex"),
    "zero": ((HEAD + "element vertex 0\n" + XYZ + "end_header\n").encode(), "vertex count"),
    "huge": ((HEAD + "element vertex 2147483648\n" + XYZ + "end_header\n").encode() + bytes(12), "vertex count"),
    "stride": ((HEAD + "element vertex 1\n" + XYZ + "".join(f"property double p{i}\n" for i in range(511)) + "end_header\n").encode() + bytes(4100), "4096"),
    "size": ((HEAD + "element vertex 3\n" + XYZ + "end_header\n").encode() + bytes(35), "too short"),
    "ascii_rows": (("ply\nformat ascii 1.0\nelement vertex 3\n" + XYZ + "end_header\n1.25 2.5 3.75\n4.0 5.0 6.0\n# no third row\n\n").encode(), "ASCII"),
}


def test_refused_files_are_all_named_and_the_good_ones_still_read(tmp_path, pool):
    bad = {}
    for name, (data, _) in REFUSALS.items():
        bad[name] = str(tmp_path / (name + ".ply"))
        open(bad[name], "wb").write(data)
    bad["missing"] = str(tmp_path / "no such file.ply")
    bad["directory"] = str(tmp_path)
    causes = dict({k: v[1] for k, v in REFUSALS.items()}, missing="No such file", directory="not a regular file")
    good = [f for f in pool if f[2] == 257][:len(bad) + 1]
    paths, kind = [], []
    for i, g in enumerate(good):                                               # good and bad files in turn
        paths.append(g[0]), kind.append(None)
        if i < len(bad):
            paths.append(list(bad.values())[i]), kind.append(list(bad)[i])
    for threads in (1, 0):
        table, msgs = plyio.scan_point_clouds(paths, threads, check=False)
        staging, off = guarded(table)
        want_bytes = plyio.block_bytes(table).copy()
        msgs2 = plyio.load_point_clouds(paths, table, staging, off, threads, check=False)
        gi = 0
        for b, k in enumerate(kind):
            text = (bytes(msgs[b]) + bytes(msgs2[b])).replace(bytes(1), b" ").decode()
            if k is None:
                path, fmt, n, layout, head, body = good[gi]
                gi += 1
                assert table[b, 0] == 0 and table[b, plyio.N_VERTEX] == n
                got = staging[off[b]:off[b] + want_bytes[b]].tobytes()
                assert got == (plyio.read_point_cloud(path).tobytes() if fmt == pc.ASCII else body), path
            else:
                assert table[b, 0] != 0 and causes[k] in text, (k, table[b, 0], text)
        assert guards_intact(staging, table, off, want_bytes)
    # the raising form names every bad path, with its cause, in one ValueError
    with pytest.raises(ValueError) as e:
        plyio.scan_point_clouds(paths)
    for k, p in bad.items():
        if k != "ascii_rows":                                                  # its header is good: refused by the load
            assert f"{p}: " in str(e.value) and causes[k] in str(e.value), k
    assert not any(g[0] + ": " in str(e.value) for g in good)
    ok = [p for p, k in zip(paths, kind) if k in (None, "ascii_rows")]
    table = plyio.scan_point_clouds(ok)
    staging, off = guarded(table)
    with pytest.raises(ValueError, match="ascii_rows.ply: fewer complete ASCII rows"):
        plyio.load_point_clouds(ok, table, staging, off)
    # a range that does not hold its file, or is not 16-byte aligned, is refused by name too, and nothing is written
    staging, off = guarded(table)
    msgs = plyio.load_point_clouds(ok[:1], table[:1].copy(), staging[:32], off[:1] * 0, check=False)
    assert b"does not hold" in bytes(msgs[0])
    msgs = plyio.load_point_clouds(ok[:1], table[:1].copy(), staging, off[:1] * 0 + 8, check=False)
    assert b"not 16-byte aligned" in bytes(msgs[0])
    assert (staging == 0xA5).all()


def test_a_property_name_declared_twice_is_read_as_the_python_reader_reads_it(tmp_path):
    """ASCII: read_point_cloud takes the first column of a name, and so does the scan; binary: its structured dtype refuses the file"""
    props = "property float q\nproperty float x\nproperty float y\nproperty float q\nproperty float z\n"
    a, b = str(tmp_path / "dup_ascii.ply"), str(tmp_path / "dup_binary.ply")
    open(a, "w").write("ply\nformat ascii 1.0\nelement vertex 2\n" + props + "end_header\n9 1 2 8 3\n9 4.5 5 8 nan\n")
    open(b, "wb").write((HEAD + "element vertex 1\n" + props + "end_header\n").encode() + bytes(20))
    table, msgs = plyio.scan_point_clouds([a, b], check=False)
    assert table[:, 0].tolist() == [0, 12] and b"declared twice" in bytes(msgs[1])
    with pytest.raises(ValueError):
        plyio.read_point_cloud(b)
    staging, off = guarded(table[:1])
    plyio.load_point_clouds([a], table[:1].copy(), staging, off)
    want = plyio.read_point_cloud(a)
    assert np.array_equal(staging[off[0]:off[0] + 24].view(np.float32).reshape(2, 3), want, equal_nan=True) and want[0].tolist() == [1, 2, 3]
    # nan(...) is a number to from_chars and none to Python's float: refused, as np.loadtxt refuses it
    open(a, "w").write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2 nan(7)\n")
    with pytest.raises(ValueError):
        plyio.read_point_cloud(a)
    table = plyio.scan_point_clouds([a])
    with pytest.raises(ValueError, match="no number"):
        plyio.load_point_clouds([a], table, *guarded(table))


def test_writer_equals_save_point_cloud(tmp_path):
    rng = np.random.default_rng(5)
    slab = torch.from_numpy(rng.standard_normal((3, 9000, 3)).astype(np.float32))
    slab[1, 7, 2] = float("nan")
    counts, names = [1, 128, 8192], ["a.b c.ply", "second cloud", "x.y.z"]
    ours, ref = tmp_path / "ours", tmp_path / "ref"
    ours.mkdir(), ref.mkdir()
    (ours / "second cloud.ply").write_bytes(b"old content " * 4000)              # an existing, longer file is replaced
    for threads in (1, 0):
        plyio.save_point_clouds(slab, counts, str(ours), names, threads=threads)
    for b, n in enumerate(names):
        plyio.save_point_cloud(slab[b, :counts[b]].numpy(), str(ref / (n + ".ply")))
        assert (ours / (n + ".ply")).read_bytes() == (ref / (n + ".ply")).read_bytes(), n
        assert np.array_equal(plyio.read_point_cloud(str(ours / (n + ".ply"))), slab[b, :counts[b]].numpy(), equal_nan=True)
    assert sorted(os.listdir(ours)) == sorted(os.listdir(ref))
    # the packed arrangement and another suffix
    packed = torch.cat([slab[b, :c] for b, c in enumerate(counts)])
    plyio.save_point_clouds(packed, counts, str(ours), names, suffix=".bin.ply", threads=3)
    for b, n in enumerate(names):
        assert (ours / (n + ".bin.ply")).read_bytes() == (ref / (n + ".ply")).read_bytes()
    # a list of views, as the decoders hand them out: rows of one slab in any order beside a tensor of its own
    own = torch.from_numpy(rng.standard_normal((5, 3)).astype(np.float32))
    views, vnames = [slab[2, :8192], own, slab[0, :1], slab[1, :128]], ["v2", "own", "v0", "v1"]
    plyio.save_point_clouds(views, None, str(ours), vnames, suffix=".v.ply")
    for t, n in zip(views, vnames):
        plyio.save_point_cloud(t.numpy(), str(tmp_path / "one.ply"))
        assert (ours / (n + ".v.ply")).read_bytes() == (tmp_path / "one.ply").read_bytes(), n
    with pytest.raises(ValueError, match="contiguous"):
        plyio.save_point_clouds([slab[:, 0]], None, str(ours), ["t"])
    plyio.release_pinned()                                                       # nothing held on a machine without a GPU: a no-op
    for threads in (0, 3, 1, 0, 3, 0):                                           # every open fails at once: the lowest cloud's is the one named
        with pytest.raises(_lib.PccxError, match="no such dir/a.b c.ply.ply"):
            plyio.save_point_clouds(slab, counts, str(tmp_path / "no such dir"), names, threads=threads)
    with pytest.raises(ValueError, match="rows"):
        plyio.save_point_clouds(slab, [1, 128, 9001], str(ours), names)
    with pytest.raises(ValueError):
        plyio.save_point_clouds(slab, counts, str(ours), ["a/b", "c", "d"])


MAIN = r"""
#include "ply_host.h"
#include <stdlib.h>
#include <string>
// Seeded mutations of valid headers, each in a heap block of exactly its length (the sanitizer sees any byte read past it): every case
// must come back accepted or refused, and an accepted one must describe records the caller can trust.
static unsigned long long state = 88172645463325252ull;
static unsigned rnd(unsigned n) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (unsigned)(state % n); }
static const char *types[16] = {"char", "int8", "uchar", "uint8", "short", "int16", "ushort", "uint16", "int", "int32", "uint", "uint32",
                                "float", "float32", "double", "float64"};
int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 1000;
    int ok = 0, refused = 0;
    for (int r = 0; r < rounds; ++r) {
        std::string h = "ply\n";
        const char *fmts[3] = {"ascii", "binary_little_endian", "binary_big_endian"};
        h += std::string("format ") + fmts[rnd(3)] + " 1.0" + (rnd(4) ? "\n" : "\r\n");
        if (rnd(3) == 0) h += "comment hello world\n\n";
        const int mode = rnd(10);
        if (mode == 8) h += "element vertex 99999999999999999999999\n";              // a huge count
        else if (mode == 9) h += "element vertex 2147483647\n";
        else h += "element vertex " + std::to_string(1 + rnd(50)) + "\n";
        const int extra = mode == 7 ? 1000 + (int)rnd(4000) : (int)rnd(12);          // thousands of properties
        const int at = (int)rnd((unsigned)extra + 1);
        const bool upper = rnd(2);
        for (int i = 0; i <= extra; ++i) {
            if (i == at) {
                h += std::string("property ") + types[rnd(16)] + (upper ? " X\n" : " x\n");
                h += std::string("property ") + types[rnd(16)] + (upper ? " Y\n" : " y\n");
                h += std::string("property ") + types[rnd(16)] + (rnd(8) ? (upper ? " Z\n" : " z\n") : " w\n");
            }
            if (i < extra) h += std::string("property ") + (mode == 7 ? "uchar" : types[rnd(16)]) + " p" + std::to_string(i) + "\n";
        }
        if (rnd(4) == 0) h += "element face 3\nproperty list uchar int vertex_indices\n";
        h += rnd(6) ? "end_header\n" : "end_header";                                 // no newline at the end of the buffer
        std::string body(rnd(64), 'x');
        std::string all = h + (h.back() == '\n' ? body : "");
        size_t n = all.size();
        const int mut = rnd(5);
        if (mut == 1) n = rnd((unsigned)n + 1);                                       // truncated anywhere
        if (mut == 2) for (int k = 1 + (int)rnd(3); k > 0; --k) all[rnd((unsigned)all.size())] ^= (char)(1u << rnd(8));   // bits flipped
        if (mut == 3) all[rnd((unsigned)all.size())] = (char)rnd(256);
        uint8_t *arg = (uint8_t *)malloc(n ? n : 1);
        memcpy(arg, all.data(), n);
        PlyHeader ph;
        char msg[64];
        const int64_t file_size = rnd(3) == 0 ? -1 : (int64_t)n + (rnd(2) ? 0 : (int64_t)rnd(100000));
        const int st = ply_parse_header(arg, n, file_size, &ph, msg, sizeof(msg));
        if (st < PLY_OK || st > PLY_MALFORMED) return 2;
        if (st == PLY_OK) {
            if (ph.n_vertex < 1 || ph.n_vertex > PLY_MAX_VERTICES || ph.stride < 1 || ph.stride > PLY_MAX_STRIDE) return 3;
            if (ph.data_offset < 0 || (size_t)ph.data_offset > n) return 4;
            for (int c = 0; c < 3; ++c) {
                if (ph.off[c] < 0 || ply_type_size(ph.type[c]) == 0 || ph.off[c] + ply_type_size(ph.type[c]) > ph.stride) return 5;
                if (ph.col[c] < 0 || ph.col[c] >= ph.n_props) return 6;
            }
            if (file_size >= 0 && ph.format != PLY_ASCII && ph.data_offset + ph.n_vertex * ph.stride > file_size) return 7;
            if (msg[0]) return 8;
            ++ok;
        } else {
            if (!msg[0] || ph.n_vertex != 0 || ph.stride != 0) return 9;           // a cause is named, nothing half-filled is handed out
            ++refused;
        }
        // a prefix of the file, cut anywhere: "hand me more" or the verdict on the whole, never a verdict on half a line
        PlyHeader whole, part;
        const int full = ply_parse_header(arg, n, (int64_t)n, &whole, msg, sizeof(msg));
        const size_t cut = rnd((unsigned)n + 1);
        const int pre = ply_parse_header(arg, cut, (int64_t)n, &part, msg, sizeof(msg));
        if (cut < n && pre != PLY_TRUNCATED && (pre != full || memcmp(&part, &whole, sizeof(part)) != 0)) return 12;
        free(arg);
        // the text side: a random token, and random rows, in blocks of their exact length
        const char alphabet[] = "0123456789+-.eEinfa #\n\t";
        const size_t tn = rnd(24);
        uint8_t *tok = (uint8_t *)malloc(tn ? tn : 1);
        for (size_t i = 0; i < tn; ++i) tok[i] = (uint8_t)alphabet[rnd(sizeof(alphabet) - 1)];
        double v;
        (void)ply_token_to_double(tok, tn, &v);
        PlyHeader th;
        memset(&th, 0, sizeof(th));
        th.n_vertex = 1 + rnd(3), th.n_props = 3, th.col[0] = 2, th.col[1] = 0, th.col[2] = 1;
        float out[9];
        const int ts = ply_parse_ascii_rows(tok, tn, th, out, msg, sizeof(msg));
        if (ts != PLY_OK && ts != PLY_ROWS) return 10;
        free(tok);
    }
    printf("ok %d refused %d\n", ok, refused);
    return ok > 0 && refused > 0 ? 0 : 11;
}
"""


def test_ply_header_parser_alone_under_sanitizers(tmp_path):
    """csrc/ply_host.h is plain C++ with no dependency: a stand-alone host program that includes nothing else of the project, built with
    the address and undefined-behaviour sanitizers, runs the parser over 20 000 seeded mutations of valid headers -- truncations, flipped
    bits, huge counts, thousands of properties, a missing newline at the end of the buffer."""
    src, exe = tmp_path / "ply_host_main.cc", tmp_path / "ply_host_main"
    src.write_text(MAIN)
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ")
