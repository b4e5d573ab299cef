"""CPU: the mesh sampler's restatement (tests/mesh_cases.py) against its known answers, the OFF parser (csrc/off_host.h) and the host
threads that scan and load OFF files (pccx_off_scan_host / pccx_off_load_host, csrc/hostio.hip; no GPU call) against meshes.read_off."""
import itertools
import os
import subprocess
from decimal import Decimal

import numpy as np
import pytest

from pccx import _lib, meshes
from tests import mesh_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-compression_amd", "csrc")
MASK = 0xFFFFFFFF
GAP = 48                                  # guard bytes in front of, between and behind the ranges of a staging buffer


def test_philox_known_answers():
    hexs = lambda t: " ".join("%08x" % v for v in t)
    assert hexs(mc.philox((0, 0), (0, 0, 0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexs(mc.philox((MASK, MASK), (MASK,) * 4)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexs(mc.philox((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # the vectorised form the samples come from is the same function: key = the seed's halves, counter = (i, 0, 0, 0)
    seed = 0x299f31d0a4093822
    x = mc.philox_stream(seed, 300)
    for i in (0, 1, 255, 299):
        assert tuple(x[i].tolist()) == mc.philox((0xa4093822, 0x299f31d0), (i, 0, 0, 0))


def test_selection_is_area_weighted_and_never_draws_a_face_without_area():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 4, 0], [0, 6, 0], [0, 8, 0], [2, 0, 0]], dtype=np.float32)
    F = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 5], [0, 1, 6]], dtype=np.int32)     # areas 1 : 2 : 3 : 4 : 0
    n = 65536
    a, w, I, status = mc.weights(V, F)
    assert status == 0 and a.tolist() == [1, 2, 3, 4, 0] and w.tolist() == [2**38, 2**39, 3 * 2**38, 2**40, 0]
    _, _, t = mc.sample(V, F, 11, n, None)                                                    # key (11, 0)
    got = np.bincount(t, minlength=5)
    print("counts", got.tolist())
    assert got[4] == 0 and got.sum() == n
    p = w.astype(np.float64) / float(I[-1])
    sigma = np.sqrt(n * p * (1 - p))
    dev = np.abs(got[:4] - n * p[:4]) / sigma[:4]
    print("deviations in sigma", dev.tolist())
    assert (dev < 6).all()
    assert got.tolist() == [6658, 13177, 19687, 26014, 0]                                     # the restatement is a fixed function


SIZES = ((3, 1), (4, 2), (300, 257), (5000, 4097))
SWITCHES = ("glued", "comments", "crlf", "colours", "blanks")


@pytest.fixture(scope="module")
def pool(tmp_path_factory):
    """every combination of the writer's five switches, the four sizes in turn -> [(path, V, F)]"""
    d = tmp_path_factory.mktemp("off_pool")
    rng = np.random.default_rng(3)
    shapes = {}
    for nv, nf in SIZES:
        V = (rng.standard_normal((nv, 3)) * 10).astype(np.float32)
        shapes[(nv, nf)] = (V, rng.integers(0, nv, (nf, 3)).astype(np.int32))
    out = []
    for i, sw in enumerate(itertools.product((False, True), repeat=len(SWITCHES))):
        for j, size in enumerate(SIZES):
            if size[0] > 300 and i % 8 != j:                 # the large mesh with four of the 32 combinations, which between them flip every switch
                continue
            V, F = shapes[size]
            path = str(d / f"m{i}_{size[1]}.off")
            mc.write_off(path, V, F, final_newline=(i + j) % 3 != 0, **dict(zip(SWITCHES, sw)))
            out.append((path, V, F))
    return out


def guarded(table, gap=GAP):
    """(staging (uint8 array at a multiple of 16, filled with 0xA5), v_dst, f_dst): per file its vertex range and then its face range,
    `gap` guard bytes around each"""
    size = np.stack([12 * table[:, meshes.NV], 12 * table[:, meshes.NF]], axis=1).reshape(-1)
    off = np.cumsum(size + gap) - size
    total = int(off[-1] + size[-1]) + gap
    raw = np.full(total + 16, 0xA5, dtype=np.uint8)
    return raw[(-raw.ctypes.data) % 16:][:total], off[0::2].astype(np.int64), off[1::2].astype(np.int64)


def guards_intact(staging, ranges):
    mask = np.ones(staging.shape[0], dtype=bool)
    for o, w in ranges:
        mask[int(o):int(o) + int(w)] = False
    return bool((staging[mask] == 0xA5).all())


@pytest.mark.parametrize("threads", [1, 3, 0])
def test_scan_and_load_equal_read_off(pool, threads):
    paths = [p for p, _, _ in pool]
    table = meshes.scan_meshes(paths, threads)
    staging, v_dst, f_dst = guarded(table)
    meshes.load_meshes(paths, table, staging, v_dst, f_dst, threads)
    ranges = []
    for b, (path, V, F) in enumerate(pool):
        rv, rf = meshes.read_off(path)
        assert rv.tobytes() == V.tobytes() and rf.tobytes() == F.tobytes(), path       # the writer's texts read back as the float32 they came from
        assert table[b, :3].tolist() == [0, len(V), len(F)] and table[b, meshes.FILE_SIZE] == os.path.getsize(path)
        assert staging[v_dst[b]:v_dst[b] + 12 * len(V)].tobytes() == rv.tobytes(), path
        assert staging[f_dst[b]:f_dst[b] + 12 * len(F)].tobytes() == rf.tobytes(), path
        ranges += [(v_dst[b], 12 * len(V)), (f_dst[b], 12 * len(F))]
    assert guards_intact(staging, ranges)
    # the packed form read_meshes uses: all vertices, then all faces, nothing between them
    v_dst, f_dst, total = meshes.staging_offsets(table)
    packed = np.full(total, 0xA5, dtype=np.uint8)
    meshes.load_meshes(paths, table, packed, v_dst, f_dst, threads)
    assert packed.tobytes() == b"".join(V.tobytes() for _, V, _ in pool) + b"".join(F.tobytes() for _, _, F in pool)


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


def test_coordinates_round_twice_as_read_off_does(tmp_path):
    tokens = double_rounding_tokens()
    for tok, two_step, direct in tokens:                                       # the case is real: the two rules differ on these strings
        assert two_step.view(np.uint32) != direct.view(np.uint32), tok
    toks = [t for t, _, _ in tokens] + ["1e3", "-2.5E-3", "+4.75", "+1e+2", "1e-50", "1e-400", ".5", "5.", "16777217", "-0", "3.4028234e38",
                                        "0.000000000000000000000000000000000000000000001"]
    toks += ["0"] * (-len(toks) % 3)
    rows = [toks[i:i + 3] for i in range(0, len(toks), 3)]
    path = str(tmp_path / "tokens.off")
    F = np.array([[0, 1, 2], [len(rows) - 1, 0, 1]], dtype=np.int32)
    open(path, "wb").write(mc.off_bytes(np.zeros((len(rows), 3), np.float32), F, tokens=rows, comments=True))
    V, F2 = meshes.read_off(path)
    flat = V.reshape(-1)
    for i, (tok, two_step, direct) in enumerate(tokens):
        assert flat[i].view(np.uint32) == two_step.view(np.uint32)
    table = meshes.scan_meshes([path])
    staging, v_dst, f_dst = guarded(table)
    meshes.load_meshes([path], table, staging, v_dst, f_dst)
    assert staging[v_dst[0]:v_dst[0] + 12 * len(rows)].tobytes() == V.tobytes()
    assert staging[f_dst[0]:f_dst[0] + 24].tobytes() == F.tobytes() == F2.tobytes()
    assert guards_intact(staging, [(v_dst[0], 12 * len(rows)), (f_dst[0], 24)])


TRI = "0 0 0\n1 0 0\n0 1 0\n"
REFUSALS = {                 # name -> (bytes, OffStatus, a piece of the cause, refused by the scan?)
    "not_off": (("OFX\n3 1 0\n" + TRI + "3 0 1 2\n").encode(), meshes.NOT_OFF, "not an OFF", True),
    "truncated_head": (b"# only a comment\nOFF\n", meshes.TRUNCATED, "truncated", True),
    "truncated_short": (("OFF\n300 1 0\n" + TRI + "3 0 1 2\n").encode(), meshes.TRUNCATED, "too short", True),
    "truncated_body": (("OFF\n4 2 0\n" + TRI + "0 0 1\n3 0 1 2\n# the second face is missing" + " " * 40 + "\n").encode(), meshes.TRUNCATED, "fewer face lines", False),
    "nv_small": (("OFF\n2 1 0\n" + TRI + "3 0 1 1\n").encode(), meshes.BAD_NV, "nv must be", True),
    "nv_huge": (("OFF2147483648 1 0\n" + TRI + "3 0 1 2\n").encode(), meshes.BAD_NV, "nv must be", True),
    "nf_zero": (("OFF\n3 0 0\n" + TRI).encode(), meshes.BAD_NF, "nf must be", True),
    "nf_huge": (("OFF\n3 4194305 0\n" + TRI + "3 0 1 2\n").encode(), meshes.BAD_NF, "nf must be", True),
    "quad": (("OFF\n4 2 0\n" + TRI + "1 1 0\n3 0 1 2\n4 0 1 3 2\n").encode(), meshes.NOT_TRIANGLE, "not a triangle", False),
    "index_high": (("OFF\n3 2 0\n" + TRI + "3 0 1 2\n3 0 1 3\n").encode(), meshes.BAD_INDEX, "outside 0 .. nv - 1", False),
    "index_negative": (("OFF\n3 2 0\n" + TRI + "3 0 1 2\n3 0 -1 2\n").encode(), meshes.BAD_INDEX, "outside 0 .. nv - 1", False),
    "coord_nan": (("OFF\n3 1 0\n0 0 0\n1 nan 0\n0 1 0\n3 0 1 2\n      \n").encode(), meshes.BAD_COORD, "not finite", False),
    "coord_inf": (("OFF\n3 1 0\n0 0 0\n1 0 1e39\n0 1 0\n3 0 1 2\n      \n").encode(), meshes.BAD_COORD, "not finite", False),
    "coord_text": (("OFF\n3 1 0\n0 0 0\n1 0 1,5\n0 1 0\n3 0 1 2\n      \n").encode(), meshes.BAD_COORD, "no number", False),
    "coord_two": (("OFF\n3 1 0\n0 0 0\n1 0\n0 1 0\n3 0 1 2\n        \n").encode(), meshes.BAD_COORD, "three numbers", False),
}


def test_refused_files_are_all_named_and_the_good_ones_still_read(tmp_path, pool):
    bad = {}
    for name, (data, _, _, _) in REFUSALS.items():
        bad[name] = str(tmp_path / (name + ".off"))
        open(bad[name], "wb").write(data)
        with pytest.raises(ValueError) as e:                                       # the Python reader refuses the same file for the same cause
            meshes.read_off(bad[name])
        assert e.value.status == REFUSALS[name][1] and REFUSALS[name][2] in str(e.value) and bad[name] in str(e.value), name
    bad["missing"] = str(tmp_path / "no such file.off")
    bad["directory"] = str(tmp_path)
    causes = dict({k: v[2] for k, v in REFUSALS.items()}, missing="No such file", directory="not a regular file")
    status = dict({k: v[1] for k, v in REFUSALS.items()}, missing=meshes.IO, directory=meshes.IO)
    good = [f for f in pool if len(f[2]) == 257][:len(bad) + 1]
    paths, kind = [], []
    for i, g in enumerate(good):                                                   # a good file between every two bad ones
        paths.append(g[0]), kind.append(None)
        if i < len(bad):
            paths.append(list(bad.values())[i]), kind.append(list(bad)[i])
    before = {p: os.stat(p).st_mtime_ns for p in paths if os.path.isfile(p)}
    listing = sorted(os.listdir(tmp_path))
    for threads in (1, 0):
        table, msgs = meshes.scan_meshes(paths, threads, check=False)
        for b, k in enumerate(kind):
            assert (table[b, 0] != 0) == (k is not None and (k in ("missing", "directory") or REFUSALS[k][3])), k
        ok_rows = np.where(table[:, 0] == 0, 1, 0)[:, None] * table
        staging, v_dst, f_dst = guarded(ok_rows)
        msgs2 = meshes.load_meshes(paths, table, staging, v_dst, f_dst, threads, check=False)
        gi, ranges = 0, []
        for b, k in enumerate(kind):
            text = (bytes(msgs[b]) + bytes(msgs2[b])).replace(bytes(1), b" ").decode()
            ranges += [(v_dst[b], 12 * ok_rows[b, meshes.NV]), (f_dst[b], 12 * ok_rows[b, meshes.NF])]
            if k is None:
                path, V, F = good[gi]
                gi += 1
                assert table[b, :3].tolist() == [0, len(V), len(F)]
                assert staging[v_dst[b]:v_dst[b] + 12 * len(V)].tobytes() == V.tobytes() and staging[f_dst[b]:f_dst[b] + 12 * len(F)].tobytes() == F.tobytes()
            else:
                assert table[b, 0] == status[k] and causes[k] in text, (k, table[b, 0], text)
        assert guards_intact(staging, ranges)
    # read_meshes names every bad path, with its cause, in one ValueError, whether the header or the body is refused -- before any GPU work
    with pytest.raises(ValueError) as e:
        meshes.read_meshes(paths, "cuda")
    for k, p in bad.items():
        assert f"{p}: " in str(e.value) and causes[k] in str(e.value), k
    assert not any(g[0] + ": " in str(e.value) for g in good)
    # check_meshes, which the CLI runs in front of any GPU work, names them all at once
    found = dict(meshes.check_meshes(paths))
    assert sorted(found) == [b for b, k in enumerate(kind) if k is not None]
    for b, k in enumerate(kind):
        if k is not None:
            assert causes[k] in found[b], (k, found[b])
    # nothing was written anywhere
    assert sorted(os.listdir(tmp_path)) == listing and before == {p: os.stat(p).st_mtime_ns for p in before}
    # ranges that do not hold their file, overlap or are misaligned are refused by name too, and nothing is written
    one = meshes.scan_meshes(paths[:1])
    staging, v_dst, f_dst = guarded(one)
    for v, f, n, why in ((v_dst, f_dst, 64, b"do not hold"), (v_dst + 2, f_dst, None, b"not 4-byte aligned"), (v_dst, v_dst + 12, None, b"overlap")):
        msgs = meshes.load_meshes(paths[:1], one.copy(), staging[:n], v, f, check=False)
        assert why in bytes(msgs[0]), (why, bytes(msgs[0])[:80])
    assert (staging == 0xA5).all()


def test_new_symbols_are_declared_exported_and_bound():
    names = ("pccx_off_scan_host", "pccx_off_load_host", "pccx_mesh_sample", "pccx_mesh_sample_workspace_bytes")
    lib = _lib.load()
    for n in names:
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.pccx_mesh_sample_workspace_bytes(2, 1000, 8192) >= 3 * 8 * 1000 + 2 * 64
    assert lib.pccx_mesh_sample(None, 1, None, 1, None, None, None, 2000, 1, 1, None, None, None, None) == -1 and b"MESH_MAX_B" in lib.pccx_last_error()
    assert meshes.stream_seed(11, "a/train/x.off") == meshes.stream_seed(11, "a/train/x.off") != meshes.stream_seed(11, "a/train/y.off")
    assert meshes.stream_seed(11, "x") != meshes.stream_seed(12, "x") and 0 <= meshes.stream_seed(2**64 - 1, "x") < 2**64


MAIN = r"""
#include "off_host.h"
#include <stdlib.h>
#include <string>
#include <vector>
// Seeded mutations of valid OFF files, each in a heap block of exactly its length (the sanitizer sees any byte read past it), the
// outputs in blocks of exactly nv * 3 and nf * 3: every case must come back parsed or refused, and a parsed one must hold indices
// inside 0 .. nv - 1 and finite coordinates.
static unsigned long long state = 88172645463325252ull;
static unsigned rnd(unsigned n) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (unsigned)(state % n); }
int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 1000;
    int ok = 0, refused = 0;
    for (int r = 0; r < rounds; ++r) {
        const int nv = 3 + (int)rnd(40), nf = 1 + (int)rnd(60);
        const char *nl = rnd(4) ? "\n" : "\r\n";
        std::string h;
        if (rnd(4) == 0) h += std::string("# a comment") + nl;
        const int mode = rnd(12);
        std::string counts = mode == 9 ? "99999999999999999999999 1 0" : mode == 10 ? "2147483647 4194304 0" : mode == 11 ? "3 99999999999 0"
                                       : std::to_string(nv) + " " + std::to_string(nf) + " " + std::to_string(rnd(100));
        if (rnd(2)) h += "OFF" + counts + nl;
        else h += std::string("OFF") + nl + (rnd(3) ? "" : nl) + counts + nl;
        for (int i = 0; i < nv; ++i) {
            char line[128];
            snprintf(line, sizeof(line), "%g %.9g %de-%d%s", (double)rnd(2000) / 7 - 100, (double)rnd(100000) / 3e4, (int)rnd(1000), (int)rnd(60), rnd(9) ? "" : " # v");
            h += line;
            h += nl;
            if (rnd(10) == 0) h += nl;
        }
        for (int i = 0; i < nf; ++i) {
            h += "3 " + std::to_string(rnd((unsigned)nv)) + " " + std::to_string(rnd((unsigned)nv)) + " " + std::to_string(rnd((unsigned)nv)) + (rnd(5) ? "" : " 255 0 0");
            if (i + 1 < nf || rnd(3)) h += nl;                                        // a missing final newline
        }
        std::string all = h;
        size_t n = all.size();
        const int mut = rnd(6);
        if (mut == 1) n = rnd((unsigned)n + 1);                                       // truncated anywhere
        if (mut == 2) for (int k = 1 + (int)rnd(3); k > 0; --k) all[rnd((unsigned)all.size())] ^= (char)(1u << rnd(8));   // bits flipped
        if (mut == 3) all[rnd((unsigned)all.size())] = (char)rnd(256);
        if (mut == 4) all[rnd((unsigned)all.size())] = "0123456789 \n#-+.e"[rnd(17)];
        uint8_t *arg = (uint8_t *)malloc(n ? n : 1);
        memcpy(arg, all.data(), n);
        OffHeader oh;
        char msg[64];
        const int64_t file_size = rnd(3) == 0 ? -1 : (int64_t)n;
        const int st = off_parse_header(arg, n, file_size, &oh, msg, sizeof(msg));
        if (st < OFF_OK || st > OFF_MALFORMED) return 2;
        if (st != OFF_OK) {
            if (!msg[0] || oh.nv != 0 || oh.nf != 0) return 3;                        // a cause is named, nothing half-filled is handed out
            ++refused;
        } else {
            if (oh.nv < 3 || oh.nv > OFF_MAX_VERTICES || oh.nf < 1 || oh.nf > OFF_MAX_FACES || oh.body_offset < 0 || (size_t)oh.body_offset > n) return 4;
            if (file_size >= 0 && oh.nv * 6 + oh.nf * 8 - 1 > file_size - oh.body_offset) return 5;
            if (msg[0]) return 6;
            if (file_size >= 0) {                                                     // the size check bounds the blocks a caller allocates
                float *V = (float *)malloc(12 * (size_t)oh.nv);
                int32_t *F = (int32_t *)malloc(12 * (size_t)oh.nf);
                const int bs = off_parse_body(arg + oh.body_offset, n - (size_t)oh.body_offset, oh, V, F, msg, sizeof(msg));
                if (bs != OFF_OK && bs != OFF_TRUNCATED && (bs < OFF_NOT_TRIANGLE || bs > OFF_BAD_COORD)) return 7;
                if (bs == OFF_OK) {
                    for (int64_t i = 0; i < 3 * oh.nv; ++i) if (!isfinite(V[i])) return 8;
                    for (int64_t i = 0; i < 3 * oh.nf; ++i) if (F[i] < 0 || F[i] >= oh.nv) return 9;
                    ++ok;
                } else {
                    if (!msg[0]) return 10;
                    ++refused;
                }
                free(V), free(F);
            }
            // a prefix of the file, cut anywhere: "hand me more" or the verdict on the whole, never a verdict on half a line
            OffHeader whole, part;
            const int full = off_parse_header(arg, n, (int64_t)n, &whole, msg, sizeof(msg));
            const size_t cut = rnd((unsigned)n + 1);
            const int pre = off_parse_header(arg, cut, (int64_t)n, &part, msg, sizeof(msg));
            if (cut < n && pre != OFF_TRUNCATED && (pre != full || memcmp(&part, &whole, sizeof(part)) != 0)) return 12;
        }
        free(arg);
        // a random token, in a block of its exact length
        const char alphabet[] = "0123456789+-.eEinfa";
        const size_t tn = rnd(24);
        uint8_t *tok = (uint8_t *)malloc(tn ? tn : 1);
        for (size_t i = 0; i < tn; ++i) tok[i] = (uint8_t)alphabet[rnd(sizeof(alphabet) - 1)];
        double v;
        (void)off_token_to_double(tok, tn, &v);
        free(tok);
    }
    printf("ok %d refused %d\n", ok, refused);
    return ok > 0 && refused > 0 ? 0 : 11;
}
"""


def test_off_parser_alone_under_sanitizers(tmp_path):
    """csrc/off_host.h is plain C++ with no dependency: a stand-alone host program that includes nothing else of the project, built with
    the address and undefined-behaviour sanitizers, runs the parser over 8 000 seeded mutations of good files -- truncations, flipped
    bits, replaced bytes, huge counts, a missing final newline."""
    src, exe = tmp_path / "off_host_main.cc", tmp_path / "off_host_main"
    src.write_text(MAIN)
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe), "8000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ")
