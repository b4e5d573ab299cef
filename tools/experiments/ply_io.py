#!/usr/bin/env python3
"""PLY files in and out: the Python loop against the host threads + GPU unpack, and the CLIs against another tree.

    python tools/experiments/ply_io.py [--rounds 3] [--reps 5] [--legs ...] [--other PATH_TO_ANOTHER_CHECKOUT] [--small]

Same box, ALTERNATING runs, one fresh process per figure (each settles the clocks with 0.3 s of untimed fill kernels, runs the call
once untimed -- that also leaves the files in the page cache and the pinned buffers allocated -- then times `reps` calls, each
ending in a device synchronise; the figure is their median).  The data is written once, seeded, under --work.

  read legs    f32: 1024 files of 8192 points, float32 little-endian, stride 12     f64rgb: the same count, float64 + rgb, stride 27
               ascii: 64 ASCII files of 8192 points     room: one file of 1 048 576 points     mixed: 256 files of 2048 .. 16384 points
               python = read_point_cloud per file, np.stack or codec.pad_clouds, .to(device); threads = plyio.read_point_clouds
  write legs   w_f32 / w_room: a (B, N, 3) device tensor to files; python = .cpu().numpy() and save_point_cloud per file,
               threads = plyio.save_point_clouds
  unpack       pccx_ply_unpack alone on f32, f64rgb and room, every round: device events around 20 calls on the same buffers (so
               they are read from the Infinity Cache where they fit it), GB/s of staging bytes read
  cli          compress.py and decompress.py on the f32 folder: wall time of the whole command and the per-cloud time the tool prints,
               this tree without and with --ply-io threads and, with --other, that checkout (the parent) without; one untimed
               run of each tool first, and the order of the trees rotates from round to round

One JSON line per figure, summary tables at the end."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
READ = {"f32": (1024, 8192), "f64rgb": (1024, 8192), "ascii": (64, 8192), "room": (1, 1 << 20), "mixed": (256, None)}
WRITE = {"w_f32": "f32", "w_room": "room"}
K, D, L = 256, 16, 7


def paths_of(work, leg, small):
    count, _ = READ[leg]
    return [os.path.join(work, leg, f"{i:04d}.ply") for i in range(max(1, count // 16) if small else count)]


def make_data(work, small):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-compression_amd")]
    import numpy as np
    from pccx import plyio, synth
    for leg, (count, n) in READ.items():
        os.makedirs(os.path.join(work, leg), exist_ok=True)
        rng = np.random.default_rng(len(leg))
        for i, path in enumerate(paths_of(work, leg, small)):
            if os.path.exists(path):
                continue
            m = n if n else int(rng.integers(2048, 16385))
            pts = rng.random((m, 3), dtype=np.float32) if leg == "room" else synth.cad_cloud(1000 + i, m)
            if leg in ("f32", "room", "mixed"):
                plyio.save_point_cloud(pts, path)
            elif leg == "f64rgb":
                rec = np.zeros(len(pts), dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
                rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
                head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(pts) + "".join(
                    f"property {t} {nm}\n" for nm, t in (("x", "double"), ("y", "double"), ("z", "double"), ("red", "uchar"), ("green", "uchar"), ("blue", "uchar")))
                open(path, "wb").write(head.encode() + b"end_header\n" + rec.tobytes())
            else:
                head = "ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(pts)
                open(path, "w").write(head + "".join(f"{float(a)!r} {float(b)!r} {float(c)!r}\n" for a, b, c in pts))
    mdl = os.path.join(work, "model")
    if not os.path.exists(os.path.join(mdl, "prob.pkl")):
        import torch
        from oracle import ref_model
        from pccx import models
        os.makedirs(mdl, exist_ok=True)
        ae, prob = models.AE(K, K // 2, D, L), models.ConditionalProbabilityModel(L, D)
        ae.load_state_dict(ref_model.seeded_state_dict(ae, 11, last_gain={"pn.mlp_Modules.3.0": 40.0}))
        prob.load_state_dict(ref_model.seeded_state_dict(prob, 12, gain=2.0))
        torch.save(ae.state_dict(), os.path.join(mdl, "ae.pkl"))
        torch.save(prob.state_dict(), os.path.join(mdl, "prob.pkl"))


def settle(torch):
    buf = torch.empty(64 << 20, device="cuda", dtype=torch.float32)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:
        for _ in range(8):
            buf.fill_(1.0)
        torch.cuda.synchronize()


def timed(torch, fn, reps):
    fn()                                                   # warm-up: code objects, page cache, pinned buffers
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def child(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-compression_amd")]
    import numpy as np
    import torch
    from pccx import codec, ops, plyio
    settle(torch)
    kind, leg, side = a.child.split(":")
    out = dict(kind=kind, leg=leg, side=side)
    if kind == "read":
        files = paths_of(a.work, leg, a.small)
        one_size = leg != "mixed"

        def python():
            clouds = [plyio.read_point_cloud(f) for f in files]
            return torch.from_numpy(np.stack(clouds)).to("cuda") if one_size else codec.pad_clouds(clouds)[0].to("cuda")
        ms = timed(torch, python if side == "python" else (lambda: plyio.read_point_clouds(files, "cuda")), a.reps)
        out.update(files=len(files), bytes=sum(os.path.getsize(f) for f in files))
    elif kind == "write":
        files = paths_of(a.work, WRITE[leg], a.small)
        rows = plyio.read_point_clouds(files, "cuda")[0]
        names, dst = [os.path.basename(f) for f in files], os.path.join(a.work, "out_" + leg + "_" + side)
        os.makedirs(dst, exist_ok=True)

        def python():
            for name, cloud in zip(names, rows.cpu().numpy()):
                plyio.save_point_cloud(cloud, os.path.join(dst, name))
        ms = timed(torch, python if side == "python" else (lambda: plyio.save_point_clouds(rows, [rows.shape[1]] * len(names), dst, names, "")), a.reps)
        out.update(files=len(files), bytes=rows.numel() * 4)
    else:                                                  # the kernel alone
        files = paths_of(a.work, leg, a.small)
        table = plyio.scan_point_clouds(files)
        off, nbytes = plyio.staging_offsets(table)
        host = torch.zeros(nbytes, dtype=torch.uint8)
        plyio.load_point_clouds(files, table, host, off)
        n = table[:, plyio.N_VERTEX]
        dev, prefix = plyio.device_tables(table, off, np.cumsum(n) - n, n)
        args = [host.cuda(), torch.from_numpy(dev).cuda(), torch.from_numpy(prefix).cuda(), torch.empty(int(n.sum()), 3, device="cuda")]
        for _ in range(3):
            ops.ply_unpack(*args, total_tiles=int(prefix[-1]))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(20):
            ops.ply_unpack(*args, total_tiles=int(prefix[-1]))
        ev[1].record()
        torch.cuda.synchronize()
        ms = [ev[0].elapsed_time(ev[1]) / 20]
        out.update(staging_bytes=nbytes, out_bytes=int(n.sum()) * 12, gb_per_s_staging_read=round(nbytes / ms[0] / 1e6, 1))
    out.update(ms=round(statistics.median(ms), 3), ms_all=[round(v, 3) for v in ms])
    print(json.dumps(out))


def run_child(a, spec):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", spec, "--work", a.work, "--reps", str(a.reps)] + (["--small"] if a.small else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"{spec} ended with {p.returncode}: stop here\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def run_cli(a, tree, tool, flags, tag):
    cli = os.path.join(tree, "point-cloud-compression_amd", "cli", tool)
    src = os.path.join(a.work, "f32", "*.ply") if tool == "compress.py" else os.path.join(a.work, "cli_bin")
    dst = os.path.join(a.work, "cli_bin" if tool == "compress.py" else "cli_out_" + tag)
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, cli, src, dst, os.path.join(a.work, "model"), "--batch", "1024", *flags], capture_output=True, text=True, timeout=900)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit(f"{tool} {flags} in {tree} ended with {p.returncode}: stop here\n{p.stderr[-2000:]}")
    per = float(p.stdout.split("Execution time: ")[1].split("s per point cloud")[0])
    return dict(kind="cli", tool=tool, leg=tag, wall_s=round(wall, 3), per_cloud_ms=round(per * 1e3, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="read,write,unpack,cli")
    ap.add_argument("--other", default=None)
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "pccx_ply_io_work"), help="where the seeded folders are written (kept between runs)")
    ap.add_argument("--small", action="store_true", help="a sixteenth of every folder: a rehearsal of the tool, not a measurement")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    make_data(a.work, a.small)
    legs, rows = a.legs.split(","), []

    def note(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
    for r in range(a.rounds):
        for kind, names in (("read", READ), ("write", WRITE)):
            if kind in legs:
                for leg in names:
                    for side in ("python", "threads"):
                        note(dict(run_child(a, f"{kind}:{leg}:{side}"), round=r))
        if "unpack" in legs:
            for leg in ("f32", "f64rgb", "room"):
                note(dict(run_child(a, f"unpack:{leg}:kernel"), round=r))
        if "cli" in legs:
            trees = [("this", ROOT, []), ("this_threads", ROOT, ["--ply-io", "threads"])] + ([("other", os.path.abspath(a.other), [])] if a.other else [])
            for tool in ("compress.py", "decompress.py"):
                if r == 0:
                    run_cli(a, ROOT, tool, [], "untimed")                            # the first command to touch the folder through the CLI is no figure
                for tag, tree, flags in trees[r % len(trees):] + trees[:r % len(trees)]:   # another tree goes first in every round
                    note(dict(run_cli(a, tree, tool, flags, tag), round=r))
    print("\n| figure | side | each round |")
    seen = {}
    for r in rows:
        if r["kind"] in ("read", "write"):
            seen.setdefault((f"{r['kind']} {r['leg']} ({r['files']} files, {r['bytes'] / 1e6:.1f} MB)", r["side"]), []).append(r["ms"])
        elif r["kind"] == "cli":
            seen.setdefault((f"{r['tool']} wall s", r["leg"]), []).append(r["wall_s"])
            seen.setdefault((f"{r['tool']} per cloud ms (printed)", r["leg"]), []).append(r["per_cloud_ms"])
        else:
            seen.setdefault((f"pccx_ply_unpack {r['leg']} ({r['staging_bytes'] / 1e6:.1f} MB staged), GB/s of staging read", "kernel"), []).append(r["gb_per_s_staging_read"])
            seen.setdefault((f"pccx_ply_unpack {r['leg']}, ms per call", "kernel"), []).append(r["ms"])
    for (what, side), vs in seen.items():
        print(f"| {what} | {side} | " + ", ".join(f"{v:.3f}" for v in vs) + " |")


if __name__ == "__main__":
    main()
