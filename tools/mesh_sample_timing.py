#!/usr/bin/env python3
"""Times sample_modelnet's chunked path (pccx.meshes.read_meshes -> sample_meshes -> plyio.save_point_clouds) beside the file-by-file
Python path (meshes.read_off -> the numpy restatement of the sampler, tests/mesh_cases.py -> plyio.save_point_cloud) on a synthetic set
of OFF files built from a seed: --meshes files of --min-faces .. --max-faces triangles (log-uniform), --n_point points each.

Host to host with a final synchronise, after one warm pass of either leg, --repeats times with the two legs in turn inside this one
process.  Prints one JSON line: seconds and files per second of the chunked path split into check (the host-only pass in front of any
GPU work) / read / sample / write, and seconds per file of the Python path on its first --python-files files.

    python tools/mesh_sample_timing.py [--meshes 1024] [--batch 256] [--repeats 3]

The set is synthetic (deformed tori, --distinct different meshes written several times under different names): its figures are this
set's, not ModelNet40's."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "point-cloud-compression_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def torus(rng, faces):
    """a deformed torus of about `faces` triangles -> (V float32, F int32)"""
    r = max(int(np.sqrt(faces / 2)), 2)
    c = max(faces // (2 * r), 2)
    a, b = np.meshgrid(np.arange(r) * (2 * np.pi / r), np.arange(c) * (2 * np.pi / c), indexing="ij")
    R, w = rng.uniform(5, 40), rng.uniform(0.2, 0.8)
    rad = R * (1 + w * np.cos(b) * (1 + 0.2 * np.sin(3 * a)))
    V = np.stack([rad * np.cos(a), rad * np.sin(a), R * w * np.sin(b) * rng.uniform(0.3, 2)], axis=-1).reshape(-1, 3) + rng.uniform(-50, 50, 3)
    i, j = np.meshgrid(np.arange(r), np.arange(c), indexing="ij")
    p00, p10, p01, p11 = i * c + j, (i + 1) % r * c + j, i * c + (j + 1) % c, (i + 1) % r * c + (j + 1) % c
    F = np.concatenate([np.stack([p00, p10, p11], -1).reshape(-1, 3), np.stack([p00, p11, p01], -1).reshape(-1, 3)])
    return V.astype(np.float32), F.astype(np.int32)


def off_text(V, F, glued):
    lines = ["OFF%d %d 0" % (len(V), len(F))] if glued else ["OFF", "%d %d 0" % (len(V), len(F))]
    lines += ["%.6g %.6g %.6g" % tuple(v) for v in V.tolist()]
    lines += ["3 %d %d %d" % tuple(f) for f in F.tolist()]
    return ("\n".join(lines) + "\n").encode("ascii")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--meshes", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--min-faces", type=int, default=1000)
    ap.add_argument("--max-faces", type=int, default=100000)
    ap.add_argument("--n_point", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--python-files", type=int, default=16)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--dir", default=None, help="where the set and the clouds go (default: a temporary directory, removed at the end)")
    args = ap.parse_args()

    import torch
    from pccx import meshes, plyio
    from tests import mesh_cases as mc

    work = args.dir or tempfile.mkdtemp(prefix="mesh_timing_")
    src = os.path.join(work, "src")
    os.makedirs(src, exist_ok=True)
    rng = np.random.default_rng(args.seed)
    texts, n_faces = [], []
    for k in range(args.distinct):
        V, F = torus(rng, int(np.exp(rng.uniform(np.log(args.min_faces), np.log(args.max_faces)))))
        texts.append(off_text(V, F, k % 2 == 0))
        n_faces.append(len(F))
    rels = []
    for i in range(args.meshes):
        rel = "class_%02d/%s/m_%04d.off" % (i * 40 // args.meshes, "train" if i % 5 else "test", i)
        os.makedirs(os.path.dirname(os.path.join(src, rel)), exist_ok=True)
        with open(os.path.join(src, rel), "wb") as f:
            f.write(texts[i % args.distinct])
        rels.append(rel)
    rels.sort()
    paths = [os.path.join(src, r) for r in rels]
    set_bytes = sum(os.path.getsize(p) for p in paths)
    dev = torch.device("cuda:0")

    def chunked(files, out):
        t = dict(check=0.0, read=0.0, sample=0.0, write=0.0)
        for at in range(0, len(files), args.batch):
            chunk = files[at:at + args.batch]
            t0 = time.perf_counter()
            assert meshes.check_meshes([p for p, _ in chunk], args.threads) == []
            t1 = time.perf_counter()
            packed = meshes.read_meshes([p for p, _ in chunk], dev, args.threads)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            points, status = meshes.sample_meshes(*packed, args.n_point, [meshes.stream_seed(args.seed, r) for _, r in chunk])
            assert not status.any().item()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            plyio.save_point_clouds(points, [args.n_point] * len(chunk), out, ["c%05d" % (at + b) for b in range(len(chunk))], threads=args.threads)
            t4 = time.perf_counter()
            t["check"] += t1 - t0
            t["read"] += t2 - t1
            t["sample"] += t3 - t2
            t["write"] += t4 - t3
        return t

    def by_file(files, out):
        t0 = time.perf_counter()
        for k, (p, r) in enumerate(files):
            V, F = meshes.read_off(p)
            cloud, status, _ = mc.sample(V, F, meshes.stream_seed(args.seed, r), args.n_point)
            plyio.save_point_cloud(cloud, os.path.join(out, "p%05d.ply" % k))
        return time.perf_counter() - t0

    files = list(zip(paths, rels))
    subset = files[:args.python_files]
    out = os.path.join(work, "out")
    os.makedirs(out, exist_ok=True)
    chunked(files[:args.batch], out)                                             # warm: library, pinned buffers, page cache of the writer
    by_file(subset[:2], out)
    runs, py = [], []
    for _ in range(args.repeats):
        runs.append(chunked(files, out))
        py.append(by_file(subset, out))
    best = min(runs, key=lambda t: sum(t.values()))
    total = sum(best.values())
    result = {
        "set": {"meshes": args.meshes, "distinct": args.distinct, "faces_min": min(n_faces), "faces_max": max(n_faces),
                "faces_mean": float(np.mean([n_faces[i % args.distinct] for i in range(args.meshes)])), "bytes": set_bytes},
        "n_point": args.n_point, "batch": args.batch, "threads": args.threads, "repeats": args.repeats,
        "chunked_s": {k: round(v, 4) for k, v in best.items()}, "chunked_total_s": round(total, 4),
        "chunked_files_per_s": round(args.meshes / total, 1), "chunked_files_per_s_without_check": round(args.meshes / (total - best["check"]), 1),
        "chunked_all_runs_total_s": [round(sum(t.values()), 4) for t in runs],
        "python_files": len(subset), 
        "python_faces_mean": float(np.mean([n_faces[int(r[-8:-4]) % args.distinct] for _, r in subset])),
        "python_s_per_file": round(min(py) / len(subset), 4), "python_files_per_s": round(len(subset) / min(py), 2),
        "python_all_runs_s": [round(v, 4) for v in py],
    }
    print(json.dumps(result))
    meshes.release_pinned()
    plyio.release_pinned()
    if args.dir is None:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
