#!/usr/bin/env python3
"""What scoring a folder of scans with different point counts costs per file: eval.py's file-by-file loop against
codec.evaluate_ragged.

    python tools/experiments/eval_ragged_cost.py [--rounds 3] [--pairs 256] [--reps 3] [--stages]

The workload: `pairs` seeded clouds with n_b uniform in [2048, 16384], each with a reconstruction of the size the codec returns at
K = 256 (n_b * 2 // 256 patches of 128 points: a jittered subset), both on the host as a reader leaves them.  Host to host, read-backs
included:
  leg "per_file"   the loop of cli/eval.py without --ragged: upload the pair, d1_psnr, d2_psnr, normalized_chamfer, calc_uc, five float()s
  leg "ragged64"   pad 64 pairs into two slabs on the host, upload, ONE codec.evaluate_ragged call, ONE read-back of the four vectors
Same box, ALTERNATING legs, `rounds` rounds, one fresh process per measurement (bench.settle first, one untimed pass, then `reps` timed
passes; the figure is their mean).  The parent checks every child's exit status and stops at the first that is not 0.  Nothing is
gated: the figures are recorded.  --stages: the per-stage milliseconds of one ragged64 pass (30-NN + PCA, the three scans, the regions).
One JSON line per measurement, the table at the end."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEGS = ("per_file", "ragged64")
K = 256


def child(leg, pairs, reps, stages):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-compression_amd"), os.path.join(ROOT, "point-cloud-compression_amd", "cli")]
    import numpy as np
    import torch
    import bench
    from pccx import codec, ops, synth as cloud_synth
    argv, sys.argv = sys.argv, ["eval.py"]
    ev = importlib.import_module("eval")
    sys.argv = argv
    rng = np.random.default_rng(2024)
    sizes = [int(v) for v in rng.integers(2048, 16385, pairs)]
    origs = [cloud_synth.cad_cloud(5000 + i, n) for i, n in enumerate(sizes)]
    recons = [(a[rng.permutation(n)[:n * 2 // K * (K // 2)]] + rng.normal(0, 2e-3, (n * 2 // K * (K // 2), 3))).astype(np.float32)
              for a, n in zip(origs, sizes)]

    def one_pass():
        rows = []
        if leg == "per_file":
            for a, b in zip(origs, recons):
                a, b = torch.from_numpy(a)[None].cuda(), torch.from_numpy(b)[None].cuda()
                rows.append((float(codec.d1_psnr(a, b)[0]), float(codec.d2_psnr(a, b)[0]), float(codec.normalized_chamfer(a, b)[0]), ev.calc_uc(a, b)))
        else:
            per = int(leg[6:])
            for i in range(0, pairs, per):
                pa, na = codec.pad_clouds(origs[i:i + per])
                pb, nb = codec.pad_clouds(recons[i:i + per])
                res = codec.evaluate_ragged(pa.cuda(), na, pb.cuda(), nb)
                rows += list(zip(*torch.stack([res[k] for k in ("d1_psnr", "d2_psnr", "chamfer", "uc")]).cpu().tolist()))
        torch.cuda.synchronize()
        return rows

    import types
    bench.settle(types.SimpleNamespace(gpu=True, dev="cuda"))
    rows = one_pass()                                                        # untimed: allocator, workspaces, first launches
    t0 = time.perf_counter()
    for _ in range(reps):
        one_pass()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    out = dict(leg=leg, pairs=pairs, ms_per_pass=round(ms, 3), ms_per_file=round(ms / pairs, 4), reps=reps,
               mean_d1_psnr=round(float(np.mean([r[0] for r in rows])), 6), mean_uc=round(float(np.mean([r[3] for r in rows])), 6))
    if stages and leg != "per_file":
        timer = ops.StageTimer()
        ops.set_timer(timer)
        one_pass()
        ops.set_timer(None)
        out["stage_ms"] = {k_: round(v[0], 3) for k_, v in timer.totals_ms().items()}
    print(json.dumps(out))


def run(leg, pairs, reps, stages=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--pairs", str(pairs), "--reps", str(reps)] + (["--stages"] if stages else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if p.returncode != 0:
        raise SystemExit(f"{leg} ended with {p.returncode}: stop here\n{p.stderr[-2000:]}")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.pairs, a.reps, a.stages)
    table = {}
    for r in range(a.rounds):
        for leg in LEGS:
            res = run(leg, a.pairs, a.reps)
            table.setdefault(leg, []).append(res["ms_per_file"])
            print(json.dumps(dict(res, round=r)), flush=True)
    if a.stages:
        print(json.dumps(run("ragged64", a.pairs, 1, stages=True)), flush=True)
    print("\n| leg | ms per file, each round |")
    for leg, vs in table.items():
        print(f"| {leg} | " + ", ".join(f"{v:.3f}" for v in vs) + " |")
    print("per_file / ragged64, each round:", ", ".join(f"{p / q:.2f}" for p, q in zip(table["per_file"], table["ragged64"])))


if __name__ == "__main__":
    main()
