#!/usr/bin/env python3
"""What a folder of scans with different point counts costs per file: one call per distinct N against ragged batches.

    python tools/experiments/ragged_batch_ab.py [--rounds 3] [--clouds 256] [--reps 3] [--stages]

The workload: `clouds` seeded clouds with n_b uniform in [2048, 16384], K = 256, octree mode "full", default arithmetic; compress +
decompress, host to host through the packed buffer (pad / stack on the host, upload, compress, ONE device->host copy of the packed
streams, upload of that copy, decompress, the points back on the host).
  leg "per_n"      the loop the CLIs run without --ragged: one Codec.compress / Codec.decompress call per distinct point count
  leg "ragged64"   Codec.compress_ragged / decompress_ragged, 64 clouds per call
  leg "ragged256"  ... 256 clouds per call
Same box, ALTERNATING legs, `rounds` rounds, one fresh process per measurement (bench.settle first, one untimed pass, then `reps` timed
passes; the figure is their mean).  The parent checks every child's exit status and stops at the first that is not 0.  The condition
stated beforehand: both ragged legs faster than per_n in every round.  --stages: the per-stage milliseconds of one ragged256 pass.
One JSON line per measurement, the table at the end."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEGS = ("per_n", "ragged64", "ragged256")
K, D, L = 256, 16, 7


def child(leg, clouds, reps, stages):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-compression_amd")]
    import numpy as np
    import torch
    import bench
    from oracle import ref_model
    from pccx import codec, models, ops, synth as cloud_synth
    ae = models.AE(K, K // 2, D, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, 3, last_gain={"pn.mlp_Modules.3.0": 40.0}))
    prob = models.ConditionalProbabilityModel(L, D)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, 4, gain=2.0))
    cd = codec.Codec(ae.pack("cuda"), prob.pack("cuda"), K=K, octree_mode="full")
    rng = np.random.default_rng(2024)
    sizes = [int(v) for v in rng.integers(2048, 16385, clouds)]
    pcs = [cloud_synth.cad_cloud(5000 + i, n) for i, n in enumerate(sizes)]
    starts = [int(v) for v in rng.integers(0, 2048, clouds)]

    def one_call(idx):
        """compress + decompress of the clouds idx, host to host; per_n: all of one size"""
        n = [sizes[i] for i in idx]
        st = [starts[i] for i in idx]
        if leg == "per_n":
            comp = cd.compress(torch.from_numpy(np.stack([pcs[i] for i in idx])).cuda(), st)
        else:
            comp = cd.compress_ragged(codec.pad_clouds([pcs[i] for i in idx])[0].cuda(), n, st)
        host = comp.packed.cpu()                                             # ONE D2H of the packed streams
        up = codec.Compressed.from_packed(host.cuda(), len(idx), comp.s_bytes.shape[1], comp.p_bytes.shape[1], 0)
        if leg == "per_n":
            return [cd.decompress(up, S=n[0] * 2 // K).cpu()]
        return [p.cpu() for p in cd.decompress_ragged(up, [v * 2 // K for v in n])]

    def one_pass():
        if leg == "per_n":
            by_n = {}
            for i, n in enumerate(sizes):
                by_n.setdefault(n, []).append(i)
            calls = list(by_n.values())
        else:
            per = int(leg[6:])
            calls = [list(range(i, min(i + per, clouds))) for i in range(0, clouds, per)]
        for idx in calls:
            one_call(idx)
        torch.cuda.synchronize()
        return len(calls)

    import types
    bench.settle(types.SimpleNamespace(gpu=True, dev="cuda"))
    ncalls = one_pass()                                                      # untimed: allocator, workspaces, first launches
    t0 = time.perf_counter()
    for _ in range(reps):
        one_pass()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    out = dict(leg=leg, clouds=clouds, calls=ncalls, ms_per_pass=round(ms, 3), ms_per_cloud=round(ms / clouds, 4), reps=reps)
    if stages:
        timer = ops.StageTimer()
        ops.set_timer(timer)
        one_pass()
        ops.set_timer(None)
        out["stage_ms"] = {k_: round(v[0], 3) for k_, v in timer.totals_ms().items()}
    print(json.dumps(out))


def run(leg, clouds, reps, stages=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--clouds", str(clouds), "--reps", str(reps)] + (["--stages"] if stages else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"{leg} ended with {p.returncode}: stop here\n{p.stderr[-2000:]}")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.clouds, a.reps, a.stages)
    table = {}
    for r in range(a.rounds):
        for leg in LEGS:
            res = run(leg, a.clouds, a.reps)
            table.setdefault(leg, []).append(res["ms_per_cloud"])
            print(json.dumps(dict(res, round=r)), flush=True)
    if a.stages:
        print(json.dumps(run("ragged256", a.clouds, 1, stages=True)), flush=True)
    print("\n| leg | ms per cloud, each round |")
    for leg, vs in table.items():
        print(f"| {leg} | " + ", ".join(f"{v:.3f}" for v in vs) + " |")
    ok = all(table[leg][r] < table["per_n"][r] for leg in LEGS[1:] for r in range(a.rounds))
    print("condition (both ragged legs faster than per_n in every round):", "met" if ok else "NOT met")


if __name__ == "__main__":
    main()
