#!/usr/bin/env python3
"""Step time of IPDAE training in octree_mode="full" against the "reference"-mode step, and against another tree.

    python tools/experiments/full_mode_step_cost.py [--rounds 3] [--steps 50] [--other PATH_TO_ANOTHER_CHECKOUT]

In the style of deterministic_cost.py: same box, ALTERNATING runs, one fresh process per measurement (0.3 s of untimed fill kernels,
warm-up steps, then `steps` steps between two synchronisations).  The shape is the reference's (batch 1, 8192 points, K = 256, S = 64),
the one shape both modes take; eager and as a graph.  --other: a built checkout of another commit (the parent), whose "reference"-mode
step joins the alternation -- the check that the default path did not slow down.  One JSON line per measurement, a table at the end."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.environ.get("FULLCOST_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = ("ipdae_eager", "ipdae_graph")


def child(case, mode, steps):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-compression_amd")]
    import numpy as np
    import torch
    from oracle import ref_model
    from pccx import models, synth as cloud_synth, train_ipdae
    from tests import synth
    buf = torch.empty(64 << 20, device="cuda", dtype=torch.float32)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:
        for _ in range(8):
            buf.fill_(1.0)
        torch.cuda.synchronize()
    del buf
    K, k, d, L, N = 256, 128, 16, 7, 8192
    ae, prob = models.AE(K=K, k=k, d=d, L=L), models.ConditionalProbabilityModel(L, d)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    kw = {} if mode == "default" else dict(octree_mode=mode)         # "default": no keyword, which another commit's tree also takes
    tr = train_ipdae.IpdaeTrainer(ae.cuda(), prob.cuda(), N=N, K=K, **kw)
    x = torch.from_numpy(cloud_synth.cad_cloud(900, N)[None].astype(np.float32)).cuda()
    st = torch.tensor([11], dtype=torch.int32, device="cuda")
    if case == "ipdae_graph":
        g = tr.graphed(x, st, warmup=2)
        fn = lambda: g(sync=False)
    else:
        fn = lambda: tr.step(x, st)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(case=case, mode=mode, ms_per_step=round((time.perf_counter() - t0) * 1e3 / steps, 4), steps=steps)))


def run(tree, case, mode, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--mode", mode, "--steps", str(steps)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, FULLCOST_ROOT=tree))
    if p.returncode != 0:
        raise SystemExit(f"{case} mode={mode} in {tree} ended with {p.returncode}: stop here\n{p.stderr[-2000:]}")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--other", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--child", default=None)
    ap.add_argument("--mode", default="default")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.mode, a.steps)
    table = {}
    for case in a.cases.split(","):
        for r in range(a.rounds):
            legs = [("reference", ROOT, "reference"), ("full", ROOT, "full")] + ([("other_reference", os.path.abspath(a.other), "default")] if a.other else [])
            for name, tree, mode in legs:
                ms = run(tree, case, mode, a.steps)
                table.setdefault(case, {}).setdefault(name, []).append(ms)
                print(json.dumps(dict(case=case, leg=name, round=r, ms_per_step=ms)), flush=True)
    print("\n| case | " + " | ".join(f"{n} (ms/step, each round)" for n in next(iter(table.values()))) + " |")
    for case, legs in table.items():
        print(f"| {case} | " + " | ".join(", ".join(f"{v:.3f}" for v in vs) for vs in legs.values()) + " |")


if __name__ == "__main__":
    main()
