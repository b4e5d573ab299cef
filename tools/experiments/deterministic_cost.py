#!/usr/bin/env python3
"""Cost of the deterministic training mode, and the default path against another tree.

    python tools/experiments/deterministic_cost.py [--rounds 3] [--steps 20] [--other PATH_TO_ANOTHER_CHECKOUT]

Same box, ALTERNATING runs, one fresh process per measurement (each settles the clocks with 0.3 s of untimed fill kernels, then runs
warm-up steps, then times `steps` steps between two synchronisations): for every case -- IPDAE at the reference's shape (batch 1, 8192
points, K = 256) eager and as a graph, pppe at batch 4 and batch 64 as a graph -- the switch off and on take turns `rounds` times.
--other: a built checkout of another commit (the parent); its switch-off step time is then measured in the same alternation, which is
the check that the default path did not slow down.  --band: the step-10 loss of the 20-step bf16-vs-fp32 comparison of
tests/test_train_step.py under the switch, `--band` repeats.  One JSON line per measurement, a summary table at the end."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = ("ipdae_eager", "ipdae_graph", "pppe4_graph", "pppe64_graph")


def child(case, det, steps):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-compression_amd")]
    import numpy as np
    import torch
    from oracle import ref_families as rf, ref_model
    from pccx import families, models, synth as cloud_synth, train, train_ipdae
    from tests import synth
    kw = dict(deterministic=True) if det else {}
    buf = torch.empty(64 << 20, device="cuda", dtype=torch.float32)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:
        for _ in range(8):
            buf.fill_(1.0)
        torch.cuda.synchronize()
    del buf
    if case.startswith("ipdae"):
        K, k, d, L, N = 256, 128, 16, 7, 8192
        ae, prob = models.AE(K=K, k=k, d=d, L=L), models.ConditionalProbabilityModel(L, d)
        ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
        prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
        tr = train_ipdae.IpdaeTrainer(ae.cuda(), prob.cuda(), N=N, K=K, **kw)
        x = torch.from_numpy(cloud_synth.cad_cloud(900, N)[None].astype(np.float32)).cuda()
        st = torch.tensor([11], dtype=torch.int32, device="cuda")
        if case == "ipdae_graph":
            g = tr.graphed(x, st, warmup=2)
            fn = lambda: g(sync=False)
        else:
            fn = lambda: tr.step(x, st)
    else:
        B, N = int(case[4:].split("_")[0]), 2048
        o = rf.PointCloudAE(64, 16, N)
        o.load_state_dict(synth.family_tweak(rf.seeded_with_bn(o, synth.PPPE_SEED), "pppe"))
        g_ = families.PointCloudAE(64, 16, N)
        g_.load_state_dict(o.state_dict())
        g_ = g_.cuda()
        opt = train.Adam(g_.parameters(), lr=1e-3)
        x = torch.from_numpy(np.stack([cloud_synth.cad_cloud(700 + b, N) for b in range(B)]).astype(np.float32)).cuda()
        rng = np.random.default_rng(5)
        starts = [[rng.integers(0, N, B), rng.integers(0, N, B)], rng.integers(0, 512, B), rng.integers(0, 128, B)]
        gs = train.GraphedTrainStep(g_, opt, x, starts, lam=0.5, warmup=2, **kw)
        fn = lambda: gs(sync=False)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(case=case, det=bool(det), ms_per_step=round((time.perf_counter() - t0) * 1e3 / steps, 4), steps=steps)))


def band(repeats, det):
    """step-10 loss of the 20-step bf16-vs-fp32 comparison (tests/test_train_step.py's last test), `repeats` runs of each arithmetic"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-compression_amd")]
    import numpy as np
    import torch
    from oracle import ref_families as rf
    from pccx import families, synth as cloud_synth, train
    from tests import synth
    N, B = 2048, 4
    x = torch.from_numpy(np.stack([cloud_synth.cad_cloud(700 + b, N) for b in range(B)]).astype(np.float32)).cuda()
    o = rf.PointCloudAE(64, 16, N)
    o.load_state_dict(synth.family_tweak(rf.seeded_with_bn(o, synth.PPPE_SEED), "pppe"))
    for rep in range(repeats):
        row = {}
        for ac in (False, True):
            g = families.PointCloudAE(64, 16, N)
            g.load_state_dict(o.state_dict())
            g = g.cuda()
            opt = train.Adam(g.parameters(), lr=1e-3)
            rng = np.random.default_rng(9)
            for it in range(11):
                starts = [[rng.integers(0, N, B), rng.integers(0, N, B)], rng.integers(0, 512, B), rng.integers(0, 128, B)]
                loss, dist, rate = train.train_step(g, opt, x, starts, lam=0.5, autocast=ac, **(dict(deterministic=True) if det else {}))
            row["bf16" if ac else "fp32"] = loss
        print(json.dumps(dict(band_repeat=rep, det=bool(det), step10_loss=row, ratio=row["bf16"] / row["fp32"])))


def run(tree, case, det, steps):
    cmd = [sys.executable, os.path.join(tree, "tools", "experiments", "deterministic_cost.py"), "--child", case, "--steps", str(steps)] + (["--det"] if det else [])
    if not os.path.exists(cmd[1]):                      # another commit's tree has no copy of this script: run this one against its package
        cmd[1] = os.path.abspath(__file__)
    env = dict(os.environ, DETCOST_ROOT=tree)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    if p.returncode != 0:
        raise SystemExit(f"{case} det={det} in {tree} ended with {p.returncode}: stop here\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--other", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--band", type=int, default=0)
    ap.add_argument("--child", default=None)
    ap.add_argument("--det", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.det, a.steps)
    if a.band:
        band(a.band, False)
        return band(a.band, True)
    table = {}
    for case in a.cases.split(","):
        for r in range(a.rounds):
            legs = [("off", ROOT, False), ("on", ROOT, True)] + ([("other_off", os.path.abspath(a.other), False)] if a.other else [])
            for name, tree, det in legs:
                ms = run(tree, case, det, a.steps)
                table.setdefault(case, {}).setdefault(name, []).append(ms)
                print(json.dumps(dict(case=case, leg=name, round=r, ms_per_step=ms)), flush=True)
    print("\n| case | " + " | ".join(f"{n} (ms/step, each round)" for n in next(iter(table.values()))) + " |")
    for case, legs in table.items():
        print(f"| {case} | " + " | ".join(", ".join(f"{v:.3f}" for v in vs) for vs in legs.values()) + " |")


if __name__ == "__main__":
    if os.environ.get("DETCOST_ROOT"):
        ROOT = os.environ["DETCOST_ROOT"]
    main()
