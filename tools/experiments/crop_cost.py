#!/usr/bin/env python3
"""Cost of cutting training crops on the GPU: ops.crop_nearest beside what a user would write in torch, and beside the
training step the crops feed.

    python tools/experiments/crop_cost.py [--rounds 3] [--calls 50]

Same box, ALTERNATING legs, one fresh process per figure (each settles the clocks with 0.3 s of untimed fill kernels, warms its leg up,
then times `calls` calls -- twenty times as many of the crop, whose call is short -- between two synchronisations), `rounds` times round:
  crop_b4 / torch_b4        B = 4 crops of 8192 points from one room_cloud of 1 048 576 points (four seed points of that room)
  crop_b1 / torch_b1        B = 1 crop of 131072 points from the same room
  step                      the dense full-mode IPDAE step at --N 8192, --batch_size 4, K = 256, as a captured graph
The torch legs do the same job per crop: ((p - s) ** 2).sum(1), a stable sort, the first n, their indices sorted, a gather.  The crop
legs run with host tables, as CropSampler calls them (three small uploads per call included).  One JSON line per figure, a table at the end."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEGS = ("crop_b4", "torch_b4", "crop_b1", "torch_b1", "step")
M = 1 << 20


def child(leg, calls):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-compression_amd")]
    import numpy as np
    import torch
    from pccx import codec, models, ops, synth as cloud_synth, train_ipdae
    buf = torch.empty(64 << 20, device="cuda", dtype=torch.float32)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:
        for _ in range(8):
            buf.fill_(1.0)
        torch.cuda.synchronize()
    del buf
    if leg == "step":
        from oracle import ref_model
        from tests import synth
        K, k, d, L, N = 256, 128, 16, 7, 8192
        ae, prob = models.AE(K=K, k=k, d=d, L=L), models.ConditionalProbabilityModel(L, d)
        ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
        prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
        tr = train_ipdae.IpdaeTrainer(ae.cuda(), prob.cuda(), N=N, K=K, octree_mode="full")
        x = torch.from_numpy(cloud_synth.cad_batch(900, 4, N).astype(np.float32)).cuda()
        g = tr.graphed(x, torch.tensor([11, 7, 4000, 8191], dtype=torch.int32, device="cuda"), warmup=2)
        fn = lambda: g(sync=False)
    else:
        B, n = (4, 8192) if leg.endswith("b4") else (1, 131072)
        points, offsets, sizes = codec.pack_clouds([cloud_synth.room_cloud(7, M)], device="cuda")
        seeds = [5, 400000, 777777, M - 1][:B]
        if leg.startswith("crop"):
            ws = torch.empty(ops._lib.load().pccx_crop_nearest_workspace_bytes(B, M), dtype=torch.uint8, device="cuda")
            out = torch.empty(B, n, 3, device="cuda")
            fn = lambda: ops.crop_nearest(points, offsets, [0] * B, seeds, [n] * B, n, workspace=ws, sizes=sizes, out=out)
        else:
            def fn():
                outs = []
                for s in seeds:
                    d2 = ((points - points[s]) ** 2).sum(1)
                    idx = torch.sort(d2, stable=True).indices[:n].sort().values
                    outs.append(points[idx])
                return torch.stack(outs)
    calls *= 20 if leg.startswith("crop") else 1
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(leg=leg, ms_per_call=round((time.perf_counter() - t0) * 1e3 / calls, 4), calls=calls)))


def run(leg, calls):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--calls", str(calls)], capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"{leg} ended with {p.returncode}: stop here\n{p.stderr[-2000:]}")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])["ms_per_call"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls)
    table = {}
    for r in range(a.rounds):
        for leg in a.legs.split(","):
            ms = run(leg, a.calls)
            table.setdefault(leg, []).append(ms)
            print(json.dumps(dict(leg=leg, round=r, ms_per_call=ms)), flush=True)
    print("\n| leg | ms per call, each round |")
    for leg, vs in table.items():
        print(f"| {leg} | " + ", ".join(f"{v:.3f}" for v in vs) + " |")


if __name__ == "__main__":
    main()
