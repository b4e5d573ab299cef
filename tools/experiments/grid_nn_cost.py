#!/usr/bin/env python3
"""Cost of the grid-indexed searches (csrc/grid_nn.hip, ops.GridIndex) against the all-pairs kernels.

    python tools/experiments/grid_nn_cost.py [--rounds 3] [--cases 8192,65536,1000000,8192x256] [--variants t1,t4] [--out FILE] [--base FILE]
    python tools/experiments/grid_nn_cost.py --cases "" --wide 64x64x8192x256,4x256x32768x256 [--targets 2,8,32] --codec 65536,131072

One FRESH process per figure; each settles the clocks with 0.3 s of untimed fill kernels, warms its call up once and then
times it between two synchronisations (as many repeats as fit in about half a second, at least one).  Grid and brute force take turns,
`rounds` times.  Cases: the synthetic room (pccx.synth.room_cloud) with P = Q points and B = 1, and 256 CAD clouds of 8192 points.
Figures per case: the index build, nn, knn(30) and the whole of large.evaluate_large through the grid; nn_dist, knn_points(30) and
the three codec metrics by the all-pairs calls.  pccx_knn takes at most 32768 reference points: above that its two figures are
recorded as unsupported, not estimated.
Every child runs under a time limit of its own, sized from the 8192-point figures (quadratic in the points for the all-pairs calls,
linear for the grid, with a wide margin), and the first child that fails or runs out of time ends the script.
--variants: libraries built with another GRID_TARGET or GRID_MAX_CELLS in csrc/grid_nn.hip (edit the constant, then PCCX_BUILD_TAG=<tag>
python -m pccx.build, which leaves pccx/lib/libpccx_<tag>.so beside the product); their build, nn and knn(30) figures are taken once,
after the rounds, for the cases of 65536 points and more.  --base: the --out file of an earlier run whose 8192-point figures size the limits when
this run leaves that case out.
--wide BxMxNxK: the codec's patch search (M centres per cloud, the K nearest of N points, patches only) by pccx_knn_list and by
GridIndex.knn_wide, for every --targets value (points per cell of the index; 2 = the library's own build) with the index prebuilt
(wide_query) and built inside the timed call (wide_total).  --codec N: one CAD cloud of N points, K = 256, octree_mode "full", seeded
weights, through Codec.compress + decompress as one cloud (codec_whole) and through large.compress_large + decompress_large in
8192-point blocks (codec_blocks): ms per cloud, ops.StageTimer's per-stage totals, bits per point and codec.d1_psnr of the result.
All of these run in the same alternating rounds, one fresh process per figure, under a limit of 300 s each."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "point-cloud-compression_amd")
GRID = ("grid_build", "grid_nn", "grid_knn30", "grid_evaluate")
BRUTE = ("brute_nn", "brute_knn30", "brute_evaluate")
KNN_LIMIT = 32768


def clouds(case):
    import numpy as np
    import torch
    from pccx import synth
    if "x" in case:
        n, B = (int(v) for v in case.split("x"))
        y = synth.cad_batch(300, B, n)
    else:
        n, B = int(case), 1
        y = synth.room_cloud(3, n)[None]
    rng = np.random.default_rng(4)
    x = (y + rng.normal(0, 0.004 * float(y.max() - y.min()), size=y.shape)).astype(np.float32)      # a reconstruction: jittered copy
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def child(case, what):
    sys.path[:0] = [ROOT, PKG]
    import torch
    from pccx import codec, large, ops
    x, y = clouds(case)
    buf = torch.empty(64 << 20, device="cuda", dtype=torch.float32)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:
        for _ in range(8):
            buf.fill_(1.0)
        torch.cuda.synchronize()
    del buf
    index = ops.GridIndex(y) if what in ("grid_nn", "grid_knn30") else None
    fn = {"grid_build": lambda: ops.GridIndex(y),
          "grid_nn": lambda: index.nn(x, return_idx=True),
          "grid_knn30": lambda: index.knn(y, 30),
          "grid_evaluate": lambda: ([large.evaluate_large(y[b], x[b]) for b in range(y.shape[0])] if y.shape[0] <= 4 else
                                    (codec.d1_psnr(y, x, search="grid").sum() + codec.d2_psnr(y, x, search="grid").sum()
                                     + codec.normalized_chamfer(y, x, search="grid").sum()).item()),
          "brute_nn": lambda: ops.nn_dist(x, y, return_idx=True),
          "brute_knn30": lambda: ops.knn_points(y, y, 30, return_nn=False),
          "brute_evaluate": lambda: (codec.d1_psnr(y, x).sum() + codec.d2_psnr(y, x).sum() + codec.normalized_chamfer(y, x).sum()).item()}[what]
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    reps = max(1, min(50, int(0.5 / max(first, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(case=case, what=what, ms=round((time.perf_counter() - t0) * 1e3 / reps, 4), reps=reps, lib=os.environ.get("PCCX_LIB", ""))))


def settle():
    import torch
    buf = torch.empty(64 << 20, device="cuda", dtype=torch.float32)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:
        for _ in range(8):
            buf.fill_(1.0)
        torch.cuda.synchronize()


def timed(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    reps = max(1, min(50, int(0.5 / max(first, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / reps, 4), reps


def child_wide(case, what):
    sys.path[:0] = [ROOT, PKG]
    import torch
    from pccx import ops, synth
    B, M, N, K = (int(v) for v in case.split("x"))
    y = torch.from_numpy(synth.cad_batch(300, B, N)).cuda()
    x = ops.index_points(y, ops.farthest_point_sample_batch(y, M, [0] * B))       # FPS centres, as the codec's are
    scale = float((N / 1024) ** (1 / 3))
    kw = dict(return_nn=True, patch_scale=scale, return_dists=False, return_idx=False)
    settle()
    name, _, t = what.partition("@")
    target = None if t in ("", "2") else int(t)
    index = ops.GridIndex(y, target) if name == "wide_query" else None
    fn = {"brute_knn_list": lambda: ops.knn_points(x, y, K, **kw),
          "wide_query": lambda: index.knn_wide(x, K, **kw),
          "wide_total": lambda: ops.GridIndex(y, target).knn_wide(x, K, **kw)}[name]
    ms, reps = timed(fn)
    print(json.dumps(dict(case=case, what=what, ms=ms, reps=reps)))


def child_codec(case, what):
    sys.path[:0] = [ROOT, PKG]
    import numpy as np
    import torch
    from oracle import ref_model
    from pccx import codec, large, models, ops, synth
    N, K, d, L = int(case), 256, 16, 7
    ae = models.AE(K, K // 2, d, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, 3, last_gain={"pn.mlp_Modules.3.0": 40.0}))
    prob = models.ConditionalProbabilityModel(L, d)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, 4, gain=2.0))
    cd = codec.Codec(ae.pack("cuda"), prob.pack("cuda"), K=K, octree_mode="full")
    pc = torch.from_numpy(synth.cad_batch(900, 1, N)).cuda()
    res = {}
    if what == "codec_whole":
        def fn():
            res["comp"] = [cd.compress(pc, np.array([1]))]
            res["out"] = cd.decompress(res["comp"][0], S=N * 2 // K)
    else:
        def fn():
            parts, nb, order, _ = large.compress_large(cd, pc[0])
            res["comp"] = [c for _, c in parts]
            res["out"] = large.decompress_large(cd, parts, nb, order, N)[None]
    settle()
    ms, reps = timed(fn)
    timer = ops.StageTimer()
    ops.set_timer(timer)
    fn()
    stages = {k: round(v[0], 3) for k, v in timer.totals_ms().items()}
    ops.set_timer(None)
    nbytes = sum(len(f) for c in res["comp"] for b in range(c.s_bytes.shape[0]) for f in c.files(b))
    print(json.dumps(dict(case=case, what=what, ms=ms, reps=reps, bpp=round(8 * nbytes / N, 4),
                          d1_psnr=round(float(codec.d1_psnr(pc, res["out"].reshape(1, -1, 3), search="grid")[0]), 3), stages=stages)))


def run(case, what, limit_s, lib=None, mode=None):
    env = dict(os.environ)
    if lib:
        env["PCCX_LIB"] = lib
    cmd = ["timeout", "-k", "10", str(int(limit_s)), sys.executable, os.path.abspath(__file__), "--child", case, "--what", what]
    cmd += ["--mode", mode] if mode else []
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if p.returncode != 0:
        raise SystemExit(f"{what} at {case} ended with {p.returncode} (limit {int(limit_s)} s): stop here\n{p.stderr[-2000:]}")
    rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    return rec if mode else rec["ms"]


def points(case):
    n, B = (int(v) for v in case.split("x")) if "x" in case else (int(case), 1)
    return n, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="8192,65536,1000000,8192x256")
    ap.add_argument("--variants", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--base", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--what", default=None)
    ap.add_argument("--wide", default="")
    ap.add_argument("--targets", default="2,8,32")
    ap.add_argument("--codec", default="")
    ap.add_argument("--mode", default=None)
    a = ap.parse_args()
    if a.child:
        return {"wide": child_wide, "codec": child_codec, None: child}[a.mode](a.child, a.what)
    cases = [c for c in a.cases.split(",") if c]
    table, base = {}, {}
    out = open(a.out, "a") if a.out else None
    if a.base:
        for line in open(a.base):
            rec = json.loads(line) if line.startswith("{") else {}
            if rec.get("case") == "8192" and "variant" not in rec:
                base[rec["what"]] = max(base.get(rec["what"], 0.0), rec["ms"])

    def note(rec):
        print(json.dumps(rec), flush=True)
        if out:
            out.write(json.dumps(rec) + "\n")
            out.flush()

    for case in cases:
        n, B = points(case)
        for r in range(a.rounds):
            for g, b in zip(GRID, BRUTE + (None,)):                      # grid and brute force take turns
                for what in (g, b):
                    if what is None:
                        continue
                    if what in ("brute_knn30", "brute_evaluate") and n > KNN_LIMIT:
                        table.setdefault(case, {}).setdefault(what, "unsupported: pccx_knn takes at most 32768 reference points")
                        continue
                    # the limit: start-up + the 8192-point figure scaled to this case (n^2 for all pairs, n for the grid), times 20
                    ref_ms = base.get(what, 1000.0)
                    scale = (n / 8192.0) ** 2 * B if what.startswith("brute") else (n / 8192.0) * B
                    limit = 90 + 20 * 3 * ref_ms * 1e-3 * scale                  # a child makes three calls when one takes long
                    ms = run(case, what, min(limit, 900))
                    if case == "8192":
                        base[what] = max(base.get(what, 0.0), ms)
                    table.setdefault(case, {}).setdefault(what, []).append(ms)
                    note(dict(case=case, what=what, round=r, ms=ms))
        for tag in [t for t in a.variants.split(",") if t and n >= 65536]:
            lib = os.path.join(PKG, "pccx", "lib", f"libpccx_{tag}.so")
            for what in ("grid_build", "grid_nn", "grid_knn30"):
                ms = run(case, what, 300, lib=lib)
                table.setdefault(case, {}).setdefault(f"{what}[{tag}]", []).append(ms)
                note(dict(case=case, what=what, variant=tag, ms=ms))
    wide_whats = ["brute_knn_list"] + [f"{w}@{t}" for t in a.targets.split(",") for w in ("wide_query", "wide_total")]
    for r in range(a.rounds):
        for mode, mcases, whats in (("wide", a.wide, wide_whats), ("codec", a.codec, ["codec_whole", "codec_blocks"])):
            for case in [c for c in mcases.split(",") if c]:
                for what in whats:
                    rec = run(case, what, 300, mode=mode)
                    table.setdefault(f"{mode} {case}", {}).setdefault(what, []).append(rec["ms"])
                    note(dict(rec, round=r))
    lines = ["| case | figure | ms, each round |", "|---|---|---|"]
    for case, row in table.items():
        for what, v in row.items():
            lines.append(f"| {case} | {what} | {v if isinstance(v, str) else ', '.join(f'{m:.3f}' for m in v)} |")
    print("\n" + "\n".join(lines))
    if out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
