#!/usr/bin/env python3
"""Cost of the entry-point index: Codec(p_index=G) against the single-stream codec and against Codec(p_split=G) on one
whole-room cloud.  A sibling of rooms_cost.py and region_cost.py with the same discipline: one FRESH process per figure, 0.3 s of
untimed fill kernels to settle the clocks, one warm-up call, then as many repeats as fit in about half a second (at least one)
between two synchronisations; the contenders take turns, `rounds` times; every child runs under a time limit of its own and the
first that fails or runs out of time ends the script.

    python tools/experiments/rooms_index_cost.py [--points 65536,1048576] [--g 16,64,128] [--rounds 3] [--parent-lib PATH]
                                                 [--only FIGURE,...] [--out profiles/rooms_index_cost.jsonl]

G is bounded by split_max_seg_sym(L) // d = 202 patches at d = 16, L = 7 (a segment is staged in LDS by one wave), so 256 is refused
on the host and the sweep's upper value is 128.

Per (points, G), K = 256 so S = points / 128 patches:
    encode_plain      models.range_encode on the cloud's tables and latents (the default path; with --parent-lib also from the
                      parent commit's library, the two taking turns: the spread the indexed encode is held against)
    encode_indexed    models.range_encode_indexed (the same stream + one 12-byte store per segment)
    decode_plain      models.range_decode (sequential)
    decode_indexed    models.range_decode_indexed (one wave per segment)
    decode_split      models.range_decode_split on the p_split stream of the same symbols
    build_index       models.range_index_build (the sequential decoder once)
    region_whole / region_64th  Codec.decompress_region through the index, and the same two through p_split (region_*_split)
--parent-lib: a libpccx.so built from the parent commit for the *_parent figures.  The child gets it as PCCX_LIB together with
PCCX_LIB_PARTIAL=1, because that library lacks the entry points this header declares beyond the parent's; the *_parent figures call
none of them."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "point-cloud-compression_amd")
sys.path[:0] = [HERE]
from grid_nn_cost import settle, timed  # noqa: E402

CODER = ["encode_plain", "encode_indexed", "decode_plain", "decode_indexed", "decode_split", "build_index"]
REGION = ["region_whole", "region_whole_split", "region_64th", "region_64th_split"]
PARENT = ["encode_plain_parent", "decode_plain_parent"]


def child(case, what):
    sys.path[:0] = [ROOT, PKG]
    import numpy as np
    import torch
    from oracle import ref_model
    from pccx import codec, models, ops, synth
    n, g = (int(v) for v in case.split("@"))
    K, d, L = 256, 16, 7
    S = n * 2 // K
    what = what.replace("_parent", "")
    ae = models.AE(K, K // 2, d, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, 3, last_gain={"pn.mlp_Modules.3.0": 40.0}))
    prob = models.ConditionalProbabilityModel(L, d)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, 4, gain=2.0))
    split = what.endswith("_split")
    kw = dict(p_split=g) if split else dict(p_index=g) if what in ("region_whole", "region_64th") else {}
    cd = codec.Codec(ae.pack("cuda"), prob.pack("cuda"), K=K, octree_mode="full", max_centres=codec.OCTREE_WIDE_MAX_S, **kw)
    pc = torch.from_numpy(synth.cad_batch(900, 1, n)).cuda()
    comp = cd.compress(pc, np.array([1]), keep_extras=True)
    cdf, q = comp.extras["cdf_int"], comp.extras["latent_q"].view(1, S * d)
    extra = {}
    if what.startswith("region"):
        side = comp.p_index
        comp = codec.Compressed.from_packed(comp.packed.clone(), 1, comp.s_bytes.shape[1], comp.p_bytes.shape[1], n)
        comp.p_index = side
        c = comp.c[0].tolist()
        rec, _ = ops.octree_decode(comp.s_bytes, comp.s_nbytes, "full", S)
        w = ops.denormalize(rec, comp.c[:, :3].contiguous(), comp.c[:, 3].contiguous(), cd.margin)[0]
        mid = w[S // 2].tolist()
        box = (w.amin(dim=0).tolist(), w.amax(dim=0).tolist()) if "whole" in what else ([v - c[3] / 8 for v in mid], [v + c[3] / 8 for v in mid])
        res = {}

        def fn():
            res["out"] = cd.decompress_region(comp, S, box)
    elif what == "encode_plain":
        fn = lambda: models.range_encode(cdf, q, L)
    elif what == "encode_indexed":
        fn = lambda: models.range_encode_indexed(cdf, q, L, g * d)
    elif what == "decode_plain":
        by, nb = models.range_encode(cdf, q, L)
        fn = lambda: models.range_decode(cdf, by, nb, L)
    elif what == "decode_indexed":
        by, nb, idx = models.range_encode_indexed(cdf, q, L, g * d)
        assert torch.equal(models.range_decode_indexed(cdf, by, nb, idx, L, g * d), models.range_decode(cdf, by, nb, L))
        fn = lambda: models.range_decode_indexed(cdf, by, nb, idx, L, g * d, check=False)
    elif what == "decode_split":
        by, nb = models.range_encode_split(cdf, q, L, g * d)
        fn = lambda: models.range_decode_split(cdf, by, nb, L, g * d, check=False)
    elif what == "build_index":
        by, nb = models.range_encode(cdf, q, L)
        fn = lambda: models.range_index_build(cdf, by, nb, L, g * d)
    else:
        raise SystemExit(f"unknown figure {what}")
    settle()
    ms, reps = timed(fn)
    if what.startswith("region"):
        extra = dict(patches=res["out"].patch_idx.numel(), segments=res["out"].segments.numel())
    print(json.dumps(dict(case=case, ms=ms, reps=reps, **extra)))


def run(case, what, limit_s, parent_lib):
    env = dict(os.environ)
    if what.endswith("_parent"):
        env["PCCX_LIB"], env["PCCX_LIB_PARTIAL"] = os.path.abspath(parent_lib), "1"
    cmd = ["timeout", "-k", "10", str(int(limit_s)), sys.executable, os.path.abspath(__file__), "--child", case, "--what", what]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if p.returncode != 0:
        raise SystemExit(f"{what} at {case} ended with {p.returncode} (limit {int(limit_s)} s): stop here\n{p.stderr[-2000:]}")
    return dict(json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1]), what=what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="65536,1048576")
    ap.add_argument("--g", default="16,64,128")
    ap.add_argument("--only", default=None, help="comma-separated figures to run instead of all")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-region", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--what", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.what)
    out = open(a.out, "a") if a.out else None
    whats = CODER + (PARENT if a.parent_lib else []) + ([] if a.skip_region else REGION)
    if a.only:
        whats = [w for w in a.only.split(",") if w in CODER + PARENT + REGION]
    # the contenders of one comparison next to each other in every round
    order = ["encode_plain_parent", "encode_plain", "encode_indexed", "decode_plain_parent", "decode_plain", "decode_indexed", "decode_split",
             "build_index"] + REGION
    whats = [w for w in order if w in whats]
    table = {}
    for n in (int(v) for v in a.points.split(",")):
        for g in (int(v) for v in a.g.split(",")):
            case = f"{n}@{g}"
            for r in range(a.rounds):
                for what in whats:
                    rec = dict(run(case, what, 180, a.parent_lib), round=r)
                    table.setdefault((case, what), []).append(rec)
                    print(json.dumps(rec), flush=True)
                    if out:
                        out.write(json.dumps(rec) + "\n")
                        out.flush()
    lines = ["| points@G | figure | ms, each round |", "|---|---|---|"]
    lines += [f"| {case} | {what} | {', '.join('%.3f' % rec['ms'] for rec in v)} |" for (case, what), v in table.items()]
    print("\n" + "\n".join(lines))
    if out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
