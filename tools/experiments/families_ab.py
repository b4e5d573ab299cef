"""A/B record of pccx.families for a host-only change: every library call the forwards issue and a hash of every output.

  python tools/experiments/families_ab.py --dump DIR [--root CHECKOUT]    one side, in a fresh process (writes DIR/families_ab.json)
  python tools/experiments/families_ab.py --compare DIR_A DIR_B           exit 0 iff no hash and no call sequence differs
  python tools/experiments/families_ab.py --time-pppe B [--h2-stacks off] [--root CHECKOUT]
                                                                          ms per PointCloudAE(64, 16, 8192).forward on B clouds (f16x2), one
                                                                          figure per fresh process; off = the bf16x3 rows path of the parent

--dump wraps _lib.call and records each entry point's name with its non-pointer arguments (pointers change from run to run; the
header's types say which arguments they are), then runs PPPF_AE.forward in f32 / bf16x3 / f16x2 under each class switch, one at a
time, on the fixture input, a ragged batch and an empty batch, and one PointCloudAE.forward in f32, bf16x3 and f16x2, the last one
also with PointCloudAE.h2_stacks = False (the rows path; a checkout without the switch runs it either way).  Every combination
gets a freshly packed model, so the lazily built weight streams appear in its record at the call that first needs them.  An
exception is part of the record (the empty batch: whatever one side does, the other must do).  --root runs another checkout of
the project (the parent commit) with this same script.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ARITHMETICS = ("f32", "bf16x3", "f16x2")
SWITCHES = (None, ("PointnetSAModule", "dedup"), ("PointnetSAModule", "union_max"), ("PointnetSAModule", "padded_levels"), ("PPPF_AE", "split_fold"))


def digest(t):
    a = t.detach().cpu().contiguous().numpy()
    return "%s %s %s" % (tuple(a.shape), a.dtype, hashlib.sha256(a.tobytes()).hexdigest())


def dump(out_dir, root):
    sys.path[:0] = [root, os.path.join(root, "point-cloud-compression_amd")]
    import numpy as np
    import torch
    import pccx
    from oracle import ref_families as rf
    from pccx import _lib, families
    from tests import synth

    print("pccx.families from", os.path.relpath(families.__file__, root), "under", root, flush=True)
    sig = _lib.signatures()
    calls, real_call = [], _lib.call

    def recording_call(name, *args):
        types = sig[name][1]
        calls.append([name] + [repr(a) for a, t in zip(args, types) if t not in (ctypes.c_void_p, ctypes.c_char_p)])
        return real_call(name, *args)

    _lib.call = recording_call

    def record(fn):
        """outputs (or the exception) and the calls of one forward"""
        del calls[:]
        try:
            res = {"out": [digest(t) for t in fn()]}
            torch.cuda.synchronize()
        except (_lib.PccxError, RuntimeError, ValueError, IndexError, ZeroDivisionError) as e:
            res = {"error": "%s: %s" % (type(e).__name__, e)}
            if "PccxError" not in res["error"]:
                torch.cuda.synchronize()              # a device fault surfaces here and ends the run: nothing more is started
        res["calls"] = [list(c) for c in calls]
        return res

    inputs = {"fixture": synth.pppf_input(), "ragged": (np.random.default_rng(2).random((3, 512, 3)) * 1.6).astype(np.float32),
              "empty": np.zeros((0, 512, 3), np.float32)}
    old, results = pccx.DEFAULT_MATMUL, {}
    try:
        for arith in ARITHMETICS:
            pccx.DEFAULT_MATMUL = arith
            for sw in SWITCHES:
                g = families.PPPF_AE(512, 0, 16, 7)
                g.load_state_dict(synth.family_tweak(rf.seeded_with_bn(g, synth.PPPF_SEED), "pppf"))
                if sw is not None:
                    setattr(getattr(families, sw[0]), sw[1], False)
                try:
                    for name, x in inputs.items():
                        key = "pppf %s %s %s" % (arith, "default" if sw is None else sw[1] + "=False", name)
                        results[key] = record(lambda: g(torch.from_numpy(x).cuda()))
                        print(key, results[key].get("error", "ok"), len(results[key]["calls"]), "calls", flush=True)
                finally:
                    if sw is not None:
                        setattr(getattr(families, sw[0]), sw[1], True)
        s = np.load(os.path.join(root, "tests", "golden", "families.npz"))["pppe_starts"]
        for arith, h2 in (("f32", True), ("bf16x3", True), ("f16x2", True), ("f16x2", False)):
            pccx.DEFAULT_MATMUL = arith
            p = families.PointCloudAE(64, 16, 8192)
            p.load_state_dict(synth.family_tweak(rf.seeded_with_bn(p, synth.PPPE_SEED), "pppe"))
            key = "pppe %s%s" % (arith, "" if h2 else " h2_stacks=False")
            default = getattr(families.PointCloudAE, "h2_stacks", None)
            families.PointCloudAE.h2_stacks = h2
            try:
                results[key] = record(lambda: p(torch.from_numpy(synth.pppe_input()).cuda(), [[s[0], s[1]], s[2], s[3]]))
            finally:
                families.PointCloudAE.h2_stacks = default
            print(key, results[key].get("error", "ok"), len(results[key]["calls"]), "calls", flush=True)
    finally:
        pccx.DEFAULT_MATMUL = old
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "families_ab.json"), "w") as f:
        json.dump(results, f, indent=0)


def time_pppe(B, h2, root, steps=20):
    """ms per PointCloudAE(64, 16, 8192).forward on B clouds in f16x2 (h2=False: the rows path), after bench.settle() and two warm-up calls"""
    sys.path[:0] = [root, os.path.join(root, "point-cloud-compression_amd")]
    import time
    import types
    import numpy as np
    import torch
    import bench
    import pccx
    from oracle import ref_families as rf
    from pccx import families, synth as cloud_synth
    from tests import synth

    pccx.DEFAULT_MATMUL = "f16x2"
    families.PointCloudAE.h2_stacks = h2
    p = families.PointCloudAE(64, 16, 8192)
    p.load_state_dict(synth.family_tweak(rf.seeded_with_bn(p, synth.PPPE_SEED), "pppe"))
    x = torch.from_numpy(np.stack([cloud_synth.cad_cloud(300 + b % 8, 8192) for b in range(B)]).astype(np.float32)).cuda()
    rng = np.random.default_rng(0)
    starts = [[rng.integers(0, 8192, B), rng.integers(0, 8192, B)], rng.integers(0, 512, B), rng.integers(0, 128, B)]
    bench.settle(types.SimpleNamespace(gpu=True, dev="cuda:0"))
    for _ in range(2):
        p(x, starts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        p(x, starts)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    print(json.dumps({"pppe_forward_ms": round(ms, 4), "B": B, "h2_stacks": bool(h2 and "h2" in p._packed), "steps": steps}), flush=True)


def compare(dir_a, dir_b):
    a, b = (json.load(open(os.path.join(d, "families_ab.json"))) for d in (dir_a, dir_b))
    bad = 0
    for key in sorted(set(a) | set(b)):
        ra, rb = a.get(key), b.get(key)
        if ra is None or rb is None:
            print("%s: only on one side" % key)
            bad += 1
            continue
        for field in ("out", "error"):
            if ra.get(field) != rb.get(field):
                print("%s: %s differs\n  A %s\n  B %s" % (key, field, ra.get(field), rb.get(field)))
                bad += 1
        if ra["calls"] != rb["calls"]:
            i = next((i for i, (x, y) in enumerate(zip(ra["calls"], rb["calls"])) if x != y), min(len(ra["calls"]), len(rb["calls"])))
            print("%s: call %d differs (%d / %d calls)\n  A %s\n  B %s" % (key, i, len(ra["calls"]), len(rb["calls"]),
                                                                         ra["calls"][i:i + 1], rb["calls"][i:i + 1]))
            bad += 1
    print("%d combinations, %d library calls a side, %d differences" % (len(a), sum(len(r["calls"]) for r in a.values()), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    ap.add_argument("--time-pppe", type=int, metavar="B")
    ap.add_argument("--h2-stacks", choices=("on", "off"), default="on")
    args = ap.parse_args()
    if args.time_pppe:
        sys.exit(time_pppe(args.time_pppe, args.h2_stacks == "on", os.path.abspath(args.root)))
    if args.compare:
        sys.exit(compare(*args.compare))
    dump(args.dump, os.path.abspath(args.root))
