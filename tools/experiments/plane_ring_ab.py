"""A/B record for a restructuring of the plane-ring GEMM loop (csrc/plane_ring.h): SHA-256 over the raw output bytes of every kernel
that runs it, at the smallest shapes where tiling, register rotation or clamping can go wrong, for a fixed seed.

  python tools/experiments/plane_ring_ab.py [--root CHECKOUT] > side.json      one side, in a fresh process

Run it once on a checkout of the parent commit (--root) and once on this tree; the two JSONs must be equal.
  decoders   AE.decode in f32, bf16x3 (PCCX_DEC_NT unset and 4) and f16x2 (PCCX_DEC_H2_NT unset and 2; with and without the list of
             distinct patches), patches and reassembled cloud; P in {1, 17, 129, 257}, d in {1, 16}, k in {128 (the default), 1}
  layer      pccx_planes_gemm / _gather (both arithmetics; row, planes and max epilogue); M in {1, 17, 129}, K in {3, 32, 33, 64, 96, 128}
             (1, 1, 2, 2, 3, 4 k-steps: every branch of the conditional rotation, and a dead third set), N in {16, 75, 128}; the max
             epilogue reduces groups of 32 rows, so it runs on 32 M rows
  chain4     pccx_planes_chain4 / _gather (both arithmetics) on the four width cases of tests/test_planes_h2.py at M in {17, 129} rows,
             and their max over groups of 32 on 32 M rows
"""
import argparse
import hashlib
import json
import os
import sys

CHAIN_CASES = [(3, (3, 64, 64, 128)), (131, (128, 128, 128, 256)), (7, (20, 40, 64, 100)), (70, (100, 128, 97, 200))]


def digest(t):
    a = t.detach().cpu().contiguous().numpy()
    return hashlib.sha256(a.tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    root = os.path.abspath(ap.parse_args().root)
    sys.path[:0] = [os.path.join(root, "point-cloud-compression_amd")]
    import numpy as np
    import torch
    from pccx import families, models

    out = {}
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    # ---- decoders
    for kx in (128, 1):
        for dx in (1, 16):
            torch.manual_seed(1000 * kx + dx)
            ae = models.AE(256, kx, dx, 7).pack("cuda")
            for P in (1, 17, 129, 257):
                rng = np.random.default_rng(P)
                lq = cu(rng.integers(-3, 4, size=(P, dx)).astype(np.float32))
                # every third patch repeats its neighbour's centre and latent: the list of distinct patches is shorter than P
                rep = np.arange(P) - (np.arange(P) % 3 == 2)
                lq = lq[cu(rep)].contiguous()
                centres = cu(((rng.integers(0, 128, size=(1, P, 3)) + 0.5) / 128).astype(np.float32)[:, rep])
                cloud = dict(centres=centres, center=cu(rng.normal(size=(1, 3)).astype(np.float32)),
                             longest=cu((1 + rng.random(1)).astype(np.float32)), S=P, scale=float((P * kx / 1024) ** (1 / 3)))
                for mode, env, values in (("f32", "PCCX_DEC_NT", (None,)), ("bf16x3", "PCCX_DEC_NT", (None, "4")), ("f16x2", "PCCX_DEC_H2_NT", (None, "2"))):
                    for v in values:
                        os.environ.pop(env, None)
                        if v is not None:
                            os.environ[env] = v
                        tag = f"decode {mode} {env}={v} k={kx} d={dx} P={P}"
                        out[tag + " patches"] = digest(ae.decode(lq, matmul=mode))
                        out[tag + " cloud"] = digest(ae.decode(lq, matmul=mode, **cloud))
                        if mode == "f16x2":
                            out[tag + " cloud uniq"] = digest(ae.decode(lq, matmul=mode, group=True, **cloud))
                        os.environ.pop(env, None)

    # ---- one layer
    def layer(rng, N, K, relu, ar):
        W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        b = rng.standard_normal(N).astype(np.float32)
        return families.FoldedLinear(torch.from_numpy(W), torch.from_numpy(b), relu, matmul=ar)

    def prepared(layers, ar):
        stack = families.Stack(layers)
        if ar == "f16x2":
            families.h2_prepare_stack(stack, np.full(stack[0].K, -1.0), np.ones(stack[0].K))
        return stack

    def inputs(rng, rows, K, group, stack, ar):
        """the same `rows` input rows as planes and as (source rows, idx) of the gathering form; -1 -> row 0 as the ball query pads"""
        n_src = 23
        src = cu(rng.uniform(-1.0, 1.0, (1, n_src, K)).astype(np.float32))
        idx = cu(rng.integers(-1, n_src, (1, rows // group, group)))
        sig = stack[0].h2["sig"] if ar == "f16x2" else None
        pl, r = families.group_planes(src, None, idx, ar=ar, sig=sig)
        assert r == rows
        return pl, families.padded_rows(src, None)[0], idx

    for ar in ("bf16x3", "f16x2"):
        for K in (3, 32, 33, 64, 96, 128):
            for N in (16, 75, 128):
                rng = np.random.default_rng(1000 * K + N)
                lyr = layer(rng, N, K, True, ar)
                nxt = layer(rng, 8, N, True, ar)                 # only its input scale matters: the planes epilogue writes its operand
                stack = prepared([lyr, nxt], ar)
                sig_next = nxt.h2["sig"] if ar == "f16x2" else None
                for M in (1, 17, 129):
                    for epi, group in ((1, 1), (0, 1), (2, 32)):
                        rows = M * group
                        pl, src, idx = inputs(rng, rows, K, group, stack, ar)
                        tag = f"gemm {ar} K={K} N={N} M={M} epilogue={epi}"
                        out[tag] = digest(lyr.planes(pl, rows, epi, group if epi == 2 else 0, ar=ar, sig_next=sig_next))
                        out[tag + " gather"] = digest(lyr.planes(src, rows, epi, group if epi == 2 else 0, idx=idx, ar=ar, sig_next=sig_next))

    # ---- four layers in one kernel
    for ar in ("bf16x3", "f16x2"):
        for K0, widths in CHAIN_CASES:
            rng = np.random.default_rng(900 + K0)
            layers, k = [], K0
            for nw in widths:
                layers.append(layer(rng, nw, k, True, ar))
                k = nw
            stack = prepared(layers, ar)
            assert families.chain4_fits(stack)
            for M in (17, 129):
                for want, group in (("rows", 1), ("max", 32)):
                    rows = M * group
                    pl, src, idx = inputs(rng, rows, K0, group, stack, ar)
                    tag = f"chain4 {ar} K0={K0} widths={widths} M={M} {want}"
                    out[tag] = digest(families.run_planes(stack, pl, rows, want, group, ar=ar))
                    out[tag + " gather"] = digest(families.run_planes(stack, src, rows, want, group, idx=idx, ar=ar))
    torch.cuda.synchronize()
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    print()


if __name__ == "__main__":
    main()
