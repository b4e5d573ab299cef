#!/usr/bin/env python3
"""eval.py with the reference's command line (eval.py:20-35): D1 (point-to-point) PSNR, bpp from the
three file sizes, D2 (point-to-plane) PSNR with 30-NN PCA normals, Chamfer distance on min-max-normalised
clouds, uniformity coefficient -> CSV with the reference's columns."""
import argparse
import os
from glob import glob

import numpy as np
import pandas as pd

import _common  # noqa: F401
import torch
from pccx import codec, dist, ops, plyio

parser = argparse.ArgumentParser(prog='eval.py', description='Evaluate point cloud patches',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument('--input_glob', default='./data/ModelNet40_pc_01_8192p/**/test/*.ply')
parser.add_argument('--compressed_path', default='./data/ModelNet40_K256_compressed/')
parser.add_argument('--decompressed_path', default='./data/ModelNet40_K256_decompressed/')
parser.add_argument('--output_file', default='./eval/ModelNet40_K256.csv')
parser.add_argument('--device', default='cuda')
parser.add_argument('--search', choices=['brute', 'grid'], default='brute',
                    help='nearest-neighbour search of the metrics: all-pairs kernels (files of at most 32768 points), or the exact grid index '
                         '(same values, files of any size)')
parser.add_argument('--ragged', action='store_true',
                    help='score the files in chunks: every chunk in one launch sequence and one read-back (codec.evaluate_ragged), whatever the '
                         'point counts; a file outside its limits (an original below 30 or any cloud above 32768 points) is scored the usual way')
parser.add_argument('--ragged-batch', type=int, default=64, help='files per chunk of --ragged')
_common.add_ply_io_flag(parser)


KNN_POINTS_MAX = 32768          # reference points pccx_knn takes (csrc/knn.hip)


def region_of_point0(pc, K, search='brute', chunk=KNN_POINTS_MAX):
    """The K points nearest to point 0 of pc (1,N,3), as offsets from point 0: (1,K,3), nearest first (eval.py:130-136).  One query with K = 1024
    is a single scan of the cloud, beyond the grid walk's K <= 32, so it stays with knn_points.  That kernel takes at most `chunk`
    reference points; search='grid' lifts the limit by chunks: the K nearest of every chunk of the cloud, then the K nearest among those
    candidates, again by chunks while they are too many.  The same points in the same order as one scan would give: each pair keeps
    its fp32 distance, a chunk's candidates come out ascending by (distance, index) and the chunks follow in index order, so a tie
    between candidates still goes to the lower index of the cloud."""
    centre = pc[:, :1].contiguous()
    if search == 'grid':
        while pc.shape[1] > chunk:
            if chunk < 2 * K:
                raise ValueError(f"region_of_point0: chunks of {chunk} points cannot narrow a search for {K}")
            parts = pc.split(chunk, dim=1)
            pc = torch.cat([ops.knn_points(centre, p.contiguous(), min(K, p.shape[1]), return_dists=False, return_idx=False).knn[:, 0]
                            for p in parts], dim=1)
    return ops.knn_points(centre, pc, K, patch_scale=1.0).knn[:, 0]


def calc_uc(input_pc, decomp_pc, search='brute'):
    """eval.py:127-151: variance ratio of nearest-neighbour distances inside the 1024-NN region of point 0.  search='grid' finds the
    region in clouds of any size (region_of_point0) and takes the 2-NN inside it from the index; 'brute' is limited to
    KNN_POINTS_MAX points by knn_points."""
    def nn_var(pc):
        K = min(1024, pc.shape[1])
        region = region_of_point0(pc, K, search)                                    # (1,K,3), centred on point 0
        nn2 = ops.GridIndex(region).knn(region, 2) if search == 'grid' else ops.knn_points(region, region, 2)
        d2 = nn2.dists[..., 1]                                                      # nearest other point (:138-144)
        return torch.sqrt(d2).double().var(unbiased=False)
    return float(nn_var(decomp_pc) / nn_var(input_pc))


def main():
    args = parser.parse_args()
    if args.ragged and args.search == 'grid':
        parser.error("--ragged excludes --search grid: the ragged evaluation runs the all-pairs kernels")
    if args.ragged_batch < 1:
        parser.error("--ragged-batch needs at least one file per chunk")
    print(f"Processing on device (gpu/cpu): {args.device}")
    files = sorted(glob(args.input_glob, recursive=True))
    rank, world = _common.setup_ranks(args)
    pairs = []
    for f in [files[i] for i in dist.shard_indices(len(files), rank, world)]:                 # file i -> rank i mod world
        name = os.path.split(f)[1]
        cand = [os.path.join(args.decompressed_path, name + '.bin.ply'), os.path.join(args.decompressed_path, name)]
        decomp_f = next((c for c in cand if os.path.exists(c)), None)                # eval.py:172 vs decompress.py:121
        if decomp_f is not None:
            pairs.append((name, f, decomp_f))
    rows = []
    step = args.ragged_batch if args.ragged else 1
    # --ply-io threads: the headers of both sides of every pair first (a file that cannot be read ends the run here, before any GPU work)
    tables = [_common.scan_plys([p[side] for p in pairs]) for side in (1, 2)] if args.ply_io == 'threads' else None
    for c0 in range(0, len(pairs), step):
        chunk = pairs[c0:c0 + step]
        if tables is not None:
            # a chunk's originals in one call, its reconstructions in another: each cloud a slice of the packed rows on the device
            sides = []
            for side in (1, 2):
                pts, _, sizes = plyio.read_point_clouds([p[side] for p in chunk], args.device, "packed", table=tables[side - 1][c0:c0 + step])
                sides.append(pts.split(sizes))
            clouds = list(zip(*sides))
        else:
            clouds = [(torch.from_numpy(plyio.read_point_cloud(f)), torch.from_numpy(plyio.read_point_cloud(g))) for _, f, g in chunk]
        # --ragged: every pair eval_ragged_refusal lets through is scored in ONE evaluate_ragged call and read back once; the others,
        # and every pair without the flag, go file by file
        inside = [i for i, (a, b) in enumerate(clouds)
                  if args.ragged and codec.eval_ragged_refusal([a.shape[0]], [b.shape[0]]) is None]
        scores = {}
        if inside:
            pa, na = codec.pad_clouds([clouds[i][0] for i in inside], device=args.device)
            pb, nb = codec.pad_clouds([clouds[i][1] for i in inside], device=args.device)
            res = codec.evaluate_ragged(pa, na, pb, nb)
            table = torch.stack([res[k] for k in ('d1_psnr', 'd2_psnr', 'chamfer', 'uc')]).cpu().tolist()
            scores = {i: [col[j] for col in table] for j, i in enumerate(inside)}
        for i, ((name, _, _), (a, b)) in enumerate(zip(chunk, clouds)):
            if i in scores:
                d1, d2, cd, uc = scores[i]
            else:
                a, b = a[None].to(args.device), b[None].to(args.device)
                d1, d2 = float(codec.d1_psnr(a, b, search=args.search)[0]), float(codec.d2_psnr(a, b, search=args.search)[0])
                cd, uc = float(codec.normalized_chamfer(a, b, search=args.search)[0]), calc_uc(a, b, args.search)
            bits = sum(os.stat(os.path.join(args.compressed_path, name + e)).st_size * 8 for e in ('.s.bin', '.p.bin', '.c.bin'))
            rows.append(dict(filename=name, p2pointPSNR=round(d1, 3), p2planePSNR=round(d2, 3), chamfer_distance=cd,
                             n_points_input=a.shape[-2], n_points_output=b.shape[-2], bpp=bits / a.shape[-2],     # eval.py:189
                             **{'uniformity coefficient': round(uc, 3)}))
    if world > 1:                                            # per-file rows travel to rank 0 (a few hundred bytes per file)
        import torch.distributed as tdist
        gathered = [None] * world
        tdist.all_gather_object(gathered, rows)
        rows = sorted((r for part in gathered for r in part), key=lambda r: r["filename"])
        _common.finish_ranks(world)
        if rank != 0:
            return
    df = pd.DataFrame(rows, columns=['filename', 'p2pointPSNR', 'p2planePSNR', 'chamfer_distance', 'n_points_input',
                                     'n_points_output', 'bpp', 'uniformity coefficient'])
    if len(df):
        print(f"Done! The average p2pointPSNR: {round(df.p2pointPSNR.mean(), 3)} | p2plane PSNR: {round(df.p2planePSNR.mean(), 3)} | chamfer distance: "
              f"{round(df.chamfer_distance.mean(), 8)} | bpp: {round(df.bpp.mean(), 3)} | uc: {round(df['uniformity coefficient'].mean(), 3)}")
    os.makedirs(os.path.dirname(os.path.abspath(args.output_file)), exist_ok=True)
    df.to_csv(args.output_file)
    print(f"Evaluation results saved to {args.output_file}")


if __name__ == '__main__':
    main()
