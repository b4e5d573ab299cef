#!/usr/bin/env python3
"""compress.py with the reference's command line (compress.py:20-40), on the MI355X path.
Writes <name>.p.bin / .s.bin / .c.bin per input file (compress.py:139-152)."""
import argparse
import os
import time
from glob import glob

import numpy as np

import _common  # noqa: F401
import torch
from pccx import codec, dist, plyio

parser = argparse.ArgumentParser(prog='compress.py', description='Compress Point Clouds Using Trained Model.',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument('input_glob', help='Point clouds glob pattern for compression.')
parser.add_argument('compressed_path', help='Comressed .bin files folder.')
parser.add_argument('model_load_folder', help='Directory where to load trained models.')
_common.add_codec_flags(parser)
# how the centres are chosen concerns the encoder alone: decompress.py reads the files of either choice without a flag
parser.add_argument('--centres', choices=['fps', 'blocks'], default='fps',
                    help="Patch centres: 'fps' = the reference's farthest point sampling over the whole cloud; 'blocks' = an independent "
                         "sampling in every run of --fps-block points of the cloud's Morton order, all runs side by side (whole rooms: "
                         "a fraction of the time, other centres, hence other bytes and quality).  The files are read by decompress.py as they are.")
parser.add_argument('--fps-block', type=int, default=8192, metavar='N',
                    help="Points per block of --centres blocks, 1024..16384; a cloud of at most N points gets the exact sampling.")


def main():
    args = parser.parse_args()
    if args.ragged and (args.octree_mode != 'full' or args.p_split or args.p_index or args.centres != 'fps' or args.knn_search == 'grid'):
        raise SystemExit("--ragged needs --octree-mode full and excludes --p-split, --p-index, --centres blocks and --knn-search grid")
    print(f"Processing on device (gpu/cpu): {args.device}")
    os.makedirs(args.compressed_path, exist_ok=True)
    files = sorted(glob(args.input_glob, recursive=True))
    rank, world = _common.setup_ranks(args)
    mine = sorted(dist.shard_indices(len(files), rank, world))                                   # file i -> rank i mod world
    # --ply-io threads: the headers of this rank's files first, on the host threads -- a file that cannot be read ends the run here,
    # before any GPU work, and the point counts route the files below before a single vertex is read
    rows = dict(zip(mine, _common.scan_plys([files[i] for i in mine]))) if args.ply_io == 'threads' else None
    ae, prob = _common.load_models(args)
    cd = codec.Codec(ae, prob, K=args.K, ALPHA=args.ALPHA, N0=args.N0, octree_mode=args.octree_mode, knn_search=args.knn_search,
                     max_centres=codec.OCTREE_WIDE_MAX_S,             # whole clouds up to 8192 patches: 1048576 points at K = 256
                     p_split=args.p_split or None, p_index=args.p_index or None, centres=args.centres, fps_block=args.fps_block,
                     prob_path=args.prob)
    times, todo, bits, points, index_bits = [], [(i, files[i]) for i in mine], 0, 0, 0
    with torch.no_grad():
        while todo:
            # (file index, path, point count, the cloud -- or with --ply-io threads its row of the header table); outside the timed window
            if rows is not None:
                clouds = [(i, f, int(rows[i][plyio.N_VERTEX]), rows[i]) for i, f in todo[:args.batch]]
            else:
                clouds = [(i, f, a.shape[0], a) for i, f, a in ((i, f, plyio.read_point_cloud(f)) for i, f in todo[:args.batch])]
            n0 = clouds[0][2]
            # --ragged: every file of the chunk that is inside the ragged path's limits, whatever its point count, in one launch sequence
            fits = [c for c in clouds if cd.ragged_refusal([c[2]]) is None] if args.ragged else []
            batch = fits or [c for c in clouds if c[2] == n0]                                    # otherwise one launch = one N
            if args.ragged and not fits:                                                         # all of one N: one reason
                print(f"{', '.join(os.path.split(c[1])[1] for c in batch)}: outside --ragged, compressed the usual way: {cd.ragged_refusal([n0])}")
            done = {c[0] for c in batch}
            todo = [t for t in todo if t[0] not in done]
            sizes = [c[2] for c in batch]
            starts = [dist.fps_start_index(args.seed, c[0], n) for c, n in zip(batch, sizes)]
            if rows is not None:
                # the batch's vertex blocks by the host threads into one pinned buffer, one copy, one unpack kernel: the padded slab
                # (for files of one size, N_cap = n, that is the stack below)
                pc = plyio.read_point_clouds([c[1] for c in batch], args.device, "padded", table=np.stack([c[3] for c in batch]))[0]
            elif fits:
                pc = codec.pad_clouds([c[3] for c in batch])[0].to(args.device)
            else:
                pc = torch.from_numpy(np.stack([c[3] for c in batch])).to(args.device)
            torch.cuda.synchronize()
            t0 = time.time()                                                                     # compress.py:85
            comp = cd.compress_ragged(pc, sizes, starts) if fits else cd.compress(pc, starts)
            # ONE D2H of the batch's packed streams, then the library's host threads cut the three files of every cloud out of it
            # (pccx_write_streams_host): <name>.p.bin / .s.bin / .c.bin, the bytes of compress.py:139-152; with --p-index also <name>.p.idx
            nbytes = comp.write_files(args.compressed_path, [os.path.split(c[1])[1] for c in batch])
            times += [(time.time() - t0) / len(batch)] * len(batch)                              # compress.py:154
            bits += 8 * nbytes
            index_bits += int(comp.index_bits().sum())                                           # derived from the shape: no transfer
            points += sum(sizes)
    # the six-slot vector of dist.SUMMARY_FIELDS; this tool has no PSNR to report, so slot 2 ("psnr_sum") carries the sidecars' bits.
    # Summed over ranks here, never passed to dist.reduce_summaries.
    g = dist.gather_summaries([bits, points, index_bits, 0.0, len(times), float(np.sum(times))], _common.summary_device(args))
    if rank == 0 and float(g[:, 4].sum()) > 0:
        tot = g.sum(dim=0)
        print(f"Done! Execution time: {round(float(tot[5] / tot[4]), 5)}s per point cloud." +
              (f" ({int(tot[4])} clouds on {world} ranks, {float(tot[0] / tot[1]):.4f} bpp)" if world > 1 else "") +
              (f" Files {float(tot[0] / tot[1]):.4f} bpp, index {float(tot[2] / tot[1]):.4f} bpp beside them." if args.p_index else ""))
    _common.finish_ranks(world)


if __name__ == '__main__':
    main()
