#!/usr/bin/env python3
"""decompress.py with the reference's command line (decompress.py:19-39), on the MI355X path."""
import argparse
import os
import time
from glob import glob

import numpy as np

import _common  # noqa: F401
import torch
from pccx import codec, dist, models, ops, plyio
from pccx._lib import PccxError

parser = argparse.ArgumentParser(prog='decompress.py', description='Deompress Point Clouds Using Trained Model.',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument('compressed_path', help='Comressed .bin files folder.')
parser.add_argument('decompressed_path', help='Decompressed .ply files folder.')
parser.add_argument('model_load_folder', help='Directory where to load trained models.')
_common.add_codec_flags(parser)
parser.add_argument('--S', type=int, default=None,
                    help="Patches per cloud with --octree-mode full (default: the number of centres each .s.bin holds; "
                         "'reference' mode is octree_np.decode as written, always 64).")
parser.add_argument('--bin-ply-suffix', action='store_true',
                    help="Write <name>.bin.ply (what eval.py:172 looks for) instead of <name> (decompress.py:121).")
parser.add_argument('--region', type=float, nargs=6, default=None, metavar=('X0', 'Y0', 'Z0', 'X1', 'Y1', 'Z1'),
                    help="Decode only the patches whose centre lies in this box of the cloud's original coordinates "
                         "(Codec.decompress_region); needs --p-split or --p-index, and --octree-mode full.")
parser.add_argument('--region-halo', type=float, default=0.0, help="Grow the --region box by this much on every side when selecting patches.")
parser.add_argument('--build-index', action='store_true',
                    help="With --p-index: where <name>.p.idx is missing, build it from the .p.bin first (one sequential decode) and write it.")
parser.add_argument('--crop', action='store_true', help="With --region: drop the decoded points outside the box (the halo does not count).")


def main():
    args = parser.parse_args()
    if args.region is not None:
        if not args.p_split and not args.p_index:
            raise SystemExit("--region needs --p-split G or --p-index G (a stream is entered at a segment through the split .p.bin's "
                             "directory or the single stream's entry-point index)")
        if args.octree_mode != 'full':
            raise SystemExit("--region needs --octree-mode full")
    elif args.crop or args.region_halo:
        raise SystemExit("--crop / --region-halo need --region")
    if args.p_split and args.p_index:
        raise SystemExit("--p-index and --p-split exclude each other")
    if args.ragged and (args.octree_mode != 'full' or args.region is not None or args.p_split or args.p_index or args.S is not None
                        or args.knn_search == 'grid'):
        raise SystemExit("--ragged needs --octree-mode full and excludes --region, --p-split, --p-index, --knn-search grid and --S")
    if args.build_index and not args.p_index:
        raise SystemExit("--build-index needs --p-index G")
    print(f"Processing on device (gpu/cpu): {args.device}")
    os.makedirs(args.decompressed_path, exist_ok=True)
    names = sorted(os.path.split(x)[1][:-6] for x in glob(os.path.join(args.compressed_path, '*.s.bin')))
    rank, world = _common.setup_ranks(args)
    names = [names[i] for i in dist.shard_indices(len(names), rank, world)]                      # file i -> rank i mod world
    ae, prob = _common.load_models(args)
    cd = codec.Codec(ae, prob, K=args.K, ALPHA=args.ALPHA, N0=args.N0, octree_mode=args.octree_mode, max_centres=codec.OCTREE_WIDE_MAX_S,
                     p_split=args.p_split or None, p_index=args.p_index or None,
                     prob_path=args.prob)         # decompress, --build-index, and --region's fallback through decompress()
    times, index_bits, points = [], 0, 0
    # --ply-io threads: the decoded clouds stay on the device until the chunk's one copy (plyio.save_point_clouds)
    to_host = (lambda t: t.contiguous()) if args.ply_io == 'threads' else (lambda t: t.cpu().numpy())
    with torch.no_grad():
        for b0 in range(0, len(names), args.batch):
            chunk = names[b0:b0 + args.batch]
            torch.cuda.synchronize()
            t0 = time.time()                                                                     # decompress.py:77
            # the three files of every cloud of the chunk into ONE packed host buffer by the library's host threads
            # (pccx_read_streams_host; decompress.py:80-91,113 reads them one by one), then one upload
            if args.p_split:
                # split .p.bin: the header rules on every file's bytes (pccx_split_stream_check_host) before the upload; the symbol count
                # is taken from the file here and compared with the centres its .s.bin holds once those are decoded
                up = codec.Compressed.read_files(args.compressed_path, chunk)
                split_nsym = []
                for n, row, nb in zip(chunk, up.p_bytes.numpy(), up.p_nbytes.numpy()):
                    split_nsym.append(int.from_bytes(bytes(row[4:8]), 'little') if nb >= 8 else 0)
                    why = models.split_stream_status(row[:nb], split_nsym[-1], args.p_split * args.d)
                    if why:
                        raise SystemExit(f"{n}.p.bin is not a split stream of --p-split {args.p_split}: {models.SPLIT_STATUS[why]}")
                up = codec.Compressed.from_packed(up.packed.to(args.device, non_blocking=True), len(chunk), up.s_bytes.shape[1], up.p_bytes.shape[1], 0)
            else:
                up = codec.Compressed.read_files(args.compressed_path, chunk, device=args.device)
            s_b, s_n, p_b, p_n, c = up.s_bytes, up.s_nbytes, up.p_bytes, up.p_nbytes, up.c
            # number of centres each stream holds (decompress.py:85 takes S from the decoded array)
            _, count = ops.octree_decode(s_b, s_n, args.octree_mode, 64 if args.octree_mode == 'reference' else 1, wide=args.octree_mode == 'full')   # up to 8192 centres
            count = count.cpu().numpy()
            if (count < 0).any():
                raise PccxError("corrupt .s.bin stream(s): " + ", ".join(n for n, k_ in zip(chunk, count) if k_ < 0))
            if args.octree_mode == 'full' and (count == 0).any():
                # an empty / truncated / root-bit-0 stream decodes to NO centres: there are no patches to decode the .p.bin against
                # (S = 0 would mean zero-size launches and an empty .ply); more centres than the decoder holds come back as -1 above
                bad = [n for n, k_ in zip(chunk, count) if k_ == 0]
                raise PccxError("corrupt or empty .s.bin stream(s) (0 centres decoded; their .p.bin cannot be decoded): " + ", ".join(bad))
            S_of = np.full(len(chunk), 64) if args.octree_mode == 'reference' else (count if args.S is None else np.full(len(chunk), args.S))
            if args.octree_mode == 'full' and args.S is not None and (count != args.S).any():
                raise PccxError(f"--S {args.S} given but the streams hold {sorted(set(count.tolist()))} centres")
            if args.p_split:
                for n, nsym, S in zip(chunk, split_nsym, S_of.tolist()):
                    if nsym != int(S) * args.d:
                        raise SystemExit(f"{n}.p.bin holds {nsym} symbols but {n}.s.bin gives S={int(S)} patches of d={args.d}: "
                                         + models.SPLIT_STATUS[2])
            side = None
            if args.p_index:
                # the sidecars as the three streams: per distinct S (their size follows from it) ONE threaded read of every file
                # (pccx_read_index_host), the check on the host bytes against each .p.bin's length, ONE upload.  A missing one is built
                # first with --build-index (the sequential decoder once) and written beside the three files.
                side, seg = {}, args.p_index * args.d
                p_n_host = p_n.cpu().numpy()
                for S in sorted(set(S_of.tolist())):
                    js = np.flatnonzero(S_of == S).tolist()
                    for j in js:
                        n = chunk[j]
                        if os.path.exists(os.path.join(args.compressed_path, n + '.p.idx')):
                            continue
                        if not args.build_index:
                            raise SystemExit(f"{n}.p.idx is missing: pass --build-index to make it from {n}.p.bin, or compress with --p-index {args.p_index}")
                        one = codec.Compressed(s_b[j:j + 1], s_n[j:j + 1], p_b[j:j + 1], p_n[j:j + 1], c[j:j + 1], 0)
                        cd.build_index(one, int(S))
                        codec.write_index(one.p_index.cpu().contiguous(), args.compressed_path, [n])
                        print(f"{n}: built {n}.p.idx ({one.p_index.shape[1]} bytes)")
                    idx, cnt = codec.read_index(args.compressed_path, [chunk[j] for j in js], models.index_bytes(int(S) * args.d, seg))
                    for r, j in enumerate(js):
                        why = models.index_status(bytes(idx[r, :int(cnt[r])].numpy()), int(p_n_host[j]), int(S) * args.d, seg)
                        if why:
                            raise SystemExit(f"{chunk[j]}.p.idx is not the index of {chunk[j]}.p.bin at --p-index {args.p_index}: {models.INDEX_STATUS[why]}")
                    side[int(S)] = (idx.to(args.device, non_blocking=True), {j: r for r, j in enumerate(js)})   # whole rows: the check passed
                    index_bits += 8 * int(cnt.sum())
                    points += int(S) * args.K // args.ALPHA * len(js)
            clouds = [None] * len(chunk)
            if args.region is not None:
                box = (args.region[:3], args.region[3:])
                for j, n in enumerate(chunk):                                                    # one decompress_region call per file
                    comp = codec.Compressed(s_b[j:j + 1], s_n[j:j + 1], p_b[j:j + 1], p_n[j:j + 1], c[j:j + 1], 0)
                    if side is not None:
                        rows, at = side[int(S_of[j])]
                        comp.p_index = rows[at[j]:at[j] + 1]
                    reg = cd.decompress_region(comp, int(S_of[j]), box, halo=args.region_halo)
                    pts = reg.points
                    if args.crop:
                        lo, hi = (torch.tensor(v, device=pts.device, dtype=torch.float32) for v in box)
                        pts = pts[((pts >= lo) & (pts <= hi)).all(dim=1)]
                    if pts.shape[0] == 0:
                        print(f"{n}: no point in the region ({reg.segments.numel()} of {reg.n_segments_total} segments touched), skipped")
                        continue
                    print(f"{n}: {reg.patch_idx.numel()} patches from {reg.segments.numel()} of {reg.n_segments_total} segments")
                    clouds[j] = to_host(pts)
            else:
                usual = np.ones(len(chunk), dtype=bool)
                if args.ragged:
                    # file by file, by the rule compress.py --ragged routes by (Codec.ragged_patch_range): every file inside it in one
                    # launch sequence whatever its S, the others the way they were written
                    why = [cd.ragged_decode_refusal([int(S)]) for S in S_of.tolist()]
                    usual = np.array([w is not None for w in why])
                    for n, w in zip(chunk, why):
                        if w is not None:
                            print(f"{n}: outside --ragged, decompressed the usual way: {w}")
                    if not usual.all():
                        sel = torch.from_numpy(np.flatnonzero(~usual)).to(args.device)
                        pcs = cd.decompress_ragged(codec.Compressed(s_b[sel], s_n[sel], p_b[sel], p_n[sel], c[sel], 0), S_of[~usual].tolist())
                        for j, pts in zip(sel.cpu().tolist(), pcs):
                            clouds[j] = to_host(pts)
                for S in sorted(set(S_of[usual].tolist())):                                      # one launch sequence per S
                    sel = torch.from_numpy(np.flatnonzero((S_of == S) & usual)).to(args.device)
                    comp = codec.Compressed(s_b[sel], s_n[sel], p_b[sel], p_n[sel], c[sel], 0)
                    if side is not None:
                        comp.p_index = side[int(S)][0]                                           # rows in the order of `sel`: ascending j
                    pc = to_host(cd.decompress(comp, S=int(S)))
                    for j, cloud in zip(sel.cpu().tolist(), pc):
                        clouds[j] = cloud
            if args.ply_io == 'threads':
                # the window ends with the points decoded on the device: their read-back (decompress.py:116, inside the window without
                # the flag) is the one copy of save_point_clouds below, outside it
                torch.cuda.synchronize()
            times += [(time.time() - t0) / len(chunk)] * len(chunk)                              # decompress.py:118
            suffix = '.bin.ply' if args.bin_ply_suffix else ''
            kept = [(n, cloud) for n, cloud in zip(chunk, clouds) if cloud is not None]         # --region: None = nothing of this file in the box
            if args.ply_io == 'threads' and kept:
                # the clouds are rows of the decoders' slabs: each slab's span travels once, as it lies, into pinned memory (no gathering
                # copy on the device), and the host threads write the files
                plyio.save_point_clouds([cloud for _, cloud in kept], None, args.decompressed_path, [n for n, _ in kept], suffix)
            else:
                for n, cloud in kept:
                    plyio.save_point_cloud(cloud, os.path.join(args.decompressed_path, n + suffix))
    # the six-slot vector of dist.SUMMARY_FIELDS; this tool has no PSNR to report, so slot 2 ("psnr_sum") carries the sidecars' bits and
    # slot 1 the points they index.  Summed over ranks here, never passed to dist.reduce_summaries.
    g = dist.gather_summaries([0.0, points, index_bits, 0.0, len(times), float(np.sum(times))], _common.summary_device(args))
    if rank == 0 and float(g[:, 4].sum()) > 0:
        tot = g.sum(dim=0)
        print(f"Done! Execution time: {round(float(tot[5] / tot[4]), 5)}s per point cloud." + (f" ({int(tot[4])} clouds on {world} ranks)" if world > 1 else "")
              + (f" Index {float(tot[2] / tot[1]):.4f} bpp beside the files." if args.p_index and float(tot[1]) > 0 else ""))
    _common.finish_ranks(world)


if __name__ == '__main__':
    main()
