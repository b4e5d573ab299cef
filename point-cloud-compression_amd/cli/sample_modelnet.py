#!/usr/bin/env python3
"""sample_modelnet.py with the reference's command line (sample_modelnet.py:72-80), on the MI355X path: a folder tree of OFF triangle
meshes (ModelNet40) -> the same tree of .ply point clouds of --n_point points each, area-weighted samples of the surface normalised into
the unit cube (sample_modelnet.py:44-48).

Files go in chunks of --batch through pccx.meshes.read_meshes (host threads, one copy to the device), sample_meshes (the sampler of
DESIGN.md section 4.5, "meshes") and plyio.save_point_clouds (host threads): no per-file Python loop.

Where this differs from the reference, on purpose:
  * the sampler is defined here, not by pyntcloud's mesh_random, whose draws are unpinned: same distribution, other points.  A file's
    cloud is a function of (--seed, its path relative to `source`, its mesh) alone, not of the glob's order, --batch or the other files;
  * drop_duplicates is not reproduced: two samples coincide only on the same or a coincident triangle with the same 64 random bits, so
    every output file has exactly --n_point rows;
  * every file is read once on the host before any GPU work.  A file that is refused (not OFF, truncated, a polygon, an index out of
    range, a coordinate that is no finite number, ...) ends the run there with every such file named and nothing written; with
    --skip-bad such files, and meshes without area, are left out and listed at the end, which is closest to the reference's "is gone
    wrong" and carry on;
  * --quantize with a true value is refused: in the reference it rounds unit-cube coordinates, which leaves at most 8 distinct points;
  * only --source_extension .off is read."""
import argparse
import os
from glob import glob
from os.path import join, split, splitext

import _common  # noqa: F401
import torch
from pccx import meshes, plyio

parser = argparse.ArgumentParser(prog='sample_modelnet.py', description='Converts a folder containing meshes to point clouds',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument('source', help='Source directory', default='./data/ModelNet40')
parser.add_argument('dest', help='Destination directory', default='./data/ModelNet40_pc_8192')
parser.add_argument('--vg_size', type=int, help='Voxel Grid resolution for x, y, z dimensions (accepted and unused, as in the reference)', default=1)
parser.add_argument('--n_point', type=int, help='Number of samples', default=8192)
parser.add_argument('--quantize', type=bool, help='Whether to round the numbers (refused: see the docstring)', default=False)
parser.add_argument('--source_extension', help='Mesh files extension', default='.off')
parser.add_argument('--target_extension', help='Point cloud extension', default='.ply')
parser.add_argument('--seed', type=int, default=11, help="Seed of the run; a file's stream is meshes.stream_seed(seed, its relative path).")
parser.add_argument('--batch', type=int, default=256, help='Meshes per launch sequence (1..1024).')
parser.add_argument('--threads', type=int, default=0, help='Host threads that read meshes and write clouds; 0 = min(8, hardware threads).')
parser.add_argument('--skip-bad', action='store_true', help='Leave out files that are refused and meshes without area, and list them at the end.')
parser.add_argument('--device', help='Device (cuda)', default='cuda')


def main():
    args = parser.parse_args()
    assert os.path.exists(args.source), f'{args.source} does not exist'
    assert not os.path.exists(args.dest), f'{args.dest} already exists'
    assert args.vg_size > 0, 'vg_size must be positive'
    assert args.n_point > 0, 'n_point must be positive'
    if args.quantize:
        raise SystemExit("--quantize is refused: rounding unit-cube coordinates leaves at most 8 distinct points per cloud")
    if args.source_extension.lower() != '.off':
        raise SystemExit(f"--source_extension {args.source_extension}: only .off meshes are read")
    if not 1 <= args.batch <= 1024:
        raise SystemExit("--batch must be 1..1024")
    if not torch.cuda.is_available():
        raise SystemExit("pccx needs a ROCm GPU: there is no CPU path")
    source = args.source.rstrip(os.sep) or os.sep
    paths = sorted(glob(join(source, '**', f'*{args.source_extension}'), recursive=True))
    files = [os.path.relpath(p, source) for p in paths]
    assert len(files) > 0, f'no *{args.source_extension} file under {args.source}'
    print(f'Found {len(files)} models in {args.source}')

    # every file once on the host, before any GPU work and before anything is written
    refused = []
    for at in range(0, len(paths), args.batch):
        refused += [(files[at + b], why) for b, why in meshes.check_meshes(paths[at:at + args.batch], args.threads)]
    if refused and not args.skip_bad:
        raise SystemExit(f"{len(refused)} of {len(files)} files refused, nothing written (--skip-bad leaves them out):\n  " +
                         "\n  ".join(f"{join(args.source, f)}: {why}" for f, why in refused))
    bad = {f for f, _ in refused}
    good = [(p, f) for p, f in zip(paths, files) if f not in bad]

    written = 0
    for at in range(0, len(good), args.batch):
        chunk = good[at:at + args.batch]
        verts, faces, v_off, f_off = meshes.read_meshes([p for p, _ in chunk], args.device, args.threads)
        seeds = [meshes.stream_seed(args.seed, f.replace(os.sep, '/')) for _, f in chunk]
        points, status = meshes.sample_meshes(verts, faces, v_off, f_off, args.n_point, seeds, normalize="unit")
        status = status.tolist()
        flat = [(f, "the mesh has no area" if s == 1 else "every sampled value is the same") for (_, f), s in zip(chunk, status) if s != 0]
        if flat and not args.skip_bad:
            raise SystemExit(f"{len(flat)} meshes cannot be sampled (--skip-bad leaves them out):\n  " + "\n  ".join(f"{join(args.source, f)}: {why}" for f, why in flat))
        refused += flat
        # the files of one folder stand side by side in the sorted chunk: one slab of the result and one call of the writer per folder
        lo = 0
        while lo < len(chunk):
            folder = split(chunk[lo][1])[0]
            hi = lo
            while hi < len(chunk) and split(chunk[hi][1])[0] == folder:
                hi += 1
            keep = [b for b in range(lo, hi) if status[b] == 0]
            if keep:
                os.makedirs(join(args.dest, folder), exist_ok=True)
                plyio.save_point_clouds(points[lo:hi], [args.n_point] * len(keep), join(args.dest, folder),
                                        [splitext(split(chunk[b][1])[1])[0] for b in keep], suffix=args.target_extension, threads=args.threads,
                                        first_rows=[(b - lo) * args.n_point for b in keep])
                written += len(keep)
            lo = hi
    meshes.release_pinned()
    plyio.release_pinned()
    if refused:
        print(f"{len(refused)} files left out:\n  " + "\n  ".join(f"{join(args.source, f)}: {why}" for f, why in refused))
    print(f'{written} models written to {args.dest}')


if __name__ == '__main__':
    main()
