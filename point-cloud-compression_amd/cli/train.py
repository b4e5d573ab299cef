#!/usr/bin/env python3
"""train.py with the reference's command line (train.py:22-50), on the MI355X path: ``--model AE`` (the IPDAE autoencoder) trains through
pccx.train_ipdae; checkpoints carry the reference's names (ae_step{N}.pkl, prob_step{N}.pkl, optimizer_step{N}.pkl, global_step{N}.pkl,
train.py:103-108) and the reference's state_dict keys, so compress.py / decompress.py load them unchanged.  Two flags are this
path's own: --octree-mode (the spelling of compress.py / decompress.py; 'full' trains on the centres those decode in that mode, the
mode is not stored in the .pkl files) and --val_glob (the real codec's bpp and D1 on held-out files at every step window).
--ragged (with --octree-mode full) trains on files of different point counts, several sizes in one step: the trainer's side of
``compress.py --ragged``.  --crop trains either step on compact crops cut on the GPU from files of any size (whole rooms)."""
import argparse
import os
from glob import glob

import numpy as np

import _common  # noqa: F401
import torch
from pccx import _lib, codec, models, ops, plyio, train_ipdae

torch.manual_seed(11)                                                                  # train.py:17-19
np.random.seed(11)

parser = argparse.ArgumentParser(prog='train_ae.py', description='Train autoencoder using point cloud patches',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument('--train_glob', default='./data/ModelNet40_pc_01_8192p/**/train/*.ply', help='Point clouds glob pattern for training.')
parser.add_argument('--model_save_folder', default='./model/K256/', help='Directory where to save trained models.')
parser.add_argument('--model', default='AE', help='Type of the model (AE or PPPF-AE).')
parser.add_argument('--N', type=int, default=8192, help='Point cloud resolution.')
parser.add_argument('--N0', type=int, default=1024, help='Scale Transformation constant.')
parser.add_argument('--ALPHA', type=int, default=2, help='The factor of patch coverage ratio.')
parser.add_argument('--K', type=int, default=256, help='Number of points in each patch.')
parser.add_argument('--d', type=int, default=16, help='Bottleneck size.')
parser.add_argument('--L', type=int, default=7, help='Quantization Level.')
parser.add_argument('--lr', type=float, default=0.0005, help='Learning rate.')
parser.add_argument('--batch_size', type=int, default=1, help='Batch size (must be 1).')
parser.add_argument('--step_window', type=float, default=100, help='Number of steps per window to iterate in epoch.')
parser.add_argument('--lamda', type=float, default=1e-06, help='Lambda for rate-distortion tradeoff.')
parser.add_argument('--rate_loss_enable_step', type=int, default=40000, help='Apply rate-distortion tradeoff at x steps.')
parser.add_argument('--lr_decay', type=float, default=0.1, help='Decays the learning rate to x times the original.')
parser.add_argument('--lr_decay_steps', type=int, default=60000, help='Decays the learning rate every x steps.')
parser.add_argument('--max_steps', type=int, default=80000, help='Train up to this number of steps.')
parser.add_argument('--device', default='cuda', help='AE Model Device (cuda)')
parser.add_argument('--reset', action='store_true', help='Reset training and start from scratch (ignore saved model).')
parser.add_argument('--autocast', action='store_true', help='bf16 operands on the matrix cores (the reference wraps its CUDA step in autocast, train.py:175).')
parser.add_argument('--eager', action='store_true', help='launch every kernel of every step from Python instead of replaying the captured step.')
parser.add_argument('--octree-mode', choices=['reference', 'full'], default='reference',
                    help="the patch centres a step trains on: 'reference' = octree_np.decode as written (S must be 64); 'full' = the level-by-level "
                         "decode, the centres compress.py / decompress.py --octree-mode full use (any S = N*ALPHA/K in 1..1024, at every --K of the table).")
parser.add_argument('--val_glob', default=None, help='Point clouds glob pattern (files of --N points) run through the real codec at every --step_window.')
parser.add_argument('--deterministic', action='store_true', help='every reduction of a step in a fixed order: the same inputs give the same bits, run after run (one GPU).')
parser.add_argument('--ragged', action='store_true',
                    help="files of different point counts, mixed in one step (needs --octree-mode full; --N is ignored): every file must hold "
                         "K..32768 points and S = n*ALPHA//K patches inside the range compress.py --ragged takes; --val_glob files likewise.")
parser.add_argument('--crop', action='store_true',
                    help="files of any size >= --N (with --ragged: >= --K): every step trains on --batch_size compact crops cut on the GPU, each the "
                         "points nearest to a seed point drawn uniformly over all points of all files (--N points; with --ragged a size drawn "
                         "in --crop-min..--crop-max).  --val_glob files are cropped once, around their first point.")
parser.add_argument('--crop-min', type=int, default=None, help='--crop --ragged: the smallest crop, in points.')
parser.add_argument('--crop-max', type=int, default=None, help='--crop --ragged: the largest crop, in points (the step is built for it).')
_common.add_ply_io_flag(parser)
parser.add_argument('--crop-seed', type=int, default=11, help='--crop: seed of the generator the seed points, crop sizes and FPS starts are drawn from.')


VAL_CHUNK = 16                         # clouds per codec batch of a --val_glob pass: the validation set's size does not bound the codec's buffers


def latest(folder, prefix):
    """train.py:67-77: the file <prefix>_step{largest N}.pkl, or '' when there is none"""
    steps = []
    for f in os.listdir(folder):
        if f.startswith(prefix + "_step") and f.endswith(".pkl"):
            try:
                steps.append(int(f[len(prefix) + 5:-4]))
            except ValueError:
                pass                                                                   # the final dump's "<prefix>_step.pkl"
    return os.path.join(folder, f"{prefix}_step{max(steps)}.pkl") if steps else ''


def load_checkpoints(tr, folder):                                                      # train.py:80-100
    start = 0
    for prefix, target in (("ae", tr.ae), ("prob", tr.prob), ("optimizer", tr.opt)):
        p = latest(folder, prefix)
        if p:
            print(f"Loading {prefix} from:", p)
            sd = torch.load(p, map_location="cpu", weights_only=True)                  # tensors, numbers and containers only
            target.load_state_dict(sd)
    p = latest(folder, "global")
    if p:
        start = int(torch.load(p, map_location="cpu", weights_only=True)) + 1          # :97-99
        print("Starting step:", start)
    return start


def dump_checkpoints(tr, folder, global_step=''):                                      # train.py:103-108
    torch.save(tr.ae.state_dict(), os.path.join(folder, f'ae_step{global_step}.pkl'))
    torch.save(tr.prob.state_dict(), os.path.join(folder, f'prob_step{global_step}.pkl'))
    torch.save(tr.opt.state_dict(), os.path.join(folder, f'optimizer_step{global_step}.pkl'))
    torch.save(global_step, os.path.join(folder, f'global_step{global_step}.pkl'))


def window_report(tr, args, epoch, losses, fbpps, bpps, validate, n_val):
    """the window's line, its checkpoints and, with validation files, the real codec on the current weights (validate(i): the clouds
    [i, i + VAL_CHUNK), repacked by the trainer): means weighted by v['n']"""
    print(f"[Epoch {epoch}] Step {tr.global_step} | Feature bpp: {np.mean(fbpps):.5f} | Bpp: {np.mean(bpps):.5f} | "
          f"Loss: {np.mean(losses):.5f}")
    dump_checkpoints(tr, args.model_save_folder, tr.global_step)
    if validate is not None:
        vs = [validate(i) for i in range(0, n_val, VAL_CHUNK)]
        n = sum(v['n'] for v in vs)
        print(f"[Epoch {epoch}] Step {tr.global_step} | Val bpp: {sum(v['bpp'] * v['n'] for v in vs) / n:.5f} | "
              f"Val D1: {sum(v['d1_psnr'] * v['n'] for v in vs) / n:.3f} dB ({n} clouds)")


def read_clouds(files, ply_io):
    """the clouds of `files`: arrays read one by one, or with --ply-io threads their headers only (_common.ScannedClouds: the shapes now,
    the points in one call once nothing is left to refuse)"""
    if ply_io == 'threads':
        return _common.ScannedClouds(files)
    return [plyio.read_point_cloud(f).astype(np.float32) for f in files]


def pad_all(clouds, device):
    return clouds.padded(device) if isinstance(clouds, _common.ScannedClouds) else codec.pad_clouds(clouds, device=device)


def pack_all(clouds, device):
    return clouds.packed(device) if isinstance(clouds, _common.ScannedClouds) else codec.pack_clouds(clouds, device=device)


def read_ragged(pattern, flag, K, ALPHA, ply_io='python'):
    """the files of a glob, read once, each checked against the shape rule of a ragged batch (codec.ragged_shape_refusal)
    -> (files, clouds, refusals: one line per file outside the rule)"""
    files = sorted(glob(pattern, recursive=True))
    clouds = read_clouds(files, ply_io)
    why = [(f, codec.ragged_shape_refusal([c.shape[0]], K, ALPHA)) for f, c in zip(files, clouds)]
    refused = [f"{flag} {f}: {w}" for f, w in why if w] if files else [f"{flag} {pattern}: no file matches"]
    return files, clouds, refused


def main_ragged(args):
    """--ragged: the loop of main() over files of different point counts.  The files live in HBM as one padded (F, N_cap, 3) tensor
    (codec.pad_clouds) with their counts; a step takes --batch_size of them, whatever their sizes, and by default replays ONE step
    captured at (N_cap, S_cap).  --eager, or a short last batch, goes through IpdaeTrainer.step_ragged."""
    K = args.K
    args.k = K // args.ALPHA
    print(f"Training {args.model} on {args.device}")
    print(f"autocast={args.autocast}, eager={args.eager}")
    print("octree_mode=full: these checkpoints are for compress.py/decompress.py --octree-mode full")
    try:
        train_ipdae.check_selection(args.ALPHA, K, args.octree_mode)                   # --K, before anything is read or allocated
    except _lib.PccxError as e:
        raise SystemExit(str(e))
    os.makedirs(args.model_save_folder, exist_ok=True)
    files, clouds, refused = read_ragged(args.train_glob, "--train_glob", K, args.ALPHA, args.ply_io)
    val_files, val_clouds = [], []
    if args.val_glob:
        val_files, val_clouds, more = read_ragged(args.val_glob, "--val_glob", K, args.ALPHA, args.ply_io)
        refused += more
    if refused:
        raise SystemExit("--ragged: nothing is dropped silently; these files are outside what a ragged batch takes:\n" + "\n".join(refused))
    data, counts = pad_all(clouds, args.device)                                        # the whole training set lives in HBM
    N_cap, S_cap = int(data.shape[1]), codec.ragged_plan(counts, K, args.ALPHA, args.N0, args.d).S_pad
    print(f"--ragged: --N is ignored; {len(files)} files of {min(counts)}..{max(counts)} points, N_cap={N_cap}, S_cap={S_cap}, K={K}, d={args.d}, L={args.L}")
    if val_files and args.ply_io == 'threads':
        vp, _, vs = val_clouds.packed(args.device)
        val = list(vp.split(vs))
    else:
        val = [torch.from_numpy(c).to(args.device) for c in val_clouds]
    if val:
        print(f"Loaded {len(val)} validation clouds of {min(len(c) for c in val)}..{max(len(c) for c in val)} points")
    ae = models.AE(K=K, k=args.k, d=args.d, L=args.L).to(args.device)
    prob = models.ConditionalProbabilityModel(args.L, args.d).to(args.device)
    tr = train_ipdae.IpdaeTrainer(ae, prob, N=N_cap, N0=args.N0, ALPHA=args.ALPHA, K=K, lr=args.lr, lamda=args.lamda,
                                  rate_loss_enable_step=args.rate_loss_enable_step, lr_decay=args.lr_decay,
                                  lr_decay_steps=args.lr_decay_steps, autocast=args.autocast, octree_mode=args.octree_mode)
    if not args.reset:
        tr.global_step = load_checkpoints(tr, args.model_save_folder)
        print(f"Resuming from step {tr.global_step}")
    else:
        print("Resetting training from scratch.")
    validate = (lambda i: tr.validate_ragged(val[i:i + VAL_CHUNK], [0] * len(val[i:i + VAL_CHUNK]))) if val else None
    losses, fbpps, bpps = [], [], []
    graph = None                       # train_ipdae.RaggedGraphedIpdaeStep, captured on the first full batch at the capacities
    for epoch in range(9999):
        order = torch.randperm(len(files))
        for b0 in range(0, len(files), args.batch_size):
            if tr.global_step > args.max_steps:
                break
            pick = order[b0:b0 + args.batch_size]
            batch, n = data[pick.to(args.device)], [counts[i] for i in pick.tolist()]
            lr_before = tr.lr
            starts = torch.cat([torch.randint(0, nb, (1,), dtype=torch.long) for nb in n])   # the draw of pn_kit.py:321, inside each cloud
            if args.eager or len(n) != args.batch_size:
                out = tr.step_ragged(batch, n, starts, S_cap=S_cap)
            elif graph is None:
                graph = tr.graphed_ragged(N_cap, S_cap, args.batch_size, batch, n, starts, warmup=1)   # the warm-up iteration IS this step
                out = {k_: float(v) for k_, v in zip(("loss", "fbpp", "bpp"), graph.warm_out)}
            else:
                out = graph(batch, n, starts)
            losses.append(out["loss"]), fbpps.append(out["fbpp"]), bpps.append(out["bpp"])
            if tr.global_step % args.step_window == 0:
                window_report(tr, args, epoch, losses, fbpps, bpps, validate, len(val))
                losses, fbpps, bpps = [], [], []
            if tr.lr != lr_before:
                print(f"LR decayed to {tr.lr} at step {tr.global_step}")
        if tr.global_step > args.max_steps:
            break
    dump_checkpoints(tr, args.model_save_folder)


def read_crop_store(pattern, flag, least, what, ply_io='python'):
    """the files of a glob for --crop, read once -> (files, clouds, refusals: one line per file below `least` points)"""
    files = sorted(glob(pattern, recursive=True))
    clouds = read_clouds(files, ply_io)
    refused = [f"{flag} {f}: {c.shape[0]} points, below {what} = {least}" for f, c in zip(files, clouds) if c.shape[0] < least]
    return files, clouds, refused if files else [f"{flag} {pattern}: no file matches"]


def main_crop(args):
    """--crop: the loops of main() and main_ragged() over crops instead of files.  The files, of any size, live in HBM one behind the
    other (codec.pack_clouds); a step takes --batch_size crops cut in front of it on the same stream (train_ipdae.CropSampler), --N
    points each, or with --ragged a size drawn in --crop-min..--crop-max, and is the dense / ragged step as it stands, captured or
    eager.  Everything that can be refused is refused before the GPU check."""
    K, ragged = args.K, args.ragged
    args.k = K // args.ALPHA
    if not args.crop:
        raise SystemExit("--crop-min / --crop-max size the crops of --crop --ragged: they need --crop")
    if not ragged and (args.crop_min is not None or args.crop_max is not None):
        raise SystemExit("--crop-min / --crop-max need --ragged (with --octree-mode full): without it every crop holds exactly --N points")
    if ragged:
        if args.crop_min is None or args.crop_max is None or not 1 <= args.crop_min <= args.crop_max:
            raise SystemExit(f"--crop --ragged needs --crop-min <= --crop-max, got {args.crop_min} and {args.crop_max}")
        why = codec.ragged_shape_refusal([args.crop_min, args.crop_max], K, args.ALPHA)
        if why:
            raise SystemExit(f"--crop-min {args.crop_min} --crop-max {args.crop_max}: the crops are outside what a ragged batch takes: {why}")
        n_lo, n_hi, least, what = args.crop_min, args.crop_max, K, "--K"
    else:
        n_lo = n_hi = least = args.N
        what = "--N"
        args.S = args.N * args.ALPHA // K
    n_mean = (n_lo + n_hi) // 2
    try:                                                                               # --K (and S), before anything is read or allocated
        if ragged:
            train_ipdae.check_selection(args.ALPHA, K, args.octree_mode)
        elif args.octree_mode == 'full':
            train_ipdae.check_selection(args.S, K, args.octree_mode)
    except _lib.PccxError as e:
        raise SystemExit(str(e))
    files, clouds, refused = read_crop_store(args.train_glob, "--train_glob", least, what, args.ply_io)
    val_files, val_clouds = [], []
    if args.val_glob:
        val_files, val_clouds, more = read_crop_store(args.val_glob, "--val_glob", least, what, args.ply_io)
        refused += more
    big = [f"{f}: {c.shape[0]} points, a crop is cut from at most {ops.CROP_MAX_M} per file" for f, c in zip(files + val_files, list(clouds) + list(val_clouds))
           if c.shape[0] > ops.CROP_MAX_M]
    if refused or big:
        raise SystemExit("--crop: nothing is dropped silently; these files cannot be cropped:\n" + "\n".join(refused + big))
    if not torch.cuda.is_available():
        raise SystemExit("pccx needs a ROCm GPU: there is no CPU path")
    print(f"Training {args.model} on {args.device}")
    if ragged:
        print(f"autocast={args.autocast}, eager={args.eager}")
    else:
        print(f"N={args.N}, K={K}, S={args.S}, d={args.d}, L={args.L}")
        print(f"deterministic={args.deterministic}, autocast={args.autocast}, eager={args.eager}")
    if args.octree_mode == 'full':
        print("octree_mode=full: these checkpoints are for compress.py/decompress.py --octree-mode full")
    os.makedirs(args.model_save_folder, exist_ok=True)
    gen = torch.Generator()
    gen.manual_seed(args.crop_seed)
    points, offsets, sizes = pack_all(clouds, args.device)                            # the whole training set lives in HBM
    sampler = train_ipdae.CropSampler(points, offsets, sizes, args.batch_size, n_hi, gen)
    N_cap, S_cap = n_hi, codec.ragged_plan([n_hi], K, args.ALPHA, args.N0, args.d).S_pad
    per_epoch = -(-sampler.M_total // (args.batch_size * n_mean))
    print(f"--crop: {len(files)} files of {min(sizes)}..{max(sizes)} points, {sampler.M_total} in all; crops of "
          f"{n_lo if n_lo == n_hi else f'{n_lo}..{n_hi}'} points, {per_epoch} steps per epoch" + (f", N_cap={N_cap}, S_cap={S_cap}" if ragged else ""))
    val = None
    if val_files:                                                                      # one fixed crop per file, cut once: the same clouds at every window
        vp, vo, vs = pack_all(val_clouds, args.device)
        cuts = [ops.crop_nearest(vp, vo, list(range(i, min(i + ops.CROP_MAX_B, len(vs)))), [0] * len(vs[i:i + ops.CROP_MAX_B]),
                                 [min(n_hi, m) for m in vs[i:i + ops.CROP_MAX_B]], n_hi, sizes=vs) for i in range(0, len(vs), ops.CROP_MAX_B)]
        val = torch.cat(cuts)
        if ragged:
            val = [v[:min(n_hi, m)].contiguous() for v, m in zip(val, vs)]
            print(f"Loaded {len(val)} validation crops of {min(len(c) for c in val)}..{max(len(c) for c in val)} points")
        else:
            print(f"Loaded {tuple(val.shape)} validation points")
    ae = models.AE(K=K, k=args.k, d=args.d, L=args.L).to(args.device)
    prob = models.ConditionalProbabilityModel(args.L, args.d).to(args.device)
    tr = train_ipdae.IpdaeTrainer(ae, prob, N=N_cap, N0=args.N0, ALPHA=args.ALPHA, K=K, lr=args.lr, lamda=args.lamda,
                                  rate_loss_enable_step=args.rate_loss_enable_step, lr_decay=args.lr_decay,
                                  lr_decay_steps=args.lr_decay_steps, autocast=args.autocast, deterministic=args.deterministic,
                                  octree_mode=args.octree_mode)
    if not args.reset:
        tr.global_step = load_checkpoints(tr, args.model_save_folder)
        print(f"Resuming from step {tr.global_step}")
    else:
        print("Resetting training from scratch.")
    if val is None:
        validate = None
    elif ragged:
        validate = lambda i: tr.validate_ragged(val[i:i + VAL_CHUNK], [0] * len(val[i:i + VAL_CHUNK]))
    else:
        validate = lambda i: tr.validate(val[i:i + VAL_CHUNK], torch.zeros(len(val[i:i + VAL_CHUNK]), dtype=torch.long))
    losses, fbpps, bpps = [], [], []
    graph = None                       # the step as one hipGraph, captured on the first batch; the crop runs in front of every replay
    for epoch in range(9999):
        for _ in range(per_epoch):
            if tr.global_step > args.max_steps:
                break
            want = torch.randint(n_lo, n_hi + 1, (args.batch_size,), generator=gen).tolist() if ragged else n_hi
            batch, n, starts = sampler.draw(want)                                      # on the current stream, into the sampler's buffer
            lr_before = tr.lr
            if ragged:
                if args.eager:
                    out = tr.step_ragged(batch, n, starts, S_cap=S_cap)
                elif graph is None:
                    graph = tr.graphed_ragged(N_cap, S_cap, args.batch_size, batch, n, starts, warmup=1)
                    out = {k_: float(v) for k_, v in zip(("loss", "fbpp", "bpp"), graph.warm_out)}
                else:
                    out = graph(batch, n, starts)
            elif args.eager:
                out = tr.step(batch, starts)
            elif graph is None:
                graph = tr.graphed(batch, starts, warmup=1)                            # the warm-up iteration IS this step
                out = {k_: float(v) for k_, v in zip(("loss", "fbpp", "bpp"), graph.warm_out)}
            else:
                out = graph(batch, starts)
            losses.append(out["loss"]), fbpps.append(out["fbpp"]), bpps.append(out["bpp"])
            if tr.global_step % args.step_window == 0:
                window_report(tr, args, epoch, losses, fbpps, bpps, validate, 0 if val is None else len(val))
                losses, fbpps, bpps = [], [], []
            if tr.lr != lr_before:
                print(f"LR decayed to {tr.lr} at step {tr.global_step}")
        if tr.global_step > args.max_steps:
            break
    dump_checkpoints(tr, args.model_save_folder)


def main():
    args = parser.parse_args()
    if args.model != 'AE':
        raise SystemExit(f"--model {args.model}: only AE (the IPDAE autoencoder, AE.py) trains on this path; PPPF-AE's train-mode BatchNorm "
                         f"stacks are not built (pccx/train_ipdae.py)")
    if args.ragged and (args.octree_mode != 'full' or args.deterministic):
        raise SystemExit("--ragged needs --octree-mode full (octree_mode 'reference' is S = 64 by definition) and excludes --deterministic "
                         "(the ordered Chamfer scatter is dense only)")
    if args.crop or args.crop_min is not None or args.crop_max is not None:
        return main_crop(args)
    if not torch.cuda.is_available():
        raise SystemExit("pccx needs a ROCm GPU: there is no CPU path")
    if args.ragged:
        return main_ragged(args)
    N, K = args.N, args.K
    args.S, args.k = N * args.ALPHA // K, K // args.ALPHA                              # train.py:253
    print(f"Training {args.model} on {args.device}")
    print(f"N={N}, K={K}, S={args.S}, d={args.d}, L={args.L}")
    print(f"deterministic={args.deterministic}, autocast={args.autocast}, eager={args.eager}")
    if args.octree_mode == 'full':
        # the mode is NOT stored in the reference-named .pkl files: both sides of the codec have to be told
        print("octree_mode=full: these checkpoints are for compress.py/decompress.py --octree-mode full")
        try:
            train_ipdae.check_selection(args.S, K, args.octree_mode)                   # any S in range, before anything is read or allocated
        except _lib.PccxError as e:
            raise SystemExit(str(e))
    os.makedirs(args.model_save_folder, exist_ok=True)
    files = sorted(glob(args.train_glob, recursive=True))
    if args.ply_io == 'threads':
        clouds = _common.ScannedClouds(files)
        if len({c.shape for c in clouds}) != 1:                                        # np.stack's refusal below, from the headers
            raise SystemExit(f"--train_glob: the files must all hold the same number of points, got {sorted({c.shape[0] for c in clouds})}")
        data = clouds.padded(args.device)[0]                                           # one size: the padded slab is the stack
        print(f"Loaded {tuple(data.shape)} points, range: [{np.float32(data.min().item())}, {np.float32(data.max().item())}]")
    else:
        points = np.stack([plyio.read_point_cloud(f) for f in files]).astype(np.float32)   # pn_kit.read_point_clouds (pn_kit.py:36-42)
        print(f"Loaded {points.shape} points, range: [{points.min()}, {points.max()}]")
        data = torch.from_numpy(points).to(args.device)                                # the whole training set lives in HBM
    val = None
    if args.val_glob:
        val_files = sorted(glob(args.val_glob, recursive=True))
        val_points = read_clouds(val_files, args.ply_io)                               # read once
        bad = [f for f, p in zip(val_files, val_points) if p.shape[0] != N]
        if bad or not val_files:
            raise SystemExit(f"--val_glob: {'no file matches' if not val_files else f'files without --N = {N} points: {bad}'}")
        val = val_points.padded(args.device)[0] if args.ply_io == 'threads' else torch.from_numpy(np.stack(val_points).astype(np.float32)).to(args.device)
        val_starts = torch.zeros(len(val_files), dtype=torch.long)                     # the same patches at every window
        print(f"Loaded {tuple(val.shape)} validation points")
    ae = models.AE(K=K, k=args.k, d=args.d, L=args.L).to(args.device)
    prob = models.ConditionalProbabilityModel(args.L, args.d).to(args.device)
    tr = train_ipdae.IpdaeTrainer(ae, prob, N=N, N0=args.N0, ALPHA=args.ALPHA, K=K, lr=args.lr, lamda=args.lamda,
                                  rate_loss_enable_step=args.rate_loss_enable_step, lr_decay=args.lr_decay,
                                  lr_decay_steps=args.lr_decay_steps, autocast=args.autocast, deterministic=args.deterministic,
                                  octree_mode=args.octree_mode)
    if not args.reset:
        tr.global_step = load_checkpoints(tr, args.model_save_folder)                  # :137-144
        print(f"Resuming from step {tr.global_step}")
    else:
        print("Resetting training from scratch.")
    losses, fbpps, bpps = [], [], []
    graph = None                       # the iteration as one hipGraph (pccx.train_ipdae.GraphedIpdaeStep), captured on the first full batch
    for epoch in range(9999):
        order = torch.randperm(len(files))                                             # DataLoader(shuffle=True), train.py:117
        for b0 in range(0, len(files), args.batch_size):
            if tr.global_step > args.max_steps:                                        # :163-164
                break
            batch = data[order[b0:b0 + args.batch_size].to(args.device)]
            lr_before = tr.lr
            starts = torch.randint(0, N, (batch.shape[0],), dtype=torch.long)         # the draw of pn_kit.py:321
            if args.eager or batch.shape[0] != args.batch_size:
                out = tr.step(batch, starts)                                           # (a short last batch has another shape: eager)
            elif graph is None:
                graph = tr.graphed(batch, starts, warmup=1)                            # the warm-up iteration IS this step
                out = {k_: float(v) for k_, v in zip(("loss", "fbpp", "bpp"), graph.warm_out)}
            else:
                out = graph(batch, starts)
            losses.append(out["loss"]), fbpps.append(out["fbpp"]), bpps.append(out["bpp"])
            if tr.global_step % args.step_window == 0:                                 # :241-247
                window_report(tr, args, epoch, losses, fbpps, bpps,
                              None if val is None else lambda i: tr.validate(val[i:i + VAL_CHUNK], val_starts[i:i + VAL_CHUNK]), 0 if val is None else len(val))
                losses, fbpps, bpps = [], [], []
            if tr.lr != lr_before:
                print(f"LR decayed to {tr.lr} at step {tr.global_step}")               # :254
        if tr.global_step > args.max_steps:
            break
    dump_checkpoints(tr, args.model_save_folder)                                       # :286 (the final, un-numbered dump)


if __name__ == '__main__':
    main()
