import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import torch  # noqa: E402


def find_checkpoint(folder, prefix):
    """The CLIs load <prefix>.pkl (compress.py:58-59) but the trainer writes <prefix>_step{N}.pkl
    (train.py:105): accept both, preferring the plain name, else the largest step."""
    p = os.path.join(folder, prefix + ".pkl")
    if os.path.exists(p):
        return p
    steps = []
    for f in os.listdir(folder) if os.path.isdir(folder) else []:
        if f.startswith(prefix + "_step") and f.endswith(".pkl"):
            try:
                steps.append((int(f[len(prefix) + 5:-4]), f))
            except ValueError:
                pass
    if not steps:
        raise FileNotFoundError(f"no {prefix}.pkl or {prefix}_step*.pkl under {folder}")
    return os.path.join(folder, max(steps)[1])


def setup_ranks(args):
    """One process per GPU: under torchrun / pccx.launch (RANK, LOCAL_RANK, WORLD_SIZE in the environment) pin this
    process to its GPU and join the process group (RCCL); files are then sharded file i -> rank i mod world
    (dist.shard_indices) and the per-rank summaries all-gathered at the end.  Returns (rank, world)."""
    from pccx import launch
    rank, local, world = launch.rank_env()
    if world > 1:
        if str(args.device).startswith("cuda"):
            local = local % max(torch.cuda.device_count(), 1)
            args.device = f"cuda:{local}"
            torch.cuda.set_device(local)
        backend = os.environ.get("PCCX_DIST_BACKEND", "nccl")
        launch.init_process_group(backend, torch.device(args.device) if backend == "nccl" else None)
    return rank, world


def finish_ranks(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def summary_device(args):
    return torch.device(args.device) if os.environ.get("PCCX_DIST_BACKEND", "nccl") == "nccl" else torch.device("cpu")


def load_models(args, need_gpu=True):
    from pccx import models
    if need_gpu and not torch.cuda.is_available():
        raise SystemExit("pccx needs a ROCm GPU: there is no CPU path")
    k = args.K // args.ALPHA
    ae = models.AE(K=args.K, k=k, d=args.d, L=args.L)
    prob = models.ConditionalProbabilityModel(args.L, args.d)
    ae.load_state_dict(torch.load(find_checkpoint(args.model_load_folder, "ae"), map_location="cpu", weights_only=True))
    prob.load_state_dict(torch.load(find_checkpoint(args.model_load_folder, "prob"), map_location="cpu", weights_only=True))
    return ae.pack(args.device), prob.pack(args.device)


def add_ply_io_flag(parser):
    parser.add_argument('--ply-io', choices=['python', 'threads'], default='python',
                        help="How .ply files are read and written: 'python' = one file at a time (plyio.read_point_cloud / save_point_cloud); "
                             "'threads' = a batch at a time on the library's host threads, unpacked to float32 on the GPU "
                             "(plyio.read_point_clouds / save_point_clouds).  The same arrays and the same files, bit for bit.")


def scan_plys(files):
    """--ply-io threads: the headers of `files` on the host threads (plyio.scan_point_clouds) -> their table; a file that cannot be read
    ends the tool, naming every such file and its cause -- called before any GPU work."""
    from pccx import plyio
    try:
        return plyio.scan_point_clouds(files)
    except ValueError as e:
        raise SystemExit(str(e))


class ScannedClouds(list):
    """--ply-io threads: what a tool knows of the files of a glob before it reads them -- one entry per file with the .shape its array
    will have, from the headers alone -- and the two calls that read them all at once (plyio.read_point_clouds)."""

    class Entry:
        def __init__(self, n):
            self.shape = (int(n), 3)

    def __init__(self, files):
        from pccx import plyio
        self.files = list(files)
        self.table = scan_plys(self.files)
        super().__init__(self.Entry(n) for n in self.table[:, plyio.N_VERTEX])

    def padded(self, device):
        """codec.pad_clouds of the files: (pc (F, N_max, 3), n list)"""
        return self._read(device, "padded")

    def packed(self, device):
        """codec.pack_clouds of the files: (points (M_total, 3), offsets (F + 1,), sizes list)"""
        return self._read(device, "packed")

    def _read(self, device, layout):
        # a whole set in one call, once: the pinned staging buffer of its size is not kept beside the copy in HBM
        from pccx import plyio
        out = plyio.read_point_clouds(self.files, device, layout, table=self.table)
        plyio.release_pinned()
        return out


def add_codec_flags(parser):
    parser.add_argument('--N0', type=int, help='Scale Transformation constant.', default=1024)
    parser.add_argument('--ALPHA', type=int, help='The factor of patch coverage ratio.', default=2)
    parser.add_argument('--K', type=int, help='Number of points in each patch.', default=256)
    parser.add_argument('--d', type=int, help='Bottleneck size.', default=16)
    parser.add_argument('--L', type=int, help='Quantization Level.', default=7)
    parser.add_argument('--device', help='AE Model Device (cuda)', default='cuda')
    parser.add_argument('--octree-mode', choices=['reference', 'full'], default='reference',
                        help="'reference' reproduces octree_np.decode as written (8 bits consumed, S=64); "
                             "'full' is the level-by-level decode.")
    parser.add_argument('--knn-search', choices=['auto', 'brute', 'grid'], default='auto',
                        help="Patch search of compress.py: 'brute' = the all-pairs kernels (clouds of up to 32768 points), 'grid' = the "
                             "exact grid index (any size, same patches), 'auto' = brute up to 32768 points and the grid above.")
    parser.add_argument('--p-split', type=int, default=0, metavar='G',
                        help="Write / read .p.bin in the split form: segments of G patches, each range-coded on its own behind a directory "
                             "of segment lengths, coded and decoded in parallel (whole rooms; 64 is the measured choice).  0 = the "
                             "reference's single stream.  Both sides must pass the same G; a split .p.bin is not a file the reference reads.")
    parser.add_argument('--prob', choices=['cloud', 'tiles'], default='cloud',
                        help="Probability model: 'cloud' = one workgroup per cloud (many small clouds); 'tiles' = every cloud's 16-centre "
                             "tiles dealt over the chip (whole rooms: a fraction of the time).  The same tables bit for bit, hence the same "
                             "files: the two sides need not agree.")
    parser.add_argument('--p-index', type=int, default=0, metavar='G',
                        help="Keep .p.bin the reference's single stream and write / read an entry-point index <name>.p.idx beside it: the "
                             "coder's state every G patches (12 bytes each), so that decompress.py decodes the one stream with one wave "
                             "per G patches and --region can enter it.  0 = no index.  Excludes --p-split.")
    parser.add_argument('--ragged', action='store_true',
                        help="Needs --octree-mode full.  Files of different point counts share a launch sequence (Codec.compress_ragged / "
                             "decompress_ragged): up to --batch files per call, each of K..32768 points and at most 1024 patches; other files "
                             "go the usual way, one point count per call, on both tools (they route file by file by the same rule on the "
                             "patch count).  Excludes --p-split, --p-index, --knn-search grid and compress.py's block centres.  The file formats do not change, and a cloud whose patch count "
                             "S = N*ALPHA/K is a multiple of 16 gets the very files written without this flag.  For every other S the "
                             "probability tables are the fused kernel's on the centres padded to a multiple of 16, which may differ in the "
                             "last unit from the tables used without the flag: such files must be written AND read with --ragged.")
    parser.add_argument('--batch', type=int, default=256, help='Clouds per launch sequence.')
    add_ply_io_flag(parser)
    parser.add_argument('--seed', type=int, default=11, help='Seed of the per-file FPS start index.')
