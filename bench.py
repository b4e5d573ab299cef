#!/usr/bin/env python3
"""bench.py -- points/s of compress + decompress (BASELINE.json metric) on N MI355X GPUs.

A "step" is one pass of the hot path over one batch of synthetic clouds: the loop bodies of
compress.py:90-152 and decompress.py:80-116 for ``--batch`` clouds of 8192 points (IPDAE K=256,
configs[1]).  Multi-GPU: clouds are sharded by file across ranks (one process per GPU, no data-path
collective; the collectives are the MAX of the wall time and one all-gather of a six-number summary per
rank), so scaling is weak.  ``python bench.py --gpus N`` without a torchrun environment starts the N rank
processes itself (pccx/launch.py) before anything touches a GPU.

The timed WINDOW is the reference's (``"window": "host-to-host"``): compress starts with the cloud in device
memory (compress.py:82-85 moves it before start_time) and ends with the bytes of the three files on the host
(compress.py:139-152); decompress starts from those host bytes (decompress.py:77-82) and ends with the
reconstructed XYZ on the host (decompress.py:110-116).  Every kernel stays on ONE compute stream (compress(i), then decompress(i-1)); only the
copies run beside them, on a copy stream ordered by events, into pinned double buffers, so kernel durations are
the same in both legs.  The HBM-resident rate (no copies) is reported beside it as ``value_resident``; its leg is
where the per-stage HIP-event times and the roofline of the dominant kernel are taken.

Prints ONE JSON line on rank 0.  A plain run (``bench.py --gpus N --steps K --warmup W``) does only what the headline needs: it
builds the codec, warms up, times the K host-to-host steps of the default arithmetic and prints the line (metric, value, unit,
ms_per_step, dtype, ...).  ``--dump-outputs DIR`` then writes what the last timed step handed its caller (a fixed sample of clouds: the
reconstructed XYZ and the three files' contents) as float32 / float64 .npy files; the inputs are the same from run to run.
Everything else is measured with ``--full`` only, which adds to the line
  roofline     -- the dominant kernel: algorithmic FLOPs per launch / its HIP-event duration against the
                  matrix-core peak of the arithmetic used (MI355X_MICROARCH.md: fp32 matrix 157.3 TFLOP/s;
                  bf16 dense 16x that, / 6 products for the three-way split = 419.5 fp32-equivalent);
  f32, bf16x3  -- the same step in the other arithmetic modes, each with its own host-to-host value, resident value, window checks,
                  stage table and roofline; ``precision_matched`` names the leg whose products are as wide as the reference's (f32);
  full_mode    -- the same clouds with octree_mode="full" (the decode that reconstructs all 64 centres) in the default arithmetic;
  cpu_baseline -- the CPU restatement of the reference loop (oracle/ref_pipeline.py), timed on this node's host
                  cores on a bounded sample, with its bpp / D1-PSNR and a 1-thread figure, rank 0 at N=1 only;
  and the resident leg, with_files, f16x2_vs_f32, bpp / D1-PSNR and the `secondary` block (configs[2], [3], [4]).
The other workloads (``--workload ...``) follow the same rule: CPU baselines, batch sweeps, other arithmetics, stage tables and
agreement checks only with ``--full``.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "point-cloud-compression_amd"))

# The host-to-host window overlaps its copies (packed streams out and back, 100 MB of XYZ out per step) with the kernels of the neighbouring
# steps.  That only holds while the copies run on the DMA ENGINES: as blit kernels (`__amd_rocclr_copyBuffer`, what the runtime uses with
# HSA_ENABLE_SDMA=0 and under rocprofv3) a 100 MB device-to-host copy stalls whatever kernel runs beside it for its whole 1.8 ms (the
# kernel's end-of-kernel release waits for the shader's PCIe writes; profiles/round4_kernel_trace.csv: normalize_kernel 52 us alone, 1838 us
# beside the copy) -- measured +2.2 ms per step with SDMA off against +0.0-0.3 with it on.  Said before the runtime starts; a value the
# environment already holds is left alone and reported in the line (`copy_engine`).
os.environ.setdefault("HSA_ENABLE_SDMA", "1")

N_POINTS, K_PATCH, ALPHA, N0, D_LAT, L_LEV = 8192, 256, 2, 1024, 16, 7
S_PATCH = N_POINTS * ALPHA // K_PATCH
AE_SEED, PROB_SEED = 11, 12
AE_LAST_GAIN = {"pn.mlp_Modules.3.0": 40.0}
PROB_GAIN = 2.0
F32_MATRIX_PEAK_TFLOPS = 157.3                      # MI355X_MICROARCH.md, "Peak FP32 (matrix)"
BF16_DENSE_PEAK_TFLOPS = 16 * F32_MATRIX_PEAK_TFLOPS  # same table: the f32 MFMA runs at 1/16 of BF16 (~2.5 PF dense)
B3_PRODUCTS = 6                                     # bf16 MFMA products per fp32 product in the three-way split
H2_PRODUCTS = 3                                     # fp16 MFMA products per fp32 product in the two-way split (fp16 dense peak = bf16's)

# algorithmic FLOPs per PATCH (2*MACs), from the layer shapes of AE.py:16-27
FLOP_SA = K_PATCH * 16 * (3 * 32 + 32 * 64 + 64 * 128) * 2
FLOP_PN = K_PATCH * (131 * 128 + 128 * 256 + 256 * 512 + 512 * D_LAT) * 2
K_SMALL = K_PATCH // ALPHA
FLOP_DEC = (D_LAT * 256 + 256 * 1024 + 1024 * K_SMALL * 128) * 2 + K_SMALL * (144 * 128 + 128 * 64 + 64 * 32 + 32 * 3) * 2
STAGE_FLOP = {"sa_forward": FLOP_SA, "pn_forward": FLOP_PN, "ae_decode": FLOP_DEC, "sa_pn_forward": FLOP_SA + FLOP_PN}
STAGE_KERNEL = {"sa_forward": "sa_forward_kernel", "pn_forward": "pn_forward_kernel", "ae_decode": "dec_main_kernel",
                "sa_pn_forward": "sa_pn_forward_b3_kernel"}
STAGE_KERNEL_H2 = {"ae_decode": "dec_main_h2_kernel", "sa_pn_forward": "sa_pn_forward_h2_kernel"}
MODE_DTYPE = {"f32": "f32",
              "bf16x3": "f32 (operands split into three bf16 pieces, six bf16-MFMA products per fp32 product, fp32 accumulate)",
              "f16x2": "f32 (operands split into two scaled fp16 pieces of 22-23 bits together, three fp16-MFMA products per fp32 product, fp32 accumulate)"}


def stage_kernel(stage, matmul):
    return STAGE_KERNEL_H2.get(stage, STAGE_KERNEL[stage]) if matmul == "f16x2" else STAGE_KERNEL[stage]


# the instantiation each mode launches at the bench shape (K = 256): the key of a kernel in profiles/round4*_traffic.json, whose PMC passes
# run all modes at once (older files are keyed by the bare name)
STAGE_KERNEL_FULL = {"f32": {"sa_forward": "sa_forward_kernel<false>", "pn_forward": "pn_forward_kernel<2>", "ae_decode": "dec_main_kernel<false, 2>"},
                     "bf16x3": {"sa_pn_forward": "sa_pn_forward_b3_kernel<true>", "ae_decode": "dec_main_kernel<true, 2>"},
                     "f16x2": {"sa_pn_forward": "sa_pn_forward_h2_kernel<true>", "ae_decode": "dec_main_h2_kernel<4>"}}


def _traffic_entry(kernels, stage, matmul):
    full = STAGE_KERNEL_FULL.get(matmul, {}).get(stage)
    if full in kernels:
        return kernels[full]
    return kernels[stage_kernel(stage, matmul)]          # KeyError -> the caller tries the next (older) file


def committed_traffic(stage, batch, matmul="bf16x3"):
    """HBM bytes per launch of the stage's kernel, NOT measured in this run: read from the newest committed rocprofv3
    --pmc pass (profiles/round*_traffic.json, separate passes, gfx950 corrections applied) and scaled linearly from the
    batch that pass ran at.  Returns (bytes or None, source)."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_traffic.json")), reverse=True):
        try:
            j = json.load(open(path))
            t = _traffic_entry(j["kernels"], stage, matmul)
            return int(t["hbm_bytes_per_launch"] * batch / j.get("batch", 256)), "scaled from committed PMC pass " + os.path.relpath(path, ROOT)
        except (OSError, KeyError, ValueError):
            continue
    return None, None


def committed_traffic_of(kernel, batch):
    """the same lookup by kernel name"""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_traffic.json")), reverse=True):
        try:
            j = json.load(open(path))
            ks = j["kernels"]
            t = ks[kernel] if kernel in ks else next(v for k_, v in ks.items() if k_.split("<")[0] == kernel)
            return int(t["hbm_bytes_per_launch"] * batch / j.get("batch", 256)), os.path.relpath(path, ROOT)
        except (OSError, KeyError, ValueError, StopIteration):
            continue
    return None, None


def committed_pmc(stage, matmul="bf16x3"):
    """Matrix-pipe busy fraction (SQ_VALU_MFMA_BUSY_CYCLES over the cycles of all SIMDs) and the clock the chip held during the
    stage's kernel (GRBM_GUI_ACTIVE / 8 / duration), from the same committed PMC passes -- NOT measured in this run."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_traffic.json")), reverse=True):
        try:
            t = _traffic_entry(json.load(open(path))["kernels"], stage, matmul)
            if "mfma_pipe_busy" in t:
                return {"mfma_pipe_busy": round(t["mfma_pipe_busy"], 4), "clock_ghz_under_load": round(t.get("clock_ghz_under_load", 0.0), 3) or None,
                        "peak_quoted_at_ghz": 2.4, "source": "committed PMC pass " + os.path.relpath(path, ROOT)}
        except (OSError, KeyError, ValueError):
            continue
    return None


def seeded_state_dict(module, seed, gain=1.0, last_gain=None):
    """Same deterministic fill as oracle.ref_model.seeded_state_dict (kept local: the product side
    of bench.py must not import the oracle)."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    sd = {}
    cur = module.state_dict()
    for k, v in cur.items():
        shape = tuple(v.shape)
        if len(shape) == 0:
            sd[k] = v.clone()
            continue
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else int(shape[0])
        if k.endswith("bias"):
            fan_in = int(np.prod(tuple(cur[k[:-4] + "weight"].shape)[1:]))
        b = gain / np.sqrt(max(fan_in, 1))
        a = rng.uniform(-b, b, size=shape).astype(np.float32)
        for sub, g in (last_gain or {}).items():
            if sub in k:
                a = a * np.float32(g)
        sd[k] = torch.from_numpy(a)
    return sd


def host_cores_available():
    """Cores this process may use: the affinity mask capped by the cgroup CPU quota (the CPU leg runs on all of them)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // per))
        except (OSError, ValueError):
            pass
    return max(1, n)


def host_cores():
    """Threads of the CPU legs: every core this process may use, unless PCCX_CPU_THREADS names a number (then `cores` in the line is that
    number and `cores_available` beside it shows what was left unused)."""
    n = host_cores_available()
    forced = os.environ.get("PCCX_CPU_THREADS")
    return max(1, min(n, int(forced))) if forced else n


def cores_fields():
    return {"cores": host_cores(), "cores_available": host_cores_available(), "cpu_count": os.cpu_count()}


def cpu_baseline(max_clouds, budget_s):
    """Reference-structured CPU loop (oracle) on a bounded sample of the same workload: all host cores for ~2/3 of the
    budget (the reported value, with bpp and D1-PSNR of those clouds), then one thread for the rest."""
    from pccx import launch as _launch
    _launch.restore_affinity()                 # the CPU leg runs on every core the process was given, not only the GPU's NUMA node
    import numpy as np
    import torch
    from oracle import ref_model, ref_pipeline
    from pccx import synth
    ae = ref_model.AE(K_PATCH, K_SMALL, D_LAT, L_LEV).eval()
    ae.load_state_dict(ref_model.seeded_state_dict(ae, AE_SEED, last_gain=AE_LAST_GAIN))
    prob = ref_model.ConditionalProbabilityModel(L_LEV, D_LAT).eval()
    prob.load_state_dict(ref_model.seeded_state_dict(prob, PROB_SEED, gain=PROB_GAIN))

    def leg(threads, max_n, min_n, budget):
        torch.set_num_threads(threads)
        ref_pipeline.compress_one(synth.cad_cloud(11, N_POINTS), ae, prob, 0)          # warm-up, discarded
        tot, n, bits, psnr, t_start, per = 0.0, 0, 0, 0.0, time.time(), []
        while n < max_n and (n < min_n or time.time() - t_start < budget):
            pc = synth.cad_cloud(11 + n, N_POINTS)
            o, tc = ref_pipeline.compress_one(pc, ae, prob, (n * 97) % N_POINTS)
            rec, td = ref_pipeline.decompress_one(o["s"], o["p"], o["c"], ae, prob)
            tot += tc + td
            per.append((8 * (len(o["s"]) + len(o["p"]) + len(o["c"])), ref_pipeline.d1_psnr(pc, rec)))   # eval.py:189; outside the windows
            n += 1
        bits, psnr = sum(p[0] for p in per), sum(p[1] for p in per)
        same = per[:32] if n >= 32 else None       # the GPU leg's 32 base shapes are exactly seeds 11..42 with these FPS starts
        q32 = {"bpp": sum(p[0] for p in same) / (32 * N_POINTS), "d1_psnr_db": sum(p[1] for p in same) / 32} if same else None
        return n, tot, bits / (n * N_POINTS), psnr / n, q32

    cores = host_cores()
    n, tot, bpp, psnr, q32 = leg(cores, max_clouds, 4, budget_s * 2 / 3)
    n1, tot1, _, _, _ = leg(1, max(2, max_clouds // 4), 2, budget_s / 3)
    return {"value": n * N_POINTS / tot, "unit": "points/s", **cores_fields(), "kind": "port",
            "sample": f"{n} synthetic 8192-pt clouds (the first {n} of the GPU leg's seeds), compress+decompress windows of "
                      f"compress.py:85-154 / decompress.py:77-118, CPU restatement of the reference loop (torch CPU fp32 + C oracle)",
            "ms_per_cloud": 1e3 * tot / n, "bpp": bpp, "d1_psnr_db": psnr,
            "same_clouds_as_gpu": q32,      # bpp / D1-PSNR on the first 32 clouds = the 32 base shapes of the GPU leg at N = 1 (its "base_shapes")
            "one_thread": {"value": n1 * N_POINTS / tot1, "unit": "points/s", "cores": 1, "sample": f"{n1} clouds", "ms_per_cloud": 1e3 * tot1 / n1}}


def cpu_baseline_blocks(blocks, starts, budget_s):
    """configs[3] beside the GPU number: the CPU restatement of the reference loop (oracle/ref_pipeline.py) on a bounded sample of the
    SAME 8192-point Morton blocks the GPU leg compresses (handed over from the device: the partition itself, one sort per room, is not
    re-done on the CPU), compress + decompress windows as in cpu_baseline()."""
    from pccx import launch as _launch
    _launch.restore_affinity()                 # the CPU leg runs on every core the process was given, not only the GPU's NUMA node
    import torch
    from oracle import ref_model, ref_pipeline
    ae = ref_model.AE(K_PATCH, K_SMALL, D_LAT, L_LEV).eval()
    ae.load_state_dict(ref_model.seeded_state_dict(ae, AE_SEED, last_gain=AE_LAST_GAIN))
    prob = ref_model.ConditionalProbabilityModel(L_LEV, D_LAT).eval()
    prob.load_state_dict(ref_model.seeded_state_dict(prob, PROB_SEED, gain=PROB_GAIN))
    cores = host_cores()
    torch.set_num_threads(cores)
    ref_pipeline.compress_one(blocks[0], ae, prob, int(starts[0]))                    # warm-up, discarded
    tot, n, bits, psnr, t0 = 0.0, 0, 0, 0.0, time.time()
    while n < len(blocks) and (n < 2 or time.time() - t0 < budget_s):
        o, tc = ref_pipeline.compress_one(blocks[n], ae, prob, int(starts[n]))
        rec, td = ref_pipeline.decompress_one(o["s"], o["p"], o["c"], ae, prob)
        tot += tc + td
        bits += 8 * (len(o["s"]) + len(o["p"]) + len(o["c"]))
        psnr += ref_pipeline.d1_psnr(blocks[n], rec)
        n += 1
    return {"value": n * N_POINTS / tot, "unit": "points/s", **cores_fields(), "kind": "port",
            "sample": f"the first {n} of the GPU leg's 8192-point Morton blocks (room 0), compress+decompress windows of compress.py:85-154 / "
                      f"decompress.py:77-118 per block, CPU restatement of the reference loop (torch CPU fp32 + C oracle); partition not re-done",
            "ms_per_block": 1e3 * tot / n, "bpp": bits / (n * N_POINTS), "d1_psnr_db": psnr / n}


def cpu_baseline_pppf(state_dict, patches, Kp, budget_s):
    """configs[2] beside the GPU number: the oracle's PPPF_AE forward (oracle/ref_families.py, torch CPU fp32, eval mode) on a bounded
    sample of the same patches, 8 patches (one cloud) per call as the reference's patch loop feeds the model."""
    from pccx import launch as _launch
    _launch.restore_affinity()                 # the CPU leg runs on every core the process was given, not only the GPU's NUMA node
    import torch
    from oracle import ref_families
    m = ref_families.PPPF_AE(K=Kp, k=Kp // ALPHA, d=16, L=7).eval()
    m.load_state_dict(state_dict)
    cores = host_cores()
    torch.set_num_threads(cores)
    x = patches.cpu()
    with torch.no_grad():
        m(x[:8])                                                                     # warm-up, discarded
        tot, n, t0 = 0.0, 0, time.time()
        while n + 8 <= x.shape[0] and (n < 16 or time.time() - t0 < budget_s):
            t1 = time.time()
            m(x[n:n + 8])
            tot += time.time() - t1
            n += 8
    return {"value": n * Kp / tot, "unit": "points/s", **cores_fields(), "kind": "port",
            "sample": f"the first {n} of the GPU leg's {Kp}-point patches, PPPF_AE forward (encode + decode) 8 patches per call, CPU restatement of "
                      f"PPPF_AE.py:114-150 (torch CPU fp32)", "ms_per_patch": 1e3 * tot / n}


def cpu_baseline_pppe_train(state_dict, x, starts, budget_s):
    """configs[4] beside the GPU number: the oracle's training iteration (oracle/ref_train.py: torch autograd + torch.optim.Adam on the
    restated PointCloudAE) on the same batch; the brute-force Chamfer of an 8192-point cloud makes one step seconds long, so the sample
    is a few steps (at least one after the warm-up)."""
    from pccx import launch as _launch
    _launch.restore_affinity()                 # the CPU leg runs on every core the process was given, not only the GPU's NUMA node
    import torch
    from oracle import ref_families, ref_train
    m = ref_families.PointCloudAE(64, 16, N_POINTS)
    m.load_state_dict(state_dict)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    cores = host_cores()
    torch.set_num_threads(cores)
    xb = x.cpu()
    ref_train.train_step(m, opt, xb, starts, lam=1e-3)                               # warm-up, discarded
    tot, n, t0 = 0.0, 0, time.time()
    while n < 1 or time.time() - t0 < budget_s:
        t1 = time.time()
        loss, _, _ = ref_train.train_step(m, opt, xb, starts, lam=1e-3)
        tot += time.time() - t1
        n += 1
    return {"value": n * xb.shape[0] / tot, "unit": "clouds/s", **cores_fields(), "kind": "port",
            "sample": f"{n} optimisation step(s) on the GPU leg's batch of {xb.shape[0]} x {N_POINTS} points, CPU restatement of "
                      f"train_pppe_pcd_ae.py:184-226 without autocast (torch autograd + torch.optim.Adam)", "ms_per_step": 1e3 * tot / n, "loss": loss}


def cpu_baseline_ipdae_train(cfg, cloud, start, budget_s):
    """The IPDAE training step beside the GPU number: oracle.ref_train.ipdae_train_step (train.py:162-236 restated on torch CPU, pinned to
    the reference's own run by tests/test_train_ipdae.py) from the same weights on the same cloud; the brute-force Chamfer of 8192 x 8192
    points makes one step seconds long, so the sample is a few steps (at least one after the warm-up)."""
    from pccx import launch as _launch
    _launch.restore_affinity()
    import torch
    from oracle import ref_model, ref_train
    K, k, d, L = cfg
    ae, prob = ref_model.AE(K=K, k=k, d=d, L=L), ref_model.ConditionalProbabilityModel(L, d)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, 3)), prob.load_state_dict(ref_model.seeded_state_dict(prob, 4, gain=2.0))
    opt = torch.optim.Adam(list(ae.parameters()) + list(prob.parameters()), lr=5e-4)
    cores = host_cores()
    torch.set_num_threads(cores)
    xb = cloud.cpu()
    ref_train.ipdae_train_step(ae, prob, opt, xb, start, 1e-6, K=K)                    # warm-up, discarded
    tot, n, t0 = 0.0, 0, time.time()
    while n < 1 or time.time() - t0 < budget_s:
        t1 = time.time()
        out = ref_train.ipdae_train_step(ae, prob, opt, xb, start, 1e-6, K=K)
        tot += time.time() - t1
        n += 1
    return {"value": n * xb.shape[0] / tot, "unit": "clouds/s", **cores_fields(), "kind": "port",
            "sample": f"{n} optimisation step(s) on the GPU leg's first cloud ({xb.shape[1]} points, 64 patches of {K}), CPU restatement of "
                      f"train.py:162-236 (torch autograd + torch.optim.Adam; the Chamfer term by brute force over 8192 x 8192 pairs -- pytorch3d is "
                      f"absent here -- which is most of a step)", "ms_per_step": 1e3 * tot / n, "loss": out["loss"]}


# =====================================================================================================================
# distributed plumbing
# =====================================================================================================================
class Ranks:
    def __init__(self, args):
        import torch
        from pccx import launch
        self.rank, self.local, self.world = launch.rank_env()
        self.backend = args.dist_backend
        if self.backend == "gloo":
            self.local = self.local % max(torch.cuda.device_count(), 1)      # rehearsal: ranks may share a GPU
        self.gpu = args.workload != "launch-check"
        if self.gpu:
            have = torch.cuda.device_count()
            if self.local >= have:                                           # the launcher parent does not look at the GPUs: we do
                raise SystemExit(f"bench.py rank {self.rank}: LOCAL_RANK {self.local} but only {have} GPU(s) visible "
                                 f"(--gpus {self.world}; use --dist-backend gloo to rehearse the N>1 path on fewer GPUs)")
            torch.cuda.set_device(self.local)
            self.dev = torch.device("cuda", self.local)
        else:
            self.dev = torch.device("cpu")
        self.cdev = self.dev if self.backend == "nccl" else torch.device("cpu")   # where the tiny collectives live
        numa = getattr(args, "numa", None) or {"numa_node": -1, "cpus_bound": 0, "mempolicy": False}
        self.info = {"rccl_world": 1, "dist_backend": None, "rank_devices": [self.local if self.gpu else None],
                     "rank_numa": [{"rank": 0, "numa_node": numa["numa_node"], "cpus_bound": numa["cpus_bound"], "mempolicy": bool(numa["mempolicy"]),
                                    "note": numa.get("note")}]}
        self.rank_seconds = {}
        # PCCX_DIST_SINGLE_RANK=1: a ONE-rank process group whose collectives really run (pccx.dist.collectives_active) -- the rehearsal of
        # the RCCL plumbing a one-GPU box allows; the line then says dist_backend "rccl ... one-rank rehearsal"
        self.grouped = self.world > 1 or os.environ.get("PCCX_DIST_SINGLE_RANK") == "1"
        if self.grouped:
            import torch.distributed as dist
            if self.world == 1:
                os.environ.setdefault("RANK", "0"), os.environ.setdefault("WORLD_SIZE", "1")
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1"), os.environ.setdefault("MASTER_PORT", str(launch.free_port()))
            launch.init_process_group(self.backend, self.dev if self.backend == "nccl" else None)
            # what the driver can check an N-rank run by: the size of the process group the collectives ran on and the device
            # index every rank bound (one all_gather of an int, outside every timed region)
            mine = torch.tensor([self.local if self.gpu else -1, numa["numa_node"], numa["cpus_bound"], int(bool(numa["mempolicy"]))],
                                dtype=torch.int64, device=self.cdev)
            got = [torch.zeros_like(mine) for _ in range(self.world)]
            dist.all_gather(got, mine)
            got = [[int(v) for v in t.tolist()] for t in got]
            self.info = {"rccl_world": dist.get_world_size(),
                         "dist_backend": ("rccl (torch 'nccl')" if self.backend == "nccl" else "gloo") + (", one-rank rehearsal" if self.world == 1 else ""),
                         "rank_devices": [t[0] if t[0] >= 0 else None for t in got],
                         # where every rank's host threads and new pages were placed BEFORE its first GPU call (pccx/launch.py)
                         "rank_numa": [{"rank": r, "numa_node": t[1], "cpus_bound": t[2], "mempolicy": bool(t[3])} for r, t in enumerate(got)]}

    def barrier(self):
        if self.grouped:
            import torch.distributed as dist
            dist.barrier()

    def max_seconds(self, dt, tag=None):
        """MAX over ranks of a timed region's wall time; with `tag`, every rank's own time is kept too (rank_seconds[tag]: a straggler
        is visible in the line as per-rank ms_per_step min / max)."""
        from pccx import dist as pdist
        if not self.grouped:
            if tag:
                self.rank_seconds[tag] = [dt]
            return dt
        if tag:
            self.rank_seconds[tag] = [float(v) for v in pdist.gather_summaries([dt], self.cdev)[:, 0].tolist()]
            return max(self.rank_seconds[tag])
        return pdist.max_over_ranks(dt, self.cdev)

    def rank_ms(self, tag, steps):
        v = [1e3 * s_ / max(steps, 1) for s_ in self.rank_seconds.get(tag, [])]
        return {"min": min(v), "max": max(v), "per_rank": [round(x, 4) for x in v]} if v else None

    def summaries(self, local_vec):
        """RCCL all_gather of the dist.SUMMARY_FIELDS vector (bits, points, psnr_sum, chamfer_sum, files, seconds)."""
        from pccx import dist as pdist
        return pdist.reduce_summaries(pdist.gather_summaries(local_vec, self.cdev))

    def close(self):
        if self.grouped:
            import torch.distributed as dist
            dist.destroy_process_group()


_SETTLED = [False]


def settle(rk, seconds=0.3):
    """Once per process, in front of its FIRST timed region: `seconds` of untimed GPU fill kernels.  On this pool a fresh process stalls once
    for 50-90 ms somewhere in its first ~0.1 s of GPU activity (three probes, tools/experiments/r5/pppf_alloc_probe.py: the stall follows
    the elapsed busy time, not the launch count, the allocator or a kernel -- a clock / power-state transition); a short workload (PPPF
    forward: W = 2 warm-up steps of 6 ms) would otherwise time it inside its K steps (19 ms per step measured instead of 6.2)."""
    if _SETTLED[0] or not getattr(rk, "gpu", False):
        return
    _SETTLED[0] = True
    import torch
    buf = torch.empty(64 << 20, device=rk.dev, dtype=torch.float32)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(8):
            buf.fill_(1.0)
        torch.cuda.synchronize()
    del buf


def timed(rk, fn, steps, sync, tag=None):
    """EXACTLY ``steps`` calls of fn between barrier + synchronize on both sides; MAX over ranks.  With `tag`, each rank's time up to its
    own synchronize (before the closing barrier) is kept as well (Ranks.rank_ms)."""
    settle(rk)
    rk.barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    sync()
    own = time.perf_counter() - t0
    rk.barrier()
    dt = time.perf_counter() - t0
    if tag:
        rk.max_seconds(own, tag)
    return rk.max_seconds(dt)


# =====================================================================================================================
# workloads
# =====================================================================================================================
def cpu_leg_allowed(args, rk):
    """The CPU baseline runs with --full, on rank 0 at N = 1 only (with N > 1 the ranks would wait in a barrier for a leg that says nothing
    about them)."""
    return args.full and rk.world == 1 and args.cpu_clouds > 0


def run_launch_stub(args, rk):
    """A secondary 'workload' without GPU work, for the launch-check: one timed region (the same barriers as the real ones), a dict from rank 0."""
    dt = timed(rk, lambda i: None, args.steps, lambda: None)
    if rk.rank != 0:
        return None
    return {"metric": "launch-check stub", "value": float(rk.world), "n_gpus": rk.world, "steps": args.steps, "ms_per_step": 1e3 * dt / max(args.steps, 1),
            "cpu_baseline": {"value": 1.0, "cores": 1, "kind": "port", "sample": "none"} if cpu_leg_allowed(args, rk) else None}


def bench_launch_check(args, rk):
    """No GPU: proves the self-launch (rank environment, rendezvous on 127.0.0.1, one JSON line from rank 0) and the
    summary all-gather; used by tests/test_sharding_gloo.py on CPU."""
    local = [1000.0 * (rk.rank + 1), 8192.0 * (rk.rank + 1), 30.0 + rk.rank, 1e-4 * (rk.rank + 1), float(rk.rank + 1), 0.5 + rk.rank]
    dt = timed(rk, lambda i: None, args.steps, lambda: None)
    s = rk.summaries(local)
    res = None
    if rk.rank == 0:
        res = {"metric": "launch-check", "value": float(s["files"]), "unit": "files", "n_gpus": rk.world, **rk.info, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": 1e3 * dt / max(args.steps, 1), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "none", "data": "synthetic",
               "config": {"workload": "launch-check (no GPU work)", "dist_backend": rk.backend}, "summary": s,
               "cpu_baseline": {"value": 1.0, "cores": 1, "kind": "port", "sample": "none"} if cpu_leg_allowed(args, rk) else None}
    # the --full line's secondary block, with stubs for the three workloads: every rank runs them, rank 0 alone emits, once
    if args.full and not args.no_secondary:
        sec = run_secondaries(args, rk, res, specs=(("stub_a", "run_launch_stub", {}), ("stub_b", "run_launch_stub", {})))
        if res is not None:
            res["secondary"] = sec
    if res is not None:
        print(json.dumps(res), flush=True)


def build_codec(rk, matmul, octree_mode):
    from pccx import codec, models
    ae = models.AE(K_PATCH, K_SMALL, D_LAT, L_LEV)
    ae.load_state_dict(seeded_state_dict(ae, AE_SEED, last_gain=AE_LAST_GAIN))
    prob = models.ConditionalProbabilityModel(L_LEV, D_LAT)
    prob.load_state_dict(seeded_state_dict(prob, PROB_SEED, gain=PROB_GAIN))
    ae.pack(rk.dev)
    prob.pack(rk.dev)
    return codec.Codec(ae, prob, K=K_PATCH, ALPHA=ALPHA, N0=N0, octree_mode=octree_mode, matmul=matmul), ae, prob


DUMP_CLOUDS, DUMP_SEED = 256, 0       # --dump-outputs: a fixed, seeded sample of the batch's clouds (~28 MB for 256)


def dump_ipdae_outputs(directory, packed_host, out_host, B, s_stride, p_cap):
    """What the last timed step of the host-to-host window handed its caller, for the clouds of a fixed seeded sample: the
    reconstructed XYZ and the contents of the three files (.s.bin / .p.bin bytes as float32 0..255, zero past each file's end; .c.bin as
    float32; the byte counts as float64)."""
    import numpy as np
    from pccx import codec
    os.makedirs(directory, exist_ok=True)
    h = codec.Compressed.from_packed(packed_host, B, s_stride, p_cap, N_POINTS)
    idx = np.sort(np.random.default_rng(DUMP_SEED).choice(B, min(B, DUMP_CLOUDS), replace=False))

    def file_bytes(rows, nbytes):
        b = rows.numpy()[idx].astype(np.float32)
        b[np.arange(b.shape[1])[None, :] >= nbytes[:, None]] = 0.0
        return b
    s_n, p_n = h.s_nbytes.numpy()[idx], h.p_nbytes.numpy()[idx]
    arrays = {"reconstruction": out_host.numpy()[idx].astype(np.float32), "s_bin": file_bytes(h.s_bytes, s_n),
              "p_bin": file_bytes(h.p_bytes, p_n), "c_bin": h.c.numpy()[idx].astype(np.float32),
              "s_nbytes": s_n.astype(np.float64), "p_nbytes": p_n.astype(np.float64), "cloud_index": idx.astype(np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), a)
    print("[bench] outputs of the last timed step (%d of %d clouds, %.1f MB) written to %s" %
          (len(idx), B, sum(a.nbytes for a in arrays.values()) / 1e6, directory), file=sys.stderr, flush=True)


def roofline_of(stages, steps, P, matmul, batch):
    """Dominant transform kernel of a resident leg: algorithmic FLOPs per launch / mean HIP-event duration of its launches."""
    per_step_ms = {k: v[0] * v[1] / steps for k, v in stages.items()}
    dom = max((k for k in STAGE_FLOP if k in stages), key=lambda k: per_step_ms[k])
    dur_ms = stages[dom][0]
    achieved = STAGE_FLOP[dom] * P / (dur_ms * 1e-3) / 1e12
    if matmul == "bf16x3":
        peak = BF16_DENSE_PEAK_TFLOPS / B3_PRODUCTS
        note = ("fp32-equivalent TFLOP/s: each fp32 product = %d bf16 MFMA products (three-way split), so peak = bf16 dense "
                "%.0f / %d; the same fraction as real bf16 FLOP/s (%.0f) over %.0f" %
                (B3_PRODUCTS, BF16_DENSE_PEAK_TFLOPS, B3_PRODUCTS, achieved * B3_PRODUCTS, BF16_DENSE_PEAK_TFLOPS))
    elif matmul == "f16x2":
        peak = BF16_DENSE_PEAK_TFLOPS / H2_PRODUCTS
        note = ("fp32-equivalent TFLOP/s: each fp32 product = %d fp16 MFMA products (two-way split), so peak = fp16 dense "
                "%.0f / %d; the same fraction as real fp16 FLOP/s (%.0f) over %.0f" %
                (H2_PRODUCTS, BF16_DENSE_PEAK_TFLOPS, H2_PRODUCTS, achieved * H2_PRODUCTS, BF16_DENSE_PEAK_TFLOPS))
    else:
        peak, note = F32_MATRIX_PEAK_TFLOPS, "exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) against the fp32 matrix peak"
    traffic, src = committed_traffic(dom, batch, matmul)
    # every stage of STAGE_FLOP brackets ONE kernel (the in-patch neighbour tables of the fused encoders are a stage of their own,
    # "patch_knn16", since round 4): `achieved` is the kernel's algorithmic FLOPs over the HIP-event duration of its launches
    stage_kernels = [stage_kernel(dom, matmul)]
    rf = {"kernel": dom, "kernel_name": stage_kernel(dom, matmul), "stage_kernels": stage_kernels, "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
          "traffic": traffic, "traffic_source": src, "launch_ms": dur_ms, "flop_per_launch": STAGE_FLOP[dom] * P,
          "arithmetic": matmul, "note": note, "window": "resident leg (single stream; HIP events per stage)",
          "pmc": committed_pmc(dom, matmul)}
    tfl = {k: STAGE_FLOP[k] * P / (stages[k][0] * 1e-3) / 1e12 for k in STAGE_FLOP if k in stages}
    return rf, per_step_ms, tfl


def compare_modes(a, b, B, s_stride, p_cap, codec):
    """The default arithmetic against the exact-fp32 one on the SAME clouds of the timed legs: quantised symbols, the bytes of the three files
    per cloud, the reconstruction (absolute, in units of the cloud's longest side as the parity tests state it)."""
    import torch
    ca, cb = (codec.Compressed.from_packed(x["packed"], B, s_stride, p_cap, N_POINTS) for x in (a, b))

    def rows_equal(ra, na, rb, nb):
        m = torch.arange(ra.shape[1])[None, :] < na.long()[:, None]
        return (na == nb) & ((ra == rb) | ~m).all(dim=1)
    same_s = rows_equal(ca.s_bytes, ca.s_nbytes, cb.s_bytes, cb.s_nbytes)
    same_p = rows_equal(ca.p_bytes, ca.p_nbytes, cb.p_bytes, cb.p_nbytes)
    same_c = (ca.c.view(torch.int32) == cb.c.view(torch.int32)).all(dim=1)
    qa, qb = a["q"].view(B, -1), b["q"].view(B, -1)
    sym_same = (qa == qb).all(dim=1)
    diff = (a["out"] - b["out"]).abs().amax(dim=(1, 2)) / a["longest"]
    agree = diff[sym_same]
    return {"clouds": B, "symbols": int(qa.numel()), "symbols_differing": int((qa != qb).sum()),
            "clouds_with_identical_files": int((same_s & same_p & same_c).sum()),
            "clouds_with_identical_s_bin": int(same_s.sum()), "clouds_with_identical_p_bin": int(same_p.sum()), "clouds_with_identical_c_bin": int(same_c.sum()),
            "max_recon_diff": float((a["out"] - b["out"]).abs().max()), "max_recon_diff_over_longest": float(diff.max()),
            "max_recon_diff_over_longest_where_symbols_agree": float(agree.max()) if agree.numel() else None,
            "note": "both codecs run on the batch of the timed legs after them; a symbol differs only where the two arithmetics land on "
                    "opposite sides of a rounding boundary (tests allow <= 1e-5 of the symbols); .p.bin may also differ by an integer-CDF entry +-1"}


def bench_ipdae(args, rk):
    import numpy as np
    import torch
    from pccx import codec, ops, synth

    dev, B = rk.dev, args.batch
    # shard by file: global cloud i -> rank i % world; 32 distinct shapes per rank, tiled to the batch
    base = np.stack([synth.cad_cloud(11 + rk.rank + rk.world * i, N_POINTS) for i in range(min(B, 32))])
    clouds = torch.from_numpy(np.concatenate([base] * ((B + base.shape[0] - 1) // base.shape[0]))[:B]).to(dev)
    # every cloud of the batch distinct: copy c of the 32 shapes is turned by c * 2 pi / 37 about the vertical axis through the
    # cube's centre and scaled by 1 - c / 256 (the first 32 stay as generated: the CPU leg's clouds)
    cidx = torch.arange(B, device=dev) // base.shape[0]
    ang = cidx.to(torch.float32) * (2.0 * 3.141592653589793 / 37.0)
    ca, sa_, sc = torch.cos(ang)[:, None], torch.sin(ang)[:, None], (1.0 - cidx.to(torch.float32) / 256.0)[:, None]
    x0, y0 = clouds[..., 0] - 0.5, clouds[..., 1] - 0.5
    clouds = torch.stack([(ca * x0 - sa_ * y0) * sc + 0.5, (sa_ * x0 + ca * y0) * sc + 0.5, (clouds[..., 2] - 0.5) * sc + 0.5], dim=-1).contiguous()
    starts = torch.from_numpy((np.arange(B) * 97 + rk.rank) % N_POINTS).to(dev)
    P = B * S_PATCH
    sync = torch.cuda.synchronize
    modes = [args.matmul] + [m for m in ("f32", "bf16x3", "f16x2") if m != args.matmul and not args.one_mode]
    from pccx import models as _models                                            # sizes of the packed stream buffer (codec.packed_layout)
    S = S_PATCH
    s_stride, p_cap = (ops.octree_bits_capacity(S) + 7) // 8, _models.range_cap(S * D_LAT)
    row = codec.packed_layout(1, s_stride, p_cap)[-1]                             # bytes per cloud
    nb_ = min(B, int(base.shape[0]))                # the unturned base shapes = the CPU leg's first clouds (cpu_baseline.same_clouds_as_gpu)

    def measure(cd, with_files=False, keep_for_compare=False, rank_tag=None, lean=False):
        """Both legs of one (arithmetic mode, octree mode): resident (per-stage events) and host-to-host (the reference's window).
        lean (a plain run): the resident steps only warm up, the host-to-host leg alone is timed, and its last step's host buffers
        are returned (host_packed, host_out) instead of being checked against the resident leg."""
        keep = {}

        # ---- resident leg: one stream, everything stays in HBM, per-stage events -------------------------------
        def step_resident(i):
            comp = cd.compress(clouds, starts)
            return comp, cd.decompress(comp, S=S)
        for _ in range(args.warmup):
            comp, out = step_resident(0)
        sync()
        r = {}
        if not lean:
            timer = ops.StageTimer()
            ops.set_timer(timer)
            dt_res = timed(rk, lambda i: keep.__setitem__("r", step_resident(i)), args.steps, sync)
            ops.set_timer(None)
            comp, out = keep["r"]
            stages = {k: (ms / n, n) for k, (ms, n) in timer.totals_ms().items()}
            r = {"dt_res": dt_res, "stages": stages, "bits": float(comp.bits().sum()), "psnr_sum": float(codec.d1_psnr(clouds, out).sum()),
                 "chamfer_sum": float(codec.normalized_chamfer(clouds, out).sum())}
            r["base_shapes"] = {"clouds": nb_, "bpp": float(comp.bits()[:nb_].sum()) / (nb_ * N_POINTS),
                                "d1_psnr_db": float(codec.d1_psnr(clouds[:nb_], out[:nb_]).sum()) / nb_}
        if rank_tag and not lean:
            # the resident pipeline's shortcut, beside the figure above: decompress handed the Compressed object it came from takes the
            # integer CDF compress built instead of evaluating the probability model again (codec.decompress(reuse_cdf=True)); the
            # host-to-host window below never does (its decompress starts from bytes, as decompress.py:88-92)
            def step_reuse(i):
                c_ = cd.compress(clouds, starts)
                keep["rr"] = cd.decompress(c_, S=S, reuse_cdf=True)
            step_reuse(0)
            r["dt_res_reuse"] = timed(rk, step_reuse, args.steps, sync)
            r["reuse_equals_recompute"] = bool(torch.equal(keep.pop("rr"), out))

        # ---- host-to-host leg (the reference's window): two streams, pinned double buffers ---------------------
        copy_stream = torch.cuda.Stream(device=dev)
        main_stream = torch.cuda.current_stream()
        pin_comp = [torch.empty(row * B, dtype=torch.uint8).pin_memory() for _ in range(2)]
        pin_out = [torch.empty(B, N_POINTS, 3, dtype=torch.float32).pin_memory() for _ in range(2)]
        pending = []

        def finish(up, ready, j):
            """decompress(step) from the host bytes that came back on the copy stream; its XYZ goes to the host there too."""
            main_stream.wait_event(ready)
            o = cd.decompress(codec.Compressed.from_packed(up, B, s_stride, p_cap, N_POINTS), S=S)
            done = torch.cuda.Event()
            done.record(main_stream)
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(done)
                pin_out[j].copy_(o, non_blocking=True)                    # reconstructed XYZ on the host
            o.record_stream(copy_stream)

        def step_host(i, last=None):
            # ALL kernels stay on the one compute stream, in the order compress(i), decompress(i-1): their durations are what
            # the resident leg measures.  Only the copies run beside them, on the copy stream, ordered by events:
            #   compress(i) -> [D2H of the packed streams = the three files' bytes on the host, then the same bytes H2D]
            #   -> decompress(i) one step later -> [D2H of the XYZ].
            j = i % 2
            c = cd.compress(clouds, starts)
            ev = torch.cuda.Event()
            ev.record(main_stream)
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(ev)
                pin_comp[j].copy_(c.packed, non_blocking=True)            # ONE D2H per batch
                up = pin_comp[j].to(dev, non_blocking=True)               # decompress starts from the host bytes
                ready = torch.cuda.Event()
                ready.record(copy_stream)
            c.packed.record_stream(copy_stream)
            up.record_stream(main_stream)
            if pending:
                finish(*pending.pop())
            pending.append((up, ready, j))
            if i == (args.steps if last is None else last) - 1:           # the timed region ends with the last step's decompress
                finish(*pending.pop())
        copy_stream.wait_stream(main_stream)
        nw = max(args.warmup, 2)
        for i in range(nw):
            step_host(i, last=nw)
        sync()
        r["dt_host"] = timed(rk, step_host, args.steps, sync, tag=rank_tag)
        last = (args.steps - 1) % 2
        if lean:
            r["host_packed"], r["host_out"] = pin_comp[last], pin_out[last]      # what the last timed step handed its caller
            return r
        r["host_equals_resident"] = bool(torch.equal(pin_out[last], out.cpu()))
        hc = codec.Compressed.from_packed(pin_comp[last], B, s_stride, p_cap, N_POINTS)
        r["host_bytes_equal_resident"] = bool(torch.equal(hc.s_nbytes, comp.s_nbytes.cpu()) and torch.equal(hc.p_nbytes, comp.p_nbytes.cpu()))
        r["d2h_bytes_per_step"] = row * B + B * N_POINTS * 12
        del copy_stream, pin_comp, pin_out
        if with_files:
            # ---- the window WITH the file system in it (compress.py:139-152 writes the three files of a cloud inside its timer,
            # decompress.py:80-91,113 reads them back inside its own): the host-to-host leg with the files between its two copies.
            # compress(i) -> D2H of the packed streams -> [host: pccx_write_streams_host cuts the 3 x B files out of that one buffer;
            # pccx_read_streams_host fills the upload buffer from them] -> H2D -> decompress(i).  The host work of step i is done
            # while the GPU runs compress(i + 1) (the kernels are queued before the host waits for the D2H), like the copies.
            import shutil
            import tempfile
            tmp = tempfile.mkdtemp(prefix="pccx_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
            names = [f"{b_:05d}" for b_ in range(B)]
            copy_stream = torch.cuda.Stream(device=dev)
            pin_comp = [torch.empty(row * B, dtype=torch.uint8).pin_memory() for _ in range(2)]
            pin_up = [torch.zeros(row * B, dtype=torch.uint8).pin_memory() for _ in range(2)]
            pin_out = [torch.empty(B, N_POINTS, 3, dtype=torch.float32).pin_memory() for _ in range(2)]
            pending, host_s = [], [0.0, 0.0, 0]
            try:
                def finish_files(d2h, j):
                    d2h.synchronize()                                        # the packed streams of that step are on the host
                    t0 = time.perf_counter()
                    codec.write_streams(pin_comp[j], B, s_stride, p_cap, tmp, names)          # compress.py:139-152
                    t1 = time.perf_counter()
                    codec.read_streams(pin_up[j], B, s_stride, p_cap, tmp, names)             # decompress.py:80-91,113
                    t2 = time.perf_counter()
                    host_s[0] += t1 - t0
                    host_s[1] += t2 - t1
                    host_s[2] += 1
                    with torch.cuda.stream(copy_stream):
                        up = pin_up[j].to(dev, non_blocking=True)
                        ready = torch.cuda.Event()
                        ready.record(copy_stream)
                    up.record_stream(main_stream)
                    main_stream.wait_event(ready)
                    o = cd.decompress(codec.Compressed.from_packed(up, B, s_stride, p_cap, N_POINTS), S=S)
                    done = torch.cuda.Event()
                    done.record(main_stream)
                    with torch.cuda.stream(copy_stream):
                        copy_stream.wait_event(done)
                        pin_out[j].copy_(o, non_blocking=True)
                    o.record_stream(copy_stream)

                def step_files(i, last=None):
                    j = i % 2
                    c = cd.compress(clouds, starts)
                    ev = torch.cuda.Event()
                    ev.record(main_stream)
                    with torch.cuda.stream(copy_stream):
                        copy_stream.wait_event(ev)
                        pin_comp[j].copy_(c.packed, non_blocking=True)
                        d2h = torch.cuda.Event()
                        d2h.record(copy_stream)
                    c.packed.record_stream(copy_stream)
                    if pending:
                        finish_files(*pending.pop())
                    pending.append((d2h, j))
                    if i == (args.steps if last is None else last) - 1:
                        finish_files(*pending.pop())
                copy_stream.wait_stream(main_stream)
                nw = max(args.warmup, 2)
                for i in range(nw):
                    step_files(i, last=nw)
                sync()
                host_s[:] = [0.0, 0.0, 0]
                r["dt_files"], r["files_steps"] = timed(rk, step_files, args.steps, sync), args.steps
                last = (args.steps - 1) % 2
                r["files_equal_resident"] = bool(torch.equal(pin_out[last], out.cpu()))
                # the files themselves against Compressed.files(b) of the resident leg (the bytes compress.py would have written)
                same = 0
                for b_ in range(B):
                    s_, p_, c_ = comp.files(b_)
                    rd = lambda ext: open(os.path.join(tmp, names[b_] + ext), "rb").read()
                    same += int(rd(".s.bin") == s_ and rd(".p.bin") == p_ and rd(".c.bin") == c_)
                r["files_identical"] = same
                r["files_host_ms"] = {"write": 1e3 * host_s[0] / max(host_s[2], 1), "read": 1e3 * host_s[1] / max(host_s[2], 1)}
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            del copy_stream, pin_comp, pin_up, pin_out
        # what a comparison of two arithmetic modes needs (f16x2_vs_f32), kept on the host: symbols, file bytes, reconstruction
        if keep_for_compare:
            cx = cd.compress(clouds, starts, keep_extras=True)
            r["cmp"] = {"q": cx.extras["latent_q"].to(torch.int8).cpu(), "packed": cx.packed.cpu(), "out": cd.decompress(cx, S=S).cpu(),
                        "longest": cx.c[:, 3].cpu()}
        return r

    pts = B * N_POINTS * args.steps

    def headline(main):
        """The fields of the line that a plain run and a --full run share: the host-to-host leg of the default arithmetic."""
        return {
            "metric": "points/sec compress+decompress (ModelNet40-shaped 8192 K=256)",
            "value": rk.world * pts / main["dt_host"], "unit": "points/s",
            "n_gpus": rk.world, **rk.info, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * main["dt_host"] / args.steps,
            "rank_ms_per_step": rk.rank_ms("host", args.steps),      # each rank's own time for the same steps (before the closing barrier)
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": MODE_DTYPE[args.matmul], "data": "synthetic",
            "copy_engine": "HSA_ENABLE_SDMA=" + os.environ.get("HSA_ENABLE_SDMA", "unset"),
            "window": "host-to-host: cloud in HBM -> .s/.p/.c bytes on the host (compress.py:85-154) -> XYZ on the host "
                      "(decompress.py:77-118); kernels on one stream, copies overlapped on a copy stream",
            "config": {"workload": "IPDAE K=256 d=16 L=7, 8192-pt CAD-like synthetic clouds (configs[1])",
                       "clouds_per_gpu_per_step": B, "distinct_clouds_per_gpu": B, "base_shapes_per_gpu": int(base.shape[0]), "points_per_cloud": N_POINTS,
                       "patches_per_cloud": S_PATCH, "octree_mode": args.octree_mode, "sharding": f"file-sharded x{rk.world}",
                       "weights": "seeded random", "matmul": args.matmul},
        }

    if not args.full:
        # a plain run: the headline leg alone, then the line (everything else is --full's)
        cd, _, _ = build_codec(rk, args.matmul, args.octree_mode)
        main = measure(cd, rank_tag="host", lean=True)
        if rk.rank == 0:
            res = headline(main)
            if args.dump_outputs:
                dump_ipdae_outputs(args.dump_outputs, main["host_packed"], main["host_out"], B, s_stride, p_cap)
            print(json.dumps(res), flush=True)
        return

    res_by_mode = {}
    for mode in modes:
        cd, _, _ = build_codec(rk, mode, args.octree_mode)
        res_by_mode[mode] = measure(cd, with_files=(not args.no_files) and mode == args.matmul,
                                    keep_for_compare=mode in (args.matmul, "f32") and "f32" in modes and args.matmul != "f32",
                                    rank_tag="host" if mode == args.matmul else None)   # the leg whose per-rank times go into the line
        del cd
        torch.cuda.empty_cache()
    # the same clouds in the OTHER octree mode, default arithmetic: "reference" reproduces octree_np.decode as written (<= 8 distinct
    # centres per cloud), "full" is the level-by-level decode under which the codec actually reconstructs the cloud
    other_mode = None if args.one_mode else ("full" if args.octree_mode == "reference" else "reference")
    other = None
    if other_mode:
        cd, _, _ = build_codec(rk, args.matmul, other_mode)
        other = measure(cd)
        del cd
        torch.cuda.empty_cache()

    main = res_by_mode[args.matmul]
    summ = rk.summaries([main["bits"], B * N_POINTS, main["psnr_sum"], main["chamfer_sum"], B, main["dt_host"]])
    if rk.rank == 0:
        rf, per_step_ms, tfl = roofline_of(main["stages"], args.steps, P, args.matmul, B)
        res = headline(main)
        res.update({
            "value_resident": rk.world * pts / main["dt_res"], "ms_per_step_resident": 1e3 * main["dt_res"] / args.steps,
            "resident_cdf_reuse": {"value": rk.world * pts / main["dt_res_reuse"], "ms_per_step": 1e3 * main["dt_res_reuse"] / args.steps,
                                   "decoded_equals_recompute": main["reuse_equals_recompute"],
                                   "note": "resident pipeline only: decompress takes the integer CDF of the Compressed object it is handed instead "
                                           "of running the probability model a second time; `value` (from bytes) always recomputes"} if "dt_res_reuse" in main else None,
            "host_window_checks": {k: main[k] for k in ("host_equals_resident", "host_bytes_equal_resident", "d2h_bytes_per_step")},
            "roofline": rf,
            "stage_ms_per_step": {k: round(v, 4) for k, v in sorted(per_step_ms.items(), key=lambda kv: -kv[1])},
            "mfma_stage_tflops": tfl,
            "bpp": summ["bpp"], "d1_psnr_db": summ["d1_psnr_db"], "chamfer": summ["chamfer"], "summary_files": summ["files"],
            "base_shapes": main["base_shapes"],
        })
        def leg_record(r, mode, octree_mode):
            """a secondary leg in full: host-to-host value + resident value, its own window checks, stage table and roofline"""
            rf2, ps2, tfl2 = roofline_of(r["stages"], args.steps, P, mode, B)
            return {"value": rk.world * pts / r["dt_host"], "unit": "points/s", "ms_per_step": 1e3 * r["dt_host"] / args.steps,
                    "window": "host-to-host (as the top-level value)",
                    "value_resident": rk.world * pts / r["dt_res"], "ms_per_step_resident": 1e3 * r["dt_res"] / args.steps,
                    "host_window_checks": {k: r[k] for k in ("host_equals_resident", "host_bytes_equal_resident", "d2h_bytes_per_step")},
                    "dtype": MODE_DTYPE[mode], "matmul": mode, "octree_mode": octree_mode, "roofline": rf2,
                    "stage_ms_per_step": {k: round(v, 4) for k, v in sorted(ps2.items(), key=lambda kv: -kv[1])},
                    "mfma_stage_tflops": tfl2,
                    "bpp": r["bits"] / (B * N_POINTS), "d1_psnr_db": r["psnr_sum"] / B, "chamfer": r["chamfer_sum"] / B,
                    "base_shapes": r["base_shapes"]}
        for mode, r in res_by_mode.items():
            if mode != args.matmul:
                res[mode] = leg_record(r, mode, args.octree_mode)
        # which leg forms every product at the reference's own width (torch fp32): the exact-fp32 MFMA.  The split modes carry 22-24 operand
        # bits and are as close to the float64 oracle as it is (tests/test_gpu_model.py), but they are emulation on narrower matrix cores.
        res["precision_matched"] = "f32" if ("f32" in res_by_mode) else None
        if args.matmul == "f32":
            res["precision_matched"] = "value (this line's top-level figures are the exact-fp32 leg)"
        if other is not None:
            rec = leg_record(other, args.matmul, other_mode)
            rec["note"] = ("the same %d clouds, octree mode '%s'" % (B, other_mode)) + (
                ": the level-by-level decode (every one of the 64 centres distinct), i.e. the mode in which the codec reconstructs the cloud; "
                "the top-level line is the reference's decode as written (octree_np.py:47-112: <= 8 distinct centres per cloud)" if other_mode == "full" else "")
            res[other_mode + "_mode"] = rec
        if "dt_files" in main:
            wf = rk.world * B * N_POINTS * main["files_steps"] / main["dt_files"]
            res["with_files"] = {"value": wf, "unit": "points/s", "ms_per_step": 1e3 * main["dt_files"] / main["files_steps"], "steps": main["files_steps"],
                                 "frac_of_value": wf / res["value"], "decoded_equals_resident": main["files_equal_resident"],
                                 "clouds_with_files_identical_to_resident": main["files_identical"], "clouds": B,
                                 "host_ms_per_step": {k_: round(v, 3) for k_, v in main["files_host_ms"].items()},
                                 "note": "the reference's window in full: the three .bin files of every cloud are written to and read back from tmpfs "
                                         "INSIDE the timed region (compress.py:139-152, decompress.py:80-91,113) by the library's host threads "
                                         "(pccx_write_streams_host / pccx_read_streams_host, csrc/hostio.hip), between the D2H of the packed streams "
                                         "and their H2D; the host work of step i runs while the GPU executes compress(i+1)"}
        if "cmp" in main and "cmp" in res_by_mode.get("f32", {}):
            res[args.matmul + "_vs_f32"] = compare_modes(main.pop("cmp"), res_by_mode["f32"].pop("cmp"), B, s_stride, p_cap, codec)
        res["cpu_baseline"] = None
        print("[bench] gpu legs done: %.3e points/s host-to-host (%.2f ms/step), %.3e resident; dominant %s %.1f TFLOP/s (%.2f of %s peak)" %
              (res["value"], res["ms_per_step"], res["value_resident"], rf["kernel"], rf["achieved"], rf["frac"], args.matmul),
              file=sys.stderr, flush=True)
        if cpu_leg_allowed(args, rk):
            try:
                res["cpu_baseline"] = cpu_baseline(args.cpu_clouds, args.cpu_budget)
                res["gpu_over_cpu"] = res["value"] / res["cpu_baseline"]["value"]
            except Exception as e:   # the GPU line must survive a broken host toolchain
                res["cpu_baseline_error"] = repr(e)
    else:
        res = None
    # configs[2], [3], [4] in the same run (every rank takes part: their timed regions hold the same barriers), then ONE line from rank 0
    if not args.no_secondary:
        sec = run_secondaries(args, rk, res)
        if res is not None:
            res["secondary"] = sec
    if res is not None:
        print(json.dumps(res), flush=True)


SECONDARY = (("pppf", "run_pppf", {"batch": 256}), ("s3dis", "run_s3dis", {"batch": 1024}), ("pppe_train", "run_pppe_train", {"graph": True}),
             ("ipdae_train", "run_ipdae_train", {}))       # the last one is not a BASELINE config: train.py's step


def run_secondaries(args, rk, headline, specs=None):
    """BASELINE configs[2] (PPPF_AE forward), [3] (room-scale blocks) and [4] (pppe training step, hipGraph) measured by the SAME command
    as the headline, each with its own roofline, stage table and -- at N = 1 -- CPU baseline (a 3 s sample each).  A leg that raises is
    reported as {"error": ...}; a leg that HANGS cannot take the headline with it: a watchdog thread prints the line as it stands
    (rank 0) and ends the process once --secondary-budget seconds have passed."""
    import copy
    import threading
    import traceback
    import torch
    out, done = {}, threading.Event()
    t_start = time.time()

    def watchdog():
        if done.wait(args.secondary_budget):
            return
        if headline is not None:
            out_ = dict(out)
            out_["error"] = "secondary workloads exceeded --secondary-budget %.0f s; the line was printed by the watchdog" % args.secondary_budget
            headline["secondary"] = out_
            print(json.dumps(headline), flush=True)
        sys.stderr.write("[bench] secondary workloads timed out on rank %d: exiting\n" % rk.rank)
        sys.stderr.flush()
        os._exit(0)
    threading.Thread(target=watchdog, daemon=True).start()
    for name, fn, over in (SECONDARY if specs is None else specs):
        a = copy.copy(args)
        vars(a).update(over)
        a.steps, a.warmup = max(5, min(args.steps, 20)), max(2, min(args.warmup, 5))
        a.cpu_budget = 2 * args.secondary_cpu_budget                # the legs take cpu_budget / 2
        t0 = time.time()
        try:
            r = globals()[fn](a, rk)
        except Exception as e:                                      # the headline must survive a broken secondary leg
            r = {"error": repr(e), "traceback": traceback.format_exc().splitlines()[-6:]}
            if rk.rank != 0:
                sys.stderr.write("[bench] rank %d: secondary %s failed: %r\n" % (rk.rank, name, e))
        if r is not None:
            r["wall_s"] = round(time.time() - t0, 2)
            out[name] = r
        if rk.gpu:
            torch.cuda.empty_cache()
        if rk.rank == 0:
            print("[bench] secondary %s done in %.1f s" % (name, time.time() - t0), file=sys.stderr, flush=True)
    done.set()
    out["wall_s"] = round(time.time() - t_start, 2)
    return out


def run_s3dis(args, rk):
    """configs[3]: room-scale clouds (0.5-1 M points, synth.room_cloud(100+i)) cut into 8192-point Morton blocks that shard
    across ranks like files (large.py); a step = compress + decompress of every block of every room owned by this rank,
    reassembled with the inverse permutation.  Total work is fixed, so scaling is strong."""
    import torch
    from pccx import codec, large, synth
    cd, _, _ = build_codec(rk, args.matmul, "reference")
    rooms = [torch.from_numpy(synth.room_cloud(100 + i)).to(rk.dev) for i in range(args.rooms)]
    n_pts = sum(int(r.shape[0]) for r in rooms)
    keep = {}

    def step(i):
        # the blocks of all rooms in common batches (large.compress_large_many): full launches instead of one short one per room
        parts, metas = large.compress_large_many(cd, rooms, seed=11, rank=rk.rank, world=rk.world, batch=args.batch)
        keep["parts"], keep["metas"] = parts, metas
        keep["out"] = large.decompress_large_many(cd, parts, metas)
    for _ in range(args.warmup):
        step(0)
    from pccx import ops
    timer = ops.StageTimer()
    ops.set_timer(timer)
    dt = timed(rk, step, args.steps, torch.cuda.synchronize)
    ops.set_timer(None)
    stages = {k_: (ms / n_, n_) for k_, (ms, n_) in timer.totals_ms().items()}
    # quality, outside the timed region: bits of this rank's blocks and their block-level D1 (a block's decoded rows are a set;
    # with world > 1 a rank holds only its own blocks' rows, so the per-room D1 is replaced by the mean over blocks)
    bits = psnr_sum = blocks = pts = 0.0
    flat = torch.cat([large.split_blocks(pc)[0] for pc in rooms])
    for ids, c in keep["parts"]:
        blocks += len(ids)
        if args.full:
            bits += float(c.bits().sum())
            psnr_sum += float(codec.d1_psnr(flat[ids], cd.decompress(c)).sum())
            pts += len(ids) * flat.shape[1]
    summ = rk.summaries([bits, pts, psnr_sum, 0.0, blocks, dt]) if args.full else None
    if rk.rank == 0:
        # the dominant kernel is the fused encoder, as in the headline workload: its launches here cover `blocks_per_launch` blocks
        # (the last one of a step fewer), so the FLOPs of a launch are taken from the mean number of patches per launch
        n_launch = max(stages[max((k_ for k_ in STAGE_FLOP if k_ in stages), key=lambda k_: stages[k_][0] * stages[k_][1])][1] // args.steps, 1)
        rf, per_step_ms, _ = roofline_of(stages, args.steps, int(blocks) * S_PATCH / n_launch, args.matmul, int(blocks) / n_launch)
        rf["note"] += f"; mean over {n_launch} launches per step of <= {args.batch} blocks x {S_PATCH} patches"
        cpu = None
        if cpu_leg_allowed(args, rk):
            try:
                from pccx import dist as pdist
                nb0 = min(int(keep["metas"][0][1]), 64)
                cpu = cpu_baseline_blocks(flat[:nb0].cpu().numpy(), [pdist.fps_start_index(11, j, N_POINTS) for j in range(nb0)], args.cpu_budget / 2)
            except Exception as e:
                cpu = {"error": repr(e)}
        return ({
            "metric": "points/sec compress+decompress, room-scale clouds in 8192-pt Morton blocks", "value": n_pts * args.steps / dt,
            "unit": "points/s", "n_gpus": rk.world, **rk.info, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": MODE_DTYPE[args.matmul], "data": "synthetic",
            "window": "resident; the block partition (Morton keys + torch.sort) and the inverse permutation are inside the step",
            "config": {"workload": f"S3DIS-like rooms (configs[3]): {args.rooms} rooms, {n_pts} points, IPDAE K=256 per 8192-pt block",
                       "sharding": f"block-sharded x{rk.world}", "matmul": args.matmul, "blocks_per_launch": args.batch},
            "roofline": rf, "stage_ms_per_step": {k_: round(v, 4) for k_, v in sorted(per_step_ms.items(), key=lambda kv: -kv[1])},
            "cpu_baseline": cpu, "gpu_over_cpu": (n_pts * args.steps / dt / cpu["value"]) if cpu and "value" in cpu else None,
            "bpp_padded_blocks": summ["bpp"] if summ else None, "d1_psnr_db_blockwise": summ["d1_psnr_db"] if summ else None,
            "blocks": int(summ["files"]) if summ else int(blocks)})
    return None


def run_pppf(args, rk):
    """configs[2]: PPPF_AE (PointNet++ encoder + FoldingNet decoder, PPPF_AE.py:114-150) forward on K=512-point patches of
    2048-pt clouds (S = N*ALPHA/K = 8 patches per cloud), the model call of the reference's patch loop."""
    import numpy as np
    import torch
    from pccx import families, ops, synth
    Kp, N = 512, 2048
    S = N * ALPHA // Kp
    model = families.PPPF_AE(K=Kp, k=Kp // ALPHA, d=16, L=7)
    model.load_state_dict(seeded_state_dict(model, 21))
    for k_, v in model.state_dict().items():
        if k_.endswith("running_var"):
            v.fill_(1.0)
    model.pack(rk.dev)
    B = args.batch
    clouds = torch.from_numpy(np.stack([synth.cad_cloud(300 + rk.rank + rk.world * i, N) for i in range(min(B, 32))])).to(rk.dev)
    nbase = clouds.shape[0]
    clouds = clouds.repeat((B + nbase - 1) // nbase, 1, 1)[:B].contiguous()
    # every cloud distinct: copy c of the base shapes is turned by c * 2 pi / 37 about the vertical axis through the cube's centre
    ang = (torch.arange(B, device=rk.dev) // nbase).to(torch.float32) * (2.0 * 3.141592653589793 / 37.0)
    ca, sa_ = torch.cos(ang)[:, None], torch.sin(ang)[:, None]
    x0, y0 = clouds[..., 0] - 0.5, clouds[..., 1] - 0.5
    clouds = torch.stack([ca * x0 - sa_ * y0 + 0.5, sa_ * x0 + ca * y0 + 0.5, clouds[..., 2]], dim=-1).contiguous()
    cent = ops.index_points(clouds, ops.farthest_point_sample_batch(clouds, S, torch.zeros(B, dtype=torch.int32)))
    patches = ops.knn_points(cent, clouds, Kp, patch_scale=float((N / N0) ** (1 / 3))).knn.view(B * S, Kp, 3).contiguous()
    keep = {}
    for _ in range(args.warmup):
        model(patches)
    dt = timed(rk, lambda i: keep.__setitem__("o", model(patches)), args.steps, torch.cuda.synchronize)
    # the stage table comes from passes of their own AFTER the timed ones (HIP events around every stage, not inside the timed region)
    stage_ms = None
    if args.full:
        timer = ops.StageTimer()
        ops.set_timer(timer)
        for _ in range(args.steps):
            model(patches)
        ops.set_timer(None)
        stage_ms = {k_: round(ms / args.steps, 4) for k_, (ms, n_) in sorted(timer.totals_ms().items(), key=lambda kv: -kv[1][0])}
    flop_ref = families.pppf_flops_per_patch(model)                       # the reference's count: stacks on every grouped row
    flop = families.pppf_flops_per_patch(model, executed=True, n_points=Kp)  # what runs here: stacks on the source rows only
    if rk.rank == 0:
        cpu = None
        if cpu_leg_allowed(args, rk):
            try:
                cpu = cpu_baseline_pppf(model.state_dict(), patches[:min(patches.shape[0], 256)], Kp, args.cpu_budget / 2)
            except Exception as e:
                cpu = {"error": repr(e)}
        # agreement of the quoted arithmetic with the other two on the TIMED patches (the headline's f16x2_vs_f32, for this family): one
        # forward each, outside every timed region
        agree = None
        if args.full and args.matmul == "f16x2" and "h2" in (model._packed or {}):
            import pccx as _pccx
            try:
                got = [t.clone() for t in keep["o"]]
                agree = {}
                for other in ("bf16x3", "f32"):
                    _pccx.DEFAULT_MATMUL = other
                    ref = model(patches)
                    same = (got[2] == ref[2]).all(dim=1)
                    agree[other] = {"patches": int(got[2].shape[0]), "symbols": int(got[2].numel()), "symbols_differing": int((got[2] != ref[2]).sum()),
                                    "max_latent_diff": float((got[1] - ref[1]).abs().max()),
                                    "max_recon_diff_where_symbols_agree": float((got[0] - ref[0])[same].abs().max()) if bool(same.any()) else None}
                    del ref
                agree["note"] = ("rec / latent / symbols of ONE forward on the timed patches in f16x2 against the same forward in bf16x3 and in exact "
                                 "fp32 (generic layers); tests/test_families.py holds all three to the reference fixture at the same tolerances")
            except Exception as e:
                agree = {"error": repr(e)}
            finally:
                _pccx.DEFAULT_MATMUL = args.matmul
        rf = None
        # the arithmetic that RUNS: the planes stacks (set abstraction, FoldingNet chains) take the flag's arithmetic -- f16x2 since round 5 --
        # while the four small Linears on one row per patch (latent projections, the folding MLPs' per-patch parts) stay bf16x3
        eff_matmul = args.matmul if ("h2" in (model._packed or {}) or args.matmul != "f16x2") else "bf16x3"
        if flop:
            ach = flop * B * S * args.steps / dt / 1e12
            peak = F32_MATRIX_PEAK_TFLOPS if eff_matmul == "f32" else BF16_DENSE_PEAK_TFLOPS / (H2_PRODUCTS if eff_matmul == "f16x2" else B3_PRODUCTS)
            rf = {"kernel": "PPPF_AE forward (all layers)", "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                  "frac": ach / peak, "traffic": None, "flop_per_patch": flop, "arithmetic": eff_matmul,
                  # for continuity with the rounds that ran these layers in bf16x3 (round 4: 0.248 of 419.5): the same achieved rate over that peak
                  "frac_of_bf16x3_peak": ach / (BF16_DENSE_PEAK_TFLOPS / B3_PRODUCTS),
                  "reference_flop_per_patch": flop_ref, "reference_counted_tflops": flop_ref * B * S * args.steps / dt / 1e12,
                  "note": "whole-forward wall time over the FLOPs this implementation EXECUTES: PointnetSAModule gathers un-centred rows "
                          "(pointnet_sa_module.py:73-85), so its Conv-BN-ReLU stacks run on the N source rows once and the groups take their maxima "
                          "from that (pccx_gather_max) -- bit-identical outputs for 1/%.1f of the reference's matrix work "
                          "(reference_flop_per_patch); the forward is no longer matrix-bound: gather-max (LDS), the FoldingNet layers and "
                          "FPS / ball query share it (DESIGN.md section 7)" % (flop_ref / flop)}
        return ({
            "metric": "points/sec PPPF_AE forward (encode+decode) on K=512 patches", "value": rk.world * B * S * Kp * args.steps / dt,
            "unit": "points/s", "n_gpus": rk.world, **rk.info, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": MODE_DTYPE[eff_matmul], "data": "synthetic",
            "config": {"workload": "PPPF_AE K=512 d=16 (configs[2]): 2048-pt ShapeNet-shaped clouds, 8 patches per cloud", "matmul": eff_matmul,
                       "matmul_requested": args.matmul,
                       "clouds_per_gpu_per_step": B, "patches_per_step": B * S, "weights": "seeded random"},
            "roofline": rf, "stage_ms_per_step": stage_ms, "f16x2_vs_other_arithmetics": agree, "cpu_baseline": cpu,
            "gpu_over_cpu": (rk.world * B * S * Kp * args.steps / dt / cpu["value"]) if cpu and "value" in cpu else None})
    return None


def run_pppe_train(args, rk):
    """configs[4]: one optimisation step of the pppe fast path per "step" (forward in train mode, Chamfer rate-distortion
    loss as the script builds it, backward, clip, Adam; data-parallel gradient all-reduce over RCCL when N > 1).  The line is
    quoted at --train-batch clouds per GPU (4 = train_pppe_pcd_ae.py's batch_size); `batch_sweep` repeats the measurement at
    batches 4 / 16 / 64 (clouds/s and patches/s: a cloud is 512 first-level patches per set-abstraction branch)."""
    import numpy as np
    import torch
    from pccx import families, synth, train

    def run(Bt, steps, warmup, autocast=None):
        autocast = args.autocast if autocast is None else autocast
        model = families.PointCloudAE(64, 16, N_POINTS)
        model.load_state_dict(seeded_state_dict(model, 32))
        for k, v in model.state_dict().items():                  # sane BatchNorm statistics
            if k.endswith("running_var"):
                v.fill_(1.0)
        sd0 = {k_: v.detach().clone() for k_, v in model.state_dict().items()}          # the CPU leg starts from the same weights
        model = model.to(rk.dev)
        opt = train.Adam(model.parameters(), lr=1e-3)
        x = torch.from_numpy(np.stack([synth.cad_cloud(900 + rk.rank * Bt + i, N_POINTS) for i in range(Bt)])).to(rk.dev)
        rng = np.random.default_rng(rk.rank)
        starts = [[rng.integers(0, N_POINTS, Bt), rng.integers(0, N_POINTS, Bt)], rng.integers(0, 512, Bt), rng.integers(0, 128, Bt)]
        keep = {}
        kw = dict(lam=1e-3, data_parallel=rk.grouped)
        if autocast:
            kw["autocast"] = True
        extra = {}
        if args.graph:
            pre = not args.no_prefetch
            gstep = train.GraphedTrainStep(model, opt, x, starts, lam=1e-3, autocast=autocast, warmup=max(warmup, 1),
                                           data_parallel=rk.grouped, prefetch=pre)     # N > 1: two graphs cut at the gradient all-reduce
            if pre:
                # the loop of train_pppe_pcd_ae.py:184-226 software-pipelined: the FPS / kNN tables of batch i+1 (functions of the
                # coordinates and the start indices only) are computed on a side stream while the captured step i runs
                def one(i):
                    keep["o"] = gstep(sync=False, next_batch=(x, starts))
                gstep.prefetch(x, starts)
                one(0)
                torch.cuda.synchronize()
                dt = timed(rk, one, steps, torch.cuda.synchronize)
                gstep(sync=False)                                          # consume the batch the last iteration queued
                # the pieces by themselves (HIP events): selection on the side stream, and copy + replay with the tables ready
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                sel_ms = rep_ms = lat_ms = 0.0
                nrep = max(3, min(steps, 10)) if args.full else 0
                for _ in range(nrep):
                    torch.cuda.synchronize()
                    with torch.cuda.stream(gstep._side):
                        ev[0].record(gstep._side)
                    gstep.prefetch(x, starts)
                    with torch.cuda.stream(gstep._side):
                        ev[1].record(gstep._side)
                    torch.cuda.synchronize()
                    ev[2].record()
                    gstep(sync=False)
                    ev[3].record()
                    torch.cuda.synchronize()
                    sel_ms += ev[0].elapsed_time(ev[1])
                    rep_ms += ev[2].elapsed_time(ev[3])
                    t0 = time.perf_counter()                               # one isolated step, nothing in flight before or after it
                    gstep(x, starts, sync=False)
                    torch.cuda.synchronize()
                    lat_ms += 1e3 * (time.perf_counter() - t0)
                extra = {"stage_ms_per_step": {"graph_replay (forward + backward + clip + Adam, one hipGraph)": round(rep_ms / nrep, 4),
                                               "selection (FPS + kNN tables of the next batch, side stream, overlapped)": round(sel_ms / nrep, 4)},
                         "latency_ms_isolated_step": round(lat_ms / nrep, 4)} if nrep else {}
                extra["pipelining"] = "selection of batch i+1 on a side stream under the replay of step i (GraphedTrainStep(prefetch=True))"
            else:
                dt = timed(rk, lambda i: keep.__setitem__("o", gstep(sync=False)), steps, torch.cuda.synchronize)
            keep["o"] = tuple(float(t) for t in keep["o"])
        else:
            for _ in range(warmup):
                train.train_step(model, opt, x, starts, **kw)
            dt = timed(rk, lambda i: keep.__setitem__("o", train.train_step(model, opt, x, starts, **kw)), steps, torch.cuda.synchronize)
        keep["extra"] = extra
        return dt, keep["o"][0], model, sd0, x, starts, keep["extra"]

    Bt = args.train_batch
    dt, loss, model, sd0, x, starts, extra = run(Bt, args.steps, args.warmup)
    sweep = {}
    if args.full and not args.one_mode:
        for b_ in (4, 16, 64):
            if b_ == Bt:
                sweep[str(b_)] = {"clouds_per_s": rk.world * Bt * args.steps / dt, "ms_per_step": 1e3 * dt / args.steps}
                continue
            torch.cuda.empty_cache()
            st_ = max(3, args.steps // 2)
            dtb, _, _, _, _, _, _ = run(b_, st_, max(args.warmup, 1))
            sweep[str(b_)] = {"clouds_per_s": rk.world * b_ * st_ / dtb, "ms_per_step": 1e3 * dtb / st_}
        for v in sweep.values():
            v["patches_per_s"] = v["clouds_per_s"] * 512
    other = None
    if args.full and not args.one_mode:
        # the step in the OTHER arithmetic beside the quoted one (bf16 autocast <-> fp32): the reference's CUDA branch is fp16 autocast with a
        # GradScaler (three more mantissa bits than bf16), so the fp32 step is the conservative figure to read the bf16 one against
        torch.cuda.empty_cache()
        st_ = max(3, args.steps // 2)
        dto, losso, _, _, _, _, _ = run(Bt, st_, max(args.warmup, 1), autocast=not args.autocast)
        other = {"dtype": "f32" if args.autocast else "bf16 autocast", "clouds_per_s": rk.world * Bt * st_ / dto, "ms_per_step": 1e3 * dto / st_, "loss": losso}
    if rk.rank == 0:
        cpu = None
        if cpu_leg_allowed(args, rk):
            try:
                cpu = cpu_baseline_pppe_train(sd0, x, starts, args.cpu_budget / 2)
            except Exception as e:
                cpu = {"error": repr(e)}
        flop = train.step_flops(model, Bt) if hasattr(train, "step_flops") else None
        rf = None
        if flop:
            ach = flop * args.steps / dt / 1e12
            peak = BF16_DENSE_PEAK_TFLOPS if args.autocast else F32_MATRIX_PEAK_TFLOPS     # the peak of the arithmetic that RUNS
            rf = {"kernel": "training step (forward + backward GEMMs)", "bound": "mfma", "achieved": ach, "peak": peak,
                  "unit": "TFLOP/s", "frac": ach / peak, "traffic": None, "flop_per_step": flop,
                  "arithmetic": "bf16 operands on the bf16 matrix cores, fp32 accumulate (autocast)" if args.autocast else "f32",
                  "frac_of_f32_matrix_peak": ach / F32_MATRIX_PEAK_TFLOPS,
                  "note": "whole-step wall time over the algorithmic GEMM FLOPs (3x forward): a chain of ~200 small launches at batch 4 -- "
                          "latency-bound, not arithmetic-bound (DESIGN.md: training step); the batch sweep shows the rate a fuller chip reaches"}
        return ({
            "metric": "clouds/sec, pppe fast-path training step (forward+backward+Adam)", "value": rk.world * Bt * args.steps / dt,
            "unit": "clouds/s", "points_per_s": rk.world * Bt * N_POINTS * args.steps / dt, "patches_per_s": rk.world * Bt * 512 * args.steps / dt,
            "n_gpus": rk.world, **rk.info, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16 autocast (the reference's CUDA branch is fp16 autocast + GradScaler, train_pppe_pcd_ae.py:193,280; BASELINE configs[4] names bf16)"
                     if args.autocast else "f32", "data": "synthetic",
            "config": {"workload": f"pppe PointCloudAE training step (configs[4]), batch {Bt} x 8192 points per GPU",
                       "parallelism": f"dp{rk.world}", "weights": "seeded random",
                       "launch": (("one hipGraph replay per step" if not rk.grouped else "two hipGraph replays per step around the RCCL gradient all-reduce") +
                                  ("" if args.no_prefetch else "; FPS / kNN tables of the next batch on a side stream"))
                                 if args.graph else "eager" + (" (gradient all-reduce overlapped with backward)" if rk.grouped else "")},
            "batch_sweep": sweep or None, "other_arithmetic": other, **extra,
            "roofline": rf, "cpu_baseline": cpu,
            "gpu_over_cpu": (rk.world * Bt * args.steps / dt / cpu["value"]) if cpu and "value" in cpu else None, "loss": loss})
    return None


def run_ipdae_train(args, rk):
    """The IPDAE trainer's step (train.py:156-256, --model AE) at the reference's own shape: batch 1 (train.py:40: "must be 1"), 8192
    points, K = 256 -> 64 patches of 256 points, d = 16, L = 7; one optimisation step per "step", captured as one hipGraph (selection
    included) and, beside it, eager.  Not a BASELINE config (north_star names train.py's CLI); N > 1 runs independent replicas -- the
    reference has no data-parallel form of this loop and none is invented."""
    import numpy as np
    import torch
    from pccx import models, synth, train_ipdae
    K, k, d, L = 256, 128, 16, 7
    n_clouds = 8
    autocast = bool(args.autocast) if getattr(args, "autocast_given", False) else False    # fp32 is what the parity tests pin; --autocast = bf16
    x = torch.from_numpy(np.stack([synth.cad_cloud(1200 + rk.rank * n_clouds + i, N_POINTS) for i in range(n_clouds)])).to(rk.dev)
    rng = np.random.default_rng(rk.rank)
    starts = rng.integers(0, N_POINTS, (n_clouds, 1))

    def fresh():
        ae, prob = models.AE(K=K, k=k, d=d, L=L), models.ConditionalProbabilityModel(L, d)
        ae.load_state_dict(seeded_state_dict(ae, 3)), prob.load_state_dict(seeded_state_dict(prob, 4, gain=2.0))
        return train_ipdae.IpdaeTrainer(ae.to(rk.dev), prob.to(rk.dev), N=N_POINTS, K=K, lr=5e-4, lamda=1e-6, rate_loss_enable_step=0,
                                        autocast=autocast)
    keep = {}
    dt_e = None
    if args.full:
        tr = fresh()
        for i in range(max(args.warmup, 1)):
            tr.step(x[i % n_clouds:i % n_clouds + 1], starts[i % n_clouds])
        dt_e = timed(rk, lambda i: keep.__setitem__("e", tr.step(x[i % n_clouds:i % n_clouds + 1], starts[i % n_clouds])), args.steps,
                     torch.cuda.synchronize)
    tg = fresh()
    gstep = tg.graphed(x[:1], starts[0], warmup=max(args.warmup, 1))
    dstarts = torch.from_numpy(starts.astype(np.int32)).to(rk.dev)                       # the start indices live on the device, like the clouds
    dt = timed(rk, lambda i: keep.__setitem__("g", gstep(x[i % n_clouds:i % n_clouds + 1], dstarts[i % n_clouds], sync=False)), args.steps,
               torch.cuda.synchronize)
    out = {k_: float(v) for k_, v in keep["g"].items()}
    if rk.rank != 0:
        return None
    cpu = None
    if cpu_leg_allowed(args, rk):
        try:
            cpu = cpu_baseline_ipdae_train((K, k, d, L), x[:1], starts[0], args.cpu_budget / 2)
        except Exception as e:
            cpu = {"error": repr(e)}
    P, rows_sa = 64, 64 * K * 16
    macs = (rows_sa * (3 * 32 + 32 * 64 + 64 * 128) + P * K * (131 * 128 + 128 * 256 + 256 * 512 + 512 * d)
            + P * (d * 256 + 256 * 1024 + 1024 * k * 128) + P * k * ((128 + d) * 128 + 128 * 64 + 64 * 32 + 32 * 3)
            + 64 * (3 * 64 + 64 * 128 + 128 * 256 + 259 * 512 + 512 * 512 + 512 * d * L))
    flop = 3 * 2 * macs
    ach = flop * args.steps / dt / 1e12
    peak = BF16_DENSE_PEAK_TFLOPS if autocast else F32_MATRIX_PEAK_TFLOPS
    return {"metric": "clouds/sec, IPDAE training step (train.py --model AE: forward+backward+Adam)", "value": rk.world * args.steps / dt,
            "unit": "clouds/s", "patches_per_s": rk.world * 64 * args.steps / dt, "n_gpus": rk.world, **rk.info, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "ms_per_step_eager": 1e3 * dt_e / args.steps if dt_e else None, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16 autocast" if autocast else "f32", "data": "synthetic",
            "config": {"workload": "IPDAE training step (train.py:156-256, --model AE), batch 1 x 8192 points, K=256 (64 patches), d=16, L=7",
                       "parallelism": f"{rk.world} independent replica(s)", "weights": "seeded random",
                       "launch": "one hipGraph replay per step, selection (normalize, FPS, octree, kNN) inside it"},
            "roofline": {"kernel": "training step (forward + backward GEMMs)", "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                         "frac": ach / peak, "traffic": None, "flop_per_step": flop,
                         "note": "whole-step wall time over the algorithmic GEMM FLOPs (3x forward): ~400 small launches on 64 patches -- "
                                 "latency-bound, not arithmetic-bound"},
            "cpu_baseline": cpu, "gpu_over_cpu": (rk.world * args.steps / dt / cpu["value"]) if cpu and "value" in cpu else None, **out}


def _printer(fn):
    def run(args, rk):
        res = fn(args, rk)
        if res is not None:
            print(json.dumps(res), flush=True)
    return run


bench_s3dis, bench_pppf, bench_pppe_train, bench_ipdae_train = _printer(run_s3dis), _printer(run_pppf), _printer(run_pppe_train), _printer(run_ipdae_train)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1024, help="clouds per GPU per step")
    ap.add_argument("--octree-mode", default="reference", choices=["reference", "full"])
    ap.add_argument("--matmul", default=None, choices=["f32", "bf16x3", "f16x2"],
                    help="how the three transforms form their fp32 products (pccx.DEFAULT_MATMUL when omitted); the other mode is "
                         "measured beside it (resident leg) unless --one-mode")
    ap.add_argument("--one-mode", action="store_true", help="skip the second arithmetic mode")
    ap.add_argument("--cpu-clouds", type=int, default=64, help="max clouds in the CPU baseline sample (0 = skip)")
    ap.add_argument("--cpu-budget", type=float, default=24.0, help="seconds of CPU work for the baseline sample (2/3 all cores, 1/3 one thread)")
    ap.add_argument("--workload", default="ipdae", choices=["ipdae", "s3dis", "pppf", "pppe-train", "ipdae-train", "launch-check"],
                    help="ipdae = the headline compress+decompress path (default); s3dis = configs[3] room-scale clouds in Morton "
                         "blocks; pppf = configs[2] PPPF_AE forward; pppe-train = the training step of configs[4]; "
                         "launch-check = no GPU work, exercises the N-rank launch and the summary all-gather")
    ap.add_argument("--rooms", type=int, default=8, help="s3dis: number of rooms")
    ap.add_argument("--train-batch", type=int, default=4, help="pppe-train: clouds per GPU per step (train_pppe_pcd_ae.py: batch_size 4); "
                                                                 "batches 4 / 16 / 64 are swept beside it unless --one-mode")
    ap.add_argument("--autocast", action="store_true", default=None,
                    help="pppe-train: the bf16 autocast branch of train_pppe_pcd_ae.py:193-217 (the default for this workload: BASELINE "
                         "configs[4] names bf16)")
    ap.add_argument("--fp32", action="store_true", help="pppe-train: the fp32 step instead of the bf16 autocast one")
    ap.add_argument("--graph", action="store_true", help="pppe-train: capture the step once as a hipGraph and replay it (N > 1: two graphs around the gradient all-reduce)")
    ap.add_argument("--no-prefetch", action="store_true",
                    help="pppe-train --graph: keep FPS / kNN inside the captured step (the round-4 form) instead of computing the next batch's tables on a side stream")
    ap.add_argument("--with-files", action="store_true", help="(default since round 5; kept for old command lines)")
    ap.add_argument("--no-files", action="store_true",
                    help="ipdae: skip the leg with the three .bin files of every cloud written to / read from tmpfs inside the window")
    ap.add_argument("--no-secondary", action="store_true",
                    help="ipdae --full: skip the secondary block (configs[2] PPPF forward, [3] room-scale blocks, [4] training step) of the line")
    ap.add_argument("--secondary-budget", type=float, default=300.0, help="seconds after which a hung secondary leg is abandoned (the line is still printed)")
    ap.add_argument("--secondary-cpu-budget", type=float, default=3.0, help="seconds of CPU work per secondary workload's cpu_baseline")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (production); gloo only to rehearse the N>1 path on one GPU / on CPU")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: other arithmetics and octree mode, resident leg, stage tables and rooflines, "
                         "with_files, agreement checks, CPU baselines, the secondary workloads (a plain run times the headline leg only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="ipdae: write what the last timed step computed (a fixed sample of clouds) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.dump_outputs and args.workload != "ipdae":
        ap.error("--dump-outputs is implemented for --workload ipdae (the headline) only")

    from pccx import launch
    if args.gpus > 1 and not launch.launched_by_torchrun_or_us():
        # Start the N rank processes ourselves.  The parent stays GPU-free: it imports neither torch nor anything that could
        # initialise HIP (on this torch, torch.cuda.device_count() falls back to hipGetDeviceCount when amdsmi is not usable, and
        # fork+exec from a GPU-initialised process is refused on this pool).  Whether N GPUs exist is each CHILD's check
        # (Ranks.__init__): a rank whose LOCAL_RANK has no device exits non-zero and spawn_ranks reports that code.
        if os.environ.get("PCCX_ASSERT_PARENT_GPU_FREE"):      # tests/test_sharding_gloo.py: prove the claim above
            bad = [m for m in ("torch", "torch.cuda", "pccx._lib") if m in sys.modules]
            if bad:
                raise SystemExit("bench.py launcher parent imported " + ", ".join(bad))
            print("[bench] launcher parent is GPU-free (no torch import)", file=sys.stderr, flush=True)
        sys.exit(launch.spawn_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus))

    args.autocast_given = args.autocast is not None
    args.autocast = not args.fp32 if args.autocast is None else bool(args.autocast)
    # NUMA placement of this rank's host side, from sysfs, BEFORE anything touches the GPU (pccx/launch.py)
    _, local_, _ = launch.rank_env()
    args.numa = launch.bind_rank_to_gpu_numa(local_) if args.workload != "launch-check" else None
    import pccx
    if args.matmul is None:
        args.matmul = pccx.DEFAULT_MATMUL
    pccx.DEFAULT_MATMUL = args.matmul            # the generic layers of the secondary workloads follow the flag too
    rk = Ranks(args)
    if rk.world != args.gpus and rk.rank == 0:
        print(f"[bench] note: WORLD_SIZE={rk.world} from the launcher overrides --gpus {args.gpus}", file=sys.stderr)
    try:
        {"ipdae": bench_ipdae, "s3dis": bench_s3dis, "pppf": bench_pppf, "pppe-train": bench_pppe_train,
         "ipdae-train": bench_ipdae_train, "launch-check": bench_launch_check}[args.workload](args, rk)
    finally:
        rk.close()


if __name__ == "__main__":
    main()
