"""CPU: the host side of the block-parallel centre selection -- ops.fps_block_plan (the arithmetic of pccx_fps_blocks), the Codec
arguments centres / fps_block, compress.py's two flags and the fake kernel of torch.ops.pccx.fps_blocks.  Nothing here touches a GPU."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from pccx import _lib, codec, models, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "point-cloud-compression_amd", "cli")

PLANS = [(4099, 37, 1024), (32763, 33, 16384), (132096, 1032, 8192), (2048, 16, 2048), (2049, 16, 2048), (8192, 64, 2048), (65536, 512, 4096),
         (262144, 2048, 8192), (1048576, 8192, 16384), (1048576, 8192, 4096), (1000003, 7812, 8191), (16385, 2, 16384), (3000, 23, 1024)]


@pytest.mark.parametrize("N,npoint,block", PLANS)
def test_fps_block_plan(N, npoint, block):
    P, lo, o = ops.fps_block_plan(N, npoint, block)
    assert P == -(-N // block) and len(lo) == len(o) == P + 1
    assert lo[0] == 0 and o[0] == 0 and lo[-1] == N and o[-1] == npoint
    sizes = [b - a for a, b in zip(lo, lo[1:])]
    quotas = [b - a for a, b in zip(o, o[1:])]
    assert all(s > 0 for s in sizes) and all(q >= 1 for q in quotas)                 # monotone offsets, no block without a centre
    assert max(sizes) - min(sizes) <= 1 and max(quotas) - min(quotas) <= 1
    assert max(sizes) <= block and max(quotas) <= min(sizes)
    assert lo == [j * N // P for j in range(P + 1)] and o == [j * npoint // P for j in range(P + 1)]


def test_fps_block_plan_named_shapes():
    assert ops.fps_block_plan(4099, 37, 1024) == (5, [0, 819, 1639, 2459, 3279, 4099], [0, 7, 14, 22, 29, 37])
    assert ops.fps_block_plan(32763, 33, 16384) == (2, [0, 16381, 32763], [0, 16, 33])
    P, lo, o = ops.fps_block_plan(132096, 1032, 8192)
    assert P == 17 and {b - a for a, b in zip(lo, lo[1:])} == {7770, 7771} and {b - a for a, b in zip(o, o[1:])} == {60, 61}


@pytest.mark.parametrize("block", [0, 1023, 16385, -8192, 8192.0, "8192", None, True])
def test_fps_block_plan_refuses_a_block_out_of_range(block):
    with pytest.raises(ValueError, match="fps_block"):
        ops.fps_block_plan(65536, 512, block)


def test_fps_block_plan_refuses_what_the_kernel_refuses():
    with pytest.raises(ValueError, match="centre"):
        ops.fps_block_plan(4096, 3, 1024)                     # 4 blocks, 3 centres: a block without one
    with pytest.raises(ValueError, match="centre"):
        ops.fps_block_plan(2050, 2050, 1024)                  # 3 blocks of 683 or 684 points, one of them asked for 684 of its 683


def _nets():
    return models.AE(64, 32, 8, 5), models.ConditionalProbabilityModel(5, 8)      # unpacked models: nothing here may reach a kernel


def test_codec_refuses_bad_centres_and_fps_block():
    ae, prob = _nets()
    with pytest.raises(ValueError, match="centres"):
        codec.Codec(ae, prob, K=64, centres="grid")
    for bad in (1023, 16385, 0, 4096.0, "4096", None, True):
        with pytest.raises(ValueError, match="fps_block"):
            codec.Codec(ae, prob, K=64, centres="blocks", fps_block=bad)
        with pytest.raises(ValueError, match="fps_block"):
            codec.Codec(ae, prob, K=64, fps_block=bad)          # checked whatever the choice of centres
    cd = codec.Codec(ae, prob, K=64)
    assert (cd.centres, cd.fps_block) == ("fps", 8192)         # the default stays the exact sampling
    cd = codec.Codec(ae, prob, K=64, octree_mode="full", centres="blocks", fps_block=1024)
    assert (cd.centres, cd.fps_block) == ("blocks", 1024)


def test_compress_help_lists_both_flags_and_decompress_has_neither():
    run = lambda tool: subprocess.run([sys.executable, os.path.join(CLI, tool), "--help"], capture_output=True, text=True, timeout=300)
    r = run("compress.py")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--centres {fps,blocks}" in r.stdout and "--fps-block N" in r.stdout
    r = run("decompress.py")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--centres" not in r.stdout and "--fps-block" not in r.stdout


def test_fake_kernel_shape_and_registration():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from pccx import torch_ops
    assert "fps_blocks" in torch_ops.OPS and "fps" in torch_ops.OPS
    with FakeTensorMode():
        xyz = torch.empty(3, 40000, 3, device="cuda")
        start = torch.empty(3, dtype=torch.int64, device="cuda")
        out = torch.ops.pccx.fps_blocks(xyz, 310, start, 4096)
        assert tuple(out.shape) == (3, 310) and out.dtype == torch.int64
        assert tuple(torch.ops.pccx.fps_blocks(xyz, 311, start).shape) == (3, 311)          # block defaults to 8192


def test_abi_signature():
    C = ctypes
    P, i = C.c_void_p, C.c_int
    assert _lib.signatures()["pccx_fps_blocks"] == (i, [P, i, i, P, i, i, P, P, P])
