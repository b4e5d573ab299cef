"""No GPU: the host side of whole-room clouds -- the rule that picks the workgroups per cloud of the cooperative FPS, Codec's
max_centres and its refusals on meta tensors, and the new entry points in pccx.h and in the cross-compiled library."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ref_model
from pccx import _lib, build, codec, models, ops


@pytest.mark.parametrize("N", [1, 1000, 16384, 16385, 40000, 65536, 131072, 262144, 524288, 1048576])
@pytest.mark.parametrize("B", [1, 2, 7, 64, 300])
@pytest.mark.parametrize("cus", [256, 304, 64])
def test_fps_coop_workgroups(N, B, cus):
    least = -(-N // 16384)
    G = ops.fps_coop_workgroups(N, B, cus)
    assert least <= G <= min(64, cus)
    assert -(-N // (1024 * G)) <= 16                      # points per thread
    if B * G > cus:                                       # only where even the least G does not fit: the caller splits the batch
        assert G == least and cus // G >= 1
    if B * least * 2 <= cus:
        assert G == min(2 * least, 64, cus)               # the stated rule: twice the least wherever the batch stays resident


def test_fps_coop_workgroups_refuses_what_cannot_run():
    with pytest.raises(ValueError, match="1048577 points needs 65"):
        ops.fps_coop_workgroups(1048577, 1, 256)
    with pytest.raises(ValueError):
        ops.fps_coop_workgroups(16384 * 9, 1, 8)          # 9 workgroups on 8 compute units
    with pytest.raises(ValueError):
        ops.fps_coop_workgroups(0, 1, 256)


def test_fps_auto_rule():
    """cooperative above 1024 samples; in pccx_fps's global-memory range (N > 16384) for batches resident in one launch; else pccx_fps"""
    auto = ops.fps_auto_workgroups
    assert auto(8192, 64, 1024, 256) is None and auto(16384, 1024, 1, 256) is None
    assert auto(16385, 64, 1, 256) == 4 and auto(65536, 512, 1, 256) == 8 and auto(131072, 1024, 1, 256) == 16
    assert auto(32768, 64, 64, 256) == 4                   # 64 clouds x 4 workgroups: resident
    assert auto(32768, 64, 65, 256) == 3 and auto(32768, 64, 128, 256) == 2
    assert auto(32768, 64, 129, 256) is None               # does not fit in one launch: stays
    assert auto(262144, 8192, 1, 256) == 32 and auto(1048576, 8192, 1, 256) == 64
    assert auto(40000, 1100, 300, 256) == 3                # above 1024 samples always, in sub-batches
    assert auto(2000000, 64, 1, 256) is None               # beyond 64 workgroups pccx_fps is all there is
    assert auto(1000, 0, 1, 256) is None and auto(1000, 8, 0, 256) is None


def _nets(K=64, d=8, L=5):
    ae = models.AE(K, K // 2, d, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, 3))
    prob = models.ConditionalProbabilityModel(L, d)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, 4))
    return ae, prob


def test_max_centres_validation():
    ae, prob = _nets()
    assert codec.OCTREE_MAX_S == 1024 and codec.OCTREE_WIDE_MAX_S == 8192
    assert codec.Codec(ae, prob, K=64).max_centres == 1024
    for ok in (1, 64, 1024, 1025, 8192):
        assert codec.Codec(ae, prob, K=64, max_centres=ok).max_centres == ok
    for bad in (0, -1, 8193, 1 << 20, 2048.0, "8192", None, True):
        with pytest.raises(ValueError, match="max_centres"):
            codec.Codec(ae, prob, K=64, max_centres=bad)


def test_refusals_name_the_limit_in_points_on_meta_tensors():
    """unpacked models and meta tensors: nothing here may reach a kernel"""
    K = 64
    ae, prob = _nets(K)
    cloud = lambda S: torch.empty(1, S * K // 2, 3, device="meta")
    with pytest.raises(ValueError, match=r"S=1025 patches.*at most 1024.*32768 points.*compress_large"):
        codec.Codec(ae, prob, K=K, octree_mode="full").compress(cloud(1025), np.array([0]))
    wide = codec.Codec(ae, prob, K=K, octree_mode="full", max_centres=8192)
    with pytest.raises(ValueError, match=r"S=8193 patches.*at most 8192.*262144 points.*compress_large"):
        wide.compress(cloud(8193), np.array([0]))
    with pytest.raises(ValueError, match=r"S=2049 patches.*at most 2048.*65536 points"):
        codec.Codec(ae, prob, K=K, octree_mode="full", max_centres=2048).compress(cloud(2049), np.array([0]))
    comp = codec.Compressed.alloc(1, 8, 8, 0, "meta")
    with pytest.raises(ValueError, match=r"decompress\(S=8193\).*at most 8192.*compress_large"):
        wide.decompress(comp, S=8193)
    with pytest.raises(ValueError, match=r"decompress\(S=1025\).*at most 1024"):
        codec.Codec(ae, prob, K=K, octree_mode="full").decompress(comp, S=1025)


NEW = {"pccx_fps_coop_workspace_bytes": (ctypes.c_size_t, 2), "pccx_fps_coop": (ctypes.c_int, 9),
       "pccx_octree_encode_wide": (ctypes.c_int, 11), "pccx_patch_groups_wide": (ctypes.c_int, 11)}


def test_header_declares_the_new_entries_and_the_library_exports_them():
    sig = _lib.signatures()
    for name, (restype, nargs) in NEW.items():
        assert name in sig, name
        assert sig[name][0] is restype and len(sig[name][1]) == nargs, name
    assert sig["pccx_fps_coop"][1][6] is ctypes.c_int                     # G
    assert sig["pccx_octree_encode_wide"] == sig["pccx_octree_encode"]    # the same arguments as the narrow forms
    assert sig["pccx_patch_groups_wide"] == sig["pccx_patch_groups"]
    lib = ctypes.CDLL(build.LIB) if os.path.exists(build.LIB) else None
    assert lib is not None, "libpccx.so has not been built"
    for name in NEW:
        assert hasattr(lib, name), name
    fn = lib.pccx_fps_coop_workspace_bytes                                # host-only: no device is touched
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]
    assert fn(0, 64) == 0 and fn(1, 0) == 16 and fn(1, 1) == 32 and fn(3, 8192) == 3 * 8194 * 8
    assert fn(2, 64) % 16 == 0 and fn(2, 64) >= 2 * 66 * 8
