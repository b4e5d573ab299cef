"""GPU: ops.crop_nearest (csrc/crop.hip) against its float32 numpy restatement, tests/crop_cases.crop_nearest_np -- torch.equal on the
crops (compared as bits: the padding is NaN) and on their indices.  Outputs and workspace are carved from arenas with 64-word guard
bands that are compared after every call."""
import functools
import os

import numpy as np
import pytest
import torch

from pccx import codec, ops, synth
from tests import crop_cases as cc
from tests.test_no_memset_nodes import CSRC, _calls

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, 0x5A5A5A5A


class Arena:
    """`words` 32-bit words between two guard bands of GUARD sentinel words"""

    def __init__(self, words, fill=None):
        self.words = int(words)
        self.dev = torch.full((self.words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        if fill is not None:
            self.body().view(torch.uint8).fill_(fill)

    def body(self):
        return self.dev[GUARD:GUARD + self.words]

    def intact(self):
        return bool((self.dev[:GUARD] == SENTINEL).all()) and bool((self.dev[GUARD + self.words:] == SENTINEL).all())


def run(clouds, cloud, seed, n, N_cap, fill=None, device_tables=False):
    """one guarded call -> (out bits (B, N_cap, 3) int32, idx (B, N_cap) int32), both on the host"""
    points, offsets, sizes = codec.pack_clouds(clouds, device="cuda")
    B = len(cloud)
    a_out, a_idx = Arena(B * N_cap * 3), Arena(B * N_cap)
    a_ws = Arena((ops._lib.load().pccx_crop_nearest_workspace_bytes(B, max(sizes)) + 3) // 4, fill)
    if device_tables:
        cloud, seed, n = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in (cloud, seed, n))
    out, idx = ops.crop_nearest(points, offsets, cloud, seed, n, N_cap, workspace=a_ws.body().view(torch.uint8), sizes=sizes,
                                out=a_out.body().view(torch.float32).view(B, N_cap, 3), out_idx=a_idx.body().view(B, N_cap))
    torch.cuda.synchronize()
    assert a_out.intact() and a_idx.intact() and a_ws.intact(), "a guard band was written"
    return out.view(torch.int32).cpu(), idx.cpu()


def want(clouds, cloud, seed, n, N_cap):
    rows = [cc.padded(clouds[c], s, k, N_cap) for c, s, k in zip(cloud, seed, n)]
    return (torch.from_numpy(np.stack([r[0] for r in rows]).view(np.int32)), torch.from_numpy(np.stack([r[1] for r in rows])))


def check(clouds, cloud, seed, n, N_cap, **kw):
    got, ref = run(clouds, cloud, seed, n, N_cap, **kw), want(clouds, cloud, seed, n, N_cap)
    assert torch.equal(got[1], ref[1]), "indices differ"
    assert torch.equal(got[0], ref[0]), "crops differ"
    return got


@functools.lru_cache(maxsize=None)
def room300k():
    return synth.room_cloud(3, 300000)


def test_smallest_clouds():
    check([np.array([[1.5, -2.0, 0.25]], dtype=np.float32)], [0], [0], [1], 1)
    check([np.array([[1.5, -2.0, 0.25]], dtype=np.float32)], [0], [0], [1], 5)
    p = cc.uniform_cloud(1, 4099)                          # no multiple of any chunk, two workgroups
    check([p], [0, 0, 0], [4098, 7, 2500], [1, 4098, 4099], 4099)
    got, _ = run([p], [0], [123], [4099], 4099)
    assert torch.equal(got[0], torch.from_numpy(p.view(np.int32)))      # a crop of the whole cloud is the cloud


def test_lattice_ties_go_to_the_lower_index():
    p, seed = cc.lattice16()
    ns = [2, 7, 8, 100, 257, 4095, 4096]
    check([p], [0] * len(ns), [seed] * len(ns), ns, 4096)


def test_duplicates_keep_the_first_indices():
    p = cc.duplicates()
    _, idx = check([p], [0, 0], [4999, 0], [100, 100], 128)
    assert idx[0, :100].tolist() == list(range(100))


def test_low_bits_only_the_last_pass_separates():
    p, seed = cc.line_low_bits()
    check([p], [0, 0], [seed, seed], [1500, 1501], 2048)


def test_high_bits_exponents_only():
    p, seed = cc.exponents()
    ns = [1, 2, 6, 7, 303, len(p) - 1, len(p)]
    check([p], [0] * len(ns), [seed] * len(ns), ns, len(p))


def test_several_clouds_in_one_store():
    clouds = [cc.uniform_cloud(2, 1), cc.uniform_cloud(3, 5000), cc.uniform_cloud(4, 70001)]
    check(clouds, [0, 2, 2, 1, 1], [0, 0, 70000, 4999, 17], [1, 700, 8192, 5000, 33], 8192)
    check(clouds, [2, 1], [65536, 0], [8000, 8], 8192, device_tables=True)


def test_many_workgroups_per_cloud():
    p = room300k()
    check([p], [0, 0], [299999, 12345], [8192, 131072], 131072)


def test_device_tables_are_clamped_where_they_are_read():
    clouds = [cc.uniform_cloud(5, 3000), cc.uniform_cloud(6, 300)]
    got = run(clouds, [0, 1, 7, -2], [-3, 999, 10, 10], [0, 5000, 0, 100000], 1024, device_tables=True)
    ref = want(clouds, [0, 1, 1, 0], [0, 299, 10, 10], [1, 300, 1, 1024], 1024)
    assert torch.equal(got[1], ref[1]) and torch.equal(got[0], ref[0])


def test_workspace_content_does_not_matter_and_calls_repeat():
    p = room300k()[:50000]
    a = check([p], [0, 0], [1, 49999], [777, 4096], 4096, fill=0xFF)
    b = run([p], [0, 0], [1, 49999], [777, 4096], 4096, fill=0x00)
    c = run([p], [0, 0], [1, 49999], [777, 4096], 4096)
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])


def test_a_captured_call_replays_on_other_tables():
    clouds = [cc.uniform_cloud(7, 20000), cc.uniform_cloud(8, 4097), room300k()[:30000]]
    points, offsets, sizes = codec.pack_clouds(clouds, device="cuda")
    B, N_cap = 4, 2048
    tables = torch.tensor([[0, 0, 0, 0], [0, 1, 2, 3], [2048, 2048, 2048, 2048]], dtype=torch.int32, device="cuda")
    ws = torch.empty(ops._lib.load().pccx_crop_nearest_workspace_bytes(B, max(sizes)), dtype=torch.uint8, device="cuda")
    out = torch.empty(B, N_cap, 3, device="cuda")
    idx = torch.empty(B, N_cap, dtype=torch.int32, device="cuda")

    def call():
        ops.crop_nearest(points, offsets, tables[0], tables[1], tables[2], N_cap, workspace=ws, sizes=sizes, out=out, out_idx=idx)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for cloud, seed, n in (([0, 1, 2, 2], [19999, 0, 7, 29999], [2048, 1, 100, 2047]), ([2, 2, 1, 0], [5, 5, 4096, 300], [33, 1500, 2048, 64]),
                           ([1, 0, 0, 1], [1, 2, 3, 4], [5, 6, 7, 8])):
        tables.copy_(torch.tensor([cloud, seed, n], dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        got = (out.view(torch.int32).cpu(), idx.cpu())
        eager = run(clouds, cloud, seed, n, N_cap)
        ref = want(clouds, cloud, seed, n, N_cap)
        assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    # no memset / memcpy node can be in the graph: the sources of the call issue none (the lint of tests/test_no_memset_nodes.py)
    for what in ("hipMemsetAsync", "hipMemset", "hipMemcpyAsync", "hipMemcpy"):
        assert _calls(os.path.join(CSRC, "crop.hip"), what) == []


def test_torch_op_equals_the_direct_path():
    from pccx import torch_ops  # noqa: F401
    clouds = [cc.uniform_cloud(9, 6000), cc.uniform_cloud(10, 513)]
    points, offsets, sizes = codec.pack_clouds(clouds, device="cuda")
    t = [torch.tensor(v, dtype=torch.int32, device="cuda") for v in ([1, 0, 0], [512, 0, 5999], [513, 100, 1024])]
    a, ai = torch.ops.pccx.crop_nearest(points, offsets, t[0], t[1], t[2], 1024, sizes)
    b, bi = ops.crop_nearest(points, offsets, t[0], t[1], t[2], 1024, return_idx=True, sizes=sizes)
    assert torch.equal(ai, bi) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    ref = want(clouds, [1, 0, 0], [512, 0, 5999], [513, 100, 1024], 1024)
    assert torch.equal(bi.cpu(), ref[1]) and torch.equal(b.view(torch.int32).cpu(), ref[0])
