"""GPU: cli/eval.py's uniformity coefficient with --search grid (calc_uc, region_of_point0).  Up to 32768 points both searches see the
same region and the same 2-NN distances, so the coefficients are EQUAL; above it only the grid route works, and it is checked against
float64 arithmetic on the same clouds."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from pccx import _lib, synth as cloud_synth
from tests import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _eval_module():
    cli = os.path.join(ROOT, "point-cloud-compression_amd", "cli")
    if cli not in sys.path:
        sys.path.insert(0, cli)
    argv = sys.argv
    sys.argv = ["eval.py"]
    try:
        return importlib.import_module("eval")
    finally:
        sys.argv = argv


def test_calc_uc_grid_equals_brute():
    ev = _eval_module()
    for i, (a, b) in enumerate(synth.uc_cases()):
        a, b = torch.from_numpy(a)[None].cuda(), torch.from_numpy(b)[None].cuda()
        assert ev.calc_uc(a, b, "grid") == ev.calc_uc(a, b, "brute") == ev.calc_uc(a, b), i


def _tie_cloud():
    """integer / 8 coordinates on a 16^3 lattice with 4096 of the points repeated, shuffled: shells of exactly tied distances around
    point 0, cut by K = 1024 in the middle of a shell"""
    g = torch.Generator().manual_seed(11)
    r = torch.arange(16, dtype=torch.float32) / 8
    p = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1).reshape(-1, 3)
    p = torch.cat([p, p[torch.randperm(4096, generator=g)]])
    return p[torch.randperm(p.shape[0], generator=g)][None].contiguous().cuda()


@pytest.mark.parametrize("chunk", [3000, 2048])       # 8192 points: three chunks, one pass; four chunks, then two: two passes
def test_region_by_chunks_is_the_region_of_one_scan(chunk):
    ev = _eval_module()
    for pc in (torch.from_numpy(synth.uc_cases()[0][0])[None].cuda(), _tie_cloud()):
        want = ev.region_of_point0(pc, 1024)
        got = ev.region_of_point0(pc, 1024, "grid", chunk=chunk)
        assert got.shape == want.shape == (1, 1024, 3)
        assert torch.equal(got, want)
        assert torch.equal(ev.region_of_point0(pc, 1024, "brute", chunk=chunk), want)        # 'brute' never chunks
    with pytest.raises(ValueError):
        ev.region_of_point0(pc, 1024, "grid", chunk=2047)


def _uc_float64(a, b):
    def nn_var(pc):
        pc = pc[0].double()
        d = ((pc - pc[:1]) ** 2).sum(dim=1)
        region = pc[torch.topk(d, 1024, largest=False).indices]
        dd = torch.cdist(region, region)
        dd.fill_diagonal_(float("inf"))
        return dd.amin(dim=1).var(unbiased=False)
    return float(nn_var(b) / nn_var(a))


def test_calc_uc_grid_above_the_all_pairs_limit():
    """50000 points, more than pccx_knn takes: 'brute' reports that, 'grid' gives the coefficient.  Tolerance against float64: fp32
    distances carry ~1e-7 relative error, which the variance of 1024 of them amplifies by mean^2 / var, about 10 here: ~1e-5 in all.  A
    region that differed in its farthest point would move the coefficient by about 1 / 1024, so rtol 1e-4 also pins the region."""
    ev = _eval_module()
    n = 50000
    room = cloud_synth.room_cloud(7, n)
    rng = np.random.default_rng(8)
    recon = (room + rng.normal(0, 0.01, size=room.shape)).astype(np.float32)[rng.permutation(n)[:n - 500]]
    a, b = torch.from_numpy(room)[None].cuda(), torch.from_numpy(np.ascontiguousarray(recon))[None].cuda()
    with pytest.raises(_lib.PccxError):
        ev.calc_uc(a, b, "brute")
    got, want = ev.calc_uc(a, b, "grid"), _uc_float64(a, b)
    print(f"uniformity coefficient: grid {got!r}, float64 {want!r}")
    assert np.isfinite(got) and abs(got - want) <= 1e-4 * want, (got, want)
