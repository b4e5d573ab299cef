"""GPU: compress.py / decompress.py with --p-split (the split form of .p.bin), each as a fresh child process, in the style of
tests/test_cli_compat.py: the decoded points are Codec's, and files written without the flag are refused by name."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model
from pccx import codec, dist, models, plyio, synth as cloud_synth
from tests import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "point-cloud-compression_amd", "cli")


def test_cli_p_split_round_trip_and_refusal_of_unsplit_files(tmp_path):
    K, k, d, L = synth.MODEL_CFG
    N, S = 2048, 16
    data, mdl, comp, dec, plain = (tmp_path / n for n in ("data", "model", "comp", "dec", "plain"))
    data.mkdir(), mdl.mkdir()
    names = ["a.ply", "b.ply"]
    clouds = [cloud_synth.cad_cloud(70 + i, N) * np.float32(2.0) for i in range(2)]
    for n, c in zip(names, clouds):
        plyio.save_point_cloud(c, str(data / n))
    ae = models.AE(K, k, d, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    prob = models.ConditionalProbabilityModel(L, d)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    torch.save(ae.state_dict(), str(mdl / "ae.pkl"))
    torch.save(prob.state_dict(), str(mdl / "prob.pkl"))
    run = lambda *a: subprocess.run([sys.executable, *a], capture_output=True, text=True, timeout=600)
    flags = ["--octree-mode", "full", "--p-split", "4"]
    r = run(os.path.join(CLI, "compress.py"), str(data / "*.ply"), str(comp), str(mdl), *flags)
    assert r.returncode == 0 and "Execution time" in r.stdout, r.stderr[-2000:]
    r = run(os.path.join(CLI, "decompress.py"), str(comp), str(dec), str(mdl), *flags)
    assert r.returncode == 0 and "Execution time" in r.stdout, r.stderr[-2000:]
    # the same through Codec: same files, same points
    cd = codec.Codec(ae.pack("cuda"), prob.pack("cuda"), K=K, octree_mode="full", max_centres=codec.OCTREE_WIDE_MAX_S, p_split=4)
    pc = torch.from_numpy(np.stack([plyio.read_point_cloud(str(data / n)) for n in names])).cuda()
    c = cd.compress(pc, [dist.fps_start_index(11, i, N) for i in range(2)])
    out = cd.decompress(c, S=S).cpu().numpy()
    for b, n in enumerate(names):
        s, p, cc_ = c.files(b)
        assert open(comp / (n + ".p.bin"), "rb").read() == p and p[:4] == b"PXS1"
        assert open(comp / (n + ".s.bin"), "rb").read() == s and open(comp / (n + ".c.bin"), "rb").read() == cc_
        assert np.array_equal(plyio.read_point_cloud(str(dec / n)), out[b])
    # files written without the flag: decompress.py --p-split 4 names the file and fails, and writes nothing
    r = run(os.path.join(CLI, "compress.py"), str(data / "*.ply"), str(plain), str(mdl), "--octree-mode", "full")
    assert r.returncode == 0, r.stderr[-2000:]
    r = run(os.path.join(CLI, "decompress.py"), str(plain), str(tmp_path / "dec_plain"), str(mdl), *flags)
    assert r.returncode != 0 and "a.ply.p.bin" in r.stderr and "split" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "dec_plain" / "a.ply")
