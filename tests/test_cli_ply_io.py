"""GPU, end to end: compress.py / decompress.py / eval.py / train.py with --ply-io threads (PLY files on the library's host threads,
unpacked on the GPU) write the very bytes, CSV text and loss lines they write without the flag; a damaged file ends each reading
tool before any GPU work, by name."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model
from pccx import models, plyio, synth as cloud_synth
from tests import ply_cases as pc

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "point-cloud-compression_amd", "cli")
K, D, L, SEED = 64, 8, 5, 11
SHAPE = ["--K", str(K), "--d", str(D), "--L", str(L), "--seed", str(SEED)]
DAMAGED = b"ply\nformat binary_little_endian 1.0\nelement vertex 2048\nproperty float x\nproperty float y\nproperty float z\nend_header\n" + bytes(100)


def _cli(tool, *args, env=None):
    return subprocess.run([sys.executable, os.path.join(CLI, tool), *args], capture_output=True, text=True, timeout=600, env=env)


def _ok(tool, *args):
    r = _cli(tool, *args)
    assert r.returncode == 0, (tool, args, r.stderr[-3000:])
    return r.stdout


def _same_files(a, b, count):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == count, (os.listdir(a), os.listdir(b))
    for f in os.listdir(a):
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


def _coloured(path, cloud, layout, fmt):
    """`cloud` as a file of another vertex layout: its coordinates in the layout's x y z fields, random bytes in the others"""
    rec = np.zeros(len(cloud), dtype=np.dtype(layout))
    rng = np.random.default_rng(len(cloud))
    for nm, t in layout:
        rec[nm] = cloud[:, "xyz".index(nm)] if nm in "xyz" else rng.integers(0, 255, len(cloud))
    pc.write_ply(path, layout, len(cloud), fmt, 0, rec=rec, comments=True)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    mdl = tmp_path_factory.mktemp("model")
    ae = models.AE(K, K // 2, D, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, 3, last_gain={"pn.mlp_Modules.3.0": 40.0}))
    prob = models.ConditionalProbabilityModel(L, D)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, 4, gain=2.0))
    torch.save(ae.state_dict(), str(mdl / "ae.pkl"))
    torch.save(prob.state_dict(), str(mdl / "prob.pkl"))
    return str(mdl)


def test_one_size_folder_through_compress_decompress_eval(tmp_path, model):
    """four files of 2048 points -- float32, ASCII, double + colour (stride 27), big-endian float32 -- in the reference octree mode"""
    data = tmp_path / "data"
    data.mkdir()
    clouds = [cloud_synth.cad_cloud(500 + i, 2048) * np.float32(2.0) for i in range(4)]
    plyio.save_point_cloud(clouds[0], str(data / "a_f32.ply"))
    _coloured(str(data / "b_ascii.ply"), clouds[1], pc.LAYOUTS[15], pc.ASCII)
    _coloured(str(data / "c_f64_rgb.ply"), clouds[2].astype(np.float64) * 1.0000001, pc.LAYOUTS[27], pc.LE)
    _coloured(str(data / "d_big.ply"), clouds[3], pc.LAYOUTS[12], pc.BE)
    for how, flags in (("py", []), ("th", ["--ply-io", "threads"])):
        _ok("compress.py", str(data / "*.ply"), str(tmp_path / f"bin_{how}"), model, *SHAPE, *flags)
        _ok("decompress.py", str(tmp_path / "bin_py"), str(tmp_path / f"out_{how}"), model, *SHAPE, *flags)
        _ok("eval.py", "--input_glob", str(data / "*.ply"), "--compressed_path", str(tmp_path / "bin_py"), "--decompressed_path", str(tmp_path / "out_py"),
            "--output_file", str(tmp_path / f"{how}.csv"), "--ragged", *flags)
    _same_files(tmp_path / "bin_py", tmp_path / "bin_th", 12)
    _same_files(tmp_path / "out_py", tmp_path / "out_th", 4)
    assert (tmp_path / "py.csv").read_text() == (tmp_path / "th.csv").read_text() and len((tmp_path / "py.csv").read_text().splitlines()) == 5


def test_ragged_folder_through_compress_and_decompress(tmp_path, model):
    """--octree-mode full --ragged on sizes 2048 / 1300 / 300 (the header table routes the files before a vertex is read), and
    decompress.py --ragged --bin-ply-suffix"""
    data = tmp_path / "data"
    data.mkdir()
    for i, n in enumerate((2048, 1300, 300)):
        cloud = cloud_synth.cad_cloud(600 + i, n) * np.float32(2.0)
        if i == 1:
            _coloured(str(data / f"c{i}.ply"), cloud, pc.LAYOUTS[15], pc.BE)
        else:
            plyio.save_point_cloud(cloud, str(data / f"c{i}.ply"))
    full = ["--octree-mode", "full", "--ragged"]
    for how, flags in (("py", []), ("th", ["--ply-io", "threads"])):
        _ok("compress.py", str(data / "*.ply"), str(tmp_path / f"bin_{how}"), model, *SHAPE, *full, *flags)
        _ok("decompress.py", str(tmp_path / "bin_py"), str(tmp_path / f"out_{how}"), model, *SHAPE, *full, "--bin-ply-suffix", *flags)
    _same_files(tmp_path / "bin_py", tmp_path / "bin_th", 9)
    _same_files(tmp_path / "out_py", tmp_path / "out_th", 3)
    assert sorted(os.listdir(tmp_path / "out_th")) == [f"c{i}.ply.bin.ply" for i in range(3)]


SEEDED = ("import os, runpy, sys, torch; torch.manual_seed(5); sys.argv = sys.argv[1:]; sys.path.insert(0, os.path.dirname(sys.argv[0])); "
          "runpy.run_path(sys.argv[0], run_name='__main__')")


def test_train_prints_the_same_losses(tmp_path):
    """train.py --ragged --octree-mode full at the shapes of tests/test_train_ipdae_ragged.py's CLI test, each run a
    fresh child process seeded the same way (the tool itself draws its weights and batches unseeded)"""
    data, vdir = tmp_path / "data" / "train", tmp_path / "data" / "val"
    data.mkdir(parents=True), vdir.mkdir(parents=True)
    for i, n in enumerate((256, 640, 1300, 640, 256, 1300)):
        plyio.save_point_cloud(cloud_synth.cad_cloud(40 + i, n) * np.float32(2.0), str(data / f"c{i}.ply"))
    for i, n in enumerate((1300, 256)):
        plyio.save_point_cloud(cloud_synth.cad_cloud(50 + i, n) * np.float32(2.0), str(vdir / f"v{i}.ply"))
    lines = {}
    for how, flags in (("py", []), ("th", ["--ply-io", "threads"])):
        r = subprocess.run([sys.executable, "-c", SEEDED, os.path.join(CLI, "train.py"), "--train_glob", str(data / "*.ply"), "--model_save_folder",
                            str(tmp_path / f"model_{how}"), "--ragged", "--octree-mode", "full", "--K", "64", "--batch_size", "2", "--max_steps", "1",
                            "--step_window", "1", "--rate_loss_enable_step", "1", "--lamda", "10", "--reset", "--val_glob", str(vdir / "*.ply"), *flags],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[how] = [ln for ln in r.stdout.splitlines() if ln.startswith("[Epoch") or ln.startswith("--ragged:") or ln.startswith("Loaded")]
    assert len([ln for ln in lines["py"] if "Loss:" in ln]) == 2 and len([ln for ln in lines["py"] if "Val bpp" in ln]) == 2, lines["py"]
    assert lines["py"] == lines["th"]


def test_a_damaged_file_ends_each_tool_before_any_gpu_work(tmp_path):
    """compress.py, eval.py and train.py (decompress.py reads no PLY) with no GPU visible to the child: the damaged file is named, so
    it was found before the first thing that needs the GPU"""
    data = tmp_path / "data"
    data.mkdir()
    for i in range(2):
        plyio.save_point_cloud(cloud_synth.cad_cloud(700 + i, 2048), str(data / f"good{i}.ply"))
    (data / "damaged.ply").write_bytes(DAMAGED)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    glob = str(data / "*.ply")
    for tool, args in (("compress.py", [glob, str(tmp_path / "bin"), str(tmp_path / "no model")]),
                       ("eval.py", ["--input_glob", glob, "--compressed_path", str(tmp_path), "--decompressed_path", str(data), "--output_file", str(tmp_path / "e.csv")]),
                       ("train.py", ["--train_glob", glob, "--model_save_folder", str(tmp_path / "m"), "--crop", "--N", "1024"])):
        r = _cli(tool, *args, "--ply-io", "threads", env=env)
        assert r.returncode != 0 and "damaged.ply: the file is too short" in r.stderr and "good0.ply" not in r.stderr, (tool, r.stderr[-2000:])
    assert not os.path.exists(tmp_path / "e.csv") and os.listdir(tmp_path / "bin") == []
