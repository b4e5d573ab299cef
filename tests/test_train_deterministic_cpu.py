"""CPU side of the deterministic training mode: the command line, the ctypes table of the new entry points, and the step scope's flag."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "point-cloud-compression_amd", "cli", "train.py")

# the reference's flags in the reference's order with the defaults its --help prints (train.py:22-50); store_true flags print none
REFERENCE_FLAGS = [("--train_glob", "./data/ModelNet40_pc_01_8192p/**/train/*.ply"), ("--model_save_folder", "./model/K256/"), ("--model", "AE"),
                   ("--N", "8192"), ("--N0", "1024"), ("--ALPHA", "2"), ("--K", "256"), ("--d", "16"), ("--L", "7"), ("--lr", "0.0005"),
                   ("--batch_size", "1"), ("--step_window", "100"), ("--lamda", "1e-06"), ("--rate_loss_enable_step", "40000"),
                   ("--lr_decay", "0.1"), ("--lr_decay_steps", "60000"), ("--max_steps", "80000"), ("--device", "cuda"), ("--reset", None)]


def test_train_cli_lists_deterministic_after_the_references_flag_block():
    r = subprocess.run([sys.executable, CLI, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    body = r.stdout[r.stdout.index("options:"):] if "options:" in r.stdout else r.stdout
    flat = " ".join(body.split())
    pos = []
    for flag, default in REFERENCE_FLAGS:
        at = flat.find(f" {flag} ")
        assert at >= 0, flag
        pos.append(at)
        if default is not None:
            nxt = flat.find(" --", at + 1)
            assert f"(default: {default})" in flat[at:nxt if nxt > 0 else None], (flag, flat[at:nxt])
    assert pos == sorted(pos)                                                # the reference's order
    det = flat.find(" --deterministic ")
    assert det > pos[-1], "--deterministic is an additive flag: it comes after the reference's block"
    src = open(CLI).read()
    assert "deterministic=args.deterministic" in src and 'print(f"deterministic' in src      # plumbed to the trainer, printed in the first lines


NEW_ENTRIES = {
    "pccx_linear_dw_det_workspace_floats": (C.c_size_t, 3), "pccx_linear_dw_det": (C.c_int, 11),
    "pccx_linear_skinny_dx_det_workspace_floats": (C.c_size_t, 3), "pccx_linear_skinny_dx_det": (C.c_int, 11),
    "pccx_col_reduce_det_doubles": (C.c_size_t, 2), "pccx_col_reduce_det": (C.c_int, 12),
    "pccx_smooth_l1_det_doubles": (C.c_size_t, 1), "pccx_smooth_l1_det": (C.c_int, 8),
    "pccx_sumsq_multi_det_doubles": (C.c_size_t, 1), "pccx_sumsq_multi_det": (C.c_int, 6),
    "pccx_scatter_add_ordered_workspace_ints": (C.c_size_t, 3), "pccx_scatter_add_ordered": (C.c_int, 11),
    "pccx_chamfer_grad_det_workspace_floats": (C.c_size_t, 3), "pccx_chamfer_grad_det_workspace_ints": (C.c_size_t, 3),
    "pccx_chamfer_grad_det": (C.c_int, 13),
}


def test_header_parser_types_every_deterministic_entry_point():
    from pccx import _lib
    sig = _lib.signatures()
    for name, (restype, nargs) in NEW_ENTRIES.items():
        assert name in sig, name
        got_ret, got_args = sig[name]
        assert got_ret is restype and len(got_args) == nargs and all(a is not None for a in got_args), (name, got_ret, got_args)
    ret, args = sig["pccx_scatter_add_ordered"]
    assert args == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert sig["pccx_linear_dw_det_workspace_floats"][1] == [C.c_int64, C.c_int, C.c_int]
    assert sig["pccx_col_reduce_det"][1][6:8] == [C.c_int64, C.c_int] and sig["pccx_smooth_l1_det"][1][3] is C.c_float


def test_step_scope_sets_and_restores_the_deterministic_flag():
    from pccx import ops, train
    assert train._DETERMINISTIC is False and ops.deterministic_hook() is False
    with train.step_scope("cpu", deterministic=True) as forward_done:
        assert train._DETERMINISTIC is True and ops.deterministic_hook() is True
        forward_done()
        assert train._DETERMINISTIC is True                                  # it stays through backward and the optimiser step
    assert train._DETERMINISTIC is False
    with pytest.raises(ZeroDivisionError):
        with train.step_scope("cpu", deterministic=True):
            assert train._DETERMINISTIC is True
            1 / 0
    assert train._DETERMINISTIC is False and train._AUTOCAST is False and train._ARENA is None
    with train.step_scope("cpu"):
        assert train._DETERMINISTIC is False                                 # the default


def test_deterministic_with_data_parallel_raises_before_any_gpu_work():
    from pccx import _lib, train
    with pytest.raises(_lib.PccxError, match="RCCL"):
        train.train_step(None, None, None, None, data_parallel=True, deterministic=True)
    with pytest.raises(_lib.PccxError, match="RCCL"):
        train.GraphedTrainStep(None, None, None, None, data_parallel=True, deterministic=True)
