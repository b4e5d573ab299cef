"""CPU: the C-ABI library loads and exports every symbol include/pccx.h declares (no compute)."""
import ctypes
import os
import re

import pytest

from pccx import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "pccx.h")).read()
    return sorted(set(re.findall(r"PCCX_API\s+[\w\s\*]+?\b(pccx_\w+)\s*\(", txt)))


def test_header_declares_symbols():
    names = _declared()
    assert "pccx_fps" in names and "pccx_octree_encode" in names and len(names) >= 10


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        from pccx import build
        build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), f"libpccx.so does not export {name}"


def test_python_binding_covers_header():
    assert sorted(_lib.declared_symbols()) == _declared()


def test_derived_signatures():
    """The ctypes table is parsed from include/pccx.h: hand-written rows that between them hold every kind of type the header uses."""
    C = ctypes
    P, i, i64, f, dbl, s = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_char_p
    sig = _lib.signatures()
    assert sig["pccx_last_error"] == (s, [])
    assert sig["pccx_sort_keys_workspace_bytes"] == (C.c_size_t, [i64])
    assert sig["pccx_normalize"] == (i, [P, i, i, dbl, P, P, P, P])
    assert sig["pccx_write_streams_host"] == (i, [P, i, i, i, s, s, P, i])
    assert sig["pccx_range_coder_form"] == (i, [i, i, i, i])
    assert sig["pccx_replicate_rows"] == (i, [P, i64, i, P, P, P, P])
    assert sig["pccx_ae_decode_h2_list"] == (i, [P, i, i, i, P, P, P, P, f, P, P, P, i, dbl, P, P, P, P])
    assert _lib.parse_header("/* PCCX_API int pccx_a(int); */\nPCCX_API size_t pccx_b(void); // PCCX_API int pccx_c(int);\n") == {
        "pccx_b": (C.c_size_t, [])}
    for bad in ("PCCX_API int pccx_f(const float *x,\n                    uint8_t flag);", "PCCX_API long pccx_f(int n);",
                "PCCX_API int pccx_f(unsigned int n);", "PCCX_API int pccx_f(int (*callback)(int));"):
        with pytest.raises(_lib.PccxError, match="pccx_f"):
            _lib.parse_header(bad)


def test_ops_fail_loudly_without_gpu_tensor():
    import torch
    from pccx import ops
    with pytest.raises(_lib.PccxError):
        ops.normalize(torch.zeros(1, 8, 3))     # CPU tensor: no fallback


def test_version_and_error_string():
    lib = _lib.load()
    assert lib.pccx_version() >= 100
    # argument validation happens on the host, before any HIP call
    rc = lib.pccx_octree_encode(None, 1, 64, 8192, 0.25, None, None, None, None, None, None)
    assert rc == -1 and b"null pointer" in lib.pccx_last_error()


def test_range_coder_form_query_states_the_lds_budget():
    """pccx_range_coder_form is host arithmetic (no GPU): 0 = one wave per cloud while the kernel's LDS image fits 60 KiB -- encode
    nsym*8 + round4(cap), decode round4(nsym*(L+1)*2) + round4(stride) + nsym and 2 <= L <= 63 -- else 1 = one lane per cloud."""
    form = _lib.load().pccx_range_coder_form
    r4 = lambda v: (v + 3) // 4 * 4
    for nsym in (0, 1, 77, 1024, 4352, 6000, 7679, 7680, 16384):
        for cap in (8, 9, 2 * nsym + 16, 61440 - 8 * nsym - 4, 61440 - 8 * nsym - 3, 61440 - 8 * nsym, 61440 - 8 * nsym + 1, 61440):
            if cap >= 0:
                assert form(0, nsym, 7, cap) == (0 if nsym * 8 + r4(cap) <= 61440 else 1), (nsym, cap)
        for L in (1, 2, 7, 63, 64, 200):
            fixed = r4(nsym * (L + 1) * 2) + nsym
            for stride in (1, 5, 61440 - fixed - 3, 61440 - fixed, 61440 - fixed + 1, 61440):
                if stride >= 0:
                    assert form(1, nsym, L, stride) == (0 if fixed + r4(stride) <= 61440 and 2 <= L <= 63 else 1), (nsym, L, stride)
    # the shapes the codec runs: 64 patches of d = 16 take the wave kernels, the whole-cloud codec's 1024 patches the one-lane ones
    assert form(0, 1024, 7, 2 * 1024 + 16) == 0 and form(1, 1024, 7, 2 * 1024 + 16) == 0
    assert form(0, 16384, 7, 2 * 16384 + 16) == 1 and form(1, 16384, 7, 2 * 16384 + 16) == 1
    assert form(0, 383 * 16, 7, 2 * 383 * 16 + 16) == 0 and form(0, 384 * 16, 7, 2 * 384 * 16 + 16) == 1


def test_model_limits_name_the_reference_flags():
    """compress.py:30-34 accepts any --K / --d / --L.  --d and --L are unrestricted here too (widths beyond the fused kernels' 16 /
    d * L <= 128 take the generic layers, tests/test_gpu_model.py); --K must be a multiple of 16 in 16..1024 (the reference's own
    octree rate table, pn_kit.py:17-23, stops at 1024): refused loudly, naming the flag, before any GPU work."""
    import pytest as _pt
    from pccx import models
    for K, k, d, L in ((250, 125, 16, 7), (2048, 1024, 16, 7), (256, 128, 0, 7)):
        with _pt.raises(_lib.PccxError, match="--K"):
            models.AE(K, k, d, L)
    assert models.AE(256, 128, 32, 7).fused_d is False and models.AE(512, 256, 8, 16).fused_d is True
    assert models.ConditionalProbabilityModel(9, 16).fused_ok(64) is False and models.ConditionalProbabilityModel(7, 16).fused_ok(64) is True
