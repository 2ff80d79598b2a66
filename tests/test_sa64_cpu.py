"""CPU-side checks of the 64-bit text-position entry points: the built library exports
them, include/hsa_gpu.h declares them with the documented argument lists (a C file that
takes their addresses with those types compiles), and without a usable handle they fail
loudly instead of answering."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["hsa_build_bwt_index_device64", "hsa_index_set_sa64", "hsa_index_set_sa64_device", "hsa_sa_position_batch64",
       "hsa_sa_position_device64", "hsa_psi_minus_batch64", "hsa_hit_positions_device64"]

DECLS = r"""
#include "hsa_gpu.h"
int (*p_build)(int, uint64_t, const uint32_t *, uint32_t *, uint64_t *, uint64_t[5], uint32_t, uint64_t *) =
    hsa_build_bwt_index_device64;
int (*p_set)(hsa_index_t *, const uint64_t *, uint64_t, uint32_t, const uint64_t *, int) = hsa_index_set_sa64;
int (*p_setd)(hsa_index_t *, uint64_t *, uint64_t, uint32_t, const uint64_t *, int) = hsa_index_set_sa64_device;
int (*p_pos)(hsa_index_t *, size_t, const uint64_t *, uint64_t *) = hsa_sa_position_batch64;
int (*p_posd)(hsa_index_t *, size_t, const uint64_t *, uint64_t *, void *) = hsa_sa_position_device64;
int (*p_psi)(hsa_index_t *, size_t, const uint64_t *, uint64_t *) = hsa_psi_minus_batch64;
int (*p_hit)(hsa_index_t *, const hsa_hitpos_batch64_t *, void *) = hsa_hit_positions_device64;
_Static_assert(sizeof(hsa_hitpos_batch64_t) == 72, "hsa_hitpos_batch64_t layout");
"""


def test_library_exports_the_sa64_symbols():
    from hsa_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libhsa_gpu.so first"
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(_lib.EXPORTS) >= set(NEW)


def test_header_declares_the_sa64_entry_points(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(DECLS)
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "decl.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_hitpos_struct_matches_the_binding():
    from hsa_amd import _lib
    assert ctypes.sizeof(_lib.HitPosBatch64) == 72
    assert _lib.HitPosBatch64.d_pos_off.offset == 32 and _lib.HitPosBatch64.d_counters.offset == 64


def test_sa64_on_a_null_handle_fails_loudly():
    """No handle, no answer: every entry point that takes an index checks it before any
    HIP call (HSA_E_ARG), and the Python methods raise on a closed index."""
    from hsa_amd import _lib
    L = _lib.lib()
    one = np.ones(4, np.uint64)
    assert L.hsa_index_set_sa64(None, one, 4, 8, one, 1) == -2            # HSA_E_ARG (include/hsa_gpu.h)
    assert b"null" in L.hsa_last_error()
    assert L.hsa_index_set_sa64_device(None, 16, 4, 8, one, 1) == -2
    assert L.hsa_sa_position_batch64(None, 1, one, one) == -2
    assert L.hsa_sa_position_device64(None, 1, None, None, None) == -2
    assert L.hsa_psi_minus_batch64(None, 1, one, one) == -2
    assert L.hsa_hit_positions_device64(None, None, None) == -2
    gi = _lib.GpuIndex.__new__(_lib.GpuIndex)
    gi.h = None
    with pytest.raises(_lib.HsaError):
        gi.set_sa64(one, 8, [[0, 0, 3, 0]])
    with pytest.raises(_lib.HsaError):
        gi.sa_positions64(one)


def test_sa64_builder_rejects_bad_arguments_before_the_device():
    from hsa_amd import _lib
    L = _lib.lib()
    isa0 = ctypes.c_uint64()
    Cc = np.zeros(5, np.uint64)
    assert L.hsa_build_bwt_index_device64(0, 0, 16, 16, ctypes.byref(isa0), Cc, 8, 16) == -2          # T == 0
    assert L.hsa_build_bwt_index_device64(0, 1 << 36, 16, 16, ctypes.byref(isa0), Cc, 8, 16) == -2    # T >= 2^36
    assert L.hsa_build_bwt_index_device64(0, 100, 16, 16, ctypes.byref(isa0), Cc, 0, 16) == -2        # samples, no interval
    assert b"sa_interval" in L.hsa_last_error()
