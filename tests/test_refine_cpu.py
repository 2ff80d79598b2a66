"""CPU-side checks of the refinement step (position rows -> CIGAR, NM, MD on the 64-bit
path): the Python helper that turns a row's output into the SAM strings, the new
declarations (a C file that takes their addresses with the documented types compiles,
the struct sizes match the binding), and the entry points fail loudly without a handle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["hsa_index_set_text64_device", "hsa_refine_rows_device64"]

DECLS = r"""
#include "hsa_gpu.h"
int (*p_text)(hsa_index_t *, uint32_t *, uint64_t) = hsa_index_set_text64_device;
int (*p_refine)(hsa_index_t *, const hsa_refine_batch64_t *, void *) = hsa_refine_rows_device64;
_Static_assert(sizeof(hsa_refine_batch64_t) == 136, "hsa_refine_batch64_t layout");
_Static_assert(HSA_RF_OK == 0 && HSA_RF_POS == 1 && HSA_RF_TEXT == 2 && HSA_RF_CAP == 3 && HSA_RF_MD == 4, "status codes");
_Static_assert(HSA_RF_MAX_LEN >= 1023 && HSA_RF_MAX_GAP >= 16, "the layout the kernels must answer");
_Static_assert(HSA_RF_ROW_WORDS == 8, "words per row");
"""


def op(code, n):
    return ("MIDNS".index(code) << 28) | n


def test_cigar_text_prints_the_reference_encoding():
    from hsa_amd import refine
    ops = np.array([op("S", 3), op("M", 40), op("I", 2), op("M", 10), op("D", 5), op("M", 45), op("S", 1)], np.uint32)
    assert refine.cigar_text(ops) == "3S40M2I10M5D45M1S"
    assert refine.cigar_text(ops, 2) == "3S40M"                     # n_cigar of a longer stride
    assert refine.cigar_text(np.array([100], np.uint32)) == "100M"  # the ungapped row: op 0
    with pytest.raises(ValueError):
        refine.cigar_text(ops, 8)                                   # HSA_RF_MD: more ops than the stride held
    with pytest.raises(ValueError):
        refine.cigar_text(np.array([9 << 28 | 1], np.uint32))


def test_md_text_keeps_the_bytes():
    from hsa_amd import refine
    md = np.frombuffer(b"50C0C24^ACG0T23xxxx", np.uint8)
    assert refine.md_text(md, 15) == "50C0C24^ACG0T23"               # the zero-length count between two mismatches, a ^ run
    assert refine.md_text(md[:3]) == "50C"
    assert refine.md_text(md, 0) == ""
    with pytest.raises(ValueError):
        refine.md_text(md, 20)


def test_row_sam_reads_the_row_words():
    from hsa_amd import _lib, refine
    row = np.array([_lib.HSA_RF_OK, 3, 4, 9, 2, 0, 0, 0], np.uint32)
    cg = np.array([op("S", 2), op("M", 30), op("S", 4), 0xFFFFFFFF], np.uint32)
    md = np.frombuffer(b"10A0C17^T" + b"\xff" * 7, np.uint8)
    assert refine.row_sam(row, cg, md) == dict(status=0, cigar="2S30M4S", nm=4, md="10A0C17^T", trim5=2, trim3=0)
    assert len(row) == _lib.RF_ROW_WORDS


def test_library_exports_the_refine_symbols():
    from hsa_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libhsa_gpu.so first"
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(_lib.EXPORTS) >= set(NEW)


def test_header_declares_the_refine_entry_points(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(DECLS)
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "decl.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_refine_struct_matches_the_binding():
    from hsa_amd import _lib
    B = _lib.RefineBatch64
    assert ctypes.sizeof(B) == 136
    assert (B.d_pos_off.offset, B.pos_cap.offset, B.max_len.offset, B.md_stride.offset, B.d_rows.offset,
            B.d_counters.offset) == (40, 64, 80, 88, 96, 128)
    assert (_lib.HSA_RF_OK, _lib.HSA_RF_POS, _lib.HSA_RF_TEXT, _lib.HSA_RF_CAP, _lib.HSA_RF_MD) == (0, 1, 2, 3, 4)


def test_refine_on_a_null_handle_fails_loudly():
    from hsa_amd import _lib
    L = _lib.lib()
    assert L.hsa_index_set_text64_device(None, 16, 4) == -2          # HSA_E_ARG (include/hsa_gpu.h)
    assert b"null" in L.hsa_last_error()
    assert L.hsa_refine_rows_device64(None, None, None) == -2
    assert b"null" in L.hsa_last_error()
    gi = _lib.GpuIndex.__new__(_lib.GpuIndex)
    gi.h = None
    with pytest.raises(_lib.HsaError):
        gi.set_text64_device(16, 4)
    with pytest.raises(_lib.HsaError):
        gi.refine_rows64(_lib.RefineBatch64())
