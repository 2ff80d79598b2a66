"""CPU-side checks of the FASTA loader (hsa_fasta_device, hsa_bwt_files_device): the
declarations and the binding's struct agree, the entry points check their arguments before
any HIP call, the one-rule restatement the kernels implement equals parse_fasta on every
input the GPU tests use, and the random generator makes no input that is refused."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fasta_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["hsa_fasta_scratch_bytes", "hsa_fasta_device", "hsa_bwt_files_scratch_bytes", "hsa_bwt_files_device",
       "hsa_fasta_timing", "hsa_fasta_launch_times", "hsa_bwt_files_launch_times"]

DECLS = r"""
#include "hsa_gpu.h"
int (*p_size)(int, uint64_t, uint64_t *) = hsa_fasta_scratch_bytes;
int (*p_fasta)(int, const hsa_fasta_batch_t *, void *) = hsa_fasta_device;
int (*p_bsize)(int, uint64_t, uint64_t *) = hsa_bwt_files_scratch_bytes;
int (*p_files)(int, uint64_t, const uint32_t *, uint32_t *, uint32_t *, uint32_t *, void *, uint64_t, void *) = hsa_bwt_files_device;
_Static_assert(sizeof(hsa_fasta_batch_t) == 136, "hsa_fasta_batch_t layout");
_Static_assert(HSA_FA_REC_WORDS == 4 && HSA_FA_COUNTERS == 18 && HSA_FA_LAUNCHES == 8 && HSA_BF_LAUNCHES == 3, "constants");
"""


def test_library_exports_the_symbols():
    from hsa_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in NEW if not hasattr(L, n)]
    assert set(_lib.EXPORTS) >= set(NEW)


def test_header_declares_the_entry_points(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(DECLS)
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "decl.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_struct_matches_the_binding():
    from hsa_amd import _lib
    B = _lib.FastaBatch
    assert ctypes.sizeof(B) == 136
    assert (B.n_in.offset, B.d_pac.offset, B.rpac_cap.offset, B.d_rec.offset, B.d_counters.offset, B.scratch_bytes.offset) == \
        (8, 16, 40, 80, 112, 128)
    assert len(_lib.FA_COUNTERS) == 18 and len(_lib.FA_LAUNCHES) == 8 and len(_lib.BF_LAUNCHES) == 3


def test_arguments_are_checked_before_any_device_call():
    from hsa_amd import _lib
    L = _lib.lib()
    n = ctypes.c_uint64()
    assert L.hsa_fasta_device(0, None, None) == -2                     # HSA_E_ARG (include/hsa_gpu.h)
    assert b"null" in L.hsa_last_error()
    assert L.hsa_fasta_device(0, ctypes.byref(_lib.FastaBatch()), None) == -2
    assert b"null" in L.hsa_last_error()
    full = dict(d_in=256, n_in=16, d_pac=256, pac_cap=8, d_rpac=256, rpac_cap=8, d_text=256, text_cap=8, d_rtext=256,
                rtext_cap=8, d_rec=256, rec_cap=1, d_blk=256, blk_cap=1, d_counters=256, d_scratch=256, scratch_bytes=1 << 20)
    assert L.hsa_fasta_device(0, ctypes.byref(_lib.FastaBatch(**dict(full, n_in=(1 << 32) - 256))), None) == -2
    assert b"2^32 - 256" in L.hsa_last_error()
    assert L.hsa_fasta_device(0, ctypes.byref(_lib.FastaBatch(**dict(full, d_pac=258))), None) == -2
    assert b"boundaries" in L.hsa_last_error()
    assert L.hsa_fasta_scratch_bytes(0, 16, None) == -2
    assert L.hsa_fasta_scratch_bytes(0, (1 << 32) - 256, ctypes.byref(n)) == -2
    assert L.hsa_bwt_files_device(0, 16, None, 256, 256, 256, 256, 4096, None) == -2
    assert b"null" in L.hsa_last_error()
    assert L.hsa_bwt_files_device(0, 0, 256, 256, 256, 256, 256, 4096, None) == -2
    assert L.hsa_bwt_files_device(0, (1 << 32) - 1, 256, 256, 256, 256, 256, 4096, None) == -2
    assert L.hsa_bwt_files_scratch_bytes(0, 16, None) == -2


def test_build_index_refuses_an_oversized_fasta(tmp_path, monkeypatch):
    from hsa_amd import index_build
    fa = tmp_path / "big.fa"
    fa.write_bytes(b">a\nACGT\n")
    monkeypatch.setattr(os.path, "getsize", lambda p: (1 << 32) - 256)
    with pytest.raises(ValueError, match="2\\^32 - 256"):
        index_build.build_index(str(fa))


def test_the_rule_equals_parse_fasta_on_the_gpu_tests_inputs():
    """Every hand-written input, and the random generator's first 200: parse_fasta accepts
    them (none is refused) and the rule the kernels implement gives its codes, `total` and
    annotation."""
    from hsa_amd import fasta, index_build
    inputs = [fc.edge_fasta()] + fc.quirk_fastas() + fc.length_fastas() + fc.tile_fastas() + [fc.random_fasta(s) for s in range(200)]
    empty = 0
    for data in inputs:
        assert fc.refused_offset(data) is None
        codes, ann, total = index_build.parse_fasta(data)
        r_codes, rec, blk, r_total = fc.rule(data)
        assert np.array_equal(codes, r_codes) and total == r_total
        assert fasta.ann_rows(data, rec, blk) == [(n, [tuple(b) for b in bl]) for n, bl in ann]
        empty += any(e == s - 1 for _, bl in ann for s, e, _ in bl)
    assert empty > 20                                               # all-ambiguous records occur
