"""CPU-side checks of the spliced reads' SAM lines: hsa_amd.splice.pair_segments against a
direct transcription of bwt_combine_segment_splice (bwtse.c:197-235) that keeps the
reference's in-place moves, hsa_amd.sam.spliced_line against every XT:A:S line of the
committed reference SAM files, and the declarations of hsa_splice_lines_device (header,
export, binding)."""
import ctypes
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from golden_io import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAN = json.load(open(os.path.join(GOLD, "manifest_dropin.json")))
U32 = 0xFFFFFFFF


# ---------------------------------------------------------------- pairing
def transcribed(rows):
    """bwtse.c:197-235 line by line on a list of [aln_id, seq_id, ori_pos, occ_pos, tag] rows:
    the quicksort of :169-192 (pivot the first element) and the loop with its memmove of two
    rows.  Returns (n_res, the rows as they stand afterwards)."""
    m = [list(r) + [k] for k, r in enumerate(rows)]

    def qsort(l, u):
        if l >= u:
            return
        pv, i, j = m[l][3], l, u + 1
        while True:
            i += 1
            while i <= u and m[i][3] < pv:
                i += 1
            j -= 1
            while m[j][3] > pv:
                j -= 1
            if i > j:
                break
            m[i], m[j] = m[j], m[i]
        m[l], m[j] = m[j], m[l]
        qsort(l, j - 1)
        qsort(j + 1, u)

    n_multi, n_res, shortest = len(m), 0, U32
    if n_multi == 2:
        return 1, m
    qsort(0, n_multi - 1)
    for i in range(n_multi - 1):
        t, t1 = m[i], m[i + 1]
        if t[0] != 0:
            continue
        if t[0] == t1[0] or t[1] != t1[1] or ((t1[3] - t[3]) & U32) > shortest:
            continue
        d = (t1[3] - t[3]) & U32
        if d < 50 or d > 50000:
            continue
        if d < shortest:
            shortest, n_res = d, 1
            if i == 0:
                continue
        elif d == shortest:
            n_res += 1
        two = [list(m[i]), list(m[i + 1])]          # memmove(res_multi, tmp_multi, 2 rows)
        m[(n_res - 1) * 2], m[(n_res - 1) * 2 + 1] = two
    return n_res, m


def R(aln, chrom, occ):
    return [aln, chrom, occ + 1, occ]


CASES = {
    "two rows far apart": ([R(0, 0, 1000), R(1, 0, 900000)], 1),
    "two rows, second before first": ([R(0, 0, 5000), R(1, 1, 100)], 1),
    "shorter pair at i > 0 replaces": ([R(0, 0, 1000), R(0, 0, 9000), R(1, 0, 3000), R(1, 0, 9100)], 1),
    "two pairs of equal distance": ([R(0, 0, 1000), R(0, 0, 9000), R(1, 0, 1300), R(1, 0, 9300)], 2),
    "d = 49": ([R(0, 0, 1000), R(1, 0, 1049), R(1, 0, 70000)], 0),
    "d = 50": ([R(0, 0, 1000), R(1, 0, 1050), R(1, 0, 70000)], 1),
    "d = 50000": ([R(0, 0, 1000), R(1, 0, 51000), R(1, 0, 170000)], 1),
    "d = 50001": ([R(0, 0, 1000), R(1, 0, 51001), R(1, 0, 170000)], 0),
    "different chromosomes": ([R(0, 0, 1000), R(1, 1, 1300), R(1, 1, 90000)], 0),
    "adjacent rows of one segment": ([R(0, 0, 1000), R(0, 0, 1100), R(1, 0, 1400), R(1, 0, 99000)], 1),
    "new shortest at i == 0": ([R(0, 0, 1000), R(1, 0, 1200), R(0, 0, 5000), R(1, 0, 5900)], 1),
    "shortest at i == 0, equal later": ([R(0, 0, 1000), R(1, 0, 1200), R(0, 0, 5000), R(1, 0, 5200)], 2),
    "longer first, then i > 0 shorter, then equal": ([R(0, 0, 100), R(1, 0, 900), R(0, 0, 5000), R(1, 0, 5300), R(0, 0, 9000),
                                                      R(1, 0, 9300)], 2),
    "segment 1 before segment 0 only": ([R(1, 0, 1000), R(0, 0, 1300), R(0, 0, 1900)], 0),
}


def hundred_rows():
    rng = np.random.default_rng(11)
    occ = rng.choice(150000, 100, replace=False)
    return [R(int(k >= 50), int(occ[k] >= 100000), int(occ[k])) for k in range(100)]


@pytest.mark.parametrize("name", list(CASES) + ["100 rows", "random"])
def test_pair_segments_equals_the_transcription(name):
    from hsa_amd import splice
    if name == "100 rows":
        sets = [(hundred_rows(), None)]
    elif name == "random":
        rng = np.random.default_rng(5)
        sets = []
        for _ in range(300):
            n = int(rng.integers(2, 12))
            occ = rng.choice(4000, n, replace=False) * 25
            n0 = int(rng.integers(1, n))
            sets.append(([R(int(k >= n0), int(rng.integers(0, 2)), int(occ[k])) for k in range(n)], None))
    else:
        sets = [CASES[name]]
    for rows, want in sets:
        n_res, index = splice.pair_segments(np.array(rows, np.int64))
        ref_n, ref_rows = transcribed(rows)
        assert n_res == ref_n and (want is None or n_res == want)
        assert len(index) == 2 * n_res
        assert [rows[k] for k in index] == [r[:4] for r in ref_rows[:2 * n_res]]
        for p in range(n_res if len(rows) > 2 else 0):
            a, b = rows[index[2 * p]], rows[index[2 * p + 1]]
            assert a[0] == 0 and b[0] == 1 and a[1] == b[1] and 50 <= b[3] - a[3] <= 50000
    if name == "100 rows":
        assert len(rows) == 100 and n_res >= 1


def test_rows_and_cap_of_a_segment():
    from hsa_amd import splice
    assert splice.segment_rows(10, 10) == 1 and splice.segment_rows(10, 59) == 50 and splice.segment_rows(10, 500) == 50
    assert splice.segment_rows(10, 9) == 0
    assert splice.capped_multi(5, 5, 9, 9) == 2 and splice.capped_multi(0, 60, 0, 60) == 100
    assert splice.capped_multi(0, 48, 0, 49) == 99 and splice.capped_multi(0, 49, 0, 49) == 100


def test_merge_cigar_places_the_intron():
    from hsa_amd import splice
    c = splice.merge_cigar([(0, 65), (2, 2), (0, 10), (4, 2)], 9649, 76, [(0, 73)], 9649 + 76 + 386)
    assert c == [(0, 65), (2, 2), (0, 10), (4, 2), (3, 386), (0, 73)]


# ---------------------------------------------------------------- the line
NT4 = {c: i for i, c in enumerate("ACGT")}


def fastq(path):
    ls = gzip.open(path, "rt").read().split("\n")
    out = {}
    for i in range(0, len(ls) - 3, 4):
        name = ls[i][1:].split()[0]
        if name[-2:] in ("/1", "/2"):
            name = name[:-2]
        out[name] = (np.array([NT4.get(c, 4) for c in ls[i + 1].upper()], np.uint8), ls[i + 3])
    return out


def s_lines(fixture):
    raw = gzip.open(os.path.join(GOLD, fixture)).read().decode()
    return [ln for ln in raw.splitlines() if "\tXT:A:S" in ln]


FIXTURES = [("dropin_ref_splice_default.sam.gz", "splice_reads", "splice_default", 225),
            ("dropin_ref_splice_n4o1.sam.gz", "splice_reads", "splice_n4o1", 304),
            ("dropin_ref_splice_n4o1O120.sam.gz", "splice_reads", "splice_n4o1O120", None),
            ("dropin_ref_default.sam.gz", "reads", "default", 57)]


def parse_s_line(ln):
    f = ln.split("\t")
    ops = [("MIDNSHP=X".index(o), int(l)) for l, o in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
    assert "".join(f"{l}{'MIDNSHP=X'[o]}" for o, l in ops) == f[5]
    at = [k for k, (o, _) in enumerate(ops) if o == 3]
    assert len(at) == 1
    tags = dict((t[:2], t[5:]) for t in f[11:])
    return dict(name=f[0], flag=int(f[1]), chr=f[2], pos=int(f[3]), mapq=int(f[4]), c0=ops[:at[0]], n_len=ops[at[0]][1],
                c1=ops[at[0] + 1:], tags=tags, fields=f)


def test_spliced_line_reproduces_every_reference_s_line():
    from hsa_amd import align, sam, splice
    total = strand1 = interior_s = 0
    for fixture, reads_key, man_key, count in FIXTURES:
        lines = s_lines(fixture)
        if count is not None:
            assert len(lines) == count
        reads = fastq(os.path.join(GOLD, MAN[reads_key]))
        opts = align.parse_options(MAN[man_key]["args"])[0]
        for ln in lines:
            p = parse_s_line(ln)
            seq, qual = reads[p["name"]]
            strand = 1 if p["flag"] & 16 else 0
            end0 = sum(l for o, l in p["c0"] if o in (0, 1, 4)) - 1        # any value serves: N is what is printed
            cigar = splice.merge_cigar(p["c0"], p["pos"], end0, p["c1"], p["pos"] + end0 + p["n_len"])
            got = sam.spliced_line(p["name"], seq, qual, p["chr"], p["pos"], cigar, strand, int(p["tags"]["X0"]),
                                   int(p["tags"].get("X1", 0)), int(p["tags"]["XM"]), max_top2=opts["max_top2"],
                                   flag=p["flag"] & ~16, comp_read=bool(opts["mode"] & 2))
            assert got == ln
            total += 1
            strand1 += strand
            interior_s += any(o == 4 for o, _ in p["c0"][1:]) or any(o == 4 for o, _ in p["c1"][:-1])
            assert p["mapq"] == 0 and p["tags"]["NM"] == "0" and p["tags"]["XO"] == "0" and p["tags"]["XG"] == "0"
            assert "MD" not in p["tags"] and "XA" not in p["tags"]
    # (dropin_ref_n4o0.sam.gz is left out: it has a line whose N length wrapped below zero, which the
    # reference prints as 268435454 and a NUL byte; the device refuses such a read, HSA_SL_INTRON)
    assert total == 890 and strand1 > 0 and interior_s > 0                # 586 in the three files run on the GPU


# ---------------------------------------------------------------- header and bindings
DECLS = r"""
#include "hsa_gpu.h"
int (*p_lines)(hsa_index_t *, const hsa_splice_lines_batch_t *, void *) = hsa_splice_lines_device;
_Static_assert(sizeof(hsa_splice_lines_batch_t) == 184, "hsa_splice_lines_batch_t layout");
_Static_assert(HSA_SL_OK == 0 && HSA_SL_NONE == 1 && HSA_SL_HANDED == 2 && HSA_SL_NOPAIR == 3 && HSA_SL_MULTI == 4 &&
               HSA_SL_REFINE == 5 && HSA_SL_POS == 6 && HSA_SL_INTRON == 7 && HSA_SL_INPUT == 8, "status codes");
_Static_assert(HSA_SL_ROW_WORDS == 24, "words per read row");
int (*p_merge)(hsa_index_t *, const hsa_sam_merge_batch_t *, void *) = hsa_sam_merge_device;
_Static_assert(sizeof(hsa_sam_merge_batch_t) == 88, "hsa_sam_merge_batch_t layout");
"""


def test_library_exports_the_symbol():
    from hsa_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libhsa_gpu.so first"
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "hsa_splice_lines_device") and hasattr(L, "hsa_sam_merge_device")
    assert {"hsa_splice_lines_device", "hsa_sam_merge_device"} <= set(_lib.EXPORTS)


def test_header_declares_the_entry_point(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(DECLS)
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "decl.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_struct_matches_the_binding():
    from hsa_amd import _lib
    B = _lib.SpliceLinesBatch
    assert ctypes.sizeof(B) == 184
    assert (B.d_codes.offset, B.d_res.offset, B.d_chr_off.offset, B.n_chr.offset, B.max_len.offset, B.cigar_stride.offset,
            B.d_rows.offset, B.out_cap.offset, B.d_counters.offset) == (16, 40, 88, 96, 112, 120, 128, 160, 176)
    assert (_lib.HSA_SL_OK, _lib.HSA_SL_NONE, _lib.HSA_SL_HANDED, _lib.HSA_SL_NOPAIR, _lib.HSA_SL_MULTI, _lib.HSA_SL_REFINE,
            _lib.HSA_SL_POS, _lib.HSA_SL_INTRON, _lib.HSA_SL_INPUT) == tuple(range(9))
    assert _lib.SL_ROW_WORDS == 24 and _lib.HSA_SP_MAX_STACKS == 128
    M = _lib.SamMergeBatch
    assert ctypes.sizeof(M) == 88 and (M.d_line_off_a.offset, M.text_a_len.offset, M.d_line_off_b.offset, M.d_line_off.offset,
                                       M.out_cap.offset, M.d_counters.offset) == (8, 24, 32, 56, 72, 80)


def test_the_call_on_a_null_handle_fails_loudly():
    from hsa_amd import _lib
    L = _lib.lib()
    assert L.hsa_splice_lines_device(None, None, None) == -2           # HSA_E_ARG (include/hsa_gpu.h)
    assert b"null" in L.hsa_last_error()
    gi = _lib.GpuIndex.__new__(_lib.GpuIndex)
    gi.h = None
    with pytest.raises(_lib.HsaError):
        gi.splice_lines(_lib.SpliceLinesBatch())
    assert L.hsa_sam_merge_device(None, None, None) == -2
    with pytest.raises(_lib.HsaError):
        gi.sam_merge(_lib.SamMergeBatch())


def test_splice_option_and_refusals_before_any_work():
    import io

    from hsa_amd import align
    o, rest, ex = align.parse_options(["--splice", "idx", "in.fq"])
    assert ex == dict(header=False, unaligned=None, out=None, splice=True) and rest == ["idx", "in.fq"]
    assert "splice" not in align.parse_options(["idx", "in.fq"])[2]

    class Handle:
        def __init__(self, long):
            self.long = long

        def is64(self):
            return self.long
    with pytest.raises(ValueError, match="not built"):
        align.align_fastq(Handle(True), ["c"], b"@r\nACGT\n+\nIIII\n", align.parse_options([])[0], io.BytesIO(), splice=True)
    with pytest.raises(ValueError, match="not built"):                  # 159 score buckets
        align.align_fastq(Handle(False), ["c"], b"@r\nACGT\n+\nIIII\n", align.parse_options(["-n", "4", "-o", "1", "-O", "120"])[0],
                          io.BytesIO(), splice=True)
