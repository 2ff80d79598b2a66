"""CPU-side checks of the XA:Z lists of spliced reads with several splice pairs:
hsa_amd.sam.spliced_line(..., xa=...) over hsa_amd.splice.multi_entries against every XT:A:S
line of the committed reference files of the dup genome (tools/make_golden_dup.py), the order
of the entries over hsa_amd.splice.pair_segments, and the declarations of
hsa_splice_lines_device_xa (header, export, binding)."""
import ctypes
import gzip
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from golden_io import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAN = json.load(open(os.path.join(GOLD, "manifest_dup.json")))
CASES = ["default", "n4o1", "q15"]
CHRS = ["chrA", "chrB"]
NT4 = {c: i for i, c in enumerate("ACGT")}
OPS = "MIDNSHP=X"


def fastq(key):
    ls = gzip.open(os.path.join(GOLD, MAN["files"][key]), "rt").read().split("\n")
    return {ls[i][1:].split()[0]: (np.array([NT4.get(c, 4) for c in ls[i + 1].upper()], np.uint8), ls[i + 3])
            for i in range(0, len(ls) - 3, 4)}


def reference(case):
    raw = gzip.open(os.path.join(GOLD, f"dup_ref_{case}.sam.gz")).read()
    return raw, raw.decode().splitlines()


def parse_cigar(c):
    ops = [(OPS.index(o), int(l)) for l, o in re.findall(r"(\d+)([MIDNSHP=X])", c)]
    assert "".join(f"{l}{OPS[o]}" for o, l in ops) == c
    return ops


def split_entries(text, read_len):
    """The entries of an XA:Z text of a spliced read: (chromosome, strand, position, ops).
    The position and the first CIGAR length abut; the split is the one at which the CIGAR's
    M, I and S lengths sum to the read's length, and it must be unique."""
    heads = list(re.finditer(r"(%s),([+-])" % "|".join(CHRS), text))
    assert heads and heads[0].start() == 0
    out = []
    for k, h in enumerate(heads):
        body = text[h.end():heads[k + 1].start() if k + 1 < len(heads) else len(text)]
        digits = re.match(r"\d+", body).group(0)
        fits = []
        for cut in range(1, len(digits)):
            if digits[cut] == "0":
                continue                                    # (no length is printed with a leading zero)
            ops = parse_cigar(body[cut:])
            if sum(l for o, l in ops if o in (0, 1, 4)) == read_len and sum(o == 3 for o, _ in ops) == 1:
                fits.append((int(digits[:cut]), ops))
        assert len(fits) == 1, (body, fits)
        out.append((h.group(1), h.group(2) == "-", fits[0][0], fits[0][1]))
    return out


def parse_line(ln):
    f = ln.split("\t")
    ops = parse_cigar(f[5])
    tags = dict((t[:2], t[5:]) for t in f[11:])
    return dict(name=f[0], flag=int(f[1]), chr=f[2], pos=int(f[3]), ops=ops, tags=tags)


def halves(ops):
    at = [k for k, (o, _) in enumerate(ops) if o == 3]
    assert len(at) == 1
    return ops[:at[0]], ops[at[0]][1], ops[at[0] + 1:]


def unclipped(ops, strand, clip):
    """The line's own CIGAR before bwa_correct_trimmed (the reverse of sam.clipped_cigar)."""
    if not clip:
        return ops
    ops = list(ops)
    at = 0 if strand else len(ops) - 1
    assert ops[at][0] == 4 and ops[at][1] >= clip
    if ops[at][1] == clip:
        del ops[at]
    else:
        ops[at] = (4, ops[at][1] - clip)
    return ops


@pytest.mark.parametrize("case", CASES)
def test_spliced_line_with_xa_reproduces_every_reference_line(case):
    from hsa_amd import align, sam, splice
    raw, lines = reference(case)
    m = MAN[case]
    assert hashlib.sha256(raw).hexdigest() == m["sam_sha256"] and len(lines) == m["sam_lines"] and b"\0" not in raw
    reads = fastq(m["reads"])
    opts = align.parse_options(m["args"], reader_options=True)[0]
    seen = dict(s=0, xa=0, entries=0, longest=0, other_chr=0, reverse=0, clipped_xa=0, max_x0=0)
    for ln in lines:
        if "\tXT:A:S" not in ln:
            continue
        p = parse_line(ln)
        seq, qual = reads[p["name"]]
        strand = 1 if p["flag"] & 16 else 0
        clip_len = int(p["tags"].get("XC", len(seq)))
        own = unclipped(p["ops"], strand, len(seq) - clip_len)
        c0, n_len, c1 = halves(own)
        end0 = 41                                           # any value serves: N is what is printed
        pairs = [(CHRS.index(p["chr"]), strand, c0, p["pos"], end0, c1, p["pos"] + end0 + n_len)]
        if "XA" in p["tags"]:
            for chrom, st, pos, ops in split_entries(p["tags"]["XA"], clip_len):
                a0, n, a1 = halves(ops)
                pairs.append((CHRS.index(chrom), int(st), a0, pos, end0, a1, pos + end0 + n))
                seen["other_chr"] += chrom != p["chr"]
                assert int(st) == strand                    # an entry copies its first segment, whose strand is the read's
        entries = splice.multi_entries(pairs)
        assert len(entries) == len(pairs) - 1
        xa = [(CHRS[c], st, pos, cg) for c, st, pos, cg in entries]
        cigar = splice.merge_cigar(*pairs[0][2:])
        args = (p["name"], seq, qual, p["chr"], p["pos"], cigar, strand, int(p["tags"]["X0"]), int(p["tags"].get("X1", 0)),
                int(p["tags"]["XM"]))
        kw = dict(max_top2=opts["max_top2"], flag=p["flag"] & ~16, comp_read=bool(opts["mode"] & 2), clip_len=clip_len)
        assert sam.spliced_line(*args, xa=xa, **kw) == ln
        plain = sam.spliced_line(*args, **kw)
        assert plain == sam.spliced_line(*args, xa=[], **kw) == ln.split("\tXA:Z:")[0]      # without xa: as before
        seen["s"] += 1
        seen["xa"] += bool(xa)
        seen["entries"] += len(xa)
        seen["longest"] = max(seen["longest"], len(xa))
        seen["reverse"] += bool(xa) and strand
        seen["clipped_xa"] += bool(xa) and clip_len < len(seq)
        seen["max_x0"] = max(seen["max_x0"], int(p["tags"]["X0"]))
    print(case, seen)
    assert (seen["s"], seen["xa"], seen["entries"]) == (m["spliced"], m["with_XA"], m["xa_entries"])
    assert seen["longest"] == m["longest_list"] <= 49
    if case == "q15":
        assert seen["clipped_xa"] >= 5
    else:
        assert seen["xa"] >= 20 and seen["reverse"] and seen["xa"] > seen["reverse"] and seen["other_chr"] >= 5
        assert seen["longest"] >= 25 and seen["max_x0"] > 60


def test_entries_follow_the_sorted_pairs():
    """A tandem locus by hand: segment 0's rows and segment 1's at one distance, a nearer and
    a farther copy among them; multi_entries keeps pair_segments' order and drops pair 0."""
    from hsa_amd import splice
    R = lambda aln, chrom, occ: [aln, chrom, occ + 1, occ]
    rows = [R(0, 0, 9000), R(0, 0, 1000), R(0, 1, 200), R(0, 0, 5000), R(0, 0, 20000),
            R(1, 0, 5300), R(1, 1, 500), R(1, 0, 1400), R(1, 0, 9300), R(1, 0, 20300)]
    n_res, idx = splice.pair_segments(np.array(rows, np.int64))
    # sorted: 200 (chr 1), 500, 1000, 1400 (d 400: dropped when 300 is met), 5000, 5300, ...
    assert n_res == 4 and idx == [2, 6, 3, 5, 0, 8, 4, 9]
    pairs = [(rows[idx[2 * p]][1], 0, [(0, 50)], rows[idx[2 * p]][2], 49, [(0, 50)], rows[idx[2 * p + 1]][2]) for p in range(n_res)]
    got = splice.multi_entries(pairs)
    assert got == [(0, 0, 5001, [(0, 50), (3, 251), (0, 50)]), (0, 0, 9001, [(0, 50), (3, 251), (0, 50)]),
                   (0, 0, 20001, [(0, 50), (3, 251), (0, 50)])]
    assert splice.multi_entries(pairs[:1]) == []


def test_split_entries_needs_the_length():
    got = split_entries("chrA,-16053549M765N51MchrB,+1065449M765N51M", 100)
    assert got == [("chrA", True, 160535, [(0, 49), (3, 765), (0, 51)]), ("chrB", False, 10654, [(0, 49), (3, 765), (0, 51)])]


# ---------------------------------------------------------------- header and bindings
DECLS = r"""
#include "hsa_gpu.h"
int (*p_xa)(hsa_index_t *, const hsa_splice_lines_batch_t *, const hsa_sam_trim_t *, const hsa_splice_xa_t *, void *) =
    hsa_splice_lines_device_xa;
_Static_assert(sizeof(hsa_splice_xa_t) == 40, "hsa_splice_xa_t layout");
_Static_assert(sizeof(hsa_splice_lines_batch_t) == 184, "hsa_splice_lines_batch_t layout");
_Static_assert(HSA_SL_XA_WORDS == 16 && HSA_SL_XA_UNUSED == 0xFFFFFFFFu && HSA_SL_ROW_WORDS == 24 && HSA_SL_MULTI == 4, "constants");
"""


def test_header_declares_the_entry_point(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(DECLS)
    r = subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "decl.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_struct_and_export_match_the_binding():
    from hsa_amd import _lib
    X = _lib.SpliceXa
    assert ctypes.sizeof(X) == 40
    assert (X.pair_cap.offset, X.d_pair_off.offset, X.d_pair_rows.offset, X.d_pair_cigar.offset, X.d_counters.offset) == (0, 8, 16, 24, 32)
    assert _lib.SL_XA_WORDS == 16 and _lib.HSA_SL_XA_UNUSED == 0xFFFFFFFF and ctypes.sizeof(_lib.SpliceLinesBatch) == 184
    assert os.path.exists(_lib.LIB_PATH), "build libhsa_gpu.so first"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hsa_splice_lines_device_xa") and "hsa_splice_lines_device_xa" in _lib.EXPORTS


def test_the_call_on_a_null_handle_fails_loudly():
    from hsa_amd import _lib
    L = _lib.lib()
    assert L.hsa_splice_lines_device_xa(None, None, None, None, None) == -2      # HSA_E_ARG (include/hsa_gpu.h)
    assert b"null" in L.hsa_last_error()
    gi = _lib.GpuIndex.__new__(_lib.GpuIndex)
    gi.h = None
    with pytest.raises(_lib.HsaError):
        gi.splice_lines(_lib.SpliceLinesBatch(), xa=_lib.SpliceXa())


def test_the_index_fits_beside_the_tiny_one():
    for e, digest in MAN["index_sha256"].items():
        path = os.path.join(GOLD, "index", f"dup.fa.index.{e}")
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == digest
        assert os.path.getsize(path) <= max(os.path.getsize(os.path.join(GOLD, "index", f"tiny.fa.index.{e}")), 64)
