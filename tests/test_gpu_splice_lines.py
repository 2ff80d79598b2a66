"""Spliced reads through hsa_amd.align with splice=True: the committed splice reads against
the compiled reference's SAM (whole lines, file order, XT:A:S lines among them), the default
left as it is, the rows of hsa_splice_lines_device against the Python restatements
(hsa_amd.splice.pair_segments over positions from hsa_sa_position_batch, the reference's own
CIGARs), batching and the hand-over to the host parser, capacity and argument checks."""
import gzip
import hashlib
import io
import json
import os
import re

import numpy as np
import pytest

from golden_io import GOLD, INDEX

pytestmark = pytest.mark.gpu
MAN = json.load(open(os.path.join(GOLD, "manifest_dropin.json")))
CASES = [("splice_default", "splice_reads", 200), ("splice_n4o1", "splice_reads", 280), ("default", "reads", 50)]
_RUN = {}


@pytest.fixture(scope="module")
def opened():
    from hsa_amd import align
    gi, chrs = align.open_index64(INDEX["tiny"])
    yield gi, chrs
    gi.close()


def fastq_bytes(key):
    return gzip.open(os.path.join(GOLD, MAN[key])).read()


def reference(name):
    return gzip.open(os.path.join(GOLD, f"dropin_ref_{name}.sam.gz")).read().decode().splitlines()


def run(opened, name, reads_key, data=None, record=None, **kw):
    """align_fastq with splice=True; record: a list that receives the arguments and outputs
    of every chain.splice_lines call."""
    from hsa_amd import align, chain
    gi, chrs = opened
    opts = align.parse_options(MAN[name]["args"] if isinstance(name, str) else name)[0]
    out = io.BytesIO()
    real = chain.splice_lines

    def spy(gi_, b, s, first, n, strings, n_chr, max_line, out_cap, **k2):
        o, ctr = real(gi_, b, s, first, n, strings, n_chr, max_line, out_cap, **k2)
        record.append(dict(b=b, s=s, first=first, n=n, strings=strings, n_chr=n_chr, max_line=max_line, kw=k2, o=o, ctr=ctr))
        return o, ctr
    if record is not None:
        chain.splice_lines = spy
    try:
        state, stats = align.align_fastq(gi, chrs, fastq_bytes(reads_key) if data is None else data, opts, out, splice=True, **kw)
    finally:
        chain.splice_lines = real
    return out.getvalue(), state, stats


def whole(opened, name, reads_key):
    if name not in _RUN:
        rec = []
        _RUN[name] = run(opened, name, reads_key, record=rec) + (rec,)
    return _RUN[name]


# ---------------------------------------------------------------- 1. whole files
@pytest.mark.parametrize("name,reads_key,min_s", CASES)
def test_whole_files_against_the_reference(opened, name, reads_key, min_s):
    want = reference(name)
    assert len(want) == MAN[name]["sam_lines"] and all(re.search(r"\tXT:A:[URS]", ln) for ln in want)
    text, _, stats, _ = whole(opened, name, reads_key)
    assert text.endswith(b"\n")
    lines = text.decode().split("\n")[:-1]
    pos = {ln: k for k, ln in enumerate(want)}
    assert len(pos) == len(want)
    bad = [ln for ln in lines if ln not in pos]
    assert not bad, f"{len(bad)} of {len(lines)} printed lines are not reference lines, first:\n{bad[0]}"
    where = [pos[ln] for ln in lines]
    assert where == sorted(where) and len(set(where)) == len(where)              # the reference's order, each once
    missing = {ln.split("\t")[0] for ln in want} - {ln.split("\t")[0] for ln in lines}
    refused = {nm.decode() for nm in stats["refused_names"]}
    n_refused = stats["handed_back"] + stats["spliced_multi"] + stats["spliced_refused"]
    n_s = sum("\tXT:A:S" in ln for ln in lines)
    print(f"{name}: {len(lines)} of {len(want)} lines, {n_s} S lines, sent {stats['spliced_sent']}, handed back "
          f"{stats['handed_back']}, multi {stats['spliced_multi']}, refused {stats['spliced_refused']}, no pair "
          f"{stats['spliced_no_pair']}, unspliced results {stats['spliced_unspliced']}, missing {sorted(missing)}")
    assert len(refused) == n_refused
    assert missing <= refused, f"reference lines of reads that were not refused are missing: {sorted(missing - refused)}"
    assert n_refused <= 0.05 * stats["spliced_sent"]
    assert n_s >= min_s
    assert stats["lines"] == len(lines) and stats["no_line"] == stats["reads"] - len(lines)
    if n_refused == 0:
        assert hashlib.sha256(text).hexdigest() == MAN[name]["sam_sha256"]


def test_too_many_score_buckets_are_refused(opened):
    from hsa_amd import align
    gi, chrs = opened
    opts = align.parse_options(MAN["splice_n4o1O120"]["args"])[0]
    out = io.BytesIO()
    with pytest.raises(ValueError, match="not built"):
        align.align_fastq(gi, chrs, fastq_bytes("splice_reads"), opts, out, splice=True)
    assert out.getvalue() == b""


# ---------------------------------------------------------------- 2. the default
def test_default_is_unchanged(opened):
    from hsa_amd import align
    gi, chrs = opened
    got = []
    for kw in ({}, dict(splice=False)):
        out = io.BytesIO()
        state, stats = align.align_fastq(gi, chrs, fastq_bytes("splice_reads"), align.parse_options([])[0], out, **kw)
        got.append((out.getvalue(), state, stats))
    assert got[0] == got[1]
    assert not [k for k in got[0][2] if "splice" in k or k in ("handed_back", "refused_names")]
    lines = got[0][0].decode().split("\n")[:-1]
    assert lines and not [ln for ln in lines if "\tXT:A:S" in ln]
    text, _, stats, _ = whole(opened, "splice_default", "splice_reads")
    assert set(stats) > set(got[0][2]) and len(text) > len(got[0][0])
    from test_gpu_align import golden_text
    want = golden_text(opened, "default")                               # (the drop-in reads, as tests/test_gpu_align.py runs them)
    out = io.BytesIO()
    state, stats = align.align_fastq(gi, chrs, fastq_bytes("reads"), align.parse_options(MAN["default"]["args"])[0], out,
                                     splice=False)
    assert (out.getvalue(), state, stats) == want and list(stats) == list(want[2])


# ---------------------------------------------------------------- 3. the stage's rows
def parse_cigar(c):
    return [("MIDNSHP=X".index(o), int(l)) for l, o in re.findall(r"(\d+)([MIDNSHP=X])", c)]


def test_stage_rows_against_the_restatement(opened):
    from hsa_amd import splice
    from hsa_amd._lib import HSA_SL_OK, SL_ROW_WORDS, SP_RES_WORDS
    gi, _ = opened
    text, _, _, rec = whole(opened, "splice_n4o1", "splice_reads")
    by_name = {ln.split("\t")[0]: ln.split("\t") for ln in reference("splice_n4o1")}
    printed = {ln.split("\t")[0]: ln for ln in text.decode().split("\n")[:-1]}
    seen = dict(ok=0, many_rows=0, strand1=0, d_dropped=0, interior_s=0)
    for call in rec:
        n, o = call["n"], call["o"]
        rows = o["rows"].cpu().numpy().view(np.uint32).reshape(-1, SL_ROW_WORDS)[:n]
        cig = o["cigar"].cpu().numpy().view(np.uint32).reshape(-1, o["cigar_stride"])[:n]
        stat = o["stat"].cpu().numpy().view(np.uint32)[:n]
        ks = call["first"] - call["s"]["sp_first"]
        res = call["s"]["res"].cpu().numpy().view(np.uint32).reshape(-1, SP_RES_WORDS)[ks:ks + n]
        noff = call["strings"]["name_off"][:n + 1].cpu().numpy().view(np.uint64)
        names = call["strings"]["names"].cpu().numpy().tobytes()
        assert np.array_equal(rows[:, 0], stat)
        for j in np.flatnonzero(stat == HSA_SL_OK):
            name = names[int(noff[j]):int(noff[j + 1])].decode()
            r0, r1, row = res[j, 2:11], res[j, 11:20], rows[j]
            k0, l0, k1, l1 = int(r0[1]), int(r0[2]), int(r1[1]), int(r1[2])
            n0, n1 = splice.segment_rows(k0, l0), splice.segment_rows(k1, l1)
            idx = np.array(list(range(k0, k0 + n0)) + list(range(k1, k1 + n1)), np.uint32)
            p = gi.sa_positions(idx)
            found = p[:, 1] != 0xFFFFFFFF
            table = np.stack([(np.arange(len(idx)) >= n0).astype(np.int64), np.where(found, p[:, 1], 0).astype(np.int64),
                              np.where(found, p[:, 2], 0).astype(np.int64), p[:, 3].astype(np.int64)], axis=1)
            n_res, pair = splice.pair_segments(table)
            assert (int(row[1]), int(row[2]), int(row[3])) == (n0 + n1, n_res, splice.capped_multi(k0, l0, k1, l1)) and n_res == 1
            strand = int(r0[5]) >> 30
            assert int(row[4]) == strand
            ref = by_name[name]
            ops = parse_cigar(ref[5])
            at = [k for k, (op, _) in enumerate(ops) if op == 3][0]
            shifts = []
            for s, rr in ((0, r0), (1, r1)):
                a = table[pair[s]]
                chrom, ori, occ, start, end, mm = (int(v) for v in row[6 + 6 * s:12 + 6 * s])
                d5, d3 = start - int(rr[6]), int(rr[7]) - end
                assert chrom == a[1] and d5 >= 0 and d3 >= 0 and ori - a[2] == d5 and occ - a[3] == d5      # the leading-D rule
                assert mm == (int(rr[0]) & 0xFFFF) + ((int(rr[0]) >> 16) & 0xFF) + (int(rr[0]) >> 24)
                seg_ops = ops[:at] if s == 0 else ops[at + 1:]
                # the ops cover the segment as the search gave it (start and end then move by the
                # dropped D lengths, which are reference characters: they bound no part of the read)
                assert sum(l for op, l in seg_ops if op in (0, 1, 4)) == int(rr[7]) - int(rr[6]) + 1
                shifts += [d5, d3]
            merged = splice.merge_cigar(ops[:at], int(row[7]), int(row[10]), ops[at + 1:], int(row[13]))
            assert merged == ops and int(row[18]) == ops[at][1] and int(row[5]) == len(ops)
            assert [(int(w) >> 28, int(w) & 0x0FFFFFFF) for w in cig[j, :len(ops)]] == ops
            assert int(row[7]) == int(ref[3]) and int(row[19]) == int([t for t in ref if t.startswith("XM:i:")][0][5:])
            assert printed[name] == "\t".join(ref)
            seen["ok"] += 1
            seen["many_rows"] += n0 + n1 > 2
            seen["strand1"] += strand
            seen["d_dropped"] += any(shifts)
            seen["interior_s"] += any(op == 4 for op, _ in ops[1:-1])
    print(seen)
    # (every spliced read of the fixtures has one row per segment -- the 200 kbp genome has no
    # repeats of a segment's length --, so reads with more rows are made below)
    assert seen["ok"] >= 280 and seen["strand1"] and seen["interior_s"] and seen["d_dropped"]


def test_pairing_over_many_rows(opened):
    """The fixtures' spliced results with their SA intervals widened by neighbouring rows (rows
    of other positions: up to 50 per segment, 100 in all), so that the sort and the combine
    loop run: n_rows, n_splice, c1 and the status against pair_segments over positions from
    hsa_sa_position_batch; where the pair stays the true one, the line against spliced_line
    with the reference line's fields and X0 = X1 = the capped row count."""
    import torch

    from hsa_amd import chain, sam, splice
    from hsa_amd._lib import (HSA_SL_INPUT, HSA_SL_INTRON, HSA_SL_MULTI, HSA_SL_NOPAIR, HSA_SL_OK, HSA_SL_POS, HSA_SL_REFINE,
                              SL_ROW_WORDS, SP_RES_WORDS)
    gi, _ = opened
    c = first_call(opened)
    n = c["n"]
    ks = c["first"] - c["s"]["sp_first"]
    res = c["s"]["res"].cpu().numpy().view(np.uint32).reshape(-1, SP_RES_WORDS).copy()
    stat0 = c["o"]["stat"].cpu().numpy().view(np.uint32)[:n]
    rng = np.random.default_rng(3)
    picked = [int(j) for j in np.flatnonzero(stat0 == HSA_SL_OK)[:120]]
    true_rows = {}
    for q, j in enumerate(picked):
        r = res[ks + j]
        widen = [(q % 3 != 1), (q % 3 != 0)]                       # segment 0, segment 1 or both
        at = []
        for s in (0, 1):
            k = int(r[2 + 9 * s + 1])
            assert k == int(r[2 + 9 * s + 2])
            lo = hi = 0
            if widen[s]:
                lo, hi = (int(v) for v in rng.integers(0, 60 if q % 5 == 0 else 6, 2))
            if q % 15 == 5:
                lo = hi = 30                                        # 50 rows of each segment: the cap of 100
            if q % 15 == 7:                                         # segment 1 somewhere else: most such reads pair no rows
                k = 1 + (k + 7919 * q) % (gi.T - 1) if s else k
                lo, hi = (0, 0) if s else (1, 1)
            k_new, l_new = max(1, k - lo), min(gi.T, k + hi)
            r[2 + 9 * s + 1], r[2 + 9 * s + 2] = k_new, l_new
            at.append(k - k_new)
        true_rows[j] = None if q % 15 == 7 else at
    s2 = dict(c["s"], res=torch.from_numpy(res.view(np.int32).reshape(-1)).cuda())
    lb, o = chain.splice_lines_batch(c["b"], s2, c["first"], n, c["strings"], c["n_chr"], c["max_line"], int(c["ctr"][0]) + 4096,
                                     **c["kw"])
    torch.cuda.synchronize()
    gi.splice_lines(lb)
    torch.cuda.synchronize()
    rows = o["rows"].cpu().numpy().view(np.uint32).reshape(-1, SL_ROW_WORDS)[:n]
    stat = o["stat"].cpu().numpy().view(np.uint32)[:n]
    off = o["line_off"].cpu().numpy().view(np.uint64)
    text = o["out"].cpu().numpy().tobytes()
    noff = c["strings"]["name_off"][:n + 1].cpu().numpy().view(np.uint64)
    names = c["strings"]["names"].cpu().numpy().tobytes()
    by_name = {ln.split("\t")[0]: ln.split("\t") for ln in reference("splice_n4o1")}
    codes = c["b"]["codes"].cpu().numpy()
    jobs = np.frombuffer(c["b"]["jobs"].cpu().numpy().tobytes()[:(c["first"] + n) * 24], dtype=[("off", "<u8"), ("len", "<u4"), ("x", "<i4", 3)])
    untouched = np.setdiff1d(np.arange(n), picked)
    assert np.array_equal(stat[untouched], stat0[untouched])
    seen = dict(true_pair=0, other_pair=0, no_pair=0, multi=0, capped=0, sorted_differs=0, most_rows=0)
    for j in picked:
        r0, r1, row = res[ks + j, 2:11], res[ks + j, 11:20], rows[j]
        k0, l0, k1, l1 = int(r0[1]), int(r0[2]), int(r1[1]), int(r1[2])
        n0, n1 = splice.segment_rows(k0, l0), splice.segment_rows(k1, l1)
        idx = np.array(list(range(k0, k0 + n0)) + list(range(k1, k1 + n1)), np.uint32)
        p = gi.sa_positions(idx)
        found = p[:, 1] != 0xFFFFFFFF
        table = np.stack([(np.arange(len(idx)) >= n0).astype(np.int64), np.where(found, p[:, 1], 0).astype(np.int64),
                          np.where(found, p[:, 2], 0).astype(np.int64), p[:, 3].astype(np.int64)], axis=1)
        n_res, pair = splice.pair_segments(table)
        c1 = splice.capped_multi(k0, l0, k1, l1)
        assert (int(row[1]), int(row[2]), int(row[3])) == (n0 + n1, n_res, c1), j
        seen["capped"] += c1 == 100
        seen["most_rows"] = max(seen["most_rows"], n0 + n1)
        seen["sorted_differs"] += list(np.argsort(table[:, 3], kind="stable")) != list(range(len(table)))
        if n_res != 1:
            assert stat[j] == (HSA_SL_NOPAIR if n_res == 0 else HSA_SL_MULTI) and off[j + 1] == off[j]
            seen["no_pair" if n_res == 0 else "multi"] += 1
            continue
        a, b = table[pair[0]], table[pair[1]]
        if not (found[pair[0]] and found[pair[1]]) or a[1] != b[1]:
            assert stat[j] == HSA_SL_POS
            continue
        assert stat[j] in (HSA_SL_OK, HSA_SL_REFINE, HSA_SL_INTRON, HSA_SL_INPUT)
        is_true = true_rows[j] is not None and pair == [true_rows[j][0], n0 + true_rows[j][1]]
        seen["true_pair" if is_true else "other_pair"] += 1
        if stat[j] == HSA_SL_OK:
            for s, rr, z in ((0, r0, a), (1, r1, b)):
                chrom, ori, occ, start, end, mm = (int(v) for v in row[6 + 6 * s:12 + 6 * s])
                d5 = start - int(rr[6])
                assert chrom == z[1] and d5 >= 0 and ori - z[2] == d5 and occ - z[3] == d5
        if is_true:
            assert stat[j] == HSA_SL_OK
            ref = by_name[names[int(noff[j]):int(noff[j + 1])].decode()]
            J = jobs[c["first"] + j]
            strand = 1 if int(ref[1]) & 16 else 0
            want = sam.spliced_line(ref[0], codes[int(J["off"]):int(J["off"]) + int(J["len"])],
                                    ref[10][::-1] if strand else ref[10], ref[2], int(ref[3]), parse_cigar(ref[5]), strand, c1, c1,
                                    int([t for t in ref if t.startswith("XM:i:")][0][5:]), max_top2=c["kw"]["max_top2"])
            assert text[int(off[j]):int(off[j + 1])].decode() == want + "\n", j
    print(seen)
    assert seen["true_pair"] >= 20 and seen["sorted_differs"] >= 20 and seen["capped"] >= 1 and seen["most_rows"] == 100
    assert seen["other_pair"] >= 1 and seen["no_pair"] >= 1


# ---------------------------------------------------------------- 4. batching and hand-over
def test_batches_of_100_reads_give_the_same_text(opened):
    """-n 4 -o 0, as tests/test_gpu_align.py batches: no gap opens, so the GAPE bit that only the
    first batch's local options keep cannot matter, and -n 4 fixes the thresholds."""
    args = ["-n", "4", "-o", "0"]
    want, want_state, one = run(opened, args, "splice_reads")
    text, state, stats = run(opened, args, "splice_reads", batch_reads=100)
    assert one["batches"] == 1 and stats["batches"] == 8 and one["spliced"] >= 100
    assert text == want and state == want_state
    for k in ("spliced", "handed_back", "spliced_multi", "spliced_refused", "spliced_no_pair", "lines"):
        assert stats[k] == one[k], k


def test_every_seventh_record_through_the_host_parser(opened):
    ls = fastq_bytes("splice_reads").split(b"\n")
    recs = []
    for k in range(0, len(ls) - 3, 4):
        h, s, p, q = ls[k:k + 4]
        recs.append(h + b"\n" + (s[:20] + b"\n" + s[20:] if (k // 4) % 7 == 3 else s) + b"\n" + p + b"\n" + q + b"\n")
    text, state, stats = run(opened, "splice_n4o1", "splice_reads", data=b"".join(recs))
    want, want_state, _, _ = whole(opened, "splice_n4o1", "splice_reads")
    assert stats["host_records"] == len(range(3, 720, 7))
    assert text == want and state == want_state


def test_unaligned_and_printed_names_partition_the_reads(opened):
    from hsa_amd import reads
    un = io.BytesIO()
    text, _, stats = run(opened, "splice_n4o1", "splice_reads", unaligned=un)
    assert text == whole(opened, "splice_n4o1", "splice_reads")[0]
    with_line = [ln.split(b"\t")[0] for ln in text.split(b"\n")[:-1]]
    every = reads.parse_host(fastq_bytes("splice_reads"))["names"]
    without = reads.parse_host(un.getvalue())["names"]
    assert len(set(with_line)) == len(with_line) and len(without) == stats["no_line"]
    assert without == [nm for nm in every if nm not in set(with_line)] and len(with_line) + len(without) == len(every)


# ---------------------------------------------------------------- 5. capacity and arguments
def first_call(opened):
    rec = whole(opened, "splice_n4o1", "splice_reads")[3]
    return max(rec, key=lambda c: int(c["ctr"][2]))


def again(gi, c, out_cap, fill=None):
    import torch

    from hsa_amd import chain
    lb, o = chain.splice_lines_batch(c["b"], c["s"], c["first"], c["n"], c["strings"], c["n_chr"], c["max_line"], out_cap, **c["kw"])
    if fill is not None:
        o["out"] = torch.full((fill,), 0x23, dtype=torch.uint8, device="cuda")
        lb.d_out = o["out"].data_ptr()
    torch.cuda.synchronize()
    gi.splice_lines(lb)
    torch.cuda.synchronize()
    return lb, o, o["ctr"].cpu().numpy().view(np.uint64)


def test_capacity_repeat_and_scratch_release(opened):
    gi, _ = opened
    c = first_call(opened)
    total = int(c["ctr"][0])
    want = c["o"]["out"][:total].cpu().numpy().tobytes()
    assert total > 4000 and int(c["ctr"][1]) == total
    cap = total // 2 + 5
    _, o, ctr = again(gi, c, cap, fill=total + 64)
    got = o["out"].cpu().numpy().tobytes()
    assert int(ctr[0]) == total and int(ctr[1]) == cap                           # wanted > written
    assert got[:cap] == want[:cap] and got[cap:] == b"#" * (total + 64 - cap)     # no byte at or past the cap
    _, o2, ctr2 = again(gi, c, total)
    assert o2["out"][:total].cpu().numpy().tobytes() == want and np.array_equal(ctr2, c["ctr"])
    assert np.array_equal(o2["line_off"].cpu().numpy(), c["o"]["line_off"].cpu().numpy())
    assert np.array_equal(o["line_off"].cpu().numpy(), c["o"]["line_off"].cpu().numpy())
    gi.release_scratch()
    _, o3, ctr3 = again(gi, c, total)
    for k in ("out", "line_off", "stat", "rows", "cigar"):
        assert np.array_equal(o3[k].cpu().numpy(), o2[k].cpu().numpy()), k
    assert np.array_equal(ctr3, ctr2)


def test_null_pointers_and_a_long_text_are_refused(opened):
    import ctypes

    import torch

    from hsa_amd import _lib
    from hsa_amd._lib import GpuIndex, HsaError
    gi, _ = opened
    c = first_call(opened)
    for field in ("d_jobs", "d_codes", "d_flags", "d_n_aln", "d_res", "d_names", "d_name_off", "d_rows", "d_line_stat",
                  "d_line_off", "d_counters", "d_out", "d_chr_off"):
        lb, o, _ = again(gi, c, 64)
        setattr(lb, field, None)
        assert _lib.lib().hsa_splice_lines_device(gi.h, ctypes.byref(lb), None) == -2, field
    lb, o, _ = again(gi, c, 64)
    lb.d_qual_off = None
    with pytest.raises(HsaError):
        gi.splice_lines(lb)
    assert _lib.lib().hsa_splice_lines_device(gi.h, None, None) == -2
    # a handle of 2^32 + 64 characters (its rank blocks are never read: the call stops at the handle)
    T = (1 << 32) + 64
    words = torch.zeros(T // 16 + 8, dtype=torch.int32, device="cuda")
    Cc = np.array([0, T, T, T, T], np.uint64)
    big = GpuIndex.from_device_codes64(T, 1, Cc, words.data_ptr(), T, 1, Cc, words.data_ptr())
    try:
        assert big.is64()
        lb, o, _ = again(gi, c, 64)
        with pytest.raises(HsaError, match="2\\^32"):
            big.splice_lines(lb)
    finally:
        big.close()
    torch.cuda.synchronize()


def test_merge_of_two_writers(opened):
    """hsa_sam_merge_device on hand-made texts: 300 reads, a line from writer a, from writer b
    or from neither, of 1 to 400 bytes (both the 16-byte and the byte path, every alignment);
    then with room for half, and with null pointers."""
    import ctypes

    import torch

    from hsa_amd import _lib, chain
    gi, _ = opened
    rng = np.random.default_rng(9)
    n = 300
    who = rng.integers(0, 3, n)                                     # 0 none, 1 a, 2 b
    lens = rng.integers(1, 401, n)
    la, lb_ = np.where(who == 1, lens, 0), np.where(who == 2, lens, 0)
    off = lambda l: np.concatenate([[0], np.cumsum(l)]).astype(np.uint64)
    oa, ob = off(la), off(lb_)
    ta = rng.integers(33, 127, int(oa[-1]), dtype=np.uint8)
    tb = rng.integers(33, 127, int(ob[-1]), dtype=np.uint8)
    want = b"".join((ta[int(oa[j]):int(oa[j + 1])].tobytes() + tb[int(ob[j]):int(ob[j + 1])].tobytes()) for j in range(n))
    up = chain.to_device
    a = (up(ta), len(ta), up(oa))
    b = (up(tb), len(tb), up(ob))
    o, ctr = chain.sam_merge(gi, n, a, b)
    assert int(ctr[0]) == int(ctr[1]) == len(want) and o["out"][:len(want)].cpu().numpy().tobytes() == want
    assert np.array_equal(o["line_off"].cpu().numpy().view(np.uint64), off(la + lb_))
    cap = len(want) // 2 + 3
    mb, o2 = chain.sam_merge_batch(n, a, b)
    o2["out"] = torch.full((len(want) + 32,), 0x23, dtype=torch.uint8, device="cuda")
    mb.d_out, mb.out_cap = o2["out"].data_ptr(), cap
    torch.cuda.synchronize()
    gi.sam_merge(mb)
    torch.cuda.synchronize()
    got = o2["out"].cpu().numpy().tobytes()
    c2 = o2["ctr"].cpu().numpy().view(np.uint64)
    assert int(c2[0]) == len(want) and int(c2[1]) == cap and got[:cap] == want[:cap] and got[cap:] == b"#" * (len(got) - cap)
    for field in ("d_line_off_a", "d_line_off_b", "d_text_a", "d_text_b", "d_line_off", "d_out", "d_counters"):
        mb, _ = chain.sam_merge_batch(n, a, b)
        setattr(mb, field, None)
        assert _lib.lib().hsa_sam_merge_device(gi.h, ctypes.byref(mb), None) == -2, field
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. results with n_aln == 1
def test_unspliced_results_print_as_u_or_r_lines(opened):
    """A splice result that is not two records of type 4 goes through choose, refine and
    k_sam_write like a main-search hit.  The count over the three fixtures is printed; where
    there are any, those reads' reference lines are among the printed ones (test 1 holds
    every printed line to the reference and every missing one to a refusal)."""
    total = 0
    for name, reads_key, _ in CASES:
        text, _, stats, _ = whole(opened, name, reads_key)
        total += stats["spliced_unspliced"]
        print(name, "unspliced splice results:", stats["spliced_unspliced"])
    from hsa_amd import align
    gi, chrs = opened
    for name, reads_key, _ in CASES:
        out = io.BytesIO()
        _, st0 = align.align_fastq(gi, chrs, fastq_bytes(reads_key), align.parse_options(MAN[name]["args"])[0], out)
        text, _, stats, _ = whole(opened, name, reads_key)
        ur = lambda t: sum(1 for ln in t.decode().split("\n") if "\tXT:A:U" in ln or "\tXT:A:R" in ln)
        assert ur(text) == ur(out.getvalue()) + stats["spliced_unspliced"]
    print("total", total)
