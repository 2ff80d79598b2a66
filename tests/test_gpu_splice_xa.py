"""Spliced reads with several splice pairs through hsa_amd.align with splice=True on the dup
genome (tools/make_golden_dup.py): whole files against the compiled reference's SAM (XA:Z
lists on XT:A:S lines), the rows of hsa_splice_lines_device_xa against the Python
restatements (hsa_amd.splice.pair_segments over positions from hsa_sa_position_batch,
hsa_amd.sam.spliced_line), the room for extra pairs, and the paths that must not change."""
import gzip
import hashlib
import io
import json
import os

import numpy as np
import pytest

from golden_io import GOLD, INDEX
from test_splice_xa_cpu import CHRS, halves, parse_cigar, split_entries

pytestmark = pytest.mark.gpu
MAN = json.load(open(os.path.join(GOLD, "manifest_dup.json")))
TINY = json.load(open(os.path.join(GOLD, "manifest_dropin.json")))
CASES = ["default", "n4o1", "q15"]
_RUN = {}


@pytest.fixture(scope="module")
def opened():
    from hsa_amd import align
    gi, chrs = align.open_index64(os.path.join(GOLD, "index", "dup.fa"))
    assert chrs == CHRS
    yield gi, chrs
    gi.close()


def reads_bytes(case):
    return gzip.open(os.path.join(GOLD, MAN["files"][MAN[case]["reads"]])).read()


def reference(case):
    return gzip.open(os.path.join(GOLD, f"dup_ref_{case}.sam.gz")).read().decode().splitlines()


def run(opened, args, data, record=None, **kw):
    """align_fastq with splice=True; record: a list that receives the arguments and outputs
    of every chain.splice_lines call."""
    from hsa_amd import align, chain
    gi, chrs = opened
    opts = align.parse_options(args, reader_options=True)[0]
    out = io.BytesIO()
    real = chain.splice_lines

    def spy(gi_, b, s, first, n, strings, n_chr, max_line, out_cap, **k2):
        o, ctr = real(gi_, b, s, first, n, strings, n_chr, max_line, out_cap, **k2)
        record.append(dict(b=b, s=s, first=first, n=n, strings=strings, n_chr=n_chr, max_line=max_line, kw=k2, o=o, ctr=ctr))
        return o, ctr
    if record is not None:
        chain.splice_lines = spy
    try:
        state, stats = align.align_fastq(gi, chrs, data, opts, out, splice=True, **kw)
    finally:
        chain.splice_lines = real
    return out.getvalue(), state, stats


def whole(opened, case):
    if case not in _RUN:
        rec = []
        _RUN[case] = run(opened, MAN[case]["args"], reads_bytes(case), record=rec) + (rec,)
    return _RUN[case]


# ---------------------------------------------------------------- 1. whole files
@pytest.mark.parametrize("case", CASES)
def test_whole_files_against_the_reference(opened, case):
    want = reference(case)
    assert len(want) == MAN[case]["sam_lines"]
    text, _, stats, _ = whole(opened, case)
    assert text.endswith(b"\n") and b"\0" not in text
    lines = text.decode().split("\n")[:-1]
    pos = {ln: k for k, ln in enumerate(want)}
    assert len(pos) == len(want)
    bad = [ln for ln in lines if ln not in pos]
    assert not bad, f"{len(bad)} of {len(lines)} printed lines are not reference lines, first:\n{bad[0]}"
    where = [pos[ln] for ln in lines]
    assert where == sorted(where) and len(set(where)) == len(where)              # the reference's order, each once
    missing = {ln.split("\t")[0] for ln in want} - {ln.split("\t")[0] for ln in lines}
    refused = {nm.decode() for nm in stats["refused_names"]}
    n_refused = stats["handed_back"] + stats["spliced_refused"]
    want_xa = [ln for ln in want if "\tXT:A:S" in ln and "\tXA:Z:" in ln]
    got_xa = [ln for ln in lines if "\tXT:A:S" in ln and "\tXA:Z:" in ln]
    print(f"{case}: {len(lines)} of {len(want)} lines, with XA {len(got_xa)} of {len(want_xa)}, entries {stats['spliced_xa_entries']}, "
          f"sent {stats['spliced_sent']}, handed back {stats['handed_back']}, multi {stats['spliced_multi']}, refused "
          f"{stats['spliced_refused']}, no pair {stats['spliced_no_pair']}, missing {sorted(missing)}")
    assert stats["spliced_multi"] == 0
    assert len(refused) == n_refused
    assert missing <= refused, f"reference lines of reads that were not refused are missing: {sorted(missing - refused)}"
    assert n_refused <= 0.05 * stats["spliced_sent"]
    assert len(want_xa) == MAN[case]["with_XA"] and len(got_xa) >= 0.9 * len(want_xa)
    assert stats["spliced_xa"] == len(got_xa)
    assert stats["spliced_xa_entries"] == sum(len(split_entries(ln.split("\tXA:Z:")[1], int(dict((t[:2], t[5:]) for t in
                                              ln.split("\t")[11:]).get("XC", 100)))) for ln in got_xa)
    assert stats["lines"] == len(lines) and stats["no_line"] == stats["reads"] - len(lines)
    if n_refused == 0:
        assert hashlib.sha256(text).hexdigest() == MAN[case]["sam_sha256"]


# ---------------------------------------------------------------- 2. the stage's rows
def big_call(opened, case="n4o1"):
    rec = whole(opened, case)[3]
    return max(rec, key=lambda c: int(c["o"]["xa"][3]))


def host(c, o=None):
    """The arrays of a recorded call (or of another run o of its batch) on the host."""
    from hsa_amd._lib import SL_ROW_WORDS, SL_XA_WORDS, SP_RES_WORDS
    o = c["o"] if o is None else o
    n = c["n"]
    ks = c["first"] - c["s"]["sp_first"]
    h = dict(rows=o["rows"].cpu().numpy().view(np.uint32).reshape(-1, SL_ROW_WORDS)[:n],
             stat=o["stat"].cpu().numpy().view(np.uint32)[:n], off=o["line_off"].cpu().numpy().view(np.uint64),
             text=o["out"].cpu().numpy().tobytes(),
             res=c["s"]["res"].cpu().numpy().view(np.uint32).reshape(-1, SP_RES_WORDS)[ks:ks + n],
             noff=c["strings"]["name_off"][:n + 1].cpu().numpy().view(np.uint64), names=c["strings"]["names"].cpu().numpy().tobytes())
    if "pair_off" in o:
        h.update(pair_off=o["pair_off"].cpu().numpy().view(np.uint64), prow=o["pair_rows"].cpu().numpy().view(np.uint32).reshape(-1, SL_XA_WORDS),
                 pcig=o["pair_cigar"].cpu().numpy().view(np.uint32).reshape(-1, o["cigar_stride"]))
    return h


def pairs_of(gi, res_j):
    """(n_rows, n_res, the pairs' rows as (aln_id, seq_id, ori_pos, occ_pos), found per row) of
    a read's two records, by pair_segments over hsa_sa_position_batch."""
    from hsa_amd import splice
    r0, r1 = res_j[2:11], res_j[11:20]
    k0, l0, k1, l1 = int(r0[1]), int(r0[2]), int(r1[1]), int(r1[2])
    n0, n1 = splice.segment_rows(k0, l0), splice.segment_rows(k1, l1)
    idx = np.array(list(range(k0, k0 + n0)) + list(range(k1, k1 + n1)), np.uint32)
    p = gi.sa_positions(idx)
    found = p[:, 1] != 0xFFFFFFFF
    table = np.stack([(np.arange(len(idx)) >= n0).astype(np.int64), np.where(found, p[:, 1], 0).astype(np.int64),
                      np.where(found, p[:, 2], 0).astype(np.int64), p[:, 3].astype(np.int64)], axis=1)
    n_res, pair = splice.pair_segments(table)
    moved = n_res and len(table) > 2 and pair[0] != sorted(range(len(table)), key=lambda r: int(table[r, 3]))[0]
    return n0 + n1, n_res, [table[k] for k in pair], splice.capped_multi(k0, l0, k1, l1), n0, n1, moved


def test_extra_pairs_against_the_restatement(opened):
    from hsa_amd import sam
    from hsa_amd._lib import HSA_SL_OK
    gi, _ = opened
    c = big_call(opened)
    h = host(c)
    by_name = {ln.split("\t")[0]: ln for ln in reference("n4o1")}
    codes = c["b"]["codes"].cpu().numpy()
    jobs = np.frombuffer(c["b"]["jobs"].cpu().numpy().tobytes()[:(c["first"] + c["n"]) * 24], dtype=[("off", "<u8"), ("len", "<u4"), ("x", "<i4", 3)])
    seen = dict(reads=0, entries=0, longest=0, capped=0, fifty=0, moved=0, other_chr=0, strand1=0)
    assert int(h["pair_off"][c["n"]]) == int(c["o"]["xa"][0]) == int(c["o"]["xa"][1]) <= c["o"]["pair_cap"]
    for j in np.flatnonzero(h["rows"][:, 2] > 1):
        row = h["rows"][j]
        n_rows, n_res, pr, c1, n0, n1, moved = pairs_of(gi, h["res"][j])
        assert (int(row[1]), int(row[2]), int(row[3])) == (n_rows, n_res, c1)
        e0, e1 = int(h["pair_off"][j]), int(h["pair_off"][j + 1])
        assert h["stat"][j] == HSA_SL_OK and e1 - e0 == n_res - 1 == int(row[22])
        name = h["names"][int(h["noff"][j]):int(h["noff"][j + 1])].decode()
        ref = by_name[name]
        f = ref.split("\t")
        entries = split_entries(ref.split("\tXA:Z:")[1], 100)
        assert len(entries) == n_res - 1
        strand = int(row[4])
        xa = []
        for q, (chrom, st, pos, ops) in enumerate(entries):
            w = h["prow"][e0 + q]
            a, b = pr[2 * (q + 1)], pr[2 * (q + 1) + 1]
            assert (int(w[0]), int(w[1]), int(w[12])) == (HSA_SL_OK, j, strand) and st == bool(strand)
            assert int(w[6]) == a[1] == b[1] == CHRS.index(chrom)
            d5 = int(w[7]) - int(w[15])
            assert int(w[15]) == a[2] and d5 >= 0 and int(w[8]) - a[3] == d5            # the leading-D rule
            assert int(w[7]) == pos
            got_ops = [(int(x) >> 28, int(x) & 0x0FFFFFFF) for x in h["pcig"][e0 + q, :int(w[4])]]
            assert got_ops == ops and int(w[5]) == halves(ops)[1] == int(w[10]) - int(w[7]) - int(w[9])
            assert int(w[13]) + 1 + int(w[14]) == int(w[4])
            xa.append((CHRS[int(w[6])], strand, int(w[7]), got_ops))
            seen["other_chr"] += chrom != f[2]
        assert sum(int(w[2]) for w in h["prow"][e0:e1]) == int(row[23]) == len(ref.split("\tXA:Z:")[1])
        J = jobs[c["first"] + j]
        want = sam.spliced_line(name, codes[int(J["off"]):int(J["off"]) + int(J["len"])], f[10][::-1] if strand else f[10], f[2],
                                int(f[3]), parse_cigar(f[5]), strand, c1, c1, int(row[19]), max_top2=c["kw"]["max_top2"], xa=xa)
        assert want == ref and h["text"][int(h["off"][j]):int(h["off"][j + 1])].decode() == ref + "\n"
        seen["reads"] += 1
        seen["entries"] += len(xa)
        seen["longest"] = max(seen["longest"], len(xa))
        seen["capped"] += c1 == 100
        seen["fifty"] += n0 == 50 and n1 == 50
        seen["moved"] += bool(moved)
        seen["strand1"] += strand
    print(seen)
    assert seen["reads"] >= 20 and seen["entries"] == int(c["o"]["xa"][3]) and seen["reads"] == int(c["o"]["xa"][2])
    assert seen["longest"] >= 25 and seen["capped"] and seen["fifty"] and seen["moved"] and seen["other_chr"] >= 5 and seen["strand1"]


# ---------------------------------------------------------------- 3. the room
def again(gi, c, out_cap, room=None, fill=None):
    """The recorded call's batch once more: through the plain entry points (room None) or with
    room for `room` extra pairs."""
    import torch

    from hsa_amd import chain
    lb, o = chain.splice_lines_batch(c["b"], c["s"], c["first"], c["n"], c["strings"], c["n_chr"], c["max_line"], out_cap, **c["kw"])
    xa = None
    if room is not None:
        xa, ox = chain.splice_xa_batch(c["n"], room, o["cigar_stride"])
        o.update(ox)
    if fill is not None:
        o["out"] = torch.full((fill,), 0x23, dtype=torch.uint8, device="cuda")
        lb.d_out = o["out"].data_ptr()
    torch.cuda.synchronize()
    gi.splice_lines(lb, trim=chain.sam_trim(chain.trim_views(c["b"], c["first"])), xa=xa)
    torch.cuda.synchronize()
    if xa is not None:
        o["xa"] = o["xa_ctr"].cpu().numpy().view(np.uint64)
    return o, o["ctr"].cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("case", ["n4o1", "q15"])
def test_room_for_no_extra_pair_then_for_all(opened, case):
    from hsa_amd._lib import HSA_SL_MULTI, HSA_SL_OK
    gi, _ = opened
    c = big_call(opened, case)
    h = host(c)
    total, wanted = int(c["ctr"][0]), int(c["o"]["xa"][0])
    want_text = h["text"][:total]
    multi = np.flatnonzero(h["rows"][:, 22] > 0)
    assert wanted >= 100 and int(c["ctr"][1]) == total and len(multi) >= 20
    # no room: wanted > room, those reads refused as the plain entry points refuse them
    o0, ctr0 = again(gi, c, total, room=0, fill=total + 64)
    h0 = host(c, o0)
    assert int(o0["xa"][0]) == wanted and int(o0["xa"][1]) == 0 and int(o0["xa"][2]) == 0 and int(o0["xa"][3]) == 0
    assert (h0["stat"][multi] == HSA_SL_MULTI).all() and (h0["off"][multi + 1] == h0["off"][multi]).all()
    assert int(ctr0[4]) == len(multi) and int(ctr0[2]) == int(c["ctr"][2]) - len(multi)
    others = np.setdiff1d(np.arange(c["n"]), multi)
    assert np.array_equal(h0["stat"][others], h["stat"][others])
    short = int(ctr0[0])
    assert short < total and h0["text"][short:] == b"#" * (total + 64 - short)
    assert b"".join(h0["text"][int(h0["off"][j]):int(h0["off"][j + 1])] for j in others) == h0["text"][:short] == \
        b"".join(h["text"][int(h["off"][j]):int(h["off"][j + 1])] for j in others)
    assert np.array_equal(h0["pair_off"], h["pair_off"])
    # room for half of them: reads are served in read order while their pairs fit
    half = wanted // 2
    o1, ctr1 = again(gi, c, total, room=half)
    h1 = host(c, o1)
    fits = h["pair_off"][multi + 1] <= half
    assert fits.any() and not fits.all() and int(o1["xa"][0]) == wanted and int(o1["xa"][1]) == half
    assert (h1["stat"][multi[fits]] == HSA_SL_OK).all() and (h1["stat"][multi[~fits]] == HSA_SL_MULTI).all()
    for j in multi[fits]:
        assert h1["text"][int(h1["off"][j]):int(h1["off"][j + 1])] == h["text"][int(h["off"][j]):int(h["off"][j + 1])]
    # the wanted room, with half the bytes: nothing at or past out_cap
    cap = total // 2 + 5
    o2, ctr2 = again(gi, c, cap, room=wanted, fill=total + 64)
    got = o2["out"].cpu().numpy().tobytes()
    assert int(ctr2[0]) == total and int(ctr2[1]) == cap and got[:cap] == want_text[:cap] and got[cap:] == b"#" * (total + 64 - cap)
    # ... and in full, twice: equal arrays
    o3, ctr3 = again(gi, c, total, room=wanted)
    o4, ctr4 = again(gi, c, total, room=wanted)
    assert o3["out"][:total].cpu().numpy().tobytes() == want_text and np.array_equal(ctr3, c["ctr"])
    assert np.array_equal(o3["xa"], c["o"]["xa"]) and np.array_equal(ctr3, ctr4)
    for k in ("out", "line_off", "stat", "rows", "cigar", "pair_off", "pair_rows", "pair_cigar", "xa_ctr"):
        assert np.array_equal(o3[k].cpu().numpy(), o4[k].cpu().numpy()), k
    # more room than wanted: the unused slots stay marked
    o5, ctr5 = again(gi, c, total, room=wanted + 37)
    assert o5["out"][:total].cpu().numpy().tobytes() == want_text
    assert (host(c, o5)["prow"][wanted:, 0] == 0xFFFFFFFF).all() and (host(c, o5)["prow"][:wanted, 0] == HSA_SL_OK).all()


# ---------------------------------------------------------------- 4. what must not change
def test_plain_entry_points_still_refuse(opened):
    from hsa_amd._lib import HSA_SL_MULTI
    gi, _ = opened
    c = big_call(opened)
    h = host(c)
    multi = np.flatnonzero(h["rows"][:, 2] > 1)
    o, ctr = again(gi, c, int(c["ctr"][0]))
    hp = host(c, o)
    assert (hp["stat"][multi] == HSA_SL_MULTI).all() and (hp["off"][multi + 1] == hp["off"][multi]).all()
    assert int(ctr[4]) == len(multi) and (hp["rows"][:, 22:] == 0).all()
    o0, ctr0 = again(gi, c, int(c["ctr"][0]), room=0)
    for k in ("out", "line_off", "stat", "rows", "cigar"):
        a, b = o[k].cpu().numpy(), o0[k].cpu().numpy()
        assert np.array_equal(a[:int(ctr[1])] if k == "out" else a, b[:int(ctr[1])] if k == "out" else b), k
    assert np.array_equal(ctr, ctr0)


def test_tiny_fixture_gives_the_plain_text():
    """No read of the tiny genome has two pairs: the new entry point's arrays are the plain one's."""
    from hsa_amd import align
    gi, chrs = align.open_index64(INDEX["tiny"])
    try:
        rec = []
        data = gzip.open(os.path.join(GOLD, TINY["splice_reads"])).read()
        text, _, stats = run((gi, chrs), TINY["splice_n4o1"]["args"], data, record=rec)
        assert stats["spliced"] >= 280 and stats["spliced_xa"] == 0 and stats["spliced_xa_entries"] == 0 and stats["spliced_multi"] == 0
        if stats["handed_back"] + stats["spliced_refused"] == 0:
            assert hashlib.sha256(text).hexdigest() == TINY["splice_n4o1"]["sam_sha256"]
        c = max(rec, key=lambda c: int(c["ctr"][2]))
        assert int(c["o"]["xa"][0]) == 0
        total = int(c["ctr"][0])
        o, ctr = again(gi, c, total)
        assert np.array_equal(ctr, c["ctr"]) and total > 4000
        for k in ("line_off", "stat", "rows", "cigar"):
            assert np.array_equal(o[k].cpu().numpy(), c["o"][k].cpu().numpy()), k
        assert o["out"][:total].cpu().numpy().tobytes() == c["o"]["out"][:total].cpu().numpy().tobytes()
    finally:
        gi.close()


def test_batches_of_100_reads_give_the_same_text(opened):
    """-n 4 -o 0, as tests/test_gpu_splice_lines.py batches (no gap opens, -n 4 fixes the thresholds)."""
    args = ["-n", "4", "-o", "0"]
    want, want_state, one = run(opened, args, reads_bytes("default"))
    text, state, stats = run(opened, args, reads_bytes("default"), batch_reads=100)
    assert one["batches"] == 1 and stats["batches"] == 7 and one["spliced_xa"] >= 20
    assert text == want and state == want_state
    for k in ("spliced", "spliced_xa", "spliced_xa_entries", "handed_back", "spliced_multi", "spliced_refused", "spliced_no_pair", "lines"):
        assert stats[k] == one[k], k
