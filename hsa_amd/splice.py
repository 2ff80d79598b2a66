"""The splice path's seed searches (bwt_splice_match, bwtgap.c:748-848) as one batch.

For a read that found no hit on either strand, bwt_splice_match searches up to six
seeds: for strand s (0 = the read, 1 = its reverse complement) and i = 0, 1, 2, the
seed of length seed_len = len // 3 (plus len % 3 for the last one) at offset
i * seed_len.  Its widths are those of the strand sequence's PREFIX of that length,
with width_seed aliased to width_back (bwtgap.c:804-809), and its options are the
batch's local_opt with GAPE cleared, max_gapo = max_gape = 0, max_diff =
max_seed_diff and seed_len = the seed's length (bwtgap.c:769-774, :802).  Which seeds
it asks for depends on earlier answers (bwtgap.c:821-847); all six are computed here,
in one GPU pass (the C drop-in does the same and answers bwt_splice_match from the
table, hsa_amd/csrc/bwtgap_gpu.c).
"""
from __future__ import annotations

import numpy as np

GAPE = 0x01
CALL_DTYPE = np.dtype([("read", "<i8"), ("i", "<i4"), ("strand", "<i4"), ("len", "<u4"), ("off", "<u8"),
                       ("wb_off", "<u8")])


def seed_options(local_opt: dict) -> dict:
    """The option block of the seed searches (bwtgap.c:769-774); seed_len per seed."""
    o = dict(local_opt)
    o["mode"] &= ~GAPE
    o["max_gapo"] = 0
    o["max_gape"] = 0
    o["max_diff"] = local_opt["max_seed_diff"]
    return o


def n_stacks_of(local_opt: dict) -> int:
    """aln_score(max_diff+1, max_gapo+1, max_gape+1) of local_opt: the batch stack
    every call shares (bwtaln.c:279, bwtgap.c:13-18)."""
    o = local_opt
    return (o["max_diff"] + 1) * o["s_mm"] + (o["max_gapo"] + 1) * o["s_gapo"] + (o["max_gape"] + 1) * o["s_gape"]


def revcomp_rows(a: np.ndarray) -> np.ndarray:
    """seq_reverse(len, seq, 1) (bwaseqio.c:73-84) of every row: codes > 3 are kept."""
    r = a[:, ::-1].copy()
    m = r < 4
    r[m] = 3 - r[m]
    return r


def seed_calls(lens, codes, reads, local_opt: dict, width_fn):
    """The six seed calls of every read in `reads` (indices into lens / codes), in read
    order, i = 0..5 within a read (bwtgap.c:797).

    width_fn(lens, codes) -> flat widths, 2 * (len + 1) words per sequence
    (bwt_cal_width type 1: hsa_width_batch on the GPU, or the oracle on the CPU).
    Returns dict(calls: CALL_DTYPE records, codes, widths (P, 2) int32, opt), or None."""
    lens = np.asarray(lens, np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)])
    reads = np.asarray(reads, np.int64)
    reads = reads[lens[reads] >= 3]
    if len(reads) == 0:
        return None
    groups = []
    for L in np.unique(lens[reads]):
        rr = reads[lens[reads] == L]
        L = int(L)
        sl = L // 3
        idx = offs[rr][:, None] + np.arange(L)[None, :]
        fwd = np.asarray(codes, np.uint8)[idx]
        strand_seq = (fwd, revcomp_rows(fwd))
        # prefix widths: per read and strand, prefixes of sl and of sl + L % 3
        ks = (0, 1) if L % 3 else (0,)
        pre_lens, pre_codes = [], []
        for s in (0, 1):
            for k in ks:
                la = sl + (L % 3 if k else 0)
                pre_lens.append(np.full(len(rr), la, np.uint32))
                pre_codes.append(strand_seq[s][:, :la].reshape(-1))
        w = np.asarray(width_fn(np.concatenate(pre_lens), np.concatenate(pre_codes)), np.uint32).view(np.int32)
        pw = {}
        o = 0
        for s in (0, 1):
            for k in ks:
                la = sl + (L % 3 if k else 0)
                n = len(rr) * 2 * (la + 1)
                pw[(s, k)] = w[o:o + n].reshape(len(rr), la + 1, 2)
                o += n
        groups.append((rr, L, sl, strand_seq, pw))
    # assemble calls in read order
    order = np.argsort(reads, kind="stable")
    per_read = {}
    for rr, L, sl, strand_seq, pw in groups:
        for j, r in enumerate(rr):
            per_read[int(r)] = (j, L, sl, strand_seq, pw)
    calls = np.zeros(6 * len(reads), CALL_DTYPE)
    c_codes, c_widths = [], []
    co = po = 0
    q = 0
    for r in reads[order]:
        j, L, sl, strand_seq, pw = per_read[int(r)]
        for i in range(6):
            s = i // 3
            la = sl + (L % 3 if i % 3 == 2 else 0)
            k = 1 if (i % 3 == 2 and L % 3) else 0
            c_codes.append(strand_seq[s][j, (i % 3) * sl:(i % 3) * sl + la])
            c_widths.append(pw[(s, k)][j])
            calls[q] = (r, i, s, la, co, po)
            co += la
            po += la + 1
            q += 1
    return dict(calls=calls, codes=np.concatenate(c_codes).astype(np.uint8),
                widths=np.concatenate(c_widths).astype(np.int32), opt=seed_options(local_opt))


def seed_calls_fixed(reads2d: np.ndarray, local_opt: dict, width_fn):
    """seed_calls for reads of one length given as an (n, L) array (vectorised: the
    bench's path).  Same call order and layout as seed_calls."""
    n, L = reads2d.shape
    sl = L // 3
    fwd = np.asarray(reads2d, np.uint8)
    strand_seq = (fwd, revcomp_rows(fwd))
    ks = (0, 1) if L % 3 else (0,)
    pre_lens, pre_codes, keys = [], [], []
    for s in (0, 1):
        for k in ks:
            la = sl + (L % 3 if k else 0)
            pre_lens.append(np.full(n, la, np.uint32))
            pre_codes.append(strand_seq[s][:, :la].reshape(-1))
            keys.append((s, k, la))
    w = np.asarray(width_fn(np.concatenate(pre_lens), np.concatenate(pre_codes)), np.uint32).view(np.int32)
    pw, o = {}, 0
    for s, k, la in keys:
        m = n * 2 * (la + 1)
        pw[(s, k)] = w[o:o + m].reshape(n, la + 1, 2)
        o += m
    las = [sl + (L % 3 if i % 3 == 2 else 0) for i in range(6)]
    per_read_codes = sum(las)
    per_read_pairs = sum(la + 1 for la in las)
    codes = np.empty((n, per_read_codes), np.uint8)
    widths = np.empty((n, per_read_pairs, 2), np.int32)
    calls = np.zeros((n, 6), CALL_DTYPE)
    co = po = 0
    for i in range(6):
        s, la = i // 3, las[i]
        k = 1 if (i % 3 == 2 and L % 3) else 0
        codes[:, co:co + la] = strand_seq[s][:, (i % 3) * sl:(i % 3) * sl + la]
        widths[:, po:po + la + 1] = pw[(s, k)]
        calls[:, i]["read"] = np.arange(n)
        calls[:, i]["i"] = i
        calls[:, i]["strand"] = s
        calls[:, i]["len"] = la
        calls[:, i]["off"] = np.arange(n, dtype=np.uint64) * per_read_codes + co
        calls[:, i]["wb_off"] = np.arange(n, dtype=np.uint64) * per_read_pairs + po
        co += la
        po += la + 1
    return dict(calls=calls.reshape(-1), codes=codes.reshape(-1), widths=widths.reshape(-1, 2),
                opt=seed_options(local_opt))


def seed_jobs(batch):
    """hsa_job_t / hsa_mg_job_t arrays of a seed batch (width_seed aliased)."""
    from hsa_amd._lib import JOB_DTYPE, MG_DTYPE, SEED_ALIAS
    c = batch["calls"]
    so = batch["opt"]
    jobs = np.zeros(len(c), JOB_DTYPE)
    jobs["off"] = c["off"]
    jobs["len"] = c["len"]
    jobs["max_diff"] = so["max_diff"]
    jobs["seed_len"] = c["len"]
    mg = np.zeros(len(c), MG_DTYPE)
    mg["wb_off"] = c["wb_off"]
    mg["strand"] = c["strand"]
    mg["seed"] = SEED_ALIAS
    return jobs, mg


# ---------------------------------------------------------------- after the search: pairing the two segments
# The restatements hsa_splice_lines_device (hsa_amd/csrc/hsa_splice_rows.hip) is tested against.
ROW_COLS = ("aln_id", "seq_id", "ori_pos", "occ_pos")
SPLICE_MIN, SPLICE_MAX = 50, 50000          # bwtse.c:219
U32 = 0xFFFFFFFF


def segment_rows(k: int, l: int) -> int:
    """The SA rows bwt_aln2pos_splicing looks up for a segment (bwtse.c:320): k, k + 1, ...
    while <= l and < k + 50."""
    return max(0, min(l, k + 49) - k + 1)


def capped_multi(k0: int, l0: int, k1: int, l1: int) -> int:
    """n_multi of bwtse.c:310-312, the value of c1 and c2 (X0, X1)."""
    return min(100, (l0 - k0 + l1 - k1 + 2) & U32)


def pair_segments(rows):
    """bwt_combine_segment_splice (bwtse.c:197-235) over the rows of both segments in the
    order bwt_aln2pos_splicing fills them (segment 0's, then segment 1's): rows is an (n, 4)
    integer array of ROW_COLS.  Returns (n_res, index): index[2 p], index[2 p + 1] are the
    rows (indices into `rows`) of pair p as the reference leaves them at multi[2 p],
    multi[2 p + 1].

    Two rows are one pair as they stand, unsorted and whatever lies between them (:204).
    Otherwise the rows are sorted by occ_pos -- they are distinct SA rows, so their positions
    are distinct and any correct sort gives the reference's order -- and one pass keeps the
    pairs (segment 0 directly followed by segment 1 on one chromosome, 50 <= d <= 50 000) at
    the shortest distance so far.  The reference moves a kept pair to multi[2 (n_res - 1)]
    in place; the k-th kept pair starts at a sorted index >= 2 (k - 1), so a move never
    touches a row the loop has yet to read, and `if (i == 0) continue` skips a move of rows
    0, 1 onto themselves: collecting the pairs in a list is the same."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    n = len(rows)
    if n == 2:
        return 1, [0, 1]
    order = sorted(range(n), key=lambda r: (int(rows[r, 3]), r))
    shortest, pairs = U32, []
    for i in range(n - 1):
        a, b = rows[order[i]], rows[order[i + 1]]
        if a[0] != 0:
            continue
        d = int(b[3] - a[3]) & U32
        if a[0] == b[0] or a[1] != b[1] or d > shortest:
            continue
        if d < SPLICE_MIN or d > SPLICE_MAX:
            continue
        if d < shortest:
            shortest, pairs = d, [i]
        else:
            pairs.append(i)
    return len(pairs), [order[i + s] for i in pairs for s in (0, 1)]


def merge_cigar(cigar0, ori0: int, end0: int, cigar1, ori1: int):
    """The merged CIGAR of a spliced read (bwtse.c:578-582): segment 0's ops, N of length
    ori_pos1 - ori_pos0 - end0 (end0: segment 0's `end` field, all three after
    refine_gapped_core's adjustments), segment 1's ops; (op, length) pairs, N = 3."""
    return list(cigar0) + [(3, ori1 - ori0 - end0)] + list(cigar1)


def multi_entries(pairs):
    """What bwa_refine_gapped leaves in multi[0 .. n_multi - 2] of a spliced read with n_multi
    splice pairs (bwtse.c:603-618), the entries of its XA list.  pairs: per pair of
    pair_segments, in its order and pair 0 (the read's own alignment) included,
    (seq_id, strand, cigar0, ori0, end0, cigar1, ori1) after refine_gapped_core (the arguments
    of merge_cigar).  Pair i >= 1 becomes entry i - 1: a copy of the pair's first segment
    (seq_id, strand, ori_pos) with the merged CIGAR.  Returns (seq_id, strand, ori_pos,
    cigar) per entry."""
    return [(seq_id, strand, ori0, merge_cigar(c0, ori0, end0, c1, ori1)) for seq_id, strand, c0, ori0, end0, c1, ori1 in pairs[1:]]


def run_seed_calls(gi, batch, n_stacks: int):
    """All seed calls of `batch` in one hsa_match_gap_batch pass.
    Returns (n_aln, hit_off, hits, widths after, stats)."""
    from hsa_amd._lib import regime_of
    jobs, mg = seed_jobs(batch)
    so = batch["opt"]
    rg = regime_of(so, n_stacks, so["max_diff"])
    return gi.match_gap([rg], jobs, mg, batch["codes"], batch["widths"])
