"""The device chain of the 64-bit path, stage by stage: search (hsa_search_device64), hit
positions (hsa_hit_positions_device64), choose (hsa_choose_hits_device64), refine
(hsa_refine_rows_device64) and the SAM lines (hsa_sam_lines_device64); beside them, for the
reads the search leaves without a hit, the splice search (hsa_splice_device) and the spliced
reads' lines (hsa_splice_lines_device).

The convention.  Everything a stage reads or writes is a device tensor (anything with
data_ptr()) in one dict, by these keys; a stage returns the dict it was given with its own
outputs added, so the dict of the last stage holds the whole chain:

  the batch       jobs (hsa_job_t rows as bytes), codes (padded: _lib.pad_codes), n_jobs,
                  max_len; a sub-range of a batch is the same keys with offset views;
                  optional, for trimmed reads and barcodes (hsa_amd.reads.load_device with
                  the reader's options): full_len (u32 per job: the stored length, jobs' len
                  being the trimmed one), bc and bc_len (bc_len bytes per job).  trim_views
                  cuts them for a sub-range and sam_trim hands them to the two line writers;
  search          n_aln, flags, hit_off, hits, sc (the 16 counters), hit_cap, first (the
                  batch's job the arrays start at);
  positions       pos_off, pos, pos_hit, pos_ctr (optional for the SAM lines), pos_cap:
                  written by hit_positions64 or, the chosen and XA rows, by choose64;
  choose          sel, sel64, rng (the generator's state after the last read);
  refine          rows, rpos, cigar, md, ctr, cigar_stride, md_stride;
  splice          res (HSA_SP_RES_WORDS words per job), sp_ctr, sp_first (the batch's job
                  the arrays start at), sp_flags and sp_n_aln (what the call was given);
  splice lines    line_off, stat, ctr, out, rows (SL_ROW_WORDS words per job), cigar;
  junction table  a row buffer of its own (JN_ROW_WORDS words per row) that the three junction
                  stages append to, reduce in place and print (hsa_amd.junctions.Accumulator
                  owns it over the batches of a run).

Every stage is a builder and a driver.  The builder (`*_batch`) allocates the outputs and
returns the filled ctypes struct of _lib with the tensors; a probe builds once and times many
GpuIndex calls on a stream of its own.  The driver synchronises, calls, synchronises, reads
the counters and runs the call again with more room where a stage has a retry rule."""
from __future__ import annotations

import numpy as np

from . import reads
from ._lib import (ALN64_WORDS, HSA_RF_MAX_LEN, HSA_RF_MD, JOB_DTYPE, RF_ROW_WORDS, SL_ROW_WORDS, SL_XA_WORDS, SP_RES_WORDS, ChooseBatch64,
                   DeviceBatch, HitPosBatch64, HsaError, JunctionReduceBatch, JunctionRowsBatch, JunctionTextBatch, RefineBatch64, SamBatch64,
                   SamMergeBatch, SamTrim, SpliceBatch,
                   SpliceLinesBatch, SpliceXa,
                   anchor_regime, ext_regime, regime_of)

N_MULTI = 3                      # bwtaln.c:514


def to_device(a):
    """A NumPy array on the device, flat: unsigned types through their signed twins, a
    structured array (JOB_DTYPE) as its bytes."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "V":
        a = a.view(np.uint8)
    elif a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view(f"i{a.dtype.itemsize}")
    return torch.from_numpy(a.reshape(-1).copy()).cuda()


def make_jobs(lens, max_diff, seed_len):
    """The job rows of reads laid end to end: off the running sum of len, max_diff a value or
    one per read, seed_len as bwtaln.c:332 sets it (none for a read not longer than it)."""
    lens = np.asarray(lens, np.uint32)
    jobs = np.zeros(len(lens), JOB_DTYPE)
    jobs["off"][1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    jobs["len"] = lens
    jobs["max_diff"] = max_diff
    jobs["seed_len"] = np.where(lens > seed_len, seed_len, reads.SEED_NONE)
    return jobs


def local_regime(opt, max_len):
    """What bwa_cal_sa_reg_gap derives from an option dict for a batch whose longest read has
    max_len bases (bwtaln.c:254-276): (local_opt, n_stacks, the Regime of local_opt)."""
    local = dict(opt)
    if opt["fnr"] > 0:
        local["max_diff"] = reads.cal_maxdiff(int(max_len), reads.BWA_AVG_ERR, opt["fnr"])
    local["max_gapo"] = min(local["max_gapo"], local["max_diff"])
    n_stacks = (local["max_diff"] + 1) * local["s_mm"] + (local["max_gapo"] + 1) * local["s_gapo"] + \
        (local["max_gape"] + 1) * local["s_gape"]
    return local, n_stacks, regime_of(local, n_stacks, local["max_diff"])


def _new(n, dtype, fill=0):
    import torch
    return torch.full((n,), fill, dtype=getattr(torch, dtype), device="cuda")


def _ptr(d, k):
    return d[k].data_ptr() if d.get(k) is not None else None


def _call(fn, *args, **kw):
    import torch
    torch.cuda.synchronize()
    fn(*args, **kw)
    torch.cuda.synchronize()


def trim_views(b, first):
    """The batch's optional keys of trimmed reads and barcodes (full_len, bc, bc_len) from job
    `first` on: what a sub-range's dict takes over.  Empty for a batch without them."""
    o = {}
    if b.get("full_len") is not None:
        o["full_len"] = b["full_len"][first:]
    if b.get("bc_len"):
        o.update(bc=b["bc"][first * b["bc_len"]:], bc_len=b["bc_len"])
    return o


def sam_trim(d):
    """The SamTrim (hsa_sam_trim_t) of a dict's full_len / bc / bc_len, or None without them:
    the line writers then run their plain entry points."""
    if d.get("full_len") is None and not d.get("bc_len"):
        return None
    return SamTrim(d_full_len=_ptr(d, "full_len"), d_bc=_ptr(d, "bc") if d.get("bc_len") else None, bc_len=int(d.get("bc_len") or 0))


# ---------------------------------------------------------------- search
def search64_batch(b, first, n, hit_cap, max_seed):
    """(DeviceBatch, search tensors) for jobs [first, first + n) of the batch b with room for
    hit_cap records."""
    t = dict(n_aln=_new(n, "int32"), flags=_new(n, "int32"), hit_off=_new(n, "int64"),
             hits=_new(hit_cap * ALN64_WORDS + 2, "int32"), sc=_new(16, "int64"), hit_cap=hit_cap, first=first)
    db = DeviceBatch(d_jobs=b["jobs"].data_ptr() + first * JOB_DTYPE.itemsize, n_jobs=n, d_codes=b["codes"].data_ptr(),
                     d_n_aln=t["n_aln"].data_ptr(), d_flags=t["flags"].data_ptr(), d_hit_off=t["hit_off"].data_ptr(),
                     d_hits=t["hits"].data_ptr(), hit_cap=hit_cap, d_counters=t["sc"].data_ptr(), max_len=b["max_len"],
                     max_seed=max_seed)
    return db, t


def search64(gi, b, first, n, regime, max_seed, hit_cap=None):
    """hsa_search_device64 of jobs [first, first + n) of the batch under `regime`: the search
    tensors.  hit_cap: the records to start with (64 per read); the search runs again with
    eight times the room while reads are left unfinished, four times in all."""
    cap = 64 * n if hit_cap is None else hit_cap
    for _ in range(4):
        db, t = search64_batch(b, first, n, cap, max_seed)
        _call(gi.search_device64, [regime], db)
        if int(t["sc"][11]) == 0:
            return t
        cap *= 8
    raise HsaError("reads left unfinished by the search with 32 768 hit records per read")


# ---------------------------------------------------------------- hit positions
def hit_positions64_batch(t, n, max_occ, fill=0, out=None):
    """(HitPosBatch64, position tensors) for the hit lists of the search tensors t, up to
    max_occ rows per read.  fill: what pos and pos_hit hold before the call; out: the
    position tensors of another builder (of the same pos_cap) to write into instead."""
    cap = n * max_occ
    o = out or dict(pos_off=_new(n + 1, "int64"), pos=_new(cap * 4, "int64", fill), pos_hit=_new(cap, "int32", fill),
                    pos_ctr=_new(8, "int64"))
    hb = HitPosBatch64(d_n_aln=t["n_aln"].data_ptr(), d_hit_off=t["hit_off"].data_ptr(), d_hits=t["hits"].data_ptr(), n_jobs=n,
                       max_occ=max_occ, d_pos_off=o["pos_off"].data_ptr(), d_pos=o["pos"].data_ptr(),
                       d_pos_hit=o["pos_hit"].data_ptr(), pos_cap=cap, d_counters=o["pos_ctr"].data_ptr())
    return hb, dict(pos_off=o["pos_off"], pos=o["pos"], pos_hit=o["pos_hit"], pos_ctr=o["pos_ctr"], pos_cap=cap)


def hit_positions64(gi, t, n, max_occ, fill=0):
    """hsa_hit_positions_device64 of the search tensors t: t with the position tensors."""
    hb, o = hit_positions64_batch(t, n, max_occ, fill)
    _call(gi.hit_positions64, hb)
    return dict(t, **o)


# ---------------------------------------------------------------- choose
def choose64_batch(b, t, first, n, state, n_multi=N_MULTI):
    """(ChooseBatch64, the sub-range's dict) for jobs [first, first + n) of the batch b, whose
    search tensors are t (which start at job t["first"]): offset views of the batch and of
    the search, the choice's outputs and its rows (pos_cap = n (n_multi + 1))."""
    k = first - t["first"]
    cap = max(n * (n_multi + 1), 1)
    sub = dict(jobs=b["jobs"][first * JOB_DTYPE.itemsize:], codes=b["codes"], n_aln=t["n_aln"][k:], hit_off=t["hit_off"][k:],
               hits=t["hits"], n_jobs=n, max_len=b["max_len"], sel=_new(max(n, 1) * 4, "int32"),
               sel64=_new(max(n, 1) * 4, "int64"), rng=_new(1, "int64"), pos_off=_new(n + 1, "int64"),
               pos=_new(cap * 4, "int64"), pos_hit=_new(cap, "int32"), pos_ctr=_new(8, "int64"), pos_cap=cap,
               **trim_views(b, first))
    cb = ChooseBatch64(d_jobs=sub["jobs"].data_ptr(), n_jobs=n, d_n_aln=sub["n_aln"].data_ptr(),
                       d_hit_off=sub["hit_off"].data_ptr(), d_hits=sub["hits"].data_ptr(), n_multi=n_multi, rng_state=state,
                       d_sel=sub["sel"].data_ptr(), d_sel64=sub["sel64"].data_ptr(), d_rng_out=sub["rng"].data_ptr(),
                       d_pos_off=sub["pos_off"].data_ptr(), d_pos=sub["pos"].data_ptr(), d_pos_hit=sub["pos_hit"].data_ptr(),
                       pos_cap=cap, d_counters=sub["pos_ctr"].data_ptr())
    return cb, sub


def choose64(gi, b, t, first, n, state):
    """hsa_choose_hits_device64 over jobs [first, first + n) of the batch: (the sub-range's
    dict, the generator's new state).  A zero-draw read is an error."""
    cb, sub = choose64_batch(b, t, first, n, state)
    _call(gi.choose_hits64, cb)
    ctr = sub["pos_ctr"].cpu().numpy().view(np.uint64)
    if int(ctr[6]):
        raise HsaError(f"read {first + int(ctr[7])} of the batch draws exactly 0.0 (a zero-draw read): not handled")
    assert int(ctr[0]) == int(ctr[1])
    return sub, int(sub["rng"].cpu().numpy().view(np.uint64)[0])


# ---------------------------------------------------------------- refine
def refine64_batch(sub, cigar_stride, md_stride):
    """(RefineBatch64, sub with the refinement's tensors) for the position rows of sub."""
    m = sub["pos_cap"]
    o = dict(sub, rows=_new(m * RF_ROW_WORDS, "int32"), rpos=_new(m * 2, "int64"), cigar=_new(m * cigar_stride, "int32"),
             md=_new(m * md_stride, "uint8"), ctr=_new(8, "int64"), cigar_stride=cigar_stride, md_stride=md_stride)
    rb = RefineBatch64(d_jobs=sub["jobs"].data_ptr(), n_jobs=sub["n_jobs"], d_codes=sub["codes"].data_ptr(),
                       d_hit_off=sub["hit_off"].data_ptr(), d_hits=sub["hits"].data_ptr(), d_pos_off=sub["pos_off"].data_ptr(),
                       d_pos=sub["pos"].data_ptr(), d_pos_hit=sub["pos_hit"].data_ptr(), pos_cap=m,
                       d_pos_counters=_ptr(sub, "pos_ctr"), max_len=min(max(sub["max_len"], 1), HSA_RF_MAX_LEN),
                       cigar_stride=cigar_stride, md_stride=md_stride, d_rows=o["rows"].data_ptr(), d_rpos=o["rpos"].data_ptr(),
                       d_cigar=o["cigar"].data_ptr(), d_md=o["md"].data_ptr(), d_counters=o["ctr"].data_ptr())
    return rb, o


def refine64(gi, sub, cigar_stride=16, md_stride=128):
    """hsa_refine_rows_device64 of the rows of sub; both strides double while a CIGAR or an
    MD string does not fit and md_stride is under 16 384."""
    while True:
        rb, o = refine64_batch(sub, cigar_stride, md_stride)
        _call(gi.refine_rows64, rb)
        if int(o["ctr"][1 + HSA_RF_MD]) == 0 or md_stride >= 16384:
            return o
        cigar_stride, md_stride = cigar_stride * 2, md_stride * 2


# ---------------------------------------------------------------- the splice search and its lines
def splice_regimes(local, n_stacks):
    """(seed, anchor, extension) regimes of bwt_splice_match for a batch's local options:
    aux_seed (bwtgap.c:769-774) and aux_ext (:776-782)."""
    from . import splice
    so = splice.seed_options(local)
    return (regime_of(so, n_stacks, so["max_diff"]), anchor_regime(local, n_stacks, local["max_diff"]),
            ext_regime(local, n_stacks, local["max_diff"]))


def splice32_batch(b, t, first, n, jobs=None, flags=None):
    """(SpliceBatch, the splice tensors res, sp_ctr, sp_first) for jobs [first, first + n) of
    the batch b, whose search tensors are t.  jobs, flags: tensors to take these jobs' rows
    and flags from instead of the batch's and the search's (from job `first` on)."""
    k = first - t["first"]
    jobs = b["jobs"][first * JOB_DTYPE.itemsize:] if jobs is None else jobs
    flags = t["flags"][k:] if flags is None else flags
    o = dict(res=_new(max(n, 1) * SP_RES_WORDS, "int32"), sp_ctr=_new(8, "int64"), sp_first=first, sp_flags=flags,
             sp_n_aln=t["n_aln"][k:])
    sb = SpliceBatch(d_jobs=jobs.data_ptr(), n_jobs=n, d_codes=b["codes"].data_ptr(), d_flags=flags.data_ptr(),
                     d_n_aln=o["sp_n_aln"].data_ptr(), d_res=o["res"].data_ptr(), d_counters=o["sp_ctr"].data_ptr(),
                     max_len=b["max_len"])
    return sb, o


def splice32(gi, b, t, first, n, regimes, jobs=None, flags=None):
    """hsa_splice_device over jobs [first, first + n) of the batch: bwt_splice_match of every
    job the search flagged HSA_F_FALLBACK and left without a hit, under the (seed, anchor,
    extension) regimes of splice_regimes.  Each read's max_diff is its job's.  Returns the
    splice tensors: res (HSA_SP_RES_WORDS words per job, written for those reads only)."""
    sb, o = splice32_batch(b, t, first, n, jobs, flags)
    _call(gi.splice_device, regimes[0], regimes[1], regimes[2], sb)
    return o


def splice_lines_batch(b, s, first, n, strings, n_chr, max_line, out_cap, cigar_stride=33, flag=0, max_top2=30, comp_read=True):
    """(SpliceLinesBatch, the output tensors line_off, stat, ctr, out, rows, cigar) for jobs
    [first, first + n) of the batch b and the splice tensors s (of splice32).  strings: as
    sam_lines64_batch takes them, the offsets from job `first` on."""
    import torch
    k = first - s["sp_first"]
    o = dict(line_off=_new(n + 1, "int64"), stat=_new(max(n, 1), "int32"), ctr=_new(8, "int64"),
             out=torch.empty(max(out_cap, 1), dtype=torch.uint8, device="cuda"), rows=_new(max(n, 1) * SL_ROW_WORDS, "int32"),
             cigar=_new(max(n, 1) * cigar_stride, "int32"), cigar_stride=cigar_stride)
    lb = SpliceLinesBatch(d_jobs=b["jobs"].data_ptr() + first * JOB_DTYPE.itemsize, n_jobs=n, d_codes=b["codes"].data_ptr(),
                          d_flags=s["sp_flags"][k:].data_ptr(), d_n_aln=s["sp_n_aln"][k:].data_ptr(),
                          d_res=s["res"][k * SP_RES_WORDS:].data_ptr(), d_names=strings["names"].data_ptr(),
                          d_name_off=strings["name_off"].data_ptr(), d_quals=_ptr(strings, "quals"),
                          d_qual_off=_ptr(strings, "qual_off"), d_chr_names=strings["chrs"].data_ptr(),
                          d_chr_off=strings["chr_off"].data_ptr(), n_chr=n_chr, flag=int(flag), max_top2=int(max_top2),
                          comp_read=int(bool(comp_read)), max_len=b["max_len"], max_line=max_line, cigar_stride=cigar_stride,
                          d_rows=o["rows"].data_ptr(), d_cigar=o["cigar"].data_ptr(), d_line_off=o["line_off"].data_ptr(),
                          d_out=o["out"].data_ptr(), out_cap=out_cap, d_line_stat=o["stat"].data_ptr(),
                          d_counters=o["ctr"].data_ptr())
    return lb, o


def splice_xa_batch(n, room, cigar_stride=33):
    """(SpliceXa, its output tensors pair_off, pair_rows, pair_cigar, xa_ctr) for a splice-lines
    batch of n jobs with room for `room` extra splice pairs (the XA:Z entries of reads with
    several pairs)."""
    o = dict(pair_off=_new(n + 1, "int64"), pair_rows=_new(max(room, 1) * SL_XA_WORDS, "int32"),
             pair_cigar=_new(max(room, 1) * max(cigar_stride, 1), "int32"), xa_ctr=_new(8, "int64"), pair_cap=room)
    xa = SpliceXa(pair_cap=room, d_pair_off=o["pair_off"].data_ptr(), d_pair_rows=o["pair_rows"].data_ptr(),
                  d_pair_cigar=o["pair_cigar"].data_ptr(), d_counters=o["xa_ctr"].data_ptr())
    return xa, o


def xa_room(n):
    """The extra pairs a first run of splice_lines has room for: every slot is two more rows
    for the refinement, used or not, so a sixteenth of the reads and 64."""
    return n // 16 + 64


def splice_lines(gi, b, s, first, n, strings, n_chr, max_line, out_cap, **kw):
    """hsa_splice_lines_device_xa over jobs [first, first + n) with room for out_cap bytes and
    xa_room(n) extra splice pairs, run again with the room the counters ask for while a run
    reports wanted > served (pairs: xa_ctr[0] > the room; bytes: ctr[0] > ctr[1]): (the output
    tensors, those of splice_xa_batch among them and the list counters as o["xa"], 8 u64 on the
    host; the counters as 8 u64 on the host)."""
    room = xa_room(n)
    coff = strings["chr_off"][:n_chr + 1].cpu().numpy().view(np.uint64).astype(np.int64)
    entry_chr = int(np.diff(coff).max()) if n_chr else 0
    for _ in range(4):
        lb, o = splice_lines_batch(b, s, first, n, strings, n_chr, max_line, out_cap, **kw)
        xa, ox = splice_xa_batch(n, room, o["cigar_stride"])
        _call(gi.splice_lines, lb, trim=sam_trim(trim_views(b, first)), xa=xa)
        ctr = o["ctr"].cpu().numpy().view(np.uint64)
        xc = ox["xa_ctr"].cpu().numpy().view(np.uint64)
        o.update(ox, xa=xc)
        if int(xc[0]) <= room and int(ctr[0]) <= int(ctr[1]):
            break
        # a run short of room counted no byte of the lists it left out: allow for them, so that
        # the next run is the last (an entry: the chromosome, ",+", a position, some ten ops)
        more = max(0, int(xc[0]) - room) * (entry_chr + 64)
        room, out_cap = max(room, int(xc[0])), max(out_cap, int(ctr[0]) + more)
    return o, ctr


def sam_merge_batch(n, a, b):
    """(SamMergeBatch, the output tensors line_off, out, ctr) for the lines of two writers over
    the same n reads.  a, b: (the text tensor, its bytes, the writer's line_off tensor)."""
    import torch
    cap = int(a[1]) + int(b[1])
    o = dict(line_off=_new(n + 1, "int64"), out=torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda"), ctr=_new(8, "int64"))
    mb = SamMergeBatch(n_jobs=n, d_line_off_a=a[2].data_ptr(), d_text_a=a[0].data_ptr(), text_a_len=int(a[1]),
                       d_line_off_b=b[2].data_ptr(), d_text_b=b[0].data_ptr(), text_b_len=int(b[1]),
                       d_line_off=o["line_off"].data_ptr(), d_out=o["out"].data_ptr(), out_cap=cap, d_counters=o["ctr"].data_ptr())
    return mb, o


def sam_merge(gi, n, a, b):
    """hsa_sam_merge_device: (the output tensors, the counters as 8 u64 on the host)."""
    mb, o = sam_merge_batch(n, a, b)
    _call(gi.sam_merge, mb)
    return o, o["ctr"].cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------- junction table
def junction_rows_batch(o, n, jrows, n_have, row_cap):
    """(JunctionRowsBatch, the counters' tensor) for the n jobs of splice_lines' output tensors
    o (rows, cigar, stat, cigar_stride) and a row buffer jrows (JN_ROW_WORDS int32 per row,
    row_cap rows) that holds n_have rows."""
    ctr = _new(8, "int64")
    jb = JunctionRowsBatch(n_jobs=n, cigar_stride=int(o["cigar_stride"]), d_rows=o["rows"].data_ptr(), d_cigar=o["cigar"].data_ptr(),
                           d_line_stat=o["stat"].data_ptr(), d_jrows=jrows.data_ptr(), n_have=int(n_have), row_cap=int(row_cap),
                           d_counters=ctr.data_ptr())
    return jb, ctr


def junction_rows(gi, o, n, jrows, n_have, row_cap):
    """hsa_junction_rows_device: the counters as 8 u64 on the host ([0] rows wanted, [1] rows
    written behind the n_have the buffer held).  hsa_amd.junctions.Accumulator grows the buffer
    and runs it again when wanted > written."""
    jb, ctr = junction_rows_batch(o, n, jrows, n_have, row_cap)
    _call(gi.junction_rows, jb)
    return ctr.cpu().numpy().view(np.uint64)


def junction_reduce_batch(jrows, n_rows):
    """(JunctionReduceBatch, the counters' tensor) for the first n_rows rows of a row buffer."""
    ctr = _new(8, "int64")
    return JunctionReduceBatch(d_jrows=jrows.data_ptr(), n_rows=int(n_rows), d_counters=ctr.data_ptr()), ctr


def junction_reduce(gi, jrows, n_rows):
    """hsa_junction_reduce_device, in place: the counters as 8 u64 on the host ([0] rows in,
    [1] rows out)."""
    rb, ctr = junction_reduce_batch(jrows, n_rows)
    _call(gi.junction_reduce, rb)
    return ctr.cpu().numpy().view(np.uint64)


def junction_text_batch(jrows, n_rows, chrs, chr_off, n_chr, out_cap):
    """(JunctionTextBatch, the output tensors line_off, out, ctr) for a reduced table of n_rows
    rows; chrs, chr_off: the chromosome names as the line writers take them."""
    import torch
    o = dict(line_off=_new(n_rows + 1, "int64"), out=torch.empty(max(out_cap, 1), dtype=torch.uint8, device="cuda"), ctr=_new(8, "int64"))
    tb = JunctionTextBatch(d_jrows=jrows.data_ptr(), n_rows=int(n_rows), d_chr_names=chrs.data_ptr(), d_chr_off=chr_off.data_ptr(),
                           n_chr=n_chr, d_line_off=o["line_off"].data_ptr(), d_out=o["out"].data_ptr(), out_cap=int(out_cap),
                           d_counters=o["ctr"].data_ptr())
    return tb, o


def junction_text(gi, jrows, n_rows, chrs, chr_off, n_chr, out_cap):
    """hsa_junction_text_device with room for out_cap bytes, run a second time with counters[0]
    bytes of room when the first reports wanted > written: (the output tensors, the counters as
    8 u64 on the host)."""
    for _ in range(2):
        tb, o = junction_text_batch(jrows, n_rows, chrs, chr_off, n_chr, out_cap)
        _call(gi.junction_text, tb)
        ctr = o["ctr"].cpu().numpy().view(np.uint64)
        if int(ctr[0]) <= int(ctr[1]):
            break
        out_cap = int(ctr[0])
    return o, ctr


# ---------------------------------------------------------------- SAM lines
def sam_lines64_batch(dev, strings, n_chr, max_line, out_cap, flag=0, max_top2=30, comp_read=True):
    """(SamBatch64, the output tensors line_off, stat, ctr, out) for the chain's dict dev.
    strings: names, name_off, chrs, chr_off and, unless the lines print "*", quals, qual_off."""
    import torch
    n = int(dev["n_jobs"])
    o = dict(line_off=_new(n + 1, "int64"), stat=_new(max(n, 1), "int32"), ctr=_new(8, "int64"),
             out=torch.empty(max(out_cap, 1), dtype=torch.uint8, device="cuda"))
    sb = SamBatch64(d_jobs=_ptr(dev, "jobs"), n_jobs=n, d_codes=_ptr(dev, "codes"), d_n_aln=_ptr(dev, "n_aln"),
                    d_hit_off=_ptr(dev, "hit_off"), d_hits=_ptr(dev, "hits"), d_sel=_ptr(dev, "sel"), d_sel64=_ptr(dev, "sel64"),
                    d_pos_off=_ptr(dev, "pos_off"), d_pos=_ptr(dev, "pos"), d_pos_hit=_ptr(dev, "pos_hit"),
                    pos_cap=int(dev["pos_cap"]), d_pos_counters=_ptr(dev, "pos_ctr"), d_rows=_ptr(dev, "rows"),
                    d_rpos=_ptr(dev, "rpos"), d_cigar=_ptr(dev, "cigar"), d_md=_ptr(dev, "md"),
                    cigar_stride=int(dev["cigar_stride"]), md_stride=int(dev["md_stride"]), d_names=strings["names"].data_ptr(),
                    d_name_off=strings["name_off"].data_ptr(), d_quals=_ptr(strings, "quals"), d_qual_off=_ptr(strings, "qual_off"),
                    d_chr_names=strings["chrs"].data_ptr(), d_chr_off=strings["chr_off"].data_ptr(), n_chr=n_chr,
                    flag=int(flag), max_top2=int(max_top2), comp_read=int(bool(comp_read)), max_line=max_line,
                    d_line_off=o["line_off"].data_ptr(), d_out=o["out"].data_ptr(), out_cap=out_cap,
                    d_line_stat=o["stat"].data_ptr(), d_counters=o["ctr"].data_ptr())
    return sb, o


def sam_lines64(gi, dev, strings, n_chr, max_line, out_cap, **kw):
    """hsa_sam_lines_device64 of the chain's dict dev with room for out_cap bytes, run a second
    time with counters[0] bytes of room when the first reports wanted > written: (the output
    tensors, the counters as 8 u64 on the host)."""
    for _ in range(2):
        sb, o = sam_lines64_batch(dev, strings, n_chr, max_line, out_cap, **kw)
        _call(gi.sam_lines64, sb, trim=sam_trim(dev))
        ctr = o["ctr"].cpu().numpy().view(np.uint64)
        if int(ctr[0]) <= int(ctr[1]):
            break
        out_cap = int(ctr[0])
    return o, ctr
