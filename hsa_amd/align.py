"""FASTQ to SAM on the 64-bit path: `python -m hsa_amd.align [options] <prefix> <in.fq>`.

open_index64 opens the index files `python -m hsa_amd.index_build` writes as a 64-bit
GpuIndex; align_fastq drives, per batch of 0x186A0 reads (bwtaln.c:477), what
bwa_aln_core does with it (bwtaln.c:452-531):

  1. load the batch: hsa_reads_device (hsa_amd.reads.load_device) takes the canonical
     records, hsa_amd.reads.parse_host the ones it refuses, one or a few at a time, and the
     device loader goes on behind them;
  2. search every kept read with the options as bwa_cal_sa_reg_gap sets them through
     aux->opt (`mode &= ~BWA_MODE_GAPE`, bwtaln.c:261);
  3. find the first read without a hit and search the reads after it again with the batch's
     local options (bwtaln.c:363: aux->opt stays &local_opt for the rest of the batch);
  4. choose, refine and write the SAM lines per part, the drand48 state chained through the
     parts and the batches (the stage calls of steps 2 to 4: hsa_amd.chain);
  5. append the text to `out`.

What the reference's loop does to its option block is kept over the batches: the GAPE bit
stays cleared after the first batch (so only the first batch's local options have it), and
opt->seed_len turns to 0x7fffffff for good at the first searched read, up to the switch, that
is not longer than it (bwtaln.c:332 writes through aux->opt).

Contract.  One line per read with a main-search hit, in read order, byte for byte
bwa_print_sam1's (bwtse.c:698-799).  A read without one goes to bwt_splice_match in the
reference.  Without --splice (splice=False, the default) it gets no line; such reads are
counted and, with --unaligned FILE, written back out as FASTQ, and the text equals the
reference's up to the first read whose line the reference prints from its splice path,
because that read's drand48 draws are not seen here (tests/test_gpu_choose.py documents the
condition).

With --splice (splice=True; an index under 2^32 characters and at most HSA_SP_MAX_STACKS
score buckets, ValueError otherwise) every such read goes through hsa_splice_device
(chain.splice32) with the batch's local options, the first one with local_opt.max_diff as
the batch has it (bwtaln.c:331 wrote that read's own through the caller's block).  A result
that is not two records of type BWA_TYPE_SPLICING is appended to the read's hit list on the
device and is chosen, refined and printed like any other (its draws are made in read
order); a spliced result is paired, refined and printed by hsa_splice_lines_device_xa
(chain.splice_lines: XT:A:S, CIGAR with an N, and for a read whose segments combine into
several pairs at the shortest distance the others as an XA:Z list in the reference's format
for them, bwtse.c:782-797; `spliced_xa` such reads, `spliced_xa_entries` entries), and the two
writers' lines are merged in read order.  Then every line the reference prints is printed, except for reads the device
refuses, each of which gets no line (exact or nothing), counts towards no_line and goes to
--unaligned: `handed_back` (hsa_splice_device's status > 0: there is no host
bwt_splice_match here), `spliced_multi` (several pairs that found no room: 0, since
chain.splice_lines runs again with the room the device asks for), `spliced_refused` (a segment's alignment not answered, a position in
no chromosome block, an N length that is not positive, a line past the bound).  After a
handed-back read that the reference would have printed as U / R the generator state is no
longer the reference's, and R reads after it may choose differently; the committed
fixtures have no such read (0 of 601, 614 and 203 reads sent are handed back).  No @SQ
header unless --header is given; with it, "@SQ\\tSN:<name>\\tLN:<length>" per chromosome of the
.ann file, the reference's format (bwt_print_sam_SQ, bwtse.c:826-834).

The reader's options are bwa_read_seq's (bwaseqio.c:161-231), on the device for the canonical
records and in parse_host for the rest: -q INT trims a read's end by quality (bwa_trim_read):
the search, the refinement and MD see the trimmed read, and the line has the whole read's SEQ
and QUAL, the trimmed bases as an S op (bwa_correct_trimmed) and XC:i; -B INT cuts a barcode
off the front (BC:Z); -Y skips the records Casava marks as filtered; -I takes 31 off every
quality.  A skipped record is no read: it counts towards no batch, gets no line, is not
written to --unaligned, and is counted as `filtered`; `trimmed_bases` of `total_bases` is what
the reference reports as "% bases are trimmed".  --unaligned writes a read's record as it was
given, barcode included.

BAM input (-b, with -0, -1, -2 to select the records; hsa_amd.bam states the rule): align_fastq
with the BAM bit of opts["mode"] takes a path or the file's bytes, opens the text through
bam.open_text (BGZF inflated on the device, the text kept resident), reads the header on the
host and loads every batch through hsa_bam_reads_device (_load_batch_bam): windows of the
resident text, or of the host text uploaded when the inflater needed several groups, with the
BGZF members' first bytes inside the window as anchors.  A call that ends on an anchor that is
not on the record chain keeps what it loaded and the rest of the batch comes from the
single-anchor walk; records the device does not take (an empty name, a read past the max_diff
table) go through bam.parse_host.  Everything after the load is the code above.  -B, -I and
-Y have no effect on BAM input (bwaseqio.c:172) and are ignored; -0, -1, -2 without -b have
none either (the file is then opened as FASTQ, bwtaln.c:441).  --unaligned writes a BAM read
as a FASTQ record in the read's own orientation.  The statistics gain inflate_* (the
inflater's), bam_segments (the segments the calls were given: one more key than the loader's
issue lists, the figure bam_segments_verified is read against) and bam_segments_verified,
bam_serial_records (records found by a
single-anchor walk) and bam_truncated: a truncated or inconsistent record ends the input
there, the reads before it are aligned, and main returns 1.  Without the BAM bit nothing
changes, the keys of the statistics included.

--junctions FILE (with --splice; align_fastq's junctions=<binary file object>) writes the run's
splice junction table after the last batch: one row per distinct intron of the printed XT:A:S
lines in the nine columns of STAR's SJ.out.tab, made on the device from what
hsa_splice_lines_device_xa leaves there (hsa_amd.junctions states the table and restates it on
the host from the SAM text; hsa_junctions.hip).  The statistics gain junction_rows (rows fed:
the spliced lines) and junctions (distinct introns).  Without the option the text, the
statistics' keys and the calls made are the same as before.

Not built: colour space (-c): refused.  -t is accepted and
ignored.  A read the choice counts as a zero-draw read (probability 2^-48 per read) stops the
run with an error."""
from __future__ import annotations

import functools
import gzip
import sys

import numpy as np

from . import bam, chain, index_io, reads, sam
from ._lib import (ALN64_WORDS, DRAND48_SEED0, HSA_RD_NDROP, HSA_RD_POLYAT, HSA_RD_SEARCHED, HSA_RF_MAX_LEN, HSA_SP_MAX_STACKS,
                   JOB_DTYPE, SP_RES_WORDS, GapOpt, GpuIndex, regime_of)

HSA_DRAND48_SEED0 = DRAND48_SEED0
BATCH_READS = 0x186A0            # bwtaln.c:477
MODE_GAPE, MODE_COMPREAD, MODE_LOGGAP, MODE_NONSTOP = 0x01, 0x02, 0x04, 0x10
MODE_CFY, MODE_IL13 = reads.MODE_CFY, reads.MODE_IL13
MODE_READER = MODE_CFY | MODE_IL13 | 0xFF000000          # what bwa_read_seq takes of gap_opt_t.mode (the barcode length on top)
MODE_BAM, MODE_BAM_ALL = bam.MODE_BAM, bam.MODE_BAM_ALL   # -b; with -0, -1, -2 (bwtaln.h:127-130)
_BAM_BITS = {"-b": bam.MODE_BAM, "-0": bam.MODE_BAM_SE, "-1": bam.MODE_BAM_READ1, "-2": bam.MODE_BAM_READ2}
SEED_NONE = reads.SEED_NONE
TABLE_LEN = HSA_RF_MAX_LEN + 1   # reads past it go through the host parser (and are not refined)
ONES = 0xFFFFFFFFFFFFFFFF
TYPE_SPLICING = 4                # bwtaln.h:13
OPTSTRING = "n:o:e:i:d:l:k:cLR:m:t:NM:O:E:q:f:b012IYB:"       # bwtaln.c:539


# ---------------------------------------------------------------- options
def default_opts() -> dict:
    """gap_init_opt (bwtaln.c:21-44); fnr as the float the reference stores."""
    return GapOpt.default().as_dict()


def _atoi(s: str) -> int:
    """C's atoi: optional blanks and sign, then digits; 0 when there are none."""
    s = s.lstrip(" \t\n\v\f\r")
    k = 1 if s[:1] in ("+", "-") else 0
    e = k
    while e < len(s) and s[e].isascii() and s[e].isdigit():
        e += 1
    v = int(s[:e]) if e > k else 0
    return ((v + 0x80000000) & 0xFFFFFFFF) - 0x80000000


def _atof(s: str) -> float:
    """C's atof on the longest decimal prefix; 0.0 when there is none."""
    import re
    m = re.match(r"[ \t\n\v\f\r]*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?)", s)
    return float(m.group(0)) if m else 0.0


def parse_options(args, reader_options=False, bam_options=False):
    """bwa_aln's option switch (bwtaln.c:539-575) over `args`: (the option dict, the
    positional arguments, dict(header, unaligned, out), with the keys splice and junctions only
    when --splice and --junctions FILE are given).  Options of what is not built raise
    ValueError.  reader_options: take the reader's options as the switch sets them (:558,
    :566-568): -q INT (trim_qual), -B INT (mode |= n << 24), -I (MODE_IL13), -Y (MODE_CFY); a
    barcode over BWA_MAX_BCLEN (the reference then reads nothing) and a trim_qual over
    reads.MAX_TRIM_QUAL are ValueError.  Without it they are refused, as before the reader
    had them; the command line (main) sets it.  bam_options: take -b, -0, -1, -2 as the switch
    sets them (:562-565: MODE_BAM, MODE_BAM_SE, MODE_BAM_READ1, MODE_BAM_READ2); without it they
    are refused, whatever reader_options says."""
    import getopt
    o = default_opts()
    extra = dict(header=False, unaligned=None, out=None)
    opte = -1
    optlist, rest = getopt.gnu_getopt(list(args), OPTSTRING, ["header", "unaligned=", "splice", "junctions="])
    plain = {"-o": "max_gapo", "-M": "s_mm", "-O": "s_gapo", "-E": "s_gape", "-d": "max_del_occ", "-i": "indel_end_skip",
             "-l": "seed_len", "-k": "max_seed_diff", "-m": "max_entries", "-t": "n_threads", "-R": "max_top2"}
    for k, v in optlist:
        if k == "-n":
            if "." in v:
                o["fnr"], o["max_diff"] = float(np.float32(_atof(v))), -1
            else:
                o["max_diff"], o["fnr"] = _atoi(v), -1.0
        elif k in plain:
            o[plain[k]] = _atoi(v)
        elif k == "-e":
            opte = _atoi(v)
        elif k == "-L":
            o["mode"] |= MODE_LOGGAP
        elif k == "-N":
            o["mode"] |= MODE_NONSTOP
            o["max_top2"] = 0x7FFFFFFF
        elif k == "-q":
            o["trim_qual"] = _atoi(v)
        elif k == "-B" and reader_options:
            n = _atoi(v)
            if not 0 <= n <= reads.BWA_MAX_BCLEN:
                raise ValueError(f"-B {n}: the maximum barcode length is {reads.BWA_MAX_BCLEN}")
            o["mode"] |= n << 24
        elif k == "-I" and reader_options:
            o["mode"] |= MODE_IL13
        elif k == "-Y" and reader_options:
            o["mode"] |= MODE_CFY
        elif k in _BAM_BITS and bam_options:
            o["mode"] |= _BAM_BITS[k]
        elif k == "-f":
            extra["out"] = v
        elif k == "--header":
            extra["header"] = True
        elif k == "--unaligned":
            extra["unaligned"] = v
        elif k == "--splice":
            extra["splice"] = True                          # (the key is there only when the option is)
        elif k == "--junctions":
            extra["junctions"] = v                          # (likewise)
        else:
            raise ValueError(f"option {k} is not built" + (" (colour space)" if bam_options else " (BAM input, colour space)" if reader_options else
                                                           " (barcodes, Casava filter, Illumina-1.3 qualities, BAM, colour space)"))
    if opte > 0:
        o["max_gape"] = opte
        o["mode"] &= ~MODE_GAPE
    if o["trim_qual"] != 0 and not reader_options:
        raise ValueError("quality trimming (-q) is not built")
    if o["trim_qual"] > reads.MAX_TRIM_QUAL:
        raise ValueError(f"-q {o['trim_qual']}: at most {reads.MAX_TRIM_QUAL} (the trimming sum of a {0xFFFF}-base read stays in 32 bits)")
    return o, rest, extra


# ---------------------------------------------------------------- the index
def _msb_to_lsb(code, T):
    """.bwt words (character j of a word at bits 31-2j .. 30-2j) to LSB-first words, the
    codes past T cleared."""
    x = np.ascontiguousarray(code, np.uint32).copy()
    x = (x >> 16) | (x << 16)
    x = ((x & 0xFF00FF00) >> 8) | ((x & 0x00FF00FF) << 8)
    x = ((x & 0xF0F0F0F0) >> 4) | ((x & 0x0F0F0F0F) << 4)
    x = (((x & 0xCCCCCCCC) >> 2) | ((x & 0x33333333) << 2)).astype(np.uint32)
    if T % 16:
        x[-1] &= np.uint32((1 << (2 * (T % 16))) - 1)
    return x


def read_chromosomes(prefix: str):
    """(names, lengths) by chrID from prefix.index.ann; a length is the span of the
    chromosome's blocks."""
    with open(prefix + ".index.ann") as f:
        ls = f.read().split("\n")
    n_chr = int(ls[0].split()[1])
    names = [ls[1 + k].split()[1] for k in range(n_chr)]
    blocks = index_io.read_blocks(prefix).astype(np.int64)
    lens = []
    for c in range(n_chr):
        b = blocks[blocks[:, 0] == c]
        lens.append(int(b[:, 2].max() - b[:, 1].min() + 1) if len(b) else 0)
    return names, lens


def open_index64(prefix: str, device: int = 0):
    """(GpuIndex, chromosome names) from the index files of `prefix` (prefix.index.*): a
    64-bit index (hsa_index_create_device64) with both BWTs, the SA samples (as they are for
    the 32-bit calls, and widened to u64 for the 64-bit ones) with the block table, and the
    packed text."""
    import torch
    fwd, rev = index_io.read_index(prefix)
    up = lambda b: torch.from_numpy(np.concatenate([_msb_to_lsb(b.code, b.T), np.zeros(8, np.uint32)]).view(np.int32)).cuda(device)
    d_f, d_r = up(fwd), up(rev)
    torch.cuda.synchronize()
    gi = GpuIndex.from_device_codes64(fwd.T, fwd.isa0, np.asarray(fwd.C, np.uint64), d_f.data_ptr(), rev.T, rev.isa0,
                                      np.asarray(rev.C, np.uint64), d_r.data_ptr(), device=device)
    sa, blocks = index_io.read_sa(prefix), index_io.read_blocks(prefix)
    gi.set_sa(sa, blocks)
    vals = np.asarray(sa.values, np.uint32)
    gi.set_sa64(np.where(vals == np.uint32(0xFFFFFFFF), np.uint64(ONES), vals.astype(np.uint64)), sa.interval,
                blocks.astype(np.uint64))
    gi.set_text(*index_io.read_packed_dna(prefix))
    return gi, read_chromosomes(prefix)[0]


# ---------------------------------------------------------------- the option switch's side effects
def post_switch_skips(lens, n_n, polyat, first, maxdiff_of, thr0):
    """The records from `first` on (the one after the first read without a hit) that
    bwa_cal_sa_reg_gap skips at bwtaln.c:314-317.  After the switch aux->opt is &local_opt, so
    :331 writes each searched read's max_diff into local_opt.max_diff, the value :316 compares
    the next read's N count with: the threshold is the max_diff of the latest searched read,
    thr0 (the batch's) until there is one.  A skipped read and a poly-A/T read (:324-325) leave
    it as it is.  maxdiff_of(len): bwa_cal_maxdiff for fnr > 0 (never more than thr0)."""
    cur, out = thr0, []
    for r in range(first, len(lens)):
        if n_n[r] > cur:
            out.append(r)
        elif not polyat[r]:
            cur = maxdiff_of(int(lens[r]))
    return out


@functools.lru_cache(maxsize=8)
def _table(fnr: float):
    return reads.maxdiff_table(fnr, TABLE_LEN)


def _maxdiff_of(opt):
    if opt["fnr"] > 0:
        t = _table(opt["fnr"])
        return lambda l: int(t[l]) if l < len(t) else reads.cal_maxdiff(l, reads.BWA_AVG_ERR, opt["fnr"])
    return lambda l: opt["max_diff"]


# ---------------------------------------------------------------- loading a batch
def _host_segment(p, thr, md_of, seed_len):
    """The arrays of a parse_host result as the device loader would leave them: a read is
    stored whole, and everything the search sees is of its trimmed length."""
    n = len(p["names"])
    rec = np.zeros((n, 4), np.uint32)
    jobs, codes, names, quals, has_q, full, bcs = [], [], [], [], [], [], []
    off = 0
    for k in range(n):
        sq, ln = p["seqs"][k], p["lens"][k]
        nn = int((sq[:ln] > 3).sum())
        poly = ln >= 15 and bool((sq[:15] == 0).all() or (sq[:15] == 3).all())
        st = HSA_RD_NDROP if nn > thr else HSA_RD_POLYAT if poly else HSA_RD_SEARCHED
        rec[k] = (st, ln, nn, len(jobs) if st == HSA_RD_SEARCHED else 0xFFFFFFFF)
        if st == HSA_RD_SEARCHED:
            jobs.append((off, ln, md_of(ln), seed_len if seed_len < ln else SEED_NONE, 0))
            off += len(sq)
            codes.append(sq)
            names.append(p["names"][k])
            quals.append(p["quals"][k] or b"")
            has_q.append(p["quals"][k] is not None)
            full.append(len(sq))
            bcs.append(p["bcs"][k])
    nb, noff = sam.pack_strings(names)
    qb, qoff = sam.pack_strings(quals)
    return dict(rec=rec, jobs=np.array(jobs, JOB_DTYPE) if jobs else np.zeros(0, JOB_DTYPE),
                codes=np.concatenate(codes) if codes else np.zeros(0, np.uint8), names=nb, name_off=noff, quals=qb,
                qual_off=qoff, has_qual=np.array(has_q, bool), max_all=max(p["lens"], default=0),
                full_len=np.array(full, np.uint32), bc=np.frombuffer(b"".join(bcs), np.uint8))


def _load_batch(gi, data, pos, opt, d_table, batch_reads, window):
    """Records of `data` from `pos` on, up to batch_reads: (segments in read order, the
    offset after them, the window size to go on with).  A device segment is a load_device
    result, a host segment a parse_host result.  Both readers take the reader's options of opt;
    a record they skip (the Casava filter, a read not longer than the barcode) does not count."""
    segs, have, host_n = [], 0, 1
    rd = dict(mode=opt["mode"] & MODE_READER, trim_qual=opt["trim_qual"])
    while have < batch_reads and pos < len(data):
        w = min(len(data) - pos, window)
        at_eof = pos + w == len(data)
        t = reads.load_device(gi, reads.upload(data[pos:pos + w]), w, at_eof, batch_reads - have, opt["max_diff"],
                              opt["seed_len"], maxdiff=d_table, **rd)
        c, got = t["ctr"], t["n_loaded"]
        if t["n_rows"]:
            segs.append(dict(kind="dev", t=t, span=(pos, w, at_eof, batch_reads - have)))
            have += got
        pos += c["consumed"]
        if c["bad_record"] != ONES:
            host_n = 1 if got else min(2 * host_n, 1 << 20)     # (more at a time while the device takes nothing)
            p = reads.parse_host(data, min(host_n, batch_reads - have), start=pos, **rd)
            if p["names"] or p["filtered"]:
                segs.append(dict(kind="host", p=p))
                have += len(p["names"])
            pos = p["consumed"]
            if p["end"] == -2:               # the reference's batch ends at a truncated quality (bwaseqio.c:175)
                break
            if p["end"] == -1:
                pos = len(data)
        elif got == 0 and c["consumed"] == 0:
            if at_eof:
                pos = len(data)
            else:
                window *= 2                  # a record longer than the window
    return segs, pos, window


def _load_batch_bam(gi, src, pos, opt, d_table, batch_reads, window, stats):
    """_load_batch for the BAM text of src (dict: text, d_text or None, cand: the anchor
    candidates as offsets in the text, which): records from the record start `pos` on, through
    hsa_bam_reads_device (bam.load_device) on a window of the resident text, or of the host
    text uploaded when the inflater left none.  Anchors: the window's start and the candidates
    inside the window behind it.  A call that ends on an anchor that is not on the chain keeps
    what it loaded (exact up to there), and the rest of the batch is loaded with the
    single-anchor walk.  A record the device does not take goes through bam.parse_host, and
    the loader goes on behind it.  A truncated or inconsistent record ends the input:
    stats["bam_truncated"]."""
    from ._lib import HSA_BAM_END_ANCHOR, HSA_BAM_END_MALFORMED
    text, cand, which = src["text"], src["cand"], src["which"]
    segs, have, host_n, serial = [], 0, 1, False
    while have < batch_reads and pos < len(text):
        w = min(len(text) - pos, window)
        at_eof = pos + w == len(text)
        d_in, first = (src["d_text"], pos) if src["d_text"] is not None else (reads.upload(text[pos:pos + w]), 0)
        inside = cand[(cand > pos) & (cand < pos + w)] - np.uint64(pos) if not serial else cand[:0]
        anchors = np.concatenate([np.zeros(1, np.uint64), inside.astype(np.uint64)])
        room = batch_reads - have

        def call(floor=0, d_in=d_in, first=first, w=w, at_eof=at_eof, room=room, anchors=anchors):
            return bam.load_device(gi, d_in, w, at_eof, room, opt["max_diff"], opt["seed_len"], anchors=anchors, which=which,
                                   maxdiff=d_table, trim_qual=opt["trim_qual"], first=first, len_floor=floor)
        t = call()
        c, got, reason = t["ctr"], t["n_loaded"], t["bctr"]["reason"]
        stats["bam_segments"] += len(anchors)
        stats["bam_segments_verified"] += t["bctr"]["segments_verified"]
        if len(anchors) == 1:
            stats["bam_serial_records"] += t["n_rows"]
        if t["n_rows"]:
            segs.append(dict(kind="dev", t=t, span=(pos, w, at_eof, room), reload=call,
                             host=lambda t, pos=pos: bam.parse_host(text[pos:pos + t["ctr"]["consumed"]], None, which=which,
                                                                    trim_qual=opt["trim_qual"])))
            have += got
        pos += c["consumed"]
        if reason == HSA_BAM_END_ANCHOR:
            serial = True
        elif reason == HSA_BAM_END_MALFORMED:
            stats["bam_truncated"] = 1
            return segs, len(text), window
        elif c["bad_record"] != ONES:
            host_n = 1 if got else min(2 * host_n, 1 << 20)
            p = bam.parse_host(text, min(host_n, batch_reads - have), start=pos, which=which, trim_qual=opt["trim_qual"])
            if p["names"] or p["filtered"]:
                segs.append(dict(kind="host", p=p))
                have += len(p["names"])
            pos = p["consumed"]
            if p["end"] == -2:
                stats["bam_truncated"] = 1
                return segs, len(text), window
        elif t["n_rows"] == 0 and c["consumed"] == 0:
            if at_eof:
                pos = len(text)
            else:
                window *= 2                  # a record longer than the window
    return segs, pos, window


def _merge(gi, data, segs, opt, d_table):
    """One device batch of the segments: the tensors of load_device's keys, the per-record
    rows on the host (job indices of the batch; the records the reader skipped have none),
    has_qual per job, the batch's threshold; with trimming full_len, with a barcode bc and
    bc_len (hsa_amd.chain's optional batch keys); the reader's statistics."""
    import torch
    from ._lib import HSA_RD_FILTERED
    md_of = _maxdiff_of(opt)
    rd = dict(mode=opt["mode"] & MODE_READER, trim_qual=opt["trim_qual"])
    bc_len = rd["mode"] >> 24
    max_all = max([s["t"]["ctr"]["max_loaded"] if s["kind"] == "dev" else max(s["p"]["lens"], default=0) for s in segs])
    thr = md_of(max_all)                                   # local_opt.max_diff, bwtaln.c:273-274
    dev = chain.to_device
    parts = []
    reader = dict(filtered=0, trimmed_bases=0, total_bases=0)
    for s in segs:
        if s["kind"] == "dev":
            t, n_rec = s["t"], s["t"]["n_rows"]
            rec = t["rec"][:4 * n_rec].cpu().numpy().view(np.uint32).reshape(-1, 4).copy()
            if opt["fnr"] > 0 and t["ctr"]["threshold"] != (thr & ONES) and \
                    ((rec[:, 0] == HSA_RD_NDROP) & (rec[:, 2].astype(np.int64) <= thr)).any():
                pos, w, at_eof, room = s["span"]           # the chunk alone set a narrower threshold
                if max_all < TABLE_LEN:
                    t = s["reload"](max_all) if "reload" in s else \
                        reads.load_device(gi, reads.upload(data[pos:pos + w]), w, at_eof, room, opt["max_diff"], opt["seed_len"],
                                          maxdiff=d_table, len_floor=max_all, **rd)
                    assert t["n_rows"] == n_rec and t["ctr"]["threshold"] == (thr & ONES)
                    rec = t["rec"][:4 * n_rec].cpu().numpy().view(np.uint32).reshape(-1, 4).copy()
                elif "host" in s:
                    s = dict(kind="host", p=s["host"](t))
                else:
                    s = dict(kind="host", p=reads.parse_host(data[pos:pos + t["ctr"]["consumed"]], t["n_loaded"], **rd))
        if s["kind"] == "dev":
            c, n = t["ctr"], t["n_jobs"]
            reader["filtered"] += t["octr"]["filtered"]
            reader["trimmed_bases"] += t["octr"]["trimmed_bases"]
            reader["total_bases"] += t["octr"]["total_bases"]
            rec = rec[rec[:, 0] != HSA_RD_FILTERED]
            parts.append(dict(rec=rec, n=n, full_len=t["full_len"][:n], bc=t["bc"][:n * bc_len], jobs=t["jobs"][:n * JOB_DTYPE.itemsize], codes=t["codes"][:c["code_wanted"] - 16],
                              names=t["names"][:c["name_wanted"]], quals=t["quals"][:c["qual_wanted"]],
                              name_off=t["name_off"][:n + 1], qual_off=t["qual_off"][:n + 1], has_qual=np.ones(n, bool)))
        else:
            h = _host_segment(s["p"], thr, md_of, opt["seed_len"])
            n = len(h["jobs"])
            for k in reader:
                reader[k] += s["p"][k]
            parts.append(dict(rec=h["rec"], n=n, full_len=dev(h["full_len"]), bc=dev(h["bc"]), jobs=dev(h["jobs"]), codes=dev(h["codes"]), names=dev(h["names"]),
                              quals=dev(h["quals"]), name_off=dev(h["name_off"]), qual_off=dev(h["qual_off"]),
                              has_qual=h["has_qual"]))
    jobs, name_off, qual_off, recs = [], [], [], []
    nj = cb = nb = qb = 0
    for p in parts:
        if p["n"]:
            j = p["jobs"].contiguous().clone().view(torch.int64).view(-1, 3)
            j[:, 0] += cb                                   # hsa_job_t.off
            jobs.append(j.view(-1).view(torch.uint8))
        name_off.append(p["name_off"][:-1] + nb)
        qual_off.append(p["qual_off"][:-1] + qb)
        r = p["rec"].copy()
        r[r[:, 0] == HSA_RD_SEARCHED, 3] += np.uint32(nj)
        recs.append(r)
        nj, cb, nb, qb = nj + p["n"], cb + len(p["codes"]), nb + len(p["names"]), qb + len(p["quals"])
    end = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda")
    pad = torch.zeros(64, dtype=torch.uint8, device="cuda")
    rec = np.concatenate(recs)
    kept = rec[rec[:, 0] == HSA_RD_SEARCHED, 1]
    extra = dict(reader=reader)
    full = torch.cat([p["full_len"].view(torch.int32) for p in parts] + [pad[:4].view(torch.int32)])
    extra["max_full"] = int(full[:nj].max().item()) if nj else 0
    if opt["trim_qual"] >= 1:                               # (without the options the writers run their plain entry points)
        extra["full_len"] = full
    if bc_len:
        extra.update(bc=torch.cat([p["bc"] for p in parts] + [pad[:1]]), bc_len=bc_len)
    return dict(extra, jobs=torch.cat(jobs + [pad[:24]]), codes=torch.cat([p["codes"] for p in parts] + [pad]),
                names=torch.cat([p["names"] for p in parts] + [pad[:1]]), quals=torch.cat([p["quals"] for p in parts] + [pad[:1]]),
                name_off=torch.cat(name_off + [end(nb)]), qual_off=torch.cat(qual_off + [end(qb)]), n_jobs=nj, rec=rec,
                has_qual=np.concatenate([p["has_qual"] for p in parts]), thr=thr, max_all=max_all,
                max_len=int(kept.max()) if len(kept) else 0)


# ---------------------------------------------------------------- search, choose, refine (hsa_amd.chain)
def _runs(flags, first, end):
    """[first, end) cut into runs of equal flags."""
    out, s = [], first
    for j in range(first + 1, end + 1):
        if j == end or flags[j] != flags[s]:
            out.append((s, j - s))
            s = j
    return out if end > first else []


def _splice_hits(t, s, first, cnt, stats):
    """The search tensors t with the unspliced results of the splice search s appended as
    hits, for jobs [first, first + cnt): a result that is not two records of type
    BWA_TYPE_SPLICING goes through bwt_aln2seq_core like a main-search hit (bwtse.c:901-907).
    Its bwt_aln1_t records (9 words) become hsa_aln64_t records (14 words) behind the
    search's own, two slots per read, and the read's n_aln and hit_off point at them; all on
    the device.  t itself is left as it is (the lines stage reads the search's n_aln)."""
    import torch
    k, ks = first - t["first"], first - s["sp_first"]
    r = s["res"][ks * SP_RES_WORDS:(ks + cnt) * SP_RES_WORDS].view(cnt, SP_RES_WORDS)
    sent = ((s["sp_flags"][ks:ks + cnt] & 1) != 0) & (s["sp_n_aln"][ks:ks + cnt] == 0)
    spliced = (r[:, 1] == 2) & ((r[:, 7] & 0x3FFFFFFF) == TYPE_SPLICING)
    idx = torch.nonzero(sent & (r[:, 0] == 0) & (r[:, 1] >= 1) & (r[:, 1] <= 2) & ~spliced).view(-1)
    if idx.numel() == 0:
        return t
    rec = r[idx, 2:].reshape(-1, 2, 9)
    w = torch.zeros((idx.numel(), 2, ALN64_WORDS), dtype=torch.int32, device="cuda")
    for dst, src in ((0, 0), (1, 5), (2, 1), (4, 2), (6, 3), (8, 4), (10, 6), (11, 7), (12, 8)):
        w[:, :, dst] = rec[:, :, src]                       # (k, l, rev_k, rev_l: the low words; the high ones are 0)
    cap = t["hit_cap"]
    n_aln, hit_off = t["n_aln"].clone(), t["hit_off"].clone()
    n_aln[k + idx] = r[idx, 1]
    hit_off[k + idx] = cap + 2 * torch.arange(idx.numel(), device="cuda")
    stats["spliced_unspliced"] += int(idx.numel())
    return dict(t, n_aln=n_aln, hit_off=hit_off, hit_cap=cap + 2 * idx.numel(),
                hits=torch.cat([t["hits"][:cap * ALN64_WORDS], w.view(-1), t["hits"][cap * ALN64_WORDS:]]))


def _splice_lines(gi, b, s, first, cnt, chrs, has_qual, opt, stats):
    """hsa_splice_lines_device_xa over jobs [first, first + cnt): (its output tensors, the bytes
    of its text, line_stat on the host, the names of the reads it refused).  The text's room
    allows for the lists of the extra pairs the first run serves (chain.xa_room);
    chain.splice_lines runs again with what the counters ask for."""
    import torch
    from ._lib import HSA_SL_NONE, HSA_SL_NOPAIR, HSA_SL_OK
    strings = dict(names=b["names"], name_off=b["name_off"][first:], chrs=chrs["chrs"], chr_off=chrs["chr_off"])
    if has_qual:
        strings.update(quals=b["quals"], qual_off=b["qual_off"][first:])
    noff = b["name_off"][first:first + cnt + 1].cpu().numpy().view(np.uint64)
    max_name = int(np.diff(noff.astype(np.int64)).max()) if cnt else 0
    stride = 33                                             # two segments' ops and the N
    # (a list has at most 49 entries, each a chromosome, a position and a merged CIGAR)
    max_line = max(1, sam.line_bound(max_name, b["max_full"], chrs["max_chr"], stride, 0, 49, "full_len" in b, b.get("bc_len", 0)))
    ks = first - s["sp_first"]
    n_two = int((s["res"][ks * SP_RES_WORDS:(ks + cnt) * SP_RES_WORDS].view(cnt, SP_RES_WORDS)[:, 1] == 2).sum())
    cap = n_two * (max_name + 2 * b["max_full"] + chrs["max_chr"] + b.get("bc_len", 0) + 200) + 64
    cap += chain.xa_room(cnt) * (chrs["max_chr"] + 64)      # the lists of the extra pairs the first run has room for
    o, ctr = chain.splice_lines(gi, b, s, first, cnt, strings, chrs["n"], max_line, cap, cigar_stride=stride,
                                max_top2=opt["max_top2"], comp_read=bool(opt["mode"] & MODE_COMPREAD))
    stat = o["stat"].cpu().numpy().view(np.uint32)[:cnt]
    stats["lines"] += int(ctr[2])
    stats["spliced"] += int(ctr[2])
    stats["handed_back"] += int(ctr[3])
    stats["spliced_multi"] += int(ctr[4])                    # (none once the extra pairs had room)
    stats["spliced_xa"] += int(o["xa"][2])
    stats["spliced_xa_entries"] += int(o["xa"][3])
    stats["spliced_refused"] += int(ctr[5])
    stats["spliced_no_pair"] += int(ctr[6])
    names = b["names"]
    refused = [bytes(names[int(noff[j]):int(noff[j + 1])].cpu().numpy().tobytes())
               for j in np.flatnonzero((stat != HSA_SL_OK) & (stat != HSA_SL_NONE) & (stat != HSA_SL_NOPAIR))]
    return o, int(ctr[1]), stat, refused


def _run_batch(gi, chr_names, b, opt, out, state, stats, splice=False, junctions=None):
    """Steps 2 to 5 for a merged batch; returns the generator's state and, per job, whether
    it got a line.  junctions: a junctions.Accumulator that takes the rows of every
    splice-lines call, or None."""
    import torch
    n = b["n_jobs"]
    local, n_stacks, rg_b = chain.local_regime(opt, b["max_all"])      # bwtaln.c:254, :273-276
    assert local["max_diff"] == b["thr"]
    if splice and n_stacks > HSA_SP_MAX_STACKS:
        raise ValueError(f"the splice path with {n_stacks} score buckets (over {HSA_SP_MAX_STACKS}) is not built")
    opt["mode"] &= ~MODE_GAPE                               # :261, through aux->opt: it stays
    has_line = np.zeros(n, bool)
    if n == 0:
        return state, has_line
    rg_a = regime_of(opt, n_stacks, local["max_diff"])
    rec = b["rec"]
    rec_of_job = np.flatnonzero(rec[:, 0] == HSA_RD_SEARCHED)
    lens = rec[rec_of_job, 1].astype(np.int64)
    # bwtaln.c:332 writes through aux->opt: before the switch opt->seed_len itself turns to
    # "none" at the first searched read that is not longer than it, and stays
    s0 = opt["seed_len"]
    plain = np.where(lens > s0, s0, SEED_NONE).astype(np.int32)
    short = np.flatnonzero(lens <= s0)
    sticky = plain.copy()
    if len(short):
        sticky[short[0]:] = SEED_NONE
    col = b["jobs"][:n * JOB_DTYPE.itemsize].view(torch.int32).view(-1, 6)[:, 4]
    set_seeds = lambda a: col.copy_(torch.from_numpy(a).cuda())
    max_seed = s0 if 0 < s0 < b["max_len"] else 0
    if not np.array_equal(sticky, plain):
        set_seeds(sticky)
    t1 = chain.search64(gi, b, 0, n, rg_a, max_seed)
    fb = np.flatnonzero(t1["flags"].cpu().numpy() & 1)
    switch = int(fb[0]) if len(fb) else n                  # the first read without a hit
    kept_sticky = len(short) and short[0] <= min(switch, n - 1)
    if kept_sticky:
        opt["seed_len"] = SEED_NONE
    parts = _runs(b["has_qual"], 0, min(switch + 1, n))
    s1 = s2 = None
    if splice:
        # bwt_splice_match always gets &local_opt (bwtaln.c:363).  For the first read without a
        # hit :331 wrote the read's own max_diff through aux->opt, which was still the caller's
        # block: local_opt.max_diff is the batch's there.  From the next read on aux->opt is
        # &local_opt and :331 writes each read's own into it.
        srg = chain.splice_regimes(local, n_stacks)
        if switch < n:
            jobs1 = b["jobs"][:(switch + 1) * JOB_DTYPE.itemsize].clone()
            jobs1.view(torch.int32).view(-1, 6)[switch, 3] = local["max_diff"]
            s1 = chain.splice32(gi, b, t1, 0, switch + 1, srg, jobs=jobs1)
            stats["spliced_sent"] += int(s1["sp_ctr"][0])
    parts = [(t1, f, c, s1) for f, c in parts]
    stats["searched"] += n
    if switch < n - 1:
        first2 = switch + 1
        seeds2 = sticky if kept_sticky else plain
        t2 = t1
        if bytes(rg_a) != bytes(rg_b) or not np.array_equal(seeds2[first2:], sticky[first2:]):
            if not np.array_equal(seeds2, sticky):
                set_seeds(seeds2)
            t2 = chain.search64(gi, b, first2, n - first2, rg_b, max_seed)
            stats["searched_again"] += n - first2
        if opt["fnr"] > 0:
            md_of = _maxdiff_of(opt)
            r0 = int(rec_of_job[switch]) + 1
            if (rec[r0:, 2].astype(np.int64) > min(md_of(int(l)) for l in np.unique(rec[r0:, 1]))).any():
                skip = post_switch_skips(rec[:, 1], rec[:, 2], rec[:, 0] == HSA_RD_POLYAT, r0, md_of, b["thr"])
                jobs = [int(rec[r, 3]) for r in skip if rec[r, 0] == HSA_RD_SEARCHED]
                if jobs:                                    # the reference did not search them: no hits
                    if t2 is t1:
                        t2 = dict(t1, n_aln=t1["n_aln"].clone(), flags=t1["flags"].clone())
                    at = torch.tensor(jobs, device="cuda") - t2["first"]
                    t2["n_aln"][at] = 0
                    t2["flags"][at] = 0                     # ... and did not send them to bwt_splice_match
                    stats["n_drop_after_switch"] += len(jobs)
        if splice:
            s2 = chain.splice32(gi, b, t2, first2, n - first2, srg)
            stats["spliced_sent"] += int(s2["sp_ctr"][0])
        parts += [(t2, f, c, s2) for f, c in _runs(b["has_qual"], first2, n)]
    if splice:
        cb, coff = sam.pack_strings(chr_names)
        up = lambda a: chain.to_device(a if len(a) else np.zeros(1, a.dtype))
        chrs = dict(chrs=up(cb), chr_off=up(coff), n=len(chr_names),
                    max_chr=int(np.diff(coff.astype(np.int64)).max()) if len(chr_names) else 0)
    for t, first, cnt, s in parts:
        if s is not None:
            t = _splice_hits(t, s, first, cnt, stats)
        sub, state = chain.choose64(gi, b, t, first, cnt, state)
        m = chain.refine64(gi, sub)
        q = (b["quals"], b["qual_off"][first:]) if b["has_qual"][first] else None
        text, off, stat, ctr = sam.device_sam(gi, m, (b["names"], b["name_off"][first:]), q, chr_names, max_top2=opt["max_top2"],
                                              comp_read=bool(opt["mode"] & MODE_COMPREAD), on_device=s is not None)
        if s is not None:
            # the two writers' lines in read order (hsa_sam_merge_device), then one copy to the host
            o2, written2, stat2, refused = _splice_lines(gi, b, s, first, cnt, chrs, bool(b["has_qual"][first]), opt, stats)
            if junctions is not None:
                junctions.add(o2, cnt)
            mo, mc = chain.sam_merge(gi, cnt, (text, int(ctr[1]), off), (o2["out"], written2, o2["line_off"]))
            assert int(mc[0]) == int(mc[1]) == int(ctr[1]) + written2
            out.write(mo["out"][:int(mc[1])].cpu().numpy().tobytes())
            stats["refused_names"] += refused
            stat = np.where(stat2 == 0, 0, stat)
        else:
            out.write(text)
        has_line[first:first + cnt] = stat == 0
        stats["lines"] += int(ctr[2])
        stats["refused"] += int(ctr[4]) + int(ctr[5]) + int(ctr[6])
    return state, has_line


def _read_input(data_or_path) -> bytes:
    if isinstance(data_or_path, (bytes, bytearray, memoryview)):
        return bytes(data_or_path)
    with open(data_or_path, "rb") as f:
        head = f.read(2)
    op = gzip.open if head == b"\x1f\x8b" else open          # (the reference reads through zlib: either way)
    with op(data_or_path, "rb") as f:
        return f.read()


def align_fastq(gi, chr_names, data_or_path, opts, out, batch_reads=BATCH_READS, rng_state=HSA_DRAND48_SEED0, unaligned=None,
                splice=False, junctions=None, junction_threshold=None):
    """FASTQ (bytes, or a path; gzip is read through Python's gzip), or with the BAM bit of
    opts["mode"] a BAM file (bytes or a path; the module docstring), to SAM text written to
    `out` (a binary file object), as the module docstring states it.  opts: an option dict
    (default_opts / parse_options), not modified.  unaligned: a binary file object for the
    reads without a line.  splice: send the reads without a main-search hit through the splice
    path and print its lines too (the module docstring's contract).  junctions: a binary file
    object that receives the run's splice junction table after the last batch (hsa_amd.junctions;
    with splice only, ValueError otherwise; junction_threshold: the rows after which the device
    row buffer is compacted, junctions.Accumulator's default when None); the statistics then
    gain junction_rows and junctions.  Returns (the drand48 state after the last read,
    statistics)."""
    import collections
    import torch
    if junctions is not None and not splice:
        raise ValueError("--junctions goes with --splice: the table is made of the spliced reads' lines")
    opt = dict(opts)
    opt.setdefault("trim_qual", 0)
    is_bam = bool(opt["mode"] & MODE_BAM)
    if opt["mode"] & ~(MODE_GAPE | MODE_COMPREAD | MODE_LOGGAP | MODE_NONSTOP | MODE_READER | MODE_BAM_ALL):
        raise ValueError("a mode bit that is not built")
    src = None
    if is_bam:
        # -B, -I and -Y have no effect on BAM input (bwaseqio.c:172): accepted and ignored
        src = dict(which=bam.which_of(opt["mode"]))
        opt["mode"] &= ~(MODE_BAM_ALL | MODE_READER)
        src["text"], src["d_text"], src["cand"], inflate = bam.open_text(gi, data_or_path)
        data = src["text"]
    else:
        opt["mode"] &= ~MODE_BAM_ALL                         # -0, -1, -2 without -b: the file is opened as FASTQ (bwtaln.c:441)
        data = _read_input(data_or_path)
    if (opt["mode"] >> 24) > reads.BWA_MAX_BCLEN or opt["trim_qual"] > reads.MAX_TRIM_QUAL:
        raise ValueError(f"a barcode of at most {reads.BWA_MAX_BCLEN} bases, trim_qual at most {reads.MAX_TRIM_QUAL}")
    rd = dict(mode=opt["mode"] & MODE_READER, trim_qual=opt["trim_qual"])
    if not opt["mode"] & MODE_COMPREAD:
        raise ValueError("colour-space reads (-c) are not built")
    if splice:
        if gi.is64():
            raise ValueError("the splice path for a text of 2^32 characters or more is not built")
        if opt["fnr"] <= 0 and chain.local_regime(opt, 0)[1] > HSA_SP_MAX_STACKS:
            raise ValueError(f"the splice path with more than {HSA_SP_MAX_STACKS} score buckets is not built")
    d_table = torch.from_numpy(_table(opt["fnr"])).cuda() if opt["fnr"] > 0 else None
    stats = collections.Counter(reads=0, searched=0, searched_again=0, n_drop=0, polyat=0, n_drop_after_switch=0, lines=0,
                                refused=0, batches=0, device_records=0, host_records=0, filtered=0, trimmed_bases=0, total_bases=0)
    if splice:
        stats.update(spliced_sent=0, spliced=0, spliced_unspliced=0, spliced_no_pair=0, handed_back=0, spliced_multi=0,
                     spliced_refused=0, spliced_xa=0, spliced_xa_entries=0)
        stats["refused_names"] = []
    acc = None
    if junctions is not None:
        from .junctions import Accumulator
        acc = Accumulator(gi, chr_names, **({} if junction_threshold is None else dict(threshold=junction_threshold)))
    pos, state, window = 0, int(rng_state), max(4 << 20, 1024 * int(batch_reads))
    if is_bam:
        stats.update({"inflate_" + k: v for k, v in inflate.items()})
        stats.update(bam_segments=0, bam_segments_verified=0, bam_serial_records=0, bam_truncated=0)
        pos, window = bam.read_header(data)[0], max(1 << 20, 256 * int(batch_reads))
    while pos < len(data):
        start = pos
        if is_bam:
            segs, pos, window = _load_batch_bam(gi, src, pos, opt, d_table, int(batch_reads), window, stats)
        else:
            segs, pos, window = _load_batch(gi, data, pos, opt, d_table, int(batch_reads), window)
        if not segs:
            break                                           # bwa_read_seq returned no read: bwtaln.c:477 ends
        b = _merge(gi, data, segs, opt, d_table)
        rec = b["rec"]
        stats["batches"] += 1
        stats["reads"] += len(rec)
        stats["n_drop"] += int((rec[:, 0] == HSA_RD_NDROP).sum())
        stats["polyat"] += int((rec[:, 0] == HSA_RD_POLYAT).sum())
        stats.update(b["reader"])                           # (a Counter: adds)
        stats["device_records"] += sum(s["t"]["n_loaded"] for s in segs if s["kind"] == "dev")
        stats["host_records"] += sum(len(s["p"]["names"]) for s in segs if s["kind"] == "host")
        state, has_line = _run_batch(gi, chr_names, b, opt, out, state, stats, splice=splice, junctions=acc)
        if unaligned is not None:
            p = bam.parse_host(data[start:pos], len(rec), which=src["which"], trim_qual=opt["trim_qual"]) if is_bam else \
                reads.parse_host(data[start:pos], len(rec), **rd)
            assert len(p["names"]) == len(rec)
            for r in range(len(rec)):
                if rec[r, 0] == HSA_RD_SEARCHED and has_line[int(rec[r, 3])]:
                    continue
                seq, qual = p["orig"][r]                     # the record as given: barcode and quality offset included
                if qual is None:
                    unaligned.write(b">" + p["names"][r] + b"\n" + seq + b"\n")
                else:
                    unaligned.write(b"@" + p["names"][r] + b"\n" + seq + b"\n+\n" + qual + b"\n")
    stats["no_line"] = stats["reads"] - stats["lines"]
    if acc is not None:
        junctions.write(acc.finish())                       # (an empty table for a run without a spliced line)
        stats["junction_rows"], stats["junctions"] = acc.fed, acc.distinct
    return state, dict(stats)


def sam_header(prefix: str) -> bytes:
    """The @SQ lines of the index, in the reference's format (bwt_print_sam_SQ)."""
    names, lens = read_chromosomes(prefix)
    return "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(names, lens)).encode()


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    try:
        opts, rest, extra = parse_options(argv, reader_options=True, bam_options=True)
    except Exception as e:                                  # getopt's and ours
        print(f"hsa_amd.align: {e}", file=sys.stderr)
        return 1
    if len(rest) < 2:
        print("usage: python -m hsa_amd.align [bwa-aln options] [--header] [--unaligned FILE] [--splice [--junctions FILE]] [-f OUT] "
              "<prefix> <in.fq | -b in.bam>",
              file=sys.stderr)
        return 1
    if "junctions" in extra and not extra.get("splice"):
        print("hsa_amd.align: --junctions goes with --splice", file=sys.stderr)
        return 1
    gi, chrs = open_index64(rest[0])
    out = open(extra["out"], "wb") if extra["out"] else sys.stdout.buffer
    un = open(extra["unaligned"], "wb") if extra["unaligned"] else None
    jn = open(extra["junctions"], "wb") if "junctions" in extra else None
    try:
        if extra["header"]:
            out.write(sam_header(rest[0]))
        _, stats = align_fastq(gi, chrs, rest[1], opts, out, unaligned=un, splice=extra.get("splice", False), junctions=jn)
        out.flush()
    except bam.BamError as e:                               # a file that is not BAM
        print(f"hsa_amd.align: {e}", file=sys.stderr)
        return 1
    finally:
        if un:
            un.close()
        if jn:
            jn.close()
        if extra["out"]:
            out.close()
        gi.close()
    if opts["trim_qual"] >= 1 and stats["total_bases"]:       # bwaseqio.c:224-225
        print(f"[hsa_amd.align] {100.0 * stats['trimmed_bases'] / stats['total_bases']:.1f}% bases are trimmed.", file=sys.stderr)
    print("[hsa_amd.align] " + ", ".join(f"{k} {v}" for k, v in stats.items() if k != "refused_names"), file=sys.stderr)
    if stats.get("bam_truncated"):                            # the reads before it are aligned (bam_read1 < 0 ends the reference's loop)
        print("hsa_amd.align: the BAM input ends in a truncated or inconsistent record", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
