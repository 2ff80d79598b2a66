"""Reads from FASTQ / FASTA text: the head of the reference's pipeline, bwa_read_seq
(bwaseqio.c:161-231) over kseq_read (kseq.h:155-193).

Two ways to the same reads:
* parse_host: a restatement of kseq_read + bwa_read_seq in Python for any input the reference
  accepts (records over several lines, FASTA, blank lines, CRLF).  It is the text the device
  loader is tested against and the fallback for the bytes the device loader refuses.
* load_device: the batch path.  GpuIndex.reads_device_opts (hsa_reads_device_opts) parses the canonical
  records of a chunk that sits in device memory and leaves the search batch, the names and the
  qualities on the device; load_device uploads nothing itself (upload() does), sizes the
  outputs, runs the call, and runs it again with the counters' sizes when room was short.

Both take the reader's options: quality trimming (-q), barcodes (-B), the Casava filter (-Y)
and Illumina-1.3 qualities (-I), as bwa_read_seq applies them.  BAM input (-b) is hsa_amd.bam's:
bwa_read_bam takes none of these options but the trimming.
An input that ends in a lone header character reads as
ended (the reference's answer there depends on the file size modulo its 4 096-byte buffer)."""
from __future__ import annotations

import math
import re

import numpy as np

BWA_AVG_ERR = 0.02               # bwtaln.h:25
SEED_NONE = 0x7FFFFFFF
MODE_CFY, MODE_IL13 = 0x08, 0x200  # bwtaln.h:125, :131; the barcode length is mode >> 24
BWA_MIN_RDLEN = 35               # bwtaln.h:26: bwa_trim_read leaves at least this many bases
BWA_MAX_BCLEN = 63               # bwtaln.h:28
BARCODE_LOW_QUAL = 13            # bwaseqio.c:159
# the most trim_qual for which a read's sum of trim_qual - (q - 33), q - 33 in -31..94, fits int32
MAX_TRIM_QUAL = 0x7FFFFFFF // 65535 - 94

# nst_nt4_table (bwaseqio.c:10-27)
NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    NT4[_c] = NT4[_c | 0x20] = _i
NT4[ord("-")] = 5

_HEADER = re.compile(rb"[>@]")
_SPACE = re.compile(rb"[ \t\n\v\f\r]")                       # isspace in the C locale
_SEQ_STOP = re.compile(rb"[>+@]")
_NOT_GRAPH = bytes(c for c in range(256) if not 33 <= c <= 126)
_QUAL_OK = bytes(range(33, 128))


def cal_maxdiff(l: int, err: float = BWA_AVG_ERR, thres: float = 0.04) -> int:
    """bwa_cal_maxdiff (bwtaln.c:46-58); x is the reference's int and wraps as it does."""
    el = math.exp(-l * err)
    y, x, s = 1.0, 1, el
    for k in range(1, 1000):
        y *= l * err
        x = ((x * k + 0x80000000) & 0xFFFFFFFF) - 0x80000000
        t = el * y
        s += t / x if x else (math.nan if t == 0.0 or t != t else math.inf)      # (34! is 0 in 32 bits)
        if 1.0 - s < thres:
            return k
    return 2


def maxdiff_table(fnr: float, n: int) -> np.ndarray:
    """bwa_cal_maxdiff(l, BWA_AVG_ERR, fnr) for l = 0 .. n - 1, as int32: the table
    hsa_reads_device indexes by a read's length."""
    return np.array([cal_maxdiff(l, BWA_AVG_ERR, fnr) for l in range(n)], np.int32)


def _kseq_read(data, pos, last_char, comment=None):
    """One kseq_read call on `data` from `pos`: (ret, name, seq, qual, pos, last_char); ret
    is the sequence length, -1 at the end of the input, -2 for a truncated quality.  comment:
    a list that receives the record's comment (kseq.h:167; empty when the name ends its line)."""
    n = len(data)
    if last_char == 0:                                        # kseq.h:160-164
        m = _HEADER.search(data, pos)
        if not m:
            return -1, b"", b"", None, n, 0
        last_char, pos = data[m.start()], m.end()
    if comment is not None:
        comment[:] = [b""]                                    # :165
    if pos >= n:                                              # :166, ks_getuntil at the end
        return -1, b"", b"", None, n, last_char
    m = _SPACE.search(data, pos)
    if m:
        name, c, pos = data[pos:m.start()], data[m.start()], m.end()
    else:
        name, c, pos = data[pos:], 0, n
    if c != 0x0A:                                             # :167 the comment
        j = data.find(b"\n", pos)
        if comment is not None:
            comment[:] = [data[pos:j if j >= 0 else n]]
        pos = j + 1 if j >= 0 else n
    m = _SEQ_STOP.search(data, pos)                           # :168-177
    seq = data[pos:m.start() if m else n].translate(None, _NOT_GRAPH)
    c, pos = (data[m.start()], m.end()) if m else (-1, n)
    if c in (0x3E, 0x40):
        last_char = c                                         # :178
    if c != 0x2B:
        return len(seq), name, seq, None, pos, last_char      # :180 FASTA
    j = data.find(b"\n", pos)                                 # :185
    if j < 0:
        return -2, name, seq, None, n, last_char              # :186
    pos = j + 1
    want = len(seq)
    qual = data[pos:pos + want]
    if len(qual) == want and not qual.translate(None, _QUAL_OK):
        pos = min(pos + want + 1, n)                          # (the byte after the last one is read and dropped)
    else:                                                     # :187-188 byte by byte
        q = bytearray()
        while pos < n:
            c = data[pos]
            pos += 1
            if len(q) >= want:
                break
            if 33 <= c <= 127:
                q.append(c)
        qual = bytes(q)
    if len(qual) != want:
        return -2, name, seq, qual, pos, 0                    # :190-191
    return want, name, seq, qual, pos, 0


def casava_filtered(comment: bytes) -> bool:
    """bwaseqio.c:176-181: the comment, a C string, holds a ':' and the byte after the first
    one is 'Y'."""
    c = comment.split(b"\0")[0]
    i = c.find(b":")
    return i >= 0 and c[i + 1:i + 2] == b"Y"


def trim_read(trim_qual: int, qual, length: int) -> int:
    """bwa_trim_read (bwaseqio.c:92-103): the length the read keeps."""
    if trim_qual < 1 or qual is None:
        return length
    s = best = 0
    best_l = length
    for l in range(length - 1, BWA_MIN_RDLEN - 1, -1):
        s += trim_qual - (qual[l] - 33)
        if s < 0:
            break
        if s > best:
            best, best_l = s, l
    return best_l


def parse_host(data, max_records=None, start=0, mode=0, trim_qual=0):
    """bwa_read_seq over kseq_read for `data` (bytes) from offset `start`, at most max_records records:
    dict(names: list of bytes (comment cut, a trailing /1 or /2 removed, bwaseqio.c:217-220),
    seqs: list of uint8 code arrays (nst_nt4_table), quals: list of bytes or None (FASTA),
    raw: the sequences' bytes as given, consumed: the offset parsing goes on from, end: 0 max_records reached, -1 the end of the
    input, -2 a truncated quality (where the reference ends its batch, bwaseqio.c:175)).

    mode (gap_opt_t.mode: MODE_CFY, MODE_IL13, the barcode length in the top byte) and
    trim_qual as bwa_read_seq takes them, in its order per record (:176-211): a record the
    Casava filter takes, or one not longer than the barcode, is skipped and counted in
    `filtered` (it does not count towards max_records); with MODE_IL13 31 comes off every
    quality byte; the barcode comes off the front of sequence and quality (bcs: its bases,
    lower case where the quality is under 13, else upper; b"" without a barcode); then
    bwa_trim_read.  seqs, quals and raw stay whole (full_len, without the barcode); lens holds
    p->len, the trimmed lengths, the only length the search sees.  orig: (sequence, quality)
    as the record gave them.  trimmed_bases / total_bases: what the reference reports."""
    data = bytes(data)
    mode, trim_qual = int(mode), int(trim_qual)
    l_bc = (mode >> 24) & 0xFF
    if l_bc > BWA_MAX_BCLEN:
        raise ValueError(f"the maximum barcode length is {BWA_MAX_BCLEN}")
    names, seqs, quals, raw, lens, bcs, orig = [], [], [], [], [], [], []
    pos, last, end, filtered = int(start), 0, 0, 0
    comment = [b""]
    while max_records is None or len(names) < max_records:
        ret, name, seq, qual, pos, last = _kseq_read(data, pos, last, comment)
        if ret < 0:
            end = ret
            break
        if mode & MODE_CFY and comment[0] and casava_filtered(comment[0]):
            filtered += 1
            continue
        qual = qual if qual else None                         # (seq->qual.l == 0)
        if ret <= l_bc:
            filtered += ret > 0                               # (an empty record is no read at all)
            continue                                          # :185
        orig.append((seq, qual))
        if mode & MODE_IL13 and qual is not None:
            qual = bytes(c - 31 for c in qual)                # :183-184
        bc = b""
        if l_bc:                                              # :187-199
            low = [qual is not None and qual[i] - 33 < BARCODE_LOW_QUAL for i in range(l_bc)]
            bc = bytes((seq[i:i + 1].lower() if low[i] else seq[i:i + 1].upper())[0] for i in range(l_bc))
            seq = seq[l_bc:]
            qual = qual[l_bc:] if qual is not None else None
        name = name.split(b"\0")[0]                           # strdup, :216
        if len(name) > 2 and name[-2:] in (b"/1", b"/2"):
            name = name[:-2]
        names.append(name)
        seqs.append(NT4[np.frombuffer(seq, np.uint8)])
        quals.append(qual)                                    # :208
        raw.append(seq)
        bcs.append(bc)
        lens.append(trim_read(trim_qual, qual, len(seq)))     # :210
    if last:                                                  # the next record's header character was read
        pos -= 1
    total = sum(len(s) for s in seqs)
    return dict(names=names, seqs=seqs, quals=quals, raw=raw, consumed=pos, end=end, lens=lens, bcs=bcs, orig=orig,
                filtered=filtered, total_bases=total, trimmed_bases=total - sum(lens))


# ---------------------------------------------------------------- the device path
def upload(data):
    """The bytes of a chunk as a uint8 tensor on the device."""
    import torch
    a = np.frombuffer(bytes(data), np.uint8)
    return torch.from_numpy(a.copy() if len(a) else np.zeros(1, np.uint8)).cuda()


def load_device(gi, d_in, n_in, at_eof, max_records, max_diff, seed_len, maxdiff=None, regime=0, caps=None, mode=0,
                trim_qual=0, first=0, len_floor=0):
    """hsa_reads_device_opts on bytes [first, first + n_in) of the device tensor d_in: a dict of
    device tensors by the keys device_sam and the search take (jobs, codes, n_jobs, max_len,
    names, name_off, quals, qual_off) and rec (the per-record rows), ctr (the counters by
    _lib.RD_COUNTERS' names), n_loaded, consumed.  mode, trim_qual: the reader's options as
    parse_host takes them; then also full_len (u32 per job: the stored length, jobs' len being
    the trimmed one), bc and bc_len (the barcodes at stride bc_len), n_rows (the rows of rec:
    the loaded records with the filtered ones, which n_loaded leaves out) and octr (the
    counters by _lib.RD_OPT_COUNTERS' names).  maxdiff: the device tensor (int32) of
    maxdiff_table for fnr > 0, or None; len_floor: the longest read of the batch's other
    chunks.  caps: capacities by jobs / codes / names / quals,
    for a caller that knows better than the bounds taken here (no record is shorter than 8
    bytes, a read's bases are under half its record); the call runs again with the
    counters' sizes when one was short."""
    import torch
    from ._lib import JOB_DTYPE, RD_COUNTERS, RD_OPT_COUNTERS, RD_ROW_WORDS, ReadsBatch
    n_in, max_records, mode = int(n_in), int(max_records), int(mode) & 0xFFFFFFFF
    bc_len = mode >> 24
    # with a filter the call may look at every record of the chunk to find max_records it keeps
    rows = min(n_in // 8 + 1, 1 << 28) if bc_len or mode & MODE_CFY else max_records
    cap = dict(jobs=min(max_records, n_in // 8 + 1), codes=n_in // 2 + 32, names=n_in // 2 + 32, quals=n_in // 2 + 32)
    cap.update(caps or {})
    rec = torch.zeros(max(rows, max_records) * RD_ROW_WORDS, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda")
    octr = torch.zeros(len(RD_OPT_COUNTERS), dtype=torch.int64, device="cuda")
    for _ in range(2):
        o = dict(jobs=torch.zeros(max(cap["jobs"], 1) * JOB_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
                 codes=torch.zeros(max(cap["codes"], 1), dtype=torch.uint8, device="cuda"),
                 names=torch.zeros(max(cap["names"], 1), dtype=torch.uint8, device="cuda"),
                 quals=torch.zeros(max(cap["quals"], 1), dtype=torch.uint8, device="cuda"),
                 name_off=torch.zeros(cap["jobs"] + 1, dtype=torch.int64, device="cuda"),
                 qual_off=torch.zeros(cap["jobs"] + 1, dtype=torch.int64, device="cuda"),
                 full_len=torch.zeros(max(cap["jobs"], 1), dtype=torch.int32, device="cuda"),
                 bc=torch.zeros(max(cap["jobs"] * bc_len, 1), dtype=torch.uint8, device="cuda"))
        b = ReadsBatch(d_in=d_in.data_ptr() + int(first), n_in=n_in, at_eof=int(bool(at_eof)), max_records=max_records,
                       max_diff=int(max_diff), d_maxdiff=maxdiff.data_ptr() if maxdiff is not None else None,
                       n_maxdiff=len(maxdiff) if maxdiff is not None else 0, len_floor=int(len_floor), seed_len=int(seed_len), regime=int(regime),
                       trim_qual=int(trim_qual), mode=mode, d_jobs=o["jobs"].data_ptr(), job_cap=cap["jobs"],
                       d_codes=o["codes"].data_ptr(), code_cap=cap["codes"], d_names=o["names"].data_ptr(),
                       name_cap=cap["names"], d_name_off=o["name_off"].data_ptr(), d_quals=o["quals"].data_ptr(),
                       qual_cap=cap["quals"], d_qual_off=o["qual_off"].data_ptr(), d_rec=rec.data_ptr(),
                       d_counters=ctr.data_ptr(), d_full_len=o["full_len"].data_ptr(), d_bc=o["bc"].data_ptr(), rec_cap=rows,
                       d_opt_counters=octr.data_ptr())
        torch.cuda.synchronize()
        gi.reads_device_opts(b)
        torch.cuda.synchronize()
        c = dict(zip(RD_COUNTERS, (int(v) for v in ctr.cpu().numpy().view(np.uint64))))
        short = [k for k, w in (("jobs", "jobs"), ("codes", "code"), ("names", "name"), ("quals", "qual"))
                 if c[w + "_wanted"] > c[w + "_written"]]
        if not short:
            break
        cap = dict(jobs=c["jobs_wanted"], codes=c["code_wanted"], names=c["name_wanted"], quals=c["qual_wanted"])
    o.update(n_jobs=c["jobs_written"], max_len=c["max_kept"], rec=rec, ctr=c, n_loaded=c["loaded"], consumed=c["consumed"],
             caps=cap, bc_len=bc_len, octr=dict(zip(RD_OPT_COUNTERS, (int(v) for v in octr.cpu().numpy().view(np.uint64)))))
    o["n_rows"] = o["octr"]["rows"]
    return o
