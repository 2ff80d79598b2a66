"""Reads from unaligned BAM: bwa_read_bam (bwaseqio.c:105-157) over bamlite's bam_read1, with one
departure, the rule of DESIGN.md ("BAM input").

The rule.  bwa_read_bam differs from bwa_read_seq in one harmful way: line 142 reverses p->seq
"to be reversed back in bwa_refine_gapped", and that reverse-back is commented out in this
reference (bwtse.c:545), as is the matching line of the FASTQ reader (bwaseqio.c:214).  The
reference's -b therefore searches every read backwards, a left-over of the code it was derived
from.  Here a BAM record is read exactly as bwa_read_bam reads it, except that line 142 is not
applied: a record gives the bwa_seq_t the FASTQ reader gives for the equivalent FASTQ record.

Per record (parse_host is the restatement, hsa_bam_reads_device the batch path):
* selection (bwtaln.c:441-447, bwaseqio.c:118-121): `which` is 4 for -0, 1 for -1, 2 for -2,
  OR-ed, and 7 when none is given; a record is taken when which & 1 and FLAG has 0x40, or
  which & 2 and FLAG has 0x80, or which & 4 and FLAG has neither.  Nothing else in FLAG
  filters: secondary (0x100) and supplementary (0x800) records are read, as the reference
  reads them;
* bases through bam_nt16_nt4_table (:29): 1, 2, 4, 8 are 0..3, everything else ('=' too) 4;
* qualities q + 33 < 126 ? q + 33 : 126 (:133): a record without qualities (0xFF) has '~';
* with FLAG 0x10 the codes are reverse-complemented and the qualities reversed (:135-138)
  before anything else looks at them; -q trims with bwa_trim_read after that (:139);
* the name is the l_read_name bytes up to the first NUL (strdup, :144); no /1 or /2 is cut;
* -B, -I and -Y have no effect (bwa_read_bam takes only is_comp and trim_qual): no barcode;
* a record with l_seq == 0 is no read: skipped and counted as `filtered`, like a record the
  selection skips;
* a truncated or inconsistent record ends the input there, as bam_read1 returning < 0 ends the
  reference's loop: end == -2.

The container is read as bamlite reads it, through gzread (open_text): BGZF on the device
(hsa_amd.bgzf), one general gzip stream through Python's gzip, or uncompressed bytes."""
from __future__ import annotations

import gzip
import struct

import numpy as np

from . import bgzf, reads

MODE_BAM, MODE_BAM_SE, MODE_BAM_READ1, MODE_BAM_READ2 = 0x20, 0x40, 0x80, 0x100      # bwtaln.h:127-130
MODE_BAM_ALL = MODE_BAM | MODE_BAM_SE | MODE_BAM_READ1 | MODE_BAM_READ2
FLAG_REVERSE, FLAG_READ1, FLAG_READ2 = 0x10, 0x40, 0x80
FIXED = 36                       # block_size and the 32 bytes of the core
HOP_OK, HOP_INCOMPLETE, HOP_MALFORMED = range(3)

# bam_nt16_nt4_table (bwaseqio.c:29)
NT16_NT4 = np.array([4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4], np.uint8)
_COMP = np.array([3, 2, 1, 0, 4], np.uint8)
_LETTERS = np.frombuffer(b"ACGTN", np.uint8)


class BamError(ValueError):
    """A BAM file that cannot be opened as one: a bad magic, a header the text does not hold."""


def which_of(mode: int) -> int:
    """bwtaln.c:442-446."""
    w = (4 if mode & MODE_BAM_SE else 0) | (1 if mode & MODE_BAM_READ1 else 0) | (2 if mode & MODE_BAM_READ2 else 0)
    return w or 7


def selected(which: int, flag: int) -> bool:
    """bwaseqio.c:118-121."""
    r1, r2 = bool(flag & FLAG_READ1), bool(flag & FLAG_READ2)
    return bool((which & 1 and r1) or (which & 2 and r2) or (which & 4 and not r1 and not r2))


def read_header(text):
    """(the header's length, [(name, length) per reference]) of the BAM text: magic, l_text,
    text, n_ref, then per reference l_name, name, l_ref.  BamError (a ValueError) on a bad magic (as
    bam_header_read reports one) or a header the text does not hold whole."""
    text = memoryview(text)
    if bytes(text[:4]) != b"BAM\x01":
        raise BamError("invalid BAM binary header (bad magic)")
    try:
        l_text = struct.unpack_from("<i", text, 4)[0]
        if l_text < 0:
            raise struct.error
        pos = 8 + l_text
        n_ref = struct.unpack_from("<i", text, pos)[0]
        pos += 4
        refs = []
        for _ in range(max(n_ref, 0)):
            l_name = struct.unpack_from("<i", text, pos)[0]
            if l_name < 0 or pos + 4 + l_name + 4 > len(text):
                raise struct.error
            name = bytes(text[pos + 4:pos + 4 + l_name]).split(b"\0")[0]
            refs.append((name, struct.unpack_from("<i", text, pos + 4 + l_name)[0]))
            pos += 8 + l_name
    except struct.error:
        raise BamError("truncated BAM header") from None
    return pos, refs


def record_at(text, pos):
    """The hop check of hsa_bam.h (bam_hop) at offset pos: (status, dict of the record's fields
    and offsets or None).  OK: l_read_name >= 1, block_size >= 32 + l_read_name + 4 n_cigar +
    (l_seq + 1) / 2 + l_seq, and the record ends inside the text."""
    n = len(text)
    if pos > n or n - pos < 24:
        return HOP_INCOMPLETE, None
    block_size, = struct.unpack_from("<I", text, pos)
    l_read_name = text[pos + 12]
    n_cigar, flag, l_seq = struct.unpack_from("<HHI", text, pos + 16)
    if l_read_name == 0 or block_size < 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:
        return HOP_MALFORMED, None
    if n - pos < 4 + block_size:
        return HOP_INCOMPLETE, None
    name = pos + FIXED
    seq = name + l_read_name + 4 * n_cigar
    return HOP_OK, dict(flag=flag, l_seq=l_seq, l_read_name=l_read_name, name=name, seq=seq, qual=seq + (l_seq + 1) // 2,
                        end=pos + 4 + block_size)


def decode(text, r):
    """(name, codes, qualities) of the record r (record_at) as bwa_read_bam leaves them before
    its line 142: the read in its own orientation."""
    L = r["l_seq"]
    name = bytes(text[r["name"]:r["name"] + r["l_read_name"]]).split(b"\0")[0]
    packed = np.frombuffer(text, np.uint8, (L + 1) // 2, r["seq"])
    codes = NT16_NT4[np.stack([packed >> 4, packed & 15], 1).reshape(-1)[:L]]
    q = np.frombuffer(text, np.uint8, L, r["qual"]).astype(np.int64) + 33
    qual = np.where(q < 126, q, 126).astype(np.uint8)
    if r["flag"] & FLAG_REVERSE:
        codes, qual = _COMP[codes[::-1]], qual[::-1]
    return name, np.ascontiguousarray(codes), qual.tobytes()


def parse_host(text, max_records=None, start=0, which=7, trim_qual=0):
    """bwa_read_bam, without its line 142, over the BAM records of `text` (bytes) from the
    record start `start`, at most max_records reads: what reads.parse_host returns, so
    align._host_segment takes it unchanged.  names, seqs (uint8 codes), quals, lens (the trimmed
    lengths), raw and orig (the read as FASTQ text, in its own orientation: what --unaligned
    writes), bcs (all b""), consumed, end (0 max_records reached, -1 the end of the input, -2 a
    truncated or inconsistent record, where consumed stays at its start), filtered (records the
    selection skips and records with l_seq == 0: they count towards no batch), trimmed_bases,
    total_bases."""
    text = bytes(text)
    names, seqs, quals, raw, lens, orig = [], [], [], [], [], []
    pos, end, filtered = int(start), 0, 0
    while max_records is None or len(names) < max_records:
        if pos == len(text):
            end = -1
            break
        st, r = record_at(text, pos)
        if st != HOP_OK:
            end = -2
            break
        pos = r["end"]
        if not selected(which, r["flag"]) or r["l_seq"] == 0:
            filtered += 1
            continue
        name, codes, qual = decode(text, r)
        seq = _LETTERS[codes].tobytes()                       # ("ACGTN"[code]: what --unaligned writes)
        names.append(name)
        seqs.append(codes)
        quals.append(qual)
        raw.append(seq)
        orig.append((seq, qual))
        lens.append(reads.trim_read(trim_qual, qual, len(codes)))
    total = sum(len(s) for s in seqs)
    return dict(names=names, seqs=seqs, quals=quals, raw=raw, consumed=pos, end=end, lens=lens, bcs=[b""] * len(names),
                orig=orig, filtered=filtered, total_bases=total, trimmed_bases=total - sum(lens))


# ---------------------------------------------------------------- the device path
def load_device(gi, d_in, n_in, at_eof, max_records, max_diff, seed_len, anchors=(0,), which=7, maxdiff=None, regime=0, caps=None,
                trim_qual=0, first=0, len_floor=0, rows=None):
    """hsa_bam_reads_device on bytes [first, first + n_in) of the device tensor d_in, which
    start at a record: reads.load_device's result (the same keys; bc empty, bc_len 0) with
    bctr, the BAM counters by _lib.BAM_COUNTERS' names.  anchors: ascending offsets inside the
    bytes, the first 0 (ValueError otherwise), at which records are expected to start.  rows:
    the most records looked at (the rows of rec); by default every record the bytes can hold.
    The call runs again with the counters' sizes when a capacity was short."""
    import torch
    from ._lib import BAM_COUNTERS, JOB_DTYPE, RD_COUNTERS, RD_OPT_COUNTERS, RD_ROW_WORDS, BamBatch
    n_in, max_records = int(n_in), int(max_records)
    anchors = np.asarray(anchors, np.uint64).reshape(-1)
    if len(anchors) < 1 or anchors[0] != 0 or (np.diff(anchors.astype(np.int64)) < 0).any() or int(anchors[-1]) > n_in:
        raise ValueError("anchors: ascending offsets inside the bytes, the first one 0")
    rows = min(n_in // 37 + 1, 1 << 28) if rows is None else int(rows)
    cap = dict(jobs=min(max_records, n_in // 37 + 1), codes=n_in + 32, names=n_in // 2 + 32, quals=n_in + 32)
    cap.update(caps or {})
    d_anchor = torch.from_numpy(anchors.view(np.int64).copy()).cuda()
    rec = torch.zeros(max(rows, 1) * RD_ROW_WORDS, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda")
    octr = torch.zeros(len(RD_OPT_COUNTERS), dtype=torch.int64, device="cuda")
    bctr = torch.zeros(len(BAM_COUNTERS), dtype=torch.int64, device="cuda")
    for _ in range(2):
        o = dict(jobs=torch.zeros(max(cap["jobs"], 1) * JOB_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
                 codes=torch.zeros(max(cap["codes"], 1), dtype=torch.uint8, device="cuda"),
                 names=torch.zeros(max(cap["names"], 1), dtype=torch.uint8, device="cuda"),
                 quals=torch.zeros(max(cap["quals"], 1), dtype=torch.uint8, device="cuda"),
                 name_off=torch.zeros(cap["jobs"] + 1, dtype=torch.int64, device="cuda"),
                 qual_off=torch.zeros(cap["jobs"] + 1, dtype=torch.int64, device="cuda"),
                 full_len=torch.zeros(max(cap["jobs"], 1), dtype=torch.int32, device="cuda"),
                 bc=torch.zeros(1, dtype=torch.uint8, device="cuda"))
        b = BamBatch(d_in=d_in.data_ptr() + int(first), n_in=n_in, at_eof=int(bool(at_eof)), max_records=max_records,
                     which=int(which), trim_qual=int(trim_qual), max_diff=int(max_diff),
                     d_maxdiff=maxdiff.data_ptr() if maxdiff is not None else None,
                     n_maxdiff=len(maxdiff) if maxdiff is not None else 0, len_floor=int(len_floor), seed_len=int(seed_len),
                     regime=int(regime), d_anchor=d_anchor.data_ptr(), n_anchor=len(anchors), d_jobs=o["jobs"].data_ptr(),
                     job_cap=cap["jobs"], d_codes=o["codes"].data_ptr(), code_cap=cap["codes"], d_names=o["names"].data_ptr(),
                     name_cap=cap["names"], d_name_off=o["name_off"].data_ptr(), d_quals=o["quals"].data_ptr(),
                     qual_cap=cap["quals"], d_qual_off=o["qual_off"].data_ptr(), d_full_len=o["full_len"].data_ptr(),
                     d_rec=rec.data_ptr(), rec_cap=max(rows, 1), d_counters=ctr.data_ptr(), d_opt_counters=octr.data_ptr(),
                     d_bam_counters=bctr.data_ptr())
        torch.cuda.synchronize()
        gi.bam_reads_device(b)
        torch.cuda.synchronize()
        c = dict(zip(RD_COUNTERS, (int(v) for v in ctr.cpu().numpy().view(np.uint64))))
        short = [k for k, w in (("jobs", "jobs"), ("codes", "code"), ("names", "name"), ("quals", "qual"))
                 if c[w + "_wanted"] > c[w + "_written"]]
        if not short:
            break
        cap = dict(jobs=c["jobs_wanted"], codes=c["code_wanted"], names=c["name_wanted"], quals=c["qual_wanted"])
    o.update(n_jobs=c["jobs_written"], max_len=c["max_kept"], rec=rec, ctr=c, n_loaded=c["loaded"], consumed=c["consumed"],
             caps=cap, bc_len=0, octr=dict(zip(RD_OPT_COUNTERS, (int(v) for v in octr.cpu().numpy().view(np.uint64)))),
             bctr=dict(zip(BAM_COUNTERS, (int(v) for v in bctr.cpu().numpy().view(np.uint64)))))
    o["n_rows"] = o["octr"]["rows"]
    return o


def open_text(gi, path_or_bytes):
    """The inflated bytes of a BAM file (a path, or the file's bytes) as bamlite's gzread gives
    them: (the text as host bytes, the text as a uint8 device tensor or None, the anchor
    candidates, statistics).  BGZF goes through bgzf.inflate_device, and the resident tensor is
    kept when all of it was inflated in one group; any other gzip stream through Python's gzip;
    bytes that begin "BAM\\1" are taken as they are.  The anchor candidates are the member
    table's output offsets (uint64, ascending, empty for the other two): where htslib starts a
    record whenever it fits.  Statistics: bgzf.NO_STATS' keys."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    none = np.zeros(0, np.uint64)
    if data[:2] != bgzf.MAGIC:
        return data, None, none, dict(bgzf.NO_STATS)
    t = bgzf.scan(data)
    if t is None:
        return gzip.decompress(data), None, none, dict(bgzf.NO_STATS)
    text, d_text, stats = bgzf.inflate_device(gi, data, table=t)
    return text, d_text, np.unique(t["out_off"][t["isize"] > 0].astype(np.uint64)), stats
