"""The SAM line of an unspliced single-end read with a hit, as bwa_print_sam1 prints it
with mate == NULL (bwtse.c:698-799), from the device's outputs: the choice
(GpuIndex.choose_hits64: the read's d_sel and d_sel64 words), its rows (row 0 the chosen
one, rows 1.. the XA list) and their refinement (GpuIndex.refine_rows64).

Two ways to the same bytes:
* sam_line: one read, in Python, from NumPy slices of arrays copied to the host.  It is the
  per-read restatement, the text the batch path is tested against, and far too slow for a
  batch (an interpreter call per read).
* device_sam: the batch path.  GpuIndex.sam_lines64 (hsa_sam_lines_device64) writes every
  line of a batch into device memory in read order; device_sam uploads the strings (names,
  qualities, chromosome names, laid out by pack_strings), sizes the output, runs the call
  and returns the text after one copy to the host.

spliced_line is the same restatement for a spliced read (type BWA_TYPE_SPLICING, XT:A:S):
the text hsa_splice_lines_device (hsa_amd/csrc/hsa_splice_rows.hip) is tested against.

A trimmed read (bwa aln -q) and a barcode (-B) reach both: SEQ and QUAL over the whole read,
bwa_correct_trimmed on the line's own CIGAR, BC:Z and XC:i behind QUAL.  Not printed: the RG
tag (no read group reaches the 64-bit path)."""
from __future__ import annotations

import numpy as np

from . import refine

SAM_FSR = 16
XT = "NURMS"                 # bwtse.c:762
SEQ_FWD, SEQ_REV = "ACGTN", "TGCAN"      # bwtse.c:737-742


def _record(rec):
    """n_mm, n_gapo, n_gape, strand of an hsa_aln64_t."""
    w0, w1 = int(rec[0]), int(rec[1])
    return w0 & 0xFFFF, (w0 >> 16) & 0xFF, (w0 >> 24) & 0xFF, (w1 >> 30) & 3


def clipped_cigar(ops, strand, clip) -> str:
    """The CIGAR column of bwa_cigar_t words `ops` after bwa_correct_trimmed (bwtse.c:496-534):
    the `clip` bases trimming took off join a last S op on the forward strand, a first one on
    the reverse strand, or are an S op of their own there."""
    ops = [(int(w) >> 28, int(w) & 0x0FFFFFFF) for w in np.asarray(ops, np.uint32).reshape(-1)]
    if clip:
        at = 0 if strand else len(ops) - 1
        if ops and ops[at][0] == 4:
            ops[at] = (4, ops[at][1] + clip)
        else:
            ops.insert(0 if strand else len(ops), (4, clip))
    return "".join(f"{l}{CIGAR_OPS[op]}" for op, l in ops)


def clip_tags(clip_len, full_len, bc) -> list:
    """The tags between QUAL and XT (bwtse.c:755-758)."""
    out = [f"BC:Z:{bc.decode('latin-1') if isinstance(bc, bytes) else bc}"] if bc else []
    return out + ([f"XC:i:{clip_len}"] if clip_len < full_len else [])


def sam_line(name, seq_codes, qual, chr_names, sel, sel64, rows, rpos, cigar, md, pos, hits, max_top2=30,
             flag=0, comp_read=True, clip_len=None, bc=None) -> str:
    """One line, without the newline.

    seq_codes: the read as it was given (codes 0-4); qual: its quality string or None;
    chr_names: chromosome names by the position rows' chrID (HSP chrName by seq_id); sel, sel64: the read's 4 + 4 words of the choice; rows, rpos, cigar,
    md, pos: the read's rows of the refinement and of the position arrays, chosen row
    first; hits: the hit record of each of those rows (d_hits[d_hit_off[j] + d_pos_hit[t]]);
    max_top2: gap_opt_t.max_top2 (X1 is printed when X0 <= max_top2); comp_read:
    BWA_MODE_COMPREAD (NM, else CM).  clip_len: the length the read was trimmed to and searched
    with (bwa aln -q; seq_codes and qual stay whole), or None; bc: its barcode (-B), or None."""
    typ, _, mapq, n_xa = (int(v) for v in np.asarray(sel).reshape(-1)[:4])
    _, c1, c2, _ = (int(v) for v in np.asarray(sel64).reshape(-1)[:4])
    if typ not in (1, 2):
        raise ValueError("the read has no hit: the reference prints no line for it")
    rows, rpos, pos, hits = np.asarray(rows), np.asarray(rpos), np.asarray(pos), np.asarray(hits)
    if len(rows) < 1 + n_xa:
        raise ValueError(f"{1 + n_xa} rows wanted, {len(rows)} given")
    seq_codes = np.asarray(seq_codes, np.uint8)
    n_mm, n_gapo, n_gape, strand = _record(hits[0])
    main = refine.row_sam(rows[0], cigar[0], md[0])
    if main["status"] != 0:
        raise ValueError(f"the chosen row was not answered (status {main['status']})")
    if strand:
        flag |= SAM_FSR
    full = len(seq_codes)
    clip_len = full if clip_len is None else int(clip_len)
    n_cigar = int(np.asarray(rows[0], np.uint32).reshape(-1)[1])
    text = clipped_cigar(np.asarray(cigar[0]).reshape(-1)[:n_cigar], strand, full - clip_len) if clip_len < full else main["cigar"]
    out = [name, str(flag), chr_names[int(pos[0][1])], str(int(rpos[0][1])), str(mapq), text, "*", "0", "0"]
    if strand == 0:
        out.append("".join(SEQ_FWD[c] for c in seq_codes))
    else:
        out.append("".join(SEQ_REV[c] for c in seq_codes[::-1]))
    out.append("*" if qual is None else (qual[::-1] if strand else qual))
    out += clip_tags(clip_len, full, bc)
    out += [f"XT:A:{XT[typ]}", f"{'NM' if comp_read else 'CM'}:i:{main['nm']}", f"X0:i:{c1}"]
    if c1 <= max_top2:
        out.append(f"X1:i:{c2}")
    out += [f"XM:i:{n_mm}", f"XO:i:{n_gapo}", f"XG:i:{n_gapo + n_gape}", f"MD:Z:{main['md']}"]
    if n_xa:
        # bwtse.c:781-796: an entry with a CIGAR (a gapped one, :551-557) prints neither its
        # difference count nor the ';', an ungapped one prints ",<gap + mm>;" and no CIGAR
        xa = []
        for t in range(1, 1 + n_xa):
            q_mm, q_gapo, q_gape, q_strand = _record(hits[t])
            r = refine.row_sam(rows[t], cigar[t], md[t])
            if r["status"] != 0:
                raise ValueError(f"XA row {t} was not answered (status {r['status']})")
            xa.append(f"{chr_names[int(pos[t][1])]},{'-' if q_strand else '+'}{int(rpos[t][1])}")
            xa.append(r["cigar"] if q_gapo + q_gape else f",{q_gapo + q_gape + q_mm};")
        out.append("XA:Z:" + "".join(xa))
    return "\t".join(out)


CIGAR_OPS = "MIDNSHP=X"      # bwtse.c:713


def spliced_line(name, seq_codes, qual, chr_name, ori_pos, cigar, strand, c1, c2, n_mm, max_top2=30, flag=0,
                 comp_read=True, clip_len=None, bc=None, xa=None) -> str:
    """The line of a spliced read (bwa_print_sam1 for type BWA_TYPE_SPLICING, bwtse.c:677-799),
    without the newline.

    chr_name, ori_pos: segment 0's chromosome and 1-based position; cigar: the merged CIGAR
    as (op, length) pairs, op an index into "MIDNSHP=X" (hsa_amd.splice.merge_cigar); strand:
    res_aln[0]'s; c1, c2: the capped row count bwt_aln2pos_splicing leaves in both
    (bwtse.c:310-315); n_mm: mm of segment 0 plus mm of segment 1 (:594).  mapQ is 0 (the
    value of :345 is dropped), NM is 0 (nm is never computed for these reads), XO and XG are
    0 (gap is never set), and there is no MD.  clip_len, bc: as sam_line takes them (the
    segments lie in the trimmed read).  xa: the read's further splice pairs
    (hsa_amd.splice.multi_entries: chromosome name, strand, 1-based position, merged CIGAR as
    (op, length) pairs), printed as the reference does (:782-797): "<chr>,<+|-><position>"
    and the CIGAR's ops from "MIDNS" directly behind it, no edit count, no ';', the entries
    abutting; bwa_correct_trimmed does not touch these CIGARs."""
    seq_codes = np.asarray(seq_codes, np.uint8)
    if strand:
        flag |= SAM_FSR
    full = len(seq_codes)
    clip_len = full if clip_len is None else int(clip_len)
    text = clipped_cigar([(int(op) << 28) | int(l) for op, l in cigar], strand, full - clip_len)
    out = [name, str(flag), chr_name, str(int(ori_pos)), "0", text, "*", "0", "0"]
    if strand == 0:
        out.append("".join(SEQ_FWD[c] for c in seq_codes))
    else:
        out.append("".join(SEQ_REV[c] for c in seq_codes[::-1]))
    out.append("*" if qual is None else (qual[::-1] if strand else qual))
    out += clip_tags(clip_len, full, bc)
    out += [f"XT:A:{XT[4]}", f"{'NM' if comp_read else 'CM'}:i:0", f"X0:i:{int(c1)}"]
    if c1 <= max_top2:
        out.append(f"X1:i:{int(c2)}")
    out += [f"XM:i:{int(n_mm)}", "XO:i:0", "XG:i:0"]
    if xa:
        out.append("XA:Z:" + "".join(f"{c},{'-' if st else '+'}{int(pos)}" + "".join(f"{int(l)}{'MIDNS'[op]}" for op, l in cg)
                                     for c, st, pos, cg in xa))
    return "\t".join(out)


# ---------------------------------------------------------------- the batch path
def pack_strings(items):
    """Strings (str or bytes) laid out for the device: (their bytes end to end as a uint8
    array, len(items) + 1 u64 offsets).  Pure NumPy; item k is bytes[off[k]:off[k + 1]]."""
    raw = [x.encode("ascii") if isinstance(x, str) else bytes(x) for x in items]
    off = np.zeros(len(raw) + 1, np.uint64)
    if raw:
        off[1:] = np.cumsum([len(x) for x in raw], dtype=np.uint64)
    return np.frombuffer(b"".join(raw), np.uint8).copy(), off


def line_bound(max_name, max_len, max_chr, cigar_stride, md_stride, max_xa, trimmed=False, bc_len=0) -> int:
    """An upper bound of a line's length with its newline (hsa_sam_batch64_t.max_line): every
    number at the most digits its type has (u32: 10, u64: 20, a CIGAR length 9, n_mm 5, a
    gap count 3), cut to the most the call takes.  max_len: the longest stored read.  trimmed:
    reads may be trimmed (one more CIGAR op and the XC tag); bc_len: the BC tag's bytes."""
    from ._lib import HSA_SAM_MAX_LINE
    cigar = 10 * cigar_stride
    max_name += (10 + 6 + 10 if trimmed else 0) + (6 + bc_len if bc_len else 0)
    n = (max_name + 1 + 10 + 1 + max_chr + 1 + 20 + 1 + 10 + 1 + cigar + 7 + max_len + 1 + max(max_len, 1)
         + 7 + 6 + 10 + 6 + 20 + 6 + 20 + 6 + 5 + 6 + 3 + 6 + 3 + 6 + md_stride + 1)
    if max_xa:
        n += 6 + max_xa * (max_chr + 2 + 20 + max(cigar, 7))
    return min(n, HSA_SAM_MAX_LINE)


def device_sam(gi, dev, names, quals, chr_names, max_top2=30, flag=0, comp_read=True, on_device=False, full_len=None, bc=None):
    """The SAM text of a batch: (text as bytes, line_off (n + 1 u64), line_stat (n u32),
    counters (8 u64)) of one hsa_sam_lines_device64 call, run a second time with
    counters[0] bytes of room when the first reports wanted > written.

    dev: the device tensors of search, choose and refine by the keys of hsa_amd.chain (the
    dict chain.refine64 returns, or any dict with those keys).  names: the reads' names
    (FASTQ comment cut); quals: their quality strings, or None ("*"); chr_names: by chrID.
    Names and qualities that are on the device already (hsa_amd.reads.load_device) are given
    as a pair of tensors instead of a list: (the bytes, the n + 1 u64 offsets of these reads; a
    sub-range's offsets are a view from its first read on).  on_device: the text and line_off stay
    device tensors (the text's first counters[1] bytes hold).  full_len: a device tensor of
    the reads' stored lengths (u32 per job; jobs' len is then the trimmed length), or None;
    bc: (a device tensor of the reads' barcodes, the bytes per read), or None.  Both default
    to what dev holds (hsa_amd.chain's optional batch keys)."""
    import torch
    from . import chain
    from ._lib import JOB_DTYPE
    n = int(dev["n_jobs"])
    if full_len is not None:
        dev = dict(dev, full_len=full_len)
    if bc is not None:
        dev = dict(dev, bc=bc[0], bc_len=int(bc[1]))
    on_dev = isinstance(names, tuple)
    if quals is not None and on_dev != isinstance(quals, tuple):
        raise ValueError("names and qualities come both as lists or both as device tensors")
    if not on_dev and (len(names) != n or (quals is not None and len(quals) != n)):
        raise ValueError(f"{n} reads, {len(names)} names" + ("" if quals is None else f", {len(quals)} qualities"))

    up = lambda a: chain.to_device(a if len(a) else np.zeros(1, a.dtype))       # (no null pointer for an empty array)
    cb, coff = pack_strings(chr_names)
    if on_dev:
        noff = names[1][:n + 1].cpu().numpy().view(np.uint64)
        nb = np.zeros(int(noff[-1] - noff[0]) if n else 0, np.uint8)        # (its length sizes the room below)
        t = dict(names=names[0], name_off=names[1], chrs=up(cb), chr_off=up(coff))
        if quals is not None:
            t.update(quals=quals[0], qual_off=quals[1])
    else:
        nb, noff = pack_strings(names)
        t = dict(names=up(nb), name_off=up(noff), chrs=up(cb), chr_off=up(coff))
        if quals is not None:
            qb, qoff = pack_strings(quals)
            t.update(quals=up(qb), qual_off=up(qoff))
    jobs = np.frombuffer(dev["jobs"][:n * JOB_DTYPE.itemsize].cpu().numpy().tobytes(), JOB_DTYPE) if n else np.zeros(0, JOB_DTYPE)
    lens = jobs["len"].astype(np.int64)
    trimmed = dev.get("full_len") is not None
    if trimmed and n:
        lens = dev["full_len"][:n].cpu().numpy().view(np.uint32).astype(np.int64)
    max_xa = int(dev["sel"][:4 * n].view(-1, 4)[:, 3].max().item()) & 0xFFFFFFFF if n else 0
    max_chr = int(np.diff(coff.astype(np.int64)).max()) if len(chr_names) else 0
    max_line = max(1, line_bound(int(np.diff(noff.astype(np.int64)).max()) if n else 0, int(lens.max()) if n else 0, max_chr,
                                 int(dev["cigar_stride"]), int(dev["md_stride"]), min(max_xa, 1 << 16), trimmed,
                                 int(dev.get("bc_len") or 0)))
    # room: the strings as they are, a typical line's numbers and tags; a batch that needs
    # more says so in counters[0]
    cap = int(len(nb) + (2 if quals is not None else 1) * lens.sum() + n * (160 + max_chr + int(dev.get("bc_len") or 0)) + 64)
    o, ctr = chain.sam_lines64(gi, dev, t, len(chr_names), max_line, cap, flag=flag, max_top2=max_top2, comp_read=comp_read)
    out = o["out"]
    written = int(ctr[1])
    if on_device:
        return out, o["line_off"], o["stat"].cpu().numpy().view(np.uint32)[:n], ctr
    host = torch.empty(max(written, 1), dtype=torch.uint8).pin_memory()
    host[:written].copy_(out[:written])
    torch.cuda.synchronize()
    return (host[:written].numpy().tobytes(), o["line_off"].cpu().numpy().view(np.uint64),
            o["stat"].cpu().numpy().view(np.uint32)[:n], ctr)
