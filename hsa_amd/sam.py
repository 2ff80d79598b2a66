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

Not printed: RG / BC / XC tags (no read group, barcode or trimmed read reaches the 64-bit
path) and spliced reads."""
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


def sam_line(name, seq_codes, qual, chr_names, sel, sel64, rows, rpos, cigar, md, pos, hits, max_top2=30,
             flag=0, comp_read=True) -> str:
    """One line, without the newline.

    seq_codes: the read as it was given (codes 0-4); qual: its quality string or None;
    chr_names: chromosome names by the position rows' chrID (HSP chrName by seq_id); sel, sel64: the read's 4 + 4 words of the choice; rows, rpos, cigar,
    md, pos: the read's rows of the refinement and of the position arrays, chosen row
    first; hits: the hit record of each of those rows (d_hits[d_hit_off[j] + d_pos_hit[t]]);
    max_top2: gap_opt_t.max_top2 (X1 is printed when X0 <= max_top2); comp_read:
    BWA_MODE_COMPREAD (NM, else CM)."""
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
    out = [name, str(flag), chr_names[int(pos[0][1])], str(int(rpos[0][1])), str(mapq), main["cigar"], "*", "0", "0"]
    if strand == 0:
        out.append("".join(SEQ_FWD[c] for c in seq_codes))
    else:
        out.append("".join(SEQ_REV[c] for c in seq_codes[::-1]))
    out.append("*" if qual is None else (qual[::-1] if strand else qual))
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


# ---------------------------------------------------------------- the batch path
def pack_strings(items):
    """Strings (str or bytes) laid out for the device: (their bytes end to end as a uint8
    array, len(items) + 1 u64 offsets).  Pure NumPy; item k is bytes[off[k]:off[k + 1]]."""
    raw = [x.encode("ascii") if isinstance(x, str) else bytes(x) for x in items]
    off = np.zeros(len(raw) + 1, np.uint64)
    if raw:
        off[1:] = np.cumsum([len(x) for x in raw], dtype=np.uint64)
    return np.frombuffer(b"".join(raw), np.uint8).copy(), off


def line_bound(max_name, max_len, max_chr, cigar_stride, md_stride, max_xa) -> int:
    """An upper bound of a line's length with its newline (hsa_sam_batch64_t.max_line): every
    number at the most digits its type has (u32: 10, u64: 20, a CIGAR length 9, n_mm 5, a
    gap count 3), cut to the most the call takes."""
    from ._lib import HSA_SAM_MAX_LINE
    cigar = 10 * cigar_stride
    n = (max_name + 1 + 10 + 1 + max_chr + 1 + 20 + 1 + 10 + 1 + cigar + 7 + max_len + 1 + max(max_len, 1)
         + 7 + 6 + 10 + 6 + 20 + 6 + 20 + 6 + 5 + 6 + 3 + 6 + 3 + 6 + md_stride + 1)
    if max_xa:
        n += 6 + max_xa * (max_chr + 2 + 20 + max(cigar, 7))
    return min(n, HSA_SAM_MAX_LINE)


def device_sam(gi, dev, names, quals, chr_names, max_top2=30, flag=0, comp_read=True):
    """The SAM text of a batch: (text as bytes, line_off (n + 1 u64), line_stat (n u32),
    counters (8 u64)) of one hsa_sam_lines_device64 call, run a second time with
    counters[0] bytes of room when the first reports wanted > written.

    dev: the device tensors of search, choose and refine (anything with data_ptr()) by the
    keys jobs, codes, n_aln, hit_off, hits, n_jobs (the search batch, or a sub-range's offset
    views), sel, sel64, pos_off, pos, pos_hit, pos_cap, pos_ctr (optional: the choice's
    counters), rows, rpos, cigar, md, cigar_stride, md_stride.  names: the reads' names
    (FASTQ comment cut); quals: their quality strings, or None ("*"); chr_names: by chrID.
    Names and qualities that are on the device already (hsa_amd.reads.load_device) are given
    as a pair of tensors instead of a list: (the bytes, the n + 1 u64 offsets of these reads; a
    sub-range's offsets are a view from its first read on)."""
    import torch
    from ._lib import JOB_DTYPE, SamBatch64
    n = int(dev["n_jobs"])
    on_dev = isinstance(names, tuple)
    if quals is not None and on_dev != isinstance(quals, tuple):
        raise ValueError("names and qualities come both as lists or both as device tensors")
    if not on_dev and (len(names) != n or (quals is not None and len(quals) != n)):
        raise ValueError(f"{n} reads, {len(names)} names" + ("" if quals is None else f", {len(quals)} qualities"))

    def up(a):
        a = np.ascontiguousarray(a)
        a = a.view(f"i{a.dtype.itemsize}") if a.dtype.kind == "u" and a.dtype.itemsize > 1 else a
        return torch.from_numpy(a if len(a) else np.zeros(1, a.dtype)).cuda()

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
    max_xa = int(dev["sel"][:4 * n].view(-1, 4)[:, 3].max().item()) & 0xFFFFFFFF if n else 0
    max_chr = int(np.diff(coff.astype(np.int64)).max()) if len(chr_names) else 0
    max_line = max(1, line_bound(int(np.diff(noff.astype(np.int64)).max()) if n else 0, int(lens.max()) if n else 0, max_chr,
                                 int(dev["cigar_stride"]), int(dev["md_stride"]), min(max_xa, 1 << 16)))
    # room: the strings as they are, a typical line's numbers and tags; a batch that needs
    # more says so in counters[0]
    cap = int(len(nb) + (2 if quals is not None else 1) * lens.sum() + n * (160 + max_chr) + 64)
    o = dict(line_off=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
             stat=torch.zeros(max(n, 1), dtype=torch.int32, device="cuda"),
             ctr=torch.zeros(8, dtype=torch.int64, device="cuda"))
    ptr = lambda k: dev[k].data_ptr() if dev.get(k) is not None else None
    for _ in range(2):
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda")
        b = SamBatch64(d_jobs=ptr("jobs"), n_jobs=n, d_codes=ptr("codes"), d_n_aln=ptr("n_aln"), d_hit_off=ptr("hit_off"),
                       d_hits=ptr("hits"), d_sel=ptr("sel"), d_sel64=ptr("sel64"), d_pos_off=ptr("pos_off"),
                       d_pos=ptr("pos"), d_pos_hit=ptr("pos_hit"), pos_cap=int(dev["pos_cap"]), d_pos_counters=ptr("pos_ctr"),
                       d_rows=ptr("rows"), d_rpos=ptr("rpos"), d_cigar=ptr("cigar"), d_md=ptr("md"),
                       cigar_stride=int(dev["cigar_stride"]), md_stride=int(dev["md_stride"]),
                       d_names=t["names"].data_ptr(), d_name_off=t["name_off"].data_ptr(),
                       d_quals=t["quals"].data_ptr() if quals is not None else None,
                       d_qual_off=t["qual_off"].data_ptr() if quals is not None else None,
                       d_chr_names=t["chrs"].data_ptr(), d_chr_off=t["chr_off"].data_ptr(), n_chr=len(chr_names),
                       flag=int(flag), max_top2=int(max_top2), comp_read=int(bool(comp_read)), max_line=max_line,
                       d_line_off=o["line_off"].data_ptr(), d_out=out.data_ptr(), out_cap=cap,
                       d_line_stat=o["stat"].data_ptr(), d_counters=o["ctr"].data_ptr())
        torch.cuda.synchronize()
        gi.sam_lines64(b)
        torch.cuda.synchronize()
        ctr = o["ctr"].cpu().numpy().view(np.uint64)
        if int(ctr[0]) <= int(ctr[1]):
            break
        cap = int(ctr[0])
    written = int(ctr[1])
    host = torch.empty(max(written, 1), dtype=torch.uint8).pin_memory()
    host[:written].copy_(out[:written])
    torch.cuda.synchronize()
    return (host[:written].numpy().tobytes(), o["line_off"].cpu().numpy().view(np.uint64),
            o["stat"].cpu().numpy().view(np.uint32)[:n], ctr)
