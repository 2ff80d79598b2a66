"""The SAM line of an unspliced single-end read with a hit, as bwa_print_sam1 prints it
with mate == NULL (bwtse.c:698-799), from the device's outputs: the choice
(GpuIndex.choose_hits64: the read's d_sel and d_sel64 words), its rows (row 0 the chosen
one, rows 1.. the XA list) and their refinement (GpuIndex.refine_rows64).

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
