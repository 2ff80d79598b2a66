"""One row of hsa_refine_rows_device64 (GpuIndex.refine_rows64) as the SAM strings.

The device writes a row's CIGAR as bwa_cigar_t words (bwtaln.h:70-80: op << 28 | length)
and its MD string as bytes; the reference prints them at bwtse.c:713 and :779."""
from __future__ import annotations

import numpy as np

CIGAR_OPS = "MIDNSHP=X"      # bwtse.c:713


def cigar_text(ops, n_cigar=None) -> str:
    """The CIGAR column: the first n_cigar words of `ops` (all of them by default)."""
    ops = np.asarray(ops, np.uint32).reshape(-1)
    if n_cigar is not None:
        if n_cigar > len(ops):
            raise ValueError(f"{n_cigar} ops asked for, {len(ops)} given (HSA_RF_MD: enlarge cigar_stride)")
        ops = ops[:n_cigar]
    out = []
    for w in ops:
        op, ln = int(w) >> 28, int(w) & 0x0FFFFFFF
        if op >= len(CIGAR_OPS):
            raise ValueError(f"no CIGAR letter for op {op}")
        out.append(f"{ln}{CIGAR_OPS[op]}")
    return "".join(out)


def md_text(md, md_len=None) -> str:
    """The MD:Z value: the first md_len bytes of `md` (all of them by default)."""
    md = np.asarray(md, np.uint8).reshape(-1)
    if md_len is not None:
        if md_len > len(md):
            raise ValueError(f"{md_len} bytes asked for, {len(md)} given (HSA_RF_MD: enlarge md_stride)")
        md = md[:md_len]
    return md.tobytes().decode("ascii")


def row_sam(row_words, cigar_row, md_row) -> dict:
    """A row's HSA_RF_ROW_WORDS words, CIGAR words and MD bytes as a dict: status, cigar,
    nm, md (the SAM strings), trim5 / trim3 (reference bases dropped at the ends)."""
    r = np.asarray(row_words, np.uint32).reshape(-1)
    status, n_cigar, nm, md_len, trim5, trim3 = (int(x) for x in r[:6])
    return dict(status=status, cigar=cigar_text(cigar_row, n_cigar), nm=nm, md=md_text(md_row, md_len),
                trim5=trim5, trim3=trim3)
