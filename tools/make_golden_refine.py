#!/usr/bin/env python3
"""tests/golden/refine_cases.npz from the COMPILED REFERENCE: the fabricated rows of
tests/refine_cases.py answered by bwa_refine_gapped through oracle/_ref/ref_refine (built by
`make -C oracle`).  Test infrastructure, CPU only.

The file holds the inputs (text, per case len / strand / pos / ori / gap, the reads' codes,
the family and the CIGAR of the events where they were made) and the reference's answers
(per case occ_pos, ori_pos, start, end, nm, n_cigar, md_len; the CIGAR words; the MD bytes).
The maker fails when the driver does, when a row is missing, or when an answered row does not
replay against the text; nothing is dropped.

    python tools/make_golden_refine.py
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refine_cases as rc  # noqa: E402

DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_refine")
OUT = os.path.join(ROOT, "tests", "golden", "refine_cases.npz")
LARGEST = os.path.join(ROOT, "tests", "golden", "nrun_sa.npz")


def main() -> None:
    c = rc.generate()
    with tempfile.TemporaryDirectory() as tmp:
        a = rc.run_reference(DRIVER, c, tmp)
    n = len(c["lens"])
    if len(a["head"]) != n:
        raise SystemExit(f"{len(a['head'])} answers for {n} cases")
    rows = rc.rows_of(c, a)
    for r in rows:
        span, nm, md, _ = rc.replay(r, c["text"])
        if (span, nm, md) != (r["len"], r["nm"], r["md"]):
            raise SystemExit(f"case {r['k']} ({r['family']}): {r['cigar']} NM {r['nm']} MD {r['md']} does not replay")
    np.savez_compressed(OUT, **{k: c[k] for k in rc.INPUTS}, **{k: a[k] for k in rc.ANSWERS})
    size = os.path.getsize(OUT)
    if size >= os.path.getsize(LARGEST):
        raise SystemExit(f"{OUT}: {size} bytes, not smaller than {os.path.basename(LARGEST)}")
    fam = sorted({r["family"].split("_")[0] for r in rows})
    print(f"{n} cases, {size} bytes; families {fam}")
    print("longest CIGAR", max(len(r["words"]) for r in rows), "ops, longest MD", max(len(r["md"]) for r in rows), "bytes")
    for name, v in rc.census(rows).items():
        print(f"  {name}: {v}")


if __name__ == "__main__":
    main()
