#!/usr/bin/env python3
"""Fixtures for the reader's options (-q, -B, -Y, -I) under tests/golden/, from the COMPILED
REFERENCE (oracle/_ref/HSA, built by `make -C oracle -f ref.mk`): test infrastructure, CPU only.

The committed drop-in reads carry one quality ('I') and no comment, so none of these options
does anything on them.  Here every 3rd read of dropin_reads.fq.gz (the main set) and every
2nd of dropin_splice_reads.fq.gz (the splice set) get, from a fixed seed:
  * the comment "1:Y:0:ACG" on every 7th read (i % 7 == 3), else "1:N:0:ACG";
  * qualities: 15 % all Q40, 10 % all Q2, the rest a head of Q25-40 and a tail of Q2-30 of
    0-70 bases;
  * a variant with 6 random barcode bases (and such qualities) in front, for -B 6;
  * a variant of the main set with 31 added to every quality byte, for -I.
The reference's SAM for each case of CASES is kept gzipped (mtime 0) next to the reads, and
manifest_opts.json holds the arguments, the line counts and the digests.

    python tools/make_golden_opts.py
"""
from __future__ import annotations

import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hsa_amd import reads  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 20240611
BC_LEN = 6

# case -> (read file key, arguments)
CASES = {
    "q15": ("main", ["-q", "15"]),
    "Y": ("main", ["-Y"]),
    "B6": ("main_bc", ["-B", "6"]),
    "Iq15": ("main_il13", ["-I", "-q", "15"]),
    "B6q15Y": ("main_bc", ["-B", "6", "-q", "15", "-Y"]),
    "splice_q15": ("splice", ["-q", "15"]),
    "splice_q20n4o1": ("splice", ["-q", "20", "-n", "4", "-o", "1"]),
    "splice_B6q15Y": ("splice_bc", ["-B", "6", "-q", "15", "-Y"]),
}
FILES = {"main": "opts_reads.fq.gz", "main_bc": "opts_reads_bc.fq.gz", "main_il13": "opts_reads_il13.fq.gz",
         "splice": "opts_splice_reads.fq.gz", "splice_bc": "opts_splice_reads_bc.fq.gz"}


def qualities(rng, n: int) -> bytes:
    u = rng.random()
    if u < 0.15:
        q = np.full(n, 40)
    elif u < 0.25:
        q = np.full(n, 2)
    else:
        tail = min(int(rng.integers(0, 71)), n)
        q = np.concatenate([rng.integers(25, 41, n - tail), rng.integers(2, 31, tail)])
    return (q + 33).astype(np.uint8).tobytes()


def make_set(src: str, step: int, rng):
    """(plain, barcoded) records of every step-th read of the committed file `src`."""
    with gzip.open(os.path.join(GOLD, src), "rb") as f:
        p = reads.parse_host(f.read())
    plain, coded = [], []
    for i, k in enumerate(range(0, len(p["names"]), step)):
        head = p["names"][k] + (b" 1:Y:0:ACG" if i % 7 == 3 else b" 1:N:0:ACG")
        seq = p["raw"][k]
        q = qualities(rng, len(seq))
        bc = bytes(b"ACGT"[c] for c in rng.integers(0, 4, BC_LEN))
        plain.append((head, seq, q))
        coded.append((head, bc + seq, qualities(rng, BC_LEN + 64)[-BC_LEN:] + q))
    return plain, coded


def fastq(recs, shift=0) -> bytes:
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + bytes(c + shift for c in q) + b"\n" for h, s, q in recs)


def gz_write(path: str, data: bytes) -> None:
    with gzip.GzipFile(path, "wb", compresslevel=9, mtime=0) as f:
        f.write(data)


def main() -> None:
    rng = np.random.default_rng(SEED)
    main_plain, main_bc = make_set("dropin_reads.fq.gz", 3, rng)
    sp_plain, sp_bc = make_set("dropin_splice_reads.fq.gz", 2, rng)
    texts = {"main": fastq(main_plain), "main_bc": fastq(main_bc), "main_il13": fastq(main_plain, 31),
             "splice": fastq(sp_plain), "splice_bc": fastq(sp_bc)}
    man = {"index": "tiny", "bc_len": BC_LEN, "files": FILES, "n": {k: t.count(b"\n") // 4 for k, t in texts.items()}}
    for k, t in texts.items():
        gz_write(os.path.join(GOLD, FILES[k]), t)
    idx = os.path.join(GOLD, "index", "tiny.fa")
    for name, (key, args) in CASES.items():
        r = subprocess.run([os.path.join(REF, "HSA"), "aln", *args, idx, os.path.join(GOLD, FILES[key])], check=True,
                           capture_output=True)
        sam = r.stdout
        gz_write(os.path.join(GOLD, f"opts_ref_{name}.sam.gz"), sam)
        man[name] = {"reads": key, "args": args, "sam_sha256": hashlib.sha256(sam).hexdigest(), "sam_lines": sam.count(b"\n"),
                     "with_XC": sam.count(b"\tXC:i:"), "spliced": sam.count(b"\tXT:A:S"), "with_BC": sam.count(b"\tBC:Z:")}
        print(name, man[name])
    with open(os.path.join(GOLD, "manifest_opts.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
