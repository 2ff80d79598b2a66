#!/usr/bin/env python3
"""Fixtures for spliced reads with several splice pairs (XA:Z lists on XT:A:S lines) under
tests/golden/, from the COMPILED REFERENCE (oracle/_ref/HSA, built by `make -C oracle -f
ref.mk`): test infrastructure, CPU only.

The tiny genome repeats nothing, so no spliced read of the other fixtures combines into more
than one pair.  dup.fa (chrA 150 000 bp, chrB 50 003 bp, random filler between the loci) holds, from
a fixed seed:
  * N_LOCI loci of exon (100 bp) - intron (GT...AG, random in between) - exon (100 bp), copied
    2-4 times on chrA with identical exons and one intron length but different intron text;
  * for the loci with i % 4 == 0 one more copy with a longer intron (never in a list), with
    i % 4 == 1 one with a shorter intron (it alone wins: no list), with i % 4 == 2 one more
    equal copy on chrB;
  * three tandem loci of 12, 30 and 60 adjacent copies (the last: 50 rows of each segment,
    X0 = 100).
Reads: 12 per locus, 100 bp, the last 40-60 bases of the first exon and the first bases of the
second, 0-2 substitutions, alternating strands; dup_reads.fq.gz with quality 'I', and
dup_reads_q.fq.gz with the same bases and qualities that decay over a tail of 0-35 bases
(for -q 15).  The reference's SAM for each case of CASES is kept gzipped (mtime 0), and
manifest_dup.json holds the arguments, the line counts and the digests.  The conditions of
check() are asserted: the fixtures are only written when the reference's output shows what
the tests need.

    python tools/make_golden_dup.py
"""
from __future__ import annotations

import gzip
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hsa_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(ROOT, "tests", "golden")
INDEX_EXT = ["bwt", "fmv", "rev.bwt", "rev.fmv", "sa", "pac", "rev.pac", "ann"]
SEED = 20240917
LEN_A, LEN_B = 150000, 50003        # the tiny genome's length (on a text of 200 000 characters the reference's seeds find nothing)
N_LOCI, EXON, READ_LEN, PER_LOCUS = 49, 100, 100, 12
TANDEM = (12, 30, 60)
INTRON = (150, 500)          # the loci's intron lengths
TANDEM_INTRON = 80
MAX_MM = 2
COPIES = (2, 3, 4)
EXTRAS = True

CASES = {
    "default": ("reads", []),
    "n4o1": ("reads", ["-n", "4", "-o", "1"]),
    "q15": ("reads_q", ["-q", "15"]),
}
FILES = {"reads": "dup_reads.fq.gz", "reads_q": "dup_reads_q.fq.gz"}


def intron(rng, n: int) -> np.ndarray:
    x = rng.integers(0, 4, n, dtype=np.uint8)
    x[:2] = (2, 3)                       # GT
    x[-2:] = (0, 2)                      # AG
    return x


def genome(rng):
    """(chrA, chrB, the loci's (exon 1, exon 2))."""
    loci, blocks_a, blocks_b = [], [], []
    for i in range(N_LOCI):
        e1, e2 = rng.integers(0, 4, EXON, dtype=np.uint8), rng.integers(0, 4, EXON, dtype=np.uint8)
        n_int = int(rng.integers(*INTRON))
        copy = lambda n: np.concatenate([e1, intron(rng, n), e2])
        blocks_a += [copy(n_int) for _ in range(COPIES[i % 3])]
        if not EXTRAS:
            pass
        elif i % 4 == 0:
            blocks_a.append(copy(n_int + int(rng.integers(100, 400))))
        elif i % 4 == 1:
            blocks_a.append(copy(n_int - int(rng.integers(40, 90))))
        elif i % 4 == 2:
            blocks_b.append(copy(n_int))
        loci.append((e1, e2))
    for copies in TANDEM:
        e1, e2 = rng.integers(0, 4, EXON, dtype=np.uint8), rng.integers(0, 4, EXON, dtype=np.uint8)
        blocks_a.append(np.concatenate([np.concatenate([e1, intron(rng, TANDEM_INTRON), e2]) for _ in range(copies)]))
        loci.append((e1, e2))

    def lay(blocks, total):
        order = rng.permutation(len(blocks))
        used = sum(len(b) for b in blocks)
        assert used + 50 * (len(blocks) + 1) <= total, (used, total)
        gaps = rng.multinomial(total - used - 50 * (len(blocks) + 1), np.full(len(blocks) + 1, 1.0 / (len(blocks) + 1))) + 50
        parts = []
        for k, b in enumerate(order):
            parts += [rng.integers(0, 4, int(gaps[k]), dtype=np.uint8), blocks[b]]
        parts.append(rng.integers(0, 4, int(gaps[-1]), dtype=np.uint8))
        out = np.concatenate(parts)
        assert len(out) == total
        return out
    return lay(blocks_a, LEN_A), lay(blocks_b, LEN_B), loci


def quality_tail(rng, n: int) -> bytes:
    tail = int(rng.integers(0, 36))
    q = np.concatenate([rng.integers(30, 41, n - tail), np.clip(28 - 2 * np.arange(tail) + rng.integers(-3, 4, tail), 2, 40)])
    return (q + 33).astype(np.uint8).tobytes()


def reads(rng, loci):
    recs, recs_q = [], []
    for i, (e1, e2) in enumerate(loci):
        for r in range(PER_LOCUS):
            cut = int(rng.integers(40, 61))
            s = np.concatenate([e1[EXON - cut:], e2[:READ_LEN - cut]])
            for p in rng.choice(READ_LEN, r % (MAX_MM + 1), replace=False):
                s[p] = (s[p] + 1 + int(rng.integers(0, 3))) % 4
            if r % 2:
                s = synth.revcomp_codes(s)
            seq = bytes(b"ACGT"[c] for c in s)
            name = f"d{i:02d}_{r:02d}".encode()
            recs.append((name, seq, b"I" * READ_LEN))
            recs_q.append((name, seq, quality_tail(rng, READ_LEN)))
    return recs, recs_q


def fastq(recs) -> bytes:
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in recs)


def gz_write(path: str, data: bytes) -> None:
    with gzip.GzipFile(path, "wb", compresslevel=9, mtime=0) as f:
        f.write(data)


def check(name: str, sam: bytes) -> dict:
    lines = sam.decode("latin-1").splitlines()
    s = [ln for ln in lines if "\tXT:A:S" in ln]
    xa = [ln for ln in s if "\tXA:Z:" in ln]
    entries = [len(re.findall(r"chr[AB],[+-]", ln.split("\tXA:Z:")[1])) for ln in xa]
    other = [ln for ln in xa if ("chrB" if ln.split("\t")[2] == "chrA" else "chrA") in ln.split("\tXA:Z:")[1]]
    x0 = [int(re.search(r"\tX0:i:(\d+)", ln).group(1)) for ln in s]
    both = [ln for ln in xa if "\tXC:i:" in ln]
    got = dict(sam_lines=len(lines), spliced=len(s), with_XA=len(xa), xa_entries=sum(entries), longest_list=max(entries, default=0),
               xa_forward=sum(not int(ln.split("\t")[1]) & 16 for ln in xa), xa_reverse=sum(bool(int(ln.split("\t")[1]) & 16) for ln in xa),
               xa_other_chr=len(other), max_X0=max(x0, default=0), with_XC=sam.count(b"\tXC:i:"), with_XC_and_XA=len(both),
               longest_line=max((len(ln) + 1 for ln in lines), default=0))
    assert b"\0" not in sam, name
    if name == "q15":
        assert got["with_XC_and_XA"] >= 5, (name, got)
    else:
        assert got["with_XA"] >= 20 and got["xa_forward"] and got["xa_reverse"] and got["xa_other_chr"] >= 5, (name, got)
        assert got["longest_list"] >= 25 and got["max_X0"] > 60, (name, got)
    return got


def main() -> None:
    rng = np.random.default_rng(SEED)
    chr_a, chr_b, loci = genome(rng)
    recs, recs_q = reads(rng, loci)
    texts = {"reads": fastq(recs), "reads_q": fastq(recs_q)}
    with tempfile.TemporaryDirectory() as work:
        fa = os.path.join(work, "dup.fa")
        synth.write_fasta(fa, np.concatenate([chr_a, chr_b]), [(0, LEN_A), (LEN_A, LEN_B)], names=["chrA", "chrB"])
        subprocess.run([os.path.join(REF, "HSA"), "index", "dup.fa"], check=True, capture_output=True, cwd=work)
        for e in INDEX_EXT:
            assert os.path.getsize(f"{fa}.index.{e}") <= max(os.path.getsize(os.path.join(GOLD, "index", f"tiny.fa.index.{e}")), 64), e
        man = {"index": "dup", "genome": {"chrA": LEN_A, "chrB": LEN_B, "seed": SEED, "loci": N_LOCI, "tandem": list(TANDEM)},
               "files": FILES, "n": {k: t.count(b"\n") // 4 for k, t in texts.items()}, "index_sha256": {}}
        sams = {}
        for k, t in texts.items():
            with open(os.path.join(work, FILES[k][:-3]), "wb") as f:
                f.write(t)
        for name, (key, args) in CASES.items():
            r = subprocess.run([os.path.join(REF, "HSA"), "aln", *args, fa, os.path.join(work, FILES[key][:-3])], check=True,
                               capture_output=True)
            sams[name] = r.stdout
            man[name] = dict(check(name, r.stdout), reads=key, args=args, sam_sha256=hashlib.sha256(r.stdout).hexdigest())
            print(name, man[name])
        # every condition held: write
        for e in INDEX_EXT:
            shutil.copy(f"{fa}.index.{e}", os.path.join(GOLD, "index", f"dup.fa.index.{e}"))
            man["index_sha256"][e] = hashlib.sha256(open(f"{fa}.index.{e}", "rb").read()).hexdigest()
    for k, t in texts.items():
        gz_write(os.path.join(GOLD, FILES[k]), t)
    for name, sam in sams.items():
        gz_write(os.path.join(GOLD, f"dup_ref_{name}.sam.gz"), sam)
    with open(os.path.join(GOLD, "manifest_dup.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
