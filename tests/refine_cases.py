"""Fabricated rows for the refinement (hsa_refine_rows_device64), stated once: a seeded
generator of a small text and of reads cut from it, the case file that oracle/ref_refine.c
reads and the answer file it writes.  tools/make_golden_refine.py runs the generator through
the compiled reference's bwa_refine_gapped into tests/golden/refine_cases.npz;
tests/test_refine_cases_cpu.py guards the file, tests/test_gpu_refine.py compares the device
with it byte for byte.

The text: i.i.d. stretches, a homopolymer run, two dinucleotide and one trinucleotide tandem
repeat, and a final stretch (with a short repeat and a short run) that ends the text.  A read
is a piece of the text from `pos` on with events applied at read offsets: D (text characters
left out), I (bases put in: inside a repeat the next bases of the text, so that the repeat
goes on), X (a substitution), N (code 4).  It is stored as the FASTQ would hold it: reverse
complemented for strand 1.  `made` is the CIGAR of the events where they were made, ends
treated as the reference treats them (a D at an end dropped, an I at an end printed S); the
reference may place an indel elsewhere at an equal score, which is what the fixture pins.

Every case is inside the contract: 1 <= len <= 1023, gap <= 16, pos inside the text, and a
row without a gap lies wholly inside the text."""
import functools
import os
import struct
import subprocess

import numpy as np

SEED = 20241021
MAX_LEN, MAX_GAP = 1023, 16
ODD_LENS = (1, 2, 15, 16, 17, 49, 50, 51, 63, 64, 65, 127, 128, 129, 1023)
CUT_KEEPS = (1, 2, 49, 50, 51, 63, 64, 65, 99, 100, 101)
CHUNK_OFFS = (5, 36, 37, 50, 63, 64, 65, -6)                 # -6: len - 6
CASE_MAGIC, ANSWER_MAGIC = 0x43525348, 0x41525348            # 'HSRC', 'HSRA'
HEAD = ("occ_pos", "ori_pos", "start", "end", "nm", "n_cigar", "md_len")
OPS = "MIDNS"


def revcomp(c):
    c = np.asarray(c, np.uint8)[::-1]
    return np.where(c < 4, 3 - c, c).astype(np.uint8)


def made_cigar(ops):
    """(op, n) runs in text order -> the CIGAR string with the reference's end rules."""
    runs = []
    for op, n in ops:
        if n == 0:
            continue
        if runs and runs[-1][0] == op:
            runs[-1][1] += n
        else:
            runs.append([op, n])
    if runs and runs[0][0] == "D":
        runs.pop(0)
    if runs and runs[-1][0] == "D":
        runs.pop()
    for k in (0, -1):
        if runs and runs[k][0] == "I":
            runs[k][0] = "S"
    return "".join(f"{n}{op}" for op, n in runs)


class Maker:
    def __init__(self, seed, vary):
        self.rng = np.random.default_rng(seed)
        self.vary = vary
        self.rows = []
        self._text()

    # ------------------------------------------------------------ the text
    def _text(self):
        rng, parts, self.reg, at = self.rng, [], {}, 0

        def put(name, codes):
            nonlocal at
            codes = np.asarray(codes, np.uint8)
            self.reg[name] = (at, at + len(codes))
            parts.append(codes)
            at += len(codes)

        def pad(n):
            put(f"_pad{len(parts)}", rng.integers(0, 4, n + (int(rng.integers(0, 16)) if self.vary else 0)))

        units = dict(homo=[3], di=[0, 1], di2=[0, 3], tri=[1, 0, 2])
        if self.vary:                                # other motifs of the same periods
            units = dict(homo=[int(rng.integers(0, 4))], di=[2, 1], di2=[3, 2], tri=[2, 3, 3])
        put("rand", rng.integers(0, 4, 1300))
        for name, reps in (("homo", 70), ("di", 40), ("di2", 60), ("tri", 30)):
            pad(110)
            put(name, np.tile(units[name], reps))
        pad(110)
        put("tail", np.concatenate([rng.integers(0, 4, 260), np.tile([2, 3], 12), rng.integers(0, 4, 30),
                                    np.zeros(9, np.uint8), rng.integers(0, 4, 17)]))
        self.text = np.concatenate(parts)
        self.T = len(self.text)
        self.ext = np.concatenate([self.text, rng.integers(0, 4, MAX_LEN + MAX_GAP).astype(np.uint8)])

    def mid(self, name):
        a, b = self.reg[name]
        return (a + b) // 2 + (int(self.rng.integers(-5, 6)) if self.vary else 0)

    def off(self, o, L):
        """A family's read offset; the random set moves it a little."""
        if o < 0:
            o += L
        if self.vary:
            o += int(self.rng.integers(-3, 4))
        return min(max(o, 0), L)

    # ------------------------------------------------------------ one row
    def add(self, family, start, L, events, strand, gap, cut=False):
        """The read of L bases from text position `start` on with `events` = (read offset,
        kind, n) in offset order; past the text's end (cut rows only) it goes on at random."""
        assert 1 <= L <= MAX_LEN and 0 <= gap <= MAX_GAP and 0 <= start < self.T, (family, start, L, gap)
        out, ops, x, y = [], [], start, 0
        for o, kind, n in events:
            assert y <= o and (kind == "D" or o + n <= L), (family, events)
            out.append(self.ext[x:x + o - y])
            ops.append(("M", o - y))
            x += o - y
            y = o
            if kind == "D":
                x += n
            elif kind == "I":                      # the text's next bases: a repeat goes on
                ins = self.ext[x:x + n].copy()
                if family.endswith("rand"):
                    ins = self.rng.integers(0, 4, n).astype(np.uint8)
                out.append(ins)
                y += n
            else:
                assert n == 1
                out.append(np.array([4 if kind == "N" else (int(self.ext[x]) + 1 + int(self.rng.integers(0, 3))) % 4], np.uint8))
                x += 1
                y += 1
            ops.append((kind if kind in "DI" else "M", n))
        out.append(self.ext[x:x + L - y])
        ops.append(("M", L - y))
        seq = np.concatenate(out).astype(np.uint8)
        assert len(seq) == L, (family, len(seq), L)
        if not cut:
            assert x + L - y <= self.T and start + L + gap <= self.T, (family, start, L, gap)
        ori = start + 1 + (1000 if strand else 0)
        self.rows.append(dict(family=family, len=L, strand=strand, pos=start, ori=ori, gap=gap,
                              codes=revcomp(seq) if strand else seq, made="" if cut else made_cigar(ops)))

    # ------------------------------------------------------------ the families
    def ties(self):
        for name in ("homo", "di", "di2", "tri"):
            for n in range(1, 17):
                for kind in "DI":
                    for sub in (0, 1, 2):          # none, directly before, directly after
                        for strand in (0, 1):
                            if sub and (n + strand + (kind == "I")) % 2 == 0 and not self.vary:
                                continue           # (half of the substitution rows: enough)
                            o = self.off(50, 100 - n)
                            ev = [(o, kind, n)]
                            if sub == 1 and o > 0:
                                ev = [(o - 1, "X", 1)] + ev
                            if sub == 2:
                                ev = ev + [(o + (n if kind == "I" else 0), "X", 1)]
                            self.add("ties_" + name, self.mid(name) - o, 100, ev, strand, n)

    def chunk(self):
        for name in ("di", "homo", "rand"):
            for n in range(12, 17):
                for o in CHUNK_OFFS:
                    for strand in (0, 1):
                        o2 = self.off(o, 100)
                        self.add("chunk_" + name, self.mid(name) - o2, 100, [(o2, "D", n)], strand, n)

    def carried(self):
        """Deletions of 14..16 in a repeat with a substitution directly beside them, at the
        read offsets around 50 where the deletion's run crosses the 64th column of the band:
        there the open-or-extend choice of set_D (the strict `>`) meets an equal pair of
        scores in about every fifth row, in the first cell of the band's second chunk."""
        for name in ("di", "di2", "tri"):
            for n in (14, 15, 16):
                for o in range(47, 60):
                    for sub in (1, 2):
                        o2 = self.off(o, 100)
                        ev = [(o2 - 1, "X", 1), (o2, "D", n)] if sub == 1 else [(o2, "D", n), (o2, "X", 1)]
                        self.add("carried_" + name, self.mid(name) - o2, 100, ev, (o + n + sub) % 2, n)

    def ends(self):
        for name in ("rand", "di2"):
            for d in range(7):
                for side in (5, 3):
                    for kind in "DI":
                        for n in (1, 3, 8):
                            for strand in (0, 1):
                                if kind == "D":
                                    o = d if side == 5 else 100 - d
                                else:
                                    o = d if side == 5 else 100 - d - n
                                self.add(f"ends{side}_" + name, self.mid(name) - o, 100, [(o, kind, n)], strand, n)

    def declared(self):
        for name in ("rand", "tri"):
            for strand in (0, 1):
                for g in range(1, 17):
                    self.add("declared_" + name, self.mid(name) - 50, 100, [], strand, g)
                for n in (1, 2, 3):
                    for g in (n + 1, n + 3, 16):
                        for kind in "DI":
                            o = self.off(40, 100 - n)
                            self.add("declared_" + name, self.mid(name) - o, 100, [(o, kind, n)], strand, g)

    def two(self):
        for name in ("rand", "di"):
            for a, b in ((1, 1), (2, 3), (3, 5), (8, 8), (4, 12)):
                for k1, k2 in ("ID", "DI", "DD"):
                    for strand in (0, 1):
                        o1, o2 = self.off(30, 60), self.off(70, 80)
                        self.add("two_" + name, self.mid(name) - 50, 100, [(o1, k1, a), (o2, k2, b)], strand, a + b)

    def with_n(self):
        for strand in (0, 1):
            for kind in "DI":
                for n in (1, 3, 14):
                    o = self.off(50, 80)
                    after = o + (n if kind == "I" else 0)
                    self.add("n_first_rand", self.mid("rand") - 50, 100, [(0, "N", 1), (o, kind, n)], strand, n)
                    self.add("n_last_rand", self.mid("rand") - 50, 100, [(o, kind, n), (99, "N", 1)], strand, n)
                    self.add("n_beside_rand", self.mid("rand") - 50, 100, [(o - 1, "N", 1), (o, kind, n)], strand, n)
                    self.add("n_beside_rand", self.mid("rand") - 50, 100, [(o, kind, n), (after, "N", 1)], strand, n)
                    self.add("n_repeat_di", self.mid("di") - o, 100, [(o - 7, "N", 1), (o, kind, n)], strand, n)
                    self.add("n_repeat_homo", self.mid("homo") - o, 100, [(o, kind, n), (after + 4, "N", 1)], strand, n)

    def lengths(self):
        lens = ODD_LENS if not self.vary else tuple(int(v) for v in self.rng.integers(1, 200, 14)) + (1023,)
        a = self.reg["rand"][0]
        for L in lens:
            for g in (1, 2, 3):
                for kind in "DI":
                    for strand in (0, 1):
                        ev = [(L // 2, kind, g)] if L >= 15 else []
                        self.add("lengths_rand", a + 3 * g + (L % 7), L, ev, strand, g)
        for kind in "DI":                              # the layout's longest read with its widest gap
            for strand in (0, 1):
                self.add("longest_rand", a + 11 + strand, 1023, [(self.off(400 + 100 * strand, 1000), kind, 16)], strand, 16)

    def cut(self):
        keeps = CUT_KEEPS if not self.vary else tuple(int(v) for v in self.rng.integers(1, 116, 11))
        for keep in keeps:
            for g in (1, 3, 16):
                for strand in (0, 1):
                    start = self.T - keep
                    self.add("cut", start, 100, [], strand, g, cut=True)
                    if keep >= 49:
                        self.add("cut", start, 100, [(self.off(20, 40), "D", 2)], strand, g, cut=True)
                        self.add("cut", start, 100, [(self.off(20, 40), "I", 2)], strand, g, cut=True)

    def addressing(self):
        for p in [0] + list(range(161, 177)):          # pos = 0, then every pos mod 16
            for strand in (0, 1):
                self.add("addressing_rand", p, 100, [(50, "D", 2)], strand, 2)
                self.add("addressing_rand", p, 100, [(31, "X", 1)], strand, 0)

    def ungapped(self):
        a = self.reg["rand"][0] + 200
        for strand in (0, 1):
            for ev in ([(0, "X", 1)], [(99, "X", 1)], [(0, "X", 1), (99, "X", 1)], [(40, "X", 1), (41, "X", 1)],
                       [(40, "X", 1), (41, "X", 1), (42, "X", 1)], [(0, "N", 1)], [(99, "N", 1)], [(57, "N", 1)],
                       [(12, "X", 1), (13, "N", 1)], []):
                self.add("ungapped_rand", a + 5 + strand, 100, ev, strand, 0)
            for r in range(16):                        # both sides of every word boundary of the text
                p = a + 32 + r
                ev = [(z, "X", 1) for z in range(100) if (p + z) % 16 in (15, 0)]
                self.add("ungapped_rand", p, 100, ev, strand, 0)
                L = 17 + r                             # ... and reads that end just before, at and after one
                self.add("ungapped_rand", p, L, [(L - 1, "X", 1)], strand, 0)
            for name in ("homo", "di"):
                self.add("ungapped_" + name, self.mid(name) - 50, 100, [(50, "X", 1)], strand, 0)

    def all(self):
        for f in (self.ties, self.chunk, self.carried, self.ends, self.declared, self.two, self.with_n, self.lengths, self.cut,
                  self.addressing, self.ungapped):
            f()
        return self


def generate(seed=SEED, vary=False):
    """The case set as arrays.  vary: the random set of the GPU's live comparison -- other
    motifs and stretch lengths in the text, offsets moved, other lengths."""
    m = Maker(seed, vary).all()
    r = m.rows
    return dict(text=m.text, lens=np.array([x["len"] for x in r], np.uint32), strand=np.array([x["strand"] for x in r], np.uint8),
                pos=np.array([x["pos"] for x in r], np.uint32), ori=np.array([x["ori"] for x in r], np.uint32),
                gap=np.array([x["gap"] for x in r], np.uint8), codes=np.concatenate([x["codes"] for x in r]).astype(np.uint8),
                family=np.array([x["family"] for x in r]), made=np.array([x["made"] for x in r]))


@functools.lru_cache(maxsize=None)
def cases():
    return generate()


INPUTS = ("text", "lens", "strand", "pos", "ori", "gap", "codes", "family", "made")
ANSWERS = ("head", "cigar", "md")


# ---------------------------------------------------------------- the driver's files
def write_cases(path, c):
    n = len(c["lens"])
    table = np.stack([c["lens"], c["strand"], c["pos"], c["ori"], c["gap"]], axis=1).astype("<u4")
    with open(path, "wb") as f:
        f.write(struct.pack("<III", CASE_MAGIC, len(c["text"]), n))
        f.write(table.tobytes())
        f.write(np.asarray(c["text"], np.uint8).tobytes())
        f.write(np.asarray(c["codes"], np.uint8).tobytes())


def read_answers(path, n):
    """head (n, 7) u32 in the order of HEAD, the CIGAR words and the MD bytes, case after case."""
    raw = open(path, "rb").read()
    magic, got = struct.unpack_from("<II", raw)
    if magic != ANSWER_MAGIC or got != n:
        raise ValueError(f"{path}: not the answers of {n} cases")
    head = np.frombuffer(raw, "<u4", n * len(HEAD), 8).reshape(n, len(HEAD)).copy()
    at = 8 + head.nbytes
    n_words, n_md = int(head[:, 5].sum()), int(head[:, 6].sum())
    if len(raw) != at + 4 * n_words + n_md:
        raise ValueError(f"{path}: {len(raw)} bytes, the rows need {at + 4 * n_words + n_md}")
    return dict(head=head, cigar=np.frombuffer(raw, "<u4", n_words, at).copy(),
                md=np.frombuffer(raw, np.uint8, n_md, at + 4 * n_words).copy())


def run_reference(binary, c, workdir):
    """The reference's answers to every case of `c`; raises when any case is left out."""
    src, dst = os.path.join(workdir, "refine_cases.bin"), os.path.join(workdir, "refine_answers.bin")
    write_cases(src, c)
    r = subprocess.run([binary, src, dst], capture_output=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{binary} ended with {r.returncode}: {r.stderr.decode()[-2000:]}")
    return read_answers(dst, len(c["lens"]))


# ---------------------------------------------------------------- reading a set
def rows_of(c, a):
    """Per row what the device must give: the oriented read, the CIGAR words (a row without a
    gap has the one op `len`M the reference prints for it), MD, NM, the trims, the position."""
    cg_off = np.concatenate([[0], np.cumsum(a["head"][:, 5].astype(np.int64))])
    md_off = np.concatenate([[0], np.cumsum(a["head"][:, 6].astype(np.int64))])
    rd_off = np.concatenate([[0], np.cumsum(c["lens"].astype(np.int64))])
    out = []
    for k in range(len(c["lens"])):
        h, L = a["head"][k], int(c["lens"][k])
        words = a["cigar"][cg_off[k]:cg_off[k + 1]]
        if len(words) == 0:
            words = np.array([L], np.uint32)                     # op M is 0
        seq = c["codes"][rd_off[k]:rd_off[k + 1]]
        out.append(dict(k=k, family=str(c["family"][k]), made=str(c["made"][k]), len=L, gap=int(c["gap"][k]),
                        strand=int(c["strand"][k]), pos=int(c["pos"][k]), ori=int(c["ori"][k]), codes=seq,
                        oriented=revcomp(seq) if c["strand"][k] else seq, words=words.astype(np.uint32),
                        cigar="".join(f"{int(w) & 0x0FFFFFFF}{OPS[int(w) >> 28]}" for w in words),
                        md=a["md"][md_off[k]:md_off[k + 1]].tobytes().decode("ascii"), nm=int(h[4]),
                        trim5=int(np.int32(h[2])), trim3=L - 1 - int(np.int32(h[3])), occ_pos=int(h[0]), ori_pos=int(h[1]),
                        cut=int(c["pos"][k]) + L + int(c["gap"][k]) > len(c["text"])))
    return out


def replay(row, text):
    """A plain replay of one answered row: (read bases the CIGAR spans, NM, MD) as the text
    at the refined position spells them."""
    x, y, nm, md, u, seq = row["occ_pos"], 0, 0, "", 0, row["oriented"]
    for w in row["words"]:
        op, n = OPS[int(w) >> 28], int(w) & 0x0FFFFFFF
        if op == "M":
            for z in range(n):
                if seq[y + z] > 3 or text[x + z] != seq[y + z]:
                    md += f"{u}{'ACGT'[text[x + z]]}"
                    nm += 1
                    u = 0
                else:
                    u += 1
            x += n
            y += n
        elif op in "IS":
            y += n
            nm += n if op == "I" else 0
        else:
            assert op == "D", op
            md += f"{u}^" + "".join("ACGT"[b] for b in text[x:x + n])
            u = 0
            x += n
            nm += n
    return y, nm, md + str(u), x


def census(rows):
    """What a set holds, so that an edit cannot hollow it out."""
    import re
    return dict(
        rows=len(rows), gapped=sum(r["gap"] > 0 for r in rows),
        trim5=sum(r["trim5"] > 0 for r in rows), trim3=sum(r["trim3"] > 0 for r in rows),
        lead_s=sum(re.match(r"\d+S", r["cigar"]) is not None for r in rows), trail_s=sum(r["cigar"].endswith("S") for r in rows),
        moved=sum(bool(r["made"]) and r["cigar"] != r["made"] for r in rows),
        del14=sum(any(int(n) >= 14 for n in re.findall(r"(\d+)D", r["cigar"])) for r in rows),
        cut=sum(r["cut"] for r in rows), forward=sum(r["strand"] == 0 for r in rows), reverse=sum(r["strand"] == 1 for r in rows))


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_cases.npz")


@functools.lru_cache(maxsize=None)
def golden():
    """The committed fixture: (inputs, answers, rows_of them).  Shared, not to be changed."""
    with np.load(GOLDEN) as z:
        c, a = {k: z[k] for k in INPUTS}, {k: z[k] for k in ANSWERS}
    return c, a, rows_of(c, a)
