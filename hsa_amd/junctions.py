"""The splice junction table of a run of `python -m hsa_amd.align --splice --junctions FILE`.

One row per distinct intron of the printed XT:A:S lines, tab-separated, '\\n' line ends, no
header, the nine columns of STAR's SJ.out.tab:

  1. chromosome name, as in the .ann file;
  2. first base of the intron, 1-based: POS plus the lengths of the M and D ops before the N;
  3. last base: column 2 plus the N length minus 1;
  4. strand from the motif: 1 for motifs 1, 3, 5; 2 for 2, 4, 6; 0 for 0;
  5. motif, from the forward text's two first and two last intron bases: 1 GT/AG, 2 CT/AC,
     3 GC/AG, 4 CT/GC, 5 AT/AC, 6 GT/AT, 0 anything else;
  6. 0 (there is no annotation);
  7. printed XT:A:S lines with this intron and no XA:Z list;
  8. printed XT:A:S lines with this intron and an XA:Z list;
  9. the maximum over those lines of min(sum of the M lengths before the N, sum of the M
     lengths behind it); S, I and D ops are not counted.

Rows are sorted by (chromosome index in the .ann file, column 2, column 3).

The reference prints no such table.  It is defined as a pure function of the SAM text the
command prints and the index's .pac and .ann files, and from_sam is that function on the
host; the device stages (hsa_junctions.hip, driven by Accumulator) are held to it.  Only the
primary alignment of a printed line counts: the reference prints an XA:Z entry's position and
first op length with nothing between them ("chrA,+13386752M221N48M" is position 133867 and
52M), so the text does not determine the introns of the entries.  A read the command refuses
has no line and contributes nothing.

The motif's four bases are read from the packed text.  Each base's chromosome coordinate maps
to a text position through the block table on its own: text distance is not chromosome
distance across an N run.  A base that lies in no block (inside an N run, or past the
chromosome) makes the motif 0, and so does an intron of fewer than two bases."""
from __future__ import annotations

import re

import numpy as np

from . import index_io
from ._lib import JN_ROW_WORDS

# motif code by the four bases' codes (A C G T = 0 1 2 3): GT/AG, CT/AC, GC/AG, CT/GC, AT/AC, GT/AT
MOTIFS = {(2, 3, 0, 2): 1, (1, 3, 0, 1): 2, (2, 1, 0, 2): 3, (1, 3, 2, 1): 4, (0, 3, 0, 1): 5, (2, 3, 0, 3): 6}
_OP = re.compile(r"(\d+)([MIDNSHP=X])")


def strand_of(motif: int) -> int:
    return 0 if motif == 0 else 1 if motif & 1 else 2


def read_names(prefix: str):
    """The chromosome names of prefix.index.ann, by chrID."""
    with open(prefix + ".index.ann") as f:
        ls = f.read().split("\n")
    return [ls[1 + k].split()[1] for k in range(int(ls[0].split()[1]))]


def text_pos(blocks, c: int, p: int):
    """The text position of base p (1-based) of chromosome c through the block table (rows
    chrID, blockStart, blockEnd, ori), or None when no block holds it."""
    for cid, start, end, ori in blocks:
        if int(cid) == c and int(ori) + 1 <= p <= int(ori) + 1 + int(end) - int(start):
            return int(start) + p - 1 - int(ori)
    return None


def motif_of(pac, blocks, c: int, start: int, end: int) -> int:
    if end <= start:
        return 0
    t = [text_pos(blocks, c, p) for p in (start, start + 1, end - 1, end)]
    if any(x is None or x >= len(pac) for x in t):
        return 0
    return MOTIFS.get(tuple(int(pac[x]) for x in t), 0)


def line_intron(line: str):
    """(chromosome name, first base, last base, has an XA:Z list, overhang) of a printed
    XT:A:S line, or None for any other line."""
    f = line.split("\t")
    if line.startswith("@") or len(f) < 12 or "XT:A:S" not in f[11:]:
        return None
    ops = [(int(n), op) for n, op in _OP.findall(f[5])]
    at = [k for k, (_, op) in enumerate(ops) if op == "N"]
    if len(at) != 1:
        return None
    at = at[0]
    start = int(f[3]) + sum(n for n, op in ops[:at] if op in "MD")
    over = min(sum(n for n, op in ops[:at] if op == "M"), sum(n for n, op in ops[at + 1:] if op == "M"))
    return f[2], start, start + ops[at][0] - 1, any(t.startswith("XA:Z:") for t in f[11:]), over


def table_bytes(rows, names) -> bytes:
    """The text of a reduced table: rows of JN_ROW_WORDS words (chrID, first base, last base,
    lines without a list, lines with one, overhang, motif, 0)."""
    return "".join(f"{names[int(r[0])]}\t{int(r[1])}\t{int(r[2])}\t{strand_of(int(r[6]))}\t{int(r[6])}\t0\t{int(r[3])}\t{int(r[4])}\t{int(r[5])}\n"
                   for r in rows).encode()


def reduce_rows(rows, pac, blocks):
    """The host restatement of the reduction: rows of JN_ROW_WORDS words sorted by (chrID,
    first base, last base), equal introns merged (sums of the two counts, max of the overhang),
    the motif read from the text."""
    acc = {}
    for r in np.asarray(rows, np.int64).reshape(-1, JN_ROW_WORDS):
        k = (int(r[0]), int(r[1]), int(r[2]))
        a = acc.setdefault(k, [0, 0, 0])
        a[0] += int(r[3])
        a[1] += int(r[4])
        a[2] = max(a[2], int(r[5]))
    out = np.zeros((len(acc), JN_ROW_WORDS), np.uint32)
    for i, k in enumerate(sorted(acc)):
        out[i] = (*k, *acc[k], motif_of(pac, blocks, *k), 0)
    return out


def from_sam(text, prefix: str):
    """The junction table of SAM text (bytes or str) over the index files of `prefix`
    (prefix.index.pac, .ann): (the reduced rows, JN_ROW_WORDS u32 each, the table's bytes)."""
    return table_of(text, read_names(prefix), index_io.read_pac(prefix), index_io.read_blocks(prefix))


def table_of(text, names, pac, blocks):
    """from_sam over an index in memory: the chromosome names by chrID, the forward text's
    codes, the block table."""
    if isinstance(text, (bytes, bytearray, memoryview)):
        text = bytes(text).decode()
    chr_id = {n: k for k, n in enumerate(names)}
    rows = []
    for line in text.split("\n"):
        j = line_intron(line)
        if j is not None:
            rows.append((chr_id[j[0]], j[1], j[2], 0 if j[3] else 1, 1 if j[3] else 0, j[4], 0, 0))
    rows = reduce_rows(np.array(rows, np.int64).reshape(-1, JN_ROW_WORDS), pac, blocks)
    return rows, table_bytes(rows, names)


class Accumulator:
    """The device row buffer of a run's junction table.  add() appends the rows of one
    splice-lines call (hsa_junction_rows_device), growing the buffer when the call reports
    wanted > room and running it again; the buffer is compacted by the reduction
    (hsa_junction_reduce_device) whenever it holds more than `threshold` rows (after a
    compaction that leaves more than half of that, twice what it left); finish() reduces once
    more and returns the table's bytes (hsa_junction_text_device).  fed: rows appended over the
    run; distinct: rows of the final table."""

    def __init__(self, gi, chr_names, threshold: int = 1 << 22, room: int = 1 << 16):
        self.gi, self.names = gi, list(chr_names)
        self.threshold = self.limit = max(1, int(threshold))
        self.cap, self.n, self.fed, self.distinct, self.compactions = max(1, int(room)), 0, 0, 0, 0
        self.rows = self._alloc(self.cap)

    @staticmethod
    def _alloc(cap):
        import torch
        return torch.zeros(cap * JN_ROW_WORDS, dtype=torch.int32, device="cuda")

    def _grow(self, need):
        cap = max(2 * self.cap, need)
        rows = self._alloc(cap)
        rows[:self.n * JN_ROW_WORDS] = self.rows[:self.n * JN_ROW_WORDS]
        self.rows, self.cap = rows, cap

    def add(self, o, n):
        """The n jobs of splice_lines' output tensors o."""
        from . import chain
        ctr = chain.junction_rows(self.gi, o, n, self.rows, self.n, self.cap)
        if int(ctr[0]) > int(ctr[1]):
            self._grow(self.n + int(ctr[0]))
            ctr = chain.junction_rows(self.gi, o, n, self.rows, self.n, self.cap)
            assert int(ctr[0]) == int(ctr[1])
        self.n += int(ctr[1])
        self.fed += int(ctr[1])
        if self.n > self.limit:
            self.compact()
            self.limit = max(self.threshold, 2 * self.n)

    def compact(self):
        from . import chain
        ctr = chain.junction_reduce(self.gi, self.rows, self.n)
        assert int(ctr[0]) == self.n and int(ctr[1]) <= self.n
        self.n = int(ctr[1])
        self.compactions += 1

    def finish(self) -> bytes:
        from . import chain, sam
        self.compact()
        self.distinct = self.n
        cb, coff = sam.pack_strings(self.names)
        up = lambda a: chain.to_device(a if len(a) else np.zeros(1, a.dtype))
        max_chr = int(np.diff(coff.astype(np.int64)).max()) if self.names else 0
        o, ctr = chain.junction_text(self.gi, self.rows, self.n, up(cb), up(coff), len(self.names), self.n * (max_chr + 48))
        assert int(ctr[0]) == int(ctr[1]) and int(ctr[2]) == self.n, "a junction row without a line"
        return o["out"][:int(ctr[1])].cpu().numpy().tobytes()
