"""hsa_amd.junctions.from_sam, the host statement of the splice junction table: a hand-written
SAM text over a hand-written two-chromosome index with the expected table written out, and the
committed reference SAM files' tables by their counts."""
import gzip
import io
import os

import numpy as np
import pytest

from golden_io import GOLD

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def prefix_of(index):
    return os.path.join(GOLD, "index", index + ".fa")


def small_index(tmp_path):
    """c1: 400 bases with an N run at 201..230 (two blocks); c2: 700 bases (one block).  All A
    but for the planted intron ends."""
    from hsa_amd import index_build
    c1, c2 = ["A"] * 400, ["A"] * 700

    def plant(c, at, two):
        c[at - 1], c[at] = two[0], two[1]
    for at, two in ((31, "GT"), (59, "AG"), (71, "CT"), (99, "AC"), (111, "GC"), (139, "AG"), (149, "AG"), (161, "GT"), (181, "GT"),
                    (259, "AT")):
        plant(c1, at, two)
    for at, two in ((82, "CT"), (466, "GC"), (500, "AT"), (559, "AC")):
        plant(c2, at, two)
    text = c1[:200] + c1[230:] + c2                         # the N run is not in the text
    codes = np.array([CODE[ch] for ch in text], np.uint8)
    ann = [("c1", [(0, 199, 0), (200, 369, 230)]), ("c2", [(370, 1069, 0)])]
    prefix = str(tmp_path / "two.fa")
    with open(prefix + ".index.pac", "wb") as f:
        f.write(index_build.pac_bytes(codes, 1100))
    with open(prefix + ".index.ann", "w") as f:
        f.write(index_build.ann_text(ann, 1100))
    return prefix


def sam_line(name, chrom, pos, cigar, xt="S", xa=None):
    tags = [f"XT:A:{xt}", "NM:i:0", "X0:i:1", "X1:i:1", "XM:i:0", "XO:i:0", "XG:i:0"] + ([f"XA:Z:{xa}"] if xa else [])
    return "\t".join([name, "0", chrom, str(pos), "0", cigar, "*", "0", "0", "ACGT", "IIII"] + tags)


SAM = "\n".join([
    "@SQ\tSN:c1\tLN:400",
    sam_line("r01", "c1", 11, "20M30N20M", xa="c2,+10020M61N30M"),      # GT/AG, a line with a list only
    sam_line("r02", "c1", 41, "10M2D18M30N20M"),                        # CT/AC, a D before the N
    sam_line("r03", "c1", 86, "25M30N10M"),                             # GC/AG, shared ...
    sam_line("r04", "c1", 99, "12M30N30M", xa="c1,+4110M2D18M30N20M"),  # ... with a line that has a list
    sam_line("r05", "c1", 101, "10M40N22M"),                            # the same start, another end
    sam_line("r06", "c1", 141, "20M55N20M"),                            # the end inside the N run
    sam_line("r07", "c1", 171, "10M80N15M"),                            # GT/AT, the ends in two blocks
    sam_line("r08", "c2", 5, "65M2D10M2S386N73M"),                      # CT/GC, an S inside the merged CIGAR
    sam_line("r09", "c2", 480, "20M61N30M5S"),                          # AT/AC, the S of trimming
    sam_line("r10", "c2", 590, "10M51N10M"),                            # AA/AA
    sam_line("r11", "c2", 100, "50M", xt="U"),                          # not a spliced line
]) + "\n"

TABLE = (b"c1\t31\t60\t1\t1\t0\t0\t1\t20\n"
         b"c1\t71\t100\t2\t2\t0\t1\t0\t20\n"
         b"c1\t111\t140\t1\t3\t0\t1\t1\t12\n"
         b"c1\t111\t150\t1\t3\t0\t1\t0\t10\n"
         b"c1\t161\t215\t0\t0\t0\t1\t0\t20\n"
         b"c1\t181\t260\t2\t6\t0\t1\t0\t10\n"
         b"c2\t82\t467\t2\t4\t0\t1\t0\t73\n"
         b"c2\t500\t560\t1\t5\t0\t1\t0\t20\n"
         b"c2\t600\t650\t0\t0\t0\t1\t0\t10\n")


def test_hand_written_sam_gives_the_written_table(tmp_path):
    from hsa_amd import junctions
    prefix = small_index(tmp_path)
    rows, table = junctions.from_sam(SAM, prefix)
    assert table == TABLE
    assert junctions.from_sam(SAM.encode(), prefix)[1] == TABLE
    assert sorted(set(rows[:, 6].tolist())) == [0, 1, 2, 3, 4, 5, 6]            # each of the seven motif codes
    assert rows.dtype == np.uint32 and rows.shape == (9, 8) and (rows[:, 7] == 0).all()
    assert int(rows[:, 3].sum() + rows[:, 4].sum()) == SAM.count("XT:A:S")
    # the order of the lines does not matter, and no line gives no row
    lines = SAM.split("\n")[:-1]
    assert junctions.from_sam("\n".join(lines[::-1]) + "\n", prefix)[1] == TABLE
    assert junctions.from_sam("", prefix)[1] == b"" and junctions.from_sam(lines[-1] + "\n", prefix)[0].shape == (0, 8)


def test_each_end_maps_through_the_block_table(tmp_path):
    """r07's intron starts in c1's first block and ends in its second: 79 bases apart on the
    chromosome, 49 in the text.  r06's last base lies in the N run: no block, motif 0 whatever
    its first two bases are."""
    from hsa_amd import index_io, junctions
    prefix = small_index(tmp_path)
    blocks, pac = index_io.read_blocks(prefix), index_io.read_pac(prefix)
    assert junctions.text_pos(blocks, 0, 181) == 180 and junctions.text_pos(blocks, 0, 260) == 229
    assert junctions.text_pos(blocks, 0, 200) == 199 and junctions.text_pos(blocks, 0, 231) == 200
    assert all(junctions.text_pos(blocks, 0, p) is None for p in (0, 201, 215, 230, 401))
    assert junctions.text_pos(blocks, 1, 1) == 370 and junctions.text_pos(blocks, 1, 700) == 1069 and junctions.text_pos(blocks, 1, 701) is None
    assert junctions.text_pos(blocks, 2, 1) is None
    assert junctions.motif_of(pac, blocks, 0, 181, 260) == 6
    assert [int(pac[180]), int(pac[181])] == [2, 3] and junctions.motif_of(pac, blocks, 0, 161, 215) == 0
    assert junctions.motif_of(pac, blocks, 0, 161, 200) == 0 and junctions.motif_of(pac, blocks, 0, 31, 31) == 0
    assert [junctions.strand_of(m) for m in range(7)] == [0, 1, 2, 1, 2, 1, 2]


# file, index, rows, lines without a list, lines with one
FILES = [("dup_ref_default", "dup", 80, 149, 224), ("dup_ref_n4o1", "dup", 81, 137, 228), ("dup_ref_q15", "dup", 132, 163, 214),
         ("dropin_ref_splice_default", "tiny", 225, 225, 0), ("dropin_ref_splice_n4o1", "tiny", 304, 304, 0),
         ("dropin_ref_default", "tiny", 57, 57, 0), ("opts_ref_splice_q15", "tiny", 115, 115, 0),
         ("opts_ref_splice_B6q15Y", "tiny", 99, 99, 0), ("opts_ref_splice_q20n4o1", "tiny", 124, 124, 0)]
_TABLES = {}


def reference_table(name, index):
    if name not in _TABLES:
        from hsa_amd import junctions
        text = gzip.open(os.path.join(GOLD, name + ".sam.gz")).read()
        _TABLES[name] = (text,) + junctions.from_sam(text, prefix_of(index))
    return _TABLES[name]


@pytest.mark.parametrize("name,index,n_rows,unique,multi", FILES)
def test_reference_files(name, index, n_rows, unique, multi):
    text, rows, table = reference_table(name, index)
    assert (len(rows), int(rows[:, 3].sum()), int(rows[:, 4].sum())) == (n_rows, unique, multi)
    assert unique + multi == sum("\tXT:A:S" in ln for ln in text.decode().split("\n"))
    keys = [tuple(r[:3]) for r in rows.tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    lines = table.split(b"\n")
    assert lines[-1] == b"" and len(lines) == n_rows + 1 and all(ln.count(b"\t") == 8 for ln in lines[:-1])


def test_reference_files_details():
    from hsa_amd import junctions
    _, rows, table = reference_table("dup_ref_default", "dup")
    assert int((rows[:, 3] + rows[:, 4]).max()) == 6
    _, rows, _ = reference_table("dup_ref_n4o1", "dup")
    names = junctions.read_names(prefix_of("dup"))
    assert [names[c] for c in rows[:, 0]].count("chrA") == 80 and [names[c] for c in rows[:, 0]].count("chrB") == 1
    starts = [tuple(r[:2]) for r in rows.tolist()]
    assert len(starts) - len(set(starts)) == 1                                  # one pair of rows shares a start
    assert {1, 2} <= set(rows[:, 6].tolist())
    _, rows, _ = reference_table("dropin_ref_splice_default", "tiny")
    assert int((rows[:, 3] + rows[:, 4]).max()) == 1 and len(set(rows[:, 0].tolist())) == 3
    assert {0, 2, 3, 4, 5, 6} <= set(rows[:, 6].tolist())


def test_reduce_rows_merges_counts():
    """Rows that arrive already reduced: counts add, the overhang is the maximum."""
    from hsa_amd import index_io, junctions
    blocks, pac = index_io.read_blocks(prefix_of("tiny")), index_io.read_pac(prefix_of("tiny"))
    rows = np.array([[1, 500, 900, 3, 0, 20, 0, 0], [0, 700, 800, 1, 0, 9, 0, 0], [1, 500, 900, 0, 4, 31, 0, 0],
                     [1, 500, 899, 1, 0, 7, 0, 0], [1, 500, 900, 1, 1, 25, 0, 0]], np.uint32)
    out = junctions.reduce_rows(rows, pac, blocks)
    assert out[:, :6].tolist() == [[0, 700, 800, 1, 0, 9], [1, 500, 899, 1, 0, 7], [1, 500, 900, 4, 5, 31]]
    assert np.array_equal(junctions.reduce_rows(out, pac, blocks), out)


def test_option_and_its_absence():
    from hsa_amd import align
    _, rest, extra = align.parse_options(["--splice", "--junctions", "sj.tab", "p", "r.fq"], reader_options=True)
    assert extra["junctions"] == "sj.tab" and extra["splice"] is True and rest == ["p", "r.fq"]
    assert "junctions" not in align.parse_options(["--splice", "p", "r.fq"], reader_options=True)[2]
    assert "junctions" not in align.parse_options(["p", "r.fq"])[2]
    with pytest.raises(ValueError, match="--splice"):       # before any device work: no index is needed to get here
        align.align_fastq(None, [], b"", align.default_opts(), io.BytesIO(), junctions=io.BytesIO())
