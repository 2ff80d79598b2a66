"""Trimmed reads and barcodes in the SAM restatements (no GPU): hsa_amd.sam.sam_line and
spliced_line with clip_len / bc reprint every line of the reference's SAM for the fixtures of
tools/make_golden_opts.py byte for byte, from what the line itself says (CIGAR with
bwa_correct_trimmed undone, strand, positions, tags) and the read as hsa_amd.reads.parse_host
gives it; hsa_amd.align.parse_options with the reader's options."""
import re

import numpy as np
import pytest

from reads_opts_cases import CASES, MANIFEST, MODE_CFY, MODE_IL13, case_options, case_reads, case_sam

OPS = "MIDNSHP=X"
XA = re.compile(r"([^,;]+),([+-])(\d+)((?:\d+[MIDNS])+|,\d+;)")


def cigar_ops(text):
    ops = [(OPS.index(o), int(l)) for l, o in re.findall(r"(\d+)([MIDNSHP=X])", text)]
    assert "".join(f"{l}{OPS[o]}" for o, l in ops) == text
    return ops


def uncorrect(ops, strand, clip):
    """The CIGAR before bwa_correct_trimmed: the clip comes off the edge S op, which goes when
    nothing is left of it."""
    if not clip:
        return ops
    at = 0 if strand else len(ops) - 1
    assert ops[at][0] == 4 and ops[at][1] >= clip
    rest = ops[at][1] - clip
    return ops[:at] + ([(4, rest)] if rest else []) + ops[at + 1:]


def words(ops):
    return np.array([(o << 28) | l for o, l in ops], np.uint32)


def reprint(ln, read, opts):
    """The line again, through sam_line or spliced_line."""
    from hsa_amd import sam, splice
    f = ln.split("\t")
    tags = {t[:2]: t[5:] for t in f[11:]}
    flag = int(f[1])
    strand = 1 if flag & 16 else 0
    seq, qual, clip_len, bc = read
    full = len(seq)
    assert len(f[9]) == full
    ops = uncorrect(cigar_ops(f[5]), strand, full - clip_len)
    assert sum(l for o, l in ops if o in (0, 1, 4)) == clip_len          # the alignment is of the trimmed read
    kw = dict(max_top2=opts["max_top2"], flag=flag & ~16, comp_read=bool(opts["mode"] & 2), clip_len=clip_len, bc=bc)
    if tags["XT"] == "S":
        at = [k for k, (o, _) in enumerate(ops) if o == 3]
        assert len(at) == 1
        c0, c1, n_len = ops[:at[0]], ops[at[0] + 1:], ops[at[0]][1]
        end0 = sum(l for o, l in c0 if o in (0, 1, 4)) - 1
        cigar = splice.merge_cigar(c0, int(f[3]), end0, c1, int(f[3]) + end0 + n_len)
        return sam.spliced_line(f[0], seq, qual, f[2], int(f[3]), cigar, strand, int(tags["X0"]), int(tags.get("X1", 0)),
                                int(tags["XM"]), **kw)
    chrs = [f[2]]
    xa = XA.findall(tags["XA"]) if "XA" in tags else []
    assert "".join(a + "," + b + c + d for a, b, c, d in xa) == tags.get("XA", "")
    n = 1 + len(xa)
    rows, rpos, pos, hits = np.zeros((n, 8), np.uint32), np.zeros((n, 2), np.uint64), np.zeros((n, 4), np.uint64), np.zeros((n, 14), np.uint32)
    mdb = tags["MD"].encode()
    cig, md = np.zeros((n, 64), np.uint32), np.zeros((n, max(256, len(mdb))), np.uint8)
    rows[0, :4] = (0, len(ops), int(tags["NM" if opts["mode"] & 2 else "CM"]), len(mdb))
    cig[0, :len(ops)] = words(ops)
    md[0, :len(mdb)] = np.frombuffer(mdb, np.uint8)
    rpos[0, 1] = int(f[3])
    xo, xg = int(tags["XO"]), int(tags["XG"])
    hits[0, 0], hits[0, 1] = int(tags["XM"]) | (xo << 16) | ((xg - xo) << 24), strand << 30
    for t, (c, sg, p, tail) in enumerate(xa, 1):
        if c not in chrs:
            chrs.append(c)
        pos[t, 1], rpos[t, 1], hits[t, 1] = chrs.index(c), int(p), (1 << 30) if sg == "-" else 0
        if tail[0] == ",":
            hits[t, 0] = int(tail[1:-1])                                 # no gap: the count is all mismatches
        else:
            q = cigar_ops(tail)
            hits[t, 0] = 1 << 16
            rows[t, 1] = len(q)
            cig[t, :len(q)] = words(q)
    sel = (1 if tags["XT"] == "U" else 2, 0, int(f[4]), len(xa))
    return sam.sam_line(f[0], seq, qual, chrs, sel, (0, int(tags["X0"]), int(tags.get("X1", 0)), 0), rows, rpos, cig, md, pos,
                        hits, **kw)


@pytest.mark.parametrize("name", CASES)
def test_lines_with_trimmed_reads_and_barcodes(name):
    from hsa_amd import align, reads
    mode, trim = case_options(name)
    p = reads.parse_host(case_reads(name), mode=mode, trim_qual=trim)
    by_name = {n.decode(): k for k, n in enumerate(p["names"])}
    opts = align.default_opts()
    args = MANIFEST[name]["args"]
    for k, a in enumerate(args):
        if a in ("-n", "-o"):
            opts[{"-n": "max_diff", "-o": "max_gapo"}[a]] = int(args[k + 1])
    seen = dict(xc=0, bc=0, s=0, xa=0, rev_xc=0, fwd_xc=0, edge_s=0, refused=0)
    for ln in case_sam(name).decode("latin-1").splitlines():
        if "\0" in ln:
            seen["refused"] += 1                                # an N length that wrapped: the project refuses such a read
            continue
        k = by_name[ln.split("\t")[0]]
        read = (p["seqs"][k], p["quals"][k].decode("latin-1"), p["lens"][k], p["bcs"][k].decode() or None)
        assert reprint(ln, read, opts) == ln
        xc = "\tXC:i:" in ln
        seen["xc"] += xc
        seen["bc"] += "\tBC:Z:" in ln
        seen["s"] += "\tXT:A:S" in ln
        seen["xa"] += "\tXA:Z:" in ln
        seen["rev_xc"] += xc and bool(int(ln.split("\t")[1]) & 16)
        seen["fwd_xc"] += xc and not int(ln.split("\t")[1]) & 16
        if xc:
            ops = cigar_ops(ln.split("\t")[5])
            clip = len(p["seqs"][k]) - p["lens"][k]
            seen["edge_s"] += ops[0 if int(ln.split("\t")[1]) & 16 else -1][1] > clip
    m = MANIFEST[name]
    assert seen["xc"] == m["with_XC"] and seen["bc"] == m["with_BC"] and seen["s"] + seen["refused"] >= m["spliced"] > 0
    assert seen["refused"] <= 1
    if trim:
        assert seen["rev_xc"] > 0 and seen["fwd_xc"] > 0
    print(name, seen)


def test_option_parser_takes_the_readers_options():
    """bwtaln.c:558, :566-568; what is not built stays refused, and without reader_options the
    parser is the one of before."""
    from hsa_amd import align, reads
    po = lambda a: align.parse_options(a, reader_options=True)[0]
    base = align.default_opts()["mode"]
    assert po(["-q", "15"])["trim_qual"] == 15 and po(["-q", "15"])["mode"] == base and po([])["trim_qual"] == 0
    assert po(["-B", "6"])["mode"] == base | (6 << 24) and po(["-B", "63"])["mode"] >> 24 == 63 and po(["-B", "0"])["mode"] == base
    assert po(["-I"])["mode"] == base | MODE_IL13 == base | 0x200 and po(["-Y"])["mode"] == base | MODE_CFY == base | 0x08
    o = po(["-B", "6", "-q", "15", "-Y", "-I", "-n", "4"])
    assert o["mode"] == base | (6 << 24) | 0x208 and o["trim_qual"] == 15 and o["max_diff"] == 4
    assert po(["-q", str(reads.MAX_TRIM_QUAL)])["trim_qual"] == reads.MAX_TRIM_QUAL == 32674
    for bad in (["-b"], ["-0"], ["-1"], ["-2"], ["-c"], ["-B", "64"], ["-B", "-1"], ["-q", str(reads.MAX_TRIM_QUAL + 1)]):
        with pytest.raises(ValueError):
            po(bad)
    for name in CASES:
        mode, trim = case_options(name)
        o = po(MANIFEST[name]["args"])
        assert o["mode"] & ~base == mode and o["trim_qual"] == trim
    for bad in (["-q", "15"], ["-B", "6"], ["-I"], ["-Y"]):
        with pytest.raises(ValueError):
            align.parse_options(bad)


def test_clipped_cigar():
    from hsa_amd import sam
    w = lambda *ops: [(o << 28) | l for o, l in ops]
    assert sam.clipped_cigar(w((0, 35)), 0, 65) == "35M65S" and sam.clipped_cigar(w((0, 35)), 1, 65) == "65S35M"
    assert sam.clipped_cigar(w((0, 30), (4, 5)), 0, 65) == "30M70S" and sam.clipped_cigar(w((0, 30), (4, 5)), 1, 65) == "65S30M5S"
    assert sam.clipped_cigar(w((4, 5), (0, 30)), 1, 65) == "70S30M" and sam.clipped_cigar(w((4, 5), (0, 30)), 0, 65) == "5S30M65S"
    assert sam.clipped_cigar(w((0, 30), (2, 1), (0, 5)), 0, 0) == "30M1D5M"
    assert sam.clip_tags(35, 100, b"GGatAC") == ["BC:Z:GGatAC", "XC:i:35"] and sam.clip_tags(100, 100, None) == []
    assert sam.line_bound(7, 50, 5, 4, 20, 2, True, 6) == sam.line_bound(7, 50, 5, 4, 20, 2) + 26 + 12
