"""hsa_amd.bam on the host: parse_host, the restatement of bwa_read_bam without its line 142,
gives for BAMs made of the option fixtures' reads what reads.parse_host gives for the FASTQ;
selection by `which`; the nt16 table, missing qualities, empty records, names; the header; the
command line's -b, -0, -1, -2."""
import gzip

import numpy as np
import pytest

import bam_cases as bm
from reads_opts_cases import case_reads


def body(text):
    from hsa_amd import bam
    return bam.read_header(text)[0]


@pytest.mark.parametrize("name,trim", [("q15", 15), ("q15", 0), ("splice_q15", 15), ("splice_q20n4o1", 20)])
def test_fixture_reads_come_back_as_the_fastq_reader_gives_them(name, trim):
    from hsa_amd import bam, reads
    fq = case_reads(name)
    want = reads.parse_host(fq, trim_qual=trim)
    text = bm.text_of(bm.from_fastq(fq))
    p = bam.parse_host(text, start=body(text), trim_qual=trim)
    assert p["names"] == want["names"] and p["quals"] == want["quals"] and p["lens"] == want["lens"]
    assert all(np.array_equal(a, b) for a, b in zip(p["seqs"], want["seqs"]))
    assert p["raw"] == [s.upper() for s in want["raw"]]
    assert (p["end"], p["consumed"], p["filtered"]) == (-1, len(text), 0) and p["bcs"] == [b""] * len(want["names"])
    assert p["trimmed_bases"] == want["trimmed_bases"] and p["total_bases"] == want["total_bases"]
    if trim:
        assert p["trimmed_bases"] > 0
    # the three containers hold the same text
    recs = bm.from_fastq(fq)
    assert gzip.decompress(bm.aligned(recs, 4096)) == gzip.decompress(bm.straddling(recs, 512)) == gzip.decompress(bm.one_stream(recs)) == text


def test_max_records_and_start():
    from hsa_amd import bam
    from hsa_amd import reads
    recs = bm.from_fastq(bm.small_fastq())
    text = b"".join(recs)
    every, want = bam.parse_host(text), reads.parse_host(bm.small_fastq())
    assert {len(s) % 2 for s in every["seqs"]} == {0, 1}                     # odd and even lengths
    assert every["names"] == want["names"] and every["quals"] == want["quals"]
    assert all(np.array_equal(a, b) for a, b in zip(every["seqs"], want["seqs"]))
    p = bam.parse_host(text, 5)
    assert len(p["names"]) == 5 and p["end"] == 0 and p["consumed"] == sum(len(r) for r in recs[:5])
    q = bam.parse_host(text, start=p["consumed"])
    assert len(q["names"]) == len(recs) - 5 and q["end"] == -1
    cut = bam.parse_host(text[:-1])
    assert cut["end"] == -2 and len(cut["names"]) == len(recs) - 1 and cut["consumed"] == len(text) - len(recs[-1])


@pytest.mark.parametrize("args,which", [(["-b", "-0"], 4), (["-b", "-1"], 1), (["-b", "-2"], 2), (["-b", "-1", "-2"], 3), (["-b"], 7)])
def test_selection_by_which(args, which):
    from hsa_amd import align, bam
    mode = align.parse_options(args, bam_options=True)[0]["mode"]
    assert mode & bam.MODE_BAM and bam.which_of(mode) == which
    recs = bm.edge_records()
    p = bam.parse_host(b"".join(recs), which=which)
    flags = {b"pair/1": 1, b"pair/2": 2, b"both": 3, b"supplementary": 2, b"polyTrev": 1}
    names = [b"all16", b"all16rev", b"noqual", b"cut", b"pair/1", b"pair/2", b"both", b"secondary", b"supplementary", b"trimfwd",
             b"trimrev", b"highq", b"polyA", b"polyTrev", b"n" * 254]
    want = [n for n in names if (flags.get(n, 0) & which) or (which & 4 and n not in flags)]
    assert p["names"] == want and p["filtered"] == len(recs) - len(want) and p["end"] == -1
    if which == 7:
        assert b"secondary" in want and b"supplementary" in want


def test_codes_qualities_empty_records_and_names():
    from hsa_amd import bam
    p = bam.parse_host(b"".join(bm.edge_records()))
    r = dict(zip(p["names"], zip(p["seqs"], p["quals"], p["lens"])))
    nt4 = {1: 0, 2: 1, 4: 2, 8: 3}
    want = [nt4.get(k, 4) for k in range(16)] * 3
    assert list(r[b"all16"][0]) == want and want[0] == 4              # '=' is 4
    assert list(r[b"all16rev"][0]) == [c if c > 3 else 3 - c for c in want[::-1]]
    assert r[b"all16"][1] == bytes(range(33, 33 + 48)) and r[b"all16rev"][1] == bytes(range(33, 33 + 48))[::-1]
    assert r[b"noqual"][1] == b"~" * 21
    assert r[b"highq"][1] == bytes([125, 126, 126, 126] * 10)
    assert b"empty" not in r and p["filtered"] == 1
    assert b"cut" in r and b"pair/1" in r and b"pair/2" in r       # the NUL cuts, /1 stays
    q20 = bam.parse_host(b"".join(bm.edge_records()), trim_qual=20)
    t = dict(zip(q20["names"], q20["lens"]))
    assert t[b"trimfwd"] == t[b"trimrev"] == 60 and q20["trimmed_bases"] >= 40


def test_header():
    from hsa_amd import bam
    text = bm.header(b"@HD\tVN:1.6\n@SQ\tSN:a\tLN:10\n", ((b"a", 10), (b"chr2", 12345)))
    assert bam.read_header(text + b"rest") == (len(text), [(b"a", 10), (b"chr2", 12345)])
    assert bam.read_header(bm.header(b"", ())) == (12, [])
    with pytest.raises(ValueError, match="magic"):
        bam.read_header(b"BAM\x02" + text[4:])
    with pytest.raises(ValueError, match="magic"):
        bam.read_header(b"@r0\nACGT\n+\nIIII\n")
    with pytest.raises(ValueError, match="truncated"):
        bam.read_header(text[:-3])


def test_parser_takes_the_bam_options_only_when_asked():
    from hsa_amd import align
    base = align.default_opts()["mode"]
    po = lambda a: align.parse_options(a, reader_options=True, bam_options=True)[0]["mode"]
    assert po(["-b"]) == base | 0x20 and po(["-0"]) == base | 0x40 and po(["-1"]) == base | 0x80 and po(["-2"]) == base | 0x100
    assert po(["-b", "-1", "-2", "-q", "15", "-Y"]) == base | 0x1A0 | 0x08
    for opt in ("-b", "-0", "-1", "-2"):
        for kw in ({}, dict(reader_options=True)):
            with pytest.raises(ValueError, match="not built"):
                align.parse_options([opt], **kw)
    with pytest.raises(ValueError, match="not built"):
        align.parse_options(["-c"], reader_options=True, bam_options=True)
