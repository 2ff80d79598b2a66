"""The reader's options on the host (no GPU): hsa_amd.reads.parse_host with mode / trim_qual
(-q, -B, -Y, -I; bwaseqio.c:161-231) against the reference program's SAM for the fixtures of
tools/make_golden_opts.py, and bwa_trim_read's and the Casava filter's corner cases against
hand-written expectations."""
import hashlib

import numpy as np
import pytest

from reads_opts_cases import CASES, MANIFEST, MODE_CFY, MODE_IL13, case_options, case_reads, case_sam, sam_fields

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def test_fixtures_are_the_manifests():
    for name in CASES:
        sam = case_sam(name)
        m = MANIFEST[name]
        assert hashlib.sha256(sam).hexdigest() == m["sam_sha256"] and sam.count(b"\n") == m["sam_lines"]
    assert case_sam("Iq15") == case_sam("q15")                # -I on the shifted file: byte for byte
    assert MANIFEST["q15"]["with_XC"] > 100 and MANIFEST["splice_q15"]["with_XC"] > 50
    assert MANIFEST["B6"]["with_BC"] == MANIFEST["B6"]["sam_lines"]
    assert MANIFEST["Y"]["sam_lines"] < MANIFEST["q15"]["sam_lines"]


@pytest.mark.parametrize("name", CASES)
def test_parse_host_against_the_reference(name):
    """Per reference line: XC is the restated trimmed length (no XC: the read is whole), BC:Z
    the restated barcode, SEQ and QUAL the whole read; a filtered read has no line."""
    from hsa_amd import reads
    mode, trim = case_options(name)
    data = case_reads(name)
    p = reads.parse_host(data, mode=mode, trim_qual=trim)
    every = reads.parse_host(data)
    by_name = {n: k for k, n in enumerate(p["names"])}
    assert len(by_name) == len(p["names"]) and len(every["names"]) == MANIFEST["n"][MANIFEST[name]["reads"]]
    assert p["filtered"] == len(every["names"]) - len(p["names"])
    assert (p["filtered"] > 0) == bool(mode & MODE_CFY)
    lines = case_sam(name).splitlines()
    seen_xc = seen_bc = 0
    for ln in lines:
        f = sam_fields(ln)
        assert f["name"] in by_name, "a filtered read has a line"
        k = by_name[f["name"]]
        full = len(p["seqs"][k])
        want = int(f["tags"][b"XC"]) if b"XC" in f["tags"] else full
        assert p["lens"][k] == want and (b"XC" in f["tags"]) == (p["lens"][k] < full)
        assert f["tags"].get(b"BC", b"") == p["bcs"][k]
        seq, qual = p["raw"][k].upper(), p["quals"][k]
        if f["flag"] & 16:
            seq, qual = seq.translate(COMP)[::-1], qual[::-1]
        assert f["seq"] == seq and f["qual"] == qual
        if b"BC" in f["tags"] and b"XC" in f["tags"]:
            assert f["order"].index(b"BC") < f["order"].index(b"XC") < f["order"].index(b"XT")
        seen_xc += b"XC" in f["tags"]
        seen_bc += b"BC" in f["tags"]
    assert seen_xc == MANIFEST[name]["with_XC"] and seen_bc == MANIFEST[name]["with_BC"]
    assert (seen_xc > 0) == (trim > 0) and (seen_bc > 0) == (mode >> 24 > 0)
    assert p["total_bases"] == sum(len(s) for s in p["seqs"]) and p["trimmed_bases"] == p["total_bases"] - sum(p["lens"])


def test_defaults_keep_the_results():
    from hsa_amd import reads
    data = case_reads("q15")
    a, b = reads.parse_host(data), reads.parse_host(data, mode=0x17, trim_qual=0)      # (the search's bits: no concern)
    assert a["names"] == b["names"] and a["quals"] == b["quals"] and a["raw"] == b["raw"] and a["consumed"] == b["consumed"]
    assert a["lens"] == [len(s) for s in a["seqs"]] and a["filtered"] == 0 and set(a["bcs"]) == {b""}
    assert a["trimmed_bases"] == 0 and a["orig"] == list(zip(a["raw"], a["quals"]))


def q(*runs):
    """Quality bytes from (phred, count) runs."""
    return b"".join(bytes([33 + v]) * n for v, n in runs)


# (quality, trim_qual, the length kept): bwa_trim_read walks l from len - 1 down to 35 with
# s += trim_qual - (q[l] - 33); s < 0 ends it; a strictly greater s moves the cut
TRIM = [
    (q((40, 100)), 20, 100),                                  # all high: whole
    (q((2, 100)), 20, 35),                                    # all low: cut to the floor
    (q((2, 35)), 20, 35), (q((2, 34)), 20, 34), (q((2, 36)), 20, 35),
    (q((2, 99), (21, 1)), 20, 100),                           # the last base alone above: the walk ends at once
    (q((40, 60), (15, 5), (25, 5), (10, 10)), 20, 70),        # two equal maxima (100 at l = 70 and, after -25 +25, at 60): the larger l
    (q((40, 35), (10, 65)), 20, 35),                          # the maximum exactly at l = 35
    (q((40, 34), (10, 66)), 20, 35),                          # ... and never under it
    (q((40, 50), (30, 10), (10, 10)), 20, 60),                # 100 at l = 60, exactly 0 at l = 50, negative at 49
    (q((40, 40), (5, 11), (30, 10), (10, 10)), 20, 40),       # a prefix sum of exactly 0 (l = 51) is not negative: the walk goes on to 165
    (q((40, 50), (10, 10), (30, 10), (10, 10)), 20, 70),      # 100 at l = 70, back to 0, 100 again at 50: not strictly greater
    (q((40, 50), (10, 11), (30, 10), (10, 10)), 20, 50),      # a dip that recovers to a strict maximum
    (q((40, 50), (0, 50)), 20, 50), (q((40, 50), (94, 1), (0, 49)), 1, 51),      # bytes 33 and 127
    (q((40, 200), (3, 100)), 15, 200), (q((40, 10), (3, 290)), 15, 35),
]


@pytest.mark.parametrize("k", range(len(TRIM)))
def test_trim_read(k):
    from hsa_amd import reads
    qual, tq, want = TRIM[k]
    assert reads.trim_read(tq, qual, len(qual)) == want
    assert reads.trim_read(0, qual, len(qual)) == len(qual) and reads.trim_read(tq, None, len(qual)) == len(qual)
    data = b"@r\n" + b"A" * len(qual) + b"\n+\n" + qual + b"\n"
    assert reads.parse_host(data, trim_qual=tq)["lens"] == [want]
    shifted = b"@r\n" + b"A" * len(qual) + b"\n+\n" + bytes(min(c + 31, 127) for c in qual) + b"\n"
    if max(qual) + 31 <= 127:
        p = reads.parse_host(shifted, trim_qual=tq, mode=MODE_IL13)
        assert p["lens"] == [want] and p["quals"] == [qual]


COMMENTS = [(b" :Y", True), (b" 1:Y:0", True), (b" 1:N:0", False), (b" Y", False), (b" a:b:Y", False), (b" x:", False),
            (b"", False), (b"\t1:Y:0", True), (b" \0:Y", False), (b" a\0b:Y", False), (b" N:N:Y", False), (b"  :Y", True)]


def test_casava_filter():
    from hsa_amd import reads
    data = b"".join(b"@r%d" % i + c + b"\nACGT\n+\nIIII\n" for i, (c, _) in enumerate(COMMENTS))
    p = reads.parse_host(data, mode=MODE_CFY)
    assert p["names"] == [b"r%d" % i for i, (_, gone) in enumerate(COMMENTS) if not gone]
    assert p["filtered"] == sum(g for _, g in COMMENTS)
    assert len(reads.parse_host(data)["names"]) == len(COMMENTS)
    few = reads.parse_host(data, max_records=2, mode=MODE_CFY)        # filtered records do not count
    assert few["names"] == [b"r2", b"r3"] and data[few["consumed"]:].startswith(b"@r4")


def test_barcode():
    from hsa_amd import reads
    rec = lambda s, ql: b"@r\n" + s + b"\n+\n" + ql + b"\n"
    mode = 3 << 24
    data = rec(b"acG", b"III") + rec(b"acGt", bytes([33 + 12, 33 + 13, 33 + 12, 73])) + rec(b"ACGTA", b"IIIII") + \
        b">f\nacgtn\n"
    p = reads.parse_host(data, mode=mode)
    assert p["names"] == [b"r", b"r", b"f"] and p["filtered"] == 1           # a read of the barcode's length goes
    assert p["bcs"] == [b"aCg", b"ACG", b"ACG"] and p["raw"] == [b"t", b"TA", b"tn"] and p["quals"] == [b"I", b"II", None]
    assert p["lens"] == [1, 2, 2] and p["orig"][0] == (b"acGt", bytes([45, 46, 45, 73]))
    il = reads.parse_host(rec(b"acgt", bytes([33 + 12 + 31, 33 + 13 + 31, 33 + 43, 33 + 44])), mode=mode | MODE_IL13)
    assert il["bcs"] == [b"aCg"] and il["quals"] == [bytes([33 + 13])]          # (43 - 31 = 12: low; 44 - 31 = 13: not)
    with pytest.raises(ValueError):
        reads.parse_host(data, mode=64 << 24)
    np.testing.assert_array_equal(p["seqs"][1], [3, 0])
