"""The host side of the FASTQ path (no GPU): hsa_amd.reads.parse_host against hand-written
expectations and against the reference program's own reader, maxdiff_table against
bwa_cal_maxdiff's arithmetic, hsa_amd.align's option parser against bwa_aln's switch, and
the post-switch N-count rule against a restatement of bwa_cal_sa_reg_gap's control flow."""
import os
import subprocess

import numpy as np
import pytest

from golden_io import INDEX
from hsa_amd import index_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HSA = os.path.join(ROOT, "oracle", "_ref", "HSA")


def parsed(data, **kw):
    from hsa_amd import reads
    p = reads.parse_host(data, **kw)
    return [(n, "".join("ACGTN-"[c] for c in s), q) for n, s, q in zip(p["names"], p["seqs"], p["quals"])], p


CASES = [
    # comments are cut at the first white space of any kind
    (b"@r1 a comment\nACGT\n+\nIIII\n@r2\tx\nAC\n+r2\nII\n", [(b"r1", "ACGT", b"IIII"), (b"r2", "AC", b"II")], -1),
    # /1 and /2 go, /3 stays; "a/1" becomes "a", "/1" is kept (bwaseqio.c:219: t > 2)
    (b"@x/1\nA\n+\nI\n@x/2\nC\n+\nI\n@x/3\nG\n+\nI\n@a/1\nT\n+\nI\n@/1\nA\n+\nI\n@y/1 z/2\nA\n+\nI\n",
     [(b"x", "A", b"I"), (b"x", "C", b"I"), (b"x/3", "G", b"I"), (b"a", "T", b"I"), (b"/1", "A", b"I"), (b"y", "A", b"I")], -1),
    # lower case, N, '.', and '-' (code 5)
    (b"@l\nacgtNn.-RX\n+\nIIIIIIIIII\n", [(b"l", "ACGTNNN-NN", b"IIIIIIIIII")], -1),
    # a sequence and a quality over several lines, blank lines, leading junk
    (b"junk\n\n@m\nAC\nGT\n\nA\n+\nII\nII\nI\n\n\n@n\nC\n+\nI\n", [(b"m", "ACGTA", b"IIIII"), (b"n", "C", b"I")], -1),
    # quality lines that start with '@' and with '+'
    (b"@q1\nACGT\n+\n@III\n@q2\nACGT\n+\n+III\n@q3\nAC\n+\n@+\n", [(b"q1", "ACGT", b"@III"), (b"q2", "ACGT", b"+III"),
                                                               (b"q3", "AC", b"@+")], -1),
    # no final newline
    (b"@e\nACGT\n+\nIIII", [(b"e", "ACGT", b"IIII")], -1),
    # FASTA, then FASTQ, then FASTA without a final newline
    (b">f1 d\nACGT\nAC\n@q\nAC\n+\nII\n>f2\nGG", [(b"f1", "ACGTAC", None), (b"q", "AC", b"II"), (b"f2", "GG", None)], -1),
    # CRLF: '\r' ends the name and is no base; the quality's '\r' is the byte read and dropped
    (b"@c x\r\nACGT\r\n+\r\nIIII\r\n@d\r\nAC\r\n+\r\nII\r\n", [(b"c", "ACGT", b"IIII"), (b"d", "AC", b"II")], -1),
    # a truncated quality at the end of the input: the reference stops reading (-2)
    (b"@ok\nAC\n+\nII\n@t\nACGT\n+\nII", [(b"ok", "AC", b"II")], -2),
    (b"@ok\nAC\n+\nII\n@t\nACGT\n+", [(b"ok", "AC", b"II")], -2),
    # an empty sequence is passed over (bwaseqio.c:185); an empty name is a name
    (b"@z\n\n+\n\n@ y\nA\n+\nI\n", [(b"", "A", b"I")], -1),
    # a quality byte outside 33..127 is skipped, not stored
    (b"@s\nACG\n+\nI I\tI\n", [(b"s", "ACG", b"III")], -1),
    (b"", [], -1),
]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_parse_host_cases(k):
    data, want, end = CASES[k]
    got, p = parsed(data)
    assert got == want and p["end"] == end


def test_parse_host_resumes_where_it_stopped():
    """max_records and `consumed`: parsing on from there gives the rest, FASTA records (whose
    end is the next record's header character) included."""
    data = b">f1\nAC\nGT\n@q1\nAC\n+\nII\n>f2\nG\n>f3\nT\n@q2\nA\n+\nI\n"
    whole, _ = parsed(data)
    assert len(whole) == 5
    for k in range(1, 5):
        head, p = parsed(data, max_records=k)
        assert p["end"] == 0 and data[p["consumed"]:p["consumed"] + 1] in (b">", b"@")
        rest, q = parsed(data, start=p["consumed"])
        assert head + rest == whole and q["end"] == -1 and q["consumed"] == len(data)


@pytest.mark.skipif(not os.path.exists(HSA), reason="oracle/_ref/HSA not built (make -C oracle)")
def test_reference_program_reads_what_parse_host_reads(tmp_path):
    """`HSA aln` on an oddly formatted FASTQ of reads cut from the tiny genome: the name, SEQ
    and QUAL of every line it prints are parse_host's for that read."""
    from hsa_amd import reads, synth
    text = index_io.read_pac(INDEX["tiny"])
    rng = np.random.default_rng(5)
    recs = []
    for k in range(120):
        l = int(rng.integers(36, 90))
        at = int(rng.integers(0, len(text) - l))
        sq = text[at:at + l]
        if k % 2:
            sq = synth.revcomp_codes(sq)
        s = "".join("ACGT"[c] for c in sq)
        if k % 5 == 0:
            s = s.lower()
        if k % 7 == 0:
            s = s[:10] + "N" + s[11:]
        q = rng.integers(33, 127, l).astype(np.uint8).tobytes().decode()
        if k % 9 == 0:
            q = "@" + q[1:]
        if k % 11 == 0:
            q = "+" + q[1:]
        name = f"read{k}" + ("", "/1", "/2", "/3", " comment/1", "\tc")[k % 6]
        kind = k % 4
        if kind == 0:
            recs.append(f"@{name}\n{s}\n+\n{q}\n")
        elif kind == 1:
            recs.append(f"\n@{name}\n{s[:17]}\n{s[17:]}\n+{name}\n{q[:5]}\n{q[5:]}\n\n")
        elif kind == 2:
            recs.append(f"@{name}\r\n{s}\r\n+\r\n{q}\r\n")
        else:
            recs.append(f">{name}\n{s[:30]}\n{s[30:]}\n")
    data = "".join(recs).encode()
    fq = tmp_path / "odd.fq"
    fq.write_bytes(data)
    r = subprocess.run([HSA, "aln", "-n", "4", "-o", "0", INDEX["tiny"], str(fq)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    p = reads.parse_host(data)
    assert len(p["names"]) == 120 and p["end"] == -1
    at = {n.decode(): k for k, n in enumerate(p["names"])}
    lines = [ln.split("\t") for ln in r.stdout.decode().split("\n") if ln and ln[0] != "@"]
    assert len(lines) >= 100
    for f in lines:
        k = at[f[0]]
        rev = int(f[1]) & 16
        sq = p["seqs"][k]
        want = "".join("TGCAN"[c] for c in sq[::-1]) if rev else "".join("ACGTN"[c] for c in sq)
        assert f[9] == want, f[0]
        q = p["quals"][k]
        assert f[10] == ("*" if q is None else (q[::-1] if rev else q).decode()), f[0]


# ---------------------------------------------------------------- max_diff
def c_maxdiff(l, err, thres):
    """bwa_cal_maxdiff (bwtaln.c:46-58) with C's types: doubles, and an int x that wraps."""
    with np.errstate(all="ignore"):
        el = np.exp(np.float64(-l * err))
        y, x, s = np.float64(1.0), np.int32(1), el
        for k in range(1, 1000):
            y = y * np.float64(l * err)
            x = np.int32((int(x) * k + 2 ** 31) % 2 ** 32 - 2 ** 31)
            s = s + el * y / np.float64(x)
            if np.float64(1.0) - s < thres:
                return k
    return 2


def test_maxdiff_table():
    from hsa_amd import reads
    fnr = float(np.float32(0.04))
    t = reads.maxdiff_table(fnr, 300)
    assert t.dtype == np.int32 and len(t) == 300
    # the lengths at which `HSA aln` announces a new max_diff (bwtaln.c:609-616)
    assert [(l, int(t[l])) for l in range(17, 251) if t[l] != t[l - 1] or l == 17] == \
        [(17, 2), (38, 3), (64, 4), (93, 5), (124, 6), (157, 7), (190, 8), (225, 9)]
    for f in (fnr, 0.01, 0.2, 0.5):
        tab = reads.maxdiff_table(f, 64)
        assert [int(v) for v in tab] == [c_maxdiff(l, 0.02, f) for l in range(64)]
    for l in (300, 1000, 2500, 4095, 20000, 65535):           # where x has wrapped, and where exp underflows
        assert reads.cal_maxdiff(l, 0.02, fnr) == c_maxdiff(l, 0.02, fnr), l


# ---------------------------------------------------------------- options
def test_option_parser_follows_the_switch():
    from hsa_amd import align
    d = align.default_opts()
    assert d["mode"] == 0x03 and d["max_diff"] == -1 and abs(d["fnr"] - 0.04) < 1e-8 and d["fnr"] == float(np.float32(0.04))
    assert (d["s_mm"], d["s_gapo"], d["s_gape"], d["max_gapo"], d["max_gape"], d["seed_len"], d["max_seed_diff"]) == (3, 11, 4, 1, 6, 32, 2)
    assert (d["indel_end_skip"], d["max_del_occ"], d["max_entries"], d["max_top2"], d["trim_qual"]) == (5, 10, 2000000, 30, 0)
    o, rest, ex = align.parse_options(["-n", "4", "-o", "0", "idx", "in.fq"])
    assert (o["max_diff"], o["fnr"], o["max_gapo"]) == (4, -1.0, 0) and rest == ["idx", "in.fq"] and not ex["header"]
    o, _, _ = align.parse_options(["-n", "0.01"])
    assert o["max_diff"] == -1 and o["fnr"] == float(np.float32(0.01))
    o, _, _ = align.parse_options(["-n", "5.", "-n", "3"])                # the last one holds
    assert (o["max_diff"], o["fnr"]) == (3, -1.0)
    o, _, _ = align.parse_options("-e 3 -M 2 -O 9 -E 5 -d 7 -i 2 -l 25 -k 1 -m 1000 -R 4 -L".split())
    assert o["max_gape"] == 3 and not o["mode"] & 0x01 and o["mode"] & 0x04            # opte > 0 clears GAPE
    assert (o["s_mm"], o["s_gapo"], o["s_gape"], o["max_del_occ"], o["indel_end_skip"], o["seed_len"], o["max_seed_diff"],
            o["max_entries"], o["max_top2"]) == (2, 9, 5, 7, 2, 25, 1, 1000, 4)
    o, _, _ = align.parse_options(["-e", "0"])                            # opte > 0 only
    assert o["max_gape"] == 6 and o["mode"] & 0x01
    o, _, _ = align.parse_options(["-e", "-1"])
    assert o["max_gape"] == 6 and o["mode"] & 0x01
    o, _, _ = align.parse_options(["-N", "-R", "7"])                      # in order: -R after -N holds
    assert o["mode"] & 0x10 and o["max_top2"] == 7
    o, _, _ = align.parse_options(["-R", "7", "-N"])
    assert o["max_top2"] == 0x7FFFFFFF
    o, _, _ = align.parse_options(["-o", "2x", "-l", "abc", "-t", "8"])    # atoi
    assert o["max_gapo"] == 2 and o["seed_len"] == 0 and o["n_threads"] == 8
    o, rest, ex = align.parse_options(["idx", "-n", "2", "in.fq", "--header", "--unaligned", "u.fq", "-f", "out.sam"])
    assert rest == ["idx", "in.fq"] and ex == dict(header=True, unaligned="u.fq", out="out.sam") and o["max_diff"] == 2
    for bad in (["-q", "20"], ["-b"], ["-0"], ["-1"], ["-2"], ["-I"], ["-Y"], ["-B", "6"], ["-c"]):
        with pytest.raises(ValueError):
            align.parse_options(bad)
    assert align.parse_options(["-q", "0"])[0]["trim_qual"] == 0


# ---------------------------------------------------------------- the threshold after the switch
def loop_skips(lens, n_n, polyat, hit, table):
    """bwtaln.c:303-373's control flow: the reads skipped at :316.  aux->opt points at the
    caller's block until the first searched read without a hit, at local_opt from there on;
    :331 writes through it, :316 reads local_opt."""
    local_max = int(table[max(lens)])                         # :273-274
    through_local, skipped = False, []
    for i in range(len(lens)):
        if n_n[i] > local_max:                                # :314-317
            skipped.append(i)
            continue
        if polyat[i]:                                         # :324-325
            continue
        if through_local:                                     # :330-331
            local_max = int(table[lens[i]])
        if not hit[i]:                                        # :362-363
            through_local = True
    return skipped


@pytest.mark.parametrize("seed", range(8))
def test_post_switch_threshold_rule(seed):
    from hsa_amd import align, reads
    table = reads.maxdiff_table(float(np.float32(0.04)), 260)
    rng = np.random.default_rng(seed)
    n = 400
    lens = rng.choice([20, 36, 40, 70, 100, 130, 250], n)
    n_n = rng.choice([0, 0, 1, 2, 3, 4, 5, 6, 7, 9, 12], n)
    polyat = rng.random(n) < 0.05
    hit = rng.random(n) < (1.0 if seed == 0 else 0.97)
    want = loop_skips(lens, n_n, polyat, hit, table)
    thr0 = int(table[lens.max()])
    status = np.where(n_n > thr0, 1, np.where(polyat, 2, 0))  # the loader's, with the batch's threshold
    searched = np.flatnonzero(status == 0)
    nohit = [r for r in searched if not hit[r]]
    got = set(np.flatnonzero(status == 1).tolist())
    if nohit:
        after = align.post_switch_skips(lens, n_n, status == 2, nohit[0] + 1, lambda l: int(table[l]), thr0)
        assert all(r > nohit[0] for r in after)
        got |= set(after)
    assert sorted(got) == want
    if seed:
        assert nohit and len(want) > int((status == 1).sum())  # the rule narrowed something
