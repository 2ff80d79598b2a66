"""The serial core of the BAM loader (hsa_amd/csrc/hsa_bam.h: the hop check, the field offsets,
the per-position decode) as plain host C++ under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/san/bam_main.cpp, its own executable, nothing preloaded).  Every text is a heap block of
its exact size.  The valid texts of tests/bam_cases.py must give hsa_amd.bam.parse_host's
records; a valid text cut at every length, and with each of its first 600 bytes replaced by
0x00, 0x7F and 0xFF, must end where parse_host ends, with its records, and without a report.
This is where the bounds checks are proven, before a corrupt byte reaches a GPU."""
import os
import shutil
import struct
import subprocess

import pytest

import bam_cases as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("san") / "bam_main")
    r = subprocess.run(["g++", *FLAGS, os.path.join(ROOT, "tests/san/bam_main.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(san_bin, tmp_path, cases):
    """cases: (text, which, trim_qual) -> [dict(end, consumed, filtered, reads: [(name, codes, quals, len)])]"""
    (tmp_path / "cases.bin").write_bytes(b"".join(struct.pack("<IIi", len(t), w, q) + t for t, w, q in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([san_bin, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    raw, at, got = (tmp_path / "out.bin").read_bytes(), 0, []
    for _ in cases:
        end, consumed, filtered, n = struct.unpack_from("<IIII", raw, at)
        at += 16
        rs = []
        for _ in range(n):
            nl, = struct.unpack_from("<I", raw, at)
            name = raw[at + 4:at + 4 + nl]
            l_seq, ln = struct.unpack_from("<II", raw, at + 4 + nl)
            at += 12 + nl
            rs.append((name, raw[at:at + l_seq], raw[at + l_seq:at + 2 * l_seq], ln))
            at += 2 * l_seq
        got.append(dict(end=end, consumed=consumed, filtered=filtered, reads=rs))
    assert at == len(raw)
    return got


def expected(text, which, trim_qual):
    from hsa_amd import bam
    p = bam.parse_host(text, which=which, trim_qual=trim_qual)
    return dict(end={-1: 1, -2: 2}[p["end"]], consumed=p["consumed"], filtered=p["filtered"],
                reads=[(n, s.tobytes(), q, l) for n, s, q, l in zip(p["names"], p["seqs"], p["quals"], p["lens"])])


def test_valid_texts_give_the_restatements_records(san_bin, tmp_path):
    cases = [(t, w, q) for _, t, w, q in bm.texts()]
    got = run(san_bin, tmp_path, cases)
    for (name, *_), c, g in zip(bm.texts(), cases, got):
        assert g == expected(*c), name
        assert g["end"] == 1 and g["consumed"] == len(c[0]), name
    assert sum(len(g["reads"]) for g in got) > 100 and any(l != len(s) for g in got for _, s, _, l in g["reads"])


def test_every_truncation_and_byte_replacement_stays_inside(san_bin, tmp_path):
    """One small valid text cut at every length, and with each of its first 600 bytes replaced
    by 0x00, 0x7F and 0xFF in turn: the walk ends where the restatement's ends, with its
    records, and nothing is read outside the block."""
    text = b"".join(bm.from_fastq(bm.small_fastq(6))[:6] + bm.edge_records()[:4])
    assert len(text) > 700
    cases = [(text[:k], 7, 15) for k in range(len(text))]
    for k in range(600):
        for v in (0x00, 0x7F, 0xFF):
            if text[k] != v:
                cases.append((text[:k] + bytes([v]) + text[k + 1:], 7, 15))
    got = run(san_bin, tmp_path, cases)
    n_bad = 0
    for c, g in zip(cases, got):
        want = expected(*c)
        assert g == want, (len(c[0]), [k for k in range(min(len(c[0]), len(text))) if c[0][k] != text[k]][:1])
        n_bad += g["end"] == 2
    # a cut inside a record is a truncated record; a cut at one of the 10 boundaries is a shorter valid text
    assert n_bad >= len(text) - 12 and n_bad < len(cases)
