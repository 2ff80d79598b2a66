"""The serial core of the BGZF inflater (hsa_amd/csrc/hsa_inflate.h: bit reader, code tables,
symbol loop, CRC pieces) as plain host C++ under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/san/inflate_main.cpp, its own executable, nothing preloaded).  Every payload and every
output slice is a heap block of its exact size: the valid blocks must give zlib's bytes, the
corrupt ones the status hsa_gpu.h names, and neither a sanitizer report.  This is where the
bounds checks are proven, before a corrupt byte reaches a GPU."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import bgzf_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("san") / "inflate_main")
    r = subprocess.run(["g++", *FLAGS, os.path.join(ROOT, "tests/san/inflate_main.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(san_bin, tmp_path, cases):
    """cases: (payload, isize, crc) -> [(status, the slice's bytes)]"""
    (tmp_path / "cases.bin").write_bytes(b"".join(struct.pack("<III", len(p), n, c) + p for p, n, c in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([san_bin, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    raw, got, at = (tmp_path / "out.bin").read_bytes(), [], 0
    for _, n, _ in cases:
        got.append((struct.unpack_from("<I", raw, at)[0], raw[at + 4:at + 4 + n]))
        at += 4 + n
    assert at == len(raw)
    return got


def test_valid_blocks_give_zlibs_bytes(san_bin, tmp_path):
    cases = bc.valid_cases()
    got = run(san_bin, tmp_path, [(p, len(raw), zlib.crc32(raw)) for _, p, raw in cases])
    for (name, p, raw), (st, data) in zip(cases, got):
        assert st == bc.OK, (name, st)
        assert data == zlib.decompress(p, -15) == raw, name


def test_corrupt_blocks_end_as_their_status(san_bin, tmp_path):
    cases = bc.corrupt_cases()
    got = run(san_bin, tmp_path, [(p, n, c) for _, p, n, c, _ in cases])
    assert [(name, st) for (name, *_), (st, _) in zip(cases, got)] == [(name, want) for name, *_, want in cases]


def test_every_truncation_and_bit_flip_stays_inside(san_bin, tmp_path):
    """A dynamic block cut at every length, and with each of its first 600 bits flipped: any
    status, the right bytes where it is OK, and no report."""
    raw = bc.fastq_snippet(1200)
    good = bc.deflate(raw, 9)
    crc = zlib.crc32(raw)
    cases = [(good[:k], len(raw), crc) for k in range(len(good))]
    for k in range(min(600, 8 * len(good))):
        bad = bytearray(good)
        bad[k >> 3] ^= 1 << (k & 7)
        cases.append((bytes(bad), len(raw), crc))
    got = run(san_bin, tmp_path, cases)
    assert all(st != bc.OK for st, _ in got[:len(good)])
    assert all(data == raw for st, data in got if st == bc.OK)
