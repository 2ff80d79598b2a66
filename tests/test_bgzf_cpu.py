"""hsa_amd.bgzf.scan: the host walk over a BGZF file's members.  It takes the files the writer
of tests/bgzf_cases.py makes (bgzip's format) and nothing else: any member that is not BGZF
makes the whole file the host's (None)."""
import gzip
import struct
import zlib

import numpy as np

import bgzf_cases as bc
from hsa_amd import bgzf

RAW = bc.fastq_snippet(5000)


def members(data, table):
    """The members' decompressed bytes by the table's payload spans."""
    return [zlib.decompress(data[int(r["in_off"]):int(r["in_off"]) + int(r["in_len"])], -15) for r in table]


def test_scan_takes_the_writers_files():
    for block, eof in ((65280, True), (700, True), (700, False), (1, True)):
        raw = RAW[:40] if block == 1 else RAW
        data = bc.bgzf_file(raw, block=block, eof=eof)
        t = bgzf.scan(data)
        assert t is not None and len(t) == -(-len(raw) // block) + eof
        got = members(data, t)
        assert b"".join(got) == raw == gzip.decompress(data)
        assert [int(v) for v in t["isize"]] == [len(g) for g in got]
        assert [int(v) for v in t["crc"]] == [zlib.crc32(g) for g in got]
        if eof:
            assert data.endswith(bc.EOF_MARKER) and len(bc.EOF_MARKER) == 28 and t["isize"][-1] == 0 and t["in_len"][-1] == 2


def test_output_offsets_are_the_running_sums():
    data = bc.bgzf_file(RAW, block=300) + bc.bgzf_file(RAW[:777], block=1000, eof=False) + bc.bgzf_file(b"", eof=True)
    t = bgzf.scan(data)
    lens = [len(m) for m in members(data, t)]
    assert [int(v) for v in t["out_off"]] == [sum(lens[:k]) for k in range(len(lens))]
    assert t["out_off"].dtype == np.uint64 and t.dtype.itemsize == 32


def test_empty_file_is_an_empty_table():
    t = bgzf.scan(b"")
    assert t is not None and len(t) == 0


def test_scan_refuses_what_is_not_bgzf():
    good = bc.bgzf_file(RAW, block=2000)
    assert bgzf.scan(good) is not None
    assert bgzf.scan(gzip.compress(RAW)) is None
    # FNAME set next to FEXTRA, the name behind the extra field
    m = bytearray(bc.bgzf_member(bc.deflate(RAW[:100]), RAW[:100]))
    m[3] |= 0x08
    named = bytes(m[:18]) + b"name\0" + bytes(m[18:])
    assert bgzf.scan(named) is None and bgzf.scan(bytes(m)) is None
    # BSIZE past the end: the last member cut, and a BSIZE made larger
    assert bgzf.scan(good[:-1]) is None
    m = bytearray(bc.bgzf_member(bc.deflate(RAW[:100]), RAW[:100]))
    struct.pack_into("<H", m, 16, len(m) + 5)
    assert bgzf.scan(bytes(m)) is None
    assert bgzf.scan(good + b"\0\0\0") is None and bgzf.scan(good + b"garbage behind the last member") is None
    assert bgzf.scan(good + gzip.compress(b"plain member")) is None
    assert bgzf.scan(gzip.compress(b"plain member") + good) is None
    # an extra field without BC, and a BC of another length
    m = bytearray(bc.bgzf_member(bc.deflate(b"x"), b"x"))
    m[12:14] = b"XY"
    assert bgzf.scan(bytes(m)) is None
    m = bytearray(bc.bgzf_member(bc.deflate(b"x"), b"x"))
    m[14:16] = struct.pack("<H", 1)
    assert bgzf.scan(bytes(m)) is None


def test_other_subfields_are_skipped():
    """BC need not be the only subfield (RFC 1952's extra field is a list)."""
    raw = RAW[:500]
    payload = bc.deflate(raw)
    size = 12 + 12 + len(payload) + 8
    head = b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff" + struct.pack("<H", 12) + b"ZZ" + struct.pack("<H", 2) + b"ab" + \
        b"BC" + struct.pack("<HH", 2, size - 1)
    data = head + payload + struct.pack("<II", zlib.crc32(raw), len(raw))
    t = bgzf.scan(data)
    assert t is not None and members(data, t) == [raw] and gzip.decompress(data) == raw


def test_read_input_of_plain_and_general_gzip_files(tmp_path):
    """Neither touches the device: a plain file as it is, general gzip through Python's gzip,
    both with all-zero statistics and no device tensor."""
    (tmp_path / "a.fq").write_bytes(RAW)
    (tmp_path / "a.fq.gz").write_bytes(gzip.compress(RAW))
    (tmp_path / "mixed.fq.gz").write_bytes(bc.bgzf_file(RAW[:1000], eof=False) + gzip.compress(RAW[1000:]))
    for name in ("a.fq", "a.fq.gz", "mixed.fq.gz"):
        text, d_text, stats = bgzf.read_input(None, str(tmp_path / name))
        assert text == RAW and d_text is None and stats == bgzf.NO_STATS and not any(stats.values()), name
