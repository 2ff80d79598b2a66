"""hsa_inflate_bgzf_device and hsa_amd.bgzf.inflate_device: the valid blocks of
tests/bgzf_cases.py (every block type, every kind of header and match) come back OK with
zlib's bytes and none handed to the host; the corrupt ones (proven to stay inside their
buffers on the host first, tests/test_inflate_san.py) come back with their status and leave
their neighbours alone; whole files across the grouping by `budget`."""
import gzip
import zlib

import numpy as np
import pytest

import bgzf_cases as bc

pytestmark = pytest.mark.gpu


def run_members(members):
    """hsa_inflate_bgzf_device over the BGZF file the members make: (the table, the status per
    block, the counters, the output's bytes)."""
    import torch
    from hsa_amd import _lib, bgzf
    data = b"".join(members)
    t = bgzf.scan(data)
    assert t is not None and len(t) == len(members)
    cap = int(t["isize"].sum())
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_rows = torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_status = torch.full((len(t),), -1, dtype=torch.int32, device="cuda")
    d_ctr = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _lib.inflate_bgzf_device(_lib.InflateBatch(d_in=d_in.data_ptr(), n_in=len(data), d_blocks=d_rows.data_ptr(), n_blocks=len(t),
                                               d_out=d_out.data_ptr(), out_cap=cap, d_status=d_status.data_ptr(),
                                               d_counters=d_ctr.data_ptr()))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[cap:] == 0xEE).all()                       # nothing behind the capacity
    return t, d_status.cpu().numpy().view(np.uint32), [int(v) for v in d_ctr.cpu().numpy()], out[:cap].tobytes()


@pytest.fixture(scope="module")
def valid():
    cases = bc.valid_cases()
    return cases, run_members([bc.bgzf_member(p, raw) for _, p, raw in cases])


def test_every_valid_block_is_ok_in_one_call(valid):
    cases, (t, status, ctr, out) = valid
    assert [(c[0], int(s)) for c, s in zip(cases, status)] == [(c[0], bc.OK) for c in cases]
    assert ctr == [len(cases), 0, sum(len(c[2]) for c in cases)]


@pytest.mark.parametrize("k", range(len(bc.valid_cases())), ids=[c[0] for c in bc.valid_cases()])
def test_valid_block_gives_zlibs_bytes(valid, k):
    cases, (t, status, ctr, out) = valid
    name, payload, raw = cases[k]
    at = int(t["out_off"][k])
    got = out[at:at + int(t["isize"][k])]
    assert status[k] == bc.OK and got == zlib.decompress(payload, -15) == raw
    assert zlib.crc32(got) == int(t["crc"][k])


def test_the_empty_block_alone():
    for payload in (bc.deflate(b""), bc.deflate(b"", 0)):
        t, status, ctr, out = run_members([bc.bgzf_member(payload, b"")])
        assert list(status) == [bc.OK] and ctr == [1, 0, 0] and out == b""
    t, status, ctr, out = run_members([bc.EOF_MARKER])
    assert list(status) == [bc.OK] and ctr == [1, 0, 0]


def test_valid_blocks_through_inflate_device(valid):
    from hsa_amd import bgzf
    cases = valid[0]
    data = b"".join(bc.bgzf_member(p, raw) for _, p, raw in cases) + bc.EOF_MARKER
    text, d_text, stats = bgzf.inflate_device(None, data)
    want = b"".join(c[2] for c in cases)
    assert text == want == gzip.decompress(data)
    assert d_text is not None and d_text[:len(want)].cpu().numpy().tobytes() == want
    assert stats["device_blocks"] == stats["blocks"] == len(cases) + 1 and stats["host_blocks"] == 0 and stats["groups"] == 1
    assert stats["bytes_in"] == len(data) and stats["bytes_out"] == len(want)


def test_corrupt_blocks_end_as_their_status_and_leave_their_neighbours():
    fq = bc.fastq_snippet()
    good = bc.bgzf_member(bc.deflate(fq, 9), fq)
    corrupt = bc.corrupt_cases()
    members = [good]
    for _, payload, isize, crc, _ in corrupt:
        members += [bc.bgzf_member(payload, b"", crc=crc, isize=isize), good]
    t, status, ctr, out = run_members(members)
    assert [(c[0], int(s)) for c, s in zip(corrupt, status[1::2])] == [(c[0], c[4]) for c in corrupt]
    assert (status[0::2] == bc.OK).all()
    for k in range(0, len(members), 2):
        at = int(t["out_off"][k])
        assert out[at:at + len(fq)] == fq, k
    assert ctr == [len(corrupt) + 1, len(corrupt), (len(corrupt) + 1) * len(fq)]


def test_a_row_outside_the_buffers_is_refused():
    """in_len past the file's end, a slice past the capacity: HSA_INF_E_ROW, nothing touched."""
    import torch
    from hsa_amd import _lib, bgzf
    fq = bc.fastq_snippet(500)
    data = bc.bgzf_member(bc.deflate(fq), fq)
    t = np.concatenate([bgzf.scan(data)] * 3)
    t["out_off"] = [0, 0, 1]
    t["in_len"][0] = len(data)                             # (from in_off on: past the end)
    t["isize"][2] = len(fq)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_rows = torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.zeros(len(fq) + 8, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(3, dtype=torch.int32, device="cuda")
    d_ctr = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _lib.inflate_bgzf_device(_lib.InflateBatch(d_in=d_in.data_ptr(), n_in=len(data), d_blocks=d_rows.data_ptr(), n_blocks=3,
                                               d_out=d_out.data_ptr(), out_cap=len(fq), d_status=d_status.data_ptr(),
                                               d_counters=d_ctr.data_ptr()))
    torch.cuda.synchronize()
    assert list(d_status.cpu().numpy()) == [bc.E_ROW, bc.OK, bc.E_ROW]
    assert d_out.cpu().numpy().tobytes() == fq + bytes(8)


def test_a_wrong_crc_raises_from_the_host_path():
    from hsa_amd import bgzf
    fq = bc.fastq_snippet()
    good = bc.bgzf_member(bc.deflate(fq, 9), fq)
    bad = bc.bgzf_member(bc.deflate(fq, 9), fq, crc=zlib.crc32(fq) ^ 1)
    with pytest.raises(gzip.BadGzipFile, match="CRC"):
        bgzf.inflate_device(None, good + bad + good + bc.EOF_MARKER)
    with pytest.raises(gzip.BadGzipFile):
        gzip.decompress(good + bad + good + bc.EOF_MARKER)


@pytest.mark.parametrize("blocks", [1, 2, 65, 130])
def test_files_of_small_blocks(blocks):
    """300-byte blocks: more blocks than any grouping by 64 holds."""
    from hsa_amd import bgzf
    raw = (bc.fastq_snippet(20000) * 2)[:300 * blocks]
    data = bc.bgzf_file(raw, block=300, level=6)
    text, d_text, stats = bgzf.inflate_device(None, data)
    assert text == raw and d_text[:len(raw)].cpu().numpy().tobytes() == raw
    assert stats["blocks"] == stats["device_blocks"] == blocks + 1 and stats["host_blocks"] == 0


def test_a_small_budget_makes_three_groups():
    from hsa_amd import bgzf
    raw = bc.fastq_snippet(20000)[:300 * 9]
    data = bc.bgzf_file(raw, block=300, eof=False)
    text, d_text, stats = bgzf.inflate_device(None, data, budget=900)
    assert text == raw and d_text is None
    assert stats["groups"] == 3 and stats["blocks"] == stats["device_blocks"] == 9 and stats["host_blocks"] == 0
    # a budget under one block still takes a block at a time
    text, d_text, stats = bgzf.inflate_device(None, data, budget=1)
    assert text == raw and stats["groups"] == 9


def test_read_input_of_a_bgzf_file(tmp_path):
    from hsa_amd import bgzf
    raw = bc.fastq_snippet(20000)
    p = tmp_path / "reads.fq.gz"
    p.write_bytes(bc.bgzf_file(raw, block=700))
    text, d_text, stats = bgzf.read_input(None, str(p))
    assert text == raw and d_text[:len(raw)].cpu().numpy().tobytes() == raw
    assert stats["blocks"] == stats["device_blocks"] == -(-len(raw) // 700) + 1 and stats["host_blocks"] == 0
