"""SAM lines written on the device (hsa_sam_lines_device64, hsa_amd.sam.device_sam):

* fabricated arrays against the per-read restatement hsa_amd.sam.sam_line: the text, the
  offsets, the statuses and every counter; the statuses' causes; short out_cap and guard
  bytes; empty batches; two chained sub-range calls;
* search -> choose -> refine -> device_sam on the tiny index against the compiled
  reference's committed SAM, whole lines in file order;
* past 2^32, where no reference exists: the device text equals the restatement's."""
import gzip
import os

import numpy as np
import pytest

import choose_ref as cr
from golden_io import GOLD, parse_opts
from test_gpu_choose import choose, chrom_names, expect, fastq_quals, reference_lines  # noqa: F401
from test_gpu_refine import (BIG_T, MAN, U64, big_text64, dev, fastq_codes, index_text, refine,  # noqa: F401
                             search_rows, searched)

pytestmark = pytest.mark.gpu

ONES = 0xFFFFFFFFFFFFFFFF
CS, MS = 6, 24                       # cigar_stride, md_stride of the fabricated batches
MAX_TOP2 = 30
LENS = [1, 15, 16, 17, 36, 100, 250, 1023]
# 9, 10, 99, 100, 2^32 - 1, 2^32, 10^19, 2^64 - 1 and both ends of every digit count up to 20
VALUES = [9, 10, 99, 100, 2 ** 32 - 1, 2 ** 32, 10 ** 19, 2 ** 64 - 1] + \
         [v for k in range(1, 20) for v in (10 ** k - 1, 10 ** k)]
CHRS = ["c", "chr2", "a_rather_long_chromosome_name.1"]
NAME_CHARS = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_.:/#-", np.uint8)
MD_CHARS = np.frombuffer(b"0123456789ACGT^", np.uint8)


@pytest.fixture(scope="module")
def tiny():
    return index_text("tiny")


def fabricate(n, seed, nohit=()):
    """The host arrays of a batch of n reads made by hand (no search): every read has a hit
    except those in `nohit`; a read's records are its rows' (one record per row)."""
    from hsa_amd._lib import ALN64_WORDS, JOB_DTYPE, RF_ROW_WORDS
    rng = np.random.default_rng(seed)
    lens = np.array([LENS[j % len(LENS)] if j % 5 else LENS[int(rng.integers(len(LENS)))] for j in range(n)], np.uint32)
    lens[rng.permutation(n)[:n // 3]] = 36                              # (mostly short: the restatement is per base)
    jobs = np.zeros(n, JOB_DTYPE)
    jobs["off"] = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]) if n else []
    jobs["len"] = lens
    jobs["max_diff"] = 4
    codes = rng.integers(0, 5, int(lens.sum()) if n else 0).astype(np.uint8)
    hit = np.array([j not in nohit for j in range(n)], bool)
    n_xa = np.where(hit, np.array([(0, 1, 3, 0)[j % 4] for j in range(n)]), 0).astype(np.int64)
    n_rows = np.where(hit, 1 + n_xa, 0)
    pos_off = np.concatenate([[0], np.cumsum(n_rows)]).astype(U64)
    R = int(pos_off[-1])
    hits = np.zeros((max(R, 1), ALN64_WORDS), np.uint32)
    gapped = rng.integers(0, 2, max(R, 1)).astype(bool)
    n_gapo = np.where(gapped, rng.integers(1, 4, max(R, 1)), 0)
    n_gape = np.where(gapped, rng.integers(0, 200, max(R, 1)), 0)
    n_mm = rng.choice([0, 1, 9, 10, 99, 100, 65535], max(R, 1))
    hits[:, 0] = n_mm | (n_gapo << 16) | (n_gape << 24)
    hits[:, 1] = rng.integers(0, 2, max(R, 1)).astype(np.uint32) << 30
    pos = np.zeros((max(R, 1), 4), U64)
    pos[:, 1] = rng.integers(0, len(CHRS), max(R, 1))
    rows = np.zeros((max(R, 1), RF_ROW_WORDS), np.uint32)
    rpos = np.zeros((max(R, 1), 2), U64)
    cigar = np.full((max(R, 1), CS), 0x77777777, np.uint32)
    md = np.full((max(R, 1), MS), 0x77, np.uint8)
    for t in range(R):
        nc = (1, CS, int(rng.integers(1, CS + 1)))[t % 3]
        rows[t, 1] = nc
        ops = rng.choice([0, 1, 2, 4], nc) if nc > 1 else np.zeros(1, np.int64)
        cigar[t, :nc] = (ops.astype(np.uint32) << 28) | rng.choice([1, 9, 10, 100, 4095, (1 << 28) - 1], nc).astype(np.uint32)
        rows[t, 2] = rng.choice([0, 1, 10, 255, 2 ** 32 - 1])
        ml = (1, MS, int(rng.integers(1, MS + 1)))[(t // 3) % 3]
        rows[t, 3] = ml
        md[t, :ml] = rng.choice(MD_CHARS, ml)
        rpos[t] = (VALUES[(t * 7) % len(VALUES)], VALUES[t % len(VALUES)])
    pos_hit = np.zeros(max(R, 1), np.uint32)
    for j in np.flatnonzero(hit):
        r0 = int(pos_off[j])
        pos_hit[r0:r0 + int(n_rows[j])] = rng.permutation(int(n_rows[j]))        # (any record of the read's list)
    sel = np.zeros((max(n, 1), 4), np.uint32)
    sel64 = np.zeros((max(n, 1), 4), U64)
    c1s = VALUES + [MAX_TOP2, MAX_TOP2 + 1, 1, 2]
    for j in range(n):
        c1 = c1s[j % len(c1s)]
        sel[j] = (0, 0, 0, 0) if not hit[j] else (2 if c1 > 1 else 1, int(pos_hit[int(pos_off[j])]),
                                                   (0, 23, 25, 37, 255)[j % 5], n_xa[j])
        sel64[j] = (j, c1, VALUES[(j * 3 + 1) % len(VALUES)] if j % 6 else 0, 0)
    name_len = np.array([(1, 255, 7, 20)[j % 4] if j % 9 == 0 else int(rng.integers(1, 24)) for j in range(n)], np.int64)
    names = [rng.choice(NAME_CHARS, int(k)).tobytes().decode() for k in name_len]
    quals = [(rng.integers(33, 127, int(k)).astype(np.uint8)).tobytes().decode() for k in lens]
    return dict(n=n, jobs=jobs, lens=lens, codes=codes, n_aln=n_rows.astype(np.int32), hit_off=pos_off[:-1].copy(),
                hits=hits, sel=sel, sel64=sel64, pos_off=pos_off, pos=pos, pos_hit=pos_hit, rows=rows, rpos=rpos,
                cigar=cigar, md=md, names=names, quals=quals, pos_cap=R)


def strings(h):
    """The names' and qualities' bytes and offsets of a fabricated batch (made once: the
    status tests bend the offsets)."""
    from hsa_amd.sam import pack_strings
    if "name_b" not in h:
        h["name_b"], h["name_off"] = pack_strings(h["names"])
        h["qual_b"], h["qual_off"] = pack_strings(h["quals"])
    return h


def upload(h):
    import torch
    from hsa_amd._lib import pad_codes
    from hsa_amd.sam import pack_strings
    strings(h)
    cb, coff = pack_strings(CHRS)
    one = lambda a: a if len(a) else np.zeros(1, a.dtype)
    d = {k: dev(one(h[k])) for k in ("n_aln", "hit_off", "hits", "sel", "sel64", "pos_off", "pos", "pos_hit", "rows", "rpos",
                                     "cigar", "md", "name_off", "qual_off")}
    d.update(jobs=dev(one(h["jobs"].view(np.uint8))), codes=dev(pad_codes(h["codes"])), name_b=dev(one(h["name_b"])),
             qual_b=dev(one(h["qual_b"])), chr_b=dev(cb), chr_off=dev(coff))
    torch.cuda.synchronize()
    return d


def run(gi, h, d, quals=True, comp_read=1, flag=0, out_cap=None, tail=0, first=0, n=None, pos_cap=None, max_line=None,
        n_chr=len(CHRS)):
    """One hsa_sam_lines_device64 call over reads [first, first + n) of an uploaded batch:
    the outputs as NumPy arrays.  The output buffer holds out_cap + tail bytes and a 64-byte
    guard, all filled with 0xA5.  A sub-range is served as the header says: the per-read
    pointers offset, the row arrays from the sub-range's first row, its own pos_off."""
    import torch
    from hsa_amd import sam
    from hsa_amd._lib import ALN64_WORDS, JOB_DTYPE, RF_ROW_WORDS, SamBatch64
    n = h["n"] - first if n is None else n
    r0 = int(h["pos_off"][first])
    pos_off = dev(h["pos_off"][first:first + n + 1] - h["pos_off"][first])
    cap = (int(h["pos_cap"]) - r0) if pos_cap is None else pos_cap
    if max_line is None:
        max_line = sam.line_bound(255, int(h["lens"].max()) if h["n"] else 0, max(len(c) for c in CHRS), CS, MS, 3)
    if out_cap is None:
        out_cap = int(h["n"]) * max_line
    buf = torch.full((out_cap + tail + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    o = dict(line_off=torch.full((n + 1,), 0x77, dtype=torch.int64, device="cuda"),
             stat=torch.full((max(n, 1),), 0x77, dtype=torch.int32, device="cuda"),
             ctr=torch.full((8,), 0x33, dtype=torch.int64, device="cuda"))
    at = lambda k, i, size: d[k].data_ptr() + i * size
    b = SamBatch64(d_jobs=at("jobs", first, JOB_DTYPE.itemsize), n_jobs=n, d_codes=d["codes"].data_ptr(),
                   d_n_aln=at("n_aln", first, 4), d_hit_off=at("hit_off", first, 8), d_hits=d["hits"].data_ptr(),
                   d_sel=at("sel", first, 16), d_sel64=at("sel64", first, 32), d_pos_off=pos_off.data_ptr(),
                   d_pos=at("pos", r0, 32), d_pos_hit=at("pos_hit", r0, 4), pos_cap=cap, d_pos_counters=None,
                   d_rows=at("rows", r0, 4 * RF_ROW_WORDS), d_rpos=at("rpos", r0, 16), d_cigar=at("cigar", r0, 4 * CS),
                   d_md=at("md", r0, MS), cigar_stride=CS, md_stride=MS, d_names=d["name_b"].data_ptr(),
                   d_name_off=at("name_off", first, 8), d_quals=d["qual_b"].data_ptr() if quals else None,
                   d_qual_off=at("qual_off", first, 8) if quals else None, d_chr_names=d["chr_b"].data_ptr(),
                   d_chr_off=d["chr_off"].data_ptr(), n_chr=n_chr, flag=flag, max_top2=MAX_TOP2, comp_read=comp_read,
                   max_line=max_line, d_line_off=o["line_off"].data_ptr(), d_out=buf.data_ptr(), out_cap=out_cap,
                   d_line_stat=o["stat"].data_ptr(), d_counters=o["ctr"].data_ptr())
    assert ALN64_WORDS == 14
    torch.cuda.synchronize()
    gi.sam_lines64(b)
    torch.cuda.synchronize()
    return dict(buf=buf.cpu().numpy(), line_off=o["line_off"].cpu().numpy().view(U64),
                stat=o["stat"].cpu().numpy().view(np.uint32)[:n], ctr=o["ctr"].cpu().numpy().view(U64), out_cap=out_cap)


def restate(h, j, quals=True, comp_read=1, flag=0):
    """sam_line for read j of a fabricated batch, with its newline."""
    from hsa_amd import sam
    strings(h)
    r0, r1 = int(h["pos_off"][j]), int(h["pos_off"][j + 1])
    o = int(h["jobs"]["off"][j])
    name = h["name_b"][int(h["name_off"][j]):int(h["name_off"][j + 1])].tobytes().decode()
    qual = h["qual_b"][int(h["qual_off"][j]):int(h["qual_off"][j + 1])].tobytes().decode() if quals else None
    recs = h["hits"][int(h["hit_off"][j]) + h["pos_hit"][r0:r1].astype(np.int64)]
    return sam.sam_line(name, h["codes"][o:o + int(h["lens"][j])], qual, CHRS, h["sel"][j], h["sel64"][j], h["rows"][r0:r1],
                        h["rpos"][r0:r1], h["cigar"][r0:r1], h["md"][r0:r1], h["pos"][r0:r1], recs, max_top2=MAX_TOP2,
                        flag=flag, comp_read=bool(comp_read)) + "\n"


def expected(h, stat, first=0, **kw):
    """(text, line_off, counters) for the statuses given: the restatement over the
    status-0 reads."""
    lines = [restate(h, first + j, **kw).encode() if s == 0 else b"" for j, s in enumerate(stat)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(U64)
    text = b"".join(lines)
    bad = [j for j, s in enumerate(stat) if s >= 2]
    ctr = [len(text), len(text), sum(1 for s in stat if s == 0)] + [sum(1 for s in stat if s == k) for k in (1, 2, 3, 4)] + \
        [bad[0] if bad else ONES]
    return text, off, ctr


_WANT = {}


def expected_once(key, h, stat, **kw):
    """expected() of a module-wide batch, computed once per variant."""
    if key not in _WANT:
        _WANT[key] = expected(h, stat, **kw)
    return _WANT[key]


def assert_call(got, text, off, ctr, stat):
    assert [int(c) for c in got["ctr"]] == ctr
    assert np.array_equal(got["stat"], np.asarray(stat, np.uint32))
    assert np.array_equal(got["line_off"], off)
    out = got["buf"][:len(text)].tobytes()
    if out != text:
        k = next(i for i in range(len(text)) if out[i] != text[i])
        j = int(np.searchsorted(off, k, side="right")) - 1
        raise AssertionError(f"first difference at byte {k}, read {j}:\n{text[int(off[j]):int(off[j + 1])]!r}\n"
                             f"{out[int(off[j]):int(off[j + 1])]!r}")
    assert (got["buf"][len(text):] == 0xA5).all()


@pytest.fixture(scope="module")
def batch(tiny):
    h = fabricate(5003, 23, nohit=set(range(13, 5003, 61)))
    return h, upload(h)


def test_fabricated_batch_covers_the_cases(batch):
    h, _ = batch
    hit = h["sel"][:h["n"], 0] != 0
    strand = (h["hits"][:, 1] >> 30)[h["pos_off"][:-1][hit].astype(np.int64)]
    assert set(np.unique(h["lens"])) == set(LENS) and set(np.unique(h["codes"])) == {0, 1, 2, 3, 4}
    assert {1, 255} <= {len(x) for x in h["names"]} and set(np.unique(strand)) == {0, 1}
    assert set(VALUES) | {MAX_TOP2, MAX_TOP2 + 1} <= {int(v) for v in h["sel64"][:, 1]}
    assert set(VALUES) <= {int(v) for v in h["sel64"][:, 2]} and set(VALUES) <= {int(v) for v in h["rpos"][:, 1]}
    assert {len(str(v)) for v in VALUES} == set(range(1, 21))
    assert set(np.unique(h["sel"][:h["n"], 3][hit])) == {0, 1, 3}
    assert {1, CS} <= set(np.unique(h["rows"][:, 1])) and {1, MS} <= set(np.unique(h["rows"][:, 3]))
    assert {0, 1, 2, 4} <= set(np.unique(h["cigar"][h["rows"][:, 1] == CS] >> 28))
    mixed = 0                                                           # gapped and ungapped XA entries in one list
    for j in np.flatnonzero(h["sel"][:h["n"], 3] == 3):
        r0 = int(h["pos_off"][j])
        w0 = h["hits"][int(h["hit_off"][j]) + h["pos_hit"][r0 + 1:r0 + 4].astype(np.int64), 0]
        mixed += len({bool(w >> 16) for w in w0}) == 2
    assert mixed > 100


@pytest.mark.parametrize("quals,comp_read,flag", [(True, 1, 0), (False, 0, 0x200)])
def test_fabricated_batch_equals_the_restatement(tiny, batch, quals, comp_read, flag):
    h, d = batch
    stat = [0 if t else 1 for t in h["sel"][:h["n"], 0]]
    text, off, ctr = expected_once((quals, comp_read, flag), h, stat, quals=quals, comp_read=comp_read, flag=flag)
    got = run(tiny, h, d, quals=quals, comp_read=comp_read, flag=flag)
    assert_call(got, text, off, ctr, stat)
    assert ctr[2] > 4900 and ctr[3] == len(range(13, 5003, 61)) and len(text) > 5003 * 100
    if quals:
        again = run(tiny, h, d, quals=quals, comp_read=comp_read, flag=flag)     # two runs give equal arrays
        for k in ("buf", "line_off", "stat", "ctr"):
            assert np.array_equal(got[k], again[k]), k


def test_device_sam_on_the_fabricated_batch(tiny, batch):
    """The Python driver: it uploads the strings, sizes the room (and runs again where the
    first run reports too little) and returns the same text."""
    from hsa_amd import sam
    h, d = batch
    m = dict(d, n_jobs=h["n"], pos_cap=h["pos_cap"], cigar_stride=CS, md_stride=MS)
    text, off, stat, ctr = sam.device_sam(tiny, m, h["names"], h["quals"], CHRS, max_top2=MAX_TOP2)
    want_stat = [0 if t else 1 for t in h["sel"][:h["n"], 0]]
    want, want_off, want_ctr = expected_once((True, 1, 0), h, want_stat, quals=True, comp_read=1, flag=0)
    assert text == want and np.array_equal(off, want_off) and [int(c) for c in ctr] == want_ctr
    assert np.array_equal(stat, np.asarray(want_stat, np.uint32))


# ---------------------------------------------------------------- statuses
def test_statuses(tiny):
    """Every cause of a refused read, each among printable reads."""
    from hsa_amd._lib import HSA_RF_MD, HSA_RF_POS
    n = 299
    h = strings(fabricate(n, 5, nohit={7, 150}))
    want = {7: 1, 150: 1}
    row0 = lambda j: int(h["pos_off"][j])
    xa = [j for j in range(n) if h["sel"][j, 3] == 3]                   # reads with XA rows
    h["rows"][row0(20), 0] = HSA_RF_MD; want[20] = 3                    # the chosen row did not fit its stride
    h["rows"][row0(20), 1] = CS + 9                                     # (HSA_RF_MD leaves the needed length: still status 3)
    h["rows"][row0(31), 0] = HSA_RF_POS; want[31] = 3
    h["rows"][row0(xa[5]) + 2, 0] = HSA_RF_MD; want[xa[5]] = 3          # an XA row
    h["pos"][row0(40), 1] = len(CHRS); want[40] = 4                     # chrID >= n_chr
    h["pos"][row0(xa[8]) + 3, 1] = ONES; want[xa[8]] = 4                #   in an XA row
    h["pos_hit"][row0(50)] = h["n_aln"][50]; want[50] = 4               # d_pos_hit >= n_aln
    h["cigar"][row0(60), 0] = (9 << 28) | 5; want[60] = 4               # op code > 8
    h["rows"][row0(70), 1] = CS + 1; want[70] = 4                       # n_cigar > cigar_stride
    h["rows"][row0(80), 3] = MS + 1; want[80] = 4                       # md_len > md_stride
    h["codes"][int(h["jobs"]["off"][90]) + int(h["lens"][90]) - 1] = 5; want[90] = 4      # a base code > 4
    h["name_off"][101] = h["name_off"][100] - U64(1); want[100] = 4     # a decreasing name offset (101 prints a longer name)
    h["qual_off"][111] = h["qual_off"][110] - U64(1); want[110] = 4     # a decreasing quality offset, and
    want[111] = 4                                                       #   its neighbour's length is one too many
    h["qual_off"][121:] += U64(1); want[120] = 4                        # quality length != read length (one byte more)
    h["qual_b"] = np.concatenate([h["qual_b"], np.full(1, 0x21, np.uint8)])
    h["sel"][130, 0] = 3; want[130] = 4                                 # no such type
    last = n - 1
    assert h["sel"][last, 3] == 3 and last not in want
    want[last] = 2                                                      # its last XA row lies past pos_cap
    stat = [want.get(j, 0) for j in range(n)]
    assert h["sel"][19, 0] and h["sel"][21, 0] and h["sel"][101, 0] and len(set(want.values())) == 4
    text, off, ctr = expected(h, stat)
    got = run(tiny, h, upload(h), pos_cap=h["pos_cap"] - 1)
    assert_call(got, text, off, ctr, stat)
    assert ctr[3:] == [2, 1, 3, 12, 20]
    for j in want:
        assert off[j + 1] == off[j]


def test_a_line_longer_than_max_line_is_refused(tiny):
    h = fabricate(64, 9)
    stat0 = [0] * 64
    full, off, _ = expected(h, stat0)
    longest = int(np.diff(off.astype(np.int64)).max())
    stat = [4 if int(off[j + 1] - off[j]) > longest - 1 else 0 for j in range(64)]
    text, off2, ctr = expected(h, stat)
    got = run(tiny, h, upload(h), max_line=longest - 1)
    assert_call(got, text, off2, ctr, stat)
    assert 1 <= ctr[6] < 64
    assert_call(run(tiny, h, upload(h), max_line=longest), full, off, expected(h, stat0)[2], stat0)


# ---------------------------------------------------------------- room
@pytest.fixture(scope="module")
def small(tiny):
    h = fabricate(400, 3, nohit={5, 399})
    stat = [0 if t else 1 for t in h["sel"][:400, 0]]
    return h, upload(h), stat, expected(h, stat)


@pytest.mark.parametrize("cut", ["zero", "one_less", "mid_tile", "mid_first_unit"])
def test_short_out_cap_and_guard_bytes(tiny, small, cut):
    h, d, stat, (text, off, ctr) = small
    cap = dict(zero=0, one_less=len(text) - 1, mid_tile=int(off[203]) + 41, mid_first_unit=7)[cut]
    got = run(tiny, h, d, out_cap=cap, tail=333)
    assert [int(c) for c in got["ctr"]] == [len(text), cap] + ctr[2:]
    assert np.array_equal(got["line_off"], off) and np.array_equal(got["stat"], np.asarray(stat, np.uint32))
    assert got["buf"][:cap].tobytes() == text[:cap]
    assert len(got["buf"]) == cap + 333 + 64 and (got["buf"][cap:] == 0xA5).all()


def test_unaligned_output_pointer(tiny, small):
    """The 16-byte stores follow the output's address, not its offset: d_out + 5."""
    import torch
    from hsa_amd._lib import SamBatch64
    h, d, stat, (text, off, ctr) = small
    got = run(tiny, h, d, out_cap=len(text) + 5)                        # (the arrays of an aligned call, for the struct below)
    assert got["buf"][:len(text)].tobytes() == text
    buf = torch.full((len(text) + 5 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    lo = torch.zeros(401, dtype=torch.int64, device="cuda")
    st = torch.zeros(400, dtype=torch.int32, device="cuda")
    c = torch.zeros(8, dtype=torch.int64, device="cuda")
    po = dev(h["pos_off"])
    b = SamBatch64(d_jobs=d["jobs"].data_ptr(), n_jobs=400, d_codes=d["codes"].data_ptr(), d_n_aln=d["n_aln"].data_ptr(),
                   d_hit_off=d["hit_off"].data_ptr(), d_hits=d["hits"].data_ptr(), d_sel=d["sel"].data_ptr(),
                   d_sel64=d["sel64"].data_ptr(), d_pos_off=po.data_ptr(), d_pos=d["pos"].data_ptr(),
                   d_pos_hit=d["pos_hit"].data_ptr(), pos_cap=h["pos_cap"], d_rows=d["rows"].data_ptr(),
                   d_rpos=d["rpos"].data_ptr(), d_cigar=d["cigar"].data_ptr(), d_md=d["md"].data_ptr(), cigar_stride=CS,
                   md_stride=MS, d_names=d["name_b"].data_ptr(), d_name_off=d["name_off"].data_ptr(),
                   d_quals=d["qual_b"].data_ptr(), d_qual_off=d["qual_off"].data_ptr(), d_chr_names=d["chr_b"].data_ptr(),
                   d_chr_off=d["chr_off"].data_ptr(), n_chr=len(CHRS), flag=0, max_top2=MAX_TOP2, comp_read=1,
                   max_line=4000, d_line_off=lo.data_ptr(), d_out=buf.data_ptr() + 5, out_cap=len(text),
                   d_line_stat=st.data_ptr(), d_counters=c.data_ptr())
    torch.cuda.synchronize()
    tiny.sam_lines64(b)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert out[5:5 + len(text)].tobytes() == text and (out[:5] == 0xA5).all() and (out[5 + len(text):] == 0xA5).all()


# ---------------------------------------------------------------- empty and tiny batches
@pytest.mark.parametrize("n,nohit", [(0, ()), (1, ()), (1, (0,)), (70, tuple(range(70)))])
def test_empty_and_tiny_batches(tiny, n, nohit):
    h = fabricate(n, 2, nohit=set(nohit))
    stat = [1 if j in nohit else 0 for j in range(n)]
    text, off, ctr = expected(h, stat)
    got = run(tiny, h, upload(h), out_cap=5000)
    assert_call(got, text, off, ctr, stat)
    if len(nohit) == n:
        assert not got["line_off"].any() and len(got["line_off"]) == n + 1 and int(got["ctr"][0]) == 0


def test_bad_arguments(tiny):
    from hsa_amd._lib import HSA_SAM_MAX_LINE, GpuIndex, HsaError, SamBatch64
    from hsa_amd import index_io
    from golden_io import INDEX
    h = fabricate(10, 1)
    d = upload(h)
    with pytest.raises(HsaError, match="-2"):                        # null outputs
        tiny.sam_lines64(SamBatch64(n_jobs=3))
    with pytest.raises(HsaError, match="-2"):
        run(tiny, h, d, max_line=HSA_SAM_MAX_LINE + 1)
    with pytest.raises(HsaError, match="-2"):
        run(tiny, h, d, max_line=0)
    narrow = GpuIndex(*index_io.read_index(INDEX["tiny"]))           # not a 64-bit index
    with pytest.raises(HsaError, match="-2"):
        run(narrow, h, d)
    narrow.close()


# ---------------------------------------------------------------- sub-ranges
def test_two_chained_sub_range_calls_equal_one(tiny, small):
    h, d, stat, (text, off, ctr) = small
    s = 203
    a = run(tiny, h, d, first=0, n=s)
    b = run(tiny, h, d, first=s)
    na, nb = int(a["ctr"][0]), int(b["ctr"][0])
    assert a["buf"][:na].tobytes() + b["buf"][:nb].tobytes() == text
    assert np.array_equal(np.concatenate([a["line_off"], b["line_off"][1:] + a["line_off"][-1]]), off)
    assert np.array_equal(np.concatenate([a["stat"], b["stat"]]), np.asarray(stat, np.uint32))
    assert [int(x) + int(y) for x, y in zip(a["ctr"][:7], b["ctr"][:7])] == ctr[:7]


# ---------------------------------------------------------------- the reference's SAM, whole file order
def device_text(gi, index, names, seqs, quals, args):
    """search -> choose -> refine -> device_sam for every read the reference searches, driven
    as test_gpu_choose.device_lines drives it: two parts around the reference's option
    switch, chained.  Returns the text and the names of the reads with a line, in read
    order."""
    from hsa_amd import sam
    from oracle_ctypes import default_opt
    base = parse_opts(args, default_opt())
    keep = searched(seqs, base)
    lens = np.array([len(seqs[r]) for r in keep], np.uint32)
    codes = np.concatenate([seqs[r] for r in keep])
    od_a = dict(base)
    od_a["mode"] &= ~0x01
    t, host = search_rows(gi, lens, codes, od_a, 1)
    fb = np.flatnonzero(host["flags"] & 1)
    switch = int(fb[0]) if len(fb) else len(lens)
    parts = [(t, 0, min(switch + 1, len(lens)))]
    if switch < len(lens) - 1:
        t2, _ = search_rows(gi, lens, codes, base, 1)
        parts.append((t2, switch + 1, len(lens) - switch - 1))
    chrs = chrom_names(index)
    state, text, order = cr.SEED0, b"", []
    for t, first, n in parts:
        got, sub = choose(gi, t, state=state, first=first, n=n)
        assert int(got["ctr"][0]) == int(got["ctr"][1]) and int(got["ctr"][6]) == 0
        state = got["rng"]
        out = refine(gi, sub, cigar_stride=16, md_stride=128)
        m = dict(sub, sel=dev(got["sel"]), sel64=dev(got["sel64"]), rows=dev(out["rows"]), rpos=dev(out["rpos"]),
                 cigar=dev(out["cigar"]), md=dev(out["md"]), cigar_stride=16, md_stride=128)
        part, off, stat, ctr = sam.device_sam(gi, m, [names[keep[first + j]] for j in range(n)],
                                              [quals[keep[first + j]] for j in range(n)], chrs, max_top2=base["max_top2"])
        assert int(ctr[0]) == int(ctr[1]) == len(part) == int(off[-1])
        assert [int(c) for c in ctr[4:7]] == [0, 0, 0] and int(ctr[7]) == ONES
        assert np.array_equal(stat == 0, got["sel"][:, 0] != 0)
        text += part
        order += [names[keep[first + j]] for j in range(n) if stat[j] == 0]
    return text, order


@pytest.mark.parametrize("name,count", [("default", 890), ("n4o0", 526)])
def test_golden_sam_whole_file_order(name, count):
    gi = index_text("tiny")
    fq = os.path.join(GOLD, MAN["reads"])
    names, seqs = fastq_codes(fq)
    raw = gzip.open(os.path.join(GOLD, f"dropin_ref_{name}.sam.gz")).read()
    want = reference_lines(raw)
    assert len(want) == count
    text, order = device_text(gi, "tiny", names, seqs, fastq_quals(fq), MAN[name]["args"])
    assert text.endswith(b"\n")
    lines = text.decode().split("\n")[:-1]
    assert [ln.split("\t")[0] for ln in lines] == order                  # one line per read with a hit, in read order
    at = {nm: k for k, nm in enumerate(names)}
    assert all(at[a] < at[b] for a, b in zip(order, order[1:]))
    have = set(lines)
    bad = [ln for ln in want if ln not in have]
    assert not bad, f"{len(bad)} of {len(want)} reference lines are not in the device text, first:\n{bad[0]}"
    # and in the reference's own order: its U / R lines are a subsequence of the device text
    pos = {ln: k for k, ln in enumerate(lines)}
    where = [pos[ln] for ln in want]
    assert where == sorted(where)


# ---------------------------------------------------------------- past 2^32
def test_sam_text_past_2_32(big_text64):
    from hsa_amd import sam, synth
    from oracle_ctypes import default_opt
    gi, genome = big_text64
    n = 2000
    reads, _ = synth.make_reads(genome, [(0, BIG_T)], n, 100, 47, indel=True, max_mm_indel=2)
    od = default_opt()
    od.update(max_diff=4, fnr=-1.0, max_gapo=1)
    od["mode"] &= ~0x01
    t, host = search_rows(gi, np.full(n, 100, np.uint32), reads.reshape(-1), od, 1)
    got, sub = choose(gi, t)
    out = refine(gi, sub)
    rng = np.random.default_rng(4)
    names = [f"r{j}/{j % 7}" for j in range(n)]
    quals = [rng.integers(33, 127, 100).astype(np.uint8).tobytes().decode() for _ in range(n)]
    chrs = ["none", "big64"]                                            # (the fixture's one block has chrID 1)
    m = dict(sub, sel=dev(got["sel"]), sel64=dev(got["sel64"]), rows=dev(out["rows"]), rpos=dev(out["rpos"]),
             cigar=dev(out["cigar"]), md=dev(out["md"]), cigar_stride=out["cigar"].shape[1], md_stride=out["md"].shape[1])
    text, off, stat, ctr = sam.device_sam(gi, m, names, quals, chrs, max_top2=od["max_top2"])
    want, want_stat, past = [], [], 0
    for j in range(n):
        if int(got["sel"][j, 0]) == 0:
            want_stat.append(1)
            continue
        r0, r1 = int(got["pos_off"][j]), int(got["pos_off"][j + 1])
        if any(int(s) for s in out["rows"][r0:r1, 0]):
            want_stat.append(3)
            continue
        recs = host["hits"][int(host["hit_off"][j]) + got["pos_hit"][r0:r1].astype(np.int64)]
        want.append(sam.sam_line(names[j], reads[j], quals[j], chrs, got["sel"][j], got["sel64"][j], out["rows"][r0:r1],
                                 out["rpos"][r0:r1], out["cigar"][r0:r1], out["md"][r0:r1], got["pos"][r0:r1], recs,
                                 max_top2=od["max_top2"]) + "\n")
        want_stat.append(0)
        past += int(out["rpos"][r0, 1]) >= (1 << 32)
    assert np.array_equal(stat, np.asarray(want_stat, np.uint32))
    assert text == "".join(want).encode()
    assert len(want) >= 1500 and past > 0, "no printed position past 2^32"
    assert int(ctr[0]) == int(ctr[1]) == len(text) and int(ctr[2]) == len(want)
