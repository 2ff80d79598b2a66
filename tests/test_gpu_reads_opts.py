"""The reader's options on the device (hsa_reads_device_opts, hsa_amd.reads.load_device with
mode / trim_qual) against the host restatement hsa_amd.reads.parse_host, which
tests/test_reads_opts_cpu.py holds against the reference: quality trimming over every chunk
boundary of the backward walk and the 35-base floor, barcodes, the Casava filter, Illumina-1.3
qualities; jobs, codes, names, qualities, full lengths, barcodes, offsets, rows and every
counter, exact capacities with guard bytes, unaligned inputs, two runs."""
import numpy as np
import pytest

from reads_opts_cases import CASES, MODE_CFY, MODE_IL13, case_options, case_reads

pytestmark = pytest.mark.gpu

ONES = 0xFFFFFFFFFFFFFFFF
GUARD = 64
FILTERED = 3
TRIM_LENS = (35, 36, 37, 63, 64, 65, 99, 100, 127, 128, 129, 192, 193, 300)


@pytest.fixture(scope="module")
def gi():
    from test_gpu_refine import index_text
    return index_text("tiny")


def record(name, seq, qual):
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def expected(recs, mode=0, trim_qual=0, max_diff=4, table=None, seed_len=32, max_records=1 << 20, rec_cap=None, at_eof=1):
    """What the call must leave for the canonical records `recs` (each one's bytes), from
    parse_host record by record: the rows in input order, the arrays of the searched reads."""
    from hsa_amd import reads
    from hsa_amd._lib import JOB_DTYPE
    filt = bool(mode & MODE_CFY or mode >> 24)
    cap = (rec_cap or max_records) if filt else max_records
    rows, kept = [], []
    for rb in recs:
        if len(rows) >= cap or len(kept) >= max_records:
            break
        p = reads.parse_host(rb, mode=mode, trim_qual=trim_qual)
        assert len(p["names"]) + p["filtered"] == 1
        rows.append(None if p["filtered"] else len(kept))
        if not p["filtered"]:
            kept.append((p["names"][0], p["seqs"][0], p["quals"][0], p["lens"][0], p["bcs"][0]))
    consumed = sum(len(rb) for rb in recs[:len(rows)])
    data = b"".join(recs)
    whole = reads.parse_host(data[:consumed], mode=mode, trim_qual=trim_qual)        # ... and in one piece
    assert whole["names"] == [k[0] for k in kept] and whole["lens"] == [k[3] for k in kept] and whole["filtered"] == rows.count(None)
    if len(rows) < len(recs) and len(kept) == max_records:
        assert reads.parse_host(data, max_records, mode=mode, trim_qual=trim_qual)["consumed"] == consumed
    lens = [k[3] for k in kept]
    thr = int(table[max(lens + [0])]) if table is not None else max_diff
    rec = np.zeros((len(rows), 4), np.uint32)
    jobs, codes, names, quals, full, bcs = [], [], [], [], [], []
    for r, i in enumerate(rows):
        if i is None:
            rec[r] = (FILTERED, 0, 0, 0xFFFFFFFF)
            continue
        nm, sq, ql, ln, bc = kept[i]
        nn = int((sq[:ln] > 3).sum())
        st = 1 if nn > thr else 2 if ln >= 15 and ((sq[:15] == 0).all() or (sq[:15] == 3).all()) else 0
        rec[r] = (st, ln, nn, len(jobs) if st == 0 else 0xFFFFFFFF)
        if st == 0:
            jobs.append((sum(len(c) for c in codes), ln, int(table[ln]) if table is not None else max_diff,
                         seed_len if seed_len < ln else 0x7FFFFFFF, 0))
            codes.append(sq), names.append(nm), quals.append(ql), full.append(len(sq)), bcs.append(bc)
    cb = np.concatenate(codes + [np.zeros(16, np.uint8)])
    nb, qb = b"".join(names), b"".join(quals)
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)
    total = sum(len(k[1]) for k in kept)
    ctr = [len(rows), len(kept), len(jobs), len(jobs), len(cb), len(cb), len(nb), len(nb), len(qb), len(qb), consumed, ONES, ONES,
           max(lens, default=0), max((j[1] for j in jobs), default=0), thr & ONES]
    return dict(rec=rec, jobs=np.array(jobs, JOB_DTYPE) if jobs else np.zeros(0, JOB_DTYPE), codes=cb,
                names=np.frombuffer(nb, np.uint8), quals=np.frombuffer(qb, np.uint8), name_off=off(names), qual_off=off(quals),
                full_len=np.array(full, np.uint32), bc=np.frombuffer(b"".join(bcs), np.uint8), ctr=ctr,
                octr=[len(rows), rows.count(None), total - sum(lens), total], rows=len(rows), consumed=consumed, data=data)


def run(gi, w, mode=0, trim_qual=0, max_diff=4, table=None, seed_len=32, max_records=None, rec_cap=0, shift=0, caps=None,
        at_eof=1, data=None):
    """One hsa_reads_device_opts call on w's bytes placed `shift` bytes into a device buffer;
    every output holds exactly what `w` needs (or `caps`) and GUARD bytes of 0xA5 behind."""
    import torch
    from hsa_amd._lib import JOB_DTYPE, ReadsBatch
    data = w["data"] if data is None else data
    if max_records is None:
        max_records = max(len(data) // 8 + 1, 1)
    bcn = mode >> 24
    cap = dict(jobs=len(w["jobs"]), codes=len(w["codes"]), names=len(w["names"]), quals=len(w["quals"]))
    cap.update(caps or {})
    buf = np.full(shift + len(data) + 48, 0x0A, np.uint8)
    buf[shift:shift + len(data)] = np.frombuffer(data, np.uint8)
    d_in = torch.from_numpy(buf).cuda()
    JB = JOB_DTYPE.itemsize
    fill = lambda n: torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    n_rows = rec_cap or max_records
    o = dict(jobs=fill(cap["jobs"] * JB), codes=fill(cap["codes"]), names=fill(cap["names"]), quals=fill(cap["quals"]),
             name_off=fill((cap["jobs"] + 1) * 8), qual_off=fill((cap["jobs"] + 1) * 8), rec=fill(n_rows * 16),
             full_len=fill(cap["jobs"] * 4), bc=fill(cap["jobs"] * bcn), ctr=fill(16 * 8), octr=fill(4 * 8))
    d_tab = torch.from_numpy(np.ascontiguousarray(table, np.int32)).cuda() if table is not None else None
    b = ReadsBatch(d_in=d_in.data_ptr() + shift, n_in=len(data), at_eof=at_eof, max_records=max_records, max_diff=max_diff,
                   d_maxdiff=d_tab.data_ptr() if table is not None else None, n_maxdiff=len(table) if table is not None else 0,
                   seed_len=seed_len, trim_qual=trim_qual, mode=mode, d_jobs=o["jobs"].data_ptr(), job_cap=cap["jobs"],
                   d_codes=o["codes"].data_ptr(), code_cap=cap["codes"], d_names=o["names"].data_ptr(), name_cap=cap["names"],
                   d_name_off=o["name_off"].data_ptr(), d_quals=o["quals"].data_ptr(), qual_cap=cap["quals"],
                   d_qual_off=o["qual_off"].data_ptr(), d_rec=o["rec"].data_ptr(), d_counters=o["ctr"].data_ptr(),
                   d_full_len=o["full_len"].data_ptr(), d_bc=o["bc"].data_ptr(), rec_cap=rec_cap, d_opt_counters=o["octr"].data_ptr())
    torch.cuda.synchronize()
    gi.reads_device_opts(b)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["cap"], got["bcn"] = cap, bcn
    return got


def assert_equal(got, w):
    """Every output against the expectation, cut at the capacities; guards untouched."""
    from hsa_amd._lib import JOB_DTYPE
    cap, bcn = got["cap"], got["bcn"]
    JB = JOB_DTYPE.itemsize
    nj = min(len(w["jobs"]), cap["jobs"])
    ctr = list(w["ctr"])
    ctr[3] = nj
    for i, k in ((5, "codes"), (7, "names"), (9, "quals")):
        ctr[i] = min(ctr[i - 1], cap[k])
    assert [int(v) for v in got["ctr"][:128].view(np.uint64)] == ctr and (got["ctr"][128:] == 0xA5).all()
    assert [int(v) for v in got["octr"][:32].view(np.uint64)] == w["octr"] and (got["octr"][32:] == 0xA5).all()
    assert np.array_equal(got["jobs"][:nj * JB].view(JOB_DTYPE), w["jobs"][:nj])
    assert (got["jobs"][nj * JB:] == 0xA5).all()
    for k in ("codes", "names", "quals"):
        m = min(len(w[k]), cap[k])
        assert np.array_equal(got[k][:m], w[k][:m]), k
        assert (got[k][m:] == 0xA5).all(), k + " past its capacity or its end"
    assert np.array_equal(got["full_len"][:nj * 4].view(np.uint32), w["full_len"][:nj]) and (got["full_len"][nj * 4:] == 0xA5).all()
    assert np.array_equal(got["bc"][:nj * bcn], w["bc"][:nj * bcn]) and (got["bc"][nj * bcn:] == 0xA5).all()
    for k in ("name_off", "qual_off"):
        assert np.array_equal(got[k][:(nj + 1) * 8].view(np.uint64), w[k][:nj + 1]), k
        assert (got[k][(nj + 1) * 8:] == 0xA5).all(), k
    L = w["rows"]
    assert np.array_equal(got["rec"][:L * 16].view(np.uint32).reshape(-1, 4), w["rec"])
    assert (got["rec"][L * 16:] == 0xA5).all()


def check(gi, recs, shift=0, caps=None, **kw):
    w = expected(recs, **kw)
    got = run(gi, w, shift=shift, caps=caps, **{k: v for k, v in kw.items() if k != "at_eof"})
    assert_equal(got, w)
    return got, w


# ---------------------------------------------------------------- trimming
def ph(*runs):
    """Quality bytes, phred + 33, from (phred, count) runs given from the read's END backwards."""
    return b"".join(bytes([33 + v]) * n for v, n in runs)[::-1]


def trim_patterns(L, tq=20):
    """Qualities of length L by name; t: the steps bwa_trim_read may walk (l = L - 1 .. 35)."""
    t, n = L - 35, (L - 35) // 4
    pad = lambda tail: (b"I" * L + tail)[-L:]
    rng = np.random.default_rng(L)
    return dict(
        high=ph((40, L)), low=ph((2, L)), last_high=pad(ph((tq + 1, 1), (2, L - 1))),
        two_max=pad(ph((10, n), (30, n), (10, n))),                           # 10n, back to exactly 0, 10n again: the larger l
        max_at_35=pad(ph((10, t))), past_35=pad(ph((10, t + 1))),
        zero_goes_on=pad(ph((10, n), (30, n), (5, n))),                       # a prefix sum of exactly 0, then a strict maximum
        dip=pad(ph((10, n), (25, n), (10, n + 1))),
        ends=pad(ph((0, 5), (94, 1), (0, 5))),                                # bytes 33 and 127
        drift=pad(bytes(rng.integers(33 + 12, 33 + 30, L).astype(np.uint8))),  # around trim_qual: many sign changes
        noise=bytes(rng.integers(33, 128, L).astype(np.uint8)))


def trim_records(il13=False):
    rng = np.random.default_rng(5)
    recs = []
    for L in TRIM_LENS:
        for name, qual in sorted(trim_patterns(L).items()):
            if il13:
                if name == "noise":
                    continue
                qual = bytes(c if name == "ends" else c + 31 for c in qual)       # ("ends": the raw bytes 33 and 127, 2 and 96 after the shift)
            seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), L, p=[.249, .249, .249, .249, .004]).tobytes()
            recs.append(record(b"%s_%d extra:N" % (name.encode(), L), seq, qual))
    return recs


@pytest.mark.parametrize("shift", [0, 1, 15])
@pytest.mark.parametrize("il13", [False, True])
def test_trimming(gi, shift, il13):
    recs = trim_records(il13)
    got, w = check(gi, recs, shift=shift, trim_qual=20, mode=MODE_IL13 if il13 else 0)
    lens, full = w["jobs"]["len"], w["full_len"]
    assert (lens < full).sum() > 30 and (lens == 35).sum() > 10 and (lens == full).sum() > 10 and w["octr"][2] > 0
    assert len(set(TRIM_LENS) - set(full.tolist())) == 0
    if shift == 0 and not il13:
        again = run(gi, w, trim_qual=20)                        # two runs give equal arrays
        for k in ("jobs", "codes", "names", "quals", "name_off", "qual_off", "rec", "ctr", "octr", "full_len"):
            assert np.array_equal(got[k], again[k]), k


def test_trimmed_lengths_set_the_filter_and_the_options(gi):
    """The N count, the poly test, max_diff, seed_len and the threshold are of the trimmed read."""
    from hsa_amd import reads
    table = reads.maxdiff_table(0.04, 256)
    good, badq = b"I" * 40, b"#" * 60
    recs = [record(b"n_in_tail", b"ACGTTGCAGT" * 4 + b"N" * 60, good + badq),      # its Ns are trimmed away: searched
            record(b"n_in_head", b"N" * 6 + b"ACGTTGCAGT" * 9 + b"ACGT", good + badq),
            record(b"whole", b"ACGTTGCAGT" * 10, b"I" * 100),
            record(b"polya", b"A" * 15 + b"C" * 85, good + badq)]
    got, w = check(gi, recs, trim_qual=20, table=table, seed_len=38)
    assert w["rec"][:, 0].tolist() == [0, 1, 0, 2] and w["rec"][:, 1].tolist() == [40, 40, 100, 40]
    assert w["jobs"]["max_diff"].tolist() == [int(table[40]), int(table[100])] and w["jobs"]["seed_len"].tolist() == [38, 38]
    assert w["ctr"][13] == 100 and w["ctr"][15] == int(table[100])
    got, w = check(gi, recs[:2], trim_qual=20, table=table, seed_len=40)           # the longest TRIMMED read: 40
    assert w["ctr"][13] == 40 and w["ctr"][15] == int(table[40]) and w["jobs"]["seed_len"].tolist() == [0x7FFFFFFF]


# ---------------------------------------------------------------- barcodes
def barcode_records(bcn, il13=False):
    rng = np.random.default_rng(bcn)
    al = np.frombuffer(b"ACGTacgtNn", np.uint8)
    sh = 31 if il13 else 0
    recs = []
    for k, L in enumerate((bcn, bcn + 1, bcn + 36, bcn + 100, max(bcn - 1, 1), bcn + 15, bcn + 64)):
        seq = rng.choice(al, L).tobytes()
        q = rng.integers(33 + 2, 33 + 41, L).astype(np.uint8)
        q[:min(2, L)] = (33 + 12, 33 + 13)[:min(2, L)]                            # the two sides of BARCODE_LOW_QUAL
        q[L // 2:] = np.minimum(q[L // 2:], 33 + 12 + k)
        recs.append(record(b"b%d_%d/1" % (bcn, L), seq, bytes(c + sh for c in q)))
    return recs


@pytest.mark.parametrize("bcn", [1, 6, 63])
@pytest.mark.parametrize("il13", [False, True])
def test_barcodes(gi, bcn, il13):
    mode = (bcn << 24) | (MODE_IL13 if il13 else 0)
    recs = barcode_records(bcn, il13)
    got, w = check(gi, recs, mode=mode)
    assert w["rec"][:, 0].tolist()[:2] == [FILTERED, 0] and w["rec"][1, 1] == 1 and w["octr"][1] == 2
    bc0 = w["bc"][:bcn].tobytes()
    assert bc0[:1].islower() and (bcn < 2 or bc0[1:2].isupper())
    check(gi, recs, mode=mode, trim_qual=15, shift=3)
    check(gi, recs, mode=mode, trim_qual=15, caps=dict(jobs=len(w["jobs"]) - 1))       # no barcode, no full_len past job_cap


# ---------------------------------------------------------------- the Casava filter
COMMENTS = [(b" :Y", True), (b" 1:Y:0", True), (b" 1:N:0", False), (b" Y", False), (b" a:b:Y", False), (b" x:", False),
            (b"", False), (b"\t1:Y:0", True), (b" \0:Y", False), (b" a\0b:Y", False), (b"  :Y", True),
            (b" " + b"c" * 130 + b":Y", True), (b" " + b"c" * 62 + b":Y", True), (b" " + b"c" * 63 + b":", False),
            (b" " + b"c" * 63 + b":N", False), (b" " + b"c" * 63 + b":Y", True), (b" " + b"c" * 200, False)]


def casava_records(n=96):
    rng = np.random.default_rng(1)
    al = np.frombuffer(b"ACGT", np.uint8)
    return [record(b"c%d" % k + COMMENTS[k % len(COMMENTS)][0], rng.choice(al, 20 + k % 7).tobytes(), b"I" * (20 + k % 7))
            for k in range(n)]


def test_casava(gi):
    recs = casava_records()
    got, w = check(gi, recs, mode=MODE_CFY)
    gone = [g for _, g in COMMENTS]
    assert (w["rec"][:, 0] == FILTERED).tolist() == [gone[k % len(gone)] for k in range(len(recs))]
    plain, wp = check(gi, recs, mode=0)                       # without -Y every record is a read
    assert wp["ctr"][1] == len(recs) and wp["octr"][1] == 0


@pytest.mark.parametrize("max_records,rec_cap", [(1, 0), (1, 96), (10, 96), (10, 12), (37, 96), (60, 96), (96, 0), (5, 3)])
def test_filtered_records_do_not_count(gi, max_records, rec_cap):
    """max_records counts the reads the reader keeps, rec_cap the records looked at; consumed
    lands on a record's start (expected() checks it against parse_host's own)."""
    recs = casava_records()
    got, w = check(gi, recs, mode=MODE_CFY, max_records=max_records, rec_cap=rec_cap)
    assert w["ctr"][1] <= max_records and w["rows"] <= (rec_cap or max_records)
    if rec_cap == 96 and max_records < 60:
        assert w["ctr"][1] == max_records and w["rows"] > max_records and w["rec"][-1, 0] != FILTERED


def test_all_options_and_a_record_that_is_not_canonical(gi):
    recs = barcode_records(6) + casava_records(40) + trim_records()[:30]
    mode = (6 << 24) | MODE_CFY
    at = len(recs)
    w = expected(recs, mode=mode, trim_qual=20)
    two_line = b"@bad 1:N:0\nACGTACGTAC\nACGTACGTAC\n+\n" + b"I" * 20 + b"\n"
    data = w["data"] + two_line + b"".join(recs[:5])
    got = run(gi, w, mode=mode, trim_qual=20, data=data)
    w["ctr"][0], w["ctr"][11], w["ctr"][12] = at + 1, at, len(w["data"])
    assert_equal(got, w)


def test_fixture_reads(gi):
    """load_device on the committed option fixtures: the lengths parse_host gives (which the
    CPU test holds against the reference's XC and BC tags)."""
    from hsa_amd import reads
    for name in CASES:
        mode, trim = case_options(name)
        data = case_reads(name)
        p = reads.parse_host(data, mode=mode, trim_qual=trim)
        t = reads.load_device(gi, reads.upload(data), len(data), True, 1 << 20, 1 << 20, 32, mode=mode, trim_qual=trim)
        assert t["n_loaded"] == len(p["names"]) and t["octr"]["filtered"] == p["filtered"] and t["consumed"] == len(data)
        assert t["octr"]["trimmed_bases"] == p["trimmed_bases"] and t["octr"]["total_bases"] == p["total_bases"]
        rows = t["rec"].cpu().numpy()[:4 * t["n_rows"]].view(np.uint32).reshape(-1, 4)
        assert len(rows) == len(p["names"]) + p["filtered"]
        read = rows[rows[:, 0] != FILTERED]
        assert read[:, 1].tolist() == p["lens"]
        full, bc, bcn = t["full_len"].cpu().numpy().view(np.uint32), t["bc"].cpu().numpy(), t["bc_len"]
        quals, qoff = t["quals"].cpu().numpy(), t["qual_off"].cpu().numpy().view(np.uint64)
        jobs = np.flatnonzero(read[:, 0] == 0)
        assert len(jobs) == t["n_jobs"] > 100 and read[jobs, 3].tolist() == list(range(len(jobs)))
        for j, i in enumerate(jobs):
            assert full[j] == len(p["seqs"][i]) and bc[j * bcn:(j + 1) * bcn].tobytes() == p["bcs"][i]
            assert quals[int(qoff[j]):int(qoff[j + 1])].tobytes() == p["quals"][i]


def test_bad_arguments(gi):
    from hsa_amd._lib import HsaError
    from hsa_amd.reads import MAX_TRIM_QUAL
    recs = trim_records()[:20]
    assert MAX_TRIM_QUAL == 32674 and 65535 * (MAX_TRIM_QUAL + 94) <= 0x7FFFFFFF < 65535 * (MAX_TRIM_QUAL + 95)
    check(gi, recs, trim_qual=MAX_TRIM_QUAL)
    check(gi, recs, trim_qual=-3)                               # bwa_trim_read: trim_qual < 1 trims nothing
    w = expected(recs)
    for kw in (dict(trim_qual=MAX_TRIM_QUAL + 1), dict(mode=64 << 24), dict(mode=0x20), dict(mode=0x40), dict(mode=0x80),
               dict(mode=0x100), dict(rec_cap=(1 << 28) + 1)):
        with pytest.raises(HsaError, match="-2"):
            run(gi, w, **kw)
