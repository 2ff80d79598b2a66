"""FASTQ bytes to a search batch on the device (hsa_reads_device, hsa_amd.reads.load_device)
against the host restatement hsa_amd.reads.parse_host, word for word: jobs, codes, names,
qualities, offsets, the per-record rows and every counter; the canonical-record rule and the
hand-over at the first record that is not canonical; a cut last record; the filter; short
capacities and guard bytes; unaligned inputs; bad arguments."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ONES = 0xFFFFFFFFFFFFFFFF
TILE = 4096                      # HSA_RD_TILE: bytes per block of the newline passes
GUARD = 64


@pytest.fixture(scope="module")
def gi():
    from test_gpu_refine import index_text
    return index_text("tiny")


def fq(recs):
    """FASTQ text of (name line without '@', sequence, quality) triples."""
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in recs)


def rand_recs(n, seed, lens=(1, 14, 15, 16, 17, 64), alphabet=b"ACGTacgtNn.-"):
    rng = np.random.default_rng(seed)
    al = np.frombuffer(alphabet, np.uint8)
    out = []
    for k in range(n):
        l = int(lens[k % len(lens)])
        s = rng.choice(al[:8] if k % 3 else al, l).tobytes()
        q = rng.integers(33, 128, l).astype(np.uint8).tobytes()
        name = (b"r%d" % k) + (b"", b"/1", b"/2", b"/3", b" a comment", b"\tc/1")[k % 6]
        out.append((name, s, q))
    return out


def canonical_prefix(data, at_eof, n_table=None, max_records=1 << 20):
    """The rule of the header, restated: (records loaded, bytes consumed, first non-canonical
    record or None, records seen)."""
    lines, pos = [], 0
    while pos < len(data):
        j = data.find(b"\n", pos)
        if j < 0:
            lines.append((pos, len(data), False))
            break
        lines.append((pos, j, True))
        pos = j + 1
    space = b" \t\n\v\f\r"
    k = 0
    while k < max_records:
        grp = lines[4 * k:4 * k + 4]
        if not grp:
            return k, len(data), None, k
        if len(grp) < 4 or not grp[3][2]:
            if not at_eof:
                return k, grp[0][0], None, k
            if len(grp) < 4:
                return k, grp[0][0], k, k + 1
        (h0, h1, _), (s0, s1, _), (p0, p1, _), (q0, q1, _) = grp
        head, seq, plus, qual = data[h0:h1], data[s0:s1], data[p0:p1], data[q0:q1]
        name = head[1:]
        for i, c in enumerate(name):
            if c in space:
                name = name[:i]
                break
        ok = (head[:1] == b"@" and len(name) >= 1 and 0 not in name and 1 <= len(seq) <= 65535
              and all(33 <= c <= 126 and c not in b">+@" for c in seq) and plus[:1] == b"+" and len(qual) == len(seq)
              and all(33 <= c <= 127 for c in qual) and (n_table is None or len(seq) < n_table))
        if not ok:
            return k, h0, k, k + 1
        k += 1
    return k, lines[4 * k][0] if 4 * k < len(lines) else len(data), None, k


def expected(data, at_eof, max_diff=4, table=None, seed_len=32, regime=0, max_records=1 << 20, len_floor=0):
    """What the call must leave, from parse_host of the canonical prefix."""
    from hsa_amd import reads
    from hsa_amd._lib import JOB_DTYPE
    loaded, consumed, bad, seen = canonical_prefix(data, at_eof, None if table is None else len(table), max_records)
    p = reads.parse_host(data[:consumed])
    assert len(p["names"]) == loaded and p["end"] == -1
    lens = [len(s) for s in p["seqs"]]
    thr = int(table[max(lens + [len_floor])]) if table is not None else max_diff
    rec = np.zeros((loaded, 4), np.uint32)
    jobs, codes, names, quals = [], [], [], []
    for k, (nm, sq, ql) in enumerate(zip(p["names"], p["seqs"], p["quals"])):
        nn = int((sq > 3).sum())
        st = 1 if nn > thr else 2 if len(sq) >= 15 and ((sq[:15] == 0).all() or (sq[:15] == 3).all()) else 0
        rec[k] = (st, len(sq), nn, len(jobs) if st == 0 else 0xFFFFFFFF)
        if st == 0:
            jobs.append((sum(len(c) for c in codes), len(sq), int(table[len(sq)]) if table is not None else max_diff,
                         seed_len if seed_len < len(sq) else 0x7FFFFFFF, regime))
            codes.append(sq)
            names.append(nm)
            quals.append(ql)
    cb = np.concatenate(codes + [np.zeros(16, np.uint8)])
    nb, qb = b"".join(names), b"".join(quals)
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)
    ctr = [seen, loaded, len(jobs), len(jobs), len(cb), len(cb), len(nb), len(nb), len(qb), len(qb), consumed,
           ONES if bad is None else bad, ONES if bad is None else consumed, max(lens, default=0),
           max((j[1] for j in jobs), default=0), thr & ONES]
    return dict(rec=rec, jobs=np.array(jobs, JOB_DTYPE) if jobs else np.zeros(0, JOB_DTYPE), codes=cb,
                names=np.frombuffer(nb, np.uint8), quals=np.frombuffer(qb, np.uint8), name_off=off(names), qual_off=off(quals),
                ctr=ctr, loaded=loaded, consumed=consumed, bad=bad)


def run(gi, data, at_eof, want=None, caps=None, max_diff=4, table=None, seed_len=32, regime=0, max_records=None, shift=0,
        mode=0, trim_qual=0, len_floor=0):
    """One hsa_reads_device call on `data` placed `shift` bytes into a device buffer (the
    bytes around it 0x0A, which a kernel that read them would count); the outputs hold the
    capacities given (default: exactly what `want` needs) and GUARD bytes of 0xA5 after them."""
    import torch
    from hsa_amd._lib import JOB_DTYPE, ReadsBatch
    if max_records is None:
        max_records = max(len(data) // 8 + 1, 1)
    w = want or expected(data, at_eof, max_diff, table, seed_len, regime, max_records, len_floor)
    cap = dict(jobs=len(w["jobs"]), codes=len(w["codes"]), names=len(w["names"]), quals=len(w["quals"]))
    cap.update(caps or {})
    buf = np.full(shift + len(data) + 48, 0x0A, np.uint8)
    buf[shift:shift + len(data)] = np.frombuffer(data, np.uint8)
    d_in = torch.from_numpy(buf).cuda()
    JB = JOB_DTYPE.itemsize
    fill = lambda n: torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    o = dict(jobs=fill(cap["jobs"] * JB), codes=fill(cap["codes"]), names=fill(cap["names"]), quals=fill(cap["quals"]),
             name_off=fill((cap["jobs"] + 1) * 8), qual_off=fill((cap["jobs"] + 1) * 8), rec=fill(max_records * 16),
             ctr=torch.full((16,), 0x33, dtype=torch.int64, device="cuda"))
    d_tab = torch.from_numpy(np.ascontiguousarray(table, np.int32)).cuda() if table is not None else None
    b = ReadsBatch(d_in=d_in.data_ptr() + shift, n_in=len(data), at_eof=at_eof, max_records=max_records, max_diff=max_diff,
                   d_maxdiff=d_tab.data_ptr() if table is not None else None, n_maxdiff=len(table) if table is not None else 0,
                   len_floor=len_floor, seed_len=seed_len, regime=regime, trim_qual=trim_qual, mode=mode, d_jobs=o["jobs"].data_ptr(),
                   job_cap=cap["jobs"], d_codes=o["codes"].data_ptr(), code_cap=cap["codes"], d_names=o["names"].data_ptr(),
                   name_cap=cap["names"], d_name_off=o["name_off"].data_ptr(), d_quals=o["quals"].data_ptr(),
                   qual_cap=cap["quals"], d_qual_off=o["qual_off"].data_ptr(), d_rec=o["rec"].data_ptr(),
                   d_counters=o["ctr"].data_ptr())
    torch.cuda.synchronize()
    gi.reads_device(b)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["ctr"] = [int(v) for v in got["ctr"].view(np.uint64)]
    got["cap"] = cap
    return got, w


def assert_equal(got, w):
    """Every output against the expectation, cut at the capacities; guards untouched."""
    from hsa_amd._lib import JOB_DTYPE
    cap = got["cap"]
    JB = JOB_DTYPE.itemsize
    nj = min(len(w["jobs"]), cap["jobs"])
    ctr = list(w["ctr"])
    ctr[3] = nj
    for i, k in ((5, "codes"), (7, "names"), (9, "quals")):
        ctr[i] = min(ctr[i - 1], cap[k])
    assert got["ctr"] == ctr
    assert np.array_equal(got["jobs"][:nj * JB].view(JOB_DTYPE), w["jobs"][:nj])
    for k in ("codes", "names", "quals"):
        m = min(len(w[k]), cap[k])
        assert np.array_equal(got[k][:m], w[k][:m]), k
        assert (got[k][m:] == 0xA5).all(), k + " past its capacity or its end"
    assert (got["jobs"][nj * JB:] == 0xA5).all()
    no = min(len(w["jobs"]), cap["jobs"]) + 1
    for k in ("name_off", "qual_off"):
        assert np.array_equal(got[k][:no * 8].view(np.uint64), w[k][:no]), k
        assert (got[k][no * 8:] == 0xA5).all(), k
    L = w["loaded"]
    assert np.array_equal(got["rec"][:L * 16].view(np.uint32).reshape(-1, 4), w["rec"])
    assert (got["rec"][L * 16:] == 0xA5).all()


def check(gi, data, at_eof=1, **kw):
    got, w = run(gi, data, at_eof, **kw)
    assert_equal(got, w)
    return got, w


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", [0, 1, 65, 700])
def test_record_counts(gi, n):
    data = fq(rand_recs(n, n))
    _, w = check(gi, data)
    assert w["loaded"] == n and w["bad"] is None and w["consumed"] == len(data)
    if n:
        check(gi, data[:-1])                                  # no final newline: the end of the input ends the record
    if n == 700:
        st = w["rec"][:, 0]
        assert set(np.unique(w["rec"][:, 1])) == {1, 14, 15, 16, 17, 64} and 5 in w["codes"] and (st == 1).any()
        assert len(data) > 8 * TILE
        again, _ = run(gi, data, 1, want=w)                   # two runs give equal arrays
        first, _ = run(gi, data, 1, want=w)
        for k in ("jobs", "codes", "names", "quals", "name_off", "qual_off", "rec", "ctr"):
            assert np.array_equal(first[k], again[k]), k


def test_a_record_across_every_tile_edge(gi):
    """The first record grows a byte at a time, so the byte at TILE is in turn every part of
    a later record: header, sequence, '+', quality and each newline."""
    recs = rand_recs(170, 3, lens=(17, 30))
    size = len(fq(recs[:1]))
    assert len(fq(recs)) > 2 * TILE
    for grow in range(0, 80):
        head = (b"x" * (1 + grow), b"ACGT", b"IIII")
        data = fq([head] + recs)
        assert len(data) > 2 * TILE + size
        check(gi, data)


def test_names_and_qualities(gi):
    recs = [(b"a/1", b"ACGT", b"@III"), (b"/1", b"ACGT", b"+III"), (b"b/3", b"acgt", b"I@+I"), (b"c/2 x/1", b"N.-A", b"!~\x7f!"),
            (b"d\tcomment", b"ACGTACGTACGTACGTA", b"@" * 17), (b"e//1", b"A", b"+"), (b"f\x01\xff/1\r", b"G", b"I"),
            (b"+plus", b"T", b"@"), (b"@at", b"C", b"+")]
    got, w = check(gi, fq(recs))
    assert w["loaded"] == len(recs)
    names = [w["names"][int(a):int(b)].tobytes() for a, b in zip(w["name_off"], w["name_off"][1:])]
    assert names == [b"a", b"/1", b"b/3", b"c", b"d", b"e/", b"f\x01\xff", b"+plus", b"@at"]
    assert w["codes"][:12].tolist() == [0, 1, 2, 3] * 3
    assert w["codes"][12:16].tolist() == [4, 4, 5, 0]


BAD = dict(blank=lambda r: b"\n" + fq([r]), crlf=lambda r: b"@" + r[0] + b"\r\n" + r[1] + b"\r\n+\r\n" + r[2] + b"\r\n",
           two_line=lambda r: b"@" + r[0] + b"\n" + r[1][:5] + b"\n" + r[1][5:] + b"\n+\n" + r[2] + b"\n",
           short_qual=lambda r: b"@" + r[0] + b"\n" + r[1] + b"\n+\n" + r[2][:-1] + b"\n",
           fasta=lambda r: b">" + r[0] + b"\n" + r[1] + b"\n", empty_name=lambda r: b"@ " + r[0] + b"\n" + r[1] + b"\n+\n" + r[2] + b"\n")


@pytest.mark.parametrize("kind", sorted(BAD))
def test_a_non_canonical_record_stops_the_load(gi, kind):
    from hsa_amd import reads
    recs = rand_recs(200, 11, lens=(17, 30, 41))
    at = 97
    head = fq(recs[:at])
    data = head + BAD[kind](recs[at]) + fq(recs[at + 1:])
    got, w = check(gi, data)
    assert w["loaded"] == at and w["bad"] == at and got["ctr"][11] == at and got["ctr"][12] == len(head)
    whole = reads.parse_host(data)
    front, rest = reads.parse_host(data[:got["ctr"][12]]), reads.parse_host(data[got["ctr"][12]:])
    assert front["names"] + rest["names"] == whole["names"] and len(whole["names"]) >= 199
    assert all(np.array_equal(a, b) for a, b in zip(front["seqs"] + rest["seqs"], whole["seqs"]))
    assert front["quals"] + rest["quals"] == whole["quals"]


def test_long_reads_and_the_table_end(gi):
    from hsa_amd import reads
    table = reads.maxdiff_table(0.04, 40)
    recs = rand_recs(30, 2, lens=(20, 39), alphabet=b"ACGTacgt")
    recs[20] = (b"long", b"A" * 40, b"I" * 40)                # of n_maxdiff bases: past the table
    got, w = check(gi, fq(recs), table=table)
    assert w["bad"] == 20 and w["loaded"] == 20
    big = (b"big", b"ACGT" * 16384, b"I" * 65536)             # one base past HSA_RD_MAX_LEN
    ok = (b"ok", b"ACGT" * 16383 + b"ACG", b"I" * 65535)
    got, w = check(gi, fq([ok, big]))
    assert w["bad"] == 1 and w["loaded"] == 1 and got["ctr"][13] == 65535


def test_a_cut_last_record(gi):
    recs = rand_recs(40, 6, lens=(30,))
    data = fq(recs)
    start = len(fq(recs[:39]))
    for cut in (start + 1, start + 5, len(data) - 33, len(data) - 3, len(data) - 1):
        got, w = check(gi, data[:cut], at_eof=0)              # (len - 1: the quality may go on in the next chunk)
        assert w["loaded"] == 39 and got["ctr"][10] == start and got["ctr"][11] == ONES
    got, w = check(gi, data[:len(data) - 3], at_eof=1)
    assert w["bad"] == 39 and got["ctr"][12] == start
    got, w = check(gi, data[:start + 5], at_eof=1)
    assert w["bad"] == 39 and got["ctr"][0] == 40
    got, w = check(gi, data[:len(data) - 1], at_eof=1)        # complete but for its newline
    assert w["loaded"] == 40 and w["bad"] is None


def test_max_records(gi):
    data = fq(rand_recs(100, 8))
    got, w = check(gi, data, max_records=37)
    assert w["loaded"] == 37 and got["ctr"][10] == len(fq(rand_recs(100, 8)[:37])) and got["ctr"][11] == ONES


# ---------------------------------------------------------------- the filter
def test_filter(gi):
    from hsa_amd import reads
    from hsa_amd._lib import HsaError
    L = 40
    q = b"I" * L
    mk = lambda s: (b"r", (s + b"ACGTTGCAGT" * 4)[:L], q)
    recs = [mk(b"N" * 4), mk(b"N" * 5), mk(b"A" * 15 + b"C"), mk(b"T" * 15 + b"G"), mk(b"A" * 14 + b"C"), mk(b"a" * 15),
            (b"s", b"A" * 14, b"I" * 14), mk(b"n.-R")]
    got, w = check(gi, fq(recs), max_diff=4)
    assert w["rec"][:, 0].tolist() == [0, 1, 2, 2, 0, 2, 0, 0] and w["rec"][:, 2].tolist() == [4, 5, 0, 0, 0, 0, 0, 4]
    table = reads.maxdiff_table(0.04, 256)
    thr = int(table[100])
    assert thr == 5 and int(table[L]) == 3
    long = (b"l", b"ACGTTGCAGT" * 10, b"I" * 100)             # the longest loaded read sets the threshold
    recs = [mk(b"N" * thr), mk(b"N" * (thr + 1)), long, mk(b"N" * 3)]
    got, w = check(gi, fq(recs), table=table, seed_len=32)
    assert w["rec"][:, 0].tolist() == [0, 1, 0, 0] and got["ctr"][15] == thr
    assert w["jobs"]["max_diff"].tolist() == [3, 5, 3] and w["jobs"]["seed_len"].tolist() == [32, 32, 32]
    got, w = check(gi, fq(recs), table=table, seed_len=40, regime=1)
    assert w["jobs"]["seed_len"].tolist() == [0x7FFFFFFF, 40, 0x7FFFFFFF] and w["jobs"]["regime"].tolist() == [1, 1, 1]
    got, w = check(gi, fq(recs[:2] + recs[3:]), table=table)  # without it the same reads are dropped
    assert w["rec"][:, 0].tolist() == [1, 1, 0]
    got, w = check(gi, fq(recs[:2] + recs[3:]), table=table, len_floor=100)      # another chunk of the batch holds it
    assert w["rec"][:, 0].tolist() == [0, 1, 0] and got["ctr"][15] == thr and got["ctr"][13] == L
    with pytest.raises(HsaError, match="-2"):
        run(gi, fq(recs), 1, want=w, table=table, len_floor=256)
    got, w = check(gi, fq([mk(b"N" * 2)]), max_diff=-1)       # a negative threshold drops every read with an N
    assert w["rec"][:, 0].tolist() == [1]


# ---------------------------------------------------------------- room
@pytest.mark.parametrize("which", ["jobs", "codes", "names", "quals"])
def test_each_capacity_one_too_small(gi, which):
    data = fq(rand_recs(300, 4))
    roomy, w = check(gi, data)
    full = roomy["cap"]
    got, _ = run(gi, data, 1, want=w, caps={which: full[which] - 1})
    assert_equal(got, w)
    i = dict(jobs=2, codes=4, names=6, quals=8)[which]
    assert got["ctr"][i] == got["ctr"][i + 1] + 1
    sized = dict(jobs=got["ctr"][2], codes=got["ctr"][4], names=got["ctr"][6], quals=got["ctr"][8])
    again, _ = run(gi, data, 1, want=w, caps=sized)
    for k in ("jobs", "codes", "names", "quals", "name_off", "qual_off", "rec", "ctr"):
        assert np.array_equal(again[k], roomy[k]), k


def test_zero_capacities(gi):
    data = fq(rand_recs(50, 5))
    got, w = run(gi, data, 1, caps=dict(jobs=0, codes=0, names=0, quals=0))
    assert_equal(got, w)


@pytest.mark.parametrize("shift,cut", [(0, 0), (1, 0), (5, 3), (15, 7), (16, 1)])
def test_unaligned_input(gi, shift, cut):
    data = fq(rand_recs(300, 9))
    check(gi, data[:len(data) - cut], at_eof=0 if cut else 1, shift=shift)


def test_load_device_runs_again_when_room_is_short(gi):
    from hsa_amd import reads
    from hsa_amd._lib import JOB_DTYPE
    data = fq(rand_recs(300, 4))
    w = expected(data, 1)
    for caps in (None, dict(jobs=3, codes=10, names=1, quals=0)):
        t = reads.load_device(gi, reads.upload(data), len(data), True, 1000, 4, 32, caps=caps)
        n = t["n_jobs"]
        assert n == len(w["jobs"]) and t["max_len"] == 64 and t["n_loaded"] == 300 and t["consumed"] == len(data)
        assert np.array_equal(t["jobs"].cpu().numpy()[:n * JOB_DTYPE.itemsize].view(JOB_DTYPE), w["jobs"])
        for k in ("codes", "names", "quals"):
            assert np.array_equal(t[k].cpu().numpy()[:len(w[k])], w[k]), k
        for k in ("name_off", "qual_off"):
            assert np.array_equal(t[k].cpu().numpy().view(np.uint64)[:n + 1], w[k]), k


def test_bad_arguments(gi):
    from hsa_amd._lib import HsaError, ReadsBatch
    data = fq(rand_recs(10, 1))
    with pytest.raises(HsaError, match="-2"):                        # null outputs
        gi.reads_device(ReadsBatch(n_in=0, max_records=1))
    for kw in (dict(trim_qual=20), dict(mode=0x200), dict(mode=0x08), dict(mode=0x20), dict(mode=5 << 24),
               dict(max_records=0)):
        with pytest.raises(HsaError, match="-2"):
            run(gi, data, 1, want=expected(data, 1), **kw)
    with pytest.raises(HsaError, match="-2"):
        run(gi, data, 2, want=expected(data, 1))
    got, w = run(gi, data, 1, mode=0x03 | 0x04 | 0x10)               # the search's bits are no concern of the loader
    assert_equal(got, w)
