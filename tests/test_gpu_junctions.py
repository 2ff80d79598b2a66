"""The splice junction table on the device (hsa_junctions.hip through hsa_amd.junctions.Accumulator
and `align_fastq(..., splice=True, junctions=...)`): whole runs against from_sam over the text the
run printed and over the reference's committed SAM, batches with forced compaction, the three
entry points on fabricated rows against a NumPy restatement, the room rules, idempotence, and
the paths that must not change."""
import gzip
import io
import json
import os

import numpy as np
import pytest

from golden_io import GOLD, INDEX

pytestmark = pytest.mark.gpu
DUP = json.load(open(os.path.join(GOLD, "manifest_dup.json")))
TINY = json.load(open(os.path.join(GOLD, "manifest_dropin.json")))
OPTS = json.load(open(os.path.join(GOLD, "manifest_opts.json")))
PREFIX = dict(INDEX, dup=os.path.join(GOLD, "index", "dup.fa"))
# the reference's SAM file: (index, arguments, reads)
WHOLE = {
    "dup_ref_default": ("dup", DUP["default"]["args"], DUP["files"][DUP["default"]["reads"]]),
    "dup_ref_n4o1": ("dup", DUP["n4o1"]["args"], DUP["files"][DUP["n4o1"]["reads"]]),
    "dup_ref_q15": ("dup", DUP["q15"]["args"], DUP["files"][DUP["q15"]["reads"]]),
    "dropin_ref_splice_default": ("tiny", TINY["splice_default"]["args"], TINY["splice_reads"]),
    "dropin_ref_splice_n4o1": ("tiny", TINY["splice_n4o1"]["args"], TINY["splice_reads"]),
    "dropin_ref_default": ("tiny", TINY["default"]["args"], TINY["reads"]),
    "opts_ref_splice_q15": ("tiny", OPTS["splice_q15"]["args"], OPTS["files"][OPTS["splice_q15"]["reads"]]),
    "opts_ref_splice_B6q15Y": ("tiny", OPTS["splice_B6q15Y"]["args"], OPTS["files"][OPTS["splice_B6q15Y"]["reads"]]),
    "opts_ref_splice_q20n4o1": ("tiny", OPTS["splice_q20n4o1"]["args"], OPTS["files"][OPTS["splice_q20n4o1"]["reads"]]),
}
_OPEN, _RUNS = {}, {}


@pytest.fixture(scope="module")
def indexes():
    from hsa_amd import align

    def get(name):
        if name not in _OPEN:
            _OPEN[name] = align.open_index64(PREFIX[name])
        return _OPEN[name]
    yield get
    for gi, _ in _OPEN.values():
        gi.close()
    _OPEN.clear()


def run(opened, args, reads, junctions=True, calls=None, **kw):
    """align_fastq with splice=True: (the SAM text, the table's bytes or None, the statistics).
    calls: a dict that receives the number of calls of each junction stage."""
    from hsa_amd import align, chain
    gi, chrs = opened
    opts = align.parse_options(args, reader_options=True)[0]
    out, table = io.BytesIO(), io.BytesIO() if junctions else None
    real = {k: getattr(chain, k) for k in ("junction_rows", "junction_reduce", "junction_text")}

    def counted(k):
        def f(*a, **k2):
            calls[k] = calls.get(k, 0) + 1
            return real[k](*a, **k2)
        return f
    if calls is not None:
        for k in real:
            setattr(chain, k, counted(k))
    try:
        _, stats = align.align_fastq(gi, chrs, gzip.open(os.path.join(GOLD, reads)).read(), opts, out, splice=True,
                                     **(dict(junctions=table) if junctions else {}), **kw)
    finally:
        for k, f in real.items():
            setattr(chain, k, f)
    return out.getvalue(), table.getvalue() if junctions else None, stats


def whole(indexes, name):
    if name not in _RUNS:
        index, args, reads = WHOLE[name]
        _RUNS[name] = run(indexes(index), args, reads)
    return _RUNS[name]


# ---------------------------------------------------------------- 1. the whole command
@pytest.mark.parametrize("name", list(WHOLE))
def test_whole_command(indexes, name):
    from hsa_amd import junctions
    text, table, stats = whole(indexes, name)
    prefix = PREFIX[WHOLE[name][0]]
    rows, want = junctions.from_sam(text, prefix)
    n_spliced = sum("\tXT:A:S" in ln for ln in text.decode().split("\n"))
    same = text == gzip.open(os.path.join(GOLD, name + ".sam.gz")).read()
    print(f"{name}: {len(rows)} introns of {n_spliced} spliced lines, the text is the reference's: {same}; handed back "
          f"{stats['handed_back']}, refused {stats['spliced_refused']}")
    assert n_spliced > 50 and table == want
    assert stats["junction_rows"] == n_spliced == stats["spliced"] and stats["junctions"] == len(rows)
    assert int(rows[:, 3].sum()) + int(rows[:, 4].sum()) == n_spliced and int(rows[:, 4].sum()) == stats["spliced_xa"]
    # every committed run but dup's default one (3 lines lost to hand-backs) prints the reference's text
    assert same or name == "dup_ref_default"
    if same:
        assert table == junctions.from_sam(gzip.open(os.path.join(GOLD, name + ".sam.gz")).read(), prefix)[1]


# ---------------------------------------------------------------- 2. batches and compaction
def test_batches_and_compaction(indexes):
    _, want, one = whole(indexes, "dup_ref_n4o1")
    index, args, reads = WHOLE["dup_ref_n4o1"]
    calls = {}
    _, table, stats = run(indexes(index), args, reads, calls=calls, batch_reads=100, junction_threshold=32)
    print(calls, stats["batches"], stats["junction_rows"], stats["junctions"])
    assert one["batches"] == 1 and stats["batches"] == 7
    # compacted on the way: the first batch alone passes 32 rows; then once more for the table
    assert calls["junction_reduce"] >= 2 and calls["junction_rows"] >= 7 and calls["junction_text"] == 1
    assert table == want
    assert (stats["junction_rows"], stats["junctions"]) == (365, 81) == (one["junction_rows"], one["junctions"])


# ---------------------------------------------------------------- 3. fabricated rows
STRIDE = 12
GARBAGE = 0xFFFFFFFF


def motif_sites(prefix):
    """Per chromosome and motif code: (first base, last base) of an intron with that motif, found
    by scanning the text; and the block table."""
    from hsa_amd import index_io, junctions
    pac, blocks = index_io.read_pac(prefix), index_io.read_blocks(prefix).astype(np.int64)
    two = pac[:-1].astype(np.int64) * 4 + pac[1:]                      # the bases at text t, t + 1
    sites = {}
    for c in sorted(set(blocks[:, 0].tolist())):
        bl = blocks[blocks[:, 0] == c]
        first, last = bl[0], bl[-1]                                    # the intron starts in the first block, ends in the last
        for (b0, b1, b2, b3), m in list(junctions.MOTIFS.items()) + [((0, 0, 0, 0), 0)]:
            lo = np.flatnonzero(two[first[1]:first[2]] == b0 * 4 + b1)
            hi = np.flatnonzero(two[last[1]:last[2]] == b2 * 4 + b3)
            s = int(first[3]) + 1 + int(lo[len(lo) // 3])
            ends = int(last[3]) + 2 + hi
            e = int(ends[ends > s + 60][m])
            assert junctions.motif_of(pac, blocks, c, s, e) == m
            sites[c, m] = (s, e)
    return sites, pac, blocks


def fabricate(prefix, n=5000, seed=5):
    """Lines-stage arrays of n reads (d_rows, d_cigar, d_line_stat) and 40 rows that arrive already
    reduced, with the junction rows they must give (the rows call's restatement)."""
    from hsa_amd import junctions
    from hsa_amd._lib import SL_ROW_WORDS
    rng = np.random.default_rng(seed)
    sites, pac, blocks = motif_sites(prefix)
    chroms = sorted({c for c, _ in sites})
    introns = [(c, *sites[c, m]) for c in chroms for m in range(7)]                # all chromosomes, all seven codes
    c0 = chroms[0]
    a, b, c = (c0, *sites[c0, 1]), (c0, *sites[c0, 2]), (chroms[-1], *sites[chroms[-1], 3])
    introns += [(a[0], a[1], a[2] + 7), (a[0], a[1], a[2] + 1), (a[0], a[1] - 5, a[2]), (a[0], a[1] + 1, a[2])]      # equal starts, equal ends
    if len(blocks) > len(chroms):                                      # nrun: an end in a gap, ends in different blocks
        for ch in chroms:
            bl = blocks[blocks[:, 0] == ch]
            gap_first = int(bl[0][3] + bl[0][2] - bl[0][1] + 2)        # the first base of the N run behind the first block
            assert gap_first < int(bl[1][3]) + 1 and junctions.text_pos(blocks, ch, gap_first) is None
            introns += [(ch, gap_first - 40, gap_first + 3), (ch, gap_first, int(bl[1][3]) + 30), (ch, gap_first - 1, int(bl[1][3]) + 1)]
            assert junctions.text_pos(blocks, ch, gap_first - 1) + 1 == junctions.text_pos(blocks, ch, int(bl[1][3]) + 1)
    ids = [0] * (n // 2) + [1] * 65 + [2] * 64                         # a run over several workgroups, 65, 64, singletons
    big = [a, b, c]
    n_bad = n * 9 // 100
    singles = list(range(3, 3 + len(introns)))
    fill = n - n_bad - len(ids) - len(singles)
    # the rest: distinct singletons behind the first chromosome's motif-0 site, a few in pairs
    s0, e0 = sites[c0, 0]
    extra = [(c0, s0 + 2 * k, e0 + 3 * k) for k in range(1, fill - 40 + 1)]
    table = big + introns + extra
    ids = ids + singles + list(range(3 + len(introns), len(table))) + list(rng.integers(3, len(table), 40))
    ids = np.array(ids + [-1] * n_bad)
    assert len(ids) == n
    rng.shuffle(ids)
    over = rng.integers(1, 41, n)
    for k in range(3):                                                 # the maximum neither first nor last in its run
        at = np.flatnonzero(ids == k)
        over[at[len(at) // 2]] = 60
        assert over[at[0]] < 60 and over[at[-1]] < 60
    rows = np.zeros((n, SL_ROW_WORDS), np.uint32)
    cigar = np.full((n, STRIDE), GARBAGE, np.uint32)
    stat = np.zeros(n, np.uint32)
    want = []
    op = lambda o, l: (o << 28) | int(l)
    for j in range(n):
        if ids[j] < 0:                                                 # a read without a line: nothing of it is read
            stat[j] = 1 + j % 8
            rows[j] = GARBAGE
            rows[j, 0] = stat[j]
            continue
        ch, s, e = table[ids[j]]
        ov, shape, xa = int(over[j]), j % 3, int(rng.integers(0, 3) == 0) * int(rng.integers(1, 9))
        if shape == 0:
            ops = [op(0, ov), op(3, e - s + 1), op(0, ov + j % 5)]
            ref = ov
        elif shape == 1:                                               # S, M, D, M | N | M, I, M
            ops = [op(4, 3), op(0, ov + 4), op(2, 2), op(0, 6), op(3, e - s + 1), op(0, ov - ov // 2), op(1, 1), op(0, ov // 2)]
            ref = ov + 12
        else:                                                          # M, I, M, S | N | M, S
            ops = [op(0, ov + 7 - ov // 3), op(1, 2), op(0, ov // 3), op(4, 2), op(3, e - s + 1), op(0, ov), op(4, 9)]
            ref = ov + 7
        at = [k for k, w in enumerate(ops) if w >> 28 == 3][0]
        cigar[j, :len(ops)] = ops
        rows[j, 5], rows[j, 6], rows[j, 7], rows[j, 18], rows[j, 20], rows[j, 21], rows[j, 22] = len(ops), ch, s - ref, e - s + 1, at, len(ops) - at - 1, xa
        want.append((ch, s, e, 0 if xa else 1, 1 if xa else 0, ov, 0, 0))
    pre = np.array([(*table[k], 2 + k % 3, k % 4, 30 + k, k % 7, 0) for k in ([0, 1, 2, 0] + list(range(5, 41)))], np.uint32)
    assert len(pre) == 40
    return dict(rows=rows, cigar=cigar, stat=stat, pre=pre, want=np.concatenate([pre, np.array(want, np.uint32)]), pac=pac, blocks=blocks,
                n_runs=[n // 2, 65, 64])


def lines_tensors(f, lo=0, hi=None):
    from hsa_amd import chain
    hi = len(f["stat"]) if hi is None else hi
    return dict(rows=chain.to_device(f["rows"][lo:hi]), cigar=chain.to_device(f["cigar"][lo:hi]), stat=chain.to_device(f["stat"][lo:hi]),
                cigar_stride=STRIDE), hi - lo


def buffer(cap, pre=None, guard=16):
    """A row buffer of cap rows with `guard` rows of '#' behind it, the rows of pre at its start."""
    import torch
    from hsa_amd._lib import JN_ROW_WORDS
    t = torch.full(((cap + guard) * JN_ROW_WORDS,), 0x23232323, dtype=torch.int32, device="cuda")
    if pre is not None and len(pre):
        t[:pre.size] = torch.from_numpy(pre.reshape(-1).view(np.int32).copy()).cuda()
    return t


def host_rows(t, n):
    from hsa_amd._lib import JN_ROW_WORDS
    return t[:n * JN_ROW_WORDS].cpu().numpy().view(np.uint32).reshape(-1, JN_ROW_WORDS)


def guard_untouched(t, cap):
    from hsa_amd._lib import JN_ROW_WORDS
    return bool((t[cap * JN_ROW_WORDS:] == 0x23232323).all().item())


def chr_strings(names):
    from hsa_amd import chain, sam
    cb, coff = sam.pack_strings(names)
    return chain.to_device(cb), chain.to_device(coff)


@pytest.mark.parametrize("index", ["tiny", "nrun"])
def test_fabricated_rows(indexes, index):
    from hsa_amd import chain, junctions
    gi, names = indexes(index)
    f = fabricate(PREFIX[index])
    o, n = lines_tensors(f)
    want = f["want"]
    cap = len(want) + 11
    t = buffer(cap, f["pre"])
    ctr = chain.junction_rows(gi, o, n, t, len(f["pre"]), cap)
    assert (int(ctr[0]), int(ctr[1])) == (len(want) - 40, len(want) - 40) and int((f["stat"] == 0).sum()) == len(want) - 40
    got = host_rows(t, len(want))
    assert np.array_equal(got, want)                                    # read order behind the rows that were there
    assert (host_rows(t, cap)[len(want):] == 0x23232323).all() and guard_untouched(t, cap)
    reduced = junctions.reduce_rows(want, f["pac"], f["blocks"])
    support = np.sort(reduced[:, 3] + reduced[:, 4])[::-1]
    assert support[0] > 2500 and len(reduced) > 1500 and set(reduced[:, 6].tolist()) == set(range(7))
    assert len(set(reduced[:, 0].tolist())) == len(names)
    assert (reduced[:, 3] > 1).any() and (reduced[:, 4] > 1).any() and int(reduced[:, 5].max()) >= 60
    rc = chain.junction_reduce(gi, t, len(want))
    assert (int(rc[0]), int(rc[1])) == (len(want), len(reduced))
    assert np.array_equal(host_rows(t, len(reduced)), reduced)
    assert guard_untouched(t, cap)
    if index == "nrun":                                                 # ends in two blocks with a motif, an end in a gap without
        bl = f["blocks"]
        two = [r for r in reduced if junctions.text_pos(bl, int(r[0]), int(r[1])) is not None and
               junctions.text_pos(bl, int(r[0]), int(r[2])) is not None and
               junctions.text_pos(bl, int(r[0]), int(r[2])) - junctions.text_pos(bl, int(r[0]), int(r[1])) != int(r[2]) - int(r[1])]
        gap = [r for r in reduced if junctions.text_pos(bl, int(r[0]), int(r[1])) is None or junctions.text_pos(bl, int(r[0]), int(r[2])) is None]
        assert len({int(r[6]) for r in two}) == 7 and len(gap) >= 6 and all(int(r[6]) == 0 for r in gap)
    cb, coff = chr_strings(names)
    text = junctions.table_bytes(reduced, names)
    ot, tc = chain.junction_text(gi, t, len(reduced), cb, coff, len(names), len(text) + 9)
    assert (int(tc[0]), int(tc[1]), int(tc[2]), int(tc[3])) == (len(text), len(text), len(reduced), 0)
    assert ot["out"][:len(text)].cpu().numpy().tobytes() == text
    off = ot["line_off"].cpu().numpy().view(np.uint64)
    assert int(off[0]) == 0 and int(off[-1]) == len(text) and all(text[int(k) - 1:int(k)] == b"\n" for k in off[1:])


# ---------------------------------------------------------------- 4. room
def test_room(indexes):
    import torch
    from hsa_amd import chain, junctions
    gi, names = indexes("tiny")
    f = fabricate(PREFIX["tiny"], n=700, seed=9)
    ok = np.flatnonzero(f["stat"] == 0)
    hi = int(ok[99]) + 1                                                # the first 100 reads with a line
    o, n = lines_tensors(f, 0, hi)
    want = f["want"][40:140]
    t = buffer(10)
    ctr = chain.junction_rows(gi, o, n, t, 0, 10)
    assert (int(ctr[0]), int(ctr[1])) == (100, 10)
    assert np.array_equal(host_rows(t, 10), want[:10]) and guard_untouched(t, 10)
    # a buffer that holds 7 rows already: 3 more fit
    t = buffer(10, want[:7])
    ctr = chain.junction_rows(gi, o, n, t, 7, 10)
    assert (int(ctr[0]), int(ctr[1])) == (100, 3)
    assert np.array_equal(host_rows(t, 10), np.concatenate([want[:7], want[:3]])) and guard_untouched(t, 10)
    t = buffer(100)
    ctr = chain.junction_rows(gi, o, n, t, 0, 100)
    assert (int(ctr[0]), int(ctr[1])) == (100, 100) and np.array_equal(host_rows(t, 100), want) and guard_untouched(t, 100)
    # the text's room
    rc = chain.junction_reduce(gi, t, 100)
    m = int(rc[1])
    text = junctions.table_bytes(host_rows(t, m), names)
    cb, coff = chr_strings(names)
    cap = len(text) // 2 + 5
    tb, ot = chain.junction_text_batch(t, m, cb, coff, len(names), cap)
    ot["out"] = torch.full((len(text) + 64,), 0x23, dtype=torch.uint8, device="cuda")
    tb.d_out = ot["out"].data_ptr()
    torch.cuda.synchronize()
    gi.junction_text(tb)
    torch.cuda.synchronize()
    tc = ot["ctr"].cpu().numpy().view(np.uint64)
    got = ot["out"].cpu().numpy().tobytes()
    assert (int(tc[0]), int(tc[1]), int(tc[2])) == (len(text), cap, m)
    assert got[:cap] == text[:cap] and got[cap:] == b"#" * (len(text) + 64 - cap)
    ot, tc = chain.junction_text(gi, t, m, cb, coff, len(names), cap)              # the driver asks again with the room wanted
    assert int(tc[0]) == int(tc[1]) == len(text) and ot["out"][:len(text)].cpu().numpy().tobytes() == text


def test_zero_rows(indexes):
    import torch
    from hsa_amd import chain, junctions
    gi, names = indexes("tiny")
    f = fabricate(PREFIX["tiny"], n=700, seed=9)
    o, _ = lines_tensors(f, 0, 1)
    t = buffer(4)
    assert not chain.junction_rows(gi, o, 0, t, 0, 4).any()
    bad = dict(o, stat=chain.to_device(np.array([3], np.uint32)))       # one read, no line
    assert not chain.junction_rows(gi, bad, 1, t, 0, 4).any()
    assert not chain.junction_reduce(gi, t, 0).any()
    cb, coff = chr_strings(names)
    ot, tc = chain.junction_text(gi, t, 0, cb, coff, len(names), 0)
    assert not tc.any() and int(ot["line_off"][0].item()) == 0 and guard_untouched(t, 0)
    torch.cuda.synchronize()
    acc = junctions.Accumulator(gi, names)
    assert acc.finish() == b"" and (acc.fed, acc.distinct) == (0, 0)


# ---------------------------------------------------------------- 5. idempotence and determinism
def test_idempotence_and_determinism(indexes):
    from hsa_amd import chain, junctions
    gi, names = indexes("nrun")
    f = fabricate(PREFIX["nrun"], n=3000, seed=21)
    o, n = lines_tensors(f)
    cb, coff = chr_strings(names)

    def full():
        t = buffer(len(f["want"]), f["pre"])
        ctr = chain.junction_rows(gi, o, n, t, 40, len(f["want"]))
        rc = chain.junction_reduce(gi, t, 40 + int(ctr[1]))
        m = int(rc[1])
        ot, tc = chain.junction_text(gi, t, m, cb, coff, len(names), 64 * m)
        return t, m, ot["out"][:int(tc[1])].cpu().numpy().tobytes(), ot["line_off"].cpu().numpy()
    t1, m1, text1, off1 = full()
    t2, m2, text2, off2 = full()
    assert m1 == m2 and text1 == text2 and np.array_equal(off1, off2) and np.array_equal(t1.cpu().numpy(), t2.cpu().numpy())
    before = host_rows(t1, m1).copy()
    rc = chain.junction_reduce(gi, t1, m1)                              # a reduced table reduced again
    assert (int(rc[0]), int(rc[1])) == (m1, m1) and np.array_equal(host_rows(t1, m1), before)
    assert text1 == junctions.table_bytes(before, names)
    # the accumulator with a threshold of a few dozen rows, fed in slices: the same table
    acc = junctions.Accumulator(gi, names, threshold=48, room=40)
    acc.rows[:f["pre"].size] = chain.to_device(f["pre"])
    acc.n = 40
    for lo in range(0, n, 500):
        acc.add(*lines_tensors(f, lo, min(lo + 500, n)))
    # (compactions: the first slice passes 48 rows, the second passes twice what that left, and finish())
    assert acc.finish() == text1 and acc.compactions >= 3 and acc.distinct == m1 and acc.fed == len(f["want"]) - 40


# ---------------------------------------------------------------- 6. off means off
def test_off_means_off(indexes):
    from hsa_amd import align
    index, args, reads = WHOLE["opts_ref_splice_q15"]
    calls = {}
    text, table, stats = run(indexes(index), args, reads, junctions=False, calls=calls)
    assert table is None and calls == {} and not [k for k in stats if k.startswith("junction")]
    assert text == whole(indexes, "opts_ref_splice_q15")[0]
    assert {k: v for k, v in whole(indexes, "opts_ref_splice_q15")[2].items() if not k.startswith("junction")} == stats
    assert "junctions" not in align.parse_options(["--splice", "x", "y"], reader_options=True)[2]
    assert align.parse_options(["--splice", "--junctions", "t", "x", "y"], reader_options=True)[2]["junctions"] == "t"
    gi, chrs = indexes(index)
    calls = {}
    with pytest.raises(ValueError, match="--splice"):
        align.align_fastq(None, chrs, b"@r\nACGT\n+\nIIII\n", align.default_opts(), io.BytesIO(), junctions=io.BytesIO())
