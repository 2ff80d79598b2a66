"""Strands that cannot hit (hsa_search_kernels.h): k_widths_lazy computes the rc row of every
read and, in the same launch, the forward row of the reads whose rc root is pruned at its
first pop (the bid of the last base exceeds max_diff, bwtgap.c:170); every width kernel flags
such strands in wq and k_search's begin_item starts none of them: it counts the root's pop and
goes on to the forward strand, or ends the read when that one is doomed too.

Every search here equals the oracle's: n_aln, the fallback flag, every word of every hit, the
rank-query count (d_counters[2]) and the pop count (d_counters[4]).  Each batch is searched
with HSA_LAZY=0 and HSA_LAZY=1 (HSA_SPLIT=0: one read per lane, the path that has the
shortcut) and once in cost order (HSA_ORDER=1).

The reads are drawn once (POOL reads in a fixed shuffled order) and a batch of n reads is its
first n, so the small batches cross the wave and workgroup edges of k_widths_lazy's compaction
with the same mixture.  The classes are computed from the oracle's cal_width bids and hits, and
every class must hold at least 8 reads in the pool (and in every batch of 255 reads or more; a
batch of one read cannot hold six classes) before anything is compared."""
import numpy as np
import pytest

from hsa_amd import synth
from test_gpu_implicit import _draw, _opts, _search, _syn
from test_gpu_seednib import _assert_device

pytestmark = pytest.mark.gpu

POOL = 1000
SIZES = [1, 63, 64, 65, 255, 257, 1000]
MODES = [("0", None), ("1", None), ("1", "1")]          # (HSA_LAZY, HSA_ORDER)
MODE_IDS = ["eager", "lazy", "lazy-ordered"]
CLASSES = ("rc_doomed_fwd_hits", "rc_hits", "both_doomed", "rc_open_no_hit", "with_n")


@pytest.fixture
def mode(request, monkeypatch):
    lazy, order = request.param
    monkeypatch.setenv("HSA_SPLIT", "0")
    monkeypatch.setenv("HSA_LAZY", lazy)
    if order is None:
        monkeypatch.delenv("HSA_ORDER", raising=False)
    else:
        monkeypatch.setenv("HSA_ORDER", order)
    return request.param


def _searchable(r, od):
    """Not one of the reads bwa_cal_sa_reg_gap skips (bwtaln.c:314-325; test_gpu_implicit._check)."""
    return int((r > 3).sum()) <= od["max_diff"] and not (len(r) >= 15 and ((r[:15] == 0).all() or (r[:15] == 3).all()))


def _indel(r, rng):
    """One base deleted or inserted away from the read's ends, the length kept (a base is
    appended or dropped at the far end)."""
    p = int(rng.integers(20, len(r) - 20))
    if rng.integers(0, 2):
        return np.concatenate([r[:p], r[p + 1:], [np.uint8(rng.integers(0, 4))]]).astype(np.uint8)
    return np.concatenate([r[:p], [np.uint8(rng.integers(0, 4))], r[p:-1]]).astype(np.uint8)


def _mixture(codes, rng, n, od, indel=False):
    """n reads of every class in shuffled order: forward-origin and rc-origin 100-base
    reads with 0-4 substitutions, random 100-mers, forward-origin 36-44-base reads (their rc
    strand meets about three resets: not doomed at -n 4, and without a hit), and an N in every
    seventh read."""
    reads = []
    while len(reads) < n:
        k = len(reads) % 4
        if k < 2:
            r = _draw(codes, rng, 1, [100], 4, rc=False)[0]
            if indel and rng.integers(0, 2):
                r = _indel(r, rng)
            if k == 1:
                r = synth.revcomp_codes(r)
        elif k == 2:
            r = rng.integers(0, 4, 100).astype(np.uint8)
        else:
            r = _draw(codes, rng, 1, np.arange(36, 45), 1, rc=False)[0]
        if len(reads) % 7 == 3:
            r[int(rng.integers(0, len(r)))] = 4
        if _searchable(r, od):
            reads.append(r)
    order = rng.permutation(n)
    return [reads[i] for i in order]


def _classes(ox, reads, od, e_n, e_h):
    """Each read's classes from the oracle: a strand is doomed when the bid of its last base
    (bwt_cal_width, bwtaln.c:84-97) exceeds max_diff; the strand of a read's hits is bit 30 of
    their word 5."""
    md = od["max_diff"]
    rc_d = np.array([int(ox.cal_width(synth.revcomp_codes(r))[len(r) - 1, 1]) > md for r in reads])
    fw_d = np.array([int(ox.cal_width(r)[len(r) - 1, 1]) > md for r in reads])
    off = np.concatenate([[0], np.cumsum(np.maximum(e_n, 0))[:-1]])
    rc_hit = np.array([e_n[i] > 0 and (int(e_h[off[i], 5]) >> 30) & 1 == 1 for i in range(len(reads))])
    fw_hit = (e_n > 0) & ~rc_hit
    assert not (rc_d & rc_hit).any() and not (fw_d & fw_hit).any(), "a doomed strand has hits"
    return {"rc_doomed_fwd_hits": rc_d & fw_hit, "rc_hits": rc_hit, "both_doomed": rc_d & fw_d,
            "rc_open_no_hit": ~rc_d & ~rc_hit, "with_n": np.array([(r > 3).any() for r in reads]),
            "rc_doomed": rc_d, "fwd_doomed": fw_d}


def _expect(ox, reads, od):
    from oracle_ctypes import Opt
    lens = np.array([len(r) for r in reads], np.uint32)
    codes = np.concatenate(reads).astype(np.uint8)
    assert (lens > od["seed_len"]).all() or (lens <= od["seed_len"]).all()
    return lens, codes, ox.cal_sa_reg_gap(lens, codes, Opt.from_dict(od))


def _assert_classes(cls, at_least=8):
    for name in CLASSES:
        assert int(cls[name].sum()) >= at_least, (name, int(cls[name].sum()))


_POOL = {}


def _pool(kind="ungapped"):
    """The shared reads of a kind with the oracle's answer for every batch size, computed once."""
    if kind not in _POOL:
        S = _syn()
        od = _opts(4)
        if kind == "gapped":
            od.update(max_gapo=1)
        rng = np.random.default_rng({"ungapped": 101, "gapped": 102}[kind])
        reads = _mixture(S["codes"], rng, POOL if kind == "ungapped" else 320, od, indel=kind == "gapped")
        _POOL[kind] = dict(od=od, reads=reads, exp={})
    return _POOL[kind]


def _batch(kind, n):
    P = _pool(kind)
    if n not in P["exp"]:
        S = _syn()
        reads = P["reads"][:n]
        lens, codes, exp = _expect(S["ox"], reads, P["od"])
        P["exp"][n] = (lens, codes, exp, _classes(S["ox"], reads, P["od"], exp[0], exp[2]))
    return P["exp"][n]


def _both_doomed_fall_back(g, cls):
    """A read with both strands doomed: HSA_F_FALLBACK and no hit."""
    both = cls["both_doomed"]
    assert (g["n"][both] == 0).all() and ((g["f"][both] & 1) == 1).all()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS, indirect=True)
@pytest.mark.parametrize("n", SIZES)
def test_mixed_batches_match_the_oracle(n, mode):
    S = _syn()
    lens, codes, exp, cls = _batch("ungapped", n)
    _assert_classes(_batch("ungapped", POOL)[3])
    if n >= 255:
        _assert_classes(cls)
    g = _search(S["on"], lens, codes, _pool()["od"])
    assert g["c"][8] == 0 and g["c"][5] == 0
    _assert_device(g, exp)
    _both_doomed_fall_back(g, cls)


def test_both_doomed_reads_issue_no_search_query():
    """Random 100-mers alone: every strand doomed, so the whole search is each read's two root
    pops and the rank queries of its two width rows, the reference's counts."""
    S = _syn()
    od = _opts(4)
    rng = np.random.default_rng(103)
    reads = [r for r in (rng.integers(0, 4, 100).astype(np.uint8) for _ in range(80)) if _searchable(r, od)]
    lens, codes, exp = _expect(S["ox"], reads, od)
    cls = _classes(S["ox"], reads, od, exp[0], exp[2])
    assert cls["both_doomed"].all()
    assert int(exp[3][1]) == 2 * len(reads), exp[3]
    for lazy in ("0", "1"):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("HSA_SPLIT", "0")
            mp.setenv("HSA_LAZY", lazy)
            g = _search(S["on"], lens, codes, od)
        _assert_device(g, exp)
        assert int(g["c"][4]) == 2 * len(reads)
        assert int(g["c"][2]) == int(g["c"][7]), "rank queries beyond the width rows'"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS, indirect=True)
@pytest.mark.parametrize("doomed", [False, True], ids=["no-rc-row-doomed", "every-rc-row-doomed"])
def test_uniform_workgroups(doomed, mode):
    """A workgroup of 256 reads in which no rc row is doomed (rc-origin reads: k_widths_lazy
    computes no forward row, every wave leaves after the barrier) and one in which every rc row
    is (forward-origin reads: all 256 lanes compute a second row)."""
    S = _syn()
    od = _opts(4)
    rng = np.random.default_rng(104 + int(doomed))
    reads = []
    while len(reads) < 256:
        r = _draw(S["codes"], rng, 1, [100], 4, rc=False)[0]
        if not doomed:
            r = synth.revcomp_codes(r)
        rc_bid = int(S["ox"].cal_width(synth.revcomp_codes(r))[len(r) - 1, 1])
        if _searchable(r, od) and (rc_bid > od["max_diff"]) == doomed:
            reads.append(r)
    lens, codes, exp = _expect(S["ox"], reads, od)
    cls = _classes(S["ox"], reads, od, exp[0], exp[2])
    assert cls["rc_doomed"].all() if doomed else not cls["rc_doomed"].any()
    g = _search(S["on"], lens, codes, od)
    _assert_device(g, exp)


@pytest.mark.parametrize("mode", MODES[:2], ids=MODE_IDS[:2], indirect=True)
def test_reads_without_a_seed_row(mode):
    """Reads of at most seed_len bases (no seed row), in a batch of their own as the reference
    requires (bwtaln.c:332): at -n 1 the random ones are doomed on both strands."""
    S = _syn()
    od = _opts(1)
    rng = np.random.default_rng(106)
    reads = _draw(S["codes"], rng, 120, np.arange(20, od["seed_len"] + 1), 1)
    reads += [rng.integers(0, 4, int(L)).astype(np.uint8) for L in rng.integers(24, od["seed_len"] + 1, 80)]
    reads = [r for r in reads if _searchable(r, od)]
    lens, codes, exp = _expect(S["ox"], reads, od)
    cls = _classes(S["ox"], reads, od, exp[0], exp[2])
    for name in ("rc_doomed_fwd_hits", "rc_hits", "both_doomed"):
        assert int(cls[name].sum()) >= 8, (name, int(cls[name].sum()))
    g = _search(S["on"], lens, codes, od)
    _assert_device(g, exp)


@pytest.mark.parametrize("mode", MODES[:2], ids=MODE_IDS[:2], indirect=True)
def test_gapped_reads(mode):
    """-n 4 -o 1, half of the mapped reads with a one-base indel: the gapped kernels' begin_item."""
    S = _syn()
    lens, codes, exp, cls = _batch("gapped", 320)
    _assert_classes(cls)
    g = _search(S["on"], lens, codes, _pool("gapped")["od"])
    assert g["c"][8] == 0
    _assert_device(g, exp)


@pytest.mark.parametrize("mode", MODES[:2], ids=MODE_IDS[:2], indirect=True)
def test_64bit_index(mode):
    """hsa_search_device64 over the same text (the IT = uint64_t kernels)."""
    from oracle_ctypes import Opt
    from golden_io import split_hits
    from test_gpu_poollink import _wide_syn
    from test_gpu_wide import per_read, search
    W = _wide_syn()
    P = _pool()
    reads = P["reads"][:300]
    lens = np.array([len(r) for r in reads], np.uint32)
    codes = np.concatenate(reads).astype(np.uint8)
    if "exp64" not in P:
        P["exp64"] = W["ox"].cal_sa_reg_gap(lens, codes, Opt.from_dict(P["od"]))
    e_n, e_f, e_h, st = P["exp64"]
    _assert_classes(_batch("ungapped", 300)[3])
    n, f, o, h, c = search(W["gi"], lens, codes, P["od"], True)
    assert c[8] == 0
    assert np.array_equal(n, e_n) and np.array_equal(f & 1, e_f & 1)
    got, exp = per_read(n, o, h), split_hits(e_n, e_h)
    bad = [i for i in range(len(got)) if not np.array_equal(got[i], exp[i])]
    assert not bad, f"{len(bad)} reads differ from the 64-bit oracle; first {bad[0]}"
    assert int(c[2]) == int(st[0]), ("rank queries", int(c[2]), int(st[0]))
    assert int(c[4]) == int(st[1]), ("gap_pop count", int(c[4]), int(st[1]))


@pytest.mark.parametrize("mode", MODES[:2], ids=MODE_IDS[:2], indirect=True)
def test_overflow_cascade(mode):
    """pool_entries=64: the reads with a search of any size outgrow their MAIN lane and run again
    in the BIG pass, whose k_widths flags wq by the re-run list's positions.  (A re-run read counts
    its work twice, so the hits are compared and not the counts.)"""
    from hsa_amd._lib import configure
    S = _syn()
    lens, codes, exp, cls = _batch("ungapped", 257)
    configure(pool_entries=64)
    try:
        g = _search(S["on"], lens, codes, _pool()["od"])
    finally:
        configure(pool_entries=-1)
    assert g["c"][8] > 0, "no read took the BIG pass"
    _assert_device(g, exp, counts=False)
    _both_doomed_fall_back(g, cls)


@pytest.mark.parametrize("mode", MODES[1:], ids=MODE_IDS[1:], indirect=True)
def test_one_handle_changing_batch_sizes(mode):
    """A handle of its own searches 255, then 1 000, then 65 other reads: the row planes, rmap
    and wq move with the batch size inside the grown scratch, and nothing of an earlier batch
    may be read."""
    S = _syn()
    P = _pool()
    cl = S["on"].clone()
    try:
        for n, rev in ((255, False), (POOL, False), (65, True)):
            if rev:
                reads = P["reads"][::-1][:n]
                lens, codes, exp = _expect(S["ox"], reads, P["od"])
            else:
                lens, codes, exp, _ = _batch("ungapped", n)
            _assert_device(_search(cl, lens, codes, P["od"]), exp)
    finally:
        cl.close()


@pytest.mark.parametrize("mode", MODES[:2], ids=MODE_IDS[:2], indirect=True)
def test_clone_searches_concurrently(mode):
    """A clone and its parent search different batches at once, each on its own stream and
    scratch: both searches are queued before either is waited for."""
    import torch
    from hsa_amd._lib import JOB_DTYPE, DeviceBatch, GapOpt, pad_codes, regime_of
    S = _syn()
    P = _pool()
    od = P["od"]
    o = GapOpt.from_dict(od)
    rg = regime_of(od, (o.max_diff + 1) * o.s_mm + (o.max_gapo + 1) * o.s_gapo + (o.max_gape + 1) * o.s_gape, o.max_diff)
    cl = S["on"].clone()
    runs = []
    try:
        for ix, n in ((S["on"], 257), (cl, POOL)):
            lens, codes, exp, _ = _batch("ungapped", n)
            jobs = np.zeros(n, JOB_DTYPE)
            jobs["off"] = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]])
            jobs["len"] = lens
            jobs["max_diff"] = o.max_diff
            jobs["seed_len"] = np.where(lens > o.seed_len, o.seed_len, 0x7FFFFFFF)
            t = dict(j=torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), q=torch.from_numpy(pad_codes(codes)).cuda(),
                     n=torch.zeros(n, dtype=torch.int32, device="cuda"), f=torch.zeros(n, dtype=torch.int32, device="cuda"),
                     o=torch.zeros(n, dtype=torch.int64, device="cuda"),
                     h=torch.zeros(n * 64 * 9, dtype=torch.int32, device="cuda"),
                     c=torch.zeros(16, dtype=torch.int64, device="cuda"))
            runs.append((ix, lens, exp, t))
        torch.cuda.synchronize()
        for ix, lens, exp, t in runs:
            ix.search_device([rg], DeviceBatch(
                d_jobs=t["j"].data_ptr(), n_jobs=len(lens), d_codes=t["q"].data_ptr(), d_n_aln=t["n"].data_ptr(),
                d_flags=t["f"].data_ptr(), d_hit_off=t["o"].data_ptr(), d_hits=t["h"].data_ptr(), hit_cap=len(lens) * 64,
                d_counters=t["c"].data_ptr(), max_len=int(lens.max()), max_seed=o.seed_len))
        torch.cuda.synchronize()
    finally:
        cl.close()
    for ix, lens, exp, t in runs:
        g = dict(n=t["n"].cpu().numpy(), f=t["f"].cpu().numpy().astype(np.uint32), o=t["o"].cpu().numpy(),
                 h=t["h"].cpu().numpy().view(np.uint32).reshape(-1, 9), c=t["c"].cpu().numpy())
        assert g["c"][8] == 0
        _assert_device(g, exp)
