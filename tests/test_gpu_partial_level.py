"""The table level of k_search's implicit root levels (hsa_amd/csrc/hsa_trie.h): the table
sits on the first level that need not be complete, one below the deepest complete level
Dc, and a string of it that does not occur is stored with the empty interval the rank step
computes.  The synthetic text of test_gpu_implicit has Dc = 8 and 127 absent 9-mers: the
reads here end in them (or begin with their reverse complements), so that exact tails and
mismatched children land on absent table nodes.  Every search must equal the oracle's bit
for bit -- hits in order, n_aln, flags, rank queries, pops -- and equal the same index built
with HSA_SPARTIAL=0 (the table on level Dc) and with HSA_SDEPTH=0 (no levels)."""
import numpy as np
import pytest

from golden_io import load_case, split_hits
from hsa_amd import index_io, synth
from test_gpu_implicit import (INDEX, SYN_T, _build, _draw, _env, _golden_depth, _gpu_index, _opts, _per_read, _search,
                               _syn)
from test_gpu_trie import CASES

pytestmark = pytest.mark.gpu

LEVEL = 9                  # the synthetic text's table level: Dc + 1
N_ABSENT = 127             # 9-mers the text lacks (CPU census below)
_P = {}


def census(codes, d):
    """The strings of d characters that do not occur in the text, as arrays of codes."""
    codes = np.asarray(codes, np.int64)
    n = len(codes) - d + 1
    km = np.zeros(n, np.int64)
    for j in range(d):
        km = km * 4 + codes[j:j + n]
    miss = np.setdiff1d(np.arange(4 ** d, dtype=np.int64), km)
    return [np.array([(int(v) >> (2 * (d - 1 - j))) & 3 for j in range(d)], np.uint8) for v in miss]


def _part():
    """The synthetic text's further indexes (HSA_SPARTIAL=0, HSA_SDEPTH=5) and its census."""
    if not _P:
        S = _syn()
        res = _build(S["codes"])
        with _env(HSA_SPARTIAL=0):
            p0 = _gpu_index(res, SYN_T)
        _P.update(res=res, p0=p0, sd5=_gpu_index(res, SYN_T, 5), absent=census(S["codes"], LEVEL))
    return _P


def _usable(r):
    """Not a read bwa_cal_sa_reg_gap skips (bwtaln.c:314-325)."""
    return len(r) < 15 or not ((r[:15] == 0).all() or (r[:15] == 3).all())


def _absent_reads(rng, tails=True, heads=True, lens=np.arange(36, 51)):
    """Per absent 9-mer: a read that ends in it (a text window, then the 9-mer) and one that
    begins with its reverse complement."""
    S, P = _syn(), _part()
    ends, begins = [], []
    for a in P["absent"]:
        for kind in (0, 1):
            while True:
                L = int(rng.choice(lens))
                s = int(rng.integers(0, SYN_T - L))
                w = S["codes"][s:s + L - LEVEL]
                r = np.concatenate([w, a]) if kind == 0 else np.concatenate([synth.revcomp_codes(a), w])
                r = r.astype(np.uint8)
                if _usable(r):
                    break
            (ends if kind == 0 else begins).append(r)
    return (ends if tails else []) + (begins if heads else []), len(ends), len(begins)


def _check3(reads, od, order=True):
    """The default index against the oracle, against HSA_SPARTIAL=0 and against HSA_SDEPTH=0:
    every field.  Returns the oracle's n_aln and the three sector counts."""
    from oracle_ctypes import Opt
    S, P = _syn(), _part()
    lens = np.array([len(r) for r in reads], np.uint32)
    codes = np.concatenate(reads).astype(np.uint8)
    assert (lens > od["seed_len"]).all() or (lens <= od["seed_len"]).all()
    for r in reads:
        assert int((r > 3).sum()) <= od["max_diff"] and _usable(r)
    e_n, e_f, e_h, st = S["ox"].cal_sa_reg_gap(lens, codes, Opt.from_dict(od))
    exp = split_hits(e_n, e_h)
    runs = [(name, _search(ix, lens, codes, od))
            for name, ix in (("default", S["on"]), ("HSA_SPARTIAL=0", P["p0"]), ("HSA_SDEPTH=0", S["off"]))]
    for name, g in runs:
        assert g["c"][11] == 0 and g["c"][5] == 0, name
        assert np.array_equal(g["n"], e_n), name
        assert np.array_equal(g["f"] & 1, e_f & 1), name
        got = _per_read(g)
        bad = [i for i in range(len(exp)) if not np.array_equal(got[i], exp[i])]
        assert not bad, f"{name}: {len(bad)} reads differ; first {bad[0]} (length {lens[bad[0]]})"
        assert int(g["c"][2]) == int(st[0]), (name, "rank queries", int(g["c"][2]), int(st[0]))
        assert int(g["c"][4]) == int(st[1]), (name, "gap_pop count", int(g["c"][4]), int(st[1]))
        assert np.array_equal(g["f"], runs[0][1]["f"]), name
        assert np.array_equal(g["c"][[1, 2, 4, 7, 8, 11]], runs[0][1]["c"][[1, 2, 4, 7, 8, 11]]), name
    sec = [int(g["c"][3]) for _, g in runs]
    print(f"rank sectors: {sec[0]} default, {sec[1]} with HSA_SPARTIAL=0, {sec[2]} with HSA_SDEPTH=0; "
          f"{int((e_n > 0).sum())} of {len(reads)} reads with hits")
    if order:
        assert sec[0] < sec[1] < sec[2], sec
    return e_n, sec


# ---------------------------------------------------------------- builder
def test_census_of_the_synthetic_text():
    S, P = _syn(), _part()
    assert S["depth"] == LEVEL - 1
    assert len(P["absent"]) == N_ABSENT
    assert not census(S["codes"], LEVEL - 1)


def test_builder_levels():
    S, P = _syn(), _part()
    assert S["on"].trie()[1] == LEVEL - 1 and S["on"].levels() == (LEVEL, N_ABSENT)
    assert P["p0"].trie()[1] == LEVEL - 1 and P["p0"].levels() == (LEVEL - 1, 0)
    assert P["sd5"].trie()[1] == 5 and P["sd5"].levels() == (6, 0)
    assert S["off"].trie()[1] == 0 and S["off"].levels() == (0, 0)
    cl = S["on"].clone()
    try:
        assert cl.trie()[1] == LEVEL - 1 and cl.levels() == (LEVEL, N_ABSENT)
    finally:
        cl.close()


def test_text_missing_a_base_has_no_table():
    rng = np.random.default_rng(8)
    T = 100_003
    codes = rng.integers(0, 3, T).astype(np.uint8)
    ix = _gpu_index(_build(codes), T)
    try:
        assert ix.trie()[1] == 0 and ix.levels() == (0, 0)
    finally:
        ix.close()


def test_capped_depth_builds_a_complete_table_level():
    """HSA_SDEPTH=5: five load-free levels and the (complete) table on level 6."""
    from oracle_ctypes import Opt
    S, P = _syn(), _part()
    rng = np.random.default_rng(21)
    reads = _draw(S["codes"], rng, 200, np.arange(36, 51), 2, zone=6)
    reads += _absent_reads(rng)[0][::8]
    lens = np.array([len(r) for r in reads], np.uint32)
    codes = np.concatenate(reads).astype(np.uint8)
    od = _opts(2)
    e_n, e_f, e_h, st = S["ox"].cal_sa_reg_gap(lens, codes, Opt.from_dict(od))
    g, off = _search(P["sd5"], lens, codes, od), _search(S["off"], lens, codes, od)
    assert g["c"][11] == 0 and np.array_equal(g["n"], e_n) and np.array_equal(g["f"], off["f"])
    assert all(np.array_equal(a, b) for a, b in zip(_per_read(g), split_hits(e_n, e_h)))
    assert int(g["c"][2]) == int(st[0]) and int(g["c"][4]) == int(st[1])
    assert np.array_equal(g["c"][[1, 2, 4, 7, 8, 11]], off["c"][[1, 2, 4, 7, 8, 11]])
    assert int(g["c"][3]) < int(off["c"][3])


# ---------------------------------------------------------------- absent nodes
@pytest.mark.parametrize("max_diff", [0, 1, 2])
def test_reads_on_absent_nodes(max_diff):
    """Reads that end in an absent 9-mer or begin with its reverse complement: the matching
    child of the level-8 node is absent in the table, the mismatched ones go on (-n 1, -n 2).
    At -n 0 no such read can match, and none is searched at all: its width row already
    demands a difference (bid 1 at the last base), so the strand's root is pruned and the
    three indexes fetch the same sectors, all of them k_widths'."""
    rng = np.random.default_rng(30 + max_diff)
    reads, n_end, n_begin = _absent_reads(rng)
    assert n_end >= N_ABSENT and n_begin >= N_ABSENT
    e_n, sec = _check3(reads, _opts(max_diff), order=max_diff > 0)
    if max_diff == 0:
        assert (e_n == 0).all()       # a read holding a string the text lacks has no exact match
        assert sec[0] == sec[1] == sec[2], sec


@pytest.mark.parametrize("max_diff", [1, 2])
def test_exact_tails_die_on_absent_nodes(max_diff):
    """The same reads with one base of the absent 9-mer substituted: the search's mismatched
    child that restores the 9-mer has (at -n 1) no difference left, runs its exact tail from a
    node entry and reaches the table level on an absent node (bwt_match_exact's empty
    interval, 2BWT-Interface.c:378-382): no hit, the failing step's two queries counted."""
    rng = np.random.default_rng(35 + max_diff)
    reads, n_end, n_begin = _absent_reads(rng)
    assert n_end >= N_ABSENT and n_begin >= N_ABSENT
    for i, r in enumerate(reads):
        j = i % LEVEL
        p = len(r) - 1 - j if i < n_end else j
        r[p] = (r[p] + 1 + i % 3) & 3
    _check3([r for r in reads if _usable(r)], _opts(max_diff))


@pytest.mark.parametrize("max_diff", [1, 2])
def test_substitutions_around_the_table_level(max_diff):
    """Substitutions inside the last (or first) 9 bases: mismatched children fall on absent
    nodes by chance, and exact tails start from node entries."""
    S = _syn()
    rng = np.random.default_rng(40 + max_diff)
    reads = _draw(S["codes"], rng, 400, [36, 41, 50], max_diff, zone=LEVEL)
    e_n, _ = _check3(reads, _opts(max_diff))
    assert (e_n > 0).mean() > 0.5


@pytest.mark.parametrize("max_diff", [0, 1])
def test_reads_of_9_10_and_11_bases(max_diff):
    """A read of exactly 9 bases is not longer than the table's level and walks the rank
    steps; 10 and 11 bases leave the table one or two steps before their hits.  Text reads,
    the absent 9-mers themselves, and 10- and 11-base reads around them."""
    S, P = _syn(), _part()
    rng = np.random.default_rng(50 + max_diff)
    reads = []
    for L in (LEVEL, LEVEL + 1, LEVEL + 2):
        reads += _draw(S["codes"], rng, 40, [L], max_diff)
        if L > LEVEL:
            reads += _absent_reads(rng, lens=[L])[0][::4]
    reads += P["absent"][::4]
    _, sec = _check3(reads, _opts(max_diff), order=False)
    assert sec[0] < sec[2], sec
    _check3([r for r in reads if len(r) > LEVEL], _opts(max_diff))
    nine = [r for r in reads if len(r) == LEVEL]
    _, sec = _check3(nine, _opts(max_diff), order=False)
    assert sec[1] < sec[0] == sec[2], sec      # (with the table on level 8 a 9-base read walks the levels)


# ---------------------------------------------------------------- golden cases, the BIG pass
@pytest.mark.parametrize("case,args", CASES)
def test_golden_cases_with_the_table_on_the_complete_level(case, args):
    from hsa_amd._lib import GpuIndex
    from test_gpu_parity import _device_run
    genome = load_case(case)["index"]
    full = _golden_depth(genome)
    with _env(HSA_SPARTIAL=0):
        ix = GpuIndex(*index_io.read_index(INDEX[genome]))
    try:
        assert ix.trie()[1] == full and ix.levels() == (full, 0)
        got, (e_n, e_f, e_h, st) = _device_run(case, ix=ix, args=args)
    finally:
        ix.close()
    assert got["c"][11] == 0
    assert np.array_equal(got["f"] & 1, e_f & 1)
    assert np.array_equal(got["n"], e_n)
    got_h = [got["h"][got["o"][i]:got["o"][i] + max(got["n"][i], 0)] for i in range(len(e_n))]
    assert all(np.array_equal(a, b) for a, b in zip(got_h, split_hits(e_n, e_h)))
    assert int(got["c"][2]) == int(st[0]) and int(got["c"][4]) == int(st[1])


def test_big_rerun_on_the_partial_table():
    """With 8 pool entries per lane the -n 4 reads overflow the main pass and are searched
    again by the BIG pass, which walks the implicit levels and the table too."""
    from hsa_amd._lib import configure
    from oracle_ctypes import Opt
    S = _syn()
    rng = np.random.default_rng(60)
    reads = _draw(S["codes"], rng, 100, [50], 4, zone=LEVEL) + _absent_reads(rng, lens=[50])[0][::4]
    lens = np.array([len(r) for r in reads], np.uint32)
    codes = np.concatenate(reads).astype(np.uint8)
    od = _opts(4)
    e_n, e_f, e_h, st = S["ox"].cal_sa_reg_gap(lens, codes, Opt.from_dict(od))
    configure(pool_entries=8)
    try:
        g = _search(S["on"], lens, codes, od)
    finally:
        configure(pool_entries=-1)
    assert g["c"][8] > 0 and g["c"][11] == 0
    assert np.array_equal(g["n"], e_n) and np.array_equal(g["f"] & 1, e_f & 1)
    assert all(np.array_equal(a, b) for a, b in zip(_per_read(g), split_hits(e_n, e_h)))


def test_golden_case_through_the_big_rerun():
    from hsa_amd._lib import GpuIndex
    from test_gpu_parity import _device_run
    ix = GpuIndex(*index_io.read_index(INDEX[load_case("tiny_gap100_n4o1")["index"]]))
    try:
        got, (e_n, e_f, e_h, st) = _device_run("tiny_gap100_n4o1", pool_entries=8, ix=ix, args="-n 4 -o 0")
    finally:
        ix.close()
    assert got["c"][8] > 0 and got["c"][11] == 0
    assert np.array_equal(got["n"], e_n) and np.array_equal(got["f"] & 1, e_f & 1)
    got_h = [got["h"][got["o"][i]:got["o"][i] + max(got["n"][i], 0)] for i in range(len(e_n))]
    assert all(np.array_equal(a, b) for a, b in zip(got_h, split_hits(e_n, e_h)))


# ---------------------------------------------------------------- the shared table
def test_clone_and_parent_search_the_shared_table_at_once():
    """A clone and its parent search different batches at once, each on its own stream: both
    searches are queued before either is waited for."""
    import torch
    from hsa_amd._lib import JOB_DTYPE, DeviceBatch, GapOpt, pad_codes, regime_of
    from oracle_ctypes import Opt
    S = _syn()
    rng = np.random.default_rng(70)
    od = _opts(2)
    o = GapOpt.from_dict(od)
    rg = regime_of(od, (o.max_diff + 1) * o.s_mm + (o.max_gapo + 1) * o.s_gapo + (o.max_gape + 1) * o.s_gape, o.max_diff)
    cl = S["on"].clone()
    runs = []
    try:
        for ix, lens_of in ((S["on"], [36, 50]), (cl, [41, 47])):
            reads = _draw(S["codes"], rng, 136, lens_of, 2, zone=LEVEL) + _absent_reads(rng, lens=lens_of)[0][::4]
            assert len(reads) == 200
            lens = np.array([len(r) for r in reads], np.uint32)
            codes = np.concatenate(reads).astype(np.uint8)
            n = len(lens)
            jobs = np.zeros(n, JOB_DTYPE)
            jobs["off"] = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]])
            jobs["len"] = lens
            jobs["max_diff"] = o.max_diff
            jobs["seed_len"] = o.seed_len
            t = dict(j=torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), q=torch.from_numpy(pad_codes(codes)).cuda(),
                     n=torch.zeros(n, dtype=torch.int32, device="cuda"), f=torch.zeros(n, dtype=torch.int32, device="cuda"),
                     o=torch.zeros(n, dtype=torch.int64, device="cuda"),
                     h=torch.zeros(n * 64 * 9, dtype=torch.int32, device="cuda"),
                     c=torch.zeros(16, dtype=torch.int64, device="cuda"))
            runs.append((ix, lens, codes, t))
        torch.cuda.synchronize()
        for ix, lens, codes, t in runs:
            ix.search_device([rg], DeviceBatch(
                d_jobs=t["j"].data_ptr(), n_jobs=len(lens), d_codes=t["q"].data_ptr(), d_n_aln=t["n"].data_ptr(),
                d_flags=t["f"].data_ptr(), d_hit_off=t["o"].data_ptr(), d_hits=t["h"].data_ptr(), hit_cap=len(lens) * 64,
                d_counters=t["c"].data_ptr(), max_len=int(lens.max()), max_seed=o.seed_len))
        torch.cuda.synchronize()
    finally:
        cl.close()
    for ix, lens, codes, t in runs:
        e_n, e_f, e_h, st = S["ox"].cal_sa_reg_gap(lens, codes, Opt.from_dict(od))
        g = dict(n=t["n"].cpu().numpy(), f=t["f"].cpu().numpy().astype(np.uint32), o=t["o"].cpu().numpy(),
                 h=t["h"].cpu().numpy().view(np.uint32).reshape(-1, 9), c=t["c"].cpu().numpy())
        assert g["c"][11] == 0 and np.array_equal(g["n"], e_n) and np.array_equal(g["f"] & 1, e_f & 1)
        assert all(np.array_equal(a, b) for a, b in zip(_per_read(g), split_hits(e_n, e_h)))
        assert int(g["c"][2]) == int(st[0]) and int(g["c"][4]) == int(st[1])
