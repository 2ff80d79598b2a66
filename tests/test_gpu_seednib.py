"""k_search's mixed row format (SeedFmt, hsa_search_kernels.h): the 8-bit read row without
element len, and a 4-bit seed row that k_widths writes to HBM already packed.  HSA_WFMT=seednib
forces it wherever it is exact (8-bit rows, max_seed_diff <= 6, rows of k_widths, not the HUGE
pass), so the golden cases and small built texts run through it; HSA_VERBOSE's launch line
shows that they did.  Every search must equal the oracle's bit for bit: hits, flags, hit
order, pops and the rank-query count."""
import numpy as np
import pytest

from golden_io import cases, load_case, parse_opts, split_hits
from test_gpu_implicit import _draw, _opts, _per_read, _search, _syn
from test_gpu_parity import _compare, _device_run

pytestmark = pytest.mark.gpu

TAG = "4-bit seed row"


@pytest.fixture
def seednib(monkeypatch):
    monkeypatch.setenv("HSA_WFMT", "seednib")
    monkeypatch.setenv("HSA_VERBOSE", "1")


def _eligible(name):
    """8-bit rows (every bid bound <= 14; an fnr-derived max_diff of the golden reads' lengths
    stays below that) and max_seed_diff <= 6."""
    from oracle_ctypes import default_opt
    o = parse_opts(load_case(name)["args"], default_opt())
    return o["max_diff"] <= 14 and o["max_seed_diff"] <= 6


def _launch_lines(err):
    return [ln for ln in err.splitlines() if ln.startswith("[hsa] launch:")]


# ---------------------------------------------------------------- golden cases
@pytest.mark.parametrize("name", sorted(cases().keys()))
def test_search_matches_reference_seednib(name, seednib, capfd):
    _compare(name)
    err = capfd.readouterr().err
    if _eligible(name):
        assert TAG in err, "the mixed format was not used"
    assert "4-bit rows" not in err


def _assert_device(got, exp_all, counts=True):
    e_n, e_f, e_h, st = exp_all
    assert got["c"][11] == 0, "reads left unfinished"
    assert np.array_equal(got["f"] & 1, e_f & 1)
    assert np.array_equal(got["n"], e_n)
    exp = split_hits(e_n, e_h)
    bad = [i for i in range(len(exp)) if not np.array_equal(got["h"][got["o"][i]:got["o"][i] + max(got["n"][i], 0)],
                                                             exp[i])]
    assert not bad, f"{len(bad)} reads differ; first {bad[0]}"
    if counts and got["c"][8] == 0:
        assert int(got["c"][2]) == int(st[0]), ("rank queries", int(got["c"][2]), int(st[0]))
        assert int(got["c"][4]) == int(st[1]), "gap_pop count"


@pytest.mark.parametrize("case", ["tiny_mm100_n4o0", "tiny_gap100_n4o1", "rep_mm100_n4o1", "tiny_edge_n3o1e3L"])
def test_device_path_seednib_matches_oracle(case, seednib, capfd):
    """hsa_search_device (the bench's path) under the mixed format: n_aln, flags, every hit
    word, and the rank-query and pop counts equal the oracle's."""
    got, exp = _device_run(case)
    assert TAG in capfd.readouterr().err
    _assert_device(got, exp)


def test_device_path_seednib_rerun_is_exact(seednib, capfd):
    """The BIG re-run pass uses the mixed format too (the HUGE pass keeps byte rows)."""
    got, exp = _device_run("tiny_gap100_n4o1", pool_entries=8)
    lines = _launch_lines(capfd.readouterr().err)
    assert len(lines) == 3 and TAG in lines[0] and TAG in lines[1] and TAG not in lines[2], lines
    assert got["c"][8] > 0 and got["c"][11] == 0
    _assert_device(got, exp, counts=False)


# ---------------------------------------------------------------- row-packing edges (built text)
def _check(ix, ox, reads, od, err_of=None, tag=True):
    """reads (a list of code arrays) through hsa_search_device on ix against the oracle:
    every field, the rank queries and the pops.  err_of: capfd, to see the launch line."""
    from oracle_ctypes import Opt
    lens = np.array([len(r) for r in reads], np.uint32)
    codes = np.concatenate(reads).astype(np.uint8)
    # (reads of up to seed_len bases are not mixed with longer ones: in such a batch the
    # reference's seed length depends on the reads before, bwtaln.c:332)
    assert (lens > od["seed_len"]).all() or (lens <= od["seed_len"]).all()
    for r in reads:
        assert int((r > 3).sum()) <= od["max_diff"]
        assert not (len(r) >= 15 and ((r[:15] == 0).all() or (r[:15] == 3).all()))
    e_n, e_f, e_h, st = ox.cal_sa_reg_gap(lens, codes, Opt.from_dict(od))
    if err_of is not None:
        err_of.readouterr()
    g = _search(ix, lens, codes, od)
    if err_of is not None:
        main = _launch_lines(err_of.readouterr().err)[0]
        assert (TAG in main) == tag, main
    assert g["c"][11] == 0 and g["c"][5] == 0
    assert np.array_equal(g["n"], e_n)
    assert np.array_equal(g["f"] & 1, e_f & 1)
    exp, got = split_hits(e_n, e_h), _per_read(g)
    bad = [i for i in range(len(exp)) if not np.array_equal(got[i], exp[i])]
    assert not bad, f"{len(bad)} reads differ; first {bad[0]} (length {lens[bad[0]]})"
    assert int(g["c"][2]) == int(st[0]), ("rank queries", int(g["c"][2]), int(st[0]))
    assert int(g["c"][4]) == int(st[1]), ("gap_pop count", int(g["c"][4]), int(st[1]))
    return e_n


def _seed_opts(seed_len, max_diff=4, **kw):
    od = _opts(max_diff)
    od.update(seed_len=seed_len, **kw)
    return od


@pytest.mark.parametrize("seed_len", [25, 31, 32, 33])
def test_seed_lengths_at_the_word_boundaries(seed_len, seednib, capfd):
    """Seeds of 25, 31, 32 and 33 bases (the nibble words' boundaries and the seed row's last
    element) under reads of seed_len + 1, 36, 50 and 100 bases, substitutions inside and
    outside the seed."""
    S = _syn()
    rng = np.random.default_rng(100 + seed_len)
    some = 0
    for L in sorted({seed_len + 1, 36, 50, 100}):
        if L <= seed_len:
            continue
        reads = _draw(S["codes"], rng, 100, [L], 4) + _draw(S["codes"], rng, 100, [L], 3, zone=seed_len)
        some += int((_check(S["on"], S["ox"], reads, _seed_opts(seed_len), capfd) > 0).sum())
    assert some > 100


def test_reads_without_a_seed_row(seednib, capfd):
    """len <= seed_len: no seed row is written or read."""
    S = _syn()
    rng = np.random.default_rng(11)
    reads = _draw(S["codes"], rng, 200, [20, 24, 31, 32], 2)
    _check(S["on"], S["ox"], reads, _seed_opts(32, 2), capfd)


def test_n_inside_and_beside_the_seed(seednib, capfd):
    """An N in the seed's last and first bases, and in the two bases just outside it (both
    strands: the seed is the strand sequence's last seed_len bases)."""
    S = _syn()
    rng = np.random.default_rng(12)
    sl, L = 32, 50
    reads = []
    for i, r in enumerate(_draw(S["codes"], rng, 200, [L], 2, rc=False)):
        p = [L - 1, L - sl, L - sl - 1, L - sl - 2, 0, sl - 1, sl, sl + 1][i % 8]
        r[p] = 4
        reads.append(r)
    _check(S["on"], S["ox"], reads, _seed_opts(sl), capfd)


def test_lengths_97_to_101_in_one_batch(seednib, capfd):
    """The read row's last LDS word with element len dropped: lengths around a multiple of 4."""
    S = _syn()
    rng = np.random.default_rng(13)
    reads = _draw(S["codes"], rng, 200, [97, 98, 99, 100, 101], 4)
    e_n = _check(S["on"], S["ox"], reads, _seed_opts(32), capfd)
    assert (e_n > 0).mean() > 0.3


@pytest.mark.parametrize("max_diff", [0, 1])
def test_exact_tails(max_diff, seednib, capfd):
    """-n 0 and -n 1: the exact tails read the read row's bases up to its last LDS word."""
    S = _syn()
    rng = np.random.default_rng(14 + max_diff)
    reads = _draw(S["codes"], rng, 200, [33, 50, 99, 100], max_diff)
    od = _seed_opts(32, max_diff, max_seed_diff=min(2, max_diff))
    e_n = _check(S["on"], S["ox"], reads, od, capfd)
    assert (e_n > 0).mean() > 0.5


def test_clone_searches_beside_its_parent(seednib):
    """A clone and its parent search different batches at once, each on its own stream:
    both searches are queued before either is waited for."""
    import torch
    from hsa_amd._lib import JOB_DTYPE, DeviceBatch, GapOpt, pad_codes, regime_of
    from oracle_ctypes import Opt
    S = _syn()
    rng = np.random.default_rng(16)
    od = _seed_opts(32)
    o = GapOpt.from_dict(od)
    rg = regime_of(od, (o.max_diff + 1) * o.s_mm + (o.max_gapo + 1) * o.s_gapo + (o.max_gape + 1) * o.s_gape, o.max_diff)
    cl = S["on"].clone()
    runs = []
    try:
        for ix, lens_of in ((S["on"], [50, 100]), (cl, [36, 99])):
            reads = _draw(S["codes"], rng, 200, lens_of, 4)
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
        exp, got = split_hits(e_n, e_h), _per_read(g)
        assert all(np.array_equal(a, b) for a, b in zip(got, exp))
        assert int(g["c"][2]) == int(st[0]) and int(g["c"][4]) == int(st[1])


# ---------------------------------------------------------------- fallback and off switch
def test_max_seed_diff_7_falls_back_to_byte_rows(seednib, capfd):
    """A bid bound of 7 does not fit min(bid, 7): the forced format is refused, exactly."""
    S = _syn()
    rng = np.random.default_rng(17)
    reads = _draw(S["codes"], rng, 200, [50, 100], 4)
    _check(S["on"], S["ox"], reads, _seed_opts(32, 4, max_seed_diff=7), capfd, tag=False)


def test_off_switch_gives_the_byte_rows_launch_line(monkeypatch, capfd):
    """HSA_WFMT=byte: the byte rows' layout, len / 4 + 1 and seed_len / 4 + 1 LDS words per lane
    (26 + 9 for 100 bp reads with a 32-base seed), after 240 B of tables and regimes and the 6
    bucket heads of 2 B per lane of -n 4 -o 0."""
    monkeypatch.setenv("HSA_WFMT", "byte")
    monkeypatch.setenv("HSA_VERBOSE", "1")
    got, exp = _device_run("tiny_mm100_n4o0")
    main = _launch_lines(capfd.readouterr().err)[0]
    assert TAG not in main and "4-bit rows" not in main, main
    _assert_device(got, exp)
    import re
    m = re.search(r"workgroups of (\d+) lanes .*LDS (\d+) B", main)
    nt, lds = int(m.group(1)), int(m.group(2))
    L = int(load_case("tiny_mm100_n4o0")["lens"].max())
    assert lds == (240 + nt * (6 * 2 + (L // 4 + 1) * 4 + 9 * 4) + 15) // 16 * 16, main
