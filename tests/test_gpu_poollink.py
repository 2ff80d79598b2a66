"""k_search's pool entries that carry their own bucket-list link (LK, hsa_search_kernels.h):
every pass but HUGE of the 64-bit kernels, and of the 32-bit ungapped kernels with 8-bit,
mixed or 4-bit rows, keeps the link in the entry (the meta word's upper half, or the 64-bit
entry's spare word) and reserves no link array; a pop loads one sector, a push stores once.
The gapped 32-bit kernels, the 16-bit rows and the HUGE pass keep the array.  HSA_VERBOSE's
launch line says which a pass runs.  Every search must equal the oracle's bit for bit: hits,
flags, n_aln, the rank-query count and the pop count."""
import numpy as np
import pytest

from golden_io import INDEX, cases, parse_opts, split_hits
from hsa_amd import index_io
from test_gpu_implicit import _build, _draw, _opts, _search, _syn
from test_gpu_parity import _compare, _device_run
from test_gpu_seednib import _assert_device, _launch_lines

pytestmark = pytest.mark.gpu

TAG = "links in the entries"


@pytest.fixture
def verbose(monkeypatch):
    monkeypatch.setenv("HSA_VERBOSE", "1")


# the defaults of the two options that decide it (gap_init_opt: -n from fnr, -o 1); read from the
# cases' arguments alone, so collecting this file loads no library
_BASE = {"max_diff": -1, "fnr": 0.04, "max_gapo": 1, "mode": 0}


def _case_opts(name):
    return parse_opts(cases()[name]["args"], _BASE)


def _ungapped(name):
    """The golden cases the drop-in searches without gap opens: a fixed -n with -o 0, or -n 0
    (the drop-in lowers max_gapo to max_diff, bwtaln.c:275)."""
    o = _case_opts(name)
    return o["max_diff"] >= 0 and min(o["max_gapo"], o["max_diff"]) == 0


UNGAPPED = [n for n in sorted(cases().keys()) if _ungapped(n)]


def _device_args(name):
    """The case's options with the drop-in's clamp applied (the device path takes max_gapo as given)."""
    a = list(cases()[name]["args"])
    return " ".join(a if "-o" in a else a + ["-o", "0"])


def test_the_ungapped_cases():
    assert "tiny_mm100_n4o0" in UNGAPPED and "tiny_exact36_n0" in UNGAPPED, UNGAPPED


# ---------------------------------------------------------------- golden cases
@pytest.mark.parametrize("name", UNGAPPED)
def test_dropin_ungapped_matches_reference(name, verbose, capfd):
    """The drop-in on every ungapped golden case.  Its first regime takes the options as given
    (the reference's opt before the first fallback, bwtaln.c:261), so a case without -o 0
    (tiny_exact36_n0: -n 0, max_gapo still 1 there) runs the gapped 32-bit kernel, which keeps
    the link array; with -o 0 every k_search pass but HUGE names the entry links."""
    _compare(name)
    lines = _launch_lines(capfd.readouterr().err)
    assert lines
    if _case_opts(name)["max_gapo"] == 0:
        assert any(TAG in ln for ln in lines), "no pass kept its links in the entries"
    else:
        assert not any(TAG in ln for ln in lines), lines


@pytest.mark.parametrize("name", UNGAPPED)
def test_device_path_ungapped_matches_oracle(name, verbose, capfd):
    got, exp = _device_run(name, args=_device_args(name))
    lines = _launch_lines(capfd.readouterr().err)
    assert TAG in lines[0] and TAG in lines[1] and TAG not in lines[2], lines      # MAIN, BIG; HUGE keeps the array
    assert got["c"][8] == 0
    _assert_device(got, exp)


def test_big_rerun_keeps_links_in_the_entries(verbose, capfd):
    """pool_entries=8: most reads overflow their MAIN lane and finish in the BIG pass, whose
    entries carry their links too."""
    got, exp = _device_run("tiny_mm100_n4o0", pool_entries=8)
    lines = _launch_lines(capfd.readouterr().err)
    assert len(lines) == 3 and TAG in lines[0] and TAG in lines[1] and TAG not in lines[2], lines
    assert got["c"][8] > 0 and got["c"][11] == 0
    _assert_device(got, exp, counts=False)


def test_deepest_ungapped_stack_of_the_fixtures(verbose, capfd):
    """The repeat genome's 100 bp reads under -n 4 -o 0 with pool_entries=8, so nearly every
    read builds its whole stack in the BIG pass, where slots are numbered up to 65 534.  The
    costliest of these reads pops 1 187 entries over both strands (the oracle, one read at a
    time) and an ungapped expansion pushes at most 4, so its slot numbers stay below 4 748:
    slot 32 768 (the link's high bit) is NOT reached by any fixture.  The static_assert round
    trips beside meta_link_pack cover links 0x8000, 0xFFFE and NIL16."""
    got, exp = _device_run("rep_mm100_n4o1", args="-n 4 -o 0", pool_entries=8)
    lines = _launch_lines(capfd.readouterr().err)
    assert TAG in lines[0] and TAG in lines[1], lines
    assert got["c"][8] > 0 and got["c"][11] == 0
    _assert_device(got, exp, counts=False)


# ---------------------------------------------------------------- kernels that keep the link array
@pytest.mark.parametrize("case,args", [("tiny_gap100_n4o1", None), ("tiny_mm100_n4o0", "-n 15 -o 0")])
def test_link_array_kernels_are_unchanged(case, args, verbose, capfd):
    """A gapped 32-bit search (full meta word), and an ungapped one whose max_diff of 15 selects
    the 16-bit rows: neither launch line names entry links, both equal the oracle."""
    got, exp = _device_run(case, args=args)
    lines = _launch_lines(capfd.readouterr().err)
    assert lines and not any(TAG in ln for ln in lines), lines
    _assert_device(got, exp)


# ---------------------------------------------------------------- 64-bit intervals, small built text
_W = {}


def _wide_syn():
    """test_gpu_implicit's 2 Mbp text as a 64-bit index (hsa_index_create_device64) and the
    64-bit restatement's index over the same BWT words."""
    if not _W:
        from hsa_amd._lib import GpuIndex
        from oracle_ctypes import OracleIndex64
        S = _syn()
        T = len(S["codes"])
        res = _build(S["codes"])
        nw = (T + 15) // 16
        C64 = [np.asarray(res[r][2], np.uint64) for r in (0, 1)]
        gi = GpuIndex.from_device_codes64(T, res[0][1], C64[0], res[0][0].data_ptr(), T, res[1][1], C64[1],
                                          res[1][0].data_ptr())
        host = [res[r][0][:nw].cpu().numpy().view(np.uint32) for r in (0, 1)]
        _W.update(gi=gi, keep=res, codes=S["codes"],
                  ox=OracleIndex64(T, res[0][1], C64[0], host[0], T, res[1][1], C64[1], host[1]))
    return _W


def _wide_reads(kind):
    W = _wide_syn()
    rng = np.random.default_rng({"ungapped": 21, "gapped": 22, "nib250": 23}[kind])
    if kind == "nib250":
        return _draw(W["codes"], rng, 150, [250], 4), dict(_opts(4)), "4-bit rows"
    od = _opts(4)
    if kind == "gapped":
        od.update(max_gapo=1)
    return _draw(W["codes"], rng, 200, [50, 99, 100], 4), od, None


@pytest.mark.parametrize("pool_entries", [0, 8])
@pytest.mark.parametrize("kind", ["ungapped", "gapped", "nib250"])
def test_wide_kernels_match_the_64bit_oracle(kind, pool_entries, verbose, monkeypatch, capfd):
    """hsa_search_device64 over the built text: ungapped reads, -o 1 reads, and 250-base reads for
    which the planner picks the 4-bit rows, all with their links in the entries (MAIN and BIG);
    every hsa_aln64_t word, the flags and both counts equal the 64-bit oracle's.  pool_entries=8:
    the same through the BIG re-run (a re-run read counts its work twice, so hits only)."""
    from hsa_amd._lib import configure
    from oracle_ctypes import Opt
    from test_gpu_wide import per_read, search
    monkeypatch.delenv("HSA_WFMT", raising=False)
    W = _wide_syn()
    reads, od, rows = _wide_reads(kind)
    lens = np.array([len(r) for r in reads], np.uint32)
    codes = np.concatenate(reads).astype(np.uint8)
    e_n, e_f, e_h, st = W["ox"].cal_sa_reg_gap(lens, codes, Opt.from_dict(od))
    capfd.readouterr()
    if pool_entries:
        configure(pool_entries=pool_entries)
    try:
        n, f, o, h, c = search(W["gi"], lens, codes, od, True)
    finally:
        if pool_entries:
            configure(pool_entries=-1)
    lines = _launch_lines(capfd.readouterr().err)
    assert TAG in lines[0] and TAG in lines[1] and TAG not in lines[2], lines
    if rows:
        assert rows in lines[0], lines[0]
    assert np.array_equal(n, e_n) and np.array_equal(f & 1, e_f & 1)
    got, exp = per_read(n, o, h), split_hits(e_n, e_h)
    bad = [i for i in range(len(got)) if not np.array_equal(got[i], exp[i])]
    assert not bad, f"{len(bad)} reads differ from the 64-bit oracle; first {bad[0]}"
    assert (e_n > 0).mean() > 0.3
    if pool_entries:
        assert c[8] > 0, "no read took the BIG pass"
    else:
        assert c[8] == 0
        assert int(c[2]) == int(st[0]), ("rank queries", int(c[2]), int(st[0]))
        assert int(c[4]) == int(st[1]), ("gap_pop count", int(c[4]), int(st[1]))


# ---------------------------------------------------------------- implicit levels
@pytest.mark.parametrize("pool_entries", [64, 8])
def test_node_entries_through_the_pool(pool_entries, verbose, capfd):
    """Reads of Dc - 1 .. Dc + 2 bases under -n 1 on the 2 Mbp text (Dc: the complete depth of the
    implicit levels): the mismatch children of the root levels are node-number entries, and all
    but the virtual top go through the pool, packed and unpacked.  64 slots hold a strand's
    pushes (3 per level), so the MAIN pass finishes every read and both counts are compared; 8
    sends them through the BIG pass as well."""
    from hsa_amd._lib import configure
    from oracle_ctypes import Opt
    S = _syn()
    rng = np.random.default_rng(31)
    d = S["depth"]
    reads = []
    for L in (d - 1, d, d + 1, d + 2):
        reads += _draw(S["codes"], rng, 60, [L], 1)
    od = _opts(1)
    lens = np.array([len(r) for r in reads], np.uint32)
    codes = np.concatenate(reads).astype(np.uint8)
    exp = S["ox"].cal_sa_reg_gap(lens, codes, Opt.from_dict(od))
    capfd.readouterr()
    configure(pool_entries=pool_entries)
    try:
        g = _search(S["on"], lens, codes, od)
    finally:
        configure(pool_entries=-1)
    lines = _launch_lines(capfd.readouterr().err)
    assert TAG in lines[0] and TAG in lines[1], lines
    assert (g["c"][8] == 0) == (pool_entries == 64), int(g["c"][8])
    _assert_device(g, exp)                       # (compares the counts when no read was re-run)
    assert (exp[0] > 0).all()


# ---------------------------------------------------------------- scratch: passes with and without a link array
def test_one_handle_alternates_link_layouts(monkeypatch, capfd):
    """A fresh handle runs an ungapped search (no link array reserved), a gapped one that reaches
    the HUGE pass (the MAIN and BIG scratch gain their link arrays beside the pools they hold;
    HUGE has 32-bit links), then the ungapped one again on the scratch that now has an array.
    Once it has run each kind, the same searches allocate nothing: HSA_VERBOSE=2 logs every
    scratch allocation, and none appears."""
    from hsa_amd._lib import GpuIndex
    monkeypatch.setenv("HSA_VERBOSE", "2")
    ix = GpuIndex(*index_io.read_index(INDEX["rep"]))
    ungapped, huge, gapped = ("rep_mm100_n4o1", "-n 4 -o 0", 8), ("rep_deep_n6o2N", None, 0), ("rep_mm100_n4o1", None, 8)
    logged = []
    try:
        for rnd, runs in enumerate(((ungapped, huge, ungapped, gapped), (ungapped, gapped, ungapped))):
            for case, args, pe in runs:
                capfd.readouterr()
                got, exp = _device_run(case, args=args, pool_entries=pe, ix=ix)
                alloc = [ln for ln in capfd.readouterr().err.splitlines() if "search scratch" in ln]
                assert got["c"][11] == 0, (case, args)
                if case == "rep_deep_n6o2N":
                    assert got["c"][12] > 0, "no read reached the huge pass"
                _assert_device(got, exp, counts=False)
                if rnd == 0:
                    logged += alloc
                else:
                    assert not alloc, alloc
        assert any("search scratch pool" in ln for ln in logged), "HSA_VERBOSE=2 logged no pool allocation"
    finally:
        ix.close()


# ---------------------------------------------------------------- a clone beside its parent
def test_clone_searches_beside_its_parent():
    """A clone and its parent search different ungapped batches at once, each on its own stream
    and its own scratch: both searches are queued before either is waited for."""
    import torch
    from hsa_amd._lib import JOB_DTYPE, DeviceBatch, GapOpt, pad_codes, regime_of
    from oracle_ctypes import Opt
    S = _syn()
    rng = np.random.default_rng(41)
    od = _opts(4)
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
        exp = S["ox"].cal_sa_reg_gap(lens, codes, Opt.from_dict(od))
        g = dict(n=t["n"].cpu().numpy(), f=t["f"].cpu().numpy().astype(np.uint32), o=t["o"].cpu().numpy(),
                 h=t["h"].cpu().numpy().view(np.uint32).reshape(-1, 9), c=t["c"].cpu().numpy())
        assert g["c"][8] == 0
        _assert_device(g, exp)
