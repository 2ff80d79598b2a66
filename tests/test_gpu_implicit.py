"""k_search's implicit root levels (hsa_amd/csrc/hsa_trie.h): on the levels of the prepend
trie of which every string occurs in the text, an ungapped search carries node numbers
and takes no rank step.  Every search must equal the oracle's bit for bit -- hits, flags,
pops and the rank-query count -- whatever HSA_SDEPTH, and equal the same index built
with HSA_SDEPTH=0, with fewer rank sectors fetched."""
import ctypes as C
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from golden_io import INDEX, load_case, split_hits  # noqa: E402
from hsa_amd import index_io, synth  # noqa: E402
from test_gpu_trie import CASES  # noqa: E402

pytestmark = pytest.mark.gpu

SYN_T = 2_000_003          # i.i.d. text: every 8-mer occurs (30 expected copies), ~130 9-mers do not
SYN_SEED = 4242
SDEPTH_MAX = 13            # HSA_SDEPTH_MAX


def complete_depth(codes, cap=SDEPTH_MAX):
    """The deepest d <= cap with all 4^d strings of d characters in the text."""
    codes = np.asarray(codes, np.int64)
    d = 0
    while d < cap and 4 ** (d + 1) <= len(codes):
        n = len(codes) - d
        km = np.zeros(n, np.int64)
        for j in range(d + 1):
            km = km * 4 + codes[j:j + n]
        if len(np.unique(km)) != 4 ** (d + 1):
            break
        d += 1
    return d


@contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------- golden cases
_DEPTH = {}


def _golden_depth(genome):
    if genome not in _DEPTH:
        _DEPTH[genome] = complete_depth(index_io.read_pac(INDEX[genome]))
    return _DEPTH[genome]


@pytest.mark.parametrize("sd", [0, 1, 2, "complete", 15])
@pytest.mark.parametrize("case,args", CASES)
def test_golden_cases_match_oracle(case, args, sd):
    from hsa_amd._lib import GpuIndex
    from test_gpu_parity import _device_run
    genome = load_case(case)["index"]
    full = _golden_depth(genome)
    want = full if sd == "complete" else min(int(sd), full)
    with _env(HSA_SDEPTH=full if sd == "complete" else sd):
        ix = GpuIndex(*index_io.read_index(INDEX[genome]))
    try:
        assert ix.trie()[1] == want, (ix.trie(), want, full)
        got, (e_n, e_f, e_h, st) = _device_run(case, ix=ix, args=args)
    finally:
        ix.close()
    assert got["c"][11] == 0
    assert np.array_equal(got["f"] & 1, e_f & 1)
    assert np.array_equal(got["n"], e_n)
    exp = split_hits(e_n, e_h)
    bad = [i for i in range(len(exp)) if not np.array_equal(got["h"][got["o"][i]:got["o"][i] + max(got["n"][i], 0)],
                                                             exp[i])]
    assert not bad, f"{len(bad)} reads differ; first {bad[0]}"
    assert int(got["c"][2]) == int(st[0]), ("rank queries", int(got["c"][2]), int(st[0]))
    assert int(got["c"][4]) == int(st[1]), "gap_pop count"


# ---------------------------------------------------------------- built texts
def _build(codes):
    """Both BWTs of a text on the device: {rev: (codes tensor, isa0, C)} (bench.build_index's)."""
    import torch
    from hsa_amd._lib import check, lib
    T = len(codes)
    nw = (T + 15) // 16
    w = np.zeros(nw + 8, np.uint32)
    w[:nw] = index_io.pack_lsb_u32(codes)
    text = torch.from_numpy(w.view(np.int32)).cuda()
    res = {}
    for rev in (0, 1):
        bw = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
        isa0 = C.c_uint32()
        Cc = np.zeros(5, np.uint32)
        check(lib().hsa_build_bwt_device(0, T, text.data_ptr(), rev, bw.data_ptr(), C.byref(isa0), Cc))
        res[rev] = (bw, int(isa0.value), Cc)
    torch.cuda.synchronize()
    return res


def _gpu_index(res, T, sdepth=None):
    from hsa_amd._lib import GpuIndex
    env = {} if sdepth is None else {"HSA_SDEPTH": sdepth}
    with _env(**env):
        return GpuIndex.from_device_codes(T, res[0][1], res[0][2], res[0][0].data_ptr(), T, res[1][1], res[1][2],
                                          res[1][0].data_ptr())


_SYN = {}


def _syn():
    """The synthetic text, its index as built by default and with HSA_SDEPTH=0, the oracle's."""
    if not _SYN:
        import bench
        codes = synth.genome_codes(SYN_T, SYN_SEED)
        res = _build(codes)
        _SYN.update(codes=codes, depth=complete_depth(codes), on=_gpu_index(res, SYN_T), off=_gpu_index(res, SYN_T, 0),
                    ox=bench.host_oracle_index(res, SYN_T))
    return _SYN


def _search(ix, lens, codes, od):
    """One hsa_search_device call over reads of any lengths (test_gpu_parity._device_run's)."""
    import torch
    from hsa_amd._lib import JOB_DTYPE, DeviceBatch, GapOpt, pad_codes, regime_of
    n = len(lens)
    o = GapOpt.from_dict(od)
    n_stacks = (o.max_diff + 1) * o.s_mm + (o.max_gapo + 1) * o.s_gapo + (o.max_gape + 1) * o.s_gape
    rg = regime_of(od, n_stacks, o.max_diff)
    jobs = np.zeros(n, JOB_DTYPE)
    jobs["off"] = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]])
    jobs["len"] = lens
    jobs["max_diff"] = o.max_diff
    jobs["seed_len"] = np.where(lens > o.seed_len, o.seed_len, 0x7FFFFFFF)
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_codes = torch.from_numpy(pad_codes(codes)).cuda()
    cap = n * 64
    t = dict(n=torch.zeros(n, dtype=torch.int32, device="cuda"), f=torch.zeros(n, dtype=torch.int32, device="cuda"),
             o=torch.zeros(n, dtype=torch.int64, device="cuda"), h=torch.zeros(cap * 9, dtype=torch.int32, device="cuda"),
             c=torch.zeros(16, dtype=torch.int64, device="cuda"))
    b = DeviceBatch(d_jobs=d_jobs.data_ptr(), n_jobs=n, d_codes=d_codes.data_ptr(), d_n_aln=t["n"].data_ptr(),
                    d_flags=t["f"].data_ptr(), d_hit_off=t["o"].data_ptr(), d_hits=t["h"].data_ptr(), hit_cap=cap,
                    d_counters=t["c"].data_ptr(), max_len=int(lens.max()), max_seed=o.seed_len)
    ix.search_device([rg], b)
    torch.cuda.synchronize()
    return dict(n=t["n"].cpu().numpy(), f=t["f"].cpu().numpy().astype(np.uint32), o=t["o"].cpu().numpy(),
                h=t["h"].cpu().numpy().view(np.uint32).reshape(-1, 9), c=t["c"].cpu().numpy())


def _per_read(g):
    return [g["h"][g["o"][i]:g["o"][i] + max(int(g["n"][i]), 0)] for i in range(len(g["n"]))]


def _opts(max_diff):
    from oracle_ctypes import default_opt
    od = default_opt()
    od.update(max_diff=max_diff, fnr=-1.0, max_gapo=0)
    od["mode"] &= ~0x01
    return od


def _check(ix_on, ix_off, ox, reads, od, fewer_sectors=True):
    """reads: a list of code arrays.  The index with implicit levels against the oracle and
    against the index without them, every field."""
    from oracle_ctypes import Opt
    lens = np.array([len(r) for r in reads], np.uint32)
    codes = np.concatenate(reads).astype(np.uint8)
    # the device path searches every job it is given: none of these is one bwa_cal_sa_reg_gap
    # skips (bwtaln.c:314-325)
    # ... and reads of up to seed_len bases are not mixed with longer ones (in such a batch the
    # reference's seed length depends on the reads before, bwtaln.c:332)
    assert (lens > od["seed_len"]).all() or (lens <= od["seed_len"]).all()
    for r in reads:
        assert int((r > 3).sum()) <= od["max_diff"]
        assert not (len(r) >= 15 and ((r[:15] == 0).all() or (r[:15] == 3).all()))
    e_n, e_f, e_h, st = ox.cal_sa_reg_gap(lens, codes, Opt.from_dict(od))
    exp = split_hits(e_n, e_h)
    on = _search(ix_on, lens, codes, od)
    off = _search(ix_off, lens, codes, od)
    for name, g in (("implicit levels", on), ("HSA_SDEPTH=0", off)):
        assert g["c"][11] == 0 and g["c"][5] == 0, name
        assert np.array_equal(g["n"], e_n), name
        assert np.array_equal(g["f"] & 1, e_f & 1), name
        got = _per_read(g)
        bad = [i for i in range(len(exp)) if not np.array_equal(got[i], exp[i])]
        assert not bad, f"{name}: {len(bad)} reads differ; first {bad[0]} (length {lens[bad[0]]})"
        assert int(g["c"][2]) == int(st[0]), (name, "rank queries", int(g["c"][2]), int(st[0]))
        assert int(g["c"][4]) == int(st[1]), (name, "gap_pop count", int(g["c"][4]), int(st[1]))
    assert np.array_equal(on["f"], off["f"])
    assert np.array_equal(on["c"][[1, 2, 4, 7, 8, 11]], off["c"][[1, 2, 4, 7, 8, 11]])
    print(f"rank sectors: {int(on['c'][3])} with the implicit levels, {int(off['c'][3])} without; "
          f"{int((e_n > 0).sum())} of {len(reads)} reads with hits")
    if fewer_sectors:
        assert int(on["c"][3]) < int(off["c"][3]), "the implicit levels saved no rank sector"
    else:
        assert int(on["c"][3]) == int(off["c"][3])
    return e_n


def _draw(codes, rng, n, lens, max_mm, zone=None, n_at=None, rc=True):
    """n reads from the text: length drawn from lens, 0..max_mm substitutions (inside the
    last or first `zone` bases when given), an N at a position of that zone (n_at), half
    of them reverse-complemented."""
    out = []
    for i in range(n):
        L = int(rng.choice(lens))
        s = int(rng.integers(0, len(codes) - L))
        r = codes[s:s + L].copy()
        zn = min(zone, L) if zone else L
        where = np.arange(L - zn, L) if (zone is None or i % 2 == 0) else np.arange(zn)
        k = int(rng.integers(0, max_mm + 1))
        for p in rng.choice(where, size=min(k, len(where)), replace=False):
            r[p] = (r[p] + 1 + rng.integers(0, 3)) & 3
        if n_at:
            r[int(rng.choice(where))] = 4
        if rc and rng.integers(0, 2):
            r = synth.revcomp_codes(r)
        out.append(r)
    return out


def test_synthetic_complete_depth():
    S = _syn()
    assert 7 <= S["depth"] <= 8, S["depth"]
    assert S["on"].trie()[1] == S["depth"]
    assert S["off"].trie()[1] == 0


def test_synthetic_mismatch_reads():
    """36-50 bp, 0-4 substitutions anywhere, -n 4 -o 0, both strands."""
    S = _syn()
    rng = np.random.default_rng(1)
    reads = _draw(S["codes"], rng, 600, np.arange(36, 51), 4)
    e_n = _check(S["on"], S["off"], S["ox"], reads, _opts(4))
    # not a vacuous pass: the reads with at most 2 substitutions (3 in 5 of them) are within
    # the seed's limit (-k 2) wherever they fall, and map
    assert (e_n > 0).mean() > 0.5


def test_synthetic_substitutions_in_the_root_levels():
    """Every substitution inside the last (or first) Dc bases: the strings the implicit
    levels hold are the mismatched ones."""
    S = _syn()
    rng = np.random.default_rng(2)
    reads = _draw(S["codes"], rng, 400, [36, 41, 50], 4, zone=S["depth"])
    _check(S["on"], S["off"], S["ox"], reads, _opts(4))


def test_synthetic_n_in_the_root_levels():
    """An N inside the last (or first) Dc bases: all four children are mismatches there."""
    S = _syn()
    rng = np.random.default_rng(3)
    reads = _draw(S["codes"], rng, 400, [36, 44, 50], 2, zone=S["depth"], n_at=True)
    _check(S["on"], S["off"], S["ox"], reads, _opts(4))


def test_synthetic_reads_around_the_depth():
    """Reads of Dc - 1, Dc and Dc + 1 bases: only the last kind walks the implicit levels
    (its entries of Dc bases are explicit, one rank step from its hits)."""
    S = _syn()
    rng = np.random.default_rng(4)
    d = S["depth"]
    reads = []
    for L in (d - 1, d, d + 1, d + 2):
        reads += _draw(S["codes"], rng, 40, [L], 1)
    _check(S["on"], S["off"], S["ox"], reads, _opts(1))
    short = [r for r in reads if len(r) <= d]
    _check(S["on"], S["off"], S["ox"], short, _opts(1), fewer_sectors=False)


def test_synthetic_exact_reads():
    """-n 0: the root itself starts the exact tail (bwt_match_exact's write-back guard sees
    the root's zero k and rev_k), across the table into the rank steps.  (Reads of up to
    seed_len bases go in a batch of their own: in a batch with longer ones the reference's
    seed length depends on the reads before, bwtaln.c:332.)"""
    S = _syn()
    rng = np.random.default_rng(5)
    reads = _draw(S["codes"], rng, 300, [36, 50], 0)
    reads += _draw(S["codes"], rng, 100, [36, 50], 1)               # half of them: no exact match
    e_n = _check(S["on"], S["off"], S["ox"], reads, _opts(0))
    assert 0.5 < (e_n > 0).mean() < 1.0
    short = _draw(S["codes"], rng, 100, [S["depth"] + 1, S["depth"] + 2], 0)
    e_n = _check(S["on"], S["off"], S["ox"], short, _opts(0))
    assert (e_n > 0).all()


def test_synthetic_exact_tails_from_nodes():
    """-n 1 with the substitution inside the root levels: the mismatched child has no
    difference left and runs its exact tail from a node entry."""
    S = _syn()
    rng = np.random.default_rng(6)
    _check(S["on"], S["off"], S["ox"], _draw(S["codes"], rng, 300, [36, 44], 1, zone=S["depth"]), _opts(1))
    _check(S["on"], S["off"], S["ox"], _draw(S["codes"], rng, 100, [S["depth"] + 1, S["depth"] + 3], 1,
                                             zone=S["depth"]), _opts(1))


def test_clone_shares_the_levels():
    S = _syn()
    cl = S["on"].clone()
    try:
        assert cl.trie()[1] == S["depth"]
        rng = np.random.default_rng(7)
        reads = _draw(S["codes"], rng, 200, [36, 50], 4)
        _check(cl, S["off"], S["ox"], reads, _opts(4))
    finally:
        cl.close()


def test_text_missing_a_base_has_no_levels():
    """No T in the text: level 1 is not complete, the feature is off, results unchanged."""
    import bench
    rng = np.random.default_rng(8)
    T = 100_003
    codes = rng.integers(0, 3, T).astype(np.uint8)
    assert complete_depth(codes) == 0
    res = _build(codes)
    on, off = _gpu_index(res, T), _gpu_index(res, T, 0)
    try:
        assert on.trie()[1] == 0
        reads = _draw(codes, rng, 200, [36, 50], 3)
        _check(on, off, bench.host_oracle_index(res, T), reads, _opts(4), fewer_sectors=False)
    finally:
        on.close()
        off.close()
