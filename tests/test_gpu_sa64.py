"""Text positions on the 64-bit path: the sampled suffix array of a 64-bit text
(hsa_build_bwt_index_device64), SA index -> position (hsa_sa_position_*64, one LF step:
hsa_psi_minus_batch64) and the hit lists of hsa_search_device64 to positions
(hsa_hit_positions_device64).

* small texts, against the compiled reference's values: the golden SA positions of
  test_gpu_sa.py through the 64-bit path, the 64-bit builder's samples against the
  32-bit builder's and the .sa files, the walk's bound, and hit lists against a NumPy
  restatement;
* past 2^32, where no reference exists, against the text itself: a 2^32 + 2^22 + 7
  character text, its BWT against hsa_build_bwt_device64's, LF steps against the pinned
  64-bit rank of the restatement, walk consistency at the 2^32 edges, and the positions
  of searched reads against the genome they were cut from."""
import ctypes as C
import os

import numpy as np
import pytest

from golden_io import GOLD, INDEX, load_case, parse_opts
from hsa_amd import index_io

pytestmark = pytest.mark.gpu

U64 = np.uint64
ONES = U64(0xFFFFFFFFFFFFFFFF)
BIG_T = (1 << 32) + (1 << 22) + 7
_IX = {}


def widen(a):
    """u32 -> u64, the 32-bit all-ones to the 64-bit all-ones."""
    a = np.asarray(a, np.uint32)
    return np.where(a == np.uint32(0xFFFFFFFF), ONES, a.astype(U64))


def index64(name):
    """hsa_index_create_device64 over a golden index with both suffix arrays attached:
    the .sa file's through hsa_index_set_sa, the same widened through hsa_index_set_sa64."""
    from test_gpu_wide import _upload_lsb
    from hsa_amd._lib import GpuIndex
    if name not in _IX:
        fwd, rev = index_io.read_index(INDEX[name])
        d_f, d_r = _upload_lsb(fwd), _upload_lsb(rev)
        gi = GpuIndex.from_device_codes64(fwd.T, fwd.isa0, np.asarray(fwd.C, U64), d_f.data_ptr(), rev.T, rev.isa0,
                                          np.asarray(rev.C, U64), d_r.data_ptr())
        sa, blocks = index_io.read_sa(INDEX[name]), index_io.read_blocks(INDEX[name])
        gi.set_sa(sa, blocks)
        gi.set_sa64(widen(sa.values), sa.interval, blocks.astype(U64))
        gi.isa0, gi.interval = int(fwd.isa0), int(sa.interval)
        _IX[name] = gi
    return _IX[name]


def hit_positions(gi, n_aln, hit_off, hits, max_occ, pos_cap):
    """One hsa_hit_positions_device64 call over host copies of a search's outputs:
    (pos_off, pos (pos_cap, 4), pos_hit, counters); unwritten rows keep the fill."""
    import torch
    from hsa_amd._lib import HitPosBatch64
    n = len(n_aln)
    t = dict(n=torch.from_numpy(np.ascontiguousarray(n_aln, np.int32)).cuda(),
             o=torch.from_numpy(np.ascontiguousarray(hit_off, np.int64)).cuda(),
             h=torch.from_numpy(np.ascontiguousarray(hits, np.uint32).view(np.int32).reshape(-1)).cuda(),
             po=torch.full((n + 1,), 0x55, dtype=torch.int64, device="cuda"),
             p=torch.full((max(pos_cap, 1) * 4,), 0x77, dtype=torch.int64, device="cuda"),
             ph=torch.full((max(pos_cap, 1),), 0x77, dtype=torch.int32, device="cuda"),
             c=torch.full((4,), 0x33, dtype=torch.int64, device="cuda"))
    b = HitPosBatch64(d_n_aln=t["n"].data_ptr(), d_hit_off=t["o"].data_ptr(), d_hits=t["h"].data_ptr(), n_jobs=n,
                      max_occ=max_occ, d_pos_off=t["po"].data_ptr(), d_pos=t["p"].data_ptr(),
                      d_pos_hit=t["ph"].data_ptr(), pos_cap=pos_cap, d_counters=t["c"].data_ptr())
    torch.cuda.synchronize()
    gi.hit_positions64(b)
    torch.cuda.synchronize()
    return (t["po"].cpu().numpy().view(U64), t["p"].cpu().numpy().view(U64).reshape(-1, 4)[:pos_cap],
            t["ph"].cpu().numpy().view(np.uint32)[:pos_cap], t["c"].cpu().numpy().view(U64))


def rec_kl(rec):
    """k, l of an hsa_aln64_t record (14 u32)."""
    return int(rec[2]) | int(rec[3]) << 32, int(rec[4]) | int(rec[5]) << 32


# ---------------------------------------------------------------- small texts
@pytest.mark.parametrize("name", ["nrun", "tiny"])
def test_golden_positions_through_the_64bit_path(name):
    g = np.load(f"{GOLD}/{name}_sa.npz")
    gi = index64(name)
    got = gi.sa_positions64(g["idx"].astype(U64))
    for col, key in enumerate(("sa", "seq_id", "ori_pos", "occ_pos")):
        bad = np.flatnonzero(got[:, col] != widen(g[key]))
        assert len(bad) == 0, f"{key}: {len(bad)} differ, first index {int(g['idx'][bad[0]])}"
    got32 = gi.sa_positions(g["idx"])                      # the 32-bit arrays beside them, untouched
    for col, key in enumerate(("sa", "seq_id", "ori_pos", "occ_pos")):
        assert np.array_equal(got32[:, col], g[key]), key


@pytest.mark.parametrize("interval", [8, 5])
@pytest.mark.parametrize("name", ["tiny", "nrun"])
def test_builder64_samples_match_the_32bit_builder(name, interval):
    import torch
    from hsa_amd import index_build
    from hsa_amd._lib import build_bwt_index64
    with open(INDEX[name] + ".index.pac", "rb") as f:
        text = index_build.pac_text(f.read())
    T = len(text)
    bwt32, isa32, C32, sa32 = index_build._device_bwt(text, interval)
    d_text = torch.from_numpy(np.concatenate([index_io.pack_lsb_u32(text), np.zeros(8, np.uint32)]).view(np.int32)).cuda()
    torch.cuda.synchronize()
    bw, isa0, Cc, sa = build_bwt_index64(T, d_text.data_ptr(), interval)
    try:
        got = sa.to_host()
    finally:
        sa.free()
    assert isa0 == isa32 and np.array_equal(Cc, C32.astype(U64))
    assert np.array_equal(index_io.unpack_lsb_u32(bw.cpu().numpy().view(np.uint32), T), bwt32)
    assert len(got) == (T + interval) // interval == len(sa32)
    assert int(got[0]) == T                                    # entry 0: set by build_bwt_index64
    assert np.array_equal(got[1:], sa32[1:].astype(U64))
    if interval == 8:
        f = index_io.read_sa(INDEX[name])
        assert f.interval == 8 and np.array_equal(got[1:], f.values[1:].astype(U64))


def walk_steps(gi, idx):
    """LF steps the walk of each index takes: to a sampled row or to row isa0."""
    cur = np.asarray(idx, U64).copy()
    steps = np.zeros(len(cur), np.int64)
    while True:
        act = (cur % U64(gi.interval) != 0) & (cur != U64(gi.isa0))
        if not act.any():
            return steps
        steps[act] += 1
        cur[act] = gi.psi_minus64(cur[act])


def test_walk_bound_cuts_exactly_the_long_walks(monkeypatch):
    g = np.load(f"{GOLD}/tiny_sa.npz")
    gi = index64("tiny")
    idx = g["idx"].astype(U64)
    monkeypatch.delenv("HSA_SA_MAX_WALK", raising=False)
    free = gi.sa_positions64(idx)
    assert not (free[idx != 0, 0] == ONES).any()           # (index 0 answers the file's own entry 0, -1)
    long = walk_steps(gi, idx) > 1
    assert long.any() and (~long).any()
    monkeypatch.setenv("HSA_SA_MAX_WALK", "1")
    cut = gi.sa_positions64(idx)
    assert (cut[long] == ONES).all(), "a walk of more than one step was not cut"
    assert np.array_equal(cut[~long], free[~long])
    # the same through the hit lists: one record k = l = idx per read
    n = len(idx)
    hits = np.zeros((n, 14), np.uint32)
    hits[:, 2], hits[:, 3] = idx & U64(0xFFFFFFFF), idx >> U64(32)
    hits[:, 4], hits[:, 5] = hits[:, 2], hits[:, 3]
    off, pos, ph, ctr = hit_positions(gi, np.ones(n, np.int32), np.arange(n), hits, 4, n)
    assert np.array_equal(off, np.arange(n + 1, dtype=U64))
    assert int(ctr[0]) == n and int(ctr[1]) == n and int(ctr[2]) == int(long.sum())
    assert np.array_equal(pos, cut) and not ph.any()
    monkeypatch.delenv("HSA_SA_MAX_WALK")
    assert np.array_equal(gi.sa_positions64(idx), free)


def expected_rows(n_aln, hit_off, hits, max_occ):
    """The NumPy restatement: per read the SA rows of its records in list order, k .. l
    ascending, the first max_occ of the read; (row counts, SA rows, record indices)."""
    cnt, rows, rec_i = [], [], []
    for j in range(len(n_aln)):
        mine = []
        for i in range(max(int(n_aln[j]), 0)):
            k, l = rec_kl(hits[int(hit_off[j]) + i])
            mine += [(r, i) for r in range(k, min(l, k + max_occ) + 1)]
        mine = mine[:max_occ]
        cnt.append(len(mine))
        rows += [m[0] for m in mine]
        rec_i += [m[1] for m in mine]
    return np.array(cnt, np.int64), np.array(rows, U64), np.array(rec_i, np.uint32)


@pytest.fixture(scope="module")
def rep_search():
    """The repeat genome's reads, -n 4 -o 1, through hsa_search_device64."""
    from oracle_ctypes import default_opt
    from test_gpu_wide import _device_jobs, search
    g = load_case("rep_mm100_n4o1")
    od = parse_opts(g["args"], default_opt())
    od["mode"] &= ~0x01
    lens, codes = _device_jobs(g, od)
    gi = index64("rep")
    n_aln, flags, hit_off, hits, _ = search(gi, lens, codes, od, True, cap_per_read=64)
    # and a read left with HSA_F_OVERFLOW and one without a hit, as the search leaves them:
    # n_aln 0, whatever their hit_off
    n_aln = np.concatenate([[0], n_aln, [0]]).astype(np.int32)
    flags = np.concatenate([[2], flags, [1]]).astype(np.uint32)
    hit_off = np.concatenate([[3], hit_off, [0]]).astype(np.int64)
    return gi, n_aln, flags, hit_off, hits


@pytest.mark.parametrize("max_occ", [1, 3, 64])
def test_hit_lists_to_positions(rep_search, max_occ):
    gi, n_aln, flags, hit_off, hits = rep_search
    cnt, rows, rec_i = expected_rows(n_aln, hit_off, hits, max_occ)
    total = int(cnt.sum())
    full = np.array([sum(rec_kl(hits[int(hit_off[j]) + i])[1] - rec_kl(hits[int(hit_off[j]) + i])[0] + 1
                         for i in range(max(int(n_aln[j]), 0))) for j in range(len(n_aln))])
    # the case has what the test is about: several records per read, records of many rows
    assert (n_aln > 1).any() and full.max() > 3 and (full == 0).any() and total > len(n_aln) // 2
    assert (cnt == np.minimum(full, max_occ)).all()                          # truncation at max_occ rows per read
    assert not cnt[(n_aln <= 0) | ((flags & 2) != 0)].any()                  # no-hit and overflow reads: no rows
    exp_off = np.concatenate([[0], np.cumsum(cnt)]).astype(U64)
    exp_pos = gi.sa_positions64(rows)
    off, pos, ph, ctr = hit_positions(gi, n_aln, hit_off, hits, max_occ, total + 7)
    assert np.array_equal(off, exp_off)
    assert int(ctr[0]) == total and int(ctr[1]) == total and int(ctr[2]) == 0
    assert np.array_equal(pos[:total], exp_pos), "rows differ from sa_positions64 of the restated row list"
    assert np.array_equal(ph[:total], rec_i)
    assert (pos[total:] == U64(0x77)).all() and (ph[total:] == 0x77).all()   # nothing past the last row
    # a second run gives the same arrays
    off2, pos2, ph2, ctr2 = hit_positions(gi, n_aln, hit_off, hits, max_occ, total + 7)
    assert np.array_equal(off, off2) and np.array_equal(pos, pos2) and np.array_equal(ph, ph2)
    assert np.array_equal(ctr[:3], ctr2[:3])
    # less room than rows: the offsets are whole, nothing is written past the cap
    cap = total // 2
    off3, pos3, ph3, ctr3 = hit_positions(gi, n_aln, hit_off, hits, max_occ, cap)
    assert np.array_equal(off3, exp_off)
    assert int(ctr3[0]) == total and int(ctr3[1]) == cap and ctr3[0] > ctr3[1]
    assert np.array_equal(pos3, exp_pos[:cap]) and np.array_equal(ph3, rec_i[:cap])


def test_hit_positions_leave_the_guard_rows_untouched(rep_search):
    """pos_cap rows are the buffer: with room for cap + 16 the rows past cap keep their fill."""
    import torch
    from hsa_amd._lib import HitPosBatch64
    gi, n_aln, flags, hit_off, hits = rep_search
    cnt, rows, _ = expected_rows(n_aln, hit_off, hits, 3)
    cap = int(cnt.sum()) // 3
    n = len(n_aln)
    d_n = torch.from_numpy(n_aln.astype(np.int32)).cuda()
    d_o = torch.from_numpy(hit_off.astype(np.int64)).cuda()
    d_h = torch.from_numpy(hits.view(np.int32).reshape(-1).copy()).cuda()
    po = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    p = torch.full(((cap + 16) * 4,), 0x77, dtype=torch.int64, device="cuda")
    ph = torch.full((cap + 16,), 0x77, dtype=torch.int32, device="cuda")
    c = torch.zeros(4, dtype=torch.int64, device="cuda")
    b = HitPosBatch64(d_n_aln=d_n.data_ptr(), d_hit_off=d_o.data_ptr(), d_hits=d_h.data_ptr(), n_jobs=n, max_occ=3,
                      d_pos_off=po.data_ptr(), d_pos=p.data_ptr(), d_pos_hit=ph.data_ptr(), pos_cap=cap,
                      d_counters=c.data_ptr())
    torch.cuda.synchronize()
    gi.hit_positions64(b)
    torch.cuda.synchronize()
    assert (p.cpu().numpy()[4 * cap:] == 0x77).all() and (ph.cpu().numpy()[cap:] == 0x77).all()
    assert np.array_equal(p.cpu().numpy().view(U64).reshape(-1, 4)[:cap], gi.sa_positions64(rows[:cap]))


def test_sa64_argument_errors():
    from hsa_amd._lib import GpuIndex, HitPosBatch64, HsaError
    from test_gpu_wide import _upload_lsb
    gi = index64("tiny")
    fwd, rev = index_io.read_index(INDEX["tiny"])
    sa, blocks = index_io.read_sa(INDEX["tiny"]), index_io.read_blocks(INDEX["tiny"]).astype(U64)
    vals = widen(sa.values)
    d_f, d_r = _upload_lsb(fwd), _upload_lsb(rev)
    fresh = GpuIndex.from_device_codes64(fwd.T, fwd.isa0, np.asarray(fwd.C, U64), d_f.data_ptr(), rev.T, rev.isa0,
                                         np.asarray(rev.C, U64), d_r.data_ptr())
    with pytest.raises(HsaError, match="-2"):                        # no suffix array yet
        fresh.sa_positions64(np.array([1], U64))
    with pytest.raises(HsaError, match="-2"):
        fresh.hit_positions64(HitPosBatch64(n_jobs=0, max_occ=1), 1)
    with pytest.raises(HsaError, match="-2"):                        # too few values
        fresh.set_sa64(vals[:-1], sa.interval, blocks)
    with pytest.raises(HsaError, match="-2"):                        # interval 0
        fresh.set_sa64(vals, 0, blocks)
    with pytest.raises(HsaError, match="-2"):                        # an index past T
        fresh.psi_minus64(np.array([fwd.T + 1], U64))
    c = fresh.clone()
    with pytest.raises(HsaError, match="-2"):                        # a clone
        c.set_sa64(vals, sa.interval, blocks)
    with pytest.raises(HsaError, match="-2"):                        # an index with live clones
        fresh.set_sa64(vals, sa.interval, blocks)
    c.close()
    fresh.set_sa64(vals, sa.interval, blocks)
    c = fresh.clone()                                                # a clone shares the arrays
    idx = np.arange(0, fwd.T + 1, 97, dtype=U64)
    assert np.array_equal(c.sa_positions64(idx), gi.sa_positions64(idx))
    c.close()
    fresh.close()
    narrow = GpuIndex(fwd, rev)                                      # not an index of hsa_index_create_device64
    with pytest.raises(HsaError, match="-2"):
        narrow.set_sa64(vals, sa.interval, blocks)
    narrow.close()


# ---------------------------------------------------------------- past 2^32
@pytest.fixture(scope="module")
def big64():
    """A 4.3 Gbp synthetic text (seed 77): the forward BWT and its suffix array sampled
    every 32 rows from hsa_build_bwt_index_device64 (134 M u64 samples that never leave
    the device), the reverse BWT and a second forward BWT from hsa_build_bwt_device64,
    one block row over the whole text, the 64-bit restatement's index and the genome."""
    import torch
    from hsa_amd import synth
    from hsa_amd._lib import GpuIndex, build_bwt_index64, check, lib
    from oracle_ctypes import OracleIndex64
    T = BIG_T
    nw = (T + 15) // 16
    text = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
    check(lib().hsa_synth_genome_device(0, T, 77, text.data_ptr()))
    torch.cuda.synchronize()
    bw, isa0, Cf, sa = build_bwt_index64(T, text.data_ptr(), 32)
    ref = []
    for rev in (0, 1):
        b = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
        i0 = C.c_uint64()
        Cc = np.zeros(5, U64)
        check(lib().hsa_build_bwt_device64(0, T, text.data_ptr(), rev, b.data_ptr(), C.byref(i0), Cc))
        ref.append((b, int(i0.value), Cc))
    del text
    torch.cuda.synchronize()
    same = dict(bwt=bool(torch.equal(bw[:nw], ref[0][0][:nw])), isa0=isa0 == ref[0][1],
                C=bool(np.array_equal(Cf, ref[0][2])) and int(Cf[4]) == T)
    gi = GpuIndex.from_device_codes64(T, isa0, Cf, bw.data_ptr(), T, ref[1][1], ref[1][2], ref[1][0].data_ptr())
    assert gi.is64()
    gi.set_sa64_device(sa, sa.n, 32, np.array([[1, 0, T - 1, 0]], U64))
    host = [bw[:nw].cpu().numpy().view(np.uint32), ref[1][0][:nw].cpu().numpy().view(np.uint32)]
    ox = OracleIndex64(T, isa0, Cf, host[0], T, ref[1][1], ref[1][2], host[1])
    gi.isa0, gi.C0 = isa0, [int(x) for x in Cf]
    yield gi, ox, synth.PackedGenome(T, 77), same
    gi.close()


def psi_oracle(ox, isa0, C0, rows):
    """One LF step from the pinned 64-bit rank: the character of a row is the base whose
    count differs between the two adjacent positions."""
    out = []
    for r in (int(x) for x in rows):
        if r == isa0:
            out.append(0)
            continue
        a, b = ox.occ4(0, r), ox.occ4(0, r + 1)
        c = np.flatnonzero(a != b)
        assert len(c) == 1 and int(b[c[0]]) == int(a[c[0]]) + 1
        out.append(C0[int(c[0])] + int(b[c[0]]))
    return np.array(out, U64)


def test_builder64_bwt_matches_build_bwt_device64(big64):
    same = big64[3]
    assert same["bwt"] and same["isa0"] and same["C"], same


def test_walk_is_consistent_at_the_2_32_edges(big64):
    gi, ox, _, _ = big64
    T, isa0 = BIG_T, gi.isa0
    e = 1 << 32
    rows = [1, 2, 31, 32, 33, e - 1, e, e + 1, e + 31, e + 32, T - 1, T, isa0, isa0 - 1, isa0 + 1]
    rows = np.concatenate([np.array(rows, U64), np.random.default_rng(6).integers(1, T + 1, 4000, dtype=U64)])
    out = gi.sa_positions64(rows)
    pos = out[:, 0]
    assert (pos < U64(T)).all() and np.array_equal(out[:, 3], pos)
    assert (out[:, 1] == 1).all() and np.array_equal(out[:, 2], pos + U64(1))    # the one block row
    assert int(pos[rows == U64(isa0)][0]) == 0
    nxt = gi.psi_minus64(rows)
    assert np.array_equal(nxt, psi_oracle(ox, isa0, gi.C0, rows))
    m = rows != U64(isa0)
    assert (pos[m] > 0).all()
    assert np.array_equal(gi.sa_positions64(nxt[m])[:, 0], pos[m] - U64(1))
    assert (rows > U64(e)).any() and (nxt > U64(e)).any() and (pos > U64(e)).any()


def test_positions_of_searched_reads_match_the_text(big64):
    """2 000 reads of 100 bp with up to 3 substitutions from the whole text, -n 4 -o 0,
    max_occ 8.  8 rows never cut the truth: a second occurrence of a 100-mer within 4
    substitutions in an i.i.d. text of T = 4.3e9 has probability <= 2 T sum_{d<=4}
    C(100, d) 3^d / 4^100 < 1e-41 per read (the text's own overlapping windows included)."""
    from hsa_amd import synth
    from oracle_ctypes import default_opt
    from test_gpu_wide import search
    import math
    gi, _, genome, _ = big64
    L, n = 100, 2000
    assert 2 * BIG_T * sum(math.comb(L, d) * 3 ** d for d in range(5)) / 4 ** L < 1e-41
    reads, truth = synth.make_reads(genome, [(0, BIG_T)], n, L, 41, max_mm=3)
    od = default_opt()
    od.update(max_diff=4, fnr=-1.0, max_gapo=0)
    od["mode"] &= ~0x01
    n_aln, flags, hit_off, hits, _ = search(gi, np.full(n, L, np.uint32), reads.reshape(-1), od, True)
    # No read is left out: a read has rows, or it is one the search itself cannot return --
    # more than max_seed_diff substitutions inside its seed, the last seed_len bases of the
    # strand sequence that occurs in the text (bwtaln.c:332, :345) -- which its truth shows.
    w0 = genome[truth["start"][:, None] + np.arange(L)[None, :]]
    sq0 = np.where(truth["strand"].astype(bool)[:, None], synth.revcomp_codes(reads), reads)
    mm = w0 != sq0
    assert np.array_equal(mm.sum(axis=1), truth["n_mm"])
    in_seed = mm[:, L - od["seed_len"]:].sum(axis=1)
    lost = np.flatnonzero(n_aln <= 0)
    assert (in_seed[lost] > od["max_seed_diff"]).all(), \
        f"reads without a hit that the seed rule does not explain: {lost[in_seed[lost] <= od['max_seed_diff']][:8]}"
    assert len(lost) < n // 20
    off, pos, ph, ctr = hit_positions(gi, n_aln, hit_off, hits, 8, 8 * n)
    total = int(off[n])
    assert int(ctr[0]) == total == int(ctr[1]) and int(ctr[2]) == 0 and total >= n - len(lost)
    assert np.array_equal(np.diff(off.astype(np.int64)) >= 1, n_aln > 0)
    read_of = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    rec = hits[hit_off[read_of].astype(np.int64) + ph[:total]]
    q = pos[:total, 3].astype(np.int64)
    assert (q >= 0).all() and (q + L <= BIG_T).all()
    window = genome[q[:, None] + np.arange(L)[None, :]]
    strand = (rec[:, 1] >> 30) & 3
    seq = np.where((strand == 1)[:, None], synth.revcomp_codes(reads[read_of]), reads[read_of])
    ham = (window != seq).sum(axis=1)
    bad = np.flatnonzero(ham != (rec[:, 0] & 0xFFFF))
    assert len(bad) == 0, f"{len(bad)} rows: the text at the position is not the hit (first row {bad[0]}, {ham[bad[0]]} mismatches)"
    found = np.zeros(n, bool)
    found[read_of[q == truth["start"][read_of]]] = True
    assert found[n_aln > 0].all(), f"{int((~found[n_aln > 0]).sum())} reads: the true start is not among the rows"
    assert (q >= (1 << 32)).any()


def test_lf_step_across_real_count_wraps():
    """One LF step where the rank blocks' counts wrap: the mostly-A (forward) 4.3
    G-character string of test_rank_count_wraps_match_oracle, built as it builds it.
    The string is no BWT, so it is stepped once and never walked."""
    import torch
    from hsa_amd._lib import GpuIndex, check, lib
    from oracle_ctypes import OracleIndex64
    from test_gpu_wide import _counts_lsb
    T = BIG_T
    nw = (T + 15) // 16
    t = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
    check(lib().hsa_synth_genome_device(0, T, 31, t.data_ptr()))
    g = torch.Generator(device="cuda").manual_seed(31)
    keep = torch.rand(nw + 8, device="cuda", generator=g) < 1.0 / 2000
    t = torch.where(keep, t, torch.tensor(np.int32(0), device="cuda"))
    if T % 16:
        last = int(np.uint32(t[nw - 1].item() & 0xFFFFFFFF)) & ((1 << (2 * (T % 16))) - 1)
        t[nw - 1] = int(np.uint32(last).view(np.int32))
    t[nw:] = 0
    torch.cuda.synchronize()
    w = t[:nw].cpu().numpy().view(np.uint32)
    cnt = _counts_lsb(w, T)
    assert cnt[0] > (1 << 32)
    Cc = np.concatenate([[0], np.cumsum(cnt)]).astype(U64)
    lo = w & np.uint32(0x55555555)
    hi = (w >> np.uint32(1)) & np.uint32(0x55555555)
    per = (16 - np.bitwise_count((lo | hi) & np.uint32(0x55555555))).astype(np.int64)
    per[-1] -= 16 - (T - 16 * (nw - 1))
    wrap = 16 * int(np.searchsorted(np.cumsum(per), 1 << 32))        # the block where Occ(A) reaches 2^32
    isa0 = T // 5 + 3
    gi = GpuIndex.from_device_codes64(T, isa0, Cc, t.data_ptr(), T, isa0, Cc, t.data_ptr())
    ox = OracleIndex64(T, isa0, Cc, w, T, isa0, Cc, w)
    rows = [wrap + 16 * b + e for b in (-1, 0, 1) for e in (-16, -1, 0, 1, 16)] + [isa0 - 1, isa0, isa0 + 1, T - 1, T]
    rows = np.concatenate([np.array(rows, U64), np.random.default_rng(8).integers(wrap - 4096, wrap + 4096, 500, dtype=U64)])
    got = gi.psi_minus64(rows)
    exp = psi_oracle(ox, isa0, [int(x) for x in Cc], rows)
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, f"{len(bad)} rows differ, first {int(rows[bad[0]])}: {int(got[bad[0]])} vs {int(exp[bad[0]])}"
    assert (got > U64(1 << 32)).any() and (got < U64(1 << 32)).any()     # both sides of the wrap
    gi.close()
