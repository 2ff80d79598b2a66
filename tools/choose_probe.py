#!/usr/bin/env python3
"""Time hsa_choose_hits_device64 (each read's hit, mapQ and XA rows on the 64-bit path).

Builds the synthetic hg19-sized text of tools/refine_probe.py with
hsa_index_create_device64 (suffix array sampled every `--interval` rows, text attached),
and for one config-2 read set (100 bp, up to 4 substitutions, -n 4 -o 0) and the config-3
set of refine_probe (one indel of 1-3 bp and 0-2 substitutions, -n 4 -o 1) searches the
batch with hsa_search_device64 and times, with HIP events on one stream, the median of
--launches runs after --warmup warm-ups of

  choose          hsa_choose_hits_device64 (n_multi 3), and its launches one by one
                  (hsa_choose_timing), with the number of reads walked in order;
  choose_refine   the same followed by hsa_refine_rows_device64 of its rows;
  all_rows        what the information cost before the choice existed:
                  hsa_hit_positions_device64 at max_occ = n_multi + 1, then
                  hsa_refine_rows_device64 of all those rows (and the choice still to be
                  made on the host);

beside the batch's k_search time (hsa_last_pass_ms), the rows walked and the DP rows run
on each side.  The synthetic text is i.i.d., so its reads have one record of one row each
and none is walked in order; a third leg therefore times the choice alone on fabricated
hit lists of the same batch size in which --variable-share of the reads have 2-4
equal-best records of 1-3 rows (what a repeat-rich genome gives), against
hsa_hit_positions_device64 at max_occ = n_multi + 1.  One JSON object on stdout (and in
--out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENOME_T = 3_000_000_005        # bench.py's hg19-sized text
GENOME_SEED = 1234              # bench.py's GENOME_SEED
RECORDS = 24                    # bench.py's RECORDS
N_MULTI = 3                     # bwtaln.c:514


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn, stream_obj, launches, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    ev[0].record(stream_obj)
    for i in range(launches):
        fn()
        ev[i + 1].record(stream_obj)
    torch.cuda.synchronize()
    ms = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(launches)])
    return dict(ms_median=round(float(np.median(ms)), 4), ms_min=round(float(ms.min()), 4), ms_max=round(float(ms.max()), 4))


def one_set(gi, a, name, reads, max_gapo, tst):
    import torch
    from hsa_amd import _lib
    from hsa_amd._lib import ChooseBatch64, DeviceBatch, GapOpt, HitPosBatch64, RefineBatch64, Regime
    n, RL, stream = a.batch, a.read_len, tst.cuda_stream
    opt = GapOpt.default()
    opt.max_diff, opt.fnr, opt.max_gapo = 4, -1.0, max_gapo
    opt.mode &= ~0x01
    n_stacks = (opt.max_diff + 1) * opt.s_mm + (opt.max_gapo + 1) * opt.s_gapo + (opt.max_gape + 1) * opt.s_gape
    rg = Regime(s_mm=opt.s_mm, s_gapo=opt.s_gapo, s_gape=opt.s_gape, mode=0, indel_end_skip=opt.indel_end_skip,
                max_del_occ=opt.max_del_occ, max_entries=opt.max_entries, max_gapo=max_gapo, max_gape=opt.max_gape,
                max_seed_diff=opt.max_seed_diff, max_top2=opt.max_top2, n_stacks=n_stacks, max_diff=opt.max_diff)
    jobs = np.zeros(n, _lib.JOB_DTYPE)
    jobs["off"] = np.arange(n, dtype=np.uint64) * RL
    jobs["len"] = RL
    jobs["max_diff"] = opt.max_diff
    jobs["seed_len"] = opt.seed_len
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_codes = torch.from_numpy(_lib.pad_codes(reads.reshape(-1))).cuda()
    hit_cap = n * 16
    z = lambda m, dt: torch.zeros(m, dtype=dt, device="cuda")          # noqa: E731
    o = dict(n=z(n, torch.int32), f=z(n, torch.int32), o=z(n, torch.int64), h=z(hit_cap * _lib.ALN64_WORDS + 2, torch.int32),
             c=z(16, torch.int64))
    b = DeviceBatch(d_jobs=d_jobs.data_ptr(), n_jobs=n, d_codes=d_codes.data_ptr(), d_n_aln=o["n"].data_ptr(),
                    d_flags=o["f"].data_ptr(), d_hit_off=o["o"].data_ptr(), d_hits=o["h"].data_ptr(), hit_cap=hit_cap,
                    d_counters=o["c"].data_ptr(), max_len=RL, max_seed=opt.seed_len)
    search_ms = []
    for _ in range(3):              # the last pass's kernel times: a warm search of the same batch
        gi.search_device64([rg], b)
        torch.cuda.synchronize()
        search_ms.append(gi.last_pass_ms())
    sc = o["c"].cpu().numpy()
    log(f"[choose_probe] {name}: {int((o['n'] > 0).sum())} reads with hits, {int(sc[1])} records, {int(sc[11])} unfinished; "
        f"k_search {search_ms[-1][1]:.2f} ms")

    cap = n * (N_MULTI + 1)
    cs, ms_ = 8, 64
    pos = dict(off=z(n + 1, torch.int64), p=z(cap * 4, torch.int64), h=z(cap, torch.int32), c=z(8, torch.int64))
    sel, sel64, rng = z(n * 4, torch.int32), z(n * 4, torch.int64), z(1, torch.int64)
    out = dict(rows=z(cap * _lib.RF_ROW_WORDS, torch.int32), rpos=z(cap * 2, torch.int64), cigar=z(cap * cs, torch.int32),
               md=z(cap * ms_, torch.uint8), ctr=z(8, torch.int64))
    cb = ChooseBatch64(d_jobs=d_jobs.data_ptr(), n_jobs=n, d_n_aln=o["n"].data_ptr(), d_hit_off=o["o"].data_ptr(),
                       d_hits=o["h"].data_ptr(), n_multi=N_MULTI, rng_state=_lib.DRAND48_SEED0, d_sel=sel.data_ptr(),
                       d_sel64=sel64.data_ptr(), d_rng_out=rng.data_ptr(), d_pos_off=pos["off"].data_ptr(),
                       d_pos=pos["p"].data_ptr(), d_pos_hit=pos["h"].data_ptr(), pos_cap=cap, d_counters=pos["c"].data_ptr())
    hb = HitPosBatch64(d_n_aln=o["n"].data_ptr(), d_hit_off=o["o"].data_ptr(), d_hits=o["h"].data_ptr(), n_jobs=n,
                       max_occ=N_MULTI + 1, d_pos_off=pos["off"].data_ptr(), d_pos=pos["p"].data_ptr(),
                       d_pos_hit=pos["h"].data_ptr(), pos_cap=cap, d_counters=pos["c"].data_ptr())
    rb = RefineBatch64(d_jobs=d_jobs.data_ptr(), n_jobs=n, d_codes=d_codes.data_ptr(), d_hit_off=o["o"].data_ptr(),
                       d_hits=o["h"].data_ptr(), d_pos_off=pos["off"].data_ptr(), d_pos=pos["p"].data_ptr(),
                       d_pos_hit=pos["h"].data_ptr(), pos_cap=cap, d_pos_counters=pos["c"].data_ptr(), max_len=RL,
                       cigar_stride=cs, md_stride=ms_, d_rows=out["rows"].data_ptr(), d_rpos=out["rpos"].data_ptr(),
                       d_cigar=out["cigar"].data_ptr(), d_md=out["md"].data_ptr(), d_counters=out["ctr"].data_ptr())
    torch.cuda.synchronize()

    def choose():
        gi.choose_hits64(cb, stream=stream)

    def choose_refine():
        gi.choose_hits64(cb, stream=stream)
        gi.refine_rows64(rb, stream=stream)

    def all_rows():
        gi.hit_positions64(hb, stream=stream)
        gi.refine_rows64(rb, stream=stream)

    res = dict(options=f"-n 4 -o {max_gapo}", reads_with_hits=int((o["n"] > 0).sum()), hit_records=int(sc[1]),
               k_widths_ms=round(float(search_ms[-1][0]), 4), k_search_ms=round(float(search_ms[-1][1]), 4))
    res["choose"] = timed(choose, tst, a.launches, a.warmup)
    # the launches one by one: the events cost a little, so this is a run of its own
    _lib.lib().hsa_choose_timing(1)
    split = []
    for _ in range(a.launches):
        choose()
        split.append(gi.choose_launch_times())
    _lib.lib().hsa_choose_timing(0)
    res["choose"]["launch_ms_median"] = {k: round(float(np.median([s[k] for s in split])), 4) for k in split[0]}
    cc = pos["c"].cpu().numpy()
    res["choose"].update(rows=int(cc[1]), reads_with_hit=int(cc[3]), repeat_reads=int(cc[4]), reads_walked_in_order=int(cc[5]),
                         zero_draw_reads=int(cc[6]))
    res["choose_refine"] = timed(choose_refine, tst, a.launches, a.warmup)
    rc = out["ctr"].cpu().numpy()
    res["choose_refine"].update(rows_walked=int(cc[1]), dp_rows=int(rc[6]))
    res["all_rows"] = timed(all_rows, tst, a.launches, a.warmup)
    pc, rc = pos["c"].cpu().numpy(), out["ctr"].cpu().numpy()
    res["all_rows"].update(max_occ=N_MULTI + 1, rows_walked=int(pc[1]), dp_rows=int(rc[6]))
    w = res["choose"]["launch_ms_median"]["walk"]
    res["choose"]["walk_share"] = round(w / max(sum(res["choose"]["launch_ms_median"].values()), 1e-9), 4)
    log(f"[choose_probe] {name}: choose {res['choose']['ms_median']:.3f} ms ({res['choose']['reads_walked_in_order']} reads "
        f"walked in order, walk {w:.3f} ms), choose + refine {res['choose_refine']['ms_median']:.3f} ms, "
        f"all rows {res['all_rows']['ms_median']:.3f} ms")
    return res


def fabricated_set(gi, a, tst):
    """The choice alone on fabricated lists: every read has a hit, a share of them two to
    four equal-best records; up to one worse record; 1-3 rows per record."""
    import torch
    from hsa_amd import _lib
    from hsa_amd._lib import ChooseBatch64, HitPosBatch64
    n, stream = a.batch, tst.cuda_stream
    rng = np.random.default_rng(9)
    nb = np.where(rng.random(n) < a.variable_share, rng.integers(2, 5, n), 1)
    na = (nb + rng.integers(0, 2, n)).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(na)]).astype(np.int64)
    R = int(off[-1])
    within = np.arange(R) - np.repeat(off[:-1], na)
    hits = np.zeros((R, _lib.ALN64_WORDS), np.uint32)
    k = rng.integers(1, gi.T - 4, R).astype(np.uint64)
    l = k + rng.integers(0, 3, R).astype(np.uint64)
    hits[:, 2], hits[:, 3] = k & np.uint64(0xFFFFFFFF), k >> np.uint64(32)
    hits[:, 4], hits[:, 5] = l & np.uint64(0xFFFFFFFF), l >> np.uint64(32)
    hits[:, 12] = np.where(within < np.repeat(nb, na), 9, 12)
    jobs = np.zeros(n, _lib.JOB_DTYPE)
    jobs["len"], jobs["max_diff"] = a.read_len, 4
    d = dict(jobs=torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), n=torch.from_numpy(na).cuda(),
             o=torch.from_numpy(off[:-1].copy()).cuda(), h=torch.from_numpy(hits.view(np.int32).reshape(-1).copy()).cuda())
    cap = n * (N_MULTI + 1)
    z = lambda m, dt: torch.zeros(m, dtype=dt, device="cuda")          # noqa: E731
    pos = dict(off=z(n + 1, torch.int64), p=z(cap * 4, torch.int64), h=z(cap, torch.int32), c=z(8, torch.int64))
    sel, sel64, rs = z(n * 4, torch.int32), z(n * 4, torch.int64), z(1, torch.int64)
    cb = ChooseBatch64(d_jobs=d["jobs"].data_ptr(), n_jobs=n, d_n_aln=d["n"].data_ptr(), d_hit_off=d["o"].data_ptr(),
                       d_hits=d["h"].data_ptr(), n_multi=N_MULTI, rng_state=_lib.DRAND48_SEED0, d_sel=sel.data_ptr(),
                       d_sel64=sel64.data_ptr(), d_rng_out=rs.data_ptr(), d_pos_off=pos["off"].data_ptr(),
                       d_pos=pos["p"].data_ptr(), d_pos_hit=pos["h"].data_ptr(), pos_cap=cap, d_counters=pos["c"].data_ptr())
    hb = HitPosBatch64(d_n_aln=d["n"].data_ptr(), d_hit_off=d["o"].data_ptr(), d_hits=d["h"].data_ptr(), n_jobs=n,
                       max_occ=N_MULTI + 1, d_pos_off=pos["off"].data_ptr(), d_pos=pos["p"].data_ptr(),
                       d_pos_hit=pos["h"].data_ptr(), pos_cap=cap, d_counters=pos["c"].data_ptr())
    torch.cuda.synchronize()

    def choose():
        gi.choose_hits64(cb, stream=stream)

    res = dict(variable_share=a.variable_share, hit_records=R, equal_best_records_of_walked_reads=int(nb[nb > 1].sum()))
    res["choose"] = timed(choose, tst, a.launches, a.warmup)
    _lib.lib().hsa_choose_timing(1)
    split = []
    for _ in range(a.launches):
        choose()
        split.append(gi.choose_launch_times())
    _lib.lib().hsa_choose_timing(0)
    lm = {k: round(float(np.median([s[k] for s in split])), 4) for k in split[0]}
    cc = pos["c"].cpu().numpy()
    res["choose"].update(launch_ms_median=lm, walk_share=round(lm["walk"] / max(sum(lm.values()), 1e-9), 4), rows=int(cc[1]),
                         repeat_reads=int(cc[4]), reads_walked_in_order=int(cc[5]), zero_draw_reads=int(cc[6]))
    res["hit_positions"] = timed(lambda: gi.hit_positions64(hb, stream=stream), tst, a.launches, a.warmup)
    res["hit_positions"].update(max_occ=N_MULTI + 1, rows=int(pos["c"].cpu().numpy()[1]))
    log(f"[choose_probe] fabricated: choose {res['choose']['ms_median']:.3f} ms, {int(cc[5])} reads walked in order in "
        f"{lm['walk']:.3f} ms; hit_positions {res['hit_positions']['ms_median']:.3f} ms")
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genome", type=int, default=GENOME_T, help="text length (default: hg19-sized)")
    ap.add_argument("--interval", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variable-share", type=float, default=0.2,
                    help="the fabricated leg's share of reads with two or more equal-best records")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from hsa_amd import _lib, synth
    import torch
    from hsa_amd._lib import DeviceU64
    L = _lib.lib()
    T, s, n, RL = a.genome, a.interval, a.batch, a.read_len
    nw = (T + 15) // 16
    t0 = time.time()
    text = DeviceU64((nw + 10) // 2)
    L.hipMemset(C.c_void_p(text.ptr), 0, C.c_size_t(8 * text.n))
    _lib.check(L.hsa_synth_genome_device(0, T, GENOME_SEED, C.c_void_p(text.ptr)))
    torch.cuda.synchronize()
    bw, isa0, Cf, sa = _lib.build_bwt_index64(T, text.ptr, s)
    rb = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
    ri = C.c_uint64()
    Cr = np.zeros(5, np.uint64)
    _lib.check(L.hsa_build_bwt_device64(0, T, C.c_void_p(text.ptr), 1, rb.data_ptr(), C.byref(ri), Cr))
    gi = _lib.GpuIndex.from_device_codes64(T, isa0, Cf, bw.data_ptr(), T, int(ri.value), Cr, rb.data_ptr())
    del bw, rb
    torch.cuda.empty_cache()
    recs = synth.record_layout(T, RECORDS)
    blocks = np.array([[r, s0, s0 + m - 1, 0] for r, (s0, m) in enumerate(recs)], np.uint64)
    gi.set_sa64_device(sa, sa.n, s, blocks)
    gi.set_text64_device(text, T)
    log(f"[choose_probe] index of {T} bp with samples and text in {time.time() - t0:.1f} s")
    genome = synth.PackedGenome(T, GENOME_SEED)
    tst = torch.cuda.Stream()
    assert tst.cuda_stream, "need a non-default stream (the library maps NULL to the index's own)"
    res = dict(tool="choose_probe", text_bp=T, interval=s, batch=n, read_len=RL, n_multi=N_MULTI, launches=a.launches,
               warmup=a.warmup)
    for name, seed, kw, gapo in (("config2", 5 * 1_000_000, dict(max_mm=4), 0),
                                 ("config3", 6 * 1_000_000, dict(indel=True, max_mm_indel=2), 1)):
        t0 = time.time()
        reads, _ = synth.make_reads(genome, recs, n, RL, seed, **kw)
        log(f"[choose_probe] {name}: {n} reads in {time.time() - t0:.1f} s")
        res[name] = one_set(gi, a, name, reads, gapo, tst)
        del reads
        gi.release_scratch()
        torch.cuda.empty_cache()
    res["fabricated"] = fabricated_set(gi, a, tst)
    gi.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
