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


def timed_ms(fn, stream_obj, launches, warmup):
    """The ms of each of `launches` calls of fn after `warmup` of them, by events on stream_obj."""
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
    return np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(launches)])


def timed(fn, stream_obj, launches, warmup):
    ms = timed_ms(fn, stream_obj, launches, warmup)
    return dict(ms_median=round(float(np.median(ms)), 4), ms_min=round(float(ms.min()), 4), ms_max=round(float(ms.max()), 4))


def probe_opts(max_gapo):
    """-n 4 -o max_gapo as an option dict, the GAPE bit cleared as bwa_cal_sa_reg_gap clears it."""
    from hsa_amd._lib import GapOpt
    opt = GapOpt.default()
    opt.max_diff, opt.fnr, opt.max_gapo = 4, -1.0, max_gapo
    opt.mode &= ~0x01
    return opt.as_dict()


def probe_batch(reads, read_len, opt):
    """The batch dict (hsa_amd.chain) of n reads of read_len bases."""
    from hsa_amd import _lib, chain
    n = len(reads)
    return dict(jobs=chain.to_device(chain.make_jobs(np.full(n, read_len), opt["max_diff"], opt["seed_len"])),
                codes=chain.to_device(_lib.pad_codes(reads.reshape(-1))), n_jobs=n, max_len=read_len)


def one_set(gi, a, name, reads, max_gapo, tst):
    import torch
    from hsa_amd import _lib, chain
    n, RL, stream = a.batch, a.read_len, tst.cuda_stream
    opt = probe_opts(max_gapo)
    rg = chain.local_regime(opt, RL)[2]
    bt = probe_batch(reads, RL, opt)
    b, o = chain.search64_batch(bt, 0, n, n * 16, opt["seed_len"])
    search_ms = []
    for _ in range(3):              # the last pass's kernel times: a warm search of the same batch
        gi.search_device64([rg], b)
        torch.cuda.synchronize()
        search_ms.append(gi.last_pass_ms())
    sc = o["sc"].cpu().numpy()
    log(f"[choose_probe] {name}: {int((o['n_aln'] > 0).sum())} reads with hits, {int(sc[1])} records, {int(sc[11])} unfinished; "
        f"k_search {search_ms[-1][1]:.2f} ms")

    cb, pos = chain.choose64_batch(bt, o, 0, n, _lib.DRAND48_SEED0)
    hb, _ = chain.hit_positions64_batch(o, n, N_MULTI + 1, out=pos)
    rb, out = chain.refine64_batch(pos, 8, 64)
    torch.cuda.synchronize()

    def choose():
        gi.choose_hits64(cb, stream=stream)

    def choose_refine():
        gi.choose_hits64(cb, stream=stream)
        gi.refine_rows64(rb, stream=stream)

    def all_rows():
        gi.hit_positions64(hb, stream=stream)
        gi.refine_rows64(rb, stream=stream)

    res = dict(options=f"-n 4 -o {max_gapo}", reads_with_hits=int((o["n_aln"] > 0).sum()), hit_records=int(sc[1]),
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
    cc = pos["pos_ctr"].cpu().numpy()
    res["choose"].update(rows=int(cc[1]), reads_with_hit=int(cc[3]), repeat_reads=int(cc[4]), reads_walked_in_order=int(cc[5]),
                         zero_draw_reads=int(cc[6]))
    res["choose_refine"] = timed(choose_refine, tst, a.launches, a.warmup)
    rc = out["ctr"].cpu().numpy()
    res["choose_refine"].update(rows_walked=int(cc[1]), dp_rows=int(rc[6]))
    res["all_rows"] = timed(all_rows, tst, a.launches, a.warmup)
    pc, rc = pos["pos_ctr"].cpu().numpy(), out["ctr"].cpu().numpy()
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
    from hsa_amd import _lib, chain
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
    bt = dict(jobs=chain.to_device(jobs), codes=None, max_len=a.read_len)
    d = dict(n_aln=chain.to_device(na), hit_off=chain.to_device(off[:-1]), hits=chain.to_device(hits), first=0)
    cb, pos = chain.choose64_batch(bt, d, 0, n, _lib.DRAND48_SEED0)
    hb, _ = chain.hit_positions64_batch(d, n, N_MULTI + 1, out=pos)
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
    cc = pos["pos_ctr"].cpu().numpy()
    res["choose"].update(launch_ms_median=lm, walk_share=round(lm["walk"] / max(sum(lm.values()), 1e-9), 4), rows=int(cc[1]),
                         repeat_reads=int(cc[4]), reads_walked_in_order=int(cc[5]), zero_draw_reads=int(cc[6]))
    res["hit_positions"] = timed(lambda: gi.hit_positions64(hb, stream=stream), tst, a.launches, a.warmup)
    res["hit_positions"].update(max_occ=N_MULTI + 1, rows=int(pos["pos_ctr"].cpu().numpy()[1]))
    log(f"[choose_probe] fabricated: choose {res['choose']['ms_median']:.3f} ms, {int(cc[5])} reads walked in order in "
        f"{lm['walk']:.3f} ms; hit_positions {res['hit_positions']['ms_median']:.3f} ms")
    return res


def parser(doc, genome=GENOME_T, genome_help="text length (default: hg19-sized)", read_len=100):
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genome", type=int, default=genome, help=genome_help)
    ap.add_argument("--interval", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=read_len)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    return ap


def synthetic_index(a, tag):
    """The synthetic text of a.genome bp as a 64-bit index with its samples and the text
    attached: (the index, the text's record layout)."""
    from hsa_amd import _lib, synth
    import torch
    from hsa_amd._lib import DeviceU64
    L = _lib.lib()
    T, s = a.genome, a.interval
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
    log(f"[{tag}] index of {T} bp with samples and text in {time.time() - t0:.1f} s")
    return gi, recs


def emit(res, out):
    """The result as JSON on stdout and in `out`."""
    txt = json.dumps(res, indent=1)
    print(txt)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(txt + "\n")
    return 0


def run_sets(tag, a, one_set):
    """one_set on the config-2 and the config-3 read set: (the index, the stream, the result so far)."""
    from hsa_amd import synth
    import torch
    gi, recs = synthetic_index(a, tag)
    genome = synth.PackedGenome(a.genome, GENOME_SEED)
    tst = torch.cuda.Stream()
    assert tst.cuda_stream, "need a non-default stream (the library maps NULL to the index's own)"
    res = dict(tool=tag, text_bp=a.genome, interval=a.interval, batch=a.batch, read_len=a.read_len, n_multi=N_MULTI,
               launches=a.launches, warmup=a.warmup)
    for name, seed, kw, gapo in (("config2", 5 * 1_000_000, dict(max_mm=4), 0),
                                 ("config3", 6 * 1_000_000, dict(indel=True, max_mm_indel=2), 1)):
        t0 = time.time()
        reads, _ = synth.make_reads(genome, recs, a.batch, a.read_len, seed, **kw)
        log(f"[{tag}] {name}: {a.batch} reads in {time.time() - t0:.1f} s")
        res[name] = one_set(gi, a, name, reads, gapo, tst)
        del reads
        gi.release_scratch()
        torch.cuda.empty_cache()
    return gi, tst, res


def main(argv=None):
    ap = parser(__doc__)
    ap.add_argument("--variable-share", type=float, default=0.2,
                    help="the fabricated leg's share of reads with two or more equal-best records")
    a = ap.parse_args(argv)
    gi, tst, res = run_sets("choose_probe", a, one_set)
    res["fabricated"] = fabricated_set(gi, a, tst)
    gi.close()
    return emit(res, a.out)


if __name__ == "__main__":
    sys.exit(main())
