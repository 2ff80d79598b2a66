#!/usr/bin/env python3
"""Time hsa_hit_positions_device64 (the hit lists of the 64-bit search to text positions).

Builds a synthetic text (default: config 5's 15 Gbp) with its suffix array sampled every
`--interval` rows on the device (hsa_build_bwt_index_device64; the samples never leave
it), searches one of config 5's read sets (250 bp, 0-4 substitutions, -n 4 -o 0) with
hsa_search_device64, and times hsa_hit_positions_device64 at each --max-occ with HIP
events over --launches launches after --warmup warm-ups.

Reported per max_occ: rows/s and LF steps/s.  LF steps are rows x the mean walk, the mean
measured on a sample of the launch's own rows by stepping them with hsa_psi_minus_batch64
until a sampled row (not a counter in the kernel).  A walk is a chain of dependent random
16-byte loads, so the yardstick is tools/gather_probe's chain16 rate: give its output with
--chain-log (run `tools/gather_probe chain16` on the same device first) and the ratio to
the rate at the nearest table size, 32 waves per CU, is reported.

One JSON object on stdout (and in --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENOME5_T = 15_000_000_003      # bench.py's config 5
GENOME_SEED = 1234              # bench.py's GENOME_SEED
RECORDS = 24                    # bench.py's RECORDS


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def chain_rate(path, table_bytes):
    """gather_probe's chain16 G sectors/s at 32 waves per CU, at the table size nearest to
    table_bytes: (rate, that size)."""
    best = None
    with open(path) as f:
        for ln in f:
            if not ln.startswith("{"):
                continue
            r = json.loads(ln)
            if r.get("mode") != "chain16" or r.get("waves_per_cu") != 32:
                continue
            d = abs(r["table_bytes"] - table_bytes)
            if best is None or d < best[0]:
                best = (d, r["Gsectors_per_s"], r["table_bytes"])
    return (best[1], best[2]) if best else (None, None)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genome", type=int, default=GENOME5_T, help="text length (default: config 5's 15 Gbp)")
    ap.add_argument("--interval", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=250)
    ap.add_argument("--max-occ", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--walk-sample", type=int, default=20_000)
    ap.add_argument("--chain-log", default=None, help="output of `tools/gather_probe chain16`")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from hsa_amd import _lib, synth
    import torch
    from hsa_amd._lib import DeviceBatch, GapOpt, HitPosBatch64, Regime
    L = _lib.lib()
    T, s = a.genome, a.interval
    nw = (T + 15) // 16
    t0 = time.time()
    text = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
    _lib.check(L.hsa_synth_genome_device(0, T, GENOME_SEED, text.data_ptr()))
    torch.cuda.synchronize()
    bw, isa0, Cf, sa = _lib.build_bwt_index64(T, text.data_ptr(), s)
    log(f"[sa64_probe] forward BWT + {sa.n} samples of {T} bp in {time.time() - t0:.1f} s")
    rb = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
    ri = C.c_uint64()
    Cr = np.zeros(5, np.uint64)
    _lib.check(L.hsa_build_bwt_device64(0, T, text.data_ptr(), 1, rb.data_ptr(), C.byref(ri), Cr))
    del text
    torch.cuda.empty_cache()
    gi = _lib.GpuIndex.from_device_codes64(T, isa0, Cf, bw.data_ptr(), T, int(ri.value), Cr, rb.data_ptr())
    del bw, rb
    torch.cuda.empty_cache()
    recs = synth.record_layout(T, RECORDS)
    blocks = np.array([[r, s0, s0 + n - 1, 0] for r, (s0, n) in enumerate(recs)], np.uint64)
    gi.set_sa64_device(sa, sa.n, s, blocks)
    log(f"[sa64_probe] index ready in {time.time() - t0:.1f} s")

    t0 = time.time()
    genome = synth.PackedGenome(T, GENOME_SEED)
    reads, _ = synth.make_reads(genome, recs, a.batch, a.read_len, 8 * 1_000_000, max_mm=4)
    del genome
    log(f"[sa64_probe] {a.batch} reads in {time.time() - t0:.1f} s")
    opt = GapOpt.default()
    opt.max_diff, opt.fnr, opt.max_gapo = 4, -1.0, 0
    opt.mode &= ~0x01
    n_stacks = (opt.max_diff + 1) * opt.s_mm + (opt.max_gapo + 1) * opt.s_gapo + (opt.max_gape + 1) * opt.s_gape
    rg = Regime(s_mm=opt.s_mm, s_gapo=opt.s_gapo, s_gape=opt.s_gape, mode=0, indel_end_skip=opt.indel_end_skip,
                max_del_occ=opt.max_del_occ, max_entries=opt.max_entries, max_gapo=0, max_gape=opt.max_gape,
                max_seed_diff=opt.max_seed_diff, max_top2=opt.max_top2, n_stacks=n_stacks, max_diff=opt.max_diff)
    n = a.batch
    jobs = np.zeros(n, _lib.JOB_DTYPE)
    jobs["off"] = np.arange(n, dtype=np.uint64) * a.read_len
    jobs["len"] = a.read_len
    jobs["max_diff"] = opt.max_diff
    jobs["seed_len"] = opt.seed_len
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_codes = torch.from_numpy(_lib.pad_codes(reads.reshape(-1))).cuda()
    hit_cap = n * 8
    o = dict(n=torch.zeros(n, dtype=torch.int32, device="cuda"), f=torch.zeros(n, dtype=torch.int32, device="cuda"),
             o=torch.zeros(n, dtype=torch.int64, device="cuda"),
             h=torch.zeros(hit_cap * _lib.ALN64_WORDS + 2, dtype=torch.int32, device="cuda"),
             c=torch.zeros(16, dtype=torch.int64, device="cuda"))
    b = DeviceBatch(d_jobs=d_jobs.data_ptr(), n_jobs=n, d_codes=d_codes.data_ptr(), d_n_aln=o["n"].data_ptr(),
                    d_flags=o["f"].data_ptr(), d_hit_off=o["o"].data_ptr(), d_hits=o["h"].data_ptr(), hit_cap=hit_cap,
                    d_counters=o["c"].data_ptr(), max_len=a.read_len, max_seed=opt.seed_len)
    gi.search_device64([rg], b)
    torch.cuda.synchronize()
    ctr = o["c"].cpu().numpy()
    log(f"[sa64_probe] searched: {int((o['n'] > 0).sum())} reads with hits, {int(ctr[1])} records, "
        f"{int(ctr[11])} unfinished")

    res = dict(tool="sa64_probe", text_bp=T, interval=s, batch=n, read_len=a.read_len, options="-n 4 -o 0",
               reads_with_hits=int((o["n"] > 0).sum()), hit_records=int(ctr[1]), launches=a.launches, warmup=a.warmup,
               rank_table_bytes=int(T), samples_bytes=int(8 * ((T + s) // s)),
               lf_steps="rows x mean walk of a sample of the rows (hsa_psi_minus_batch64 until a sampled row)", runs=[])
    rng = np.random.default_rng(1)
    # a stream of our own: the launches and the events that time them go to the same one
    tst = torch.cuda.Stream()
    stream = tst.cuda_stream
    assert stream, "need a non-default stream (the library maps NULL to the index's own)"
    for mo in a.max_occ:
        cap = n * mo
        po = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        p = torch.zeros(cap * 4, dtype=torch.int64, device="cuda")
        ph = torch.zeros(cap, dtype=torch.int32, device="cuda")
        c = torch.zeros(4, dtype=torch.int64, device="cuda")
        hb = HitPosBatch64(d_n_aln=o["n"].data_ptr(), d_hit_off=o["o"].data_ptr(), d_hits=o["h"].data_ptr(), n_jobs=n,
                           max_occ=mo, d_pos_off=po.data_ptr(), d_pos=p.data_ptr(), d_pos_hit=ph.data_ptr(),
                           pos_cap=cap, d_counters=c.data_ptr())
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            gi.hit_positions64(hb, stream=stream)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.launches + 1)]
        ev[0].record(tst)
        for i in range(a.launches):
            gi.hit_positions64(hb, stream=stream)
            ev[i + 1].record(tst)
        torch.cuda.synchronize()
        ms = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(a.launches)])
        cc = c.cpu().numpy()
        rows = int(cc[1])
        # the mean walk of a sample of these rows
        tot = int(po[n].item())
        pick = np.sort(rng.choice(tot, min(a.walk_sample, tot), replace=False))
        off = po.cpu().numpy()
        rd = np.searchsorted(off, pick, side="right") - 1
        n_aln, hoff = o["n"].cpu().numpy(), o["o"].cpu().numpy()
        hits = o["h"].cpu().numpy().view(np.uint32)[:hit_cap * _lib.ALN64_WORDS].reshape(-1, _lib.ALN64_WORDS)
        phh = ph.cpu().numpy()
        cur = np.zeros(len(pick), np.uint64)
        for j, (t, r) in enumerate(zip(pick, rd)):
            rest = int(t - off[r])
            for i in range(int(n_aln[r])):
                rec = hits[int(hoff[r]) + i]
                k = int(rec[2]) | int(rec[3]) << 32
                l = int(rec[4]) | int(rec[5]) << 32
                if rest <= l - k:
                    assert i == int(phh[t])
                    cur[j] = k + rest
                    break
                rest -= l - k + 1
        steps = np.zeros(len(cur), np.int64)
        while True:
            act = (cur % np.uint64(s) != 0) & (cur != np.uint64(isa0))
            if not act.any():
                break
            steps[act] += 1
            cur[act] = gi.psi_minus64(cur[act])
        walk = float(steps.mean())
        med = float(np.median(ms))
        run = dict(max_occ=mo, rows=rows, rows_wanted=int(cc[0]), walks_cut=int(cc[2]), ms_median=round(med, 4),
                   ms_min=round(float(ms.min()), 4), ms_max=round(float(ms.max()), 4),
                   rows_per_s=rows / (med * 1e-3), mean_walk=round(walk, 3), max_walk_in_sample=int(steps.max()),
                   lf_steps_per_s=rows * walk / (med * 1e-3))
        if a.chain_log:
            g, tb = chain_rate(a.chain_log, T)
            if g:
                run.update(chain16_Gsectors_per_s=g, chain16_table_bytes=tb,
                           ratio_to_chain16=round(run["lf_steps_per_s"] / (g * 1e9), 4))
        log(f"[sa64_probe] max_occ {mo}: {rows} rows in {med:.3f} ms, {run['rows_per_s'] / 1e6:.1f} M rows/s, "
            f"mean walk {walk:.1f}, {run['lf_steps_per_s'] / 1e9:.2f} G LF steps/s")
        res["runs"].append(run)
        del po, p, ph, c
        torch.cuda.empty_cache()
    gi.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
