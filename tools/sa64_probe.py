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
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from choose_probe import GENOME_SEED, RECORDS, emit, log, parser, probe_batch, probe_opts, timed_ms  # noqa: E402

GENOME5_T = 15_000_000_003      # bench.py's config 5


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
    ap = parser(__doc__, GENOME5_T, "text length (default: config 5's 15 Gbp)", 250)
    ap.add_argument("--max-occ", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--walk-sample", type=int, default=20_000)
    ap.add_argument("--chain-log", default=None, help="output of `tools/gather_probe chain16`")
    a = ap.parse_args(argv)

    from hsa_amd import _lib, chain, synth
    import torch
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
    opt = probe_opts(0)
    rg = chain.local_regime(opt, a.read_len)[2]
    n = a.batch
    hit_cap = n * 8
    bt = probe_batch(reads, a.read_len, opt)             # (kept: b holds addresses into its tensors)
    b, o = chain.search64_batch(bt, 0, n, hit_cap, opt["seed_len"])
    gi.search_device64([rg], b)
    torch.cuda.synchronize()
    ctr = o["sc"].cpu().numpy()
    log(f"[sa64_probe] searched: {int((o['n_aln'] > 0).sum())} reads with hits, {int(ctr[1])} records, "
        f"{int(ctr[11])} unfinished")

    res = dict(tool="sa64_probe", text_bp=T, interval=s, batch=n, read_len=a.read_len, options="-n 4 -o 0",
               reads_with_hits=int((o["n_aln"] > 0).sum()), hit_records=int(ctr[1]), launches=a.launches, warmup=a.warmup,
               rank_table_bytes=int(T), samples_bytes=int(8 * ((T + s) // s)),
               lf_steps="rows x mean walk of a sample of the rows (hsa_psi_minus_batch64 until a sampled row)", runs=[])
    rng = np.random.default_rng(1)
    # a stream of our own: the launches and the events that time them go to the same one
    tst = torch.cuda.Stream()
    stream = tst.cuda_stream
    assert stream, "need a non-default stream (the library maps NULL to the index's own)"
    for mo in a.max_occ:
        hb, pos = chain.hit_positions64_batch(o, n, mo)
        po, ph, c = pos["pos_off"], pos["pos_hit"], pos["pos_ctr"]
        torch.cuda.synchronize()
        ms = timed_ms(lambda: gi.hit_positions64(hb, stream=stream), tst, a.launches, a.warmup)
        cc = c.cpu().numpy()
        rows = int(cc[1])
        # the mean walk of a sample of these rows
        tot = int(po[n].item())
        pick = np.sort(rng.choice(tot, min(a.walk_sample, tot), replace=False))
        off = po.cpu().numpy()
        rd = np.searchsorted(off, pick, side="right") - 1
        n_aln, hoff = o["n_aln"].cpu().numpy(), o["hit_off"].cpu().numpy()
        hits = o["hits"].cpu().numpy().view(np.uint32)[:hit_cap * _lib.ALN64_WORDS].reshape(-1, _lib.ALN64_WORDS)
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
        del hb, pos, po, ph, c
        torch.cuda.empty_cache()
    gi.close()
    return emit(res, a.out)


if __name__ == "__main__":
    sys.exit(main())
