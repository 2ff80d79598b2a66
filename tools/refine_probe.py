#!/usr/bin/env python3
"""Time hsa_refine_rows_device64 (position rows of the 64-bit path to CIGAR, NM and MD).

Builds a synthetic hg19-sized text with hsa_index_create_device64 (the text kept on the
device and attached with hsa_index_set_text64_device, its suffix array sampled every
`--interval` rows), searches one config-3 read set (100 bp, one indel of 1-3 bp and 0-2
substitutions, -n 4 -o 1) with hsa_search_device64, turns the hit lists into position
rows (hsa_hit_positions_device64, --max-occ rows per read) and times
hsa_refine_rows_device64 with HIP events over --launches launches after --warmup
warm-ups.

Reported: the call's time (median), rows/s, DP rows/s, DP cells/s (a DP row's cells: the
in-band cells of its len x (len + gap) matrix, computed from the rows' shapes on the
host), the share of rows per status, and beside them the k_search time of the same batch
(hsa_last_pass_ms), so that a reader sees what the step adds to a search.

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

GENOME_T = 3_000_000_005        # bench.py's hg19-sized text
GENOME_SEED = 1234              # bench.py's GENOME_SEED
RECORDS = 24                    # bench.py's RECORDS
BAND = 50                       # aln_param_bwa's band_width (stdaln.c:227)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def band_cells(len2, len1):
    """In-band cells of aln_global_core's matrix (stdaln.c:372-485): rows 1..len2, columns
    lo(j) + 1 .. min(j + b1 - 1, len1)."""
    if len1 > len2:
        b1, b2 = len1 - len2 + BAND, BAND
    else:
        b1, b2 = BAND, len2 - len1 + BAND
    b1, b2 = min(b1, len1), min(b2, len2)
    j = np.arange(1, len2 + 1)
    lo = np.where(j <= b2, 0, j - b2)
    return int((np.minimum(j + b1 - 1, len1) - lo).sum())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genome", type=int, default=GENOME_T, help="text length (default: hg19-sized)")
    ap.add_argument("--interval", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--max-occ", type=int, default=8)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from hsa_amd import _lib, synth
    import torch
    from hsa_amd._lib import DeviceBatch, DeviceU64, GapOpt, HitPosBatch64, RefineBatch64, Regime
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
    log(f"[refine_probe] index of {T} bp with samples and text in {time.time() - t0:.1f} s")

    t0 = time.time()
    genome = synth.PackedGenome(T, GENOME_SEED)
    reads, _ = synth.make_reads(genome, recs, n, RL, 6 * 1_000_000, indel=True, max_mm_indel=2)
    del genome
    log(f"[refine_probe] {n} reads in {time.time() - t0:.1f} s")
    opt = GapOpt.default()
    opt.max_diff, opt.fnr, opt.max_gapo = 4, -1.0, 1
    opt.mode &= ~0x01
    n_stacks = (opt.max_diff + 1) * opt.s_mm + (opt.max_gapo + 1) * opt.s_gapo + (opt.max_gape + 1) * opt.s_gape
    rg = Regime(s_mm=opt.s_mm, s_gapo=opt.s_gapo, s_gape=opt.s_gape, mode=0, indel_end_skip=opt.indel_end_skip,
                max_del_occ=opt.max_del_occ, max_entries=opt.max_entries, max_gapo=1, max_gape=opt.max_gape,
                max_seed_diff=opt.max_seed_diff, max_top2=opt.max_top2, n_stacks=n_stacks, max_diff=opt.max_diff)
    jobs = np.zeros(n, _lib.JOB_DTYPE)
    jobs["off"] = np.arange(n, dtype=np.uint64) * RL
    jobs["len"] = RL
    jobs["max_diff"] = opt.max_diff
    jobs["seed_len"] = opt.seed_len
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_codes = torch.from_numpy(_lib.pad_codes(reads.reshape(-1))).cuda()
    hit_cap = n * 16
    o = dict(n=torch.zeros(n, dtype=torch.int32, device="cuda"), f=torch.zeros(n, dtype=torch.int32, device="cuda"),
             o=torch.zeros(n, dtype=torch.int64, device="cuda"),
             h=torch.zeros(hit_cap * _lib.ALN64_WORDS + 2, dtype=torch.int32, device="cuda"),
             c=torch.zeros(16, dtype=torch.int64, device="cuda"))
    b = DeviceBatch(d_jobs=d_jobs.data_ptr(), n_jobs=n, d_codes=d_codes.data_ptr(), d_n_aln=o["n"].data_ptr(),
                    d_flags=o["f"].data_ptr(), d_hit_off=o["o"].data_ptr(), d_hits=o["h"].data_ptr(), hit_cap=hit_cap,
                    d_counters=o["c"].data_ptr(), max_len=RL, max_seed=opt.seed_len)
    search_ms = []
    for _ in range(3):              # the last pass's kernel times: a warm search of the same batch
        gi.search_device64([rg], b)
        torch.cuda.synchronize()
        search_ms.append(gi.last_pass_ms())
    ctr = o["c"].cpu().numpy()
    log(f"[refine_probe] searched: {int((o['n'] > 0).sum())} reads with hits, {int(ctr[1])} records, "
        f"{int(ctr[11])} unfinished; k_widths {search_ms[-1][0]:.2f} ms, k_search {search_ms[-1][1]:.2f} ms")

    cap = n * a.max_occ
    po = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    p = torch.zeros(cap * 4, dtype=torch.int64, device="cuda")
    ph = torch.zeros(cap, dtype=torch.int32, device="cuda")
    pc = torch.zeros(4, dtype=torch.int64, device="cuda")
    hb = HitPosBatch64(d_n_aln=o["n"].data_ptr(), d_hit_off=o["o"].data_ptr(), d_hits=o["h"].data_ptr(), n_jobs=n,
                       max_occ=a.max_occ, d_pos_off=po.data_ptr(), d_pos=p.data_ptr(), d_pos_hit=ph.data_ptr(),
                       pos_cap=cap, d_counters=pc.data_ptr())
    gi.hit_positions64(hb)
    torch.cuda.synchronize()
    cs, ms_ = 8, 64
    out = dict(rows=torch.zeros(cap * _lib.RF_ROW_WORDS, dtype=torch.int32, device="cuda"),
               rpos=torch.zeros(cap * 2, dtype=torch.int64, device="cuda"),
               cigar=torch.zeros(cap * cs, dtype=torch.int32, device="cuda"),
               md=torch.zeros(cap * ms_, dtype=torch.uint8, device="cuda"),
               ctr=torch.zeros(8, dtype=torch.int64, device="cuda"))
    rbatch = RefineBatch64(d_jobs=d_jobs.data_ptr(), n_jobs=n, d_codes=d_codes.data_ptr(), d_hit_off=o["o"].data_ptr(),
                           d_hits=o["h"].data_ptr(), d_pos_off=po.data_ptr(), d_pos=p.data_ptr(),
                           d_pos_hit=ph.data_ptr(), pos_cap=cap, d_pos_counters=pc.data_ptr(), max_len=RL,
                           cigar_stride=cs, md_stride=ms_, d_rows=out["rows"].data_ptr(), d_rpos=out["rpos"].data_ptr(),
                           d_cigar=out["cigar"].data_ptr(), d_md=out["md"].data_ptr(), d_counters=out["ctr"].data_ptr())
    # a stream of our own: the launches and the events that time them go to the same one
    tst = torch.cuda.Stream()
    stream = tst.cuda_stream
    assert stream, "need a non-default stream (the library maps NULL to the index's own)"
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        gi.refine_rows64(rbatch, stream=stream)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.launches + 1)]
    ev[0].record(tst)
    for i in range(a.launches):
        gi.refine_rows64(rbatch, stream=stream)
        ev[i + 1].record(tst)
    torch.cuda.synchronize()
    ms = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(a.launches)])
    rc = out["ctr"].cpu().numpy()
    rows, dp_rows = int(rc[0]), int(rc[6])
    # the DP rows' cells, from their shapes (every window of these reads is whole: len + gap)
    rw = out["rows"].cpu().numpy().view(np.uint32).reshape(-1, _lib.RF_ROW_WORDS)[:rows]
    off = po.cpu().numpy()
    hits = o["h"].cpu().numpy().view(np.uint32)[:hit_cap * _lib.ALN64_WORDS].reshape(-1, _lib.ALN64_WORDS)
    read_of = np.repeat(np.arange(n), np.diff(off))[:rows]
    rec = hits[o["o"].cpu().numpy()[read_of] + ph.cpu().numpy().view(np.uint32)[:rows]]
    gap = ((rec[:, 0] >> 16) & 0xFF) + (rec[:, 0] >> 24)
    cells = sum(int(c) * band_cells(RL, RL + int(g)) for g, c in zip(*np.unique(gap[gap > 0], return_counts=True)))
    med = float(np.median(ms))
    names = ["ok", "pos", "text", "cap", "md"]
    res = dict(tool="refine_probe", text_bp=T, interval=s, batch=n, read_len=RL, options="-n 4 -o 1",
               max_occ=a.max_occ, reads_with_hits=int((o["n"] > 0).sum()), hit_records=int(ctr[1]),
               launches=a.launches, warmup=a.warmup, rows=rows, dp_rows=dp_rows, dp_cells=cells,
               ms_median=round(med, 4), ms_min=round(float(ms.min()), 4), ms_max=round(float(ms.max()), 4),
               rows_per_s=rows / (med * 1e-3), dp_rows_per_s=dp_rows / (med * 1e-3), dp_cells_per_s=cells / (med * 1e-3),
               status_share={k: (int(rc[1 + i]) / rows if rows else 0.0) for i, k in enumerate(names)},
               mean_nm=float(rw[rw[:, 0] == 0, 2].mean()) if rows else 0.0,
               k_widths_ms=round(float(search_ms[-1][0]), 4), k_search_ms=round(float(search_ms[-1][1]), 4),
               traceback="per-wave HBM scratch", host_sam_refine_ms=None)
    log(f"[refine_probe] {rows} rows ({dp_rows} DP) in {med:.3f} ms: {res['rows_per_s'] / 1e6:.1f} M rows/s, "
        f"{res['dp_rows_per_s'] / 1e6:.2f} M DP rows/s, {res['dp_cells_per_s'] / 1e9:.1f} G cells/s; "
        f"k_search of the batch {res['k_search_ms']:.2f} ms")
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
