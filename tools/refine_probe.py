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
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from choose_probe import GENOME_SEED, emit, log, parser, probe_batch, probe_opts, synthetic_index, timed_ms  # noqa: E402

BAND = 50                       # aln_param_bwa's band_width (stdaln.c:227)


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
    ap = parser(__doc__)
    ap.add_argument("--max-occ", type=int, default=8)
    a = ap.parse_args(argv)

    from hsa_amd import _lib, chain, synth
    import torch
    T, s, n, RL = a.genome, a.interval, a.batch, a.read_len
    gi, recs = synthetic_index(a, "refine_probe")

    t0 = time.time()
    genome = synth.PackedGenome(T, GENOME_SEED)
    reads, _ = synth.make_reads(genome, recs, n, RL, 6 * 1_000_000, indel=True, max_mm_indel=2)
    del genome
    log(f"[refine_probe] {n} reads in {time.time() - t0:.1f} s")
    opt = probe_opts(1)
    rg = chain.local_regime(opt, RL)[2]
    bt = probe_batch(reads, RL, opt)
    hit_cap = n * 16
    b, o = chain.search64_batch(bt, 0, n, hit_cap, opt["seed_len"])
    search_ms = []
    for _ in range(3):              # the last pass's kernel times: a warm search of the same batch
        gi.search_device64([rg], b)
        torch.cuda.synchronize()
        search_ms.append(gi.last_pass_ms())
    ctr = o["sc"].cpu().numpy()
    log(f"[refine_probe] searched: {int((o['n_aln'] > 0).sum())} reads with hits, {int(ctr[1])} records, "
        f"{int(ctr[11])} unfinished; k_widths {search_ms[-1][0]:.2f} ms, k_search {search_ms[-1][1]:.2f} ms")

    hb, pos = chain.hit_positions64_batch(o, n, a.max_occ)
    gi.hit_positions64(hb)
    torch.cuda.synchronize()
    rbatch, out = chain.refine64_batch(dict(bt, **o, **pos), 8, 64)
    # a stream of our own: the launches and the events that time them go to the same one
    tst = torch.cuda.Stream()
    assert tst.cuda_stream, "need a non-default stream (the library maps NULL to the index's own)"
    torch.cuda.synchronize()
    ms = timed_ms(lambda: gi.refine_rows64(rbatch, stream=tst.cuda_stream), tst, a.launches, a.warmup)
    rc = out["ctr"].cpu().numpy()
    rows, dp_rows = int(rc[0]), int(rc[6])
    # the DP rows' cells, from their shapes (every window of these reads is whole: len + gap)
    rw = out["rows"].cpu().numpy().view(np.uint32).reshape(-1, _lib.RF_ROW_WORDS)[:rows]
    off = pos["pos_off"].cpu().numpy()
    hits = o["hits"].cpu().numpy().view(np.uint32)[:hit_cap * _lib.ALN64_WORDS].reshape(-1, _lib.ALN64_WORDS)
    read_of = np.repeat(np.arange(n), np.diff(off))[:rows]
    rec = hits[o["hit_off"].cpu().numpy()[read_of] + pos["pos_hit"].cpu().numpy().view(np.uint32)[:rows]]
    gap = ((rec[:, 0] >> 16) & 0xFF) + (rec[:, 0] >> 24)
    cells = sum(int(c) * band_cells(RL, RL + int(g)) for g, c in zip(*np.unique(gap[gap > 0], return_counts=True)))
    med = float(np.median(ms))
    names = ["ok", "pos", "text", "cap", "md"]
    res = dict(tool="refine_probe", text_bp=T, interval=s, batch=n, read_len=RL, options="-n 4 -o 1",
               max_occ=a.max_occ, reads_with_hits=int((o["n_aln"] > 0).sum()), hit_records=int(ctr[1]),
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
    return emit(res, a.out)


if __name__ == "__main__":
    sys.exit(main())
