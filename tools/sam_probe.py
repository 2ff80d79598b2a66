#!/usr/bin/env python3
"""Time hsa_sam_lines_device64 (the SAM lines of a batch written on the device).

Builds the synthetic hg19-sized text of tools/choose_probe.py with
hsa_index_create_device64 (suffix array sampled every `--interval` rows, text attached),
and for the config-2 read set (100 bp, up to 4 substitutions, -n 4 -o 0) and the config-3
set (one indel of 1-3 bp and 0-2 substitutions, -n 4 -o 1) searches the batch with
hsa_search_device64, chooses and refines it, and times, with HIP events on one stream,
the median of --launches runs after --warmup warm-ups of

  sam             hsa_sam_lines_device64 of the batch (names r0000000.., random qualities,
                  chromosome names chr1..), and its three launches one by one
                  (hsa_sam_timing); the bytes written, and GB/s of (bytes read + written)
                  with the bytes read counted once per input array as the line needs them;
  copy            a device-to-device copy of exactly the bytes written: the streaming
                  yardstick;
  choose_refine   hsa_choose_hits_device64 then hsa_refine_rows_device64 of the same batch;
  python          hsa_amd.sam.sam_line over a fixed sample of --sample reads, with the
                  device-to-host copies of the arrays it slices, scaled to the batch
                  ("sampled": true).  The sample's lines are also compared with the device
                  text.

One JSON object on stdout (and in --out)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from choose_probe import N_MULTI, RECORDS, emit, log, parser, probe_batch, probe_opts, run_sets, timed  # noqa: E402

CS, MS = 8, 64                  # cigar_stride, md_stride


def one_set(gi, a, name, reads, max_gapo, tst):
    import torch
    from hsa_amd import _lib, chain, sam
    n, RL, stream = a.batch, a.read_len, tst.cuda_stream
    opt = probe_opts(max_gapo)
    bt = probe_batch(reads, RL, opt)
    hit_cap = n * 16
    b, o = chain.search64_batch(bt, 0, n, hit_cap, opt["seed_len"])
    gi.search_device64([chain.local_regime(opt, RL)[2]], b)
    torch.cuda.synchronize()
    sc = o["sc"].cpu().numpy()
    log(f"[sam_probe] {name}: {int((o['n_aln'] > 0).sum())} reads with hits, {int(sc[1])} records, {int(sc[11])} unfinished")

    cb, pos = chain.choose64_batch(bt, o, 0, n, _lib.DRAND48_SEED0)
    rb, out = chain.refine64_batch(pos, CS, MS)

    def choose_refine():
        gi.choose_hits64(cb, stream=stream)
        gi.refine_rows64(rb, stream=stream)

    res = dict(options=f"-n 4 -o {max_gapo}", reads_with_hits=int((o["n_aln"] > 0).sum()), hit_records=int(sc[1]))
    res["choose_refine"] = timed(choose_refine, tst, a.launches, a.warmup)
    n_rows = int(pos["pos_ctr"].cpu().numpy()[1])

    # the strings
    names = [f"r{j:07d}" for j in range(n)]
    chrs = [f"chr{r + 1}" for r in range(RECORDS)]
    nb, noff = sam.pack_strings(names)
    cbytes, coff = sam.pack_strings(chrs)
    qual = np.random.default_rng(3).integers(33, 74, n * RL, dtype=np.uint8)
    qoff = np.arange(n + 1, dtype=np.uint64) * np.uint64(RL)
    up = chain.to_device
    s = dict(names=up(nb), name_off=up(noff), chrs=up(cbytes), chr_off=up(coff), quals=up(qual), qual_off=up(qoff))
    max_line = sam.line_bound(8, RL, max(len(c) for c in chrs), CS, MS, N_MULTI)
    sb, so = chain.sam_lines64_batch(out, s, len(chrs), max_line, n * 512, max_top2=opt["max_top2"])
    text = so["out"]
    torch.cuda.synchronize()

    def sam_call():
        gi.sam_lines64(sb, stream=stream)

    res["sam"] = timed(sam_call, tst, a.launches, a.warmup)
    _lib.lib().hsa_sam_timing(1)
    split = []
    for _ in range(a.launches):
        sam_call()
        split.append(gi.sam_launch_times())
    _lib.lib().hsa_sam_timing(0)
    ctr = so["ctr"].cpu().numpy().view(np.uint64)
    assert int(ctr[0]) == int(ctr[1]), "the probe's out_cap is too small"
    written, lines = int(ctr[1]), int(ctr[2])
    # bytes the lines need, each input array once: per read its job, selection words, offsets
    # and strings; per row its position, record, refinement words, the ops and MD bytes used
    rows_np = out["rows"].cpu().numpy().view(np.uint32).reshape(-1, _lib.RF_ROW_WORDS)[:n_rows]
    read_b = n * (24 + 16 + 32 + 8 + 8 + 4 + 8 + 8) + lines * (2 * RL) + int(len(nb)) + \
        n_rows * (32 + 4 + 56 + 32 + 16) + int(rows_np[:, 1].sum()) * 4 + int(rows_np[:, 3].sum())
    ms = res["sam"]["ms_median"]
    lm = {k: round(float(np.median([x[k] for x in split])), 4) for k in split[0]}
    res["sam"].update(launch_ms_median=lm, bytes_written=written, bytes_read=read_b, lines=lines,
                      reads_by_status=[lines] + [int(c) for c in ctr[3:7]], max_line=max_line,
                      gb_per_s=round((read_b + written) / ms / 1e6, 1),
                      write_kernel_gb_per_s=round((read_b + written) / max(lm["write"], 1e-9) / 1e6, 1))
    dst = torch.empty(max(written, 1), dtype=torch.uint8, device="cuda")

    def copy():
        with torch.cuda.stream(tst):
            dst[:written].copy_(text[:written])

    res["copy"] = timed(copy, tst, a.launches, a.warmup)
    res["copy"].update(bytes=written, gb_per_s=round(2 * written / res["copy"]["ms_median"] / 1e6, 1))
    res["sam"]["write_kernel_vs_copy"] = round(res["copy"]["ms_median"] / max(lm["write"], 1e-9), 4)

    # the Python loop on a fixed sample, with the copies of the arrays it slices
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = dict(sel=pos["sel"].cpu().numpy().view(np.uint32).reshape(-1, 4),
             sel64=pos["sel64"].cpu().numpy().view(np.uint64).reshape(-1, 4),
             pos_off=pos["pos_off"].cpu().numpy(), pos=pos["pos"].cpu().numpy().view(np.uint64).reshape(-1, 4),
             pos_hit=pos["pos_hit"].cpu().numpy().view(np.uint32), rows=out["rows"].cpu().numpy().view(np.uint32).reshape(-1, 8),
             rpos=out["rpos"].cpu().numpy().view(np.uint64).reshape(-1, 2),
             cigar=out["cigar"].cpu().numpy().view(np.uint32).reshape(-1, CS), md=out["md"].cpu().numpy().reshape(-1, MS),
             hits=o["hits"].cpu().numpy().view(np.uint32)[:hit_cap * _lib.ALN64_WORDS].reshape(-1, _lib.ALN64_WORDS),
             hit_off=o["hit_off"].cpu().numpy())
    t_copy = time.perf_counter() - t0
    stat = so["stat"].cpu().numpy()
    loff = so["line_off"].cpu().numpy()
    host_text = text[:written].cpu().numpy()
    sample = np.sort(np.random.default_rng(11).choice(n, min(a.sample, n), replace=False))
    qs = qual.reshape(n, RL)
    t0 = time.perf_counter()
    got = {}
    for j in sample:
        if stat[j] != 0:
            continue
        r0, r1 = int(h["pos_off"][j]), int(h["pos_off"][j + 1])
        recs = h["hits"][int(h["hit_off"][j]) + h["pos_hit"][r0:r1].astype(np.int64)]
        got[int(j)] = sam.sam_line(names[j], reads[j], qs[j].tobytes().decode(), chrs, h["sel"][j], h["sel64"][j],
                                   h["rows"][r0:r1], h["rpos"][r0:r1], h["cigar"][r0:r1], h["md"][r0:r1], h["pos"][r0:r1], recs,
                                   max_top2=opt["max_top2"])
    t_loop = time.perf_counter() - t0
    same = all(host_text[int(loff[j]):int(loff[j + 1])].tobytes() == (ln + "\n").encode() for j, ln in got.items())
    res["python"] = dict(sampled=True, sample_reads=int(len(sample)), sample_lines=len(got), copies_s=round(t_copy, 3),
                         loop_s=round(t_loop, 3), batch_s=round(t_copy + t_loop * n / max(len(sample), 1), 1),
                         sample_lines_equal_device_text=bool(same))
    log(f"[sam_probe] {name}: sam {ms:.3f} ms ({lm}), {written} bytes, copy {res['copy']['ms_median']:.3f} ms, "
        f"choose + refine {res['choose_refine']['ms_median']:.3f} ms, python {res['python']['batch_s']} s (sampled), "
        f"sample equal: {same}")
    return res


def main(argv=None):
    ap = parser(__doc__)
    ap.add_argument("--sample", type=int, default=10_000, help="reads of the Python loop's sample")
    a = ap.parse_args(argv)
    gi, _, res = run_sets("sam_probe", a, one_set)
    gi.close()
    return emit(res, a.out)


if __name__ == "__main__":
    sys.exit(main())
