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
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from choose_probe import GENOME_SEED, GENOME_T, N_MULTI, RECORDS, log, timed  # noqa: E402

CS, MS = 8, 64                  # cigar_stride, md_stride


def one_set(gi, a, name, reads, max_gapo, tst):
    import torch
    from hsa_amd import _lib, sam
    from hsa_amd._lib import ChooseBatch64, DeviceBatch, GapOpt, RefineBatch64, Regime, SamBatch64
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
    gi.search_device64([rg], b)
    torch.cuda.synchronize()
    sc = o["c"].cpu().numpy()
    log(f"[sam_probe] {name}: {int((o['n'] > 0).sum())} reads with hits, {int(sc[1])} records, {int(sc[11])} unfinished")

    cap = n * (N_MULTI + 1)
    pos = dict(off=z(n + 1, torch.int64), p=z(cap * 4, torch.int64), h=z(cap, torch.int32), c=z(8, torch.int64))
    sel, sel64, rng = z(n * 4, torch.int32), z(n * 4, torch.int64), z(1, torch.int64)
    out = dict(rows=z(cap * _lib.RF_ROW_WORDS, torch.int32), rpos=z(cap * 2, torch.int64), cigar=z(cap * CS, torch.int32),
               md=z(cap * MS, torch.uint8), ctr=z(8, torch.int64))
    cb = ChooseBatch64(d_jobs=d_jobs.data_ptr(), n_jobs=n, d_n_aln=o["n"].data_ptr(), d_hit_off=o["o"].data_ptr(),
                       d_hits=o["h"].data_ptr(), n_multi=N_MULTI, rng_state=_lib.DRAND48_SEED0, d_sel=sel.data_ptr(),
                       d_sel64=sel64.data_ptr(), d_rng_out=rng.data_ptr(), d_pos_off=pos["off"].data_ptr(),
                       d_pos=pos["p"].data_ptr(), d_pos_hit=pos["h"].data_ptr(), pos_cap=cap, d_counters=pos["c"].data_ptr())
    rb = RefineBatch64(d_jobs=d_jobs.data_ptr(), n_jobs=n, d_codes=d_codes.data_ptr(), d_hit_off=o["o"].data_ptr(),
                       d_hits=o["h"].data_ptr(), d_pos_off=pos["off"].data_ptr(), d_pos=pos["p"].data_ptr(),
                       d_pos_hit=pos["h"].data_ptr(), pos_cap=cap, d_pos_counters=pos["c"].data_ptr(), max_len=RL,
                       cigar_stride=CS, md_stride=MS, d_rows=out["rows"].data_ptr(), d_rpos=out["rpos"].data_ptr(),
                       d_cigar=out["cigar"].data_ptr(), d_md=out["md"].data_ptr(), d_counters=out["ctr"].data_ptr())

    def choose_refine():
        gi.choose_hits64(cb, stream=stream)
        gi.refine_rows64(rb, stream=stream)

    res = dict(options=f"-n 4 -o {max_gapo}", reads_with_hits=int((o["n"] > 0).sum()), hit_records=int(sc[1]))
    res["choose_refine"] = timed(choose_refine, tst, a.launches, a.warmup)
    n_rows = int(pos["c"].cpu().numpy()[1])

    # the strings
    names = [f"r{j:07d}" for j in range(n)]
    chrs = [f"chr{r + 1}" for r in range(RECORDS)]
    nb, noff = sam.pack_strings(names)
    cbytes, coff = sam.pack_strings(chrs)
    qual = np.random.default_rng(3).integers(33, 74, n * RL, dtype=np.uint8)
    qoff = np.arange(n + 1, dtype=np.uint64) * np.uint64(RL)
    up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()      # noqa: E731
    s = dict(names=up(nb), name_off=up(noff), chrs=up(cbytes), chr_off=up(coff), quals=up(qual), qual_off=up(qoff))
    max_line = sam.line_bound(8, RL, max(len(c) for c in chrs), CS, MS, N_MULTI)
    out_cap = n * 512
    text = torch.empty(out_cap, dtype=torch.uint8, device="cuda")
    so = dict(off=z(n + 1, torch.int64), st=z(n, torch.int32), c=z(8, torch.int64))
    sb = SamBatch64(d_jobs=d_jobs.data_ptr(), n_jobs=n, d_codes=d_codes.data_ptr(), d_n_aln=o["n"].data_ptr(),
                    d_hit_off=o["o"].data_ptr(), d_hits=o["h"].data_ptr(), d_sel=sel.data_ptr(), d_sel64=sel64.data_ptr(),
                    d_pos_off=pos["off"].data_ptr(), d_pos=pos["p"].data_ptr(), d_pos_hit=pos["h"].data_ptr(), pos_cap=cap,
                    d_pos_counters=pos["c"].data_ptr(), d_rows=out["rows"].data_ptr(), d_rpos=out["rpos"].data_ptr(),
                    d_cigar=out["cigar"].data_ptr(), d_md=out["md"].data_ptr(), cigar_stride=CS, md_stride=MS,
                    d_names=s["names"].data_ptr(), d_name_off=s["name_off"].data_ptr(), d_quals=s["quals"].data_ptr(),
                    d_qual_off=s["qual_off"].data_ptr(), d_chr_names=s["chrs"].data_ptr(), d_chr_off=s["chr_off"].data_ptr(),
                    n_chr=len(chrs), flag=0, max_top2=opt.max_top2, comp_read=1, max_line=max_line,
                    d_line_off=so["off"].data_ptr(), d_out=text.data_ptr(), out_cap=out_cap, d_line_stat=so["st"].data_ptr(),
                    d_counters=so["c"].data_ptr())
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
    ctr = so["c"].cpu().numpy().view(np.uint64)
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
    h = dict(sel=sel.cpu().numpy().view(np.uint32).reshape(-1, 4), sel64=sel64.cpu().numpy().view(np.uint64).reshape(-1, 4),
             pos_off=pos["off"].cpu().numpy(), pos=pos["p"].cpu().numpy().view(np.uint64).reshape(-1, 4),
             pos_hit=pos["h"].cpu().numpy().view(np.uint32), rows=out["rows"].cpu().numpy().view(np.uint32).reshape(-1, 8),
             rpos=out["rpos"].cpu().numpy().view(np.uint64).reshape(-1, 2),
             cigar=out["cigar"].cpu().numpy().view(np.uint32).reshape(-1, CS), md=out["md"].cpu().numpy().reshape(-1, MS),
             hits=o["h"].cpu().numpy().view(np.uint32)[:hit_cap * _lib.ALN64_WORDS].reshape(-1, _lib.ALN64_WORDS),
             hit_off=o["o"].cpu().numpy())
    t_copy = time.perf_counter() - t0
    stat = so["st"].cpu().numpy()
    loff = so["off"].cpu().numpy()
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
                                   max_top2=opt.max_top2)
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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genome", type=int, default=GENOME_T, help="text length (default: hg19-sized)")
    ap.add_argument("--interval", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=10_000, help="reads of the Python loop's sample")
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
    log(f"[sam_probe] index of {T} bp with samples and text in {time.time() - t0:.1f} s")
    genome = synth.PackedGenome(T, GENOME_SEED)
    tst = torch.cuda.Stream()
    assert tst.cuda_stream, "need a non-default stream (the library maps NULL to the index's own)"
    res = dict(tool="sam_probe", text_bp=T, interval=s, batch=n, read_len=RL, n_multi=N_MULTI, launches=a.launches,
               warmup=a.warmup)
    for name, seed, kw, gapo in (("config2", 5 * 1_000_000, dict(max_mm=4), 0),
                                 ("config3", 6 * 1_000_000, dict(indel=True, max_mm_indel=2), 1)):
        t0 = time.time()
        reads, _ = synth.make_reads(genome, recs, n, RL, seed, **kw)
        log(f"[sam_probe] {name}: {n} reads in {time.time() - t0:.1f} s")
        res[name] = one_set(gi, a, name, reads, gapo, tst)
        del reads
        gi.release_scratch()
        torch.cuda.empty_cache()
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
