#!/usr/bin/env python3
"""Time hsa_splice_lines_device (the SAM lines of a batch's spliced reads, on the device).

Builds bench.py's synthetic text at --genome bp (default 100 Mbp) as a 32-bit index with
the sampled SA, the record blocks and the packed text attached (bench.build_index,
bench.attach_splice_arrays), makes --batch spliced reads of --read-len bases
(hsa_amd.synth.make_spliced_reads, config 4's reads), searches them with -n 4 -o 1, runs
hsa_splice_device over the reads without a hit, and times, with HIP events on one stream,
the median of --launches runs after --warmup warm-ups of

  lines    hsa_splice_lines_device of the batch (names r0000000.., random qualities,
           chromosome names chr1..): reads by status, lines and bytes written;
  splice   hsa_splice_device of the same batch: the search the lines come from, expected to
           dominate;
  python   hsa_amd.splice.pair_segments and hsa_amd.sam.spliced_line over a fixed sample of
           --sample printed reads, from host copies of the stage's rows and the SA positions
           of the reads' rows (GpuIndex.sa_positions), scaled to the printed reads
           ("sampled": true).  The sample's lines are also compared with the device text.

No threshold is set: nobody has measured this stage before.  One JSON object on stdout (and
in --out)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from choose_probe import emit, log, parser, probe_batch, timed  # noqa: E402


def main(argv=None):
    ap = parser(__doc__, genome=100_000_000, genome_help="text length (default: 100 Mbp)", read_len=150)
    ap.set_defaults(batch=100_000)
    ap.add_argument("--sample", type=int, default=2_000, help="printed reads of the Python loop's sample")
    a = ap.parse_args(argv)
    from hsa_amd import _lib, chain, sam, splice, synth     # (before torch: _lib loads the HIP runtime it was built for)
    import torch

    import bench
    T, n, RL = a.genome, a.batch, a.read_len
    gi, res_, extra = bench.build_index(T, bench.GENOME_SEED, torch.cuda.current_device(), with_files=True)
    bench.attach_splice_arrays(gi, T, extra)
    del extra
    recs = synth.record_layout(T, bench.RECORDS)
    reads, _ = synth.make_spliced_reads(synth.PackedGenome(T, bench.GENOME_SEED), recs, n, RL, 7 * 1_000_000 + 91)
    tst = torch.cuda.Stream()
    stream = tst.cuda_stream
    assert stream, "need a non-default stream (the library maps NULL to the index's own)"
    opt = _lib.GapOpt.default()
    opt.max_diff, opt.fnr, opt.max_gapo = 4, -1.0, 1
    opt = opt.as_dict()
    local, n_stacks, rg = chain.local_regime(opt, RL)
    bt = probe_batch(reads, RL, opt)
    db, t = chain.search64_batch(bt, 0, n, n * 16, opt["seed_len"])
    db.hit_cap = n * 16
    # (the 32-bit search writes 9-word records; only n_aln and the flags are used here)
    gi.search_device([rg], db)
    torch.cuda.synchronize()
    srg = chain.splice_regimes(local, n_stacks)
    sb, s = chain.splice32_batch(bt, t, 0, n)
    res = dict(tool="splice_lines_probe", text_bp=T, batch=n, read_len=RL, options="-n 4 -o 1", launches=a.launches,
               warmup=a.warmup)

    def splice_call():
        gi.splice_device(srg[0], srg[1], srg[2], sb)        # (on the index's own stream: the events wait for it)
        torch.cuda.synchronize()

    t0 = time.perf_counter()
    splice_call()
    first_s = time.perf_counter() - t0
    ms = []
    for _ in range(max(1, a.launches // 2)):
        t0 = time.perf_counter()
        splice_call()
        ms.append((time.perf_counter() - t0) * 1e3)
    sp = s["sp_ctr"].cpu().numpy()
    res["splice"] = dict(ms_median=round(float(np.median(ms)), 3), first_call_s=round(first_s, 3), wall_clock=True,
                         reads_sent=int(sp[0]), not_answered=int(sp[4]))

    names = [f"r{j:07d}" for j in range(n)]
    chrs = [f"chr{r + 1}" for r in range(bench.RECORDS)]
    nb, noff = sam.pack_strings(names)
    cbytes, coff = sam.pack_strings(chrs)
    qual = np.random.default_rng(3).integers(33, 74, n * RL, dtype=np.uint8)
    qoff = np.arange(n + 1, dtype=np.uint64) * np.uint64(RL)
    up = chain.to_device
    strings = dict(names=up(nb), name_off=up(noff), chrs=up(cbytes), chr_off=up(coff), quals=up(qual), qual_off=up(qoff))
    stride = 33
    max_line = sam.line_bound(8, RL, max(len(c) for c in chrs), stride, 0, 0)
    lb, o = chain.splice_lines_batch(bt, s, 0, n, strings, len(chrs), max_line, n * (2 * RL + 160), cigar_stride=stride,
                                     max_top2=opt["max_top2"])
    torch.cuda.synchronize()

    def lines_call():
        gi.splice_lines(lb, stream=stream)

    res["lines"] = timed(lines_call, tst, a.launches, a.warmup)
    ctr = o["ctr"].cpu().numpy().view(np.uint64)
    assert int(ctr[0]) == int(ctr[1]), "the probe's out_cap is too small"
    res["lines"].update(bytes_written=int(ctr[1]), lines=int(ctr[2]), handed_back=int(ctr[3]), multi=int(ctr[4]),
                        refused=int(ctr[5]), no_pair=int(ctr[6]), spliced_results=int(ctr[7]), max_line=max_line,
                        share_of_splice=round(res["lines"]["ms_median"] / max(res["splice"]["ms_median"], 1e-9), 4))

    # the Python restatement on a sample of the printed reads
    stat = o["stat"].cpu().numpy().view(np.uint32)[:n]
    rows = o["rows"].cpu().numpy().view(np.uint32).reshape(-1, _lib.SL_ROW_WORDS)
    cig = o["cigar"].cpu().numpy().view(np.uint32).reshape(-1, stride)
    r = s["res"].cpu().numpy().view(np.uint32).reshape(-1, _lib.SP_RES_WORDS)
    loff = o["line_off"].cpu().numpy().view(np.uint64)
    text = o["out"][:int(ctr[1])].cpu().numpy()
    ok = np.flatnonzero(stat == _lib.HSA_SL_OK)
    sample = np.sort(np.random.default_rng(11).choice(ok, min(a.sample, len(ok)), replace=False)) if len(ok) else ok
    qs = qual.reshape(n, RL)
    t0 = time.perf_counter()
    same = True
    for j in sample:
        k0, l0, k1, l1 = int(r[j, 3]), int(r[j, 4]), int(r[j, 12]), int(r[j, 13])
        n0, n1 = splice.segment_rows(k0, l0), splice.segment_rows(k1, l1)
        p = gi.sa_positions(np.array(list(range(k0, k0 + n0)) + list(range(k1, k1 + n1)), np.uint32))
        found = p[:, 1] != 0xFFFFFFFF
        table = np.stack([(np.arange(len(p)) >= n0).astype(np.int64), np.where(found, p[:, 1], 0).astype(np.int64),
                          np.where(found, p[:, 2], 0).astype(np.int64), p[:, 3].astype(np.int64)], axis=1)
        n_res, pair = splice.pair_segments(table)
        row = rows[j]
        strand = int(row[4])
        cigar = [(int(w) >> 28, int(w) & 0x0FFFFFFF) for w in cig[j, :int(row[5])]]
        line = sam.spliced_line(names[j], reads[j], qs[j].tobytes().decode(), chrs[int(table[pair[0], 1])], int(row[7]), cigar,
                                strand, splice.capped_multi(k0, l0, k1, l1), int(row[3]), int(row[19]), max_top2=opt["max_top2"])
        same = same and n_res == 1 and text[int(loff[j]):int(loff[j + 1])].tobytes() == (line + "\n").encode()
    t_loop = time.perf_counter() - t0
    res["python"] = dict(sampled=True, sample_lines=int(len(sample)), loop_s=round(t_loop, 3),
                         batch_s=round(t_loop * len(ok) / max(len(sample), 1), 2), sample_lines_equal_device_text=bool(same))
    log(f"[splice_lines_probe] lines {res['lines']['ms_median']:.3f} ms for {int(ctr[2])} lines, splice "
        f"{res['splice']['ms_median']:.1f} ms, python {res['python']['batch_s']} s (sampled), sample equal: {same}")
    gi.close()
    return emit(res, a.out)


if __name__ == "__main__":
    sys.exit(main())
