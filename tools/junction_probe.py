#!/usr/bin/env python3
"""Time the junction table's device stages (hsa_junction_rows_device, hsa_junction_reduce_device,
hsa_junction_text_device) on the batch of tools/splice_lines_probe.py.

Builds bench.py's synthetic text at --genome bp (default 100 Mbp) as a 32-bit index with the
sampled SA, the record blocks and the packed text attached, makes --batch spliced reads of
--read-len bases, searches them with -n 4 -o 1, runs hsa_splice_device over the reads without a
hit and hsa_splice_lines_device_xa over its results, and times, with HIP events on one stream,
the median of --launches runs after --warmup warm-ups of

  junctions  rows + reduce + text of the batch, each run from an empty row buffer (the three
             calls back to back, no host round trip: the row count the reduction is given is
             the lines call's printed lines, known from its counters);
  rows, rows_reduce, text   the rows call, the rows and the reduce call (the reduction works in
             place, so its input is put back first), the text call;
  lines      hsa_splice_lines_device_xa of the same batch, in the same process;
  python     hsa_amd.junctions.table_of (from_sam on an index in memory) over the batch's SAM
             text, wall clock, once; its bytes are compared with the device's.

No threshold is set: nobody has measured this stage before.  One JSON object on stdout (and in
--out)."""
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
    ap.set_defaults(batch=100_000, warmup=3, out=os.path.join(ROOT, "profiles", "junction_probe.json"))
    a = ap.parse_args(argv)
    from hsa_amd import _lib, chain, index_io, junctions, sam, synth     # (before torch: _lib loads the HIP runtime it was built for)
    import torch

    import bench
    T, n, RL = a.genome, a.batch, a.read_len
    gi, res_, extra = bench.build_index(T, bench.GENOME_SEED, torch.cuda.current_device(), with_files=True)
    bench.attach_splice_arrays(gi, T, extra)
    pac = index_io.unpack_lsb_u32(extra["text"], T)
    del extra
    recs = synth.record_layout(T, bench.RECORDS)
    blocks = np.array([[r, s0, s0 + m - 1, 0] for r, (s0, m) in enumerate(recs)], np.int64)
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
    gi.search_device([rg], db)
    torch.cuda.synchronize()
    srg = chain.splice_regimes(local, n_stacks)
    sb, s = chain.splice32_batch(bt, t, 0, n)
    gi.splice_device(srg[0], srg[1], srg[2], sb)
    torch.cuda.synchronize()
    res = dict(tool="junction_probe", text_bp=T, batch=n, read_len=RL, options="-n 4 -o 1", launches=a.launches, warmup=a.warmup)

    names = [f"r{j:07d}" for j in range(n)]
    chrs = [f"chr{r + 1}" for r in range(bench.RECORDS)]
    nb, noff = sam.pack_strings(names)
    cbytes, coff = sam.pack_strings(chrs)
    qual = np.random.default_rng(3).integers(33, 74, n * RL, dtype=np.uint8)
    qoff = np.arange(n + 1, dtype=np.uint64) * np.uint64(RL)
    up = chain.to_device
    strings = dict(names=up(nb), name_off=up(noff), chrs=up(cbytes), chr_off=up(coff), quals=up(qual), qual_off=up(qoff))
    stride = 33
    max_line = sam.line_bound(8, RL, max(len(c) for c in chrs), stride, 0, 49)
    o, ctr = chain.splice_lines(gi, bt, s, 0, n, strings, len(chrs), max_line, n * (2 * RL + 160), cigar_stride=stride,
                                max_top2=opt["max_top2"])
    n_lines, room = int(ctr[2]), int(o["pair_cap"])
    lb, o = chain.splice_lines_batch(bt, s, 0, n, strings, len(chrs), max_line, int(ctr[0]), cigar_stride=stride, max_top2=opt["max_top2"])
    xa, ox = chain.splice_xa_batch(n, room, stride)
    torch.cuda.synchronize()
    res["lines"] = timed(lambda: gi.splice_lines(lb, stream=stream, xa=xa), tst, a.launches, a.warmup)
    c2 = o["ctr"].cpu().numpy().view(np.uint64)
    assert int(c2[2]) == n_lines and int(c2[0]) == int(c2[1]), "the timed lines call is not the driver's"
    res["lines"].update(lines=n_lines, bytes_written=int(c2[1]), with_xa=int(ox["xa_ctr"].cpu().numpy().view(np.uint64)[2]))
    sam_text = o["out"][:int(c2[1])].cpu().numpy().tobytes()

    # the three calls, from an empty buffer each run
    jrows = torch.zeros(max(n_lines, 1) * _lib.JN_ROW_WORDS, dtype=torch.int32, device="cuda")
    jb, jctr = chain.junction_rows_batch(o, n, jrows, 0, n_lines)
    rb, rctr = chain.junction_reduce_batch(jrows, n_lines)
    gi.junction_rows(jb, stream=stream)
    gi.junction_reduce(rb, stream=stream)
    torch.cuda.synchronize()
    assert int(jctr.cpu().numpy().view(np.uint64)[1]) == n_lines
    m = int(rctr.cpu().numpy().view(np.uint64)[1])
    tb, to = chain.junction_text_batch(jrows, m, strings["chrs"], strings["chr_off"], len(chrs), 64 * max(m, 1))

    def all_three():
        gi.junction_rows(jb, stream=stream)
        gi.junction_reduce(rb, stream=stream)
        gi.junction_text(tb, stream=stream)

    res["junctions"] = timed(all_three, tst, a.launches, a.warmup)
    tc = to["ctr"].cpu().numpy().view(np.uint64)
    assert int(tc[0]) == int(tc[1]) and int(tc[2]) == m
    table = to["out"][:int(tc[1])].cpu().numpy().tobytes()
    res["junctions"].update(rows_in=n_lines, distinct=m, bytes_written=int(tc[1]),
                            share_of_lines=round(res["junctions"]["ms_median"] / max(res["lines"]["ms_median"], 1e-9), 4))
    res["rows"] = timed(lambda: gi.junction_rows(jb, stream=stream), tst, a.launches, a.warmup)

    def reduce_again():                                     # (the reduction works in place: its input is put back first)
        gi.junction_rows(jb, stream=stream)
        gi.junction_reduce(rb, stream=stream)

    res["rows_reduce"] = timed(reduce_again, tst, a.launches, a.warmup)
    res["text"] = timed(lambda: gi.junction_text(tb, stream=stream), tst, a.launches, a.warmup)

    t0 = time.perf_counter()
    rows, want = junctions.table_of(sam_text, chrs, pac, blocks)
    res["python"] = dict(table_of_s=round(time.perf_counter() - t0, 3), sam_bytes=len(sam_text), rows=int(len(rows)),
                         table_equals_device_text=bool(want == table))
    log(f"[junction_probe] rows + reduce + text {res['junctions']['ms_median']:.3f} ms for {n_lines} lines, {m} introns; lines "
        f"{res['lines']['ms_median']:.3f} ms; python {res['python']['table_of_s']} s; equal: {want == table}")
    gi.close()
    return emit(res, a.out)


if __name__ == "__main__":
    sys.exit(main())
