#!/usr/bin/env python3
"""Time hsa_splice_lines_device_xa against hsa_splice_lines_device.

(a) tools/splice_lines_probe.py's batch (bench.py's synthetic text at --genome bp, --batch
    spliced reads, -n 4 -o 1; no read has two splice pairs there): the median of --launches
    calls after --warmup, by HIP events on one stream, of the new entry point with
    chain.xa_room(batch) extra pairs of room (--entry xa) or of the plain one (--entry plain).
    With HSA_GPU_LIB naming another build of the library in hsa_amd/ (the parent commit's)
    and --entry plain, the same batch through that library.
(b) --dup-share 0.1: the same text with the fixture's recipe on it (duplicate_loci: for every
    tenth read one or two more copies of its two exons at its own intron length, GT and AG at
    the intron's ends), so that about a tenth of the reads carry lists: time per call with the
    room and the bytes the batch wants, reads with a list, entries printed, bytes of text; with
    --entry plain the plain entry point on that batch (those reads refused).
    --dup: the committed dup fixture (tests/golden, tools/make_golden_dup.py; 624 reads on a
    200 kbp genome, a third of them with lists), a call that launch latency dominates.

--series PARENT_LIB runs (a) in fresh child processes, alternating the new entry point of this
build and the plain one of PARENT_LIB, three of each, every child under its own time limit and
the series stopping at the first child that fails, and writes all of it as one JSON object.
No threshold is set: nobody has measured this before."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from choose_probe import emit, log, parser, probe_batch, timed_ms  # noqa: E402


def summary(ms):
    return dict(ms_median=round(float(np.median(ms)), 4), ms_min=round(float(ms.min()), 4), ms_max=round(float(ms.max()), 4),
                calls=int(len(ms)))


def time_entry(gi, lb, xa, tst, a):
    import torch
    torch.cuda.synchronize()
    return summary(timed_ms(lambda: gi.splice_lines(lb, stream=tst.cuda_stream, xa=xa), tst, a.launches, a.warmup))


def put_codes(words, pos, codes):
    """codes at text positions pos of a packed text (16 two-bit codes per u32, code j of a word at bits 2 j)."""
    w, sh = pos >> 4, ((pos & 15) * 2).astype(np.uint32)
    np.bitwise_and.at(words, w, ~(np.uint32(3) << sh))
    np.bitwise_or.at(words, w, codes.astype(np.uint32) << sh)


def duplicate_loci(words, T, reads, truth, share, records, rl):
    """The fixture's recipe on the synthetic text: for every (1 / share)-th read one or two more
    copies of its two exons elsewhere in its record, at the read's own intron length, with GT
    and AG at the intron's ends and the text that was there between them.  Only the exons and
    the four motif bases are written, so the reads drawn from the untouched text keep theirs
    but for the few a copy lands on.  Returns the number of copies written."""
    from hsa_amd import synth
    step = max(1, int(round(1 / share)))
    picked = np.arange(0, len(reads), step)
    slots = int(len(picked) * 1.5) + 2
    stride = (T - 20000) // slots
    assert stride > 5000 + rl + 200, "too many copies for this text"
    pos, codes, used, made = [], [], {}, 0
    for q, r in enumerate(picked):
        fwd = synth.revcomp_codes(reads[r]) if truth["strand"][r] else reads[r]
        ea, it = int(truth["exon_a"][r]), int(truth["intron"][r])
        rec = next(((s0, n) for s0, n in records if s0 <= truth["start"][r] < s0 + n), None)
        for _ in range(1 + q % 2):
            if rec is None:
                continue
            at = rec[0] + 10000 + used.get(rec, 0) * stride  # the copy stays in the read's record (one chromosome)
            used[rec] = used.get(rec, 0) + 1
            if at + it + rl > rec[0] + rec[1]:
                continue
            pos += [np.arange(at, at + ea), np.array([at + ea, at + ea + 1, at + ea + it - 2, at + ea + it - 1]),
                    np.arange(at + ea + it, at + it + rl)]
            codes += [fwd[:ea], np.array([2, 3, 0, 2], np.uint8), fwd[ea:]]
            made += 1
    if made:
        put_codes(words, np.concatenate(pos).astype(np.int64), np.concatenate(codes))
    return made


def build_index_of(words, T, device):
    """bench.build_index for a text given as packed words on the host (its with_files form)."""
    import ctypes as C

    import torch

    import bench
    from hsa_amd import _lib
    L = _lib.lib()
    nw = (T + 15) // 16
    text = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
    text[:nw] = torch.from_numpy(words[:nw].view(np.int32)).cuda()
    res, extra = {}, {}
    for rev in (0, 1):
        bw = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
        Cc = np.zeros(5, np.uint32)
        if rev == 0:
            i64, C64 = C.c_uint64(), np.zeros(5, np.uint64)
            sa = torch.zeros(T // bench.SA_INTERVAL + 2, dtype=torch.int32, device="cuda")
            _lib.check(L.hsa_build_bwt_index_device(device, T, text.data_ptr(), bw.data_ptr(), C.byref(i64), C64, bench.SA_INTERVAL,
                                                    sa.data_ptr()))
            isa0, Cc[:] = int(i64.value), C64.astype(np.uint32)
            extra["sa"] = sa[:T // bench.SA_INTERVAL + 1].cpu().numpy().view(np.uint32)
        else:
            i32 = C.c_uint32()
            _lib.check(L.hsa_build_bwt_device(device, T, text.data_ptr(), rev, bw.data_ptr(), C.byref(i32), Cc))
            isa0 = int(i32.value)
        res[rev] = (bw, isa0, Cc)
    extra["text"] = words[:nw]
    gi = _lib.GpuIndex.from_device_codes(T, res[0][1], res[0][2], res[0][0].data_ptr(), T, res[1][1], res[1][2],
                                         res[1][0].data_ptr(), device=device)
    return gi, res, extra


def synthetic(a):
    from hsa_amd import _lib, chain, sam, synth     # (before torch: _lib loads the HIP runtime it was built for)
    import torch

    import bench
    T, n, RL = a.genome, a.batch, a.read_len
    recs = synth.record_layout(T, bench.RECORDS)
    reads, truth = synth.make_spliced_reads(synth.PackedGenome(T, bench.GENOME_SEED), recs, n, RL, 7 * 1_000_000 + 91)
    copies = 0
    if a.dup_share > 0:
        words = synth.genome_words(T, bench.GENOME_SEED).view(np.uint32).copy()      # (32 codes per u64, little-endian: the same bits)
        copies = duplicate_loci(words, T, reads, truth, a.dup_share, recs, RL)
        gi, keep, extra = build_index_of(words, T, torch.cuda.current_device())
    else:
        gi, keep, extra = bench.build_index(T, bench.GENOME_SEED, torch.cuda.current_device(), with_files=True)
    bench.attach_splice_arrays(gi, T, extra)
    del extra
    tst = torch.cuda.Stream()
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
    chrs = [f"chr{r + 1}" for r in range(bench.RECORDS)]
    nb, noff = sam.pack_strings([f"r{j:07d}" for j in range(n)])
    cbytes, coff = sam.pack_strings(chrs)
    up = chain.to_device
    strings = dict(names=up(nb), name_off=up(noff), chrs=up(cbytes), chr_off=up(coff),
                   quals=up(np.random.default_rng(3).integers(33, 74, n * RL, dtype=np.uint8)),
                   qual_off=up(np.arange(n + 1, dtype=np.uint64) * np.uint64(RL)))
    stride = 33
    max_line = sam.line_bound(8, RL, 4, stride, 0, 49)
    kw = dict(cigar_stride=stride, max_top2=opt["max_top2"])
    res = dict(entry=a.entry, library=os.path.basename(_lib.LIB_PATH), text_bp=T, batch=n, read_len=RL, options="-n 4 -o 1",
               dup_share=a.dup_share, copies_written=copies)
    room, cap = chain.xa_room(n), n * (2 * RL + 160)
    if a.dup_share > 0 and a.entry == "xa":
        # the room and the bytes this batch wants, as align finds them: chain.splice_lines' reruns
        o, ctr = chain.splice_lines(gi, bt, s, 0, n, strings, len(chrs), max_line, cap, **kw)
        room, cap = int(o["xa"][0]), int(ctr[0])
        res.update(reads_with_list=int(o["xa"][2]), entries=int(o["xa"][3]), extra_pairs=int(o["xa"][0]),
                   longest_line=int(np.diff(o["line_off"].cpu().numpy().view(np.uint64).astype(np.int64)).max()))
    lb, o = chain.splice_lines_batch(bt, s, 0, n, strings, len(chrs), max_line, cap, **kw)
    xa = ox = None
    if a.entry == "xa":
        xa, ox = chain.splice_xa_batch(n, room, stride)
    res["lines_call"] = time_entry(gi, lb, xa, tst, a)
    ctr = o["ctr"].cpu().numpy().view(np.uint64)
    assert int(ctr[0]) == int(ctr[1]), "the probe's out_cap is too small"
    res.update(bytes_written=int(ctr[1]), lines=int(ctr[2]), handed_back=int(ctr[3]), multi=int(ctr[4]), refused=int(ctr[5]),
               no_pair=int(ctr[6]))
    if ox:
        res.update(room=int(ox["pair_cap"]), extra_pairs_wanted=int(ox["xa_ctr"].cpu().numpy().view(np.uint64)[0]))
    gi.close()
    del keep
    return res


def dup(a):
    """The committed fixture through align_fastq once (its batch recorded), then the recorded
    splice-lines call alone, timed."""
    import gzip
    import io

    from hsa_amd import align, chain
    import torch
    gold = os.path.join(ROOT, "tests", "golden")
    man = json.load(open(os.path.join(gold, "manifest_dup.json")))
    gi, chrs = align.open_index64(os.path.join(gold, "index", "dup.fa"))
    rec, real = [], chain.splice_lines

    def spy(*args, **kw):
        o, ctr = real(*args, **kw)
        rec.append((args, kw, o, ctr))
        return o, ctr
    chain.splice_lines = spy
    try:
        align.align_fastq(gi, chrs, gzip.open(os.path.join(gold, man["files"]["reads"])).read(), align.parse_options(["-n", "4", "-o", "1"])[0],
                          io.BytesIO(), splice=True)
    finally:
        chain.splice_lines = real
    (gi_, b, s, first, n, strings, n_chr, max_line, out_cap), kw, o, ctr = max(rec, key=lambda r: int(r[2]["xa"][3]))
    tst = torch.cuda.Stream()
    lb, o2 = chain.splice_lines_batch(b, s, first, n, strings, n_chr, max_line, int(ctr[0]), **kw)
    res = dict(fixture="dup n4o1", reads=n, lines=int(ctr[2]), bytes_written=int(ctr[1]), reads_with_list=int(o["xa"][2]),
               entries=int(o["xa"][3]))
    xa, _ = chain.splice_xa_batch(n, int(o["xa"][0]), o2["cigar_stride"])
    res["xa_call"] = time_entry(gi, lb, xa, tst, a)
    res["plain_call"] = time_entry(gi, lb, None, tst, a)     # (those reads refused: HSA_SL_MULTI)
    gi.close()
    return res


def last_json(text):
    """The object emit() printed last (indented over several lines, '{' alone on its first)."""
    at = text.rfind("\n{\n")
    return json.loads(text[at + 1:] if at >= 0 else text[text.index("{"):])


def series(a):
    out = dict(tool="splice_xa_probe", parent_library=a.series, runs=[])
    here = os.path.abspath(__file__)
    common = ["--genome", str(a.genome), "--batch", str(a.batch), "--read-len", str(a.read_len), "--launches", str(a.launches),
              "--warmup", str(a.warmup)]
    for k in range(3):
        for entry, lib in (("xa", None), ("plain", a.series)):
            env = dict(os.environ)
            if lib:
                env["HSA_GPU_LIB"] = lib
            r = subprocess.run(["timeout", "-k", "10", str(a.child_limit), sys.executable, here, "--entry", entry, *common], env=env,
                               capture_output=True, text=True)
            if r.returncode != 0:
                log(r.stderr[-2000:])
                out["stopped"] = f"child {entry} #{k} ended with {r.returncode}"
                return emit(out, a.out) or r.returncode
            out["runs"].append(last_json(r.stdout))
            log(f"[splice_xa_probe] {entry} #{k}: {out['runs'][-1]['lines_call']}")
    med = lambda e: [r["lines_call"]["ms_median"] for r in out["runs"] if r["entry"] == e]
    out["xa_ms_medians"], out["parent_plain_ms_medians"] = med("xa"), med("plain")
    if a.no_dup:
        return emit(out, a.out)
    r = subprocess.run(["timeout", "-k", "10", str(a.child_limit), sys.executable, here, "--dup", "--launches", str(a.launches), "--warmup",
                        str(a.warmup)], capture_output=True, text=True)
    if r.returncode != 0:
        log(r.stderr[-2000:])
        out["stopped"] = f"child --dup ended with {r.returncode}"
        return emit(out, a.out) or r.returncode
    out["dup"] = last_json(r.stdout)
    return emit(out, a.out)


def main(argv=None):
    ap = parser(__doc__, genome=100_000_000, genome_help="text length (default: 100 Mbp)", read_len=150)
    ap.set_defaults(batch=100_000, launches=10, warmup=3)
    ap.add_argument("--entry", choices=("xa", "plain"), default="xa")
    ap.add_argument("--dup", action="store_true", help="the committed dup fixture instead of the synthetic text")
    ap.add_argument("--dup-share", type=float, default=0.0, help="(b): the share of the reads whose locus is copied once or twice")
    ap.add_argument("--series", metavar="PARENT_LIB", help="file name under hsa_amd/ of the parent commit's library")
    ap.add_argument("--no-dup", action="store_true", help="--series without the last child (b)")
    ap.add_argument("--child-limit", type=int, default=300, help="seconds a child of --series may run")
    a = ap.parse_args(argv)
    if a.series:
        return series(a)
    return emit(dup(a) if a.dup else synthetic(a), a.out)


if __name__ == "__main__":
    sys.exit(main())
