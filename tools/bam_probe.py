#!/usr/bin/env python3
"""Time the BAM loader (hsa_bam_reads_device) alone: nothing behind it runs, no search and no
align_fastq at this size.

--batch reads of --read-len bases from hsa_amd.synth over the tiny index's text, as BAM records
of fixed width (name "SRR062634.0000001", every third stored reversed with FLAG 0x10, Phred
2-41), the text resident on the device.  Times are the median of --launches calls after
--warmup warm-ups, by HIP events on one stream, with min-max:

  aligned     the call with the anchors of the aligned layout (members of at most 65 280 bytes
              that end at record boundaries, as htslib writes them): whole call and per launch;
  straddling  the same text with the single anchor 0, the serial walk a file whose members cut
              through records gets: whole call and per launch;
  walk_ab     both again with hsa_bam_walk_mode 0, 1 and 2: one wavefront per segment hopping
              inside a window staged in LDS (the default), one wavefront per segment with hops
              that load from memory, and one lane per segment;
  parse_host  hsa_amd.bam.parse_host on the first --sample records, scaled to the batch;
  fastq       hsa_reads_device_opts on the same reads as FASTQ, in the same session;
  open_text   hsa_amd.bam.open_text from the path of the BGZF file (zlib level 1), with the
              inflater's share (bgzf.inflate_device alone on the file's bytes);
  kernels     the compiler's resource report per kernel (profiles/bam_kres.txt, written at
              build time with -Rpass-analysis=kernel-resource-usage), when it is there.

One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from choose_probe import log, timed  # noqa: E402
from reads_probe import digits  # noqa: E402

NAME = b"SRR062634.0000000\0"
MEMBER = 65280


def make_reads(n, L, seed):
    from hsa_amd import index_io, synth
    genome = index_io.read_pac(os.path.join(ROOT, "tests", "golden", "index", "tiny.fa"))
    return synth.make_reads(genome, [(0, len(genome))], n, L, seed)[0]


def make_bam(reads, seed):
    """(the BAM text as a uint8 array, the header's length, the record width, the qualities as
    the reads have them)."""
    import bam_cases as bm
    n, L = reads.shape
    rng = np.random.default_rng(seed)
    qual = rng.integers(2, 42, (n, L), dtype=np.uint8)
    rev = np.arange(n) % 3 == 2
    stored, sq = reads.copy(), qual.copy()
    stored[rev] = (3 - reads[rev])[:, ::-1]
    sq[rev] = qual[rev][:, ::-1]
    nib = np.array([1, 2, 4, 8], np.uint8)[stored]
    if L % 2:
        nib = np.concatenate([nib, np.zeros((n, 1), np.uint8)], 1)
    packed = (nib[:, 0::2] << 4) | nib[:, 1::2]
    W = 36 + len(NAME) + packed.shape[1] + L
    rec = np.zeros((n, W), np.uint8)
    core = np.frombuffer(bm.record(NAME[:-1], b"A" * L, bytes(L))[:36], np.uint8)
    rec[:, :36] = core
    rec[rev, 18] = core[18] | 0x10
    rec[:, 36:36 + len(NAME)] = np.frombuffer(NAME, np.uint8)
    p1 = 36 + NAME.index(b"0000000")
    rec[:, p1:p1 + 7] = digits(np.arange(1, n + 1, dtype=np.int64), 7)
    rec[:, 36 + len(NAME):36 + len(NAME) + packed.shape[1]] = packed
    rec[:, W - L:] = sq
    head = np.frombuffer(bm.header(), np.uint8)
    return np.concatenate([head, rec.reshape(-1)]), len(head), W, qual


def make_fastq(reads, qual):
    n, L = reads.shape
    head = b"@" + NAME[:-1] + b"\n"
    rec = np.zeros((n, len(head) + L + 3 + L + 1), np.uint8)
    rec[:, :len(head)] = np.frombuffer(head, np.uint8)
    p1 = head.index(b"0000000")
    rec[:, p1:p1 + 7] = digits(np.arange(1, n + 1, dtype=np.int64), 7)
    s0 = len(head)
    rec[:, s0:s0 + L] = np.frombuffer(b"ACGT", np.uint8)[reads]
    rec[:, s0 + L:s0 + L + 3] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, s0 + L + 3:s0 + 2 * L + 3] = qual + 33
    rec[:, -1] = 10
    return rec.reshape(-1)


def outputs(n, L, name_len):
    import torch
    from hsa_amd import _lib
    z = lambda m, dt: torch.zeros(m, dtype=dt, device="cuda")          # noqa: E731
    return dict(jobs=z(n * _lib.JOB_DTYPE.itemsize, torch.uint8), codes=z(n * L + 16, torch.uint8), names=z(n * name_len, torch.uint8),
                quals=z(n * L, torch.uint8), name_off=z(n + 1, torch.int64), qual_off=z(n + 1, torch.int64),
                rec=z((n + 1) * _lib.RD_ROW_WORDS, torch.int32), ctr=z(16, torch.int64), full_len=z(n, torch.int32),
                octr=z(4, torch.int64), bctr=z(4, torch.int64))


def bam_case(gi, d_text, first, n_in, anchors, n, L, d_tab, n_tab, a, tst):
    import torch
    from hsa_amd import _lib
    o = outputs(n, L, len(NAME))
    d_anchor = torch.from_numpy(np.asarray(anchors, np.int64)).cuda()
    b = _lib.BamBatch(d_in=d_text.data_ptr() + first, n_in=n_in, at_eof=1, max_records=n, which=7, trim_qual=0, max_diff=-1,
                      d_maxdiff=d_tab.data_ptr(), n_maxdiff=n_tab, len_floor=0, seed_len=32, regime=0, d_anchor=d_anchor.data_ptr(),
                      n_anchor=len(anchors), d_jobs=o["jobs"].data_ptr(), job_cap=n, d_codes=o["codes"].data_ptr(), code_cap=n * L + 16,
                      d_names=o["names"].data_ptr(), name_cap=n * len(NAME), d_name_off=o["name_off"].data_ptr(),
                      d_quals=o["quals"].data_ptr(), qual_cap=n * L, d_qual_off=o["qual_off"].data_ptr(),
                      d_full_len=o["full_len"].data_ptr(), d_rec=o["rec"].data_ptr(), rec_cap=n + 1, d_counters=o["ctr"].data_ptr(),
                      d_opt_counters=o["octr"].data_ptr(), d_bam_counters=o["bctr"].data_ptr())
    call = lambda: gi.bam_reads_device(b, stream=tst.cuda_stream)       # noqa: E731
    torch.cuda.synchronize()
    r = timed(call, tst, a.launches, a.warmup)
    _lib.lib().hsa_bam_timing(1)
    call()
    torch.cuda.synchronize()
    r["launch_ms"] = {k: round(v, 4) for k, v in gi.bam_launch_times().items()}
    _lib.lib().hsa_bam_timing(0)
    c = dict(zip(_lib.RD_COUNTERS, (int(v) for v in o["ctr"].cpu().numpy().view(np.uint64))))
    bc = dict(zip(_lib.BAM_COUNTERS, (int(v) for v in o["bctr"].cpu().numpy().view(np.uint64))))
    assert c["loaded"] == n and c["consumed"] == n_in and bc["reason"] == _lib.HSA_BAM_END_INPUT, (c, bc)
    for k in ("jobs", "code", "name", "qual"):
        assert c[k + "_wanted"] == c[k + "_written"], "the probe's capacities are too small"
    r.update(input_bytes=int(n_in), anchors=len(anchors), loaded=c["loaded"], jobs=c["jobs_written"], **bc)
    return r, o


def fastq_case(gi, fq, n, L, d_tab, n_tab, a, tst):
    import torch
    from hsa_amd import _lib
    d_in = torch.from_numpy(fq).cuda()
    o = outputs(n, L, len(NAME))
    b = _lib.ReadsBatch(d_in=d_in.data_ptr(), n_in=len(fq), at_eof=1, max_records=n, max_diff=-1, d_maxdiff=d_tab.data_ptr(),
                        n_maxdiff=n_tab, len_floor=0, seed_len=32, regime=0, trim_qual=0, mode=0x03, d_jobs=o["jobs"].data_ptr(),
                        job_cap=n, d_codes=o["codes"].data_ptr(), code_cap=n * L + 16, d_names=o["names"].data_ptr(),
                        name_cap=n * len(NAME), d_name_off=o["name_off"].data_ptr(), d_quals=o["quals"].data_ptr(), qual_cap=n * L,
                        d_qual_off=o["qual_off"].data_ptr(), d_rec=o["rec"].data_ptr(), d_counters=o["ctr"].data_ptr(),
                        d_full_len=o["full_len"].data_ptr(), rec_cap=n, d_opt_counters=o["octr"].data_ptr())
    torch.cuda.synchronize()
    r = timed(lambda: gi.reads_device_opts(b, stream=tst.cuda_stream), tst, a.launches, a.warmup)
    c = dict(zip(_lib.RD_COUNTERS, (int(v) for v in o["ctr"].cpu().numpy().view(np.uint64))))
    assert c["loaded"] == n and c["consumed"] == len(fq)
    r.update(input_bytes=int(len(fq)), loaded=c["loaded"])
    return r, o


def kernel_resources():
    """{kernel: {SGPRs, VGPRs, ScratchSize, Occupancy, LDS}} from profiles/bam_kres.txt."""
    path = os.path.join(ROOT, "profiles", "bam_kres.txt")
    if not os.path.exists(path):
        return None
    out, cur = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    for ln in open(path):
        m = re.match(r"Function Name: _Z\d+(k_bam_\w+?)7BamArgs", ln)
        if m:
            cur = out.setdefault(re.sub(r"ILi(\d)EEv$", r"<\1>", m.group(1)), {})
        for k, name in keys.items():
            m = re.match(re.escape(k) + r": (\d+)", ln)
            if m and cur is not None:
                cur[name] = int(m.group(1))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from hsa_amd import _lib, align, bam, bgzf, reads      # (before torch: the library's HIP runtime loads first)
    import torch
    import bgzf_cases as bc
    n, L = a.batch, a.read_len
    rd = make_reads(n, L, 47)
    text, hdr, W, qual = make_bam(rd, 5)
    log(f"[bam_probe] {n} records of {W} bytes, text {len(text)} bytes")
    gi, _ = align.open_index64(os.path.join(ROOT, "tests", "golden", "index", "tiny.fa"))
    tst = torch.cuda.Stream()
    assert tst.cuda_stream, "need a non-default stream (the library maps NULL to the index's own)"
    table = reads.maxdiff_table(float(np.float32(0.04)), 4096)
    d_tab = torch.from_numpy(table).cuda()
    d_text = torch.from_numpy(text).cuda()
    res = dict(tool="bam_probe", lib=os.path.basename(_lib.LIB_PATH), batch=n, read_len=L, record_bytes=W, launches=a.launches,
               warmup=a.warmup)
    per = MEMBER // W * W
    anchors = np.arange(0, n * W, per, dtype=np.int64)
    res["aligned"], o_al = bam_case(gi, d_text, hdr, n * W, anchors, n, L, d_tab, len(table), a, tst)
    log(f"[bam_probe] aligned: {res['aligned']['ms_median']:.3f} ms, {len(anchors)} anchors")
    res["straddling"], o_st = bam_case(gi, d_text, hdr, n * W, [0], n, L, d_tab, len(table), a, tst)
    log(f"[bam_probe] straddling (one anchor): {res['straddling']['ms_median']:.3f} ms")
    for k in ("jobs", "codes", "names", "quals", "name_off", "qual_off", "full_len", "rec"):
        assert torch.equal(o_al[k], o_st[k]), k
    # the A/B of the walk (hsa_bam_walk_mode): the same calls with the hops loading from memory,
    # one wavefront per segment and one lane per segment; the results must not differ
    res["walk_ab"] = {}
    for layout, anc in (("aligned", anchors), ("straddling", [0])):
        res["walk_ab"][layout] = {}
        for mode, name in ((0, "wave_lds_window"), (1, "wave_direct_loads"), (2, "lane_direct_loads")):
            _lib.lib().hsa_bam_walk_mode(mode)
            r, o = bam_case(gi, d_text, hdr, n * W, anc, n, L, d_tab, len(table), a, tst)
            _lib.lib().hsa_bam_walk_mode(0)
            for k in ("jobs", "codes", "names", "quals", "name_off", "qual_off", "full_len", "rec"):
                assert torch.equal(o_al[k], o[k]), (layout, name, k)
            res["walk_ab"][layout][name] = dict(ms_median=r["ms_median"], ms_min=r["ms_min"], ms_max=r["ms_max"],
                                                walk_ms=r["launch_ms"]["walk"], starts_ms=r["launch_ms"]["starts"])
            log(f"[bam_probe] {layout} {name}: {r['ms_median']:.3f} ms")
    fq = make_fastq(rd, qual)
    res["fastq"], o_fq = fastq_case(gi, fq, n, L, d_tab, len(table), a, tst)
    log(f"[bam_probe] fastq: {res['fastq']['ms_median']:.3f} ms")
    for k in ("jobs", "codes", "names", "quals", "name_off", "qual_off"):
        assert torch.equal(o_al[k], o_fq[k]), k               # the same reads either way
    m = min(a.sample, n)
    body = text[hdr:hdr + m * W].tobytes()
    t0 = time.perf_counter()
    p = bam.parse_host(body)
    dt = time.perf_counter() - t0
    assert len(p["names"]) == m
    res["parse_host"] = dict(sample=m, sample_s=round(dt, 4), scaled_to_batch_s=round(dt * n / m, 2))
    # the file: members that end at record boundaries, zlib level 1
    raw = text.tobytes()
    cuts = [0, hdr] + [hdr + int(v) for v in anchors[1:]] + [len(raw)]
    data = b"".join(bc.bgzf_member(bc.deflate(raw[s:e], 1), raw[s:e]) for s, e in zip(cuts, cuts[1:])) + bc.EOF_MARKER
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.bam")
        with open(path, "wb") as f:
            f.write(data)
        ts, ti = [], []
        for k in range(a.launches + a.warmup):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got, d_got, cand, st = bam.open_text(gi, path)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            tb = bgzf.scan(data)
            t2 = time.perf_counter()
            bgzf.inflate_device(gi, data, table=tb)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if k >= a.warmup:
                ts.append((t1 - t0) * 1e3)
                ti.append((t3 - t2) * 1e3)
        assert got == raw and d_got is not None and len(cand) == len(anchors) + 1 and st["host_blocks"] == 0
    res["open_text"] = dict(file_bytes=len(data), text_bytes=len(raw), blocks=st["blocks"], ms_median=round(float(np.median(ts)), 2),
                            ms_min=round(min(ts), 2), ms_max=round(max(ts), 2), inflate_device_ms_median=round(float(np.median(ti)), 2),
                            inflate_device_ms_min=round(min(ti), 2), inflate_device_ms_max=round(max(ti), 2))
    log(f"[bam_probe] open_text: {res['open_text']['ms_median']:.1f} ms, of which inflate_device {res['open_text']['inflate_device_ms_median']:.1f} ms")
    res["kernels"] = kernel_resources()
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
