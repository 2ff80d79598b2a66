#!/usr/bin/env python3
"""Time the FASTQ loader with the reader's options (hsa_reads_device_opts), a sibling of
tools/reads_probe.py.

Makes --batch canonical records of --read-len bases ("@SRR062634.0000001 1:N:0:ACGTAC", a
few N) and times, with HIP events on one stream, --launches calls after --warmup warm-ups of

  none   no option, through hsa_reads_device (the entry point the library had before the
         options: the same call on a library built from an earlier commit, chosen with
         HSA_GPU_LIB, is the comparison the options' code has to stand);
  q20    -q 20 on qualities whose last 0-70 bases decay to Phred 2-16 (the rest Phred 2-41);
  all    -B 6 -q 20 -I -Y: six barcode bases in front, the qualities 31 higher, the comment
         "1:Y:0:ACGTAC" on every 7th record.

One JSON object on stdout (and in --out).  --merge FILE... reads such objects of runs that
alternated two libraries (their "lib" fields) and prints, per library, the median of the runs'
medians of `none` and the spread (max - min) between the runs."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from choose_probe import log, timed  # noqa: E402
from reads_probe import digits  # noqa: E402

HEAD = b"@SRR062634.0000000 1:N:0:ACGTAC\n"
CASES = dict(none=dict(), q20=dict(trim_qual=20, tails=True), all=dict(trim_qual=20, tails=True, bc=6, shift=31, casava=True))


def make_fastq(n, L, seed, bc=0, tails=False, shift=0, casava=False, **_):
    """n records of fixed width as one uint8 array."""
    rng = np.random.default_rng(seed)
    W = L + bc
    rec = np.zeros((n, len(HEAD) + W + 3 + W + 1), np.uint8)
    rec[:, :len(HEAD)] = np.frombuffer(HEAD, np.uint8)
    p1 = HEAD.index(b"0000000")
    rec[:, p1:p1 + 7] = digits(np.arange(1, n + 1, dtype=np.int64), 7)
    if casava:
        rec[3::7, HEAD.index(b":N:") + 1] = ord("Y")
    s0 = len(HEAD)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, W))]
    seq[rng.random((n, W)) < 0.002] = ord("N")
    rec[:, s0:s0 + W] = seq
    rec[:, s0 + W:s0 + W + 3] = np.frombuffer(b"\n+\n", np.uint8)
    q = rng.integers(35, 75, (n, W), dtype=np.uint8)
    if tails:
        low = np.arange(W)[None, :] >= (W - rng.integers(0, 71, n))[:, None]
        q[low] = rng.integers(35, 50, int(low.sum()), dtype=np.uint8)
    rec[:, s0 + W + 3:s0 + 2 * W + 3] = q + shift
    rec[:, -1] = 10
    return rec.reshape(-1)


def one_case(gi, name, n, L, a, tst):
    import torch
    from hsa_amd import _lib, reads
    kw = CASES[name]
    text = make_fastq(n, L, 7, **kw)
    bc = kw.get("bc", 0)
    mode = 0x03 | (bc << 24) | (reads.MODE_IL13 if kw.get("shift") else 0) | (reads.MODE_CFY if kw.get("casava") else 0)
    table = reads.maxdiff_table(float(np.float32(0.04)), 4096)
    d_in, d_tab = torch.from_numpy(text).cuda(), torch.from_numpy(table).cuda()
    z = lambda m, dt: torch.zeros(m, dtype=dt, device="cuda")          # noqa: E731
    JB = _lib.JOB_DTYPE.itemsize
    o = dict(jobs=z(n * JB, torch.uint8), codes=z(n * L + 16, torch.uint8), names=z(n * len(HEAD), torch.uint8),
             quals=z(n * L, torch.uint8), name_off=z(n + 1, torch.int64), qual_off=z(n + 1, torch.int64),
             rec=z(n * _lib.RD_ROW_WORDS, torch.int32), ctr=z(16, torch.int64), full_len=z(n, torch.int32),
             bc=z(max(n * bc, 1), torch.uint8), octr=z(4, torch.int64))
    b = _lib.ReadsBatch(d_in=d_in.data_ptr(), n_in=len(text), at_eof=1, max_records=n, max_diff=-1, d_maxdiff=d_tab.data_ptr(),
                        n_maxdiff=len(table), len_floor=0, seed_len=32, regime=0, trim_qual=kw.get("trim_qual", 0), mode=mode,
                        d_jobs=o["jobs"].data_ptr(), job_cap=n, d_codes=o["codes"].data_ptr(), code_cap=n * L + 16,
                        d_names=o["names"].data_ptr(), name_cap=n * len(HEAD), d_name_off=o["name_off"].data_ptr(),
                        d_quals=o["quals"].data_ptr(), qual_cap=n * L, d_qual_off=o["qual_off"].data_ptr(),
                        d_rec=o["rec"].data_ptr(), d_counters=o["ctr"].data_ptr())
    if name != "none":
        b.d_full_len, b.d_bc, b.rec_cap, b.d_opt_counters = o["full_len"].data_ptr(), o["bc"].data_ptr(), n, o["octr"].data_ptr()
    call = (lambda: gi.reads_device(b, stream=tst.cuda_stream)) if name == "none" else \
        (lambda: gi.reads_device_opts(b, stream=tst.cuda_stream))
    torch.cuda.synchronize()
    r = timed(call, tst, a.launches, a.warmup)
    c = dict(zip(_lib.RD_COUNTERS, (int(v) for v in o["ctr"].cpu().numpy().view(np.uint64))))
    assert c["bad_record"] == 0xFFFFFFFFFFFFFFFF and c["consumed"] == len(text)
    for k in ("jobs", "code", "name", "qual"):
        assert c[k + "_wanted"] == c[k + "_written"], "the probe's capacities are too small"
    r.update(input_bytes=int(len(text)), loaded=c["loaded"], jobs=c["jobs_written"], max_loaded=c["max_loaded"])
    if name != "none":
        r.update(zip(_lib.RD_OPT_COUNTERS, (int(v) for v in o["octr"].cpu().numpy().view(np.uint64))))
    log(f"[reads_opts_probe] {name}: {r['ms_median']:.3f} ms ({r['ms_min']:.3f}-{r['ms_max']:.3f}), {r['loaded']} loaded")
    return r


def merge(files):
    runs = [json.load(open(f)) for f in files]
    out = {}
    for lib in sorted({r["lib"] for r in runs}):
        ms = [r["cases"]["none"]["ms_median"] for r in runs if r["lib"] == lib and "none" in r["cases"]]
        out[lib] = dict(runs=len(ms), none_ms_medians=ms, none_ms=round(float(np.median(ms)), 4), spread_ms=round(max(ms) - min(ms), 4))
    return dict(tool="reads_opts_probe --merge", batch=runs[0]["batch"], read_len=runs[0]["read_len"], launches=runs[0]["launches"],
                warmup=runs[0]["warmup"], libraries=out,
                options={k: v for r in runs for k, v in r["cases"].items() if k != "none" and r["lib"] == "libhsa_gpu.so"})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="none,q20,all")
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.merge:
        res = merge(a.merge)
    else:
        from hsa_amd import _lib, align
        import torch
        gi, _ = align.open_index64(os.path.join(ROOT, "tests", "golden", "index", "tiny.fa"))
        tst = torch.cuda.Stream()
        assert tst.cuda_stream, "need a non-default stream (the library maps NULL to the index's own)"
        res = dict(tool="reads_opts_probe", lib=os.path.basename(_lib.LIB_PATH), batch=a.batch, read_len=a.read_len,
                   launches=a.launches, warmup=a.warmup, cases={})
        for name in a.cases.split(","):
            res["cases"][name] = one_case(gi, name, a.batch, a.read_len, a, tst)
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
