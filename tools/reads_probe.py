#!/usr/bin/env python3
"""Time hsa_reads_device (FASTQ bytes to a search batch on the device).

Makes --batch records of --read-len bases with hg19-style names
("SRR062634.0000001 HWI-EAS110_103327062:6:001:01092:08469/1"), a few N and Phred+33
qualities in '#'..'J', uploads the text, and times, with HIP events on one stream, the median
of --launches runs after --warmup warm-ups of

  reads     hsa_reads_device of the whole text (-n 0.04: the max_diff table) and its launches
            one by one (hsa_reads_timing), the bytes it
            reads (the input, once) and writes (jobs, codes, names, qualities, offsets,
            rows), and GB/s of their sum;
  copy      a device-to-device copy whose traffic equals that sum (it copies half of it:
            every byte is read once and written once): the floor;
  python    the way to the same arrays without the call: a per-read Python loop over the text
            (names cut, codes through a table, qualities), hsa_amd.sam.pack_strings and the job
            rows in NumPy, on a sample of --sample records scaled to the batch
            ("sampled": true).  The sample's arrays are also compared with the device's.

The index is the tiny golden one (the call takes a handle for its stream and scratch only).
One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from choose_probe import log, timed  # noqa: E402

HEAD = b"@SRR062634.0000000 HWI-EAS110_103327062:6:000:00000:00000/1\n"


def digits(col, width):
    """`width` ASCII digits of every value of col, most significant first: (n, width) uint8."""
    p = 10 ** np.arange(width - 1, -1, -1, dtype=np.int64)
    return ((col[:, None] // p[None, :]) % 10 + 48).astype(np.uint8)


def make_fastq(n, L, seed):
    """n records of fixed width as one uint8 array."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, len(HEAD) + L + 3 + L + 1), np.uint8)
    rec[:, :len(HEAD)] = np.frombuffer(HEAD, np.uint8)
    k = np.arange(1, n + 1, dtype=np.int64)
    p1, p2 = HEAD.index(b"0000000"), HEAD.index(b":000:") + 1
    rec[:, p1:p1 + 7] = digits(k, 7)
    rec[:, p2:p2 + 3] = digits(rng.integers(1, 121, n), 3)
    rec[:, p2 + 4:p2 + 9] = digits(rng.integers(1000, 20000, n), 5)
    rec[:, p2 + 10:p2 + 15] = digits(rng.integers(1000, 20000, n), 5)
    s0 = len(HEAD)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, L))]
    seq[rng.random((n, L)) < 0.002] = ord("N")
    rec[:, s0:s0 + L] = seq
    rec[:, s0 + L:s0 + L + 3] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, s0 + L + 3:s0 + 2 * L + 3] = rng.integers(35, 75, (n, L), dtype=np.uint8)
    rec[:, -1] = 10
    return rec.reshape(-1)


def python_way(text, table, seed_len):
    """The arrays without the device call: a Python loop over the records, pack_strings, job
    rows in NumPy (what tests and tools did before hsa_reads_device)."""
    from hsa_amd import _lib, sam
    lut = np.full(256, 4, np.uint8)
    for i, c in enumerate("ACGT"):
        lut[ord(c)] = lut[ord(c.lower())] = i
    ls = text.split(b"\n")
    names, seqs, quals = [], [], []
    for k in range(0, len(ls) - 3, 4):
        nm = ls[k][1:].split()[0]
        names.append(nm[:-2] if len(nm) > 2 and nm[-2:] in (b"/1", b"/2") else nm)
        seqs.append(lut[np.frombuffer(ls[k + 1], np.uint8)])
        quals.append(ls[k + 3])
    lens = np.array([len(s) for s in seqs], np.uint32)
    thr = int(table[lens.max()])
    keep = [r for r, s in enumerate(seqs) if int((s > 3).sum()) <= thr and
            not (len(s) >= 15 and ((s[:15] == 0).all() or (s[:15] == 3).all()))]
    jobs = np.zeros(len(keep), _lib.JOB_DTYPE)
    kl = lens[keep]
    jobs["off"] = np.concatenate([[0], np.cumsum(kl.astype(np.uint64))[:-1]])
    jobs["len"] = kl
    jobs["max_diff"] = table[kl]
    jobs["seed_len"] = np.where(kl > seed_len, seed_len, 0x7FFFFFFF)
    codes = _lib.pad_codes(np.concatenate([seqs[r] for r in keep]))
    nb, noff = sam.pack_strings([names[r] for r in keep])
    qb, qoff = sam.pack_strings([quals[r] for r in keep])
    return dict(jobs=jobs, codes=codes, names=nb, name_off=noff, quals=qb, qual_off=qoff)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=10_000, help="records of the Python loop's sample")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from hsa_amd import _lib, align, reads
    import torch
    n, L = a.batch, a.read_len
    gi, _ = align.open_index64(os.path.join(ROOT, "tests", "golden", "index", "tiny.fa"))
    t0 = time.time()
    text = make_fastq(n, L, 7)
    log(f"[reads_probe] {n} records, {len(text)} bytes in {time.time() - t0:.1f} s")
    table = reads.maxdiff_table(float(np.float32(0.04)), 4096)
    d_in = torch.from_numpy(text).cuda()
    d_tab = torch.from_numpy(table).cuda()
    tst = torch.cuda.Stream()
    assert tst.cuda_stream, "need a non-default stream (the library maps NULL to the index's own)"
    z = lambda m, dt: torch.zeros(m, dtype=dt, device="cuda")          # noqa: E731
    JB = _lib.JOB_DTYPE.itemsize
    cap = dict(jobs=n, codes=n * L + 16, names=n * len(HEAD), quals=n * L)
    o = dict(jobs=z(n * JB, torch.uint8), codes=z(cap["codes"], torch.uint8), names=z(cap["names"], torch.uint8),
             quals=z(cap["quals"], torch.uint8), name_off=z(n + 1, torch.int64), qual_off=z(n + 1, torch.int64),
             rec=z(n * _lib.RD_ROW_WORDS, torch.int32), ctr=z(16, torch.int64))
    b = _lib.ReadsBatch(d_in=d_in.data_ptr(), n_in=len(text), at_eof=1, max_records=n, max_diff=-1, d_maxdiff=d_tab.data_ptr(),
                        n_maxdiff=len(table), len_floor=0, seed_len=32, regime=0, trim_qual=0, mode=0x03,
                        d_jobs=o["jobs"].data_ptr(), job_cap=cap["jobs"], d_codes=o["codes"].data_ptr(), code_cap=cap["codes"],
                        d_names=o["names"].data_ptr(), name_cap=cap["names"], d_name_off=o["name_off"].data_ptr(),
                        d_quals=o["quals"].data_ptr(), qual_cap=cap["quals"], d_qual_off=o["qual_off"].data_ptr(),
                        d_rec=o["rec"].data_ptr(), d_counters=o["ctr"].data_ptr())
    torch.cuda.synchronize()

    def call():
        gi.reads_device(b, stream=tst.cuda_stream)

    res = dict(tool="reads_probe", command="python tools/reads_probe.py " + " ".join(sys.argv[1:] if argv is None else argv),
               batch=n, read_len=L, launches=a.launches, warmup=a.warmup, input_bytes=int(len(text)))
    res["reads"] = timed(call, tst, a.launches, a.warmup)
    _lib.lib().hsa_reads_timing(1)
    split = []
    for _ in range(a.launches):
        call()
        split.append(gi.reads_launch_times())
    _lib.lib().hsa_reads_timing(0)
    res["reads"]["launch_ms_median"] = {k: round(float(np.median([x[k] for x in split])), 4) for k in split[0]}
    c = dict(zip(_lib.RD_COUNTERS, (int(v) for v in o["ctr"].cpu().numpy().view(np.uint64))))
    assert c["loaded"] == n and c["bad_record"] == 0xFFFFFFFFFFFFFFFF
    for k in ("jobs", "code", "name", "qual"):
        assert c[k + "_wanted"] == c[k + "_written"], "the probe's capacities are too small"
    nj = c["jobs_written"]
    written = nj * JB + c["code_written"] + c["name_written"] + c["qual_written"] + 2 * 8 * (nj + 1) + n * 16 + 16 * 8
    ms = res["reads"]["ms_median"]
    res["reads"].update(counters=c, bytes_read=int(len(text)), bytes_written=written,
                        gb_per_s=round((len(text) + written) / ms / 1e6, 1))
    half = (len(text) + written) // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")

    def copy():
        with torch.cuda.stream(tst):
            dst.copy_(src)

    res["copy"] = timed(copy, tst, a.launches, a.warmup)
    res["copy"].update(bytes_copied=half, gb_per_s=round(2 * half / res["copy"]["ms_median"] / 1e6, 1))
    res["reads"]["copy_over_reads"] = round(res["copy"]["ms_median"] / ms, 4)

    # the Python way on a sample of leading records, with the upload of its arrays
    m = min(a.sample, n)
    rec_bytes = len(text) // n
    t0 = time.perf_counter()
    h = python_way(text[:m * rec_bytes].tobytes(), table, 32)
    up = {k: torch.from_numpy(v.view(np.uint8) if v.dtype.kind == "V" else (v.view(np.int64) if v.dtype == np.uint64 else v)).cuda()
          for k, v in h.items()}
    torch.cuda.synchronize()
    t_py = time.perf_counter() - t0
    del up
    k = len(h["jobs"])
    same = (np.array_equal(o["jobs"][:k * JB].cpu().numpy().view(_lib.JOB_DTYPE), h["jobs"]) and
            np.array_equal(o["codes"][:len(h["codes"]) - 64].cpu().numpy(), h["codes"][:-64]) and
            np.array_equal(o["names"][:len(h["names"])].cpu().numpy(), h["names"]) and
            np.array_equal(o["quals"][:len(h["quals"])].cpu().numpy(), h["quals"]) and
            np.array_equal(o["name_off"][:k + 1].cpu().numpy().view(np.uint64), h["name_off"]) and
            np.array_equal(o["qual_off"][:k + 1].cpu().numpy().view(np.uint64), h["qual_off"]))
    res["python"] = dict(sampled=True, sample_records=m, sample_s=round(t_py, 3), batch_s=round(t_py * n / m, 1),
                         sample_arrays_equal_device=bool(same))
    log(f"[reads_probe] reads {ms:.3f} ms ({res['reads']['gb_per_s']} GB/s), copy {res['copy']['ms_median']:.3f} ms, "
        f"python {res['python']['batch_s']} s (sampled), sample equal: {same}")
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
