#!/usr/bin/env python3
"""Time the BGZF inflater (hsa_inflate_bgzf_device, hsa_amd.bgzf) against the host paths.

Input: --reads reads of --read-len bases made by hsa_amd.synth from a synthetic genome of
--genome-mbp Mbp (up to 2 substitutions, random Phred+33 qualities in '#'..'J'), written as
FASTQ, then (a) as BGZF at level 6 with 65 280-byte blocks and (b) as one gzip.compress
stream.  Every figure is the median of --runs runs after --warmup warm-ups, with min and max:

  host_gzip_bgzf     Python's gzip over the BGZF file, from its path: what align._read_input
                     does with any gzip file, and the yardstick of read_input;
  host_gzip_stream   the same over the one-stream file (context);
  host_zlib_threads  zlib over the BGZF blocks on 16 host threads, from bytes (context);
  kernel             hsa_inflate_bgzf_device alone, by events on its stream, in GB/s of text;
  inflate_device     hsa_amd.bgzf.inflate_device whole, from bytes: upload, kernel, copy back;
  read_input         hsa_amd.bgzf.read_input from the BGZF file's path (file read, scan,
                     inflate_device): like for like with host_gzip_bgzf;

align_fastq is not timed here: hsa_amd.align does not read through hsa_amd.bgzf yet.

`faster_beyond_spread` is true when the slower run of the new path beats the fastest run of the
old one (the spans do not overlap).  kernel_report: the compiler's resource usage of
k_inflate_bgzf, read from --kres (tools/kres.sh style text) when the file is there.
One JSON object on stdout (and in --out)."""
import argparse
import concurrent.futures as cf
import gzip
import json
import os
import re
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from choose_probe import log, timed  # noqa: E402

BLOCK = 65280
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")    # bgzip's empty last block


def wall(fn, runs, warmup):
    """Seconds of fn(): median, min and max of `runs` calls after `warmup`; fn ends synchronised."""
    for _ in range(warmup):
        fn()
    s = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        s.append(time.perf_counter() - t0)
    return dict(s_median=round(float(np.median(s)), 4), s_min=round(min(s), 4), s_max=round(max(s), 4), runs=runs)


def bgzf_member(raw):
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    payload = co.compress(raw) + co.flush()
    size = 18 + len(payload) + 8
    assert size <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff\x06\x00BC\x02\x00" + (size - 1).to_bytes(2, "little") + payload +
            zlib.crc32(raw).to_bytes(4, "little") + len(raw).to_bytes(4, "little"))


def kernel_report(path):
    if not os.path.exists(path):
        return None
    txt = open(path).read()
    out = {}
    for key, pat in (("sgprs", r"TotalSGPRs: (\d+)"), ("vgprs", r"VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"),
                     ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                     ("lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)")):
        m = re.search(pat, txt)
        out[key] = int(m.group(1)) if m else None
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--genome-mbp", type=float, default=4.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--kres", default=os.path.join(ROOT, "profiles", "inflate_kres.txt"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from hsa_amd import _lib, bgzf, synth
    import torch
    assert _lib.device_count() > 0, "no GPU visible: nothing is measured without one"
    res = dict(tool="inflate_probe", command="python tools/inflate_probe.py " + " ".join(sys.argv[1:] if argv is None else argv),
               reads=a.reads, read_len=a.read_len, runs=a.runs, warmup=a.warmup)
    tmp = tempfile.mkdtemp(prefix="inflate_probe_")

    def save():
        """The results so far: a run that stops early leaves what it measured."""
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    res["kernel_report"] = kernel_report(a.kres)
    T = int(a.genome_mbp * 1e6)
    t0 = time.time()
    genome = synth.genome_codes(T, 11)
    records = synth.record_layout(T, 3)
    reads, _ = synth.make_reads(genome, records, a.reads, a.read_len, 5, max_mm=2)
    fq = os.path.join(tmp, "reads.fq")
    synth.write_fastq(fq, reads, qual_seed=9)
    text = open(fq, "rb").read()
    log(f"[inflate_probe] {a.reads} reads ({len(text)} bytes of text) in {time.time() - t0:.1f} s")
    t0 = time.time()
    with cf.ThreadPoolExecutor(16) as ex:
        members = list(ex.map(bgzf_member, [text[k:k + BLOCK] for k in range(0, len(text), BLOCK)]))
    data = b"".join(members) + EOF_MARKER
    p_bgzf, p_gz = os.path.join(tmp, "reads.bgzf.fq.gz"), os.path.join(tmp, "reads.stream.fq.gz")
    open(p_bgzf, "wb").write(data)
    open(p_gz, "wb").write(gzip.compress(text, 6))
    table = bgzf.scan(data)
    res.update(text_bytes=len(text), bgzf_bytes=len(data), gzip_stream_bytes=os.path.getsize(p_gz), blocks=int(len(table)))
    log(f"[inflate_probe] compressed in {time.time() - t0:.1f} s: BGZF {len(data)} bytes in {len(table)} blocks")

    # 1. the host paths
    def host_gzip(path):
        with gzip.open(path, "rb") as f:
            return f.read()
    assert host_gzip(p_bgzf) == text
    res["host_gzip_bgzf"] = wall(lambda: host_gzip(p_bgzf), a.runs, a.warmup)
    res["host_gzip_stream"] = wall(lambda: host_gzip(p_gz), a.runs, a.warmup)
    spans = [(int(r["in_off"]), int(r["in_off"]) + int(r["in_len"])) for r in table]

    def host_threads():
        with cf.ThreadPoolExecutor(16) as ex:
            return b"".join(ex.map(lambda s: zlib.decompress(data[s[0]:s[1]], -15), spans))
    assert host_threads() == text
    res["host_zlib_threads"] = wall(host_threads, a.runs, a.warmup)
    save()

    # 2. the kernel alone
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_rows = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.empty(len(text), dtype=torch.uint8, device="cuda")
    d_status = torch.empty(len(table), dtype=torch.int32, device="cuda")
    d_ctr = torch.zeros(3, dtype=torch.int64, device="cuda")
    tst = torch.cuda.Stream()
    b = _lib.InflateBatch(d_in=d_in.data_ptr(), n_in=len(data), d_blocks=d_rows.data_ptr(), n_blocks=len(table),
                          d_out=d_out.data_ptr(), out_cap=len(text), d_status=d_status.data_ptr(), d_counters=d_ctr.data_ptr())
    torch.cuda.synchronize()
    res["kernel"] = timed(lambda: _lib.inflate_bgzf_device(b, stream=tst.cuda_stream), tst, a.launches, 2)
    res["kernel"].update(launches=a.launches, gb_per_s_out=round(len(text) / res["kernel"]["ms_median"] / 1e6, 2),
                         all_ok=bool((d_status.cpu().numpy() == 0).all()), bytes_equal=bool(d_out.cpu().numpy().tobytes() == text))
    del d_in, d_out
    save()
    log(f"[inflate_probe] kernel {res['kernel']['ms_median']} ms, {res['kernel']['gb_per_s_out']} GB/s of text")

    # 3. inflate_device whole, and read_input from the path
    def whole():
        out, d_text, stats = bgzf.inflate_device(None, data, table=table)
        assert stats["host_blocks"] == 0 and len(out) == len(text)

    def from_path():
        out, d_text, stats = bgzf.read_input(None, p_bgzf)
        assert stats["host_blocks"] == 0 and len(out) == len(text)
    assert bgzf.read_input(None, p_bgzf)[0] == text
    res["inflate_device"] = wall(whole, a.runs, a.warmup)
    res["read_input"] = wall(from_path, a.runs, a.warmup)
    res["read_input"]["faster_beyond_spread"] = bool(res["read_input"]["s_max"] < res["host_gzip_bgzf"]["s_min"])
    res["read_input"]["speedup_median"] = round(res["host_gzip_bgzf"]["s_median"] / res["read_input"]["s_median"], 2)
    save()
    log(f"[inflate_probe] host gzip {res['host_gzip_bgzf']['s_median']} s, read_input {res['read_input']['s_median']} s")

    shutil.rmtree(tmp, ignore_errors=True)
    save()
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
