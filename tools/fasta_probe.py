#!/usr/bin/env python3
"""Time the index builder's stages around the suffix sorts on the device.

Writes a synthetic FASTA on the host (--mbp million bases in --records records of 60-base
lines, with N runs of 5 to 100 000 bytes), uploads it, and times, with HIP events on one
stream, the median of --launches runs after --warmup warm-ups of

  fasta      hsa_fasta_device of the whole file and its launches one by one
             (hsa_fasta_timing); the bytes it must read (the input, once) and write (.pac,
             .rev.pac, both texts), and GB/s of their sum.  The kernels read the input four
             times (marks, spans, count, pack): the launch times say where the rest goes;
  bwt_files  hsa_bwt_files_device on a BWT of the text's length (random codes: the time
             does not depend on them) and its launches;
  copy       a device-to-device copy whose traffic equals fasta's sum: the floor;
  build      hsa_amd.index_build.build_index on a FASTA of --build-mbp million bases made the
             same way, with host=True and without: seconds per stage (parse: FASTA to both
             texts; sort: the two suffix sorts, with host=True also packing the text and
             unpacking the BWT; bodies: the .bwt / .fmv bodies; write: the eight files), and
             whether the two sets of files are equal.

One JSON object on stdout (and in --out)."""
import argparse
import filecmp
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from choose_probe import log, timed  # noqa: E402

EXTS = ("pac", "ann", "rev.pac", "bwt", "fmv", "rev.bwt", "rev.fmv", "sa")


def make_fasta(mbp, records, seed):
    """`records` records of 60-base lines, mbp * 10^6 bases in all, as one uint8 array; every
    record holds N runs of 5, 9, 10, 50, 1000 and 100 000 bytes (the last only when it fits)."""
    rng = np.random.default_rng(seed)
    per = mbp * 1_000_000 // records // 60 * 60
    parts = []
    for r in range(records):
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, per, dtype=np.uint8)]
        for k in (5, 9, 10, 50, 1000, 100_000):
            if 4 * k < per:
                at = int(rng.integers(0, per - k))
                seq[at:at + k] = ord("N")
        body = np.empty((per // 60, 61), np.uint8)
        body[:, :60] = seq.reshape(-1, 60)
        body[:, 60] = 10
        parts += [np.frombuffer(b">chr%d synthetic record %d\n" % (r + 1, r + 1), np.uint8), body.reshape(-1)]
    return np.concatenate(parts)


def save(res, path):
    """The result so far as JSON text, also written to `path` (a later stage may take long)."""
    txt = json.dumps(res, indent=1)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(txt + "\n")
    return txt


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=int, default=1000)
    ap.add_argument("--build-mbp", type=int, default=1000)
    ap.add_argument("--records", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    import ctypes as C
    from hsa_amd import _lib, fasta, index_build
    import torch
    L = _lib.lib()
    res = dict(tool="fasta_probe", command="python tools/fasta_probe.py " + " ".join(sys.argv[1:] if argv is None else argv),
               mbp=a.mbp, build_mbp=a.build_mbp, records=a.records, launches=a.launches, warmup=a.warmup)
    t0 = time.time()
    text = make_fasta(a.mbp, a.records, 7)
    n = len(text)
    log(f"[fasta_probe] {n} bytes in {time.time() - t0:.1f} s")
    d_in = torch.from_numpy(text).cuda()
    tst = torch.cuda.Stream()
    caps = fasta.first_caps(n)
    out = dict(pac=torch.empty(caps["pac"] + 3 & ~3, dtype=torch.uint8, device="cuda"),
               rpac=torch.empty(caps["rpac"] + 3 & ~3, dtype=torch.uint8, device="cuda"),
               text=torch.empty(caps["text"], dtype=torch.int32, device="cuda"),
               rtext=torch.empty(caps["rtext"], dtype=torch.int32, device="cuda"),
               rec=torch.empty(caps["rec"] * 4, dtype=torch.int32, device="cuda"),
               blk=torch.empty(caps["blk"] * 4, dtype=torch.int32, device="cuda"))
    ctr = torch.zeros(len(_lib.FA_COUNTERS), dtype=torch.int64, device="cuda")
    scratch = torch.empty(fasta.scratch_bytes(n), dtype=torch.uint8, device="cuda")
    b = _lib.FastaBatch(d_in=d_in.data_ptr(), n_in=n, d_counters=ctr.data_ptr(), d_scratch=scratch.data_ptr(),
                        scratch_bytes=scratch.numel())
    for k in caps:
        setattr(b, "d_" + k, out[k].data_ptr())
        setattr(b, k + "_cap", caps[k])
    torch.cuda.synchronize()

    def call():
        _lib.check(L.hsa_fasta_device(0, C.byref(b), tst.cuda_stream))

    res["fasta"] = timed(call, tst, a.launches, a.warmup)
    L.hsa_fasta_timing(1)
    split = []
    for _ in range(a.launches):
        call()
        split.append(fasta.launch_times("fasta"))
    L.hsa_fasta_timing(0)
    c = fasta.counters(ctr)
    assert c["refused"] == fasta.NOT_REFUSED and all(c[w] == c[g] for w, g in (
        ("pac_wanted", "pac_written"), ("rpac_wanted", "rpac_written"), ("text_wanted", "text_written"),
        ("rtext_wanted", "rtext_written"), ("kept", "rec_written"), ("blocks", "blk_written"))), c
    written = c["pac_written"] + c["rpac_written"] + 4 * (c["text_written"] + c["rtext_written"])
    ms = res["fasta"]["ms_median"]
    res["fasta"].update(launch_ms_median={k: round(float(np.median([x[k] for x in split])), 4) for k in split[0]},
                        counters=c, bytes_read=n, bytes_written=written, scratch_bytes=int(scratch.numel()),
                        gb_per_s=round((n + written) / ms / 1e6, 1))
    half = (n + written) // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")

    def copy():
        with torch.cuda.stream(tst):
            dst.copy_(src)

    res["copy"] = timed(copy, tst, a.launches, a.warmup)
    res["copy"].update(bytes_copied=half, gb_per_s=round(2 * half / res["copy"]["ms_median"] / 1e6, 1))
    res["fasta"]["copy_over_fasta"] = round(res["copy"]["ms_median"] / ms, 4)
    del src, dst
    save(res, a.out)

    T = c["T"]
    bwt = torch.randint(-2 ** 31, 2 ** 31 - 1, ((T + 15) // 16 + 8,), dtype=torch.int32, device="cuda")
    n_occ = (T + 255) // 256 + 1
    msb = torch.empty((T + 15) // 16, dtype=torch.int32, device="cuda")
    minor = torch.empty((n_occ + 1) // 2 * 4, dtype=torch.int32, device="cuda")
    major = torch.empty((n_occ + 255) // 256 * 4, dtype=torch.int32, device="cuda")
    nb = C.c_uint64()
    _lib.check(L.hsa_bwt_files_scratch_bytes(0, T, C.byref(nb)))
    bs = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def files():
        _lib.check(L.hsa_bwt_files_device(0, T, bwt.data_ptr(), msb.data_ptr(), minor.data_ptr(), major.data_ptr(),
                                          bs.data_ptr(), bs.numel(), tst.cuda_stream))

    res["bwt_files"] = timed(files, tst, a.launches, a.warmup)
    L.hsa_fasta_timing(1)
    split = []
    for _ in range(a.launches):
        files()
        split.append(fasta.launch_times("bwt"))
    L.hsa_fasta_timing(0)
    moved = 4 * (2 * msb.numel() + minor.numel() + major.numel())
    res["bwt_files"].update(launch_ms_median={k: round(float(np.median([x[k] for x in split])), 4) for k in split[0]},
                            T=T, bytes_read_and_written=moved,
                            gb_per_s=round(moved / res["bwt_files"]["ms_median"] / 1e6, 1))
    save(res, a.out)
    del d_in, out, scratch, bwt, msb, minor, major, bs
    torch.cuda.empty_cache()

    # build_index, both ways, on one file
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "probe.fa")
        (text if a.build_mbp == a.mbp else make_fasta(a.build_mbp, a.records, 7)).tofile(fa)
        del text
        res["build"] = dict(fasta_bytes=os.path.getsize(fa))
        for key, host in (("device", False), ("host", True)):
            tm = {}
            t0 = time.perf_counter()
            lens = index_build.build_index(fa, os.path.join(tmp, key), host=host, times=tm)
            wall = time.perf_counter() - t0
            res["build"][key] = dict(stage_s={k: round(v, 3) for k, v in tm.items()}, wall_s=round(wall, 3),
                                     outside_sort_and_write_s=round(tm["parse"] + tm["bodies"], 3), lengths=lens)
            log(f"[fasta_probe] build_index host={host}: {res['build'][key]}")
        res["build"]["files_equal"] = all(filecmp.cmp(os.path.join(tmp, f"device.index.{e}"), os.path.join(tmp, f"host.index.{e}"),
                                                      shallow=False) for e in EXTS)
    log(f"[fasta_probe] fasta {ms:.3f} ms ({res['fasta']['gb_per_s']} GB/s), copy {res['copy']['ms_median']:.3f} ms, "
        f"bwt_files {res['bwt_files']['ms_median']:.3f} ms")
    print(save(res, a.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
