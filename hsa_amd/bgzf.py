"""BGZF input: the blocked gzip `bgzip` writes, inflated on the device.

A BGZF file is a series of independent gzip members of at most 64 KB, each with its size in a
`BC` extra subfield and CRC32 and ISIZE in its last 8 bytes; gzread in the reference reads it
like any other gzip file.  scan() walks the members on the host (nothing is inflated for it),
inflate_device() uploads the file's bytes and runs hsa_inflate_bgzf_device, one wavefront per
block, and read_input() opens a file as the readers take it: plain, BGZF or general gzip.
hsa_amd.bam.open_text reads a BAM file through it (`hsa_amd.align -b`); FASTQ and FASTA in front
of hsa_amd.align and hsa_amd.index_build do not go through it yet ("BGZF input").

A block the device refuses (any status but HSA_INF_OK) is inflated again on the host with
zlib, which also decides whether the file is corrupt: the errors are zlib's and the CRC and
length checks gzip makes.  General gzip, one serial DEFLATE stream, stays on the host whole."""
from __future__ import annotations

import gzip
import struct
import zlib

import numpy as np

from ._lib import BGZF_BLOCK_DTYPE, HSA_INF_OK, INF_COUNTERS, InflateBatch, inflate_bgzf_device

MAGIC = b"\x1f\x8b"
NO_STATS = dict(blocks=0, device_blocks=0, host_blocks=0, bytes_in=0, bytes_out=0, groups=0)


def scan(data):
    """The block table (BGZF_BLOCK_DTYPE: the deflate payload's offset and length, ISIZE, the
    output offset as the running sum of ISIZE, CRC32) of the BGZF file `data`, or None when any
    member is not BGZF: no gzip magic, a method other than 8, a flag other than FEXTRA, no `BC`
    subfield of length 2, a BSIZE that is too small or reaches past the end (so also trailing
    bytes).  All or nothing: a mixed file is the host's."""
    data = memoryview(data)
    n, pos, rows = len(data), 0, []
    while pos < n:
        if n - pos < 12 + 8 or bytes(data[pos:pos + 4]) != b"\x1f\x8b\x08\x04":
            return None
        xlen = struct.unpack_from("<H", data, pos + 10)[0]
        x, xend, bsize = pos + 12, pos + 12 + xlen, None
        if xend > n:
            return None
        while x + 4 <= xend:
            si, slen = bytes(data[x:x + 2]), struct.unpack_from("<H", data, x + 2)[0]
            if x + 4 + slen > xend:
                return None
            if si == b"BC":
                if slen != 2 or bsize is not None:
                    return None
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        if x != xend or bsize is None:
            return None
        end = pos + bsize + 1
        if end > n or end - 8 < xend:
            return None
        crc, isize = struct.unpack_from("<II", data, end - 8)
        rows.append((xend, end - 8 - xend, isize, 0, crc, 0))
        pos = end
    t = np.array(rows, BGZF_BLOCK_DTYPE) if rows else np.zeros(0, BGZF_BLOCK_DTYPE)
    t["out_off"] = np.cumsum(t["isize"], dtype=np.uint64) - t["isize"]
    return t


def _inflate_host(data, row):
    """One block through zlib, checked as gzip checks a member."""
    d = zlib.decompressobj(-15)
    raw = d.decompress(bytes(data[int(row["in_off"]):int(row["in_off"]) + int(row["in_len"])]))
    if not d.eof:
        raise EOFError("Compressed file ended before the end-of-stream marker was reached")
    if d.unused_data:
        raise gzip.BadGzipFile("bytes behind the end of a BGZF block's stream")
    if zlib.crc32(raw) != int(row["crc"]):
        raise gzip.BadGzipFile("CRC check failed")
    if len(raw) != int(row["isize"]):
        raise gzip.BadGzipFile("Incorrect length of data produced")
    return raw


def inflate_device(gi, data, budget=1 << 30, table=None):
    """The text of the BGZF file `data` (bytes; table: its scan): (the text as host bytes, the
    text as a uint8 device tensor when all of it was inflated in one group, else None,
    statistics).  The file's bytes go to the device once; the blocks are inflated in groups
    whose output stays within `budget` bytes (one block at least), each group's text copied
    back; a block with a status other than OK is inflated on the host, which raises as reading
    the file through gzip does when the block is truly corrupt.  gi: the GpuIndex whose device
    is used (None: the current one).  Statistics: blocks, device_blocks, host_blocks,
    bytes_in, bytes_out, groups."""
    import torch
    from ._lib import lib
    t = scan(data) if table is None else table
    if t is None:
        raise ValueError("not a BGZF file")
    device = lib().hsa_index_device(gi.h) if getattr(gi, "h", None) else torch.cuda.current_device()
    stats = dict(NO_STATS, blocks=len(t), bytes_in=len(data), bytes_out=int(t["isize"].sum(dtype=np.uint64)))
    if not len(t):
        return b"", torch.zeros(1, dtype=torch.uint8, device=f"cuda:{device}"), stats
    with torch.cuda.device(device):
        d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
        ends = (t["out_off"] + t["isize"]).astype(np.uint64)
        parts, first, d_text = [], 0, None
        while first < len(t):
            base = int(t["out_off"][first])
            last = max(int(np.searchsorted(ends, base + int(budget), side="right")), first + 1)
            g = t[first:last].copy()
            g["out_off"] -= np.uint64(base)
            cap = int(ends[last - 1]) - base
            d_out = torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda")
            d_rows = torch.from_numpy(g.view(np.uint8).reshape(-1)).cuda()
            d_status = torch.empty(len(g), dtype=torch.int32, device="cuda")
            d_ctr = torch.zeros(len(INF_COUNTERS), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            inflate_bgzf_device(InflateBatch(d_in=d_in.data_ptr(), n_in=len(data), d_blocks=d_rows.data_ptr(), n_blocks=len(g),
                                             d_out=d_out.data_ptr(), out_cap=cap, d_status=d_status.data_ptr(),
                                             d_counters=d_ctr.data_ptr()), device)
            torch.cuda.synchronize()
            ctr = dict(zip(INF_COUNTERS, (int(v) for v in d_ctr.cpu().numpy())))
            assert ctr["done"] + ctr["refused"] == len(g)
            text = d_out[:cap].cpu().numpy()
            if ctr["refused"]:
                status = d_status.cpu().numpy().view(np.uint32)
                for k in np.flatnonzero(status != HSA_INF_OK):
                    raw = _inflate_host(data, g[k])
                    at = int(g["out_off"][k])
                    text[at:at + len(raw)] = np.frombuffer(raw, np.uint8)
                if first == 0 and last == len(t):
                    d_out[:cap] = torch.from_numpy(text).cuda()      # (the resident text with the host's blocks)
            stats["device_blocks"] += ctr["done"]
            stats["host_blocks"] += ctr["refused"]
            stats["groups"] += 1
            parts.append(text)
            if first == 0 and last == len(t):
                d_text = d_out
            first = last
    return (parts[0] if len(parts) == 1 else np.concatenate(parts)).tobytes(), d_text, stats


def read_input(gi, path):
    """The bytes of the file at `path` as the readers take them: (the text as host bytes, the
    text as a device tensor or None, statistics).  A plain file is read as it is; a file with
    the gzip magic that scan() takes goes through inflate_device; any other gzip file through
    Python's gzip, as the reference reads either through zlib.  The statistics are 0 for all
    but BGZF."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] != MAGIC:
        return data, None, dict(NO_STATS)
    t = scan(data)
    if t is None:
        with gzip.open(path, "rb") as f:
            return f.read(), None, dict(NO_STATS)
    return inflate_device(gi, data, table=t)
