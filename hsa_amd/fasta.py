"""The index builder's device stages around the suffix sorts: FASTA bytes to the packed
texts and the annotation tables (hsa_fasta_device), and a BWT to its .bwt / .fmv file
bodies (hsa_bwt_files_device).  hsa_amd/index_build.py's parse_fasta, pac_bytes,
reverse_pac, pac_text and index_io's occ_files, pack_codes_msb are the host restatement
these are tested against."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

MAX_INPUT = (1 << 32) - 256     # hsa_fasta_device: n_in under 2^32 - 256
NOT_REFUSED = (1 << 64) - 1


@dataclass
class FastaDevice:
    """What hsa_fasta_device left: device tensors cut to what was written (the texts keep
    their 8 zero words), the two small tables on the host, the counters by name."""
    pac: object            # uint8, the .pac bytes
    rpac: object           # uint8, the .rev.pac bytes
    text: object           # int32 words, LSB-first, T characters + padding
    rtext: object
    rec: np.ndarray        # uint32 (kept records, 4): name offset, name length, L, first block
    blk: np.ndarray        # uint32 (blocks, 4): kept record, start, end, ori
    counters: dict

    @property
    def refused(self):
        """The byte offset at which the input is refused, or None."""
        r = self.counters["refused"]
        return None if r == NOT_REFUSED else r


def _stream(stream):
    import torch
    return torch.cuda.current_stream().cuda_stream if stream is None else stream


def scratch_bytes(n_in: int, device: int = 0) -> int:
    n = C.c_uint64()
    _lib.check(_lib.lib().hsa_fasta_scratch_bytes(device, n_in, C.byref(n)))
    return n.value


def run_device(d_in, n_in: int, caps: dict, device: int = 0, stream=None):
    """One hsa_fasta_device call over the first n_in bytes of the uint8 device tensor
    `d_in` with the capacities `caps` (pac, rpac in bytes; text, rtext in words; rec, blk in
    rows).  Returns (tensors by name, counters tensor); launches on `stream` (default:
    torch's current stream) and does not synchronise."""
    import torch
    dev = d_in.device
    out = dict(pac=torch.empty(caps["pac"] + 3 & ~3, dtype=torch.uint8, device=dev),
               rpac=torch.empty(caps["rpac"] + 3 & ~3, dtype=torch.uint8, device=dev),
               text=torch.empty(caps["text"], dtype=torch.int32, device=dev),
               rtext=torch.empty(caps["rtext"], dtype=torch.int32, device=dev),
               rec=torch.empty((caps["rec"], _lib.FA_REC_WORDS), dtype=torch.int32, device=dev),
               blk=torch.empty((caps["blk"], 4), dtype=torch.int32, device=dev))
    ctr = torch.zeros(len(_lib.FA_COUNTERS), dtype=torch.int64, device=dev)
    scratch = torch.empty(scratch_bytes(n_in, device), dtype=torch.uint8, device=dev)
    b = _lib.FastaBatch(d_in=d_in.data_ptr() if n_in else None, n_in=n_in,
                        d_pac=out["pac"].data_ptr(), pac_cap=caps["pac"], d_rpac=out["rpac"].data_ptr(), rpac_cap=caps["rpac"],
                        d_text=out["text"].data_ptr(), text_cap=caps["text"], d_rtext=out["rtext"].data_ptr(),
                        rtext_cap=caps["rtext"], d_rec=out["rec"].data_ptr(), rec_cap=caps["rec"],
                        d_blk=out["blk"].data_ptr(), blk_cap=caps["blk"], d_counters=ctr.data_ptr(),
                        d_scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    _lib.check(_lib.lib().hsa_fasta_device(device, C.byref(b), _stream(stream)))
    return out, ctr


def counters(ctr) -> dict:
    return dict(zip(_lib.FA_COUNTERS, (int(v) for v in ctr.cpu().numpy().view(np.uint64))))


def first_caps(n_in: int) -> dict:
    """Capacities that hold every text an input of n_in bytes can give, and tables for a
    genome-like record and block count: a FASTA with more asks for a second run."""
    words = (n_in + 3 + 15) // 16 + 2 + _lib.FA_PAD_WORDS
    return dict(pac=n_in // 4 + 8, rpac=n_in // 4 + 8, text=words, rtext=words,
                rec=1024 + (n_in >> 16), blk=4096 + (n_in >> 14))


def parse_device(d_in, n_in: int | None = None, device: int = 0, stream=None) -> FastaDevice:
    """hsa_fasta_device over a whole FASTA on the device; runs again with the wanted table
    sizes when the first capacities were short.  Synchronises (it reads the counters)."""
    n_in = int(d_in.numel()) if n_in is None else n_in
    if n_in >= MAX_INPUT:
        raise ValueError(f"a FASTA of {n_in} bytes: the device loader (and the .ann and .sa formats) end under 2^32 - 256")
    caps = first_caps(n_in)
    for _ in range(2):
        out, ctr = run_device(d_in, n_in, caps, device, stream)
        c = counters(ctr)
        short = {k: c[w] for k, w, g in (("pac", "pac_wanted", "pac_written"), ("rpac", "rpac_wanted", "rpac_written"),
                                         ("text", "text_wanted", "text_written"), ("rtext", "rtext_wanted", "rtext_written"),
                                         ("rec", "kept", "rec_written"), ("blk", "blocks", "blk_written")) if c[w] > c[g]}
        if not short:
            break
        caps.update(short)
    else:
        raise _lib.HsaError(f"hsa_fasta_device: capacities still short after a second run: {short}")
    return FastaDevice(pac=out["pac"][:c["pac_wanted"]], rpac=out["rpac"][:c["rpac_wanted"]],
                       text=out["text"][:c["text_wanted"]], rtext=out["rtext"][:c["rtext_wanted"]],
                       rec=out["rec"][:c["kept"]].cpu().numpy().view(np.uint32),
                       blk=out["blk"][:c["blocks"]].cpu().numpy().view(np.uint32), counters=c)


def ann_rows(data, rec: np.ndarray, blk: np.ndarray):
    """parse_fasta's annotation rows, (name, [(start, end, ori), ...]) per kept record, from
    the device tables and the input (bytes or a uint8 array; an empty block's end is start - 1)."""
    ann = []
    for r, (off, ln, _, b0) in enumerate(rec.tolist()):
        b1 = int(rec[r + 1][3]) if r + 1 < len(rec) else len(blk)
        rows = [(int(s), int(s) - 1 + ((int(e) - int(s) + 1) & 0xFFFFFFFF), int(o)) for _, s, e, o in blk[b0:b1].tolist()]
        ann.append((bytes(data[off:off + ln]).decode("latin-1"), rows))
    return ann


def bwt_files_device(d_bwt_lsb, T: int, device: int = 0, stream=None):
    """hsa_bwt_files_device: (code words, minor, major) as int32 device tensors, the bodies
    of the .bwt and .fmv files of the builder's LSB-first BWT of T characters."""
    import torch
    dev = d_bwt_lsb.device
    n_occ = (T + 255) // 256 + 1
    msb = torch.empty((T + 15) // 16, dtype=torch.int32, device=dev)
    minor = torch.empty((n_occ + 1) // 2 * 4, dtype=torch.int32, device=dev)
    major = torch.empty((n_occ + 255) // 256 * 4, dtype=torch.int32, device=dev)
    n = C.c_uint64()
    _lib.check(_lib.lib().hsa_bwt_files_scratch_bytes(device, T, C.byref(n)))
    scratch = torch.empty(n.value, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().hsa_bwt_files_device(device, T, d_bwt_lsb.data_ptr(), msb.data_ptr(), minor.data_ptr(),
                                               major.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream(stream)))
    return msb, minor, major


def launch_times(which: str = "fasta") -> dict:
    """ms per launch of the last hsa_fasta_device ("fasta") or hsa_bwt_files_device ("bwt")
    call made after lib().hsa_fasta_timing(1); waits for it."""
    names = _lib.FA_LAUNCHES if which == "fasta" else _lib.BF_LAUNCHES
    ms = np.zeros(len(names), np.float32)
    fn = _lib.lib().hsa_fasta_launch_times if which == "fasta" else _lib.lib().hsa_bwt_files_launch_times
    _lib.check(fn(ms))
    return dict(zip(names, (float(v) for v in ms)))
