"""BGZF test input, made at run time: the member and file writers, a small DEFLATE encoder for
the payloads zlib never emits, a parser of a dynamic block's header, and the valid and corrupt
blocks that tests/test_inflate_san.py (host, under sanitizers) and tests/test_gpu_inflate.py
(device) both run.  zlib.decompress is the oracle for the bytes of every valid block."""
import functools
import gzip
import os
import struct
import zlib

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

# hsa_gpu.h's HSA_INF_*
OK, E_INPUT, E_BTYPE, E_STORED, E_CODES, E_SYMBOL, E_DIST, E_OUTPUT, E_SIZE, E_CRC, E_TRAIL, E_ROW = range(12)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(raw) + co.flush()


def bgzf_member(payload_deflate, raw, crc=None, isize=None):
    """One BGZF member around a deflate payload: the gzip header with FEXTRA and the BC
    subfield (BSIZE = member size - 1), the payload, CRC32 and ISIZE of `raw`."""
    size = 18 + len(payload_deflate) + 8
    assert size <= 65536, size
    head = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, size - 1)
    return head + payload_deflate + struct.pack("<II", zlib.crc32(raw) if crc is None else crc, len(raw) if isize is None else isize)


def bgzf_file(raw, block=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True):
    """`raw` as bgzip writes it: members of `block` input bytes each, then the 28-byte EOF marker."""
    out = [bgzf_member(deflate(raw[k:k + block], level, strategy), raw[k:k + block]) for k in range(0, len(raw), block)]
    return b"".join(out) + (EOF_MARKER if eof else b"")


@functools.lru_cache(maxsize=None)
def fastq_snippet(n=3000):
    return gzip.open(os.path.join(GOLD, "dropin_reads.fq.gz")).read()[:n]


# ---------------------------------------------------------------- a DEFLATE encoder for hand-made payloads
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        """nbits of value, lowest first (header fields, extra bits)."""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """A Huffman code: highest bit first."""
        for k in range(length - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def done(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def canonical(lengths):
    """symbol -> (code, length) of the canonical code of `lengths` (RFC 1951, 3.2.2)."""
    codes, code = {}, 0
    for l in range(1, 16):
        for s, ls in enumerate(lengths):
            if ls == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# complete sets that give every symbol a code: 226 x 8 + 60 x 9 bits; 2 x 4 + 28 x 5 bits; 13 x 4 + 6 x 5 bits
ALL_LITLEN = [8] * 226 + [9] * 60
ALL_DIST = [4] * 2 + [5] * 28
CL_LENS = [4] * 13 + [5] * 6


def _rle(lens):
    """The lengths as code-length symbols (symbol, extra value, extra bits), runs taken
    greedily over the whole list: a run does not stop where the distance lengths begin."""
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        run, v = j - i, lens[i]
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11, 7))
                run -= r
            if run >= 3:
                out.append((17, run - 3, 3))
                run = 0
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3, 2))
                run -= r
        out += [(v, 0, 0)] * run
        i = j
    return out


def dynamic_block(tokens, litlen, dist, final=True, w=None, end=True):
    """A dynamic-Huffman block with the given code lengths (len(litlen) = HLIT + 257, len(dist)
    = HDIST + 1) holding `tokens`: an int is a literal, (length, distance) a match.  The
    code-length code is CL_LENS; runs of lengths are encoded across the two sets.  Returns the
    payload's bytes, or goes on in the BitWriter w (then returns None)."""
    own = w is None
    w = w or BitWriter()
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(len(litlen) - 257, 5)
    w.put(len(dist) - 1, 5)
    w.put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    for s, v, nb in _rle(list(litlen) + list(dist)):
        w.code(*cl[s])
        w.put(v, nb)
    lc, dc = canonical(litlen), canonical(dist)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lc[t])
            continue
        ln, d = t
        s = max(k for k in range(29) if LEN_BASE[k] <= ln and (k == 28 or ln < 258))
        w.code(*lc[257 + s])
        w.put(ln - LEN_BASE[s], LEN_EXTRA[s])
        s = max(k for k in range(30) if DIST_BASE[k] <= d)
        w.code(*dc[s])
        w.put(d - DIST_BASE[s], DIST_EXTRA[s])
    if end:
        w.code(*lc[256])
    return w.done() if own else None


def apply_tokens(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


# ---------------------------------------------------------------- a dynamic block's header, parsed
def dynamic_header(payload):
    """The header of the dynamic block `payload` begins with: dict(final, nlen, ndist, lengths,
    crossing: a code-length repeat ran from the literal/length lengths into the distance ones)."""
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for k in range(n):
            v |= ((payload[pos >> 3] >> (pos & 7)) & 1) << k
            pos += 1
        return v

    final, typ = bits(1), bits(2)
    assert typ == 2, f"block type {typ}"
    nlen, ndist, ncode = bits(5) + 257, bits(5) + 1, bits(4) + 4
    cl = [0] * 19
    for k in range(ncode):
        cl[CL_ORDER[k]] = bits(3)
    by_code = {v: s for s, v in canonical(cl).items()}
    lens, crossing = [], False
    while len(lens) < nlen + ndist:
        code = ln = 0
        while (code, ln) not in by_code:
            code, ln = (code << 1) | bits(1), ln + 1
            assert ln <= 7
        s = by_code[(code, ln)]
        if s < 16:
            lens.append(s)
            continue
        rep, v = (3 + bits(2), lens[-1]) if s == 16 else (3 + bits(3), 0) if s == 17 else (11 + bits(7), 0)
        crossing |= len(lens) < nlen < len(lens) + rep
        lens += [v] * rep
    assert len(lens) == nlen + ndist
    return dict(final=final, nlen=nlen, ndist=ndist, lengths=lens, crossing=crossing)


def block_type(payload):
    return (payload[0] >> 1) & 3


# ---------------------------------------------------------------- the cases
def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def crossing_repeat():
    """'abc' and two matches of 6 at distance 3, under a header whose zero lengths of literal/length
    symbols 261..285 and of distance symbols 0 and 1 are one code-18 run; the distance set is
    the single code of symbol 2, one bit long."""
    litlen = [0] * 286
    for s, l in ((97, 2), (98, 2), (99, 2), (256, 3), (260, 3)):   # a, b, c, end, length 6
        litlen[s] = l
    tokens = [97, 98, 99, (6, 3), (6, 3)]
    return dynamic_block(tokens, litlen, [0, 0, 1]), apply_tokens(tokens)


def single_distance_code():
    litlen = [0] * 258
    for s, l in ((120, 1), (256, 2), (257, 2)):                    # x, end, length 3
        litlen[s] = l
    tokens = [120, (3, 1), (3, 1), 120]
    return dynamic_block(tokens, litlen, [1]), apply_tokens(tokens)


def distinct_256():
    """256 distinct literals in a dynamic block whose distance set is one zero length (zlib
    stores such bytes): 255 codes of 8 bits, 2 of 9."""
    tokens = list(range(256))
    return dynamic_block(tokens, [8] * 255 + [9] * 2, [0]), bytes(tokens)


def max_distance():
    """40 000 bytes whose last 7 232 repeat what lies 32 768 back (zlib stops at 32 506)."""
    first = _rand(32768, 5)
    tokens = list(first) + [(258, 32768)] * 28 + [(8, 32768)]
    raw = apply_tokens(tokens)
    assert len(raw) == 40000 and raw[32768:] == first[:7232]
    return dynamic_block(tokens, ALL_LITLEN, ALL_DIST), raw


def three_types():
    """One payload of a stored, a fixed and a dynamic block with a Z_SYNC_FLUSH (an empty stored
    block) behind the first two."""
    fq = fastq_snippet(6000)
    parts, raws = [], (fq[:500], fq[500:1500], fq[1500:])
    for k, (raw, level, strategy) in enumerate(zip(raws, (0, 9, 9), (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_DEFAULT_STRATEGY))):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        part = co.compress(raw) + (co.flush(zlib.Z_SYNC_FLUSH) if k < 2 else co.flush())
        assert block_type(part) == k
        parts.append(part)
    return b"".join(parts), b"".join(raws)


@functools.lru_cache(maxsize=None)
def valid_cases():
    """(name, deflate payload, the bytes it holds)."""
    fq = fastq_snippet()
    cases = [("empty", deflate(b""), b""),
             ("one_literal", deflate(b"A"), b"A"),
             ("stored_0", deflate(b"", 0), b""),
             ("stored_1", deflate(b"Q", 0), b"Q"),
             ("stored_65280", deflate(_rand(65280, 1), 0), _rand(65280, 1)),
             ("fixed_fastq", deflate(fq, 9, zlib.Z_FIXED), fq),
             ("dynamic_fastq", deflate(fq, 9), fq),
             ("dynamic_256_distinct", *distinct_256()),
             ("dynamic_A60000", deflate(b"A" * 60000, 9), b"A" * 60000),
             ("dynamic_single_distance", *single_distance_code())]
    for period in (2, 3, 63, 64, 65):
        raw = (_rand(period, 10 + period) * 1000)[:1000]
        cases.append((f"overlap_{period}", deflate(raw, 9), raw))
    cases.append(("max_distance", *max_distance()))
    big = (fastq_snippet(20000) * 4)[:65536]
    cases += [("isize_65536", deflate(big, 6), big), ("three_types", *three_types()), ("crossing_repeat", *crossing_repeat())]
    for name, payload, raw in cases:
        assert zlib.decompress(payload, -15) == raw, name
    by = {c[0]: c for c in cases}
    assert block_type(by["stored_0"][1]) == 0 and block_type(by["stored_65280"][1]) == 0
    assert block_type(by["fixed_fastq"][1]) == 1
    for name in ("dynamic_fastq", "dynamic_256_distinct", "dynamic_A60000", "dynamic_single_distance", "max_distance",
                 "crossing_repeat"):
        assert block_type(by[name][1]) == 2, name
    h = dynamic_header(by["crossing_repeat"][1])
    assert h["crossing"] and h["lengths"][h["nlen"]:] == [0, 0, 1]
    h = dynamic_header(by["dynamic_single_distance"][1])
    assert h["lengths"][h["nlen"]:] == [1] and not h["crossing"]
    assert dynamic_header(by["dynamic_256_distinct"][1])["lengths"][257:] == [0]
    return cases


@functools.lru_cache(maxsize=None)
def corrupt_cases():
    """(name, payload, isize, crc, the status hsa_gpu.h names for it)."""
    fq = fastq_snippet()
    good = deflate(fq, 9)
    crc = zlib.crc32(fq)
    far = dynamic_block([97, 98, 99, (3, 4)], ALL_LITLEN, ALL_DIST)          # 3 bytes out, distance 4
    over = [8] * 226 + [9] * 60
    over[0] = over[1] = over[2] = 1                                          # three codes of one bit
    return [("cut_by_one", good[:-1], len(fq), crc, E_INPUT),
            ("block_type_3", b"\x07", 0, 0, E_BTYPE),
            ("len_nlen", b"\x01\x05\x00\x00\x00hello", 5, zlib.crc32(b"hello"), E_STORED),
            ("distance_before_start", far, 6, 0, E_DIST),
            ("wrong_crc", good, len(fq), crc ^ 1, E_CRC),
            ("isize_one_small", good, len(fq) - 1, crc, E_OUTPUT),
            ("isize_one_large", good, len(fq) + 1, crc, E_SIZE),
            ("oversubscribed", dynamic_block([], over, ALL_DIST), 0, 0, E_CODES)]
