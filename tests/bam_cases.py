"""BAM test input, made at run time with struct and zlib: records, the header, three layouts
of the container (members that end at record boundaries as htslib writes them, the text cut
every N bytes regardless of records, one gzip stream), BAMs made of a FASTQ fixture's reads, and
the small valid and edge-case texts that tests/test_bam_san.py (host, under sanitizers),
tests/test_bam_cpu.py and tests/test_gpu_bam.py share.  hsa_amd.bam.parse_host is the
restatement the device loader and the sanitizer program are compared with."""
import functools
import gzip
import struct

import bgzf_cases as bc

NT16 = b"=ACMGRSVTWYHKDBN"
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
FLAG_UNMAPPED, FLAG_REVERSE, FLAG_READ1, FLAG_READ2, FLAG_SECONDARY, FLAG_SUPPLEMENTARY = 0x4, 0x10, 0x40, 0x80, 0x100, 0x800


def header(text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=((b"chrT", 5000),)):
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def pack_bases(seq: bytes) -> bytes:
    """Two bases per byte, the first in the high nibble; a letter NT16 lacks is N."""
    nib = [NT16.find(bytes([c]).upper()) for c in seq]
    nib = [15 if v < 0 else v for v in nib] + [0]
    return bytes((nib[k] << 4) | nib[k + 1] for k in range(0, len(seq), 2))


def record(name, seq, qual=None, flag=FLAG_UNMAPPED, cigar=(), aux=b"", name_field=None):
    """One record.  seq: the stored bases as letters; qual: the stored phred bytes (None: 0xFF,
    no qualities); cigar: u32 operations; name_field: the bytes of the name field when they
    are not name + NUL (an embedded NUL, an empty name)."""
    nm = name + b"\0" if name_field is None else name_field
    qual = b"\xff" * len(seq) if qual is None else qual
    assert len(qual) == len(seq) and 1 <= len(nm) <= 255
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(nm), 0, 4680, len(cigar), flag, len(seq), -1, -1, 0)
    body += nm + b"".join(struct.pack("<I", c) for c in cigar) + pack_bases(seq) + qual + aux
    return struct.pack("<I", len(body)) + body


def revcomp(seq: bytes) -> bytes:
    return seq.translate(_COMP)[::-1]


def from_fastq(fq: bytes, flags=None):
    """Records that the rule maps back to the reads of the FASTQ text: names as
    reads.parse_host gives them; every third record stored reversed with FLAG 0x10; records
    with CIGAR operations (k % 5 == 1) and auxiliary tags (k % 4 == 2), so that the field
    offsets move.  flags: per-read extra FLAG bits (0x40, 0x80, ...)."""
    from hsa_amd import reads
    p = reads.parse_host(fq)
    out = []
    for k, (name, seq, qual) in enumerate(zip(p["names"], p["raw"], p["quals"])):
        q = bytes(c - 33 for c in qual)
        flag = FLAG_UNMAPPED | (flags[k] if flags is not None else 0)
        if k % 3 == 2:
            seq, q, flag = revcomp(seq), q[::-1], flag | FLAG_REVERSE
        cigar = ((len(seq) - 3) << 4, 3 << 4 | 4) if k % 5 == 1 else ()
        aux = b"NMC\x02" + b"RGZgroup1\0" if k % 4 == 2 else b"XSi\x2a\0\0\0" if k % 4 == 3 else b""
        out.append(record(name, seq, q, flag, cigar, aux))
    return out


def fastq_of(records_fq: bytes, keep):
    """The FASTQ records keep(k) is true for."""
    ls = records_fq.split(b"\n")
    return b"".join(b"\n".join(ls[4 * k:4 * k + 4]) + b"\n" for k in range(len(ls) // 4) if keep(k))


# ---------------------------------------------------------------- layouts
def text_of(records, head=None):
    return (header() if head is None else head) + b"".join(records)


def aligned(records, member=65280, head=None, level=6):
    """The file as htslib writes it: the header in members of its own; a member is flushed
    before a record that does not fit in what is left of it, and a record larger than a member
    runs over as many as it needs, the next records joining its tail."""
    head = header() if head is None else head
    chunks = [head[k:k + member] for k in range(0, len(head), member)]
    cur = b""
    for rec in records:
        if cur and len(cur) + len(rec) > member:
            chunks.append(cur)
            cur = b""
        while len(cur) + len(rec) > member:
            take = member - len(cur)
            chunks.append(cur + rec[:take])
            cur, rec = b"", rec[take:]
        cur += rec
    if cur:
        chunks.append(cur)
    return b"".join(bc.bgzf_member(bc.deflate(c, level), c) for c in chunks) + bc.EOF_MARKER


def straddling(records, every, head=None):
    """The text cut every `every` bytes, regardless of records (as htsjdk may)."""
    return bc.bgzf_file(text_of(records, head), block=every)


def one_stream(records, head=None):
    return gzip.compress(text_of(records, head), 6)


# ---------------------------------------------------------------- small texts for the serial core
@functools.lru_cache(maxsize=None)
def small_fastq(n=12):
    """n records of the drop-in fixture, cut to lengths odd and even, short and over 35."""
    ls = bc.fastq_snippet(20000).split(b"\n")
    out = []
    for k in range(n):
        h, s, _, q = ls[4 * k:4 * k + 4]
        cut = (100, 37, 36, 51, 1, 2, 64, 65, 99, 15, 14, 70)[k % 12]
        out.append(h + b"\n" + s[:cut] + b"\n+\n" + q[:cut] + b"\n")
    return b"".join(out)


def edge_records():
    """Records for the rules beside the plain case: every nt16 code, no qualities, an empty
    read, names with an embedded NUL and with /1, FLAG 0x40 / 0x80 / neither, secondary and
    supplementary, low qualities at the end of a reversed and of a forward read (trimming)."""
    every = NT16 * 3
    low_tail = bytes([30] * 60 + [2] * 20)
    return [
        record(b"all16", every, bytes(range(len(every)))),
        record(b"all16rev", every, bytes(range(len(every))), FLAG_UNMAPPED | FLAG_REVERSE),
        record(b"noqual", b"ACGTACGTACGTACGTACGTA"),
        record(b"empty", b"", b""),
        record(b"cut", b"ACGTTGCA", bytes([20] * 8), name_field=b"cut\0tail\0"),
        record(b"pair/1", b"ACGTTGCAA", bytes([20] * 9), FLAG_UNMAPPED | FLAG_READ1),
        record(b"pair/2", b"ACGTTGCAAC", bytes([20] * 10), FLAG_UNMAPPED | FLAG_READ2),
        record(b"both", b"ACGTTGCAACG", bytes([20] * 11), FLAG_UNMAPPED | FLAG_READ1 | FLAG_READ2),
        record(b"secondary", b"GATTACA" * 3, bytes([40] * 21), FLAG_SECONDARY),
        record(b"supplementary", b"GATTACA" * 3, bytes([40] * 21), FLAG_SUPPLEMENTARY | FLAG_READ2),
        record(b"trimfwd", b"ACGTGGTCAT" * 8, low_tail, cigar=(80 << 4,), aux=b"XTAU"),
        record(b"trimrev", b"ACGTGGTCAT" * 8, low_tail[::-1], FLAG_UNMAPPED | FLAG_REVERSE),
        record(b"highq", b"ACGT" * 10, bytes([92, 93, 94, 200] * 10)),
        record(b"polyA", b"A" * 40, bytes([30] * 40)),
        record(b"polyTrev", b"A" * 40, bytes([30] * 40), FLAG_UNMAPPED | FLAG_REVERSE | FLAG_READ1),
        record(b"n" * 254, b"NNNNNACGTNN", bytes([10] * 11)),
    ]


def texts():
    """(name, text, which, trim_qual) the serial core is run on, all valid: the text from the
    first record on (no header)."""
    fq = from_fastq(small_fastq())
    edge = edge_records()
    out = [("fastq", b"".join(fq), 7, 0), ("fastq_q15", b"".join(fq), 7, 15), ("edge", b"".join(edge), 7, 0),
           ("edge_q20", b"".join(edge), 7, 20), ("empty_text", b"", 7, 0)]
    out += [(f"edge_which{w}", b"".join(edge), w, 0) for w in range(1, 7)]
    return out
