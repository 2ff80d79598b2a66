"""Inputs and the host oracle of the FASTA loader's tests (test_gpu_fasta.py on the device,
test_fasta_cpu.py without one): hand-written edge records, tile-edge layouts, the seeded
random generator, and `rule`, the one-rule restatement of parse_fasta that the kernels
implement (include/hsa_gpu.h, hsa_fasta_device)."""
import numpy as np

from hsa_amd import index_build, index_io, synth

TILE = 4096                      # FA_TILE: input bytes per block
PAD = 8                          # zero words behind a text


def bases(n, seed=1):
    return bytes(b"ACGT"[int(c)] for c in synth.genome_codes(n, seed))


def edge_fasta():
    """Every record kind of the issue's list, in one file (no final newline)."""
    N = lambda k: b"N" * k
    recs = [b">r74\n" + bases(74, 2), b">r75\n" + bases(75, 3), b">r76 comment\n" + bases(76, 4)]
    for k in (9, 10, 11):
        recs += [b">start%d\n" % k + N(k) + bases(80, 10 + k), b">mid%d\n" % k + bases(40, 20 + k) + N(k) + bases(45, 30 + k),
                 b">end%d\n" % k + bases(80, 40 + k) + N(k)]
    recs += [b">two_long\n" + bases(30, 5) + N(12) + b"C" + N(15) + bases(50, 6),
             b">all_n\n" + N(80),
             b">header_only",
             b">lower\r\n" + bases(50, 7).lower() + b"\r\n" + bases(40, 8) + b"\r\n",
             b">tab\tcut here\n" + bases(90, 9),
             b">space cut here\n" + bases(91, 10),
             b">" + b"n" * 300 + b"\n" + bases(92, 11),
             b">blank\n\n\n" + bases(50, 12) + b"\n\n" + bases(50, 13) + b"\n\n",
             b">nine_over_lines\n" + bases(40, 14) + b"NNNN\nNNNNN\n" + bases(40, 15),
             b">ten_over_lines\n" + bases(40, 16) + b"NNNN\n\nNNNNNN\n" + bases(40, 17),
             b">gt_in_sequence\n" + bases(80, 18)[:40]]
    data = b"\n".join(recs)
    # a '>' in the middle of a sequence line starts a record named by the rest of the line
    return data + b">" + bases(20, 19) + b"\n" + bases(85, 20) + b"\n>last\n" + bases(77, 21).replace(b"A", b"R", 3)


def quirk_fastas():
    """The two inputs of test_index_build.test_text_lengths_and_quirks."""
    g = synth.genome_codes(1600, 3)
    one = b">r\n" + bytes(b"ACGT"[int(c)] for c in g) + b"\n"
    seq = bytes(b"ACGT"[int(c)] for c in g[:101]) + b"N" * 9 + b"AC" + b"N" * 13
    return [one, b">x y\n" + seq + b"\n>short\nACGT\n"]


def length_fastas():
    """total % 4 = 0..3 with T % 16 == 0 and != 0: (kept bases, trailing Ns that are cut)."""
    out = []
    for k, n in ((1600, 0), (1600, 13), (1600, 14), (1600, 15), (1601, 0), (1602, 12), (1603, 0), (1599, 10), (1612, 0), (90, 11)):
        out.append(b">a\n" + bases(k, k + n) + b"N" * n + b"\n")
    return out


def lines(seq, width):
    return b"\n".join(seq[i:i + width] for i in range(0, len(seq), width)) + b"\n"


def tile_fastas():
    """Layouts whose interesting bytes sit on the edges of the 4096-byte tiles (for an input
    that starts on a 16-byte boundary; the tests also shift it by 1..15 bytes)."""
    out = []
    # one record longer than three tiles, then many short records inside one tile
    big = b">long\n" + lines(bases(3 * TILE + 500, 31), 61)
    out.append(big + b"".join(b">s%d\n" % i + bases(70 + i % 12, 100 + i) + b"\n" for i in range(40)))

    def put(prefix_len, piece, tail_seed):
        """`piece` placed so that it starts at byte prefix_len of the input."""
        head = b">p\n"
        body = lines(bases(prefix_len, tail_seed), 70)
        body = body[:prefix_len - len(head) - 1] + b"\n"
        return head + body + piece + lines(bases(300, tail_seed + 1), 70)

    out.append(put(TILE - 1, b">edge\n" + bases(100, 41) + b"\n", 42))                  # '>' on a tile's last byte
    out.append(put(TILE - 10, b">header_over_the_edge of a tile\n" + bases(100, 43) + b"\n", 44))
    out.append(put(2 * TILE - 4, b"NNNNNNNNNN", 45))                                      # a 10-run over an edge
    out.append(put(TILE - 5, b"NNNNNNNNN", 46))                                           # a 9-run over an edge
    out.append(put(TILE - 3, b"NNN\n\nNNNNNNN", 47))                                      # ... with newlines inside
    # a run of Ns longer than a tile, and a record's short tail behind a tile edge
    out.append(b">n\n" + bases(100, 48) + b"N" * (TILE + 50) + bases(100, 49) + b"\n>t\n" + bases(74, 50) + b"\n")
    return out


def random_fasta(seed):
    """1 to 20 KB over ACGTNacgtnR, '\\n', space, '\\r', and '>' only in sequence lines or at a
    line start; every header ends in '\\n'; line lengths are random."""
    rng = np.random.default_rng(seed)
    size = int(rng.integers(1000, 20000))
    al = np.frombuffer(b"ACGTNacgtnR", np.uint8)
    w = np.array([20, 20, 20, 20, 6, 3, 3, 3, 3, 2, 1], float)
    if seed % 3 == 0:
        w[4] = 60                                           # N-rich: long runs and all-N records
    w /= w.sum()
    out = [b">first\tx\n"]
    n = len(out[0])
    while n < size:
        r = rng.random()
        if r < 0.04:
            piece = b">" + rng.choice(al, int(rng.integers(0, 12))).tobytes() + (b"", b" c", b"\tc d")[int(rng.integers(0, 3))] + b"\n"
        elif r < 0.05:
            piece = b">"                                    # in a sequence line: the rest of the line is a header
            piece += rng.choice(al, int(rng.integers(0, 5))).tobytes() + b"\n"
        elif r < 0.12:                                      # a run of 1 to 24 ambiguous bytes, at times over two lines
            k = int(rng.integers(1, 25))
            piece = rng.choice(np.frombuffer(b"NnR\r", np.uint8), k).tobytes()
            if rng.random() < 0.3:
                cut = int(rng.integers(0, k + 1))
                piece = piece[:cut] + b"\n" + piece[cut:]
        elif r < 0.13:                                      # an all-ambiguous record
            piece = b"\n>alln\n" + b"N" * int(rng.integers(60, 100)) + b"\n>next\n"
        else:
            k = int(rng.integers(0, 90)) if rng.random() < 0.9 else int(rng.integers(0, 6))
            piece = rng.choice(al, k, p=w).tobytes()
            if rng.random() < 0.05:
                piece += b" "
            piece += (b"\n", b"\r\n", b"\n\n", b"")[int(rng.choice(4, p=[0.7, 0.1, 0.1, 0.1]))]
        out.append(piece)
        n += len(piece)
    data = b"".join(out)
    if seed % 5 == 0 and refused_offset(data.rstrip(b"\n")) is None:
        data = data.rstrip(b"\n")                            # no final newline
    return data


def refused_offset(data):
    """The byte offset at which hsa_fasta_device refuses `data`, or None."""
    if not data.startswith(b">"):
        return 0
    hdr = False
    start = 0
    for i, c in enumerate(data):
        if c == 62:
            if hdr:
                return i
            hdr, start = True, i
        elif c == 10:
            hdr = False
    return start if hdr else None


def rule(data):
    """parse_fasta restated as the kernels compute it: per record, ambiguous bytes in runs of
    10 or more are dropped and the others become G; a block starts at every kept character
    whose predecessor in the record is missing or dropped; an all-ambiguous record has one
    empty block.  Returns (codes, record rows, block rows, total) in the device's layouts."""
    codes, rec, blk, total = [], [], [], 0
    for name_off, name_len, seq in _spans(data):
        L = len(seq)
        if L < 75:
            continue
        code = index_build._ACGT[seq]
        amb = code == 255
        drop = np.zeros(L, bool)
        j = 0
        while j < L:
            if amb[j]:
                e = j
                while e < L and amb[e]:
                    e += 1
                if e - j >= 10:
                    drop[j:e] = True
                j = e
            else:
                j += 1
        rec.append((name_off, name_len, L, len(blk)))
        if drop.all():
            blk.append([len(rec) - 1, len(codes), 0, L])
        for j in range(L):
            if not drop[j]:
                if j == 0 or drop[j - 1]:
                    blk.append([len(rec) - 1, len(codes), 0, j])
                codes.append(2 if amb[j] else int(code[j]))
        total += L
    for b in range(len(blk)):
        blk[b][2] = ((blk[b + 1][1] if b + 1 < len(blk) else len(codes)) - 1) & 0xFFFFFFFF
    return (np.array(codes, np.uint8), np.array(rec, np.uint32).reshape(-1, 4), np.array(blk, np.uint32).reshape(-1, 4), total)


def _spans(data):
    """(name offset, name length, sequence bytes) per record, as index_build._records cuts them."""
    pos = 1
    n = len(data)
    while pos < n:
        end = data.find(b">", pos)
        end = n if end < 0 else end
        nl = data.find(b"\n", pos, end)
        head = data[pos:nl if nl >= 0 else end]
        k = min([i for i in (head.find(b"\t"), head.find(b" ")) if i >= 0] + [len(head), 256])
        body = np.frombuffer(data[nl + 1:end] if nl >= 0 else b"", np.uint8)
        body = body[body != 10].copy()
        low = (body >= 97) & (body <= 122)
        body[low] -= 32
        yield pos, k, body
        pos = end + 1


def host(data):
    """Everything the device call must leave, from the host functions."""
    codes, ann, total = index_build.parse_fasta(data)
    pac = index_build.pac_bytes(codes, total)
    rpac = index_build.reverse_pac(pac)
    text, rtext = index_build.pac_text(pac), index_build.pac_text(rpac)
    words = lambda t: np.concatenate([index_io.pack_lsb_u32(t), np.zeros(PAD, np.uint32)])
    return dict(codes=codes, ann=ann, total=total, pac=np.frombuffer(pac, np.uint8), rpac=np.frombuffer(rpac, np.uint8),
                T=len(text), rT=len(rtext), text=words(text), rtext=words(rtext),
                ann_text=index_build.ann_text(ann, total), records=data.count(b">"))
