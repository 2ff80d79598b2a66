"""bwt_aln2seq_core(p, 1, n_multi), the multi-row filter of bwa_cal_pac_pos and
bwa_approx_mapQ (bwtse.c:21-131, :360-366) restated in plain Python over hsa_aln64_t
arrays, with glibc's drand48: the sequential walk hsa_choose_hits_device64 must equal."""
import math

import numpy as np

A = 0x5DEECE66D
C = 0xB
MASK = (1 << 48) - 1
SEED0 = 0                       # glibc's state in a process that never seeds (not SVID's 0x1234ABCD330E)
ALN64_WORDS = 14


def step(x):
    return (A * x + C) & MASK


def real(x):
    """drand48's double of state x: x * 2^-48, exact."""
    return float(x) * 2.0 ** -48


def jump(x, d):
    """x after d draws, by squaring the affine map."""
    a, c = A, C
    while d:
        if d & 1:
            x = (a * x + c) & MASK
        c = (c * (a + 1)) & MASK
        a = (a * a) & MASK
        d >>= 1
    return x


def zero_predecessor():
    """The state whose successor is 0: -0xB * A^-1 mod 2^48."""
    x = (-C * pow(A, -1, 1 << 48)) & MASK
    assert step(x) == 0
    return x


def log_n_table():
    return np.array([0] + [int(4.343 * math.log(i) + 0.5) for i in range(1, 256)], np.int32)


def make_hits(reads):
    """Device-layout arrays of fabricated hit lists.  reads: per read None (n_aln 0), -1
    (n_aln -1) or a list of records (score, k, width, n_mm, gap, strand)."""
    n_aln = np.zeros(len(reads), np.int32)
    hit_off = np.zeros(len(reads), np.uint64)
    recs = []
    for j, r in enumerate(reads):
        hit_off[j] = len(recs)
        if r is None or r == -1:
            n_aln[j] = 0 if r is None else -1
            continue
        n_aln[j] = len(r)
        for score, k, w, n_mm, gap, strand in r:
            go = 1 if gap else 0
            l = k + w - 1
            rec = np.zeros(ALN64_WORDS, np.uint32)
            rec[0] = n_mm | (go << 16) | ((gap - go) << 24)
            rec[1] = strand << 30
            rec[2], rec[3], rec[4], rec[5] = k & 0xFFFFFFFF, k >> 32, l & 0xFFFFFFFF, l >> 32
            rec[12] = score
            recs.append(rec)
    hits = np.array(recs, np.uint32).reshape(-1, ALN64_WORDS) if recs else np.zeros((1, ALN64_WORDS), np.uint32)
    return n_aln, hit_off, hits


def rec_kw(rec):
    k = int(rec[2]) | (int(rec[3]) << 32)
    l = int(rec[4]) | (int(rec[5]) << 32)
    return k, (l - k + 1 if l >= k else 0)


def mapq(c1, c2, n_mm, max_diff, log_n):
    if c1 == 0:
        return 23
    if c1 > 1:
        return 0
    if n_mm == max_diff:
        return 25
    if c2 == 0:
        return 37
    g = int(log_n[255 if c2 >= 255 else c2])
    return 0 if 23 < g else 23 - g


def choose(n_aln, hit_off, hits, max_diff, n_multi, state):
    """The sequential walk.  Returns sel (n, 4) u32, sel64 (n, 4) u64, the final state,
    pos_off (n + 1), the rows as (SA row, record index) in order, and the counts (reads
    with a hit, repeat reads, reads with two or more equal-best records or a rowless
    single one, reads with one equal-best record that drew once)."""
    n = len(n_aln)
    log_n = log_n_table()
    sel = np.zeros((n, 4), np.uint32)
    sel64 = np.zeros((n, 4), np.uint64)
    pos_off = np.zeros(n + 1, np.uint64)
    rows = []
    n_hit = n_rep = n_var = 0
    zero = []
    x = state
    for j in range(n):
        sel64[j, 3] = x
        na = int(n_aln[j])
        if na <= 0:
            pos_off[j + 1] = len(rows)
            continue
        recs = hits[int(hit_off[j]):int(hit_off[j]) + na]
        best = int(np.int32(recs[0][12]))
        cnt = i = 0
        idx = sa = n_mm = draws = 0
        taken = False
        while i < na and int(np.int32(recs[i][12])) <= best:                 # bwtse.c:40-55
            k, w = rec_kw(recs[i])
            x = step(x)
            draws += 1
            if real(x) * float(w + cnt) > float(cnt):
                x = step(x)
                draws += 1
                idx, n_mm, taken = i, int(recs[i][0]) & 0xFFFF, True
                sa = k + int(float(w) * real(x))
            cnt += w
            i += 1
        nb, c1 = i, cnt
        w0 = rec_kw(recs[0])[1]
        if nb >= 2 or w0 == 0:
            n_var += 1
        elif draws != 2:
            zero.append(j)
        widths = [rec_kw(r) for r in recs]
        n_occ = sum(w for _, w in widths)
        c2 = n_occ - c1
        typ = 2 if c1 > 1 else 1
        n_hit += 1
        n_rep += typ == 2
        mine = [(sa, idx)]
        if 0 < n_occ <= n_multi + 1:           # bwtse.c:62-112 without its unreachable sample, then :360-366
            every = [(k + o, r) for r, (k, w) in enumerate(widths) for o in range(w)]
            skip = every.index((sa, idx)) if taken else 0
            mine += every[:skip] + every[skip + 1:]
        rows += mine
        sel[j] = (typ, idx, mapq(c1, c2, n_mm, int(max_diff[j]), log_n), len(mine) - 1)
        sel64[j, :3] = (sa, c1, c2)
        pos_off[j + 1] = len(rows)
    return dict(sel=sel, sel64=sel64, rng=x, pos_off=pos_off, rows=rows, n_hit=n_hit, n_rep=n_rep, n_var=n_var, zero=zero)
