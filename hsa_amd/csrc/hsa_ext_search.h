// hsa_ext_search.h -- the splice path's seed extension, once, for k_extend
// (hsa_extend.hip) and k_splice (hsa_splice.hip).
//
// bwt_extend_backward / bwt_extend_foreward (bwtgap.c:640-663) put the seed's hit on a
// fresh stack and run bwt_backtracing_search (bwtgap.c:346-511): a best-first search
// over the bucketed LIFO of bwt_match_gap, extending the interval backward on the
// forward BWT or forward on the reverse BWT, pruned by the width bids of the read, with
// an exact tail (bwt_extend_exact, 2BWT-Interface.c:394-439) once no difference is left.
// It rewrites the hit (start or end, interval, counts, score, type) whenever it reaches
// further toward max_pos.
//
// Three pieces, all forceinlined into the kernel that instantiates them:
//   * ExtStack<Bk>: the stack -- a pool of 32-byte entries (two uint4, the link in
//     e1.z) linked per bucket, popped slots reused through a free list, the entry pushed
//     last kept in registers; Bk is the bookkeeping of the buckets' heads and counts
//     (ExtBuckets32: k_extend, ExtBuckets16: k_splice);
//   * ExtCall: what a call fixes (direction, length, the hit's start / end, max_diff,
//     mode) and what it moves (max_pos, ret);
//   * ext_step(x): one gap_pop and its expansion, over a context x the kernel supplies:
//       x.a                  fwd, rev, T, rT, C of the index (the kernel's arguments)
//       x.R                  the regime (scores, bounds)
//       x.stk, x.call        the two above
//       x.seq_at(p)          the read's code at p   } EXT_E_WIN into x.stk.err where the
//       x.bid_at(p)          the width bid at p     } kernel does not let the call read
//       x.bucket(score)      the bucket of a score inside the regime's n_stacks, or -1
//       x.hit(w)             word w of the hit being rewritten (bwt_aln1_t)
//     The kernel owns the loop around it (budgets, max_entries, saved state).
#pragma once
#include "hsa_device.h"
#include "hsa_internal.h"

// why a call could not be completed (ExtStack::err); each kernel maps them to its own codes
enum {
    EXT_E_CAP = 1,     // the stack's capacity exceeded
    EXT_E_SCORE = 2,   // an entry's score outside the stack's buckets (undefined in the reference)
    EXT_E_RANK = 3,    // a rank position past the text (undefined in the reference)
    EXT_E_WIN = 4      // a read position the call may not read
};

// 32-bit heads and counts at stride hs: lane-interleaved in LDS, or per lane in HBM
struct ExtBuckets32 {
    static constexpr uint32_t NIL = 0xFFFFFFFFu;
    uint32_t *H, *N;
    uint32_t hs;
    __device__ __forceinline__ void clear(int b) { N[(uint32_t)b * hs] = 0; }
    __device__ __forceinline__ uint32_t count(int b) const { return N[(uint32_t)b * hs]; }
    // slot becomes the bucket's head; returns the head before it (NIL: the bucket was empty)
    __device__ __forceinline__ uint32_t link(int b, uint32_t slot)
    {
        const uint32_t n = N[(uint32_t)b * hs], old = n ? H[(uint32_t)b * hs] : NIL;
        H[(uint32_t)b * hs] = slot;
        N[(uint32_t)b * hs] = n + 1u;
        return old;
    }
    // the head slot of a non-empty bucket; left: the bucket's count without it
    __device__ __forceinline__ uint32_t head(int b, uint32_t &left) const
    {
        left = N[(uint32_t)b * hs] - 1u;
        return H[(uint32_t)b * hs];
    }
    __device__ __forceinline__ void unlink(int b, uint32_t next, uint32_t left)
    {
        H[(uint32_t)b * hs] = next;
        N[(uint32_t)b * hs] = left;
    }
};

// one word per bucket, head | count << 16 (16-bit slot numbers), lane-interleaved in LDS
struct ExtBuckets16 {
    static constexpr uint32_t NIL = 0xFFFFu;
    uint32_t *hn;
    uint32_t hs;
    __device__ __forceinline__ void clear(int b) { hn[(uint32_t)b * hs] = 0; }
    __device__ __forceinline__ uint32_t count(int b) const { return hn[(uint32_t)b * hs] >> 16; }
    __device__ __forceinline__ uint32_t link(int b, uint32_t slot)
    {
        const uint32_t v = hn[(uint32_t)b * hs];
        hn[(uint32_t)b * hs] = slot | ((v >> 16) + 1u) << 16;
        return (v >> 16) ? (v & 0xFFFFu) : NIL;
    }
    __device__ __forceinline__ uint32_t head(int b, uint32_t &left) const
    {
        const uint32_t v = hn[(uint32_t)b * hs];
        left = (v >> 16) - 1u;
        return v & 0xFFFFu;
    }
    __device__ __forceinline__ void unlink(int b, uint32_t next, uint32_t left)
    {
        hn[(uint32_t)b * hs] = (next & 0xFFFFu) | left << 16;
    }
};

// gap_stack_t (bwtgap.c:46-92) of one lane.  The entry pushed last stays in registers
// ("pending") until the next push or pop: the next pop takes it whenever its bucket is
// <= the lowest non-empty one (it is the top of that bucket then, bwtgap.c:77-92), so a
// chain of expansions whose last child (the match, pushed last, bwtgap.c:493-502) is
// always the best never touches the pool.
template <class Bk> struct ExtStack {
    Bk bk;
    uint4 *P;                  // the pool: cap entries x 2 uint4
    uint32_t cap;
    int nb;                    // buckets
    int best, n_ent, pscore, err;
    bool pend;
    uint32_t top, freel;
    uint4 pe0, pe1;

    __device__ __forceinline__ void reset()
    {
        for (int b = 0; b < nb; ++b) bk.clear(b);
        best = nb; n_ent = 0; err = 0;
        pend = false;
        top = 0; freel = Bk::NIL;
    }
    __device__ __forceinline__ void flush()            // the pending entry into its bucket
    {
        pend = false;
        uint32_t slot;
        if (freel != Bk::NIL) { slot = freel; freel = P[(size_t)slot * 2 + 1].z; }
        else if (top < cap) slot = top++;
        else { err = EXT_E_CAP; return; }
        pe1.z = bk.link(pscore, slot);
        P[(size_t)slot * 2] = pe0;
        P[(size_t)slot * 2 + 1] = pe1;
        if (best > pscore) best = pscore;
    }
    __device__ __forceinline__ void push(int bucket, const uint4 e0, const uint4 e1)
    {
        if (pend) flush();
        pe0 = e0;
        pe1 = e1;
        pscore = bucket;
        pend = true;
        ++n_ent;
    }
    // gap_pop (bwtgap.c:77-92) of a non-empty stack; false: the pending entry found no slot
    __device__ __forceinline__ bool pop(uint4 &e0, uint4 &e1)
    {
        if (pend && pscore <= best) {
            e0 = pe0; e1 = pe1;
            pend = false;
            --n_ent;
            return true;
        }
        if (pend) { flush(); if (err) return false; }
        uint32_t left;
        const uint32_t slot = bk.head(best, left);
        e0 = P[(size_t)slot * 2]; e1 = P[(size_t)slot * 2 + 1];
        bk.unlink(best, e1.z, left);
        --n_ent;
        P[(size_t)slot * 2 + 1].z = freel;
        freel = slot;
        if (left == 0 && n_ent > 0) {
            int b = best + 1;
            while (b < nb && bk.count(b) == 0) ++b;
            best = b;
        } else if (left == 0) {
            best = nb;
        }
        return true;
    }
};

struct ExtCall {
    int dir, len;              // 1 backward (bwt_extend_backward), 0 foreward; aux->len
    int start, end;            // the call's hit as given: fixed (bwtgap.c:365)
    int max_diff, mode, best_score;
    int max_pos, ret;

    __device__ __forceinline__ void set(int dir_, int len_, int start_, int end_, int max_pos_, int max_diff_, int mode_,
                                        const hsa_regime_t &R)
    {
        dir = dir_; len = len_; start = start_; end = end_;
        max_diff = max_diff_; mode = mode_;
        best_score = (max_diff + 1) * R.s_mm + (R.max_gapo + 1) * R.s_gapo + (R.max_gape + 1) * R.s_gape;
        max_pos = max_pos_; ret = 0;
    }
};

__device__ __forceinline__ uint32_t ext_pk4(const uint32_t v[4], uint32_t c)
{
    return hsa_sel4<uint32_t>(c, v[0], v[1], v[2], v[3]);     // select tree (hsa_device.h)
}

// gap_push (bwtgap.c:46-75): info = score << 21 | i in 32 bits; last_diff_pos is never
// read by the extension
template <class X>
__device__ __forceinline__ void ext_push(X &x, int i, uint32_t k, uint32_t l, uint32_t rk, uint32_t rl, int mm, int go,
                                         int ge, int st)
{
    const int score = mm * x.R.s_mm + go * x.R.s_gapo + ge * x.R.s_gape;
    if (score < 0 || score >= x.R.n_stacks) { x.stk.err = EXT_E_SCORE; return; }
    const int bucket = x.bucket(score);
    if (bucket < 0) { x.stk.err = EXT_E_SCORE; return; }
    x.stk.push(bucket, make_uint4(k, l, rk, rl),
               make_uint4((uint32_t)score << 21 | (uint32_t)i,
                          (uint32_t)(mm & 255) | (uint32_t)(go & 255) << 8 | (uint32_t)(ge & 255) << 16 |
                              (uint32_t)(st & 3) << 24,
                          0u, 0u));
}

// the call's first entry: the hit itself (bwtgap.c:644 / :658)
template <class X> __device__ __forceinline__ void ext_push_hit(X &x)
{
    const uint32_t a0 = x.hit(0);
    ext_push(x, x.call.len, x.hit(1), x.hit(2), x.hit(3), x.hit(4), (int)(a0 & 0xFFFFu), (int)((a0 >> 16) & 0xFFu),
             (int)(a0 >> 24), ST_M);
}

// hsa_step_all behind the check that its rank positions are inside the text
template <class X>
__device__ __forceinline__ void ext_step_all(X &x, int backward, uint32_t k, uint32_t l, uint32_t rk, uint32_t rl,
                                             uint32_t ok[4], uint32_t ol[4], uint32_t ork[4], uint32_t orl[4])
{
    const uint32_t p1 = backward ? k : rk, p2 = (backward ? l : rl) + 1u, lim = (backward ? x.a.T : x.a.rT) + 1u;
    if (p1 > lim || p2 > lim || p2 == 0u) { x.stk.err = EXT_E_RANK; return; }
    hsa_step_all(backward ? x.a.fwd : x.a.rev, x.a.C, backward, k, l, rk, rl, ok, ol, ork, orl);
}

// One gap_pop and its expansion (bwtgap.c:371-504) of a non-empty stack without an
// error.  Returns whether the search goes on: false once it reached max_pos (call.ret =
// 1), passed the score bound, or met an error (stk.err).
template <class X> __device__ __forceinline__ bool ext_step(X &x)
{
    const hsa_regime_t &R = x.R;
    ExtCall &cl = x.call;
    int &err = x.stk.err;
    uint4 e0, e1;
    if (!x.stk.pop(e0, e1)) return false;
    uint32_t k = e0.x, l = e0.y, rk = e0.z, rl = e0.w;
    const uint32_t info = e1.x;
    const int e_mm = (int)(e1.y & 255u), e_go = (int)((e1.y >> 8) & 255u), e_ge = (int)((e1.y >> 16) & 255u);
    const int e_st = (int)((e1.y >> 24) & 3u);
    int i = (int)(info & 0xffffu);
    if (!(cl.mode & MODE_NONSTOP) && (int)(info >> 21) > cl.best_score + R.s_mm) return false;
    int m = cl.max_diff - (e_mm + e_go);
    if (cl.mode & MODE_GAPE) m -= e_ge;
    const int len = cl.len, bw = cl.dir, start = cl.start, end = cl.end;
    if (m <= 0 || i == 0) {
        if (m == 0 && i != 0) {
            // bwt_extend_exact (2BWT-Interface.c:394-439)
            uint32_t xk = k, xl = l, xrk = rk, xrl = rl;
            if (bw == 1) {
                const int s0 = start - len - 1;
                while (i != 0 && !err) {
                    const uint32_t c = x.seq_at(s0 + i);
                    if (c > 3) break;
                    uint32_t ok[4], ol[4], ork[4], orl[4];
                    ext_step_all(x, 1, xk, xl, xrk, xrl, ok, ol, ork, orl);
                    xk = ext_pk4(ok, c); xl = ext_pk4(ol, c); xrk = ext_pk4(ork, c); xrl = ext_pk4(orl, c);
                    if (xk > xl) break;
                    k = xk; l = xl; rk = xrk; rl = xrl;
                    --i;
                }
            } else {
                const int rp = end + len - i + 1;          // start + leav - leav: fixed (:424)
                while (!err) {
                    const uint32_t c = x.seq_at(rp);
                    if (c > 3) break;
                    uint32_t ok[4], ol[4], ork[4], orl[4];
                    ext_step_all(x, 0, xk, xl, xrk, xrl, ok, ol, ork, orl);
                    xk = ext_pk4(ok, c); xl = ext_pk4(ol, c); xrk = ext_pk4(ork, c); xrl = ext_pk4(orl, c);
                    if (xk > xl) break;
                    k = xk; l = xl; rk = xrk; rl = xrl;
                }
            }
            if (err) return false;
        }
        if (bw == 1 && cl.max_pos >= start + i - len && (int)x.hit(6) > start + i - len) {
            x.hit(6) = (uint32_t)(start + i - len);
            cl.max_pos = start + i - len;
        } else if (bw == 0 && cl.max_pos <= end + len - i && (int)x.hit(7) < end + len - i) {
            x.hit(7) = (uint32_t)(end + len - i);
            cl.max_pos = end + len - i;
        } else {
            return true;
        }
        x.hit(1) = k; x.hit(2) = l; x.hit(3) = rk; x.hit(4) = rl;
        x.hit(5) = (x.hit(5) & 0xC0000000u) | 4u;                  // BWA_TYPE_SPLICING, strand kept
        x.hit(0) = (uint32_t)e_mm | (uint32_t)e_go << 16 | (uint32_t)e_ge << 24;
        x.hit(8) = info >> 21;
        if (i == 0) { cl.ret = 1; return false; }
        return true;
    }
    --i;
    const int real_pos = bw == 1 ? start - len + i : len + end - i;
    uint32_t ok[4], ol[4], ork[4], orl[4];
    ext_step_all(x, bw, k, l, rk, rl, ok, ol, ork, orl);
    if (err) return false;
    const uint32_t occ = l - k + 1u;
    const int max_pos = cl.max_pos;
    int allow_diff = 1;
    if (bw == 1 && max_pos < real_pos) {
        const int d = x.bid_at(real_pos) - x.bid_at(max_pos);
        if (d > m || (d == m && x.bid_at(max_pos) != x.bid_at(max_pos + 1))) allow_diff = 0;
    }
    if (bw == 0 && max_pos > real_pos) {
        const int d = x.bid_at(real_pos) - x.bid_at(max_pos);
        if (d > m || (d == m && x.bid_at(max_pos) != x.bid_at(max_pos - 1))) allow_diff = 0;
    }
    const int tmp = (cl.mode & MODE_LOGGAP) ? hsa_log2((uint32_t)(e_ge + e_go)) / 2 + 1 : e_go + e_ge;
    if (allow_diff && i >= R.indel_end_skip + tmp && len - i >= R.indel_end_skip + tmp) {
        if (e_st == ST_M) {
            if (e_go < R.max_gapo) {
                ext_push(x, i, k, l, rk, rl, e_mm, e_go + 1, e_ge, ST_I);
                for (int j = 0; j != 4; ++j)
                    if ((bw == 1 && ok[j] <= ol[j]) || (bw == 0 && ork[j] <= orl[j]))
                        ext_push(x, i + 1, ok[j], ol[j], ork[j], orl[j], e_mm, e_go + 1, e_ge, ST_D);
            }
        } else if (e_st == ST_I) {
            if (e_ge < R.max_gape) ext_push(x, i, k, l, rk, rl, e_mm, e_go, e_ge + 1, ST_I);
        } else if (e_st == ST_D) {
            if (e_ge < R.max_gape && (e_ge + e_go < cl.max_diff || occ < (uint32_t)R.max_del_occ))
                for (int j = 0; j != 4; ++j)
                    if (ok[j] <= ol[j]) ext_push(x, i + 1, ok[j], ol[j], ork[j], orl[j], e_mm, e_go, e_ge + 1, ST_D);
        }
    }
    if (allow_diff == 1) {
        const uint32_t sc = x.seq_at(real_pos);
        for (int j = 1; j <= 4; ++j) {
            const uint32_t c = (sc + (uint32_t)j) & 3u;
            const int is_mm = (j != 4 || sc > 3) ? 1 : 0;
            if ((bw == 1 && ext_pk4(ok, c) <= ext_pk4(ol, c)) || (bw == 0 && ext_pk4(ork, c) <= ext_pk4(orl, c)))
                ext_push(x, i, ext_pk4(ok, c), ext_pk4(ol, c), ext_pk4(ork, c), ext_pk4(orl, c), e_mm + is_mm, e_go, e_ge,
                         ST_M);
        }
    }
    return !err;
}
