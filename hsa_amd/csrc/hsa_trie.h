#pragma once
// hsa_trie.h -- the root width trie: every string of up to D characters (D = the index's
// trie depth, HSA_TRIE_DEPTH, default 12) with the SA interval the rank steps would
// compute for it, so that a search path's first D steps are answered by one cached
// load each instead of a rank pair on two random 64-byte sectors of the multi-GB rank
// table.
//
// Why: every read's search starts at the root (the whole SA range) and every step of
// bwt_match_gap / bwt_match_exact / bwt_cal_width near the root works on a wide
// interval, whose two rank queries (k - 1, l) fall in different blocks.  In config 2
// 45 % of k_widths' steps extend a string of <= 11 characters since the chain's last
// reset (tools/exp/depth_hist.py).  All those
// strings together are a few tens of MB -- resident in the Infinity Cache -- where the
// rank table is 5.6 GB of uniformly random sectors.
//
// The intervals are the kernel's own arithmetic applied level by level (the builder
// below calls the same occ_pair and the same formulas as k_widths' step), so a trie
// answer is bit-identical to the rank steps it replaces.
// The rank-query count stays the reference's: a step answered from a trie still
// counts its two queries (d_counters[2]); d_counters[10] counts the trie loads.
//
// The width trie (k_widths): c APPENDED (forward extension on the reverse BWT,
// BWTSARangeForeward, 2BWT-Interface.c:121-131): entry {k, l}; node p's children at
// 4 p + c on the next level.  Level d (1..D) holds 4^d entries from entry (4^d - 4) / 3.
//
// The implicit root levels (k_search, ungapped): c PREPENDED (the bidirectional backward
// step on the forward BWT, 2BWT-Interface.c:235-272); node p's children at 4 p + c.  A
// search trie that answered each shallow step with a table load was built and measured
// slower than the rank steps it replaced ("Measured and removed"): the wave
// still waited for one load per step.  Here the shallow steps take NO load.  On a level
// of which every string occurs in the text (a COMPLETE level: all of a node's four
// children exist) an ungapped search reads nothing of an entry's interval until it
// leaves the level -- pruning works on the width rows and the entry's meta word -- so
// k_search carries the node number instead, up to level Dc, the deepest complete level
// (at most HSA_SDEPTH, HSA_SDEPTH_MAX), and one level is kept as a table: {k, l, rev_k}
// per node, the four children of one node of the level above in one 64-byte sector,
// words [0,4) their k, [4,8) their l, [8,12) their rev_k.  The levels are the kernel's
// own step arithmetic applied to the previous level, so the values are bit-identical
// to the rank steps'.
//
// The table level is Dc + 1 (16 B x 4^(Dc+1), at most level HSA_STAB_MAX), the first
// level that need not be complete.  Completeness is needed only of the levels whose
// entries are node numbers without an interval; the table stores every node's interval,
// and a string that does not occur has there the empty interval (k = l + 1) the rank
// step itself computes for it, so the kernel tests k <= l of a table child as it does
// of a rank step's.  A step from level Dc - 1 to Dc then takes no load, and a step from
// Dc to Dc + 1 one table sector in place of two rank blocks.  The level is dropped (the
// table stays on level Dc) when a string of it that occurs has an unusable interval,
// when 4^(Dc+1) > T, when it does not fit in device memory, or with HSA_SPARTIAL=0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hsa_device.h"

#define HSA_TRIE_MAX_DEPTH 15u      // node numbers of a level stay below 2^32 (uint32_t)
#define HSA_TRIE_DEFAULT_DEPTH 12u

__host__ __device__ __forceinline__ uint64_t trie_base(uint32_t d) { return ((1ull << (2u * d)) - 4ull) / 3ull; }
template <typename IT> struct TrieC { IT v[4]; };   // the forward C table, by value

// width-trie entry: {k, l} of the reverse BWT
template <typename IT>
__device__ __forceinline__ void trie_w_load(const void *t, uint64_t e, IT &k, IT &l)
{
    if constexpr (sizeof(IT) == 4) {
        const uint2 v = reinterpret_cast<const uint2 *>(t)[e];
        k = v.x; l = v.y;
    } else {
        const uint4 v = reinterpret_cast<const uint4 *>(t)[e];
        k = (uint64_t)v.x | (uint64_t)v.y << 32;
        l = (uint64_t)v.z | (uint64_t)v.w << 32;
    }
}

template <typename IT>
__device__ __forceinline__ void trie_w_store(void *t, uint64_t e, IT k, IT l)
{
    if constexpr (sizeof(IT) == 4) reinterpret_cast<uint2 *>(t)[e] = make_uint2(k, l);
    else reinterpret_cast<uint4 *>(t)[e] = make_uint4((uint32_t)k, (uint32_t)(k >> 32), (uint32_t)l, (uint32_t)(l >> 32));
}

// An interval past the text (l > T) can only come from an index whose two BWTs are not
// each other's reverse (test fixtures built from unrelated texts): the builder then
// raises *bad, stores the string as absent (so no deeper level reads past the rank
// blocks), and the index keeps no trie.
// Level d -> level d + 1 of the width trie: the forward extension of k_widths' step
// (reverse BWT, forward C table; bwtaln.c:84-97).
template <typename IT, typename RD>
__global__ void __launch_bounds__(256) k_trie_width_level(RD rev, IT T, TrieC<IT> Cg, uint32_t d,
                                                          void *__restrict__ tw, unsigned *bad)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (1ull << (2u * d))) return;
    IT k = 0, l = T;
    if (d > 0) trie_w_load<IT>(tw, trie_base(d) + p, k, l);
    const uint64_t ch = trie_base(d + 1) + 4 * p;
    if (k > l) {
        for (uint32_t c = 0; c < 4; ++c) trie_w_store<IT>(tw, ch + c, (IT)1, (IT)0);
    } else {
        IT oa[4], ob[4];
        occ_pair(rev, k, l + (IT)1, oa, ob);
        for (uint32_t c = 0; c < 4; ++c) {
            IT kc = Cg.v[c] + oa[c] + (IT)1, lc = Cg.v[c] + ob[c];
            if (kc <= lc && lc > T) { *bad = 1u; kc = 1; lc = 0; }
            trie_w_store<IT>(tw, ch + c, kc, lc);
        }
    }
}

// ---------------------------------------------------------------- implicit root levels
#define HSA_SDEPTH_MAX 13u          // 16 B x 4^13 = 1 GiB
#define HSA_SDEPTH_DEFAULT 13u
#define HSA_STAB_MAX 14u            // the table's level: 16 B x 4^14 = 4 GiB

// the table sector of node p of the level above the table's: its four children's k, l, rev_k
__device__ __forceinline__ void trie_s_load4(const void *t, uint32_t p, uint32_t k[4], uint32_t l[4], uint32_t rk[4])
{
    const uint4 *s = reinterpret_cast<const uint4 *>(t) + (size_t)p * 4;
    const uint4 vk = s[0], vl = s[1], vr = s[2];
    k[0] = vk.x; k[1] = vk.y; k[2] = vk.z; k[3] = vk.w;
    l[0] = vl.x; l[1] = vl.y; l[2] = vl.z; l[3] = vl.w;
    rk[0] = vr.x; rk[1] = vr.y; rk[2] = vr.z; rk[3] = vr.w;
}

// one node n of the table's level (child n & 3 of node n >> 2)
__device__ __forceinline__ void trie_s_load1(const void *t, uint32_t n, uint32_t &k, uint32_t &l, uint32_t &rk)
{
    const uint32_t *s = reinterpret_cast<const uint32_t *>(t) + (size_t)(n >> 2) * 16 + (n & 3u);
    k = s[0]; l = s[4]; rk = s[8];
}

// Level d (src; the root when d == 0) -> level d + 1 (dst, 4^d sectors): k_search's
// expansion arithmetic (2BWT-Interface.c:235-272) on the forward BWT.  Two defects of
// level d + 1 are reported apart.  flags[0] is raised when the level is INVALID: a child
// that occurs has a zero k or rev_k (k_search's exact tail relies on both being non-zero
// below the root) or an interval past the text.  flags[1] counts the ABSENT children
// (k > l; a per-block sum, one atomic per block); they are stored with the values the
// arithmetic gives them, as every other child.  The caller launches it only on a complete
// level d, so every rank position is inside the text.
static __global__ void __launch_bounds__(256) k_trie_search_level(RankDir fwd, uint32_t T, TrieC<uint32_t> Cg, uint32_t d,
                                                                  const void *__restrict__ src, void *__restrict__ dst,
                                                                  unsigned *flags)
{
    __shared__ unsigned s_absent;
    if (threadIdx.x == 0) s_absent = 0u;
    __syncthreads();
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < (1ull << (2u * d))) {
        uint32_t k = 0, l = T, rk = 0;
        if (d > 0) trie_s_load1(src, (uint32_t)p, k, l, rk);
        uint32_t oa[4], ob[4], sr[4];
        occ_pair(fwd, k, l + 1u, oa, ob);
        const uint32_t erl = rk + (l - k);
        uint32_t oc = 0, na = 0;
        bool ok = true;
        for (int c = 3; c >= 0; --c) {
            const uint32_t n = ob[c] - oa[c];
            oa[c] = Cg.v[c] + oa[c] + 1u;
            ob[c] = Cg.v[c] + ob[c];
            sr[c] = (erl - oc) - (ob[c] - oa[c]);
            oc += n;
            if (oa[c] > ob[c]) ++na;
            else ok = ok && oa[c] >= 1u && ob[c] <= T && sr[c] >= 1u;
        }
        uint4 *s = reinterpret_cast<uint4 *>(dst) + p * 4;
        s[0] = make_uint4(oa[0], oa[1], oa[2], oa[3]);
        s[1] = make_uint4(ob[0], ob[1], ob[2], ob[3]);
        s[2] = make_uint4(sr[0], sr[1], sr[2], sr[3]);
        s[3] = make_uint4(0u, 0u, 0u, 0u);
        if (!ok) flags[0] = 1u;
        if (na) atomicAdd(&s_absent, na);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_absent) atomicAdd(&flags[1], s_absent);
}
