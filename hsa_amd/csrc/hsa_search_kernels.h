#pragma once
// hsa_search_kernels.h -- the bwa_cal_sa_reg_gap per-read loop as two persistent kernels
// (templated on the interval type: 32-bit, the reference's bwtint_t, and 64-bit for
// texts of 2^32 characters or more).  The host side that plans and launches them is
// hsa_search_launch.h, which hsa_search.hip (32-bit API) and hsa_search64.hip (64-bit
// API) include.
//
// k_widths: bwt_cal_width (bwtaln.c:73-98) for every (read, strand) of the batch --
//   the seed width and the whole-read width of the rc and the fwd strand, one work
//   item per lane, pulled from a global queue.  All lanes run the same short step
//   (one single-character rank pair on the reverse BWT), so the waves stay
//   converged.  Output: per (read, strand) a row of pruning bytes
//   min(bid,127) | (w[p] == w[p+1]) << 7 for the read and for the seed, and the
//   full w values (only gap_shadow reads them).
// k_search: per read, rc strand then fwd strand (bwtaln.c:343-359): copy the
//   strand's pruning bytes into LDS and run bwt_match_gap (bwtgap.c:118-331); the
//   first strand with hits wins; no hit on either -> HSA_F_FALLBACK (splice).
//
// One lane owns one read at a time (reads are pulled from a global queue with a
// wave-aggregated atomic, so a lane that finishes a cheap read immediately takes
// the next one: work-stealing at read granularity).  Every loop iteration of
// k_search performs at most ONE bidirectional rank step per lane (two Occ queries
// on the forward BWT, usually one 64-byte block), whatever the lane is doing --
// exact tail (bwt_match_exact) or expansion -- so all lanes issue their HBM loads
// together and the state machine in between is register/LDS work.  Control that
// needs no rank (pruned pops, hits) loops without touching the BWT.
//
// Per-lane state in LDS (160 KiB per CU): the pruning bytes of the current strand
// (everything bwt_match_gap's pruning reads: bwtgap.c:170, :256-263) and the
// stack's bucket heads.  Buckets are the REACHABLE scores only (a score table per
// regime maps aln_score -> dense bucket, order preserved), so `-n 4 -o 0` needs 6
// heads instead of the reference's 54 (bwtgap.c:18).  Stack entries (16 bytes and a
// 16-bit link: inside the entry where it has room, pool_link_in_entry, else in a link
// array) live in a per-lane pool in HBM; a bit mask in registers gives the
// lowest non-empty bucket (== gap_stack_t.best).  The child pushed LAST by an
// expansion is always the next pop when its bucket is the lowest, so it stays in
// registers ("virtual top").  A regime set without gap opens (max_gapo == 0: every
// entry stays in state M) runs a specialisation without the indel code.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "hsa_device.h"
#include "hsa_internal.h"
#include "hsa_trie.h"

#define NIL16 0xFFFFu
#define BLOCK 256
#define MAXB 128          // dense buckets per regime (BMask<2>)
#define MAXS 512          // score table length per regime (n_stacks <= MAXS)

enum : uint32_t { PH_IDLE = 0, PH_POP, PH_EXACT, PH_EXPAND, PH_EXIT, PH_END, PH_WAIT };

struct SearchArgs {
    RankDir fwd, rev;
    uint32_t T;
    uint32_t C[5];
    // 64-bit texts (IT = uint64_t kernels): the same, with superblock tables
    RankDir64 fwd64, rev64;
    uint64_t T64;
    uint64_t C64[5];
    const hsa_regime_t *regimes;
    const uint8_t *bmap;           // [2][MAXS]: aln_score -> dense bucket (0xFF: unreachable)
    uint32_t ntab;                 // score table entries per regime kept in LDS (>= every n_stacks, multiple of 8)
    const hsa_job_t *jobs;
    const int32_t *job_list;       // optional indirection (re-runs); null = identity
    int n_jobs;
    const uint8_t *codes;
    int32_t *n_aln;
    uint32_t *flags;
    uint64_t *hit_off;
    uint32_t *hits;
    uint64_t hit_cap;
    unsigned long long *ctr;       // the search's 16 counters (the CTR_* slots, hsa_internal.h)
    const uint8_t *wb, *ws;        // width rows of k_widths (row = list position * 2 + strand),
    uint32_t *wg;                  //   64 rows interleaved; wg: full w values (gap_shadow only)
    uint32_t rb, rs, rg;           //   row capacities: bytes, bytes, words
    uint4 *pool;
    void *nxt;                     // pool links: uint16_t, or uint32_t in the huge pass (unused where the entries hold them)
    uint32_t *hbuf;
    uint32_t pcap, hcap, nb;
    uint32_t off_heads, off_wb, off_ws;   // LDS byte offsets
    uint32_t lds_wb, lds_ws;              // LDS words per lane of the read / seed row (every format)
    uint32_t mm_buckets;           // 1: the bucket of every score is its n_mm (no gap opens, s_mm > 0)
    // device-side overflow re-run: the main pass appends reads that exceeded their
    // lane's capacity to ovf_list (count in ctr[ovf_ctr]); the re-run pass takes its read
    // count from n_dev and its queue head from ctr[qctr]
    int32_t *ovf_list;
    const unsigned long long *n_dev;
    uint32_t qctr;
    uint32_t ovf_ctr;              // counter that numbers this pass's ovf_list entries
    // caller-width mode (hsa_match_gap_batch, bwt_match_gap called directly): per job
    // strand and width_seed kind; k_widths_import builds the rows from the caller's
    // bwt_width_t pairs (cw), the search takes that one strand, and gap_shadow keeps
    // the full bid values (wbid) so the mutated widths can be handed back
    const hsa_mg_job_t *mg;
    int32_t *cw;
    int32_t *wbid;
    uint32_t *wq;                  // k_widths: rank queries of each forward-strand width row
    uint32_t batch_k;              // rare-event batching: at most this many lanes wait (see (A) in k_search)
    uint32_t batch_idle;           //   ... or run once the waiting lanes have idled this many lane-iterations
    // strand-split mode (small batches): work item p searches ONE strand of list position
    // p >> 1 (p even: rc, odd: fwd) on its own lane, so a read's two searches run side by
    // side instead of one after the other; k_split_finalize keeps the fwd strand only
    // when rc has no hit (bwtaln.c:343-359) and counts its work only then
    uint32_t split;
    int32_t *sp_n;                 // per item: hits, or -1 for a capacity overflow
    uint64_t *sp_off;
    uint32_t *sp_q, *sp_p;         //   its rank queries and pops (counted by the finalize)
    // the root width trie (hsa_trie.h) of the index, ktd levels (0: none, or not of this
    // instantiation's interval width): k_widths answers the steps of strings up to ktd
    // characters from ktw
    const void *ktw;
    uint32_t ktd;
    // cost order (main pass of a batch larger than the chip): k_widths writes each row's
    // final bid (wkey), k_order_* sort the list positions by it, most differences first,
    // and k_search takes its reads in that order (perm), so the costly searches do not
    // start last and set the launch's tail
    uint8_t *wkey;
    const int32_t *perm;
    uint32_t okey;                  // cost key with the tail length (default; HSA_ORDER_KEY=0: bid only)
    // lazy forward rows (k_widths_lazy): a read whose rc search found nothing and whose
    // forward row was not computed goes to fwd_list (count *fwd_n); the forward pass
    // (fwd_only) searches just that strand
    int32_t *fwd_list;
    unsigned long long *fwd_n;
    uint32_t fwd_only;
    // lazy main pass: rows in two planes, the rc row of list position q at row q and its
    // forward row (when computed) at row rmap[q], so every width lane stores coalesced;
    // null: row q * 2 + strand
    int32_t *rmap;
    // strand-split tails (helpers, k_search): a strand search with no hit yet that has run
    // fr_budget pops while more lanes wait for work than the shared frontier holds offers
    // its live entries there; waiting lanes search them (each entry a sub-search rooted at
    // it) and report only whether the item has a hit.  The owner keeps searching in the
    // reference's order; when every sub-search of its frontier ended without a hit it stops
    // with no hits, which is its own search's answer: before a hit, a strand search expands
    // the same entries in any order ("Helpers").  fr_budget 0: off.
    uint32_t fr_budget, fr_demand, fr_cap;
    uint32_t *fr_ent;              // published chunks: FR_CH entries of FR_EW words each
    uint32_t *fr_tag;              // per chunk: entries << 26 | (item + 1)
    uint32_t *fr_rq;               // ready queue: chunk + 1 once the chunk is complete (0 before)
    uint32_t *fr_st;               // per item: chunks not yet searched | FR_DONE | FR_HIT
    unsigned long long *fr_q, *fr_p;   // per item: its sub-searches' rank queries and pops
    unsigned long long *fr_c;      // [0] chunks reserved [1] ready-queue head (taken) [2] items finished
                                   // [3] lanes waiting [4] offers [5] offers refused (capacity) [6] sub-
                                   // searches ended [7] owners answered by their helpers [8] sub-searches'
                                   // rank queries [9] ready-queue tail
    // the implicit root levels (hsa_trie.h; ungapped 32-bit kernels with 8/16-bit rows, not
    // the HUGE pass): level sdc of the index's prepend trie, the table's level, one 64-byte
    // sector per level-(sdc - 1) node; every level above it is complete, level sdc itself
    // may hold strings that do not occur (k > l); sdc 0: none.  (Last in the struct: the
    // gapped kernels' argument offsets stay what they were.)
    const void *stw;
    uint32_t sdc;
};
#define FR_HIT 0x80000000u
#define FR_DONE 0x40000000u
#define FR_EW 8u                   // words per published entry (32- and 64-bit intervals)
#define FR_CH 16u                  // entries per chunk: one sub-search searches a chunk's sub-trees
#define FR_WALK 1024u              // largest stack a strand offers (the walk is a chain of dependent loads)
#ifndef HSA_HELPERS
#define HSA_HELPERS 1              // A/B builds: -DHSA_HELPERS=0 compiles the helpers out of k_search
#endif

// The kernel's arguments re-read from the kernarg segment where a rare path uses them
// (strand start and end, next read, hit staging): the asm barrier keeps the compiler
// from hoisting those loads out of the search loop, where holding every argument in
// SGPRs across the loop forced SGPR spills (v_writelane / v_readlane round trips).
typedef const __attribute__((address_space(4))) SearchArgs *ColdArgs;
__device__ __forceinline__ ColdArgs cold_args()
{
    ColdArgs p = (ColdArgs)(__builtin_amdgcn_kernarg_segment_ptr());
    asm volatile("" : "+s"(p));
    return p;
}

// entry meta word: i:10 | state:2 | is_diff:1 | n_mm:7 | n_gapo:4 | n_gape:8
constexpr __host__ __device__ __forceinline__ uint32_t meta_pack(uint32_t i, uint32_t st, uint32_t isd, uint32_t mm,
                                                                 uint32_t go, uint32_t ge)
{
    return i | st << 10 | isd << 12 | mm << 13 | go << 20 | ge << 24;
}
// The pool form of an ungapped entry's meta word when its bucket-list link travels with
// it (k_search's LK, 32-bit intervals): i:10 | is_diff:1 | n_mm:5 | link:16.  State is
// ST_M and both gap counts are 0 there, and n_mm <= 15 (8- and 4-bit rows exist only
// while every bid bound is <= 14).  Registers keep meta_pack's layout.
constexpr __host__ __device__ __forceinline__ uint32_t meta_link_pack(uint32_t m, uint32_t link)
{
    return (m & 1023u) | ((m >> 12) & 1u) << 10 | ((m >> 13) & 31u) << 11 | link << 16;
}
constexpr __host__ __device__ __forceinline__ uint32_t meta_link_meta(uint32_t w)
{
    return (w & 1023u) | ((w >> 10) & 1u) << 12 | ((w >> 11) & 31u) << 13;
}
constexpr __host__ __device__ __forceinline__ uint32_t meta_link_next(uint32_t w) { return w >> 16; }
#define META_LINK_RT(i, isd, mm, link)                                                                      \
    (meta_link_meta(meta_link_pack(meta_pack(i, ST_M, isd, mm, 0, 0), link)) == meta_pack(i, ST_M, isd, mm, 0, 0) && \
     meta_link_next(meta_link_pack(meta_pack(i, ST_M, isd, mm, 0, 0), link)) == (link))
static_assert(META_LINK_RT(1023u, 1u, 31u, 0u), "entry link: round trip at the field limits");
static_assert(META_LINK_RT(1023u, 1u, 31u, 0xFFFEu), "entry link: round trip at the field limits");
static_assert(META_LINK_RT(1023u, 1u, 31u, NIL16), "entry link: round trip at the field limits");
static_assert(META_LINK_RT(0u, 0u, 0u, NIL16) && META_LINK_RT(0u, 0u, 0u, 0u), "entry link: round trip of zero fields");
static_assert(META_LINK_RT(1023u, 0u, 0u, 0x8000u) && META_LINK_RT(0u, 1u, 0u, 0u) && META_LINK_RT(0u, 0u, 31u, 0u),
              "entry link: each field alone");
#undef META_LINK_RT
#define M_I(m) ((int)((m) & 1023u))
#define M_ST(m) ((int)(((m) >> 10) & 3u))
#define M_ISD(m) ((int)(((m) >> 12) & 1u))
#define M_MM(m) ((int)(((m) >> 13) & 127u))
#define M_GO(m) ((int)(((m) >> 20) & 15u))
#define M_GE(m) ((int)((m) >> 24))

// control word: ph:3 | strand:1 | has_seed:1 | reg:1 | has_vt:1 | seed_alias:1 | ovf:2 | len:10 | seed_len:10
#define C_PH(c) ((c) & 7u)
#define C_STRAND(c) (((c) >> 3) & 1u)
#define C_SEED(c) (((c) >> 4) & 1u)
#define C_REG(c) (((c) >> 5) & 1u)
#define C_VT(c) (((c) >> 6) & 1u)
#define C_ALIAS(c) (((c) >> 7) & 1u)
#define C_OVF(c) (((c) >> 8) & 3u)
#define C_LEN(c) ((int)(((c) >> 10) & 1023u))
#define C_SLEN(c) ((int)(((c) >> 20) & 1023u))
#define SET_PH(c, p) ((c) = ((c) & ~7u) | (p))

// v[c] for a runtime c in 0..3 as selects (hsa_sel4): a dynamically indexed register
// array would be lowered through the private segment (scratch) of the dispatch.  The
// elements are passed by value at constant indices (a select between two element
// references became a dynamically indexed load).
template <typename V>
__device__ __forceinline__ V pick4(const V v[4], uint32_t c)
{
    return hsa_sel4<V>(c, v[0], v[1], v[2], v[3]);
}

// The interval type of a kernel instantiation: uint32_t (the reference's bwtint_t,
// 2BWT-Interface.h:26) or uint64_t (texts of 2^32 characters or more).
template <typename IT> struct Ix;
template <> struct Ix<uint32_t> {
    __device__ static const RankDir &fwd(const SearchArgs &a) { return a.fwd; }
    __device__ static const RankDir &rev(const SearchArgs &a) { return a.rev; }
    __device__ static uint32_t T(const SearchArgs &a) { return a.T; }
    __device__ static const uint32_t *C(const SearchArgs &a) { return a.C; }
};
template <> struct Ix<uint64_t> {
    __device__ static const RankDir64 &fwd(const SearchArgs &a) { return a.fwd64; }
    __device__ static const RankDir64 &rev(const SearchArgs &a) { return a.rev64; }
    __device__ static uint64_t T(const SearchArgs &a) { return a.T64; }
    __device__ static const uint64_t *C(const SearchArgs &a) { return a.C64; }
};

// A stack entry (gap_entry_t, bwtaln.h:52-58): k, l, rev_k and the meta word
// (rev_l = rev_k + (l - k)).  32-bit: one uint4 in the pool; 64-bit: two.
template <typename IT> struct Ent {
    IT x, y, z;
    uint32_t w;
};
#ifndef HSA_WAVES_SIMD
#define HSA_WAVES_SIMD 4      // k_search's launch bound: waves per SIMD its VGPRs must allow
#endif
#ifndef HSA_POOL_CHUNK
#define HSA_POOL_CHUNK 1
#endif
#ifndef HSA_POOL_LINK
#define HSA_POOL_LINK 1       // A/B builds: -DHSA_POOL_LINK=0 keeps every pass's links in the link array
#endif
// The passes whose pool entries carry their bucket-list link (k_search's LK; the launch
// plan reserves no link array for them): every pass but HUGE, whose free list rewrites
// links, of 64-bit intervals (the entry has a spare word) and of 32-bit ungapped searches
// with 8- or 4-bit rows (the meta word has 16 spare bits, meta_link_pack).  The gapped
// 32-bit searches (a full meta word) and the 16-bit rows keep the link array.
constexpr __host__ __device__ bool pool_link_in_entry(bool huge, bool it64, bool gaps, bool rows16)
{
    return HSA_POOL_LINK && !huge && (it64 || (!gaps && !rows16));
}
// Slot s of a lane's pool.  Default: uint4 element base + s * 64 (32-bit entries) or the
// two elements base + s * 128 and base + s * 128 + 64 (64-bit entries); base (pool_base)
// is the lane's slot 0, computed once per launch.  HSA_POOL_CHUNK: 64-byte chunks of
// consecutive slots per lane (4 entries, or 2 of 64 bits), chunk q of lane l at
// (q * 64 + l) * 64 B in the wave's region, so an expansion's burst of pushes
// (consecutive slots) writes whole sectors; the links likewise, 32 per 64 B.  The wave's
// region is sized for pcap rounded up to 32 slots (the scratch reservation does so).
template <typename IT>
__device__ __forceinline__ size_t pool_base(size_t wv, uint32_t pcap, int lane)
{
#if HSA_POOL_CHUNK
    return (sizeof(IT) == 4 ? 1u : 2u) * wv * (size_t)((pcap + 31u) & ~31u) * 64 + (size_t)lane * 4;
#else
    return (sizeof(IT) == 4 ? 1u : 2u) * wv * pcap * 64 + (size_t)lane;
#endif
}
template <typename IT>
__device__ __forceinline__ size_t ent_at(size_t base, uint32_t slot)
{
#if HSA_POOL_CHUNK
    constexpr uint32_t EQ = sizeof(IT) == 4 ? 4u : 2u, U = sizeof(IT) == 4 ? 1u : 2u;
    return base + (size_t)(slot / EQ) * 256 + (slot % EQ) * U;
#else
    return base + (size_t)slot * (sizeof(IT) == 4 ? 64 : 128);
#endif
}
template <typename IT>
__device__ __forceinline__ Ent<IT> ent_load(const uint4 *pool, size_t base, uint32_t slot)
{
    const size_t i = ent_at<IT>(base, slot);
    if constexpr (sizeof(IT) == 4) {
        const uint4 v = pool[i];
        return Ent<IT>{v.x, v.y, v.z, v.w};
    } else {
        const uint4 u = pool[i], v = pool[i + (HSA_POOL_CHUNK ? 1 : 64)];
        return Ent<IT>{(uint64_t)u.x | (uint64_t)u.y << 32, (uint64_t)u.z | (uint64_t)u.w << 32,
                       (uint64_t)v.x | (uint64_t)v.y << 32, v.z};
    }
}
template <typename IT>
__device__ __forceinline__ void ent_store(uint4 *pool, size_t base, uint32_t slot, const Ent<IT> &e)
{
    const size_t i = ent_at<IT>(base, slot);
    if constexpr (sizeof(IT) == 4) {
        pool[i] = make_uint4(e.x, e.y, e.z, e.w);
    } else {
        pool[i] = make_uint4((uint32_t)e.x, (uint32_t)(e.x >> 32), (uint32_t)e.y, (uint32_t)(e.y >> 32));
        pool[i + (HSA_POOL_CHUNK ? 1 : 64)] = make_uint4((uint32_t)e.z, (uint32_t)(e.z >> 32), e.w, 0u);
    }
}
// The same with the entry's 16-bit bucket-list link inside it (k_search's LK): in the
// meta word's upper half (32-bit entries, meta_link_pack) or in the second element's
// last word, which ent_store leaves 0 (64-bit entries).  One sector per pop, one store
// per push, and no link array.
template <typename IT>
__device__ __forceinline__ Ent<IT> ent_load_link(const uint4 *pool, size_t base, uint32_t slot, uint32_t &link)
{
    const size_t i = ent_at<IT>(base, slot);
    if constexpr (sizeof(IT) == 4) {
        const uint4 v = pool[i];
        link = meta_link_next(v.w);
        return Ent<IT>{v.x, v.y, v.z, meta_link_meta(v.w)};
    } else {
        const uint4 u = pool[i], v = pool[i + (HSA_POOL_CHUNK ? 1 : 64)];
        link = v.w;
        return Ent<IT>{(uint64_t)u.x | (uint64_t)u.y << 32, (uint64_t)u.z | (uint64_t)u.w << 32,
                       (uint64_t)v.x | (uint64_t)v.y << 32, v.z};
    }
}
template <typename IT>
__device__ __forceinline__ void ent_store_link(uint4 *pool, size_t base, uint32_t slot, const Ent<IT> &e, uint32_t link)
{
    const size_t i = ent_at<IT>(base, slot);
    if constexpr (sizeof(IT) == 4) {
        pool[i] = make_uint4(e.x, e.y, e.z, meta_link_pack(e.w, link));
    } else {
        pool[i] = make_uint4((uint32_t)e.x, (uint32_t)(e.x >> 32), (uint32_t)e.y, (uint32_t)(e.y >> 32));
        pool[i + (HSA_POOL_CHUNK ? 1 : 64)] = make_uint4((uint32_t)e.z, (uint32_t)(e.z >> 32), e.w, link);
    }
}
// staged words per hit (HB) and words per output hit record: bwt_aln1_t (bwtaln.h:41-50)
// for 32-bit intervals; hsa_aln64_t (include/hsa_gpu.h) for 64-bit ones
template <typename IT> struct HitW { static constexpr uint32_t STAGE = sizeof(IT) == 4 ? 9u : 10u;
                                     static constexpr uint32_t OUT = sizeof(IT) == 4 ? 9u : 14u; };

template <int MW> struct BMask;
template <> struct BMask<0> {        // <= 32 buckets: one 32-bit word
    uint32_t m0 = 0;
    __device__ __forceinline__ void clear() { m0 = 0; }
    __device__ __forceinline__ bool any() const { return m0 != 0; }
    __device__ __forceinline__ int lowest() const { return m0 ? __ffs(m0) - 1 : (1 << 30); }
    __device__ __forceinline__ bool test(int b) const { return (m0 >> b) & 1u; }
    __device__ __forceinline__ void set(int b) { m0 |= 1u << b; }
    __device__ __forceinline__ void reset(int b) { m0 &= ~(1u << b); }
};
template <> struct BMask<1> {
    uint64_t m0 = 0;
    __device__ __forceinline__ void clear() { m0 = 0; }
    __device__ __forceinline__ bool any() const { return m0 != 0; }
    __device__ __forceinline__ int lowest() const { return m0 ? __ffsll((unsigned long long)m0) - 1 : (1 << 30); }
    __device__ __forceinline__ bool test(int b) const { return (m0 >> b) & 1ull; }
    __device__ __forceinline__ void set(int b) { m0 |= 1ull << b; }
    __device__ __forceinline__ void reset(int b) { m0 &= ~(1ull << b); }
};
template <> struct BMask<2> {
    uint64_t m0 = 0, m1 = 0;
    __device__ __forceinline__ void clear() { m0 = m1 = 0; }
    __device__ __forceinline__ bool any() const { return (m0 | m1) != 0; }
    __device__ __forceinline__ int lowest() const
    {
        if (m0) return __ffsll((unsigned long long)m0) - 1;
        if (m1) return 64 + __ffsll((unsigned long long)m1) - 1;
        return 1 << 30;
    }
    __device__ __forceinline__ bool test(int b) const { return b < 64 ? ((m0 >> b) & 1ull) : ((m1 >> (b - 64)) & 1ull); }
    __device__ __forceinline__ void set(int b) { if (b < 64) m0 |= 1ull << b; else m1 |= 1ull << (b - 64); }
    __device__ __forceinline__ void reset(int b) { if (b < 64) m0 &= ~(1ull << b); else m1 &= ~(1ull << (b - 64)); }
};

// Pruning element of one read position, as k_widths writes it and k_search keeps it
// in LDS: min(bid, BIDM) | (w[p] == w[p+1]) << BIDB | (code & 3) << CSH |
// (code > 3) << (CSH + 2), code being the strand sequence's base at p.  A bid is
// only ever compared with m, m - 1 or m_seed - 1 (bwtgap.c:170, :256-263), all
// <= max(max_diff, max_seed_diff), so capping it at BIDM is exact while that bound
// is < BIDM: 8-bit elements (4-bit bid) for bounds <= 14, else 16-bit (8-bit bid).
// The base code keeps exactly what bwt_match_gap derives from it: c > 3 (N) and
// (c + j) & 3 (bwtgap.c:305-306).
template <typename WT> struct WFmt {
    static constexpr bool NIB = false;
    static constexpr uint32_t BIDB = sizeof(WT) == 1 ? 4u : 8u;
    static constexpr uint32_t BIDM = (1u << BIDB) - 1u;
    static constexpr uint32_t EQ = 1u << BIDB;
    static constexpr uint32_t CSH = BIDB + 1u;
    static constexpr uint32_t EB = 8u * sizeof(WT);           // bits per element
    static constexpr uint32_t EPW = 4u / sizeof(WT);          // elements per u32
    __device__ static uint32_t code_bits(uint32_t c) { return (c & 3u) << CSH | (c > 3 ? 4u : 0u) << CSH; }
    __device__ static uint32_t code(uint32_t v) { return (v >> CSH) & 7u; }   // 0..3, or 4..7 for N
};

// 4-bit elements for long reads (k_search only): min(bid, 7) | eq << 3, eight per LDS
// word, exact while max(max_diff, max_seed_diff) <= 6.  k_widths still writes the
// 8-bit rows to HBM; k_search packs them into LDS at each strand start and reads the
// base codes from the HBM row (L2-resident), so a 250 bp read needs 126 B of LDS per
// lane instead of 252 B and the CU holds twice the waves.
struct WNib { uint8_t v; };
template <> struct WFmt<WNib> {
    static constexpr bool NIB = true;
    static constexpr uint32_t BIDB = 3u, BIDM = 7u, EQ = 8u, EB = 4u, EPW = 8u;
};

// The mixed format (SN, "seed nibbles") of 8-bit rows: the read row stays 8-bit and the seed
// row, which carries no base code and whose bids are only compared with max_seed_diff - ...
// - 1 (bwtgap.c:259-263), is 4-bit, exact while max_seed_diff <= 6.  k_widths writes it to
// HBM already packed (width_step with WFmt<WNib>'s constants), so k_search still copies both
// rows with the one-wait LDS-DMA, and the read row's LDS copy drops element len: a 100 bp
// read with a 32-base seed takes 25 + 4 LDS words per lane instead of 26 + 9.
template <typename WT, bool SN> using SeedFmt = WFmt<typename std::conditional<SN, WNib, WT>::type>;

// four 8-bit elements (WFmt<uint8_t>) -> four 4-bit ones in the low 16 bits
__device__ __forceinline__ uint32_t nib4(uint32_t x)
{
    uint32_t b = x & 0x0F0F0F0Fu;                                   // bids, <= 15 per byte
    const uint32_t ge7 = ((b + 0x09090909u) >> 4) & 0x01010101u;     // bid >= 7
    b = (b & ~(ge7 * 0x0Fu)) | ge7 * 7u;
    uint32_t n = b | ((x >> 4) & 0x01010101u) << 3;                   // | eq << 3
    n = (n | n >> 4) & 0x00FF00FFu;
    return (n | n >> 8) & 0xFFFFu;
}

#ifdef HSA_DIAG
// Diagnostic build only (-DHSA_DIAG, never the product library): per-workgroup
// start/end s_memtime and s_memrealtime of the last launch, for the in-kernel
// clock and the workgroup-duration spread.
static __device__ unsigned long long g_diag[8192 * 4];
// event counters: 0 width steps, 1 exact steps, 2 expand steps, 3 virtual-top pops,
// 4 pool pops, 5 outer iterations (per wave), 6 lanes stepping summed over outer
// iterations, 7 control-loop iterations (per wave), 8 entries flushed to the pool,
// 9..12 shader cycles per wave in acquisition / control / rank-load wait / apply,
// 13 gap_shadow calls with last_diff_pos > 0, 14 their summed last_diff_pos,
// 15 strand starts, 16/17 exact/expand steps on a unique interval (l == k), 18/19
// width steps on a unique interval / all width steps; maxima over the launch's reads
// (a read = acquisition to finish_job, both strands): 21 rank steps, 22 s_memrealtime
// ticks (100 MHz), 23 pops; 24 / 25 rank steps of the longest item that ended with /
// without hits (split mode: an item is one strand)
static __device__ unsigned long long g_dctr[32];
#define DC(i) (++dc[i])
#else
#define DC(i) ((void)0)
#endif

// ---------------------------------------------------------------- k_widths
// bwt_cal_width type 1 (bwtaln.c:84-97) of every (read, strand): the whole read
// (width_back) and its last seed_len bases (width_seed, bwtaln.c:344-348).  The
// strand-1 sequence is the reverse complement (seq_reverse(.., 1), bwtaln.c:337).
// Forward extension on the reverse BWT with the forward C table
// (BWTSARangeForeward, 2BWT-Interface.c:121-131).
//
// One lane per (read, strand) row, rows in order, so a wave's 64 rows are stored
// interleaved -- element e of row R at (R / 64 * cap + e) * 64 + R % 64 -- and every
// store of a step is one coalesced 256-byte wave store.  The two chains of a row
// (read and seed) are independent, so each iteration advances both: two rank pairs
// in flight per lane.  All reads of a batch have similar lengths, so the lanes stay
// converged without a work queue.
template <typename IT> struct WChain {
    IT k, l;
    uint32_t bid;
    IT prevw;
    uint32_t acc;
    uint32_t tl, tix;              // width trie: characters since the last reset, and their node
    uint32_t lr;                   // position of the last reset (the cost order's tail length)
};

template <typename WT, typename IT>
__device__ __forceinline__ void width_step(const SearchArgs &a, WChain<IT> &ch, uint32_t t, uint32_t n, uint32_t c,
                                           uint32_t cbits, uint32_t *__restrict__ brow, IT *__restrict__ wrow,
                                           uint32_t &st_q, uint32_t &st_b, uint32_t &st_t)
{
    using F = WFmt<WT>;
    IT w;
    if (t < n) {
        if (c < 4) {
            if (ch.tl < a.ktd) {
                // a string of <= ktd characters since the reset: its interval from the
                // width trie (the same forward extension, hsa_trie.h)
                ch.tix = ch.tix * 4u + c;
                ++ch.tl;
                trie_w_load<IT>(a.ktw, trie_base(ch.tl) + ch.tix, ch.k, ch.l);
                ++st_t;
            } else {
                IT ok, ol;
                st_b += occ1_pair(Ix<IT>::rev(a), ch.k, ch.l + 1u, c, ok, ol);
                const IT cc = pick4(Ix<IT>::C(a), c);
                ch.k = cc + ok + 1u;
                ch.l = cc + ol;
            }
            st_q += 2;
        }
        if (ch.k > ch.l || c > 3) { ch.k = 0; ch.l = Ix<IT>::T(a); ++ch.bid; ch.tl = 0; ch.tix = 0; ch.lr = t; }
        w = ch.l - ch.k + 1u;
    } else {
        w = 0; ++ch.bid;                                         // width[len] = {0, ++bid}
    }
    // element t-1 is final now (its eq bit needs w[t]); elements go out a word at a time
    if (t > 0) {
        if (ch.prevw == w) ch.acc |= F::EQ << (((t - 1) % F::EPW) * F::EB);
        if ((t - 1) % F::EPW == F::EPW - 1) { brow[((t - 1) / F::EPW) * 64] = ch.acc; ch.acc = 0; }
    }
    ch.acc |= ((ch.bid < F::BIDM ? ch.bid : F::BIDM) | cbits) << ((t % F::EPW) * F::EB);
    if (wrow) wrow[t * 64] = w;
    ch.prevw = w;
    if (t == n) brow[(t / F::EPW) * 64] = ch.acc;
}

// One width row: both chains (the whole strand sequence and its last seed_len bases) of
// list position q's strand; returns the rank queries, 64-byte sectors and trie loads it
// took, and the chain's final bid (width[len].bid = the bid of the last base + 1).
struct WRow { uint32_t q, b, t, bid, tail; };

// The cost key of a row (SearchArgs::wkey): its final bid, and with okey the length of
// its last segment (positions after the last reset, where the search starts with the
// least slack): a short one lets the search branch sooner.
__device__ __forceinline__ uint8_t cost_key(const SearchArgs &a, const WRow &w)
{
    const uint32_t b = w.bid < 15u ? w.bid : 15u;
    if (!a.okey) return (uint8_t)(w.bid < 255u ? w.bid : 255u);
    return (uint8_t)(b << 4 | (w.tail < 16u ? 2u : w.tail < 48u ? 1u : 0u));
}

template <typename WT, typename IT, bool SN = false>
__device__ __forceinline__ WRow width_row(const SearchArgs &a, uint32_t R, uint32_t strand, const hsa_job_t &J)
{
    using F = WFmt<WT>;
    const uint32_t len = J.len;
    const uint64_t off = J.off;
    const bool has_seed = (int)len > J.seed_len;
    const uint32_t slen = has_seed ? (uint32_t)J.seed_len : 0u;
    const size_t rb = R >> 6, rl = R & 63u;
    uint32_t *const brow = reinterpret_cast<uint32_t *>(const_cast<uint8_t *>(a.wb)) + rb * (a.rb / 4) * 64 + rl;
    uint32_t *const srow = reinterpret_cast<uint32_t *>(const_cast<uint8_t *>(a.ws)) + rb * (a.rs / 4) * 64 + rl;
    IT *const wrow = reinterpret_cast<IT *>(a.wg) + rb * a.rg * 64 + rl;
    WChain<IT> f{0, Ix<IT>::T(a), 0, 0, 0, 0, 0}, sd{0, Ix<IT>::T(a), 0, 0, 0, 0, 0};
    uint32_t st_q = 0, st_b = 0, st_t = 0;
    const uint32_t s0 = len - slen;
#ifndef HSA_CODECACHE
#define HSA_CODECACHE 1                    // A/B builds: -DHSA_CODECACHE=0 loads a byte every step
#endif
    // Each chain walks its read one position per step (forwards, or backwards on the rc
    // strand), so the 4-byte word of its last base is kept in registers and a load goes
    // out every fourth step.  The codes buffer is 4-byte aligned and padded past its last
    // read (hsa_device_batch_t.d_codes), so the word load stays inside it.
    uint32_t cq[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, cword[2] = {0u, 0u};
    auto base = [&](uint32_t sp, int ch) -> uint32_t {
        const uint64_t ix = off + (strand ? len - 1u - sp : sp);
        uint32_t c;
        if constexpr (HSA_CODECACHE) {
            const uint32_t wq = (uint32_t)(ix >> 2);
            if (wq != cq[ch]) {
                cword[ch] = *reinterpret_cast<const uint32_t *>(a.codes + (ix & ~(uint64_t)3));
                cq[ch] = wq;
            }
            c = (cword[ch] >> (((uint32_t)ix & 3u) * 8u)) & 0xFFu;
        } else {
            c = a.codes[ix];
        }
        return strand && c < 4 ? 3u - c : c;
    };
    for (uint32_t t = 0; t <= len; ++t) {
        const uint32_t cf = t < len ? base(t, 0) : 4u;
        // the read's elements also carry the strand sequence's base (k_search's getc)
        width_step<WT, IT>(a, f, t, len, cf, t < len ? F::code_bits(cf) : 0u, brow, wrow, st_q, st_b, st_t);
        if (has_seed && t <= slen) {
            const uint32_t cs = t < slen ? base(s0 + t, 1) : 4u;
            width_step<typename std::conditional<SN, WNib, WT>::type, IT>(a, sd, t, slen, cs, 0u, srow, nullptr, st_q,
                                                                          st_b, st_t);
        }
    }
    return WRow{st_q, st_b, st_t, f.bid, len - f.lr};
}

// one atomic per wave and counter (the kernels' lanes all reach it)
__device__ __forceinline__ void wave_add(unsigned long long *c, unsigned long long v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(c, v);
}

#define HSA_NOFWD 0xFFFFFFFFu        // wq: this read's forward row was not computed
#define HSA_F_NEEDFWD 0x100u         // k_search internal: rc had no hit, forward row missing
// wq's two high bits (a row's query count stays far below 2^30, so no flagged value equals
// HSA_NOFWD): the strand's search cannot have a hit, because the bid of its last base
// exceeds max_diff and bwt_match_gap prunes the root at its first pop (bwtgap.c:170).
// k_search counts that pop and starts no such strand (begin_item).
#define HSA_WQ_RC_DOOMED 0x80000000u
#define HSA_WQ_FWD_DOOMED 0x40000000u
#define HSA_WQ_COUNT 0x3FFFFFFFu
#ifndef HSA_DOOM_SKIP
#define HSA_DOOM_SKIP 1                    // A/B builds: -DHSA_DOOM_SKIP=0 starts every strand
#endif
#ifndef HSA_LAZY_MIN_LEN
#define HSA_LAZY_MIN_LEN 100               // lazy forward rows by default for reads this long (launch_pass) ...
#endif
#define HSA_LAZY_MIN_LEN_GAPPED 200        // ... and in searches with gap opens

// the root of a row's search is pruned: width[len - 1].bid = w.bid - 1 > max_diff
__device__ __forceinline__ bool row_doomed(const WRow &w, const hsa_job_t &J) { return (int)w.bid - 1 > J.max_diff; }

// One lane per row (rows in order): row = list position * 2 + strand.  The forward
// strand's rows are computed speculatively and count as the reference's work only
// when k_search searches that strand (ctr[CTR_FWD_Q_ALL]: all of them).
template <typename WT, typename IT = uint32_t, bool SN = false>
__global__ void __launch_bounds__(BLOCK) k_widths(SearchArgs a)
{
    const uint32_t R = blockIdx.x * BLOCK + threadIdx.x;     // row = list position * 2 + strand
    const uint32_t n_jobs = a.n_dev ? (uint32_t)*a.n_dev : (uint32_t)a.n_jobs;
    const uint32_t q = R >> 1, strand = R & 1u;
    WRow w{0, 0, 0, 0};
    uint32_t doomed = 0;
    if (R < 2u * n_jobs) {
        const hsa_job_t J = a.jobs[a.job_list ? a.job_list[q] : (int)q];
        w = width_row<WT, IT, SN>(a, R, strand, J);
        doomed = row_doomed(w, J) ? 1u : 0u;
        if (a.wkey) a.wkey[R] = cost_key(a, w);
    }
    // a read's two rows are neighbouring lanes: the forward lane writes both flags
    const uint32_t rc_doomed = (uint32_t)__shfl_xor((int)doomed, 1);
    if (R < 2u * n_jobs && !strand)
        a.wq[q] = w.q | (rc_doomed ? HSA_WQ_RC_DOOMED : 0u) | (doomed ? HSA_WQ_FWD_DOOMED : 0u);
    // rank queries: the reverse-complement strand is always searched (bwtaln.c:343)
    wave_add(&a.ctr[CTR_RANK], strand ? w.q : 0u);
    wave_add(&a.ctr[CTR_WIDTH_Q], strand ? w.q : 0u);
    wave_add(&a.ctr[CTR_FWD_Q_ALL], strand ? 0u : w.q);
    wave_add(&a.ctr[CTR_SECTORS], w.b);
    wave_add(&a.ctr[CTR_TRIE], w.t);
}

// The lazy main pass of a large batch, one launch: the rc row of every read, and the
// forward row of the reads whose rc search cannot have a hit (row_doomed); the others get
// wq = HSA_NOFWD and k_search hands them to the forward pass if rc finds nothing
// (bwtaln.c:343-359).  A workgroup takes BLOCK reads: every lane computes its read's rc row
// into the rc plane (row q); the doomed reads are compacted through LDS (a ballot per wave,
// the waves' counts and lists in LDS, one barrier), and lanes 0 .. k - 1 compute their
// forward rows into the forward plane at the workgroup's own place, row
// n_al + blockIdx.x * BLOCK + i (rmap[q]), so a step's stores stay one coalesced wave store
// per word and nothing is shared between workgroups.  A wave left without a row only adds its counts.
// The forward rows here are speculative (CTR_FWD_Q_ALL), as k_widths' are.
template <typename WT, typename IT = uint32_t, bool SN = false>
__global__ void __launch_bounds__(BLOCK) k_widths_lazy(SearchArgs a)
{
    __shared__ uint32_t s_cnt[BLOCK / 64];
    __shared__ uint8_t s_src[BLOCK];                  // wave w's doomed reads (lane numbers in the workgroup) at w * 64
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q = blockIdx.x * BLOCK + tid;
    const uint32_t n_jobs = (uint32_t)a.n_jobs;
    const uint32_t n_al = (n_jobs + 63u) & ~63u;
    uint32_t rq = 0, sq = 0, sb = 0, stt = 0;
    bool more = false;
    if (q < n_jobs) {
        const hsa_job_t J = a.jobs[a.job_list ? a.job_list[q] : (int)q];
        const WRow w = width_row<WT, IT, SN>(a, q, 1u, J);
        more = row_doomed(w, J);
        rq = w.q; sb = w.b; stt = w.t;
        if (a.wkey) a.wkey[2 * q + 1] = cost_key(a, w);
        if (!more) {
            a.wq[q] = HSA_NOFWD;
            if (a.wkey) a.wkey[2 * q] = 255u;
        }
    }
    const uint64_t m = __ballot(more);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
    if (more) s_src[wave * 64u + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint8_t)tid;
    __syncthreads();
    // lane i takes the i-th doomed read of the workgroup, in wave order
    uint32_t k = 0, src = BLOCK;
    for (uint32_t v = 0; v < BLOCK / 64; ++v) {
        const uint32_t c = s_cnt[v];
        if (tid >= k && tid < k + c) src = s_src[v * 64u + (tid - k)];
        k += c;
    }
    if (wave * 64u < k && src < BLOCK) {
        const uint32_t q2 = blockIdx.x * BLOCK + src;
        const hsa_job_t J = a.jobs[a.job_list ? a.job_list[q2] : (int)q2];
        const uint32_t R = n_al + blockIdx.x * BLOCK + tid;
        const WRow w = width_row<WT, IT, SN>(a, R, 0u, J);
        a.rmap[q2] = (int32_t)R;
        a.wq[q2] = w.q | HSA_WQ_RC_DOOMED | (row_doomed(w, J) ? HSA_WQ_FWD_DOOMED : 0u);
        if (a.wkey) a.wkey[2 * q2] = cost_key(a, w);
        sq = w.q; sb += w.b; stt += w.t;
    }
    wave_add(&a.ctr[CTR_RANK], rq);
    wave_add(&a.ctr[CTR_WIDTH_Q], rq);
    wave_add(&a.ctr[CTR_FWD_Q_ALL], sq);
    wave_add(&a.ctr[CTR_SECTORS], sb);
    wave_add(&a.ctr[CTR_TRIE], stt);
}

// The forward pass of a lazy search: one lane per read k_search listed, its forward row
// (row 2 p, no plane map), the reference's work.
template <typename WT, typename IT = uint32_t, bool SN = false>
__global__ void __launch_bounds__(BLOCK) k_widths_fwd(SearchArgs a)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t n_jobs = a.n_dev ? (uint32_t)*a.n_dev : (uint32_t)a.n_jobs;
    WRow w{0, 0, 0, 0};
    if (p < n_jobs) {
        const hsa_job_t J = a.jobs[a.job_list ? a.job_list[p] : (int)p];
        w = width_row<WT, IT, SN>(a, 2u * p, 0u, J);
        a.wq[p] = w.q | (row_doomed(w, J) ? HSA_WQ_FWD_DOOMED : 0u);
    }
    wave_add(&a.ctr[CTR_RANK], w.q);
    wave_add(&a.ctr[CTR_WIDTH_Q], w.q);
    wave_add(&a.ctr[CTR_FWD_Q_ALL], w.q);
    wave_add(&a.ctr[CTR_FWD_Q_REF], w.q);
    wave_add(&a.ctr[CTR_SECTORS], w.b);
    wave_add(&a.ctr[CTR_TRIE], w.t);
}

// Caller-width mode: the width rows of each call from the caller's bwt_width_t pairs
// (hsa_match_gap_batch) -- the same element format and row layout k_widths writes;
// the row of list position q is q * 2 + strand.  Besides the pruning elements and the
// full w values, the full bids go to wbid: gap_shadow rewrites them (bwtgap.c:101).
template <typename WT>
__global__ void __launch_bounds__(BLOCK) k_widths_import(SearchArgs a)
{
    using F = WFmt<WT>;
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t n_jobs = a.n_dev ? (uint32_t)*a.n_dev : (uint32_t)a.n_jobs;
    if (q >= n_jobs) return;
    const int job = a.job_list ? a.job_list[q] : (int)q;
    const hsa_job_t J = a.jobs[job];
    const hsa_mg_job_t M = a.mg[job];
    const uint32_t R = q * 2u + (uint32_t)(M.strand & 1);
    const size_t rb = R >> 6, rl = R & 63u;
    uint32_t *const brow = reinterpret_cast<uint32_t *>(const_cast<uint8_t *>(a.wb)) + rb * (a.rb / 4) * 64 + rl;
    uint32_t *const srow = reinterpret_cast<uint32_t *>(const_cast<uint8_t *>(a.ws)) + rb * (a.rs / 4) * 64 + rl;
    uint32_t *const wrow = a.wg + rb * a.rg * 64 + rl;
    int32_t *const drow = a.wbid + rb * a.rg * 64 + rl;
    // elements 0..n of one row; element t: min(bid, BIDM) | (w[t] == w[t+1]) | base code.
    // A prefix row (HSA_MG_PREFIX: the first n entries of a longer bwt_cal_width row, the
    // splice seeds' widths, bwtgap.c:807) has the terminal {0, bid of entry n - 1, + 1}.
    const bool prefix = M.seed == HSA_SEED_ALIAS && M.ws_off == HSA_MG_PREFIX;
    auto emit = [&](uint32_t *row, const int32_t *w, uint32_t n, bool read_row) {
        uint32_t acc = 0;
        uint32_t wt = (uint32_t)w[0];
        for (uint32_t t = 0; t <= n; ++t) {
            const uint32_t bid = prefix && t == n ? (n ? (uint32_t)w[2 * t - 1] + 1u : 1u) : (uint32_t)w[2 * t + 1];
            const uint32_t wn = t + 1 < n || (t + 1 == n && !prefix) ? (uint32_t)w[2 * t + 2] : 0u;
            uint32_t e = bid < F::BIDM ? bid : F::BIDM;
            if (t < n && wt == wn) e |= F::EQ;
            if (read_row && t < n) e |= F::code_bits(a.codes[J.off + t]);
            acc |= e << ((t % F::EPW) * F::EB);
            if (t % F::EPW == F::EPW - 1 || t == n) { row[(t / F::EPW) * 64] = acc; acc = 0; }
            if (read_row) { wrow[t * 64] = wt; drow[t * 64] = (int32_t)bid; }
            wt = wn;
        }
    };
    emit(brow, a.cw + 2 * M.wb_off, J.len, true);
    if (M.seed == HSA_SEED_OWN) emit(srow, a.cw + 2 * M.ws_off, (uint32_t)J.seed_len, false);
}

// Caller-width mode: width_back after the search (gap_shadow rewrote it in the rows)
// back into the caller's pairs.  Reads that overflowed this pass are skipped: the
// re-run that completes them exports them.
static __global__ void __launch_bounds__(BLOCK) k_widths_export(SearchArgs a)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t n_jobs = a.n_dev ? (uint32_t)*a.n_dev : (uint32_t)a.n_jobs;
    if (q >= n_jobs) return;
    const int job = a.job_list ? a.job_list[q] : (int)q;
    if (a.flags[job] & HSA_F_OVERFLOW) return;
    const hsa_job_t J = a.jobs[job];
    const hsa_mg_job_t M = a.mg[job];
    if (M.seed == HSA_SEED_ALIAS && M.ws_off == HSA_MG_PREFIX) return;   // a row's prefix, read only
    const uint32_t R = q * 2u + (uint32_t)(M.strand & 1);
    const size_t base = (R >> 6) * (size_t)a.rg * 64 + (R & 63u);
    int32_t *const o = a.cw + 2 * M.wb_off;
    for (uint32_t t = 0; t <= J.len; ++t) {
        o[2 * t] = (int32_t)a.wg[base + t * 64];
        o[2 * t + 1] = a.wbid[base + t * 64];
    }
}


// Cost order of a batch's reads (see SearchArgs::wkey): the lower bid of a read's two
// strands -- a lower bound on the differences of its best strand (bwtaln.c:84-97) --
// bucketed into 16 bins, most differences first; order within a bin is arbitrary (every
// read's result is independent of when it is searched).
__device__ __forceinline__ uint32_t order_bin(const SearchArgs &a, uint32_t q)
{
    const uint32_t k0 = a.wkey[2 * q], k1 = a.wkey[2 * q + 1];
    const uint32_t k = k0 < k1 ? k0 : k1;
    if (a.okey) {                   // bid x 3 tail classes, costly first
        const uint32_t v = (k >> 4) * 3u + (k & 15u);
        return 15u - (v < 15u ? v : 15u);
    }
    return 15u - (k < 15u ? k : 15u);
}

static __global__ void __launch_bounds__(BLOCK) k_order_hist(SearchArgs a, uint32_t *hist)
{
    __shared__ uint32_t h[16];
    if (threadIdx.x < 16) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q < (uint32_t)a.n_jobs) atomicAdd(&h[order_bin(a, q)], 1u);
    __syncthreads();
    if (threadIdx.x < 16 && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// hist[16] -> exclusive offsets in hist[16..31] (one thread)
static __global__ void k_order_scan(uint32_t *hist)
{
    uint32_t s = 0;
    for (int b = 0; b < 16; ++b) { hist[16 + b] = s; s += hist[b]; }
}

static __global__ void __launch_bounds__(BLOCK) k_order_scatter(SearchArgs a, uint32_t *hist, int32_t *perm)
{
    __shared__ uint32_t h[16], base[16];
    if (threadIdx.x < 16) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t b = 0, r = 0;
    if (q < (uint32_t)a.n_jobs) { b = order_bin(a, q); r = atomicAdd(&h[b], 1u); }
    __syncthreads();
    if (threadIdx.x < 16 && h[threadIdx.x]) base[threadIdx.x] = atomicAdd(&hist[16 + threadIdx.x], h[threadIdx.x]);
    __syncthreads();
    if (q < (uint32_t)a.n_jobs) perm[base[b] + r] = (int32_t)q;
}

// Strand-split mode, after k_search: per read, the rc strand's result if it has a hit,
// else the fwd strand's (bwtaln.c:343-359), else the splice fallback; the fwd search and
// its widths count as the reference's work only then.  A read whose deciding strand
// overflowed its lane goes to the next capacity pass whole (both strands, in order).
static __global__ void __launch_bounds__(BLOCK) k_split_finalize(SearchArgs a)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t n_jobs = a.n_dev ? (uint32_t)*a.n_dev : (uint32_t)a.n_jobs;
    unsigned long long q_add = 0, p_add = 0, w_add = 0;
    if (q < n_jobs) {
        const int job = a.job_list ? a.job_list[q] : (int)q;
        const int32_t nr = a.sp_n[2 * q], nf = a.sp_n[2 * q + 1];
        int32_t na = 0;
        uint32_t fl = 0;
        uint64_t off = 0;
        if (nr < 0 || (nr == 0 && nf < 0)) {
            fl = HSA_F_OVERFLOW;
            if (a.ovf_list) a.ovf_list[atomicAdd(&a.ctr[a.ovf_ctr], 1ull)] = job;
            else atomicAdd(&a.ctr[CTR_UNFINISHED], 1ull);
        } else if (nr > 0) {
            na = nr; off = a.sp_off[2 * q];
            q_add = a.sp_q[2 * q]; p_add = a.sp_p[2 * q];
        } else {
            w_add = a.wq[q] & HSA_WQ_COUNT;
            q_add = (unsigned long long)a.sp_q[2 * q] + a.sp_q[2 * q + 1] + w_add;
            p_add = (unsigned long long)a.sp_p[2 * q] + a.sp_p[2 * q + 1];
            if (nf > 0) { na = nf; off = a.sp_off[2 * q + 1]; }
            else fl = HSA_F_FALLBACK;
        }
        a.n_aln[job] = na;
        a.flags[job] = fl;
        a.hit_off[job] = off;
    }
    // one atomic per wave and counter
    for (int d = 32; d >= 1; d >>= 1) {
        q_add += __shfl_xor(q_add, d);
        p_add += __shfl_xor(p_add, d);
        w_add += __shfl_xor(w_add, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (q_add) atomicAdd(&a.ctr[CTR_RANK], q_add);
        if (p_add) atomicAdd(&a.ctr[CTR_POPS], p_add);
        if (w_add) { atomicAdd(&a.ctr[CTR_WIDTH_Q], w_add); atomicAdd(&a.ctr[CTR_FWD_Q_REF], w_add); }
    }
}

// NT = lanes per workgroup: 256, or 64 when that puts more waves on the CU (per-lane
// LDS: many buckets, long reads; the mixed format's 19 waves) (plan_launch)
// HUGE: the last capacity pass (reads that overflowed the big pass): 32-bit pool
// links and popped slots reused through a free list, so a lane's pool holds any
// stack the reference can build (n_entries <= max_entries + 9, bwtgap.c:150-151).
// SN: the mixed format, 4-bit seed row beside the 8-bit read row (SeedFmt)
template <int MW, bool GAPS, typename WT, int NT, bool HUGE = false, typename IT = uint32_t, bool SN = false>
__global__ void __launch_bounds__(NT, HSA_WAVES_SIMD) k_search(SearchArgs a)
{
    using F = WFmt<WT>;
    using FS = SeedFmt<WT, SN>;                      // the seed row's elements
    static_assert(!SN || (std::is_same<WT, uint8_t>::value && !HUGE), "mixed format: 8-bit rows, not the HUGE pass");
    using E = Ent<IT>;
    using CT = typename std::conditional<sizeof(IT) == 8, int64_t, int>::type;   // best_cnt (int in bwtgap.c:127)
    constexpr uint32_t HW = HitW<IT>::STAGE, OW = HitW<IT>::OUT;
    const IT TT = Ix<IT>::T(a);
    const IT *const CC = Ix<IT>::C(a);
    using LT = typename std::conditional<HUGE, uint32_t, uint16_t>::type;   // pool link
    // the helpers' code (SearchArgs::fr_*): gapped 32-bit searches only (configs 3 and 4, whose
    // small calls end in long strands); the other kernels stay as they were (their registers:
    // the 64-bit 4-bit-row kernels spilled with it)
    constexpr bool FRH = !HUGE && HSA_HELPERS && GAPS && sizeof(IT) == 4 && !WFmt<WT>::NIB;
    constexpr uint32_t NIL = HUGE ? 0xFFFFFFFFu : (uint32_t)NIL16;
    // the link of a pool entry inside the entry (pool_link_in_entry): a link is written once,
    // at the push, with the bucket's old head, so it costs no sector of its own
    constexpr bool LK = pool_link_in_entry(HUGE, sizeof(IT) == 8, GAPS, std::is_same<WT, uint16_t>::value);
    // the implicit root levels (SearchArgs::sdc, hsa_trie.h).  Without indels an entry at
    // read position i stands for a string of exactly len - i characters, and on a level of
    // which every string occurs nothing reads its interval: a read longer than sdc keeps
    // its entries of fewer than sdc characters as trie node numbers (Ent::x; y and z
    // unused) and expands them without a rank step.  The root {0, T, 0} is node 0 as it is.
    // Level sdc, the table's, need not be complete: its entries carry their intervals.
    constexpr bool IMP = !GAPS && !HUGE && sizeof(IT) == 4 && !WFmt<WT>::NIB;
#ifdef HSA_DIAG
    if (threadIdx.x == 0 && blockIdx.x < 8192) {
        g_diag[blockIdx.x * 4 + 0] = __builtin_amdgcn_s_memtime();
        g_diag[blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memrealtime();
    }
#endif
    extern __shared__ __align__(16) uint8_t s_lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t gid = blockIdx.x * NT + tid;
    const int lane = (int)(tid & 63);
    // the two regimes' score tables (ntab entries each), then the two regimes
    for (uint32_t t = tid; t < 2 * a.ntab; t += NT) s_lds[t] = a.bmap[(t / a.ntab) * MAXS + t % a.ntab];
    static_assert(2 * sizeof(hsa_regime_t) <= 128, "regime LDS slot");
    hsa_regime_t *const s_reg = reinterpret_cast<hsa_regime_t *>(s_lds + 2 * a.ntab);
    if (tid < 2 * sizeof(hsa_regime_t) / 4)
        reinterpret_cast<uint32_t *>(s_reg)[tid] = reinterpret_cast<const uint32_t *>(a.regimes)[tid];
    __syncthreads();
    LT *const s_heads = reinterpret_cast<LT *>(s_lds + a.off_heads);
    using WTL = typename std::conditional<F::NIB, uint8_t, WT>::type;     // LDS element (8/16-bit formats)
    WTL *const s_wb = reinterpret_cast<WTL *>(s_lds + a.off_wb);
    WTL *const s_ws = reinterpret_cast<WTL *>(s_lds + a.off_ws);
    uint32_t *const s_nb = reinterpret_cast<uint32_t *>(s_lds + a.off_wb);   // 4-bit format: word q * NT + tid
    uint32_t *const s_ns = reinterpret_cast<uint32_t *>(s_lds + a.off_ws);
    // per-lane HBM scratch, wave-interleaved: element e of lane l of wave w at
    // (w * cap + e) * 64 + l, so one wave's accesses stay inside one small region
    // (few pages) and lanes at equal e coalesce
    const size_t wv = gid >> 6;
#if HSA_POOL_CHUNK
    const size_t link0 = wv * (size_t)((a.pcap + 31u) & ~31u) * 64 + (size_t)lane * 32;   // the lane's slot-0 link
#define NXT(s) reinterpret_cast<LT *>(a.nxt)[link0 + (size_t)((s) >> 5) * 2048 + ((s) & 31u)]
#else
    const size_t link0 = wv * a.pcap * 64 + (size_t)lane;        // the lane's slot-0 link
#define NXT(s) reinterpret_cast<LT *>(a.nxt)[link0 + (size_t)(s) * 64]
#endif
    const size_t pbase = pool_base<IT>(wv, a.pcap, lane);        // ... and slot-0 pool entry
#define HB(i) r->hbuf[(wv * r->hcap * HW + (uint32_t)(i)) * 64 + lane]   // r = cold_args() in scope
#define HEAD(b) s_heads[(uint32_t)(b) * NT + tid]
    // pruning elements in LDS, word-interleaved: the word holding elements
    // [EPW*q, EPW*q + EPW) of a lane is word q * NT + tid, so every lane reads its
    // own bank whatever position it is at, and a row copies in one store per word
#define WB(p) s_wb[(((uint32_t)(p) / F::EPW) * NT + tid) * F::EPW + (uint32_t)(p) % F::EPW]
#define WS(p) s_ws[(((uint32_t)(p) / F::EPW) * NT + tid) * F::EPW + (uint32_t)(p) % F::EPW]
#define RG(f) (s_reg[C_REG(ctl)].f)

    // ---- persistent per-lane state
    uint32_t ctl = PH_IDLE;        // control word (C_* accessors)
    uint32_t qpos = 0;             // position of the read in the job list (width row = qpos * 2 + strand)
    uint32_t pen = 0;              // s_mm | s_gapo << 10 | s_gape << 20
    uint32_t rmode = 0;            // mode | max_gapo << 8 | max_gape << 16
    uint32_t pos = 0;              // exact tail: next position
    IT ik = 0, il = 0;             // exact-tail interval
    IT aux = 0;                    // exact tail: rev_l
    int opt_max_diff = 0, max_diff = 0, best_score = 0, n_aln = 0, n_entries = 0;
    CT best_cnt = 0;
    uint32_t pool_top = 0;
    uint32_t free_head = NIL;      // HUGE: popped slots, linked through NXT
    uint32_t idle_acc = 0;         // (A): lane-iterations the waiting lanes idled since the last batch
    BMask<MW> mask;
    // the current entry (k, l, rev_k, meta); between an expansion and the next pop
    // it holds the virtual top when C_VT is set (the last child pushed, when it is
    // the next pop: it never goes to the pool)
    E e{0, 0, 0, 0};
    // per-lane statistics (a lane's counts of one launch stay far below 2^32); kept in
    // VGPRs: wave-uniform accumulators pushed the kernel's SGPRs into spills
    uint32_t st_p = 0, st_wq = 0, st_q = 0, st_b = 0;
    uint32_t sq0 = 0, sp0 = 0;            // split mode: the counters when the item started
    // helpers (SearchArgs::fr_*): frs bit 0 the strand offered its frontier (owner), bit 1
    // this lane runs a sub-search, bit 2 no more offers from this strand; fr_p0 the pops at
    // the strand's start, then at the offer (owner) or the sub-search's start (helper), with
    // fr_q0 the rank queries at that point
    uint32_t frs = 0, fr_p0 = 0, fr_q0 = 0;
    uint32_t fr_tick = 0;          // the wave's iterations (waiting lanes poll every 128)
    uint32_t st_hs = 0, st_hq = 0; // sub-searches this lane ran, and their rank queries
    const uint32_t n_jobs = a.n_dev ? (uint32_t)*a.n_dev : (uint32_t)a.n_jobs;
#ifdef HSA_DIAG
    uint32_t dc[21] = {0};
    uint64_t tsec[4] = {0, 0, 0, 0};
    uint64_t tt = 0;
    uint64_t rd_t0 = 0;
    uint32_t rd_steps = 0, rd_p0 = 0;
#define TMARK(k) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); tsec[k] += t_ - tt; tt = t_; } while (0)
#endif

#define S_MM ((int)(pen & 1023u))
#define S_GO ((int)((pen >> 10) & 1023u))
#define S_GE ((int)(pen >> 20))
#define R_MODE ((int)(rmode & 255u))
#define R_MAXGO ((int)((rmode >> 8) & 255u))
#define R_MAXGE ((int)(rmode >> 16))
#define SCORE(mm, go, ge) ((mm) * S_MM + (go) * S_GO + (ge) * S_GE)

    // pruning elements of the read row / seed row at p (WFmt), and the element write of gap_shadow
    auto wbg = [&](int p) -> uint32_t {
        if constexpr (F::NIB) return (s_nb[((uint32_t)p >> 3) * NT + tid] >> (((uint32_t)p & 7u) * 4u)) & 15u;
        else return WB(p);
    };
    auto wsg = [&](int p) -> uint32_t {
        if constexpr (FS::NIB) return (s_ns[((uint32_t)p >> 3) * NT + tid] >> (((uint32_t)p & 7u) * 4u)) & 15u;
        else return WS(p);
    };
    auto wbs = [&](int p, uint32_t v) {
        if constexpr (F::NIB) {
            uint32_t &w = s_nb[((uint32_t)p >> 3) * NT + tid];
            const uint32_t sh = ((uint32_t)p & 7u) * 4u;
            w = (w & ~(15u << sh)) | v << sh;
        } else {
            WB(p) = (WTL)v;
        }
    };
    // 4-bit format: the strand's 8-bit HBM row (base codes), and the base the next
    // step needs, loaded in the control phase so that its latency overlaps the rank load
    const uint8_t *rowp = nullptr;
    uint32_t cur_c = 0;
    // 4-bit format: the row word (4 positions) the last base came from, kept in registers.
    // A strand's steps walk its positions downwards (the virtual top is the child at
    // i - 1, an exact tail steps pos--), so most bases come from the word already held:
    // a row load is one L2 request (the rows of the resident waves are far larger than
    // L2 and mostly missed it), and the search is request-rate bound (config 5: 1.40 L2
    // requests per rank query with a load per step, 0.97 in config 2's 8-bit rows).
#ifndef HSA_ROWCACHE
#define HSA_ROWCACHE 1                     // A/B builds: -DHSA_ROWCACHE=0 loads the byte every step
#endif
    uint32_t rw_q = 0xFFFFFFFFu, rw_w = 0;
    // base of the current strand's sequence at p (from the LDS element, or the HBM row)
    auto getc = [&](int p) -> uint32_t {
        if constexpr (F::NIB && !HSA_ROWCACHE) {
            return WFmt<uint8_t>::code(rowp[((uint32_t)p >> 2) * 256u + ((uint32_t)p & 3u)]);
        } else if constexpr (F::NIB) {
            const uint32_t q = (uint32_t)p >> 2;
            if (q != rw_q) {
                rw_w = *reinterpret_cast<const uint32_t *>(rowp + q * 256u);
                rw_q = q;
            }
            return WFmt<uint8_t>::code((rw_w >> (((uint32_t)p & 3u) * 8u)) & 0xFFu);
        } else {
            return F::code(WB(p));
        }
    };
    // stack bucket of an entry: dense index of its score (bwtgap.c:46-75)
    auto bucket_of = [&](uint32_t m) -> int {
        if (!GAPS && a.mm_buckets) return M_MM(m);
        const int sc = SCORE(M_MM(m), M_GO(m), M_GE(m));
        return (uint32_t)sc < a.ntab ? (int)s_lds[C_REG(ctl) * a.ntab + sc] : 0xFF;
    };
    // push to the pool (gap_push, bwtgap.c:46-75)
    auto flush = [&](const E &v, int b) {
        if constexpr (LK) {
            // one store, the old head folded in.  (The overflow bit is set on one path for
            // both outcomes: with `ctl |= bit; return` beside `mask.set(b)` the compiler merged
            // the two updates into one store through a selected address, and ctl and the mask
            // went to the private segment.)
            uint32_t ovf = 1u;
            if ((uint32_t)b < a.nb && pool_top < a.pcap) {
                const uint32_t slot = pool_top++;
                DC(8);
                ent_store_link<IT>(a.pool, pbase, slot, v, mask.test(b) ? (uint32_t)HEAD(b) : NIL);
                HEAD(b) = (LT)slot;
                mask.set(b);
                ovf = 0u;
            }
            ctl |= ovf << 8;
            return;
        }
        if ((uint32_t)b >= a.nb) { ctl |= 1u << 8; return; }
        uint32_t slot;
        if (HUGE && free_head != NIL) {
            slot = free_head;
            free_head = NXT(slot);
        } else {
            if (pool_top >= a.pcap) { ctl |= 1u << 8; return; }
            slot = pool_top++;
        }
        DC(8);
        ent_store<IT>(a.pool, pbase, slot, v);
        const uint32_t old = mask.test(b) ? (uint32_t)HEAD(b) : NIL;
        NXT(slot) = (LT)old;
        HEAD(b) = (LT)slot;
        mask.set(b);
    };
    auto start_search = [&]() {
        best_score = SCORE(opt_max_diff + 1, R_MAXGO + 1, R_MAXGE + 1);
        max_diff = opt_max_diff;
        best_cnt = 0; n_aln = 0;
        mask.clear(); pool_top = 0; free_head = NIL;
        e = E{0, TT, 0, meta_pack((uint32_t)C_LEN(ctl), ST_M, 0, 0, 0, 0)};   // root (bwtgap.c:142)
        ctl |= 1u << 6;
        n_entries = 1;
        frs = 0; fr_p0 = st_p;
        SET_PH(ctl, PH_POP);
    };
    // the item number of the strand this lane searches (split mode: list position * 2 + 1 for fwd)
    auto fr_key = [&]() -> uint32_t { return qpos * 2u + (1u - C_STRAND(ctl)); };
    // width row of the current strand: row qpos * 2 + strand, 64 rows interleaved
    auto row_base = [&](uint32_t cap_words) -> size_t {
        const int32_t *const rm = cold_args()->rmap;
        const uint32_t r = rm ? (C_STRAND(ctl) ? qpos : (uint32_t)rm[qpos]) : qpos * 2u + C_STRAND(ctl);
        return (size_t)(r >> 6) * cap_words * 64 + (r & 63u);
    };
    // copy the strand's pruning elements (k_widths) into the lane's LDS columns, then
    // start bwt_match_gap (bwtgap.c:141-142)
    auto start_strand = [&]() {
        // LDS-DMA (global_load_lds_dword): word q of every active lane lands at
        // word q * NT + tid, which is exactly the wave's slice of the LDS layout, so
        // the whole row is in flight at once and one wait covers it
        const ColdArgs r = cold_args();
        const uint32_t *src = reinterpret_cast<const uint32_t *>(r->wb) + row_base(r->rb / 4);
        const uint32_t nwb = r->rb / 4;                // row capacity in words (uniform)
        if constexpr (F::NIB) {
            // two 8-bit words per LDS word, eight loads in flight
            rowp = reinterpret_cast<const uint8_t *>(src);
            rw_q = 0xFFFFFFFFu;
            auto pack = [&](const uint32_t *row, uint32_t nw, uint32_t *dst, uint32_t cap) {
                const uint32_t nn = (nw + 1u) / 2u < cap ? (nw + 1u) / 2u : cap;   // LDS words of the row
                for (uint32_t j = 0; j < nn; j += 4) {
                    uint32_t w[8];
#pragma unroll
                    for (uint32_t u = 0; u < 8; ++u) w[u] = 2u * j + u < nw ? row[(2u * j + u) * 64u] : 0u;
#pragma unroll
                    for (uint32_t u = 0; u < 4; ++u)
                        if (j + u < nn) dst[(j + u) * NT + tid] = nib4(w[2u * u]) | nib4(w[2u * u + 1u]) << 16;
                }
            };
            pack(src, nwb, s_nb, r->lds_wb);
            if (C_SEED(ctl) && !C_ALIAS(ctl))
                pack(reinterpret_cast<const uint32_t *>(r->ws) + row_base(r->rs / 4), r->rs / 4, s_ns, r->lds_ws);
        } else {
        // the words the lane's LDS columns hold: the whole HBM row, or in the mixed format
        // the words of elements 0 .. len - 1 (the HBM rows' last word may hold element len alone)
        uint32_t *const db = reinterpret_cast<uint32_t *>(s_wb) + (tid & ~63u);
        const uint32_t lwb = SN ? r->lds_wb : nwb;
        for (uint32_t q = 0; q < lwb; ++q)
            __builtin_amdgcn_global_load_lds(src + q * 64, db + q * NT, 4, 0, 0);
        if (C_SEED(ctl) && !C_ALIAS(ctl)) {
            const uint32_t *ss = reinterpret_cast<const uint32_t *>(r->ws) + row_base(r->rs / 4);
            uint32_t *const ds = reinterpret_cast<uint32_t *>(s_ws) + (tid & ~63u);
            const uint32_t nws = SN ? r->lds_ws : r->rs / 4;
            for (uint32_t q = 0; q < nws; ++q)
                __builtin_amdgcn_global_load_lds(ss + q * 64, ds + q * NT, 4, 0, 0);
        }
        }
        __builtin_amdgcn_s_waitcnt(0);                 // the DMA writes are visible to LDS reads
        DC(15);
        start_search();
    };
    auto finish_job = [&](uint32_t fl, int na, uint64_t ho) {
        const ColdArgs r = cold_args();
#ifdef HSA_DIAG
        atomicMax(&g_dctr[21], (unsigned long long)rd_steps);
        atomicMax(&g_dctr[22], (unsigned long long)(__builtin_amdgcn_s_memrealtime() - rd_t0));
        atomicMax(&g_dctr[23], (unsigned long long)(st_p - rd_p0));
        atomicMax(&g_dctr[na > 0 ? 24 : 25], (unsigned long long)rd_steps);
#endif
        if (r->split) {                       // one strand of a read: k_split_finalize decides
            const uint32_t pi = qpos * 2u + (1u - C_STRAND(ctl));
            r->sp_n[pi] = (fl & HSA_F_OVERFLOW) ? -1 : na;
            r->sp_off[pi] = ho;
            r->sp_q[pi] = st_q - sq0;
            r->sp_p[pi] = st_p - sp0;
            st_q = sq0; st_p = sp0;
            if constexpr (FRH) {
                if (a.fr_budget) {
                    if (frs & 1u) atomicOr(&r->fr_st[pi], FR_DONE);   // its helpers stop
                    atomicAdd(&r->fr_c[2], 1ull);                      // items finished (the exit test)
                    frs = 0;
                }
            }
            SET_PH(ctl, PH_IDLE);
            return;
        }
        const int job = r->job_list ? r->job_list[qpos] : (int)qpos;
        if (fl & HSA_F_NEEDFWD) {                 // the forward pass writes its outputs
            r->fwd_list[atomicAdd(r->fwd_n, 1ull)] = job;
            SET_PH(ctl, PH_IDLE);
            return;
        }
        if (fl & HSA_F_OVERFLOW) {
            if (r->ovf_list) r->ovf_list[atomicAdd(&r->ctr[r->ovf_ctr], 1ull)] = job;   // re-run by the next pass
            else atomicAdd(&r->ctr[CTR_UNFINISHED], 1ull);                       // the last pass: stays unfinished
        }
        r->n_aln[job] = na;
        r->flags[job] = fl;
        r->hit_off[job] = ho;
        SET_PH(ctl, PH_IDLE);
    };
    // a sub-search ends (no hit, a hit, its item decided, or its entries offered on): its
    // work goes to the item's sums, then its count leaves the item's open sub-searches
    auto help_done = [&]() {
        const ColdArgs r = cold_args();
        const uint32_t key = fr_key();
        const unsigned long long dq = st_q - fr_q0, dp = st_p - fr_p0;
        st_q = fr_q0; st_p = fr_p0;
        const unsigned long long o1 = atomicAdd(&r->fr_q[key], dq), o2 = atomicAdd(&r->fr_p[key], dp);
        asm volatile("s_waitcnt vmcnt(0)" :: "v"(o1), "v"(o2) : "memory");   // the sums land first
        atomicSub(&r->fr_st[key], 1u);
        ++st_hs; st_hq += (uint32_t)dq;
        frs = 0;
        SET_PH(ctl, PH_IDLE);
    };
    auto end_strand = [&]() {
        if constexpr (FRH) {
            if (frs & 2u) { help_done(); return; }
        }
        if (n_aln > 0) {
            const ColdArgs r = cold_args();
            const unsigned long long o = atomicAdd(&r->ctr[CTR_HITS], (unsigned long long)n_aln);
            if (o + (uint64_t)n_aln > r->hit_cap) { finish_job(HSA_F_OVERFLOW, 0, 0); return; }
            uint32_t *dst = r->hits + o * OW;
            const uint32_t s30 = C_STRAND(ctl) << 30;
            for (int h = 0; h < n_aln; ++h) {
                // bwtaln.c:371-372 (a direct bwt_match_gap call leaves start/end 0)
                const uint32_t end = h == 0 && !r->mg ? (uint32_t)(C_LEN(ctl) - 1) : 0u;
                if constexpr (sizeof(IT) == 4) {
                    // the six staged words first, then the record: one memory round trip per hit
                    const uint32_t v0 = HB(h * 9 + 0), v1 = HB(h * 9 + 1), v2 = HB(h * 9 + 2), v3 = HB(h * 9 + 3),
                                   v4 = HB(h * 9 + 4), v8 = HB(h * 9 + 8);
                    dst[h * 9 + 0] = v0;
                    dst[h * 9 + 1] = v1;
                    dst[h * 9 + 2] = v2;
                    dst[h * 9 + 3] = v3;
                    dst[h * 9 + 4] = v4;
                    dst[h * 9 + 5] = s30;
                    dst[h * 9 + 6] = 0;
                    dst[h * 9 + 7] = end;
                    dst[h * 9 + 8] = v8;
                } else {
                    // hsa_aln64_t (include/hsa_gpu.h): 14 words
                    uint32_t v[10];
#pragma unroll
                    for (int j = 0; j < 10; ++j) v[j] = HB(h * 10 + j);
                    dst[h * 14 + 0] = v[0];
                    dst[h * 14 + 1] = s30;
#pragma unroll
                    for (int j = 1; j < 9; ++j) dst[h * 14 + 1 + j] = v[j];
                    dst[h * 14 + 10] = 0;
                    dst[h * 14 + 11] = end;
                    dst[h * 14 + 12] = v[9];
                    dst[h * 14 + 13] = 0;
                }
            }
            finish_job(0, n_aln, o);
        } else if (cold_args()->mg || cold_args()->split) {
            finish_job(0, 0, 0);        // one call (or one split item), one strand
        } else if (C_STRAND(ctl)) {
            const uint32_t wq = cold_args()->wq[qpos];
            if (wq == HSA_NOFWD) {
                finish_job(HSA_F_NEEDFWD, 0, 0);   // its forward row is computed by the forward pass
            } else {
                ctl &= ~(1u << 3);          // strand 0
                st_wq += wq & HSA_WQ_COUNT; // its widths are the reference's work now (bwtaln.c:344-348)
                start_strand();
            }
        } else {
            finish_job(HSA_F_FALLBACK, 0, 0);
        }
    };
    // hit handling (bwtgap.c:188-243) for entry e with final interval (k,l,rk,rl);
    // returns false when the search must stop
    auto on_hit = [&](IT k, IT l, IT rk, IT rl) -> bool {
        const ColdArgs r = cold_args();
        if constexpr (FRH) {
            if (frs & 3u) {
                atomicOr(&r->fr_st[fr_key()], FR_HIT);   // the item has a hit: its sub-searches stop
                if (frs & 2u) return false;              // a helper records nothing
            }
        }
        const uint32_t m = e.w;
        const int score = SCORE(M_MM(m), M_GO(m), M_GE(m));
        if (n_aln == 0) {
            best_score = score;
            const int best_diff = M_MM(m) + M_GO(m) + ((R_MODE & MODE_GAPE) ? M_GE(m) : 0);
            if (!(R_MODE & MODE_NONSTOP)) max_diff = (best_diff + 1 > opt_max_diff) ? opt_max_diff : best_diff + 1;
        }
        if (score == best_score) {
            if constexpr (sizeof(IT) == 4) best_cnt = (int)((uint32_t)best_cnt + (l - k + 1u));
            else best_cnt += (CT)(l - k + 1u);
        } else if (best_cnt > RG(max_top2)) {
            return false;
        }
        bool add = true;
        if (M_GO(m)) {
            for (int j = 0; j < n_aln; ++j) {
                if constexpr (sizeof(IT) == 4) {
                    if (HB(j * 9 + 1) == k && HB(j * 9 + 2) == l) { add = false; break; }
                } else {
                    const uint64_t hk = (uint64_t)HB(j * 10 + 1) | (uint64_t)HB(j * 10 + 2) << 32;
                    const uint64_t hl = (uint64_t)HB(j * 10 + 3) | (uint64_t)HB(j * 10 + 4) << 32;
                    if (hk == k && hl == l) { add = false; break; }
                }
            }
        }
        if (add) {
            if ((uint32_t)n_aln >= r->hcap) { ctl |= 1u << 8; return false; }
            // gap_shadow (bwtgap.c:94-105) on width_back[0, last_diff_pos), then the
            // pruning elements of those positions (eq bit of p needs w[p+1])
            const IT x = l - k + 1u;
            const int ldp = M_ISD(m) ? M_I(m) : 0;
            if (ldp > 0) {
#ifdef HSA_DIAG
                DC(13); dc[14] += (uint32_t)ldp;
#endif
                IT *const wg = reinterpret_cast<IT *>(r->wg) + row_base(r->rg);
                int32_t *const wd = r->wbid ? r->wbid + row_base(r->rg) : nullptr;
#define WG(p) wg[(uint32_t)(p) * 64]
                IT jj = 0;
                for (int p = 0; p < ldp; ++p) {
                    IT w = WG(p);
                    if (w > x) { w -= x; WG(p) = w; }
                    else if (w == x) {
                        wbs(p, (wbg(p) & ~F::BIDM) | 1u);
                        WG(p) = TT - (++jj);
                        if (wd) wd[(uint32_t)p * 64] = 1;
                    }
                }
                IT wnext = WG(ldp);
                for (int p = ldp - 1; p >= 0; --p) {
                    const IT w = WG(p);
                    wbs(p, (wbg(p) & ~F::EQ) | (w == wnext ? F::EQ : 0u));
                    wnext = w;
                }
#undef WG
            }
            const uint32_t mw = (uint32_t)M_MM(m) | (uint32_t)M_GO(m) << 16 | (uint32_t)M_GE(m) << 24;
            if constexpr (sizeof(IT) == 4) {
                HB(n_aln * 9 + 0) = mw;
                HB(n_aln * 9 + 1) = k; HB(n_aln * 9 + 2) = l; HB(n_aln * 9 + 3) = rk; HB(n_aln * 9 + 4) = rl;
                HB(n_aln * 9 + 8) = (uint32_t)score;
            } else {
                HB(n_aln * 10 + 0) = mw;
                HB(n_aln * 10 + 1) = (uint32_t)k; HB(n_aln * 10 + 2) = (uint32_t)(k >> 32);
                HB(n_aln * 10 + 3) = (uint32_t)l; HB(n_aln * 10 + 4) = (uint32_t)(l >> 32);
                HB(n_aln * 10 + 5) = (uint32_t)rk; HB(n_aln * 10 + 6) = (uint32_t)(rk >> 32);
                HB(n_aln * 10 + 7) = (uint32_t)rl; HB(n_aln * 10 + 8) = (uint32_t)(rl >> 32);
                HB(n_aln * 10 + 9) = (uint32_t)score;
            }
            ++n_aln;
        }
        return true;
    };
    // m (available differences) of entry e (bwtgap.c:160-163)
    auto m_of = [&](uint32_t m) -> int {
        int mm = max_diff - (M_MM(m) + M_GO(m));
        if (R_MODE & MODE_GAPE) mm -= M_GE(m);
        return mm;
    };

    // start work item `item` (a read, a strand in split mode, or a direct call)
    auto begin_item = [&](uint32_t item) {
        const ColdArgs r = cold_args();
#ifdef HSA_DIAG
        rd_t0 = __builtin_amdgcn_s_memrealtime(); rd_steps = 0; rd_p0 = st_p;
#endif
        qpos = r->split ? item >> 1 : item;
        if (r->perm) qpos = (uint32_t)r->perm[qpos];
        const int job = r->job_list ? r->job_list[qpos] : (int)qpos;
        const hsa_job_t J = r->jobs[job];
        opt_max_diff = J.max_diff;
        const uint32_t len = J.len;
        if (r->mg) {
            // one direct bwt_match_gap call: its strand, its width_seed kind
            // (host-checked: 0 <= seed_len <= len when width_seed is given)
            const hsa_mg_job_t M = r->mg[job];
            const uint32_t has_seed = M.seed != HSA_SEED_NONE;
            ctl = (uint32_t)(M.strand & 1) << 3 | has_seed << 4 | (uint32_t)(J.regime & 1) << 5 |
                  (M.seed == HSA_SEED_ALIAS ? 1u : 0u) << 7 | len << 10 |
                  (has_seed ? (uint32_t)J.seed_len : 0u) << 20;
        } else {
            const uint32_t has_seed = (int)len > J.seed_len;
            ctl = 8u | has_seed << 4 | (uint32_t)(J.regime & 1) << 5 | len << 10 |
                  (has_seed ? (uint32_t)J.seed_len : 0u) << 20;     // strand 1 (rc first, bwtaln.c:343)
            if ((r->split && (item & 1u)) || r->fwd_only) ctl &= ~8u;   // split: odd items search fwd
            sq0 = st_q; sp0 = st_p;
        }
        const hsa_regime_t *R = s_reg + (J.regime & 1);
        pen = (uint32_t)R->s_mm | (uint32_t)R->s_gapo << 10 | (uint32_t)R->s_gape << 20;
        rmode = (uint32_t)R->mode | (uint32_t)R->max_gapo << 8 | (uint32_t)R->max_gape << 16;
        if (opt_max_diff > R->max_diff) ctl |= 2u << 8;
        if constexpr (HSA_DOOM_SKIP) {
            // an ordinary two-strand item whose rc root is pruned at its first pop (k_widths'
            // flag in wq): that pop is counted here and the forward strand starts at once, as
            // end_strand would start it a batch of (A) later; with the forward root pruned as
            // well the read ends here, without a row copy.  (Selects and one branch: each
            // nested divergent branch here costs the 64-bit kernels a saved exec mask they
            // have no SGPRs for.)
            uint32_t wq = HSA_NOFWD;
            if (!r->mg && !r->split && !r->fwd_only) wq = r->wq[qpos];      // uniform conditions
            const bool rcd = wq != HSA_NOFWD && (wq & HSA_WQ_RC_DOOMED) != 0u && !C_OVF(ctl);
            const bool both = rcd && (wq & HSA_WQ_FWD_DOOMED) != 0u;
            st_p += (rcd ? 1u : 0u) + (both ? 1u : 0u);
            ctl &= ~(rcd ? 8u : 0u);                         // strand 0
            st_wq += rcd ? wq & HSA_WQ_COUNT : 0u;           // its widths are the reference's work (bwtaln.c:344-348)
            if (both) {
                finish_job(HSA_F_FALLBACK, 0, 0);
                return;
            }
        }
        start_strand();
    };
    // helpers: publish this strand's live entries -- the virtual top, then every bucket's
    // list -- as sub-search roots of its item.  An entry's words are stored at agent scope
    // and its tag after a release, and the item's open-sub-search count is raised first, so
    // the count never reaches zero while one of them is unsearched.  False (nothing
    // published): the frontier is full, or the lists do not add up to n_entries.
    auto fr_offer = [&]() -> bool {
        const ColdArgs r = cold_args();
        const uint32_t cnt = (uint32_t)n_entries, nch = (cnt + FR_CH - 1u) / FR_CH;
        unsigned long long o = __hip_atomic_load(&r->fr_c[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (;;) {                                       // reserve nch chunks (no walk when they do not fit)
            if (o + nch > (unsigned long long)r->fr_cap) { atomicAdd(&r->fr_c[5], 1ull); return false; }
            const unsigned long long w = atomicCAS(&r->fr_c[0], o, o + nch);
            if (w == o) break;
            o = w;
        }
        const uint32_t key = fr_key();
        const unsigned int pend = atomicAdd(&r->fr_st[key], nch);     // before any chunk is published
        asm volatile("s_waitcnt vmcnt(0)" :: "v"(pend) : "memory");
        auto put = [&](uint32_t j, const E &v) {      // two 16-byte stores (the release below covers them)
            uint4 *d = reinterpret_cast<uint4 *>(r->fr_ent + ((o + j / FR_CH) * FR_CH + j % FR_CH) * FR_EW);
            if constexpr (sizeof(IT) == 4) {
                d[0] = make_uint4(v.x, v.y, v.z, v.w);
            } else {
                d[0] = make_uint4((uint32_t)v.x, (uint32_t)(v.x >> 32), (uint32_t)v.y, v.w);
                d[1] = make_uint4((uint32_t)(v.y >> 32), (uint32_t)v.z, (uint32_t)(v.z >> 32), 0u);
            }
        };
        uint32_t j = 0;
        if (C_VT(ctl)) put(j++, e);
        {
            BMask<MW> mm = mask;
            while (mm.any() && j < cnt) {
                const int b = mm.lowest();
                mm.reset(b);
                for (uint32_t sl = HEAD(b); sl != NIL && j < cnt; sl = NXT(sl)) put(j++, ent_load<IT>(a.pool, pbase, sl));
            }
        }
        // the lists must hold exactly n_entries: otherwise publish what was written, and mark
        // the item as having a hit, so that nothing is concluded from its sub-searches
        if (j != cnt) atomicOr(&r->fr_st[key], FR_HIT);
        for (uint32_t c = 0; c < nch; ++c) {
            const uint32_t in = j > c * FR_CH ? (j - c * FR_CH < FR_CH ? j - c * FR_CH : FR_CH) : 0u;
            r->fr_tag[o + c] = in << 26 | (key + 1u);
        }
        // complete chunks only enter the ready queue: a taker never waits on a walk
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long q0 = atomicAdd(&r->fr_c[9], (unsigned long long)nch);
        for (uint32_t c = 0; c < nch; ++c)
            __hip_atomic_store(&r->fr_rq[q0 + c], (uint32_t)(o + c) + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(&r->fr_c[4], 1ull);
        return true;
    };
    // helpers: a waiting lane starts a sub-search at ready-queue position qp: the chunk's
    // entries go to the lane's own stack (their order does not matter before a hit), under
    // its item's row and regime.  The queue slot is written right after the tail moved; the
    // chunk itself was released before that (agent-scope acquire, then plain loads).
    auto help_start = [&](unsigned long long qp) {
        const ColdArgs r = cold_args();
        uint32_t c1;
        while ((c1 = __hip_atomic_load(&r->fr_rq[qp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u)
            __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const size_t c = c1 - 1u;
        const uint32_t t = r->fr_tag[c];
        begin_item((t & 0x3FFFFFFu) - 1u);               // its strand's row and regime, a fresh stack
        ctl &= ~(1u << 6);                               // no virtual top: every entry from the pool
        const uint32_t in = t >> 26;
        const uint4 *s4 = reinterpret_cast<const uint4 *>(r->fr_ent + c * FR_CH * FR_EW);
        for (uint32_t q = 0; q < in; ++q) {
            const uint4 u = s4[2 * q], w = s4[2 * q + 1];
            E v;
            if constexpr (sizeof(IT) == 4) {
                v.x = u.x; v.y = u.y; v.z = u.z;
            } else {
                v.x = (uint64_t)u.x | (uint64_t)u.y << 32;
                v.y = (uint64_t)u.z | (uint64_t)w.x << 32;
                v.z = (uint64_t)w.y | (uint64_t)w.z << 32;
            }
            v.w = u.w;
            flush(v, bucket_of(v.w));
        }
        n_entries = (int)in;
        frs = 2u; fr_p0 = st_p; fr_q0 = st_q;
    };
    // helpers: the waiting lanes of the wave take published chunks (one CAS for the wave), or
    // leave once every item has finished and every chunk was taken (a sub-search still
    // running then belongs to a finished item, and stops at its next poll)
    auto fr_take = [&]() {
        const uint64_t wb = __ballot(C_PH(ctl) == PH_WAIT);
        if (!wb) return;
        const ColdArgs r = cold_args();
        const int leader = __ffsll((unsigned long long)wb) - 1;
        unsigned long long t0 = 0;
        uint32_t k = 0, fin = 0;
        if (lane == leader) {
            const unsigned long long want = (unsigned long long)__popcll(wb);
            unsigned long long tk = __hip_atomic_load(&r->fr_c[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long rs = __hip_atomic_load(&r->fr_c[9], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tk < rs) {
                for (int tries = 0; tries < 4 && tk < rs; ++tries) {     // (lost races: the next poll)
                    const unsigned long long kk = rs - tk < want ? rs - tk : want;
                    const unsigned long long w = atomicCAS(&r->fr_c[1], tk, tk + kk);
                    if (w == tk) { t0 = tk; k = (uint32_t)kk; break; }
                    tk = w;
                }
                if (k) atomicSub(&r->fr_c[3], (unsigned long long)k);
            } else if (__hip_atomic_load(&r->fr_c[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >=
                           (unsigned long long)n_jobs * 2ull &&
                       __hip_atomic_load(&r->fr_c[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >=
                           __hip_atomic_load(&r->fr_c[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                // every item has finished (none can offer more) and every reserved chunk was taken
                fin = 1;
                atomicSub(&r->fr_c[3], want);
            }
        }
        t0 = __shfl(t0, leader); k = __shfl(k, leader); fin = __shfl(fin, leader);
        if (C_PH(ctl) == PH_WAIT) {
            const uint32_t rank = (uint32_t)__popcll(wb & ((1ull << lane) - 1ull));
            if (rank < k) help_start(t0 + rank);
            else if (fin) SET_PH(ctl, PH_EXIT);
        }
    };

#ifdef HSA_DIAG
    tt = __builtin_amdgcn_s_memtime();
#endif
    for (;;) {
        ++fr_tick;
        // ---------------- (A) strand ends and read acquisition, batched per wave.
        // The rare steps of a read -- copying its hits out (end_strand), the switch to
        // the forward strand with its row DMA, taking the next read -- are long code
        // paths that the whole wave executes whenever one lane needs one.  A lane that
        // reaches one waits (PH_END / PH_IDLE) and the wave then runs each path once for
        // all waiting lanes, when running it costs less than the waiting has (ski
        // rental): once the waiting lanes have idled batch_idle lane-iterations since
        // the last run (or batch_k lanes wait, or no lane is searching).  Reads that end
        // often (config 2: ~430 pops per read) gather ~16 waiters first; long gapped
        // searches (config 3: ~6 600 pops) run it with a few, instead of idling lanes
        // for hundreds of iterations.
        const uint64_t wm = __ballot(C_PH(ctl) == PH_IDLE || C_PH(ctl) == PH_END);
        idle_acc += (uint32_t)__popcll(wm);
        const bool none_searching = __ballot(C_PH(ctl) != PH_EXIT && C_PH(ctl) != PH_IDLE && C_PH(ctl) != PH_END &&
                                             C_PH(ctl) != PH_WAIT) == 0;
        if (wm && (idle_acc >= a.batch_idle || (uint32_t)__popcll(wm) >= a.batch_k || none_searching)) {
            idle_acc = 0;
            if (C_PH(ctl) == PH_END) end_strand();
            const bool need = C_PH(ctl) == PH_IDLE;
            const uint64_t mb = __ballot(need);
            if (mb) {
                const int leader = __ffsll((unsigned long long)mb) - 1;
                unsigned long long base = 0;
                const ColdArgs r = cold_args();
                if (lane == leader) base = atomicAdd(&r->ctr[r->qctr], (unsigned long long)__popcll(mb));
                base = __shfl(base, leader);
                {
                    const unsigned long long j = base + (unsigned long long)__popcll(mb & ((1ull << lane) - 1ull));
                    const bool got = need && j < (unsigned long long)n_jobs << (r->split ? 1 : 0);
                    if constexpr (FRH) {
                        if (a.fr_budget) {             // the lanes that found the queue empty wait for entries
                            const uint32_t nf = (uint32_t)(__popcll(mb) - __popcll(__ballot(got)));
                            if (lane == leader && nf) atomicAdd(&r->fr_c[3], (unsigned long long)nf);
                        }
                    }
                    if (need) {
                        if (got) begin_item((uint32_t)j);
                        else SET_PH(ctl, (FRH && a.fr_budget) ? PH_WAIT : PH_EXIT);
                    }
                }
            }
            if constexpr (FRH) {
                if (a.fr_budget) fr_take();
            }
        } else if constexpr (FRH) {
            // waiting lanes beside searching ones look for entries every 128 iterations (a poll
            // is a dependent load the whole wave waits for); a wave with none searching, every
            // iteration, after a sleep
            if (a.fr_budget && (none_searching || (fr_tick & 127u) == 64u)) fr_take();
        }
        if (__all(C_PH(ctl) == PH_EXIT)) break;
        if constexpr (FRH) {
            if (a.fr_budget && __ballot(C_PH(ctl) != PH_WAIT && C_PH(ctl) != PH_EXIT) == 0) {
#pragma unroll
                for (int z = 0; z < 4; ++z) __builtin_amdgcn_s_sleep(127);
            }
        }

#ifdef HSA_DIAG
        TMARK(0);
#endif
        // ---------------- (B) control until a rank step is needed
        // req: 1 a rank pair at rp1, rp2
        int req = 0;
        IT rp1 = 0, rp2 = 0;
#ifdef HSA_DIAG
        if (lane == 0) DC(5);
#endif
        // One control pass per iteration: a lane whose pop needs no rank step (pruned,
        // hit, strand change) just skips this iteration's step instead of making the whole
        // wave run the control code again.
        if (C_PH(ctl) != PH_EXIT && C_PH(ctl) != PH_IDLE && C_PH(ctl) != PH_END && C_PH(ctl) != PH_WAIT) do {
#ifdef HSA_DIAG
            { const uint64_t em = __ballot(1); if (lane == __ffsll((unsigned long long)em) - 1) DC(7); }
#endif
            if (C_OVF(ctl)) {
                if constexpr (FRH) {
                    if (frs & 2u) {       // a sub-search outgrew the lane: no proof, the owner searches on
                        atomicOr(&cold_args()->fr_st[fr_key()], FR_HIT);
                        help_done();
                        break;
                    }
                }
                if (C_OVF(ctl) > 1) atomicAdd(&cold_args()->ctr[CTR_ERRORS], 1ull);
                finish_job(HSA_F_OVERFLOW, 0, 0);
                break;
            }
            const uint32_t ph = C_PH(ctl);
            if (ph == PH_EXACT) {
                if constexpr (IMP) {
                    // an exact tail inside the implicit levels (the string so far has
                    // len - 1 - pos characters, ik is its node): the bases up to level sdc
                    // are appended here, without a load (the reference issues the two
                    // queries of each), and the level-sdc node's interval comes from the
                    // table in (C); the rank steps go on from there.  len > sdc: pos stays > 0.
                    const uint32_t len = (uint32_t)C_LEN(ctl);
                    if (len > a.sdc && len - 1u - pos < a.sdc) {
                        uint32_t c;
                        for (;;) {
                            c = getc((int)pos);
                            if (c > 3) break;                                 // 2BWT-Interface.c:377
                            ik = ik * 4u + c;
                            st_q += 2u;
                            if (len - pos == a.sdc) break;
                            --pos;
                        }
                        if (c > 3) { SET_PH(ctl, PH_POP); continue; }
                        req = 3; rp1 = ik;
                        break;
                    }
                }
                if constexpr (F::NIB) {
                    // the rank step goes out with the base load; an N (c > 3) drops it in (D)
                    cur_c = getc((int)pos);
                    req = 1; rp1 = ik; rp2 = il + 1u;
                    break;
                }
                const uint32_t c = getc((int)pos);
                if (c > 3) { SET_PH(ctl, PH_POP); continue; }              // 2BWT-Interface.c:377
                req = 1; rp1 = ik; rp2 = il + 1u;
                break;
            }
            // PH_POP: bwtgap.c:144-186
            if (n_entries == 0 || n_entries > RG(max_entries)) { SET_PH(ctl, PH_END); continue; }
            if constexpr (FRH) {
                // helpers, every 16 pops of a strand: a sub-search stops once its item is decided
                // (a hit, or its owner ended); an owner whose offered entries have all been
                // searched without a hit has its answer -- no hit -- and its work: what it did
                // before the offer plus its sub-searches'.  Every 64 pops past fr_budget, a strand
                // with no hit yet offers its entries while more lanes wait than entries do.
                // (the polls run on the wave's iteration count, so that all its lanes load
                // together: a lane's own cadence made some lane of the wave wait on a load
                // nearly every iteration)
                const uint32_t ps = st_p - fr_p0;
                if (a.fr_budget && (fr_tick & 31u) == 0u) {
                    const ColdArgs r = cold_args();
                    bool stop = false;
                    if (frs & 3u) {
                        const uint32_t key = fr_key();
                        const uint32_t sv = __hip_atomic_load(&r->fr_st[key], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (frs & 2u) {
                            stop = (sv & (FR_HIT | FR_DONE)) != 0u;
                        } else if (sv == 0u && n_aln == 0) {
                            st_q = fr_q0 + (uint32_t)atomicAdd(&r->fr_q[key], 0ull);
                            st_p = fr_p0 + (uint32_t)atomicAdd(&r->fr_p[key], 0ull);
                            atomicAdd(&r->fr_c[7], 1ull);
                            stop = true;
                        }
                    }
                    // one offer per wave per 64 iterations, by its first eligible lane (an offer
                    // walks the lane's lists: the wave waits for it)
                    const bool elig = !stop && !(frs & 5u) && n_aln == 0 && !C_OVF(ctl) && n_entries > 1 &&
                                      n_entries <= (int)FR_WALK && ps >= a.fr_budget && (fr_tick & 63u) == 0u;
                    const uint64_t em = __ballot(elig);
                    if (elig && lane == __ffsll((unsigned long long)em) - 1) {
                        const unsigned long long wt = __hip_atomic_load(&r->fr_c[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const unsigned long long rs = __hip_atomic_load(&r->fr_c[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const unsigned long long tk = __hip_atomic_load(&r->fr_c[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (wt > rs - tk + a.fr_demand) {     // more lanes wait than chunks do
                            if (!fr_offer()) frs |= 4u;
                            else if (frs & 2u) stop = true;      // a helper hands its rest on and ends
                            else { frs |= 1u; fr_p0 = st_p; fr_q0 = st_q; }
                        }
                    }
                    if (stop) { SET_PH(ctl, PH_END); continue; }
                }
            }
            if (C_VT(ctl)) {
                DC(3);
                ctl &= ~(1u << 6);                                        // e already holds it
            } else {
                DC(4);
                // pop the head of the lowest non-empty bucket
                const int b = mask.lowest();
                const uint32_t slot = HEAD(b);
                uint32_t nx;
                if constexpr (LK) {
                    e = ent_load_link<IT>(a.pool, pbase, slot, nx);
                } else {
                    e = ent_load<IT>(a.pool, pbase, slot);
                    nx = NXT(slot);
                }
                if (nx == NIL) mask.reset(b);
                else HEAD(b) = (LT)nx;
                if (HUGE) { NXT(slot) = (LT)free_head; free_head = slot; }
            }
            --n_entries;
            ++st_p;
            const uint32_t m = e.w;
            if (!(R_MODE & MODE_NONSTOP) && SCORE(M_MM(m), M_GO(m), M_GE(m)) > best_score + S_MM) {
                SET_PH(ctl, PH_END);
                continue;
            }
            const int em = m_of(m);
            if (em < 0) { DC(18); continue; }
            const int ei = M_I(m);
            if (ei > 0 && em < (int)(wbg(ei - 1) & F::BIDM)) { DC(18); continue; }
            if (ei == 0) {
                DC(20);
                if (!on_hit(e.x, e.y, e.z, e.z + (e.y - e.x)) && !C_OVF(ctl)) SET_PH(ctl, PH_END);
                continue;
            }
            if (em == 0 && (M_ST(m) == ST_M || (R_MODE & MODE_GAPE) || M_GE(m) == R_MAXGE)) {
                ik = e.x; il = e.y; aux = e.z + (e.y - e.x); pos = (uint32_t)(ei - 1);   // bwt_match_exact
                SET_PH(ctl, PH_EXACT);
                continue;
            }
            req = 1; rp1 = e.x; rp2 = e.y + 1u;
            if constexpr (IMP) {
                // an implicit entry (node e.x, fewer than sdc characters): its children are
                // nodes too and need no load (req 4), or, on level sdc, come with their
                // intervals from the node's table sector (req 2)
                const uint32_t len = (uint32_t)C_LEN(ctl), dp = len - (uint32_t)ei;
                if (len > a.sdc && dp < a.sdc) req = dp + 1u == a.sdc ? 2 : 4;
            }
            if constexpr (F::NIB) cur_c = getc(ei - 1);                  // the expansion's base (D)
            SET_PH(ctl, PH_EXPAND);
        } while (0);

#ifdef HSA_DIAG
        TMARK(1);
#endif
        // ---------------- (C) the rank step
        IT oa[4], ob[4], srk[4];
#ifdef HSA_DIAG
        {
            const uint64_t rq = __ballot(req == 1);
            if (lane == 0) dc[6] += (uint32_t)__popcll(rq);
            const uint32_t ph0 = C_PH(ctl);
            if (req == 1) DC(ph0 == PH_EXACT ? 1 : 2);
            if (req == 1 && rp2 == rp1 + 1u) DC(ph0 == PH_EXACT ? 16 : 17);
        }
#endif
        uint32_t two = 0;
#ifdef HSA_DIAG
        rd_steps += req == 1 ? 1u : 0u;
#endif
        if constexpr (IMP) {
            // the implicit levels' table loads, issued ahead of the other lanes' rank loads
            // so that the wave waits for both at once
            if (req == 2) {
                trie_s_load4(a.stw, rp1, oa, ob, srk);
            } else if (req == 3) {
                trie_s_load1(a.stw, rp1, oa[0], ob[0], srk[0]);
            }
        }
        if (req == 1) {
            two = occ_pair(Ix<IT>::fwd(a), rp1, rp2, oa, ob) - 1u;
            st_q += 2u; st_b += 1u + two;
        }

#ifdef HSA_DIAG
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        TMARK(2);
#endif
        // ---------------- (D) apply
        const uint32_t ph = C_PH(ctl);
        if (IMP && req == 3) {
            // the exact tail leaves the implicit levels: the level-sdc node's interval.  The
            // write-back guard below tests which fields of the entry the tail started from
            // are zero.  That entry has fewer than sdc characters, so it is on a complete
            // level, and of a string on a complete level none is (the builder checks
            // k >= 1 and rev_k >= 1, and l >= k, rev_l >= rev_k), so a node entry gets
            // non-zero fields here; the root keeps its own, {0, T, 0}.
            // Level sdc itself may lack the string (k > l in the table): the tail ends as
            // bwt_match_exact does on an empty interval (2BWT-Interface.c:378-382), without a
            // hit; the failing step's two queries are counted by the appending loop.
            ik = oa[0]; il = ob[0]; aux = srk[0] + (il - ik);
            if (M_I(e.w) != C_LEN(ctl)) e.x = e.y = e.z = 1u;
            --pos;
            if (ik > il) SET_PH(ctl, PH_POP);
        } else if (F::NIB && req == 1 && ph == PH_EXACT && cur_c > 3) {
            st_q -= 2u; st_b -= 1u + two;                                // not a step (2BWT-Interface.c:377)
            SET_PH(ctl, PH_POP);
        } else if (req && ph == PH_EXACT) {
            // BWTSARangeBackward_Bidirection (2BWT-Interface.c:135-170), one character
            const uint32_t c = F::NIB ? cur_c : getc((int)pos);
            IT oc = 0;
#pragma unroll
            for (uint32_t d = 1; d < 4; ++d) oc += d > c ? ob[d] - oa[d] : (IT)0;
            const IT cc = pick4(CC, c);
            ik = cc + pick4(oa, c) + 1u;
            il = cc + pick4(ob, c);
            aux -= oc;                                                   // rev_l
            if (ik > il) {
                SET_PH(ctl, PH_POP);                                     // no match: continue (bwtgap.c:185)
            } else if (pos-- == 0) {
                // write-back guard of bwt_match_exact (2BWT-Interface.c:383-386)
                const IT rk = aux - (il - ik), erl = e.z + (e.y - e.x);
                const IT hk = e.x ? ik : (IT)0, hl = e.y ? il : (IT)0, hrk = e.z ? rk : (IT)0, hrl = erl ? aux : (IT)0;
                SET_PH(ctl, PH_POP);
                if (!on_hit(hk, hl, hrk, hrl) && !C_OVF(ctl)) SET_PH(ctl, PH_END);
            }
        } else if (req && ph == PH_EXPAND) {
            // children of the bidirectional step (2BWT-Interface.c:235-272), in place:
            // oa -> k, ob -> l of child c; srk = rev_k
            const uint32_t m = e.w;
            const IT ek = e.x, el = e.y, erk = e.z, erl = erk + (el - ek);
            const int i = M_I(m) - 1;                                    // --i (bwtgap.c:245)
            const int est = M_ST(m), emm = M_MM(m), ego = M_GO(m), ege = M_GE(m);
            const int em = m_of(m);
            const int len = C_LEN(ctl);
            uint32_t ne = 0;                                             // children that occur
            if (IMP && req != 1) {
                // implicit levels: the children are the nodes 4 p + c, all four of which
                // occur (req 4), or the table's level-sdc intervals, already in oa, ob, srk
                // (req 2), of which a string that does not occur has k > l as a rank step
                // gives it.  The reference issues the step's two queries.
                ne = 0xFu;
                if (req == 4) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) { oa[c] = ek * 4u + (IT)c; ob[c] = 0; srk[c] = 0; }
                } else {
                    ne = 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) ne |= (oa[c] <= ob[c] ? 1u : 0u) << c;
                }
                st_q += 2u;
            } else {
                IT oc = 0;
#pragma unroll
                for (int c = 3; c >= 0; --c) {
                    const IT d = ob[c] - oa[c];
                    oa[c] = CC[c] + oa[c] + 1u;
                    ob[c] = CC[c] + ob[c];
                    srk[c] = (erl - oc) - (ob[c] - oa[c]);
                    oc += d;
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) ne |= (oa[c] <= ob[c] ? 1u : 0u) << c;
            }
            int allow_diff = 1, allow_M = 1;
            if (i > 0) {
                // width[i-1].bid, width[i].bid and w[i-1] == w[i] (bwtgap.c:256-258)
                const uint32_t w1 = wbg(i - 1), w0 = wbg(i);
                const int b1 = (int)(w1 & F::BIDM), b0 = (int)(w0 & F::BIDM);
                if (b1 > em - 1) allow_diff = 0;
                else if (b1 == em - 1 && b0 == em - 1 && (w1 & F::EQ)) allow_M = 0;
                const int ii = i - (len - C_SLEN(ctl));
                if (C_SEED(ctl) && ii > 0) {
                    int ems = RG(max_seed_diff) - (emm + ego);
                    if (R_MODE & MODE_GAPE) ems -= ege;
                    // width_seed aliased to width_back (bwtgap.c:809): the same LDS row
                    // (never in the mixed format: caller-width passes keep byte rows)
                    const bool alias = !SN && C_ALIAS(ctl);
                    const uint32_t s1 = alias ? wbg(ii - 1) : wsg(ii - 1);
                    const uint32_t s0 = alias ? wbg(ii) : wsg(ii);
                    const int c1 = (int)(s1 & FS::BIDM), c0 = (int)(s0 & FS::BIDM);
                    if (c1 > ems - 1) allow_diff = 0;
                    else if (c1 == ems - 1 && c0 == ems - 1 && (s1 & FS::EQ)) allow_M = 0;
                }
            }
            // The pushes of bwtgap.c:267-325 as a candidate mask in push order:
            // bit 0 insertion, bits 1-4 deletion with child j = bit-1, bits 5-8
            // match/mismatch with child (seq[i] + bit-4) & 3.  All but the last go to the
            // pool in order; the last becomes the virtual top when it is the next pop.
            const uint32_t sc = F::NIB ? cur_c : getc(i);
            // (as selects over every case: nested ifs here were divergent branches)
            uint32_t cand = 0;
            if constexpr (GAPS) {
                const int ies = RG(indel_end_skip);
                const int tmp = (R_MODE & MODE_LOGGAP) ? hsa_log2((uint32_t)(ege + ego)) / 2 + 1 : ego + ege;
                const bool ok = (allow_diff != 0) & ((R_MAXGO > 0) | (ego > 0)) & (i >= ies + tmp) & (len - i >= ies + tmp);
                const IT occ = el - ek + 1u;
                const uint32_t c_m = ego < R_MAXGO ? (1u | ne << 1) : 0u;
                const uint32_t c_i = ege < R_MAXGE ? 1u : 0u;
                const bool d_ok = (ege < R_MAXGE) & ((ege + ego < max_diff) | (occ < (IT)RG(max_del_occ)));
                const uint32_t c_d = d_ok ? ne << 1 : 0u;
                const uint32_t c_g = est == ST_M ? c_m : est == ST_I ? c_i : c_d;
                cand = ok ? c_g : 0u;
            }
            {
                uint32_t c_mm = 0;
#pragma unroll
                for (int j = 1; j <= 4; ++j) {
                    const uint32_t c = (sc + (uint32_t)j) & 3u;
                    c_mm |= ((ne >> c) & 1u) << (4 + j);
                }
                const uint32_t c_eq = sc < 4 ? ((ne >> (sc & 3u)) & 1u) << 8 : 0u;   // == bit 8: c = sc, no mismatch
                cand |= (allow_diff & allow_M) ? c_mm : c_eq;
            }
            // entry of candidate bit b
            auto entry = [&](uint32_t b) -> E {
                const bool ins = GAPS && b == 0, del = GAPS && b >= 1 && b <= 4;
                const uint32_t c = del ? b - 1u : (sc + b - 4u) & 3u;
                const uint32_t is_mm = (b != 8u || sc > 3) ? 1u : 0u;
                IT k = pick4(oa, c), l = pick4(ob, c), rk = pick4(srk, c);
                uint32_t meta;
                if (GAPS && (ins || del)) {
                    if (ins) { k = ek; l = el; rk = erk; }
                    const uint32_t go = (uint32_t)ego + (est == ST_M), ge = (uint32_t)ege + (est != ST_M);
                    meta = meta_pack((uint32_t)(del ? i + 1 : i), ins ? ST_I : ST_D, 1u, (uint32_t)emm, go, ge);
                } else {
                    meta = meta_pack((uint32_t)i, ST_M, is_mm, (uint32_t)emm + is_mm, (uint32_t)ego, (uint32_t)ege);
                }
                return E{k, l, rk, meta};
            };
#ifdef HSA_DIAG
            // pushes whose pop would be pruned under the current max_diff and bids
            auto doomed = [&](uint32_t mw) {
                const int em2 = m_of(mw), i2 = M_I(mw);
                return em2 < 0 || (i2 > 0 && em2 < (int)(wbg(i2 - 1) & F::BIDM));
            };
#endif
            if (cand) {
                const uint32_t last = 31u - (uint32_t)__clz(cand);
                n_entries += __popc(cand);
                uint32_t rest = cand & ~(1u << last);
                if constexpr (HUGE) {
                    for (; rest; rest &= rest - 1u) {
                        const E v = entry((uint32_t)__ffs(rest) - 1u);
#ifdef HSA_DIAG
                        if (doomed(v.w)) DC(19);
#endif
                        flush(v, bucket_of(v.w));
                    }
                } else if (rest) {
                    // Every candidate but the last, in push order (gap_push, bwtgap.c:46-75),
                    // with each group's meta word and bucket computed once: the insertion
                    // and the deletions share one score, the mismatches another, the bit-8
                    // match child has the parent's.  The groups' bucket heads are kept in
                    // registers across the loop (equal buckets updated together, so the
                    // links are flush()'s) and written back once: the divergent loop does
                    // one store per candidate (two with a link array) and no LDS round trip.
                    const uint32_t g_go = (uint32_t)ego + (est == ST_M), g_ge = (uint32_t)ege + (est != ST_M);
                    const uint32_t mI = meta_pack((uint32_t)i, ST_I, 1u, (uint32_t)emm, g_go, g_ge);
                    const uint32_t mD = meta_pack((uint32_t)(i + 1), ST_D, 1u, (uint32_t)emm, g_go, g_ge);
                    const uint32_t mM = meta_pack((uint32_t)i, ST_M, 1u, (uint32_t)emm + 1u, (uint32_t)ego, (uint32_t)ege);
                    const uint32_t mP = meta_pack((uint32_t)i, ST_M, 0u, (uint32_t)emm, (uint32_t)ego, (uint32_t)ege);
                    const int bG = GAPS ? bucket_of(mI) : -1, bM = bucket_of(mM), bP = bucket_of(mP);
                    auto head0 = [&](int b) -> uint32_t {
                        return b >= 0 && (uint32_t)b < a.nb && mask.test(b) ? (uint32_t)HEAD(b) : NIL;
                    };
                    const uint32_t hG0 = GAPS ? head0(bG) : NIL, hM0 = head0(bM), hP0 = head0(bP);
                    uint32_t hG = hG0, hM = hM0, hP = hP0;
                    for (; rest; rest &= rest - 1u) {
                        const uint32_t b = (uint32_t)__ffs(rest) - 1u;
                        const bool ins = GAPS && b == 0, gap = GAPS && b <= 4u;
                        const bool mt = b == 8u && sc < 4;               // the match child
                        const uint32_t c = gap ? b - 1u : (sc + b - 4u) & 3u;
                        IT k = pick4(oa, c), l = pick4(ob, c), rk = pick4(srk, c);
                        if (ins) { k = ek; l = el; rk = erk; }
                        const uint32_t meta = ins ? mI : gap ? mD : mt ? mP : mM;
                        const int bk = gap ? bG : mt ? bP : bM;
#ifdef HSA_DIAG
                        if (doomed(meta)) DC(19);
#endif
                        if ((uint32_t)bk >= a.nb || pool_top >= a.pcap) { ctl |= 1u << 8; continue; }
                        const uint32_t slot = pool_top++;
                        DC(8);
                        if constexpr (LK) {
                            ent_store_link<IT>(a.pool, pbase, slot, E{k, l, rk, meta}, bk == bG ? hG : bk == bM ? hM : hP);
                        } else {
                            ent_store<IT>(a.pool, pbase, slot, E{k, l, rk, meta});
                            NXT(slot) = (LT)(bk == bG ? hG : bk == bM ? hM : hP);
                        }
                        hG = bk == bG ? slot : hG;
                        hM = bk == bM ? slot : hM;
                        hP = bk == bP ? slot : hP;
                    }
                    if (GAPS && hG != hG0) { HEAD(bG) = (LT)hG; mask.set(bG); }
                    if (hM != hM0) { HEAD(bM) = (LT)hM; mask.set(bM); }
                    if (hP != hP0) { HEAD(bP) = (LT)hP; mask.set(bP); }
                }
                const E v = entry(last);
#ifdef HSA_DIAG
                if (doomed(v.w)) DC(19);
#endif
                const int bk = bucket_of(v.w);
                if (bk <= mask.lowest()) { e = v; ctl |= 1u << 6; }
                else flush(v, bk);
            }
            SET_PH(ctl, PH_POP);
        }
#ifdef HSA_DIAG
        TMARK(3);
#endif
    }

#ifdef HSA_DIAG
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < 8192) {
        g_diag[blockIdx.x * 4 + 2] = __builtin_amdgcn_s_memtime();
        g_diag[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memrealtime();
    }
    for (int i = 0; i < 18; ++i)
        if (i < 9 || i > 12) atomicAdd(&g_dctr[i], (unsigned long long)dc[i]);
    for (int i = 18; i < 21; ++i) atomicAdd(&g_dctr[i], (unsigned long long)dc[i]);
    if (lane == 0)
        for (int i = 0; i < 4; ++i) atomicAdd(&g_dctr[9 + i], (unsigned long long)tsec[i]);
#endif
    // statistics
    if constexpr (FRH) {
        if (a.fr_budget) {
            unsigned long long hs = st_hs, hq = st_hq;
            for (int d = 32; d >= 1; d >>= 1) { hs += __shfl_xor(hs, d); hq += __shfl_xor(hq, d); }
            if (lane == 0) { atomicAdd(&a.fr_c[6], hs); atomicAdd(&a.fr_c[8], hq); }
        }
    }
    atomicAdd(&a.ctr[CTR_RANK], (unsigned long long)st_q);
    atomicAdd(&a.ctr[CTR_SECTORS], (unsigned long long)st_b);
    atomicAdd(&a.ctr[CTR_POPS], (unsigned long long)st_p);
    if (st_wq) {
        atomicAdd(&a.ctr[CTR_RANK], (unsigned long long)st_wq);
        atomicAdd(&a.ctr[CTR_WIDTH_Q], (unsigned long long)st_wq);
        atomicAdd(&a.ctr[CTR_FWD_Q_REF], (unsigned long long)st_wq);
    }
#undef HEAD
#undef WB
#undef WS
#undef NXT
#undef HB
#undef RG
#undef S_MM
#undef S_GO
#undef S_GE
#undef R_MODE
#undef R_MAXGO
#undef R_MAXGE
#undef SCORE
}

#include "hsa_search_any.h"

// jobs up to fast_max bases go to k_search's list, longer ones to k_search_any's
static __global__ void __launch_bounds__(BLOCK) k_partition(const hsa_job_t *jobs, int n, uint32_t fast_max,
                                                            int32_t *l_fast, int32_t *l_any, unsigned long long *cnt)
{
    const int j = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (j >= n) return;
    if (jobs[j].len <= fast_max) l_fast[atomicAdd(&cnt[0], 1ull)] = j;
    else l_any[atomicAdd(&cnt[1], 1ull)] = j;
}
