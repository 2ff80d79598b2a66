// hsa_sa.h -- SA index -> text position on the device, shared by
// k_sa_position (hsa_sa.hip) and the splice path's kernel (hsa_splice.hip).
//
// BWTSaValue (BWT.c:1195-1220) walks LF (BWTPsiMinusValue, BWT.c:1142-1162, via
// BWTOccValueOnSpot, BWT.c:924-959) until the SA index is a multiple of the sampling
// interval, then adds the steps to the sampled value; BWTRetrievePositionFromSAIndex
// (2BWT-Interface.c:329-361) then binary-searches the chromosome block table for
// (chrID, 1-based position).  Every LF step is one 16-byte rank-block load (the
// character before the position and its count come from the same block).
#pragma once
#include "hsa_device.h"

struct SaView {
    const uint4 *blk;              // forward rank blocks
    uint32_t isa0;
    uint32_t C[4];
    const uint32_t *sa;            // sampled values; sa[0] = -1 as BWTLoad leaves it (BWT.c:222)
    uint32_t interval;
    const uint32_t *blocks;        // n_blocks rows (chrID, blockStart, blockEnd, ori), HSP.h:41-46
    uint32_t n_blocks;
};

// BWTPsiMinusValue: the LF map of SA index `index` (index != inverseSa0).
__device__ __forceinline__ uint32_t hsa_psi_minus(const SaView &a, uint32_t index)
{
    uint32_t i = index + 1u;
    i -= (i > a.isa0);                         // BWTOccValueOnSpot: '$' is not encoded (BWT.c:949)
    const uint32_t p = i - 1u;                 // the BWT character before i ...
    const uint4 q = a.blk[p >> 4];
    const uint32_t r = p & 15u;
    const uint32_t c = (q.w >> (2u * r)) & 3u;
    const uint32_t x = q.w ^ ~(c * 0x55555555u);
    const uint32_t n = __popc(x & (x >> 1) & 0x55555555u & ((1u << (2u * r)) - 1u));
    const uint32_t base = hsa_sel4(c, q.x, q.y, q.z, (p & ~15u) - q.x - q.y - q.z);
    const uint32_t cc = hsa_sel4(c, a.C[0], a.C[1], a.C[2], a.C[3]);
    return cc + base + n + 1u;                 // ... and its count up to and including it
}

// BWTSaValue: the text position of SA index `index`.
__device__ __forceinline__ uint32_t hsa_sa_value(const SaView &a, uint32_t index)
{
    uint32_t skipped = 0;
    while (index % a.interval != 0) {
        ++skipped;
        index = index == a.isa0 ? 0u : hsa_psi_minus(a, index);
    }
    return a.sa[index / a.interval] + skipped;
}

// The block search of BWTRetrievePositionFromSAIndex (h starts at nblock; where the
// reference would read past the table -- m >= nblock -- it stops as "not found", see
// oracle/hsa_oracle.c).  Returns whether a block holds occ; sid / ori only then.
__device__ __forceinline__ bool hsa_sa_block(const SaView &a, uint32_t occ, uint32_t &sid, uint32_t &ori)
{
    uint32_t l = 0, h = a.n_blocks;
    while (l <= h) {
        const uint32_t m = (h + l) >> 1;
        if (m >= a.n_blocks) break;
        const uint32_t start = a.blocks[4 * m + 1];
        if (start > occ) { h = m - 1u; continue; }
        const uint32_t end = a.blocks[4 * m + 2];
        if (end < occ) { l = m + 1u; continue; }
        sid = a.blocks[4 * m];
        ori = occ - start + a.blocks[4 * m + 3] + 1u;
        return true;
    }
    return false;
}

// ---------------------------------------------------------------- 64-bit texts
// The same walk for an index of hsa_index_create_device64 (no reference counterpart:
// bwtint_t is 32-bit).  SA values, rows, the '$' row and the C table are 64-bit; the
// rank blocks keep their counts modulo 2^32 and RankDir64's wrap table supplies the high
// words (hsa_device.h), read only under its uniform `any` branch.  One LF step stays one
// 16-byte block load.  The blocks are rows of four u64.
struct SaView64 {
    RankDir64 d;                   // forward rank blocks, '$' row, wrap flag
    uint64_t T;
    uint64_t C[4];
    const uint64_t *sa;            // sampled values; sa[0] (the '$' row) is the caller's
    uint32_t interval;
    uint32_t pow2, shift;          // the interval is a power of two: 2^shift
    uint32_t n_blocks;
    const uint64_t *blocks;        // n_blocks rows (chrID, blockStart, blockEnd, ori)
    uint32_t max_walk;             // LF steps after which a walk is given up (HSA_SA_MAX_WALK)
};

#define HSA_SA64_NONE 0xFFFFFFFFFFFFFFFFull
#define HSA_ALN64_WORDS 14u                    // hsa_aln64_t: k at words 2-3, l at words 4-5

// rows k .. l of a hit record of the 64-bit search (none for a malformed one)
__device__ __forceinline__ uint64_t hsa_aln64_rows(const uint32_t *__restrict__ rec, uint64_t &k)
{
    const uint2 kw = *reinterpret_cast<const uint2 *>(rec + 2), lw = *reinterpret_cast<const uint2 *>(rec + 4);
    k = (uint64_t)kw.x | ((uint64_t)kw.y << 32);
    const uint64_t l = (uint64_t)lw.x | ((uint64_t)lw.y << 32);
    return l >= k ? l - k + 1u : 0u;
}

// index % interval without a 64-bit division where the interval is a power of two (a
// uniform branch: the usual intervals are)
__device__ __forceinline__ uint32_t hsa_sa_rem64(const SaView64 &a, uint64_t index)
{
    return a.pow2 ? ((uint32_t)index & (a.interval - 1u)) : (uint32_t)(index % a.interval);
}

// The LF map of SA index `index` (index != isa0, index <= T).
__device__ __forceinline__ uint64_t hsa_psi_minus64(const SaView64 &a, uint64_t index)
{
    uint64_t i = index + 1u;
    i -= (i > a.d.isa0);                       // '$' is not encoded
    const uint64_t p = i - 1u;                 // the BWT character before i ...
    const uint4 q = a.d.blk[p >> 4];
    const uint32_t c = (q.w >> (2u * ((uint32_t)p & 15u))) & 3u;
    const uint64_t cc = hsa_sel4(c, a.C[0], a.C[1], a.C[2], a.C[3]);
    return cc + hsa_occ1_q64(q, a.d, p, c) + 1u;   // ... and its count up to and including it
}

// The text position of SA index `index` (<= T); false when the walk took more than
// max_walk steps (a sampled array that does not belong to this BWT).  The walk ends at a
// sampled row or at row isa0, the suffix at position 0: the 32-bit walk steps on from
// there to row 0 and relies on sa[0] = -1; here sa[0] stays the caller's (SA = T).
__device__ __forceinline__ bool hsa_sa_value64(const SaView64 &a, uint64_t index, uint64_t &value)
{
    uint32_t skipped = 0;
    while (hsa_sa_rem64(a, index) != 0) {
        if (index == a.d.isa0) { value = skipped; return true; }
        if (skipped >= a.max_walk) return false;
        ++skipped;
        index = hsa_psi_minus64(a, index);
    }
    value = a.sa[a.pow2 ? index >> a.shift : index / a.interval] + skipped;
    return true;
}

// hsa_sa_block on 64-bit fields: the same search, the same m >= n_blocks stop.
__device__ __forceinline__ bool hsa_sa_block64(const SaView64 &a, uint64_t occ, uint64_t &sid, uint64_t &ori)
{
    uint32_t l = 0, h = a.n_blocks;
    while (l <= h) {
        const uint32_t m = (h + l) >> 1;
        if (m >= a.n_blocks) break;
        const uint64_t start = a.blocks[4 * (size_t)m + 1];
        if (start > occ) { h = m - 1u; continue; }
        const uint64_t end = a.blocks[4 * (size_t)m + 2];
        if (end < occ) { l = m + 1u; continue; }
        sid = a.blocks[4 * (size_t)m];
        ori = occ - start + a.blocks[4 * (size_t)m + 3] + 1u;
        return true;
    }
    return false;
}

// One output row (SA value, chrID, 1-based position, text position) of SA index `index`;
// all-ones in all four words for an index past T or a walk cut by the bound (returns
// false for the latter).
__device__ __forceinline__ bool hsa_sa_row64(const SaView64 &a, uint64_t index, uint64_t *out)
{
    uint64_t occ = HSA_SA64_NONE, sid = HSA_SA64_NONE, ori = HSA_SA64_NONE;
    const bool ok = index <= a.T && hsa_sa_value64(a, index, occ);
    if (ok) hsa_sa_block64(a, occ, sid, ori);
    else occ = HSA_SA64_NONE;
    reinterpret_cast<ulonglong2 *>(out)[0] = make_ulonglong2(occ, sid);
    reinterpret_cast<ulonglong2 *>(out)[1] = make_ulonglong2(ori, occ);
    return ok || index > a.T;
}
