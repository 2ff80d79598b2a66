// hsa_splice_rows.hip -- the SAM lines of spliced reads, from hsa_splice_device's results.
//
// Restates what the reference does with a read whose bwt_splice_match result is two records
// of type BWA_TYPE_SPLICING, after the search:
//   bwt_aln2pos_splicing (bwtse.c:295-348) with bwt_combine_segment_splice (:197-235),
//   the splicing branch of bwa_refine_gapped (:562-595, over refine_gapped_core :380-440),
//   the XT:A:S line of bwa_print_sam1 (:677-799).
// hsa_amd/splice.py: pair_segments / merge_cigar and hsa_amd/sam.py: spliced_line say the
// same in Python; the tests hold this file to them and to the reference's SAM files.
//
// hsa_splice_lines_device is four launches and a scan on one stream, no host round trip:
//   k_sl_pair   one wavefront per read.  Lanes along the rows of both segments (at most 50
//               each): a lane walks its row's SA index to a text position (hsa_sa.h, the
//               dependent-load part) and finds its chromosome block.  The rows are then
//               sorted by text position, each lane ranking its rows against all of them in
//               LDS, and the reference's combine loop runs over the sorted rows, the same
//               in every lane.  The chosen pair becomes two rows of a refine batch (slots
//               2 j and 2 j + 1 of read j; all-ones rows for a read without a pair).
//   k_refine_rows, k_refine_dp (hsa_refine.hip) with every row aligned: the alignment is
//               shared with the unspliced path by running its kernels, not by a copy.
//   k_sl_len    one lane per read: the end rules' results, the N length, the merged CIGAR,
//               the read's status and the exact length of its line.
//   rocPRIM exclusive scan of the lengths in read order: d_line_off.  No atomic places a
//               byte, so two runs give equal arrays.
//   k_sl_write  one wavefront per read: lane 0 formats the small fields, the lanes copy
//               name, SEQ and QUAL along the bytes.
// sl_emit walks the fields of a line for both kernels (a sink that counts, one that stores:
// hsa_sam_sinks.h).
//
// hsa_splice_lines_device_xa adds the XA:Z list of a read with several pairs at the shortest
// distance (bwtse.c:596-618, :782-797; hsa_amd/splice.py: multi_entries).  The plain entry
// points give such a read HSA_SL_MULTI; with an hsa_splice_xa_t:
//   k_sl_pair   also leaves each read's extra pairs (n_res - 1) in a count array;
//   a scan      gives d_pair_off; reads are served in read order while their pairs fit the room;
//   k_sl_room   blanks the extra refine rows (slots 2 n + 2 e, 2 n + 2 e + 1 of extra pair e);
//   k_sl_fill   one wavefront per read, leaving at once without extra pairs: the SA walks, the
//               sort and the combine loop again (such reads are few: cheaper than keeping every
//               read's sorted rows), then the lanes test the sorted indices behind `first`
//               and number the kept pairs by ballot and prefix popcount, in sorted order;
//   the refinement serves all 2 n + 2 pair_cap rows in its one launch;
//   k_sl_xlen   one lane per extra pair: end rules, N length, merged CIGAR, the entry's bytes;
//   k_sl_len    sums a read's entries (and takes over the first failing pair's status);
//   k_sl_write  lanes format a read's entries side by side (sl_xa_emit, counted and stored
//               by the same function).
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <string.h>

#include "hsa_device.h"
#include "hsa_internal.h"
#include "hsa_sa.h"
#include "hsa_sam_sinks.h"

#define SL_MAX_ROWS 100u           // bwtse.c:312
#define SL_SEG_ROWS 50u            // :320
#define SL_SEG_CIGAR 16u           // ops of one segment's CIGAR
#define SL_TYPE_SPLICING 4u        // bwtaln.h:13
#define SL_MIN_DIST 50u            // bwtse.c:219
#define SL_MAX_DIST 50000u

struct SlArgs {
    SaView sv;
    uint32_t T;                    // SA indices are 0..T
    const hsa_job_t *jobs;
    uint32_t n_jobs;
    const uint8_t *codes;
    const uint32_t *flags;
    const int32_t *n_aln;
    const uint32_t *res;
    const uint8_t *names; const uint64_t *name_off;
    const uint8_t *quals; const uint64_t *qual_off;
    const uint8_t *chr_names; const uint64_t *chr_off;
    uint32_t n_chr, flag;
    int32_t max_top2, comp_read;
    uint32_t max_len, max_line, cigar_stride;
    uint32_t *rows, *cigar;
    const uint32_t *full_len; const uint8_t *bc; uint32_t bc_len;      // hsa_sam_trim_t; null / 0 without
    uint64_t *line_off;
    uint8_t *out;
    uint64_t out_cap;
    uint32_t *stat;
    unsigned long long *ctr;
    // the refine batch of the segments: 2 n_jobs rows, row t its own read t
    hsa_job_t *s_jobs;
    uint64_t *s_hit_off, *s_pos_off, *s_pos, *s_rpos;
    uint32_t *s_hits, *s_pos_hit, *s_rows, *s_cigar;
    uint64_t *lens;                // n_jobs + 1
    // hsa_splice_xa_t (all null / 0 through the plain entry points)
    uint64_t *xcnt;                // n_jobs + 1: extra pairs per read
    uint64_t *pair_off;            // n_jobs + 1
    uint64_t pair_cap;
    uint32_t *prow, *pcigar;
    unsigned long long *xctr;
};

__device__ __forceinline__ void sl_row_words(uint32_t *o, uint32_t st, uint32_t n_rows, uint32_t n_splice, uint32_t c1,
                                             uint32_t strand)
{
    for (uint32_t i = 0; i < HSA_SL_ROW_WORDS; ++i) o[i] = 0u;
    o[0] = st; o[1] = n_rows; o[2] = n_splice; o[3] = c1; o[4] = strand;
}

// A refine row no kernel answers (HSA_RF_POS): the slots of a read without a pair.
__device__ __forceinline__ void sl_no_segment(const SlArgs &a, uint64_t t)
{
    hsa_job_t jb;
    memset(&jb, 0, sizeof jb);
    a.s_jobs[t] = jb;
    a.s_hits[HSA_ALN64_WORDS * t] = 0u;
    a.s_hits[HSA_ALN64_WORDS * t + 1] = 0u;
    for (uint32_t i = 0; i < 4u; ++i) a.s_pos[4 * t + i] = ~0ull;
}

// The rows of one read in LDS: text position, chromosome, 1-based position and whether a
// block holds the row, by row index; ord: the row indices sorted by text position.
struct SlLds {
    uint32_t occ[128], sid[128], ori[128], ord[128];
    uint8_t found[128];
};

// The two records of a spliced result (bwt_aln1_t, 9 words): n_mm | n_gapo | n_gape, k, l,
// rev_k, rev_l, type | strand, start, end, score
struct SlRec {
    uint32_t k0, l0, k1, l1, strand, mm0, mm1, n0, n1, n, c1;
    int32_t s0, e0, s1, e1;
};

// false: a field outside what the layout holds.  Every index used later comes from device
// memory: SA rows within 0..T, the segments within the read, the read within the layout.
__device__ __forceinline__ bool sl_decode(const SlArgs &a, const uint32_t *res, const hsa_job_t &jb, SlRec &r)
{
    const uint32_t *r0 = res + 2, *r1 = res + 11;
    r.k0 = r0[1]; r.l0 = r0[2]; r.k1 = r1[1]; r.l1 = r1[2];
    r.strand = r0[5] >> 30;                                // bwtse.c:307
    r.s0 = (int32_t)r0[6]; r.e0 = (int32_t)r0[7]; r.s1 = (int32_t)r1[6]; r.e1 = (int32_t)r1[7];
    r.mm0 = (r0[0] & 0xFFFFu) + ((r0[0] >> 16) & 0xFFu) + (r0[0] >> 24);
    r.mm1 = (r1[0] & 0xFFFFu) + ((r1[0] >> 16) & 0xFFu) + (r1[0] >> 24);
    const bool ok = r.k0 <= r.l0 && r.l0 <= a.T && r.k1 <= r.l1 && r.l1 <= a.T && r.s0 >= 0 && r.e0 >= r.s0 &&
                    (uint32_t)r.e0 < jb.len && r.s1 >= 0 && r.e1 >= r.s1 && (uint32_t)r.e1 < jb.len && jb.len <= a.max_len &&
                    r.strand < 2u;
    if (!ok) return false;
    r.n0 = r.l0 - r.k0 < SL_SEG_ROWS ? r.l0 - r.k0 + 1u : SL_SEG_ROWS;      // :320
    r.n1 = r.l1 - r.k1 < SL_SEG_ROWS ? r.l1 - r.k1 + 1u : SL_SEG_ROWS;
    r.n = r.n0 + r.n1;
    r.c1 = r.l0 - r.k0 + r.l1 - r.k1 + 2u;                                 // :310-312
    if (r.c1 >= SL_MAX_ROWS) r.c1 = SL_MAX_ROWS;
    return true;
}

// The rows of both segments into LDS, lanes along them, and their order by text position.
__device__ __forceinline__ void sl_rows_sorted(const SlArgs &a, SlLds &L, const SlRec &r, uint32_t lane)
{
    const uint32_t n = r.n, n0 = r.n0;
    for (uint32_t t = lane; t < n; t += 64u) {
        const uint32_t idx = t < n0 ? r.k0 + t : r.k1 + (t - n0);
        const uint32_t occ = hsa_sa_value(a.sv, idx);
        uint32_t sid = 0u, ori = 0u;                       // (calloc'ed rows: they stay 0 where no block holds occ)
        const bool found = hsa_sa_block(a.sv, occ, sid, ori);
        L.occ[t] = occ; L.sid[t] = found ? sid : 0u; L.ori[t] = found ? ori : 0u; L.found[t] = found ? 1u : 0u;
    }
    __syncthreads();
    // qsort_for_bwt (:169-192) sorts by occ_pos.  The rows are distinct SA rows, so their
    // positions are distinct: any correct sort gives the reference's order, and the
    // instability of its hand-written quicksort cannot show.  Here each lane ranks its
    // rows (ties, which cannot occur, by row index: the result is a permutation anyway).
    if (n == 2u) { if (lane < 2u) L.ord[lane] = lane; }     // :204: as they stand
    else
        for (uint32_t t = lane; t < n; t += 64u) {
            const uint32_t key = L.occ[t];
            uint32_t rank = 0;
            for (uint32_t u = 0; u < n; ++u) rank += (L.occ[u] < key || (L.occ[u] == key && u < t)) ? 1u : 0u;
            L.ord[rank] = t;
        }
    __syncthreads();
}

// bwt_combine_segment_splice's loop (:209-232), the same in every lane.  The k-th kept pair
// starts at a sorted index >= 2 (k - 1), so the reference's memmove to multi[2 (n_res - 1)]
// never touches a row the loop has yet to read, and `if (i == 0) continue` skips a move of
// rows 0, 1 onto themselves: pair 0 is the pair at `first`.
__device__ __forceinline__ uint32_t sl_combine(const SlLds &L, uint32_t n0, uint32_t n, uint32_t &first, uint32_t &shortest)
{
    uint32_t n_res = 0;
    first = 0; shortest = 0xFFFFFFFFu;
    if (n == 2u) return 1u;
    for (uint32_t i = 0; i + 1u < n; ++i) {
        const uint32_t x = L.ord[i], y = L.ord[i + 1u];
        if (x >= n0) continue;                             // aln_id != 0
        const uint32_t d = L.occ[y] - L.occ[x];
        if (y < n0 || L.sid[x] != L.sid[y] || d > shortest) continue;
        if (d < SL_MIN_DIST || d > SL_MAX_DIST) continue;
        if (d < shortest) { shortest = d; n_res = 1u; first = i; }
        else ++n_res;                                      // d == shortest
    }
    return n_res;
}

// Behind `first` the shortest distance is final, so the loop above keeps sorted index i
// exactly when this holds: an independent test per index (the distance is within 50..50 000
// because `shortest` is).
__device__ __forceinline__ bool sl_later_pair(const SlLds &L, uint32_t i, uint32_t n0, uint32_t n, uint32_t shortest)
{
    if (i + 1u >= n) return false;
    const uint32_t x = L.ord[i], y = L.ord[i + 1u];
    return x < n0 && y >= n0 && L.sid[x] == L.sid[y] && L.occ[y] - L.occ[x] == shortest;
}

// Segment s of a pair as a refine row of its own (slot t): (strand ? rseq : seq) + start,
// seg_len characters (:569-570).  rf_read_code reverses and complements a strand-1 read, so
// its bytes are the original read's len - 1 - end .. len - 1 - start.
__device__ __forceinline__ void sl_segment(const SlArgs &a, uint64_t t, const hsa_job_t &jb, const SlRec &r, uint32_t s,
                                           const SlLds &L, uint32_t z)
{
    const uint32_t ss = s ? (uint32_t)r.s1 : (uint32_t)r.s0, ee = s ? (uint32_t)r.e1 : (uint32_t)r.e0;
    hsa_job_t sj;
    memset(&sj, 0, sizeof sj);
    sj.off = jb.off + (r.strand ? jb.len - 1u - ee : ss);
    sj.len = ee - ss + 1u;
    a.s_jobs[t] = sj;
    a.s_hits[HSA_ALN64_WORDS * t] = 0u;                    // gap 0: the window is seg_len characters
    a.s_hits[HSA_ALN64_WORDS * t + 1] = r.strand << 30;
    a.s_pos[4 * t] = L.occ[z]; a.s_pos[4 * t + 1] = L.sid[z]; a.s_pos[4 * t + 2] = L.ori[z]; a.s_pos[4 * t + 3] = L.occ[z];
}

__global__ void __launch_bounds__(64) k_sl_pair(SlArgs a)
{
    __shared__ SlLds L;
    const uint32_t lane = threadIdx.x;
    for (uint32_t j = blockIdx.x; j < a.n_jobs; j += gridDim.x) {
        __syncthreads();                                   // the last read's LDS is read no more
        if (lane == 0) {                                   // refine's identity maps: row t of read t, record t
            for (uint32_t s = 0; s < 2u; ++s) {
                const uint64_t t = 2ull * j + s;
                a.s_hit_off[t] = t; a.s_pos_off[t] = t; a.s_pos_hit[t] = 0u;
            }
            if (j + 1u == a.n_jobs) a.s_pos_off[2ull * a.n_jobs] = 2ull * a.n_jobs;
            if (a.xcnt) {
                a.xcnt[j] = 0u;
                if (j + 1u == a.n_jobs) a.xcnt[a.n_jobs] = 0u;
            }
        }
        uint32_t *row = a.rows + (size_t)HSA_SL_ROW_WORDS * j;
        const uint32_t *res = a.res + (size_t)HSA_SP_RES_WORDS * j;
        const hsa_job_t jb = a.jobs[j];
        uint32_t st = HSA_SL_OK;
        const bool sent = (a.flags[j] & HSA_F_FALLBACK) && a.n_aln[j] == 0;
        if (!sent) st = HSA_SL_NONE;
        else if (res[0] != HSA_SP_OK) st = HSA_SL_HANDED;
        else if (res[1] != 2u || (res[2 + 5] & 0x3FFFFFFFu) != SL_TYPE_SPLICING) st = HSA_SL_NONE;
        if (st != HSA_SL_OK) {
            if (lane == 0) {
                sl_row_words(row, st, 0u, 0u, 0u, 0u);
                sl_no_segment(a, 2ull * j); sl_no_segment(a, 2ull * j + 1u);
            }
            continue;
        }
        SlRec r;
        if (!sl_decode(a, res, jb, r)) {
            if (lane == 0) {
                sl_row_words(row, HSA_SL_INPUT, 0u, 0u, 0u, r.strand);
                sl_no_segment(a, 2ull * j); sl_no_segment(a, 2ull * j + 1u);
            }
            continue;
        }
        sl_rows_sorted(a, L, r, lane);
        uint32_t first, shortest;
        const uint32_t n_res = sl_combine(L, r.n0, r.n, first, shortest);
        st = n_res == 0u ? HSA_SL_NOPAIR : n_res > 1u ? HSA_SL_MULTI : HSA_SL_OK;
        const uint32_t x = L.ord[first], y = L.ord[first + 1u];
        if (st == HSA_SL_MULTI && a.xcnt) {
            // the later pairs are printed too (k_sl_fill): each of their rows needs a block
            bool bad = false;
            for (uint32_t i = first + 1u + lane; i + 1u < r.n; i += 64u)
                bad |= sl_later_pair(L, i, r.n0, r.n, shortest) && (!L.found[L.ord[i]] || !L.found[L.ord[i + 1u]]);
            st = __ballot(bad) ? HSA_SL_POS : HSA_SL_OK;
            if (st == HSA_SL_OK && lane == 0) a.xcnt[j] = n_res - 1u;
        }
        if (st == HSA_SL_OK && (!L.found[x] || !L.found[y] || L.sid[x] != L.sid[y])) st = HSA_SL_POS;
        if (lane == 0) {
            if (st != HSA_SL_OK && a.xcnt) a.xcnt[j] = 0u;
            sl_row_words(row, st, r.n, n_res, r.c1, r.strand);
            if (n_res) {
                row[6] = L.sid[x]; row[7] = L.ori[x]; row[8] = L.occ[x]; row[9] = (uint32_t)r.s0; row[10] = (uint32_t)r.e0; row[11] = r.mm0;
                row[12] = L.sid[y]; row[13] = L.ori[y]; row[14] = L.occ[y]; row[15] = (uint32_t)r.s1; row[16] = (uint32_t)r.e1; row[17] = r.mm1;
                row[19] = r.mm0 + r.mm1;
            }
            if (st != HSA_SL_OK) { sl_no_segment(a, 2ull * j); sl_no_segment(a, 2ull * j + 1u); }
            else
                for (uint32_t s = 0; s < 2u; ++s) sl_segment(a, 2ull * j + s, jb, r, s, L, s ? y : x);
        }
    }
}

// The extra refine rows before k_sl_fill: rows no kernel answers, refine's identity maps over
// them and the end of its offsets, and every extra pair's slot marked unused.
__global__ void __launch_bounds__(256) k_sl_room(SlArgs a)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t base = 2ull * a.n_jobs;
    if (e == 0) a.s_pos_off[base + 2ull * a.pair_cap] = base + 2ull * a.pair_cap;
    if (e >= a.pair_cap) return;
    for (uint32_t s = 0; s < 2u; ++s) {
        const uint64_t t = base + 2ull * e + s;
        a.s_hit_off[t] = t; a.s_pos_off[t] = t; a.s_pos_hit[t] = 0u;
        sl_no_segment(a, t);
    }
    a.prow[(size_t)HSA_SL_XA_WORDS * e] = HSA_SL_XA_UNUSED;
}

// The extra pairs of the reads that have some, into the room: refine rows and pair rows.
__global__ void __launch_bounds__(64) k_sl_fill(SlArgs a)
{
    __shared__ SlLds L;
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x == 0 && lane == 0) {
        const uint64_t want = a.pair_off[a.n_jobs];
        a.xctr[0] = want;
        a.xctr[1] = want < a.pair_cap ? want : a.pair_cap;
    }
    for (uint32_t j = blockIdx.x; j < a.n_jobs; j += gridDim.x) {
        const uint64_t e0 = a.pair_off[j], e1 = a.pair_off[j + 1u];
        if (e1 == e0) continue;                            // (most reads)
        uint32_t *row = a.rows + (size_t)HSA_SL_ROW_WORDS * j;
        // no room: the plain entry points' answer.  k_sl_pair has filled pair 0's two refine rows
        // already and they are aligned for nothing; the caller's second run has the room.
        if (e1 > a.pair_cap || e1 - e0 >= SL_SEG_ROWS) {
            if (lane == 0) row[0] = HSA_SL_MULTI;
            continue;
        }
        __syncthreads();                                   // the last read's LDS is read no more
        const hsa_job_t jb = a.jobs[j];
        SlRec r;
        if (!sl_decode(a, a.res + (size_t)HSA_SP_RES_WORDS * j, jb, r)) continue;      // (k_sl_pair saw the same words)
        sl_rows_sorted(a, L, r, lane);
        uint32_t first, shortest;
        sl_combine(L, r.n0, r.n, first, shortest);
        uint32_t seen = 0;                                 // kept pairs at lower sorted indices
        for (uint32_t lo = first + 1u; lo + 1u < r.n; lo += 64u) {
            const uint32_t i = lo + lane;
            const bool kept = sl_later_pair(L, i, r.n0, r.n, shortest);
            const unsigned long long mask = __ballot(kept);
            const uint64_t e = e0 + seen + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (kept && e < e1) {
                const uint32_t x = L.ord[i], y = L.ord[i + 1u];
                const uint64_t t = 2ull * a.n_jobs + 2ull * e;
                sl_segment(a, t, jb, r, 0u, L, x);
                sl_segment(a, t + 1u, jb, r, 1u, L, y);
                uint32_t *pr = a.prow + (size_t)HSA_SL_XA_WORDS * e;
                for (uint32_t w = 0; w < HSA_SL_XA_WORDS; ++w) pr[w] = 0u;
                pr[0] = HSA_SL_OK; pr[1] = j; pr[6] = L.sid[x]; pr[7] = L.ori[x]; pr[8] = L.occ[x]; pr[9] = (uint32_t)r.e0;
                pr[10] = L.ori[y]; pr[11] = L.occ[y]; pr[12] = r.strand; pr[15] = L.ori[x];
            }
            seen += (uint32_t)__popcll(mask);
        }
        if (lane == 0) row[22] = (uint32_t)(e1 - e0);
    }
}

// The stored length of read j (hsa_sam_trim_t): SEQ and QUAL are printed over it, the segments lie in hsa_job_t.len
__device__ __forceinline__ uint32_t sl_full_len(const SlArgs &a, uint32_t j, uint32_t len) { return a.full_len ? a.full_len[j] : len; }

// The merged CIGAR (:578-582) into d_cigar, the row words after the end rules; HSA_SL_OK or
// why not.
__device__ __forceinline__ uint32_t sl_merge(const SlArgs &a, uint32_t j)
{
    uint32_t *row = a.rows + (size_t)HSA_SL_ROW_WORDS * j;
    uint32_t nc[2];
    for (uint32_t s = 0; s < 2u; ++s) {
        const uint64_t t = 2ull * j + s;
        const uint32_t *rr = a.s_rows + HSA_RF_ROW_WORDS * t;
        // (no MD is kept for a segment, so a row that is right but for its MD says HSA_RF_MD)
        if (rr[0] != HSA_RF_OK && rr[0] != HSA_RF_MD) return HSA_SL_REFINE;
        nc[s] = rr[1];
        if (nc[s] == 0u || nc[s] > SL_SEG_CIGAR) return HSA_SL_REFINE;
        const uint32_t trim5 = rr[4], trim3 = rr[5];
        row[7 + 6 * s] = (uint32_t)a.s_rpos[2 * t + 1];    // ori_pos, occ_pos and start after a leading D,
        row[8 + 6 * s] = (uint32_t)a.s_rpos[2 * t];        // end after a trailing one (:413-426)
        row[9 + 6 * s] += trim5;
        row[10 + 6 * s] -= trim3;
    }
    const int64_t n_len = (int64_t)row[13] - (int64_t)row[7] - (int64_t)(int32_t)row[10];      // :581
    row[20] = nc[0]; row[21] = nc[1];
    if (n_len <= 0 || n_len > 0x0FFFFFFF) return HSA_SL_INTRON;
    row[18] = (uint32_t)n_len;
    const uint32_t n_cigar = nc[0] + 1u + nc[1];
    row[5] = n_cigar;
    if (n_cigar > a.cigar_stride) return HSA_SL_INPUT;
    uint32_t *cg = a.cigar + (size_t)a.cigar_stride * j;
    for (uint32_t i = 0; i < nc[0]; ++i) cg[i] = a.s_cigar[(size_t)SL_SEG_CIGAR * (2ull * j) + i];
    cg[nc[0]] = (3u << 28) | (uint32_t)n_len;
    for (uint32_t i = 0; i < nc[1]; ++i) cg[nc[0] + 1u + i] = a.s_cigar[(size_t)SL_SEG_CIGAR * (2ull * j + 1u) + i];
    for (uint32_t i = 0; i < n_cigar; ++i)
        if ((cg[i] >> 28) > 8u) return HSA_SL_INPUT;
    if (row[6] >= a.n_chr) return HSA_SL_POS;
    const uint64_t c = row[6];
    if (a.chr_off[c + 1] < a.chr_off[c] || a.chr_off[c + 1] - a.chr_off[c] > a.max_line) return HSA_SL_INPUT;
    const hsa_job_t jb = a.jobs[j];
    const uint32_t full = sl_full_len(a, j, jb.len);
    if (a.name_off[j + 1] < a.name_off[j] || a.name_off[j + 1] - a.name_off[j] > a.max_line || full > a.max_line || full < jb.len)
        return HSA_SL_INPUT;
    if (a.quals && (a.qual_off[j + 1] < a.qual_off[j] || a.qual_off[j + 1] - a.qual_off[j] != full)) return HSA_SL_INPUT;
    return HSA_SL_OK;
}

// where the lanes find and put a read's long fields
struct SlMark {
    uint32_t name_dst, name_len, seq_dst, qual_dst, xa_dst;
};

// The line of read j (status HSA_SL_OK: sl_merge checked every index), bwtse.c:707-799 for
// type BWA_TYPE_SPLICING.  Name, SEQ and QUAL are skipped and their places left in mk.
template <class S> __device__ __forceinline__ void sl_emit(const SlArgs &a, uint32_t j, S &s, SlMark &mk)
{
    const uint32_t *row = a.rows + (size_t)HSA_SL_ROW_WORDS * j;
    const uint32_t len = a.jobs[j].len, strand = row[4], c1 = row[3];
    const uint32_t full = sl_full_len(a, j, len);
    mk.name_len = (uint32_t)(a.name_off[j + 1] - a.name_off[j]);
    mk.name_dst = s.pos();
    s.skip(mk.name_len);
    s.ch('\t'); s.dec(a.flag | (strand ? 16u : 0u));
    s.ch('\t');
    const uint64_t co = a.chr_off[row[6]];
    s.bytes(a.chr_names + co, (uint32_t)(a.chr_off[row[6] + 1u] - co));
    s.ch('\t'); s.dec(row[7]);
    s.lit("\t0\t");                                        // mapQ: the value of :345 is dropped
    const uint32_t *cg = a.cigar + (size_t)a.cigar_stride * j;
    sm_cigar_clipped(cg, row[5], strand, full - len, s);     // bwa_correct_trimmed holds for a spliced read too (bwtse.c:637)
    s.lit("\t*\t0\t0\t");
    mk.seq_dst = s.pos();
    s.skip(full);
    s.ch('\t');
    mk.qual_dst = s.pos();
    if (a.quals) s.skip(full); else s.ch('*');
    sm_clip_tags(a.bc ? a.bc + (size_t)a.bc_len * j : nullptr, a.bc_len, len, full, s);
    s.lit("\tXT:A:S\t"); s.ch(a.comp_read ? 'N' : 'C'); s.lit("M:i:0");      // nm is never computed for these reads
    s.lit("\tX0:i:"); s.dec(c1);
    if (a.max_top2 >= 0 && c1 <= (uint32_t)a.max_top2) { s.lit("\tX1:i:"); s.dec(c1); }     // c2 = c1, :315
    s.lit("\tXM:i:"); s.dec(row[19]);
    s.lit("\tXO:i:0\tXG:i:0");                             // gap is never set; no MD
    mk.xa_dst = 0u;
    if (row[22]) {                                         // :782-797, the entries by sl_xa_emit
        s.lit("\tXA:Z:");
        mk.xa_dst = s.pos();
        s.skip(row[23]);
    }
    s.ch('\n');
}

// Extra pair e after the refinement: the end rules (:413-426), the N length and the merged
// CIGAR as sl_merge has them for pair 0, into the pair's row and d_pair_cigar; HSA_SL_OK or
// why not.
__device__ __forceinline__ uint32_t sl_xa_merge(const SlArgs &a, uint64_t e)
{
    uint32_t *pr = a.prow + (size_t)HSA_SL_XA_WORDS * e;
    const uint64_t t0 = 2ull * a.n_jobs + 2ull * e;
    uint32_t nc[2];
    for (uint32_t s = 0; s < 2u; ++s) {
        const uint32_t *rr = a.s_rows + HSA_RF_ROW_WORDS * (t0 + s);
        if (rr[0] != HSA_RF_OK && rr[0] != HSA_RF_MD) return HSA_SL_REFINE;
        nc[s] = rr[1];
        if (nc[s] == 0u || nc[s] > SL_SEG_CIGAR) return HSA_SL_REFINE;
        pr[s ? 10 : 7] = (uint32_t)a.s_rpos[2 * (t0 + s) + 1];
        pr[s ? 11 : 8] = (uint32_t)a.s_rpos[2 * (t0 + s)];
        if (!s) pr[9] -= rr[5];                            // end after a trailing D
    }
    const int64_t n_len = (int64_t)pr[10] - (int64_t)pr[7] - (int64_t)(int32_t)pr[9];        // :612
    pr[13] = nc[0]; pr[14] = nc[1];
    if (n_len <= 0 || n_len > 0x0FFFFFFF) return HSA_SL_INTRON;
    pr[5] = (uint32_t)n_len;
    const uint32_t n_cigar = nc[0] + 1u + nc[1];
    pr[4] = n_cigar;
    if (n_cigar > a.cigar_stride) return HSA_SL_INPUT;
    uint32_t *cg = a.pcigar + (size_t)a.cigar_stride * e;
    for (uint32_t i = 0; i < nc[0]; ++i) cg[i] = a.s_cigar[(size_t)SL_SEG_CIGAR * t0 + i];
    cg[nc[0]] = (3u << 28) | (uint32_t)n_len;
    for (uint32_t i = 0; i < nc[1]; ++i) cg[nc[0] + 1u + i] = a.s_cigar[(size_t)SL_SEG_CIGAR * (t0 + 1u) + i];
    for (uint32_t i = 0; i < n_cigar; ++i)
        if ((cg[i] >> 28) > 4u) return HSA_SL_INPUT;       // "MIDNS"[op], :794
    if (pr[6] >= a.n_chr) return HSA_SL_POS;
    const uint64_t c = pr[6];
    if (a.chr_off[c + 1] < a.chr_off[c] || a.chr_off[c + 1] - a.chr_off[c] > a.max_line) return HSA_SL_INPUT;
    if (pr[7] > 0x7FFFFFFFu) return HSA_SL_INPUT;          // printed with %d
    return HSA_SL_OK;
}

// The XA entry of extra pair e (status HSA_SL_OK), :788-795: "<chr>,<+|-><ori_pos>" and the
// CIGAR directly behind it
template <class S> __device__ __forceinline__ void sl_xa_emit(const SlArgs &a, uint64_t e, S &s)
{
    const uint32_t *pr = a.prow + (size_t)HSA_SL_XA_WORDS * e;
    const uint64_t co = a.chr_off[pr[6]];
    s.bytes(a.chr_names + co, (uint32_t)(a.chr_off[pr[6] + 1u] - co));
    s.ch(','); s.ch(pr[12] ? '-' : '+'); s.dec(pr[7]);
    const uint32_t *cg = a.pcigar + (size_t)a.cigar_stride * e;
    for (uint32_t i = 0; i < pr[4]; ++i) { s.dec(cg[i] & 0x0FFFFFFFu); s.ch((char)sm_op_letter(cg[i] >> 28)); }
}

__global__ void __launch_bounds__(256) k_sl_xlen(SlArgs a)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.pair_cap) return;
    uint32_t *pr = a.prow + (size_t)HSA_SL_XA_WORDS * e;
    if (pr[0] != HSA_SL_OK) return;                        // HSA_SL_XA_UNUSED
    const uint32_t st = sl_xa_merge(a, e);
    pr[0] = st;
    if (st != HSA_SL_OK) return;
    SmCount s;
    sl_xa_emit(a, e, s);
    pr[2] = (uint32_t)s.n;
}

__global__ void __launch_bounds__(256) k_sl_len(SlArgs a)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t len = 0;
    if (j < a.n_jobs) {
        uint32_t *row = a.rows + (size_t)HSA_SL_ROW_WORDS * j;
        uint32_t st = row[0];
        const bool spliced = st != HSA_SL_NONE && st != HSA_SL_HANDED;
        if (st == HSA_SL_OK) st = sl_merge(a, j);
        // row[22] is set by k_sl_fill alone, for a read whose extra pairs found room: through the
        // plain entry points (sl_row_words zeroes the row; xctr, pair_off and prow are null) it is 0
        const uint32_t n_xa = row[22];
        if (st == HSA_SL_OK && n_xa) {
            // the entries' places in the read's XA text; a pair that failed refuses the read
            uint32_t at = 0;
            for (uint32_t q = 0; q < n_xa && st == HSA_SL_OK; ++q) {
                uint32_t *pr = a.prow + (size_t)HSA_SL_XA_WORDS * (a.pair_off[j] + q);
                st = pr[0];
                pr[3] = at;
                at += pr[2];
            }
            row[23] = at;
        }
        if (st == HSA_SL_OK) {
            SmCount s;
            SlMark mk;
            sl_emit(a, j, s, mk);
            if (s.n > a.max_line) st = HSA_SL_INPUT;
            else len = s.n;
        }
        row[0] = st;
        a.stat[j] = st;
        // (a handful of reads per batch leave this path with anything but HSA_SL_NONE)
        if (spliced) atomicAdd(&a.ctr[7], 1ull);
        if (st == HSA_SL_OK && n_xa) { atomicAdd(&a.xctr[2], 1ull); atomicAdd(&a.xctr[3], (unsigned long long)n_xa); }
        if (st == HSA_SL_OK) atomicAdd(&a.ctr[2], 1ull);
        else if (st == HSA_SL_HANDED) atomicAdd(&a.ctr[3], 1ull);
        else if (st == HSA_SL_MULTI) atomicAdd(&a.ctr[4], 1ull);
        else if (st == HSA_SL_NOPAIR) atomicAdd(&a.ctr[6], 1ull);
        else if (st != HSA_SL_NONE) atomicAdd(&a.ctr[5], 1ull);
    }
    if (j <= a.n_jobs) a.lens[j] = len;
}

__global__ void __launch_bounds__(64) k_sl_write(SlArgs a)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t total = a.line_off[a.n_jobs];
    if (blockIdx.x == 0 && lane == 0) {
        a.ctr[0] = total;
        a.ctr[1] = total < a.out_cap ? total : a.out_cap;
    }
    for (uint32_t j = blockIdx.x; j < a.n_jobs; j += gridDim.x) {
        if (a.stat[j] != HSA_SL_OK) continue;
        const uint64_t base = a.line_off[j], end = a.line_off[j + 1];
        if (end <= base || base >= a.out_cap) continue;
        const uint64_t room = a.out_cap - base;
        const uint32_t cap = (uint32_t)(end - base < room ? end - base : room);      // no byte at or past out_cap
        uint8_t *g = a.out + base;
        // every lane walks the line for the places of the long fields; lane 0 alone has room
        // to store (a sink of capacity 0 stores nothing)
        SmStore s{g, 0u, lane == 0 ? cap : 0u};
        SlMark mk;
        sl_emit(a, j, s, mk);
        const hsa_job_t jb = a.jobs[j];
        const uint32_t strand = a.rows[(size_t)HSA_SL_ROW_WORDS * j + 4];
        const uint8_t *name = a.names + a.name_off[j];
        for (uint32_t k = lane; k < mk.name_len; k += 64u)
            if (mk.name_dst + k < cap) g[mk.name_dst + k] = name[k];
        const uint64_t letters = strand ? SM_REV : SM_FWD;
        const uint8_t *code = a.codes + jb.off;
        const uint8_t *qual = a.quals ? a.quals + a.qual_off[j] : nullptr;
        const uint32_t full = sl_full_len(a, j, jb.len);
        for (uint32_t k = lane; k < full; k += 64u) {
            const uint32_t i = strand ? full - 1u - k : k;
            const uint32_t c = code[i];
            if (mk.seq_dst + k < cap) g[mk.seq_dst + k] = (uint8_t)(letters >> (8u * (c < 4u ? c : 4u)));
            if (qual && mk.qual_dst + k < cap) g[mk.qual_dst + k] = qual[i];
        }
        const uint32_t n_xa = a.rows[(size_t)HSA_SL_ROW_WORDS * j + 22];
        for (uint32_t q = lane; q < n_xa; q += 64u) {       // the entries side by side
            const uint64_t e = a.pair_off[j] + q;
            SmStore x{g, mk.xa_dst + a.prow[(size_t)HSA_SL_XA_WORDS * e + 3], cap};
            sl_xa_emit(a, e, x);
        }
    }
}

extern "C" int hsa_splice_lines_device(hsa_index_t *ix, const hsa_splice_lines_batch_t *b, void *stream)
{
    return hsa_splice_lines_device_trim(ix, b, nullptr, stream);
}

extern "C" int hsa_splice_lines_device_trim(hsa_index_t *ix, const hsa_splice_lines_batch_t *b, const hsa_sam_trim_t *trim,
                                            void *stream)
{
    return hsa_splice_lines_device_xa(ix, b, trim, nullptr, stream);
}

extern "C" int hsa_splice_lines_device_xa(hsa_index_t *ix, const hsa_splice_lines_batch_t *b, const hsa_sam_trim_t *trim,
                                          const hsa_splice_xa_t *xa, void *stream)
{
    const char *what = xa ? "hsa_splice_lines_device_xa" : "hsa_splice_lines_device";
    if (!ix) { hsa_set_error("%s: null handle", what); return HSA_E_ARG; }
    if (ix->is64) { hsa_set_error("%s: the index text has 2^32 characters or more: the splice path is 32-bit", what); return HSA_E_ARG; }
    if (!b || b->n_jobs < 0 || !b->d_counters || !b->d_line_off || (b->out_cap && !b->d_out) || b->max_len < 0) {
        hsa_set_error("%s: bad arguments", what);
        return HSA_E_ARG;
    }
    if (b->n_jobs && (!b->d_jobs || !b->d_codes || !b->d_flags || !b->d_n_aln || !b->d_res || !b->d_names || !b->d_name_off ||
                      !b->d_rows || !b->d_line_stat || (b->cigar_stride && !b->d_cigar) ||
                      (b->n_chr && (!b->d_chr_names || !b->d_chr_off)))) {
        hsa_set_error("%s: null argument", what);
        return HSA_E_ARG;
    }
    if (trim && (trim->bc_len > HSA_SAM_MAX_BC || (trim->bc_len != 0u) != (trim->d_bc != nullptr))) {
        hsa_set_error("%s: a barcode of 1..%u bytes per read goes with d_bc", what, HSA_SAM_MAX_BC);
        return HSA_E_ARG;
    }
    if ((b->d_quals == nullptr) != (b->d_qual_off == nullptr)) {
        hsa_set_error("%s: d_quals and d_qual_off go together", what);
        return HSA_E_ARG;
    }
    if (xa && (!xa->d_pair_off || !xa->d_counters || (xa->pair_cap && (!xa->d_pair_rows || (b->cigar_stride && !xa->d_pair_cigar))) ||
               xa->pair_cap > 0x3FFFFFFFull)) {
        hsa_set_error("%s: the extra pairs' arrays (d_pair_off, d_counters, and with room d_pair_rows, d_pair_cigar)", what);
        return HSA_E_ARG;
    }
    // the refinement counts its rows in an int: two per read and two per extra pair of room
    if (xa && 2ull * (uint64_t)b->n_jobs + 2ull * xa->pair_cap > 0x7FFFFFFFull) {
        hsa_set_error("%s: 2 n_jobs + 2 pair_cap = %llu rows for the refinement, over 2^31 - 1: less room or a smaller batch", what,
                      (unsigned long long)(2ull * (uint64_t)b->n_jobs + 2ull * xa->pair_cap));
        return HSA_E_ARG;
    }
    if (b->max_line < 1u || b->max_line > HSA_SAM_MAX_LINE) {
        hsa_set_error("%s: max_line %u is not in 1..%u", what, b->max_line, HSA_SAM_MAX_LINE);
        return HSA_E_ARG;
    }
    if (!ix->d_sa || !ix->d_blocks || ix->sa_interval == 0 || (!ix->d_text && !ix->d_text64)) {
        hsa_set_error("%s: needs hsa_index_set_sa and a text (hsa_index_set_text)", what);
        return HSA_E_ARG;
    }
    const uint64_t n = (uint64_t)b->n_jobs;
    const uint64_t room = xa ? xa->pair_cap : 0u;
    const uint64_t m = 2 * n + 2 * room;                   // refine rows: the first pairs', then the extra pairs'
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    size_t tmp_bytes = 0;
    HSA_TRY(hsa_scan_bytes(tmp_bytes, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
    SlArgs A;
    void *d_tmp = nullptr;
    uint64_t *rf_ctr = nullptr;
    A.xcnt = nullptr;
    auto layout = [&](Carver c) {
        A.s_jobs = c.take<hsa_job_t>(m + 1);
        A.s_hit_off = c.take<uint64_t>(m + 1);
        A.s_pos_off = c.take<uint64_t>(m + 1);
        A.s_pos = c.take<uint64_t>(4 * (m + 1));
        A.s_rpos = c.take<uint64_t>(2 * (m + 1));
        A.s_hits = c.take<uint32_t>(HSA_ALN64_WORDS * (m + 1));
        A.s_pos_hit = c.take<uint32_t>(m + 1);
        A.s_rows = c.take<uint32_t>(HSA_RF_ROW_WORDS * (m + 1));
        A.s_cigar = c.take<uint32_t>(SL_SEG_CIGAR * (m + 1));
        A.lens = c.take<uint64_t>(n + 1);
        if (xa) A.xcnt = c.take<uint64_t>(n + 1);
        rf_ctr = c.take<uint64_t>(8);
        d_tmp = c.take<char>(tmp_bytes);
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_sl, &ix->d_sl_cap, layout(Carver())));
    layout(Carver(ix->d_sl));
    A.sv = hsa_sa_view(ix);
    A.T = ix->T;
    A.jobs = b->d_jobs; A.n_jobs = (uint32_t)n; A.codes = b->d_codes; A.flags = b->d_flags; A.n_aln = b->d_n_aln;
    A.res = b->d_res;
    A.names = b->d_names; A.name_off = b->d_name_off; A.quals = b->d_quals; A.qual_off = b->d_qual_off;
    A.chr_names = b->d_chr_names; A.chr_off = b->d_chr_off; A.n_chr = b->n_chr;
    A.flag = b->flag; A.max_top2 = b->max_top2; A.comp_read = b->comp_read;
    A.max_len = (uint32_t)b->max_len; A.max_line = b->max_line; A.cigar_stride = b->cigar_stride;
    A.rows = b->d_rows; A.cigar = b->d_cigar;
    A.full_len = trim ? trim->d_full_len : nullptr; A.bc = trim ? trim->d_bc : nullptr; A.bc_len = trim ? trim->bc_len : 0u;
    A.line_off = b->d_line_off; A.out = b->d_out; A.out_cap = b->out_cap; A.stat = b->d_line_stat;
    A.ctr = (unsigned long long *)b->d_counters;
    A.pair_off = xa ? xa->d_pair_off : nullptr; A.pair_cap = room;
    A.prow = xa ? xa->d_pair_rows : nullptr; A.pcigar = xa ? xa->d_pair_cigar : nullptr;
    A.xctr = xa ? (unsigned long long *)xa->d_counters : nullptr;
    HSA_HIP(hipMemsetAsync(b->d_counters, 0, 8 * sizeof(uint64_t), st));
    if (xa) HSA_HIP(hipMemsetAsync(xa->d_counters, 0, 8 * sizeof(uint64_t), st));
    if (n == 0) {
        HSA_HIP(hipMemsetAsync(b->d_line_off, 0, sizeof(uint64_t), st));
        if (xa) HSA_HIP(hipMemsetAsync(xa->d_pair_off, 0, sizeof(uint64_t), st));
        return 0;
    }
    const unsigned waves = (unsigned)(n < 65536u ? n : 65536u);
    hipLaunchKernelGGL(k_sl_pair, dim3(waves), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    if (xa) {
        HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, A.xcnt, A.pair_off, (uint64_t)0, (size_t)(n + 1),
                                        rocprim::plus<uint64_t>(), st));
        if (room) {
            hipLaunchKernelGGL(k_sl_room, dim3((unsigned)((room + 255) / 256)), dim3(256), 0, st, A);
            HSA_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(k_sl_fill, dim3(waves), dim3(64), 0, st, A);
        HSA_HIP(hipGetLastError());
    }
    hsa_refine_batch64_t rb;
    memset(&rb, 0, sizeof rb);
    rb.d_jobs = A.s_jobs; rb.n_jobs = (int)m; rb.d_codes = b->d_codes;
    rb.d_hit_off = A.s_hit_off; rb.d_hits = A.s_hits;
    rb.d_pos_off = A.s_pos_off; rb.d_pos = A.s_pos; rb.d_pos_hit = A.s_pos_hit;
    rb.pos_cap = m; rb.d_pos_counters = nullptr;
    rb.max_len = b->max_len;
    rb.cigar_stride = SL_SEG_CIGAR; rb.md_stride = 0;      // (no MD is printed for a spliced read)
    rb.d_rows = A.s_rows; rb.d_rpos = A.s_rpos; rb.d_cigar = A.s_cigar; rb.d_md = nullptr;
    rb.d_counters = rf_ctr;
    HSA_HIP(hipMemsetAsync(rf_ctr, 0, 8 * sizeof(uint64_t), st));
    HSA_TRY(hsa_refine_rows_launch(ix, &rb, st, true, what));
    if (room) {
        hipLaunchKernelGGL(k_sl_xlen, dim3((unsigned)((room + 255) / 256)), dim3(256), 0, st, A);
        HSA_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_sl_len, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, A.lens, A.line_off, (uint64_t)0, (size_t)(n + 1),
                                    rocprim::plus<uint64_t>(), st));
    hipLaunchKernelGGL(k_sl_write, dim3(waves), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- two writers' lines in read order
// hsa_sam_merge_device: a read has a line from at most one of the two writers (k_sam_write
// for the unspliced reads, k_sl_write for the spliced ones); the lengths of both are added
// per read, scanned, and one wavefront per read copies its line (writer a's bytes, then
// writer b's) to its place, in 16-byte stores where source and destination are congruent
// modulo 16 and in byte stores otherwise.
struct MgArgs {
    uint32_t n;
    const uint64_t *off_a, *off_b;
    const uint8_t *txt_a, *txt_b;
    uint64_t len_a, len_b;
    uint64_t *line_off;
    uint8_t *out;
    uint64_t out_cap;
    unsigned long long *ctr;
    uint64_t *lens;
};

// line j of a writer: its offset and length; none for offsets that run backwards or past the text
__device__ __forceinline__ uint64_t mg_span(const uint64_t *off, uint32_t j, uint64_t cap, uint64_t &lo)
{
    lo = off[j];
    const uint64_t hi = off[j + 1];
    return hi < lo || hi > cap ? 0u : hi - lo;
}

__global__ void __launch_bounds__(256) k_mg_len(MgArgs a)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t len = 0;
    if (j < a.n) {
        uint64_t lo;
        len = mg_span(a.off_a, j, a.len_a, lo) + mg_span(a.off_b, j, a.len_b, lo);
    }
    if (j <= a.n) a.lens[j] = len;
}

__device__ __forceinline__ void mg_copy(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t lane)
{
    if (((reinterpret_cast<uintptr_t>(dst) ^ reinterpret_cast<uintptr_t>(src)) & 15u) != 0) {
        for (uint64_t k = lane; k < n; k += 64u) dst[k] = src[k];
        return;
    }
    const uint64_t lead = (16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    const uint64_t head = lead < n ? lead : n;
    const uint64_t units = (n - head) >> 4, tail = head + (units << 4);
    for (uint64_t k = lane; k < head; k += 64u) dst[k] = src[k];
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    for (uint64_t u = lane; u < units; u += 64u) d4[u] = s4[u];
    for (uint64_t k = tail + lane; k < n; k += 64u) dst[k] = src[k];
}

__global__ void __launch_bounds__(64) k_mg_copy(MgArgs a)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t total = a.line_off[a.n];
    if (blockIdx.x == 0 && lane == 0) {
        a.ctr[0] = total;
        a.ctr[1] = total < a.out_cap ? total : a.out_cap;
    }
    for (uint32_t j = blockIdx.x; j < a.n; j += gridDim.x) {
        uint64_t lo_a, lo_b;
        uint64_t na = mg_span(a.off_a, j, a.len_a, lo_a), nb = mg_span(a.off_b, j, a.len_b, lo_b);
        const uint64_t base = a.line_off[j];
        if (base >= a.out_cap) continue;
        const uint64_t room = a.out_cap - base;              // no byte at or past out_cap
        if (na > room) na = room;
        if (nb > room - na) nb = room - na;
        if (na) mg_copy(a.out + base, a.txt_a + lo_a, na, lane);
        if (nb) mg_copy(a.out + base + na, a.txt_b + lo_b, nb, lane);
    }
}

extern "C" int hsa_sam_merge_device(hsa_index_t *ix, const hsa_sam_merge_batch_t *b, void *stream)
{
    const char *what = "hsa_sam_merge_device";
    if (!ix) { hsa_set_error("%s: null handle", what); return HSA_E_ARG; }
    if (!b || b->n_jobs < 0 || !b->d_counters || !b->d_line_off || (b->out_cap && !b->d_out)) {
        hsa_set_error("%s: bad arguments", what);
        return HSA_E_ARG;
    }
    if (b->n_jobs && (!b->d_line_off_a || !b->d_line_off_b || (b->text_a_len && !b->d_text_a) || (b->text_b_len && !b->d_text_b))) {
        hsa_set_error("%s: null argument", what);
        return HSA_E_ARG;
    }
    const uint64_t n = (uint64_t)b->n_jobs;
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    size_t tmp_bytes = 0;
    HSA_TRY(hsa_scan_bytes(tmp_bytes, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
    MgArgs A;
    void *d_tmp = nullptr;
    auto layout = [&](Carver c) {
        A.lens = c.take<uint64_t>(n + 1);
        d_tmp = c.take<char>(tmp_bytes);
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_sl, &ix->d_sl_cap, layout(Carver())));
    layout(Carver(ix->d_sl));
    A.n = (uint32_t)n;
    A.off_a = b->d_line_off_a; A.off_b = b->d_line_off_b; A.txt_a = b->d_text_a; A.txt_b = b->d_text_b;
    A.len_a = b->text_a_len; A.len_b = b->text_b_len;
    A.line_off = b->d_line_off; A.out = b->d_out; A.out_cap = b->out_cap;
    A.ctr = (unsigned long long *)b->d_counters;
    HSA_HIP(hipMemsetAsync(b->d_counters, 0, 8 * sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_mg_len, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, A.lens, A.line_off, (uint64_t)0, (size_t)(n + 1),
                                    rocprim::plus<uint64_t>(), st));
    hipLaunchKernelGGL(k_mg_copy, dim3((unsigned)(n ? (n < 65536u ? n : 65536u) : 1u)), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    return 0;
}
