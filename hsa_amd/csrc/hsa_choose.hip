// hsa_choose.hip -- each read's hit, mapQ and XA rows on the 64-bit path.
//
// bwt_aln2seq_core(p, 1, n_multi) (bwtse.c:21-113), the row filter of bwa_cal_pac_pos
// (:350-369) and bwa_approx_mapQ (:122-131) for the hit lists of hsa_search_device64 as
// they sit on the device.  The choice draws from the process-wide drand48 sequence in
// read order (:44, :51), and how many numbers a read draws depends on their values, so
// the per-read generator states are not a prefix sum.  What the number of draws depends
// on is small, though:
//   no hit                          0 draws;
//   one equal-best record           2 draws (the first test is u * w > 0: true unless
//                                   u == 0, probability 2^-48; detected and reported);
//   two or more equal-best records  between nb + 1 and 2 nb draws: a *variable* read.
// Only the variable reads are walked in order.  The launches, all on one stream:
//   k_choose_class    one lane per read: its class, its row count;
//   rocPRIM exclusive scan of (variable reads, fixed draws, rows) in read order;
//   k_choose_compact  one lane per read: the row offsets; a variable read goes to its
//                     place in the dense list with the fixed draws made before it;
//   k_choose_maps     one lane per variable read: the affine map X -> A^d X + C_d of the
//                     d fixed draws since the variable read before it, by squaring;
//   k_choose_walk     ONE wave walks the dense list in order: a multiply-add per read, then
//                     the read's draws; writes the state after every variable read;
//   k_choose_pick     one lane per read: its start state by a jump from the end state of
//                     the variable read before it, then the reference's choice from that
//                     state, c1, c2, the type and mapQ;
//   k_choose_rows     one lane per output row: the walk (hsa_sa_row64).
// The multi rows make no draw: the reference keeps them only when the read's rows n_occ <=
// n_multi + 1, and then rest == n_occ at bwtse.c:78, every record has l - k + 1 <= rest at
// :82, and the random-sample branch (:93-108) cannot be reached.
//
// The generator is glibc's: X <- (0x5DEECE66D X + 0xB) mod 2^48, drand48 = X 2^-48 (exact
// in a double).  The tests u * (w + cnt) > cnt and (int)(w * v) are one double multiply
// and a compare or a convert: no add, so nothing for contraction to fuse.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <string.h>

#include "hsa_device.h"
#include "hsa_internal.h"
#include "hsa_sa.h"

#define CH_A 0x5DEECE66Dull
#define CH_C 0xBull
#define CH_MASK 0xFFFFFFFFFFFFull
#define CH_TILE 64u                // variable reads per tile of the walk
#define CH_TILE_W 4u               // widths per read a tile holds in LDS (the others are loaded when met)

// what the scan adds up, per read
struct ChCls {
    uint64_t vf;                   // variable reads << 32 | fixed draws (2 n_jobs < 2^32)
    uint64_t rows;
};
struct ChPlus {
    __host__ __device__ ChCls operator()(const ChCls &a, const ChCls &b) const { return ChCls{a.vf + b.vf, a.rows + b.rows}; }
};

struct ChooseArgs {
    SaView64 v;
    const hsa_job_t *jobs;
    const int32_t *n_aln;
    const uint64_t *hit_off;
    const uint32_t *hits;
    const int32_t *log_n;          // g_log_n, 256 entries
    uint32_t n_jobs, n_multi;
    uint64_t rng;
    uint32_t *sel;                 // 4 u32 per read
    uint64_t *sel64;               // 4 u64 per read
    uint64_t *rng_out;
    uint64_t *pos_off, *pos;
    uint32_t *pos_hit;
    uint64_t pos_cap;
    unsigned long long *ctr;
    // scratch
    ChCls *cls, *scn;              // n_jobs + 1 each
    uint32_t *nbs;                 // per read: its equal-best records
    uint32_t *var_fix, *var_nb;    // per variable read: fixed draws before it, its equal-best records
    uint64_t *var_hoff;            //   its first record
    uint64_t *var_A, *var_C;       //   the map of the fixed draws since the variable read before it
    uint64_t *var_end;             //   the state after it
};

__device__ __forceinline__ uint64_t ch_step(uint64_t x) { return (CH_A * x + CH_C) & CH_MASK; }
__device__ __forceinline__ double ch_real(uint64_t x) { return (double)x * 0x1p-48; }

// x after d draws: the maps of 1, 2, 4, ... draws by squaring
__device__ __forceinline__ uint64_t ch_jump(uint64_t x, uint32_t d)
{
    uint64_t A = CH_A, C = CH_C;
    for (; d; d >>= 1) {
        if (d & 1u) x = A * x + C;
        C *= A + 1u;
        A *= A;
    }
    return x & CH_MASK;
}

__device__ __forceinline__ int32_t ch_score(const uint32_t *rec) { return (int32_t)rec[12]; }

// a read's equal-best records (bwtse.c:40-43), its first width, its rows
__device__ __forceinline__ uint32_t ch_scan_read(const ChooseArgs &a, uint32_t j, uint64_t &w0, uint64_t &n_occ, int32_t &na)
{
    na = a.n_aln[j];
    w0 = n_occ = 0;
    if (na <= 0) return 0;
    const uint32_t *rec = a.hits + a.hit_off[j] * HSA_ALN64_WORDS;
    const int32_t best = ch_score(rec);
    uint32_t nb = 0;
    bool lead = true;
    for (int32_t i = 0; i < na; ++i, rec += HSA_ALN64_WORDS) {
        uint64_t k;
        const uint64_t w = hsa_aln64_rows(rec, k);
        if (lead && ch_score(rec) > best) lead = false;
        if (lead) ++nb;
        if (i == 0) w0 = w;
        n_occ += w;
    }
    return nb;
}

// rows of a read: the chosen one, and the others when there are at most n_multi of them
__device__ __forceinline__ uint64_t ch_n_rows(const ChooseArgs &a, int32_t na, uint64_t n_occ)
{
    if (na <= 0) return 0;
    return (n_occ == 0 || n_occ > (uint64_t)a.n_multi + 1u) ? 1u : n_occ;
}

// a read whose draw count is not known without drawing: two or more equal-best records,
// or one without rows (a malformed record: its test is never true)
__device__ __forceinline__ bool ch_variable(uint32_t nb, uint64_t w0) { return nb >= 2u || (nb == 1u && w0 == 0); }

__global__ void __launch_bounds__(256) k_choose_class(ChooseArgs a)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > a.n_jobs) return;
    ChCls c{0, 0};
    if (j < a.n_jobs) {
        uint64_t w0, n_occ;
        int32_t na;
        const uint32_t nb = ch_scan_read(a, j, w0, n_occ, na);
        a.nbs[j] = nb;
        c.vf = ch_variable(nb, w0) ? 1ull << 32 : (nb ? 2ull : 0ull);
        c.rows = ch_n_rows(a, na, n_occ);
    } else {
        a.ctr[7] = ~0ull;          // no zero-draw read yet
    }
    a.cls[j] = c;
}

__global__ void __launch_bounds__(256) k_choose_compact(ChooseArgs a)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > a.n_jobs) return;
    const ChCls s = a.scn[j];
    a.pos_off[j] = s.rows;
    if (j == a.n_jobs) { a.ctr[5] = s.vf >> 32; return; }
    if (!(a.cls[j].vf >> 32)) return;
    const uint32_t i = (uint32_t)(s.vf >> 32);
    a.var_fix[i] = (uint32_t)s.vf;
    a.var_nb[i] = a.nbs[j];
    a.var_hoff[i] = a.hit_off[j];
}

__global__ void __launch_bounds__(256) k_choose_maps(ChooseArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)(a.scn[a.n_jobs].vf >> 32)) return;
    uint32_t d = a.var_fix[i] - (i ? a.var_fix[i - 1] : 0u);
    uint64_t A = CH_A, C = CH_C, mA = 1, mC = 0;
    for (; d; d >>= 1) {
        if (d & 1u) { mC = A * mC + C; mA *= A; }
        C *= A + 1u;
        A *= A;
    }
    a.var_A[i] = mA & CH_MASK;
    a.var_C[i] = mC & CH_MASK;
}

// One wave.  Every lane computes the same states from the same LDS words; the only
// lane-dependent code is the tile's load and the store of its end states, each a region
// of its own between two barriers.  No region of the loop is entered by one lane alone.
__global__ void __launch_bounds__(64) k_choose_walk(ChooseArgs a)
{
    __shared__ uint64_t sA[CH_TILE], sC[CH_TILE], sHoff[CH_TILE], sEnd[CH_TILE], sW[CH_TILE * CH_TILE_W];
    __shared__ uint32_t sNb[CH_TILE];
    const uint32_t lane = threadIdx.x;
    const uint32_t n_var = (uint32_t)(a.scn[a.n_jobs].vf >> 32);
    uint64_t x = a.rng;
    for (uint32_t base = 0; base < n_var; base += CH_TILE) {
        const uint32_t cnt = n_var - base < CH_TILE ? n_var - base : CH_TILE;
        if (lane < cnt) {
            const uint32_t i = base + lane;
            const uint32_t nb = a.var_nb[i];
            const uint64_t ho = a.var_hoff[i];
            sA[lane] = a.var_A[i]; sC[lane] = a.var_C[i]; sNb[lane] = nb; sHoff[lane] = ho;
            const uint32_t *rec = a.hits + ho * HSA_ALN64_WORDS;
            for (uint32_t r = 0; r < CH_TILE_W && r < nb; ++r, rec += HSA_ALN64_WORDS) {
                uint64_t k;
                sW[lane * CH_TILE_W + r] = hsa_aln64_rows(rec, k);
            }
        }
        __syncthreads();
        for (uint32_t t = 0; t < cnt; ++t) {
            x = (sA[t] * x + sC[t]) & CH_MASK;     // the fixed draws since the variable read before
            const uint32_t nb = sNb[t];
            const uint32_t *rec = a.hits + sHoff[t] * HSA_ALN64_WORDS;
            uint64_t c = 0;
            for (uint32_t r = 0; r < nb; ++r) {
                uint64_t w, k;
                if (r < CH_TILE_W) w = sW[t * CH_TILE_W + r];
                else w = hsa_aln64_rows(rec + (size_t)r * HSA_ALN64_WORDS, k);
                x = ch_step(x);
                const uint64_t x2 = ch_step(x);
                x = ch_real(x) * (double)(w + c) > (double)c ? x2 : x;   // bwtse.c:44, :51
                c += w;
            }
            sEnd[t] = x;
        }
        __syncthreads();
        if (lane < cnt) a.var_end[base + lane] = sEnd[lane];
        __syncthreads();
    }
}

// the state at the start of read j (j == n_jobs: after the last read)
__device__ __forceinline__ uint64_t ch_start(const ChooseArgs &a, uint32_t j)
{
    const uint64_t vf = a.scn[j].vf;
    const uint32_t i = (uint32_t)(vf >> 32), fix = (uint32_t)vf;
    return i ? ch_jump(a.var_end[i - 1], fix - a.var_fix[i - 1]) : ch_jump(a.rng, fix);
}

// bwa_approx_mapQ (bwtse.c:122-131)
__device__ __forceinline__ uint32_t ch_mapq(const ChooseArgs &a, uint64_t c1, uint64_t c2, uint32_t n_mm, int32_t max_diff)
{
    if (c1 == 0) return 23;
    if (c1 > 1) return 0;
    if ((int32_t)n_mm == max_diff) return 25;
    if (c2 == 0) return 37;
    const int32_t g = a.log_n[c2 >= 255 ? 255 : c2];
    return 23 < g ? 0u : (uint32_t)(23 - g);
}

__global__ void __launch_bounds__(256) k_choose_pick(ChooseArgs a)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > a.n_jobs) return;
    uint64_t x = ch_start(a, j);
    if (j == a.n_jobs) { *a.rng_out = x; return; }
    const uint64_t x0 = x;
    const int32_t na = a.n_aln[j];
    uint32_t type = 0, idx = 0, mapq = 0, n_mm = 0, draws = 0, nb = 0;
    uint64_t sa = 0, c1 = 0, c2 = 0, w0 = 0;
    if (na > 0) {
        const uint32_t *rec = a.hits + a.hit_off[j] * HSA_ALN64_WORDS;
        const int32_t best = ch_score(rec);
        int32_t i = 0;
        uint64_t cnt = 0;
        for (; i < na; ++i, rec += HSA_ALN64_WORDS) {                    // bwtse.c:40-55
            if (ch_score(rec) > best) break;
            uint64_t k;
            const uint64_t w = hsa_aln64_rows(rec, k);
            if (i == 0) w0 = w;
            ++nb;
            x = ch_step(x); ++draws;
            if (ch_real(x) * (double)(w + cnt) > (double)cnt) {
                x = ch_step(x); ++draws;
                idx = (uint32_t)i;
                n_mm = rec[0] & 0xFFFFu;
                sa = k + (uint64_t)((double)w * ch_real(x));
            }
            cnt += w;
        }
        c1 = cnt;
        for (; i < na; ++i, rec += HSA_ALN64_WORDS) {
            uint64_t k;
            cnt += hsa_aln64_rows(rec, k);
        }
        c2 = cnt - c1;
        type = c1 > 1 ? 2u : 1u;
        mapq = ch_mapq(a, c1, c2, n_mm, a.jobs[j].max_diff);
        atomicAdd(&a.ctr[3], 1ull);
        if (type == 2u) atomicAdd(&a.ctr[4], 1ull);
        // counted as two draws, made one: the states after this read are not the sequential ones
        if (!ch_variable(nb, w0) && draws != 2u) {
            atomicAdd(&a.ctr[6], 1ull);
            atomicMin(&a.ctr[7], (unsigned long long)j);
        }
    }
    const uint64_t rows = a.scn[j + 1].rows - a.scn[j].rows;
    reinterpret_cast<uint4 *>(a.sel)[j] = make_uint4(type, idx, mapq, rows ? (uint32_t)(rows - 1u) : 0u);
    reinterpret_cast<ulonglong2 *>(a.sel64)[2 * (size_t)j] = make_ulonglong2(sa, c1);
    reinterpret_cast<ulonglong2 *>(a.sel64)[2 * (size_t)j + 1] = make_ulonglong2(c2, x0);
}

__global__ void __launch_bounds__(256, 8) k_choose_rows(ChooseArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t total = a.pos_off[a.n_jobs];
    const uint64_t lim = total < a.pos_cap ? total : a.pos_cap;
    if (t == 0) { a.ctr[0] = total; a.ctr[1] = lim; }
    if (t >= lim) return;
    const uint32_t lo = hsa_row_read(a.pos_off, a.n_jobs, t);
    const uint64_t r = t - a.pos_off[lo];
    const uint32_t idx = a.sel[4 * (size_t)lo + 1];
    const uint64_t sa = a.sel64[4 * (size_t)lo];
    uint64_t row = sa;
    uint32_t hit = idx;
    if (r) {
        // the r-th row of the read's records in list order, k .. l ascending, the chosen one
        // left out (bwtse.c:360-366 drops the multi row at the main row's position)
        const uint32_t *rec = a.hits + a.hit_off[lo] * HSA_ALN64_WORDS;
        const int32_t na = a.n_aln[lo];
        uint64_t chosen = 0, k = 0;            // the chosen row's place among the read's rows
        for (int32_t i = 0; i < na && (uint32_t)i <= idx; ++i) {
            const uint64_t n = hsa_aln64_rows(rec + (size_t)i * HSA_ALN64_WORDS, k);
            if ((uint32_t)i < idx) chosen += n;
            else chosen = (sa >= k && sa - k < n) ? chosen + (sa - k) : 0u;   // (nothing chosen: the first row)
        }
        uint64_t rest = r - 1u;
        if (rest >= chosen) ++rest;
        int32_t i = 0;
        for (; i < na; ++i, rec += HSA_ALN64_WORDS) {
            const uint64_t n = hsa_aln64_rows(rec, k);
            if (rest < n) break;
            rest -= n;
        }
        if (i >= na) return;                   // (the counts and the lists disagree: not this call's)
        row = k + rest;
        hit = (uint32_t)i;
    }
    a.pos_hit[t] = hit;
    if (!hsa_sa_row64(a.v, row, a.pos + 4 * t)) atomicAdd(&a.ctr[2], 1ull);
}

static int g_choose_timing = 0;

extern "C" void hsa_choose_timing(int on) { g_choose_timing = on; }

extern "C" int hsa_choose_launch_times(hsa_index_t *ix, float *ms) { return hsa_stage_times(ix, &hsa_index::ch_t, ms, "hsa_choose"); }

extern "C" int hsa_choose_hits_device64(hsa_index_t *ix, const hsa_choose_batch64_t *b, void *stream)
{
    const char *what = "hsa_choose_hits_device64";
    if (int rc = hsa_need_sa64(ix, what)) return rc;
    if (!b || b->n_jobs < 0 || !b->d_pos_off || !b->d_counters || !b->d_rng_out || !b->d_log_n ||
        (b->n_jobs && (!b->d_jobs || !b->d_n_aln || !b->d_hit_off || !b->d_hits || !b->d_sel || !b->d_sel64)) ||
        (b->pos_cap && (!b->d_pos || !b->d_pos_hit))) {
        hsa_set_error("%s: bad arguments", what);
        return HSA_E_ARG;
    }
    if (b->rng_state > CH_MASK) { hsa_set_error("%s: a generator state of 2^48 or more", what); return HSA_E_ARG; }
    const uint64_t n = (uint64_t)b->n_jobs;
    const uint64_t most = n * ((uint64_t)b->n_multi + 1u) < b->pos_cap ? n * ((uint64_t)b->n_multi + 1u) : b->pos_cap;
    if ((most + 255) / 256 > 0x7FFFFFFFull) { hsa_set_error("%s: too many rows", what); return HSA_E_ARG; }
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    size_t tmp_bytes = 0;
    HSA_TRY(hsa_scan_bytes(tmp_bytes, ChCls{0, 0}, (size_t)(n + 1), ChPlus(), st));
    ChooseArgs A;
    void *d_tmp = nullptr;
    auto layout = [&](Carver c) {
        A.cls = c.take<ChCls>(n + 1);
        A.scn = c.take<ChCls>(n + 1);
        A.nbs = c.take<uint32_t>(n + 1);
        A.var_fix = c.take<uint32_t>(n + 1);
        A.var_nb = c.take<uint32_t>(n + 1);
        A.var_hoff = c.take<uint64_t>(n + 1);
        A.var_A = c.take<uint64_t>(n + 1);
        A.var_C = c.take<uint64_t>(n + 1);
        A.var_end = c.take<uint64_t>(n + 1);
        d_tmp = c.take<char>(tmp_bytes);
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_ch, &ix->d_ch_cap, layout(Carver())));
    layout(Carver(ix->d_ch));
    A.v = hsa_sa_view64(ix, hsa_sa_max_walk());
    A.jobs = b->d_jobs; A.n_aln = b->d_n_aln; A.hit_off = b->d_hit_off; A.hits = b->d_hits; A.log_n = b->d_log_n;
    A.n_jobs = (uint32_t)n; A.n_multi = b->n_multi; A.rng = b->rng_state;
    A.sel = b->d_sel; A.sel64 = b->d_sel64; A.rng_out = b->d_rng_out;
    A.pos_off = b->d_pos_off; A.pos = b->d_pos; A.pos_hit = b->d_pos_hit; A.pos_cap = b->pos_cap;
    A.ctr = (unsigned long long *)b->d_counters;
    const dim3 per_read((unsigned)((n + 1 + 255) / 256)), blk(256);
    StageTimer &tm = ix->ch_t;                 // records only when hsa_choose_timing asked for it
    HSA_TRY(tm.begin(g_choose_timing != 0));
    HSA_TRY(tm.mark(0, st));
    HSA_HIP(hipMemsetAsync(b->d_counters, 0, 8 * sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_choose_class, per_read, blk, 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(1, st));
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, A.cls, A.scn, ChCls{0, 0}, (size_t)(n + 1), ChPlus(), st));
    HSA_TRY(tm.mark(2, st));
    hipLaunchKernelGGL(k_choose_compact, per_read, blk, 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(3, st));
    if (n) {
        hipLaunchKernelGGL(k_choose_maps, dim3((unsigned)((n + 255) / 256)), blk, 0, st, A);
        HSA_HIP(hipGetLastError());
    }
    HSA_TRY(tm.mark(4, st));
    if (n) {
        hipLaunchKernelGGL(k_choose_walk, dim3(1), dim3(64), 0, st, A);
        HSA_HIP(hipGetLastError());
    }
    HSA_TRY(tm.mark(5, st));
    hipLaunchKernelGGL(k_choose_pick, per_read, blk, 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(6, st));
    hipLaunchKernelGGL(k_choose_rows, dim3(hsa_stage_blocks(most, 256)), blk, 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(7, st));
    tm.end();
    return 0;
}
