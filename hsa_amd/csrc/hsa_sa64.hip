// hsa_sa64.hip -- SA index -> text position for a 64-bit index (texts of 2^32
// characters or more), and the hit lists of hsa_search_device64 to positions.
//
// The walk and the block search: hsa_sa.h (SaView64).  No reference counterpart (the
// reference's bwtint_t is 32-bit); the 32-bit path is hsa_sa.hip.
//
// hsa_hit_positions_device64 is three launches on one stream, no host round trip:
//   k_hitpos_count   one lane per read: its rows, cut to max_occ;
//   rocPRIM exclusive scan of the counts: d_pos_off, in read order;
//   k_hitpos_rows    one lane per OUTPUT ROW: the read by binary search of d_pos_off,
//                    then the record and the row within it, then the walk.
// One lane per row, not per read: a walk is a chain of dependent random 16-byte loads
// (about interval / 2 of them), and a repeat read's max_occ rows in one lane would be
// max_occ such chains back to back while the lane's wave waits.  The only lever on a
// dependent chain is the number of independent chains in flight, so the kernels keep
// their registers within 8 waves per SIMD and use no LDS.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdlib.h>
#include <string.h>

#include "hsa_device.h"
#include "hsa_internal.h"
#include "hsa_sa.h"

#define HSA_SA_MAX_WALK_DEFAULT (1u << 22)

uint32_t hsa_sa_max_walk()
{
    const char *e = getenv("HSA_SA_MAX_WALK");
    if (!e || !*e) return HSA_SA_MAX_WALK_DEFAULT;
    const unsigned long long v = strtoull(e, nullptr, 0);
    return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
}

SaView64 hsa_sa_view64(const hsa_index *ix, uint32_t max_walk)
{
    SaView64 v;
    v.d = hsa_rank_dir64(ix, 0);
    v.T = ix->T64;
    memcpy(v.C, ix->C64, sizeof v.C);
    v.sa = ix->d_sa64; v.interval = ix->sa64_interval;
    v.pow2 = v.interval && (v.interval & (v.interval - 1u)) == 0;
    v.shift = v.pow2 ? (uint32_t)__builtin_ctz(v.interval) : 0u;
    v.blocks = ix->d_blocks64; v.n_blocks = ix->n_blocks64;
    v.max_walk = max_walk;
    return v;
}

struct Sa64Args {
    SaView64 v;
    const uint64_t *idx;
    uint64_t *out;                 // 4 u64 per index: sa value, seq id, 1-based position, text position
    size_t n;
};

__global__ void __launch_bounds__(256, 8) k_sa_position64(Sa64Args a)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n) return;
    hsa_sa_row64(a.v, a.idx[t], a.out + 4 * t);
}

// one LF step per index; the '$' row (and an index past T) answers 0
__global__ void __launch_bounds__(256) k_psi_minus64(Sa64Args a)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n) return;
    const uint64_t i = a.idx[t];
    a.out[t] = (i == a.v.d.isa0 || i > a.v.T) ? 0ull : hsa_psi_minus64(a.v, i);
}

static int need_wide(const hsa_index *ix, const char *what)
{
    if (!ix) { hsa_set_error("%s: null handle", what); return HSA_E_ARG; }
    if (!ix->wide) { hsa_set_error("%s: not a 64-bit index (hsa_index_create_device64)", what); return HSA_E_ARG; }
    return 0;
}

int hsa_need_sa64(const hsa_index *ix, const char *what)
{
    if (int rc = need_wide(ix, what)) return rc;
    if (!ix->d_sa64) { hsa_set_error("%s: no suffix array attached (hsa_index_set_sa64)", what); return HSA_E_ARG; }
    return 0;
}

// d_vals: a device array the index takes (own = true) or null with host values to upload
static int set_sa64(hsa_index *ix, const uint64_t *h_vals, uint64_t *d_vals, uint64_t n_values, uint32_t interval,
                    const uint64_t *blocks, int n_blocks, const char *what)
{
    if (int rc = need_wide(ix, what)) return rc;
    if ((!h_vals && !d_vals) || interval == 0 || n_values == 0 || n_blocks < 0 || (n_blocks && !blocks)) {
        hsa_set_error("%s: bad arguments", what);
        return HSA_E_ARG;
    }
    if (int rc = hsa_need_unshared(ix, what)) return rc;
    if (n_values < (ix->T64 + interval) / interval) {
        hsa_set_error("%s: %llu values < (T + s) / s", what, (unsigned long long)n_values);
        return HSA_E_ARG;
    }
    HSA_HIP(hipSetDevice(ix->device));
    uint64_t *nb = nullptr, *nv = d_vals;
    if (hipMalloc(&nb, (size_t)(n_blocks ? n_blocks : 1) * 32) != hipSuccess ||
        (!d_vals && hipMalloc(&nv, n_values * 8) != hipSuccess)) {
        (void)hipGetLastError();
        (void)hipFree(nb);
        hsa_set_error("%s: hipMalloc failed", what);
        return HSA_E_MEM;
    }
    hipError_t e = hipSuccess;
    if (!d_vals) e = hipMemcpy(nv, h_vals, n_values * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && n_blocks) e = hipMemcpy(nb, blocks, (size_t)n_blocks * 32, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(nb);
        if (!d_vals) (void)hipFree(nv);
        hsa_set_error("%s: %s", what, hipGetErrorString(e));
        return HSA_E_HIP;
    }
    HSA_HIP(hipStreamSynchronize(ix->stream));     // no walk of the old arrays in flight
    (void)hipFree(ix->d_sa64); (void)hipFree(ix->d_blocks64);
    ix->d_sa64 = nv; ix->d_blocks64 = nb;
    ix->sa64_interval = interval;
    ix->n_blocks64 = (uint32_t)n_blocks;
    return 0;
}

extern "C" int hsa_index_set_sa64(hsa_index_t *ix, const uint64_t *sa_values, uint64_t n_values, uint32_t interval,
                                  const uint64_t *blocks, int n_blocks)
{
    return set_sa64(ix, sa_values, nullptr, n_values, interval, blocks, n_blocks, "hsa_index_set_sa64");
}

extern "C" int hsa_index_set_sa64_device(hsa_index_t *ix, uint64_t *d_sa_values, uint64_t n_values, uint32_t interval,
                                         const uint64_t *blocks, int n_blocks)
{
    if (!d_sa_values) { hsa_set_error("hsa_index_set_sa64_device: bad arguments"); return HSA_E_ARG; }
    return set_sa64(ix, nullptr, d_sa_values, n_values, interval, blocks, n_blocks, "hsa_index_set_sa64_device");
}

extern "C" int hsa_sa_position_device64(hsa_index_t *ix, size_t n, const uint64_t *d_idx, uint64_t *d_out4, void *stream)
{
    if (int rc = hsa_need_sa64(ix, "hsa_sa_position_device64")) return rc;
    if (n && (!d_idx || !d_out4)) { hsa_set_error("hsa_sa_position_device64: null argument"); return HSA_E_ARG; }
    if ((n + 255) / 256 > 0x7FFFFFFFull) { hsa_set_error("hsa_sa_position_device64: too many indices"); return HSA_E_ARG; }
    HSA_HIP(hipSetDevice(ix->device));
    Sa64Args A;
    A.v = hsa_sa_view64(ix, hsa_sa_max_walk());
    A.idx = d_idx; A.out = d_out4; A.n = n;
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    if (n) hipLaunchKernelGGL(k_sa_position64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    return 0;
}

extern "C" int hsa_sa_position_batch64(hsa_index_t *ix, size_t n, const uint64_t *sa_index, uint64_t *out4)
{
    if (int rc = hsa_need_sa64(ix, "hsa_sa_position_batch64")) return rc;
    if (n && (!sa_index || !out4)) { hsa_set_error("hsa_sa_position_batch64: null argument"); return HSA_E_ARG; }
    int rc;
    if ((rc = hsa_grow(&ix->d_in, &ix->d_in_cap, n * 8 + 64)) || (rc = hsa_grow(&ix->d_out, &ix->d_out_cap, n * 32 + 64)))
        return rc;
    ix->staged_valid = 0;                      // d_in no longer holds the staged regimes
    HSA_HIP(hipSetDevice(ix->device));
    HSA_HIP(hipMemcpyAsync(ix->d_in, sa_index, n * 8, hipMemcpyHostToDevice, ix->stream));
    if ((rc = hsa_sa_position_device64(ix, n, (const uint64_t *)ix->d_in, (uint64_t *)ix->d_out, ix->stream))) return rc;
    HSA_HIP(hipMemcpyAsync(out4, ix->d_out, n * 32, hipMemcpyDeviceToHost, ix->stream));
    HSA_HIP(hipStreamSynchronize(ix->stream));
    return 0;
}

extern "C" int hsa_psi_minus_batch64(hsa_index_t *ix, size_t n, const uint64_t *sa_index, uint64_t *out)
{
    if (int rc = need_wide(ix, "hsa_psi_minus_batch64")) return rc;
    if (n && (!sa_index || !out)) { hsa_set_error("hsa_psi_minus_batch64: null argument"); return HSA_E_ARG; }
    for (size_t i = 0; i < n; ++i)
        if (sa_index[i] > ix->T64) {
            hsa_set_error("hsa_psi_minus_batch64: index %llu > T", (unsigned long long)sa_index[i]);
            return HSA_E_ARG;
        }
    if ((n + 255) / 256 > 0x7FFFFFFFull) { hsa_set_error("hsa_psi_minus_batch64: too many indices"); return HSA_E_ARG; }
    int rc;
    if ((rc = hsa_grow(&ix->d_in, &ix->d_in_cap, n * 8 + 64)) || (rc = hsa_grow(&ix->d_out, &ix->d_out_cap, n * 8 + 64)))
        return rc;
    ix->staged_valid = 0;
    HSA_HIP(hipSetDevice(ix->device));
    HSA_HIP(hipMemcpyAsync(ix->d_in, sa_index, n * 8, hipMemcpyHostToDevice, ix->stream));
    Sa64Args A;
    A.v = hsa_sa_view64(ix, 0);                // the step reads neither the samples nor the blocks
    A.idx = (const uint64_t *)ix->d_in; A.out = (uint64_t *)ix->d_out; A.n = n;
    if (n) hipLaunchKernelGGL(k_psi_minus64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ix->stream, A);
    HSA_HIP(hipGetLastError());
    HSA_HIP(hipMemcpyAsync(out, ix->d_out, n * 8, hipMemcpyDeviceToHost, ix->stream));
    HSA_HIP(hipStreamSynchronize(ix->stream));
    return 0;
}

// ---------------------------------------------------------------- hit lists -> positions
struct HitPosArgs {
    SaView64 v;
    const int32_t *n_aln;
    const uint64_t *hit_off;
    const uint32_t *hits;
    uint32_t n_jobs, max_occ;
    uint64_t *pos_off;             // n_jobs + 1
    uint64_t *pos;
    uint32_t *pos_hit;
    uint64_t pos_cap;
    unsigned long long *ctr;
};

// counts[j]: the rows of read j, at most max_occ; counts[n_jobs] = 0 (the scan's last slot)
__global__ void __launch_bounds__(256) k_hitpos_count(HitPosArgs a, uint64_t *counts)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > a.n_jobs) return;
    uint64_t n = 0;
    if (j < a.n_jobs) {
        const int32_t na = a.n_aln[j];
        const uint32_t *rec = a.hits + a.hit_off[j] * HSA_ALN64_WORDS;
        for (int32_t i = 0; i < na && n < a.max_occ; ++i, rec += HSA_ALN64_WORDS) {
            uint64_t k;
            n += hsa_aln64_rows(rec, k);
        }
        if (n > a.max_occ) n = a.max_occ;
    }
    counts[j] = n;
}

__global__ void __launch_bounds__(256, 8) k_hitpos_rows(HitPosArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t total = a.pos_off[a.n_jobs];
    const uint64_t lim = total < a.pos_cap ? total : a.pos_cap;
    if (t == 0) { a.ctr[0] = total; a.ctr[1] = lim; }
    if (t >= lim) return;
    const uint32_t lo = hsa_row_read(a.pos_off, a.n_jobs, t);
    uint64_t rest = t - a.pos_off[lo];
    // the record and the row within it: rest < the read's rows <= the sum of its records' rows
    const uint32_t *rec = a.hits + a.hit_off[lo] * HSA_ALN64_WORDS;
    const int32_t na = a.n_aln[lo];
    uint64_t k = 0;
    int32_t i = 0;
    for (; i < na; ++i, rec += HSA_ALN64_WORDS) {
        const uint64_t n = hsa_aln64_rows(rec, k);
        if (rest < n) break;
        rest -= n;
    }
    if (i >= na) return;                       // (the counts and the lists disagree: not this call's)
    a.pos_hit[t] = (uint32_t)i;
    if (!hsa_sa_row64(a.v, k + rest, a.pos + 4 * t)) atomicAdd(&a.ctr[2], 1ull);
}

extern "C" int hsa_hit_positions_device64(hsa_index_t *ix, const hsa_hitpos_batch64_t *b, void *stream)
{
    if (int rc = hsa_need_sa64(ix, "hsa_hit_positions_device64")) return rc;
    if (!b || b->n_jobs < 0 || b->max_occ == 0 || !b->d_pos_off || !b->d_counters ||
        (b->n_jobs && (!b->d_n_aln || !b->d_hit_off || !b->d_hits)) || (b->pos_cap && (!b->d_pos || !b->d_pos_hit))) {
        hsa_set_error("hsa_hit_positions_device64: bad arguments");
        return HSA_E_ARG;
    }
    const uint64_t n = (uint64_t)b->n_jobs;
    const uint64_t most = n * b->max_occ < b->pos_cap ? n * b->max_occ : b->pos_cap;   // rows that can be written
    if ((most + 255) / 256 > 0x7FFFFFFFull) { hsa_set_error("hsa_hit_positions_device64: too many rows"); return HSA_E_ARG; }
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    size_t tmp_bytes = 0;
    HSA_TRY(hsa_scan_bytes(tmp_bytes, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
    // scratch: the counts, then the scan's temporary storage
    uint64_t *d_cnt = nullptr;
    void *d_tmp = nullptr;
    auto layout = [&](Carver c) {
        d_cnt = c.take<uint64_t>(n + 1);
        d_tmp = c.take<char>(tmp_bytes);
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_hp, &ix->d_hp_cap, layout(Carver())));
    layout(Carver(ix->d_hp));
    HitPosArgs A;
    A.v = hsa_sa_view64(ix, hsa_sa_max_walk());
    A.n_aln = b->d_n_aln; A.hit_off = b->d_hit_off; A.hits = b->d_hits;
    A.n_jobs = (uint32_t)n; A.max_occ = b->max_occ;
    A.pos_off = b->d_pos_off; A.pos = b->d_pos; A.pos_hit = b->d_pos_hit; A.pos_cap = b->pos_cap;
    A.ctr = (unsigned long long *)b->d_counters;
    HSA_HIP(hipMemsetAsync(b->d_counters, 0, 4 * sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_hitpos_count, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, A, d_cnt);
    HSA_HIP(hipGetLastError());
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, d_cnt, b->d_pos_off, (uint64_t)0, (size_t)(n + 1),
                                    rocprim::plus<uint64_t>(), st));
    hipLaunchKernelGGL(k_hitpos_rows, dim3(hsa_stage_blocks(most, 256)), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    return 0;
}
