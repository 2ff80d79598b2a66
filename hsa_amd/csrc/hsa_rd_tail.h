// hsa_rd_tail.h -- the tail of a read loader that does not depend on the input's format, stated
// once for the FASTQ loader (hsa_reads.hip, RdArgs) and the BAM loader (hsa_bam.hip, BamArgs):
// the longest loaded read, the status per record with the three lengths of a kept read for the
// scan, and a record's row and job.  Each loader's kernels say how many records it loaded (a
// functor `loaded`: the line table there, the record chain here) and call these bodies.
//
// A: the loader's argument struct, with g (g[1]: the longest loaded read, g[2]: the longest
// kept one), r_len, r_nn, r_fl, r_name_len, r_full (may be null: the length is the full one),
// s_in / s_out (M + 1 entries), M, maxdiff / len_floor / max_diff, seed_len, regime, octr (may be
// null), rec, jobs / job_cap, name_off, qual_off, full_len (may be null).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsa_gpu.h"    // hsa_job_t, HSA_RD_*

#define RD_FL_FILTERED 0x80u          // r_fl between the record kernel and the keep kernel: the reader skips the record

struct Rd3 {
    uint64_t j, c, n;       // jobs, code bytes, name bytes
};
struct Rd3Plus {
    __host__ __device__ Rd3 operator()(const Rd3 &a, const Rd3 &b) const { return Rd3{a.j + b.j, a.c + b.c, a.n + b.n}; }
};

template <class A, class L> __device__ __forceinline__ void rd_tail_max(const A &a, L loaded)
{
    __shared__ uint32_t sMax;
    if (threadIdx.x == 0) sMax = 0u;
    __syncthreads();
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < loaded() && a.r_fl[k] != RD_FL_FILTERED) atomicMax(&sMax, a.r_len[k]);
    __syncthreads();
    if (threadIdx.x == 0 && sMax) atomicMax(&a.g[1], sMax);
}

// bwtaln.c:273-274: local_opt.max_diff before the option switch
template <class A> __device__ __forceinline__ int32_t rd_threshold(const A &a)
{
    return a.maxdiff ? a.maxdiff[a.g[1] > a.len_floor ? a.g[1] : a.len_floor] : a.max_diff;
}

template <class A, class L> __device__ __forceinline__ void rd_tail_keep(const A &a, L loaded)
{
    __shared__ uint32_t sMax, sTrim, sTotal;               // (a block's bases: 256 reads of at most 65 535)
    if (threadIdx.x == 0) sMax = sTrim = sTotal = 0u;
    __syncthreads();
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k <= a.M) {
        Rd3 v{0, 0, 0};
        if (k < loaded()) {
            const uint32_t fl = a.r_fl[k], len = a.r_len[k];
            const uint32_t full = a.r_full ? a.r_full[k] : len;             // the code and quality bytes stay whole
            const uint32_t st = fl == RD_FL_FILTERED ? HSA_RD_FILTERED : (int64_t)a.r_nn[k] > (int64_t)rd_threshold(a) ? HSA_RD_NDROP
                                : fl ? HSA_RD_POLYAT : HSA_RD_SEARCHED;
            a.r_fl[k] = st;
            if (st == HSA_RD_SEARCHED) {
                v = Rd3{1u, full, a.r_name_len[k]};
                atomicMax(&sMax, len);
            }
            if (a.octr && st != HSA_RD_FILTERED) {                          // bwaseqio.c:204, :210: every read returned
                atomicAdd(&sTotal, full);
                if (full != len) atomicAdd(&sTrim, full - len);
            }
        }
        a.s_in[k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0 && sMax) atomicMax(&a.g[2], sMax);
    if (threadIdx.x == 0 && sTotal) {                                       // (sums: any order gives the same)
        atomicAdd(&a.octr[3], (unsigned long long)sTotal);
        if (sTrim) atomicAdd(&a.octr[2], (unsigned long long)sTrim);
    }
}

// Record k's row, and the job and offsets of a kept one
template <class A> __device__ __forceinline__ void rd_tail_row(const A &a, uint32_t k)
{
    const uint32_t st = a.r_fl[k], len = a.r_len[k];
    const Rd3 at = a.s_out[k];
    const bool kept = st == HSA_RD_SEARCHED;
    uint32_t *row = a.rec + (size_t)HSA_RD_ROW_WORDS * k;
    const bool skipped = st == HSA_RD_FILTERED;          // (no read: no length, no count)
    row[0] = st; row[1] = skipped ? 0u : len; row[2] = skipped ? 0u : a.r_nn[k]; row[3] = kept ? (uint32_t)at.j : 0xFFFFFFFFu;
    if (kept && at.j <= a.job_cap) {
        a.name_off[at.j] = at.n;
        a.qual_off[at.j] = at.c;
        if (at.j < a.job_cap) {
            hsa_job_t jb;
            jb.off = at.c; jb.len = len;
            jb.max_diff = a.maxdiff ? a.maxdiff[len] : a.max_diff;                    // bwtaln.c:330-331
            jb.seed_len = a.seed_len < (int32_t)len ? a.seed_len : 0x7fffffff;        // :332
            jb.regime = a.regime;
            a.jobs[at.j] = jb;
            if (a.full_len) a.full_len[at.j] = a.r_full ? a.r_full[k] : len;
        }
    }
}
