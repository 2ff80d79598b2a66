// hsa_rd_wave.h -- what the FASTQ loader (hsa_reads.hip) and the BAM loader (hsa_bam.hip)
// share of the per-record wavefront code: the wave-wide sum and maximum, and bwa_trim_read as
// a wave-wide walk over a quality the caller states per position.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RD_MIN_RDLEN 35u              // BWA_MIN_RDLEN, bwtaln.h:26

// The inclusive sum and the maximum over a wavefront's 64 lanes; every lane calls.
__device__ __forceinline__ int32_t rd_wave_scan(int32_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const int32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ int32_t rd_wave_max(int32_t v)
{
#pragma unroll
    for (uint32_t d = 32u; d; d >>= 1) {
        const int32_t t = __shfl_xor(v, (int)d, 64);
        v = t > v ? t : v;
    }
    return v;
}

// bwa_trim_read (bwaseqio.c:92-103) on a read of len bases whose quality at position l,
// 33 taken off, is qv(l): the length the read keeps.  The reference walks l from len - 1 down
// to RD_MIN_RDLEN with s += trim_qual - qv(l), ends at the first s < 0, and cuts at the l of
// the first strictly greater s.  Here 64 steps of the walk at a time, lane i at step p0 + i: a
// wave-wide inclusive sum on top of the carried one gives every step's s, a ballot the
// first negative one (the steps from there on do not count), a maximum over the steps
// before it the chunk's best s, and the lowest lane that holds it the largest l of equal
// maxima.  The carry (sum, best, best_l) and the trip count are the same in all lanes.
// (A lane without a step asks for the last position.)
template <class Q> __device__ __forceinline__ uint32_t rd_trim_walk(Q qv, uint32_t len, int32_t trim_qual, uint32_t lane)
{
    if (len <= RD_MIN_RDLEN) return len;
    const uint32_t steps = len - RD_MIN_RDLEN;
    int32_t sum = 0, best = 0;
    uint32_t best_l = len;
    for (uint32_t p0 = 0; p0 < steps; p0 += 64u) {
        const uint32_t p = p0 + lane;
        const bool on = p < steps;
        const uint32_t l = len - 1u - (on ? p : 0u);
        const int32_t v = qv(l);
        const int32_t s = sum + rd_wave_scan(on ? trim_qual - v : 0, lane);
        const unsigned long long neg = __ballot(on && s < 0);
        const uint32_t stop = neg ? (uint32_t)__ffsll((long long)neg) - 1u : 64u;
        const bool counts = on && lane < stop;
        const int32_t top = rd_wave_max(counts ? s : (int32_t)0x80000000);
        const unsigned long long at_top = __ballot(counts && s == top);
        if (top > best) {
            best = top;
            best_l = len - (p0 + (uint32_t)__ffsll((long long)at_top));      // len - 1 - step
        }
        if (neg) break;
        sum = __shfl(s, 63, 64);
    }
    return best_l;
}
