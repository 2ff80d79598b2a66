// hsa_inflate.hip -- hsa_inflate_bgzf_device: the members of a BGZF file, one wavefront each.
//
// A member's DEFLATE stream is serial, the members are independent: a workgroup is one wave
// and takes one member.  All 64 lanes run the serial core of hsa_inflate.h with the same
// values (no divergence, no broadcasts; the code tables, 1.4 KB in LDS, are read by the lane
// that wrote them) and share what is parallel:
//   * literals: lane p % 64 keeps the byte of output position p; 64 of them leave in one
//     coalesced store;
//   * a match: lane i copies bytes i, i + 64, ... of it, each from src + i % distance, which
//     also repeats the period of an overlapping match (distance < length);
//   * the CRC32: every lane takes one 64th of the block and the terms are combined with
//     multiplications in GF(2)[x] (hsa_inflate.h).
// The window is the block's slice of the output in global memory (64 KB per wave do not fit
// LDS at any occupancy).  A match may read bytes that other lanes of the wave stored: stores
// and loads are ordered by a workgroup-scope fence (the wave's lanes share one L1), taken
// only when the source reaches past the last fence.
#include <cstring>
#include <hip/hip_runtime.h>
#include <string.h>

#include "hsa_internal.h"
#include "hsa_inflate.h"

namespace {

struct WaveSink {
    uint8_t *out;                      // the block's slice
    uint32_t isize;
    uint32_t lane;
    uint32_t pos = 0;                  // bytes emitted
    uint32_t flushed = 0;              // bytes stored; [flushed, pos) wait in `mine`, at most 64
    uint32_t synced = 0;               // bytes stored before the last fence
    uint32_t mine = 0;

    __device__ __forceinline__ void flush()
    {
        const uint32_t p = flushed + ((lane - flushed) & 63u);
        if (p < pos) out[p] = (uint8_t)mine;
        flushed = pos;
    }
    __device__ __forceinline__ void fence()
    {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        synced = flushed;
    }
    __device__ __forceinline__ int literal(uint8_t c)
    {
        if (pos >= isize) return HSA_INF_E_OUTPUT;
        if ((pos & 63u) == lane) mine = c;
        ++pos;
        if (pos - flushed == 64u) flush();
        return 0;
    }
    __device__ __forceinline__ int match(uint32_t dist, uint32_t len)
    {
        if (dist > pos) return HSA_INF_E_DIST;
        if (len > isize - pos) return HSA_INF_E_OUTPUT;
        flush();
        const uint32_t src = pos - dist;
        if (src + (dist < len ? dist : len) > synced) fence();
        for (uint32_t i = lane; i < len; i += 64u)
            out[pos + i] = out[src + (i < dist ? i : i % dist)];
        pos += len;
        flushed = pos;
        return 0;
    }
};

__global__ __launch_bounds__(64) void k_inflate_bgzf(const uint8_t *__restrict__ in, uint64_t n_in,
                                                     const hsa_bgzf_block_t *__restrict__ blocks, uint8_t *out,
                                                     uint64_t out_cap, uint32_t *__restrict__ status,
                                                     unsigned long long *ctr)
{
    __shared__ InfTables tables;
    __shared__ uint32_t crc_tab[256];
    const uint32_t lane = threadIdx.x;
    const hsa_bgzf_block_t row = blocks[blockIdx.x];
    for (uint32_t i = lane; i < 256u; i += 64u) crc_tab[i] = inf_crc_entry(i);
    __syncthreads();

    uint32_t st;
    if (row.in_off > n_in || row.in_len > n_in - row.in_off || row.out_off > out_cap || row.isize > out_cap - row.out_off) {
        st = HSA_INF_E_ROW;
    } else {
        InfBits bits;
        inf_open(bits, in + row.in_off, row.in_len);
        WaveSink sink{out + row.out_off, row.isize, lane};
        st = (uint32_t)inf_stream(bits, tables, sink);
        if (st == HSA_INF_OK && sink.pos != row.isize) st = HSA_INF_E_SIZE;
        if (st == HSA_INF_OK) {
            sink.flush();
            sink.fence();
            uint32_t term = inf_crc_term(crc_tab, sink.out, row.isize, lane, 64u);
            for (int m = 32; m; m >>= 1) term ^= __shfl_xor(term, m, 64);
            if (~term != row.crc) st = HSA_INF_E_CRC;
        }
    }
    if (lane == 0) {
        status[blockIdx.x] = st;
        if (st == HSA_INF_OK) {
            atomicAdd(&ctr[0], 1ull);
            atomicAdd(&ctr[2], (unsigned long long)row.isize);
        } else {
            atomicAdd(&ctr[1], 1ull);
        }
    }
}

}  // namespace

extern "C" int hsa_inflate_bgzf_device(int device, const hsa_inflate_batch_t *b, void *stream)
{
    const char *what = "hsa_inflate_bgzf_device";
    if (!b || !b->d_counters || (b->n_blocks && (!b->d_blocks || !b->d_status)) || (b->n_in && !b->d_in) ||
        (b->out_cap && !b->d_out)) {
        hsa_set_error("%s: null argument", what);
        return HSA_E_ARG;
    }
    if (b->n_blocks >= 0x80000000ull) { hsa_set_error("%s: under 2^31 blocks per call", what); return HSA_E_ARG; }
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) { hsa_set_error("%s: no HIP device visible", what); return HSA_E_NODEV; }
    if (device < 0 || device >= nd) { hsa_set_error("%s: device %d of %d", what, device, nd); return HSA_E_ARG; }
    HSA_HIP(hipSetDevice(device));
    if (!b->n_blocks) return 0;
    hipLaunchKernelGGL(k_inflate_bgzf, dim3((unsigned)b->n_blocks), dim3(64), 0, (hipStream_t)stream, b->d_in, b->n_in,
                       b->d_blocks, b->d_out, b->out_cap, b->d_status, (unsigned long long *)b->d_counters);
    HSA_HIP(hipGetLastError());
    return 0;
}
