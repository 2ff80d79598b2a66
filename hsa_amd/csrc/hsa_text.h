// hsa_text.h -- the reference text on the device, read through one accessor (in the
// spirit of SaView64, hsa_sa.h).
//
// Two layouts reach the kernels:
//   lsb = 1  the 64-bit builder's input (hsa_index_set_text64_device): 2-bit codes,
//            LSB-first, 16 per u32, n = T characters (any length under 2^36);
//   lsb = 0  the host's packed text (hsa_index_set_text): the HSP's words, the first
//            code in the high bits (hsp->packedDNA[k>>4] >> ((~k&15)<<1) & 3,
//            bwtse.c:394), n = dnaLength.
// `lsb` is a kernel argument, so the branch on it is wave-uniform.
#pragma once
#include <stdint.h>

#include "hsa_device.h"

struct TextView {
    const uint32_t *w;             // ceil(n / 16) words
    uint64_t n;                    // characters (the reference's hsp->dnaLength)
    uint32_t lsb;
};

// Word wi (characters 16 wi .. 16 wi + 15) with character 16 wi + r at bits 2r + 1 : 2r.
__device__ __forceinline__ uint32_t hsa_text_word(const TextView &t, uint64_t wi)
{
    uint32_t x = t.w[wi];
    if (!t.lsb) {                  // MSB-first: reverse the sixteen 2-bit groups
        x = __brev(x);
        x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    }
    return x;
}

// Character p (p < n).
__device__ __forceinline__ uint32_t hsa_text_code(const TextView &t, uint64_t p)
{
    return (hsa_text_word(t, p >> 4) >> (2u * ((uint32_t)p & 15u))) & 3u;
}
