// hsa_sam_sinks.h -- the byte sinks and small formatters of the SAM writers (hsa_sam.hip,
// hsa_splice_rows.hip): one emit function walks the fields of a line for a sink that counts
// and for one that stores, so the length and the bytes cannot disagree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SM_FWD 0x4E54474341ull     // "ACGTN", first letter in the low byte (bwtse.c:737-742)
#define SM_REV 0x4E41434754ull     // "TGCAN"
__device__ __forceinline__ uint32_t sm_digits(uint64_t v)
{
    uint32_t n = 1;
    for (; v >= 10u; v /= 10u) ++n;
    return n;
}

// The sinks.  pos(): where the next byte goes; skip(): a field another phase fills.
struct SmCount {
    uint64_t n = 0;
    __device__ __forceinline__ uint32_t pos() const { return 0; }
    __device__ __forceinline__ void ch(char) { ++n; }
    __device__ __forceinline__ void skip(uint64_t k) { n += k; }
    __device__ __forceinline__ void dec(uint64_t v) { n += sm_digits(v); }
    __device__ __forceinline__ void bytes(const uint8_t *, uint32_t k) { n += k; }
    template <int N> __device__ __forceinline__ void lit(const char (&)[N]) { n += N - 1; }
};
struct SmStore {
    uint8_t *buf;
    uint32_t p, cap;
    __device__ __forceinline__ uint32_t pos() const { return p; }
    __device__ __forceinline__ void at(uint32_t q, uint32_t c) { if (q < cap) buf[q] = (uint8_t)c; }
    __device__ __forceinline__ void ch(char c) { at(p, (uint8_t)c); ++p; }
    __device__ __forceinline__ void skip(uint64_t k) { p += (uint32_t)k; }
    __device__ __forceinline__ void dec(uint64_t v)
    {
        const uint32_t n = sm_digits(v);
        for (uint32_t i = n; i-- > 0u; v /= 10u) at(p + i, '0' + (uint32_t)(v % 10u));
        p += n;
    }
    __device__ __forceinline__ void bytes(const uint8_t *s, uint32_t k)
    {
        for (uint32_t i = 0; i < k; i += 8u) {     // eight loads, then their stores: one wait
            uint32_t v[8];
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) v[q] = s[i + q < k ? i + q : i];
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q)
                if (i + q < k) at(p + i + q, v[q]);
        }
        p += k;
    }
    template <int N> __device__ __forceinline__ void lit(const char (&s)[N])
    {
#pragma unroll
        for (int i = 0; i < N - 1; ++i) at(p + i, (uint8_t)s[i]);
        p += N - 1;
    }
};

__device__ __forceinline__ uint32_t sm_op_letter(uint32_t op)
{
    // "MIDNSHP=X" (bwtse.c:713): eight letters in a word, X apart
    return op < 8u ? (uint32_t)(0x3D504853'4E44494Dull >> (8u * op)) & 0xFFu : (uint32_t)'X';
}

// A CIGAR of n ops with bwa_correct_trimmed applied while it is printed (bwtse.c:496-534): the
// `clip` bases that trimming took off the read's end join a last S op on the forward strand
// and a first one on the reverse strand, or are an S op of their own there (a read without
// a CIGAR is "<len>M" in `ops` already).  clip == 0: the ops as they are.
template <class S> __device__ __forceinline__ void sm_cigar_clipped(const uint32_t *ops, uint32_t n, uint32_t strand, uint32_t clip, S &s)
{
    if (clip && strand && (n == 0u || (ops[0] >> 28) != 4u)) { s.dec(clip); s.ch('S'); }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t w = ops[i], op = w >> 28;
        const bool edge = clip && op == 4u && i == (strand ? 0u : n - 1u);
        s.dec((uint64_t)(w & 0x0FFFFFFFu) + (edge ? clip : 0u));
        s.ch((char)sm_op_letter(op));
    }
    if (clip && !strand && (n == 0u || (ops[n - 1u] >> 28) != 4u)) { s.dec(clip); s.ch('S'); }
}

// The tags between QUAL and XT (bwtse.c:755-758): BC:Z with the read's barcode, XC:i with
// clip_len where the read was trimmed
template <class S> __device__ __forceinline__ void sm_clip_tags(const uint8_t *bc, uint32_t bc_len, uint32_t len, uint32_t full, S &s)
{
    if (bc && bc_len) { s.lit("\tBC:Z:"); s.bytes(bc, bc_len); }
    if (len < full) { s.lit("\tXC:i:"); s.dec(len); }
}
