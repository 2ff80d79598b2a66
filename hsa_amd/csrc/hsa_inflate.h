// hsa_inflate.h -- the serial core of the BGZF inflater (hsa_inflate.hip): DEFLATE (RFC 1951)
// for one payload, written once for the device and for plain host C++.  The bit reader, the
// code tables built from code lengths and the symbol loop are here, with every bounds check;
// what a decoded symbol does to the output is the sink's: emit a literal, copy a match.  The
// kernel passes a sink whose 64 lanes share the copies, a host program a byte loop, and so
// the checks that keep a corrupt payload inside the buffers run under a host sanitizer too.
//
// Every lane of the kernel's wave runs this code with the same values (uniform control flow):
// a table entry is read by the lane that wrote it, so the tables in LDS need no barrier.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/hsa_gpu.h"

#ifdef __HIPCC__
#define HSA_INF_HD __host__ __device__ __forceinline__
#else
#define HSA_INF_HD inline
#endif

#define HSA_INF_TRY(call) do { if (int rc_ = (call)) return rc_; } while (0)

// Canonical codes: count[l] codes of length l, their symbols in order of (length, symbol).
struct InfTables {
    uint16_t lcount[16], lsym[288];    // literal/length code (and, while a dynamic header is read, the code-length code)
    uint16_t dcount[16], dsym[32];     // distance code
    uint16_t offs[16];                 // inf_build's first slot per length
    uint8_t lens[320];                 // the code lengths a header gives: 286 + 30 at most
};

// The payload's bits, LSB first.  `ahead` holds the next four bytes, loaded when the four
// before them went into buf, so that the load's latency passes while they are decoded.
struct InfBits {
    const uint8_t *p;
    uint32_t n, pos;                   // pos: the first byte neither in buf nor consumed (ahead's, when has)
    uint64_t buf;
    uint32_t cnt;                      // bits in buf
    uint32_t ahead;
    bool has;
};

HSA_INF_HD void inf_fetch(InfBits &b)
{
    b.has = b.n - b.pos >= 4u;
    if (b.has) memcpy(&b.ahead, b.p + b.pos, 4);         // (little endian on both sides)
}

HSA_INF_HD void inf_open(InfBits &b, const uint8_t *p, uint32_t n)
{
    b.p = p; b.n = n; b.pos = 0; b.buf = 0; b.cnt = 0; b.ahead = 0;
    inf_fetch(b);
}

// At least 32 bits in buf unless the payload ends first; no byte at or past p + n is read.
HSA_INF_HD void inf_refill(InfBits &b)
{
    if (b.cnt > 32u) return;
    if (b.has) {
        b.buf |= (uint64_t)b.ahead << b.cnt;
        b.cnt += 32u;
        b.pos += 4u;
        inf_fetch(b);
    } else {
        while (b.cnt <= 56u && b.pos < b.n) {
            b.buf |= (uint64_t)b.p[b.pos++] << b.cnt;
            b.cnt += 8u;
        }
    }
}

// need <= 16
HSA_INF_HD int inf_bits(InfBits &b, uint32_t need, uint32_t &v)
{
    if (b.cnt < need) {
        inf_refill(b);
        if (b.cnt < need) return HSA_INF_E_INPUT;
    }
    v = (uint32_t)b.buf & ((1u << need) - 1u);
    b.buf >>= need;
    b.cnt -= need;
    return 0;
}

// Whole payload bytes not consumed yet.
HSA_INF_HD uint32_t inf_bytes_left(const InfBits &b) { return (b.n - b.pos) + (b.cnt >> 3); }

// One symbol of a canonical code: a code of length l is the l bits read so far, first bit
// highest; `first` is the first code of that length and `index` its slot in symbol[].
HSA_INF_HD int inf_decode(InfBits &b, const uint16_t *count, const uint16_t *symbol, uint32_t &sym)
{
    if (b.cnt < 15u) inf_refill(b);
    uint64_t bits = b.buf;
    int32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= 15u; ++len) {
        if (len > b.cnt) return HSA_INF_E_INPUT;
        code |= (int32_t)(bits & 1u);
        bits >>= 1;
        const int32_t c = count[len];
        if (code - c < first) {
            sym = symbol[index + (code - first)];
            b.buf = bits;
            b.cnt -= len;
            return 0;
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return HSA_INF_E_SYMBOL;
}

// count[] and symbol[] of the n code lengths in lens (each 0..15).  Returns what the set
// leaves of the code space: 0 complete (or no code at all), > 0 incomplete, < 0
// over-subscribed (the tables are then of no use).
HSA_INF_HD int inf_build(uint16_t *count, uint16_t *symbol, uint16_t *offs, const uint8_t *lens, uint32_t n)
{
    for (uint32_t l = 0; l < 16u; ++l) count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) count[lens[s] & 15u]++;
    if (count[0] == n) return 0;
    int32_t left = 1;
    for (uint32_t l = 1; l < 16u; ++l) {
        left = (left << 1) - (int32_t)count[l];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (uint32_t l = 1; l < 15u; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s] & 15u;
        if (l) symbol[offs[l]++] = (uint16_t)s;
    }
    return left;
}

// A set with room left is taken only as zlib takes it: a single code of length 1.
HSA_INF_HD bool inf_usable(int left, const uint16_t *count, uint32_t n)
{
    return left == 0 || (left > 0 && n - count[0] == 1u && count[1] == 1u);
}

HSA_INF_HD int inf_fixed_tables(InfTables &t)
{
    for (uint32_t s = 0; s < 288u; ++s) t.lens[s] = s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8;
    inf_build(t.lcount, t.lsym, t.offs, t.lens, 288u);
    for (uint32_t s = 0; s < 30u; ++s) t.lens[s] = 5;
    inf_build(t.dcount, t.dsym, t.offs, t.lens, 30u);    // (codes 30 and 31 stay undefined)
    return 0;
}

HSA_INF_HD int inf_dynamic_tables(InfBits &b, InfTables &t)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t v, nlen, ndist, ncode;
    HSA_INF_TRY(inf_bits(b, 5, v)); nlen = v + 257u;
    HSA_INF_TRY(inf_bits(b, 5, v)); ndist = v + 1u;
    HSA_INF_TRY(inf_bits(b, 4, v)); ncode = v + 4u;
    if (nlen > 286u || ndist > 30u) return HSA_INF_E_CODES;
    for (uint32_t i = 0; i < 19u; ++i) t.lens[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) {
        HSA_INF_TRY(inf_bits(b, 3, v));
        t.lens[order[i]] = (uint8_t)v;
    }
    if (inf_build(t.lcount, t.lsym, t.offs, t.lens, 19u) != 0) return HSA_INF_E_CODES;   // (complete, as zlib asks)
    // one run of nlen + ndist lengths: a repeat may cross from the first set into the second
    const uint32_t total = nlen + ndist;
    uint32_t idx = 0;
    while (idx < total) {
        uint32_t sym;
        HSA_INF_TRY(inf_decode(b, t.lcount, t.lsym, sym));
        if (sym < 16u) {
            t.lens[idx++] = (uint8_t)sym;
            continue;
        }
        uint8_t prev = 0;
        uint32_t rep;
        if (sym == 16u) {
            if (idx == 0) return HSA_INF_E_CODES;
            prev = t.lens[idx - 1];
            HSA_INF_TRY(inf_bits(b, 2, v)); rep = 3u + v;
        } else if (sym == 17u) {
            HSA_INF_TRY(inf_bits(b, 3, v)); rep = 3u + v;
        } else {
            HSA_INF_TRY(inf_bits(b, 7, v)); rep = 11u + v;
        }
        if (idx + rep > total) return HSA_INF_E_CODES;
        while (rep--) t.lens[idx++] = prev;
    }
    if (t.lens[256] == 0) return HSA_INF_E_CODES;          // no end-of-block code
    int left = inf_build(t.lcount, t.lsym, t.offs, t.lens, nlen);
    if (!inf_usable(left, t.lcount, nlen)) return HSA_INF_E_CODES;
    left = inf_build(t.dcount, t.dsym, t.offs, t.lens + nlen, ndist);
    if (!inf_usable(left, t.dcount, ndist)) return HSA_INF_E_CODES;
    return 0;
}

// The symbols of a Huffman block up to its end-of-block code.
template <class Sink> HSA_INF_HD int inf_symbols(InfBits &b, const InfTables &t, Sink &sink)
{
    for (;;) {
        uint32_t sym, v;
        HSA_INF_TRY(inf_decode(b, t.lcount, t.lsym, sym));
        if (sym < 256u) {
            HSA_INF_TRY(sink.literal((uint8_t)sym));
            continue;
        }
        if (sym == 256u) return 0;
        sym -= 257u;
        if (sym >= 29u) return HSA_INF_E_SYMBOL;           // 286 and 287 have codes in the fixed set only
        uint32_t len;
        if (sym < 8u) {
            len = 3u + sym;
        } else if (sym == 28u) {
            len = 258u;
        } else {
            const uint32_t extra = (sym >> 2) - 1u;        // 8..27: 1..5 extra bits
            HSA_INF_TRY(inf_bits(b, extra, v));
            len = 3u + ((4u + (sym & 3u)) << extra) + v;
        }
        HSA_INF_TRY(inf_decode(b, t.dcount, t.dsym, sym));
        if (sym >= 30u) return HSA_INF_E_SYMBOL;
        uint32_t dist;
        if (sym < 4u) {
            dist = 1u + sym;
        } else {
            const uint32_t extra = (sym >> 1) - 1u;        // 4..29: 1..13 extra bits
            HSA_INF_TRY(inf_bits(b, extra, v));
            dist = 1u + ((2u + (sym & 1u)) << extra) + v;
        }
        HSA_INF_TRY(sink.match(dist, len));
    }
}

// A whole DEFLATE stream: blocks up to the final one.  The sink refuses what leaves the
// block's slice (HSA_INF_E_OUTPUT, HSA_INF_E_DIST); HSA_INF_E_TRAIL when whole payload bytes
// follow the final block.
template <class Sink> HSA_INF_HD int inf_stream(InfBits &b, InfTables &t, Sink &sink)
{
    uint32_t last, type, v;
    do {
        HSA_INF_TRY(inf_bits(b, 1, last));
        HSA_INF_TRY(inf_bits(b, 2, type));
        if (type == 0u) {
            b.buf >>= b.cnt & 7u;                          // to the byte boundary
            b.cnt &= ~7u;
            uint32_t len, nlen;
            HSA_INF_TRY(inf_bits(b, 16, len));
            HSA_INF_TRY(inf_bits(b, 16, nlen));
            if (len != (nlen ^ 0xFFFFu)) return HSA_INF_E_STORED;
            if (len > inf_bytes_left(b)) return HSA_INF_E_INPUT;
            for (uint32_t i = 0; i < len; ++i) {
                HSA_INF_TRY(inf_bits(b, 8, v));
                HSA_INF_TRY(sink.literal((uint8_t)v));
            }
        } else if (type == 3u) {
            return HSA_INF_E_BTYPE;
        } else {
            HSA_INF_TRY(type == 1u ? inf_fixed_tables(t) : inf_dynamic_tables(b, t));
            HSA_INF_TRY(inf_symbols(b, t, sink));
        }
    } while (!last);
    return inf_bytes_left(b) ? HSA_INF_E_TRAIL : 0;
}

// ---- CRC32 (the gzip trailer's), in pieces that 64 lanes can share ----
// Polynomials over GF(2) modulo the CRC's, reflected: bit 31 is x^0.  The register of a
// message with initial value 0 and no final inversion is linear in the message, and
// appending z zero bytes multiplies it by x^(8z).  So a block cut into segments has
//   crc = ~( sum_k raw0(seg_k) * x^(8 * bytes behind seg_k)  +  0xFFFFFFFF * x^(8n) ),
// each term a lane's own work, the sum an XOR across the lanes.
#define HSA_INF_CRC_POLY 0xEDB88320u

HSA_INF_HD uint32_t inf_crc_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ HSA_INF_CRC_POLY : c >> 1;
    return c;
}

HSA_INF_HD uint32_t inf_crc_raw0(const uint32_t *tab, const uint8_t *p, uint32_t n)
{
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255u] ^ (c >> 8);
    return c;
}

HSA_INF_HD uint32_t inf_gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ HSA_INF_CRC_POLY : b >> 1;     // b * x
    }
    return p;
}

// x^(8 * nbytes)
HSA_INF_HD uint32_t inf_gf_xpow8(uint32_t nbytes)
{
    uint32_t r = 0x80000000u, base = 0x00800000u;               // 1, x^8
    for (uint32_t e = nbytes; e; e >>= 1) {
        if (e & 1u) r = inf_gf_mul(r, base);
        base = inf_gf_mul(base, base);
    }
    return r;
}

// Lane `lane` of `lanes`: its term of the sum above for the n bytes at p (XOR the terms of
// all lanes, then invert).  Lane 0 adds the initial value's term.
HSA_INF_HD uint32_t inf_crc_term(const uint32_t *tab, const uint8_t *p, uint32_t n, uint32_t lane, uint32_t lanes)
{
    const uint32_t seg = (n + lanes - 1u) / lanes;
    const uint64_t b0 = (uint64_t)lane * seg;
    uint32_t term = lane == 0 ? inf_gf_mul(0xFFFFFFFFu, inf_gf_xpow8(n)) : 0u;
    if (b0 < n) {
        const uint32_t beg = (uint32_t)b0, end = n - beg < seg ? n : beg + seg;
        term ^= inf_gf_mul(inf_crc_raw0(tab, p + beg, end - beg), inf_gf_xpow8(n - end));
    }
    return term;
}
