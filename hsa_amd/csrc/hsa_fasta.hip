// hsa_fasta.hip -- FASTA bytes to the packed texts and the annotation tables, and a BWT to
// its .bwt / .fmv file bodies, on the device.
//
// hsa_fasta_device restates HSPParseFASTAToPacked (HSP.c:180-343) and BuildReversePacked
// (2BWT-Builder.c:116-213) for a whole FASTA whose bytes sit in device memory, with the
// grammar hsa_amd/index_build.py states (_records, parse_fasta, pac_bytes, reverse_pac,
// pac_text): those functions are the text these kernels are tested against.
//
// Why a device number and a caller's scratch, not a handle: the call runs before an index
// exists (it makes the texts an index is built from), as the builders do
// (hsa_build_bwt_index_device takes a device number too).  With no handle to grow scratch
// on, and no allocation that would synchronise, the caller passes the scratch
// (hsa_fasta_scratch_bytes states its size).
//
// Bytes.  Every '>' starts a record; a byte is in a header line when the last '>' at or
// before it has no '\n' between them (the '\n' that ends the line included); every other
// byte after the first '>' except '\n' is sequence; a-z count as A-Z; only A, C, G, T are
// unambiguous.  Within a record the sequence bytes are numbered without the newlines.
// Record length L = its sequence bytes; L < 75: dropped.  In a kept record an ambiguous
// byte is dropped when its run of ambiguous bytes (newlines between them do not break
// it) has 10 bytes or more, and is 'G' otherwise.  parse_fasta's cases follow from that
// one rule: a block starts at every kept character whose predecessor in the record is
// missing or dropped (ori: its number in the record), a dropped run at the end leaves
// no block behind it, and a kept record with no kept character (all ambiguous) has one
// empty block with ori = L.  Blocks lie back to back in the packed text, so a block's end
// is the next block's start - 1 and the last block's end is K - 1 (K kept characters).
//
// Refused (counter [17] gives the lowest offset; the outputs are then of no use but stay
// inside their capacities): a '>' inside a header line (its offset), a last header line
// without '\n' (the offset of its '>'), an input that does not begin with '>' (0).
//
// Launches, all on one stream, no host round trip, no atomics that place anything (the
// one atomicMin is the refused offset: a minimum is order-free):
//   k_fa_marks   per tile of FA_TILE bytes: the last '>', the last '\n', the '>' count;
//   scan         exclusive (max, max, +) over the tiles: is a tile's first byte in a header;
//   k_fa_spans   per tile a span summary (FaSum): sequence bytes before the first and after
//                the last '>', ambiguous bytes before the first and after the last byte that
//                ends a run; stored twice, the second time in reverse tile order;
//   scans        exclusive over the tiles with fa_cat, forward and (on the reversed copy)
//                backward: what lies before and behind every tile of the record and of the
//                run that cross its edges;
//   k_fa_count   the same loads, block scans of the summaries in both directions, the
//                decision per byte (fa_decide); per tile: kept characters, kept records,
//                blocks, `total`, and the last 15 kept codes;
//   scan         exclusive over the tiles (FaCnt): every output position;
//   k_fa_pack    the decisions again; the kept codes of a tile in LDS behind the up to 15
//                codes the scan carried in; one lane per whole 16-code word: the text word
//                and the four .pac bytes; the record rows and the block rows.  The word that
//                a tile only begins is written by the tile that holds its last code;
//   k_fa_finish  the last partial word, the .pac tail, the zero padding, the last block's
//                end, the counters;
//   k_fa_reverse one lane per word of the reversed text: .rev.pac bytes and the text word.
//
// Scratch: per tile of 4096 input bytes 2 FaMark (12 B), 4 FaSum (24 B), 2 FaCnt (20 B) =
// 160 bytes, under 4 % of the input, plus rocPRIM's scan storage (a few bytes per tile) and
// 3 KB of alignment: a 3.2 GB FASTA needs about 130 MB.  Nothing is kept per byte: k_fa_pack
// recomputes what k_fa_count decided.
//
// Loops.  Every loop runs over the 16 bytes of a lane, the words of a tile (at most 257),
// the at most 256 bytes of a name, or 16 codes: all bounded by constants or the input's
// size.  The cross-lane operations (rocPRIM block scans, __syncthreads) stand outside every
// loop and every branch: all 256 lanes of a block reach them, whatever their bytes are.
//
// hsa_bwt_files_device: the .bwt code words (16 codes per word, first code in the top bits,
// tail past T cleared) and the .fmv minor / major Occ arrays as index_io.occ_files makes
// them, from the builder's LSB-first BWT: k_bf_blocks counts the four characters per 256
// (zero padding past T counted as 'A') and writes the code words, a scan over the blocks,
// k_bf_samples writes the 16-bit minor pairs and the major samples.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <string.h>

#include "hsa_internal.h"

#define FA_TILE 4096u                  // bytes of the input per block: 256 lanes x 16
#define FA_ONES32 0xFFFFFFFFu
#define FA_MIN_RECORD 75u              // HSP.c:222
#define FA_MIN_RUN 10u                 // HSP.c:250, :275
#define FA_MAX_NAME 256u
#define FA_PAD_WORDS 8u                // zero words behind a text, as the builder's caller pads it

struct FaMark {
    uint32_t gt, nl, ngt;              // last '>' and last '\n' (offset + 1; 0: none), count of '>'
};
struct FaMarkOp {
    __host__ __device__ FaMark operator()(const FaMark &a, const FaMark &b) const
    {
        return FaMark{a.gt > b.gt ? a.gt : b.gt, a.nl > b.nl ? a.nl : b.nl, a.ngt + b.ngt};
    }
};

// A span of bytes, as the record and the run that cross its edges see it.  brk: it holds a
// byte that ends a run of ambiguous bytes (a '>' or an unambiguous sequence byte)
struct FaSum {
    uint32_t ngt, brk;
    uint32_t cntHead, cntTail;         // sequence bytes before the first '>' / after the last (all, without one)
    uint32_t runHead, runTail;         // ambiguous bytes before the first brk byte / after the last
};
__host__ __device__ __forceinline__ FaSum fa_cat(const FaSum &a, const FaSum &b)      // a, then b
{
    FaSum r;
    r.ngt = a.ngt + b.ngt;
    r.brk = a.brk | b.brk;
    r.cntHead = a.ngt ? a.cntHead : a.cntHead + b.cntHead;
    r.cntTail = b.ngt ? b.cntTail : a.cntTail + b.cntTail;
    r.runHead = a.brk ? a.runHead : a.runHead + b.runHead;
    r.runTail = b.brk ? b.runTail : a.runTail + b.runTail;
    return r;
}
struct FaCat {
    __host__ __device__ FaSum operator()(const FaSum &a, const FaSum &b) const { return fa_cat(a, b); }
};
struct FaCatRev {                      // for a scan that runs from the last span to the first
    __host__ __device__ FaSum operator()(const FaSum &a, const FaSum &b) const { return fa_cat(b, a); }
};

struct FaCnt {
    uint32_t k, recs, blks, total;     // kept characters, kept records, blocks, sum of the kept records' L
    uint32_t tail;                     // the last min(15, k) kept codes, the earliest in the low bits
};
__host__ __device__ __forceinline__ FaCnt fa_cnt_cat(const FaCnt &a, const FaCnt &b)
{
    FaCnt r{a.k + b.k, a.recs + b.recs, a.blks + b.blks, a.total + b.total, b.tail};
    const uint32_t qa = a.k < 15u ? a.k : 15u, qb = b.k < 15u ? b.k : 15u;
    if (qb < 15u) {
        const uint32_t take = 15u - qb < qa ? 15u - qb : qa;
        const uint32_t from_a = take ? (a.tail >> (2u * (qa - take))) & ((1u << (2u * take)) - 1u) : 0u;
        r.tail = from_a | (b.tail << (2u * take));
    }
    return r;
}
struct FaCntCat {
    __host__ __device__ FaCnt operator()(const FaCnt &a, const FaCnt &b) const { return fa_cnt_cat(a, b); }
};

struct FaArgs {
    const uint8_t *in;
    uint32_t n, lead, ntiles;          // lead: bytes between the aligned base and in
    uint8_t *pac; uint64_t pac_cap;
    uint8_t *rpac; uint64_t rpac_cap;
    uint32_t *text; uint64_t text_cap;
    uint32_t *rtext; uint64_t rtext_cap;
    uint32_t *rec; uint64_t rec_cap;
    uint32_t *blk; uint64_t blk_cap;
    unsigned long long *ctr;
    // scratch
    uint32_t *g;                       // [0] the lowest refused offset among the '>' inside header lines
    FaMark *mark_in, *mark_out;        // ntiles + 1
    FaSum *sumf_in, *sumf_out;         // ntiles + 1
    FaSum *sumb_in, *sumb_out;         // ntiles, tile t at ntiles - 1 - t
    FaCnt *cnt_in, *cnt_out;           // ntiles + 1
};

// Every length that follows from the kept characters and `total` (pac_bytes, pac_text,
// reverse_pac of hsa_amd/index_build.py)
struct FaLen {
    uint64_t K, total, m, nb, pac_bytes, T, nw;
    uint64_t full, rem, Rb, rpac_bytes, rT, rnw, rwords;     // rwords: words that hold .rev.pac bytes
};
__host__ __device__ __forceinline__ FaLen fa_len(const FaCnt &tot)
{
    FaLen l;
    l.K = tot.k; l.total = tot.total; l.m = tot.total & 3u;
    l.nb = (l.K + 3u) / 4u;
    l.pac_bytes = l.nb + (l.m ? 1u : 2u);
    const int64_t T = ((int64_t)l.pac_bytes - 2) * 4 + (int64_t)l.m;        // TextLengthFromBytePacked
    l.T = T > 0 ? (uint64_t)T : 0u;
    l.nw = (l.T + 15u) / 16u;
    l.rem = l.T % 16u;
    l.full = l.rem ? l.T - l.rem : (l.T >= 16u ? l.T - 16u : 0u);            // a full last word is lost
    const uint64_t nbp = l.rem == 0u ? 0u : l.rem < 4u ? 1u : l.rem < 8u ? 2u : l.rem < 12u ? 3u : 4u;
    l.Rb = l.full / 4u + nbp;
    l.rpac_bytes = l.Rb + 1u;
    const int64_t rT = ((int64_t)l.Rb - 1) * 4 + (int64_t)l.m;
    l.rT = rT > 0 ? (uint64_t)rT : 0u;
    l.rnw = (l.rT + 15u) / 16u;
    l.rwords = (l.Rb + 3u) / 4u;
    return l;
}

// What a lane's 16 bytes are: bit j of a mask speaks of byte j; codes: 2 bits per byte
// (an ambiguous byte: 2, 'G').  b0: the input offset of byte 0
struct FaCls {
    uint32_t seq, amb, gt, codes;
    int64_t b0;
};

using FaMarkScan = rocprim::block_scan<FaMark, 256>;
using FaSumScan = rocprim::block_scan<FaSum, 256>;
using FaCntScan = rocprim::block_scan<FaCnt, 256>;

__device__ __forceinline__ void fa_load(const FaArgs &a, uint32_t tile, uint32_t ch[16], uint32_t &valid, int64_t &b0)
{
    const uint64_t u = (uint64_t)tile * 256u + threadIdx.x;
    b0 = (int64_t)(16u * u) - (int64_t)a.lead;
    valid = 0u;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (b0 + 16 > 0 && b0 < (int64_t)a.n) {
        w = *reinterpret_cast<const uint4 *>(a.in - a.lead + 16u * u);
        const uint32_t lo = b0 < 0 ? (uint32_t)(-b0) : 0u;
        const int64_t left = (int64_t)a.n - b0;
        const uint32_t hi = left < 16 ? (uint32_t)left : 16u;
        valid = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    }
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) ch[j] = (ws[j >> 2] >> (8 * (j & 3))) & 0xFFu;
}

__device__ __forceinline__ FaMark fa_marks_of(const uint32_t ch[16], uint32_t valid, int64_t b0)
{
    FaMark m{0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if ((valid >> j) & 1u) {
            if (ch[j] == '>') { m.gt = (uint32_t)(b0 + j) + 1u; ++m.ngt; }
            if (ch[j] == '\n') m.nl = (uint32_t)(b0 + j) + 1u;
        }
    return m;
}

__global__ void __launch_bounds__(256) k_fa_marks(FaArgs a)
{
    using Reduce = rocprim::block_reduce<FaMark, 256>;
    __shared__ typename Reduce::storage_type tmp;
    uint32_t ch[16], valid;
    int64_t b0;
    fa_load(a, blockIdx.x, ch, valid, b0);
    FaMark m = fa_marks_of(ch, valid, b0), sum{0u, 0u, 0u};
    Reduce().reduce(m, sum, tmp, FaMarkOp());           // (max, max, +): commutative
    if (threadIdx.x == 0) a.mark_in[blockIdx.x] = sum;
}

// The lane's bytes classified; with `refuse`, a '>' inside a header line lowers g[0]
__device__ __forceinline__ FaCls fa_classify(const FaArgs &a, uint32_t tile, typename FaMarkScan::storage_type &tmp, bool refuse)
{
    uint32_t ch[16], valid;
    FaCls c{0u, 0u, 0u, 0u, 0};
    fa_load(a, tile, ch, valid, c.b0);
    FaMark pre;
    FaMarkScan().exclusive_scan(fa_marks_of(ch, valid, c.b0), pre, a.mark_out[tile], tmp, FaMarkOp());
    bool hdr = pre.gt > pre.nl, any = pre.gt != 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (!((valid >> j) & 1u)) continue;
        const uint32_t x = ch[j];
        if (x == '>') {
            if (refuse && hdr) atomicMin(&a.g[0], (uint32_t)(c.b0 + j));
            hdr = true; any = true;
            c.gt |= 1u << j;
        } else if (x == '\n') hdr = false;
        else if (!hdr && any) {
            const uint32_t up = x & 0xDFu;              // ('A' and 'a' alone map to 'A', and so on)
            const uint32_t code = up == 'A' ? 0u : up == 'C' ? 1u : up == 'G' ? 2u : up == 'T' ? 3u : 4u;
            c.seq |= 1u << j;
            if (code > 3u) c.amb |= 1u << j;
            c.codes |= (code > 3u ? 2u : code) << (2 * j);
        }
    }
    return c;
}

__device__ __forceinline__ FaSum fa_sum_of(const FaCls &c)
{
    FaSum s{0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if ((c.gt >> j) & 1u) { ++s.ngt; s.brk = 1u; s.cntTail = 0u; s.runTail = 0u; }
        else if ((c.seq >> j) & 1u) {
            if (!s.ngt) ++s.cntHead;
            ++s.cntTail;
            if ((c.amb >> j) & 1u) { if (!s.brk) ++s.runHead; ++s.runTail; }
            else { s.brk = 1u; s.runTail = 0u; }
        }
    }
    return s;
}

__global__ void __launch_bounds__(256) k_fa_spans(FaArgs a)
{
    __shared__ typename FaMarkScan::storage_type tmp_m;
    __shared__ typename FaSumScan::storage_type tmp_s;
    const FaCls c = fa_classify(a, blockIdx.x, tmp_m, true);
    FaSum inc;
    FaSumScan().inclusive_scan(fa_sum_of(c), inc, tmp_s, FaCat());
    if (threadIdx.x == 255u) {
        a.sumf_in[blockIdx.x] = inc;
        a.sumb_in[a.ntiles - 1u - blockIdx.x] = inc;
    }
}

// The decision per byte.  keep: a kept character; blk: a block starts here (a kept
// character, or the '>' of a kept record without one); rec: the '>' of a kept record;
// val[j]: a record's L at its '>', a block's ori at its first character
struct FaDec {
    uint32_t keep, blk, rec, total;
    uint32_t val[16];
};
struct FaTileTmp {
    typename FaMarkScan::storage_type m;
    typename FaSumScan::storage_type s;
    FaSum x[256];
};

__device__ __forceinline__ FaDec fa_decide(const FaArgs &a, uint32_t tile, FaTileTmp &t, FaCls &c)
{
    c = fa_classify(a, tile, t.m, false);
    const FaSum mine = fa_sum_of(c);
    FaSum pre, suf;
    FaSumScan().exclusive_scan(mine, pre, a.sumf_out[tile], t.s, FaCat());
    // what lies behind the lane: the same scan over the lanes in reverse order
    t.x[threadIdx.x] = mine;
    __syncthreads();
    const FaSum rev = t.x[255u - threadIdx.x];
    __syncthreads();
    FaSumScan().exclusive_scan(rev, suf, a.sumb_out[a.ntiles - 1u - tile], t.s, FaCatRev());
    t.x[threadIdx.x] = suf;
    __syncthreads();
    suf = t.x[255u - threadIdx.x];
    __syncthreads();

    FaDec d;
    d.keep = d.blk = d.rec = d.total = 0u;
    uint32_t pc[16], pr[16];                               // sequence bytes of the record / ambiguous bytes of the run before byte j
    uint32_t cnt = pre.cntTail, run = pre.runTail;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        pc[j] = cnt; pr[j] = run; d.val[j] = 0u;
        if ((c.gt >> j) & 1u) { cnt = 0u; run = 0u; }
        else if ((c.seq >> j) & 1u) {
            ++cnt;
            run = (c.amb >> j) & 1u ? run + 1u : 0u;
        }
    }
    cnt = suf.cntHead; run = suf.runHead;                  // ... behind byte j
#pragma unroll
    for (int j = 15; j >= 0; --j) {
        if ((c.gt >> j) & 1u) {
            if (cnt >= FA_MIN_RECORD) {
                d.rec |= 1u << j;
                d.total += cnt;
                d.val[j] = cnt;
                if (run == cnt) d.blk |= 1u << j;          // all ambiguous: one empty block
            }
            cnt = 0u; run = 0u;
        } else if ((c.seq >> j) & 1u) {
            const bool amb = (c.amb >> j) & 1u;
            const bool drop = amb && pr[j] + 1u + run >= FA_MIN_RUN;
            if (pc[j] + 1u + cnt >= FA_MIN_RECORD && !drop) {
                d.keep |= 1u << j;
                if (pc[j] == 0u || (!amb && pr[j] >= FA_MIN_RUN)) { d.blk |= 1u << j; d.val[j] = pc[j]; }
            }
            ++cnt;
            run = amb ? run + 1u : 0u;
        }
    }
    return d;
}

// The lane's kept codes, the earliest in the low bits (at most 16: 32 bits), and its counts
__device__ __forceinline__ FaCnt fa_cnt_of(const FaCls &c, const FaDec &d, uint32_t &comp)
{
    comp = 0u;
    uint32_t nk = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if ((d.keep >> j) & 1u) { comp |= ((c.codes >> (2 * j)) & 3u) << (2u * nk); ++nk; }
    return FaCnt{nk, (uint32_t)__popc(d.rec), (uint32_t)__popc(d.blk), d.total, nk == 16u ? comp >> 2 : comp};
}

__global__ void __launch_bounds__(256) k_fa_count(FaArgs a)
{
    __shared__ FaTileTmp t;
    __shared__ typename FaCntScan::storage_type tmp_c;
    FaCls c;
    const FaDec d = fa_decide(a, blockIdx.x, t, c);
    uint32_t comp;
    FaCnt inc;
    FaCntScan().inclusive_scan(fa_cnt_of(c, d, comp), inc, tmp_c, FaCntCat());
    if (threadIdx.x == 255u) a.cnt_in[blockIdx.x] = inc;
}

__device__ __forceinline__ uint32_t fa_rev2_32(uint32_t x)           // the 16 codes of a word in reverse order
{
    x = (x >> 16) | (x << 16);
    x = ((x & 0xFF00FF00u) >> 8) | ((x & 0x00FF00FFu) << 8);
    x = ((x & 0xF0F0F0F0u) >> 4) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x & 0xCCCCCCCCu) >> 2) | ((x & 0x33333333u) << 2);
    return x;
}
// The low `codes` codes of a word (16 or more: all)
__device__ __forceinline__ uint32_t fa_low(uint32_t w, uint64_t codes) { return codes >= 16u ? w : w & ((1u << (2u * (uint32_t)codes)) - 1u); }

// `nbytes` file bytes of word w (its codes first-in-the-high-bits, 4 per byte) to out, below cap
__device__ __forceinline__ void fa_store_bytes(uint8_t *out, uint64_t cap, uint64_t w, uint32_t lsb, uint32_t nbytes)
{
    const uint32_t le = __builtin_bswap32(fa_rev2_32(lsb));          // byte 0 of the file in the low byte
    if (nbytes == 4u && 4u * w + 4u <= cap) { *reinterpret_cast<uint32_t *>(out + 4u * w) = le; return; }
    for (uint32_t q = 0; q < nbytes; ++q)
        if (4u * w + q < cap) out[4u * w + q] = (uint8_t)(le >> (8u * q));
}
// Word w of the forward text (cut at T) and its .pac bytes (all the kept codes)
__device__ __forceinline__ void fa_store_word(const FaArgs &a, const FaLen &l, uint64_t w, uint32_t lsb, uint32_t nbytes)
{
    if (w < a.text_cap) a.text[w] = fa_low(lsb, l.T > 16u * w ? l.T - 16u * w : 0u);
    fa_store_bytes(a.pac, a.pac_cap, w, lsb, nbytes);
}

__global__ void __launch_bounds__(256) k_fa_pack(FaArgs a)
{
    __shared__ FaTileTmp t;
    __shared__ typename FaCntScan::storage_type tmp_c;
    __shared__ uint8_t sc[16 + FA_TILE];                   // [15 - carried, 15): the carried codes; [15, 15 + kept): the tile's
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    FaCls c;
    const FaDec d = fa_decide(a, tile, t, c);
    uint32_t comp;
    const FaCnt mine = fa_cnt_of(c, d, comp), base = a.cnt_out[tile];
    FaCnt pre;
    FaCntScan().exclusive_scan(mine, pre, base, tmp_c, FaCntCat());
    const FaLen l = fa_len(a.cnt_out[a.ntiles]);
    const uint32_t K0 = base.k, carried = K0 & 15u, kt = a.cnt_out[tile + 1u].k - K0;
    if (lane < carried) {
        const uint32_t qa = K0 < 15u ? K0 : 15u;
        sc[15u - carried + lane] = (uint8_t)(((base.tail >> (2u * (qa - carried))) >> (2u * lane)) & 3u);
    }
    for (uint32_t q = 0; q < mine.k; ++q) sc[15u + (pre.k - K0) + q] = (uint8_t)((comp >> (2u * q)) & 3u);
    __syncthreads();
    const uint32_t w0 = K0 >> 4, nW = ((K0 + kt) >> 4) - w0;      // the words whose last code lies in this tile
    for (uint32_t wi = lane; wi < nW; wi += 256u) {
        const uint8_t *s = sc + 15u - carried + 16u * wi;
        uint32_t lsb = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) lsb |= (uint32_t)s[j] << (2 * j);
        fa_store_word(a, l, (uint64_t)w0 + wi, lsb, 4u);
    }
    if (!(d.rec | d.blk)) return;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t below = (1u << j) - 1u, upto = below | (1u << j);
        if ((d.rec >> j) & 1u) {
            const uint64_t row = (uint64_t)pre.recs + __popc(d.rec & below);
            if (row < a.rec_cap) {
                const uint32_t off = (uint32_t)(c.b0 + j) + 1u;
                uint32_t len = 0u;                          // to the first tab, space or newline, at most 256 bytes
                while (len < FA_MAX_NAME && off + len < a.n) {
                    const uint8_t x = a.in[off + len];
                    if (x == '\t' || x == ' ' || x == '\n') break;
                    ++len;
                }
                uint32_t *r = a.rec + HSA_FA_REC_WORDS * row;
                r[0] = off; r[1] = len; r[2] = d.val[j]; r[3] = pre.blks + __popc(d.blk & below);
            }
        }
        if ((d.blk >> j) & 1u) {
            const uint64_t bi = (uint64_t)pre.blks + __popc(d.blk & below);
            const uint32_t start = pre.k + __popc(d.keep & below);
            if (bi < a.blk_cap) {
                uint32_t *r = a.blk + 4u * bi;
                r[0] = pre.recs + __popc(d.rec & upto) - 1u; r[1] = start; r[3] = d.val[j];
            }
            if (bi > 0u && bi - 1u < a.blk_cap) a.blk[4u * (bi - 1u) + 2u] = start - 1u;
        }
    }
}

__device__ __forceinline__ uint64_t fa_min64(uint64_t x, uint64_t y) { return x < y ? x : y; }

__global__ void __launch_bounds__(64) k_fa_finish(FaArgs a)
{
    const FaCnt tot = a.cnt_out[a.ntiles];
    const FaLen l = fa_len(tot);
    const uint32_t lane = threadIdx.x;
    if (lane < FA_PAD_WORDS && l.nw + lane < a.text_cap) a.text[l.nw + lane] = 0u;
    if (lane != 0u) return;
    const uint32_t r = tot.k & 15u;
    if (r) {                                               // the last, partial word: the scan's last r codes
        const uint32_t qa = tot.k < 15u ? tot.k : 15u;
        fa_store_word(a, l, tot.k >> 4, fa_low(tot.tail >> (2u * (qa - r)), r), (r + 3u) / 4u);
    }
    if (l.m == 0u && l.nb < a.pac_cap) a.pac[l.nb] = 0u;   // HSP.c:318-323
    if (l.pac_bytes - 1u < a.pac_cap) a.pac[l.pac_bytes - 1u] = (uint8_t)l.m;
    if (tot.blks && (uint64_t)tot.blks - 1u < a.blk_cap) a.blk[4u * ((uint64_t)tot.blks - 1u) + 2u] = tot.k - 1u;
    const FaMark mk = a.mark_out[a.ntiles];
    uint32_t bad = a.g[0];
    if (mk.gt > mk.nl && mk.gt - 1u < bad) bad = mk.gt - 1u;           // the last header line never ends
    if (a.n == 0u || a.in[0] != (uint8_t)'>') bad = 0u;
    unsigned long long *c = a.ctr;
    c[0] = mk.ngt; c[1] = tot.recs; c[2] = fa_min64(tot.recs, a.rec_cap);
    c[3] = tot.blks; c[4] = fa_min64(tot.blks, a.blk_cap);
    c[5] = l.K; c[6] = l.total; c[7] = l.T; c[8] = l.rT;
    c[9] = l.pac_bytes; c[10] = fa_min64(l.pac_bytes, a.pac_cap);
    c[11] = l.rpac_bytes; c[12] = fa_min64(l.rpac_bytes, a.rpac_cap);
    c[13] = l.nw + FA_PAD_WORDS; c[14] = fa_min64(c[13], a.text_cap);
    c[15] = l.rnw + FA_PAD_WORDS; c[16] = fa_min64(c[15], a.rtext_cap);
    c[17] = bad == FA_ONES32 ? ~0ull : bad;
}

// One lane per word of the reversed text: code j of it is the forward text's code
// T - 1 - j for j < full + rem (reverse_pac), 'A' behind that; the .rev.pac holds those
// codes' bytes, the text ends at rT
__global__ void __launch_bounds__(256) k_fa_reverse(FaArgs a, uint64_t max_words)
{
    const FaLen l = fa_len(a.cnt_out[a.ntiles]);
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w == 0u && l.Rb < a.rpac_cap) a.rpac[l.Rb] = (uint8_t)l.m;
    if (w >= max_words) return;
    const uint64_t have = l.full + l.rem;
    uint32_t word = 0u;
    if (w < l.rwords) {
        const uint64_t tw = fa_min64(l.nw, a.text_cap);    // (a text cut by its capacity: the caller runs again)
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint64_t p = 16u * w + j;
            if (p >= have) break;
            const uint64_t f = l.T - 1u - p;
            if ((f >> 4) < tw) word |= ((a.text[f >> 4] >> (2u * (uint32_t)(f & 15u))) & 3u) << (2u * j);
        }
        const uint64_t left = l.Rb - 4u * w;
        fa_store_bytes(a.rpac, a.rpac_cap, w, word, left < 4u ? (uint32_t)left : 4u);
    }
    if (w < l.rnw + FA_PAD_WORDS && w < a.rtext_cap)
        a.rtext[w] = w < l.rnw ? fa_low(word, l.rT > 16u * w ? l.rT - 16u * w : 0u) : 0u;
}

static int g_fa_timing = 0;
static StageTimer g_fa_t{HSA_FA_LAUNCHES};
static StageTimer g_bf_t{HSA_BF_LAUNCHES};

extern "C" void hsa_fasta_timing(int on) { g_fa_timing = on; }
extern "C" int hsa_fasta_launch_times(float *ms)
{
    if (!ms) { hsa_set_error("hsa_fasta_launch_times: null argument"); return HSA_E_ARG; }
    return g_fa_t.times(ms, "hsa_fasta");
}
extern "C" int hsa_bwt_files_launch_times(float *ms)
{
    if (!ms) { hsa_set_error("hsa_bwt_files_launch_times: null argument"); return HSA_E_ARG; }
    if (!g_bf_t.timed) { hsa_set_error("hsa_bwt_files_launch_times: the last call was not timed (hsa_fasta_timing)"); return HSA_E_ARG; }
    return g_bf_t.times(ms, "hsa_bwt_files");
}

struct FaPlan {
    FaArgs A;
    void *d_tmp;
    size_t tmp_m, tmp_s, tmp_c, bytes;
};
// The scratch layout of an input of n_in bytes that starts `lead` bytes into a 16-byte unit
// (at most 15: the size is stated for 15)
static int fa_plan(FaPlan &p, uint64_t n_in, uint32_t lead, void *base, hipStream_t st)
{
    FaArgs &A = p.A;
    A.n = (uint32_t)n_in; A.lead = lead;
    A.ntiles = (uint32_t)(((uint64_t)lead + n_in + FA_TILE - 1u) / FA_TILE);
    const size_t nt1 = (size_t)(((uint64_t)15u + n_in + FA_TILE - 1u) / FA_TILE) + 1;      // (whatever the lead)
    HSA_TRY(hsa_scan_bytes(p.tmp_m, FaMark{0, 0, 0}, nt1, FaMarkOp(), st));
    HSA_TRY(hsa_scan_bytes(p.tmp_s, FaSum{0, 0, 0, 0, 0, 0}, nt1, FaCat(), st));
    HSA_TRY(hsa_scan_bytes(p.tmp_c, FaCnt{0, 0, 0, 0, 0}, nt1, FaCntCat(), st));
    Carver c(base);
    A.g = c.take<uint32_t>(64);
    A.mark_in = c.take<FaMark>(nt1); A.mark_out = c.take<FaMark>(nt1);
    A.sumf_in = c.take<FaSum>(nt1); A.sumf_out = c.take<FaSum>(nt1);
    A.sumb_in = c.take<FaSum>(nt1); A.sumb_out = c.take<FaSum>(nt1);
    A.cnt_in = c.take<FaCnt>(nt1); A.cnt_out = c.take<FaCnt>(nt1);
    size_t tmp = p.tmp_m > p.tmp_s ? p.tmp_m : p.tmp_s;
    if (p.tmp_c > tmp) tmp = p.tmp_c;
    p.d_tmp = c.take<char>(tmp);
    p.bytes = c.bytes();
    return 0;
}

static int fa_device(int device, const char *what)
{
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) { hsa_set_error("%s: no HIP device visible", what); return HSA_E_NODEV; }
    if (device < 0 || device >= nd) { hsa_set_error("%s: device %d of %d", what, device, nd); return HSA_E_ARG; }
    HSA_HIP(hipSetDevice(device));
    return 0;
}

extern "C" int hsa_fasta_scratch_bytes(int device, uint64_t n_in, uint64_t *bytes)
{
    const char *what = "hsa_fasta_scratch_bytes";
    if (!bytes) { hsa_set_error("%s: null argument", what); return HSA_E_ARG; }
    if (n_in >= 0xFFFFFF00ull) { hsa_set_error("%s: n_in under 2^32 - 256", what); return HSA_E_ARG; }
    HSA_TRY(fa_device(device, what));
    FaPlan p;
    HSA_TRY(fa_plan(p, n_in, 15u, nullptr, nullptr));
    *bytes = p.bytes;
    return 0;
}

extern "C" int hsa_fasta_device(int device, const hsa_fasta_batch_t *b, void *stream)
{
    const char *what = "hsa_fasta_device";
    if (!b || !b->d_counters || !b->d_scratch || (b->n_in && !b->d_in) || (b->pac_cap && !b->d_pac) ||
        (b->rpac_cap && !b->d_rpac) || (b->text_cap && !b->d_text) || (b->rtext_cap && !b->d_rtext) ||
        (b->rec_cap && !b->d_rec) || (b->blk_cap && !b->d_blk)) {
        hsa_set_error("%s: null argument", what);
        return HSA_E_ARG;
    }
    if (b->n_in >= 0xFFFFFF00ull) { hsa_set_error("%s: n_in under 2^32 - 256", what); return HSA_E_ARG; }
    if ((reinterpret_cast<uintptr_t>(b->d_pac) & 3u) || (reinterpret_cast<uintptr_t>(b->d_rpac) & 3u) ||
        (reinterpret_cast<uintptr_t>(b->d_scratch) & 255u)) {
        hsa_set_error("%s: d_pac and d_rpac on 4-byte, d_scratch on 256-byte boundaries", what);
        return HSA_E_ARG;
    }
    HSA_TRY(fa_device(device, what));
    hipStream_t st = (hipStream_t)stream;
    FaPlan p;
    HSA_TRY(fa_plan(p, b->n_in, b->n_in ? (uint32_t)(reinterpret_cast<uintptr_t>(b->d_in) & 15u) : 0u, b->d_scratch, st));
    if (b->scratch_bytes < p.bytes) {
        hsa_set_error("%s: scratch of %llu bytes, %llu needed (hsa_fasta_scratch_bytes)", what,
                      (unsigned long long)b->scratch_bytes, (unsigned long long)p.bytes);
        return HSA_E_ARG;
    }
    FaArgs &A = p.A;
    A.in = b->d_in;
    A.pac = b->d_pac; A.pac_cap = b->pac_cap; A.rpac = b->d_rpac; A.rpac_cap = b->rpac_cap;
    A.text = b->d_text; A.text_cap = b->text_cap; A.rtext = b->d_rtext; A.rtext_cap = b->rtext_cap;
    A.rec = b->d_rec; A.rec_cap = b->rec_cap; A.blk = b->d_blk; A.blk_cap = b->blk_cap;
    A.ctr = (unsigned long long *)b->d_counters;
    const uint32_t nt = A.ntiles;
    StageTimer &tm = g_fa_t;
    HSA_TRY(tm.begin(g_fa_timing != 0));
    HSA_TRY(tm.mark(0, st));
    HSA_HIP(hipMemsetAsync(A.g, 0xFF, 4, st));               // nothing refused yet
    // (the entry behind the last tile is the scans' identity: its output is the total)
    HSA_HIP(hipMemsetAsync(A.mark_in + nt, 0, sizeof(FaMark), st));
    HSA_HIP(hipMemsetAsync(A.sumf_in + nt, 0, sizeof(FaSum), st));
    HSA_HIP(hipMemsetAsync(A.sumb_in + nt, 0, sizeof(FaSum), st));
    HSA_HIP(hipMemsetAsync(A.cnt_in + nt, 0, sizeof(FaCnt), st));
    if (nt) {
        hipLaunchKernelGGL(k_fa_marks, dim3(nt), dim3(256), 0, st, A);
        HSA_HIP(hipGetLastError());
    }
    HSA_TRY(tm.mark(1, st));
    HSA_HIP(rocprim::exclusive_scan(p.d_tmp, p.tmp_m, A.mark_in, A.mark_out, FaMark{0, 0, 0}, (size_t)nt + 1, FaMarkOp(), st));
    HSA_TRY(tm.mark(2, st));
    if (nt) {
        hipLaunchKernelGGL(k_fa_spans, dim3(nt), dim3(256), 0, st, A);
        HSA_HIP(hipGetLastError());
    }
    HSA_TRY(tm.mark(3, st));
    HSA_HIP(rocprim::exclusive_scan(p.d_tmp, p.tmp_s, A.sumf_in, A.sumf_out, FaSum{0, 0, 0, 0, 0, 0}, (size_t)nt + 1, FaCat(), st));
    HSA_HIP(rocprim::exclusive_scan(p.d_tmp, p.tmp_s, A.sumb_in, A.sumb_out, FaSum{0, 0, 0, 0, 0, 0}, (size_t)nt + 1, FaCatRev(), st));
    HSA_TRY(tm.mark(4, st));
    if (nt) {
        hipLaunchKernelGGL(k_fa_count, dim3(nt), dim3(256), 0, st, A);
        HSA_HIP(hipGetLastError());
    }
    HSA_TRY(tm.mark(5, st));
    HSA_HIP(rocprim::exclusive_scan(p.d_tmp, p.tmp_c, A.cnt_in, A.cnt_out, FaCnt{0, 0, 0, 0, 0}, (size_t)nt + 1, FaCntCat(), st));
    HSA_TRY(tm.mark(6, st));
    if (nt) {
        hipLaunchKernelGGL(k_fa_pack, dim3(nt), dim3(256), 0, st, A);
        HSA_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_fa_finish, dim3(1), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(7, st));
    // (the reversed text has at most T <= n_in + 3 codes; its .rev.pac bytes fit the same words)
    const uint64_t max_words = (b->n_in + 3u + 15u) / 16u + 4u + FA_PAD_WORDS;
    hipLaunchKernelGGL(k_fa_reverse, dim3((unsigned)((max_words + 255u) / 256u)), dim3(256), 0, st, A, max_words);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(8, st));
    tm.end();
    return 0;
}

// ---- the .bwt and .fmv bodies ----

struct Bf4 {
    uint32_t c[4];
};
struct Bf4Plus {
    __host__ __device__ Bf4 operator()(const Bf4 &a, const Bf4 &b) const
    {
        return Bf4{{a.c[0] + b.c[0], a.c[1] + b.c[1], a.c[2] + b.c[2], a.c[3] + b.c[3]}};
    }
};
struct BfArgs {
    const uint32_t *lsb;
    uint64_t T, nw, n_occ, n_major;
    uint32_t *msb, *minor, *major;
    Bf4 *cnt, *pref;                   // n_occ each: the counts of block e, of the blocks before sample e
};

// One lane per 256 characters: its 16 words cut at T, their code words, the four counts
// (what lies past T counts as 'A': BWTConstruct.c:997-1090 reads the cleared tail words)
__global__ void __launch_bounds__(256) k_bf_blocks(BfArgs a)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= a.n_occ) return;
    uint32_t c1 = 0u, c2 = 0u, c3 = 0u;
    for (uint32_t q = 0; q < 16u; ++q) {
        const uint64_t w = 16u * e + q;
        if (w >= a.nw) break;
        const uint32_t x = fa_low(a.lsb[w], a.T - 16u * w);
        a.msb[w] = fa_rev2_32(x);
        const uint32_t lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
        c1 += __popc(lo & ~hi); c2 += __popc(hi & ~lo); c3 += __popc(lo & hi);
    }
    a.cnt[e] = Bf4{{256u - c1 - c2 - c3, c1, c2, c3}};
}

// One lane per pair of minor samples (a word per character), and per major sample
__global__ void __launch_bounds__(256) k_bf_samples(BfArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < (a.n_occ + 1u) / 2u) {
        const uint64_t e0 = 2u * i, e1 = e0 + 1u < a.n_occ ? e0 + 1u : e0;     // (an odd count repeats the last sample)
        const Bf4 m0 = a.pref[e0 & ~(uint64_t)255u], m1 = a.pref[e1 & ~(uint64_t)255u], p0 = a.pref[e0], p1 = a.pref[e1];
        for (int ch = 0; ch < 4; ++ch) a.minor[4u * i + ch] = ((p0.c[ch] - m0.c[ch]) << 16) | (p1.c[ch] - m1.c[ch]);
    }
    if (i < a.n_major) {
        const Bf4 p = a.pref[256u * i];
        for (int ch = 0; ch < 4; ++ch) a.major[4u * i + ch] = p.c[ch];
    }
}

static int bf_plan(BfArgs &A, uint64_t T, void *base, void *&d_tmp, size_t &tmp, size_t &bytes, hipStream_t st)
{
    A.T = T; A.nw = (T + 15u) / 16u;
    A.n_occ = (T + 255u) / 256u + 1u;                      // BWT.c:1097-1117
    A.n_major = (A.n_occ + 255u) / 256u;
    HSA_TRY(hsa_scan_bytes(tmp, Bf4{{0, 0, 0, 0}}, (size_t)A.n_occ, Bf4Plus(), st));
    Carver c(base);
    A.cnt = c.take<Bf4>(A.n_occ); A.pref = c.take<Bf4>(A.n_occ);
    d_tmp = c.take<char>(tmp);
    bytes = c.bytes();
    return 0;
}

extern "C" int hsa_bwt_files_scratch_bytes(int device, uint64_t T, uint64_t *bytes)
{
    const char *what = "hsa_bwt_files_scratch_bytes";
    if (!bytes) { hsa_set_error("%s: null argument", what); return HSA_E_ARG; }
    if (T < 1u || T >= 0xFFFFFFFFull) { hsa_set_error("%s: T in 1..2^32 - 2", what); return HSA_E_ARG; }
    HSA_TRY(fa_device(device, what));
    BfArgs A;
    void *d_tmp;
    size_t tmp, n;
    HSA_TRY(bf_plan(A, T, nullptr, d_tmp, tmp, n, nullptr));
    *bytes = n;
    return 0;
}

extern "C" int hsa_bwt_files_device(int device, uint64_t T, const uint32_t *d_bwt_lsb, uint32_t *d_bwt_msb,
                                    uint32_t *d_minor, uint32_t *d_major, void *d_scratch, uint64_t scratch_bytes,
                                    void *stream)
{
    const char *what = "hsa_bwt_files_device";
    if (!d_bwt_lsb || !d_bwt_msb || !d_minor || !d_major || !d_scratch) { hsa_set_error("%s: null argument", what); return HSA_E_ARG; }
    if (T < 1u || T >= 0xFFFFFFFFull) { hsa_set_error("%s: T in 1..2^32 - 2", what); return HSA_E_ARG; }
    if (reinterpret_cast<uintptr_t>(d_scratch) & 255u) { hsa_set_error("%s: d_scratch on a 256-byte boundary", what); return HSA_E_ARG; }
    HSA_TRY(fa_device(device, what));
    hipStream_t st = (hipStream_t)stream;
    BfArgs A;
    void *d_tmp;
    size_t tmp, need;
    HSA_TRY(bf_plan(A, T, d_scratch, d_tmp, tmp, need, st));
    if (scratch_bytes < need) {
        hsa_set_error("%s: scratch of %llu bytes, %llu needed (hsa_bwt_files_scratch_bytes)", what,
                      (unsigned long long)scratch_bytes, (unsigned long long)need);
        return HSA_E_ARG;
    }
    A.lsb = d_bwt_lsb; A.msb = d_bwt_msb; A.minor = d_minor; A.major = d_major;
    StageTimer &tm = g_bf_t;
    HSA_TRY(tm.begin(g_fa_timing != 0));
    HSA_TRY(tm.mark(0, st));
    hipLaunchKernelGGL(k_bf_blocks, dim3((unsigned)((A.n_occ + 255u) / 256u)), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(1, st));
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp, A.cnt, A.pref, Bf4{{0, 0, 0, 0}}, (size_t)A.n_occ, Bf4Plus(), st));
    HSA_TRY(tm.mark(2, st));
    hipLaunchKernelGGL(k_bf_samples, dim3((unsigned)(((A.n_occ + 1u) / 2u + 255u) / 256u)), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(3, st));
    tm.end();
    return 0;
}
