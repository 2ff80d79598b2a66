// hsa_junctions.hip -- the splice junction table of a run: one row per distinct intron of the
// printed XT:A:S lines, with its read support, in the nine columns of STAR's SJ.out.tab.
//
// The reference prints no such table; it is defined as a function of the SAM text the lines
// stage prints (hsa_splice_rows.hip) and the index's text and block table, and
// hsa_amd/junctions.py: from_sam restates it on the host from that text.  Only a line's own
// alignment counts: the introns of its XA:Z entries cannot be read back from the reference's
// format for them ("<pos><len>M..." with nothing between the two numbers).
//
// Three calls in the conventions of the lines stage (the caller's stream, no synchronisation,
// scratch on the handle, counters that say wanted against room, nothing written past a
// capacity, no atomic places a row or a byte, two runs give equal arrays):
//
// hsa_junction_rows_device    one row per read with HSA_SL_OK of one lines call, appended to
//   k_jn_flag   one lane per read: 1 for a read with a line and sound row words;
//   rocPRIM exclusive scan of the flags: the rows' places, in read order;
//   k_jn_rows   one lane per read: chrID, the intron's first and last base (POS plus the M and
//               D lengths before the N; plus the N length - 1), 1 | 0 as the unique and the
//               multi count (d_rows word 22: served extra pairs), min of the M sums on the
//               two sides of the N.
// hsa_junction_reduce_device  sorts and merges equal introns, in place; idempotent, so a
//               reduced table is a row buffer like any other (rows carry counts, not flags):
//   k_jn_keys   one lane per row: its key (chrID, start, end) and its index;
//   rocPRIM radix_sort_pairs over the three key words (a decomposer, chrID the most significant):
//               the table's order whatever the block table looks like;
//   rocPRIM reduce_by_key over the sorted keys, the values read through the sorted indices:
//               sums of the two counts, max of the overhang; a run of any length is reduced by
//               the whole device, not by one lane;
//   k_jn_pack   one lane per distinct intron: its row, with the motif from the packed text:
//               each of the four bases' chromosome coordinates goes through the block table
//               on its own (text distance is not chromosome distance across an N run), and a
//               base in no block makes the motif 0.
// hsa_junction_text_device    the table's text from a reduced table:
//   k_jn_len    one lane per row: the length of its line (jn_emit on the counting sink of
//               hsa_sam_sinks.h);
//   rocPRIM exclusive scan: d_line_off;
//   k_jn_write  one lane per row: jn_emit on the storing sink.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "hsa_device.h"
#include "hsa_internal.h"
#include "hsa_sam_sinks.h"
#include "hsa_text.h"

#define JN_NONE 0xFFFFFFFFu

struct JnKey {
    uint32_t chr, start, end;
    __host__ __device__ bool operator==(const JnKey &o) const { return chr == o.chr && start == o.start && end == o.end; }
};
struct JnKeyParts {
    __host__ __device__ rocprim::tuple<uint32_t &, uint32_t &, uint32_t &> operator()(JnKey &k) const
    {
        return rocprim::tuple<uint32_t &, uint32_t &, uint32_t &>(k.chr, k.start, k.end);
    }
};
struct JnVal {
    uint32_t uniq, multi, over;
};
struct JnMerge {
    __host__ __device__ JnVal operator()(const JnVal &a, const JnVal &b) const
    {
        return JnVal{a.uniq + b.uniq, a.multi + b.multi, a.over > b.over ? a.over : b.over};
    }
};
// the counts and the overhang of row i of a row buffer
struct JnValOf {
    const uint32_t *rows;
    __host__ __device__ JnVal operator()(uint32_t i) const
    {
        const uint32_t *r = rows + (size_t)HSA_JN_ROW_WORDS * i;
        return JnVal{r[3], r[4], r[5]};
    }
};

// ---------------------------------------------------------------- rows
struct JnRowsArgs {
    uint32_t n_jobs, cigar_stride;
    const uint32_t *rows, *cigar, *stat;
    uint32_t *jrows;
    uint64_t n_have, row_cap;
    uint64_t *flag, *off;          // n_jobs + 1
    unsigned long long *ctr;
};

// A read with a line whose row words the walk below can trust: the N where word 20 says.
__device__ __forceinline__ bool jn_sound(const JnRowsArgs &a, uint32_t j)
{
    const uint32_t *row = a.rows + (size_t)HSA_SL_ROW_WORDS * j;
    if (a.stat[j] != HSA_SL_OK || row[0] != HSA_SL_OK) return false;
    const uint32_t n_cigar = row[5], at = row[20];
    if (n_cigar > a.cigar_stride || at >= n_cigar) return false;
    const uint32_t w = a.cigar[(size_t)a.cigar_stride * j + at];
    return (w >> 28) == 3u && (w & 0x0FFFFFFFu) == row[18] && row[18] != 0u;
}

__global__ void __launch_bounds__(256) k_jn_flag(JnRowsArgs a)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > a.n_jobs) return;
    a.flag[j] = j < a.n_jobs && jn_sound(a, j) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_jn_rows(JnRowsArgs a)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t room = a.row_cap > a.n_have ? a.row_cap - a.n_have : 0u;
    if (j == 0) {
        const uint64_t want = a.off[a.n_jobs];
        a.ctr[0] = want;
        a.ctr[1] = want < room ? want : room;
    }
    if (j >= a.n_jobs || a.flag[j] == 0u) return;
    const uint64_t at = a.off[j];
    if (at >= room) return;                                // no row at or past row_cap
    const uint32_t *row = a.rows + (size_t)HSA_SL_ROW_WORDS * j;
    const uint32_t *cg = a.cigar + (size_t)a.cigar_stride * j;
    const uint32_t n_cigar = row[5], n_at = row[20];
    uint64_t ref = 0, m5 = 0, m3 = 0;                      // M + D before the N; M before; M behind
    for (uint32_t i = 0; i < n_cigar; ++i) {
        const uint32_t op = cg[i] >> 28, len = cg[i] & 0x0FFFFFFFu;
        if (i < n_at) {
            if (op == 0u) { ref += len; m5 += len; }
            else if (op == 2u) ref += len;
        } else if (i > n_at && op == 0u) m3 += len;
    }
    const uint64_t start = (uint64_t)row[7] + ref;
    const uint64_t end = start + row[18] - 1u;
    const uint64_t over = m5 < m3 ? m5 : m3;
    uint4 *o = reinterpret_cast<uint4 *>(a.jrows + (size_t)HSA_JN_ROW_WORDS * (a.n_have + at));
    const bool multi = row[22] != 0u;
    // (a coordinate past 32 bits cannot come from a 32-bit block table: all-ones, mapped to no block)
    o[0] = make_uint4(row[6], start > JN_NONE ? JN_NONE : (uint32_t)start, end > JN_NONE ? JN_NONE : (uint32_t)end, multi ? 0u : 1u);
    o[1] = make_uint4(multi ? 1u : 0u, (uint32_t)over, 0u, 0u);
}

extern "C" int hsa_junction_rows_device(hsa_index_t *ix, const hsa_junction_rows_batch_t *b, void *stream)
{
    const char *what = "hsa_junction_rows_device";
    if (!ix) { hsa_set_error("%s: null handle", what); return HSA_E_ARG; }
    if (!b || b->n_jobs < 0 || !b->d_counters || (b->row_cap && !b->d_jrows) || b->n_have > b->row_cap) {
        hsa_set_error("%s: bad arguments", what);
        return HSA_E_ARG;
    }
    if (b->n_jobs && (!b->d_rows || !b->d_line_stat || (b->cigar_stride && !b->d_cigar))) {
        hsa_set_error("%s: null argument", what);
        return HSA_E_ARG;
    }
    if (b->row_cap > 0xFFFFFFFFull) { hsa_set_error("%s: row_cap over 2^32 - 1 (rows are sorted by 32-bit indices)", what); return HSA_E_ARG; }
    const uint64_t n = (uint64_t)b->n_jobs;
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    HSA_HIP(hipMemsetAsync(b->d_counters, 0, 8 * sizeof(uint64_t), st));
    if (n == 0) return 0;
    size_t tmp_bytes = 0;
    HSA_TRY(hsa_scan_bytes(tmp_bytes, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
    JnRowsArgs A;
    void *d_tmp = nullptr;
    auto layout = [&](Carver c) {
        A.flag = c.take<uint64_t>(n + 1);
        A.off = c.take<uint64_t>(n + 1);
        d_tmp = c.take<char>(tmp_bytes);
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_sl, &ix->d_sl_cap, layout(Carver())));
    layout(Carver(ix->d_sl));
    A.n_jobs = (uint32_t)n; A.cigar_stride = b->cigar_stride;
    A.rows = b->d_rows; A.cigar = b->d_cigar; A.stat = b->d_line_stat;
    A.jrows = b->d_jrows; A.n_have = b->n_have; A.row_cap = b->row_cap;
    A.ctr = (unsigned long long *)b->d_counters;
    const unsigned blocks = (unsigned)((n + 1 + 255) / 256);
    hipLaunchKernelGGL(k_jn_flag, dim3(blocks), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, A.flag, A.off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
    hipLaunchKernelGGL(k_jn_rows, dim3(blocks), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- reduce
struct JnReduceArgs {
    uint32_t n;
    uint32_t *jrows;
    JnKey *keys;                   // n: the rows' keys; then the distinct introns'
    uint32_t *idx;
    const JnKey *ukeys;
    const JnVal *uvals;
    const uint32_t *blocks;        // n_blocks rows (chrID, blockStart, blockEnd, ori), ascending in (chrID, ori)
    uint32_t n_blocks;
    TextView text;
    unsigned long long *ctr;
};

__global__ void __launch_bounds__(256) k_jn_keys(JnReduceArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint4 r = *reinterpret_cast<const uint4 *>(a.jrows + (size_t)HSA_JN_ROW_WORDS * i);
    a.keys[i] = JnKey{r.x, r.y, r.z};
    a.idx[i] = i;
}

// The text position of base p (1-based) of chromosome c; false inside an N run, past the
// chromosome's last block or for a chromosome the table does not have.
__device__ __forceinline__ bool jn_text_pos(const JnReduceArgs &a, uint32_t c, uint64_t p, uint64_t &t)
{
    if (p == 0u) return false;
    uint32_t lo = 0, hi = a.n_blocks;                      // the first block that starts behind (c, p)
    while (lo < hi) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        const uint32_t cm = a.blocks[4 * (size_t)m];
        if (cm < c || (cm == c && (uint64_t)a.blocks[4 * (size_t)m + 3] + 1u <= p)) lo = m + 1u; else hi = m;
    }
    if (lo == 0u) return false;
    const uint32_t *bl = a.blocks + 4 * (size_t)(lo - 1u);
    if (bl[0] != c || bl[2] < bl[1]) return false;
    const uint64_t k = p - 1u - bl[3];
    if (k > (uint64_t)(bl[2] - bl[1])) return false;
    t = (uint64_t)bl[1] + k;
    return t < a.text.n;
}

// 1 GT/AG, 2 CT/AC, 3 GC/AG, 4 CT/GC, 5 AT/AC, 6 GT/AT, 0 anything else (codes A C G T = 0 1 2 3)
__device__ __forceinline__ uint32_t jn_motif_code(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3)
{
    switch ((b0 << 6) | (b1 << 4) | (b2 << 2) | b3) {
    case (2u << 6) | (3u << 4) | (0u << 2) | 2u: return 1u;
    case (1u << 6) | (3u << 4) | (0u << 2) | 1u: return 2u;
    case (2u << 6) | (1u << 4) | (0u << 2) | 2u: return 3u;
    case (1u << 6) | (3u << 4) | (2u << 2) | 1u: return 4u;
    case (0u << 6) | (3u << 4) | (0u << 2) | 1u: return 5u;
    case (2u << 6) | (3u << 4) | (0u << 2) | 3u: return 6u;
    default: return 0u;
    }
}

__device__ __forceinline__ uint32_t jn_motif(const JnReduceArgs &a, const JnKey &k)
{
    if (k.end <= k.start) return 0u;                       // (fewer than two bases)
    const uint64_t p[4] = {k.start, (uint64_t)k.start + 1u, (uint64_t)k.end - 1u, k.end};
    uint32_t b[4];
    for (uint32_t i = 0; i < 4u; ++i) {
        uint64_t t;
        if (!jn_text_pos(a, k.chr, p[i], t)) return 0u;
        b[i] = hsa_text_code(a.text, t);
    }
    return jn_motif_code(b[0], b[1], b[2], b[3]);
}

__global__ void __launch_bounds__(256) k_jn_pack(JnReduceArgs a)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long m = a.ctr[1];                 // distinct introns (rocPRIM's count)
    if (r == 0) a.ctr[0] = a.n;
    if (r >= m || r >= a.n) return;
    const JnKey k = a.ukeys[r];
    const JnVal v = a.uvals[r];
    uint4 *o = reinterpret_cast<uint4 *>(a.jrows + (size_t)HSA_JN_ROW_WORDS * r);
    o[0] = make_uint4(k.chr, k.start, k.end, v.uniq);
    o[1] = make_uint4(v.multi, v.over, jn_motif(a, k), 0u);
}

extern "C" int hsa_junction_reduce_device(hsa_index_t *ix, const hsa_junction_reduce_batch_t *b, void *stream)
{
    const char *what = "hsa_junction_reduce_device";
    if (!ix) { hsa_set_error("%s: null handle", what); return HSA_E_ARG; }
    if (ix->is64) { hsa_set_error("%s: the index text has 2^32 characters or more: the splice path is 32-bit", what); return HSA_E_ARG; }
    if (!b || !b->d_counters || (b->n_rows && !b->d_jrows) || b->n_rows > 0xFFFFFFFFull) {
        hsa_set_error("%s: bad arguments", what);
        return HSA_E_ARG;
    }
    if (!ix->d_blocks || (!ix->d_text && !ix->d_text64)) {
        hsa_set_error("%s: needs hsa_index_set_sa (the block table) and a text (hsa_index_set_text)", what);
        return HSA_E_ARG;
    }
    if (!ix->d_text64 && ((uint64_t)ix->dna_len + 15u) / 16u > ix->text_words) {
        hsa_set_error("%s: the packed text does not cover dna_len", what);
        return HSA_E_ARG;
    }
    const uint64_t n = b->n_rows;
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    HSA_HIP(hipMemsetAsync(b->d_counters, 0, 8 * sizeof(uint64_t), st));
    if (n == 0) return 0;
    JnReduceArgs A;
    A.n = (uint32_t)n; A.jrows = b->d_jrows;
    A.blocks = ix->d_blocks; A.n_blocks = ix->n_blocks;
    if (ix->d_text64) { A.text.w = ix->d_text64; A.text.n = ix->T64; A.text.lsb = 1u; }
    else { A.text.w = ix->d_text; A.text.n = ix->dna_len; A.text.lsb = 0u; }
    A.ctr = (unsigned long long *)b->d_counters;
    JnKey *keys2 = nullptr;
    uint32_t *idx2 = nullptr;
    JnVal *uvals = nullptr;
    size_t sort_bytes = 0, red_bytes = 0;
    HSA_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (JnKey *)nullptr, (JnKey *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                      (size_t)n, JnKeyParts(), 0u, 96u, st));
    auto values = [&]() { return rocprim::make_transform_iterator(idx2, JnValOf{A.jrows}); };
    HSA_HIP(rocprim::reduce_by_key(nullptr, red_bytes, (JnKey *)nullptr, values(), (size_t)n, (JnKey *)nullptr, (JnVal *)nullptr,
                                   A.ctr + 1, JnMerge(), rocprim::equal_to<JnKey>(), st));
    const size_t tmp_bytes = sort_bytes > red_bytes ? sort_bytes : red_bytes;
    void *d_tmp = nullptr;
    auto layout = [&](Carver c) {
        A.keys = c.take<JnKey>(n);
        keys2 = c.take<JnKey>(n);
        A.idx = c.take<uint32_t>(n);
        idx2 = c.take<uint32_t>(n);
        uvals = c.take<JnVal>(n);
        d_tmp = c.take<char>(tmp_bytes);
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_sl, &ix->d_sl_cap, layout(Carver())));
    layout(Carver(ix->d_sl));
    A.ukeys = A.keys; A.uvals = uvals;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_jn_keys, dim3(blocks), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    size_t bytes = tmp_bytes;
    HSA_HIP(rocprim::radix_sort_pairs(d_tmp, bytes, A.keys, keys2, A.idx, idx2, (size_t)n, JnKeyParts(), 0u, 96u, st));
    bytes = tmp_bytes;
    // (the rows' keys are read no more: the distinct introns' keys take their place)
    HSA_HIP(rocprim::reduce_by_key(d_tmp, bytes, keys2, values(), (size_t)n, A.keys, uvals, A.ctr + 1, JnMerge(),
                                   rocprim::equal_to<JnKey>(), st));
    hipLaunchKernelGGL(k_jn_pack, dim3(blocks), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- text
struct JnTextArgs {
    uint32_t n, n_chr;
    const uint32_t *jrows;
    const uint8_t *chr_names;
    const uint64_t *chr_off;
    uint64_t *lens, *line_off;     // n + 1
    uint8_t *out;
    uint64_t out_cap;
    unsigned long long *ctr;
};

// chromosome, first base, last base, strand, motif, 0, unique, multi, overhang
template <class S> __device__ __forceinline__ void jn_emit(const JnTextArgs &a, const uint4 r0, const uint4 r1, S &s)
{
    const uint64_t co = a.chr_off[r0.x];
    s.bytes(a.chr_names + co, (uint32_t)(a.chr_off[r0.x + 1u] - co));
    s.ch('\t'); s.dec(r0.y);
    s.ch('\t'); s.dec(r0.z);
    s.ch('\t'); s.dec(r1.z == 0u ? 0u : (r1.z & 1u) ? 1u : 2u);
    s.ch('\t'); s.dec(r1.z);
    s.lit("\t0\t"); s.dec(r0.w);
    s.ch('\t'); s.dec(r1.x);
    s.ch('\t'); s.dec(r1.y);
    s.ch('\n');
}

// a row the writer can print: a chromosome of the table with a name of sane offsets, a motif code
__device__ __forceinline__ bool jn_printable(const JnTextArgs &a, const uint4 r0, const uint4 r1)
{
    if (r0.x >= a.n_chr || r1.z > 6u) return false;
    const uint64_t lo = a.chr_off[r0.x], hi = a.chr_off[r0.x + 1u];
    return hi >= lo && hi - lo <= HSA_SAM_MAX_LINE;
}

__global__ void __launch_bounds__(256) k_jn_len(JnTextArgs a)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > a.n) return;
    uint64_t len = 0;
    if (r < a.n) {
        const uint4 *p = reinterpret_cast<const uint4 *>(a.jrows + (size_t)HSA_JN_ROW_WORDS * r);
        const uint4 r0 = p[0], r1 = p[1];
        if (jn_printable(a, r0, r1)) {
            SmCount s;
            jn_emit(a, r0, r1, s);
            len = s.n;
        }
    }
    a.lens[r] = len;
    // the counts only, one add per wavefront (a row without a line: none from the calls above)
    const unsigned long long printed = __ballot(len != 0u), refused = __ballot(r < a.n && len == 0u);
    if ((threadIdx.x & 63u) == 0u) {
        if (printed) atomicAdd(&a.ctr[2], (unsigned long long)__popcll(printed));
        if (refused) atomicAdd(&a.ctr[3], (unsigned long long)__popcll(refused));
    }
}

__global__ void __launch_bounds__(256) k_jn_write(JnTextArgs a)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r == 0) {
        const uint64_t total = a.line_off[a.n];
        a.ctr[0] = total;
        a.ctr[1] = total < a.out_cap ? total : a.out_cap;
    }
    if (r >= a.n) return;
    const uint64_t base = a.line_off[r], end = a.line_off[r + 1];
    if (end <= base || base >= a.out_cap) return;
    const uint64_t room = a.out_cap - base;
    const uint4 *p = reinterpret_cast<const uint4 *>(a.jrows + (size_t)HSA_JN_ROW_WORDS * r);
    SmStore s{a.out + base, 0u, (uint32_t)(end - base < room ? end - base : room)};      // no byte at or past out_cap
    jn_emit(a, p[0], p[1], s);
}

extern "C" int hsa_junction_text_device(hsa_index_t *ix, const hsa_junction_text_batch_t *b, void *stream)
{
    const char *what = "hsa_junction_text_device";
    if (!ix) { hsa_set_error("%s: null handle", what); return HSA_E_ARG; }
    if (!b || !b->d_counters || !b->d_line_off || (b->out_cap && !b->d_out) || b->n_rows > 0xFFFFFFFFull) {
        hsa_set_error("%s: bad arguments", what);
        return HSA_E_ARG;
    }
    if (b->n_rows && (!b->d_jrows || (b->n_chr && (!b->d_chr_names || !b->d_chr_off)))) {
        hsa_set_error("%s: null argument", what);
        return HSA_E_ARG;
    }
    const uint64_t n = b->n_rows;
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    HSA_HIP(hipMemsetAsync(b->d_counters, 0, 8 * sizeof(uint64_t), st));
    if (n == 0) {
        HSA_HIP(hipMemsetAsync(b->d_line_off, 0, sizeof(uint64_t), st));
        return 0;
    }
    size_t tmp_bytes = 0;
    HSA_TRY(hsa_scan_bytes(tmp_bytes, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
    JnTextArgs A;
    void *d_tmp = nullptr;
    auto layout = [&](Carver c) {
        A.lens = c.take<uint64_t>(n + 1);
        d_tmp = c.take<char>(tmp_bytes);
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_sl, &ix->d_sl_cap, layout(Carver())));
    layout(Carver(ix->d_sl));
    A.n = (uint32_t)n; A.n_chr = b->n_chr; A.jrows = b->d_jrows;
    A.chr_names = b->d_chr_names; A.chr_off = b->d_chr_off;
    A.line_off = b->d_line_off; A.out = b->d_out; A.out_cap = b->out_cap;
    A.ctr = (unsigned long long *)b->d_counters;
    const unsigned blocks = (unsigned)((n + 1 + 255) / 256);
    hipLaunchKernelGGL(k_jn_len, dim3(blocks), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, A.lens, A.line_off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
    hipLaunchKernelGGL(k_jn_write, dim3(blocks), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    return 0;
}
