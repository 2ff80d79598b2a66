// hsa_sam.hip -- the SAM lines of a batch on the 64-bit path.
//
// bwa_print_sam1 with mate == NULL (bwtse.c:698-799) for every read of a batch, from the
// device outputs of search, choose and refine: hsa_amd/sam.py: sam_line per read, byte for
// byte, and '\n'.  hsa_sam_lines_device64 is three launches on one stream:
//   k_sam_len    one lane per read: its status (every index taken from a device array is
//                checked here, before anything uses it) and the exact length of its line;
//   rocPRIM exclusive scan of the lengths in read order: d_line_off.  No atomic places a
//                byte, so two runs give equal arrays;
//   k_sam_write  one wavefront per tile of `tile` consecutive reads.  A tile owns the
//                contiguous output range [line_off[j0], line_off[j1]) and assembles it in
//                LDS, at the range's own offset within a 16-byte unit.
// One function, sm_emit, walks the fields of a line for both kernels: k_sam_len hands it a
// sink that counts, k_sam_write one that stores to LDS, so the length and the bytes cannot
// disagree.
//
// k_sam_write in three phases, a barrier between them:
//   A  lane r formats the small fields of read j0 + r (numbers, chromosome name, CIGAR,
//      tags, MD, XA) into its line's place in LDS and leaves the places of the three
//      long fields (name, SEQ, QUAL) in LDS words;
//   B  the wave walks the tile's reads and copies name, SEQ and QUAL with the lanes along
//      the bytes: consecutive lanes load consecutive input bytes.  SEQ is a shift of a
//      packed "ACGTN" / "TGCAN" word, no table load;
//   C  the range leaves LDS: the bytes before the first and after the last 16-byte
//      boundary of the output as byte stores (those units are shared with the
//      neighbouring tiles and never read back), everything between as aligned 16-byte
//      stores, lanes along units.
// Phase A is the only lane-dependent region and lies between two barriers; the loops of
// B and C hold no wave-level operation (no barrier, no cross-lane move), so no lane waits
// inside a loop for one that took another path.
//
// The tile: tile = clamp(SM_TILE_BYTES / max_line, 1, 64) reads, so the LDS of a block is
// tile * max_line + 16 bytes of text (at most HSA_SAM_MAX_LINE + 16) and 3 072 bytes of
// marks: known on the host from the batch's max_line.  k_sam_len refuses a line longer than
// max_line, and every LDS store is bounded by the buffer besides.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <string.h>

#include "hsa_device.h"
#include "hsa_internal.h"
#include "hsa_sa.h"
#include "hsa_sam_sinks.h"

#ifndef SM_TILE_BYTES
#define SM_TILE_BYTES 16384u
#endif
#define SM_TILE_MAX 64u

struct SamArgs {
    const hsa_job_t *jobs;
    uint32_t n_jobs;
    const uint8_t *codes;
    const int32_t *n_aln;
    const uint64_t *hit_off;
    const uint32_t *hits;
    const uint32_t *sel;
    const uint64_t *sel64;
    const uint64_t *pos_off, *pos;
    const uint32_t *pos_hit;
    uint64_t pos_cap;
    const uint64_t *pos_ctr;
    const uint32_t *rows;
    const uint64_t *rpos;
    const uint32_t *cigar;
    const uint8_t *md;
    uint32_t cigar_stride, md_stride;
    const uint8_t *names; const uint64_t *name_off;
    const uint8_t *quals; const uint64_t *qual_off;
    const uint8_t *chr_names; const uint64_t *chr_off;
    uint32_t n_chr, flag;
    int32_t max_top2, comp_read;
    uint32_t max_line, tile, lds_text;     // lds_text: bytes of the tile's text buffer
    uint64_t *line_off;
    uint8_t *out;
    uint64_t out_cap;
    uint32_t *stat;
    unsigned long long *ctr;
    uint64_t *lens;                        // scratch: n_jobs + 1
    // trimmed reads and barcodes (hsa_sam_trim_t); null / 0: every read is whole, no barcode
    const uint32_t *full_len;
    const uint8_t *bc;
    uint32_t bc_len;
};

// The stored length of read j: SEQ and QUAL are printed over it (bwtse.c:738-749), while
// hsa_job_t.len, what the search saw, is the XC tag's clip_len.
__device__ __forceinline__ uint32_t sm_full_len(const SamArgs &a, uint32_t j, uint32_t len) { return a.full_len ? a.full_len[j] : len; }

__device__ __forceinline__ uint64_t sm_n_rows(const SamArgs &a)
{
    uint64_t n = a.pos_off[a.n_jobs];
    if (n > a.pos_cap) n = a.pos_cap;
    if (a.pos_ctr && a.pos_ctr[1] < n) n = a.pos_ctr[1];
    return n;
}

// where phase B finds and puts a read's long fields
struct SmMark {
    uint64_t name_src, code_off, qual_off;
    uint32_t name_dst, name_len, seq_dst, qual_dst, len, strand;
};

template <class S> __device__ __forceinline__ void sm_cigar(const SamArgs &a, uint64_t t, S &s)
{
    const uint32_t n = a.rows[HSA_RF_ROW_WORDS * t + 1];
    const uint32_t *ops = a.cigar + (size_t)a.cigar_stride * t;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t w = ops[i];
        s.dec(w & 0x0FFFFFFFu);
        s.ch((char)sm_op_letter(w >> 28));
    }
}

template <class S> __device__ __forceinline__ void sm_chr(const SamArgs &a, uint64_t t, S &s)
{
    const uint64_t c = a.pos[4 * t + 1];
    const uint64_t o = a.chr_off[c];
    s.bytes(a.chr_names + o, (uint32_t)(a.chr_off[c + 1] - o));
}

// The line of read j, a read of status HSA_SAM_OK: every index below was checked by
// sm_status.  Name, SEQ and QUAL are skipped and their places left in mk.
template <class S> __device__ __forceinline__ void sm_emit(const SamArgs &a, uint32_t j, S &s, SmMark &mk)
{
    const hsa_job_t jb = a.jobs[j];
    const uint64_t r0 = a.pos_off[j];
    const uint32_t typ = a.sel[4 * (size_t)j], mapq = a.sel[4 * (size_t)j + 2], n_xa = a.sel[4 * (size_t)j + 3];
    const uint64_t c1 = a.sel64[4 * (size_t)j + 1], c2 = a.sel64[4 * (size_t)j + 2];
    const uint64_t hoff = a.hit_off[j];
    const uint32_t *rec = a.hits + (hoff + a.pos_hit[r0]) * HSA_ALN64_WORDS;
    const uint32_t w0 = rec[0], strand = rec[1] >> 30;
    const uint32_t n_mm = w0 & 0xFFFFu, n_gapo = (w0 >> 16) & 0xFFu, n_gape = w0 >> 24;
    mk.name_src = a.name_off[j];
    mk.name_len = (uint32_t)(a.name_off[j + 1] - mk.name_src);
    mk.code_off = jb.off;
    mk.qual_off = a.quals ? a.qual_off[j] : 0;
    const uint32_t full = sm_full_len(a, j, jb.len);
    mk.len = full;
    mk.strand = strand;
    mk.name_dst = s.pos();
    s.skip(mk.name_len);
    s.ch('\t'); s.dec(a.flag | (strand ? 16u : 0u));                   // bwtse.c:706
    s.ch('\t'); sm_chr(a, r0, s);
    s.ch('\t'); s.dec(a.rpos[2 * r0 + 1]);
    s.ch('\t'); s.dec(mapq);
    s.ch('\t');                                                         // the chosen row's CIGAR alone is corrected (:637)
    sm_cigar_clipped(a.cigar + (size_t)a.cigar_stride * r0, a.rows[HSA_RF_ROW_WORDS * r0 + 1], strand, full - jb.len, s);
    s.lit("\t*\t0\t0\t");                                               // :720
    mk.seq_dst = s.pos();
    s.skip(full);
    s.ch('\t');
    mk.qual_dst = a.quals ? s.pos() : 0xFFFFFFFFu;                      // (all-ones: no QUAL to copy)
    if (a.quals) s.skip(full); else s.ch('*');
    sm_clip_tags(a.bc ? a.bc + (size_t)a.bc_len * j : nullptr, a.bc_len, jb.len, full, s);
    s.lit("\tXT:A:"); s.ch(typ == 1u ? 'U' : 'R');                      // :762
    s.ch('\t'); s.ch(a.comp_read ? 'N' : 'C'); s.lit("M:i:"); s.dec(a.rows[HSA_RF_ROW_WORDS * r0 + 2]);
    s.lit("\tX0:i:"); s.dec(c1);
    if (a.max_top2 >= 0 && c1 <= (uint64_t)a.max_top2) { s.lit("\tX1:i:"); s.dec(c2); }
    s.lit("\tXM:i:"); s.dec(n_mm);
    s.lit("\tXO:i:"); s.dec(n_gapo);
    s.lit("\tXG:i:"); s.dec(n_gapo + n_gape);
    s.lit("\tMD:Z:"); s.bytes(a.md + (size_t)a.md_stride * r0, a.rows[HSA_RF_ROW_WORDS * r0 + 3]);
    if (n_xa) {                                                         // :781-796
        s.lit("\tXA:Z:");
        for (uint64_t t = r0 + 1; t <= r0 + n_xa; ++t) {
            const uint32_t *q = a.hits + (hoff + a.pos_hit[t]) * HSA_ALN64_WORDS;
            const uint32_t q0 = q[0], gaps = ((q0 >> 16) & 0xFFu) + (q0 >> 24);
            sm_chr(a, t, s);
            s.ch(','); s.ch(q[1] >> 30 ? '-' : '+'); s.dec(a.rpos[2 * t + 1]);
            if (gaps) sm_cigar(a, t, s);
            else { s.ch(','); s.dec(gaps + (q0 & 0xFFFFu)); s.ch(';'); }
        }
    }
    s.ch('\n');
}

// The bytes of `w` that are over 4, those outside [lead, total) of the run that starts at
// byte `at` left out
__device__ __forceinline__ uint32_t sm_over4(uint32_t w, uint32_t at, uint32_t lead, uint32_t total)
{
    uint32_t m = 0xFFFFFFFFu;
    if (at < lead) m = lead - at >= 4u ? 0u : m << (8u * (lead - at));
    if (at + 4u > total) m = total <= at ? 0u : m & (0xFFFFFFFFu >> (8u * (at + 4u - total)));
    w &= m;
    return (w & 0xF8F8F8F8u) | ((w >> 2) & (w | (w >> 1)) & 0x01010101u);      // 8 and up; 5, 6, 7
}

// A base code over 4 in a read.  One lane reads its read here, so it reads whole aligned
// 16-byte words as the search does (d_codes stays readable 16 bytes past the last read's
// end: hsa_device_batch_t), 7 loads for 100 bases and not 100
__device__ __forceinline__ bool sm_bad_codes(const uint8_t *p, uint32_t len)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(p) & ~(uintptr_t)15;
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(p) - a0), total = lead + len;
    uint32_t bad = 0;
    for (uint32_t o = 0; o < total; o += 16u) {
        const uint4 w = *reinterpret_cast<const uint4 *>(a0 + o);
        bad |= sm_over4(w.x, o, lead, total) | sm_over4(w.y, o + 4u, lead, total) | sm_over4(w.z, o + 8u, lead, total) |
               sm_over4(w.w, o + 12u, lead, total);
    }
    return bad != 0u;
}

// The status of read j; nothing is read through an index before the index is checked.
__device__ __forceinline__ uint32_t sm_status(const SamArgs &a, uint32_t j, uint64_t n_rows)
{
    const uint32_t typ = a.sel[4 * (size_t)j], n_xa = a.sel[4 * (size_t)j + 3];
    if (typ == 0u) return HSA_SAM_NOHIT;
    const uint64_t r0 = a.pos_off[j], r1 = a.pos_off[j + 1], need = 1ull + n_xa;
    if (r0 > n_rows || need > n_rows - r0) return HSA_SAM_ROWS;
    const int32_t na = a.n_aln[j];
    if (typ > 2u || r1 < r0 || r1 - r0 < need || na <= 0) return HSA_SAM_INPUT;
    bool refused = false, bad = false;
    for (uint64_t t = r0; t < r0 + need; ++t) {
        const uint32_t *row = a.rows + HSA_RF_ROW_WORDS * t;
        if (row[0] != HSA_RF_OK) { refused = true; continue; }
        const uint32_t n_cigar = row[1];
        if (n_cigar > a.cigar_stride) bad = true;
        else
            for (uint32_t i = 0; i < n_cigar; ++i)
                if ((a.cigar[(size_t)a.cigar_stride * t + i] >> 28) > 8u) bad = true;
        if (row[3] > a.md_stride) bad = true;
        const uint64_t c = a.pos[4 * t + 1];
        if (c >= a.n_chr) bad = true;
        else if (a.chr_off[c + 1] < a.chr_off[c] || a.chr_off[c + 1] - a.chr_off[c] > a.max_line) bad = true;
        if (a.pos_hit[t] >= (uint32_t)na) bad = true;
    }
    if (refused) return HSA_SAM_REFINE;
    if (bad) return HSA_SAM_INPUT;
    const hsa_job_t jb = a.jobs[j];
    const uint32_t full = sm_full_len(a, j, jb.len);
    if (a.name_off[j + 1] < a.name_off[j] || a.name_off[j + 1] - a.name_off[j] > a.max_line || full > a.max_line || full < jb.len)
        return HSA_SAM_INPUT;                      // (lengths past max_line: no line can hold them)
    if (a.quals && (a.qual_off[j + 1] < a.qual_off[j] || a.qual_off[j + 1] - a.qual_off[j] != full)) return HSA_SAM_INPUT;
    return sm_bad_codes(a.codes + jb.off, full) ? HSA_SAM_INPUT : HSA_SAM_OK;
}

// The counters are summed per block first: a million lanes adding to one address take
// 11.8 ms (measured; profiles/sam_probe.json has the call after this change), a block's
// five sums and its minimum one atomic each.
__global__ void __launch_bounds__(256) k_sam_len(SamArgs a)
{
    __shared__ uint32_t sCnt[5], sLow;
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (threadIdx.x < 5u) sCnt[threadIdx.x] = 0u;
    if (threadIdx.x == 5u) sLow = 0xFFFFFFFFu;
    __syncthreads();
    uint64_t len = 0;
    if (j < a.n_jobs) {
        uint32_t st = sm_status(a, j, sm_n_rows(a));
        if (st == HSA_SAM_OK) {
            SmCount s;
            SmMark mk;
            sm_emit(a, j, s, mk);
            if (s.n > a.max_line) st = HSA_SAM_INPUT;
            else len = s.n;
        }
        a.stat[j] = st;
        atomicAdd(&sCnt[st], 1u);
        if (st >= HSA_SAM_ROWS) atomicMin(&sLow, j);
    }
    if (j <= a.n_jobs) a.lens[j] = len;
    __syncthreads();
    if (threadIdx.x < 5u && sCnt[threadIdx.x]) atomicAdd(&a.ctr[2u + threadIdx.x], (unsigned long long)sCnt[threadIdx.x]);
    if (threadIdx.x == 5u && sLow != 0xFFFFFFFFu) atomicMin(&a.ctr[7], (unsigned long long)sLow);
}

// Phase B of k_sam_write: a tile's marks in LDS, and 128 bytes of a read's name, SEQ and
// QUAL on their way (two bytes of each per lane).
struct SmTile {
    const uint64_t *name_src, *code_off, *qual_off;
    const uint32_t *name_dst, *name_len, *seq_dst, *qual_dst, *len, *strand;
    uint8_t *buf;
    uint32_t cap, lane;
};
struct SmChunk {
    uint32_t vna, vnb, ca, cb, qa, qb;
};

__device__ __forceinline__ SmChunk sm_chunk_load(const SamArgs &a, const SmTile &t, uint32_t r, uint32_t k0)
{
    const uint32_t nl = t.name_len[r], len = t.len[r];
    const bool rev = t.strand[r] != 0u;
    const uint8_t *name = a.names + t.name_src[r], *code = a.codes + t.code_off[r];
    const uint8_t *qual = a.quals ? a.quals + t.qual_off[r] : code;
    // (a lane without a byte loads one that exists, so that no load hides in a branch)
    const uint8_t *idle = reinterpret_cast<const uint8_t *>(a.stat);
    const uint32_t ka = k0 + t.lane, kb = ka + 64u;
    const uint32_t ia = rev ? len - 1u - ka : ka, ib = rev ? len - 1u - kb : kb;
    SmChunk c;
    c.vna = *(ka < nl ? name + ka : idle); c.vnb = *(kb < nl ? name + kb : idle);
    c.ca = *(ka < len ? code + ia : idle); c.cb = *(kb < len ? code + ib : idle);
    c.qa = *(ka < len ? qual + ia : idle); c.qb = *(kb < len ? qual + ib : idle);
    return c;
}

__device__ __forceinline__ void sm_chunk_store(const SmTile &t, uint32_t r, uint32_t k0, const SmChunk &c)
{
    const uint32_t nl = t.name_len[r], nd = t.name_dst[r], len = t.len[r], sd = t.seq_dst[r], qd = t.qual_dst[r];
    const uint64_t letters = t.strand[r] != 0u ? SM_REV : SM_FWD;
    const uint32_t ka = k0 + t.lane, kb = ka + 64u;
    const bool has_q = qd != 0xFFFFFFFFu;
    if (ka < nl && nd + ka < t.cap) t.buf[nd + ka] = (uint8_t)c.vna;
    if (kb < nl && nd + kb < t.cap) t.buf[nd + kb] = (uint8_t)c.vnb;
    if (ka < len && sd + ka < t.cap) t.buf[sd + ka] = (uint8_t)(letters >> (8u * (c.ca < 4u ? c.ca : 4u)));
    if (kb < len && sd + kb < t.cap) t.buf[sd + kb] = (uint8_t)(letters >> (8u * (c.cb < 4u ? c.cb : 4u)));
    if (has_q && ka < len && qd + ka < t.cap) t.buf[qd + ka] = (uint8_t)c.qa;
    if (has_q && kb < len && qd + kb < t.cap) t.buf[qd + kb] = (uint8_t)c.qb;
}

// the chunks after a read's first: only names and reads over 128 bytes have any
__device__ __forceinline__ void sm_chunk_rest(const SamArgs &a, const SmTile &t, uint32_t r)
{
    const uint32_t most = t.name_len[r] > t.len[r] ? t.name_len[r] : t.len[r];
    for (uint32_t k0 = 128u; k0 < most; k0 += 128u) sm_chunk_store(t, r, k0, sm_chunk_load(a, t, r, k0));
}

extern __shared__ __attribute__((aligned(16))) uint4 sm_dyn[];

__global__ void __launch_bounds__(64) k_sam_write(SamArgs a)
{
    __shared__ uint64_t sNameSrc[SM_TILE_MAX], sCodeOff[SM_TILE_MAX], sQualOff[SM_TILE_MAX];
    __shared__ uint32_t sNameDst[SM_TILE_MAX], sNameLen[SM_TILE_MAX], sSeqDst[SM_TILE_MAX], sQualDst[SM_TILE_MAX],
        sLen[SM_TILE_MAX], sStrand[SM_TILE_MAX];
    uint8_t *buf = reinterpret_cast<uint8_t *>(sm_dyn);
    const uint32_t lane = threadIdx.x;
    const uint64_t total = a.line_off[a.n_jobs];
    if (blockIdx.x == 0 && lane == 0) {
        a.ctr[0] = total;
        a.ctr[1] = total < a.out_cap ? total : a.out_cap;
    }
    const uint64_t j0 = (uint64_t)blockIdx.x * a.tile;
    if (j0 >= a.n_jobs) return;                                         // (the whole block: n_jobs == 0)
    const uint32_t cnt = a.n_jobs - j0 < a.tile ? (uint32_t)(a.n_jobs - j0) : a.tile;
    const uint64_t base = a.line_off[j0], end = a.line_off[j0 + cnt];
    const uint64_t lim = end < a.out_cap ? end : a.out_cap;
    if (lim <= base) return;                                            // (the whole block: nothing of it fits)
    uint8_t *g = a.out + base;
    const uint32_t pad = (uint32_t)(reinterpret_cast<uintptr_t>(g) & 15u);
    // A: lane r, read j0 + r
    if (lane < cnt) {
        const uint32_t j = (uint32_t)j0 + lane;
        SmMark mk;
        mk.name_len = 0; mk.len = 0;
        mk.name_src = mk.code_off = mk.qual_off = 0;
        mk.name_dst = mk.seq_dst = mk.qual_dst = mk.strand = 0;
        if (a.stat[j] == HSA_SAM_OK) {
            SmStore s{buf, pad + (uint32_t)(a.line_off[j] - base), a.lds_text};
            sm_emit(a, j, s, mk);
        }
        sNameSrc[lane] = mk.name_src; sCodeOff[lane] = mk.code_off; sQualOff[lane] = mk.qual_off;
        sNameDst[lane] = mk.name_dst; sNameLen[lane] = mk.name_len; sSeqDst[lane] = mk.seq_dst;
        sQualDst[lane] = mk.qual_dst; sLen[lane] = mk.len; sStrand[lane] = mk.strand;
    }
    __syncthreads();
    // B: lanes along the bytes of name, SEQ and QUAL, 128 bytes of each per chunk.  The
    // chunks of a read and the reads of a tile are the same in every lane; a chunk's six
    // loads are issued together, and the first chunk of the next read before the stores of
    // this one, so that a read's stores wait for loads one read old
    SmTile tl{sNameSrc, sCodeOff, sQualOff, sNameDst, sNameLen, sSeqDst, sQualDst, sLen, sStrand, buf, a.lds_text, lane};
    // (two reads per trip, each with its own registers: a copy of the chunk from one trip
    // to the next would wait for the loads at once)
    const uint32_t last = cnt - 1u;
    SmChunk even = sm_chunk_load(a, tl, 0u, 0u);
    for (uint32_t r = 0; r < cnt; r += 2u) {
        const SmChunk odd = sm_chunk_load(a, tl, r + 1u < last ? r + 1u : last, 0u);
        __builtin_amdgcn_sched_barrier(0);         // (keeps the loads above in front of the waits below)
        sm_chunk_store(tl, r, 0u, even);
        sm_chunk_rest(a, tl, r);
        even = sm_chunk_load(a, tl, r + 2u < last ? r + 2u : last, 0u);
        __builtin_amdgcn_sched_barrier(0);
        if (r + 1u < cnt) {
            sm_chunk_store(tl, r + 1u, 0u, odd);
            sm_chunk_rest(a, tl, r + 1u);
        }
    }
    __syncthreads();
    // C: the range leaves; only whole 16-byte units of the output go as 16-byte stores
    const uint32_t cap = a.lds_text;
    uint32_t n = (uint32_t)(lim - base);
    if (n > cap - pad) n = cap - pad;                                   // (never: every line is <= max_line)
    const uint32_t head = ((16u - pad) & 15u) < n ? (16u - pad) & 15u : n;
    const uint32_t units = (n - head) >> 4, tail = head + (units << 4);
    for (uint32_t k = lane; k < head; k += 64u) g[k] = buf[pad + k];
    const uint4 *src = reinterpret_cast<const uint4 *>(buf + pad + head);
    uint4 *dst = reinterpret_cast<uint4 *>(g + head);
    if (units)
        for (uint32_t u = lane; u < units; u += 64u) dst[u] = src[u];
    for (uint32_t k = tail + lane; k < n; k += 64u) g[k] = buf[pad + k];
}

static int g_sam_timing = 0;

extern "C" void hsa_sam_timing(int on) { g_sam_timing = on; }

extern "C" int hsa_sam_launch_times(hsa_index_t *ix, float *ms) { return hsa_stage_times(ix, &hsa_index::sm_t, ms, "hsa_sam"); }

extern "C" int hsa_sam_lines_device64(hsa_index_t *ix, const hsa_sam_batch64_t *b, void *stream)
{
    return hsa_sam_lines_device64_trim(ix, b, nullptr, stream);
}

extern "C" int hsa_sam_lines_device64_trim(hsa_index_t *ix, const hsa_sam_batch64_t *b, const hsa_sam_trim_t *trim, void *stream)
{
    const char *what = "hsa_sam_lines_device64";
    if (!ix) {
        int nd = 0;
        if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) { hsa_set_error("%s: no HIP device visible", what); return HSA_E_NODEV; }
        hsa_set_error("%s: null handle", what);
        return HSA_E_ARG;
    }
    if (!ix->wide) { hsa_set_error("%s: not a 64-bit index (hsa_index_create_device64)", what); return HSA_E_ARG; }
    if (!b || b->n_jobs < 0 || !b->d_counters || !b->d_line_off || (b->out_cap && !b->d_out)) {
        hsa_set_error("%s: bad arguments", what);
        return HSA_E_ARG;
    }
    if (b->n_jobs && (!b->d_jobs || !b->d_codes || !b->d_n_aln || !b->d_hit_off || !b->d_hits || !b->d_sel || !b->d_sel64 ||
                      !b->d_pos_off || !b->d_pos || !b->d_pos_hit || !b->d_rows || !b->d_rpos || !b->d_name_off ||
                      !b->d_names || !b->d_line_stat || (b->cigar_stride && !b->d_cigar) || (b->md_stride && !b->d_md) ||
                      (b->n_chr && (!b->d_chr_names || !b->d_chr_off)))) {
        hsa_set_error("%s: null argument", what);
        return HSA_E_ARG;
    }
    if ((b->d_quals == nullptr) != (b->d_qual_off == nullptr)) {
        hsa_set_error("%s: d_quals and d_qual_off go together", what);
        return HSA_E_ARG;
    }
    if (trim && (trim->bc_len > HSA_SAM_MAX_BC || (trim->bc_len != 0u) != (trim->d_bc != nullptr))) {
        hsa_set_error("%s: a barcode of 1..%u bytes per read goes with d_bc", what, HSA_SAM_MAX_BC);
        return HSA_E_ARG;
    }
    if (b->max_line < 1u || b->max_line > HSA_SAM_MAX_LINE) {
        hsa_set_error("%s: max_line %u is not in 1..%u", what, b->max_line, HSA_SAM_MAX_LINE);
        return HSA_E_ARG;
    }
    const uint64_t n = (uint64_t)b->n_jobs;
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    size_t tmp_bytes = 0;
    HSA_TRY(hsa_scan_bytes(tmp_bytes, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
    SamArgs A;
    void *d_tmp = nullptr;
    auto layout = [&](Carver c) {
        A.lens = c.take<uint64_t>(n + 1);
        d_tmp = c.take<char>(tmp_bytes);
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_sm, &ix->d_sm_cap, layout(Carver())));
    layout(Carver(ix->d_sm));
    A.jobs = b->d_jobs; A.n_jobs = (uint32_t)n; A.codes = b->d_codes; A.n_aln = b->d_n_aln;
    A.hit_off = b->d_hit_off; A.hits = b->d_hits; A.sel = b->d_sel; A.sel64 = b->d_sel64;
    A.pos_off = b->d_pos_off; A.pos = b->d_pos; A.pos_hit = b->d_pos_hit; A.pos_cap = b->pos_cap;
    A.pos_ctr = b->d_pos_counters;
    A.rows = b->d_rows; A.rpos = b->d_rpos; A.cigar = b->d_cigar; A.md = b->d_md;
    A.cigar_stride = b->cigar_stride; A.md_stride = b->md_stride;
    A.names = b->d_names; A.name_off = b->d_name_off; A.quals = b->d_quals; A.qual_off = b->d_qual_off;
    A.chr_names = b->d_chr_names; A.chr_off = b->d_chr_off; A.n_chr = b->n_chr;
    A.flag = b->flag; A.max_top2 = b->max_top2; A.comp_read = b->comp_read;
    A.max_line = b->max_line;
    uint32_t tile = SM_TILE_BYTES / b->max_line;
    A.tile = tile < 1u ? 1u : (tile > SM_TILE_MAX ? SM_TILE_MAX : tile);
    A.lds_text = (A.tile * b->max_line + 16u + 15u) & ~15u;
    A.line_off = b->d_line_off; A.out = b->d_out; A.out_cap = b->out_cap; A.stat = b->d_line_stat;
    A.ctr = (unsigned long long *)b->d_counters;
    A.full_len = trim ? trim->d_full_len : nullptr; A.bc = trim ? trim->d_bc : nullptr; A.bc_len = trim ? trim->bc_len : 0u;
    StageTimer &tm = ix->sm_t;                 // records only when hsa_sam_timing asked for it
    HSA_TRY(tm.begin(g_sam_timing != 0));
    HSA_TRY(tm.mark(0, st));
    HSA_HIP(hipMemsetAsync(b->d_counters, 0, 7 * sizeof(uint64_t), st));
    HSA_HIP(hipMemsetAsync(b->d_counters + 7, 0xFF, sizeof(uint64_t), st));      // no refused read yet
    hipLaunchKernelGGL(k_sam_len, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(1, st));
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, A.lens, A.line_off, (uint64_t)0, (size_t)(n + 1),
                                    rocprim::plus<uint64_t>(), st));
    HSA_TRY(tm.mark(2, st));
    hipLaunchKernelGGL(k_sam_write, dim3(hsa_stage_blocks(n, A.tile)), dim3(64), A.lds_text, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(3, st));
    tm.end();
    return 0;
}
