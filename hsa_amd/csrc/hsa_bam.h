// hsa_bam.h -- the serial core of the BAM loader (hsa_bam.hip): the hop check that takes a
// walk from one record to the next, the offsets of a record's fields, and a base and a
// quality of the read in its own orientation.  Plain C++ that compiles for the host and the
// device: tests/san/bam_main.cpp runs it under AddressSanitizer on heap blocks of exact size
// before a corrupt byte reaches a GPU.
//
// A BAM record (SAM specification, section 4.2) is block_size (u32, little-endian) and then
// block_size bytes: refID, pos (i32 each), l_read_name (u8), mapq (u8), bin (u16), n_cigar_op
// (u16), flag (u16), l_seq (u32), next_refID, next_pos, tlen (i32 each): 36 fixed bytes with
// block_size; then the name (l_read_name bytes, NUL-terminated), the CIGAR (4 n_cigar_op
// bytes), the bases (two per byte, the first in the high nibble), the qualities (l_seq bytes)
// and the auxiliary fields up to the record's end.
//
// Every byte is read through `get(offset)`, offset counted from the start of the text; no
// function here asks for an offset at or past `n`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BAM_FN __host__ __device__ __forceinline__
#else
#define BAM_FN static inline
#endif

#define BAM_HOP_OK 0u           // a whole, consistent record
#define BAM_HOP_INCOMPLETE 1u   // the fixed bytes or the record's end lie past the text
#define BAM_HOP_MALFORMED 2u    // l_read_name == 0, or block_size under what its fields need
#define BAM_FIXED 36u           // block_size and the 32 bytes of the core
#define BAM_FLAG_REVERSE 0x10u
#define BAM_FLAG_READ1 0x40u
#define BAM_FLAG_READ2 0x80u

struct BamRec {
    uint32_t block_size, l_read_name, n_cigar, flag, l_seq;
    uint64_t name, cigar, seq, qual, end;      // offsets in the text; end: the next record's start
};

template <class G> BAM_FN uint32_t bam_u16(G get, uint64_t at) { return (uint32_t)get(at) | ((uint32_t)get(at + 1u) << 8); }
template <class G> BAM_FN uint32_t bam_u32(G get, uint64_t at) { return bam_u16(get, at) | (bam_u16(get, at + 2u) << 16); }

// The record at `pos` of a text of n bytes.  Only the bytes [pos, pos + 24) are read, and only
// when they lie inside the text.  OK means: l_read_name >= 1,
// block_size >= 32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq, and the record ends
// inside the text; then every field offset is inside the record and end >= pos + 37.
template <class G> BAM_FN uint32_t bam_hop(G get, uint64_t pos, uint64_t n, BamRec &r)
{
    if (pos > n || n - pos < 24u) return BAM_HOP_INCOMPLETE;
    r.block_size = bam_u32(get, pos);
    r.l_read_name = (uint32_t)get(pos + 12u);
    r.n_cigar = bam_u16(get, pos + 16u);
    r.flag = bam_u16(get, pos + 18u);
    r.l_seq = bam_u32(get, pos + 20u);
    const uint64_t need = 32ull + r.l_read_name + 4ull * r.n_cigar + ((uint64_t)r.l_seq + 1u) / 2u + r.l_seq;
    if (r.l_read_name == 0u || (uint64_t)r.block_size < need) return BAM_HOP_MALFORMED;
    if (n - pos < 4ull + r.block_size) return BAM_HOP_INCOMPLETE;
    r.name = pos + BAM_FIXED;
    r.cigar = r.name + r.l_read_name;
    r.seq = r.cigar + 4ull * r.n_cigar;
    r.qual = r.seq + ((uint64_t)r.l_seq + 1u) / 2u;
    r.end = pos + 4ull + r.block_size;
    return BAM_HOP_OK;
}

// bwtaln.c:441-447, bwaseqio.c:118-121: which & 1 takes FLAG 0x40, which & 2 FLAG 0x80,
// which & 4 a record with neither.  Nothing else in FLAG filters.
BAM_FN bool bam_selected(uint32_t which, uint32_t flag)
{
    const bool r1 = (flag & BAM_FLAG_READ1) != 0u, r2 = (flag & BAM_FLAG_READ2) != 0u;
    return ((which & 1u) && r1) || ((which & 2u) && r2) || ((which & 4u) && !r1 && !r2);
}

// bam_nt16_nt4_table (bwaseqio.c:29): 1, 2, 4, 8 are A, C, G, T
BAM_FN uint32_t bam_nt4(uint32_t nib) { return nib == 1u ? 0u : nib == 2u ? 1u : nib == 4u ? 2u : nib == 8u ? 3u : 4u; }
// bwaseqio.c:133
BAM_FN uint32_t bam_qual33(uint32_t q) { return q + 33u < 126u ? q + 33u : 126u; }

// Base p and quality p of the read as bwa_read_bam leaves them before line 142: with FLAG
// 0x10 the codes reverse-complemented and the qualities reversed (bwaseqio.c:135-138).
// p < l_seq.  `byte`: the stored byte at bam_code_at / bam_qual_at.
BAM_FN uint64_t bam_code_at(const BamRec &r, uint32_t p) { return r.seq + (((r.flag & BAM_FLAG_REVERSE) ? r.l_seq - 1u - p : p) >> 1); }
BAM_FN uint64_t bam_qual_at(const BamRec &r, uint32_t p) { return r.qual + ((r.flag & BAM_FLAG_REVERSE) ? r.l_seq - 1u - p : p); }
BAM_FN uint32_t bam_code(const BamRec &r, uint32_t p, uint32_t byte)
{
    const bool rev = (r.flag & BAM_FLAG_REVERSE) != 0u;
    const uint32_t i = rev ? r.l_seq - 1u - p : p;
    const uint32_t c = bam_nt4((i & 1u) ? (byte & 15u) : (byte >> 4));
    return rev && c < 4u ? 3u - c : c;
}
