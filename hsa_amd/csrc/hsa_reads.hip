// hsa_reads.hip -- FASTQ bytes to a search batch, on the device.
//
// The head of the reference's pipeline: bwa_read_seq (bwaseqio.c:161-231) over kseq_read
// (kseq.h:155-193), and the read filter and per-read options at the top of
// bwa_cal_sa_reg_gap (bwtaln.c:313-332).  hsa_reads_device takes the raw bytes of a FASTQ
// chunk in device memory and leaves d_jobs, d_codes, the names and the qualities in the
// layouts hsa_search_device64 and hsa_sam_lines_device64 take, and one row per record.
//
// The canonical record.  A read is answered exactly or not at all, so only records on which
// kseq_read provably consumes exactly four lines are parsed here:
//   line 0  '@', a non-empty name up to the first isspace byte (no NUL in it: the reference
//           keeps the name with strdup, bwaseqio.c:216), the rest of the line is the comment;
//   line 1  at least one byte, every byte isgraph and none of '>', '+', '@';
//   line 2  starts with '+';
//   line 3  as long as line 1, every byte in 33..127, ended by '\n' or, with at_eof, by the
//           end of the input.
// Why kseq_read consumes exactly these lines, given that it starts at the record's '@' with
// last_char == 0 (true at the start of a file and after every FASTQ record, kseq.h:190):
//   :161      the skip to the next '>' or '@' stops at once, on the '@';
//   :166-167  ks_getuntil(0) takes the name up to the first isspace byte; when that byte is
//             not '\n' the comment runs to the line's '\n' (the line holds no other '\n');
//   :168-177  the sequence loop stops at '>', '+', '@' or the end; line 1 holds none of them
//             and only isgraph bytes, so all of line 1 is appended, its '\n' is skipped (not
//             isgraph) and the loop stops on the '+' that starts line 2;
//   :185      the rest of the '+' line is skipped through its '\n';
//   :187-188  the quality loop reads a byte, then tests qual.l < seq.l: every byte of line 3
//             is in 33..127 and is stored, and with qual.l == seq.l one more byte -- the
//             '\n' that ends the line, or the end of the input -- is read and dropped;
//   :190-192  last_char = 0 and the lengths agree: the record is returned, and the next
//             call starts at the byte after that '\n': the next record's '@'.
// So in a run of canonical records record k is lines 4k .. 4k + 3, whatever byte a quality
// line starts with ('@' and '+' included): the record starts are found in parallel by
// counting newlines, and the question "is this '@' a header or a quality" never arises.
// Everything else -- a blank line, a sequence over several lines, CRLF ('\r' is not
// isgraph), FASTA, a quality of another length, an empty name, a read longer than
// HSA_RD_MAX_LEN or past the max_diff table -- is not canonical.  The first such record stops
// the load: the records before it are loaded, the counters give its index and byte offset,
// and the caller hands the bytes from there to a host parser (hsa_amd/reads.py: parse_host).
//
// Per canonical record, as the reference:
//   codes     nst_nt4_table (bwaseqio.c:10-27): ACGT in either case 0..3, '-' 5, others 4.
//             The table's value is stored; a 5 is not searched differently from a 4 (> 3),
//             and hsa_sam_lines_device64 refuses a read that holds one (HSA_SAM_INPUT, its
//             base-code check), as the reference would index "ACGTN"[5];
//   name      cut at the first isspace byte; a trailing "/1" or "/2" goes when the name is
//             longer than two bytes (bwaseqio.c:217-220);
//   quality   as given;
//   max_diff  opt->max_diff, or with fnr > 0 the entry of the caller's table of
//             bwa_cal_maxdiff(l) (bwtaln.c:330-331; the table is made on the host: no device
//             exp enters);
//   seed_len  opt->seed_len < len ? opt->seed_len : 0x7fffffff (bwtaln.c:332);
//   filter    more codes > 3 than the batch's threshold: not searched (bwtaln.c:314-317);
//             first 15 codes all A or all T: not searched (:324-325).  The threshold is
//             local_opt.max_diff before the option switch (:273-274): the table's entry of
//             the longest loaded read (or of len_floor, the longest read of the batch's
//             earlier chunks, when that is longer), or opt->max_diff.  For a read shorter than 15 bases
//             the reference's memcmp reads past its allocation; such a read is not poly-A/T
//             here, as the drop-in's host code decides (bwtaln_gpu.c:112, `len >= 15`).
//
// Launches, all on one stream, no host round trip, no atomics that place anything:
//   k_rd_count   one 16-byte load per lane, HSA_RD_TILE bytes per block: newlines per tile;
//   scan         exclusive, in byte order (rocPRIM): the first line number of every tile;
//   k_rd_lines   the same loads and a block scan: the start of every line up to 4 M + 1
//                (M = the most records the call can load);
//   k_rd_record  one wavefront per 16 consecutive records, lanes along the bytes of a record's
//                lines: validation, length, N count, poly test, name end, taken from wave-wide
//                ballots; lane 0 keeps the record's fields; the lowest non-canonical record
//                by atomicMin (a minimum: order-free);
//   k_rd_max     the longest loaded read (block maximum, one atomicMax per block);
//   k_rd_keep    status per record, the three lengths of a kept record for the scan;
//   scan         exclusive over (jobs, code bytes, name bytes) in record order: a kept
//                read's job index and offsets, so two runs give equal arrays;
//   k_rd_rows    one lane per record: its row, its job, its offsets; the counters;
//   k_rd_bytes   the three byte arrays: one wavefront per 16 consecutive records, lanes along
//                the bytes of a kept record's name, sequence and quality: a wave's load and
//                its store each cover 64 contiguous bytes.  No byte at or past a capacity is
//                touched.
// The loops of k_rd_record and k_rd_bytes run over a wavefront's records and over 64-byte
// chunks of one record: their trip counts, their breaks and the branches around the ballots
// depend on the record alone, which is the same in all 64 lanes, so no lane enters a region
// alone.  The other kernels' loops hold no barrier and no cross-lane operation.
//
// The reader's options (bwaseqio.c:176-211) come through hsa_reads_device_opts, the same code
// with k_rd_record and k_rd_bytes instantiated with OPT: the Casava filter (-Y), Illumina-1.3
// qualities (-I), barcodes (-B) and quality trimming (-q, bwa_trim_read as a wave-wide scan:
// rd_trim).  A trimmed read keeps its bytes: hsa_job_t.len is the trimmed length, d_full_len
// the stored one.  With a filter one more scan (the records the reader keeps) and k_rd_limit
// end the load behind the max_records-th kept record.  hsa_reads_device refuses the options
// (HSA_E_ARG) and then runs the same code.  BAM input (-b) is hsa_bam_reads_device's
// (hsa_bam.hip); both calls here refuse its mode bits.
#include <algorithm>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <string.h>

#include "hsa_internal.h"
#include "hsa_rd_wave.h"
#include "hsa_rd_tail.h"

#define RD_ONES32 0xFFFFFFFFu
#define RD_RT 16u                      // records per wavefront of k_rd_record and k_rd_bytes
#define RD_REFUSED_MODE 0xFF0003E8u   // barcode length, IL13, BAM*, CFY (bwtaln.h:122-131): hsa_reads_device takes none
#define RD_MODE_CFY 0x08u             // bwtaln.h:125
#define RD_MODE_IL13 0x200u           // :131
#define RD_MODE_BAM 0x1E0u            // :127-130: hsa_bam_reads_device
#define RD_MAX_BCLEN 63u              // BWA_MAX_BCLEN, bwtaln.h:28
// bwa_trim_read's sum: a byte of 33..127, 31 off with IL13, gives q - 33 in -31..94, so a
// step adds between trim_qual - 94 and trim_qual + 31 and |s| <= HSA_RD_MAX_LEN * (trim_qual + 94)
#define RD_MAX_TRIM ((int32_t)(0x7FFFFFFFu / HSA_RD_MAX_LEN) - 94)

struct RdArgs {
    const uint8_t *in;
    uint32_t n, lead, ntiles, M, ls_last;      // lead: bytes between the aligned base and in
    int32_t at_eof, max_diff, seed_len, regime;
    const int32_t *maxdiff;
    uint32_t n_maxdiff, len_floor;
    hsa_job_t *jobs; uint64_t job_cap;
    uint8_t *codes; uint64_t code_cap;
    uint8_t *names; uint64_t name_cap; uint64_t *name_off;
    uint8_t *quals; uint64_t qual_cap; uint64_t *qual_off;
    uint32_t *rec;
    unsigned long long *ctr;
    // scratch
    uint32_t *tile_cnt, *tile_base, *ls, *g;   // g: [0] first non-canonical record, [1] longest loaded, [2] longest kept
    uint32_t *r_len, *r_nn, *r_fl, *r_name_len;
    Rd3 *s_in, *s_out;
    // the reader's options (hsa_reads_device_opts); all zero / null without them
    int32_t trim_qual;                         // bwa_trim_read's, or 0
    uint32_t qshift, bc_len, casava, max_rec;  // 31 with IL13; mode >> 24; the CFY bit; max_records
    uint32_t *full_len; uint8_t *bc;           // per job: the length before trimming, the barcode
    unsigned long long *octr;
    uint32_t *r_full, *unf, *unf_scan;         // scratch: full length; 1 for a record the reader keeps, and its scan
};

// The newlines among the 16 bytes at the aligned address of unit u, as a bit mask; bytes
// outside [0, n) of the input are left out.  b0: the input offset of the unit's byte 0
__device__ __forceinline__ uint32_t rd_nl_mask(const RdArgs &a, uint64_t u, int64_t &b0)
{
    b0 = (int64_t)(16u * u) - (int64_t)a.lead;
    if (b0 + 16 <= 0 || b0 >= (int64_t)a.n) return 0u;
    const uint4 w = *reinterpret_cast<const uint4 *>(a.in - a.lead + 16u * u);
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = ws[q] ^ 0x0A0A0A0Au;
        const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);    // 0x80 in every zero byte, exact
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * q);
    }
    const uint32_t lo = b0 < 0 ? (uint32_t)(-b0) : 0u;
    const int64_t left = (int64_t)a.n - b0;
    const uint32_t hi = left < 16 ? (uint32_t)left : 16u;
    return m & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

__global__ void __launch_bounds__(256) k_rd_count(RdArgs a)
{
    using Reduce = rocprim::block_reduce<uint32_t, 256>;
    __shared__ typename Reduce::storage_type tmp;
    int64_t b0;
    uint32_t c = __popc(rd_nl_mask(a, (uint64_t)blockIdx.x * 256u + threadIdx.x, b0));
    uint32_t sum = 0;
    Reduce().reduce(c, sum, tmp);
    if (threadIdx.x == 0) a.tile_cnt[blockIdx.x] = sum;
}

// What the newline count says of the input: the records whose four lines are there and
// ended (cand, at most M), and whether lines of one more record follow them at the end of
// the input (with at_eof: a non-canonical record cand)
struct RdShape {
    uint32_t cand;
    bool tail_bad;
};
__device__ __forceinline__ RdShape rd_shape(const RdArgs &a)
{
    const uint32_t nl = a.tile_base[a.ntiles];
    const bool term = a.n == 0u || a.in[a.n - 1u] == (uint8_t)'\n';
    const uint64_t lines = (uint64_t)nl + (term ? 0u : 1u);
    uint64_t full = lines / 4u;
    const uint32_t rem = (uint32_t)(lines % 4u);
    if (!term && rem == 0u && !a.at_eof) full -= 1u;       // the last quality line may go on in the next chunk
    RdShape s;
    s.tail_bad = a.at_eof && rem != 0u && full < a.M;
    s.cand = full < a.M ? (uint32_t)full : a.M;
    return s;
}
// (g[3]: the record after the max_records-th one the reader keeps, k_rd_limit; all-ones without a filter)
__device__ __forceinline__ uint32_t rd_loaded(const RdArgs &a, const RdShape &s)
{
    const uint32_t n = a.g[0] < s.cand ? a.g[0] : s.cand;
    return a.g[3] < n ? a.g[3] : n;
}

__global__ void __launch_bounds__(256) k_rd_lines(RdArgs a)
{
    using Scan = rocprim::block_scan<uint32_t, 256>;
    __shared__ typename Scan::storage_type tmp;
    int64_t b0;
    const uint32_t m = blockIdx.x < a.ntiles ? rd_nl_mask(a, (uint64_t)blockIdx.x * 256u + threadIdx.x, b0) : 0u;
    uint32_t before = 0;
    Scan().exclusive_scan((uint32_t)__popc(m), before, 0u, tmp);
    uint64_t g = (uint64_t)(blockIdx.x < a.ntiles ? a.tile_base[blockIdx.x] : 0u) + before;     // newlines before this unit
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i)
        if ((m >> i) & 1u) {
            ++g;                                            // line g starts after newline g
            if (g <= a.ls_last) a.ls[g] = (uint32_t)(b0 + i) + 1u;
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ls[0] = 0u;
        const uint32_t nl = a.tile_base[a.ntiles];
        // a last line without '\n' ends at n: the start of the line "after" it is n + 1
        if (a.n && a.in[a.n - 1u] != (uint8_t)'\n' && (uint64_t)nl + 1u <= a.ls_last) a.ls[nl + 1u] = a.n + 1u;
    }
}

__device__ __forceinline__ bool rd_space(uint32_t c) { return c == 32u || (c >= 9u && c <= 13u); }
// nst_nt4_table (bwaseqio.c:10-27)
__device__ __forceinline__ uint32_t rd_code(uint32_t c)
{
    const uint32_t l = c | 0x20u;
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : c == '-' ? 5u : 4u;
}

// The Casava filter (bwaseqio.c:176-181) on a comment of n bytes: it is a C string, so a NUL
// before the first ':' ends the search; the byte after that ':' must be 'Y'.  Called by the
// whole wave with the same c and n.
__device__ __forceinline__ bool rd_casava(const uint8_t *c, uint32_t n, uint32_t lane)
{
    for (uint32_t p0 = 0; p0 < n; p0 += 64u) {
        const uint32_t p = p0 + lane;
        const uint32_t b = p < n ? c[p] : 1u;
        const unsigned long long colon = __ballot(b == (uint32_t)':'), nul = __ballot(b == 0u);
        if (colon | nul) {
            const uint32_t first = (uint32_t)__ffsll((long long)(colon | nul)) - 1u;
            const uint32_t at = p0 + first + 1u;
            return ((colon >> first) & 1ull) && at < n && c[at] == (uint8_t)'Y';
        }
    }
    return false;
}

// bwa_trim_read (bwaseqio.c:92-103) on the quality bytes q[0, len), qshift taken off each:
// the length the read keeps (rd_trim_walk, hsa_rd_wave.h, which the BAM loader shares).
// |s| <= len * (trim_qual + 94) fits int32 for trim_qual <= RD_MAX_TRIM.
__device__ __forceinline__ uint32_t rd_trim(const uint8_t *q, uint32_t len, int32_t trim_qual, uint32_t qshift, uint32_t lane)
{
    return rd_trim_walk([=](uint32_t l) { return (int32_t)q[l] - (int32_t)qshift - 33; }, len, trim_qual, lane);
}

// One wavefront per RD_RT consecutive records, the lanes along the bytes of a record's
// lines: consecutive lanes load consecutive bytes, and what a record's decisions need of
// them (a byte that is not allowed, the first white space of the header, the codes above 3,
// the first 15 codes) comes back as wave-wide ballots.  The record, and so every trip
// count and every branch around a ballot, is the same in all 64 lanes.
//
// OPT: the reader's options, in bwa_read_seq's order (bwaseqio.c:176-211): the Casava filter
// on the comment; the barcode off the front of lines 1 and 3 (a read not longer than it is
// filtered); bwa_trim_read on the shifted quality; then the codes above 3 and the poly test
// over the trimmed read, the only length the search sees.  Lines 1 and 3 are validated whole
// and raw first.  Without OPT none of that code is in the kernel.
template <bool OPT> __global__ void __launch_bounds__(64) k_rd_record(RdArgs a)
{
    const uint32_t lane = threadIdx.x;
    const RdShape sh = rd_shape(a);
    if (blockIdx.x == 0 && lane == 0u && sh.tail_bad) atomicMin(&a.g[0], sh.cand);
    const uint8_t *in = a.in;
    for (uint32_t r = 0; r < RD_RT; ++r) {
        const uint32_t k = blockIdx.x * RD_RT + r;
        if (k >= sh.cand) break;                            // (the whole wave)
        const uint32_t s0 = a.ls[4u * k], s1 = a.ls[4u * k + 1u], s2 = a.ls[4u * k + 2u], s3 = a.ls[4u * k + 3u], s4 = a.ls[4u * k + 4u];
        const uint32_t e0 = s1 - 1u, e1 = s2 - 1u, e2 = s3 - 1u, e3 = s4 - 1u;
        bool bad = false;
        uint32_t name_len = 0, len = e1 - s1, nn = 0, poly = 0;
        uint32_t full = len, filtered = 0;                  // (OPT: the length before trimming; a record the reader skips)
        // line 0
        if (e0 - s0 < 2u || in[s0] != (uint8_t)'@') bad = true;
        else {
            const uint32_t most = e0 - s0 - 1u > HSA_RD_MAX_LEN ? HSA_RD_MAX_LEN + 1u : e0 - s0 - 1u;
            name_len = most;
            uint32_t comment = e0;                          // where the comment starts: behind the name's white space
            for (uint32_t p0 = 0; p0 < most; p0 += 64u) {
                const uint32_t p = p0 + lane;
                const uint32_t c = p < most ? in[s0 + 1u + p] : 1u;              // (1: neither white space nor NUL)
                const unsigned long long sp = __ballot(rd_space(c)), nul = __ballot(c == 0u);
                if (sp) {
                    const uint32_t first = (uint32_t)__ffsll((long long)sp) - 1u;
                    if (nul & ((1ull << first) - 1ull)) bad = true;
                    name_len = p0 + first;
                    comment = s0 + 2u + name_len;
                    break;
                }
                if (nul) bad = true;
            }
            if constexpr (OPT)
                if (a.casava && comment < e0 && rd_casava(in + comment, e0 - comment, lane)) filtered = 1u;
            if (name_len == 0u || name_len > HSA_RD_MAX_LEN) bad = true;
            else if (name_len > 2u && in[s0 + name_len - 1u] == (uint8_t)'/' &&
                     (in[s0 + name_len] == (uint8_t)'1' || in[s0 + name_len] == (uint8_t)'2'))
                name_len -= 2u;                             // bwaseqio.c:217-220
        }
        // lines 1 and 3
        if (len < 1u || len > HSA_RD_MAX_LEN || e3 - s3 != len || (a.maxdiff && len >= a.n_maxdiff)) bad = true;
        else if constexpr (OPT) {
            for (uint32_t p0 = 0; p0 < len; p0 += 64u) {    // both lines whole, as given
                const uint32_t p = p0 + lane;
                const uint32_t c = p < len ? in[s1 + p] : (uint32_t)'A', q = p < len ? in[s3 + p] : (uint32_t)'I';
                if (__ballot(c < 33u || c > 126u || c == '>' || c == '+' || c == '@' || q < 33u || q > 127u)) bad = true;
            }
            if (len <= a.bc_len) filtered = 1u;             // bwaseqio.c:185
            else if (!bad) {
                const uint32_t c1 = s1 + a.bc_len, c3 = s3 + a.bc_len;             // the read behind its barcode
                full = len - a.bc_len;
                len = a.trim_qual >= 1 ? rd_trim(in + c3, full, a.trim_qual, a.qshift, lane) : full;
                unsigned long long not_a = 0, not_t = 0;
                for (uint32_t p0 = 0; p0 < len; p0 += 64u) {
                    const uint32_t p = p0 + lane;
                    const bool on = p < len;
                    const uint32_t code = rd_code(on ? in[c1 + p] : (uint32_t)'A');
                    nn += (uint32_t)__popcll(__ballot(on && code > 3u));
                    if (p0 == 0u) {
                        not_a = __ballot(lane < 15u && (!on || code != 0u));
                        not_t = __ballot(lane < 15u && (!on || code != 3u));
                    }
                }
                poly = len >= 15u && (not_a == 0ull || not_t == 0ull);
            }
        } else {
            unsigned long long not_a = 0, not_t = 0;
            for (uint32_t p0 = 0; p0 < len; p0 += 64u) {
                const uint32_t p = p0 + lane;
                const bool on = p < len;
                const uint32_t c = on ? in[s1 + p] : (uint32_t)'A', q = on ? in[s3 + p] : (uint32_t)'I';
                const uint32_t code = rd_code(c);
                if (__ballot(c < 33u || c > 126u || c == '>' || c == '+' || c == '@' || q < 33u || q > 127u)) bad = true;
                nn += (uint32_t)__popcll(__ballot(on && code > 3u));
                if (p0 == 0u) {
                    not_a = __ballot(lane < 15u && (!on || code != 0u));
                    not_t = __ballot(lane < 15u && (!on || code != 3u));
                }
            }
            poly = len >= 15u && (not_a == 0ull || not_t == 0ull);   // (shorter: bwtaln_gpu.c:112)
        }
        // line 2
        if (e2 - s2 < 1u || in[s2] != (uint8_t)'+') bad = true;
        if (lane == 0u) {
            a.r_len[k] = len; a.r_nn[k] = nn; a.r_fl[k] = poly; a.r_name_len[k] = name_len;
            if constexpr (OPT) {
                a.r_full[k] = full;
                if (filtered) a.r_fl[k] = RD_FL_FILTERED;
                if (a.unf) a.unf[k] = filtered ? 0u : 1u;
            }
            if (bad) atomicMin(&a.g[0], k);
        }
    }
}

// With a filter (the Casava one, a barcode) the records the reader skips do not count
// towards max_records (bwaseqio.c:221 counts n_seqs): the load ends behind the record that is
// the max_records-th it keeps.  unf_scan is the exclusive scan of unf, so one lane at most
// finds its record to be that one.
__global__ void __launch_bounds__(256) k_rd_limit(RdArgs a)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < a.M && a.unf[k] && a.unf_scan[k] + 1u == a.max_rec) a.g[3] = k + 1u;
}

// The tail that does not depend on the format (hsa_rd_tail.h, shared with hsa_bam.hip)
__global__ void __launch_bounds__(256) k_rd_max(RdArgs a) { rd_tail_max(a, [&] { return rd_loaded(a, rd_shape(a)); }); }

__global__ void __launch_bounds__(256) k_rd_keep(RdArgs a) { rd_tail_keep(a, [&] { return rd_loaded(a, rd_shape(a)); }); }

__global__ void __launch_bounds__(256) k_rd_rows(RdArgs a)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const RdShape sh = rd_shape(a);
    const uint32_t loaded = rd_loaded(a, sh);
    const Rd3 tot = a.s_out[a.M];
    if (k < loaded) rd_tail_row(a, k);
    if (k == 0u) {
        if (tot.j <= a.job_cap) { a.name_off[tot.j] = tot.n; a.qual_off[tot.j] = tot.c; }
        const uint32_t bad = a.g[0];
        const bool has_bad = bad <= sh.cand && bad != RD_ONES32;
        const uint64_t first_left = 4ull * loaded;          // the first line not loaded
        const uint32_t nl = a.tile_base[a.ntiles];
        const bool term = a.n == 0u || a.in[a.n - 1u] == (uint8_t)'\n';
        const uint64_t lines = (uint64_t)nl + (term ? 0u : 1u);
        unsigned long long *c = a.ctr;
        const uint32_t read = a.unf ? a.unf_scan[loaded] : loaded;        // the records the reader did not skip
        c[0] = loaded + (has_bad ? 1u : 0u);
        c[1] = read;
        if (a.octr) { a.octr[0] = loaded; a.octr[1] = loaded - read; }
        c[2] = tot.j; c[3] = tot.j < a.job_cap ? tot.j : a.job_cap;
        c[4] = tot.c + 16u; c[5] = c[4] < a.code_cap ? c[4] : a.code_cap;
        c[6] = tot.n; c[7] = tot.n < a.name_cap ? tot.n : a.name_cap;
        c[8] = tot.c; c[9] = tot.c < a.qual_cap ? tot.c : a.qual_cap;
        c[10] = first_left < lines ? a.ls[first_left] : a.n;
        c[11] = has_bad ? bad : ~0ull;
        c[12] = has_bad ? c[10] : ~0ull;
        c[13] = a.g[1]; c[14] = a.g[2];
        c[15] = (unsigned long long)(long long)rd_threshold(a);
    }
}

// The three byte arrays: one wavefront per RD_RT consecutive records, the lanes along the
// bytes of a kept record's name, sequence and quality.  Consecutive lanes load consecutive
// input bytes and store consecutive output bytes (a wave's store covers 64 contiguous bytes
// of one array); a byte at or past its array's capacity is not stored.
//
// OPT: the read lies behind its barcode, its bytes are those of the whole read (trimming
// moves hsa_job_t.len alone), the quality loses qshift, and the barcode's bases go to d_bc at
// stride bc_len, in lower case where the shifted quality is under 13 (bwaseqio.c:188-190).
template <bool OPT> __global__ void __launch_bounds__(64) k_rd_bytes(RdArgs a)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t loaded = rd_loaded(a, rd_shape(a));
    const uint8_t *in = a.in;
    if (blockIdx.x == 0 && lane < 16u) {                    // the codes' zero padding (hsa_device_batch_t)
        const uint64_t at = a.s_out[a.M].c + lane;
        if (at < a.code_cap) a.codes[at] = 0u;
    }
    for (uint32_t r = 0; r < RD_RT; ++r) {
        const uint32_t k = blockIdx.x * RD_RT + r;
        if (k >= loaded) break;                             // (the whole wave)
        if (a.r_fl[k] != HSA_RD_SEARCHED) continue;
        const Rd3 at = a.s_out[k];
        const uint32_t len = OPT ? a.r_full[k] : a.r_len[k], nl = a.r_name_len[k];
        const uint32_t bcn = OPT ? a.bc_len : 0u, qshift = OPT ? a.qshift : 0u;
        const uint32_t s0 = a.ls[4u * k] + 1u, s1 = a.ls[4u * k + 1u] + bcn, s3 = a.ls[4u * k + 3u] + bcn;
        if constexpr (OPT)
            if (lane < bcn && at.j < a.job_cap) {           // (bc_len <= 63: one lane per base)
                const uint32_t c = in[s1 - bcn + lane], q = in[s3 - bcn + lane] - qshift;
                const bool low = (int32_t)q - 33 < 13;
                a.bc[at.j * bcn + lane] = (uint8_t)(low ? (c >= 'A' && c <= 'Z' ? c | 0x20u : c) : (c >= 'a' && c <= 'z' ? c & ~0x20u : c));
            }
        const uint32_t most = len > nl ? len : nl;
        for (uint32_t p0 = 0; p0 < most; p0 += 64u) {
            const uint32_t p = p0 + lane;
            // (a lane without a byte loads the field's first one, so that no load hides in a branch)
            const uint32_t c = in[s1 + (p < len ? p : 0u)], q = in[s3 + (p < len ? p : 0u)], m = in[s0 + (p < nl ? p : 0u)];
            if (p < len) {
                if (at.c + p < a.code_cap) a.codes[at.c + p] = (uint8_t)rd_code(c);
                if (at.c + p < a.qual_cap) a.quals[at.c + p] = (uint8_t)(q - qshift);
            }
            if (p < nl && at.n + p < a.name_cap) a.names[at.n + p] = (uint8_t)m;
        }
    }
}

static int g_rd_timing = 0;

extern "C" void hsa_reads_timing(int on) { g_rd_timing = on; }

extern "C" int hsa_reads_launch_times(hsa_index_t *ix, float *ms) { return hsa_stage_times(ix, &hsa_index::rd_t, ms, "hsa_reads"); }

extern "C" int hsa_reads_device(hsa_index_t *ix, const hsa_reads_batch_t *b, void *stream)
{
    if (ix && b && (b->trim_qual != 0 || (b->mode & RD_REFUSED_MODE))) {
        hsa_set_error("hsa_reads_device: quality trimming, barcodes, the Casava filter and Illumina-1.3 qualities are "
                      "hsa_reads_device_opts'; BAM input is hsa_bam_reads_device's");
        return HSA_E_ARG;
    }
    return hsa_reads_device_opts(ix, b, stream);
}

extern "C" int hsa_reads_device_opts(hsa_index_t *ix, const hsa_reads_batch_t *b, void *stream)
{
    const char *what = "hsa_reads_device_opts";
    if (!ix) {
        int nd = 0;
        if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) { hsa_set_error("%s: no HIP device visible", what); return HSA_E_NODEV; }
        hsa_set_error("%s: null handle", what);
        return HSA_E_ARG;
    }
    if (!b || !b->d_counters || !b->d_rec || !b->d_name_off || !b->d_qual_off || (b->n_in && !b->d_in) ||
        (b->job_cap && !b->d_jobs) || (b->code_cap && !b->d_codes) || (b->name_cap && !b->d_names) ||
        (b->qual_cap && !b->d_quals)) {
        hsa_set_error("%s: null argument", what);
        return HSA_E_ARG;
    }
    if (b->n_in >= 0xFFFFFF00ull || b->max_records < 1u || b->max_records > (1u << 28) || (b->at_eof != 0 && b->at_eof != 1) ||
        (b->d_maxdiff && b->len_floor >= b->n_maxdiff) || b->job_cap > (1ull << 32)) {
        hsa_set_error("%s: n_in under 2^32 - 256, max_records in 1..2^28, at_eof 0 or 1, len_floor inside the table", what);
        return HSA_E_ARG;
    }
    const uint32_t bc_len = b->mode >> 24;
    const bool filter = (b->mode & RD_MODE_CFY) != 0u || bc_len != 0u;
    const bool opt = filter || b->trim_qual >= 1 || (b->mode & RD_MODE_IL13) != 0u;
    if (b->mode & RD_MODE_BAM) {
        hsa_set_error("%s: BAM input is hsa_bam_reads_device's", what);
        return HSA_E_ARG;
    }
    if (b->trim_qual > RD_MAX_TRIM || bc_len > RD_MAX_BCLEN || b->rec_cap > (1u << 28)) {
        hsa_set_error("%s: trim_qual at most %d (the walk's sum stays in 32 bits), a barcode of at most %u bases, rec_cap at most 2^28",
                      what, RD_MAX_TRIM, RD_MAX_BCLEN);
        return HSA_E_ARG;
    }
    if ((b->trim_qual >= 1 && !b->d_full_len) || (bc_len && b->job_cap && !b->d_bc)) {
        hsa_set_error("%s: trimming needs d_full_len, a barcode d_bc", what);
        return HSA_E_ARG;
    }
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    RdArgs A{};
    A.in = b->d_in; A.n = (uint32_t)b->n_in;
    A.lead = b->n_in ? (uint32_t)(reinterpret_cast<uintptr_t>(b->d_in) & 15u) : 0u;
    A.ntiles = (uint32_t)(((uint64_t)A.lead + A.n + HSA_RD_TILE - 1u) / HSA_RD_TILE);
    const uint64_t most = b->n_in / 8u + 1u;                // (the shortest record has 8 bytes)
    // (with a filter the rows of d_rec bound the records looked at, and max_records those the reader keeps)
    const uint32_t rows = filter && b->rec_cap ? b->rec_cap : b->max_records;
    A.M = (uint32_t)(most < rows ? most : rows);
    A.ls_last = 4u * A.M + 1u;
    A.at_eof = b->at_eof; A.max_diff = b->max_diff; A.seed_len = b->seed_len; A.regime = b->regime;
    A.maxdiff = b->d_maxdiff; A.n_maxdiff = b->n_maxdiff; A.len_floor = b->len_floor;
    A.jobs = b->d_jobs; A.job_cap = b->job_cap; A.codes = b->d_codes; A.code_cap = b->code_cap;
    A.names = b->d_names; A.name_cap = b->name_cap; A.name_off = b->d_name_off;
    A.quals = b->d_quals; A.qual_cap = b->qual_cap; A.qual_off = b->d_qual_off;
    A.rec = b->d_rec; A.ctr = (unsigned long long *)b->d_counters;
    A.trim_qual = b->trim_qual >= 1 ? b->trim_qual : 0; A.qshift = (b->mode & RD_MODE_IL13) ? 31u : 0u;
    A.bc_len = bc_len; A.casava = b->mode & RD_MODE_CFY; A.max_rec = b->max_records;
    A.full_len = b->d_full_len; A.bc = b->d_bc; A.octr = (unsigned long long *)b->d_opt_counters;
    size_t tmp1 = 0, tmp2 = 0, tmp3 = 0;
    if (filter) HSA_TRY(hsa_scan_bytes(tmp3, 0u, (size_t)A.M + 1, rocprim::plus<uint32_t>(), st));
    HSA_TRY(hsa_scan_bytes(tmp1, 0u, (size_t)A.ntiles + 1, rocprim::plus<uint32_t>(), st));
    HSA_TRY(hsa_scan_bytes(tmp2, Rd3{0, 0, 0}, (size_t)A.M + 1, Rd3Plus(), st));
    void *d_tmp = nullptr;
    auto layout = [&](Carver c) {
        A.g = c.take<uint32_t>(64);
        A.tile_cnt = c.take<uint32_t>((size_t)A.ntiles + 1);
        A.tile_base = c.take<uint32_t>((size_t)A.ntiles + 1);
        A.ls = c.take<uint32_t>((size_t)A.ls_last + 1);
        A.r_len = c.take<uint32_t>(A.M);
        A.r_nn = c.take<uint32_t>(A.M);
        A.r_fl = c.take<uint32_t>(A.M);
        A.r_name_len = c.take<uint32_t>(A.M);
        A.s_in = c.take<Rd3>((size_t)A.M + 1);
        A.s_out = c.take<Rd3>((size_t)A.M + 1);
        if (opt) A.r_full = c.take<uint32_t>(A.M);
        if (filter) {
            A.unf = c.take<uint32_t>((size_t)A.M + 1);
            A.unf_scan = c.take<uint32_t>((size_t)A.M + 1);
        }
        d_tmp = c.take<char>(std::max(tmp1, std::max(tmp2, tmp3)));
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_rd, &ix->d_rd_cap, layout(Carver())));
    layout(Carver(ix->d_rd));
    StageTimer &tm = ix->rd_t;                 // records only when hsa_reads_timing asked for it
    HSA_TRY(tm.begin(g_rd_timing != 0));
    HSA_TRY(tm.mark(0, st));
    HSA_HIP(hipMemsetAsync(A.g, 0xFF, 4, st));               // no non-canonical record yet
    HSA_HIP(hipMemsetAsync(A.g + 1, 0, 28, st));
    HSA_HIP(hipMemsetAsync(A.g + 3, 0xFF, 4, st));           // no limit by the records the reader keeps
    if (filter) HSA_HIP(hipMemsetAsync(A.unf, 0, ((size_t)A.M + 1) * 4, st));
    if (A.octr) HSA_HIP(hipMemsetAsync(A.octr, 0, HSA_RD_OPT_COUNTERS * sizeof(uint64_t), st));
    HSA_HIP(hipMemsetAsync(A.tile_cnt + A.ntiles, 0, 4, st));
    // (a line start the input does not reach is never read; zeroed so that no run depends on an earlier one)
    HSA_HIP(hipMemsetAsync(A.ls, 0, ((size_t)A.ls_last + 1) * 4, st));
    if (A.ntiles) {
        hipLaunchKernelGGL(k_rd_count, dim3(A.ntiles), dim3(256), 0, st, A);
        HSA_HIP(hipGetLastError());
    }
    HSA_TRY(tm.mark(1, st));
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp1, A.tile_cnt, A.tile_base, 0u, (size_t)A.ntiles + 1, rocprim::plus<uint32_t>(), st));
    HSA_TRY(tm.mark(2, st));
    hipLaunchKernelGGL(k_rd_lines, dim3(A.ntiles ? A.ntiles : 1u), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(3, st));
    const unsigned rb = (A.M + 1u + 255u) / 256u, wb = (A.M + RD_RT - 1u) / RD_RT;
    if (opt) hipLaunchKernelGGL(k_rd_record<true>, dim3(wb), dim3(64), 0, st, A);
    else hipLaunchKernelGGL(k_rd_record<false>, dim3(wb), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(4, st));
    if (filter) {
        HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp3, A.unf, A.unf_scan, 0u, (size_t)A.M + 1, rocprim::plus<uint32_t>(), st));
        hipLaunchKernelGGL(k_rd_limit, dim3(rb), dim3(256), 0, st, A);
        HSA_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rd_max, dim3(rb), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rd_keep, dim3(rb), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(5, st));
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp2, A.s_in, A.s_out, Rd3{0, 0, 0}, (size_t)A.M + 1, Rd3Plus(), st));
    HSA_TRY(tm.mark(6, st));
    hipLaunchKernelGGL(k_rd_rows, dim3(rb), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(7, st));
    if (opt) hipLaunchKernelGGL(k_rd_bytes<true>, dim3(wb), dim3(64), 0, st, A);
    else hipLaunchKernelGGL(k_rd_bytes<false>, dim3(wb), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(8, st));
    tm.end();
    return 0;
}
