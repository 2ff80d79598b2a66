// hsa_bam.hip -- inflated BAM bytes to a search batch, on the device.
//
// bwa_read_bam (bwaseqio.c:105-157) for the records of a BAM file whose bytes sit in device
// memory, with one departure.  Line 142 reverses p->seq "to be reversed back in
// bwa_refine_gapped"; that reverse-back is commented out in this reference (bwtse.c:545), as
// is the matching line of the FASTQ reader (bwaseqio.c:214), so the reference's -b searches
// every read backwards: a left-over, not a behaviour.  Here line 142 is not applied.  A BAM
// record then gives the bwa_seq_t the FASTQ reader gives for the equivalent FASTQ record, and
// the call leaves exactly hsa_reads_device_opts' outputs (hsa_reads.hip): the search, the
// choice, the refinement and the line writers run unchanged behind it.
//
// Per record, as the reference:
//   selection :118-121 by `which` and FLAG 0x40 / 0x80; nothing else in FLAG filters;
//   codes     bam_nt16_nt4_table (:29);  quality  q + 33 < 126 ? q + 33 : 126 (:133);
//   strand    with FLAG 0x10 the codes reverse-complemented, the qualities reversed (:135-138),
//             before the trimming (:139), the N count and the poly test look at them;
//   name      the l_read_name bytes up to the first NUL (strdup, :144); no "/1" is cut.
// A record that is not selected, and one with l_seq == 0, is no read: HSA_RD_FILTERED.
//
// Finding the records.  A record is block_size and that many bytes: the starts form a chain,
// which is serial.  The caller passes anchors, offsets at which it expects a record to start
// (htslib ends a BGZF member at a record boundary whenever the record fits, so for files it
// wrote every member's first byte is one); anchor 0 is offset 0, a true start.  Segment i is
// [anchor i, anchor i + 1).  k_bam_walk walks every segment on its own, one wavefront each:
// the wave stages BAM_WIN bytes in LDS with one round of 16-byte loads and hops inside them
// (a hop then waits for LDS, not for memory), staging again where a record's fixed bytes leave
// the window.  Every hop is checked before it is taken (bam_hop, hsa_bam.h): a walk that began
// inside a record reads garbage, but looks at no byte outside the text (the staging's aligned
// 16-byte units may reach up to 15 bytes past either end; those bytes are never looked at), and
// ends, since a hop advances by 37 bytes or more.  Segment i is verified when its walk lands exactly on anchor i + 1.
// Induction: anchor 0 is a true start, and a walk from a true start visits true starts only,
// so when segment i began at one and lands on anchor i + 1, segment i + 1 begins at one.  The
// records of the verified prefix are exact, and so are those of the first segment that is not
// verified (g[G_V], found as a minimum): it began at a true start and overshot its anchor
// because a record straddles it.  Everything behind is discarded.
//
// Launches, one stream, no host round trip, no atomic that places anything:
//   k_bam_walk    records, reads (selected, not empty), exit offset and status per segment;
//                 segment 0, whose records' indices need no scan, has its starts written here;
//   scan          exclusive over (records, reads) in segment order;
//   k_bam_starts  the walk again for segments 1 .. g[G_V]: every record's start and the
//                 reads before it; the record after the max_records-th read (one writer);
//   k_bam_record  one wavefront per 16 records, lanes along the bytes: name end, selection,
//                 the records for the host (lowest by atomicMin), bwa_trim_read from the
//                 read's own end, the codes above 3 and the poly test of the restored read;
//   k_bam_max, k_bam_keep, scan, k_bam_rows: the tail hsa_reads.hip has, stated once in
//   hsa_rd_tail.h (longest read, status per record, the scan's lengths, row and job); what is
//   here is what the format decides: the records loaded, the bytes consumed, why the load ended;
//   k_bam_bytes   as k_rd_bytes.  hsa_rd_wave.h: the wave-wide trim walk, shared too.
// The walk's other forms (hops that load from memory; one lane per segment) are kept behind
// hsa_bam_walk_mode for tools/bam_probe.py's A/B; DESIGN.md has the figures.
#include <algorithm>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <string.h>

#include "hsa_internal.h"
#include "hsa_bam.h"
#include "hsa_rd_wave.h"
#include "hsa_rd_tail.h"

#define BAM_ONES32 0xFFFFFFFFu
#define BAM_RT 16u                      // records per wavefront of k_bam_record and k_bam_bytes
#define BAM_WIN 4096u                   // bytes a walking wave stages in LDS: 4 x 16 per lane
#define BAM_MAX_TRIM ((int32_t)(0x7FFFFFFFu / HSA_RD_MAX_LEN) - 94)
#define BAM_FL_FILTERED RD_FL_FILTERED
#define BAM_FL_POLY 1u
#define BAM_ST_END 16u                  // a walk's status beside BAM_HOP_*: the anchor behind it is not where it landed
enum { G_BAD = 0, G_MAXL = 1, G_MAXK = 2, G_LIMIT = 3, G_V = 4, G_TOTAL = 5, G_END_ST = 6, G_WORDS = 64 };

struct Bam2 {
    uint32_t cnt, reads;
};
struct Bam2Plus {
    __host__ __device__ Bam2 operator()(const Bam2 &a, const Bam2 &b) const { return Bam2{a.cnt + b.cnt, a.reads + b.reads}; }
};
struct BamArgs {
    const uint8_t *in;
    uint32_t n, lead, M, nseg, which, max_rec;
    int32_t at_eof, max_diff, seed_len, regime, trim_qual;
    const int32_t *maxdiff;
    uint32_t n_maxdiff, len_floor;
    const uint64_t *anchor;
    hsa_job_t *jobs; uint64_t job_cap;
    uint8_t *codes; uint64_t code_cap;
    uint8_t *names; uint64_t name_cap; uint64_t *name_off;
    uint8_t *quals; uint64_t qual_cap; uint64_t *qual_off;
    uint32_t *full_len, *rec;
    unsigned long long *ctr, *octr, *bctr;
    // scratch
    uint32_t *g, *seg_exit, *seg_st, *rs, *kord;     // rs, kord: M + 2 entries
    Bam2 *seg_in, *seg_out;
    uint32_t *r_len, *r_nn, *r_fl, *r_name_len, *r_full;
    Rd3 *s_in, *s_out;
};

struct GlobalBytes {
    const uint8_t *in;
    __device__ __forceinline__ uint32_t operator()(uint64_t o) const { return in[o]; }
};
struct WindowBytes {
    const uint8_t *win;
    int64_t base;                                    // the text offset of win[0]
    __device__ __forceinline__ uint32_t operator()(uint64_t o) const { return win[(int64_t)o - base]; }
};

// Segment i's bounds: records that start in [start, end).  An anchor past the text is cut to
// it (and is then not where any walk lands).
__device__ __forceinline__ void bam_segment(const BamArgs &a, uint32_t i, uint32_t &start, uint32_t &end)
{
    const uint64_t s = i ? a.anchor[i] : 0ull, e = i + 1u < a.nseg ? a.anchor[i + 1u] : (uint64_t)a.n;
    start = (uint32_t)(s < a.n ? s : a.n);
    end = (uint32_t)(e < a.n ? e : a.n);
}

// The walk of one segment by one wavefront (block of 64); every lane runs the same hops on
// the same LDS bytes, so every branch is the whole wave's.  f(j, pos, is_read): record j of
// the segment.  Returns the status; pos: where the walk stopped.
template <class F> __device__ __forceinline__ uint32_t bam_walk(const BamArgs &a, uint32_t start, uint32_t end, uint8_t *win, uint32_t &pos,
                                                                uint32_t &cnt, uint32_t &reads, F f)
{
    const uint32_t lane = threadIdx.x;
    pos = start; cnt = 0u; reads = 0u;
    while (pos < end) {
        if (a.n - pos < 24u) return BAM_HOP_INCOMPLETE;
        // the window: BAM_WIN bytes from the 16-byte unit that holds pos
        const uint64_t u0 = ((uint64_t)pos + a.lead) >> 4;
        const int64_t base = (int64_t)(16u * u0) - (int64_t)a.lead;
        __syncthreads();                                    // (the hops of the window before are done)
#pragma unroll
        for (uint32_t q = 0; q < BAM_WIN / 1024u; ++q) {
            const uint64_t u = u0 + q * 64u + lane;
            const int64_t b0 = (int64_t)(16u * u) - (int64_t)a.lead;
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (b0 + 16 > 0 && b0 < (int64_t)a.n) w = *reinterpret_cast<const uint4 *>(a.in - a.lead + 16u * u);
            *reinterpret_cast<uint4 *>(win + 16u * (q * 64u + lane)) = w;
        }
        __syncthreads();
        const int64_t wend = base + (int64_t)BAM_WIN < (int64_t)a.n ? base + (int64_t)BAM_WIN : (int64_t)a.n;
        const WindowBytes get{win, base};
        while (pos < end && (int64_t)pos + 24 <= wend) {
            BamRec r;
            const uint32_t st = bam_hop(get, pos, a.n, r);
            if (st != BAM_HOP_OK) return st;
            const bool is_read = bam_selected(a.which, r.flag) && r.l_seq != 0u;
            f(cnt, pos, is_read);
            ++cnt;
            reads += is_read ? 1u : 0u;
            pos = (uint32_t)r.end;
        }
    }
    return BAM_HOP_OK;
}

// The same walk with every hop's bytes loaded from memory (no staging, no barrier): what one
// lane per segment runs, and the other side of the staging's A/B (hsa_bam_walk_mode).
template <class F> __device__ __forceinline__ uint32_t bam_walk_direct(const BamArgs &a, uint32_t start, uint32_t end, uint32_t &pos,
                                                                       uint32_t &cnt, uint32_t &reads, F f)
{
    const GlobalBytes get{a.in};
    pos = start; cnt = 0u; reads = 0u;
    while (pos < end) {
        BamRec r;
        const uint32_t st = bam_hop(get, pos, a.n, r);
        if (st != BAM_HOP_OK) return st;
        const bool is_read = bam_selected(a.which, r.flag) && r.l_seq != 0u;
        f(cnt, pos, is_read);
        ++cnt;
        reads += is_read ? 1u : 0u;
        pos = (uint32_t)r.end;
    }
    return BAM_HOP_OK;
}

// Record j of a segment with `before` records and reads ahead of it: its start, the reads
// before it, and the record behind the max_records-th read (one record is that one)
__device__ __forceinline__ void bam_note(const BamArgs &a, const Bam2 &before, uint32_t j, uint32_t at, bool is_read, uint32_t reads)
{
    const uint64_t k = (uint64_t)before.cnt + j;
    if (k <= a.M) {
        a.rs[k] = at;
        a.kord[k] = before.reads + reads;
        if (is_read && before.reads + reads + 1u == a.max_rec) a.g[G_LIMIT] = (uint32_t)k + 1u;
    }
}

// MODE 0: one wavefront per segment, hops inside the staged window; 1: one wavefront per
// segment, hops that load from memory; 2: one lane per segment (hops that load from memory).
// Segment 0 needs no scan to know its records' indices: its starts are written here, and
// k_bam_starts does not walk it again (the whole of a single-anchor call).
template <int MODE> __global__ void __launch_bounds__(64) k_bam_walk(BamArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t win[MODE == 0 ? BAM_WIN : 16u];
    const uint32_t i = MODE == 2 ? blockIdx.x * 64u + threadIdx.x : blockIdx.x;
    if (MODE == 2 && i >= a.nseg) return;
    const bool writer = MODE == 2 || threadIdx.x == 0u;
    uint32_t start, end, pos, cnt, reads;
    bam_segment(a, i, start, end);
    const Bam2 none{0u, 0u};
    auto note = [&](uint32_t j, uint32_t at, bool is_read) { if (i == 0u && writer) bam_note(a, none, j, at, is_read, reads); };
    const uint32_t st = MODE == 0 ? bam_walk(a, start, end, win, pos, cnt, reads, note) : bam_walk_direct(a, start, end, pos, cnt, reads, note);
    if (writer) {
        a.seg_in[i] = Bam2{cnt, reads};
        a.seg_exit[i] = pos;
        a.seg_st[i] = st;
        // verified: landed on the next anchor.  The last segment ends the prefix anyway.
        const bool ok = i + 1u < a.nseg && st == BAM_HOP_OK && (uint64_t)pos == a.anchor[i + 1u] && (i ? a.anchor[i] : 0ull) <= a.anchor[i + 1u];
        if (!ok) atomicMin(&a.g[G_V], i);                   // (a minimum: order-free)
    }
}

template <int MODE> __global__ void __launch_bounds__(64) k_bam_starts(BamArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t win[MODE == 0 ? BAM_WIN : 16u];
    const uint32_t i = MODE == 2 ? blockIdx.x * 64u + threadIdx.x : blockIdx.x, V = a.g[G_V];
    if (i >= a.nseg || i > V) return;                       // (MODE 0, 1: the whole wave)
    const bool writer = MODE == 2 || threadIdx.x == 0u;
    const Bam2 before = a.seg_out[i];
    uint32_t start, end, pos = a.seg_exit[i], cnt = a.seg_in[i].cnt, reads = a.seg_in[i].reads;
    if (i != 0u && before.cnt <= a.M) {                     // (segment 0: k_bam_walk wrote them; past M: no row of it is looked at)
        bam_segment(a, i, start, end);
        auto note = [&](uint32_t j, uint32_t at, bool is_read) { if (writer) bam_note(a, before, j, at, is_read, reads); };
        if (MODE == 0) bam_walk(a, start, end, win, pos, cnt, reads, note);
        else bam_walk_direct(a, start, end, pos, cnt, reads, note);
    }
    if (i == V && writer) {
        const uint64_t total = (uint64_t)before.cnt + cnt;
        const uint32_t st = a.seg_st[i];
        a.g[G_TOTAL] = total < BAM_ONES32 ? (uint32_t)total : BAM_ONES32;
        a.g[G_END_ST] = st != BAM_HOP_OK ? st : V + 1u < a.nseg ? BAM_ST_END : BAM_HOP_OK;
        if (total <= a.M) { a.rs[total] = pos; a.kord[total] = before.reads + reads; }
        a.bctr[3] = pos;
    }
}

__device__ __forceinline__ uint32_t bam_cand(const BamArgs &a) { return a.g[G_TOTAL] < a.M ? a.g[G_TOTAL] : a.M; }
__device__ __forceinline__ uint32_t bam_loaded(const BamArgs &a)
{
    const uint32_t c = bam_cand(a), n = a.g[G_BAD] < c ? a.g[G_BAD] : c;
    return a.g[G_LIMIT] < n ? a.g[G_LIMIT] : n;
}

// One wavefront per BAM_RT consecutive records, lanes along the bytes; the record, and so
// every trip count and every branch around a ballot, is the same in all 64 lanes.
__global__ void __launch_bounds__(64) k_bam_record(BamArgs a)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t cand = bam_cand(a);
    const GlobalBytes get{a.in};
    for (uint32_t t = 0; t < BAM_RT; ++t) {
        const uint32_t k = blockIdx.x * BAM_RT + t;
        if (k >= cand) break;                               // (the whole wave)
        BamRec r;
        bool bad = bam_hop(get, a.rs[k], a.n, r) != BAM_HOP_OK;      // (the walk took this hop: never)
        uint32_t name_len = 0, len = 0, full = 0, nn = 0, poly = 0;
        const bool filtered = bad || !bam_selected(a.which, r.flag) || r.l_seq == 0u;
        if (!filtered) {
            name_len = r.l_read_name;
            for (uint32_t p0 = 0; p0 < r.l_read_name; p0 += 64u) {
                const uint32_t p = p0 + lane;
                const uint32_t c = a.in[r.name + (p < r.l_read_name ? p : 0u)];
                const unsigned long long nul = __ballot(p < r.l_read_name && c == 0u);
                if (nul) { name_len = p0 + (uint32_t)__ffsll((long long)nul) - 1u; break; }
            }
            if (name_len == 0u || r.l_seq > HSA_RD_MAX_LEN || (a.maxdiff && r.l_seq >= a.n_maxdiff)) bad = true;
            else {
                full = r.l_seq;
                const uint8_t *in = a.in;
                len = a.trim_qual >= 1
                          ? rd_trim_walk([&](uint32_t l) { return (int32_t)bam_qual33(in[bam_qual_at(r, l)]) - 33; }, full, a.trim_qual, lane)
                          : full;
                unsigned long long not_a = 0, not_t = 0;
                for (uint32_t p0 = 0; p0 < len; p0 += 64u) {
                    const uint32_t p = p0 + lane;
                    const bool on = p < len;
                    const uint32_t code = bam_code(r, on ? p : 0u, in[bam_code_at(r, on ? p : 0u)]);
                    nn += (uint32_t)__popcll(__ballot(on && code > 3u));
                    if (p0 == 0u) {
                        not_a = __ballot(lane < 15u && (!on || code != 0u));
                        not_t = __ballot(lane < 15u && (!on || code != 3u));
                    }
                }
                poly = len >= 15u && (not_a == 0ull || not_t == 0ull);
            }
        }
        if (lane == 0u) {
            a.r_len[k] = len; a.r_nn[k] = nn; a.r_name_len[k] = name_len; a.r_full[k] = full;
            a.r_fl[k] = filtered ? BAM_FL_FILTERED : poly ? BAM_FL_POLY : 0u;
            if (bad) atomicMin(&a.g[G_BAD], k);
        }
    }
}

// The tail that does not depend on the format (hsa_rd_tail.h, shared with hsa_reads.hip)
__global__ void __launch_bounds__(256) k_bam_max(BamArgs a) { rd_tail_max(a, [&] { return bam_loaded(a); }); }

__global__ void __launch_bounds__(256) k_bam_keep(BamArgs a) { rd_tail_keep(a, [&] { return bam_loaded(a); }); }

__global__ void __launch_bounds__(256) k_bam_rows(BamArgs a)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const uint32_t loaded = bam_loaded(a);
    const Rd3 tot = a.s_out[a.M];
    if (k < loaded) rd_tail_row(a, k);
    if (k == 0u) {
        if (tot.j <= a.job_cap) { a.name_off[tot.j] = tot.n; a.qual_off[tot.j] = tot.c; }
        const uint32_t bad = a.g[G_BAD], cand = bam_cand(a), total = a.g[G_TOTAL], end_st = a.g[G_END_ST];
        const bool has_bad = bad == loaded && bad < cand && bad < a.g[G_LIMIT];
        const uint32_t read = a.kord[loaded];               // the reads among the records loaded
        unsigned long long *c = a.ctr;
        c[0] = loaded + (has_bad ? 1u : 0u);
        c[1] = read;
        a.octr[0] = loaded; a.octr[1] = loaded - read;
        c[2] = tot.j; c[3] = tot.j < a.job_cap ? tot.j : a.job_cap;
        c[4] = tot.c + 16u; c[5] = c[4] < a.code_cap ? c[4] : a.code_cap;
        c[6] = tot.n; c[7] = tot.n < a.name_cap ? tot.n : a.name_cap;
        c[8] = tot.c; c[9] = tot.c < a.qual_cap ? tot.c : a.qual_cap;
        c[10] = a.rs[loaded];
        c[11] = has_bad ? bad : ~0ull;
        c[12] = has_bad ? c[10] : ~0ull;
        c[13] = a.g[G_MAXL]; c[14] = a.g[G_MAXK];
        c[15] = (unsigned long long)(long long)rd_threshold(a);
        const uint32_t V = a.g[G_V];
        const bool to_end = end_st == BAM_HOP_OK;           // the last segment's walk reached the end of the text
        a.bctr[0] = has_bad ? HSA_BAM_END_HOST : loaded < total ? HSA_BAM_END_MAX
                    : to_end ? HSA_BAM_END_INPUT : end_st == BAM_ST_END ? HSA_BAM_END_ANCHOR
                    : end_st == BAM_HOP_INCOMPLETE && !a.at_eof ? HSA_BAM_END_INCOMPLETE : HSA_BAM_END_MALFORMED;
        a.bctr[1] = V + (to_end ? 1u : 0u);
        a.bctr[2] = total;
    }
}

// The three byte arrays, as k_rd_bytes: one wavefront per BAM_RT consecutive records, the
// lanes along the bases of a kept read in its own orientation: lane p stores code p and
// quality p (a wave's store covers 64 contiguous bytes of one array) and loads the stored
// byte that holds them, which for a reversed read runs backwards.  A byte at or past its
// array's capacity is not stored.
__global__ void __launch_bounds__(64) k_bam_bytes(BamArgs a)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t loaded = bam_loaded(a);
    const uint8_t *in = a.in;
    const GlobalBytes get{a.in};
    if (blockIdx.x == 0 && lane < 16u) {                    // the codes' zero padding (hsa_device_batch_t)
        const uint64_t at = a.s_out[a.M].c + lane;
        if (at < a.code_cap) a.codes[at] = 0u;
    }
    for (uint32_t t = 0; t < BAM_RT; ++t) {
        const uint32_t k = blockIdx.x * BAM_RT + t;
        if (k >= loaded) break;                             // (the whole wave)
        if (a.r_fl[k] != HSA_RD_SEARCHED) continue;
        BamRec r;
        if (bam_hop(get, a.rs[k], a.n, r) != BAM_HOP_OK) continue;    // (never: k_bam_record took it)
        const Rd3 at = a.s_out[k];
        const uint32_t len = r.l_seq, nl = a.r_name_len[k];
        const uint32_t most = len > nl ? len : nl;
        for (uint32_t p0 = 0; p0 < most; p0 += 64u) {
            const uint32_t p = p0 + lane;
            const uint32_t ps = p < len ? p : 0u;
            const uint32_t c = in[bam_code_at(r, ps)], q = in[bam_qual_at(r, ps)], m = in[r.name + (p < nl ? p : 0u)];
            if (p < len) {
                if (at.c + p < a.code_cap) a.codes[at.c + p] = (uint8_t)bam_code(r, p, c);
                if (at.c + p < a.qual_cap) a.quals[at.c + p] = (uint8_t)bam_qual33(q);
            }
            if (p < nl && at.n + p < a.name_cap) a.names[at.n + p] = (uint8_t)m;
        }
    }
}

static int g_rd_timing_bam = 0;

extern "C" void hsa_bam_timing(int on) { g_rd_timing_bam = on; }

// How the segments are walked (k_bam_walk's MODE): 0 by default, which tools/bam_probe.py's A/B
// chose.  hsa_bam_walk_mode is that probe's knob and is declared in no header: 0 one wavefront
// per segment hopping inside the window staged in LDS, 1 one wavefront per segment with every
// hop loading from memory, 2 one lane per segment; the results are the same.  Process-wide and
// not synchronised: a probe sets it between its own calls, nothing else does.
static int g_bam_walk_mode = 0;

extern "C" void hsa_bam_walk_mode(int mode) { g_bam_walk_mode = mode >= 0 && mode <= 2 ? mode : 0; }

extern "C" int hsa_bam_launch_times(hsa_index_t *ix, float *ms) { return hsa_stage_times(ix, &hsa_index::rd_t, ms, "hsa_bam"); }

extern "C" int hsa_bam_reads_device(hsa_index_t *ix, const hsa_bam_batch_t *b, void *stream)
{
    const char *what = "hsa_bam_reads_device";
    if (!ix) {
        int nd = 0;
        if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) { hsa_set_error("%s: no HIP device visible", what); return HSA_E_NODEV; }
        hsa_set_error("%s: null handle", what);
        return HSA_E_ARG;
    }
    if (!b || !b->d_counters || !b->d_opt_counters || !b->d_bam_counters || !b->d_rec || !b->d_name_off || !b->d_qual_off ||
        !b->d_anchor || !b->d_full_len || (b->n_in && !b->d_in) || (b->job_cap && !b->d_jobs) || (b->code_cap && !b->d_codes) ||
        (b->name_cap && !b->d_names) || (b->qual_cap && !b->d_quals)) {
        hsa_set_error("%s: null argument", what);
        return HSA_E_ARG;
    }
    if (b->n_in >= 0xFFFFFF00ull || b->max_records < 1u || b->max_records > (1u << 28) || (b->at_eof != 0 && b->at_eof != 1) ||
        (b->d_maxdiff && b->len_floor >= b->n_maxdiff) || b->job_cap > (1ull << 32) || b->rec_cap > (1u << 28)) {
        hsa_set_error("%s: n_in under 2^32 - 256, max_records in 1..2^28, rec_cap at most 2^28, at_eof 0 or 1, len_floor inside the table", what);
        return HSA_E_ARG;
    }
    if (b->n_anchor < 1u || b->n_anchor > (1u << 28) || b->which < 1u || b->which > 7u || b->trim_qual > BAM_MAX_TRIM) {
        hsa_set_error("%s: n_anchor in 1..2^28, which in 1..7, trim_qual at most %d", what, BAM_MAX_TRIM);
        return HSA_E_ARG;
    }
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = hsa_stage_stream(stream, ix->stream);
    BamArgs A{};
    A.in = b->d_in; A.n = (uint32_t)b->n_in;
    A.lead = b->n_in ? (uint32_t)(reinterpret_cast<uintptr_t>(b->d_in) & 15u) : 0u;
    const uint64_t most = b->n_in / 37u + 1u;               // (the shortest record has 37 bytes)
    const uint32_t rows = b->rec_cap ? b->rec_cap : b->max_records;
    A.M = (uint32_t)(most < rows ? most : rows);
    A.nseg = b->n_anchor; A.which = b->which; A.max_rec = b->max_records;
    A.at_eof = b->at_eof; A.max_diff = b->max_diff; A.seed_len = b->seed_len; A.regime = b->regime;
    A.trim_qual = b->trim_qual >= 1 ? b->trim_qual : 0;
    A.maxdiff = b->d_maxdiff; A.n_maxdiff = b->n_maxdiff; A.len_floor = b->len_floor;
    A.anchor = b->d_anchor;
    A.jobs = b->d_jobs; A.job_cap = b->job_cap; A.codes = b->d_codes; A.code_cap = b->code_cap;
    A.names = b->d_names; A.name_cap = b->name_cap; A.name_off = b->d_name_off;
    A.quals = b->d_quals; A.qual_cap = b->qual_cap; A.qual_off = b->d_qual_off;
    A.full_len = b->d_full_len; A.rec = b->d_rec;
    A.ctr = (unsigned long long *)b->d_counters; A.octr = (unsigned long long *)b->d_opt_counters;
    A.bctr = (unsigned long long *)b->d_bam_counters;
    size_t tmp1 = 0, tmp2 = 0;
    HSA_TRY(hsa_scan_bytes(tmp1, Bam2{0, 0}, (size_t)A.nseg + 1, Bam2Plus(), st));
    HSA_TRY(hsa_scan_bytes(tmp2, Rd3{0, 0, 0}, (size_t)A.M + 1, Rd3Plus(), st));
    void *d_tmp = nullptr;
    auto layout = [&](Carver c) {
        A.g = c.take<uint32_t>(G_WORDS);
        A.seg_in = c.take<Bam2>((size_t)A.nseg + 1);
        A.seg_out = c.take<Bam2>((size_t)A.nseg + 1);
        A.seg_exit = c.take<uint32_t>(A.nseg);
        A.seg_st = c.take<uint32_t>(A.nseg);
        A.rs = c.take<uint32_t>((size_t)A.M + 2);
        A.kord = c.take<uint32_t>((size_t)A.M + 2);
        A.r_len = c.take<uint32_t>(A.M);
        A.r_nn = c.take<uint32_t>(A.M);
        A.r_fl = c.take<uint32_t>(A.M);
        A.r_name_len = c.take<uint32_t>(A.M);
        A.r_full = c.take<uint32_t>(A.M);
        A.s_in = c.take<Rd3>((size_t)A.M + 1);
        A.s_out = c.take<Rd3>((size_t)A.M + 1);
        d_tmp = c.take<char>(std::max(tmp1, tmp2));
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_rd, &ix->d_rd_cap, layout(Carver())));
    layout(Carver(ix->d_rd));
    StageTimer &tm = ix->rd_t;
    HSA_TRY(tm.begin(g_rd_timing_bam != 0));
    HSA_TRY(tm.mark(0, st));
    HSA_HIP(hipMemsetAsync(A.g, 0, G_WORDS * 4, st));
    HSA_HIP(hipMemsetAsync(A.g + G_BAD, 0xFF, 4, st));       // no record for the host yet
    HSA_HIP(hipMemsetAsync(A.g + G_LIMIT, 0xFF, 8, st));     // no limit by the reads; G_V: no segment failed yet
    HSA_HIP(hipMemsetAsync(A.octr, 0, HSA_RD_OPT_COUNTERS * sizeof(uint64_t), st));
    HSA_HIP(hipMemsetAsync(A.bctr, 0, HSA_BAM_COUNTERS * sizeof(uint64_t), st));
    HSA_HIP(hipMemsetAsync(A.seg_in + A.nseg, 0, sizeof(Bam2), st));
    // (a start the walks do not reach is never read; zeroed so that no run depends on an earlier one)
    HSA_HIP(hipMemsetAsync(A.rs, 0, ((size_t)A.M + 2) * 4, st));
    HSA_HIP(hipMemsetAsync(A.kord, 0, ((size_t)A.M + 2) * 4, st));
    const int mode = g_bam_walk_mode;
    const unsigned sb = mode == 2 ? (A.nseg + 63u) / 64u : A.nseg;
    if (mode == 2) hipLaunchKernelGGL(k_bam_walk<2>, dim3(sb), dim3(64), 0, st, A);
    else if (mode == 1) hipLaunchKernelGGL(k_bam_walk<1>, dim3(sb), dim3(64), 0, st, A);
    else hipLaunchKernelGGL(k_bam_walk<0>, dim3(sb), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(1, st));
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp1, A.seg_in, A.seg_out, Bam2{0, 0}, (size_t)A.nseg + 1, Bam2Plus(), st));
    HSA_TRY(tm.mark(2, st));
    if (mode == 2) hipLaunchKernelGGL(k_bam_starts<2>, dim3(sb), dim3(64), 0, st, A);
    else if (mode == 1) hipLaunchKernelGGL(k_bam_starts<1>, dim3(sb), dim3(64), 0, st, A);
    else hipLaunchKernelGGL(k_bam_starts<0>, dim3(sb), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(3, st));
    const unsigned rb = (A.M + 1u + 255u) / 256u, wb = (A.M + BAM_RT - 1u) / BAM_RT;
    hipLaunchKernelGGL(k_bam_record, dim3(wb), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(4, st));
    hipLaunchKernelGGL(k_bam_max, dim3(rb), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bam_keep, dim3(rb), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(5, st));
    HSA_HIP(rocprim::exclusive_scan(d_tmp, tmp2, A.s_in, A.s_out, Rd3{0, 0, 0}, (size_t)A.M + 1, Rd3Plus(), st));
    HSA_TRY(tm.mark(6, st));
    hipLaunchKernelGGL(k_bam_rows, dim3(rb), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(7, st));
    hipLaunchKernelGGL(k_bam_bytes, dim3(wb), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    HSA_TRY(tm.mark(8, st));
    tm.end();
    return 0;
}
