// hsa_refine.hip -- position rows of the 64-bit path to CIGAR, NM and MD.
//
// Restates refine_gapped_core (bwtse.c:380-440), the banded global alignment it calls
// (aln_global_core with aln_param_bwa, stdaln.c:227, :258-319, :345-525; the path to
// CIGAR, aln_path2cigar32 :1010-1040) and bwa_cal_md1 (bwtse.c:442-494).  The first hot
// path of the project that is a dynamic program and not a rank walk.
//
// hsa_refine_rows_device64 is two launches on one stream, no host round trip:
//   k_refine_rows  one lane per position row: the row's read and record, its status,
//                  the whole answer of an ungapped row (a streaming text compare, the
//                  text read a word of 16 codes at a time), and the gapped rows appended
//                  to a list (one atomic per wave; a row's answer does not depend on its
//                  place in the list, so two runs give equal arrays);
//   k_refine_dp    one wavefront per gapped row, the list dealt to the blocks round robin.
//
// The alignment, cell by cell.  Rows j = 0..len2 are read positions, columns i = 0..len1
// window positions; b1, b2 as stdaln.c:372-380.  The reference's three loop nests
// (:401-485) compute, for 1 <= j <= len2, the cells lo(j) < i <= end(j) with end(j) =
// min(j + b1 - 1, len1) and lo(j) = 0 for j <= b2, j - b2 after; cell (j, lo(j)) is the
// column-0 cell (M = D = -inf, I from (j - 1, 0) by set_end_I; j <= b2) or a border set to
// -inf (j > b2).  For an inner cell
//   M from (j - 1, i - 1) by set_M,
//   D from (j, i - 1) by set_D, or set_end_D in the last row (:431, :479),
//   I from (j - 1, i): -inf where i = end(j) = j + b1 - 1 <= len1 (:418, :454: the cell
//     above lies outside the band), set_end_I in column len1 (:417, :468), set_I otherwise.
// Whenever rows j > b2 exist, b1 - b2 = len1 - len2 (the clamps at :379-380 then leave
// both alone or make b2 = len2), so "part 2" (:443) is exactly j + b1 - 1 <= len1 and the
// one rule above covers all three nests.  Only in-band cells are computed: the reference
// never reads a cell it did not set in the row before -- (j - 1, i - 1) needs lo(j - 1) <=
// lo(j) <= i - 1 <= end(j) - 1 <= end(j - 1), (j - 1, i) is read only where i <= end(j - 1)
// (the -inf rule above is its guard), and the border is written before it is read (:444,
// :460, :474) -- checked against stdaln.c:394-485 while restating it.
//
// One wavefront per row, lanes along a DP row (not along an anti-diagonal): a row's band
// is cut into chunks of 64 columns.  M and I depend on the row above only, which lives in
// LDS (a ring of columns, updated in place: every lane reads its two cells before any
// lane stores); D's dependence on the cell to its left is a max-plus prefix, D(i) =
// max_k (M(k - 1) - open - ext (i - k + 1)), so one 6-step wave scan of y(i) = M(i - 1) -
// open - ext + ext i gives every D of the chunk and its traceback type (M iff y(i) beats
// the prefix before it: the reference's strict `>`, :300).  This serves any band, also
// the wide ones of a window cut at the text's end (b2 = len2 - len1 + 50), which a
// lane-per-diagonal layout could not hold; the price is 7 shuffles per chunk.
// Traceback bytes (3 + 2 + 2 bits, dpcell_t :321-324) go to per-wave HBM scratch, one row
// of tb_stride bytes per read position, sized by the band and not by len^2; the wave walks
// them back (:488-513) and lane 0 stores the CIGAR, MD and NM.
#include <hip/hip_runtime.h>
#include <string.h>

#include "hsa_device.h"
#include "hsa_internal.h"
#include "hsa_text.h"

#define HSA_ALN64_WORDS 14u
#define RF_INF      (-1073741823)      // MINOR_INF, stdaln.h:88
#define RF_OPEN     26                 // aln_param_bwa, stdaln.c:227: gap_open, gap_ext, gap_end,
#define RF_EXT      9                  //   aln_sm_maq (11 match, -19 mismatch, -13 with an N),
#define RF_END      5                  //   band_width 50
#define RF_BAND     50
#define RF_M 0u
#define RF_I 1u
#define RF_D 2u
#define RF_S 4u
#define RF_SCRATCH_BUDGET ((size_t)1 << 30)   // per-wave traceback scratch of one call, at most

struct RefineArgs {
    TextView text;
    const hsa_job_t *jobs;
    uint32_t n_jobs;
    const uint8_t *codes;
    const uint64_t *hit_off;
    const uint32_t *hits;
    const uint64_t *pos_off, *pos;
    const uint32_t *pos_hit;
    uint64_t pos_cap;
    const uint64_t *pos_ctr;
    uint32_t max_len;              // the layout's read length: longer rows are HSA_RF_CAP
    uint32_t cigar_stride, md_stride;
    uint32_t *rows;
    uint64_t *rpos;
    uint32_t *cigar;
    uint8_t *md;
    unsigned long long *ctr;
    uint32_t *list;                // gapped rows, ctr[6] of them
    uint8_t *wave;                 // per-wave scratch: tb_rows x tb_stride bytes, then the runs
    size_t wave_bytes, tb_bytes;
    uint32_t tb_stride, ring, win_cap;
    uint32_t all_dp;               // every row is aligned, a row without a gap too (the spliced segments)
};

struct RfRow {
    uint64_t pos, ori, off;
    uint32_t len, gap, strand;
};

__device__ __forceinline__ uint64_t rf_n_rows(const RefineArgs &a)
{
    uint64_t n = a.pos_off[a.n_jobs];
    if (n > a.pos_cap) n = a.pos_cap;
    if (a.pos_ctr && a.pos_ctr[1] < n) n = a.pos_ctr[1];
    return n;
}

// Row t: its read (the last j with pos_off[j] <= t), its record, its position.
__device__ __forceinline__ void rf_row(const RefineArgs &a, uint64_t t, RfRow &r)
{
    const uint32_t lo = hsa_row_read(a.pos_off, a.n_jobs, t);
    const hsa_job_t jb = a.jobs[lo];
    const uint32_t *rec = a.hits + (a.hit_off[lo] + a.pos_hit[t]) * HSA_ALN64_WORDS;
    const uint32_t w0 = rec[0], w1 = rec[1];
    r.gap = ((w0 >> 16) & 0xFFu) + (w0 >> 24);         // n_gapo + n_gape (bwtse.c:89)
    r.strand = w1 >> 30;
    r.len = jb.len;
    r.off = jb.off;
    r.ori = a.pos[4 * t + 2];
    r.pos = a.pos[4 * t + 3];
}

// The read as the SAM stage hands it over: strand ? rseq : seq (bwtse.c:554), rseq the
// reverse complement (bwaseqio.c:212-215, seq_reverse :73-90: codes >= 4 stay)
__device__ __forceinline__ uint32_t rf_read_code(const RefineArgs &a, const RfRow &r, uint32_t y)
{
    if (!r.strand) return a.codes[r.off + y];
    const uint32_t c = a.codes[r.off + (r.len - 1u - y)];
    return c < 4u ? 3u - c : c;
}

struct MdOut {
    uint8_t *p;
    uint32_t cap, n;
    bool w;                        // this lane stores (every lane counts)
    __device__ __forceinline__ void put(uint32_t c)
    {
        if (w && n < cap) p[n] = (uint8_t)c;
        ++n;
    }
    __device__ __forceinline__ void num(uint32_t u)    // ksprintf("%d"), u < 100 000
    {
        bool on = false;
        for (uint32_t d = 10000u; d; d /= 10u) {
            const uint32_t q = u / d;
            u -= q * d;
            if (q || on || d == 1u) { put('0' + q); on = true; }
        }
    }
    __device__ __forceinline__ void base(uint32_t c) { put((0x54474341u >> (8u * c)) & 0xFFu); }  // "ACGT"[c]
};

__device__ __forceinline__ void rf_write_row(const RefineArgs &a, uint64_t t, uint32_t status, uint32_t n_cigar,
                                             uint32_t nm, uint32_t md_len, uint32_t trim5, uint32_t trim3, uint64_t pos,
                                             uint64_t ori)
{
    uint4 *o = reinterpret_cast<uint4 *>(a.rows + HSA_RF_ROW_WORDS * t);
    o[0] = make_uint4(status, n_cigar, nm, md_len);
    o[1] = make_uint4(trim5, trim3, 0u, 0u);
    reinterpret_cast<ulonglong2 *>(a.rpos)[t] = make_ulonglong2(pos, ori);
}

// The no-gap branch of bwa_cal_md1 (bwtse.c:478-491) and the one `len`M op.
__device__ __forceinline__ uint32_t rf_ungapped(const RefineArgs &a, uint64_t t, const RfRow &r)
{
    MdOut md{a.md + (size_t)a.md_stride * t, a.md_stride, 0u, true};
    uint32_t u = 0, nm = 0;
    uint32_t w = hsa_text_word(a.text, r.pos >> 4);
    for (uint32_t z = 0; z < r.len; ++z) {
        const uint64_t p = r.pos + z;
        if (z && ((uint32_t)p & 15u) == 0) w = hsa_text_word(a.text, p >> 4);
        const uint32_t c = (w >> (2u * ((uint32_t)p & 15u))) & 3u, s = rf_read_code(a, r, z);
        if (s > 3u || c != s) {
            md.num(u); md.base(c);
            ++nm; u = 0;
        } else ++u;
    }
    md.num(u);
    if (a.cigar_stride) a.cigar[(size_t)a.cigar_stride * t] = (RF_M << 28) | r.len;
    const uint32_t st = (a.cigar_stride < 1u || md.n > a.md_stride) ? HSA_RF_MD : HSA_RF_OK;
    rf_write_row(a, t, st, 1u, nm, md.n, 0u, 0u, r.pos, r.ori);
    return st;
}

#define RF_NONE 0xFFu      // no row in this lane
#define RF_DP   0xFEu      // a gapped row: answered by k_refine_dp

__global__ void __launch_bounds__(256) k_refine_rows(RefineArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = rf_n_rows(a);
    if (t == 0) a.ctr[0] = n;
    uint32_t st = RF_NONE;
    if (t < n) {
        RfRow r;
        rf_row(a, t, r);
        if (r.pos == ~0ull || r.ori == ~0ull) st = HSA_RF_POS;
        else if (r.len == 0 || r.len > a.max_len || r.gap > HSA_RF_MAX_GAP) st = HSA_RF_CAP;
        else if (r.gap == 0 && !a.all_dp) st = r.pos + r.len > a.text.n ? HSA_RF_TEXT : rf_ungapped(a, t, r);
        else st = r.pos >= a.text.n ? HSA_RF_TEXT : RF_DP;
        if (st != RF_DP && st != HSA_RF_OK && st != HSA_RF_MD) rf_write_row(a, t, st, 0u, 0u, 0u, 0u, 0u, r.pos, r.ori);
    }
    // the wave's counts and its gapped rows: every ballot first, then one lane's atomics,
    // then one broadcast (no wave-wide operation between two one-lane regions)
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long ms[HSA_RF_MD + 1];
#pragma unroll
    for (uint32_t s = 0; s <= HSA_RF_MD; ++s) ms[s] = __ballot(st == s);
    const unsigned long long m = __ballot(st == RF_DP);
    unsigned long long base = 0;
    if (lane == 0) {
#pragma unroll
        for (uint32_t s = 0; s <= HSA_RF_MD; ++s)
            if (ms[s]) atomicAdd(&a.ctr[1 + s], (unsigned long long)__popcll(ms[s]));
        if (m) base = atomicAdd(&a.ctr[6], (unsigned long long)__popcll(m));
    }
    base = __shfl(base, 0);
    if (st == RF_DP) a.list[base + __popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)t;
}

// set_M (stdaln.c:260-275): the best of the cell's three states, `>=` toward M, then D
// over I on a tie
__device__ __forceinline__ int rf_best(int m, int i, int d, uint32_t &ty)
{
    if (m >= i) {
        if (m >= d) { ty = RF_M; return m; }
        ty = RF_D; return d;
    }
    if (i > d) { ty = RF_I; return i; }
    ty = RF_D; return d;
}

__device__ __forceinline__ int rf_lo(int j, int b2) { return j <= b2 ? 0 : j - b2; }

__global__ void __launch_bounds__(64) k_refine_dp(RefineArgs a)
{
    extern __shared__ int rf_sm[];
    const int lane = (int)threadIdx.x;
    const int RM = (int)a.ring - 1;
    int *sM = rf_sm, *sI = rf_sm + a.ring, *sD = rf_sm + 2 * a.ring;
    uint8_t *refw = reinterpret_cast<uint8_t *>(rf_sm + 3 * a.ring);    // the text window
    uint8_t *rd = refw + a.win_cap;                                     // the read, oriented
    uint8_t *tb = a.wave + (size_t)blockIdx.x * a.wave_bytes;
    uint32_t *runs = reinterpret_cast<uint32_t *>(tb + a.tb_bytes);
    const int S = (int)a.tb_stride;
    const uint32_t n_dp = (uint32_t)a.ctr[6];
    // The rows are dealt to the blocks round robin, and everything after the DP is run by
    // every lane alike (same loads, same path; lane 0 alone stores): the loop holds no
    // one-lane region.  A first version took rows from an atomic queue in lane 0 and walked
    // the backtrace in lane 0 only; the compiler threaded the other lanes from the end of
    // one iteration past the queue's `if` into the next iteration's broadcast, where they
    // spun without lane 0.
    for (uint32_t q = blockIdx.x; q < n_dp; q += gridDim.x) {
        const uint64_t t = a.list[q];
        RfRow r;
        rf_row(a, t, r);
        const int len2 = (int)r.len;
        // the window: len + gap characters, cut at the text's end (bwtse.c:391-394); >= 1
        const uint64_t room = a.text.n - r.pos;
        const int len1 = room < (uint64_t)(r.len + r.gap) ? (int)room : (int)(r.len + r.gap);
        __syncthreads();                                   // the last row's lane 0 is done with the LDS
        for (int i = lane; i < len1; i += 64) refw[i] = (uint8_t)hsa_text_code(a.text, r.pos + i);
        for (int y = lane; y < len2; y += 64) {
            const uint32_t c = rf_read_code(a, r, (uint32_t)y);
            rd[y] = (uint8_t)(c > 4u ? 4u : c);            // (the score matrix has five rows)
        }
        int b1, b2;                                        // stdaln.c:372-380
        if (len1 > len2) { b1 = len1 - len2 + RF_BAND; b2 = RF_BAND; }
        else { b1 = RF_BAND; b2 = len2 - len1 + RF_BAND; }
        if (b1 > len1) b1 = len1;
        if (b2 > len2) b2 = len2;
        // row 0 (:394-398): M(0, 0) = 0, then end deletions
        for (int i = lane; i < b1; i += 64) {
            sM[i & RM] = i ? RF_INF : 0;
            sI[i & RM] = RF_INF;
            sD[i & RM] = i ? -RF_OPEN - RF_END * i : RF_INF;
            tb[i] = (uint8_t)((i == 1 ? RF_M : RF_D) << 5);
        }
        for (int j = 1; j <= len2; ++j) {
            __syncthreads();
            const int lo = rf_lo(j, b2);
            const int jb = j + b1 - 1;
            const int end = jb < len1 ? jb : len1;
            const bool right_inf = jb <= len1;
            const int ged = j == len2 ? RF_END : RF_EXT;   // set_end_D in the last row
            const uint32_t s2 = rd[j - 1];
            uint8_t *tbj = tb + (size_t)j * S - lo;
            int cM = RF_INF, cI = RF_INF, cD = RF_INF;     // the row above at column c - 1
            int nM = RF_INF, nD = RF_INF;                  // this row at column c - 1
            for (int c = lo; c <= end; c += 64) {
                const int i = c + lane;
                const bool act = i <= end;
                const int slot = i & RM;
                const int pM = act ? sM[slot] : RF_INF, pI = act ? sI[slot] : RF_INF, pD = act ? sD[slot] : RF_INF;
                int qM = __shfl_up(pM, 1), qI = __shfl_up(pI, 1), qD = __shfl_up(pD, 1);
                if (lane == 0) { qM = cM; qI = cI; qD = cD; }
                cM = __shfl(pM, 63); cI = __shfl(pI, 63); cD = __shfl(pD, 63);
                int M = RF_INF, I = RF_INF;
                uint32_t Mt = 0, It = 0;
                if (i == lo) {
                    if (j <= b2) {                         // column 0: set_end_I (:405, :424)
                        if (pM - RF_OPEN > pI) { It = RF_M; I = pM - RF_OPEN - RF_END; }
                        else { It = RF_I; I = pI - RF_END; }
                    }
                } else if (act) {
                    const uint32_t rc = refw[i - 1];
                    const int sc = s2 > 3u ? -13 : (s2 == rc ? 11 : -19);
                    M = rf_best(qM, qI, qD, Mt) + sc;
                    if (!(i == end && right_inf)) {        // set_I, set_end_I in column len1
                        const int gi = i == len1 ? RF_END : RF_EXT;
                        if (pM - RF_OPEN > pI) { It = RF_M; I = pM - RF_OPEN - gi; }
                        else { It = RF_I; I = pI - gi; }
                    }
                }
                // D: the prefix maximum of y
                int Ml = __shfl_up(M, 1);
                if (lane == 0) Ml = nM;
                int y, D = RF_INF;
                uint32_t Dt = RF_D;
                if (!act) y = -2000000000;
                else if (i == lo) y = RF_INF + ged * i;
                else if (lane == 0) {                      // a later chunk: the carried cell to the left
                    const int av = Ml - RF_OPEN - ged, dv = nD - ged;
                    Dt = av > dv ? RF_M : RF_D;
                    D = av > dv ? av : dv;
                    y = D + ged * i;
                } else y = Ml - RF_OPEN - ged + ged * i;
                int Y = y;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int o = __shfl_up(Y, d);
                    if (lane >= d && o > Y) Y = o;
                }
                const int Yex = __shfl_up(Y, 1);
                if (act && i != lo && lane != 0) {
                    D = Y - ged * i;
                    Dt = y > Yex ? RF_M : RF_D;
                }
                if (act) {
                    sM[slot] = M; sI[slot] = I; sD[slot] = D;
                    tbj[i] = (uint8_t)(Mt | (It << 3) | (Dt << 5));
                }
                nM = __shfl(M, 63); nD = __shfl(D, 63);
            }
        }
        __syncthreads();
        const int fM = __builtin_amdgcn_readfirstlane(sM[len1 & RM]), fI = __builtin_amdgcn_readfirstlane(sI[len1 & RM]),
                  fD = __builtin_amdgcn_readfirstlane(sD[len1 & RM]);
        __threadfence();                                   // the traceback bytes, before they are read back
        const bool w = lane == 0;
        {
            // the backtrace (stdaln.c:488-513), the ops as runs, last op first
            int i = len1, j = len2;
            uint32_t qb = __builtin_amdgcn_readfirstlane((uint32_t)tb[(size_t)j * S + (i - rf_lo(j, b2))]);
            int mx = fM;
            uint32_t type = qb & 7u, ctype = RF_M;
            if (fI > mx) { mx = fI; type = (qb >> 3) & 3u; ctype = RF_I; }
            if (fD > mx) { mx = fD; type = (qb >> 5) & 3u; ctype = RF_D; }
            uint32_t n_runs = 0, cur = ctype, cur_len = 0;
            bool lost = false;                             // a walk that leaves the band: never, on cells the DP set
            for (;;) {
                if (ctype == cur) ++cur_len;
                else {
                    if (w) runs[n_runs] = (cur << 28) | cur_len;
                    ++n_runs; cur = ctype; cur_len = 1;
                }
                if (ctype != RF_D) --j;
                if (ctype != RF_I) --i;
                if (i == 0 && j == 0) break;
                const int lo = j > 0 ? rf_lo(j, b2) : 0;
                const int end = j + b1 - 1 < len1 ? j + b1 - 1 : len1;
                if (i < 0 || j < 0 || i < lo || i > end || ctype > RF_D) { lost = true; break; }
                qb = __builtin_amdgcn_readfirstlane((uint32_t)tb[(size_t)j * S + (i - lo)]);
                ctype = type;
                type = ctype == RF_M ? (qb & 7u) : ctype == RF_I ? ((qb >> 3) & 3u) : ((qb >> 5) & 3u);
            }
            if (w) runs[n_runs] = (cur << 28) | cur_len;
            ++n_runs;
            __threadfence();                               // lane 0's runs, before every lane reads them
            uint32_t st = HSA_RF_CAP, n_cigar = 0, nm = 0, trim5 = 0, trim3 = 0, md_len = 0;
            if (!lost) {
                // refine_gapped_core's ends (bwtse.c:413-434): the CIGAR is runs[first], runs[first - 1], ...
                int first = (int)n_runs - 1, last = 0;
                const uint32_t r_first = __builtin_amdgcn_readfirstlane(runs[first]), r_last = __builtin_amdgcn_readfirstlane(runs[0]);
                if ((r_first >> 28) == RF_D) { trim5 = r_first & 0x0FFFFFFFu; --first; }
                if (first >= last && (r_last >> 28) == RF_D) { trim3 = r_last & 0x0FFFFFFFu; ++last; }
                n_cigar = (uint32_t)(first - last + 1);
                // bwa_cal_md1's CIGAR branch (:449-477, :491); x, y relative to the window and the read
                MdOut md{a.md + (size_t)a.md_stride * t, a.md_stride, 0u, w};
                uint32_t x = trim5, y = 0, u = 0;
                uint32_t *cg = a.cigar + (size_t)a.cigar_stride * t;
                for (int k = first; k >= last; --k) {
                    const uint32_t run = __builtin_amdgcn_readfirstlane(runs[k]);
                    uint32_t op = run >> 28;
                    const uint32_t l = run & 0x0FFFFFFFu;
                    if (op == RF_I && (k == first || k == last)) op = RF_S;
                    const uint32_t at = (uint32_t)(first - k);
                    if (w && at < a.cigar_stride) cg[at] = (op << 28) | l;
                    if (op == RF_M) {
                        for (uint32_t z = 0; z < l; ++z) {
                            const uint32_t c = __builtin_amdgcn_readfirstlane((uint32_t)refw[x + z]),
                                           s = __builtin_amdgcn_readfirstlane((uint32_t)rd[y + z]);
                            if (s > 3u || c != s) {
                                md.num(u); md.base(c);
                                ++nm; u = 0;
                            } else ++u;
                        }
                        x += l; y += l;
                    } else if (op == RF_I || op == RF_S) {
                        y += l;
                        if (op == RF_I) nm += l;
                    } else {
                        md.num(u); md.put('^');
                        for (uint32_t z = 0; z < l; ++z) md.base(__builtin_amdgcn_readfirstlane((uint32_t)refw[x + z]));
                        u = 0;
                        x += l; nm += l;
                    }
                }
                md.num(u);
                md_len = md.n;
                st = (n_cigar > a.cigar_stride || md_len > a.md_stride) ? HSA_RF_MD : HSA_RF_OK;
            }
            if (w) {
                rf_write_row(a, t, st, n_cigar, nm, md_len, trim5, trim3, r.pos + trim5, r.ori + trim5);
                atomicAdd(&a.ctr[1 + st], 1ull);
            }
        }
    }
}

static TextView text_view(const hsa_index *ix)
{
    TextView v;
    if (ix->d_text64) { v.w = ix->d_text64; v.n = ix->T64; v.lsb = 1u; }
    else { v.w = ix->d_text; v.n = ix->dna_len; v.lsb = 0u; }
    return v;
}

extern "C" int hsa_index_set_text64_device(hsa_index_t *ix, uint32_t *d_text_lsb, uint64_t T)
{
    const char *what = "hsa_index_set_text64_device";
    if (!ix) { hsa_set_error("%s: null handle", what); return HSA_E_ARG; }
    if (!ix->wide) { hsa_set_error("%s: not a 64-bit index (hsa_index_create_device64)", what); return HSA_E_ARG; }
    if (!d_text_lsb) { hsa_set_error("%s: null text", what); return HSA_E_ARG; }
    if (T != ix->T64) {
        hsa_set_error("%s: T %llu is not the index's %llu", what, (unsigned long long)T, (unsigned long long)ix->T64);
        return HSA_E_ARG;
    }
    if (int rc = hsa_need_unshared(ix, what)) return rc;
    HSA_HIP(hipSetDevice(ix->device));
    HSA_HIP(hipStreamSynchronize(ix->stream));     // no kernel reads the old text
    (void)hipFree(ix->d_text64);
    ix->d_text64 = d_text_lsb;
    return 0;
}

static uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1u) / m * m; }

extern "C" int hsa_refine_rows_device64(hsa_index_t *ix, const hsa_refine_batch64_t *b, void *stream)
{
    const char *what = "hsa_refine_rows_device64";
    if (!ix) { hsa_set_error("%s: null handle", what); return HSA_E_ARG; }
    if (!ix->wide) { hsa_set_error("%s: not a 64-bit index (hsa_index_create_device64)", what); return HSA_E_ARG; }
    if (!b || b->n_jobs < 0 || !b->d_counters || b->max_len < 0) { hsa_set_error("%s: bad arguments", what); return HSA_E_ARG; }
    HSA_HIP(hipSetDevice(ix->device));
    return hsa_refine_rows_launch(ix, b, hsa_stage_stream(stream, ix->stream), false, what);
}

// The call's launches on `st`; all_dp: the splicing branch of bwa_refine_gapped
// (bwtse.c:567-574), where every row is aligned whatever its gap count (hsa_splice_rows.hip).
int hsa_refine_rows_launch(hsa_index *ix, const hsa_refine_batch64_t *b, hipStream_t st, bool all_dp, const char *what)
{
    HSA_HIP(hipMemsetAsync(b->d_counters, 0, 8 * sizeof(uint64_t), st));
    if (b->n_jobs == 0 || b->pos_cap == 0) return 0;           // no rows
    if (!b->d_jobs || !b->d_codes || !b->d_hit_off || !b->d_hits || !b->d_pos_off || !b->d_pos || !b->d_pos_hit ||
        !b->d_rows || !b->d_rpos || (b->cigar_stride && !b->d_cigar) || (b->md_stride && !b->d_md)) {
        hsa_set_error("%s: null argument", what);
        return HSA_E_ARG;
    }
    if (b->pos_cap > 0xFFFFFFFFull) { hsa_set_error("%s: more than 2^32 - 1 rows", what); return HSA_E_ARG; }
    const TextView tv = text_view(ix);
    if (!tv.w) {
        hsa_set_error("%s: no text attached (hsa_index_set_text64_device, or hsa_index_set_text under 2^32)", what);
        return HSA_E_ARG;
    }
    if (!tv.lsb && (ix->is64 || ((uint64_t)ix->dna_len + 15u) / 16u > ix->text_words)) {
        hsa_set_error("%s: the packed text does not cover dna_len", what);
        return HSA_E_ARG;
    }
    // the layout.  A traceback row holds the widest band of any window: len1 > len2 gives
    // b1 + b2 + 1 <= 101 + gap columns; a window cut to len1 <= len2 gives min(len1 + 1,
    // len2 - len1 + 101) <= (len2 + 102) / 2.
    const uint32_t max_len = b->max_len > HSA_RF_MAX_LEN ? HSA_RF_MAX_LEN : (uint32_t)(b->max_len ? b->max_len : 1);
    uint32_t width = 101u + HSA_RF_MAX_GAP;
    if ((max_len + 102u) / 2u + 1u > width) width = (max_len + 102u) / 2u + 1u;
    const uint32_t tb_stride = round_up(width, 64u);
    uint32_t ring = 128;
    while (ring < tb_stride + 2u) ring <<= 1;
    const uint32_t win_cap = round_up(max_len + HSA_RF_MAX_GAP, 16u);
    const size_t tb_bytes = ((size_t)(max_len + 1u) * tb_stride + 255u) & ~(size_t)255;
    const size_t wave_bytes = tb_bytes + (((size_t)(2u * max_len + HSA_RF_MAX_GAP + 8u) * 4u + 255u) & ~(size_t)255);
    const size_t lds = (size_t)3 * ring * 4 + win_cap + round_up(max_len, 16u);
    size_t waves = (size_t)(ix->n_cu > 0 ? ix->n_cu : 256) * 8u;
    if (waves * wave_bytes > RF_SCRATCH_BUDGET) waves = RF_SCRATCH_BUDGET / wave_bytes;
    if (waves > b->pos_cap) waves = (size_t)b->pos_cap;
    if (waves < 1) waves = 1;
    RefineArgs A;
    auto layout = [&](Carver c) {
        A.list = c.take<uint32_t>((size_t)b->pos_cap);
        A.wave = c.take<uint8_t>(waves * wave_bytes);
        return c.bytes();
    };
    HSA_TRY(hsa_grow(&ix->d_rf, &ix->d_rf_cap, layout(Carver())));
    layout(Carver(ix->d_rf));
    A.text = tv;
    A.jobs = b->d_jobs; A.n_jobs = (uint32_t)b->n_jobs; A.codes = b->d_codes;
    A.hit_off = b->d_hit_off; A.hits = b->d_hits;
    A.pos_off = b->d_pos_off; A.pos = b->d_pos; A.pos_hit = b->d_pos_hit;
    A.pos_cap = b->pos_cap; A.pos_ctr = b->d_pos_counters;
    A.max_len = max_len; A.cigar_stride = b->cigar_stride; A.md_stride = b->md_stride;
    A.rows = b->d_rows; A.rpos = b->d_rpos; A.cigar = b->d_cigar; A.md = b->d_md;
    A.ctr = (unsigned long long *)b->d_counters;
    A.wave_bytes = wave_bytes; A.tb_bytes = tb_bytes;
    A.tb_stride = tb_stride; A.ring = ring; A.win_cap = win_cap;
    A.all_dp = all_dp ? 1u : 0u;
    hipLaunchKernelGGL(k_refine_rows, dim3((unsigned)((b->pos_cap + 255u) / 256u)), dim3(256), 0, st, A);
    HSA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_refine_dp, dim3((unsigned)waves), dim3(64), lds, st, A);
    HSA_HIP(hipGetLastError());
    return 0;
}
