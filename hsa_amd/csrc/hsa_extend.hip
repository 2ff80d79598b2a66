// hsa_extend.hip -- the splice path's seed extensions, batched.
//
// bwt_splice_match (bwtgap.c:748) grows a mapped seed across the rest of the read
// with bwt_extend_backward / bwt_extend_foreward (bwtgap.c:640-663), which return 1
// (max_pos reached), 2 (moved) or -1.  The search itself -- the stack, one pop and its
// expansion, the exact tail, the rewrite of the hit -- is hsa_ext_search.h, shared with
// the splice kernel (hsa_splice.hip); this file is what is k_extend's own.
//
// Here one lane per call.  The calls of one batch come from many reads (the drop-in
// runs the splice path of every fallback read of a batch as coroutines and hands each
// round of their extension calls to one launch, bwtext_gpu.c); each lane owns a pool of
// entries in HBM and one bucket per score (as gap_stack_t), the buckets' 32-bit heads
// and counts lane-interleaved in LDS, or per lane in HBM when a regime has more than
// EXT_LDS_NB of them.  A call reads its read only inside the window [lo, lo + n) its
// arguments determine (include/hsa_gpu.h); a read outside is reported, never performed.
// The kernel runs the loop around ext_step: the max_entries check before every pop and,
// in sliced mode, the pop budget and the state saved in the call's slot.  The two host
// entry points share their staging (ext_stage / ext_launch / ext_fetch).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsa_device.h"
#include "hsa_ext_search.h"
#include "hsa_internal.h"

#define EXT_NT 64
#define EXT_LDS_NB 128     // buckets per lane kept in LDS: 64 lanes x 128 x 8 B = 64 KiB
// status of a call that could not be completed: ret = EXT_ERR - EXT_E_* (hsa_ext_search.h)
#define EXT_ERR (-1000)
#define EXT_CONT (-999)    // sliced mode: not finished, state saved in its slot
#define EXT_STATE_U4 6     // saved state of a sliced call, in uint4
static_assert(EXT_ERR - EXT_E_CAP == HSA_EXT_E_CAP && EXT_CONT == HSA_EXT_CONT, "include/hsa_gpu.h");

struct ExtArgs {
    RankDir fwd, rev;
    uint32_t T, rT;
    uint32_t C[4];
    const hsa_regime_t *regimes;
    const hsa_ext_job_t *jobs;
    const int32_t *job_list;     // optional: the jobs of a re-run pass
    int n;
    const uint8_t *codes;
    const int32_t *bids;
    uint4 *pool;                 // per lane: cap entries x 2 uint4
    uint32_t *heads, *cnt;       // per lane: nb each
    uint32_t cap, nb;
    uint32_t lds;                // bucket heads and counts in LDS (nb <= EXT_LDS_NB), else in heads/cnt
    uint32_t lnb;                // buckets per lane in the LDS layout
    // sliced mode (hsa_extend_sliced): lane t works on persistent slot slots[t] (its stack
    // and the state below stay in HBM between launches), resumes it when resume[t], and
    // stops after `budget` pops with ret = EXT_CONT
    const int32_t *slots;
    const uint8_t *resume;
    uint32_t budget;
    uint4 *state;                // per slot: EXT_STATE_U4 uint4
    int32_t *ret, *mp_out;
    uint32_t *aln_out;           // 9 words per job
};

// What ext_step (hsa_ext_search.h) needs from a call of k_extend: the read through the
// call's window, every score its own bucket, the hit in registers.
struct ExtCtx {
    const ExtArgs &a;
    const hsa_regime_t &R;
    ExtStack<ExtBuckets32> stk;
    ExtCall call;
    const uint8_t *sq;
    const int32_t *bd;
    int lo, hi;
    uint32_t aln[9];
    __device__ __forceinline__ uint32_t seq_at(int p)
    {
        if (p < lo || p >= hi) { stk.err = EXT_E_WIN; return 4u; }
        return sq[p - lo];
    }
    __device__ __forceinline__ int bid_at(int p)
    {
        if (p < lo || p >= hi) { stk.err = EXT_E_WIN; return 0; }
        return bd[p - lo];
    }
    __device__ __forceinline__ int bucket(int score) const { return score; }
    __device__ __forceinline__ uint32_t &hit(int w) { return aln[w]; }
};

__global__ void __launch_bounds__(EXT_NT) k_extend(ExtArgs a)
{
    const int t = blockIdx.x * EXT_NT + threadIdx.x;
    if (t >= a.n) return;
    const int jb = a.job_list ? a.job_list[t] : t;
    const hsa_ext_job_t J = a.jobs[jb];
    const hsa_regime_t R = a.regimes[J.regime];
    const size_t sl = a.slots ? (size_t)a.slots[t] : (size_t)t;   // the lane's stack region
    const bool resume = a.resume && a.resume[t];
    ExtCtx x{a, R};
    ExtStack<ExtBuckets32> &K = x.stk;
    K.P = a.pool + sl * a.cap * 2;
    K.cap = a.cap;
    K.nb = R.n_stacks;
    // bucket heads and counts (gap_stack_t's per-score stacks): lane-interleaved in LDS,
    // or per lane in HBM when there are too many buckets
    extern __shared__ uint32_t s_hn[];
    uint32_t *const gH = a.heads + sl * a.nb, *const gN = a.cnt + sl * a.nb;
    K.bk.H = a.lds ? s_hn + threadIdx.x : gH;
    K.bk.N = a.lds ? s_hn + (size_t)a.lnb * EXT_NT + threadIdx.x : gN;
    K.bk.hs = a.lds ? EXT_NT : 1u;
    x.lo = J.lo;
    x.hi = J.lo + J.n;
    x.sq = a.codes + J.off;
    x.bd = a.bids + J.off;
#pragma unroll
    for (int w = 0; w < 9; ++w) x.aln[w] = J.aln[w];
    x.call.set(J.dir, J.len, (int)J.aln[6], (int)J.aln[7], J.max_pos, R.max_diff, R.mode, R);
    // sliced mode keeps the slot's heads, counts and state in HBM between launches; with
    // the bookkeeping in LDS the heads and counts are copied in on resume and out when
    // the call pauses
    uint4 *const S = a.state ? a.state + sl * EXT_STATE_U4 : nullptr;
    if (resume) {
        if (a.lds)
            for (int b = 0; b < K.nb; ++b) {
                K.bk.H[(uint32_t)b * K.bk.hs] = gH[b];
                K.bk.N[(uint32_t)b * K.bk.hs] = gN[b];
            }
        const uint4 s0 = S[0], s1 = S[1];
        K.err = 0;
        K.best = (int)s0.x; K.n_ent = (int)s0.y; K.top = s0.z; K.freel = s0.w;
        K.pend = s1.x != 0; K.pscore = (int)s1.y; x.call.max_pos = (int)s1.z;
        K.pe0 = S[2]; K.pe1 = S[3];
        const uint4 a0 = S[4], a1 = S[5];
        x.aln[0] = a0.x; x.aln[1] = a0.y; x.aln[2] = a0.z; x.aln[3] = a0.w;
        x.aln[4] = a1.x; x.aln[5] = a1.y; x.aln[6] = a1.z; x.aln[7] = a1.w; x.aln[8] = s1.w;
    } else {
        K.reset();
        ext_push_hit(x);
    }
    uint32_t pops = 0;
    bool cont = false;
    bool go = K.n_ent != 0 && !K.err;          // ext_step is false once the search ended or met an error
    while (go) {
        if (a.budget && pops == a.budget) { cont = true; break; }
        ++pops;
        if (K.n_ent > R.max_entries) break;
        go = ext_step(x) && K.n_ent != 0;
    }
    const int max_pos = x.call.max_pos;
    int ret = x.call.ret;
    if (K.err) ret = EXT_ERR - K.err;
    else if (cont) {
        ret = EXT_CONT;
        if (a.lds)
            for (int b = 0; b < K.nb; ++b) {
                gH[b] = K.bk.H[(uint32_t)b * K.bk.hs];
                gN[b] = K.bk.N[(uint32_t)b * K.bk.hs];
            }
        S[0] = make_uint4((uint32_t)K.best, (uint32_t)K.n_ent, K.top, K.freel);
        S[1] = make_uint4(K.pend ? 1u : 0u, (uint32_t)K.pscore, (uint32_t)max_pos, x.aln[8]);
        S[2] = K.pe0; S[3] = K.pe1;
        S[4] = make_uint4(x.aln[0], x.aln[1], x.aln[2], x.aln[3]);
        S[5] = make_uint4(x.aln[4], x.aln[5], x.aln[6], x.aln[7]);
    } else if (ret != 1) ret = max_pos != J.max_pos ? 2 : -1;
    a.ret[jb] = ret;
    a.mp_out[jb] = max_pos;
#pragma unroll
    for (int w = 0; w < 9; ++w) a.aln_out[(size_t)jb * 9 + w] = x.aln[w];
}

// Device scratch of one pass: lanes x (cap entries x 32 B + nb x 8 B).
static int ext_scratch(hsa_index_t *ix, size_t lanes, uint32_t cap, uint32_t nb, uint4 **pool, uint32_t **heads,
                       uint32_t **cnt)
{
    const size_t pb = lanes * cap * 32, hb = lanes * nb * 4;
    int rc = hsa_grow(&ix->d_ext, &ix->d_ext_cap, pb + 2 * hb + 256);
    if (rc) return rc;
    *pool = (uint4 *)ix->d_ext;
    *heads = (uint32_t *)((char *)ix->d_ext + pb);
    *cnt = (uint32_t *)((char *)ix->d_ext + pb + hb);
    return 0;
}

// What hsa_extend_batch and hsa_extend_sliced stage alike: regimes | jobs | codes | bids
// uploaded into d_in, with `own` bytes behind them for the caller's own lists (*d_own);
// ret | max_pos | aln laid out in d_out; and the fields of A that follow from these and
// from the index.  The stack, job_list / n and the sliced fields (left null) are the
// caller's.
static int ext_stage(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const hsa_ext_job_t *jobs, int n,
                     const uint8_t *codes, const int32_t *bids, size_t win_len, size_t own, ExtArgs &A, char **d_own)
{
    HSA_HIP(hipSetDevice(ix->device));
    ix->staged_valid = 0;                      // d_in is reused below
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t rb = (size_t)n_regimes * sizeof(hsa_regime_t), jbb = (size_t)n * sizeof(hsa_ext_job_t);
    const size_t o_jobs = al(rb), o_codes = o_jobs + al(jbb), o_bids = o_codes + al(win_len);
    const size_t o_own = o_bids + al(win_len * 4);
    const size_t o_mp = al((size_t)n * 4), o_aln = 2 * o_mp;
    int rc;
    if ((rc = hsa_grow(&ix->d_in, &ix->d_in_cap, o_own + own + 256)) ||
        (rc = hsa_grow(&ix->d_out, &ix->d_out_cap, o_aln + (size_t)n * 36 + 256)))
        return rc;
    char *din = (char *)ix->d_in, *dout = (char *)ix->d_out;
    HSA_HIP(hipMemcpyAsync(din, regimes, rb, hipMemcpyHostToDevice, ix->stream));
    HSA_HIP(hipMemcpyAsync(din + o_jobs, jobs, jbb, hipMemcpyHostToDevice, ix->stream));
    if (win_len) {
        HSA_HIP(hipMemcpyAsync(din + o_codes, codes, win_len, hipMemcpyHostToDevice, ix->stream));
        HSA_HIP(hipMemcpyAsync(din + o_bids, bids, win_len * 4, hipMemcpyHostToDevice, ix->stream));
    }
    *d_own = din + o_own;
    A = ExtArgs{};
    A.fwd = RankDir{ix->blk[0], ix->isa0};
    A.rev = RankDir{ix->blk[1], ix->risa0};
    A.T = ix->T; A.rT = ix->rT;
    memcpy(A.C, ix->C, sizeof A.C);
    A.regimes = (const hsa_regime_t *)din;
    A.jobs = (const hsa_ext_job_t *)(din + o_jobs);
    A.codes = (const uint8_t *)(din + o_codes);
    A.bids = (const int32_t *)(din + o_bids);
    A.ret = (int32_t *)dout;
    A.mp_out = (int32_t *)(dout + o_mp);
    A.aln_out = (uint32_t *)(dout + o_aln);
    A.lnb = 1;
    for (int r = 0; r < n_regimes; ++r) A.lnb = (uint32_t)regimes[r].n_stacks > A.lnb ? (uint32_t)regimes[r].n_stacks : A.lnb;
    A.lds = A.lnb <= EXT_LDS_NB;
    return 0;
}

static int ext_launch(hsa_index_t *ix, const ExtArgs &A)
{
    const size_t shm = A.lds ? (size_t)A.lnb * EXT_NT * 8 : 0;
    hipLaunchKernelGGL(k_extend, dim3((unsigned)((A.n + EXT_NT - 1) / EXT_NT)), dim3(EXT_NT), shm, ix->stream, A);
    HSA_HIP(hipGetLastError());
    return 0;
}

// the results of A's jobs to the host (a null destination is skipped)
static int ext_fetch(hsa_index_t *ix, const ExtArgs &A, int n, int32_t *ret, int32_t *max_pos, uint32_t *aln_out)
{
    if (ret) HSA_HIP(hipMemcpyAsync(ret, A.ret, (size_t)n * 4, hipMemcpyDeviceToHost, ix->stream));
    if (max_pos) HSA_HIP(hipMemcpyAsync(max_pos, A.mp_out, (size_t)n * 4, hipMemcpyDeviceToHost, ix->stream));
    if (aln_out) HSA_HIP(hipMemcpyAsync(aln_out, A.aln_out, (size_t)n * 36, hipMemcpyDeviceToHost, ix->stream));
    HSA_HIP(hipStreamSynchronize(ix->stream));
    return 0;
}

extern "C" int hsa_extend_batch(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const hsa_ext_job_t *jobs,
                                int n, const uint8_t *codes, const int32_t *bids, size_t win_len, int32_t *ret,
                                int32_t *max_pos, uint32_t *aln_out)
{
    if (n < 0 || n_regimes < 1 || (n > 0 && (!jobs || !regimes || !ret || !max_pos || !aln_out))) {
        hsa_set_error("hsa_extend_batch: bad arguments");
        return HSA_E_ARG;
    }
    if (n == 0) return 0;
    if (int rc0 = hsa_need32(ix)) return rc0;
    uint32_t nb = 1;
    int max_entries = 0;
    for (int r = 0; r < n_regimes; ++r) {
        if (regimes[r].n_stacks < 1 || regimes[r].n_stacks > 4096) {
            hsa_set_error("hsa_extend_batch: regime %d: n_stacks %d outside 1..4096", r, regimes[r].n_stacks);
            return HSA_E_ARG;
        }
        nb = (uint32_t)regimes[r].n_stacks > nb ? (uint32_t)regimes[r].n_stacks : nb;
        max_entries = regimes[r].max_entries > max_entries ? regimes[r].max_entries : max_entries;
    }
    for (int j = 0; j < n; ++j) {
        const hsa_ext_job_t &J = jobs[j];
        if (J.regime < 0 || J.regime >= n_regimes || J.n < 0 || (J.n > 0 && J.off + (uint64_t)J.n > win_len) ||
            (J.dir != 0 && J.dir != 1)) {
            hsa_set_error("hsa_extend_batch: call %d: bad job (regime %d, window %d at %llu of %zu)", j, J.regime, J.n,
                          (unsigned long long)J.off, win_len);
            return HSA_E_ARG;
        }
    }
    ExtArgs A;
    char *d_list;
    int rc;
    if ((rc = ext_stage(ix, regimes, n_regimes, jobs, n, codes, bids, win_len, (size_t)n * 4, A, &d_list))) return rc;
    A.nb = nb;
    // capacity passes: every call with a small stack, then the calls that overflowed it
    // with larger ones, up to what the reference's max_entries bound allows (live entries
    // <= max_entries + 9: the check precedes the pop, bwtgap.c:374)
    const uint32_t caps[3] = {256u, 65536u, (uint32_t)max_entries + 16u};
    const size_t budget = (size_t)8 << 30;     // scratch bytes per launch
    int32_t *list = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
    int n_run = n;
    for (int j = 0; j < n; ++j) list[j] = j;
    for (int pass = 0; pass < 3 && n_run > 0; ++pass) {
        const uint32_t cap = caps[pass];
        const size_t per = (size_t)cap * 32 + (size_t)nb * 8;
        const size_t chunk = budget / per > 0 ? budget / per : 1;
        HSA_HIP(hipMemcpyAsync(d_list, list, (size_t)n_run * 4, hipMemcpyHostToDevice, ix->stream));
        for (size_t c0 = 0; c0 < (size_t)n_run; c0 += chunk) {
            const size_t m = (size_t)n_run - c0 < chunk ? (size_t)n_run - c0 : chunk;
            if ((rc = ext_scratch(ix, m, cap, nb, &A.pool, &A.heads, &A.cnt))) { free(list); return rc; }
            A.cap = cap;
            A.job_list = (const int32_t *)d_list + c0;
            A.n = (int)m;
            if ((rc = ext_launch(ix, A))) { free(list); return rc; }
        }
        if ((rc = ext_fetch(ix, A, n, ret, nullptr, nullptr))) { free(list); return rc; }
        int k = 0;
        for (int t = 0; t < n_run; ++t)
            if (ret[list[t]] == EXT_ERR - EXT_E_CAP) list[k++] = list[t];
        n_run = k;
    }
    free(list);
    if ((rc = ext_fetch(ix, A, n, nullptr, max_pos, aln_out))) return rc;
    for (int j = 0; j < n; ++j) {
        if (ret[j] > EXT_ERR) continue;
        static const char *why[5] = {"", "stack capacity", "a score outside the stack's buckets",
                                     "a rank position past the text", "a read position outside the call's window"};
        const int e = EXT_ERR - ret[j];
        hsa_set_error("hsa_extend_batch: call %d needs %s (undefined in the reference or past max_entries)", j,
                      e >= 1 && e <= 4 ? why[e] : "?");
        return HSA_E_ARG;
    }
    return 0;
}

// ---------------------------------------------------------------- sliced mode
// The splice runner's calls (bwtext_gpu.c) come in rounds from coroutines that wait on
// them; one long search would hold every other read's next round.  So each launch runs
// every call in flight for at most `budget` pops: a call that finishes returns its
// result, one that does not keeps its stack and state in its slot (HBM, persistent
// across launches) and is resumed by the next launch, while the coroutines whose calls
// finished go on.  Slots hold EXT_SLICE_CAP entries and EXT_SLICE_NB buckets; a call
// that needs more reports EXT_E_CAP / EXT_E_SCORE here and is re-run by the caller
// through hsa_extend_batch.
#define EXT_SLICE_CAP 2048u
#define EXT_SLICE_NB ((uint32_t)HSA_EXT_SLICE_STACKS)

extern "C" int hsa_extend_sliced(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const hsa_ext_job_t *jobs,
                                 const int32_t *slots, const uint8_t *resume, int n, const uint8_t *codes,
                                 const int32_t *bids, size_t win_len, int n_slots, uint32_t budget, int32_t *ret,
                                 int32_t *max_pos, uint32_t *aln_out)
{
    if (n < 0 || n_regimes < 1 || n_slots < 1 || (n > 0 && (!jobs || !regimes || !slots || !resume || !ret ||
                                                           !max_pos || !aln_out))) {
        hsa_set_error("hsa_extend_sliced: bad arguments");
        return HSA_E_ARG;
    }
    if (n == 0) return 0;
    if (int rc0 = hsa_need32(ix)) return rc0;
    for (int r = 0; r < n_regimes; ++r)
        if (regimes[r].n_stacks < 1 || regimes[r].n_stacks > (int)EXT_SLICE_NB) {
            hsa_set_error("hsa_extend_sliced: regime %d: n_stacks %d outside 1..%u", r, regimes[r].n_stacks,
                          EXT_SLICE_NB);
            return HSA_E_ARG;
        }
    for (int j = 0; j < n; ++j) {
        const hsa_ext_job_t &J = jobs[j];
        if (J.regime < 0 || J.regime >= n_regimes || J.n < 0 || (J.n > 0 && J.off + (uint64_t)J.n > win_len) ||
            (J.dir != 0 && J.dir != 1) || slots[j] < 0 || slots[j] >= n_slots) {
            hsa_set_error("hsa_extend_sliced: call %d: bad job", j);
            return HSA_E_ARG;
        }
    }
    // the launch's own lists behind the common inputs: slots, then the resume flags
    const size_t o_res = ((size_t)n * 4 + 255) / 256 * 256;
    ExtArgs A;
    char *d_own;
    int rc;
    if ((rc = ext_stage(ix, regimes, n_regimes, jobs, n, codes, bids, win_len, o_res + (size_t)n, A, &d_own))) return rc;
    HSA_HIP(hipMemcpyAsync(d_own, slots, (size_t)n * 4, hipMemcpyHostToDevice, ix->stream));
    HSA_HIP(hipMemcpyAsync(d_own + o_res, resume, (size_t)n, hipMemcpyHostToDevice, ix->stream));
    A.slots = (const int32_t *)d_own;
    A.resume = (const uint8_t *)(d_own + o_res);
    A.budget = budget;
    // persistent slots: stacks, bucket heads and counts, state (grown, never shrunk:
    // contents survive between calls with the same n_slots)
    const size_t pb = (size_t)n_slots * EXT_SLICE_CAP * 32, hb = (size_t)n_slots * EXT_SLICE_NB * 4;
    const size_t sb = (size_t)n_slots * EXT_STATE_U4 * 16;
    if ((rc = hsa_grow(&ix->d_slices, &ix->d_slices_cap, pb + 2 * hb + sb + 256))) return rc;
    A.pool = (uint4 *)ix->d_slices;
    A.heads = (uint32_t *)((char *)ix->d_slices + pb);
    A.cnt = (uint32_t *)((char *)ix->d_slices + pb + hb);
    A.state = (uint4 *)((char *)ix->d_slices + pb + 2 * hb);
    A.cap = EXT_SLICE_CAP;
    A.nb = EXT_SLICE_NB;
    A.n = n;
    static const bool trace = getenv("HSA_EXT_TRACE") != nullptr;
    if (trace) {
        HSA_HIP(hipStreamSynchronize(ix->stream));
        HSA_HIP(hipEventRecord(ix->ev0, ix->stream));
    }
    if ((rc = ext_launch(ix, A))) return rc;
    if (trace) {
        HSA_HIP(hipEventRecord(ix->ev1, ix->stream));
        HSA_HIP(hipEventSynchronize(ix->ev1));
        float ms = 0.f;
        HSA_HIP(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
        fprintf(stderr, "[hsa_extend_sliced] %d calls, %zu window bytes, kernel %.3f ms\n", n, win_len, ms);
    }
    return ext_fetch(ix, A, n, ret, max_pos, aln_out);
}
