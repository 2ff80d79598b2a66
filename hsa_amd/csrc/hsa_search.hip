// hsa_search.hip -- the 32-bit search API (include/hsa_gpu.h): host-array and
// device-resident batches, direct bwt_match_gap calls; the kernels are in
// hsa_search_kernels.h, their planning and launching in hsa_search_launch.h, the splice
// path's seeds and prefetch (entry points included) in hsa_splice_prefetch.h.
#include "hsa_search_launch.h"
#include "hsa_splice_prefetch.h"

#include <memory>
#include <vector>

#ifdef HSA_DIAG
extern "C" int hsa_diag_read(unsigned long long *out, int n_blocks)
{
    HSA_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag), sizeof(unsigned long long) * 4 * (size_t)n_blocks));
    return 0;
}
extern "C" int hsa_diag_counters(unsigned long long *out, int reset)
{
    HSA_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dctr), sizeof(unsigned long long) * 32));
    if (reset) {
        unsigned long long z[32] = {0};
        HSA_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_dctr), z, sizeof z));
    }
    return 0;
}
#endif

struct MgHost {
    const hsa_mg_job_t *mg;
    const int32_t *widths;
    size_t width_pairs;
    int32_t *widths_out;
};

// A host-array batch, and where its answers go (the C ABI's arrays).
struct HostIn {
    const hsa_job_t *jobs;
    int n;
    const uint8_t *codes;
    size_t codes_len;
    const MgHost *mh;              // caller widths (hsa_match_gap_batch), or null
};

struct HostOut {
    int32_t *n_aln;
    uint32_t *flags;
    uint64_t *hit_off;
    uint32_t **hits;               // malloc'ed: the caller frees it
    hsa_stats_t *stats;
};

// Owners that let every early return (HSA_HIP) free what it holds.
using HostHits = std::unique_ptr<uint32_t, void (*)(void *)>;   // hit records until they go to HostOut::hits
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

static HostHits alloc_hits(uint64_t records)
{
    HostHits h((uint32_t *)malloc((records + 1) * 36), free);
    if (!h) hsa_set_error("host allocation of %llu hits failed", (unsigned long long)records);
    return h;
}

// Checks of a caller-width batch; max_seed = the longest own width_seed.  A width_seed
// with seed_len > len makes the reference read outside it: refused.
static int mg_limits(const hsa_job_t *jobs, const hsa_mg_job_t *mg, int n, const MgHost &mh, int &max_seed)
{
    max_seed = 0;
    for (int j = 0; j < n; ++j) {
        const hsa_mg_job_t &M = mg[j];
        const uint32_t len = jobs[j].len;
        if (M.strand != 0 && M.strand != 1) { hsa_set_error("call %d: strand %d", j, M.strand); return HSA_E_ARG; }
        if (M.seed < HSA_SEED_NONE || M.seed > HSA_SEED_ALIAS) { hsa_set_error("call %d: seed kind", j); return HSA_E_ARG; }
        if (M.seed != HSA_SEED_NONE && (jobs[j].seed_len < 0 || jobs[j].seed_len > (int)len)) {
            hsa_set_error("call %d: width_seed with seed_len %d outside [0, len %u] (undefined in the reference)", j,
                          jobs[j].seed_len, len);
            return HSA_E_ARG;
        }
        if (M.wb_off + len + 1 > mh.width_pairs ||
            (M.seed == HSA_SEED_OWN && M.ws_off + (uint64_t)jobs[j].seed_len + 1 > mh.width_pairs)) {
            hsa_set_error("call %d: widths outside the width array", j);
            return HSA_E_ARG;
        }
        for (uint32_t t = 0; t <= len; ++t)
            if (mh.widths[2 * (M.wb_off + t) + 1] < 0) { hsa_set_error("call %d: negative bid", j); return HSA_E_ARG; }
        if (M.seed == HSA_SEED_OWN) {
            for (int t = 0; t <= jobs[j].seed_len; ++t)
                if (mh.widths[2 * (M.ws_off + t) + 1] < 0) { hsa_set_error("call %d: negative bid", j); return HSA_E_ARG; }
            if (jobs[j].seed_len > max_seed) max_seed = jobs[j].seed_len;
        }
    }
    return 0;
}

// A host batch on the device.  Inputs in ix->d_in: [regimes + bucket maps (1536) | jobs |
// job list | codes | mg jobs | caller widths]; outputs in ix->d_out: [n_aln | flags |
// hit_off | hits]; counters ix->d_ctr.  io.list, io.max_len and io.max_seed are the caller's.
struct HostStage {
    PassIO io;
    int32_t *d_list;               // the job list slot (k_search's layout only)
    int nb;                        // stack buckets (k_search's layout: stage_regimes)
};

// regimes: k_search's layout, the regimes staged with it (always copied: the call may
// have moved d_in); codes padded by 1, a job list slot, room for 4 hits per read.
// null: k_search_any's (the regimes are any_prepare's; a moved d_in invalidates the
// fast path's staging); codes padded by 64, no list, room for 64 hits per read.
static int stage_host(hsa_index *ix, const HostIn &in, const hsa_regime_t *regimes, int n_regimes, hipStream_t st,
                      HostStage &H)
{
    const bool fast = regimes != nullptr;
    const size_t n = (size_t)in.n;
    const MgHost *mh = in.mh;
    const size_t o_jobs = 1536, o_list = o_jobs + al(n * sizeof(hsa_job_t)), o_codes = o_list + (fast ? al(n * 4) : 0);
    const size_t o_mg = o_codes + al(in.codes_len + (fast ? 1 : 64)), o_cw = o_mg + (mh ? al(n * sizeof(hsa_mg_job_t)) : 0);
    const size_t cw_bytes = mh ? mh->width_pairs * 8 : 0;
    void *before = ix->d_in;
    int rc = hsa_grow(&ix->d_in, &ix->d_in_cap, o_cw + cw_bytes + 256);
    if (rc) return rc;
    char *din = (char *)ix->d_in;
    H.nb = 0;
    if (fast && (rc = stage_regimes(ix, regimes, n_regimes, H.nb, st, true))) return rc;
    if (!fast && before != ix->d_in) ix->staged_valid = 0;
    HSA_HIP(hipMemcpyAsync(din + o_jobs, in.jobs, sizeof(hsa_job_t) * n, hipMemcpyHostToDevice, st));
    HSA_HIP(hipMemcpyAsync(din + o_codes, in.codes, in.codes_len, hipMemcpyHostToDevice, st));
    if (mh) {
        HSA_HIP(hipMemcpyAsync(din + o_mg, mh->mg, sizeof(hsa_mg_job_t) * n, hipMemcpyHostToDevice, st));
        HSA_HIP(hipMemcpyAsync(din + o_cw, mh->widths, cw_bytes, hipMemcpyHostToDevice, st));
    }
    H.d_list = (int32_t *)(din + o_list);
    const uint64_t hit_cap = fast ? (uint64_t)n * 4 + 4096 : (uint64_t)n * 64 + 65536;
    const size_t o_fl = al(n * 4), o_ho = o_fl + al(n * 4), o_hits = o_ho + al(n * 8);
    if ((rc = hsa_grow(&ix->d_out, &ix->d_out_cap, o_hits + hit_cap * 36 + 256))) return rc;
    char *dout = (char *)ix->d_out;
    H.io = PassIO{.jobs = (const hsa_job_t *)(din + o_jobs), .list = nullptr, .n = in.n,
                  .codes = (const uint8_t *)(din + o_codes), .n_aln = (int32_t *)dout, .flags = (uint32_t *)(dout + o_fl),
                  .hit_off = (uint64_t *)(dout + o_ho), .hits = (uint32_t *)(dout + o_hits), .hit_cap = hit_cap,
                  .ctr = (unsigned long long *)ix->d_ctr, .max_len = 0, .max_seed = 0,
                  .mg = mh ? MgPass{(const hsa_mg_job_t *)(din + o_mg), (int32_t *)(din + o_cw)} : MgPass{}};
    return 0;
}

// The counters and the per-job arrays of a pass (n entries each) to the host, complete on return.
static int copy_back(const PassIO &io, int n, const HostOut &to, unsigned long long *ctr, hipStream_t st)
{
    HSA_HIP(hipMemcpyAsync(ctr, io.ctr, CTR_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HSA_HIP(hipMemcpyAsync(to.n_aln, io.n_aln, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HSA_HIP(hipMemcpyAsync(to.flags, io.flags, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HSA_HIP(hipMemcpyAsync(to.hit_off, io.hit_off, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HSA_HIP(hipStreamSynchronize(st));
    return 0;
}

// width_back of every call after its search (k_widths_export wrote them in place)
static int export_widths(const HostIn &in, const HostStage &H)
{
    const MgHost *mh = in.mh;
    std::vector<int32_t> cw(2 * mh->width_pairs + 2);
    HSA_HIP(hipMemcpy(cw.data(), H.io.mg.d_cw, mh->width_pairs * 8, hipMemcpyDeviceToHost));
    for (int j = 0; j < in.n; ++j)
        memcpy(mh->widths_out + 2 * mh->mg[j].wb_off, cw.data() + 2 * mh->mg[j].wb_off, 8 * ((size_t)in.jobs[j].len + 1));
    return 0;
}

// main: the batch's first pass (a re-run round adds to the work and the kernel time only)
static void add_stats(hsa_stats_t *stats, const unsigned long long *ctr, float ms, bool main)
{
    if (!stats) return;
    stats->rank_queries += ctr[CTR_RANK]; stats->blocks_loaded += ctr[CTR_SECTORS]; stats->pops += ctr[CTR_POPS];
    stats->kernel_ms += ms;
    if (main) { stats->main_kernel_ms += ms; stats->main_launches += 1; }
}

// k_search_any over host arrays (hsa_search_any.h): reads longer than k_search holds,
// or every read of a regime outside its layouts.  Same outputs as search_batch_impl.
static long search_any_host(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const HostIn &in,
                            const HostOut &out)
{
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = ix->stream;
    const hsa_job_t *jobs = in.jobs;
    uint32_t max_len = 1, max_seed = 0;
    for (int j = 0; j < in.n; ++j) {
        if (jobs[j].len > max_len) max_len = jobs[j].len;
        const bool own = in.mh ? in.mh->mg[j].seed == HSA_SEED_OWN : (int)jobs[j].len > jobs[j].seed_len;
        if (own && (uint32_t)jobs[j].seed_len > max_seed) max_seed = (uint32_t)jobs[j].seed_len;
    }
    AnyBufs AB;
    int rc = any_prepare(ix, regimes, n_regimes, (size_t)in.n, st, AB);
    if (rc) return rc;
    HostStage H;
    if ((rc = stage_host(ix, in, nullptr, 0, st, H))) return rc;
    H.io.max_len = (int)max_len; H.io.max_seed = (int)max_seed;
    HSA_HIP(hipMemsetAsync(H.io.ctr, 0, CTR_SLOTS * sizeof(unsigned long long), st));
    HSA_HIP(hipEventRecord(ix->ev0, st));
    if ((rc = any_passes<uint32_t>(ix, AB, H.io, nullptr, st))) return rc;
    HSA_HIP(hipEventRecord(ix->ev1, st));
    unsigned long long ctr[CTR_SLOTS];
    if ((rc = copy_back(H.io, in.n, out, ctr, st))) return rc;
    if (ctr[CTR_ERRORS]) { hsa_set_error("%llu reads pushed a score past the regime's n_stacks", ctr[CTR_ERRORS]); return HSA_E_ARG; }
    if (ctr[CTR_UNFINISHED]) { hsa_set_error("%llu reads exceed the large-pass capacity", ctr[CTR_UNFINISHED]); return HSA_E_ARG; }
    float ms = 0;
    HSA_HIP(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    const uint64_t total = ctr[CTR_HITS] < H.io.hit_cap ? ctr[CTR_HITS] : H.io.hit_cap;
    HostHits h = alloc_hits(total);
    if (!h) return HSA_E_MEM;
    if (total) HSA_HIP(hipMemcpy(h.get(), H.io.hits, total * 36, hipMemcpyDeviceToHost));
    if (in.mh && (rc = export_widths(in, H))) return rc;
    add_stats(out.stats, ctr, ms, true);
    *out.hits = h.release();
    return (long)total;
}

static long search_batch_impl(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const HostIn &in,
                              const HostOut &out);

// A batch with reads (or a regime) k_search cannot hold: the reads it can hold through
// search_batch_impl, the others through k_search_any; outputs merged in job order.
static long search_split(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const HostIn &in, const HostOut &out,
                         bool fast_rg)
{
    const MgHost *mh = in.mh;
    hsa_stats_t *stats = out.stats;
    std::vector<int> part[2];                        // 0: k_search, 1: k_search_any
    for (int j = 0; j < in.n; ++j) part[fast_rg && in.jobs[j].len <= FAST_MAX_LEN ? 0 : 1].push_back(j);
    HostHits hs[2] = {HostHits(nullptr, free), HostHits(nullptr, free)};
    long tot[2] = {0, 0};
    if (stats) memset(stats, 0, sizeof *stats);
    for (int k = 0; k < 2; ++k) {
        const int m = (int)part[k].size();
        if (m == 0) continue;
        std::vector<hsa_job_t> pj(m);
        std::vector<hsa_mg_job_t> pm(mh ? m : 0);
        for (int q = 0; q < m; ++q) {
            pj[q] = in.jobs[part[k][q]];
            if (mh) pm[q] = mh->mg[part[k][q]];
        }
        const MgHost pmh = mh ? MgHost{pm.data(), mh->widths, mh->width_pairs, mh->widths_out} : MgHost{};
        std::vector<int32_t> na(m);
        std::vector<uint32_t> fl(m);
        std::vector<uint64_t> ho(m);
        hsa_stats_t ps{};
        uint32_t *ph = nullptr;
        const HostIn pin{pj.data(), m, in.codes, in.codes_len, mh ? &pmh : nullptr};
        const HostOut pout{na.data(), fl.data(), ho.data(), &ph, &ps};
        const long t = k == 0 ? search_batch_impl(ix, regimes, n_regimes, pin, pout)
                              : search_any_host(ix, regimes, n_regimes, pin, pout);
        hs[k].reset(ph);
        if (t < 0) return t;
        tot[k] = t;
        for (int q = 0; q < m; ++q) {
            const int j = part[k][q];
            out.n_aln[j] = na[q]; out.flags[j] = fl[q]; out.hit_off[j] = ho[q] + (k ? (uint64_t)tot[0] : 0);
        }
        if (stats) {
            stats->rank_queries += ps.rank_queries; stats->blocks_loaded += ps.blocks_loaded; stats->pops += ps.pops;
            stats->overflow_reruns += ps.overflow_reruns; stats->kernel_ms += ps.kernel_ms;
            stats->main_kernel_ms += ps.main_kernel_ms; stats->main_launches += ps.main_launches;
        }
    }
    HostHits h = alloc_hits((uint64_t)tot[0] + (uint64_t)tot[1]);
    if (!h) return HSA_E_MEM;
    if (tot[0]) memcpy(h.get(), hs[0].get(), (size_t)tot[0] * 36);
    if (tot[1]) memcpy(h.get() + (size_t)tot[0] * 9, hs[1].get(), (size_t)tot[1] * 36);
    *out.hits = h.release();
    return tot[0] + tot[1];
}

static long search_batch_impl(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const HostIn &in,
                              const HostOut &out)
{
    const hsa_job_t *jobs = in.jobs;
    const int n_jobs = in.n;
    const size_t codes_len = in.codes_len;
    const MgHost *mh = in.mh;
    hsa_stats_t *stats = out.stats;
    *out.hits = nullptr;
    if (n_regimes < 1 || n_regimes > 2) { hsa_set_error("1 or 2 regimes"); return HSA_E_ARG; }
    if (int rc0 = hsa_need32(ix)) return rc0;
    int rc = check_regimes(regimes, n_regimes);
    if (rc) return rc;
    int max_len, max_seed;
    if ((rc = jobs_limits(jobs, n_jobs, max_len, max_seed))) return rc;
    if (mh && (rc = mg_limits(jobs, mh->mg, n_jobs, *mh, max_seed))) return rc;
    if (codes_len >= 0xFFFFFFFFull) { hsa_set_error("read codes of one call must be < 4 GiB"); return HSA_E_ARG; }
    HSA_HIP(hipSetDevice(ix->device));      // before any split: both halves allocate on ix's device
    for (int j = 0; j < n_jobs; ++j)        // the kernels read codes[off, off + len) of every job
        if (jobs[j].off > codes_len || jobs[j].len > codes_len - jobs[j].off) {
            hsa_set_error("job %d: codes [%llu, +%u) past codes_len %zu", j, (unsigned long long)jobs[j].off,
                          jobs[j].len, codes_len);
            return HSA_E_ARG;
        }
    const bool fast_rg = fast_regimes(regimes, n_regimes);
    bool all_fit = fast_rg;
    for (int j = 0; j < n_jobs && all_fit; ++j) all_fit = jobs[j].len <= FAST_MAX_LEN;
    if (!all_fit) return search_split(ix, regimes, n_regimes, in, out, fast_rg);
    hipStream_t st = ix->stream;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_jobs == 0) { *out.hits = (uint32_t *)calloc(9, 4); return 0; }
    static const bool verbose = getenv("HSA_VERBOSE") != nullptr;
    const auto now = []() { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; };
    const double tv0 = verbose ? now() : 0.0;

    HostStage H;
    if ((rc = stage_host(ix, in, regimes, n_regimes, st, H))) return rc;
    H.io.max_len = max_len; H.io.max_seed = max_seed;
    LaunchPlan P;
    RegimePlan R = regime_plan(regimes, n_regimes);
    R.nb = H.nb;
    R.nib_ok = R.nib_ok && !mh;
    R.snib_ok = R.snib_ok && !mh;            // caller widths (k_widths_import): byte rows
    for (int j = 0; j < n_jobs && R.nib_ok; ++j) R.nib_ok = jobs[j].max_diff <= 6;
    if ((rc = plan_launch(ix, n_jobs, max_len, max_seed, R, PASS_MAIN, P))) return rc;
    HSA_HIP(hipEventRecord(ix->ev0, st));
    if ((rc = launch_pass(ix, P, ix->main, H.io, PassLink{}, st))) return rc;
    HSA_HIP(hipEventRecord(ix->ev1, st));
    unsigned long long ctr[CTR_SLOTS];
    if ((rc = copy_back(H.io, n_jobs, out, ctr, st))) return rc;
    if (ctr[CTR_ERRORS]) { hsa_set_error("%llu reads exceed the regime's max_diff bound", ctr[CTR_ERRORS]); return HSA_E_ARG; }
    float ms = 0;
    HSA_HIP(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    uint64_t total = ctr[CTR_HITS] < H.io.hit_cap ? ctr[CTR_HITS] : H.io.hit_cap;
    const double tv1 = verbose ? now() : 0.0;
    HostHits h = alloc_hits(total);
    if (!h) return HSA_E_MEM;
    if (total) HSA_HIP(hipMemcpy(h.get(), H.io.hits, total * 36, hipMemcpyDeviceToHost));
    if (verbose)
        fprintf(stderr, "[hsa] search of %d reads: copies in + kernels + result arrays out %.1f ms (kernels %.1f ms), "
                        "hits out %.1f ms\n", n_jobs, 1e3 * (tv1 - tv0), ms, 1e3 * (now() - tv1));
    add_stats(stats, ctr, ms, true);

    // overflowed reads: re-run with large per-read capacity (never a CPU path), each round
    // into hit buffers of its own
    std::vector<int32_t> list, n2;
    std::vector<uint32_t> f2;
    std::vector<uint64_t> o2;
    for (int round = 0; round < 4; ++round) {
        list.clear();
        for (int j = 0; j < n_jobs; ++j) if (out.flags[j] & HSA_F_OVERFLOW) list.push_back(j);
        const int n_over = (int)list.size();
        if (n_over == 0) break;
        n2.resize(n_jobs); f2.resize(n_jobs); o2.resize(n_jobs);
        if (stats) stats->overflow_reruns += n_over;
        LaunchPlan B;
        const int mode = round == 0 ? PASS_BIG : PASS_HUGE;
        if ((rc = plan_launch(ix, n_over, max_len, max_seed, R, mode, B))) return rc;
        const uint64_t cap2 = (uint64_t)n_over * 256 * (round + 1) + 65536;
        const size_t o2_fl = al((size_t)n_jobs * 4), o2_ho = o2_fl * 2, o2_hits = o2_ho + al((size_t)n_jobs * 8);
        DevBuf d2;
        HSA_HIP(hipMalloc(&d2.p, o2_hits + cap2 * 36));
        HSA_HIP(hipMemcpyAsync(H.d_list, list.data(), sizeof(int32_t) * n_over, hipMemcpyHostToDevice, st));
        char *c2 = (char *)d2.p;
        PassIO io2 = H.io;
        io2.list = H.d_list; io2.n = n_over;
        io2.n_aln = (int32_t *)c2; io2.flags = (uint32_t *)(c2 + o2_fl); io2.hit_off = (uint64_t *)(c2 + o2_ho);
        io2.hits = (uint32_t *)(c2 + o2_hits); io2.hit_cap = cap2;
        HSA_HIP(hipEventRecord(ix->ev0, st));
        if ((rc = launch_pass(ix, B, mode == PASS_BIG ? ix->big : ix->huge, io2, PassLink{}, st))) return rc;
        HSA_HIP(hipEventRecord(ix->ev1, st));
        if ((rc = copy_back(io2, n_jobs, HostOut{n2.data(), f2.data(), o2.data(), nullptr, nullptr}, ctr, st))) return rc;
        HSA_HIP(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
        const uint64_t t2 = ctr[CTR_HITS] < cap2 ? ctr[CTR_HITS] : cap2;
        uint32_t *grown = (uint32_t *)realloc(h.get(), (total + t2 + 1) * 36);
        if (!grown) { hsa_set_error("host allocation of %llu hits failed", (unsigned long long)(total + t2)); return HSA_E_MEM; }
        (void)h.release(); h.reset(grown);
        if (t2) HSA_HIP(hipMemcpy(h.get() + total * 9, io2.hits, t2 * 36, hipMemcpyDeviceToHost));
        for (const int j : list) { out.n_aln[j] = n2[j]; out.flags[j] = f2[j]; out.hit_off[j] = o2[j] + total; }
        total += t2;
        add_stats(stats, ctr, ms, false);
    }
    for (int j = 0; j < n_jobs; ++j)
        if (out.flags[j] & HSA_F_OVERFLOW) { hsa_set_error("read %d exceeds the large-pass capacity", j); return HSA_E_ARG; }
    if (mh && (rc = export_widths(in, H))) return rc;
    *out.hits = h.release();
    return (long)total;
}

extern "C" long hsa_search_batch(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const hsa_job_t *jobs,
                                 int n_jobs, const uint8_t *codes, size_t codes_len, int32_t *n_aln, uint32_t *flags,
                                 uint64_t *hit_off, uint32_t **hits_out, hsa_stats_t *stats)
{
    return search_batch_impl(ix, regimes, n_regimes, HostIn{jobs, n_jobs, codes, codes_len, nullptr},
                             HostOut{n_aln, flags, hit_off, hits_out, stats});
}

extern "C" long hsa_match_gap_batch(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const hsa_job_t *jobs,
                                    const hsa_mg_job_t *mg, int n_jobs, const uint8_t *codes, size_t codes_len,
                                    const int32_t *widths, size_t width_pairs, int32_t *widths_out, int32_t *n_aln,
                                    uint64_t *hit_off, uint32_t **hits_out, hsa_stats_t *stats)
{
    *hits_out = nullptr;
    if (n_jobs > 0 && (!mg || !widths || !widths_out)) { hsa_set_error("hsa_match_gap_batch: null argument"); return HSA_E_ARG; }
    std::vector<uint32_t> flags((size_t)(n_jobs > 0 ? n_jobs : 0) + 1);
    const MgHost mh{mg, widths, width_pairs, widths_out};
    return search_batch_impl(ix, regimes, n_regimes, HostIn{jobs, n_jobs, codes, codes_len, &mh},
                             HostOut{n_aln, flags.data(), hit_off, hits_out, stats});
}

extern "C" int hsa_search_device(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes,
                                 const hsa_device_batch_t *b, void *stream)
{
    if (int rc = hsa_need32(ix)) return rc;
    return search_device_impl<uint32_t>(ix, regimes, n_regimes, b, stream);
}

extern "C" int hsa_pass_times(hsa_index_t *ix, int n, float *widths_ms, float *search_ms)
{
    if (n < 1 || n > hsa_index::PASS_RING || (uint64_t)n > ix->pev_n) {
        hsa_set_error("hsa_pass_times: %d passes requested, %llu recorded (ring %d)", n,
                      (unsigned long long)ix->pev_n, hsa_index::PASS_RING);
        return HSA_E_ARG;
    }
    for (int i = 0; i < n; ++i) {
        hipEvent_t *pe = ix->pev[(ix->pev_n - (uint64_t)n + (uint64_t)i) % hsa_index::PASS_RING];
        HSA_HIP(hipEventSynchronize(pe[2]));
        HSA_HIP(hipEventElapsedTime(widths_ms + i, pe[0], pe[1]));
        HSA_HIP(hipEventElapsedTime(search_ms + i, pe[1], pe[2]));
    }
    return 0;
}

extern "C" int hsa_last_pass_ms(hsa_index_t *ix, float *widths_ms, float *search_ms)
{
    if (ix->pev_n) return hsa_pass_times(ix, 1, widths_ms, search_ms);   // the newest hsa_search_device pass
    HSA_HIP(hipEventSynchronize(ix->ev1));
    HSA_HIP(hipEventElapsedTime(widths_ms, ix->ev0, ix->evm));
    HSA_HIP(hipEventElapsedTime(search_ms, ix->evm, ix->ev1));
    return 0;
}
