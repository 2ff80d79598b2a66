#pragma once
// hsa_search_launch.h -- the host side of hsa_search_kernels.h: regime checks and staging,
// a pass's launch plan, one pass (launch_pass), the MAIN -> BIG -> HUGE capacity cascade
// (run_capacity_passes), the k_search_any passes, hsa_search_device's implementation.
// Included by hsa_search.hip (32-bit API) and hsa_search64.hip (64-bit API).
#include <map>
#include <mutex>

#include "hsa_search_kernels.h"

// ---------------------------------------------------------------- host helpers (both TUs)
// What any search accepts (k_search_any's bounds); fast_regimes: what k_search's layouts hold.
static int check_regimes(const hsa_regime_t *rg, int n)
{
    for (int r = 0; r < n; ++r) {
        const hsa_regime_t &R = rg[r];
        if (R.s_mm < 0 || R.s_gapo < 0 || R.s_gape < 0) { hsa_set_error("negative penalty"); return HSA_E_ARG; }
        if (R.n_stacks <= 0 || R.n_stacks > ANY_MAX_STACKS) {
            hsa_set_error("n_stacks %d outside 1..%d", R.n_stacks, ANY_MAX_STACKS);
            return HSA_E_ARG;
        }
        if (R.max_gapo < 0 || R.max_gape < 0) { hsa_set_error("max_gapo/max_gape negative"); return HSA_E_ARG; }
        if (R.max_diff < -1) { hsa_set_error("max_diff out of range"); return HSA_E_ARG; }
    }
    return 0;
}

// Dense bucket numbering of the scores a search of this regime can push
// (bwtgap.c:46-75): n_mm <= max_diff+1, n_gapo <= min(max_gapo, max_diff), n_gape > 0
// only after a gap open.  Returns the bucket count.
static int bucket_map(const hsa_regime_t &R, uint8_t map[MAXS])
{
    bool used[MAXS] = {false};
    const int md = R.max_diff < 0 ? 0 : R.max_diff;
    const int go_max = R.max_gapo < md ? R.max_gapo : md;
    for (int mm = 0; mm <= md + 1; ++mm)
        for (int go = 0; go <= go_max; ++go)
            for (int ge = 0; ge <= (go > 0 ? R.max_gape : 0); ++ge) {
                const int s = mm * R.s_mm + go * R.s_gapo + ge * R.s_gape;
                if (s >= 0 && s < MAXS && s < R.n_stacks) used[s] = true;
            }
    int k = 0;
    for (int s = 0; s < MAXS; ++s) map[s] = used[s] && k < 0xFF ? (uint8_t)k++ : (uint8_t)0xFF;
    return k;
}

// Regimes whose every bound fits k_search's layouts: the entry meta word (n_gapo 4
// bits, n_gape 8, n_mm 7), the score table (MAXS), the bucket mask (MAXB reachable
// scores) and the 16-bit pruning elements (bids compared with bounds <= 254).  Other
// regimes run k_search_any.
static bool fast_regimes(const hsa_regime_t *rg, int n)
{
    if (getenv("HSA_FORCE_ANY")) return false;       // tests: every search through k_search_any
    for (int r = 0; r < n; ++r) {
        const hsa_regime_t &R = rg[r];
        if (R.max_gapo > 14 || R.max_gape > 254 || R.max_diff > 125 || R.max_seed_diff > 254 || R.n_stacks > MAXS)
            return false;
        uint8_t map[MAXS];
        if (bucket_map(R, map) > MAXB) return false;
    }
    return true;
}

#define FAST_MAX_LEN 1023u       // k_search: 10-bit read positions (meta word, control word)

// The dense bucket of a score is simply its n_mm when no gap opens exist and every
// reachable mismatch count has its own score (k_search skips the table then).
static bool mm_buckets(const hsa_regime_t *rg, int n, const uint8_t *bmap)
{
    for (int r = 0; r < n; ++r) {
        const hsa_regime_t &R = rg[r];
        if (R.max_gapo != 0 || R.s_mm <= 0) return false;
        const int md = R.max_diff < 0 ? 0 : R.max_diff;
        for (int mm = 0; mm <= md + 1; ++mm) {
            const int sc = mm * R.s_mm;
            if (sc >= MAXS || bmap[r * MAXS + sc] != mm) return false;
        }
    }
    return true;
}

// What the regimes of a search decide for its passes: gap opens possible; 16-bit pruning
// elements when a bid may be compared with a bound above 14 (WFmt); 4-bit ones exact while
// every such bound is <= 6 (WFmt<WNib>; a job's max_diff never exceeds its regime's); the
// mixed format (4-bit seed row, SeedFmt) exact while max_seed_diff <= 6, for rows k_widths
// writes (caller-width passes clear snib_ok); the HUGE pass's bound on live stack entries.
// nb, the stack buckets, is stage_regimes'.
struct RegimePlan {
    int nb;
    bool gaps, wide, nib_ok, snib_ok;
    int max_entries;
};

static RegimePlan regime_plan(const hsa_regime_t *rg, int n)
{
    RegimePlan C{.nb = 0, .gaps = false, .wide = false, .nib_ok = true, .snib_ok = true, .max_entries = 0};
    for (int r = 0; r < n; ++r) {
        const int bound = rg[r].max_diff > rg[r].max_seed_diff ? rg[r].max_diff : rg[r].max_seed_diff;
        C.gaps |= rg[r].max_gapo > 0;
        C.wide |= bound > 14;
        C.nib_ok &= bound <= 6;
        C.snib_ok &= rg[r].max_seed_diff <= 6;
        C.max_entries = rg[r].max_entries > C.max_entries ? rg[r].max_entries : C.max_entries;
    }
    return C;
}

struct LaunchPlan {
    size_t lanes, blocks;
    uint32_t nt;                     // lanes per workgroup of k_search (256 or 64)
    uint32_t pcap, hcap, nb;
    bool gaps, wide;                 // gap opens possible; 16-bit pruning elements (WFmt)
    bool nib;                        // 4-bit pruning elements in LDS (WFmt<WNib>)
    bool snib;                       // 8-bit read row, 4-bit seed row, in HBM and LDS (SeedFmt)
    uint32_t off_heads, off_wb, off_ws;
    uint32_t lds_wb, lds_ws;         // LDS words per lane of the read / seed row (SearchArgs)
    size_t lds;
    bool huge;                       // PASS_HUGE: 32-bit links, reused slots
    uint32_t ntab;                   // score table entries per regime in LDS
    size_t resident;                 // lanes resident on the chip (every CU full)
    size_t res_lanes = 0;            // lanes the scratch is reserved for (BIG: all its lanes)
};

// The capacity passes of one search: MAIN (every read), BIG (the reads that overflowed
// their main-pass lane: 65 535 pool slots, 16 384 hits), HUGE (the reads that overflowed
// BIG: reused slots up to max_entries + 16 live entries, 262 144 hits).
enum { PASS_MAIN = 0, PASS_BIG = 1, PASS_HUGE = 2 };

// The k_search instantiation a plan runs.
using SearchFn = void (*)(SearchArgs);

template <typename WT, int NT, typename IT, bool SN>
static SearchFn search_kernel_nt(const LaunchPlan &P)
{
    if (P.nb <= 32) return P.gaps ? k_search<0, true, WT, NT, false, IT, SN> : k_search<0, false, WT, NT, false, IT, SN>;
    if (P.nb <= 64) return P.gaps ? k_search<1, true, WT, NT, false, IT, SN> : k_search<1, false, WT, NT, false, IT, SN>;
    return P.gaps ? k_search<2, true, WT, NT, false, IT, SN> : k_search<2, false, WT, NT, false, IT, SN>;
}

template <typename IT>
static SearchFn search_kernel(const LaunchPlan &P)
{
    if (P.nib)                                       // never a HUGE pass (plan_launch)
        return P.nt == 64 ? search_kernel_nt<WNib, 64, IT, false>(P) : search_kernel_nt<WNib, 256, IT, false>(P);
    if (P.snib)                                      // nor this: 8-bit rows only
        return P.nt == 64 ? search_kernel_nt<uint8_t, 64, IT, true>(P) : search_kernel_nt<uint8_t, 256, IT, true>(P);
    if (P.huge) {
        if (P.wide) return P.gaps ? k_search<2, true, uint16_t, 64, true, IT> : k_search<2, false, uint16_t, 64, true, IT>;
        return P.gaps ? k_search<2, true, uint8_t, 64, true, IT> : k_search<2, false, uint8_t, 64, true, IT>;
    }
    if (P.wide) return P.nt == 64 ? search_kernel_nt<uint16_t, 64, IT, false>(P) : search_kernel_nt<uint16_t, 256, IT, false>(P);
    return P.nt == 64 ? search_kernel_nt<uint8_t, 64, IT, false>(P) : search_kernel_nt<uint8_t, 256, IT, false>(P);
}

// Whether the plan's k_search instantiation keeps each pool entry's link in the entry
// (k_search's LK); EW: 32-bit words per interval bound.
static bool plan_entry_links(const LaunchPlan &P, size_t EW) { return pool_link_in_entry(P.huge, EW == 2, P.gaps, P.wide); }

// Waves per SIMD a kernel's registers allow: gfx950 gives a wave its VGPRs in granules of 8
// out of 512 per lane, at most 8 waves.  Asked of the runtime once per instantiation; 4,
// what k_search's launch bound guarantees, where it does not say.
static int kernel_waves_simd(SearchFn f)
{
    static std::mutex mu;
    static std::map<SearchFn, int> known;
    std::lock_guard<std::mutex> lock(mu);
    const auto it = known.find(f);
    if (it != known.end()) return it->second;
    int w = HSA_WAVES_SIMD;
    hipFuncAttributes at{};
    if (hipFuncGetAttributes(&at, reinterpret_cast<const void *>(f)) == hipSuccess && at.numRegs > 0) {
        w = 512 / ((at.numRegs + 7) / 8 * 8);
        w = w > 8 ? 8 : w < 1 ? 1 : w;
    } else {
        (void)hipGetLastError();
    }
    known[f] = w;
    return w;
}

template <typename IT = uint32_t>
static int plan_launch(hsa_index *ix, int n_jobs, int max_len, int max_seed, const RegimePlan &R, int mode,
                       LaunchPlan &P)
{
    constexpr uint32_t ent_bytes = 4u * sizeof(IT);  // pool entry bytes
    const int nb = R.nb, max_entries = R.max_entries;
    const bool gaps = R.gaps, wide = R.wide, nib_ok = R.nib_ok;
    const bool big = mode == PASS_BIG;
    P.huge = mode == PASS_HUGE;
    P.ntab = (uint32_t)ix->staged_ntab;
    P.nb = (uint32_t)nb;
    P.gaps = gaps;
    P.wide = wide;
    const uint32_t esz = wide ? 2u : 1u;
    P.nib = false;
    P.snib = false;
    // Resident workgroups per CU, from gfx950's own limits: 160 KiB of LDS per CU, and 4
    // waves per SIMD, which __launch_bounds__(NT, 4) guarantees -- or, in the mixed
    // format, what the registers of the instantiation the plan runs allow
    // (kernel_waves_simd: the bound is a ceiling of 128 VGPRs, not the occupancy; config
    // 2's 64-lane kernel takes 95, i.e. 5 waves per SIMD, 20 per CU).  Only there: with
    // byte rows the same cap put config 4's ungapped splice-seed searches on 20 waves
    // per CU and its step went from 702 to 665 k reads/s (profiles/seednib_ab.log).
    // The per-lane LDS (bucket heads, pruning rows) decides between 256-lane
    // workgroups and 64-lane ones, which pack the CU's LDS more finely: -n 4 -o 1 has 39
    // buckets and ~220 B per lane, i.e. 2 workgroups of 256 (8 waves) but 11 of 64 (11
    // waves); -n 4 -o 0 on 100 bp reads in the mixed format has 8 432 B per 64 lanes,
    // 19 workgroups = 19 waves, where 256-lane workgroups stop at 4 = 16 waves.
    // (hipOccupancyMaxActiveBlocksPerMultiprocessor is not used: depending on which
    // HIP runtime the process loaded first it assumed 64 KiB of LDS and halved the
    // grid -- measured 512 instead of 1024 workgroups, 1.5x slower.)
    auto layout = [&](uint32_t nt) {
        const uint32_t epw = P.nib ? 8u : 4u / esz;      // elements per LDS word (WFmt::EPW)
        P.nt = nt;
        P.off_heads = 2 * P.ntab + 128;   // score tables, then the two regimes
        P.off_wb = P.off_heads + (uint32_t)nb * nt * (P.huge ? 4u : 2u);
        // k_search reads elements 0 .. len - 1 of a row (pops of position i read i - 1,
        // expansions i - 1 and i < len; seed rows ii - 1 and ii < seed_len): the 4-bit
        // rows keep just those, which takes config 5's 64-lane workgroups from 15 to 16
        // per CU, and so does the mixed format (its read row: ceil(len / 4) words, its
        // seed row ceil(seed_len / 8)); the plain 8-bit rows keep element len too (the
        // LDS-DMA copies the HBM row's whole capacity)
        P.lds_wb = P.nib ? ((uint32_t)max_len + 7u) / 8u : P.snib ? ((uint32_t)max_len + 3u) / 4u : (uint32_t)max_len / epw + 1u;
        P.lds_ws = P.nib || P.snib ? ((uint32_t)max_seed + 7u) / 8u : (uint32_t)max_seed / epw + 1u;
        P.off_ws = P.off_wb + P.lds_wb * nt * 4u;
        P.lds = ((size_t)P.off_ws + (size_t)P.lds_ws * nt * 4u + 15) / 16 * 16;
        int per_cu = (int)((160u * 1024u) / P.lds);
        const int simd = P.snib ? kernel_waves_simd(search_kernel<IT>(P)) : HSA_WAVES_SIMD;
        const int cap = 4 * simd / (int)(nt / 64);
        const int want = g_waves_per_cu / (int)(nt / 64);
        if (per_cu > cap) per_cu = cap;
        if (per_cu > want) per_cu = want > 0 ? want : 1;
        return per_cu;
    };
    static const int force256 = getenv("HSA_WG256") != nullptr;   // A/B runs only
    auto best = [&]() {                              // the workgroup size with more waves per CU
        int per_cu = layout(P.huge ? 64 : 256);
        if (!force256 && !P.huge) {
            const int p64 = layout(64);
            if (p64 > per_cu * 4) per_cu = p64;
            else per_cu = layout(256);
        }
        return per_cu;
    };
    int per_cu = best();
    const char *wf = getenv("HSA_WFMT");
    const bool force_nib = wf && !strcmp(wf, "nib"), no_nib = wf && !strcmp(wf, "byte");
    const bool force_snib = wf && !strcmp(wf, "seednib");
    // The mixed format (4-bit seed row, the read row without element len) where it puts
    // more waves on the CU, in ungapped searches: config 2 runs 19 workgroups of 64 lanes
    // per CU instead of 4 of 256.  A launch on its own takes as long as before (the gain
    // of waves ends at 16: 12 / 14 / 16 / 19 waves 16.4 / 15.7 / 14.6 / 14.8 ms); steps
    // that overlap on several handles, as the bench's do, run 3 % faster (59.1-59.8 ->
    // 60.4-61.2 M reads/s, the same library with HSA_WFMT=byte and without,
    // profiles/seednib_ab.log).  Gapped searches keep byte rows unless forced.
    // HSA_WFMT=seednib forces it where it is exact, =byte forbids it.
    if (R.snib_ok && !wide && !P.huge && !no_nib && max_seed > 0 && (force_snib || !gaps)) {
        const int waves8 = per_cu * (int)(P.nt / 64);
        const LaunchPlan keep = P;
        P.snib = true;
        const int per_sn = best();
        if (!force_snib && per_sn * (int)(P.nt / 64) <= waves8) { P = keep; }
        else per_cu = per_sn;
    }
    // long reads: 4-bit elements when the 8-bit rows leave the CU short of 16 waves, in
    // ungapped searches, which are latency-bound: config 5's k_search 45.6 -> 38.4 ms.
    // Gapped ones are issue-bound and lose more to the unpacking and the base loads
    // than they gain in waves (config 4: 1 988 -> 2 147 ms; config 3: equal).
    // HSA_WFMT=nib forces them where exact, =byte keeps 8-bit (tests and A/B runs).
    if (nib_ok && !wide && !P.huge && !no_nib && !force_snib &&
        (force_nib || (!gaps && per_cu * (int)(P.nt / 64) < 16))) {
        const int waves8 = per_cu * (int)(P.nt / 64);
        const LaunchPlan keep = P;
        P.nib = true;
        P.snib = false;
        const int per_nib = best();
        if (!force_nib && per_nib * (int)(P.nt / 64) <= waves8) { P = keep; }
        else per_cu = per_nib;
    }
    if (P.lds > 160 * 1024) { hsa_set_error("reads too long for the LDS budget (%zu bytes)", P.lds); return HSA_E_ARG; }
    if (per_cu < 1) { hsa_set_error("search kernel does not fit (LDS %zu)", P.lds); return HSA_E_ARG; }
    const uint32_t NTB = P.nt;
    size_t blocks = (size_t)ix->n_cu * per_cu;
    P.resident = blocks * NTB;
    size_t need_blocks = ((size_t)n_jobs + NTB - 1) / NTB;
    if (P.huge) {
        blocks = 1;                                          // 64 lanes: a handful of reads
    } else if (big) {
        static const size_t big_lanes = getenv("HSA_BIG_LANES") ? strtoull(getenv("HSA_BIG_LANES"), nullptr, 10) : 4096;
        const size_t big_blocks = big_lanes / NTB > 0 ? big_lanes / NTB : 1;
        blocks = need_blocks < big_blocks ? need_blocks : big_blocks;
        // the BIG pass's scratch is reserved for all its lanes whatever the pass's size:
        // the attach-time warm-up then allocates it (7.3 GB at the default shape) instead
        // of a process's first full batch
        P.res_lanes = big_blocks * NTB;
    } else if (need_blocks < blocks) {
        blocks = need_blocks;
    }
    if (blocks < 1) blocks = 1;
    P.blocks = blocks;
    P.lanes = blocks * NTB;
    if (getenv("HSA_VERBOSE")) {                   // read per plan: tests switch it on mid-process
        int occ = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_search<1, true, uint8_t, 256>, 256, P.lds);
        fprintf(stderr, "[hsa] launch: %d CUs x %d workgroups of %u lanes (runtime occupancy query says %d), "
                "LDS %zu B, %zu workgroups, %d buckets%s%s\n", ix->n_cu, per_cu, P.nt, occ, P.lds, blocks, nb,
                P.nib ? ", 4-bit rows" : P.snib ? ", 4-bit seed row" : "",
                plan_entry_links(P, sizeof(IT) / 4) ? ", links in the entries" : "");
    }
    // pool slots are not reused within a search: gapped searches push many more.  A
    // deeper main-pass pool keeps the long gapped searches inside the main pass, where
    // their tails overlap other lanes' work, instead of the serial overflow re-run:
    // config 4 (150 bp, -o 1) 2.36 -> 2.07 s per 1M reads at 32768 (49152: same)
    static const int pool_env = getenv("HSA_POOL_ENTRIES") ? atoi(getenv("HSA_POOL_ENTRIES")) : 0;   // A/B runs
    const int pool_main = g_pool_entries ? g_pool_entries : pool_env > 0 && pool_env <= 65535 ? pool_env : 0;
    // gapped reads of up to 128 bases: 16 384 (config 3 at 32 768: 106 GB of scratch per
    // handle; at 16 384 53 GB and k_search 284.9 -> 283.7 ms, profiles/r05_pool16k_ab.log);
    // longer gapped reads keep 32 768 (config 4 at 8 192: 32 s against 1.2 s)
    P.pcap = big ? 65535u : (uint32_t)(pool_main ? pool_main : (gaps ? (max_len <= 128 ? 16384 : 32768) : 8192));
    // searches of at most 32 bases (the splice path's 12-mer anchors, which run on every
    // resident lane) keep 8 192 entries with gap opens too: 155 -> 39 GB of scratch per
    // handle at config 4, the anchors' time unchanged (profiles/r05_pool_short_ab.log);
    // HSA_POOL_SHORT=n sets it (0: the regime's default)
    static const int pool_short = getenv("HSA_POOL_SHORT") ? atoi(getenv("HSA_POOL_SHORT")) : 8192;
    if (!big && !pool_main && max_len <= 32 && pool_short > 0 && pool_short <= 65535) P.pcap = (uint32_t)pool_short;
    P.hcap = big ? 16384u : (uint32_t)g_hit_cap;
    if (P.huge) {
        // live entries never exceed max_entries + 9 (bwtgap.c:150-151); the pool is
        // capped at 4 Mi entries per lane (80 MB), beyond which a read stays unfinished
        const uint64_t want = (uint64_t)(max_entries > 0 ? max_entries : 0) + 16u;
        P.pcap = (uint32_t)(want < (4ull << 20) ? want : (4ull << 20));
        P.hcap = 262144u;
    } else if (ent_bytes > 16 && !big) {
        // 64-bit entries are 32 bytes: the main pass's pools stay within 64 GB of HBM
        // (next to an index of up to ~2 x 16 GB for a 15 Gbp text); reads that need
        // more go to the big and huge passes as usual
        const size_t budget = (size_t)64 << 30;
        if (P.lanes * P.pcap * ent_bytes > budget) {
            const size_t p = budget / (P.lanes * ent_bytes);
            P.pcap = (uint32_t)(p < 1024 ? 1024 : p);
        }
    }
    return 0;
}

template <typename IT>
static void launch_search(const LaunchPlan &P, const SearchArgs &A, hipStream_t st)
{
    hipLaunchKernelGGL(search_kernel<IT>(P), dim3((unsigned)P.blocks), dim3(P.nt), P.lds, st, A);
}

// The levels of the index's root width trie that kernels of this interval width use (0:
// none; HSA_TRIE=0: rank steps only, A/B runs)
static uint32_t trie_levels(const hsa_index *ix, bool wide)
{
    const char *te = getenv("HSA_TRIE");
    return ix->trie_depth > 0 && ix->trie_wide == wide && !(te && atoi(te) == 0) ? ix->trie_depth : 0u;
}

// caller-width mode of a pass (hsa_match_gap_batch)
struct MgPass {
    const hsa_mg_job_t *d_mg;
    int32_t *d_cw;
};

// What a search pass reads and writes, all on the device.  The passes of one search
// (MAIN, BIG, HUGE; k_search_any's) share it but for the job list.
struct PassIO {
    const hsa_job_t *jobs;
    const int32_t *list;           // the pass's jobs (null: jobs 0 .. n - 1)
    int n;                         // their number, or its upper bound when the count is on the device
    const uint8_t *codes;
    int32_t *n_aln;                // per job: hits, flags, its first hit record
    uint32_t *flags;
    uint64_t *hit_off;
    uint32_t *hits;                // hit_cap records
    uint64_t hit_cap;
    unsigned long long *ctr;       // CTR_SLOTS counters
    int max_len, max_seed;
    MgPass mg;                     // caller widths (d_mg null: the search computes its own)
};

// How a pass hangs in its search's cascade.  The default is a pass on its own: host
// count, the main queue head (which makes launch_pass zero the counters), no re-run list.
struct PassLink {
    int32_t *ovf_list = nullptr;                  // out: the jobs that overflowed this pass (null: they stay unfinished)
    const unsigned long long *n_dev = nullptr;    // in: the job count on the device (null: PassIO::n)
    uint32_t qctr = CTR_Q_MAIN;                   // the counter slot of this pass's queue head
    uint32_t ovf_ctr = CTR_OVF_MAIN;              // the counter slot that numbers ovf_list's entries
};

// The kernels' arguments of one pass, its width rows sized in ix->d_wrows; the regimes and
// their bucket maps are where stage_regimes left them, at the head of ix->d_in.
template <typename IT = uint32_t>
static int pass_args(hsa_index *ix, const LaunchPlan &P, SearchScratch &S, const PassIO &io, const PassLink &lk,
                     SearchArgs &A)
{
    constexpr size_t WGB = sizeof(IT);       // bytes per full w value (wg rows)
    const bool mg = io.mg.d_mg != nullptr;
    const uint32_t esz = P.wide ? 2u : 1u;
    // HBM row capacities: elements 0 .. len (seed_len) at esz bytes each; the mixed format's seed row at 4 bits
    const uint32_t rb = (((uint32_t)io.max_len + 1u) * esz + 3u) & ~3u;
    const uint32_t rs = P.snib ? ((uint32_t)io.max_seed / 8u + 1u) * 4u : (((uint32_t)io.max_seed + 1u) * esz + 3u) & ~3u;
    const uint32_t rg = (uint32_t)io.max_len + 1u;
    const size_t rows = ((size_t)io.n + 63) / 64 * 64 * 2;     // two 64-row-aligned planes (lazy widths)
    const size_t row_bytes = rb + rs + WGB * (size_t)rg + (mg ? 4 * (size_t)rg : 0);   // + full bids (caller widths)
    // + wq (4 n), cost keys (2 n), order (4 n) and its 32 counters
    if (int rc = hsa_grow(&ix->d_wrows, &ix->d_wrows_cap, rows * row_bytes + 10 * (size_t)io.n + 1024)) return rc;
    uint8_t *wr = (uint8_t *)ix->d_wrows;
    A.fwd = RankDir{ix->blk[0], ix->isa0};
    A.rev = RankDir{ix->blk[1], ix->risa0};
    A.T = ix->T;
    memcpy(A.C, ix->C, sizeof A.C);
    A.fwd64 = hsa_rank_dir64(ix, 0);
    A.rev64 = hsa_rank_dir64(ix, 1);
    A.T64 = ix->T64;
    memcpy(A.C64, ix->C64, sizeof A.C64);
    A.regimes = (const hsa_regime_t *)ix->d_in; A.bmap = (const uint8_t *)ix->d_in + 256;
    A.jobs = io.jobs; A.job_list = io.list; A.n_jobs = io.n; A.codes = io.codes;
    A.n_aln = io.n_aln; A.flags = io.flags; A.hit_off = io.hit_off; A.hits = io.hits; A.hit_cap = io.hit_cap;
    A.ctr = io.ctr;
    A.wb = wr; A.ws = wr + rows * rb; A.wg = reinterpret_cast<uint32_t *>(wr + rows * (rb + rs));
    A.rb = rb; A.rs = rs; A.rg = rg;
    A.pool = S.pool; A.nxt = S.nxt; A.hbuf = S.hbuf;
    A.pcap = P.pcap; A.hcap = P.hcap;        // the planned capacities (the scratch may be larger)
    A.nb = P.nb; A.off_heads = P.off_heads; A.off_wb = P.off_wb; A.off_ws = P.off_ws;
    A.lds_wb = P.lds_wb; A.lds_ws = P.lds_ws;
    A.mm_buckets = ix->staged_mmb ? 1u : 0u;
    A.ntab = P.ntab;
    A.batch_k = (uint32_t)g_batch_k;
    A.batch_idle = (uint32_t)g_batch_idle;
    A.ovf_list = lk.ovf_list; A.n_dev = lk.n_dev; A.qctr = lk.qctr; A.ovf_ctr = lk.ovf_ctr;
    A.split = 0; A.sp_n = nullptr; A.sp_off = nullptr; A.sp_q = nullptr; A.sp_p = nullptr;
    A.ktd = trie_levels(ix, sizeof(IT) == 8);
    A.ktw = A.ktd ? ix->d_trie_w : nullptr;
    A.sdc = sizeof(IT) == 4 ? ix->slevel : 0u;   // the table's level (sdepth or sdepth + 1)
    A.stw = A.sdc ? ix->d_trie_s : nullptr;
    A.wkey = nullptr; A.perm = nullptr; A.okey = 0;
    A.fwd_list = nullptr; A.fwd_n = nullptr; A.fwd_only = 0; A.rmap = nullptr;
    A.fr_budget = 0; A.fr_demand = 0; A.fr_cap = 0;
    A.fr_ent = nullptr; A.fr_tag = nullptr; A.fr_rq = nullptr; A.fr_st = nullptr; A.fr_q = nullptr; A.fr_p = nullptr; A.fr_c = nullptr;
    A.mg = io.mg.d_mg; A.cw = io.mg.d_cw;
    A.wbid = mg ? reinterpret_cast<int32_t *>(wr + rows * (rb + rs + WGB * (size_t)rg)) : nullptr;
    A.wq = reinterpret_cast<uint32_t *>(wr + rows * row_bytes);
    return 0;
}

// Strand-split mode for the main pass of a small batch: each read's two strands on two
// lanes when both fit on the chip at once (HSA_SPLIT=0/1 forces it off/on).  A read's
// search chain halves (rc and fwd side by side); the fwd strand's work is speculative, so
// large batches, which fill every lane anyway, keep one read per lane.
// Helpers are opt-in (HSA_HELP=1): exact, but measured slower on the drop-in's 100 000-read
// calls ("Helpers")
static bool use_help()
{
    const char *e = getenv("HSA_HELP");
    return e && atoi(e) != 0;
}

// (helpers run in gapped 32-bit kernels only, k_search's FRH)
template <typename IT>
static bool help_kernel(const LaunchPlan &P) { return use_help() && HSA_HELPERS && P.gaps && sizeof(IT) == 4; }

static bool use_split(const LaunchPlan &P, const PassIO &io, const PassLink &lk, bool help)
{
    if (io.mg.d_mg || lk.n_dev || lk.qctr != CTR_Q_MAIN || P.huge || io.n <= 0) return false;
    const char *e = getenv("HSA_SPLIT");
    if (e) return atoi(e) != 0;
    // with helpers, also batches of up to one read per resident lane: their tails are the
    // long strand searches the waiting lanes then share
    return (help ? (size_t)io.n : 2 * (size_t)io.n) <= P.resident;
}

// Helpers of a strand-split pass (SearchArgs::fr_*): the shared frontier and the per-item
// state in ix->d_help, zeroed on the pass's stream.  HSA_HELP=0: off; HSA_HELP_BUDGET pops
// before a strand may offer its entries (default 512); HSA_HELP_DEMAND waiting lanes beyond
// the unsearched chunks before it does (default: half the pass's lanes, so that only the
// strands still running when half the chip waits -- the launch's tail -- offer); HSA_HELP_CAP
// chunks of FR_CH entries (default 1 Mi: 512 MB).
// Off when a regime's max_entries does not exceed the pool: then the main pass's stack
// stays below the reference's max_entries break (bwtgap.c:150-151) whenever it completes,
// and a strand its helpers answer counts the reference's rank queries and pops.
template <typename IT>
static int help_args(hsa_index *ix, SearchArgs &A, size_t items, const LaunchPlan &P, hipStream_t st)
{
    if (!help_kernel<IT>(P) || ix->staged_min_entries <= (int)P.pcap + 16) return 0;
    auto env = [](const char *k, long d) { const char *v = getenv(k); return v ? atol(v) : d; };
    const long budget = env("HSA_HELP_BUDGET", 512), demand = env("HSA_HELP_DEMAND", (long)(P.lanes / 2));
    const long cap = env("HSA_HELP_CAP", 1l << 20);
    if (budget <= 0 || cap <= 0 || cap > (1l << 24) || demand < 0 || items >= (1u << 26)) return 0;
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_st = 256, o_q = o_st + al(items * 4), o_p = o_q + al(items * 8), o_tag = o_p + al(items * 8);
    const size_t o_rq = o_tag + al((size_t)cap * 4);
    const size_t o_ent = o_rq + al((size_t)cap * 4), total = o_ent + (size_t)cap * FR_CH * FR_EW * 4;
    int rc = hsa_grow(&ix->d_help, &ix->d_help_cap, total);
    if (rc) return rc;
    char *d = (char *)ix->d_help;
    HSA_HIP(hipMemsetAsync(d, 0, o_ent, st));       // counters, item state and sums, tags, ready queue
    A.fr_budget = (uint32_t)budget; A.fr_demand = (uint32_t)demand; A.fr_cap = (uint32_t)cap;
    A.fr_c = (unsigned long long *)d;
    A.fr_st = (uint32_t *)(d + o_st);
    A.fr_q = (unsigned long long *)(d + o_q);
    A.fr_p = (unsigned long long *)(d + o_p);
    A.fr_tag = (uint32_t *)(d + o_tag);
    A.fr_rq = (uint32_t *)(d + o_rq);
    A.fr_ent = (uint32_t *)(d + o_ent);
    return 0;
}

// The pass's search scratch (per-lane pools, links, staged hits), sized to what the
// device can give: the pool per lane is the plan's capacity unless that would not fit in
// the free HBM (less a 2 GiB margin) or in HSA_SCRATCH_MB, in which case it is halved
// until it does (down to 512 entries), and again if the allocation itself fails.  A
// smaller pool changes no result: a read that outgrows its lane is re-run in the BIG and
// HUGE passes as before, so the cost is speed, never an error (the reference's capacity
// bound is max_entries, bwtgap.c:150-151, which the HUGE pass keeps).
static int scratch_fit(hsa_index *ix, SearchScratch &S, LaunchPlan &P, size_t EW)
{
    // link bytes per pool entry: none where the pass's kernel keeps the links in the entries;
    // the scratch's link array stays as wide as an earlier pass made it (hsa_scratch_reserve)
    const size_t lb = P.huge ? 4 : plan_entry_links(P, EW) ? 0 : 2, floor_cap = 512;
    const size_t lba = lb > S.link_bytes ? lb : S.link_bytes;
    auto pe_of = [&](uint32_t pc) { return (size_t)((pc + 31u) & ~31u) * EW; };
    const size_t rl = P.res_lanes > P.lanes ? P.res_lanes : P.lanes;
    auto bytes = [&](uint32_t pc) { return rl * (pe_of(pc) * (16 + lba) + (size_t)P.hcap * EW * 36); };
    const char *cm = getenv("HSA_SCRATCH_MB");          // read per pass: tests set it mid-process
    const size_t cap_mb = cm ? strtoull(cm, nullptr, 10) : 0;
    const bool fits = S.pool && rl * pe_of(P.pcap) <= S.pool_entries && rl * (size_t)P.hcap * EW <= S.hit_entries;
    bool held = fits && lb <= S.link_bytes;
    if (fits && !held && !P.huge) {
        // Only the link array widens: hsa_scratch_reserve allocates it for the pool the handle
        // holds (S.pool_entries, which may exceed this pass's) and leaves that pool in place.
        // Where that does not fit beside the pool, the scratch is given back first and the
        // pool and its links are planned together below, from what is then free.
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = (size_t)-1 / 2; }
        const size_t need = S.pool_entries * lb + ((size_t)2 << 30);     // the old array is freed after the new one exists
        const size_t all = S.pool_entries * (16 + lb) + S.hit_entries * 36;
        if (need <= fr && !(cap_mb && all > (cap_mb << 20))) held = true;
        else hsa_scratch_free(S);
    }
    if (!held && !P.huge) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = (size_t)-1 / 2; }
        fr += S.pool_entries * (16 + S.link_bytes) + S.hit_entries * 36;     // what the reservation frees first
        size_t avail = fr > ((size_t)2 << 30) ? fr - ((size_t)2 << 30) : 0;
        if (cap_mb && avail > (cap_mb << 20)) avail = cap_mb << 20;
        const uint32_t want = P.pcap;
        while (bytes(P.pcap) > avail && P.pcap > floor_cap) P.pcap = P.pcap / 2 > floor_cap ? P.pcap / 2 : floor_cap;
        if (P.pcap != want && getenv("HSA_VERBOSE"))
            fprintf(stderr, "[hsa] search scratch: pool %u -> %u entries per lane (%.1f GB for %zu lanes; %.1f GB "
                            "available)\n", want, P.pcap, bytes(P.pcap) / 1e9, P.lanes, avail / 1e9);
    }
    for (;;) {
        const int rc = hsa_scratch_reserve(S, rl, pe_of(P.pcap), (size_t)P.hcap * EW, lb);
        if (rc != HSA_E_MEM || P.huge || P.pcap <= floor_cap) return rc;
        P.pcap = P.pcap / 2 > floor_cap ? P.pcap / 2 : floor_cap;
        if (getenv("HSA_VERBOSE")) fprintf(stderr, "[hsa] search scratch: allocation failed, pool -> %u per lane\n", P.pcap);
    }
}

// One search pass over jobs (or a job list) with device pointers: k_widths fills the
// width rows of every (read, strand), then k_search runs the reads.
template <typename IT = uint32_t>
static int launch_pass(hsa_index *ix, const LaunchPlan &P0, SearchScratch &S, const PassIO &io, const PassLink &lk,
                       hipStream_t st)
{
    const int n = io.n;
    const bool mg = io.mg.d_mg != nullptr;
    const bool first = lk.qctr == CTR_Q_MAIN;          // the pass owns the counters: it zeroes them (not a device re-run)
    const bool split = use_split(P0, io, lk, help_kernel<IT>(P0));
    LaunchPlan P = P0;
    if (split) {                                        // lanes for 2 n items
        const size_t need = (2 * (size_t)n + P.nt - 1) / P.nt, cap = P.resident / P.nt;
        P.blocks = need < cap ? need : cap;
        P.lanes = P.blocks * P.nt;
    }
    // 64-bit intervals: two uint4 per pool entry, 10 staged words per hit (HitW)
    constexpr size_t EW = sizeof(IT) / 4;
    int rc = scratch_fit(ix, S, P, EW);
    if (rc) return rc;
    SearchArgs A;
    if (mg) {
        if constexpr (sizeof(IT) != 4) {
            hsa_set_error("caller-width searches (bwt_match_gap) take 32-bit indexes");
            return HSA_E_ARG;
        } else {
            if ((rc = pass_args<IT>(ix, P, S, io, lk, A))) return rc;
            if (first) HSA_HIP(hipMemsetAsync(io.ctr, 0, CTR_SLOTS * sizeof(unsigned long long), st));
            const unsigned nb = (unsigned)(((size_t)n + BLOCK - 1) / BLOCK);
            if (P.wide) hipLaunchKernelGGL(k_widths_import<uint16_t>, dim3(nb ? nb : 1), dim3(BLOCK), 0, st, A);
            else hipLaunchKernelGGL(k_widths_import<uint8_t>, dim3(nb ? nb : 1), dim3(BLOCK), 0, st, A);
            HSA_HIP(hipGetLastError());
            if (ix->ev_split) HSA_HIP(hipEventRecord(ix->ev_split, st));
            launch_search<uint32_t>(P, A, st);
            HSA_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_widths_export, dim3(nb ? nb : 1), dim3(BLOCK), 0, st, A);
            HSA_HIP(hipGetLastError());
            return 0;
        }
    }
    if ((rc = pass_args<IT>(ix, P, S, io, lk, A))) return rc;
    if (split) {
        const size_t m = 2 * (size_t)n, al = (m * 8 + 255) / 256 * 256;
        if ((rc = hsa_grow(&ix->d_split, &ix->d_split_cap, 3 * al))) return rc;
        char *d = (char *)ix->d_split;
        A.split = 1;
        A.sp_off = (uint64_t *)d;
        A.sp_n = (int32_t *)(d + al);
        A.sp_q = (uint32_t *)(d + al + al / 2);
        A.sp_p = (uint32_t *)(d + 2 * al);
        if (!P.huge && (rc = help_args<IT>(ix, A, m, P, st))) return rc;
    }
    if (first) HSA_HIP(hipMemsetAsync(io.ctr, 0, CTR_SLOTS * sizeof(unsigned long long), st));
    // cost order: the main pass of a batch with more reads than the chip has lanes
    // (HSA_ORDER=0/1 forbids / forces it)
    const char *oe = getenv("HSA_ORDER");
    const bool order = !split && !lk.n_dev && first && n > 0 &&
                       (oe ? atoi(oe) != 0 : (size_t)n > P.resident);
    uint32_t *d_oh = nullptr;
    if (order) {
        char *tail = (char *)A.wq + 4 * (size_t)n;
        A.wkey = (uint8_t *)tail;
        // the tail-length key: config 2 k_search 18.5-18.9 -> 17.9-18.0 ms, config 3 and 5 1-2 %
        // (profiles/r03_ab2_okey_*); HSA_ORDER_KEY=0: the final bid alone
        static const uint32_t okey = getenv("HSA_ORDER_KEY") ? (uint32_t)atoi(getenv("HSA_ORDER_KEY")) : 1u;
        A.okey = okey;
        const size_t ko = (2 * (size_t)n + 15) / 16 * 16;
        d_oh = (uint32_t *)(tail + ko);
        HSA_HIP(hipMemsetAsync(d_oh, 0, 32 * 4, st));
    }
    // lazy forward rows: the main pass of a batch searched one read per lane computes a
    // read's forward row only when its rc search cannot hit; the reads whose rc search
    // finds nothing without one get it in the forward pass below.  One launch computes both
    // kinds of row (k_widths_lazy), so it saves the rows of the reads whose rc strand can
    // hit without a second width launch.  By default for ungapped searches of reads of 100
    // bases or more (config 2, three handles: 66.7-68.1 against 64.9-67.6 M reads/s eager in
    // seven pairs, k_widths' read requests 216 -> 189 M per launch) and for gapped ones from
    // 200 bases: config 3's 100 bp reads lose 3 % to the forward pass, a second k_search
    // launch with a long gapped tail (profiles/lazyrows_ab.log).  HSA_LAZY=0 / 1 forbids /
    // forces it
    const char *le = getenv("HSA_LAZY");
    const int lazy_min = P.gaps ? HSA_LAZY_MIN_LEN_GAPPED : HSA_LAZY_MIN_LEN;
    const bool lazy = !split && !lk.n_dev && first && n > 0 && (le ? atoi(le) != 0 : io.max_len >= lazy_min);
    unsigned long long *d_fwd_n = nullptr;
    if (lazy) {
        // [count | forward-pass list (n) | rmap (n)]
        if ((rc = hsa_grow(&ix->d_fwd, &ix->d_fwd_cap, 512 + 8 * (size_t)n))) return rc;
        d_fwd_n = (unsigned long long *)ix->d_fwd;
        HSA_HIP(hipMemsetAsync(d_fwd_n, 0, 16, st));
        A.fwd_n = d_fwd_n;
        A.fwd_list = (int32_t *)((char *)ix->d_fwd + 128);
        A.rmap = A.fwd_list + ((size_t)n + 31) / 32 * 32;
    }
    if (lazy) {
        const unsigned rblocks = (unsigned)(((size_t)n + BLOCK - 1) / BLOCK);
        if (P.wide) hipLaunchKernelGGL((k_widths_lazy<uint16_t, IT>), dim3(rblocks), dim3(BLOCK), 0, st, A);
        else if (P.snib) hipLaunchKernelGGL((k_widths_lazy<uint8_t, IT, true>), dim3(rblocks), dim3(BLOCK), 0, st, A);
        else hipLaunchKernelGGL((k_widths_lazy<uint8_t, IT>), dim3(rblocks), dim3(BLOCK), 0, st, A);
    } else {
        size_t wblocks = ((size_t)n * 2 + BLOCK - 1) / BLOCK;
        if (wblocks < 1) wblocks = 1;
        if (P.wide) hipLaunchKernelGGL((k_widths<uint16_t, IT>), dim3((unsigned)wblocks), dim3(BLOCK), 0, st, A);
        else if (P.snib) hipLaunchKernelGGL((k_widths<uint8_t, IT, true>), dim3((unsigned)wblocks), dim3(BLOCK), 0, st, A);
        else hipLaunchKernelGGL((k_widths<uint8_t, IT>), dim3((unsigned)wblocks), dim3(BLOCK), 0, st, A);
    }
    HSA_HIP(hipGetLastError());
    if (order) {
        int32_t *d_perm = (int32_t *)(d_oh + 32);
        const unsigned nb = (unsigned)(((size_t)n + BLOCK - 1) / BLOCK);
        hipLaunchKernelGGL(k_order_hist, dim3(nb), dim3(BLOCK), 0, st, A, d_oh);
        hipLaunchKernelGGL(k_order_scan, dim3(1), dim3(1), 0, st, d_oh);
        hipLaunchKernelGGL(k_order_scatter, dim3(nb), dim3(BLOCK), 0, st, A, d_oh, d_perm);
        HSA_HIP(hipGetLastError());
        A.perm = d_perm;
    }
    if (ix->ev_split && first) HSA_HIP(hipEventRecord(ix->ev_split, st));   // the main pass only
    launch_search<IT>(P, A, st);
    HSA_HIP(hipGetLastError());
    if (lazy) {
        // the forward pass: the forward rows and the forward-strand searches of the reads
        // the main pass listed (count on the device; queue head ctr[CTR_Q_FWD]); its overflows go
        // to the same re-run list as the main pass's
        SearchArgs F = A;
        F.job_list = A.fwd_list; F.n_dev = d_fwd_n; F.qctr = CTR_Q_FWD; F.fwd_only = 1;
        F.fwd_list = nullptr; F.fwd_n = nullptr; F.wkey = nullptr; F.perm = nullptr; F.rmap = nullptr;
        const unsigned rblocks = (unsigned)(((size_t)n + BLOCK - 1) / BLOCK);
        if (P.wide) hipLaunchKernelGGL((k_widths_fwd<uint16_t, IT>), dim3(rblocks), dim3(BLOCK), 0, st, F);
        else if (P.snib) hipLaunchKernelGGL((k_widths_fwd<uint8_t, IT, true>), dim3(rblocks), dim3(BLOCK), 0, st, F);
        else hipLaunchKernelGGL((k_widths_fwd<uint8_t, IT>), dim3(rblocks), dim3(BLOCK), 0, st, F);
        HSA_HIP(hipGetLastError());
        launch_search<IT>(P, F, st);
        HSA_HIP(hipGetLastError());
    }
    if (split) {
        const unsigned nb = (unsigned)(((size_t)n + BLOCK - 1) / BLOCK);
        hipLaunchKernelGGL(k_split_finalize, dim3(nb), dim3(BLOCK), 0, st, A);
        HSA_HIP(hipGetLastError());
        if (getenv("HSA_VERBOSE")) {
            fprintf(stderr, "[hsa] strand-split main pass: %d reads on %zu lanes\n", n, P.lanes);
            if (A.fr_c) {
                unsigned long long c[9];
                HSA_HIP(hipMemcpyAsync(c, A.fr_c, sizeof c, hipMemcpyDeviceToHost, st));
                HSA_HIP(hipStreamSynchronize(st));
                fprintf(stderr, "[hsa] helpers: %llu offers (%llu refused), %llu chunks, %llu sub-searches, %llu strands "
                                "answered by them, %llu rank queries in sub-searches\n", c[4], c[5], c[0], c[6], c[7], c[8]);
            }
        }
    }
    return 0;
}

static int jobs_limits(const hsa_job_t *jobs, int n, int &max_len, int &max_seed)
{
    max_len = 0; max_seed = 0;
    for (int j = 0; j < n; ++j) {
        if (jobs[j].len > ANY_MAX_LEN) { hsa_set_error("read %d longer than %d (gap_entry_t.info, bwtgap.c:157)", j, ANY_MAX_LEN); return HSA_E_ARG; }
        if (jobs[j].max_diff < -1) { hsa_set_error("max_diff out of range"); return HSA_E_ARG; }
        if ((int)jobs[j].len > max_len) max_len = (int)jobs[j].len;
        if ((int)jobs[j].len > jobs[j].seed_len && jobs[j].seed_len > max_seed) max_seed = jobs[j].seed_len;
    }
    return 0;
}

// regimes + bucket maps into the staging area, the first 1536 bytes of ix->d_in:
// [regimes (256 B)][bmap 2*MAXS].  Repeated launches with the same options skip the copy
// (a pageable H2D copy would otherwise wait for the stream and stall the host between
// launches) unless the area moved or the caller forces it.
static int stage_regimes(hsa_index *ix, const hsa_regime_t *regimes, int n_regimes, int &nb, hipStream_t st,
                         bool force = false)
{
    void *before = ix->d_in;
    if (int rc = hsa_grow(&ix->d_in, &ix->d_in_cap, 1536)) return rc;
    force = force || before != ix->d_in;
    static_assert(256 + 2 * MAXS <= sizeof(ix->staged), "staging copy");
    uint8_t host[256 + 2 * MAXS];
    memset(host, 0xFF, sizeof host);
    memcpy(host, regimes, sizeof(hsa_regime_t) * n_regimes);
    nb = 1;
    int ntab = 8;
    for (int r = 0; r < n_regimes; ++r) {
        int k = bucket_map(regimes[r], host + 256 + r * MAXS);
        nb = k > nb ? k : nb;
        ntab = regimes[r].n_stacks > ntab ? regimes[r].n_stacks : ntab;
    }
    if (nb > MAXB) { hsa_set_error("%d reachable scores: at most %d stack buckets", nb, MAXB); return HSA_E_ARG; }
    ix->staged_ntab = (ntab + 7) / 8 * 8;
    ix->staged_mmb = mm_buckets(regimes, n_regimes, host + 256);
    ix->staged_min_entries = regimes[0].max_entries;
    for (int r = 1; r < n_regimes; ++r)
        if (regimes[r].max_entries < ix->staged_min_entries) ix->staged_min_entries = regimes[r].max_entries;
    if (!force && ix->staged_valid && memcmp(ix->staged, host, sizeof host) == 0) return 0;
    memcpy(ix->staged, host, sizeof host);
    ix->staged_valid = 1;
    HSA_HIP(hipMemcpyAsync(ix->d_in, ix->staged, sizeof host, hipMemcpyHostToDevice, st));
    HSA_HIP(hipStreamSynchronize(st));
    return 0;
}

// The capacity cascade of one search, queued on st without a host sync: the MAIN pass over
// io's jobs, then the exact re-runs of the reads that overflowed their lane's capacity, BIG
// for MAIN's (count ctr[CTR_OVF_MAIN]) and HUGE for BIG's (count ctr[CTR_OVF_BIG]).  The
// counts stay on the device, so an empty re-run is a launch whose lanes exit at once.
// main: the MAIN pass's device job count (or null) and queue head, CTR_Q_MAIN (the pass
// zeroes the counters) or CTR_Q_MG (zero_ctr: zeroed here; else the caller has).
// ev_split (or null: ix->evm): recorded between the MAIN pass's widths and its search.
template <typename IT = uint32_t>
static int run_capacity_passes(hsa_index *ix, const RegimePlan &C, const PassIO &io, PassLink main, bool zero_ctr,
                               hipEvent_t ev_split, hipStream_t st)
{
    LaunchPlan P, B, H;
    int rc;
    if ((rc = plan_launch<IT>(ix, io.n, io.max_len, io.max_seed, C, PASS_MAIN, P)) ||
        (rc = plan_launch<IT>(ix, io.n, io.max_len, io.max_seed, C, PASS_BIG, B)) ||
        (rc = plan_launch<IT>(ix, io.n, io.max_len, io.max_seed, C, PASS_HUGE, H)))
        return rc;
    if ((rc = hsa_grow(&ix->d_ovf, &ix->d_ovf_cap, (size_t)io.n * 4 + 64)) ||
        (rc = hsa_grow(&ix->d_ovf2, &ix->d_ovf2_cap, (size_t)io.n * 4 + 64)))
        return rc;
    if (zero_ctr) HSA_HIP(hipMemsetAsync(io.ctr, 0, CTR_SLOTS * sizeof(unsigned long long), st));
    int32_t *const ovf = (int32_t *)ix->d_ovf, *const ovf2 = (int32_t *)ix->d_ovf2;
    main.ovf_list = ovf;
    const PassLink big{.ovf_list = ovf2, .n_dev = io.ctr + CTR_OVF_MAIN, .qctr = CTR_Q_BIG, .ovf_ctr = CTR_OVF_BIG};
    const PassLink huge{.ovf_list = nullptr, .n_dev = io.ctr + CTR_OVF_BIG, .qctr = CTR_Q_HUGE};
    PassIO io_b = io, io_h = io;
    io_b.list = ovf; io_h.list = ovf2;
    if (ev_split) ix->ev_split = ev_split;
    rc = launch_pass<IT>(ix, P, ix->main, io, main, st);
    if (!rc) rc = launch_pass<IT>(ix, B, ix->big, io_b, big, st);
    if (!rc) rc = launch_pass<IT>(ix, H, ix->huge, io_h, huge, st);
    ix->ev_split = ix->evm;
    return rc;
}

// ---------------------------------------------------------------- the k_search_any passes
// Device buffers of one search's k_search_any passes (in ix->d_any_aux): the regimes, the
// counters and the job lists; and the host's regimes, which size the passes.
enum {
    ANY_N_FAST = 0,                // jobs for k_search (k_partition)
    ANY_N_ANY = 1,                 // jobs for k_search_any (k_partition)
    ANY_Q = 2,                     // the first pass's queue head
    ANY_N_OVF = 3,                 // jobs it hands to its large-capacity pass
    ANY_Q_BIG = 4                  // that pass's queue head
};

struct AnyBufs {
    hsa_regime_t *reg;
    unsigned long long *cnt;
    int32_t *l_fast, *l_any, *l_ovf;
    const hsa_regime_t *regimes;
    int n_regimes;
};

static int any_prepare(hsa_index *ix, const hsa_regime_t *regimes, int n_regimes, size_t n, hipStream_t st, AnyBufs &B)
{
    const size_t lb = (n * 4 + 255) / 256 * 256;
    if (ix->d_any_cap > ((size_t)8 << 30)) {       // a past large pass's stacks: give them back
        HSA_HIP(hipStreamSynchronize(st));
        (void)hipFree(ix->d_any);
        ix->d_any = nullptr;
        ix->d_any_cap = 0;
    }
    int rc = hsa_grow(&ix->d_any_aux, &ix->d_any_aux_cap, 512 + 3 * lb);
    if (rc) return rc;
    char *d = (char *)ix->d_any_aux;
    B.reg = (hsa_regime_t *)d;
    B.cnt = (unsigned long long *)(d + 256);
    B.l_fast = (int32_t *)(d + 512);
    B.l_any = (int32_t *)(d + 512 + lb);
    B.l_ovf = (int32_t *)(d + 512 + 2 * lb);
    B.regimes = regimes;
    B.n_regimes = n_regimes;
    HSA_HIP(hipMemcpyAsync(B.reg, regimes, sizeof(hsa_regime_t) * n_regimes, hipMemcpyHostToDevice, st));
    HSA_HIP(hipMemsetAsync(B.cnt, 0, 64, st));
    HSA_HIP(hipStreamSynchronize(st));
    return 0;
}

// One k_search_any pass over io's jobs (their count on the device in n_dev, or io.n).
// big: the large-capacity pass (pools up to the reference's max_entries bound, 262 144
// hits, few lanes) for the jobs the first pass overflowed; the first pass lists those.
template <typename IT>
static int any_pass(hsa_index *ix, const AnyBufs &B, const PassIO &io, const unsigned long long *n_dev, bool big,
                    hipStream_t st)
{
    const uint32_t max_len = (uint32_t)io.max_len, max_seed = (uint32_t)io.max_seed;
    size_t n_bound = (size_t)io.n;
    if (n_bound == 0) return 0;
    if (big && n_dev) {
        // the large pass's lanes hold whole stacks: size it by the reads that overflowed
        // (one stream sync; this path only runs for reads/regimes k_search cannot hold)
        unsigned long long cnt = 0;
        HSA_HIP(hipMemcpyAsync(&cnt, n_dev, sizeof cnt, hipMemcpyDeviceToHost, st));
        HSA_HIP(hipStreamSynchronize(st));
        if (cnt == 0) return 0;
        n_bound = (size_t)cnt;
    }
    AnyArgs A;
    memset(&A, 0, sizeof A);
    A.fwd = RankDir{ix->blk[0], ix->isa0};
    A.rev = RankDir{ix->blk[1], ix->risa0};
    A.fwd64 = hsa_rank_dir64(ix, 0);
    A.rev64 = hsa_rank_dir64(ix, 1);
    A.T = ix->T; A.T64 = ix->T64;
    memcpy(A.C, ix->C, sizeof A.C);
    memcpy(A.C64, ix->C64, sizeof A.C64);
    A.regimes = B.reg; A.jobs = io.jobs; A.list = io.list; A.n_dev = n_dev; A.n_host = n_dev ? 0 : io.n;
    A.codes = io.codes;
    A.mg = io.mg.d_mg; A.cw = io.mg.d_cw;
    A.n_aln = io.n_aln; A.flags = io.flags; A.hit_off = io.hit_off; A.hits = io.hits; A.hit_cap = io.hit_cap;
    A.ctr = io.ctr;
    A.qhead = B.cnt + (big ? ANY_Q_BIG : ANY_Q);
    A.ovf_list = big ? nullptr : B.l_ovf;
    A.ovf_n = big ? nullptr : B.cnt + ANY_N_OVF;
    uint32_t nst = 1, max_entries = 0;
    for (int r = 0; r < B.n_regimes; ++r) {
        nst = (uint32_t)B.regimes[r].n_stacks > nst ? (uint32_t)B.regimes[r].n_stacks : nst;
        max_entries = (uint32_t)B.regimes[r].max_entries > max_entries ? (uint32_t)B.regimes[r].max_entries : max_entries;
    }
    // capacities: live entries never exceed max_entries + 9 (bwtgap.c:150-151)
    const uint64_t want = (uint64_t)max_entries + 16u;
    static const uint32_t pcap1 = getenv("HSA_ANY_PCAP") ? (uint32_t)atoi(getenv("HSA_ANY_PCAP")) : 8192u;   // A/B only
    const uint32_t pcap = big ? (uint32_t)(want < (4ull << 20) ? want : (4ull << 20)) : pcap1;
    const uint32_t hcap = big ? 262144u : 512u;
    const size_t lb = any_layout<IT>(A, max_len, max_seed, nst, pcap, hcap, 10);
    // the large pass holds whole stacks (~75 MB a lane at max_entries 2 000 000) and its
    // reads are the slow ones: as many lanes as half the free HBM allows, up to 64 GB
    size_t budget = (size_t)4 << 30, lanes_max = 16384;
    if (big) {
        size_t fr = 0, tot = 0;
        HSA_HIP(hipMemGetInfo(&fr, &tot));
        budget = fr / 2 < ((size_t)64 << 30) ? fr / 2 : ((size_t)64 << 30);
        lanes_max = 4096;
    }
    size_t lanes = n_bound < lanes_max ? n_bound : lanes_max;
    if (lanes * lb > budget) lanes = budget / lb;
    if (lanes < 1) lanes = 1;
    A.nlanes = (uint32_t)lanes;
    if (lanes * lb + 256 > ix->d_any_cap) HSA_HIP(hipStreamSynchronize(st));   // a pass may still use the old one
    int rc = hsa_grow(&ix->d_any, &ix->d_any_cap, lanes * lb + 256);
    if (rc) return rc;
    A.scratch = (uint8_t *)ix->d_any;
    if (getenv("HSA_VERBOSE"))
        fprintf(stderr, "[hsa] k_search_any%s: %zu lanes x %zu B (pool %u, hits %u, %u stacks, reads <= %u bp)\n",
                big ? " (large pass)" : "", lanes, lb, pcap, hcap, nst, max_len);
    hipLaunchKernelGGL(k_search_any<IT>, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, A);
    HSA_HIP(hipGetLastError());
    return 0;
}

// k_search_any over io's jobs: the first pass, then the large pass over the jobs it listed.
template <typename IT>
static int any_passes(hsa_index *ix, const AnyBufs &B, const PassIO &io, const unsigned long long *n_dev, hipStream_t st)
{
    PassIO big = io;
    big.list = B.l_ovf;                              // the jobs the first pass could not hold
    const int rc = any_pass<IT>(ix, B, io, n_dev, false, st);
    return rc ? rc : any_pass<IT>(ix, B, big, B.cnt + ANY_N_OVF, true, st);
}

// hsa_search_device / hsa_search_device64: the main pass over a device-resident batch,
// then the BIG and HUGE capacity re-runs, all queued on one stream without a host sync.
template <typename IT>
static int search_device_impl(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const hsa_device_batch_t *b,
                              void *stream)
{
    // regimes: host array; staged into the index's staging area
    if (n_regimes < 1 || n_regimes > 2) { hsa_set_error("1 or 2 regimes"); return HSA_E_ARG; }
    if (sizeof(IT) == 8 && !ix->wide) { hsa_set_error("not a 64-bit index (hsa_index_create_device64)"); return HSA_E_ARG; }
    int rc = check_regimes(regimes, n_regimes);
    if (rc) return rc;
    if (b->max_len < 1 || b->max_len > ANY_MAX_LEN || b->max_seed < 0 || b->max_seed > ANY_MAX_LEN) {
        hsa_set_error("max_len/max_seed out of range");
        return HSA_E_ARG;
    }
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = stream ? (hipStream_t)stream : ix->stream;
    hipEvent_t *pe = ix->pev[ix->pev_n % hsa_index::PASS_RING];
    for (int j = 0; j < 3; ++j)
        if (!pe[j]) HSA_HIP(hipEventCreate(&pe[j]));
    // reads longer than k_search holds, or a regime outside its layouts: k_search_any
    // (all jobs for such a regime; the long ones, partitioned on the device, otherwise)
    const bool fast_rg = fast_regimes(regimes, n_regimes);
    const bool any_path = !fast_rg || (uint32_t)b->max_len > FAST_MAX_LEN;
    AnyBufs AB{};
    if (any_path && (rc = any_prepare(ix, regimes, n_regimes, (size_t)b->n_jobs, st, AB))) return rc;
    PassIO io{.jobs = b->d_jobs, .list = nullptr, .n = b->n_jobs, .codes = b->d_codes, .n_aln = b->d_n_aln,
              .flags = b->d_flags, .hit_off = b->d_hit_off, .hits = b->d_hits, .hit_cap = b->hit_cap,
              .ctr = (unsigned long long *)b->d_counters, .max_len = b->max_len, .max_seed = b->max_seed, .mg = {}};
    if (!fast_rg) {
        ++ix->pev_n;
        HSA_HIP(hipEventRecord(pe[0], st));
        HSA_HIP(hipEventRecord(pe[1], st));
        HSA_HIP(hipMemsetAsync(io.ctr, 0, CTR_SLOTS * sizeof(unsigned long long), st));
        if ((rc = any_passes<IT>(ix, AB, io, nullptr, st))) return rc;
        HSA_HIP(hipEventRecord(pe[2], st));
        return 0;
    }
    RegimePlan C = regime_plan(regimes, n_regimes);
    if ((rc = stage_regimes(ix, regimes, n_regimes, C.nb, st))) return rc;
    ++ix->pev_n;
    HSA_HIP(hipEventRecord(pe[0], st));
    PassIO fast = io;                                // k_search's share: the reads of up to FAST_MAX_LEN bases
    fast.max_len = (uint32_t)b->max_len > FAST_MAX_LEN ? (int)FAST_MAX_LEN : b->max_len;
    fast.max_seed = b->max_seed > fast.max_len ? fast.max_len : b->max_seed;
    PassLink main;
    if (any_path) {                                  // long reads in the batch: split it on the device
        const unsigned g = (unsigned)(((size_t)b->n_jobs + BLOCK - 1) / BLOCK);
        hipLaunchKernelGGL(k_partition, dim3(g ? g : 1), dim3(BLOCK), 0, st, b->d_jobs, b->n_jobs, FAST_MAX_LEN, AB.l_fast,
                           AB.l_any, AB.cnt);
        HSA_HIP(hipGetLastError());
        fast.list = AB.l_fast;
        main.n_dev = AB.cnt + ANY_N_FAST;
        io.list = AB.l_any;
    }
    if ((rc = run_capacity_passes<IT>(ix, C, fast, main, false, pe[1], st))) return rc;
    if (any_path && (rc = any_passes<IT>(ix, AB, io, AB.cnt + ANY_N_ANY, st))) return rc;
    HSA_HIP(hipEventRecord(pe[2], st));
    return 0;
}
