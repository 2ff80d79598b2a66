// hsa_splice_prefetch.h -- the splice path's searches ahead of its extensions: the older
// seeds-only pass, and the prefetch pass with its entry points for reads from the host
// (hsa_splice_prefetch_batch, hsa_splice_match_batch) and for a device batch
// (hsa_splice_device).  Included by hsa_search.hip alone, after hsa_search_launch.h.
#pragma once

static size_t al(size_t x) { return (x + 255) / 256 * 256; }      // device regions start 256-byte aligned

// ---------------------------------------------------------------- splice seeds
// The seed calls of bwt_splice_match (bwtgap.c:797-812) for every read the main pass
// flagged HSA_F_FALLBACK: one thread per (read, strand).  The strand's three seeds
// t = 0, 1, 2 (sl = len / 3, la_t = sl + (t == 2 ? len % 3 : 0)) search [t sl, t sl +
// la_t) of the strand sequence with the widths of its PREFIX of length la_t
// (bwtgap.c:807-809; bwt_cal_width type 1, bwtaln.c:84-97: forward extension on the
// reverse BWT).  The three prefixes share their first sl positions, so one chain over
// la_2 characters fills all three width slots; each slot ends with its own terminal
// {0, bid + 1} (bwtaln.c:113-114).
struct SeedArgs {
    RankDir rev;
    uint32_t T;
    uint32_t C[5];
    const hsa_job_t *rjobs;
    const uint8_t *rcodes;
    const uint32_t *rflags;
    uint32_t n_reads;
    int32_t max_seed_diff;
    uint32_t code_stride, pair_stride;   // per read: seed codes (bytes), width pairs
    hsa_job_t *jobs;
    hsa_mg_job_t *mg;
    uint8_t *codes;
    int32_t *cw;
    int32_t *list;
    unsigned long long *count;
    unsigned long long *ctr;
};

__global__ void __launch_bounds__(BLOCK) k_seed_prep(SeedArgs a)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t r = t >> 1, s = t & 1u;
    if (r >= a.n_reads || !(a.rflags[r] & HSA_F_FALLBACK)) return;
    const hsa_job_t R = a.rjobs[r];
    const uint32_t L = R.len, sl = L / 3u;
    if (sl < 1) return;
    const uint32_t la2 = sl + L % 3u;
    auto base = [&](uint32_t p) -> uint32_t {          // strand s, position p
        const uint32_t c = a.rcodes[R.off + (s ? L - 1u - p : p)];
        return s && c < 4 ? 3u - c : c;
    };
    // call i = 3 s + tt of read r: codes and width pairs at fixed offsets in the read's slots
    uint32_t coff[3], poff[3], la[3];
    {
        uint32_t co = 0, po = 0;
        for (uint32_t i = 0; i < 6; ++i) {
            const uint32_t l_i = sl + (i % 3 == 2 ? L % 3u : 0u);
            if (i / 3 == s) { coff[i % 3] = co; poff[i % 3] = po; la[i % 3] = l_i; }
            co += l_i; po += l_i + 1;
        }
    }
    uint8_t *const cbase = a.codes + (size_t)r * a.code_stride;
    int32_t *const wbase = a.cw + 2 * (size_t)r * a.pair_stride;
    uint32_t k = 0, l = a.T, bid = 0, bid_sl = 0, q = 0;
    for (uint32_t p = 0; p < la2; ++p) {
        const uint32_t c = base(p);
        if (c < 4) {
            uint32_t ok, ol;
            hsa_occ1_pair(a.rev, k, l + 1u, c, ok, ol);
            q += 2;
            const uint32_t cc = hsa_sel4(c, a.C[0], a.C[1], a.C[2], a.C[3]);
            k = cc + ok + 1u;
            l = cc + ol;
        }
        if (k > l || c > 3) { k = 0; l = a.T; ++bid; }
        const int32_t w = (int32_t)(l - k + 1u);
        for (uint32_t tt = 0; tt < 3; ++tt)
            if (p < la[tt]) { wbase[2 * (poff[tt] + p)] = w; wbase[2 * (poff[tt] + p) + 1] = (int32_t)bid; }
        if (p + 1 == sl) bid_sl = bid;
        // seed codes: strand position p belongs to seed tt = p / sl (the last seed runs to la2 + 2 sl)
    }
    for (uint32_t tt = 0; tt < 3; ++tt) {
        const uint32_t term_bid = (la[tt] == sl ? bid_sl : bid) + 1u;
        wbase[2 * (poff[tt] + la[tt])] = 0;
        wbase[2 * (poff[tt] + la[tt]) + 1] = (int32_t)term_bid;
        for (uint32_t p = 0; p < la[tt]; ++p) cbase[coff[tt] + p] = (uint8_t)base(tt * sl + p);
        const uint32_t j = r * 6u + 3u * s + tt;
        hsa_job_t J;
        J.off = (uint64_t)r * a.code_stride + coff[tt];
        J.len = la[tt];
        J.max_diff = a.max_seed_diff;
        J.seed_len = (int32_t)la[tt];
        J.regime = 0;
        a.jobs[j] = J;
        hsa_mg_job_t M;
        M.wb_off = (uint64_t)r * a.pair_stride + poff[tt];
        M.ws_off = 0;
        M.strand = (int32_t)s;
        M.seed = HSA_SEED_ALIAS;
        a.mg[j] = M;
    }
    const unsigned long long b0 = atomicAdd(a.count, 3ull);
    for (uint32_t tt = 0; tt < 3; ++tt) a.list[b0 + tt] = (int32_t)(r * 6u + 3u * s + tt);
    atomicAdd(&a.ctr[CTR_WIDTH_Q], (unsigned long long)q);
}

extern "C" int hsa_splice_seeds_device(hsa_index_t *ix, const hsa_regime_t *seed_regime, const hsa_seed_batch_t *b,
                                       void *stream)
{
    if (int rc0 = hsa_need32(ix)) return rc0;
    int rc = check_regimes(seed_regime, 1);
    if (rc) return rc;
    if (seed_regime->max_gapo != 0) { hsa_set_error("seed searches have no gap opens (bwtgap.c:772)"); return HSA_E_ARG; }
    if (b->max_len < 3 || b->max_len > 1023 || b->n_jobs < 0) { hsa_set_error("max_len/n_jobs out of range"); return HSA_E_ARG; }
    const size_t n = (size_t)b->n_jobs, calls = 6 * n;
    if (n == 0) return 0;
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = stream ? (hipStream_t)stream : ix->stream;
    const uint32_t code_stride = (uint32_t)(2 * b->max_len), pair_stride = (uint32_t)(2 * b->max_len + 6);
    const size_t o_mg = al(calls * sizeof(hsa_job_t)), o_list = o_mg + al(calls * sizeof(hsa_mg_job_t));
    const size_t o_fl = o_list + al(calls * 4), o_cnt = o_fl + al(calls * 4), o_codes = o_cnt + 256;
    const size_t o_cw = o_codes + al(n * code_stride), total = o_cw + n * pair_stride * 8 + 256;
    if ((rc = hsa_grow(&ix->d_seed, &ix->d_seed_cap, total))) return rc;
    char *d = (char *)ix->d_seed;
    unsigned long long *cnt = (unsigned long long *)(d + o_cnt);
    unsigned long long *ctr = (unsigned long long *)b->d_counters;
    HSA_HIP(hipMemsetAsync(cnt, 0, 8, st));
    SeedArgs S;
    S.rev = RankDir{ix->blk[1], ix->risa0};
    S.T = ix->T;
    memcpy(S.C, ix->C, sizeof S.C);
    S.rjobs = b->d_jobs; S.rcodes = b->d_codes; S.rflags = b->d_flags; S.n_reads = (uint32_t)n;
    S.max_seed_diff = seed_regime->max_diff;
    S.code_stride = code_stride; S.pair_stride = pair_stride;
    S.jobs = (hsa_job_t *)d; S.mg = (hsa_mg_job_t *)(d + o_mg); S.codes = (uint8_t *)(d + o_codes);
    S.cw = (int32_t *)(d + o_cw); S.list = (int32_t *)(d + o_list); S.count = cnt; S.ctr = ctr;
    RegimePlan C = regime_plan(seed_regime, 1);
    C.nib_ok = false; C.snib_ok = false;    // caller widths: byte rows
    if ((rc = stage_regimes(ix, seed_regime, 1, C.nb, st))) return rc;
    // the counters are zeroed here, before k_seed_prep adds the width queries to them
    HSA_HIP(hipMemsetAsync(ctr, 0, CTR_SLOTS * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_seed_prep, dim3((unsigned)((2 * n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, S);
    HSA_HIP(hipGetLastError());
    HSA_HIP(hipEventRecord(ix->ev0, st));
    const PassIO io{.jobs = S.jobs, .list = S.list, .n = (int)calls, .codes = S.codes, .n_aln = b->d_n_aln,
                    .flags = (uint32_t *)(d + o_fl), .hit_off = b->d_hit_off, .hits = b->d_hits, .hit_cap = b->hit_cap,
                    .ctr = ctr, .max_len = b->max_len / 3 + 2, .max_seed = 0, .mg = {S.mg, S.cw}};
    if ((rc = run_capacity_passes(ix, C, io, PassLink{.n_dev = cnt, .qctr = CTR_Q_MG}, false, nullptr, st))) return rc;
    HSA_HIP(hipEventRecord(ix->ev1, st));
    return 0;
}

// ---------------------------------------------------------------- splice prefetch
// hsa_splice_prefetch_batch (include/hsa_gpu.h): every width, seed search, anchor search
// and SA -> position lookup bwt_splice_match (bwtgap.c:748-1332) can make before its
// first extension, for a batch of fallback reads, in one device pass.
struct PfArgs {
    RankDir fwd, rev;
    uint32_t T;
    uint32_t C[5];
    uint32_t n, max_len, sc, rs, cws;       // reads, longest, strand-code stride (bytes), row stride, cw stride (pairs)
    const uint32_t *lens;
    const uint64_t *offs;
    const uint8_t *codes;                   // the reads as bwa_seq_t.seq holds them
    const int32_t *amd;                     // per read: the anchors' max_diff
    int32_t seed_max_diff;
    uint8_t *scodes;                        // strand s of read r at (2 r + s) * sc
    int32_t *rows;                          // 6 rows per read, rs pairs each (W1 s0/s1, W12 s0/s1, W0 s0/s1)
    hsa_job_t *jobs;                        // 8 calls per read
    hsa_mg_job_t *mg;
    int32_t *cw;                            // per call cws pairs
    int32_t *list;                          // seed calls, then anchor calls
    int32_t *call_n;                        // 8 n
    uint32_t *call_fl;
    unsigned long long *acount;             // anchor calls listed
    const unsigned long long *d_n;          // the reads' count on the device (hsa_splice_device), or null: n
    uint64_t cwd;                           // the caller-width base is rows: cw starts cwd pairs after it
    uint32_t prefix;                        // seeds read their widths from the W1 rows (HSA_MG_PREFIX)
    const void *ktw;                        // the width trie (hsa_trie.h) for type-1 rows, depth ktd (0: none)
    uint32_t ktd;
};

__device__ __forceinline__ uint32_t pf_n(const PfArgs &a) { return a.d_n ? (uint32_t)*a.d_n : a.n; }

// thread (r, s, kind): kind 0 bwt_cal_width type 1 of the whole strand (and the strand's
// codes), 1 type 1 of its last 12 bases, 2 type 0 of the whole strand (bwtaln.c:73-116;
// the same chains as k_width / k_width0)
__global__ void __launch_bounds__(BLOCK) k_pf_rows(PfArgs a)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t r = t / 6u, s = (t % 6u) & 1u, kind = (t % 6u) >> 1;
    if (r >= pf_n(a)) return;
    const uint32_t L = a.lens[r];
    const uint64_t off = a.offs[r];
    int32_t *const o = a.rows + 2 * ((size_t)r * 6u + kind * 2u + s) * a.rs;
    uint32_t k = 0, l = a.T, bid = 0;
    // the strand's base at p from the 4-byte code word of the last one, held in
    // registers: a chain walks its read one position per step (the codes are 4-byte
    // aligned and padded past the last read)
    uint32_t cq = 0xFFFFFFFFu, cword = 0;
    auto base = [&](uint32_t p) -> uint32_t {
        const uint64_t ix = off + (s ? L - 1u - p : p);
        if ((uint32_t)(ix >> 2) != cq) {
            cword = *reinterpret_cast<const uint32_t *>(a.codes + (ix & ~(uint64_t)3));
            cq = (uint32_t)(ix >> 2);
        }
        const uint32_t c = (cword >> (((uint32_t)ix & 3u) * 8u)) & 0xFFu;
        return s && c < 4 ? 3u - c : c;     // the reverse complement (bwtaln.c:326-333)
    };
    if (kind == 0 || kind == 1) {
        if (kind == 1 && L < 12u) return;
        const uint32_t p0 = kind == 1 ? L - 12u : 0u, n = kind == 1 ? 12u : L;
        uint8_t *const sc = a.scodes + (size_t)(2u * r + s) * a.sc;
        uint32_t tl = 0, tix = 0;            // characters since the last reset and their trie node
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t c = base(p0 + i);
            if (kind == 0) sc[i] = (uint8_t)c;
            if (c < 4) {
                if (tl < a.ktd) {            // the same forward extension, from the width trie
                    tix = tix * 4u + c;
                    ++tl;
                    trie_w_load<uint32_t>(a.ktw, trie_base(tl) + tix, k, l);
                } else {
                    uint32_t ok, ol;
                    hsa_occ1_pair(a.rev, k, l + 1u, c, ok, ol);
                    const uint32_t cc = hsa_sel4(c, a.C[0], a.C[1], a.C[2], a.C[3]);
                    k = cc + ok + 1u;
                    l = cc + ol;
                }
            }
            if (k > l || c > 3) { k = 0; l = a.T; ++bid; tl = 0; tix = 0; }
            *reinterpret_cast<int2 *>(o + 2 * i) = make_int2((int32_t)(l - k + 1u), (int32_t)bid);
        }
        *reinterpret_cast<int2 *>(o + 2 * n) = make_int2(0, (int32_t)(bid + 1u));
        return;
    }
    *reinterpret_cast<int2 *>(o) = make_int2(0, 0);       // entry 0: never written by the reference
    for (uint32_t i = L - 1u; i > 0 && L > 0; --i) {
        const uint32_t c = base(i);
        if (c < 4) {
            uint32_t ok, ol;
            hsa_occ1_pair(a.fwd, k, l + 1u, c, ok, ol);
            const uint32_t cc = hsa_sel4(c, a.C[0], a.C[1], a.C[2], a.C[3]);
            k = cc + ok + 1u;
            l = cc + ol;
        }
        if (k > l || c > 3) { k = 0; l = a.T; ++bid; }
        *reinterpret_cast<int2 *>(o + 2 * i) = make_int2((int32_t)(l - k + 1u), (int32_t)bid);
    }
    *reinterpret_cast<int2 *>(o + 2 * L) = make_int2(0, (int32_t)(bid + 1u));
}

// thread (r, call 0..5): seed t of strand s (bwtgap.c:797-812): the strand [t sl, t sl + la)
// with width_back = width_seed = the strand prefix's widths (bwt_cal_width of la bases,
// :807): the first la entries of W1 and the terminal {0, bid + 1}
__global__ void __launch_bounds__(BLOCK) k_pf_seeds(PfArgs a)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t r = t / 6u, i = t % 6u, s = i / 3u, tt = i % 3u;
    if (r >= pf_n(a)) return;
    const uint32_t L = a.lens[r], sl = L / 3u, la = sl + (tt == 2u ? L % 3u : 0u);
    const uint32_t call = 8u * r + i;
    a.list[6u * r + i] = (int32_t)call;
    const int32_t *const w1 = a.rows + 2 * ((size_t)r * 6u + s) * a.rs;
    hsa_mg_job_t M;
    if (a.prefix) {                         // the search reads the W1 row's prefix itself
        M.wb_off = ((uint64_t)r * 6u + s) * a.rs;
        M.ws_off = HSA_MG_PREFIX;
    } else {                                // a copy, which the search's width_back export rewrites
        int32_t *const cw = a.cw + 2 * (size_t)call * a.cws;
        for (uint32_t p = 0; p < la; ++p) { cw[2 * p] = w1[2 * p]; cw[2 * p + 1] = w1[2 * p + 1]; }
        cw[2 * la] = 0;
        cw[2 * la + 1] = (la ? w1[2 * (la - 1u) + 1] : 0) + 1;
        M.wb_off = a.cwd + (uint64_t)call * a.cws;
        M.ws_off = 0;
    }
    hsa_job_t J;
    J.off = (uint64_t)(2u * r + s) * a.sc + tt * sl;
    J.len = la;
    J.max_diff = a.seed_max_diff;
    J.seed_len = (int32_t)la;
    J.regime = 0;
    a.jobs[call] = J;
    M.strand = (int32_t)s;
    M.seed = HSA_SEED_ALIAS;
    a.mg[call] = M;
}

// thread (r, s): the 12-mer anchor bwt_splice_match searches after an extension when the
// strand's seed pattern is 3 (seeds 0 and 1 hit: its last 12 bases with their own widths,
// bwtgap.c:911-919) or 6 (seeds 1 and 2: its first 12 with the whole strand's widths,
// :1187-1192); width_seed NULL, the anchor regime, the read's max_diff
__global__ void __launch_bounds__(BLOCK) k_pf_anchors(PfArgs a)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t r = t >> 1, s = t & 1u;
    if (r >= pf_n(a)) return;
    const uint32_t L = a.lens[r], call = 8u * r + 6u + s;
    const int32_t *const cn = a.call_n + 8u * r + 3u * s;
    const uint32_t *const cf = a.call_fl + 8u * r + 3u * s;
    const bool done = !(cf[0] & HSA_F_OVERFLOW) && !(cf[1] & HSA_F_OVERFLOW) && !(cf[2] & HSA_F_OVERFLOW);
    const uint32_t mask = (cn[0] > 0) | (cn[1] > 0) << 1 | (cn[2] > 0) << 2;
    if (L <= 12u || !done || (mask != 3u && mask != 6u)) { a.call_n[call] = -1; return; }
    const bool tail = mask == 3u;
    const int32_t *const src = a.rows + 2 * ((size_t)r * 6u + (tail ? 2u : 0u) + s) * a.rs;
    int32_t *const cw = a.cw + 2 * (size_t)call * a.cws;
    for (uint32_t p = 0; p < 13u; ++p) { cw[2 * p] = src[2 * p]; cw[2 * p + 1] = src[2 * p + 1]; }
    hsa_job_t J;
    J.off = (uint64_t)(2u * r + s) * a.sc + (tail ? L - 12u : 0u);
    J.len = 12u;
    J.max_diff = a.amd[r];
    J.seed_len = 0;
    J.regime = 1;
    a.jobs[call] = J;
    hsa_mg_job_t M;
    M.wb_off = a.cwd + (uint64_t)call * a.cws;
    M.ws_off = 0;
    M.strand = (int32_t)s;
    M.seed = HSA_SEED_NONE;
    a.mg[call] = M;
    a.list[6u * a.n + atomicAdd(a.acount, 1ull)] = (int32_t)call;
}

// The SA indices bwt_aln_corelate_check can look up for a call's hits: k .. min(l, k + 49)
// (bwtgap.c:698 reads at most 10 per hit, :711 at most 50; the loop bounds in bwtint_t)
__device__ __forceinline__ uint32_t pf_sa_span(uint32_t k, uint32_t l)
{
    const uint32_t lim = k + 50u;                     // wraps as the reference's bound does
    if (k > l || lim < k) return 0;
    const uint32_t hi = l < lim - 1u ? l : lim - 1u;
    return hi - k + 1u;
}

struct PfSaArgs {
    uint32_t n_calls;
    const int32_t *call_n;
    const uint64_t *call_hit;                // relative to the call's hit region
    const uint32_t *hits_s, *hits_a;         // seed calls' and anchor calls' hit regions
    unsigned long long *call_sa;             // out: first SA result of the call
    unsigned long long *total;
    uint32_t *idx;                           // pass 2: the indices
};

__global__ void __launch_bounds__(BLOCK) k_pf_sa(PfSaArgs a, int fill)
{
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= a.n_calls) return;
    const int32_t n = a.call_n[c];
    if (n <= 0) { if (!fill) a.call_sa[c] = 0; return; }
    const uint32_t *h = ((c & 7u) >= 6u ? a.hits_a : a.hits_s) + a.call_hit[c] * 9u;
    if (!fill) {
        unsigned long long cnt = 0;
        for (int x = 0; x < n; ++x) cnt += pf_sa_span(h[9 * x + 1], h[9 * x + 2]);
        a.call_sa[c] = atomicAdd(a.total, cnt);
        return;
    }
    unsigned long long o = a.call_sa[c];
    for (int x = 0; x < n; ++x) {
        const uint32_t k = h[9 * x + 1], m = pf_sa_span(k, h[9 * x + 2]);
        for (uint32_t j = 0; j < m; ++j) a.idx[o++] = k + j;
    }
}

// hsa_splice_device: the fallback reads of a device batch (the main pass flagged them),
// compacted: their order does not matter, a read's splice path depends on the read
// alone.  A job whose length is outside [3, max_len] (the prefetch's rows and codes are
// sized from max_len) is not taken: its answer is HSA_SP_WIN (not answered), so a caller
// runs the host's path for it.
__global__ void __launch_bounds__(BLOCK) k_sp_prep(const hsa_job_t *jobs, const uint32_t *flags, const int32_t *n_aln,
                                                   uint32_t n, uint32_t max_len, uint32_t *res, uint32_t *lens,
                                                   uint64_t *offs, int32_t *amd, int32_t *idx, unsigned long long *cnt)
{
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n || !(flags[j] & HSA_F_FALLBACK) || n_aln[j] != 0) return;
    const hsa_job_t J = jobs[j];
    if (J.len < 3u || J.len > max_len) {
        res[(size_t)j * HSA_SP_RES_WORDS] = HSA_SP_WIN;
        res[(size_t)j * HSA_SP_RES_WORDS + 1] = 0u;
        return;
    }
    const uint32_t r = (uint32_t)atomicAdd(cnt, 1ull);
    lens[r] = J.len;
    offs[r] = J.off;
    amd[r] = J.max_diff;
    idx[r] = (int32_t)j;
}

__global__ void k_sp_calls(const unsigned long long *cnt, unsigned long long *scnt) { *scnt = 6ull * *cnt; }

// the batch's counters: [0] reads, [5] rank queries of the seed and anchor searches and
// their widths, [6] their hits ([1]-[4] come from the splice kernel)
__global__ void k_sp_stats(const unsigned long long *cnt, const unsigned long long *ctr_s,
                           const unsigned long long *ctr_a, unsigned long long *out)
{
    out[0] = *cnt;
    out[5] = ctr_s[CTR_RANK] + ctr_s[CTR_WIDTH_Q] + ctr_a[CTR_RANK] + ctr_a[CTR_WIDTH_Q];
    out[6] = ctr_s[CTR_HITS] + ctr_a[CTR_HITS];
}

// ---------------------------------------------------------------- host side
// the part of a prefetch's arguments that n reads of up to M bases and the index decide
static PfArgs pf_args(const hsa_index *ix, uint32_t n, uint32_t M, int32_t seed_max_diff)
{
    PfArgs A;
    A.fwd = RankDir{ix->blk[0], ix->isa0};
    A.rev = RankDir{ix->blk[1], ix->risa0};
    A.T = ix->T;
    memcpy(A.C, ix->C, sizeof A.C);
    A.n = n; A.max_len = M; A.sc = (M + 15u) / 16u * 16u + 16u; A.rs = M + 1u; A.cws = M / 3u + 3u > 13u ? M / 3u + 3u : 13u;
    A.seed_max_diff = seed_max_diff;
    A.ktd = trie_levels(ix, false);
    A.ktw = A.ktd ? ix->d_trie_w : nullptr;
    return A;
}

enum PfCtr {                                 // the counter region of d_pf, zeroed by every call: 8-byte slots
    PFC_SEED = 0,                            // the seed passes' counters (CTR_SLOTS of them)
    PFC_ANCHOR = PFC_SEED + CTR_SLOTS,       // the anchor passes'
    PFC_N_ANCHOR = PFC_ANCHOR + CTR_SLOTS,   // anchor calls k_pf_anchors listed
    PFC_SA_TOTAL,                            // SA lookups k_pf_sa counted
    PFC_N_SEED,                              // seed calls: 6 per read
    PFC_N_READS,                             // reads k_sp_prep took (a device batch)
    PFC_SPLICE = 40,                         // the splice kernel's four; the host tables read the slots before them back
    PFC_SLOTS = 128
};

// Where the regions of d_pf start (bytes), and their total.  The optional ones are empty
// unless asked for: codes and res (a device batch has the caller's), idx (a device batch:
// k_sp_prep compacts its reads, so their count is on the device too), call_sa.  call_n ..
// hits_a are one block in this order: the host path copies it to pinned memory in one
// piece and hsa_splice_pf_t points into the copy.
enum : unsigned { PF_CODES = 1, PF_IDX = 2, PF_CALL_SA = 4, PF_RES = 8 };
struct PfLayout {
    unsigned opt;
    uint64_t cap_s, cap_a;                   // hit records of the seed calls, of the anchor calls
    size_t lens, offs, amd, idx, codes, sc, jobs, mg, list, ctr;
    size_t call_n, call_fl, call_hit, call_sa, rows, cw, hits_s, hits_a;
    size_t res, total;
    bool device_batch() const { return opt & PF_IDX; }
};

static PfLayout pf_layout(size_t N, size_t codes_len, const PfArgs &A, unsigned opt)
{
    PfLayout L;
    const size_t calls = 8 * N;
    size_t o = 0;
    const auto region = [&o](size_t bytes) { const size_t at = o; o += al(bytes); return at; };
    L.opt = opt; L.cap_s = 6 * N * 16 + 65536; L.cap_a = 2 * N * 16 + 16384;
    L.lens = region(N * 4); L.offs = region(N * 8); L.amd = region(N * 4);
    L.idx = region(opt & PF_IDX ? N * 4 : 0); L.codes = region(opt & PF_CODES ? codes_len + 64 : 0);
    L.sc = region(2 * N * A.sc + 64);
    L.jobs = region(calls * sizeof(hsa_job_t)); L.mg = region(calls * sizeof(hsa_mg_job_t)); L.list = region(calls * 4);
    L.ctr = region(PFC_SLOTS * sizeof(unsigned long long));
    L.call_n = region(calls * 4); L.call_fl = region(calls * 4); L.call_hit = region(calls * 8);
    L.call_sa = region(opt & PF_CALL_SA ? calls * 8 : 0);
    L.rows = region(N * 6 * A.rs * 8); L.cw = region(calls * A.cws * 8);
    L.hits_s = region(L.cap_s * 36); L.hits_a = region(L.cap_a * 36);           // the block's end
    L.res = region(opt & PF_RES ? N * HSA_SP_RES_WORDS * 4 : 0);
    L.total = o + 256;
    return L;
}

// What the steps of one prefetch share.
struct PfSearch {
    PfArgs A;
    PfLayout L;
    const hsa_regime_t *seed_rg, *anchor_rg;
    hipStream_t st;
    char *d;                                 // d_pf, laid out by L (pf_bind)
    unsigned long long *ctr;                 // its counter region
    int nb;                                  // both regimes' staging (pf_run)
    bool wide;
    template <class T> T *at(size_t region) const { return (T *)(d + region); }
};

// What every entry point asks of its index and regimes; args_ok: its other pointers are set.
static int pf_check(const hsa_index *ix, const hsa_regime_t *seed_rg, const hsa_regime_t *anchor_rg, bool args_ok,
                    const char *entry)
{
    if (int rc = hsa_need32(ix)) return rc;
    if (!seed_rg || !anchor_rg || !args_ok) { hsa_set_error("%s: null argument", entry); return HSA_E_ARG; }
    const hsa_regime_t rg2[2] = {*seed_rg, *anchor_rg};
    if (int rc = check_regimes(rg2, 2)) return rc;
    if (seed_rg->max_gapo != 0) { hsa_set_error("seed searches have no gap opens (bwtgap.c:772)"); return HSA_E_ARG; }
    if (!fast_regimes(rg2, 2)) { hsa_set_error("%s: options outside k_search's layouts", entry); return HSA_E_ARG; }
    return 0;
}

// d_pf grown to F's layout, its counters zeroed, its regions bound into the kernels'
// arguments.  codes: the caller's on the device, or null: the layout's own region.
static int pf_bind(hsa_index *ix, PfSearch &F, const uint8_t *codes, bool prefix)
{
    const PfLayout &L = F.L;
    PfArgs &A = F.A;
    if (int rc = hsa_grow(&ix->d_pf, &ix->d_pf_cap, L.total)) return rc;
    F.d = (char *)ix->d_pf;
    F.ctr = F.at<unsigned long long>(L.ctr);
    HSA_HIP(hipMemsetAsync(F.ctr, 0, PFC_SLOTS * sizeof(unsigned long long), F.st));
    A.lens = F.at<uint32_t>(L.lens); A.offs = F.at<uint64_t>(L.offs); A.amd = F.at<int32_t>(L.amd);
    A.codes = codes ? codes : F.at<uint8_t>(L.codes);
    A.scodes = F.at<uint8_t>(L.sc); A.rows = F.at<int32_t>(L.rows); A.cw = F.at<int32_t>(L.cw);
    A.jobs = F.at<hsa_job_t>(L.jobs); A.mg = F.at<hsa_mg_job_t>(L.mg); A.list = F.at<int32_t>(L.list);
    A.call_n = F.at<int32_t>(L.call_n); A.call_fl = F.at<uint32_t>(L.call_fl);
    A.acount = F.ctr + PFC_N_ANCHOR;
    A.d_n = L.device_batch() ? F.ctr + PFC_N_READS : nullptr;
    A.cwd = (L.cw - L.rows) / 8;
    A.prefix = prefix ? 1u : 0u;
    return 0;
}

// the prefetch's outputs as the splice kernel reads them
static PfDev pf_dev(const PfSearch &F)
{
    const PfArgs &A = F.A;
    PfDev pd;
    pd.n = A.n; pd.max_len = A.max_len; pd.sc = A.sc; pd.rs = A.rs; pd.cws = A.cws;
    pd.lens = A.lens; pd.amd = A.amd; pd.scodes = A.scodes; pd.rows = A.rows; pd.cw = A.cw;
    pd.call_n = A.call_n; pd.call_fl = A.call_fl; pd.call_hit = F.at<uint64_t>(F.L.call_hit);
    pd.hits_s = F.at<uint32_t>(F.L.hits_s); pd.hits_a = F.at<uint32_t>(F.L.hits_a);
    pd.d_n = A.d_n; pd.idx = F.L.device_batch() ? F.at<int32_t>(F.L.idx) : nullptr;
    return pd;
}

// The capacity passes of the seed calls (regime 0), or of the anchor calls (regime 1, 12
// bases): caller-width searches over the calls listed on the device (their count is on
// the device, at most n_upper), hits and counters (zeroed here) in their own regions.
static int pf_passes(hsa_index *ix, const PfSearch &F, bool anchors, int n_upper)
{
    const PfArgs &A = F.A;
    const PfLayout &L = F.L;
    RegimePlan C = regime_plan(anchors ? F.anchor_rg : F.seed_rg, 1);
    C.nb = F.nb; C.wide = F.wide; C.nib_ok = false; C.snib_ok = false;
    // the caller widths are at rows + wb_off (a row's prefix, or cw + call * cws)
    const PassIO io{.jobs = A.jobs, .list = A.list + (anchors ? 6 * (size_t)A.n : 0), .n = n_upper, .codes = A.scodes,
                    .n_aln = A.call_n, .flags = A.call_fl, .hit_off = F.at<uint64_t>(L.call_hit),
                    .hits = F.at<uint32_t>(anchors ? L.hits_a : L.hits_s), .hit_cap = anchors ? L.cap_a : L.cap_s,
                    .ctr = F.ctr + (anchors ? PFC_ANCHOR : PFC_SEED), .max_len = anchors ? 12 : (int)(A.max_len / 3u + 2u),
                    .max_seed = 0, .mg = {A.mg, A.rows}};
    const PassLink link{.n_dev = F.ctr + (anchors ? PFC_N_ANCHOR : PFC_N_SEED), .qctr = CTR_Q_MG};
    return run_capacity_passes(ix, C, io, link, true, nullptr, F.st);
}

// The rows, the seed calls and their passes, the anchor calls and theirs.  Reads from the
// host: the seed calls' count is written here, ev0 opens the timed span, and the anchors'
// pass is planned, after a synchronise, for the anchors there are (a gapped regime's pool
// per lane is large: planning for all 2 n strands would size the scratch for them).  A
// device batch makes no host round trip: its passes take their counts from the device
// (k_sp_calls, k_pf_anchors) and are planned for their upper bounds.
static int pf_run(hsa_index *ix, PfSearch &F)
{
    const size_t N = F.A.n;
    const bool host = !F.L.device_batch();
    hipStream_t st = F.st;
    const unsigned grid6 = (unsigned)((6 * N + BLOCK - 1) / BLOCK), grid2 = (unsigned)((2 * N + BLOCK - 1) / BLOCK);
    HSA_HIP(hipMemsetAsync(F.A.scodes, 4, 2 * N * F.A.sc + 64, st));   // padding reads as N
    hipLaunchKernelGGL(k_pf_rows, dim3(grid6), dim3(BLOCK), 0, st, F.A);
    hipLaunchKernelGGL(k_pf_seeds, dim3(grid6), dim3(BLOCK), 0, st, F.A);
    HSA_HIP(hipGetLastError());
    // both regimes staged once: seeds use regime 0, anchors regime 1
    const hsa_regime_t rg2[2] = {*F.seed_rg, *F.anchor_rg};
    F.nb = 0; F.wide = regime_plan(rg2, 2).wide;
    if (int rc = stage_regimes(ix, rg2, 2, F.nb, st)) return rc;
    const unsigned long long n_seed = 6 * N;
    unsigned long long n_anchor = 2 * N;
    if (host) {
        HSA_HIP(hipMemcpyAsync(F.ctr + PFC_N_SEED, &n_seed, 8, hipMemcpyHostToDevice, st));
        HSA_HIP(hipEventRecord(ix->ev0, st));
    }
    if (int rc = pf_passes(ix, F, false, (int)n_seed)) return rc;
    hipLaunchKernelGGL(k_pf_anchors, dim3(grid2), dim3(BLOCK), 0, st, F.A);
    HSA_HIP(hipGetLastError());
    if (host) {
        HSA_HIP(hipMemcpyAsync(&n_anchor, F.ctr + PFC_N_ANCHOR, 8, hipMemcpyDeviceToHost, st));
        HSA_HIP(hipStreamSynchronize(st));
    }
    return n_anchor ? pf_passes(ix, F, true, (int)n_anchor) : 0;
}

// bwt_splice_match itself (hsa_splice.hip) after a prefetch of reads from the host; no host
// tables: the caller runs a prefetch of its own for the reads the kernel hands back.
static int pf_host_splice(hsa_index *ix, const PfSearch &F, const hsa_regime_t &ext_rg, uint32_t *res,
                          hsa_splice_pf_t *out, hsa_splice_stats_t *sst)
{
    const PfArgs &A = F.A;
    hipStream_t st = F.st;
    uint32_t *d_res = F.at<uint32_t>(F.L.res);
    HSA_HIP(hipEventRecord(ix->ev1, st));
    if (int rc = hsa_splice_device_launch(ix, pf_dev(F), ext_rg, d_res, F.ctr + PFC_SPLICE, st)) return rc;
    HSA_HIP(hipEventRecord(ix->ev_sp, st));
    HSA_HIP(hipMemcpyAsync(res, d_res, (size_t)A.n * HSA_SP_RES_WORDS * 4, hipMemcpyDeviceToHost, st));
    unsigned long long sc4[4];
    HSA_HIP(hipMemcpyAsync(sc4, F.ctr + PFC_SPLICE, sizeof sc4, hipMemcpyDeviceToHost, st));
    HSA_HIP(hipStreamSynchronize(st));
    float ms = 0, sms = 0;
    HSA_HIP(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    HSA_HIP(hipEventElapsedTime(&sms, ix->ev1, ix->ev_sp));
    out->n = (int)A.n; out->max_len = (int)A.max_len; out->row_stride = (int)A.rs; out->cw_stride = (int)A.cws;
    out->kernel_ms = ms;
    if (sst) {
        sst->kernel_ms = sms;
        sst->extensions = sc4[0]; sst->pops = sc4[1]; sst->sa_lookups = sc4[2]; sst->not_answered = sc4[3];
    }
    return 0;
}

// The host tables (hsa_splice_pf_t): the SA -> position lookups of the calls' hits, then
// one copy of the output block (hits up to their counts) into pinned host memory.
// Unfinished calls (hits past the caps, stacks past the HUGE pass) are not answered.
static int pf_host_tables(hsa_index *ix, const PfSearch &F, hsa_splice_pf_t *out, double t0)
{
    const PfArgs &A = F.A;
    const PfLayout &L = F.L;
    hipStream_t st = F.st;
    const size_t calls = 8 * (size_t)A.n;
    const unsigned grid = (unsigned)((calls + BLOCK - 1) / BLOCK);
    const uint32_t *d_hs = F.at<uint32_t>(L.hits_s), *d_ha = F.at<uint32_t>(L.hits_a);
    PfSaArgs S;
    S.n_calls = (uint32_t)calls;
    S.call_n = A.call_n; S.call_hit = F.at<uint64_t>(L.call_hit);
    S.hits_s = d_hs; S.hits_a = d_ha;
    S.call_sa = F.at<unsigned long long>(L.call_sa); S.total = F.ctr + PFC_SA_TOTAL; S.idx = nullptr;
    const bool with_sa = ix->d_sa != nullptr;
    if (with_sa) hipLaunchKernelGGL(k_pf_sa, dim3(grid), dim3(BLOCK), 0, st, S, 0);
    HSA_HIP(hipGetLastError());
    unsigned long long hc[PFC_SPLICE];
    HSA_HIP(hipMemcpyAsync(hc, F.ctr, sizeof hc, hipMemcpyDeviceToHost, st));
    HSA_HIP(hipStreamSynchronize(st));
    const uint64_t n_sa = with_sa ? hc[PFC_SA_TOTAL] : 0;
    if (int rc = n_sa ? hsa_grow(&ix->d_pf2, &ix->d_pf2_cap, al(n_sa * 4) + n_sa * 16 + 256) : 0) return rc;
    uint32_t *d_idx = (uint32_t *)ix->d_pf2, *d_sao = (uint32_t *)((char *)ix->d_pf2 + al(n_sa * 4));
    if (n_sa) {
        S.idx = d_idx;
        hipLaunchKernelGGL(k_pf_sa, dim3(grid), dim3(BLOCK), 0, st, S, 1);
        HSA_HIP(hipGetLastError());
        if (int rc = hsa_sa_position_device(ix, n_sa, d_idx, d_sao, st)) return rc;
    }
    HSA_HIP(hipEventRecord(ix->ev1, st));
    // the output block in pinned host memory, at the offsets it has on the device (q)
    const auto q = [&L](size_t region) { return region - L.call_n; };
    const uint64_t nh_s = hc[PFC_SEED + CTR_HITS] < L.cap_s ? hc[PFC_SEED + CTR_HITS] : L.cap_s;
    const uint64_t nh_a = hc[PFC_ANCHOR + CTR_HITS] < L.cap_a ? hc[PFC_ANCHOR + CTR_HITS] : L.cap_a;
    const size_t h_hits = q(L.hits_s), h_need = h_hits + (nh_s + nh_a) * 36 + al(n_sa * 16) + 256;
    if (h_need > ix->h_pf_cap) {
        if (ix->h_pf) (void)hipHostFree(ix->h_pf);
        ix->h_pf = nullptr; ix->h_pf_cap = 0;
        const size_t want = h_need + h_need / 4 > ((size_t)64 << 20) ? h_need + h_need / 4 : ((size_t)64 << 20);
        HSA_HIP(hipHostMalloc(&ix->h_pf, want, hipHostMallocDefault));
        ix->h_pf_cap = want;
    }
    char *h = (char *)ix->h_pf;
    HSA_HIP(hipMemcpyAsync(h, F.d + L.call_n, h_hits + nh_s * 36, hipMemcpyDeviceToHost, st));
    if (nh_a) HSA_HIP(hipMemcpyAsync(h + h_hits + nh_s * 36, d_ha, nh_a * 36, hipMemcpyDeviceToHost, st));
    const size_t h_sa = al(h_hits + (nh_s + nh_a) * 36);
    if (n_sa) HSA_HIP(hipMemcpyAsync(h + h_sa, d_sao, n_sa * 16, hipMemcpyDeviceToHost, st));
    HSA_HIP(hipStreamSynchronize(st));
    float ms = 0;
    HSA_HIP(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    // anchor calls' hit offsets into the one hits array; unfinished calls -2
    int32_t *cn = (int32_t *)h;
    const uint32_t *cf = (const uint32_t *)(h + q(L.call_fl));
    uint64_t *ch = (uint64_t *)(h + q(L.call_hit));
    for (size_t c = 0; c < calls; ++c) {
        if ((c & 7u) >= 6u && cn[c] >= 0) ch[c] += nh_s;
        if (cn[c] >= 0 && (cf[c] & HSA_F_OVERFLOW)) cn[c] = -2;
    }
    out->n = (int)A.n; out->max_len = (int)A.max_len; out->row_stride = (int)A.rs; out->cw_stride = (int)A.cws;
    out->call_n = cn; out->call_hit = ch;
    out->call_sa = with_sa ? (const uint64_t *)(h + q(L.call_sa)) : nullptr;
    out->rows = (const int32_t *)(h + q(L.rows));
    out->wafter = (const int32_t *)(h + q(L.cw));
    out->hits = (const uint32_t *)(h + h_hits);
    out->sa = n_sa ? (const uint32_t *)(h + h_sa) : nullptr;
    out->n_hits = nh_s + nh_a; out->n_sa = n_sa;
    out->kernel_ms = ms;
    if (getenv("HSA_VERBOSE")) {
        struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t);
        fprintf(stderr, "[hsa] splice prefetch on the device: %u reads, %llu seed + %llu anchor calls, %llu hits, %llu SA "
                        "lookups, %.1f ms (kernels %.1f ms)\n", A.n, 6ull * A.n, hc[PFC_N_ANCHOR],
                (unsigned long long)(nh_s + nh_a), (unsigned long long)n_sa, 1e3 * (t.tv_sec + 1e-9 * t.tv_nsec - t0), ms);
    }
    return 0;
}

// Reads from the host: the prefetch, then its host tables (which want every call's
// width_back after it: no row prefixes for the seeds) or, with ext_rg, the splice kernel.
static int pf_batch(hsa_index_t *ix, const hsa_regime_t *seed_rg, const hsa_regime_t *anchor_rg, int n,
                    const uint32_t *lens, const uint64_t *offs, const uint8_t *codes, size_t codes_len,
                    const int32_t *anchor_max_diff, hsa_splice_pf_t *out, const hsa_regime_t *ext_rg, uint32_t *res,
                    hsa_splice_stats_t *sst)
{
    memset(out, 0, sizeof *out);
    if (sst) memset(sst, 0, sizeof *sst);
    if (n <= 0) return 0;
    int rc = pf_check(ix, seed_rg, anchor_rg, lens && offs && codes && anchor_max_diff,
                      ext_rg ? "hsa_splice_match_batch" : "hsa_splice_prefetch_batch");
    if (rc) return rc;
    uint32_t M = 0;
    for (int r = 0; r < n; ++r) {
        if (lens[r] < 3 || lens[r] > 3 * (FAST_MAX_LEN - 2)) {    // seeds of at most FAST_MAX_LEN bases
            hsa_set_error("splice prefetch: read %d of %u bases", r, lens[r]);
            return HSA_E_ARG;
        }
        if (offs[r] > codes_len || lens[r] > codes_len - offs[r]) { hsa_set_error("read %d past codes_len", r); return HSA_E_ARG; }
        if (anchor_max_diff[r] > anchor_rg->max_diff) { hsa_set_error("read %d: max_diff above the regime's", r); return HSA_E_ARG; }
        M = lens[r] > M ? lens[r] : M;
    }
    HSA_HIP(hipSetDevice(ix->device));
    const double t0 = [] { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }();
    const size_t N = (size_t)n;
    PfSearch F{pf_args(ix, (uint32_t)N, M, seed_rg->max_diff), {}, seed_rg, anchor_rg, ix->stream};
    F.L = pf_layout(N, codes_len, F.A, PF_CODES | PF_CALL_SA | (ext_rg ? PF_RES : 0));
    if ((rc = pf_bind(ix, F, nullptr, ext_rg != nullptr))) return rc;
    HSA_HIP(hipMemcpyAsync(F.d + F.L.lens, lens, N * 4, hipMemcpyHostToDevice, F.st));
    HSA_HIP(hipMemcpyAsync(F.d + F.L.offs, offs, N * 8, hipMemcpyHostToDevice, F.st));
    HSA_HIP(hipMemcpyAsync(F.d + F.L.amd, anchor_max_diff, N * 4, hipMemcpyHostToDevice, F.st));
    HSA_HIP(hipMemcpyAsync(F.d + F.L.codes, codes, codes_len, hipMemcpyHostToDevice, F.st));
    if ((rc = pf_run(ix, F))) return rc;
    return ext_rg ? pf_host_splice(ix, F, *ext_rg, res, out, sst) : pf_host_tables(ix, F, out, t0);
}

extern "C" int hsa_splice_prefetch_batch(hsa_index_t *ix, const hsa_regime_t *seed_rg, const hsa_regime_t *anchor_rg,
                                         int n, const uint32_t *lens, const uint64_t *offs, const uint8_t *codes,
                                         size_t codes_len, const int32_t *anchor_max_diff, hsa_splice_pf_t *out)
{
    return pf_batch(ix, seed_rg, anchor_rg, n, lens, offs, codes, codes_len, anchor_max_diff, out, nullptr, nullptr,
                    nullptr);
}

extern "C" int hsa_splice_match_batch(hsa_index_t *ix, const hsa_regime_t *seed_rg, const hsa_regime_t *anchor_rg,
                                      const hsa_regime_t *ext_rg, int n, const uint32_t *lens, const uint64_t *offs,
                                      const uint8_t *codes, size_t codes_len, const int32_t *anchor_max_diff,
                                      hsa_splice_pf_t *pf, uint32_t *res, hsa_splice_stats_t *stats)
{
    if (!ext_rg || (n > 0 && !res) || !pf) {
        hsa_set_error("hsa_splice_match_batch: null argument");
        return HSA_E_ARG;
    }
    return pf_batch(ix, seed_rg, anchor_rg, n, lens, offs, codes, codes_len, anchor_max_diff, pf, ext_rg, res, stats);
}

// A device batch: k_sp_prep compacts its fallback reads for the prefetch, the splice
// kernel answers them at d_res, the caller's 8 counters are zeroed and filled on the device.
extern "C" int hsa_splice_device(hsa_index_t *ix, const hsa_regime_t *seed_rg, const hsa_regime_t *anchor_rg,
                                 const hsa_regime_t *ext_rg, const hsa_splice_batch_t *b, void *stream)
{
    int rc = pf_check(ix, seed_rg, anchor_rg, ext_rg && b, "hsa_splice_device");
    if (rc) return rc;
    if (b->max_len < 3 || b->max_len > 3 * (FAST_MAX_LEN - 2) || b->n_jobs < 0) {
        hsa_set_error("hsa_splice_device: max_len %d / n_jobs %d out of range", b->max_len, b->n_jobs);
        return HSA_E_ARG;
    }
    if (b->n_jobs == 0) return 0;
    HSA_HIP(hipSetDevice(ix->device));
    hipStream_t st = stream ? (hipStream_t)stream : ix->stream;
    const size_t N = (size_t)b->n_jobs;
    const uint32_t M = (uint32_t)b->max_len;
    PfSearch F{pf_args(ix, (uint32_t)N, M, seed_rg->max_diff), {}, seed_rg, anchor_rg, st};
    F.L = pf_layout(N, 0, F.A, PF_IDX);
    if ((rc = pf_bind(ix, F, b->d_codes, true))) return rc;
    const unsigned long long *rcnt = F.ctr + PFC_N_READS;
    unsigned long long *out_ctr = (unsigned long long *)b->d_counters;
    HSA_HIP(hipMemsetAsync(out_ctr, 0, 8 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_sp_prep, dim3((unsigned)((N + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, b->d_jobs, b->d_flags,
                       b->d_n_aln, (uint32_t)N, M, b->d_res, F.at<uint32_t>(F.L.lens), F.at<uint64_t>(F.L.offs),
                       F.at<int32_t>(F.L.amd), F.at<int32_t>(F.L.idx), F.ctr + PFC_N_READS);
    hipLaunchKernelGGL(k_sp_calls, dim3(1), dim3(1), 0, st, rcnt, F.ctr + PFC_N_SEED);
    if ((rc = pf_run(ix, F))) return rc;
    if ((rc = hsa_splice_device_launch(ix, pf_dev(F), *ext_rg, b->d_res, out_ctr + 1, st))) return rc;
    hipLaunchKernelGGL(k_sp_stats, dim3(1), dim3(1), 0, st, rcnt, (const unsigned long long *)(F.ctr + PFC_SEED),
                       (const unsigned long long *)(F.ctr + PFC_ANCHOR), out_ctr);
    HSA_HIP(hipGetLastError());
    return 0;
}
