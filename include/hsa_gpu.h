/*
 * hsa_gpu.h -- C ABI of the MI355X search core (libhsa_gpu.so).
 *
 * Plain pointers and sizes only.  This is the layer the reference-compatible
 * entry points (include/hsa_bwtaln.h) are built on, and the layer the Python
 * tests/bench bind with ctypes.
 *
 * What each group replaces in the reference:
 *   hsa_index_*        -- BWTLoad2BWT's in-memory BWT + Occ tables (2BWT-Interface.c:13,
 *                         BWT.c:107): uploaded once to HBM and re-laid out into 16-byte
 *                         rank blocks (3 x u32 counts + 16 two-bit codes).
 *   hsa_occ4_batch     -- BWTAllOccValue (BWT.c:793) for a batch of positions.
 *   hsa_step_batch     -- BWTAllSARangesBackward_Bidirection (2BWT-Interface.c:235).
 *   hsa_width_batch    -- bwt_cal_width type 1 (bwtaln.c:73-98); hsa_width0_batch: type 0.
 *   hsa_search_batch   -- the per-read loop of bwa_cal_sa_reg_gap (bwtaln.c:303-373):
 *                         rc strand then forward strand, bwt_cal_width x2 and
 *                         bwt_match_gap (bwtgap.c:118-331) per strand (two kernels:
 *                         the widths of every read and strand, then the searches).
 *   hsa_match_gap_batch -- bwt_match_gap (bwtgap.c:118-331) called directly with the
 *                         caller's widths, as the splice path calls it (bwtgap.c:812,
 *                         :919, :1192).
 *   hsa_splice_seeds_device -- the six seed searches of bwt_splice_match
 *                         (bwtgap.c:797-812) for every fallback read of a device batch.
 *   hsa_sa_position_*  -- BWTSaValue (BWT.c:1195) + BWTRetrievePositionFromSAIndex
 *                         (2BWT-Interface.c:329).
 *   hsa_sa_position_*64, hsa_hit_positions_device64 -- the same on a 64-bit index (texts
 *                         of 2^32 characters or more), which the reference cannot hold.
 *   hsa_refine_rows_device64 -- refine_gapped_core and bwa_cal_md1 (bwtse.c:380-494) with
 *                         aln_global_core (stdaln.c:345-525) for the position rows of a 64-bit
 *                         index: CIGAR, NM and MD.
 *   hsa_reads_device   -- bwa_read_seq over kseq_read (bwaseqio.c:161-231, kseq.h:155-193) and the
 *                         read filter of bwa_cal_sa_reg_gap (bwtaln.c:313-332) for FASTQ bytes in
 *                         device memory.
 *   hsa_inflate_bgzf_device -- gzread (zlib's inflate with the gzip trailer's CRC32 check) for
 *                         the members of a BGZF file whose bytes sit in device memory: the
 *                         step in front of hsa_reads_device and hsa_fasta_device.
 *   hsa_bam_reads_device -- bwa_read_bam (bwaseqio.c:105-157, without its line 142) for the
 *                         inflated bytes of a BAM file in device memory: hsa_reads_device's
 *                         outputs.
 *   hsa_extend_batch   -- bwt_extend_backward / bwt_extend_foreward (bwtgap.c:640-663,
 *                         bwt_backtracing_search :346-511): the splice path's seed
 *                         extensions.
 *
 * Errors: every call returns 0 on success or a negative HSA_E* code and leaves a
 * message readable with hsa_last_error().  The library never falls back to a CPU
 * path: without a usable gfx950 device the calls fail.
 */
#ifndef HSA_GPU_H
#define HSA_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSA_E_HIP     (-1)   /* a HIP runtime call failed */
#define HSA_E_ARG     (-2)   /* invalid argument / unsupported option range */
#define HSA_E_NODEV   (-3)   /* no GPU visible */
#define HSA_E_MEM     (-4)   /* device allocation failed */

/* Search options of one regime (the fields of gap_opt_t the search reads,
 * bwtaln.h:133-143).  max_diff and seed_len are per read (hsa_job_t). */
typedef struct {
    int32_t s_mm, s_gapo, s_gape;
    int32_t mode;                 /* BWA_MODE_* bits: GAPE 0x1, LOGGAP 0x4, NONSTOP 0x10 */
    int32_t indel_end_skip, max_del_occ, max_entries;
    int32_t max_gapo, max_gape;
    int32_t max_seed_diff, max_top2;
    int32_t n_stacks;             /* aln_score(max_diff+1, max_gapo+1, max_gape+1) of the batch's local_opt */
    int32_t max_diff;             /* upper bound of the per-read max_diff of this regime's reads */
} hsa_regime_t;

/* One read to search.  `off` indexes the codes buffer given to hsa_search_batch. */
typedef struct {
    uint64_t off;
    uint32_t len;
    int32_t max_diff;             /* value of aux->opt->max_diff for this read */
    int32_t seed_len;             /* aux->opt->seed_len after bwtaln.c:332 (0x7fffffff = none) */
    int32_t regime;               /* index into the regime array (0 or 1) */
} hsa_job_t;

/* Per-read result flags. */
#define HSA_F_FALLBACK  1u        /* no hit on either strand: caller runs bwt_splice_match */
#define HSA_F_OVERFLOW  2u        /* internal: per-lane stack/hit capacity exceeded (re-run) */

typedef struct hsa_index hsa_index_t;

int         hsa_device_count(void);
const char *hsa_last_error(void);

/* Upload a bidirectional index.  code/rcode are the .bwt payload words (2-bit,
 * MSB-first, ceil(T/16) words; BWT.c:156-181).  C/rC are cumulativeFreq[0..4]. */
int  hsa_index_create(int device, uint32_t T, uint32_t isa0, const uint32_t C[5], const uint32_t *code,
                      uint32_t rT, uint32_t risa0, const uint32_t rC[5], const uint32_t *rcode,
                      hsa_index_t **out);
/* Same, from codes already resident on the device (LSB-first 2-bit, 16 per u32). */
int  hsa_index_create_device(int device, uint32_t T, uint32_t isa0, const uint32_t C[5], const uint32_t *d_code_lsb,
                             uint32_t rT, uint32_t risa0, const uint32_t rC[5], const uint32_t *d_rcode_lsb,
                             hsa_index_t **out);
void hsa_index_free(hsa_index_t *ix);
/* Give back the handle's grown working buffers (search scratch of every capacity pass,
 * the splice prefetch's and splice kernel's buffers) after its stream's work is done;
 * the next call allocates them again.  For a process that hands the GPU's memory to
 * another one between batches (no reference counterpart: the reference has no device).
 * No other call may be in flight on this handle (or use its buffers from another host
 * thread) while it runs: it waits for the stream's queued work only, not for host threads
 * that are about to queue more.  The drop-in entry points never call it. */
int hsa_index_release_scratch(hsa_index_t *ix);
/* The HIP stream (hipStream_t) the library launches on for this index. */
void *hsa_index_stream(const hsa_index_t *ix);
size_t hsa_index_bytes(const hsa_index_t *ix);
int  hsa_index_device(const hsa_index_t *ix);
/* The index's root width trie (hsa_amd/csrc/hsa_trie.h): every string of up to *depth
 * characters with the interval k_widths' forward extension computes for it (0: none;
 * HSA_TRIE_DEPTH at creation, default 12); *bytes of device memory it takes.  Its loads
 * are counted in d_counters[10].  *sdepth: the implicit root levels of the ungapped
 * k_search -- the deepest level of which every string occurs in the text, at most
 * HSA_SDEPTH at creation (default and most 13; 0: none, as for a 64-bit index); its
 * table (hsa_index_levels) is not part of *bytes. */
int  hsa_index_trie(const hsa_index_t *ix, uint32_t *depth, uint32_t *sdepth, size_t *bytes);
/* The level the implicit root levels' table holds, 16 B x 4^*table_level of device memory
 * (0: none): sdepth + 1, the first level that need not be complete (at most 14; *absent of
 * its strings do not occur in the text and are stored with their empty intervals), or
 * sdepth when that level is unusable, does not fit, or HSA_SPARTIAL=0 was set at creation
 * (*absent 0).  A clone reports its parent's values. */
int  hsa_index_levels(const hsa_index_t *ix, uint32_t *table_level, uint32_t *absent);
/* A second handle on the same resident index, for passes that run concurrently: the
 * clone shares src's read-only device arrays (rank blocks, wrap tables, trie, SA) and
 * has its own stream, events and search scratch, so hsa_search_device on
 * the two handles may overlap (the next batch's k_widths fills the last waves of this
 * one's k_search).  hsa_index_free(src) while clones are live defers the free of the
 * shared arrays to the last clone's hsa_index_free (src must not be used after it);
 * hsa_index_set_sa refuses a clone and an index with live clones.  No reference
 * counterpart: the reference searches one batch at a time (bwtaln.c:477, :506). */
int  hsa_index_clone(hsa_index_t *src, hsa_index_t **out);

/* Rank/step/width primitives over host arrays (tests and tools). */
int hsa_occ4_batch(hsa_index_t *ix, int dir, size_t n, const uint32_t *pos, uint32_t *occ4_out);
int hsa_step_batch(hsa_index_t *ix, size_t n, const uint32_t *klrr, uint32_t *out16);
int hsa_width_batch(hsa_index_t *ix, size_t n, const uint64_t *offs, const uint32_t *lens,
                    const uint8_t *codes, size_t codes_len, uint32_t *width_out /* 2*(len+1) words per read, packed */);
/* bwt_cal_width type 0 (bwtaln.c:98-115, backward on the forward BWT): entries 1..len
 * as the reference writes them; entry 0, which the reference never writes, is 0. */
int hsa_width0_batch(hsa_index_t *ix, size_t n, const uint64_t *offs, const uint32_t *lens,
                     const uint8_t *codes, size_t codes_len, uint32_t *width_out);

/* One seed extension of the splice path: bwt_extend_backward (dir 1) or
 * bwt_extend_foreward (dir 0), bwtgap.c:640-663 -> bwt_backtracing_search (:346-511).
 * The call extends hit `aln` (bwt_aln1_t words, bwtaln.h:41-50) over `len` read
 * positions toward max_pos (*_left / *_right).  It reads the strand sequence and the
 * direction's width bids (width_back backward, width_fore forward) only inside the
 * read-position window [lo, lo + n) -- backward [min(start - len, max_pos),
 * max(start, max_pos + 1)], forward [min(end, max_pos - 1), max(end + len, max_pos)]
 * (an empty window for a negative len without NONSTOP, whose seed entry stops the
 * search at its first pop) -- given at codes[off .. off + n) and bids[off .. off + n).
 * The regime holds aux->opt's fields with max_diff exact, and n_stacks =
 * aux->stack->n_stacks. */
typedef struct {
    int32_t dir;
    int32_t len;
    int32_t max_pos;
    int32_t regime;
    int32_t lo, n;
    uint64_t off;
    uint32_t aln[9];
    uint32_t pad;
} hsa_ext_job_t;

/* n extensions in one batch (one lane per call; stacks in HBM, grown in capacity
 * passes up to the reference's max_entries bound).  Outputs per call: ret (1, 2 or -1
 * as the reference), max_pos after, and the 9 words of the hit after.  A call whose
 * search the reference leaves undefined (a score past the stack's buckets, a rank
 * position past the text, a read position outside its window) fails the batch with
 * HSA_E_ARG. */
int hsa_extend_batch(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const hsa_ext_job_t *jobs, int n,
                     const uint8_t *codes, const int32_t *bids, size_t win_len, int32_t *ret, int32_t *max_pos,
                     uint32_t *aln_out);

/* The same calls in slices: call j works in persistent slot slots[j] (0 <= slot <
 * n_slots; the slots' stacks and states stay on the device between calls with the same
 * n_slots), resumes its saved state when resume[j], and runs at most `budget` pops.
 * ret[j]: 1, 2, -1 (finished: max_pos / aln_out valid), HSA_EXT_CONT (not finished:
 * submit it again with resume set), HSA_EXT_E_CAP (needs more stack than a slot holds:
 * run it through hsa_extend_batch), or another negative code (undefined in the
 * reference).  The job's aln is always the call's original hit.  Every regime's
 * n_stacks must be <= HSA_EXT_SLICE_STACKS (a slot's bucket heads); a caller with a
 * larger regime runs those calls through hsa_extend_batch. */
#define HSA_EXT_CONT  (-999)
#define HSA_EXT_E_CAP (-1001)
#define HSA_EXT_SLICE_STACKS 256
int hsa_extend_sliced(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const hsa_ext_job_t *jobs,
                      const int32_t *slots, const uint8_t *resume, int n, const uint8_t *codes, const int32_t *bids,
                      size_t win_len, int n_slots, uint32_t budget, int32_t *ret, int32_t *max_pos, uint32_t *aln_out);

/* Search statistics (summed over the call). */
typedef struct {
    uint64_t rank_queries;        /* Occ evaluations the reference would issue (2 per step) */
    uint64_t blocks_loaded;       /* 64-byte rank blocks actually fetched */
    uint64_t pops;                /* gap_pop calls */
    uint64_t overflow_reruns;     /* reads re-run with large per-read capacity */
    double   kernel_ms;           /* device time of the search kernels (HIP events) */
    double   main_kernel_ms;      /* device time of the main (first) search launch */
    uint64_t main_launches;
} hsa_stats_t;

/* Search `n_jobs` reads.  Host pointers; `codes` holds the 0..255 read codes.
 * Outputs: n_aln[j], flags[j], hit_off[j] (offset in hits, in records) and the
 * packed hits, 9 u32 per record in bwt_aln1_t layout (bwtaln.h:41-50), written to
 * *hits (malloc'd by the library; free with hsa_free).  Returns total hits >= 0. */
long hsa_search_batch(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes,
                      const hsa_job_t *jobs, int n_jobs, const uint8_t *codes, size_t codes_len,
                      int32_t *n_aln, uint32_t *flags, uint64_t *hit_off, uint32_t **hits,
                      hsa_stats_t *stats);

/* Device-resident variant for throughput runs: jobs/codes already on the device,
 * outputs stay on the device (d_hits capacity in records).  Launches on `stream`
 * (a hipStream_t; NULL = the library's stream) and does not synchronise: the
 * caller reads d_counters after the stream completes.
 *
 * d_counters: >= 16 u64 of device scratch, zeroed by the call; the library writes
 *   [1]  hit records allocated (may exceed hit_cap: see [11])
 *   [2]  rank queries the reference algorithm issues for these reads: 2 per
 *        bidirectional step, 2 per width step of every strand it searches
 *        (bwtaln.c:343-359); a read re-run for capacity counts its work twice
 *   [3]  64-byte rank sectors fetched    [4] gap_pop calls
 *   [10] steps answered by a root-trie load instead of rank queries (hsa_index_trie)
 *   [7]  the width queries among [2]
 *   [8]  reads that overflowed their lane's capacity in the main pass (8 192 pool
 *        slots, 32 768 with gap opens), re-run on the device in the BIG pass (65 535
 *        slots, 16 384 hits per read)   [9] the big pass's queue head
 *   [12] reads that overflowed the big pass too, re-run in the HUGE pass: popped
 *        slots reused, so any stack up to max_entries + 16 live entries fits (the
 *        reference's own bound, bwtgap.c:150-151; capped at 4 Mi), 262 144 hits
 *        [15] the huge pass's queue head
 *   [11] reads left UNFINISHED: still over capacity in the huge pass, or their hits
 *        did not fit in d_hits; such a read keeps HSA_F_OVERFLOW, n_aln 0, no hits.
 *        Non-zero means: search those reads again with a larger hit_cap.
 *   [13] width queries of every forward-strand row (computed speculatively)
 *   [14] the part of [13] the reference issues (forward strands searched)
 * Reads past k_search's layouts (longer than 1 023 bases: split off on the device) and
 * regimes past them (n_stacks > 512, > 128 reachable scores, max_gapo > 14, max_diff >
 * 125: every read) run k_search_any (hsa_search_any.h) after k_search, into the same
 * outputs and counters; its large-capacity re-runs count a read's work once.  max_len
 * may be up to 65 535 (gap_entry_t.info's 16-bit position, bwtgap.c:157).
 * d_codes: the read codes; the kernels read whole aligned 16-byte words, so the
 *   buffer must stay readable 16 bytes past the last read's end. */
typedef struct {
    const hsa_job_t *d_jobs; int n_jobs;
    const uint8_t *d_codes;
    int32_t *d_n_aln; uint32_t *d_flags; uint64_t *d_hit_off;
    uint32_t *d_hits; uint64_t hit_cap;
    uint64_t *d_counters;         /* >= 16 u64, see above */
    int32_t max_len, max_seed;    /* longest read, longest seed among the jobs */
} hsa_device_batch_t;
int hsa_search_device(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes,
                      const hsa_device_batch_t *b, void *stream);
/* Device time of the two kernels of the last pass on this index (k_widths, then
 * k_search with its overflow re-run); waits for that pass to finish. */
int hsa_last_pass_ms(hsa_index_t *ix, float *widths_ms, float *search_ms);
/* The same for each of the last n (<= 1024) hsa_search_device passes, oldest first:
 * HIP events recorded on the launch stream around each kernel of every pass. */
int hsa_pass_times(hsa_index_t *ix, int n, float *widths_ms, float *search_ms);
/* Kernel geometry/capacity knobs: 0 leaves a knob unchanged; pool_entries < 0 restores
 * its default (8192 entries per lane, 32768 when gap opens are allowed). */
int hsa_configure(int waves_per_cu, int pool_entries, int hit_cap);

void hsa_free(void *p);

/* Synthetic workload helpers (bench data generation on the device). */
int hsa_synth_genome_device(int device, uint64_t T, uint64_t seed, uint32_t *d_code_lsb);

/* ---- bwt_match_gap with caller-supplied widths (bwtgap.c:118-331) ----
 * The splice path calls bwt_match_gap directly (bwtgap.c:812, :919, :1192) with widths
 * it computed itself -- of the read prefix, not of the searched sequence
 * (bwtgap.c:807) -- with width_seed NULL or aliased to width_back (bwtgap.c:809), and
 * the search mutates width_back through gap_shadow (bwtgap.c:217).  One
 * hsa_mg_job_t per call, next to its hsa_job_t: jobs[j].off/len address the searched
 * sequence itself (aux->seq or aux->rc_seq as aux->strand selects), jobs[j].max_diff
 * and seed_len are the call's opt->max_diff and opt->seed_len. */
#define HSA_SEED_NONE  0          /* width_seed == NULL */
#define HSA_SEED_OWN   1          /* width_seed: its own array, seed_len + 1 entries */
#define HSA_SEED_ALIAS 2          /* width_seed == width_back */
typedef struct {
    uint64_t wb_off;              /* width_back[0..len]: pairs (w, bid) at widths + 2 * wb_off */
    uint64_t ws_off;              /* width_seed[0..seed_len] (HSA_SEED_OWN only) */
    int32_t strand;               /* aux->strand (0 or 1), stamped into the hits (bwtgap.c:235) */
    int32_t seed;                 /* HSA_SEED_* */
} hsa_mg_job_t;

/* One search per job with the caller's widths (bwt_cal_width's bwt_width_t pairs, int32
 * w then bid; bids must be >= 0 as bwt_cal_width produces them).  The jobs' width
 * ranges must not overlap.  widths_out (width_pairs pairs, may equal widths) receives
 * each job's width_back after the search; other entries are left as they are.  Hits
 * as hsa_search_batch, with start = end = 0 (bwt_match_gap leaves them to its caller).
 * Returns the total hit count >= 0. */
long hsa_match_gap_batch(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes, const hsa_job_t *jobs,
                         const hsa_mg_job_t *mg, int n_jobs, const uint8_t *codes, size_t codes_len,
                         const int32_t *widths, size_t width_pairs, int32_t *widths_out,
                         int32_t *n_aln, uint64_t *hit_off, uint32_t **hits, hsa_stats_t *stats);

/* ---- the splice path's seed searches on the device ----
 * For every read of a device batch that the main pass flagged HSA_F_FALLBACK, the six
 * seed searches bwt_splice_match can make (bwtgap.c:797-812, restated in
 * hsa_amd/splice.py): seed t of strand s (t = 0, 1, 2; sl = len / 3) searches the
 * strand sequence [t sl, t sl + la) with la = sl (+ len % 3 for t = 2), width_back =
 * width_seed = the widths of the strand's PREFIX of length la, and the seed options
 * (GAPE cleared, no gaps, max_diff = max_seed_diff, seed_len = la) given as one regime.
 * Prefix widths, the calls and their searches all run on the device.  Call 3 s + t of
 * read r is output record 6 r + 3 s + t; records of other reads are left untouched. */
typedef struct {
    const hsa_job_t *d_jobs; int n_jobs;  /* the main pass's reads (off, len) */
    const uint8_t *d_codes;
    const uint32_t *d_flags;              /* the main pass's per-read flags */
    int32_t *d_n_aln; uint64_t *d_hit_off; /* 6 * n_jobs records each */
    uint32_t *d_hits; uint64_t hit_cap;   /* hit records (9 u32) */
    uint64_t *d_counters;                 /* >= 16 u64 of device scratch: [1] hits, [2] rank queries, [4] pops */
    int32_t max_len;                      /* longest read */
} hsa_seed_batch_t;
int hsa_splice_seeds_device(hsa_index_t *ix, const hsa_regime_t *seed_regime, const hsa_seed_batch_t *b, void *stream);

/* ---- the splice path's prefetch of one read batch ----
 * bwt_splice_match (bwtgap.c:748-1332) runs on the host for every read the main search
 * leaves without a hit; before its first seed extension, the searches it can make are
 * determined by the read alone.  This call runs all of them for n such reads in one
 * device pass (replacing, for the host's splice tables, one GPU call per bwt_match_gap /
 * bwt_cal_width / BWTRetrievePositionFromSAIndex the reference makes there):
 *   per read r (codes as bwa_seq_t.seq: 0-3, 4 = N; 3 <= lens[r] <= 3 063) and strand s
 *   (0: the read, 1: its reverse complement, bwtaln.c:326-333),
 *   rows (bwt_width_t pairs, int32 w then bid; row_stride pairs apart, row j of read r
 *     at rows + 2 * (6 r + j) * row_stride):
 *     j = s      bwt_cal_width type 1 of the whole strand (L + 1 pairs, bwtaln.c:84-97);
 *                the width of the strand's prefix of length la is its first la entries
 *                and {0, bid of entry la - 1, + 1};
 *     j = 2 + s  type 1 of the strand's last 12 bases (13 pairs; L >= 12 only);
 *     j = 4 + s  type 0 of the whole strand (L + 1 pairs, entry 0 = 0; bwtaln.c:98-115);
 *   calls (8 per read, call 8 r + c):
 *     c = 3 s + t, t = 0..2: seed t of strand s (bwtgap.c:797-812): the strand's bases
 *       [t sl, t sl + la) (sl = L / 3, la = sl + (t == 2 ? L % 3 : 0)), width_back =
 *       width_seed = the strand prefix's widths of length la, regime seed_rg, max_diff
 *       seed_rg->max_diff, seed_len la;
 *     c = 6 + s: the strand's 12-mer anchor when its seeds' hit pattern is 3 (seeds 0 and
 *       1 hit: its last 12 bases with row 2 + s, bwtgap.c:911-919) or 6 (seeds 1 and 2:
 *       its first 12 with the first 13 entries of row s, :1187-1192), width_seed NULL,
 *       regime anchor_rg, max_diff anchor_max_diff[r];
 *     call_n: hits (bwt_aln1_t records at hits + 9 * call_hit, start = end = 0 as
 *       bwt_match_gap returns them), -1 not searched, -2 not finished (hits past the
 *       buffer, or a stack past the reference's bound): the caller searches it itself;
 *     wafter: the call's width_back after the search (gap_shadow, bwtgap.c:217),
 *       cw_stride pairs per call;
 *   SA (with hsa_index_set_sa): BWTRetrievePositionFromSAIndex of k .. min(l, k + 49) of
 *     every hit of every call, in order (bwt_aln_corelate_check, bwtgap.c:698, :711):
 *     4 u32 each as hsa_sa_position_batch, the call's first at sa + 4 * call_sa.
 * The arrays point into pinned host memory the index owns until its next call. */
typedef struct {
    int n, max_len, row_stride, cw_stride;
    const int32_t *rows;
    const int32_t *call_n;
    const uint64_t *call_hit;
    const uint32_t *hits;
    const int32_t *wafter;
    const uint64_t *call_sa;      /* NULL without an SA */
    const uint32_t *sa;
    uint64_t n_hits, n_sa;
    double kernel_ms;
} hsa_splice_pf_t;
int hsa_splice_prefetch_batch(hsa_index_t *ix, const hsa_regime_t *seed_rg, const hsa_regime_t *anchor_rg, int n,
                              const uint32_t *lens, const uint64_t *offs, const uint8_t *codes, size_t codes_len,
                              const int32_t *anchor_max_diff, hsa_splice_pf_t *out);

/* ---- the splice path itself on the device ----
 * bwt_splice_match (bwtgap.c:748-1332) for the same n reads: the prefetch pass above,
 * then one persistent kernel that runs each read's seed correlation
 * (bwt_aln_corelate_check, :669), motif scan of the reference (splice_site_search_from_pos,
 * :523), seed extensions (bwt_extend_backward / _foreward, :640-663) and intron-end
 * checks (check_site_by_intron_end, :602) on the device (hsa_amd/csrc/hsa_splice.hip).
 * ext_rg is the extensions' regime: the read's local_opt with max_gape 3 (aux_ext,
 * :776-782; its GAPE bit is the local_opt's, the kernel clears and sets it where the
 * reference does); max_diff per read is anchor_max_diff[r]; n_stacks <=
 * HSA_SP_MAX_STACKS.  Needs hsa_index_set_sa and hsa_index_set_text.
 * res: HSA_SP_RES_WORDS u32 per read: status, n_aln (0, 1 or 2), then res_aln[0] and
 * res_aln[1] (9 words each, bwt_aln1_t) as bwt_splice_match returns them.  status 0: the
 * answer; HSA_SP_* > 0: not answered (the reference's code leaves that read undefined
 * here, or it outgrew the kernel's per-lane stack of HSA_SPLICE_CAP entries, or a
 * prefetched search of it did not finish) -- run the host's bwt_splice_match for it
 * (with hsa_splice_prefetch_batch of those reads for its tables).  `pf` receives the
 * pass's shape and kernel_ms only (no tables). */
#define HSA_SP_RES_WORDS 20
#define HSA_SP_MAX_STACKS 128
#define HSA_SP_OK     0
#define HSA_SP_CALL   1   /* a seed or anchor search of the read did not finish */
#define HSA_SP_CAP    2   /* an extension outgrew the per-lane stack */
#define HSA_SP_SCORE  3   /* an extension entry's score past the stack's buckets */
#define HSA_SP_RANK   4   /* a rank position past the text */
#define HSA_SP_WIN    5   /* a read or width position outside the read */
#define HSA_SP_SA     6   /* an SA position in no chromosome block (stale seq id in the reference) */
#define HSA_SP_TEXT   7   /* a text position past the packed reference */
#define HSA_SP_LOOP   8   /* a loop bound the reference does not keep (u32 wrap, buffer) */
int hsa_index_set_text(hsa_index_t *ix, const uint32_t *packed, uint64_t n_words, uint32_t dna_len);
typedef struct {
    double kernel_ms;             /* the splice kernel's device time */
    uint64_t extensions, pops, sa_lookups, not_answered;
} hsa_splice_stats_t;
/* The same for a device batch: the reads the main pass (hsa_search_device) left with
 * HSA_F_FALLBACK and no hit go through the prefetch pass and the splice kernel, all on
 * the device and without a host round trip.  d_res: HSA_SP_RES_WORDS u32 per job of the
 * batch, written for those reads only; d_counters (>= 8 u64): [0] reads sent to the
 * splice path, [1] extensions, [2] extension pops, [3] SA lookups, [4] reads not answered,
 * [5] rank queries of the seed and anchor searches with their widths, [6] their hits.
 * Each read's max_diff is its job's; max_len the longest read (3 * 1021 at most): a
 * fallback job shorter than 3 or longer than max_len is not taken and gets HSA_SP_WIN. */
typedef struct {
    const hsa_job_t *d_jobs; int n_jobs;
    const uint8_t *d_codes;
    const uint32_t *d_flags;              /* the main pass's per-read flags */
    const int32_t *d_n_aln;               /* the main pass's per-read hit counts */
    uint32_t *d_res;
    uint64_t *d_counters;
    int32_t max_len;
} hsa_splice_batch_t;
int hsa_splice_device(hsa_index_t *ix, const hsa_regime_t *seed_rg, const hsa_regime_t *anchor_rg,
                      const hsa_regime_t *ext_rg, const hsa_splice_batch_t *b, void *stream);
int hsa_splice_match_batch(hsa_index_t *ix, const hsa_regime_t *seed_rg, const hsa_regime_t *anchor_rg,
                           const hsa_regime_t *ext_rg, int n, const uint32_t *lens, const uint64_t *offs,
                           const uint8_t *codes, size_t codes_len, const int32_t *anchor_max_diff, hsa_splice_pf_t *pf,
                           uint32_t *res, hsa_splice_stats_t *stats);

/* SA index -> text position (BWTSaValue BWT.c:1195 + BWTRetrievePositionFromSAIndex
 * 2BWT-Interface.c:329), batched.  hsa_index_set_sa uploads the sampled suffix array
 * as BWTLoad holds it (values[0] = -1, (T+s)/s values, interval s) and the chromosome
 * block table (n_blocks rows of u32 chrID, blockStart, blockEnd, ori; ChrBlock
 * HSP.h:41-46).  Output: 4 u32 per index -- SA value, chrID, 1-based position in the
 * chromosome, position in the packed text; chrID and position are 0xFFFFFFFF when no
 * block holds it. */
int hsa_index_set_sa(hsa_index_t *ix, const uint32_t *sa_values, uint64_t n_values, uint32_t interval,
                     const uint32_t *blocks, int n_blocks);
int hsa_sa_position_batch(hsa_index_t *ix, size_t n, const uint32_t *sa_index, uint32_t *out4);
int hsa_sa_position_device(hsa_index_t *ix, size_t n, const uint32_t *d_sa_index, uint32_t *d_out4, void *stream);

/* Roofline probe: measured rate of uniformly random 64-byte-sector gathers over a
 * table of `table_bytes` (the access pattern of rank queries), in GB/s of sectors
 * touched (sectors/s x 64 B), all CUs at 16 waves each.  per_sector = 1: one 16-byte
 * load per sector (what a rank query issues); 2: four adjacent lanes load the four
 * 16-byte quarters of one sector (16 sectors per wave instruction); 4: each lane
 * loads its whole sector in four loads.  The denominator the search kernel's
 * achieved bandwidth is compared with next to the 8 TB/s spec peak (SURVEY.md §8d;
 * DESIGN.md "The random-access ceiling"). */
int hsa_probe_gather(int device, uint64_t table_bytes, int per_sector, double *gbps);

/* ---- 64-bit intervals (texts of 2^32 characters or more; config 5) ----
 * The reference's bwtint_t is 32-bit (2BWT-Interface.h:26), so its index, its hit
 * record and the drop-in ABI (hsa_bwtaln.h) end at 2^32 - 1 characters.  These entry
 * points run the same search with 64-bit SA intervals.
 *
 * hsa_index_create_device64: as hsa_index_create_device, with 64-bit lengths, '$'
 * rows and C tables, T and rT under 2^36 (HSA_E_ARG otherwise).  The rank blocks keep
 * their counts modulo 2^32 and a wrap table (the blocks where a base count passes a
 * multiple of 2^32, found at creation, 512 bytes in front of the blocks) restores the
 * high part.  An index under 2^32 characters also serves every 32-bit entry point; a
 * longer one only the *64 ones (the others return HSA_E_ARG). */
int hsa_index_create_device64(int device, uint64_t T, uint64_t isa0, const uint64_t C[5], const uint32_t *d_code_lsb,
                              uint64_t rT, uint64_t risa0, const uint64_t rC[5], const uint32_t *d_rcode_lsb,
                              hsa_index_t **out);
int hsa_index_is64(const hsa_index_t *ix);
/* BWTAllOccValue (BWT.c:793) at 64-bit positions 0..T+1: 4 u64 per position. */
int hsa_occ4_batch64(hsa_index_t *ix, int dir, size_t n, const uint64_t *pos, uint64_t *occ4_out);
/* The hit record of the 64-bit search: bwt_aln1_t (bwtaln.h:41-50) with 64-bit
 * k, l, rev_k, rev_l; 14 u32 (56 bytes). */
typedef struct {
    uint32_t n_mm:16, n_gapo:8, n_gape:8;
    uint32_t type:30, strand:2;
    uint64_t k, l, rev_k, rev_l;
    int32_t start, end;
    int32_t score, pad;
} hsa_aln64_t;
/* hsa_search_device on a 64-bit index (hsa_index_create_device64): the same batch
 * and counters; d_hits holds hit_cap hsa_aln64_t records. */
int hsa_search_device64(hsa_index_t *ix, const hsa_regime_t *regimes, int n_regimes,
                        const hsa_device_batch_t *b, void *stream);

/* Suffix-array based BWT construction on the device for a text given as LSB-first
 * 2-bit codes (16 per u32).  Produces the $-less BWT codes (LSB-first) and
 * inverseSa0 = rank of suffix 0 among T+1 suffixes incl. '$' (BWT.h:61-83).
 * `reverse` builds the BWT of the reversed text. */
int hsa_build_bwt_device(int device, uint64_t T, const uint32_t *d_text_lsb, int reverse,
                         uint32_t *d_bwt_lsb, uint32_t *isa0, uint32_t C[5]);
/* The BWT of the text as given (no reversal) and, when d_sa is given, its sampled
 * suffix array as `HSA index` stores it (BWTGenerateSaValue, BWTConstruct.c:1241):
 * d_sa[r / sa_interval] = SA[r] for every row r > 0 with r % sa_interval == 0 (row 0,
 * the '$' row, is the caller's: SA = T).  T < 2^32 - 1 (the .sa values are u32). */
int hsa_build_bwt_index_device(int device, uint64_t T, const uint32_t *d_text_lsb, uint32_t *d_bwt_lsb,
                               uint64_t *isa0, uint64_t C[5], uint32_t sa_interval, uint32_t *d_sa);
/* The same for any T >= 1 (64-bit '$' row and C table); d_bwt_lsb holds ceil(T/16)
 * words.  Device memory besides the text and the output: about T bytes plus 9 GB
 * (u64 suffix positions past 2^32 characters). */
int hsa_build_bwt_device64(int device, uint64_t T, const uint32_t *d_text_lsb, int reverse,
                           uint32_t *d_bwt_lsb, uint64_t *isa0, uint64_t C[5]);

/* ---- text positions on the 64-bit path ----
 * SA index -> text position for an index made by hsa_index_create_device64, of any
 * length under 2^36 (no reference counterpart: the reference ends at 2^32 - 1
 * characters).  CIGAR, NM and MD of the position rows: hsa_refine_rows_device64 below;
 * hit choice, mapQ and the XA rows: hsa_choose_hits_device64 below.
 * Not built: a 64-bit splice path, and an on-disk format for 64-bit samples (the .sa
 * file's values are u32).
 *
 * hsa_build_bwt_index_device64: hsa_build_bwt_index_device for any 1 <= T < 2^36, with
 * u64 samples: d_sa64[r / sa_interval] = SA[r] for every row r > 0 with r % sa_interval
 * == 0, over the T + 1 rows including '$'; entry 0 (the '$' row, SA = T) is the
 * caller's.  d_sa64 holds (T + sa_interval) / sa_interval values, or is NULL (no
 * samples); a non-null d_sa64 with sa_interval 0 is HSA_E_ARG. */
int hsa_build_bwt_index_device64(int device, uint64_t T, const uint32_t *d_text_lsb,
                                 uint32_t *d_bwt_lsb, uint64_t *isa0, uint64_t C[5],
                                 uint32_t sa_interval, uint64_t *d_sa64);
/* Attach the sampled suffix array (values[r / interval] = SA[r], values[0] = T; at least
 * (T + interval) / interval values, HSA_E_ARG otherwise) and the chromosome block table
 * (n_blocks rows of four u64: chrID, blockStart, blockEnd, ori).  Only on an index of
 * hsa_index_create_device64 (HSA_E_ARG otherwise); under 2^32 characters
 * hsa_index_set_sa keeps working beside it, with its own arrays.  Like hsa_index_set_sa
 * they refuse a clone and an index with live clones; hsa_index_clone shares the arrays
 * and hsa_index_free frees them.  The _device variant takes ownership of a device array
 * (hipMalloc'd; the builder's output), so the samples of a 15 Gbp text (3.8 GB at
 * interval 32) never cross PCIe; on an error the array stays the caller's. */
int hsa_index_set_sa64(hsa_index_t *ix, const uint64_t *sa_values, uint64_t n_values,
                       uint32_t interval, const uint64_t *blocks, int n_blocks);
int hsa_index_set_sa64_device(hsa_index_t *ix, uint64_t *d_sa_values, uint64_t n_values,
                              uint32_t interval, const uint64_t *blocks, int n_blocks);
/* Output: 4 u64 per index -- SA value, chrID, 1-based position in the chromosome,
 * position in the text; chrID and position are all-ones when no block holds it (the
 * block search is hsa_sa_position_batch's on 64-bit fields).  An index is walked by LF
 * steps (one 16-byte rank-block load each; the wrap table supplies the counts' high
 * words) to the next sampled row, or to the row of the suffix at position 0 (isa0),
 * where it ends: about `interval` steps, and values[0] is only returned for index 0.
 * The walk is bounded: after HSA_SA_MAX_WALK steps (an environment variable read at
 * each call; default 1 << 22) it stops and the index gets all-ones in all four words,
 * as does an index > T.  On a sampled array that belongs to the index's BWT the bound
 * never fires; it exists so that a mismatched pair ends instead of spinning on a shared
 * device (the 32-bit walk, which follows the reference, has no bound).
 * The _device variant launches on `stream` (NULL = the library's) and does not
 * synchronise. */
int hsa_sa_position_batch64 (hsa_index_t *ix, size_t n, const uint64_t *sa_index, uint64_t *out4);
int hsa_sa_position_device64(hsa_index_t *ix, size_t n, const uint64_t *d_sa_index,
                             uint64_t *d_out4, void *stream);
/* One LF step per index (tests and tools, beside hsa_occ4_batch64): the row of the
 * suffix one character longer; the '$' row (isa0) answers 0.  Indices 0..T (HSA_E_ARG
 * past T).  Needs no suffix array. */
int hsa_psi_minus_batch64   (hsa_index_t *ix, size_t n, const uint64_t *sa_index, uint64_t *out);

/* The hit lists of hsa_search_device64, as they sit on the device, to positions.
 * Read j's rows are its hit records in list order, each record's SA rows k .. l
 * ascending, cut to the first max_occ (> 0) rows of the read as a whole; a read with
 * n_aln <= 0 (no hit, or left with HSA_F_OVERFLOW) has none.  d_pos_off[j] is the first
 * row of read j and d_pos_off[n_jobs] the total: in read order, so two runs give the
 * same arrays (hit_off comes from the search's atomics and does not).  Row t: d_pos + 4 t
 * as hsa_sa_position_device64 writes it, d_pos_hit[t] the index of its record within the
 * read's list.  Rows past pos_cap are not written: d_counters[0] > d_counters[1] tells
 * the caller to run again with more room (the hit_cap convention).  d_counters (>= 4
 * u64, zeroed by the call): [0] rows wanted, [1] rows written, [2] walks cut by
 * HSA_SA_MAX_WALK (those rows are all-ones).  d_hits must be 8-byte aligned.
 * Three launches on `stream` (NULL = the library's), one lane per output row in the
 * last; the call does not synchronise. */
typedef struct {
    const int32_t *d_n_aln; const uint64_t *d_hit_off; const uint32_t *d_hits; /* hsa_aln64_t */
    int n_jobs; uint32_t max_occ;
    uint64_t *d_pos_off;      /* n_jobs + 1: exclusive prefix sum of the per-read row counts */
    uint64_t *d_pos;          /* 4 u64 per row, as hsa_sa_position_device64 */
    uint32_t *d_pos_hit;      /* per row: index of its hit record within the read's list */
    uint64_t pos_cap;         /* rows d_pos / d_pos_hit hold */
    uint64_t *d_counters;     /* >= 4 u64: [0] rows wanted, [1] rows written, [2] walks cut by the bound */
} hsa_hitpos_batch64_t;
int hsa_hit_positions_device64(hsa_index_t *ix, const hsa_hitpos_batch64_t *b, void *stream);

/* ---- position rows to CIGAR, NM and MD on the 64-bit path ----
 * refine_gapped_core (bwtse.c:380-440) with its banded global alignment
 * (aln_global_core with aln_param_bwa, stdaln.c:227, :345-525; aln_path2cigar32 :1010)
 * and bwa_cal_md1 (bwtse.c:442-494), for every row hsa_hit_positions_device64 wrote.
 *
 * The text.  hsa_index_set_text64_device attaches it as the 64-bit builder takes it:
 * 2-bit codes, LSB-first, 16 per u32, ceil(T / 16) words of device memory (hipMalloc'd),
 * T the index's length (HSA_E_ARG otherwise).  The handle takes ownership; only on an
 * index of hsa_index_create_device64, refused on a clone and on an index with live
 * clones, as hsa_index_set_sa64_device; clones share the array, the last free releases
 * it, and on an error the array stays the caller's.  An index under 2^32 characters that
 * has the host's packed text (hsa_index_set_text) is served from that array when no
 * 64-bit text is attached. */
int hsa_index_set_text64_device(hsa_index_t *ix, uint32_t *d_text_lsb, uint64_t T);

/* Per-row status: a row is answered exactly (HSA_RF_OK) or refused, never approximated. */
#define HSA_RF_OK    0u
#define HSA_RF_POS   1u   /* the position row is all-ones (no block, or a walk cut by the bound) */
#define HSA_RF_TEXT  2u   /* the ungapped compare would read past the text (the reference has no
                             bound at bwtse.c:480-482), or a gapped row starts at or past its end
                             (an empty window: the reference dereferences a NULL CIGAR) */
#define HSA_RF_CAP   3u   /* the read or the gap is past the kernel's layout */
#define HSA_RF_MD    4u   /* the CIGAR or the MD string did not fit its stride: n_cigar and md_len
                             hold the needed lengths, the arrays their first stride entries */
/* The layout: every row with len <= the batch's max_len (at most HSA_RF_MAX_LEN) and
 * n_gapo + n_gape <= HSA_RF_MAX_GAP is answered; HSA_RF_CAP is only for rows past that. */
#define HSA_RF_MAX_LEN 4095
#define HSA_RF_MAX_GAP 27
#define HSA_RF_ROW_WORDS 8
/* Row t (the position call's row t) gets
 *   d_rows + 8 t   status, n_cigar, NM, md_len, ref bases dropped at the 5' end, at the 3' end
 *                  (the reference's *start += / *end -= adjustments, bwtse.c:417, :424:
 *                  reported, the caller applies them), two zero words;
 *   d_rpos + 2 t   the refined text position and 1-based position in the chromosome: a
 *                  leading deletion's length is added to both without a new block lookup,
 *                  as bwtse.c:413-417 does;
 *   d_cigar + cigar_stride t   the ops as bwa_cigar_t (bwtaln.h:70-80: op << 28 | len,
 *                  op 0 M, 1 I, 2 D, 4 S);
 *   d_md + md_stride t         the MD string's bytes (md_len of them, no terminator).
 * A row's gap count is its record's n_gapo + n_gape (bwtse.c:89, :561).  Gap 0: no
 * alignment; the CIGAR is one `len`M op (a difference from the reference, which keeps a NULL
 * CIGAR there and prints "<len>M"), MD and NM from bwa_cal_md1's no-gap branch.  Gap > 0:
 * the window is len + gap text characters from the row's position, cut at the text's end
 * (:391-394); end deletions are stripped and end insertions become S (:413-434); MD and NM
 * from the CIGAR branch.  The read handed to the alignment is the reference's
 * `strand ? rseq : seq` (:554): d_codes as they are for strand 0, their reverse complement
 * for strand 1 (bwaseqio.c:212-215 with the complement the aligner's default mode sets).
 * Rows other than HSA_RF_OK / HSA_RF_MD get zero lengths and their position unrefined.
 *
 * Inputs are the search batch (d_jobs, d_codes, d_hit_off, d_hits as hsa_aln64_t) and the
 * position call's outputs as they sit on the device; the row count is
 * min(d_pos_off[n_jobs], pos_cap, d_pos_counters[1]) (d_pos_counters may be NULL), read on
 * the device: no host round trip.  d_counters (>= 8 u64, zeroed by the call): [0] rows,
 * [1 + s] rows of status s (s = 0..4), [6] rows that ran the alignment, [7] unused.
 * Two launches on `stream` (NULL = the library's); the call does not synchronise.
 * Needs a text (above); scratch grows on the handle (hsa_index_release_scratch).
 *
 * The rows may be hsa_hit_positions_device64's (every row up to max_occ) or
 * hsa_choose_hits_device64's (below: the chosen row and the XA rows, same layout).
 *
 * Not built, and left to the caller: bwa_correct_trimmed (:496-534, needs full_len, which
 * the device batch does not carry), a 32-bit-record (bwt_aln1_t) variant, and an on-disk
 * format for 64-bit samples.  The segments of a spliced read (:562-619) are aligned by these
 * kernels from hsa_splice_lines_device (below).  The drop-in's SAM stage keeps the host's
 * bwa_refine_gapped. */
typedef struct {
    const hsa_job_t *d_jobs; int n_jobs;
    const uint8_t *d_codes;
    const uint64_t *d_hit_off; const uint32_t *d_hits;       /* the search's: hsa_aln64_t */
    const uint64_t *d_pos_off; const uint64_t *d_pos; const uint32_t *d_pos_hit;
    uint64_t pos_cap;                /* rows the position arrays and the outputs hold */
    const uint64_t *d_pos_counters;  /* the position call's counters, or NULL */
    int32_t max_len;                 /* longest read of the batch: sizes the scratch */
    uint32_t cigar_stride, md_stride; /* ops / bytes per row */
    uint32_t *d_rows;                /* HSA_RF_ROW_WORDS u32 per row */
    uint64_t *d_rpos;                /* 2 u64 per row */
    uint32_t *d_cigar;
    uint8_t *d_md;
    uint64_t *d_counters;            /* >= 8 u64 */
} hsa_refine_batch64_t;
int hsa_refine_rows_device64(hsa_index_t *ix, const hsa_refine_batch64_t *b, void *stream);

/* ---- each read's hit, mapQ and XA rows on the 64-bit path ----
 * bwt_aln2seq_core(p, 1, n_multi) (bwtse.c:21-113; the reference calls it with n_multi 3,
 * bwtaln.c:514), the multi-row filter of bwa_cal_pac_pos (:360-366) and bwa_approx_mapQ
 * (:122-131) for the hit lists of hsa_search_device64 as they sit on the device; search ->
 * choose -> refine gives, without a host round trip, what bwa_print_sam1 prints for an
 * unspliced single-end read.
 *
 * The draws.  The reference picks among a read's equal-best records with the process-wide
 * drand48 sequence, consumed in read order.  rng_state is the generator's 48-bit state
 * before read 0 (HSA_DRAND48_SEED0 in a process that never seeds, as the reference: glibc
 * starts from X = 0, not from the 0x1234ABCD330E of the SVID text);
 * *d_rng_out is the state after the last read.  A sub-range [s, e) of a batch is served by
 * passing d_jobs + s, d_n_aln + s, d_hit_off + s (d_hits as it is), n_jobs = e - s, the
 * outputs offset the same way (d_sel + 4 s, d_sel64 + 4 s; the row arrays start at 0 for
 * every call) and the state the call for [0, s) left: calls chained like this give what
 * one call gives, and the reference's batches of 0x40000 reads chain the same way.
 *
 * Outputs, all in read order (two runs give equal arrays):
 *   d_sel + 4 j    type (0 no hit: n_aln <= 0; 1 unique; 2 repeat), index of the chosen
 *                  record in the read's list, mapQ (with the job's max_diff), XA rows;
 *   d_sel64 + 4 j  the chosen SA row, c1 (rows of the equal-best records: X0), c2 (rows of
 *                  the others: X1), the generator's state at the start of the read;
 *   d_pos_off, d_pos, d_pos_hit (pos_cap rows): the layout of hsa_hit_positions_device64,
 *                  which hsa_refine_rows_device64 takes unchanged.  A read with a hit has
 *                  one row, or, when its records hold n <= n_multi + 1 rows in all, n rows:
 *                  row 0 the chosen SA row, rows 1.. the others in list order, k .. l
 *                  ascending (the reference drops the multi row at the main row's position,
 *                  and distinct SA rows have distinct positions).  d_pos_hit: the row's
 *                  record.  No draw is made for them (bwtse.c:93-108 cannot be reached).
 * d_counters (>= 8 u64, zeroed by the call): [0] rows wanted, [1] rows written (rows past
 * pos_cap are not written: run again with more room), [2] walks cut by HSA_SA_MAX_WALK,
 * [3] reads with a hit, [4] repeat reads, [5] reads whose draws were walked in order (two
 * or more equal-best records), [6] zero-draw reads, [7] the lowest of them (all-ones: none).
 *
 * The zero-draw read.  A read with one equal-best record makes two draws unless the first
 * is exactly 0 (probability 2^-48), when bwtse.c:44 is false and it makes one.  The states
 * are computed for two.  Such a read is counted in [6]: it keeps the reference's zeroed
 * fields (record 0, SA row 0; its other rows omit the read's first row), the states of the
 * reads after it and *d_rng_out are NOT the sequential ones, and the caller re-runs from
 * read [7] + 1 with the successor of d_sel64[4 * [7] + 3] (one draw) as the state.  All other values are
 * the sequential walk's for every input (64-bit k, l, counts: the reference's wherever its
 * 32-bit arithmetic does not wrap).
 *
 * d_log_n: 256 int32 on the device, g_log_n[i] = (int)(4.343 * log(i) + 0.5), [0] unused
 * (bwtse.c:841; computed on the host so that no device log enters).  d_sel, d_sel64 and
 * d_hits 16-, 16- and 8-byte aligned.  Needs hsa_index_set_sa64's arrays (HSA_E_ARG
 * otherwise, as for null pointers and a state of 2^48 or more).  Six kernels and a scan
 * on `stream` (NULL = the library's); the call does not synchronise; scratch grows on the
 * handle (hsa_index_release_scratch). */
#define HSA_DRAND48_SEED0 0ull
typedef struct {
    const hsa_job_t *d_jobs; int n_jobs;
    const int32_t *d_n_aln; const uint64_t *d_hit_off; const uint32_t *d_hits;   /* hsa_aln64_t */
    uint32_t n_multi;
    uint64_t rng_state;
    const int32_t *d_log_n;
    uint32_t *d_sel;          /* 4 u32 per read */
    uint64_t *d_sel64;        /* 4 u64 per read */
    uint64_t *d_rng_out;      /* 1 u64 */
    uint64_t *d_pos_off;      /* n_jobs + 1 */
    uint64_t *d_pos;          /* 4 u64 per row */
    uint32_t *d_pos_hit;
    uint64_t pos_cap;
    uint64_t *d_counters;     /* >= 8 u64 */
} hsa_choose_batch64_t;
int hsa_choose_hits_device64(hsa_index_t *ix, const hsa_choose_batch64_t *b, void *stream);
/* Probes: hsa_choose_timing(1) makes every later call record events around its launches
 * (process-wide; off by default: nothing is recorded), and hsa_choose_launch_times waits
 * for the handle's last timed call and gives the HSA_CH_LAUNCHES times in ms: the class
 * kernel (with the counters' memset), the scan, the compaction, the maps, the one-wave
 * walk, the choice, the rows. */
#define HSA_CH_LAUNCHES 7
void hsa_choose_timing(int on);
int hsa_choose_launch_times(hsa_index_t *ix, float *ms);

/* ---- SAM lines on the 64-bit path ----
 * bwa_print_sam1 with mate == NULL (bwtse.c:698-799) for the reads of one batch, from the
 * outputs of search, choose and refine as they sit on the device: the finished text in
 * device memory, in read order, ready for one copy to the host and one write().  The
 * line of read j is what hsa_amd/sam.py: sam_line gives for it, byte for byte, and '\n':
 *   name, flag (| 16 on strand 1, :706), chromosome name, d_rpos[2 r0 + 1], mapQ, the CIGAR
 *   (len then "MIDNSHP=X"[op], :713), "*", "0", "0" (:720), SEQ ("ACGTN"[code]; on strand 1
 *   the reversed read through "TGCAN", :737-742), QUAL (reversed on strand 1, or "*",
 *   :744-749), XT:A:U|R (:762), NM|CM:i: (:763), X0:i:c1, X1:i:c2 only when c1 <= max_top2
 *   (:766-769), XM, XO, XG (:772-774), MD:Z: (:775), and with XA rows XA:Z: and per row
 *   chr,(+|-)pos and then its CIGAR for a gapped record (n_gapo + n_gape > 0) or
 *   ",<n_mm + gaps>;" for an ungapped one (:781-796);
 * tab-separated.  r0 = d_pos_off[j] is the read's chosen row, rows r0 + 1 .. r0 + n_xa
 * (d_sel[4 j + 3]) its XA rows; a row's strand and difference counts are those of its
 * record d_hits[d_hit_off[j] + d_pos_hit[t]]; a row's chromosome name is d_chr_names
 * [d_chr_off[c] .. d_chr_off[c + 1]) with c the position row's chrID word (d_pos[4 t + 1]).
 * c1, c2 and the positions print as full u64 decimals (the reference's (int) casts have no
 * counterpart past 2^32).  The row count is min(d_pos_off[n_jobs], pos_cap,
 * d_pos_counters[1]) (d_pos_counters may be NULL), read on the device as
 * hsa_refine_rows_device64 reads it.
 *
 * Names and qualities: d_names / d_quals are bytes, d_name_off / d_qual_off n_jobs + 1
 * offsets into them; the bytes are printed as given (the caller cuts the FASTQ comment, as
 * the reference's reader does).  d_quals and d_qual_off both NULL: "*" for every read.
 *
 * Outputs:
 *   d_line_off   n_jobs + 1: the exclusive prefix sum, in read order, of the line lengths
 *                with the '\n'; a read without a line has length 0.  Two runs give equal
 *                arrays.
 *   d_out        the lines, concatenated in read order; bytes at or past out_cap are not
 *                written and no byte past d_out + out_cap is touched.
 *   d_line_stat  per read: HSA_SAM_OK a line; HSA_SAM_NOHIT d_sel type 0, no line (as
 *                :922 skips it); HSA_SAM_ROWS one of its 1 + n_xa rows lies past the rows
 *                written (pos_cap too small); HSA_SAM_REFINE the chosen row or an XA row has a
 *                refine status other than HSA_RF_OK; HSA_SAM_INPUT an input that would
 *                index out of bounds: a d_sel type over 2, fewer than 1 + n_xa rows between
 *                d_pos_off[j] and [j + 1], chrID >= n_chr, d_pos_hit >= the read's n_aln, a
 *                CIGAR op code > 8, n_cigar > cigar_stride, md_len > md_stride, a base code
 *                > 4, a decreasing name, quality or chromosome-name offset, a quality
 *                length other than the read's, or a line longer than max_line.  A read is
 *                printed exactly or not at all; every index taken from a device array is
 *                checked before it is used.  HSA_SAM_REFINE goes before HSA_SAM_INPUT.
 *   d_counters   (>= 8 u64, zeroed by the call) [0] bytes wanted, [1] bytes written
 *                (min(wanted, out_cap)), [2] lines, [2 + s] reads of status s (s = 1..4), [7]
 *                the lowest read of status >= 2 (all-ones: none).  [0] > [1]: run again
 *                with more room (the hit_cap convention).
 * max_line bounds the batch's longest line (with its '\n'; 1..HSA_SAM_MAX_LINE, HSA_E_ARG otherwise):
 * it sizes the tile of the writing kernel (below), so the caller states it; hsa_amd/sam.py:
 * line_bound computes one from the strings' lengths and the strides.
 *
 * A sub-range [s, e) of a batch is served as the choice's: d_jobs + s, d_n_aln + s,
 * d_hit_off + s, d_sel + 4 s, d_sel64 + 4 s, d_name_off + s, d_qual_off + s, n_jobs = e - s;
 * d_codes, d_hits, the string bytes and the row arrays (which start at 0 for every call of
 * the choice) as they are.
 *
 * Three launches on `stream` (NULL = the library's): k_sam_len (one lane per read: status
 * and exact length), the exclusive scan, k_sam_write (one wavefront per tile of consecutive
 * reads: the tile's contiguous range is assembled in LDS and leaves in aligned 16-byte
 * stores, its ragged ends as byte stores).  No atomics place anything.  The call does not
 * synchronise; scratch grows on the handle (hsa_index_release_scratch).  Null pointers and
 * inconsistent sizes: HSA_E_ARG.
 *
 * Spliced reads (N ops, XT:A:S) have a writer of their own, hsa_splice_lines_device below.
 * Not built: trimmed reads (bwa_correct_trimmed, the XC
 * tag, the reference's reversal of only `len` quality bytes of a full_len read), RG and BC
 * tags, paired reads, the @SQ header lines, a 32-bit-record (bwt_aln1_t) variant.  The
 * drop-in's host SAM stage stays as it is. */
#define HSA_SAM_OK     0u
#define HSA_SAM_NOHIT  1u
#define HSA_SAM_ROWS   2u
#define HSA_SAM_REFINE 3u
#define HSA_SAM_INPUT  4u
#define HSA_SAM_MAX_LINE 61440u
typedef struct {
    const hsa_job_t *d_jobs; int n_jobs;
    const uint8_t *d_codes;
    const int32_t *d_n_aln; const uint64_t *d_hit_off; const uint32_t *d_hits;   /* hsa_aln64_t */
    const uint32_t *d_sel; const uint64_t *d_sel64;          /* the choice's */
    const uint64_t *d_pos_off; const uint64_t *d_pos; const uint32_t *d_pos_hit;
    uint64_t pos_cap;
    const uint64_t *d_pos_counters;  /* the choice's counters, or NULL */
    const uint32_t *d_rows; const uint64_t *d_rpos;          /* the refinement's */
    const uint32_t *d_cigar; const uint8_t *d_md;
    uint32_t cigar_stride, md_stride;
    const uint8_t *d_names; const uint64_t *d_name_off;      /* n_jobs + 1 */
    const uint8_t *d_quals; const uint64_t *d_qual_off;      /* n_jobs + 1, or both NULL */
    const uint8_t *d_chr_names; const uint64_t *d_chr_off;   /* n_chr + 1 */
    uint32_t n_chr;
    uint32_t flag;                   /* the reads' extra_flag */
    int32_t max_top2;                /* gap_opt_t.max_top2 */
    int32_t comp_read;               /* BWA_MODE_COMPREAD: NM, else CM */
    uint32_t max_line;               /* the longest line the batch can have, '\n' included */
    uint64_t *d_line_off;            /* n_jobs + 1 */
    uint8_t *d_out; uint64_t out_cap;
    uint32_t *d_line_stat;           /* n_jobs */
    uint64_t *d_counters;            /* >= 8 u64 */
} hsa_sam_batch64_t;
int hsa_sam_lines_device64(hsa_index_t *ix, const hsa_sam_batch64_t *b, void *stream);
/* Trimmed reads and barcodes (bwa aln -q, -B; hsa_reads_device_opts leaves both arrays), for
 * the two line writers.  d_full_len (n_jobs u32, or NULL: every read is whole): the length a
 * read is stored with at hsa_job_t.off and in d_quals, at least hsa_job_t.len, which is then
 * clip_len, the length the search saw.  The writers print SEQ and QUAL over the stored
 * length (reversed over it on the reverse strand), apply bwa_correct_trimmed (bwtse.c:496-534)
 * to the line's own CIGAR (the stored minus the searched length joins a last S op on the
 * forward strand, a first one on the reverse strand, or becomes an S op there; the XA
 * rows' CIGARs stay as they are), and print "\tXC:i:<hsa_job_t.len>" behind QUAL for a
 * trimmed read.  d_bc (bc_len bytes per job, bc_len 1..HSA_SAM_MAX_BC, or NULL and 0):
 * "\tBC:Z:<the read's bytes>" behind QUAL, before XC (:755-758).  max_line must bound the
 * longer lines.  With `trim` NULL the calls are hsa_sam_lines_device64 and
 * hsa_splice_lines_device, byte for byte. */
#define HSA_SAM_MAX_BC 63u
typedef struct {
    const uint32_t *d_full_len;
    const uint8_t *d_bc;
    uint32_t bc_len;
} hsa_sam_trim_t;
int hsa_sam_lines_device64_trim(hsa_index_t *ix, const hsa_sam_batch64_t *b, const hsa_sam_trim_t *trim, void *stream);
/* Probes, as hsa_choose_timing / hsa_choose_launch_times: the HSA_SAM_LAUNCHES times in ms of
 * the handle's last timed call: k_sam_len (with the counters' memsets), the scan,
 * k_sam_write. */
#define HSA_SAM_LAUNCHES 3
void hsa_sam_timing(int on);
int hsa_sam_launch_times(hsa_index_t *ix, float *ms);

/* ---- the SAM lines of spliced reads ----
 * What the reference does with a read whose bwt_splice_match result is two records of type
 * BWA_TYPE_SPLICING, after the search: bwt_aln2pos_splicing with bwt_combine_segment_splice
 * (bwtse.c:295-348, :197-235), the splicing branch of bwa_refine_gapped (:562-595, over
 * refine_gapped_core :380-440) and the XT:A:S line of bwa_print_sam1 (:677-799).  Python
 * restatements: hsa_amd.splice.pair_segments / merge_cigar, hsa_amd.sam.spliced_line.
 *
 * Inputs: the batch (d_jobs, d_codes, names and qualities as hsa_sam_batch64_t takes them),
 * d_flags and d_n_aln as hsa_splice_device took them (they say which jobs' d_res words were
 * written), d_res of hsa_splice_device, the chromosome names.  Needs hsa_index_set_sa and a
 * text (hsa_index_set_text), and an index under 2^32 characters (HSA_E_ARG otherwise).
 *
 * Outputs, in hsa_sam_lines_device64's conventions: d_line_off (n_jobs + 1 exclusive
 * offsets, a read without a line has length 0), d_out / out_cap (nothing is written at or
 * past out_cap), d_line_stat per read, d_counters: [0] bytes wanted, [1] bytes written,
 * [2] lines, [3] reads the splice kernel handed back, [4] reads with more than one pair,
 * [5] reads refused otherwise, [6] reads without a pair (the reference prints no line for
 * them either), [7] spliced results seen.  d_rows: HSA_SL_ROW_WORDS u32 per read, written
 * for every read: status, n_rows, n_splice, c1 (= c2: the capped row count of :310-312),
 * strand, the merged n_cigar, then per segment chrID, 1-based position, text position,
 * start, end and mm (after refine_gapped_core's adjustments when the status is
 * HSA_SL_OK, as paired otherwise), the N length, mm0 + mm1, and the two segments' n_cigar.
 * d_cigar: the merged CIGAR, cigar_stride words per read ((op << 28) | length, op an index
 * into "MIDNSHP=X").
 *
 * A read gets the reference's line or none (d_line_stat): HSA_SL_NONE not a spliced
 * result (not sent to the splice path, or n_aln is not 2 records of type 4); HSA_SL_HANDED
 * hsa_splice_device's status is > 0; HSA_SL_NOPAIR no pair of rows combines (the reference
 * sets BWA_TYPE_NO_MATCH, :339-342); HSA_SL_MULTI more than one pair (the reference prints
 * the others as XA in a format of its own, :596-618: hsa_splice_lines_device_xa below
 * prints them; these two calls refuse the read); HSA_SL_REFINE a segment's
 * alignment was not answered; HSA_SL_POS a paired row lies in no chromosome block, or the
 * two on different chromosomes; HSA_SL_INTRON the N length is not positive; HSA_SL_INPUT a
 * record field, string offset or CIGAR outside what the layout holds, or a line past
 * max_line.
 *
 * Four launches and a scan on the caller's stream (NULL: the index's own), no
 * synchronisation, no atomic places a byte: one wavefront per read pairs the rows (lanes
 * along the SA walks and the sort), the two segments go through hsa_refine_rows_device64's
 * kernels with every row aligned, one lane per read merges and measures, rocPRIM scans,
 * one wavefront per read writes.  Scratch grows on the handle (hsa_index_release_scratch). */
#define HSA_SL_ROW_WORDS 24
#define HSA_SL_OK     0u
#define HSA_SL_NONE   1u
#define HSA_SL_HANDED 2u
#define HSA_SL_NOPAIR 3u
#define HSA_SL_MULTI  4u
#define HSA_SL_REFINE 5u
#define HSA_SL_POS    6u
#define HSA_SL_INTRON 7u
#define HSA_SL_INPUT  8u
typedef struct {
    const hsa_job_t *d_jobs; int n_jobs;
    const uint8_t *d_codes;
    const uint32_t *d_flags; const int32_t *d_n_aln;         /* as hsa_splice_batch_t */
    const uint32_t *d_res;                                   /* HSA_SP_RES_WORDS per job */
    const uint8_t *d_names; const uint64_t *d_name_off;      /* n_jobs + 1 */
    const uint8_t *d_quals; const uint64_t *d_qual_off;      /* n_jobs + 1, or both NULL */
    const uint8_t *d_chr_names; const uint64_t *d_chr_off;   /* n_chr + 1 */
    uint32_t n_chr;
    uint32_t flag;                   /* the reads' extra_flag */
    int32_t max_top2;                /* gap_opt_t.max_top2 */
    int32_t comp_read;               /* BWA_MODE_COMPREAD: NM, else CM */
    int32_t max_len;                 /* longest read of the batch */
    uint32_t max_line;               /* the longest line the batch can have, '\n' included */
    uint32_t cigar_stride;           /* ops of a merged CIGAR */
    uint32_t pad;
    uint32_t *d_rows;                /* HSA_SL_ROW_WORDS u32 per job */
    uint32_t *d_cigar;               /* cigar_stride u32 per job */
    uint64_t *d_line_off;            /* n_jobs + 1 */
    uint8_t *d_out; uint64_t out_cap;
    uint32_t *d_line_stat;           /* n_jobs */
    uint64_t *d_counters;            /* >= 8 u64 */
} hsa_splice_lines_batch_t;
int hsa_splice_lines_device(hsa_index_t *ix, const hsa_splice_lines_batch_t *b, void *stream);
/* ... with trimmed reads and barcodes (hsa_sam_trim_t above; the segments lie in hsa_job_t.len) */
int hsa_splice_lines_device_trim(hsa_index_t *ix, const hsa_splice_lines_batch_t *b, const hsa_sam_trim_t *trim, void *stream);
/* ... and with the XA:Z lists of reads whose segments combine into several pairs at the
 * shortest distance (bwtse.c:596-618 and :782-797).  The two calls above give such a read
 * HSA_SL_MULTI and no line, and keep doing so; through this one it gets the reference's whole
 * line.  bwt_combine_segment_splice keeps the pair at the sorted index where the shortest
 * distance was last lowered and every later adjacent (segment 0, segment 1) pair on one
 * chromosome at that distance, in sorted order, at most 50.  Pair 0 is the read's own
 * alignment as before; pair i >= 1 ("extra pair" below) is XA entry i - 1: both segments go
 * through refine_gapped_core, and the entry is "<chr>,<+|-><segment 0's position>" followed
 * directly by the ops of (segment 0's CIGAR, N of ori_pos1 - ori_pos0 - end0, segment 1's
 * CIGAR) from "MIDNS" -- no comma, no edit count, no ';', the entries abut.
 * bwa_correct_trimmed does not touch these CIGARs.
 *
 * The number of extra pairs is known only on the device and the call makes no host round
 * trip, so the caller states the room (pair_cap extra pairs for the whole batch, as out_cap
 * states the text's).  Reads are served in read order while their pairs fit; a read whose
 * pairs do not fit gets HSA_SL_MULTI and no line.  d_counters (>= 8 u64, zeroed by the call):
 * [0] extra pairs wanted, [1] extra pairs served, [2] reads printed with a list, [3] entries
 * printed.  [0] > pair_cap: run again with [0] pairs of room; then no read is HSA_SL_MULTI.
 * An extra pair that fails refuses the whole read with that pair's status (a row in no
 * chromosome block HSA_SL_POS, a segment not answered HSA_SL_REFINE, an N length that is not
 * positive HSA_SL_INTRON, a CIGAR past cigar_stride HSA_SL_INPUT): exact or nothing.
 *
 * Outputs: d_pair_off (n_jobs + 1: read j's extra pairs are [d_pair_off[j], d_pair_off[j +
 * 1]), whether they were served or not), d_pair_rows (HSA_SL_XA_WORDS u32 per served extra
 * pair: status, read, bytes of its entry, the entry's offset in the read's XA text, merged
 * n_cigar, N length, chrID, then segment 0's 1-based position, text position and end and
 * segment 1's 1-based position and text position (after refine_gapped_core's adjustments
 * when the status is HSA_SL_OK), strand, the two segments' n_cigar, segment 0's position as
 * paired), d_pair_cigar (the batch's cigar_stride words per extra pair).  d_rows words 22
 * and 23 of a read hold its served extra pairs and the bytes of its XA text.  With no read
 * of several pairs the text, the rows and the eight counters are those of
 * hsa_splice_lines_device_trim.  `trim` may be NULL.
 *
 * Launches: k_sl_pair also counts each read's extra pairs, a scan gives d_pair_off, k_sl_room
 * blanks the extra refine rows, k_sl_fill (one wavefront per read with extra pairs, the
 * others leave at once; the lanes test the sorted rows and number the kept pairs by ballot
 * and prefix popcount) fills them behind the 2 n_jobs rows of the first pairs, one refine
 * launch serves all rows, k_sl_xlen (one lane per extra pair) merges and measures the entries,
 * and k_sl_write's lanes format a read's entries side by side. */
#define HSA_SL_XA_WORDS 16
#define HSA_SL_XA_UNUSED 0xFFFFFFFFu   /* d_pair_rows word 0 of a slot no pair was served in */
typedef struct {
    uint64_t pair_cap;               /* room: extra pairs of the whole batch */
    uint64_t *d_pair_off;            /* n_jobs + 1 */
    uint32_t *d_pair_rows;           /* HSA_SL_XA_WORDS u32 per extra pair (pair_cap of them) */
    uint32_t *d_pair_cigar;          /* cigar_stride u32 per extra pair */
    uint64_t *d_counters;            /* >= 8 u64 */
} hsa_splice_xa_t;
int hsa_splice_lines_device_xa(hsa_index_t *ix, const hsa_splice_lines_batch_t *b, const hsa_sam_trim_t *trim,
                               const hsa_splice_xa_t *xa, void *stream);
/* The lines of two writers over the same reads (hsa_sam_lines_device64's and
 * hsa_splice_lines_device's: a read has a line from at most one of them) as one text in read
 * order: d_line_off[j] is the sum of the two inputs' offsets, and read j's bytes are writer
 * a's, then writer b's.  A scan over the summed lengths and one copy kernel (a wavefront per
 * read, 16-byte stores where source and destination are congruent modulo 16), on the caller's
 * stream, no synchronisation.  text_a_len / text_b_len: the bytes the two texts hold (a line
 * whose offsets run backwards or past them counts as empty).  d_counters (>= 8 u64): [0]
 * bytes wanted, [1] bytes written; nothing is written at or past out_cap. */
typedef struct {
    int n_jobs;
    const uint64_t *d_line_off_a; const uint8_t *d_text_a; uint64_t text_a_len;
    const uint64_t *d_line_off_b; const uint8_t *d_text_b; uint64_t text_b_len;
    uint64_t *d_line_off;            /* n_jobs + 1 */
    uint8_t *d_out; uint64_t out_cap;
    uint64_t *d_counters;
} hsa_sam_merge_batch_t;
int hsa_sam_merge_device(hsa_index_t *ix, const hsa_sam_merge_batch_t *b, void *stream);

/* ---- the splice junction table ----
 * One row per distinct intron of the XT:A:S lines a run prints, with its read support, as text
 * in the nine tab-separated columns of STAR's SJ.out.tab: chromosome name; first base of the
 * intron, 1-based (POS plus the M and D lengths before the N); last base (first + N length -
 * 1); strand from the motif (1 for motifs 1 3 5, 2 for 2 4 6, 0 for 0); motif from the forward
 * text's two first and two last intron bases (1 GT/AG, 2 CT/AC, 3 GC/AG, 4 CT/GC, 5 AT/AC,
 * 6 GT/AT, 0 anything else); 0 (no annotation); lines with this intron and no XA:Z list;
 * lines with it and a list; the maximum over those lines of min(M lengths before the N, M
 * lengths behind it).  Rows are in (chrID, first base, last base) order, lines end in '\n',
 * no header.  The reference prints no such table: it is a function of the printed SAM text
 * and the index's text and block table (hsa_amd.junctions.from_sam restates it from them).
 * Only a line's own alignment counts; the introns of its XA:Z entries do not (the reference
 * prints an entry's position and first op length with nothing between them, so the text does
 * not determine them).
 *
 * A row buffer: HSA_JN_ROW_WORDS u32 per row: chrID, first base, last base, lines without a
 * list, lines with one, overhang, motif (written by the reduction; 0 before), 0.  Rows carry
 * counts, so a reduced table is a row buffer too.
 *
 * The three calls launch on the caller's stream (NULL: the index's own) without
 * synchronising, keep their scratch on the handle (hsa_index_release_scratch; shared with
 * hsa_splice_lines_device, so on one stream with it), zero their d_counters (>= 8 u64), write
 * nothing past a capacity, place no row or byte with an atomic, and give equal arrays when run
 * twice.  They need an index under 2^32 characters.
 *
 * hsa_junction_rows_device appends one row per read whose d_line_stat is HSA_SL_OK, in read
 * order, behind the n_have rows the buffer holds, from one lines call's d_rows, d_cigar and
 * d_line_stat (a flag per read, a scan, a write).  d_counters: [0] rows wanted, [1] rows
 * written (min of [0] and row_cap - n_have); [0] > [1]: grow the buffer and run again.
 *
 * hsa_junction_reduce_device sorts the n_rows rows (rocPRIM radix sort over the three key
 * words) and merges equal introns in place (rocPRIM reduce_by_key: sums of the two counts,
 * max of the overhang, runs of any length), then reads each distinct intron's motif from the
 * packed text: each of the four bases' chromosome coordinates maps through the block table
 * on its own, and a base in no block (inside an N run) makes the motif 0.  Idempotent.
 * Needs hsa_index_set_sa (the block table, ascending in (chrID, ori) as the .ann file lists
 * it) and hsa_index_set_text.  d_counters: [0] rows in, [1] rows out.
 *
 * hsa_junction_text_device writes the text of a reduced table in hsa_sam_lines_device64's
 * layout: d_line_off (n_rows + 1), d_out / out_cap, d_counters: [0] bytes wanted, [1] bytes
 * written, [2] rows printed, [3] rows without a line (a chrID past n_chr or a motif past 6:
 * none from the calls above). */
#define HSA_JN_ROW_WORDS 8
typedef struct {
    int n_jobs;
    uint32_t cigar_stride;
    const uint32_t *d_rows;          /* hsa_splice_lines_batch_t's d_rows, d_cigar, d_line_stat after the call */
    const uint32_t *d_cigar;
    const uint32_t *d_line_stat;
    uint32_t *d_jrows;               /* HSA_JN_ROW_WORDS u32 per row, row_cap rows, 16-byte aligned */
    uint64_t n_have;                 /* rows the buffer holds already */
    uint64_t row_cap;                /* at most 2^32 - 1 */
    uint64_t *d_counters;
} hsa_junction_rows_batch_t;
int hsa_junction_rows_device(hsa_index_t *ix, const hsa_junction_rows_batch_t *b, void *stream);
typedef struct {
    uint32_t *d_jrows;               /* n_rows rows in, d_counters[1] rows out */
    uint64_t n_rows;
    uint64_t *d_counters;
} hsa_junction_reduce_batch_t;
int hsa_junction_reduce_device(hsa_index_t *ix, const hsa_junction_reduce_batch_t *b, void *stream);
typedef struct {
    const uint32_t *d_jrows;         /* a reduced table */
    uint64_t n_rows;
    const uint8_t *d_chr_names; const uint64_t *d_chr_off;   /* n_chr + 1 */
    uint32_t n_chr;
    uint32_t pad;
    uint64_t *d_line_off;            /* n_rows + 1 */
    uint8_t *d_out; uint64_t out_cap;
    uint64_t *d_counters;
} hsa_junction_text_batch_t;
int hsa_junction_text_device(hsa_index_t *ix, const hsa_junction_text_batch_t *b, void *stream);

/* ---- FASTQ bytes to a search batch ----
 * bwa_read_seq (bwaseqio.c:161-231) over kseq_read (kseq.h:155-193), and the filter and
 * per-read options at the top of bwa_cal_sa_reg_gap (bwtaln.c:313-332), for the raw bytes of
 * a FASTQ chunk that sit in device memory: d_in[0] must be the first byte of a record.  The
 * call leaves on the device what the later calls take: d_jobs (off, len, max_diff, seed_len,
 * regime) and d_codes for hsa_search_device64 (zero-padded: 16 zero bytes follow the last
 * read), d_names / d_name_off and d_quals / d_qual_off for hsa_sam_lines_device64, and one row
 * per record.  No host round trip; launches on `stream` (NULL = the library's) and does
 * not synchronise; scratch grows on the handle (hsa_index_release_scratch).  Any index
 * serves: the handle gives the device, the stream and the scratch.
 *
 * Only canonical records are parsed (hsa_amd/csrc/hsa_reads.hip has the argument, with the
 * kseq.h lines it rests on): '@' and a non-empty name that ends at the first isspace byte
 * (the comment is dropped); a sequence line of 1..HSA_RD_MAX_LEN bytes, all isgraph and none
 * of '>', '+', '@'; a line that starts with '+'; a quality line of the sequence's length,
 * every byte in 33..127, ended by '\n' or, with at_eof, by the end of the input.  The first
 * record that is not canonical (a blank line, a sequence over several lines, CRLF, FASTA, a
 * quality of another length, an empty name, a read past HSA_RD_MAX_LEN or, with a table,
 * of n_maxdiff bases or more) stops the load: the records before it are loaded, [11] and [12]
 * name it, and the caller parses the bytes from [12] on the host (hsa_amd/reads.py:
 * parse_host).  With at_eof == 0 an incomplete last record is no error: [10] gives the bytes
 * consumed and the caller puts the rest in front of its next chunk.  At most max_records
 * (1..2^28) records are loaded; it sizes the scratch, so state the batch's size.
 *
 * Per record: codes through nst_nt4_table (bwaseqio.c:10-27; a '-' is stored as 5, which the
 * SAM call's base-code check refuses); the name loses a trailing "/1" or "/2" when longer
 * than two bytes (:217-220); max_diff is `max_diff`, or d_maxdiff[len] when d_maxdiff is
 * given (fnr > 0: bwa_cal_maxdiff(l) for l < n_maxdiff, computed on the host); seed_len =
 * seed_len < len ? seed_len : 0x7fffffff (bwtaln.c:332).  A read with more codes above 3 than
 * the batch's threshold is not searched (:314-317), nor one whose first 15 codes are all A
 * or all T (:324-325; a read under 15 bases never is, as bwtaln_gpu.c decides).  The threshold is
 * local_opt.max_diff before the option switch (:273-274): d_maxdiff[longest loaded read], or
 * max_diff.  A batch that arrives in several chunks states the longest read of its other chunks in
 * len_floor (under n_maxdiff): the table is then read at the longer of the two.  Kept reads are compacted in record order by a scan: two runs give equal arrays.
 *
 * d_rec: HSA_RD_ROW_WORDS u32 per record, max_records rows: status (HSA_RD_*), length, codes
 * above 3, job index (all-ones: not searched).  Rows of records not loaded are untouched.
 * d_name_off and d_qual_off hold job_cap + 1 entries.
 * d_counters (>= 16 u64, written by the call): [0] records seen (the loaded ones and
 * the one that stopped the load), [1] records loaded, [2] jobs
 * wanted, [3] written, [4] code bytes wanted (the 16 of padding included), [5] written, [6]
 * name bytes wanted, [7] written, [8] quality bytes wanted, [9] written, [10] bytes consumed,
 * [11] the first non-canonical record and [12] its byte offset (all-ones: none), [13] the
 * longest loaded read, [14] the longest kept read, [15] the threshold (as int64).  wanted >
 * written: run again with more room; no byte at or past a capacity is touched.
 *
 * hsa_reads_device takes none of the reader's options: trim_qual != 0, a barcode length, the
 * Casava, Illumina-1.3 or BAM bits of `mode` (gap_opt_t.mode as bwa_aln sets it) are HSA_E_ARG
 * there, as are null pointers and n_in >= 2^32 - 256.
 *
 * hsa_reads_device_opts is the same call with bwa_read_seq's options, applied per canonical
 * record in its order (bwaseqio.c:176-211):
 *   -Y  (mode & 0x08) the record is skipped when its comment (the header line behind the
 *       name's white space) is not empty, holds a ':' before any NUL, and the byte after the
 *       first ':' is 'Y';
 *   -I  (mode & 0x200) 31 comes off every quality byte; the bytes are validated as given
 *       (33..127) and stored shifted;
 *   -B n (mode >> 24, at most 63) a record of n bases or fewer is skipped; the first n bases
 *       go to d_bc (n bytes per job: lower case where the shifted quality - 33 is under 13,
 *       else upper case) and sequence and quality lose them;
 *   -q  (trim_qual >= 1, at most 32 674: the walk's sum then fits 32 bits for a read of
 *       HSA_RD_MAX_LEN) bwa_trim_read (:92-103): hsa_job_t.len, the row's length, max_diff,
 *       seed_len, the codes above 3, the poly test, the threshold and [13] / [14] are of the
 *       trimmed read.  The stored read stays whole: hsa_job_t.off, d_qual_off and the
 *       wanted / written byte counts advance by the length before trimming, which d_full_len
 *       (one u32 per job) holds.  A read of 35 bases or fewer is never trimmed.
 * A skipped record gets a row of status HSA_RD_FILTERED (length and count 0) and no job, and does not count towards
 * max_records nor [1].  With -Y or -B the call looks at no more than rec_cap records
 * (0: max_records), the rows d_rec holds, and loads up to the max_records-th record it does not
 * skip; [0] counts the skipped ones too, [10] and [11] speak of records as the input holds them.
 * d_opt_counters (>= HSA_RD_OPT_COUNTERS u64, or NULL): [0] records loaded, the skipped ones
 * included (the rows written), [1] records skipped, [2] bases trimmed and [3] bases in all, over
 * the loaded records not skipped (the reference's "% bases are trimmed").  BAM input (mode &
 * 0x1e0) is hsa_bam_reads_device's: HSA_E_ARG here. */
#define HSA_RD_SEARCHED 0u
#define HSA_RD_NDROP    1u    /* more codes above 3 than the threshold */
#define HSA_RD_POLYAT   2u    /* the first 15 codes all A or all T */
#define HSA_RD_FILTERED 3u    /* skipped by the reader: the Casava filter, or not longer than the barcode */
#define HSA_RD_OPT_COUNTERS 4
#define HSA_RD_ROW_WORDS 4
#define HSA_RD_MAX_LEN  65535u
#define HSA_RD_TILE     4096u /* bytes of the input per block of the newline passes */
typedef struct {
    const uint8_t *d_in; uint64_t n_in;
    int32_t at_eof;
    uint32_t max_records;
    int32_t max_diff;                /* opt->max_diff (used without a table) */
    const int32_t *d_maxdiff; uint32_t n_maxdiff;
    uint32_t len_floor;              /* the longest read of the batch's other chunks, or 0 */
    int32_t seed_len;                /* opt->seed_len */
    int32_t regime;                  /* written to every job */
    int32_t trim_qual; uint32_t mode; /* opt->trim_qual, opt->mode: both 0 for hsa_reads_device (its search bits aside) */
    hsa_job_t *d_jobs; uint64_t job_cap;
    uint8_t *d_codes; uint64_t code_cap;
    uint8_t *d_names; uint64_t name_cap; uint64_t *d_name_off;
    uint8_t *d_quals; uint64_t qual_cap; uint64_t *d_qual_off;
    uint32_t *d_rec;
    uint64_t *d_counters;            /* >= 16 u64 */
    /* the reader's options; 0 / NULL: none */
    uint32_t *d_full_len;            /* job_cap u32: a read's length before trimming (needed with trim_qual >= 1) */
    uint8_t *d_bc;                   /* job_cap * (mode >> 24) bytes: the barcodes (needed with a barcode) */
    uint32_t rec_cap;                /* the rows of d_rec when -Y or -B is set; 0: max_records */
    uint64_t *d_opt_counters;        /* >= HSA_RD_OPT_COUNTERS u64, or NULL */
} hsa_reads_batch_t;
int hsa_reads_device(hsa_index_t *ix, const hsa_reads_batch_t *b, void *stream);
int hsa_reads_device_opts(hsa_index_t *ix, const hsa_reads_batch_t *b, void *stream);
/* Probes, as hsa_sam_timing / hsa_sam_launch_times: the HSA_RD_LAUNCHES times in ms of the
 * handle's last timed call: k_rd_count (with the memsets), the tile scan, k_rd_lines,
 * k_rd_record, k_rd_max with k_rd_keep (and, with -Y or -B, the scan of the kept records and
 * k_rd_limit before them), the record scan, k_rd_rows, k_rd_bytes. */
#define HSA_RD_LAUNCHES 8
void hsa_reads_timing(int on);
int hsa_reads_launch_times(hsa_index_t *ix, float *ms);

/* ---- FASTA bytes to the packed texts and the annotation tables ----
 * HSPParseFASTAToPacked (HSP.c:180-343) and BuildReversePacked (2BWT-Builder.c:116-213) for
 * a whole FASTA whose bytes sit in device memory, with the grammar of
 * hsa_amd/index_build.py (_records, parse_fasta): a '>' starts a record; the name runs to
 * the first tab, space or newline, at most 256 bytes; the rest of the header line is
 * skipped; every later byte except '\n' up to the next '>' is sequence, a-z as A-Z; only A,
 * C, G, T are unambiguous ('\r' is not).  Records under 75 sequence bytes are dropped.  In a
 * kept record a run of fewer than 10 ambiguous bytes becomes 'G' and a longer one is
 * dropped: at the record's start it shifts the first block's ori, at its end it is cut,
 * inside it closes a block and opens the next; ori is the number within the record (the
 * ambiguous bytes counted, the newlines not) of the block's first character; an
 * all-ambiguous record keeps one block with end = start - 1; `total` sums the kept records'
 * lengths with their ambiguous bytes.
 *
 * Takes a device number, as the builders do: the call comes before any index exists.  With
 * no handle to grow scratch on, the caller passes d_scratch (256-byte aligned, at least
 * hsa_fasta_scratch_bytes(n_in): about 4 % of the input, nothing per byte).  Launches on
 * `stream` (NULL: the device's null stream) and does not synchronise; no host round trip
 * between the launches; output positions come from scans, never from atomics, so two runs
 * give equal arrays.
 *
 * Refused, not answered (the call still returns 0, [17] holds the lowest such offset and
 * the other outputs are of no use): a '>' inside a header line (its offset: the reference
 * skips to the line's end, _records starts a record), a last header line with no '\n'
 * before the end of the input (the offset of its '>'), an input that does not begin with
 * '>' (0).  Everything else parse_fasta accepts is answered exactly.
 *
 * Outputs (each with a capacity; no byte at or past a capacity is touched):
 *   d_pac    the .pac bytes (pac_bytes): 4 codes per byte, first in the high bits, a 0 byte
 *            when total % 4 == 0, the byte total % 4.  4-byte aligned.
 *   d_rpac   the .rev.pac bytes (reverse_pac): the forward text reversed, 1 to 4 bytes for a
 *            partial last word, a full last word lost when T % 16 == 0, the .pac's length
 *            byte.  4-byte aligned.
 *   d_text   the forward text as hsa_build_bwt_index_device takes it: LSB-first words of
 *            T = (.pac bytes - 2) * 4 + last byte characters (shorter than the kept characters
 *            or longer by up to three 'A's), then 8 zero words.  Capacity in words.
 *   d_rtext  the same for the .rev.pac's text of rT characters.
 *   d_rec    HSA_FA_REC_WORDS u32 per kept record: the name's offset in the input, its
 *            length, L, the record's first block.  Capacity in rows.
 *   d_blk    four u32 per block, in file order: kept record, start, end, ori.  Rows.
 * d_counters (HSA_FA_COUNTERS u64): [0] records seen, [1] kept (rows wanted), [2] rows
 * written, [3] blocks wanted, [4] written, [5] kept characters, [6] total, [7] T, [8] rT,
 * [9] .pac bytes wanted, [10] written, [11] .rev.pac bytes wanted, [12] written, [13] text
 * words wanted (the padding included), [14] written, [15] reversed text words wanted, [16]
 * written, [17] the refused offset (all-ones: none).  wanted > written: run again with
 * more room (a reversed text made from a forward text that was cut is of no use either).
 * An input without a kept unambiguous character has T = 0 (the host's pac_text fails on it).
 * Null pointers, a short scratch and n_in >= 2^32 - 256 are HSA_E_ARG. */
#define HSA_FA_REC_WORDS 4
#define HSA_FA_COUNTERS 18
typedef struct {
    const uint8_t *d_in; uint64_t n_in;
    uint8_t *d_pac; uint64_t pac_cap;
    uint8_t *d_rpac; uint64_t rpac_cap;
    uint32_t *d_text; uint64_t text_cap;
    uint32_t *d_rtext; uint64_t rtext_cap;
    uint32_t *d_rec; uint64_t rec_cap;
    uint32_t *d_blk; uint64_t blk_cap;
    uint64_t *d_counters;
    void *d_scratch; uint64_t scratch_bytes;
} hsa_fasta_batch_t;
int hsa_fasta_scratch_bytes(int device, uint64_t n_in, uint64_t *bytes);
int hsa_fasta_device(int device, const hsa_fasta_batch_t *b, void *stream);

/* The bodies of a .bwt and a .fmv file from the builder's output (d_bwt_lsb: the $-less BWT,
 * LSB-first, ceil(T/16) words; 1 <= T < 2^32 - 1): d_bwt_msb, ceil(T/16) words of 16 codes,
 * the first in the top bits, the tail past T cleared (index_io.pack_codes_msb); d_minor,
 * ((n_occ + 1) / 2) * 4 words, and d_major, ((n_occ + 255) / 256) * 4 words, exactly as
 * index_io.occ_files makes them: n_occ = (T + 255) / 256 + 1 samples, the zero padding past
 * T counted as 'A', 16-bit halves with the even sample in the high half, the last sample
 * repeated in the unread low half when n_occ is odd, a major sample every 65 536
 * characters.  d_scratch: 256-byte aligned, hsa_bwt_files_scratch_bytes(T).  Launches on
 * `stream`, does not synchronise. */
int hsa_bwt_files_scratch_bytes(int device, uint64_t T, uint64_t *bytes);
int hsa_bwt_files_device(int device, uint64_t T, const uint32_t *d_bwt_lsb, uint32_t *d_bwt_msb,
                         uint32_t *d_minor, uint32_t *d_major, void *d_scratch, uint64_t scratch_bytes,
                         void *stream);
/* Probes: with hsa_fasta_timing(1) both calls record events around their launches; the
 * times in ms of the last timed call (waits for it).  hsa_fasta_device: k_fa_marks (with
 * the memsets), the marks' scan, k_fa_spans, the two span scans, k_fa_count, the count scan,
 * k_fa_pack with k_fa_finish, k_fa_reverse.  hsa_bwt_files_device: k_bf_blocks, the scan,
 * k_bf_samples. */
#define HSA_FA_LAUNCHES 8
#define HSA_BF_LAUNCHES 3
void hsa_fasta_timing(int on);
int hsa_fasta_launch_times(float *ms);
int hsa_bwt_files_launch_times(float *ms);

/* ---- BGZF blocks to text ----
 * What gzread does for the reference's readers (bwaseqio.c:38, HSP.c:212) when the file is
 * BGZF, the blocked gzip `bgzip` writes: a series of independent gzip members of at most
 * 64 KB, each with its compressed size in the header and CRC32 and ISIZE in the trailer.
 * The caller walks the members on the host (hsa_amd/bgzf.py: scan) and passes the file's
 * bytes in device memory with one row per member; one wavefront inflates one member into
 * its own slice of d_out: all of DEFLATE (RFC 1951: stored, fixed and dynamic blocks, any
 * number per member), the CRC32 of the bytes computed on the device.
 *
 * d_status[i] is HSA_INF_OK only if the stream ended on a final block at the payload's last
 * byte, exactly isize bytes were written and their CRC32 is the row's; any other value names
 * the reason, and the slice of such a block is unspecified (the caller inflates it again on
 * the host, which decides whether the file is corrupt).  Every read is checked against the
 * payload's end and every write and back-reference against the block's slice before it is
 * made: a corrupt file ends as a status, and no byte outside [in_off, in_off + in_len) of
 * d_in and [out_off, out_off + isize) of d_out is touched for a block.  A row that lies
 * outside d_in or d_out is HSA_INF_E_ROW.  Rows' slices must not overlap.
 *
 * d_counters (HSA_INF_COUNTERS u64, added to: the caller zeroes them): [0] blocks with
 * status OK, [1] blocks refused, [2] bytes written by the OK blocks.  Takes a device
 * number, as hsa_fasta_device does: the FASTA reader calls it before any index exists.
 * Launches on `stream` (NULL: the null stream), does not synchronise, needs no scratch.
 * General gzip (one serial stream) is not built: it stays on the host. */
#define HSA_INF_OK        0u
#define HSA_INF_E_INPUT   1u   /* the payload ended inside the stream */
#define HSA_INF_E_BTYPE   2u   /* block type 3 */
#define HSA_INF_E_STORED  3u   /* a stored block's LEN is not ~NLEN */
#define HSA_INF_E_CODES   4u   /* an over-subscribed or unusable code-length set */
#define HSA_INF_E_SYMBOL  5u   /* a code no symbol has, or length symbol 286/287, distance symbol 30/31 */
#define HSA_INF_E_DIST    6u   /* a distance that reaches before the block's start */
#define HSA_INF_E_OUTPUT  7u   /* output past ISIZE */
#define HSA_INF_E_SIZE    8u   /* the stream ended with fewer than ISIZE bytes */
#define HSA_INF_E_CRC     9u   /* the bytes' CRC32 is not the trailer's */
#define HSA_INF_E_TRAIL   10u  /* payload bytes behind the final block */
#define HSA_INF_E_ROW     11u  /* the row's payload or slice lies outside the buffers */
#define HSA_INF_COUNTERS  3
typedef struct {
    uint64_t in_off;                 /* the deflate payload in d_in */
    uint32_t in_len;
    uint32_t isize;                  /* the trailer's ISIZE */
    uint64_t out_off;                /* the block's slice in d_out */
    uint32_t crc;                    /* the trailer's CRC32 */
    uint32_t reserved;
} hsa_bgzf_block_t;
typedef struct {
    const uint8_t *d_in; uint64_t n_in;
    const hsa_bgzf_block_t *d_blocks; uint64_t n_blocks;   /* under 2^31 */
    uint8_t *d_out; uint64_t out_cap;
    uint32_t *d_status;              /* n_blocks */
    uint64_t *d_counters;            /* HSA_INF_COUNTERS */
} hsa_inflate_batch_t;
int hsa_inflate_bgzf_device(int device, const hsa_inflate_batch_t *b, void *stream);

/* ---- BAM bytes to a search batch ----
 * bwa_read_bam (bwaseqio.c:105-157) for the inflated bytes of a BAM file in device memory,
 * with one departure: line 142, which reverses the read "to be reversed back in
 * bwa_refine_gapped", is not applied (the reverse-back is commented out in this reference,
 * bwtse.c:545).  A record then gives the read the FASTQ reader gives for the same bases, and
 * the call leaves exactly what hsa_reads_device_opts leaves: d_jobs, d_codes (16 zero bytes
 * behind the last read), names and qualities (always present) with their offsets, d_full_len,
 * the rows of d_rec (HSA_RD_SEARCHED / NDROP / POLYAT / FILTERED), d_counters [0..15] and
 * d_opt_counters in the same slots.  d_in[0] must be the first byte of a record (the header is
 * the caller's: hsa_amd/bam.py, read_header).
 *
 * Per record: taken when (which & 1 and FLAG 0x40) or (which & 2 and FLAG 0x80) or (which & 4
 * and neither), bwaseqio.c:118-121; nothing else in FLAG filters, secondary and supplementary
 * records are read.  A record not taken, and one with l_seq == 0, gets a row of status
 * HSA_RD_FILTERED and counts towards no batch.  Bases through bam_nt16_nt4_table (1, 2, 4, 8
 * are 0..3, all else 4), qualities q + 33 capped at 126 (0xFF gives '~'); with FLAG 0x10 the
 * codes are reverse-complemented and the qualities reversed before anything else looks at
 * them; trim_qual >= 1 trims with bwa_trim_read from the read's own end after that.  The name
 * is the l_read_name bytes up to the first NUL; no "/1" is cut.  Filter, max_diff, seed_len
 * and threshold as hsa_reads_device states them.
 *
 * Finding the records.  A record is block_size (u32) and that many bytes, so the starts form a
 * chain.  d_anchor holds n_anchor >= 1 ascending offsets: [0] must be 0, a true record start;
 * the others are offsets at which the caller expects a record to start (the first bytes of
 * BGZF members).  Segment i, [anchor i, anchor i + 1), is walked on its own; every hop is
 * checked before it is taken (l_read_name >= 1, block_size >= 32 + l_read_name + 4 n_cigar +
 * (l_seq + 1) / 2 + l_seq, the record ends inside the text), so a walk that began inside a
 * record looks at no byte outside the text and advances by 37 bytes or more per hop (the
 * staging loads whole aligned 16-byte units: up to 15 bytes before d_in and behind d_in + n_in,
 * inside the allocation's granule, are loaded and never looked at).  Segment i
 * is verified when its walk lands exactly on anchor i + 1, or, the last one, on the end of
 * the text (with or without at_eof: the text then ends at a record boundary).  By induction from anchor 0 the records of the longest verified prefix
 * are exact, and so is the walk of the first segment that is not verified (it began at a true
 * start); everything behind it is discarded and the load ends there (HSA_BAM_END_ANCHOR): the
 * caller goes on from [10] with a single anchor.  Anchors that do not ascend end the same way.
 *
 * The first record the device does not take (an empty name, a read over HSA_RD_MAX_LEN, or,
 * with a table, of n_maxdiff bases or more) stops the load as hsa_reads_device's first
 * non-canonical record does: [11] and [12] name it and its offset.  [10], the bytes consumed,
 * is always a true record start.  At most rec_cap records (0: max_records) are looked at,
 * the rows d_rec holds, and the load ends behind the max_records-th record that is a read.
 * d_bam_counters (HSA_BAM_COUNTERS u64): [0] why the load ended (HSA_BAM_END_*), [1] segments
 * verified, [2] records the exact walks found, [3] the offset at which they ended.
 * HSA_E_ARG: null pointers, n_anchor == 0, which outside 1..7, n_in >= 2^32 - 256, and what
 * hsa_reads_device_opts refuses of the arguments they share.  Scratch and timer are the
 * handle's, shared with hsa_reads_device. */
#define HSA_BAM_END_MAX        0u   /* max_records reads, or rec_cap records, loaded */
#define HSA_BAM_END_INPUT      1u   /* the end of the input */
#define HSA_BAM_END_INCOMPLETE 2u   /* an incomplete last record with at_eof == 0 */
#define HSA_BAM_END_ANCHOR     3u   /* an anchor is not on the chain */
#define HSA_BAM_END_HOST       4u   /* a record for the host: [11], [12] */
#define HSA_BAM_END_MALFORMED  5u   /* an inconsistent record, or with at_eof a truncated one, at [10] */
#define HSA_BAM_COUNTERS 4
typedef struct {
    const uint8_t *d_in; uint64_t n_in;
    int32_t at_eof;
    uint32_t max_records;
    uint32_t which;                  /* 1..7 */
    int32_t trim_qual;
    int32_t max_diff;
    const int32_t *d_maxdiff; uint32_t n_maxdiff;
    uint32_t len_floor;
    int32_t seed_len;
    int32_t regime;
    const uint64_t *d_anchor; uint32_t n_anchor;
    hsa_job_t *d_jobs; uint64_t job_cap;
    uint8_t *d_codes; uint64_t code_cap;
    uint8_t *d_names; uint64_t name_cap; uint64_t *d_name_off;
    uint8_t *d_quals; uint64_t qual_cap; uint64_t *d_qual_off;
    uint32_t *d_full_len;            /* job_cap u32 */
    uint32_t *d_rec; uint32_t rec_cap;
    uint64_t *d_counters;            /* >= 16 u64 */
    uint64_t *d_opt_counters;        /* >= HSA_RD_OPT_COUNTERS u64 */
    uint64_t *d_bam_counters;        /* >= HSA_BAM_COUNTERS u64 */
} hsa_bam_batch_t;
int hsa_bam_reads_device(hsa_index_t *ix, const hsa_bam_batch_t *b, void *stream);
/* The HSA_BAM_LAUNCHES times in ms of the handle's last timed call (hsa_bam_timing):
 * k_bam_walk (with the memsets), the segment scan, k_bam_starts, k_bam_record, k_bam_max
 * with k_bam_keep, the record scan, k_bam_rows, k_bam_bytes. */
#define HSA_BAM_LAUNCHES 8
void hsa_bam_timing(int on);
int hsa_bam_launch_times(hsa_index_t *ix, float *ms);

#ifdef __cplusplus
}
#endif
#endif
