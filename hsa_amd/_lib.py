"""ctypes binding of libhsa_gpu.so (the MI355X search core and its drop-in C ABI).

The library is built in-tree (hsa_amd/libhsa_gpu.so, `make -C hsa_amd/csrc`).
There is no fallback: if the library or a GPU is missing every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# HSA_GPU_LIB selects another in-tree build of the same library (A/B experiments).
LIB_PATH = os.path.join(HERE, os.environ.get("HSA_GPU_LIB", "libhsa_gpu.so"))

HSA_F_FALLBACK = 1
HSA_F_OVERFLOW = 2
HSA_RF_NFILTER = 0x10
HSA_RF_POLYAT = 0x20

EXPORTS = [  # every symbol include/hsa_gpu.h and include/hsa_bwtaln.h declare
    "hsa_device_count", "hsa_last_error", "hsa_index_create", "hsa_index_create_device", "hsa_index_free",
    "hsa_index_release_scratch",
    "hsa_index_bytes", "hsa_index_device", "hsa_occ4_batch", "hsa_step_batch", "hsa_width_batch",
    "hsa_search_batch", "hsa_search_device", "hsa_configure", "hsa_free", "hsa_synth_genome_device",
    "hsa_build_bwt_device", "bwa_cal_sa_reg_gap", "hsa_gpu_attach", "hsa_gpu_detach", "hsa_gpu_set_devices",
    "hsa_cal_sa_reg_gap_flat", "hsa_index_stream", "hsa_probe_gather", "hsa_last_pass_ms",
    "hsa_index_set_sa", "hsa_sa_position_batch", "hsa_sa_position_device", "hsa_match_gap_batch",
    "bwt_match_gap", "bwt_match_gap_batch", "hsa_splice_seeds_device", "hsa_pass_times",
    "hsa_cal_sa_reg_gap_multi", "hsa_index_create_device64", "hsa_index_is64", "hsa_occ4_batch64",
    "hsa_search_device64", "hsa_build_bwt_device64", "bwa_cal_pac_pos", "generate_sam_se_core",
    "hsa_build_bwt_index_device", "hsa_extend_batch", "bwt_extend_foreward", "bwt_extend_backward",
    "hsa_width0_batch", "bwt_cal_width", "hsa_extend_sliced", "hsa_index_trie",
    "hsa_index_clone", "hsa_splice_prefetch_batch", "hsa_index_set_text", "hsa_splice_match_batch",
    "hsa_splice_device", "hsa_build_bwt_index_device64", "hsa_index_set_sa64", "hsa_index_set_sa64_device",
    "hsa_sa_position_batch64", "hsa_sa_position_device64", "hsa_psi_minus_batch64", "hsa_hit_positions_device64",
    "hsa_index_set_text64_device", "hsa_refine_rows_device64", "hsa_choose_hits_device64",
    "hsa_choose_timing", "hsa_choose_launch_times", "hsa_sam_lines_device64", "hsa_sam_timing", "hsa_splice_lines_device", "hsa_sam_merge_device",
    "hsa_sam_launch_times", "hsa_index_levels", "hsa_reads_device", "hsa_reads_timing",
    "hsa_reads_launch_times", "hsa_reads_device_opts", "hsa_sam_lines_device64_trim", "hsa_splice_lines_device_trim", "hsa_splice_lines_device_xa", "hsa_fasta_scratch_bytes", "hsa_fasta_device", "hsa_bwt_files_scratch_bytes",
    "hsa_bwt_files_device", "hsa_fasta_timing", "hsa_fasta_launch_times", "hsa_bwt_files_launch_times",
    "hsa_inflate_bgzf_device", "hsa_bam_reads_device", "hsa_bam_timing", "hsa_bam_launch_times",
    "hsa_junction_rows_device", "hsa_junction_reduce_device", "hsa_junction_text_device",
]
SP_RES_WORDS = 20  # hsa_splice_match_batch's per-read answer (include/hsa_gpu.h)
ALN64_WORDS = 14   # hsa_aln64_t (include/hsa_gpu.h)
# hsa_refine_rows_device64 (include/hsa_gpu.h): per-row status, layout limits, words per row
HSA_RF_OK, HSA_RF_POS, HSA_RF_TEXT, HSA_RF_CAP, HSA_RF_MD = range(5)
HSA_RF_MAX_LEN = 4095
HSA_RF_MAX_GAP = 27
RF_ROW_WORDS = 8
# hsa_choose_hits_device64: glibc's drand48 state in a process that never seeds; read types
DRAND48_SEED0 = 0
CHOOSE_NONE, CHOOSE_UNIQUE, CHOOSE_REPEAT = range(3)
# hsa_sam_lines_device64: per-read status, the longest line a batch may declare
HSA_SAM_OK, HSA_SAM_NOHIT, HSA_SAM_ROWS, HSA_SAM_REFINE, HSA_SAM_INPUT = range(5)
HSA_SAM_MAX_LINE = 61440
# hsa_splice_lines_device: per-read status, words per read row, the most score buckets of hsa_splice_device
(HSA_SL_OK, HSA_SL_NONE, HSA_SL_HANDED, HSA_SL_NOPAIR, HSA_SL_MULTI, HSA_SL_REFINE, HSA_SL_POS, HSA_SL_INTRON,
 HSA_SL_INPUT) = range(9)
SL_ROW_WORDS = 24
SL_XA_WORDS = 16               # words per extra pair of hsa_splice_lines_device_xa
HSA_SL_XA_UNUSED = 0xFFFFFFFF
# the junction table's row buffers: words per row (chrID, first base, last base, lines without an XA list, lines with
# one, overhang, motif, 0)
JN_ROW_WORDS = 8
HSA_SP_MAX_STACKS = 128
# hsa_reads_device: per-record status, words per record row, the longest read, the bytes of
# the input per block of the newline passes, the counters
HSA_RD_SEARCHED, HSA_RD_NDROP, HSA_RD_POLYAT, HSA_RD_FILTERED = range(4)
RD_OPT_COUNTERS = ("rows", "filtered", "trimmed_bases", "total_bases")       # hsa_reads_device_opts' d_opt_counters
RD_ROW_WORDS = 4
HSA_RD_MAX_LEN = 65535
HSA_RD_TILE = 4096
RD_COUNTERS = ("seen", "loaded", "jobs_wanted", "jobs_written", "code_wanted", "code_written", "name_wanted",
               "name_written", "qual_wanted", "qual_written", "consumed", "bad_record", "bad_offset", "max_loaded",
               "max_kept", "threshold")
# hsa_bam_reads_device: why the load ended (d_bam_counters[0]), the BAM counters, the launches
(HSA_BAM_END_MAX, HSA_BAM_END_INPUT, HSA_BAM_END_INCOMPLETE, HSA_BAM_END_ANCHOR, HSA_BAM_END_HOST,
 HSA_BAM_END_MALFORMED) = range(6)
BAM_COUNTERS = ("reason", "segments_verified", "chain_records", "chain_end")
BAM_LAUNCHES = ("walk", "segment_scan", "starts", "record", "max_keep", "record_scan", "rows", "bytes")
# hsa_fasta_device: words per record row, the counters, the zero words behind a text
FA_REC_WORDS = 4
FA_COUNTERS = ("seen", "kept", "rec_written", "blocks", "blk_written", "characters", "total", "T", "rev_T",
               "pac_wanted", "pac_written", "rpac_wanted", "rpac_written", "text_wanted", "text_written",
               "rtext_wanted", "rtext_written", "refused")
FA_PAD_WORDS = 8
FA_LAUNCHES = ("marks", "marks_scan", "spans", "span_scans", "count", "count_scan", "pack", "reverse")
BF_LAUNCHES = ("blocks", "scan", "samples")
# hsa_inflate_bgzf_device: per-block status, the counters, a row of the block table (hsa_bgzf_block_t)
(HSA_INF_OK, HSA_INF_E_INPUT, HSA_INF_E_BTYPE, HSA_INF_E_STORED, HSA_INF_E_CODES, HSA_INF_E_SYMBOL, HSA_INF_E_DIST,
 HSA_INF_E_OUTPUT, HSA_INF_E_SIZE, HSA_INF_E_CRC, HSA_INF_E_TRAIL, HSA_INF_E_ROW) = range(12)
INF_COUNTERS = ("done", "refused", "bytes")
BGZF_BLOCK_DTYPE = np.dtype([("in_off", "<u8"), ("in_len", "<u4"), ("isize", "<u4"), ("out_off", "<u8"), ("crc", "<u4"),
                             ("reserved", "<u4")])


class HsaError(RuntimeError):
    pass


CODES_PAD = 16   # hsa_search_device reads a read's codes in aligned 16-byte loads


def pad_codes(codes) -> np.ndarray:
    """Read codes followed by the padding the device path may read past the last
    read (include/hsa_gpu.h, hsa_device_batch_t.d_codes)."""
    c = np.ascontiguousarray(codes, np.uint8).reshape(-1)
    return np.concatenate([c, np.zeros(4 * CODES_PAD, np.uint8)])


class GapOpt(C.Structure):
    """gap_opt_t (bwtaln.h:133-143)."""
    _fields_ = [("s_mm", C.c_int), ("s_gapo", C.c_int), ("s_gape", C.c_int), ("mode", C.c_int),
                ("indel_end_skip", C.c_int), ("max_del_occ", C.c_int), ("max_entries", C.c_int),
                ("fnr", C.c_float), ("max_diff", C.c_int), ("max_gapo", C.c_int), ("max_gape", C.c_int),
                ("max_seed_diff", C.c_int), ("seed_len", C.c_int), ("n_threads", C.c_int),
                ("max_top2", C.c_int), ("trim_qual", C.c_int)]

    @classmethod
    def default(cls):
        """gap_init_opt (bwtaln.c:21-44)."""
        return cls(s_mm=3, s_gapo=11, s_gape=4, mode=0x03, indel_end_skip=5, max_del_occ=10,
                   max_entries=2000000, fnr=0.04, max_diff=-1, max_gapo=1, max_gape=6,
                   max_seed_diff=2, seed_len=32, n_threads=1, max_top2=30, trim_qual=0)

    @classmethod
    def from_dict(cls, d):
        o = cls()
        for k, _ in cls._fields_:
            setattr(o, k, d[k])
        return o

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Regime(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("s_mm", "s_gapo", "s_gape", "mode", "indel_end_skip", "max_del_occ",
                                         "max_entries", "max_gapo", "max_gape", "max_seed_diff", "max_top2",
                                         "n_stacks", "max_diff")]


JOB_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("max_diff", "<i4"), ("seed_len", "<i4"),
                      ("regime", "<i4")])
# hsa_mg_job_t (include/hsa_gpu.h): one direct bwt_match_gap call's widths and strand
MG_DTYPE = np.dtype([("wb_off", "<u8"), ("ws_off", "<u8"), ("strand", "<i4"), ("seed", "<i4")])
SEED_NONE, SEED_OWN, SEED_ALIAS = 0, 1, 2
# hsa_ext_job_t (include/hsa_gpu.h): one seed extension of the splice path
EXT_DTYPE = np.dtype([("dir", "<i4"), ("len", "<i4"), ("max_pos", "<i4"), ("regime", "<i4"), ("lo", "<i4"),
                      ("n", "<i4"), ("off", "<u8"), ("aln", "<u4", (9,)), ("pad", "<u4")])
assert EXT_DTYPE.itemsize == 72


def regime_of(opt: dict, n_stacks: int, max_diff: int) -> "Regime":
    """The fields of one option block bwt_match_gap reads (bwtaln_gpu.c hsa_regime_of)."""
    mode = opt["mode"] & (0x01 | 0x04 | 0x10)
    if opt["max_gapo"] == 0:
        mode &= ~(0x01 | 0x04)
    return Regime(s_mm=opt["s_mm"], s_gapo=opt["s_gapo"], s_gape=opt["s_gape"], mode=mode,
                  indel_end_skip=opt["indel_end_skip"], max_del_occ=opt["max_del_occ"],
                  max_entries=opt["max_entries"], max_gapo=opt["max_gapo"], max_gape=opt["max_gape"],
                  max_seed_diff=opt["max_seed_diff"], max_top2=opt["max_top2"], n_stacks=n_stacks,
                  max_diff=max_diff)


class Stats(C.Structure):
    _fields_ = [("rank_queries", C.c_uint64), ("blocks_loaded", C.c_uint64), ("pops", C.c_uint64),
                ("overflow_reruns", C.c_uint64), ("kernel_ms", C.c_double), ("main_kernel_ms", C.c_double),
                ("main_launches", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DeviceBatch(C.Structure):
    _fields_ = [("d_jobs", C.c_void_p), ("n_jobs", C.c_int), ("d_codes", C.c_void_p), ("d_n_aln", C.c_void_p),
                ("d_flags", C.c_void_p), ("d_hit_off", C.c_void_p), ("d_hits", C.c_void_p),
                ("hit_cap", C.c_uint64), ("d_counters", C.c_void_p), ("max_len", C.c_int32),
                ("max_seed", C.c_int32)]


class HitPosBatch64(C.Structure):
    """hsa_hitpos_batch64_t (include/hsa_gpu.h): the hit lists of hsa_search_device64 to
    positions, all device pointers."""
    _fields_ = [("d_n_aln", C.c_void_p), ("d_hit_off", C.c_void_p), ("d_hits", C.c_void_p), ("n_jobs", C.c_int),
                ("max_occ", C.c_uint32), ("d_pos_off", C.c_void_p), ("d_pos", C.c_void_p), ("d_pos_hit", C.c_void_p),
                ("pos_cap", C.c_uint64), ("d_counters", C.c_void_p)]


class RefineBatch64(C.Structure):
    """hsa_refine_batch64_t (include/hsa_gpu.h): the search batch and the position call's
    outputs in, CIGAR / NM / MD per position row out, all device pointers."""
    _fields_ = [("d_jobs", C.c_void_p), ("n_jobs", C.c_int), ("d_codes", C.c_void_p), ("d_hit_off", C.c_void_p),
                ("d_hits", C.c_void_p), ("d_pos_off", C.c_void_p), ("d_pos", C.c_void_p), ("d_pos_hit", C.c_void_p),
                ("pos_cap", C.c_uint64), ("d_pos_counters", C.c_void_p), ("max_len", C.c_int32),
                ("cigar_stride", C.c_uint32), ("md_stride", C.c_uint32), ("d_rows", C.c_void_p),
                ("d_rpos", C.c_void_p), ("d_cigar", C.c_void_p), ("d_md", C.c_void_p), ("d_counters", C.c_void_p)]


class ChooseBatch64(C.Structure):
    """hsa_choose_batch64_t (include/hsa_gpu.h): the search's hit lists in; each read's
    chosen record, SA row, mapQ, X0 / X1 and generator state, and the chosen and XA rows in
    hit_positions64's layout out, all device pointers."""
    _fields_ = [("d_jobs", C.c_void_p), ("n_jobs", C.c_int), ("d_n_aln", C.c_void_p), ("d_hit_off", C.c_void_p),
                ("d_hits", C.c_void_p), ("n_multi", C.c_uint32), ("rng_state", C.c_uint64), ("d_log_n", C.c_void_p),
                ("d_sel", C.c_void_p), ("d_sel64", C.c_void_p), ("d_rng_out", C.c_void_p), ("d_pos_off", C.c_void_p),
                ("d_pos", C.c_void_p), ("d_pos_hit", C.c_void_p), ("pos_cap", C.c_uint64), ("d_counters", C.c_void_p)]


class SamBatch64(C.Structure):
    """hsa_sam_batch64_t (include/hsa_gpu.h): the device outputs of search, choose and
    refine and the reads' names and qualities in; the SAM text, its per-read offsets and
    statuses out, all device pointers."""
    _fields_ = [("d_jobs", C.c_void_p), ("n_jobs", C.c_int), ("d_codes", C.c_void_p), ("d_n_aln", C.c_void_p),
                ("d_hit_off", C.c_void_p), ("d_hits", C.c_void_p), ("d_sel", C.c_void_p), ("d_sel64", C.c_void_p),
                ("d_pos_off", C.c_void_p), ("d_pos", C.c_void_p), ("d_pos_hit", C.c_void_p), ("pos_cap", C.c_uint64),
                ("d_pos_counters", C.c_void_p), ("d_rows", C.c_void_p), ("d_rpos", C.c_void_p), ("d_cigar", C.c_void_p),
                ("d_md", C.c_void_p), ("cigar_stride", C.c_uint32), ("md_stride", C.c_uint32), ("d_names", C.c_void_p),
                ("d_name_off", C.c_void_p), ("d_quals", C.c_void_p), ("d_qual_off", C.c_void_p),
                ("d_chr_names", C.c_void_p), ("d_chr_off", C.c_void_p), ("n_chr", C.c_uint32), ("flag", C.c_uint32),
                ("max_top2", C.c_int32), ("comp_read", C.c_int32), ("max_line", C.c_uint32), ("d_line_off", C.c_void_p),
                ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_line_stat", C.c_void_p), ("d_counters", C.c_void_p)]


class SamTrim(C.Structure):
    """hsa_sam_trim_t (include/hsa_gpu.h): the reads' stored lengths and barcodes for the two
    line writers, device pointers."""
    _fields_ = [("d_full_len", C.c_void_p), ("d_bc", C.c_void_p), ("bc_len", C.c_uint32)]


class SpliceLinesBatch(C.Structure):
    """hsa_splice_lines_batch_t (include/hsa_gpu.h): the batch, hsa_splice_device's results and
    the reads' names and qualities in; the spliced reads' SAM text, its per-read offsets,
    statuses and row words out, all device pointers."""
    _fields_ = [("d_jobs", C.c_void_p), ("n_jobs", C.c_int), ("d_codes", C.c_void_p), ("d_flags", C.c_void_p),
                ("d_n_aln", C.c_void_p), ("d_res", C.c_void_p), ("d_names", C.c_void_p), ("d_name_off", C.c_void_p),
                ("d_quals", C.c_void_p), ("d_qual_off", C.c_void_p), ("d_chr_names", C.c_void_p), ("d_chr_off", C.c_void_p),
                ("n_chr", C.c_uint32), ("flag", C.c_uint32), ("max_top2", C.c_int32), ("comp_read", C.c_int32),
                ("max_len", C.c_int32), ("max_line", C.c_uint32), ("cigar_stride", C.c_uint32), ("pad", C.c_uint32),
                ("d_rows", C.c_void_p), ("d_cigar", C.c_void_p), ("d_line_off", C.c_void_p), ("d_out", C.c_void_p),
                ("out_cap", C.c_uint64), ("d_line_stat", C.c_void_p), ("d_counters", C.c_void_p)]


class SpliceXa(C.Structure):
    """hsa_splice_xa_t (include/hsa_gpu.h): the room for the extra splice pairs of reads with
    several pairs (their XA:Z entries), the pairs' offsets, rows and merged CIGARs and the
    list counters out, all device pointers."""
    _fields_ = [("pair_cap", C.c_uint64), ("d_pair_off", C.c_void_p), ("d_pair_rows", C.c_void_p), ("d_pair_cigar", C.c_void_p),
                ("d_counters", C.c_void_p)]


class JunctionRowsBatch(C.Structure):
    """hsa_junction_rows_batch_t (include/hsa_gpu.h): one lines call's rows, CIGARs and statuses
    in; junction rows appended to a row buffer, all device pointers."""
    _fields_ = [("n_jobs", C.c_int), ("cigar_stride", C.c_uint32), ("d_rows", C.c_void_p), ("d_cigar", C.c_void_p),
                ("d_line_stat", C.c_void_p), ("d_jrows", C.c_void_p), ("n_have", C.c_uint64), ("row_cap", C.c_uint64),
                ("d_counters", C.c_void_p)]


class JunctionReduceBatch(C.Structure):
    """hsa_junction_reduce_batch_t (include/hsa_gpu.h): a row buffer sorted and merged in place."""
    _fields_ = [("d_jrows", C.c_void_p), ("n_rows", C.c_uint64), ("d_counters", C.c_void_p)]


class JunctionTextBatch(C.Structure):
    """hsa_junction_text_batch_t (include/hsa_gpu.h): a reduced table and the chromosome names
    in; the table's text and its per-row offsets out, all device pointers."""
    _fields_ = [("d_jrows", C.c_void_p), ("n_rows", C.c_uint64), ("d_chr_names", C.c_void_p), ("d_chr_off", C.c_void_p),
                ("n_chr", C.c_uint32), ("pad", C.c_uint32), ("d_line_off", C.c_void_p), ("d_out", C.c_void_p),
                ("out_cap", C.c_uint64), ("d_counters", C.c_void_p)]


class SamMergeBatch(C.Structure):
    """hsa_sam_merge_batch_t (include/hsa_gpu.h): two writers' texts and offsets over the same
    reads in, one text in read order out, all device pointers."""
    _fields_ = [("n_jobs", C.c_int), ("d_line_off_a", C.c_void_p), ("d_text_a", C.c_void_p), ("text_a_len", C.c_uint64),
                ("d_line_off_b", C.c_void_p), ("d_text_b", C.c_void_p), ("text_b_len", C.c_uint64), ("d_line_off", C.c_void_p),
                ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_counters", C.c_void_p)]


class ReadsBatch(C.Structure):
    """hsa_reads_batch_t (include/hsa_gpu.h): the bytes of a FASTQ chunk in; the search
    batch (jobs, codes), the names and qualities in hsa_sam_lines_device64's layout, a row
    per record and the counters out, all device pointers."""
    _fields_ = [("d_in", C.c_void_p), ("n_in", C.c_uint64), ("at_eof", C.c_int32), ("max_records", C.c_uint32),
                ("max_diff", C.c_int32), ("d_maxdiff", C.c_void_p), ("n_maxdiff", C.c_uint32), ("len_floor", C.c_uint32),
                ("seed_len", C.c_int32),
                ("regime", C.c_int32), ("trim_qual", C.c_int32), ("mode", C.c_uint32), ("d_jobs", C.c_void_p),
                ("job_cap", C.c_uint64), ("d_codes", C.c_void_p), ("code_cap", C.c_uint64), ("d_names", C.c_void_p),
                ("name_cap", C.c_uint64), ("d_name_off", C.c_void_p), ("d_quals", C.c_void_p), ("qual_cap", C.c_uint64),
                ("d_qual_off", C.c_void_p), ("d_rec", C.c_void_p), ("d_counters", C.c_void_p),
                ("d_full_len", C.c_void_p), ("d_bc", C.c_void_p), ("rec_cap", C.c_uint32), ("d_opt_counters", C.c_void_p)]


class BamBatch(C.Structure):
    """hsa_bam_batch_t (include/hsa_gpu.h): the inflated bytes of a BAM file from a record start
    on and the anchors in; ReadsBatch's outputs and the BAM counters out, all device pointers."""
    _fields_ = [("d_in", C.c_void_p), ("n_in", C.c_uint64), ("at_eof", C.c_int32), ("max_records", C.c_uint32),
                ("which", C.c_uint32), ("trim_qual", C.c_int32), ("max_diff", C.c_int32), ("d_maxdiff", C.c_void_p),
                ("n_maxdiff", C.c_uint32), ("len_floor", C.c_uint32), ("seed_len", C.c_int32), ("regime", C.c_int32),
                ("d_anchor", C.c_void_p), ("n_anchor", C.c_uint32), ("d_jobs", C.c_void_p), ("job_cap", C.c_uint64),
                ("d_codes", C.c_void_p), ("code_cap", C.c_uint64), ("d_names", C.c_void_p), ("name_cap", C.c_uint64),
                ("d_name_off", C.c_void_p), ("d_quals", C.c_void_p), ("qual_cap", C.c_uint64), ("d_qual_off", C.c_void_p),
                ("d_full_len", C.c_void_p), ("d_rec", C.c_void_p), ("rec_cap", C.c_uint32), ("d_counters", C.c_void_p),
                ("d_opt_counters", C.c_void_p), ("d_bam_counters", C.c_void_p)]


class FastaBatch(C.Structure):
    """hsa_fasta_batch_t (include/hsa_gpu.h): the bytes of a FASTA in; the .pac and .rev.pac
    bytes, the two texts, the record and block tables and the counters out, each with its
    capacity; the caller's scratch.  All device pointers."""
    _fields_ = [("d_in", C.c_void_p), ("n_in", C.c_uint64), ("d_pac", C.c_void_p), ("pac_cap", C.c_uint64),
                ("d_rpac", C.c_void_p), ("rpac_cap", C.c_uint64), ("d_text", C.c_void_p), ("text_cap", C.c_uint64),
                ("d_rtext", C.c_void_p), ("rtext_cap", C.c_uint64), ("d_rec", C.c_void_p), ("rec_cap", C.c_uint64),
                ("d_blk", C.c_void_p), ("blk_cap", C.c_uint64), ("d_counters", C.c_void_p),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)]


class InflateBatch(C.Structure):
    """hsa_inflate_batch_t (include/hsa_gpu.h): the bytes of a BGZF file and its block table
    in; the text, a status per block and the counters out.  All device pointers."""
    _fields_ = [("d_in", C.c_void_p), ("n_in", C.c_uint64), ("d_blocks", C.c_void_p), ("n_blocks", C.c_uint64),
                ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_status", C.c_void_p), ("d_counters", C.c_void_p)]


def inflate_bgzf_device(batch: "InflateBatch", device: int = 0, stream=None):
    """hsa_inflate_bgzf_device: the BGZF blocks of batch.d_blocks, one wavefront each, into
    their slices of batch.d_out; queued on `stream` (an int handle; None: the null stream)."""
    if not hasattr(lib(), "hsa_inflate_bgzf_device"):
        raise HsaError("this libhsa_gpu.so has no hsa_inflate_bgzf_device: rebuild it")
    check(lib().hsa_inflate_bgzf_device(int(device), C.byref(batch), stream))


def log_n_table() -> np.ndarray:
    """g_log_n (bwtse.c:838-842): (int)(4.343 * log(i) + 0.5) for i = 1..255, [0] = 0."""
    import math
    return np.array([0] + [int(4.343 * math.log(i) + 0.5) for i in range(1, 256)], np.int32)


class SeedBatch(C.Structure):
    """hsa_seed_batch_t (include/hsa_gpu.h): the splice seeds of a device batch."""
    _fields_ = [("d_jobs", C.c_void_p), ("n_jobs", C.c_int), ("d_codes", C.c_void_p), ("d_flags", C.c_void_p),
                ("d_n_aln", C.c_void_p), ("d_hit_off", C.c_void_p), ("d_hits", C.c_void_p), ("hit_cap", C.c_uint64),
                ("d_counters", C.c_void_p), ("max_len", C.c_int32)]


class SplicePf(C.Structure):
    """hsa_splice_pf_t (include/hsa_gpu.h): the splice prefetch's outputs."""
    _fields_ = [("n", C.c_int), ("max_len", C.c_int), ("row_stride", C.c_int), ("cw_stride", C.c_int),
                ("rows", C.c_void_p), ("call_n", C.c_void_p), ("call_hit", C.c_void_p), ("hits", C.c_void_p),
                ("wafter", C.c_void_p), ("call_sa", C.c_void_p), ("sa", C.c_void_p), ("n_hits", C.c_uint64),
                ("n_sa", C.c_uint64), ("kernel_ms", C.c_double)]


class SpliceBatch(C.Structure):
    """hsa_splice_batch_t (include/hsa_gpu.h): the splice path of a device batch."""
    _fields_ = [("d_jobs", C.c_void_p), ("n_jobs", C.c_int), ("d_codes", C.c_void_p), ("d_flags", C.c_void_p),
                ("d_n_aln", C.c_void_p), ("d_res", C.c_void_p), ("d_counters", C.c_void_p), ("max_len", C.c_int32)]


def ext_regime(local_opt: dict, n_stacks: int, max_diff: int) -> "Regime":
    """The splice path's extension regime (aux_ext: local_opt with max_gape 3,
    bwtgap.c:776-782); GAPE / LOGGAP as the extension reads them, whatever max_gapo."""
    ao = dict(local_opt, max_gape=3)
    r = regime_of(ao, n_stacks, max_diff)
    r.mode = ao["mode"] & (0x01 | 0x04 | 0x10)
    return r


def anchor_regime(local_opt: dict, n_stacks: int, max_diff: int) -> "Regime":
    """The 12-mer anchors' regime (aux_ext's options, bwt_match_gap with width_seed NULL)."""
    return regime_of(dict(local_opt, max_gape=3), n_stacks, max_diff)


class SpliceStats(C.Structure):
    """hsa_splice_stats_t (include/hsa_gpu.h)."""
    _fields_ = [("kernel_ms", C.c_double), ("extensions", C.c_uint64), ("pops", C.c_uint64),
                ("sa_lookups", C.c_uint64), ("not_answered", C.c_uint64)]


_lib = None


def _check_runtime():
    """libhsa_gpu.so is built against /opt/rocm's HIP runtime.  PyTorch-ROCm bundles
    an older HIP/HSA runtime with the same sonames; whichever is loaded first serves
    both.  With torch's loaded first the library sees no device, so the package must
    be imported before torch (hsa_amd/__init__.py loads the library eagerly)."""
    try:
        maps = open("/proc/self/maps").read()
    except OSError:
        return
    hip = {ln.split()[-1] for ln in maps.splitlines() if "libamdhip64" in ln}
    if any("/torch/lib/" in h for h in hip):
        raise HsaError("the HIP runtime bundled with torch was loaded before libhsa_gpu.so: "
                       "import hsa_amd before importing torch")


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HsaError(f"{LIB_PATH} is missing: build it with `make -C hsa_amd/csrc` (no CPU fallback exists)")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    _check_runtime()
    u32 = np.ctypeslib.ndpointer(np.uint32, flags="C")
    u64 = np.ctypeslib.ndpointer(np.uint64, flags="C")
    i32 = np.ctypeslib.ndpointer(np.int32, flags="C")
    u8 = np.ctypeslib.ndpointer(np.uint8, flags="C")
    vp = C.c_void_p
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    L.hsa_device_count.restype = C.c_int
    L.hsa_last_error.restype = C.c_char_p
    L.hsa_index_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, u32, u32, C.c_uint32, C.c_uint32, u32, u32,
                                   C.POINTER(vp)]
    L.hsa_index_create_device.argtypes = [C.c_int, C.c_uint32, C.c_uint32, u32, vp, C.c_uint32, C.c_uint32, u32, vp,
                                          C.POINTER(vp)]
    L.hsa_index_free.argtypes = [vp]
    L.hsa_index_release_scratch.argtypes = [vp]
    L.hsa_index_bytes.restype = C.c_size_t
    L.hsa_index_bytes.argtypes = [vp]
    L.hsa_index_trie.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "hsa_index_levels"):              # (older A/B builds lack it)
        L.hsa_index_levels.argtypes = [vp, C.c_void_p, C.c_void_p]
    L.hsa_index_clone.argtypes = [vp, C.POINTER(vp)]
    L.hsa_index_stream.restype = vp
    L.hsa_index_stream.argtypes = [vp]
    L.hsa_occ4_batch.argtypes = [vp, C.c_int, C.c_size_t, u32, u32]
    L.hsa_step_batch.argtypes = [vp, C.c_size_t, u32, u32]
    L.hsa_width_batch.argtypes = [vp, C.c_size_t, u64, u32, u8, C.c_size_t, u32]
    if hasattr(L, "hsa_width0_batch"):
        L.hsa_width0_batch.argtypes = [vp, C.c_size_t, u64, u32, u8, C.c_size_t, u32]
    L.hsa_search_batch.restype = C.c_long
    L.hsa_search_batch.argtypes = [vp, C.POINTER(Regime), C.c_int, vp, C.c_int, u8, C.c_size_t, i32, u32, u64,
                                   C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(Stats)]
    L.hsa_search_device.argtypes = [vp, C.POINTER(Regime), C.c_int, C.POINTER(DeviceBatch), vp]
    L.hsa_configure.argtypes = [C.c_int, C.c_int, C.c_int]
    L.hsa_free.argtypes = [vp]
    L.hsa_synth_genome_device.argtypes = [C.c_int, C.c_uint64, C.c_uint64, vp]
    L.hsa_index_set_sa.argtypes = [vp, u32, C.c_uint64, C.c_uint32, u32, C.c_int]
    L.hsa_sa_position_batch.argtypes = [vp, C.c_size_t, u32, u32]
    L.hsa_probe_gather.argtypes = [C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_double)]
    L.hsa_build_bwt_device.argtypes = [C.c_int, C.c_uint64, vp, C.c_int, vp, C.POINTER(C.c_uint32), u32]
    L.hsa_match_gap_batch.restype = C.c_long
    L.hsa_match_gap_batch.argtypes = [vp, C.POINTER(Regime), C.c_int, vp, vp, C.c_int, u8, C.c_size_t, i32, C.c_size_t,
                                      i32, i32, u64, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(Stats)]
    L.hsa_splice_seeds_device.argtypes = [vp, C.POINTER(Regime), C.POINTER(SeedBatch), vp]
    if hasattr(L, "hsa_splice_prefetch_batch"):
        L.hsa_splice_prefetch_batch.argtypes = [vp, C.POINTER(Regime), C.POINTER(Regime), C.c_int, u32, u64, u8,
                                                C.c_size_t, i32, C.POINTER(SplicePf)]
    if hasattr(L, "hsa_splice_device"):
        L.hsa_splice_device.argtypes = [vp, C.POINTER(Regime), C.POINTER(Regime), C.POINTER(Regime),
                                        C.POINTER(SpliceBatch), vp]
    if hasattr(L, "hsa_splice_match_batch"):
        L.hsa_index_set_text.argtypes = [vp, u32, C.c_uint64, C.c_uint32]
        L.hsa_splice_match_batch.argtypes = [vp, C.POINTER(Regime), C.POINTER(Regime), C.POINTER(Regime), C.c_int, u32,
                                             u64, u8, C.c_size_t, i32, C.POINTER(SplicePf), u32,
                                             C.POINTER(SpliceStats)]
    if hasattr(L, "hsa_search_device64"):           # (older A/B builds lack the 64-bit path)
        L.hsa_index_create_device64.argtypes = [C.c_int, C.c_uint64, C.c_uint64, u64, vp, C.c_uint64, C.c_uint64,
                                                u64, vp, C.POINTER(vp)]
        L.hsa_index_is64.argtypes = [vp]
        L.hsa_occ4_batch64.argtypes = [vp, C.c_int, C.c_size_t, u64, u64]
        L.hsa_search_device64.argtypes = [vp, C.POINTER(Regime), C.c_int, C.POINTER(DeviceBatch), vp]
        L.hsa_build_bwt_device64.argtypes = [C.c_int, C.c_uint64, vp, C.c_int, vp, C.POINTER(C.c_uint64), u64]
    if hasattr(L, "hsa_build_bwt_index_device"):
        L.hsa_build_bwt_index_device.argtypes = [C.c_int, C.c_uint64, vp, vp, C.POINTER(C.c_uint64), u64, C.c_uint32,
                                                 vp]
    if hasattr(L, "hsa_index_set_sa64"):            # (older A/B builds lack the 64-bit positions)
        L.hsa_build_bwt_index_device64.argtypes = [C.c_int, C.c_uint64, vp, vp, C.POINTER(C.c_uint64), u64, C.c_uint32,
                                                   vp]
        L.hsa_index_set_sa64.argtypes = [vp, u64, C.c_uint64, C.c_uint32, u64, C.c_int]
        L.hsa_index_set_sa64_device.argtypes = [vp, vp, C.c_uint64, C.c_uint32, u64, C.c_int]
        L.hsa_sa_position_batch64.argtypes = [vp, C.c_size_t, u64, u64]
        L.hsa_sa_position_device64.argtypes = [vp, C.c_size_t, vp, vp, vp]
        L.hsa_psi_minus_batch64.argtypes = [vp, C.c_size_t, u64, u64]
        L.hsa_hit_positions_device64.argtypes = [vp, C.POINTER(HitPosBatch64), vp]
    if hasattr(L, "hsa_refine_rows_device64"):      # (older A/B builds lack the refinement)
        L.hsa_index_set_text64_device.argtypes = [vp, vp, C.c_uint64]
        L.hsa_refine_rows_device64.argtypes = [vp, C.POINTER(RefineBatch64), vp]
    if hasattr(L, "hsa_choose_hits_device64"):      # (older A/B builds lack the choice)
        L.hsa_choose_hits_device64.argtypes = [vp, C.POINTER(ChooseBatch64), vp]
        L.hsa_choose_timing.argtypes = [C.c_int]
        L.hsa_choose_timing.restype = None
        L.hsa_choose_launch_times.argtypes = [vp, f32]
    if hasattr(L, "hsa_sam_lines_device64"):        # (older A/B builds lack the SAM lines)
        L.hsa_sam_lines_device64.argtypes = [vp, C.POINTER(SamBatch64), vp]
        L.hsa_sam_timing.argtypes = [C.c_int]
    if hasattr(L, "hsa_sam_lines_device64_trim"):
        L.hsa_sam_lines_device64_trim.argtypes = [vp, C.POINTER(SamBatch64), C.POINTER(SamTrim), vp]
        L.hsa_splice_lines_device_trim.argtypes = [vp, C.POINTER(SpliceLinesBatch), C.POINTER(SamTrim), vp]
    if hasattr(L, "hsa_splice_lines_device_xa"):
        L.hsa_splice_lines_device_xa.argtypes = [vp, C.POINTER(SpliceLinesBatch), C.POINTER(SamTrim), C.POINTER(SpliceXa), vp]
    if hasattr(L, "hsa_splice_lines_device"):
        L.hsa_splice_lines_device.argtypes = [vp, C.POINTER(SpliceLinesBatch), vp]
        L.hsa_sam_merge_device.argtypes = [vp, C.POINTER(SamMergeBatch), vp]
        L.hsa_sam_timing.restype = None
        L.hsa_sam_launch_times.argtypes = [vp, f32]
    if hasattr(L, "hsa_junction_rows_device"):      # (older A/B builds lack the junction table)
        L.hsa_junction_rows_device.argtypes = [vp, C.POINTER(JunctionRowsBatch), vp]
        L.hsa_junction_reduce_device.argtypes = [vp, C.POINTER(JunctionReduceBatch), vp]
        L.hsa_junction_text_device.argtypes = [vp, C.POINTER(JunctionTextBatch), vp]
    if hasattr(L, "hsa_reads_device"):              # (older A/B builds lack the FASTQ loader)
        L.hsa_reads_device.argtypes = [vp, C.POINTER(ReadsBatch), vp]
        if hasattr(L, "hsa_reads_device_opts"):
            L.hsa_reads_device_opts.argtypes = [vp, C.POINTER(ReadsBatch), vp]
        L.hsa_reads_timing.argtypes = [C.c_int]
        L.hsa_reads_timing.restype = None
        L.hsa_reads_launch_times.argtypes = [vp, f32]
    if hasattr(L, "hsa_fasta_device"):              # (older A/B builds lack the FASTA loader)
        L.hsa_fasta_scratch_bytes.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]
        L.hsa_fasta_device.argtypes = [C.c_int, C.POINTER(FastaBatch), vp]
        L.hsa_bwt_files_scratch_bytes.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]
        L.hsa_bwt_files_device.argtypes = [C.c_int, C.c_uint64, vp, vp, vp, vp, vp, C.c_uint64, vp]
        L.hsa_fasta_timing.argtypes = [C.c_int]
        L.hsa_fasta_timing.restype = None
        L.hsa_fasta_launch_times.argtypes = [f32]
        L.hsa_bwt_files_launch_times.argtypes = [f32]
    if hasattr(L, "hsa_bam_reads_device"):          # (older A/B builds lack the BAM loader)
        L.hsa_bam_reads_device.argtypes = [vp, C.POINTER(BamBatch), vp]
        L.hsa_bam_timing.argtypes = [C.c_int]
        L.hsa_bam_timing.restype = None
        if hasattr(L, "hsa_bam_walk_mode"):         # (the probe's knob: not in the public header)
            L.hsa_bam_walk_mode.argtypes = [C.c_int]
            L.hsa_bam_walk_mode.restype = None
        L.hsa_bam_launch_times.argtypes = [vp, C.POINTER(C.c_float)]
    if hasattr(L, "hsa_inflate_bgzf_device"):       # (older A/B builds lack the BGZF inflater)
        L.hsa_inflate_bgzf_device.argtypes = [C.c_int, C.POINTER(InflateBatch), vp]
    if hasattr(L, "hsa_extend_batch"):
        L.hsa_extend_batch.argtypes = [vp, C.POINTER(Regime), C.c_int, vp, C.c_int, u8, i32, C.c_size_t, i32, i32,
                                       u32]
    if hasattr(L, "hsa_extend_sliced"):
        L.hsa_extend_sliced.argtypes = [vp, C.POINTER(Regime), C.c_int, vp, i32, u8, C.c_int, u8, i32, C.c_size_t,
                                        C.c_int, C.c_uint32, i32, i32, u32]
    L.hsa_pass_times.argtypes = [vp, C.c_int, f32, f32]
    if hasattr(L, "hsa_cal_sa_reg_gap_multi"):      # (older A/B builds lack it)
        L.hsa_cal_sa_reg_gap_multi.restype = C.c_long
        L.hsa_cal_sa_reg_gap_multi.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(GapOpt), C.c_int, u32, u64, u8,
                                               C.c_size_t, i32, u32, u64, C.POINTER(C.POINTER(C.c_uint32)), i32,
                                               C.POINTER(Stats)]
    L.hsa_cal_sa_reg_gap_flat.restype = C.c_long
    L.hsa_cal_sa_reg_gap_flat.argtypes = [vp, C.POINTER(GapOpt), C.c_int, u32, u64, u8, C.c_size_t, i32, u32, u64,
                                          C.POINTER(C.POINTER(C.c_uint32)), i32, C.POINTER(Stats)]
    _lib = L
    return L


def check(rc):
    if rc < 0:
        raise HsaError(f"libhsa_gpu error {rc}: {lib().hsa_last_error().decode()}")
    return rc


def device_count() -> int:
    return lib().hsa_device_count()


def probe_gather(table_bytes: int, per_sector: int = 1, device: int = 0) -> float:
    """Measured random 64-byte-sector gather rate in GB/s (hsa_probe_gather)."""
    g = C.c_double()
    check(lib().hsa_probe_gather(device, table_bytes, per_sector, C.byref(g)))
    return g.value


def configure(waves_per_cu=0, pool_entries=0, hit_cap=0):
    check(lib().hsa_configure(waves_per_cu, pool_entries, hit_cap))


class DeviceU64:
    """A hipMalloc'd array of u64 on the current device: the sample array of
    build_bwt_index64, in the form hsa_index_set_sa64_device takes over (a torch tensor's
    memory belongs to torch's allocator and cannot be handed to the library).  free()
    unless an index took it (GpuIndex.set_sa64_device)."""

    def __init__(self, n: int):
        p = C.c_void_p()
        rc = lib().hipMalloc(C.byref(p), C.c_size_t(8 * max(int(n), 1)))
        if rc != 0 or not p.value:
            raise HsaError(f"hipMalloc of {8 * n} bytes failed ({rc})")
        self.ptr, self.n = p.value, int(n)

    def write(self, first: int, values):
        v = np.ascontiguousarray(values, np.uint64)
        assert 0 <= first and first + len(v) <= self.n
        rc = lib().hipMemcpy(C.c_void_p(self.ptr + 8 * first), v.ctypes.data_as(C.c_void_p), C.c_size_t(v.nbytes), 1)
        if rc != 0:
            raise HsaError(f"hipMemcpy to the device failed ({rc})")

    def to_host(self, first: int = 0, count: int | None = None) -> np.ndarray:
        count = self.n - first if count is None else count
        assert 0 <= first and first + count <= self.n
        out = np.zeros(count, np.uint64)
        rc = lib().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr + 8 * first), C.c_size_t(out.nbytes), 2)
        if rc != 0:
            raise HsaError(f"hipMemcpy from the device failed ({rc})")
        return out

    def free(self):
        if self.ptr:
            lib().hipFree(C.c_void_p(self.ptr))
            self.ptr = None


def build_bwt_index64(T: int, d_text: int, interval: int, device: int = 0):
    """hsa_build_bwt_index_device64 of the text at device pointer d_text (LSB-first
    2-bit codes, zero-padded): (the BWT codes as a torch int32 tensor on the device,
    isa0, C[5] as u64, the samples as a DeviceU64 with entry 0 set to T).  The samples
    stay on the device: GpuIndex.set_sa64_device takes them."""
    import torch
    nw = (T + 15) // 16
    bw = torch.zeros(nw + 8, dtype=torch.int32, device=f"cuda:{device}")
    torch.cuda.synchronize()
    isa0 = C.c_uint64()
    Cc = np.zeros(5, np.uint64)
    sa = DeviceU64((T + interval) // interval) if interval else None
    try:
        check(lib().hsa_build_bwt_index_device64(device, T, d_text, bw.data_ptr(), C.byref(isa0), Cc, interval,
                                                 sa.ptr if sa else None))
        if sa:
            sa.write(0, [T])
    except Exception:
        if sa:
            sa.free()
        raise
    return bw, int(isa0.value), Cc, sa


def _take_hits(hp, n):
    if n == 0:
        lib().hsa_free(hp)
        return np.zeros((0, 9), np.uint32)
    arr = np.ctypeslib.as_array(hp, shape=(n * 9,)).reshape(n, 9).copy()
    lib().hsa_free(hp)
    return arr


class GpuIndex:
    """The bidirectional index resident in HBM as rank blocks (one device)."""

    def __init__(self, fwd, rev, device: int = 0):
        self.T = fwd.T
        self.fwd_meta = fwd
        h = C.c_void_p()
        check(lib().hsa_index_create(device, fwd.T, fwd.isa0, np.ascontiguousarray(fwd.C, np.uint32),
                                     np.ascontiguousarray(fwd.code, np.uint32), rev.T, rev.isa0,
                                     np.ascontiguousarray(rev.C, np.uint32),
                                     np.ascontiguousarray(rev.code, np.uint32), C.byref(h)))
        self.h = h

    @classmethod
    def from_device_codes(cls, T, isa0, Cf, d_code, rT, risa0, Cr, d_rcode, device=0):
        self = cls.__new__(cls)
        self.T = T
        h = C.c_void_p()
        check(lib().hsa_index_create_device(device, T, isa0, np.ascontiguousarray(Cf, np.uint32), d_code, rT, risa0,
                                            np.ascontiguousarray(Cr, np.uint32), d_rcode, C.byref(h)))
        self.h = h
        return self

    @classmethod
    def from_device_codes64(cls, T, isa0, Cf, d_code, rT, risa0, Cr, d_rcode, device=0):
        """A 64-bit interval index (hsa_index_create_device64): any text length; under
        2^32 characters the 32-bit entry points serve it too."""
        self = cls.__new__(cls)
        self.T = T
        h = C.c_void_p()
        check(lib().hsa_index_create_device64(device, T, isa0, np.ascontiguousarray(Cf, np.uint64), d_code, rT, risa0,
                                              np.ascontiguousarray(Cr, np.uint64), d_rcode, C.byref(h)))
        self.h = h
        return self

    def is64(self) -> bool:
        return bool(lib().hsa_index_is64(self.h))

    def occ4_64(self, d, pos):
        pos = np.ascontiguousarray(pos, np.uint64)
        out = np.zeros((len(pos), 4), np.uint64)
        check(lib().hsa_occ4_batch64(self.h, d, len(pos), pos, out))
        return out

    def search_device64(self, regimes, batch: "DeviceBatch"):
        """hsa_search_device64: d_hits holds hsa_aln64_t records (14 u32)."""
        rg = (Regime * len(regimes))(*regimes)
        check(lib().hsa_search_device64(self.h, rg, len(regimes), C.byref(batch), None))

    def clone(self) -> "GpuIndex":
        """A second handle on this resident index (hsa_index_clone): the rank blocks,
        tries and SA are shared, the stream and search scratch are its own, so passes on
        the two handles run concurrently.  Closing this index closes its clones first."""
        h = C.c_void_p()
        check(lib().hsa_index_clone(self.h, C.byref(h)))
        c = GpuIndex.__new__(GpuIndex)
        c.T, c.h, c._parent = self.T, h, self
        if hasattr(self, "fwd_meta"):
            c.fwd_meta = self.fwd_meta
        if not hasattr(self, "_clones"):
            self._clones = weakref.WeakSet()
        self._clones.add(c)
        return c

    def release_scratch(self):
        """hsa_index_release_scratch: the handle's search and splice working buffers go back
        (the next call allocates them again)."""
        if getattr(self, "h", None):
            check(lib().hsa_index_release_scratch(self.h))

    def close(self):
        for c in list(getattr(self, "_clones", ())):
            c.close()
        if getattr(self, "h", None):
            lib().hsa_index_free(self.h)
            self.h = None
        if getattr(self, "_log_n", None) is not None:
            self._log_n.free()
            self._log_n = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream_handle(self) -> int:
        return int(lib().hsa_index_stream(self.h))

    def search_device(self, regimes, batch: "DeviceBatch"):
        rg = (Regime * len(regimes))(*regimes)
        check(lib().hsa_search_device(self.h, rg, len(regimes), C.byref(batch), None))

    def splice_seeds_device(self, seed_regime, batch: "SeedBatch"):
        """The six splice seed searches of every fallback read of a device batch
        (hsa_splice_seeds_device); records 6 r + i on the device."""
        check(lib().hsa_splice_seeds_device(self.h, C.byref(seed_regime), C.byref(batch), None))

    def splice_prefetch(self, seed_regime, anchor_regime, lens, codes, anchor_max_diff):
        """hsa_splice_prefetch_batch over host reads: numpy copies of its outputs
        (rows (n, 6, row_stride, 2), call_n (n, 8), call_hit, hits (m, 9), wafter
        (n, 8, cw_stride, 2), call_sa, sa (k, 4))."""
        lens = np.ascontiguousarray(lens, np.uint32)
        codes = np.ascontiguousarray(codes, np.uint8)
        offs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64)
        amd = np.ascontiguousarray(anchor_max_diff, np.int32)
        o = SplicePf()
        check(lib().hsa_splice_prefetch_batch(self.h, C.byref(seed_regime), C.byref(anchor_regime), len(lens), lens,
                                              offs, codes, len(codes), amd, C.byref(o)))
        n, rs, cws = o.n, o.row_stride, o.cw_stride

        def arr(ptr, ct, count):
            if not ptr or count == 0:
                return np.zeros(0, ct)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(ct))), (count,)).copy()
        return dict(rows=arr(o.rows, np.int32, n * 6 * rs * 2).reshape(n, 6, rs, 2),
                    call_n=arr(o.call_n, np.int32, n * 8).reshape(n, 8),
                    call_hit=arr(o.call_hit, np.uint64, n * 8).reshape(n, 8),
                    hits=arr(o.hits, np.uint32, int(o.n_hits) * 9).reshape(-1, 9),
                    wafter=arr(o.wafter, np.int32, n * 8 * cws * 2).reshape(n, 8, cws, 2),
                    call_sa=arr(o.call_sa, np.uint64, n * 8).reshape(n, 8) if o.call_sa else None,
                    sa=arr(o.sa, np.uint32, int(o.n_sa) * 4).reshape(-1, 4), kernel_ms=o.kernel_ms)

    def set_text(self, packed_words, dna_len):
        """Upload the packed reference as the HSP holds it (16 codes per u32, the first in
        the high bits; hsa_index_set_text) for the splice kernel."""
        w = np.ascontiguousarray(packed_words, np.uint32)
        check(lib().hsa_index_set_text(self.h, w, len(w), int(dna_len)))

    def splice_device(self, seed_regime, anchor_regime, ext_regime, batch: "SpliceBatch"):
        """bwt_splice_match of every fallback read of a device batch, on the device
        (hsa_splice_device): HSA_SP_RES_WORDS words per job at batch.d_res."""
        check(lib().hsa_splice_device(self.h, C.byref(seed_regime), C.byref(anchor_regime), C.byref(ext_regime),
                                      C.byref(batch), None))

    def splice_match(self, seed_regime, anchor_regime, ext_regime, lens, codes, max_diff):
        """hsa_splice_match_batch: bwt_splice_match of each read on the device.  Returns
        (res (n, SP_RES_WORDS) uint32: status, n_aln, res_aln[0], res_aln[1]; stats)."""
        lens = np.ascontiguousarray(lens, np.uint32)
        codes = np.ascontiguousarray(codes, np.uint8)
        offs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64)
        amd = np.ascontiguousarray(max_diff, np.int32)
        res = np.zeros((len(lens), SP_RES_WORDS), np.uint32)
        o, st = SplicePf(), SpliceStats()
        check(lib().hsa_splice_match_batch(self.h, C.byref(seed_regime), C.byref(anchor_regime), C.byref(ext_regime),
                                           len(lens), lens, offs, codes, len(codes), amd, C.byref(o), res,
                                           C.byref(st)))
        return res, {k: getattr(st, k) for k, _ in SpliceStats._fields_}

    def set_sa(self, sa, blocks):
        """Upload the sampled SA (index_io.SaFile) and the block table (rows of
        chrID, blockStart, blockEnd, ori) for SA -> position (hsa_index_set_sa)."""
        vals = np.ascontiguousarray(sa.values, np.uint32)
        blk = np.ascontiguousarray(blocks, np.uint32).reshape(-1)
        if blk.size == 0:
            blk = np.zeros(4, np.uint32)
        check(lib().hsa_index_set_sa(self.h, vals, len(vals), sa.interval, blk, len(blocks)))

    def sa_positions(self, idx):
        """(SA value, chrID, 1-based position, packed position) per SA index."""
        idx = np.ascontiguousarray(idx, np.uint32)
        out = np.zeros((len(idx), 4), np.uint32)
        check(lib().hsa_sa_position_batch(self.h, len(idx), idx, out))
        return out

    @staticmethod
    def _blocks64(blocks):
        blk = np.ascontiguousarray(blocks, np.uint64).reshape(-1, 4)
        return (blk.reshape(-1) if len(blk) else np.zeros(4, np.uint64)), len(blk)

    def _handle(self):
        if not getattr(self, "h", None):
            raise HsaError("the index is closed (no handle)")
        return self.h

    def set_sa64(self, values, interval, blocks):
        """hsa_index_set_sa64: the sampled SA as u64 values (values[r / interval] = SA[r],
        values[0] = T) and the block table (rows of chrID, blockStart, blockEnd, ori as
        u64), on an index of from_device_codes64."""
        vals = np.ascontiguousarray(values, np.uint64)
        blk, nb = self._blocks64(blocks)
        check(lib().hsa_index_set_sa64(self._handle(), vals, len(vals), int(interval), blk, nb))

    def set_sa64_device(self, ptr, n, interval, blocks):
        """hsa_index_set_sa64_device: the same from a hipMalloc'd device array of n u64
        (a DeviceU64 or its address), which the index owns from here on."""
        blk, nb = self._blocks64(blocks)
        p = ptr.ptr if isinstance(ptr, DeviceU64) else ptr
        check(lib().hsa_index_set_sa64_device(self._handle(), p, int(n), int(interval), blk, nb))
        if isinstance(ptr, DeviceU64):
            ptr.ptr = None

    def sa_positions64(self, idx):
        """(SA value, chrID, 1-based position, text position) per SA index, u64; all-ones
        where no block holds it, in all four for a walk cut by HSA_SA_MAX_WALK."""
        idx = np.ascontiguousarray(idx, np.uint64)
        out = np.zeros((len(idx), 4), np.uint64)
        check(lib().hsa_sa_position_batch64(self._handle(), len(idx), idx, out))
        return out

    def psi_minus64(self, idx):
        """One LF step per SA index (hsa_psi_minus_batch64); the '$' row answers 0."""
        idx = np.ascontiguousarray(idx, np.uint64)
        out = np.zeros(len(idx), np.uint64)
        check(lib().hsa_psi_minus_batch64(self._handle(), len(idx), idx, out))
        return out

    def hit_positions64(self, batch: "HitPosBatch64", max_occ=None, stream=None):
        """hsa_hit_positions_device64: the device hit lists of search_device64 to
        positions (batch.d_pos_off, d_pos, d_pos_hit, d_counters) on `stream` (a
        hipStream_t address; None: the index's own); does not synchronise."""
        if max_occ is not None:
            batch.max_occ = int(max_occ)
        check(lib().hsa_hit_positions_device64(self._handle(), C.byref(batch), stream))

    def set_text64_device(self, ptr, T):
        """hsa_index_set_text64_device: the text as the 64-bit builder takes it (LSB-first
        2-bit codes, 16 per u32) from a hipMalloc'd device array (a DeviceU64 or its
        address), which the index owns from here on."""
        p = ptr.ptr if isinstance(ptr, DeviceU64) else ptr
        check(lib().hsa_index_set_text64_device(self._handle(), p, int(T)))
        if isinstance(ptr, DeviceU64):
            ptr.ptr = None

    def refine_rows64(self, batch: "RefineBatch64", stream=None):
        """hsa_refine_rows_device64: every position row of hit_positions64 to CIGAR, NM and
        MD (batch.d_rows, d_rpos, d_cigar, d_md, d_counters) on `stream` (a hipStream_t
        address; None: the index's own); does not synchronise.  hsa_amd.refine turns a
        row's output into the SAM strings."""
        check(lib().hsa_refine_rows_device64(self._handle(), C.byref(batch), stream))

    def choose_hits64(self, batch: "ChooseBatch64", stream=None):
        """hsa_choose_hits_device64: each read's hit as the reference chooses it (the
        drand48 sequence from batch.rng_state, in read order), mapQ, X0 / X1 and the chosen
        and XA rows (batch.d_sel, d_sel64, d_rng_out, d_pos_off, d_pos, d_pos_hit,
        d_counters) on `stream` (a hipStream_t address; None: the index's own); does not
        synchronise.  A batch without d_log_n gets the index's own copy of log_n_table().
        refine_rows64 takes the rows as it takes hit_positions64's; hsa_amd.sam formats the
        line."""
        if not hasattr(lib(), "hsa_choose_hits_device64"):
            raise HsaError("this libhsa_gpu.so has no hsa_choose_hits_device64: rebuild it")
        if not batch.d_log_n:
            if getattr(self, "_log_n", None) is None:
                t = log_n_table()
                self._log_n = DeviceU64(len(t) // 2)
                self._log_n.write(0, t.view(np.uint64))
            batch.d_log_n = self._log_n.ptr
        check(lib().hsa_choose_hits_device64(self._handle(), C.byref(batch), stream))

    CHOOSE_LAUNCHES = ("class", "scan", "compact", "maps", "walk", "pick", "rows")

    def choose_launch_times(self) -> dict:
        """hsa_choose_launch_times: ms per launch of this handle's last choose_hits64 call
        made after lib().hsa_choose_timing(1); waits for it."""
        ms = np.zeros(len(self.CHOOSE_LAUNCHES), np.float32)
        check(lib().hsa_choose_launch_times(self._handle(), ms))
        return {k: float(v) for k, v in zip(self.CHOOSE_LAUNCHES, ms)}

    def sam_lines64(self, batch: "SamBatch64", stream=None, trim: "SamTrim" = None):
        """hsa_sam_lines_device64: the SAM lines of a batch from the device outputs of
        search_device64, choose_hits64 and refine_rows64 (batch.d_line_off, d_out,
        d_line_stat, d_counters) on `stream` (a hipStream_t address; None: the index's own);
        does not synchronise.  hsa_amd.sam.device_sam drives it.  Without a handle the
        library answers itself: HSA_E_NODEV where no GPU is visible.  trim: the reads' stored
        lengths and barcodes (hsa_sam_lines_device64_trim), or None."""
        if not hasattr(lib(), "hsa_sam_lines_device64"):
            raise HsaError("this libhsa_gpu.so has no hsa_sam_lines_device64: rebuild it")
        if trim is None:
            check(lib().hsa_sam_lines_device64(getattr(self, "h", None), C.byref(batch), stream))
        else:
            check(lib().hsa_sam_lines_device64_trim(getattr(self, "h", None), C.byref(batch), C.byref(trim), stream))

    def splice_lines(self, batch: "SpliceLinesBatch", stream=None, trim: "SamTrim" = None, xa: "SpliceXa" = None):
        """hsa_splice_lines_device: the SAM lines of the spliced reads of a batch from
        splice_device's results (batch.d_rows, d_cigar, d_line_off, d_out, d_line_stat,
        d_counters) on `stream` (a hipStream_t address; None: the index's own); does not
        synchronise.  hsa_amd.chain.splice_lines drives it.  trim: as sam_lines64 takes it
        (hsa_splice_lines_device_trim).  xa: a SpliceXa, and the call is
        hsa_splice_lines_device_xa: a read with several splice pairs gets its line with the
        XA:Z list instead of HSA_SL_MULTI (None: the plain entry points)."""
        if not hasattr(lib(), "hsa_splice_lines_device"):
            raise HsaError("this libhsa_gpu.so has no hsa_splice_lines_device: rebuild it")
        if xa is not None:
            if not hasattr(lib(), "hsa_splice_lines_device_xa"):
                raise HsaError("this libhsa_gpu.so has no hsa_splice_lines_device_xa: rebuild it")
            check(lib().hsa_splice_lines_device_xa(getattr(self, "h", None), C.byref(batch), C.byref(trim) if trim is not None else None,
                                                   C.byref(xa), stream))
        elif trim is None:
            check(lib().hsa_splice_lines_device(getattr(self, "h", None), C.byref(batch), stream))
        else:
            check(lib().hsa_splice_lines_device_trim(getattr(self, "h", None), C.byref(batch), C.byref(trim), stream))

    def _junction_call(self, name, batch, stream):
        if not hasattr(lib(), name):
            raise HsaError(f"this libhsa_gpu.so has no {name}: rebuild it")
        check(getattr(lib(), name)(getattr(self, "h", None), C.byref(batch), stream))

    def junction_rows(self, batch: "JunctionRowsBatch", stream=None):
        """hsa_junction_rows_device: one junction row per printed spliced read of a lines call,
        appended to a row buffer.  The call does not synchronise; hsa_amd.chain.junction_rows
        drives it."""
        self._junction_call("hsa_junction_rows_device", batch, stream)

    def junction_reduce(self, batch: "JunctionReduceBatch", stream=None):
        """hsa_junction_reduce_device: a row buffer sorted, equal introns merged, the motifs
        read from the text, in place (hsa_amd.chain.junction_reduce)."""
        self._junction_call("hsa_junction_reduce_device", batch, stream)

    def junction_text(self, batch: "JunctionTextBatch", stream=None):
        """hsa_junction_text_device: the text of a reduced table (hsa_amd.chain.junction_text)."""
        self._junction_call("hsa_junction_text_device", batch, stream)

    def sam_merge(self, batch: "SamMergeBatch", stream=None):
        """hsa_sam_merge_device: the lines of sam_lines64 and of splice_lines over the same
        reads as one text in read order (batch.d_line_off, d_out, d_counters) on `stream`; does
        not synchronise."""
        if not hasattr(lib(), "hsa_sam_merge_device"):
            raise HsaError("this libhsa_gpu.so has no hsa_sam_merge_device: rebuild it")
        check(lib().hsa_sam_merge_device(getattr(self, "h", None), C.byref(batch), stream))

    def reads_device(self, batch: "ReadsBatch", stream=None):
        """hsa_reads_device: the bytes of a FASTQ chunk on the device to a search batch, the
        names and qualities and a row per record (batch.d_jobs, d_codes, d_names, d_name_off,
        d_quals, d_qual_off, d_rec, d_counters) on `stream` (a hipStream_t address; None: the
        index's own); does not synchronise.  hsa_amd.reads.load_device drives it.  Without a
        handle the library answers itself: HSA_E_NODEV where no GPU is visible."""
        if not hasattr(lib(), "hsa_reads_device"):
            raise HsaError("this libhsa_gpu.so has no hsa_reads_device: rebuild it")
        check(lib().hsa_reads_device(getattr(self, "h", None), C.byref(batch), stream))

    def bam_reads_device(self, batch: "BamBatch", stream=None):
        """hsa_bam_reads_device: the inflated bytes of a BAM file on the device to the search
        batch reads_device_opts leaves; queued on `stream` (None: the index's)."""
        if not hasattr(lib(), "hsa_bam_reads_device"):
            raise HsaError("this libhsa_gpu.so has no hsa_bam_reads_device: rebuild it")
        check(lib().hsa_bam_reads_device(getattr(self, "h", None), C.byref(batch), stream))

    def bam_launch_times(self):
        """hsa_bam_launch_times: ms per launch (BAM_LAUNCHES) of this handle's last
        bam_reads_device call made under hsa_bam_timing(1)."""
        ms = (C.c_float * len(BAM_LAUNCHES))()
        check(lib().hsa_bam_launch_times(self.h, ms))
        return dict(zip(BAM_LAUNCHES, (float(v) for v in ms)))

    def reads_device_opts(self, batch: "ReadsBatch", stream=None):
        """hsa_reads_device_opts: reads_device with the reader's options of batch.trim_qual and
        batch.mode (-q, -B, -Y, -I), batch.d_full_len, d_bc, rec_cap and d_opt_counters."""
        if not hasattr(lib(), "hsa_reads_device_opts"):
            raise HsaError("this libhsa_gpu.so has no hsa_reads_device_opts: rebuild it")
        check(lib().hsa_reads_device_opts(getattr(self, "h", None), C.byref(batch), stream))

    READS_LAUNCHES = ("count", "tile_scan", "lines", "record", "max_keep", "record_scan", "rows", "bytes")

    def reads_launch_times(self) -> dict:
        """hsa_reads_launch_times: ms per launch of this handle's last reads_device call made
        after lib().hsa_reads_timing(1); waits for it."""
        ms = np.zeros(len(self.READS_LAUNCHES), np.float32)
        check(lib().hsa_reads_launch_times(self._handle(), ms))
        return {k: float(v) for k, v in zip(self.READS_LAUNCHES, ms)}

    SAM_LAUNCHES = ("len", "scan", "write")

    def sam_launch_times(self) -> dict:
        """hsa_sam_launch_times: ms per launch of this handle's last sam_lines64 call made
        after lib().hsa_sam_timing(1); waits for it."""
        ms = np.zeros(len(self.SAM_LAUNCHES), np.float32)
        check(lib().hsa_sam_launch_times(self._handle(), ms))
        return {k: float(v) for k, v in zip(self.SAM_LAUNCHES, ms)}

    def last_pass_ms(self):
        """(k_widths ms, k_search ms) of the last device pass on this index."""
        w, q = C.c_float(), C.c_float()
        check(lib().hsa_last_pass_ms(self.h, C.byref(w), C.byref(q)))
        return w.value, q.value

    def pass_times(self, n):
        """(k_widths ms, k_search ms) arrays of the last n hsa_search_device passes."""
        w = np.zeros(n, np.float32)
        s = np.zeros(n, np.float32)
        check(lib().hsa_pass_times(self.h, n, w, s))
        return w, s

    def nbytes(self) -> int:
        return int(lib().hsa_index_bytes(self.h))

    def trie(self):
        """(width-trie depth, search-trie depth, bytes) of the index's root tries."""
        d, sd, b = C.c_uint32(), C.c_uint32(), C.c_size_t()
        check(lib().hsa_index_trie(self.h, C.byref(d), C.byref(sd), C.byref(b)))
        return int(d.value), int(sd.value), int(b.value)

    def levels(self):
        """(level of the implicit root levels' table, its strings that do not occur)."""
        lv, ab = C.c_uint32(), C.c_uint32()
        check(lib().hsa_index_levels(self.h, C.byref(lv), C.byref(ab)))
        return int(lv.value), int(ab.value)

    def occ4(self, d, pos):
        pos = np.ascontiguousarray(pos, np.uint32)
        out = np.zeros((len(pos), 4), np.uint32)
        check(lib().hsa_occ4_batch(self.h, d, len(pos), pos, out))
        return out

    def step_all(self, klrr):
        klrr = np.ascontiguousarray(klrr, np.uint32).reshape(-1, 4)
        out = np.zeros((len(klrr), 16), np.uint32)
        check(lib().hsa_step_batch(self.h, len(klrr), klrr, out))
        return out.reshape(-1, 4, 4)   # [n][k, l, rk, rl][c]

    def widths(self, lens, codes, type=1):
        """bwt_cal_width of each sequence (type 1: hsa_width_batch, 0: hsa_width0_batch):
        2 * (len + 1) words each, packed."""
        lens = np.ascontiguousarray(lens, np.uint32)
        offs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64)
        tot = int(np.sum(2 * (lens.astype(np.int64) + 1)))
        out = np.zeros(tot, np.uint32)
        codes = np.ascontiguousarray(codes, np.uint8)
        fn = lib().hsa_width_batch if type == 1 else lib().hsa_width0_batch
        check(fn(self.h, len(lens), offs, lens, codes, len(codes), out))
        return out

    def search(self, regimes, jobs, codes):
        """Raw search over a job table (JOB_DTYPE)."""
        jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
        n = len(jobs)
        rg = (Regime * len(regimes))(*regimes)
        n_aln = np.zeros(n, np.int32)
        flags = np.zeros(n, np.uint32)
        hoff = np.zeros(n, np.uint64)
        hp = C.POINTER(C.c_uint32)()
        st = Stats()
        codes = np.ascontiguousarray(codes, np.uint8)
        tot = check(lib().hsa_search_batch(self.h, rg, len(regimes), jobs.ctypes.data, n, codes, len(codes), n_aln,
                                           flags, hoff, C.byref(hp), C.byref(st)))
        return n_aln, flags, hoff, _take_hits(hp, tot), st.as_dict()

    def extend(self, regimes, jobs, codes, bids):
        """hsa_extend_batch: jobs (EXT_DTYPE), the windows' codes / bids; returns
        (ret, max_pos, aln (n, 9))."""
        n = len(jobs)
        rg = (Regime * len(regimes))(*regimes)
        ret = np.zeros(n, np.int32)
        mp = np.zeros(n, np.int32)
        aln = np.zeros((n, 9), np.uint32)
        codes = np.ascontiguousarray(codes, np.uint8)
        bids = np.ascontiguousarray(bids, np.int32)
        check(lib().hsa_extend_batch(self.h, rg, len(regimes), np.ascontiguousarray(jobs).ctypes.data, n,
                                     codes if len(codes) else np.zeros(1, np.uint8),
                                     bids if len(bids) else np.zeros(1, np.int32), len(codes), ret, mp, aln))
        return ret, mp, aln

    def extend_sliced(self, regimes, jobs, codes, bids, slots, resume, n_slots, budget):
        """One hsa_extend_sliced launch: returns (ret, max_pos, aln (n, 9))."""
        n = len(jobs)
        rg = (Regime * len(regimes))(*regimes)
        ret = np.zeros(n, np.int32)
        mp = np.zeros(n, np.int32)
        aln = np.zeros((n, 9), np.uint32)
        codes = np.ascontiguousarray(codes, np.uint8)
        bids = np.ascontiguousarray(bids, np.int32)
        check(lib().hsa_extend_sliced(self.h, rg, len(regimes), np.ascontiguousarray(jobs).ctypes.data,
                                      np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(resume, np.uint8), n,
                                      codes if len(codes) else np.zeros(1, np.uint8),
                                      bids if len(bids) else np.zeros(1, np.int32), len(codes), int(n_slots),
                                      int(budget), ret, mp, aln))
        return ret, mp, aln

    def match_gap(self, regimes, jobs, mg, codes, widths):
        """hsa_match_gap_batch: direct bwt_match_gap calls with caller widths.
        widths (P, 2) int32 pairs; returns (n_aln, hit_off, hits, widths after, stats)."""
        jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
        mg = np.ascontiguousarray(mg, MG_DTYPE)
        n = len(jobs)
        rg = (Regime * len(regimes))(*regimes)
        w = np.ascontiguousarray(widths, np.int32).reshape(-1)
        wout = w.copy()
        n_aln = np.zeros(n, np.int32)
        hoff = np.zeros(n, np.uint64)
        hp = C.POINTER(C.c_uint32)()
        st = Stats()
        codes = np.ascontiguousarray(codes, np.uint8)
        tot = check(lib().hsa_match_gap_batch(self.h, rg, len(regimes), jobs.ctypes.data, mg.ctypes.data, n, codes,
                                              len(codes), w, len(w) // 2, wout, n_aln, hoff, C.byref(hp),
                                              C.byref(st)))
        return n_aln, hoff, _take_hits(hp, tot), wout.reshape(-1, 2), st.as_dict()

    def cal_sa_reg_gap(self, lens, codes, opt: GapOpt):
        """bwa_cal_sa_reg_gap semantics over one batch (mutates opt like the reference)."""
        lens = np.ascontiguousarray(lens, np.uint32)
        n = len(lens)
        offs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64) if n else \
            np.zeros(0, np.uint64)
        codes = np.ascontiguousarray(codes, np.uint8)
        n_aln = np.zeros(n, np.int32)
        flags = np.zeros(n, np.uint32)
        hoff = np.zeros(n, np.uint64)
        sp = np.zeros(2 * n + 2, np.int32)
        hp = C.POINTER(C.c_uint32)()
        st = Stats()
        tot = check(lib().hsa_cal_sa_reg_gap_flat(self.h, C.byref(opt), n, lens, offs, codes, len(codes), n_aln,
                                                  flags, hoff, C.byref(hp), sp, C.byref(st)))
        hits = _take_hits(hp, tot)
        return n_aln, flags, hoff, hits, st.as_dict()

    def cal_sa_reg_gap_slots(self, others, lens, codes, opt: GapOpt):
        """cal_sa_reg_gap split over this index and `others` (device slots holding the
        same BWT: hsa_cal_sa_reg_gap_multi)."""
        ixs = [self] + list(others)
        arr = (C.c_void_p * len(ixs))(*[i.h for i in ixs])
        lens = np.ascontiguousarray(lens, np.uint32)
        n = len(lens)
        offs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64) if n else \
            np.zeros(0, np.uint64)
        codes = np.ascontiguousarray(codes, np.uint8)
        n_aln = np.zeros(n, np.int32)
        flags = np.zeros(n, np.uint32)
        hoff = np.zeros(n, np.uint64)
        sp = np.zeros(2 * n + 2, np.int32)
        hp = C.POINTER(C.c_uint32)()
        st = Stats()
        tot = check(lib().hsa_cal_sa_reg_gap_multi(arr, len(ixs), C.byref(opt), n, lens, offs, codes, len(codes), n_aln,
                                                   flags, hoff, C.byref(hp), sp, C.byref(st)))
        return n_aln, flags, hoff, _take_hits(hp, tot), st.as_dict()

    def run_batches(self, lens, codes, opt_dict, batch, others=()):
        """bwa_aln_core's batch loop (bwtaln.c:477-506); hits regrouped in read order.
        With `others`, each batch is split over the device slots self + others."""
        opt = GapOpt.from_dict(opt_dict)
        lens = np.asarray(lens, np.uint32)
        offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
        na_all, fl_all, per_read, stats = [], [], [], []
        for b0 in range(0, len(lens), batch):
            b1 = min(b0 + batch, len(lens))
            if others:
                na, fl, ho, hits, st = self.cal_sa_reg_gap_slots(others, lens[b0:b1], codes[offs[b0]:offs[b1]], opt)
            else:
                na, fl, ho, hits, st = self.cal_sa_reg_gap(lens[b0:b1], codes[offs[b0]:offs[b1]], opt)
            for j in range(b1 - b0):
                per_read.append(hits[int(ho[j]):int(ho[j]) + max(int(na[j]), 0)])
            na_all.append(na)
            fl_all.append(fl)
            stats.append(st)
        n_aln = np.concatenate(na_all) if na_all else np.zeros(0, np.int32)
        flags = np.concatenate(fl_all) if fl_all else np.zeros(0, np.uint32)
        return n_aln, flags, per_read, stats
