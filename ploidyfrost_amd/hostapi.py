"""ctypes binding of the C facade over the C++ host layer (include/ploidyfrost_host.h)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import hipapi

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "csrc", "libploidyfrost_host.so")


class Times(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("load_s", "upload_s", "bfs_device_s", "replay_s", "bubble_write_s", "find_total_s",
                                          "cov_device_s", "tasks_s", "align_s", "sites_s", "format_s", "write_s",
                                          "ploidy_total_s")] + \
               [(n, C.c_uint64) for n in ("unitigs", "kmers", "candidates", "superbubbles", "tasks", "align_jobs", "site_strings",
                                          "output_bytes")] + [("allele", C.c_uint64 * 4), ("core_cov", C.c_uint64),
                                                              ("core_num", C.c_uint64), ("scan_s", C.c_double), ("scan_serial_s", C.c_double),
                                                              ("bfs_large", C.c_uint64), ("bfs_max_seen", C.c_uint64), ("bfs_deferred", C.c_uint64),
                                                              ("snp_jobs", C.c_uint64), ("pair_jobs", C.c_uint64), ("wave_jobs", C.c_uint64), ("stack_jobs", C.c_uint64),
                                                              ("host_commit_records", C.c_uint64), ("host_walk_vertices", C.c_uint64)]


_lib = None
DECLARED_SYMBOLS = ["pfh_open", "pfh_close", "pfh_last_error", "pfh_set_output_dir", "pfh_set_write_files", "pfh_set_threads", "pfh_set_batch_bubbles", "pfh_set_align_pieces", "pfh_set_reference_threads", "pfh_set_overlap_output", "pfh_set_third_tier_on_host", "pfh_set_unitig_id",
                    "pfh_find_superbubbles", "pfh_ploidy_estimation", "pfh_get_times", "pfh_load_trace", "pfh_filter", "pfh_r_format_double", "pfh_device_ctx", "pfh_state", "pfh_last_allele_frequency",
                    "pfh_open_colored", "pfh_num_colors", "pfh_ploidy_estimation_colored",
                    "pfh_colors_open", "pfh_colors_close", "pfh_colors_count", "pfh_colors_unitigs", "pfh_colors_name",
                    "pfh_colors_unitig", "pfh_bifrost_kmer_hash", "pfh_gfa_abundant_kmers", "pfh_gfa_write_unitig_ids", "pfh_gfa_write_unitig_ids_given_inputs", "pfh_gfa_write_unitig_ids_given_arrays", "pfh_gfa_numbering_replays", "pfh_gfa_minimizer_counts", "pfh_host_walk", "pfh_host_walk_range", "pfh_replay_open", "pfh_replay_close", "pfh_replay_apply", "pfh_replay_state", "pfh_replay_apply_parallel", "pfh_side_components", "pfh_replay_check_footprints", "pfh_colors_check_footprints",
                    "pfh_find_shard", "pfh_shard_records", "pfh_shard_pool", "pfh_find_replay", "pfh_set_replay_threads", "pfh_set_write_super_bubble", "pfh_ploidy_select", "pfh_ploidy_select_colored", "pfh_ploidy_align", "pfh_ploidy_text", "pfh_ploidy_write",
                    "pfh_gmm_open", "pfh_gmm_close", "pfh_gmm_last_error", "pfh_gmm_read_fre", "pfh_gmm_read_cov", "pfh_gmm_set_values",
                    "pfh_gmm_size", "pfh_gmm_values", "pfh_gmm_fit", "pfh_gmm_run", "pfh_gmm_kernel_time",
                    "pfh_set_model", "pfh_model_values", "pfh_model_fit", "pfh_model_ploidy", "pfh_text_bytes_fetched", "pfh_model_rows",
                    "pfh_set_filter", "pfh_filter_rows",
                    "pfh_set_filter_multi", "pfh_filter_rows_multi", "pfh_model_color_count", "pfh_model_color_at", "pfh_model_color_values",
                    "pfh_model_color_fit", "pfh_model_color_ploidy",
                    "pfh_gmm_read_column", "pfh_gmm_density", "pfh_gmm_write_density", "pfh_gmm_density_time",
                    "pfh_set_density", "pfh_model_density_points", "pfh_model_density", "pfh_model_color_density",
                    "pfh_kmc_histogram", "pfh_cutoffs_from_rows", "pfh_set_auto_cutoffs", "pfh_cutoffs",
                    "pfh_mask_fastq", "pfh_mask_read", "pfh_mask_index_fastq", "pfh_mask_clause_text",
                    "pfh_count_fastq", "pfh_mask_fastq_counted", "pfh_count_reads_host", "pfh_count_encode_kmc1", "pfh_count_counter_bytes",
                    "pfh_count_lut_prefix_len", "pfh_count_cut_text", "pfh_build_fastq", "pfh_unitig_build_host", "pfh_unitig_no_room_text",
                    "pfh_build_colored_fastq", "pfh_build_colored_host", "pfh_bfg_colors_bytes", "pfh_color_no_room_text",
                    "pfh_run_defaults", "pfh_run_fastq", "pfh_count_masked_host", "pfh_run_multi_fastq", "pfh_union_host",
                    "pfh_trim_fastq", "pfh_trim_fastq_pair", "pfh_trim_parse_step", "pfh_trim_refusal_text", "pfh_trim_read", "pfh_trim_fastq_chunk",
                    "pfh_run_fastq_trimmed", "pfh_run_multi_fastq_trimmed", "pfh_trim_table_chunk", "pfh_trim_table_chunk_pair", "pfh_trim_table_clause_text",
                    "pfh_inflate_parse_member", "pfh_inflate_member", "pfh_inflate_bgzf_member", "pfh_inflate_crc32", "pfh_inflate_crc32_sliced",
                    "pfh_inflate_file_clause", "pfh_inflate_clause_text", "pfh_reads_gz", "pfh_reads_fasta", "pfh_fasta_index", "pfh_fasta_clause_text",
                    "pfh_gunzip_header", "pfh_gunzip_file_kind", "pfh_gunzip_candidate", "pfh_gunzip_call", "pfh_gunzip_file", "pfh_gunzip_clause_text",
                    "pfh_deflate_member", "pfh_deflate_bound", "pfh_reads_gz_out",
                    "pfh_reads_adapters", "pfh_reads_adapters_report", "pfh_clip_parse_adapters", "pfh_clip_refusal_text", "pfh_clip_read",
                    "pfh_trim_fastq_chunk_clip", "pfh_reads_adapter_pairs", "pfh_reads_adapters_pair_report", "pfh_clip_parse_adapter_pairs",
                    "pfh_clip_pair", "pfh_trim_fastq_pair_chunk_clip",
                    "pfh_reads_report", "pfh_qc_fastq", "pfh_qc_fastq_chunk", "pfh_qc_report_text", "pfh_qc_phred_hint",
                    "pfh_hetpairs_host", "pfh_smudge_report_text", "pfh_smudge_of", "pfh_smudge", "pfh_reads_smudge", "pfh_reads_smudge_result",
                    "pfh_reads_dedup", "pfh_reads_dedup_report", "pfh_dedup_key", "pfh_dedup_units", "pfh_trim_fastq_chunk_dedup",
                    "pfh_trim_fastq_pair_chunk_dedup"]


class RunOptions(C.Structure):   # pfh_run_options (include/ploidyfrost_host.h)
    _fields_ = [("k", C.c_uint32), ("ci", C.c_uint64), ("cx", C.c_uint64), ("cs", C.c_uint64), ("g", C.c_int32), ("clip_tips", C.c_int),
                ("del_isolated", C.c_int), ("chunk_bytes", C.c_uint64), ("initial_slots", C.c_uint64), ("quantile", C.c_double),
                ("mask_up", C.c_uint32), ("complex_size", C.c_uint32), ("match", C.c_double), ("mismatch", C.c_double), ("gap", C.c_double),
                ("threads", C.c_uint32), ("model_source", C.c_int), ("model_only", C.c_int), ("db_out", C.c_char_p), ("gfa_out", C.c_char_p)]


RUN_STATS_FIELDS = ("reads", "bases", "kmers", "bad", "distinct", "lower", "upper", "windows_bad", "windows_kept", "distinct_kept", "unitigs",
                    "removed", "unitigs_out", "longest")   # pfh_run_stats: the fields of `run`'s stderr line, in its order
RUN_MULTI_STATS_FIELDS = ("colors", "reads", "bases", "kmers", "bad", "distinct", "windows_bad", "windows_kept", "distinct_kept", "unitigs", "removed",
                          "unitigs_out", "longest", "kmers_colored", "kmers_unplaced", "runs", "overflow", "color_bytes")   # pfh_run_multi_stats: `run-multi`'s stderr line
RUN_MULTI_COLOR_FIELDS = ("lower", "upper", "distinct", "kept")   # of its `run-multi: color c ...` lines
MASKCOUNT_STATS_FIELDS = ("reads", "bases", "kmers", "kmers_invalid", "kmers_bad", "kmers_kept")   # pf_maskcount_stats


class ReadsRefused(RuntimeError, ValueError):
    """what count_fastq, trim_fastq, trim_fastq_pair, run_reads and run_multi_reads raise for a refusal of a call with gz=True, worded as the
    command words it (without gz= they raise RuntimeError, as before)"""


class FilterOpts(C.Structure):   # pf_filter_opts (include/ploidyfrost_hip.h)
    _fields_ = [("simple", C.c_int), ("indel", C.c_int), ("snp", C.c_int), ("low", C.c_longlong), ("up", C.c_longlong),
                ("num", C.c_longlong), ("distance", C.c_longlong), ("size", C.c_longlong), ("frequency", C.c_double)]


class FilterMultiOpts(C.Structure):   # pf_filter_multi_opts
    _fields_ = FilterOpts._fields_ + [("color", C.c_longlong), ("cramer", C.c_double)]


def load_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    hipapi.load_library()  # device layer first (and torch's HIP runtime before it)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s is missing: build with `make -C ploidyfrost_amd/csrc`" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.pfh_open.restype = vp
    L.pfh_open.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_int]
    L.pfh_close.argtypes = [vp]
    L.pfh_last_error.restype = C.c_char_p
    L.pfh_last_error.argtypes = [vp]
    L.pfh_set_output_dir.argtypes = [vp, C.c_char_p]
    L.pfh_set_write_files.argtypes = [vp, C.c_int]
    L.pfh_set_threads.argtypes = [vp, C.c_uint32]
    L.pfh_set_batch_bubbles.argtypes = [vp, C.c_uint64]
    L.pfh_set_align_pieces.argtypes = [vp, C.c_uint64]
    L.pfh_set_reference_threads.argtypes = [vp, C.c_uint32]
    L.pfh_set_overlap_output.argtypes = [vp, C.c_int]
    L.pfh_set_third_tier_on_host.argtypes = [vp, C.c_int]
    L.pfh_set_unitig_id.argtypes = [vp, C.c_char_p]
    L.pfh_find_superbubbles.argtypes = [vp, C.c_char_p]
    L.pfh_ploidy_estimation.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    L.pfh_get_times.argtypes = [vp, C.POINTER(Times)]
    L.pfh_r_format_double.restype = C.c_uint64
    L.pfh_r_format_double.argtypes = [C.c_double, C.c_char_p, C.c_uint64]
    L.pfh_load_trace.restype = C.c_uint64
    L.pfh_load_trace.argtypes = [C.c_char_p, C.c_uint64, C.c_int]
    L.pfh_device_ctx.restype = vp
    L.pfh_device_ctx.argtypes = [vp]
    L.pfh_state.argtypes = [vp, vp, vp, vp]
    L.pfh_last_allele_frequency.restype = C.c_void_p
    L.pfh_last_allele_frequency.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.pfh_open_colored.restype = vp
    L.pfh_open_colored.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_int]
    L.pfh_num_colors.restype = C.c_uint32
    L.pfh_num_colors.argtypes = [vp]
    L.pfh_ploidy_estimation_colored.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_uint32]
    L.pfh_colors_open.restype = vp
    L.pfh_colors_open.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32]
    L.pfh_colors_close.argtypes = [vp]
    L.pfh_colors_count.restype = C.c_uint32
    L.pfh_colors_count.argtypes = [vp]
    L.pfh_colors_unitigs.restype = C.c_uint32
    L.pfh_colors_unitigs.argtypes = [vp]
    L.pfh_colors_name.restype = C.c_char_p
    L.pfh_colors_name.argtypes = [vp, C.c_uint32]
    L.pfh_colors_unitig.restype = C.c_uint64
    L.pfh_colors_unitig.argtypes = [vp, C.c_uint32, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.pfh_gfa_abundant_kmers.restype = C.c_uint64
    L.pfh_gfa_abundant_kmers.argtypes = [C.c_char_p]
    L.pfh_gfa_numbering_replays.restype = C.c_uint32
    L.pfh_gfa_numbering_replays.argtypes = [C.c_char_p]
    L.pfh_gfa_minimizer_counts.restype = C.c_uint64
    L.pfh_gfa_minimizer_counts.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64]
    L.pfh_gfa_write_unitig_ids.restype = C.c_int
    L.pfh_gfa_write_unitig_ids.argtypes = [C.c_char_p, C.c_char_p]
    L.pfh_gfa_write_unitig_ids_given_inputs.restype = C.c_int
    L.pfh_gfa_write_unitig_ids_given_inputs.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.pfh_gfa_write_unitig_ids_given_arrays.restype = C.c_int
    L.pfh_gfa_write_unitig_ids_given_arrays.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    u32, u64 = C.c_uint32, C.c_uint64
    L.pfh_find_shard.argtypes = [vp, u32, u32]
    L.pfh_shard_records.restype = vp
    L.pfh_shard_records.argtypes = [vp, C.POINTER(u64)]
    L.pfh_shard_pool.restype = vp
    L.pfh_shard_pool.argtypes = [vp, C.POINTER(u64)]
    L.pfh_find_replay.argtypes = [vp, C.c_char_p, u32, vp, vp, vp, C.c_int, vp, vp, vp]
    L.pfh_set_replay_threads.argtypes = [vp, C.c_int]
    L.pfh_set_replay_threads.restype = None
    L.pfh_set_write_super_bubble.argtypes = [vp, C.c_int]
    L.pfh_set_write_super_bubble.restype = None
    L.pfh_ploidy_select.argtypes = [vp, C.c_int, C.c_int, C.POINTER(u64)]
    L.pfh_ploidy_select_colored.argtypes = [vp, vp, vp, C.c_int, C.POINTER(u64)]
    L.pfh_ploidy_align.argtypes = [vp, u64, u64, C.POINTER(u64)]
    L.pfh_ploidy_text.argtypes = [vp, u64, vp, vp]
    L.pfh_ploidy_write.argtypes = [vp, C.c_char_p, vp, vp, C.c_int]
    L.pfh_host_walk_range.restype = u64
    L.pfh_host_walk_range.argtypes = [vp, vp, u32, u32, u32, vp, u64, vp, u64, C.POINTER(u64)]
    L.pfh_replay_open.restype = vp
    L.pfh_replay_open.argtypes = [u32, u32]
    L.pfh_replay_close.argtypes = [vp]
    L.pfh_replay_apply.argtypes = [vp, vp, u64, vp]
    L.pfh_replay_apply_parallel.argtypes = [vp, vp, u64, vp, C.c_uint32]
    L.pfh_replay_apply_parallel.restype = C.c_int
    L.pfh_side_components.argtypes = [vp, u64, vp, C.c_uint32, vp]
    L.pfh_side_components.restype = None
    L.pfh_replay_check_footprints.argtypes = [vp, u64, vp, C.c_uint32, C.c_uint32, u64, C.POINTER(u64)]
    L.pfh_replay_check_footprints.restype = u64
    L.pfh_colors_check_footprints.argtypes = [vp, vp, vp, u64, vp, C.c_uint32, u64, C.POINTER(u64)]
    L.pfh_colors_check_footprints.restype = u64
    L.pfh_replay_state.argtypes = [vp, vp, vp, vp]
    L.pfh_bifrost_kmer_hash.restype = C.c_uint64
    L.pfh_bifrost_kmer_hash.argtypes = [C.c_uint64, C.c_uint64]
    d = C.c_double
    L.pfh_set_model.argtypes = [vp, C.c_int, d, C.c_int, C.c_int, d, d, C.c_int32, d, C.c_int]
    L.pfh_model_values.restype = u64
    L.pfh_model_values.argtypes = [vp, vp, u64]
    L.pfh_model_fit.argtypes = [vp, u32, vp, vp, vp, C.POINTER(d), C.POINTER(d), C.POINTER(u32)]
    L.pfh_model_ploidy.restype = d
    L.pfh_model_ploidy.argtypes = [vp]
    L.pfh_text_bytes_fetched.restype = u64
    L.pfh_text_bytes_fetched.argtypes = [vp]
    L.pfh_model_rows.argtypes = [C.c_int, d, C.POINTER(C.c_char_p), C.POINTER(u64), vp, u64, C.POINTER(u64), C.c_char_p, u64]
    L.pfh_set_filter.restype = C.c_int
    L.pfh_set_filter.argtypes = [vp, C.POINTER(FilterOpts)]
    L.pfh_filter_rows.restype = C.c_int
    L.pfh_filter_rows.argtypes = [C.c_int, d, C.POINTER(FilterOpts), C.POINTER(C.c_char_p), C.POINTER(u64), vp, u64, C.POINTER(u64), C.c_char_p, u64]
    L.pfh_set_filter_multi.restype = C.c_int
    L.pfh_set_filter_multi.argtypes = [vp, C.POINTER(FilterMultiOpts), C.c_int]
    L.pfh_filter_rows_multi.restype = C.c_int
    L.pfh_filter_rows_multi.argtypes = [C.c_int, d, C.POINTER(FilterMultiOpts), C.POINTER(C.c_char_p), C.POINTER(u64), vp, u64, C.POINTER(u64), C.c_char_p, u64]
    L.pfh_model_color_count.restype = u32
    L.pfh_model_color_count.argtypes = [vp]
    L.pfh_model_color_at.restype = C.c_int
    L.pfh_model_color_at.argtypes = [vp, u32]
    L.pfh_model_color_values.restype = u64
    L.pfh_model_color_values.argtypes = [vp, C.c_int, vp, u64]
    L.pfh_model_color_fit.argtypes = [vp, C.c_int, u32, vp, vp, vp, C.POINTER(d), C.POINTER(d), C.POINTER(u32)]
    L.pfh_model_color_ploidy.restype = d
    L.pfh_model_color_ploidy.argtypes = [vp, C.c_int]
    L.pfh_set_density.argtypes = [vp, u32, d]
    L.pfh_model_density_points.restype = u32
    L.pfh_model_density_points.argtypes = [vp, C.c_int]
    L.pfh_model_density.argtypes = [vp, vp, vp, vp]
    L.pfh_model_color_density.argtypes = [vp, C.c_int, vp, vp, vp]
    L.pfh_kmc_histogram.argtypes = [C.c_char_p, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.pfh_cutoffs_from_rows.argtypes = [vp, u64, d, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pfh_set_auto_cutoffs.argtypes = [vp, d]
    L.pfh_cutoffs.restype = u32
    L.pfh_cutoffs.argtypes = [vp, vp, vp, u32]
    L.pfh_mask_fastq.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), u32, C.c_char_p, u32, u32, C.c_int, u64, C.c_int, vp, C.POINTER(u32)]
    L.pfh_mask_read.restype = u64
    L.pfh_mask_read.argtypes = [vp, u64, u32, vp, u32, u32, vp]
    L.pfh_mask_index_fastq.argtypes = [vp, u64, C.c_int, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, vp, u64]
    L.pfh_mask_clause_text.restype = C.c_char_p
    L.pfh_mask_clause_text.argtypes = [C.c_int]
    L.pfh_count_fastq.argtypes = [C.POINTER(C.c_char_p), u32, C.c_char_p, u32, u64, u64, u64, C.c_int, C.c_char_p, u64, u64, C.c_int, vp]
    L.pfh_mask_fastq_counted.argtypes = [C.POINTER(C.c_char_p), u32, C.c_char_p, u32, u64, u64, u64, C.c_int, C.c_char_p, u32, u32, C.c_int, u64, C.c_int,
                                         vp, C.POINTER(u32)]
    L.pfh_count_reads_host.argtypes = [vp, vp, vp, u64, u32, C.c_int, u64, u64, u64, vp, vp, u64, C.POINTER(u64), vp]
    L.pfh_count_encode_kmc1.argtypes = [vp, vp, u64, u32, u64, u64, u64, C.c_int, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64)]
    L.pfh_count_counter_bytes.restype = u32
    L.pfh_count_counter_bytes.argtypes = [u64, u64]
    L.pfh_count_lut_prefix_len.restype = u32
    L.pfh_count_lut_prefix_len.argtypes = [u32]
    L.pfh_build_fastq.argtypes = [C.POINTER(C.c_char_p), u32, C.c_char_p, u32, C.c_int32, C.c_int, C.c_int, u64, u64, C.c_int, vp, vp]
    L.pfh_unitig_build_host.argtypes = [vp, u64, u32, C.c_int32, C.c_int, C.c_int, vp, u64, C.POINTER(u64), vp]
    L.pfh_run_defaults.restype = None
    L.pfh_run_defaults.argtypes = [C.POINTER(RunOptions)]
    L.pfh_run_fastq.argtypes = [C.POINTER(C.c_char_p), u32, C.c_char_p, C.POINTER(RunOptions), C.c_int, vp]
    L.pfh_run_multi_fastq.argtypes = [C.POINTER(C.c_char_p), vp, u32, C.POINTER(C.c_char_p), C.c_char_p, C.POINTER(RunOptions), C.POINTER(FilterMultiOpts),
                                      C.c_int, C.c_int, vp, vp]
    L.pfh_union_host.argtypes = [vp, vp, u32, vp, C.POINTER(C.c_uint64)]
    L.pfh_count_masked_host.argtypes = [vp, vp, vp, u64, u32, vp, u32, u32, vp, vp, u64, C.POINTER(u64), vp]
    L.pfh_unitig_no_room_text.restype = C.c_char_p
    L.pfh_unitig_no_room_text.argtypes = [u64, u64, u64]
    L.pfh_build_colored_fastq.argtypes = [C.POINTER(C.c_char_p), u32, C.c_char_p, u32, C.c_int32, C.c_int, C.c_int, u32, u64, u64, C.c_int, vp, vp, vp,
                                          C.POINTER(u64), vp]
    L.pfh_build_colored_host.argtypes = [C.POINTER(C.c_char_p), vp, u64, u32, C.POINTER(C.c_char_p), u32, C.c_int32, C.c_int, C.c_int, u32, vp, u64,
                                         C.POINTER(u64), vp, u64, C.POINTER(u64), vp, vp]
    L.pfh_bfg_colors_bytes.argtypes = [vp, vp, vp, vp, vp, u64, u32, u32, C.POINTER(C.c_char_p), u32, vp, u64, C.POINTER(u64)]
    L.pfh_color_no_room_text.restype = C.c_char_p
    L.pfh_color_no_room_text.argtypes = [u64, u64, u64, u64]
    L.pfh_count_cut_text.restype = C.c_char_p
    L.pfh_count_cut_text.argtypes = [C.c_int]
    L.pfh_trim_fastq.argtypes = [C.POINTER(C.c_char_p), u32, C.c_char_p, vp, u32, u32, C.c_char_p, u64, C.c_int, vp]
    L.pfh_trim_fastq_pair.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), vp, u32, u32, C.c_char_p, u64, C.c_int, vp]
    L.pfh_trim_parse_step.argtypes = [C.c_char_p, vp]
    L.pfh_trim_refusal_text.restype = C.c_char_p
    L.pfh_trim_refusal_text.argtypes = [C.c_int]
    L.pfh_trim_read.argtypes = [vp, u64, vp, u32, u32, C.POINTER(u32), C.POINTER(u32)]
    L.pfh_trim_fastq_chunk.argtypes = [vp, u64, C.c_int, vp, u32, u32, vp, C.POINTER(u64), C.POINTER(u64), vp, vp, u64, C.POINTER(u64), vp, C.POINTER(u64)]
    L.pfh_run_fastq_trimmed.argtypes = [C.POINTER(C.c_char_p), u32, C.c_int, vp, u32, u32, C.c_char_p, C.POINTER(RunOptions), C.c_int, vp, vp]
    L.pfh_run_multi_fastq_trimmed.argtypes = [C.POINTER(C.c_char_p), vp, vp, u32, C.POINTER(C.c_char_p), vp, u32, u32, C.c_char_p, C.POINTER(RunOptions),
                                              C.POINTER(FilterMultiOpts), C.c_int, C.c_int, vp, vp, vp]
    L.pfh_trim_table_chunk.argtypes = [vp, u64, C.c_int, vp, u32, u32, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, C.POINTER(u64)]
    L.pfh_trim_table_chunk_pair.argtypes = [vp, u64, vp, u64, C.c_int, vp, u32, u32, C.POINTER(vp), C.POINTER(vp), u64, C.POINTER(u64), C.POINTER(u64),
                                            C.POINTER(u64), vp, C.POINTER(u64)]
    L.pfh_trim_table_clause_text.restype = C.c_char_p
    L.pfh_trim_table_clause_text.argtypes = [C.c_int]
    L.pfh_reads_gz.restype = None
    L.pfh_reads_gz.argtypes = [C.c_int]
    L.pfh_reads_gz_out.restype = None
    L.pfh_reads_gz_out.argtypes = [C.c_int]
    L.pfh_reads_adapters.restype = None
    L.pfh_reads_adapters.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32]
    L.pfh_reads_adapters_report.restype = None
    L.pfh_reads_adapters_report.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p]
    L.pfh_clip_parse_adapters.restype = C.c_int
    L.pfh_clip_parse_adapters.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint64)]
    L.pfh_reads_dedup.restype = None
    L.pfh_reads_dedup.argtypes = [C.c_int, C.c_uint32, C.c_uint64]
    L.pfh_reads_dedup_report.restype = None
    L.pfh_reads_dedup_report.argtypes = [C.c_void_p]
    L.pfh_dedup_key.restype = C.c_int
    L.pfh_dedup_key.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p]
    L.pfh_dedup_units.restype = C.c_int
    L.pfh_dedup_units.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.pfh_trim_fastq_chunk_dedup.restype = C.c_int
    L.pfh_trim_fastq_chunk_dedup.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p,
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                             C.c_void_p, C.POINTER(C.c_uint64)]
    L.pfh_trim_fastq_pair_chunk_dedup.restype = C.c_int
    L.pfh_trim_fastq_pair_chunk_dedup.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                  C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                  C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64)]
    L.pfh_reads_report.restype = None
    L.pfh_reads_report.argtypes = [C.c_char_p]
    L.pfh_qc_fastq.restype = C.c_int
    L.pfh_qc_fastq.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint64, C.c_int]
    L.pfh_qc_fastq_chunk.restype = C.c_int
    L.pfh_qc_fastq_chunk.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.pfh_qc_report_text.restype = C.c_int
    L.pfh_qc_report_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.pfh_hetpairs_host.restype = C.c_int
    L.pfh_hetpairs_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
    L.pfh_smudge_report_text.restype = C.c_int
    L.pfh_smudge_report_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.pfh_smudge_of.restype = C.c_int
    L.pfh_smudge_of.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.pfh_smudge.restype = C.c_int
    L.pfh_smudge.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int,
                             C.c_double, C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
    L.pfh_reads_smudge.restype = None
    L.pfh_reads_smudge.argtypes = [C.c_int, C.c_int64, C.c_char_p]
    L.pfh_reads_smudge_result.restype = None
    L.pfh_reads_smudge_result.argtypes = [C.c_void_p]
    L.pfh_qc_phred_hint.restype = C.c_uint32
    L.pfh_qc_phred_hint.argtypes = [C.c_uint64, C.c_uint64]
    L.pfh_reads_adapter_pairs.restype = None
    L.pfh_reads_adapter_pairs.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    L.pfh_reads_adapters_pair_report.restype = None
    L.pfh_reads_adapters_pair_report.argtypes = [C.POINTER(C.c_uint32), C.c_void_p]
    L.pfh_clip_parse_adapter_pairs.restype = C.c_int
    L.pfh_clip_parse_adapter_pairs.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p,
                                               C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.pfh_clip_pair.restype = C.c_int
    L.pfh_clip_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p,
                                C.c_void_p, C.c_void_p]
    L.pfh_trim_fastq_pair_chunk_clip.restype = C.c_int
    L.pfh_trim_fastq_pair_chunk_clip.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.pfh_clip_refusal_text.restype = C.c_char_p
    L.pfh_clip_refusal_text.argtypes = [C.c_int]
    L.pfh_clip_read.restype = C.c_int
    L.pfh_clip_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.pfh_trim_fastq_chunk_clip.restype = C.c_int
    L.pfh_trim_fastq_chunk_clip.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p,
                                            C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.pfh_reads_fasta.restype = None
    L.pfh_reads_fasta.argtypes = [C.c_int]
    L.pfh_fasta_index.restype = C.c_int
    L.pfh_fasta_index.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p,
                                  C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    L.pfh_fasta_clause_text.restype = C.c_char_p
    L.pfh_fasta_clause_text.argtypes = [C.c_int]
    L.pfh_inflate_parse_member.argtypes = [vp, u64, vp]
    L.pfh_inflate_member.argtypes = [vp, u32, vp, u32, C.POINTER(u32), vp]
    L.pfh_inflate_bgzf_member.argtypes = [vp, u64, vp, C.POINTER(u32), vp]
    L.pfh_inflate_crc32.restype = u32
    L.pfh_inflate_crc32.argtypes = [vp, u64]
    L.pfh_inflate_crc32_sliced.restype = u32
    L.pfh_inflate_crc32_sliced.argtypes = [vp, u32, u32]
    L.pfh_inflate_file_clause.argtypes = [vp, u64, u64, C.POINTER(C.c_int)]
    L.pfh_inflate_clause_text.restype = C.c_char_p
    L.pfh_inflate_clause_text.argtypes = [C.c_int]
    L.pfh_deflate_member.restype = C.c_int64
    L.pfh_deflate_member.argtypes = [vp, u32, vp, u64, vp]
    L.pfh_deflate_bound.restype = u64
    L.pfh_deflate_bound.argtypes = [u64, u32]
    L.pfh_gunzip_header.argtypes = [vp, u64, C.POINTER(u64)]
    L.pfh_gunzip_file_kind.argtypes = [vp, u64, u64, C.POINTER(C.c_int)]
    L.pfh_gunzip_candidate.argtypes = [vp, u64, u64]
    L.pfh_gunzip_call.argtypes = [vp, u64, u64, vp, u32, u32, vp, u64, vp, vp, vp]
    L.pfh_gunzip_file.argtypes = [vp, u64, u32, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]
    L.pfh_gunzip_clause_text.restype = C.c_char_p
    L.pfh_gunzip_clause_text.argtypes = [C.c_int]
    _lib = L
    return L


def host_walk_range(succ: np.ndarray, pred: np.ndarray, u0: int, u1: int):
    """Records + vertex pool of every candidate entrance on unitigs [u0, u1) from the host walker alone (no device)."""
    L = load_library()
    succ = np.ascontiguousarray(succ, dtype=np.uint32).reshape(-1, 4)
    pred = np.ascontiguousarray(pred, dtype=np.uint32).reshape(-1, 4)
    n = succ.shape[0] // 2
    used = C.c_uint64()
    cnt = int(((succ[2 * u0: 2 * u1] != hipapi.NONE).sum(axis=1) > 1).sum())
    rec = np.zeros(max(cnt, 1), dtype=hipapi.BFS_RECORD)
    cap = 64 * max(cnt, 1) + 1024
    while True:
        pool = np.zeros(cap, dtype=np.uint32)
        got = L.pfh_host_walk_range(succ.ctypes.data, pred.ctypes.data, n, u0, u1, rec.ctypes.data, len(rec), pool.ctypes.data, cap, C.byref(used))
        if got != 0xFFFFFFFFFFFFFFFF:
            return rec[:got].copy(), pool[: used.value].copy()
        if used.value <= cap:
            raise RuntimeError("pfh_host_walk_range failed")
        cap = used.value + 1024


def side_components(records: np.ndarray, pool: np.ndarray, n_unitigs: int) -> np.ndarray:
    """component label of every record's entrance side (host union-find over the records' footprints)"""
    L = load_library()
    records = np.ascontiguousarray(records)
    pool = np.ascontiguousarray(pool, dtype=np.uint32) if len(pool) else np.zeros(1, dtype=np.uint32)
    labels = np.zeros(len(records), dtype=np.uint32)
    L.pfh_side_components(records.ctypes.data if len(records) else None, len(records), pool.ctypes.data, n_unitigs, labels.ctypes.data)
    return labels


def check_footprints(records: np.ndarray, pool: np.ndarray, n_unitigs: int, complex_size: int = 8, slice_len: int = 0):
    """(accesses outside the running record's component, index of the first such record or None)"""
    L = load_library()
    records = np.ascontiguousarray(records)
    pool = np.ascontiguousarray(pool, dtype=np.uint32) if len(pool) else np.zeros(1, dtype=np.uint32)
    first = C.c_uint64()
    bad = L.pfh_replay_check_footprints(records.ctypes.data if len(records) else None, len(records), pool.ctypes.data, n_unitigs,
                                        complex_size, slice_len, C.byref(first))
    return int(bad), (None if first.value == 0xFFFFFFFFFFFFFFFF else int(first.value))


class Replay:
    """The commit replay on a bare MyUnitig state (no device): shards of records in, state out."""

    def __init__(self, n_unitigs: int, complex_size: int = 8):
        self.L = load_library()
        self.n = n_unitigs
        self.h = self.L.pfh_replay_open(n_unitigs, complex_size)

    def apply(self, records: np.ndarray, pool: np.ndarray, threads: int = 0):
        """threads > 0: the parallel replay (components of record footprints side by side); 0: the sequential one"""
        records = np.ascontiguousarray(records)
        pool = np.ascontiguousarray(pool, dtype=np.uint32) if len(pool) else np.zeros(1, dtype=np.uint32)
        if threads:
            rc = self.L.pfh_replay_apply_parallel(self.h, records.ctypes.data if len(records) else None, len(records), pool.ctypes.data, threads)
        else:
            rc = self.L.pfh_replay_apply(self.h, records.ctypes.data if len(records) else None, len(records), pool.ctypes.data)
        if rc:
            raise RuntimeError("pfh_replay_apply: %d (shards must arrive in entrance order)" % rc)

    def state(self):
        f = np.empty(self.n, dtype=np.uint8)
        p = np.empty(self.n, dtype=np.uint32)
        m = np.empty(self.n, dtype=np.uint32)
        self.L.pfh_replay_state(self.h, f.ctypes.data, p.ctypes.data, m.ctypes.data)
        return f, p, m

    def close(self):
        if getattr(self, "h", None):
            self.L.pfh_replay_close(self.h)
            self.h = None


class Colors:
    """The product's reading of a colored graph's .bfg_colors (host only, no GPU)."""

    def __init__(self, gfa: str, colors: str, threads: int = 1):
        self.L = load_library()
        self.h = self.L.pfh_colors_open(gfa.encode(), colors.encode(), threads)
        if not self.h:
            raise RuntimeError("ploidyfrost host layer: " + self.L.pfh_last_error(None).decode())
        self.n_colors = self.L.pfh_colors_count(self.h)
        self.n = self.L.pfh_colors_unitigs(self.h)
        self.names = [self.L.pfh_colors_name(self.h, c).decode() for c in range(self.n_colors)]

    def close(self):
        if getattr(self, "h", None):
            self.L.pfh_colors_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check_footprints(self, succ: np.ndarray, records: np.ndarray, pool: np.ndarray, complex_size: int = 8, slice_len: int = 0):
        """the footprint check of the parallel commits with the colored gate: (accesses outside the component, first such record)"""
        succ = np.ascontiguousarray(succ, dtype=np.uint32)
        records = np.ascontiguousarray(records)
        pool = np.ascontiguousarray(pool, dtype=np.uint32) if len(pool) else np.zeros(1, dtype=np.uint32)
        first = C.c_uint64()
        bad = self.L.pfh_colors_check_footprints(self.h, succ.ctypes.data, records.ctypes.data if len(records) else None, len(records), pool.ctypes.data,
                                                 complex_size, slice_len, C.byref(first))
        return int(bad), (None if first.value == 0xFFFFFFFFFFFFFFFF else int(first.value))

    def unitig(self, u: int):
        """(presence[colour, kmer] uint8, UnitigColors::size(um), n_full_enc)"""
        km, nf = C.c_uint32(), C.c_uint32()
        self.L.pfh_colors_unitig(self.h, u, None, C.byref(km), C.byref(nf))
        out = np.zeros((self.n_colors, km.value), dtype=np.uint8)
        sz = self.L.pfh_colors_unitig(self.h, u, out.ctypes.data, C.byref(km), C.byref(nf))
        return out, sz, nf.value


MODEL_SOURCES = {"cov": 0, "fre": 1}


def model_rows(source: str, texts, q: float = 0.0) -> np.ndarray:
    """The model's values as the shared row rule (csrc/pf_model_rows.hpp, what the device kernels run) reads them from text in
    host memory: source "cov" with the bytes of (_bicov, _tricov, _tetracov), source "fre" with those of _allele_frequency.
    No device.  RuntimeError with the readers' wording for a coverage row that sums to 0 or a token that is no number."""
    L = load_library()
    if isinstance(texts, (bytes, bytearray)):
        texts = [texts]
    texts = [bytes(t) for t in texts]
    want = 3 if source == "cov" else 1
    if len(texts) != want:
        raise ValueError("source %s takes %d texts" % (source, want))
    ptrs = (C.c_char_p * 3)(*(texts + [None] * (3 - len(texts))))
    lens = (C.c_uint64 * 3)(*([len(t) for t in texts] + [0] * (3 - len(texts))))
    n = C.c_uint64()
    err = C.create_string_buffer(512)
    cap = sum(len(t) for t in texts) + 2
    out = np.zeros(cap, dtype=np.float64)
    if L.pfh_model_rows(MODEL_SOURCES[source], q, ptrs, lens, out.ctypes.data, cap, C.byref(n), err, len(err)) != 0:
        raise RuntimeError(err.value.decode() or "pfh_model_rows failed")
    return out[: n.value].copy()


def filter_opts(simple=False, low=0, up=10000, indel=False, snp=False, num=10000, distance=-1, size=10000, frequency=0.05) -> FilterOpts:
    """the options of `ploidyfrost filter` (-S -l -u -I -P -n -d -s -q) with the script's defaults"""
    return FilterOpts(int(simple), int(indel), int(snp), int(low), int(up), int(num), int(distance), int(size), float(frequency))


def filter_multi_opts(color=-1, cramer=0.0, **opts) -> FilterMultiOpts:
    """the options of `ploidyfrost filter-multi`: those of filter_opts plus -c colour (-1: all) and -v Cramer's V"""
    o = filter_opts(**opts)
    return FilterMultiOpts(*[getattr(o, n) for n, _ in FilterOpts._fields_], int(color), float(cramer))


def filter_rows(source: str, texts, q: float = 0.0, multi: bool = False, **opts) -> np.ndarray:
    """The model's values behind a row filter, as the shared rule (csrc/pf_filter_rows.hpp, what the device kernels run) reads
    them from the bytes of (_bicov, _tricov, _tetracov, _pentacov): what `filter` with **opts (see filter_opts) followed by
    `model -f` (source "cov") / `model -g <filtered>_allele_frequency.txt` ("fre") with -q q reads.  No device.  RuntimeError
    with the wording of the one-command run for what it refuses.  multi=True: the tables of a colored run and `filter-multi`,
    with color= (-1: all) and cramer= among the options."""
    L = load_library()
    texts = [bytes(t) for t in texts]
    if len(texts) != 4:
        raise ValueError("four texts: bi, tri, tetra, penta")
    ptrs = (C.c_char_p * 4)(*texts)
    lens = (C.c_uint64 * 4)(*[len(t) for t in texts])
    o = filter_multi_opts(**opts) if multi else filter_opts(**opts)
    n = C.c_uint64()
    err = C.create_string_buffer(1024)
    cap = sum(len(t) for t in texts) + 2
    out = np.zeros(cap, dtype=np.float64)
    fn = L.pfh_filter_rows_multi if multi else L.pfh_filter_rows
    if fn(MODEL_SOURCES[source], q, C.byref(o), ptrs, lens, out.ctypes.data, cap, C.byref(n), err, len(err)) != 0:
        raise RuntimeError(err.value.decode() or "pfh_filter_rows failed")
    return out[: n.value].copy()


def kmc_histogram(prefix: str):
    """(min_count, rows): the k-mer histogram of a KMC database, counted on the device from the decoded counters (K-HIST).
    rows[r] = records whose count is min_count + r, up to min(max_count, the counter's range, 2^20 - 1), zero rows included."""
    L = load_library()
    n, mn = C.c_uint64(), C.c_uint64()
    if L.pfh_kmc_histogram(prefix.encode(), None, 0, C.byref(n), C.byref(mn)):
        raise RuntimeError(L.pfh_last_error(None).decode())
    rows = np.zeros(n.value, dtype=np.uint64)
    if L.pfh_kmc_histogram(prefix.encode(), rows.ctypes.data, n.value, C.byref(n), C.byref(mn)):
        raise RuntimeError(L.pfh_last_error(None).decode())
    return int(mn.value), rows


def cutoffs_from_rows(rows, q: float = 0.998):
    """(lower, upper) of the reference's cutoffL / cutoffU (src/Main.cpp:200-277) on the second column of a histogram, in file
    order; lower is the value before the callers' max(10, lower).  Fewer than two rows: ValueError with the reference's words."""
    L = load_library()
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    lo, up = C.c_int(), C.c_int()
    rc = L.pfh_cutoffs_from_rows(r.ctypes.data, len(r), q, C.byref(lo), C.byref(up))
    if rc:
        raise ValueError("Error: Histogram File is badly Formatted.")
    return lo.value, up.value


MASK_STATS_FIELDS = ("reads", "reads_changed", "bases", "bases_masked", "kmers", "kmers_bad")   # pf_mask_stats
MASK_CLAUSES = ("none", "header", "plus", "quality", "line_count", "fasta", "gzip", "same_path")      # pf_mask::Clause, in its order


def mask_fastq(db: str, inputs, out: str, lower=None, upper=None, auto: bool = False, chunk_bytes: int = 0, gz_out: bool = False) -> dict:
    """`ploidyfrost mask` (pfh_mask_fastq): the reads of the FASTQ file(s) `inputs`, one after the other, with every base of every
    k-mer whose count in the KMC database `db` lies outside [lower, upper] replaced by N, written to `out`.  auto: lower =
    max(10, cutoffL) of the database's own histogram.  Returns the statistics plus "lower" (the threshold applied).  A refusal
    raises RuntimeError with the input's path and the 1-based record number; nothing is left under `out`.  gz_out (`--gz-out`): `out` is
    written as blocked gzip, deflated on the device (K-DEFLATE)."""
    L = load_library()
    if isinstance(inputs, (str, bytes, os.PathLike)):
        inputs = [inputs]
    if auto == (lower is not None):
        raise ValueError("mask_fastq: either lower=L or auto=True")
    paths = (C.c_char_p * max(len(inputs), 1))(*[os.fsencode(p) for p in inputs])
    stats = np.zeros(len(MASK_STATS_FIELDS), dtype=np.uint64)
    used = C.c_uint32()
    L.pfh_reads_gz_out(int(gz_out))
    rc = L.pfh_mask_fastq(os.fsencode(db), paths, len(inputs), os.fsencode(out), 0 if lower is None else int(lower),
                          0xFFFFFFFF if upper is None else int(upper), int(auto), int(chunk_bytes), 0, stats.ctypes.data, C.byref(used))
    if rc:
        raise RuntimeError(L.pfh_last_error(None).decode())
    d = {f: int(v) for f, v in zip(MASK_STATS_FIELDS, stats)}
    d["lower"] = used.value
    return d


def mask_read(seq: bytes, k: int, counters, lower: int, upper: int = 0xFFFFFFFF):
    """(masked read, bytes changed): the rule of `mask` on one read with the counters given (pfh_mask_read; no device)"""
    L = load_library()
    n = len(seq)
    c = np.ascontiguousarray(counters, dtype=np.uint32)
    assert len(c) >= max(n - k + 1, 0)
    src = np.frombuffer(bytes(seq), dtype=np.uint8)
    out = np.zeros(n, dtype=np.uint8)
    changed = L.pfh_mask_read(src.ctypes.data if n else None, n, k, c.ctypes.data if len(c) else None, lower, upper, out.ctypes.data if n else None)
    return out.tobytes(), int(changed)


def mask_index_fastq(text: bytes, final: bool = True):
    """The FASTQ index of a chunk by the shared rule header, on the host (pfh_mask_index_fastq): dict with clause (a name of
    MASK_CLAUSES), message, bad_record, bytes_used, n_records, read_off, read_len"""
    L = load_library()
    src = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(src)
    cap = text.count(b"\n") // 4 + 2
    off, ln = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
    used, recs, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
    clause = L.pfh_mask_index_fastq(src.ctypes.data if n else None, n, int(final), C.byref(used), C.byref(recs), C.byref(bad), off.ctypes.data, ln.ctypes.data, cap)
    return dict(clause=MASK_CLAUSES[clause], message=L.pfh_mask_clause_text(clause).decode(), bad_record=bad.value, bytes_used=used.value,
                n_records=recs.value, read_off=off[: recs.value].copy(), read_len=ln[: recs.value].copy())


TRIM_STATS_FIELDS = ("reads", "kept", "dropped", "bases", "bases_kept", "both", "only1", "only2", "neither")   # pf_trim_stats
TRIM_STEP = np.dtype([("kind", "<u4"), ("a", "<u4"), ("b", "<u4")])                                               # pf_trim_step
TRIM_REFUSALS = ("none", "unknown", "field", "range", "too_many", "no_step", "phred")                             # pf_trim::Refusal, in its order


def trim_parse_steps(steps) -> np.ndarray:
    """Trimmomatic's words ("LEADING:10", "SLIDINGWINDOW:3:20", ...; a list or one string) as a TRIM_STEP array, by the parser of
    the rule header (pfh_trim_parse_step).  A word that is refused raises ValueError with the refusal's text; .refusal names it."""
    L = load_library()
    if isinstance(steps, np.ndarray) and steps.dtype == TRIM_STEP:
        return np.ascontiguousarray(steps)
    if isinstance(steps, str):
        steps = steps.split()
    out = np.zeros(len(steps), dtype=TRIM_STEP)
    for j, word in enumerate(steps):
        c = L.pfh_trim_parse_step(os.fsencode(word), out[j:].ctypes.data)
        if c:
            e = ValueError("trim: %s: %s" % (word, L.pfh_trim_refusal_text(c).decode()))
            e.refusal = TRIM_REFUSALS[c]
            raise e
    return out


def trim_read(qual: bytes, steps, phred: int = 33):
    """The rule of `trim` on one quality line (pfh_trim_read; no device): (b, e) of the kept interval, or None for a dropped read.
    Steps or a phred that are refused raise ValueError."""
    L = load_library()
    st = trim_parse_steps(steps)
    src = np.frombuffer(bytes(qual), dtype=np.uint8)
    b, e = C.c_uint32(), C.c_uint32()
    rc = L.pfh_trim_read(src.ctypes.data if len(src) else None, len(src), st.ctypes.data if len(st) else None, len(st), phred, C.byref(b), C.byref(e))
    if rc < 0:
        raise ValueError(L.pfh_last_error(None).decode())
    return (b.value, e.value) if rc else None


def trim_fastq_chunk(text: bytes, steps, phred: int = 33, final: bool = True):
    """What pf_trim_fastq gives for one chunk, by the host's plain restatement (pfh_trim_fastq_chunk; no device): dict with clause (a
    name of MASK_CLAUSES), bad_record, out, bytes_used, n_records, begin, len, stats."""
    L = load_library()
    st = trim_parse_steps(steps)
    src = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(src)
    out = np.zeros(n + 1, dtype=np.uint8)
    cap = n // 4 + 1
    begin, ln = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
    stats = np.zeros(len(TRIM_STATS_FIELDS), dtype=np.uint64)
    out_n, used, recs, bad = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    clause = L.pfh_trim_fastq_chunk(src.ctypes.data if n else None, n, int(final), st.ctypes.data if len(st) else None, len(st), phred, out.ctypes.data,
                                    C.byref(out_n), C.byref(used), begin.ctypes.data, ln.ctypes.data, cap, C.byref(recs), stats.ctypes.data, C.byref(bad))
    if clause < 0:
        raise ValueError(L.pfh_last_error(None).decode())
    return dict(clause=MASK_CLAUSES[clause], bad_record=bad.value, out=out[: out_n.value].tobytes(), bytes_used=used.value, n_records=recs.value,
                begin=begin[: recs.value].tolist(), len=ln[: recs.value].tolist(), stats={f: int(v) for f, v in zip(TRIM_STATS_FIELDS, stats)})


CLIP_STATS_FIELDS = ("reads_clipped", "reads_dropped", "bases_clipped", "candidates_scored")   # pf_clip_stats: each [file 1, file 2]
CLIP_REFUSALS = ("none", "not_fasta", "byte", "length", "too_many", "no_adapter", "seed", "score", "side", "pair_partner", "pair_lengths",
                 "too_many_pairs", "no_pair", "pair_score", "pair_min")   # pf_clip::Refusal, in its order
CLIP_MAX_ADAPTERS, CLIP_MAX_LEN = 64, 128
CLIP_MAX_PAIRS, CLIP_MAX_PAIR_READ = 8, 1024
CLIP_PAIR_STATS_FIELDS = ("pairs_clipped", "pairs_dropped", "pairs_too_long", "candidates_scored", "bases_clipped")   # pf_clip_pair_stats; the last is [file 1, file 2]


def _pair_stats_dict(raw) -> dict:
    out = {f: int(v) for f, v in zip(CLIP_PAIR_STATS_FIELDS[:4], raw[:4])}
    out["bases_clipped"] = [int(raw[4]), int(raw[5])]
    return out


def clip_parse_adapters(path_or_bytes, pairs: bool = False) -> dict:
    """The adapter file of `--adapters` by the parser of the rule header (pfh_clip_parse_adapters, csrc/pf_clip_rule.hpp; no device):
    dict with bases (the usable adapters one behind the other, upper case), off (n + 1 offsets), side (0 both files, 1, 2), n and
    skipped (the `Prefix` entries of palindrome mode, which is not built).  bytes are the file's text, anything else a path.  A file
    that is refused raises ValueError with the refusal's text and the 1-based record; .refusal names it, .bad_record holds the record.
    pairs=True (`--adapter-pairs`, pfh_clip_parse_adapter_pairs): the `Prefix<X>/1`, `Prefix<X>/2` entries are prefix pairs instead --
    the dict also holds prefix_bases, prefix_off (2 * n_pairs + 1 offsets: P1, P2 of every pair) and n_pairs; n may then be 0."""
    L = load_library()
    if isinstance(path_or_bytes, (bytes, bytearray)):
        text, where = bytes(path_or_bytes), "adapters"
    else:
        with open(path_or_bytes, "rb") as f:
            text = f.read()
        where = "adapters %s" % os.fsdecode(path_or_bytes)
    src = np.frombuffer(text, dtype=np.uint8)
    bases = np.zeros(CLIP_MAX_ADAPTERS * CLIP_MAX_LEN, dtype=np.uint8)
    off = np.zeros(CLIP_MAX_ADAPTERS + 1, dtype=np.uint32)
    side = np.zeros(CLIP_MAX_ADAPTERS, dtype=np.uint8)
    n, skipped, bad = C.c_uint32(), C.c_uint32(), C.c_uint64()
    if pairs:
        pbases = np.zeros(CLIP_MAX_PAIRS * 2 * CLIP_MAX_LEN, dtype=np.uint8)
        poff = np.zeros(2 * CLIP_MAX_PAIRS + 1, dtype=np.uint32)
        nq = C.c_uint32()
        c = L.pfh_clip_parse_adapter_pairs(src.ctypes.data if len(src) else None, len(src), bases.ctypes.data, len(bases), off.ctypes.data, side.ctypes.data,
                                           C.byref(n), pbases.ctypes.data, len(pbases), poff.ctypes.data, C.byref(nq), C.byref(bad))
    else:
        c = L.pfh_clip_parse_adapters(src.ctypes.data if len(src) else None, len(src), bases.ctypes.data, len(bases), off.ctypes.data, side.ctypes.data,
                                      C.byref(n), C.byref(skipped), C.byref(bad))
    if c:
        e = ValueError("%s: %s%s" % (where, "record %d: " % bad.value if bad.value else "", L.pfh_clip_refusal_text(c).decode()))
        e.refusal, e.bad_record = CLIP_REFUSALS[c], bad.value
        raise e
    out = dict(bases=bases[: off[n.value]].tobytes(), off=off[: n.value + 1].copy(), side=side[: n.value].copy(), n=n.value, skipped=skipped.value)
    if pairs:
        out.update(prefix_bases=pbases[: poff[2 * nq.value]].tobytes(), prefix_off=poff[: 2 * nq.value + 1].copy(), n_pairs=nq.value)
    return out


def clip_adapters(adapters) -> dict:
    """adapters as the clip calls take them: the dict of clip_parse_adapters, a path or the bytes of an adapter file, or a list of
    (sequence, side) pairs (nothing is checked there: the library refuses by name)."""
    if isinstance(adapters, dict):
        return adapters
    if isinstance(adapters, (list, tuple)):
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s, _ in adapters]
        off = np.zeros(len(seqs) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64) if seqs else []
        return dict(bases=b"".join(seqs), off=off, side=np.array([sd for _, sd in adapters], dtype=np.uint8), n=len(seqs), skipped=0)
    return clip_parse_adapters(adapters)


def clip_read(seq: bytes, qual: bytes, adapters, side: int = 1, seed: int = 2, score: int = 10, phred: int = 33, scored: bool = False):
    """The rule of `--adapters` on one read of file `side` (1 or 2) (pfh_clip_read; no device): the clip end -- len(seq) for an untouched
    read, 0 for a dropped one; scored=True: (clip end, the candidates whose seed held).  Values that are refused raise ValueError."""
    L = load_library()
    A = clip_adapters(adapters)
    s, q = np.frombuffer(bytes(seq), dtype=np.uint8), np.frombuffer(bytes(qual), dtype=np.uint8)
    if len(s) != len(q):
        raise ValueError("clip_read: the quality line is as long as the sequence line")
    bases = np.frombuffer(A["bases"], dtype=np.uint8)
    end, sc = C.c_uint32(), C.c_uint64()
    rc = L.pfh_clip_read(s.ctypes.data if len(s) else None, q.ctypes.data if len(q) else None, len(s), bases.ctypes.data if len(bases) else None,
                         A["off"].ctypes.data, A["side"].ctypes.data if A["n"] else None, A["n"], int(side), int(seed), int(score), int(phred),
                         C.byref(end), C.byref(sc))
    if rc < 0:
        raise ValueError(L.pfh_last_error(None).decode())
    return (end.value, sc.value) if scored else end.value


def trim_fastq_chunk_clip(text: bytes, steps, adapters, side: int = 1, seed: int = 2, score: int = 10, phred: int = 33, final: bool = True):
    """What pf_trim_fastq gives for one chunk while a clip is open, by the host's plain restatement (pfh_trim_fastq_chunk_clip; no
    device): the dict of trim_fastq_chunk and "clip" = the statistics of CLIP_STATS_FIELDS, each [file 1, file 2].  steps may be empty."""
    L = load_library()
    st = trim_parse_steps(steps) if len(steps) else np.zeros(0, dtype=TRIM_STEP)
    A = clip_adapters(adapters)
    bases = np.frombuffer(A["bases"], dtype=np.uint8)
    src = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(src)
    out = np.zeros(n + 1, dtype=np.uint8)
    cap = n // 4 + 1
    begin, ln = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
    stats = np.zeros(len(TRIM_STATS_FIELDS), dtype=np.uint64)
    clip = np.zeros((len(CLIP_STATS_FIELDS), 2), dtype=np.uint64)
    out_n, used, recs, bad = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    clause = L.pfh_trim_fastq_chunk_clip(src.ctypes.data if n else None, n, int(final), st.ctypes.data if len(st) else None, len(st), phred,
                                         bases.ctypes.data if len(bases) else None, A["off"].ctypes.data, A["side"].ctypes.data if A["n"] else None, A["n"],
                                         int(side), int(seed), int(score), out.ctypes.data, C.byref(out_n), C.byref(used), begin.ctypes.data, ln.ctypes.data,
                                         cap, C.byref(recs), stats.ctypes.data, clip.ctypes.data, C.byref(bad))
    if clause < 0:
        raise ValueError(L.pfh_last_error(None).decode())
    return dict(clause=MASK_CLAUSES[clause], bad_record=bad.value, out=out[: out_n.value].tobytes(), bytes_used=used.value, n_records=recs.value,
                begin=begin[: recs.value].tolist(), len=ln[: recs.value].tolist(), stats={f: int(v) for f, v in zip(TRIM_STATS_FIELDS, stats)},
                clip={f: [int(v) for v in row] for f, row in zip(CLIP_STATS_FIELDS, clip)})


def _prefix_pairs(adapters) -> dict:
    """adapters with prefix pairs as the pair calls take them: the dict of clip_parse_adapters(pairs=True), a path or the bytes of an
    adapter file, or (list of (sequence, side), list of (P1, P2)) (nothing is checked there: the library refuses by name)."""
    if isinstance(adapters, dict):
        return adapters
    if isinstance(adapters, (list, tuple)):
        simple, prefix = adapters
        A = clip_adapters(list(simple))
        halves = [h.encode() if isinstance(h, str) else bytes(h) for pr in prefix for h in pr]
        poff = np.zeros(len(halves) + 1, dtype=np.uint32)
        poff[1:] = np.cumsum([len(h) for h in halves], dtype=np.uint64) if halves else []
        return dict(A, prefix_bases=b"".join(halves), prefix_off=poff, n_pairs=len(halves) // 2)
    return clip_parse_adapters(adapters, pairs=True)


def _pair_args(A):
    bases, pbases = np.frombuffer(A["bases"], dtype=np.uint8), np.frombuffer(A["prefix_bases"], dtype=np.uint8)
    keep = (bases, pbases, A["off"], A["side"], A["prefix_off"])   # (alive while the call runs)
    return keep, (bases.ctypes.data if len(bases) else None, A["off"].ctypes.data, A["side"].ctypes.data if A["n"] else None, A["n"],
                  pbases.ctypes.data if len(pbases) else None, A["prefix_off"].ctypes.data, A["n_pairs"])


def clip_pair(seq1: bytes, qual1: bytes, seq2: bytes, qual2: bytes, adapters, seed: int = 2, score: int = 10, pair_score: int = 30, pair_min: int = 8,
              keep_both: bool = False, phred: int = 33, stats: bool = False):
    """The rule of `--adapters --adapter-pairs` on the two reads of one pair (pfh_clip_pair; no device): [clip end of file 1, of file 2]
    -- simple mode and palindrome mode together.  adapters: see _prefix_pairs.  stats=True: (ends, clip statistics, pair statistics) of
    this one pair.  Values that are refused raise ValueError."""
    L = load_library()
    A = _prefix_pairs(adapters)
    arrs = [np.frombuffer(bytes(x), dtype=np.uint8) for x in (seq1, qual1, seq2, qual2)]
    if len(arrs[0]) != len(arrs[1]) or len(arrs[2]) != len(arrs[3]):
        raise ValueError("clip_pair: the quality line is as long as the sequence line")
    ptr = [a.ctypes.data if len(a) else None for a in arrs]
    keep, pa = _pair_args(A)
    end = np.zeros(2, dtype=np.uint32)
    clip = np.zeros((len(CLIP_STATS_FIELDS), 2), dtype=np.uint64)
    ps = np.zeros(6, dtype=np.uint64)
    rc = L.pfh_clip_pair(ptr[0], ptr[1], len(arrs[0]), ptr[2], ptr[3], len(arrs[2]), *pa, int(seed), int(score), int(pair_score), int(pair_min),
                         int(bool(keep_both)), int(phred), end.ctypes.data, clip.ctypes.data, ps.ctypes.data)
    if rc < 0:
        raise ValueError(L.pfh_last_error(None).decode())
    ends = [int(end[0]), int(end[1])]
    return (ends, {f: [int(v) for v in row] for f, row in zip(CLIP_STATS_FIELDS, clip)}, _pair_stats_dict(ps)) if stats else ends


TRIM_PAIR_CLIP_CLAUSES = MASK_CLAUSES + ("pair_count",)   # pf_mask::Clause, then pf_clip::PAIR_COUNTS_DIFFER


def trim_fastq_pair_chunk_clip(text1: bytes, text2: bytes, steps, adapters, seed: int = 2, score: int = 10, pair_score: int = 30, pair_min: int = 8,
                               keep_both: bool = False, phred: int = 33, final: bool = True) -> dict:
    """What pf_trim_fastq_pair gives for one chunk of each file while a clip with prefix pairs is open, by the host's plain restatement
    (pfh_trim_fastq_pair_chunk_clip; no device): dict with clause, bad_record (2 * record + file), out (o1, u1, o2, u2), bytes_used,
    begin, len, clip_end and stats per file, n_records, clip (CLIP_STATS_FIELDS) and pairs (CLIP_PAIR_STATS_FIELDS).  steps may be empty."""
    L = load_library()
    st = trim_parse_steps(steps) if len(steps) else np.zeros(0, dtype=TRIM_STEP)
    A = _prefix_pairs(adapters)
    keep, pa = _pair_args(A)
    src = [np.frombuffer(bytes(t), dtype=np.uint8) for t in (text1, text2)]
    n = [len(x) for x in src]
    outs = [np.zeros(n[d // 2] + 1, dtype=np.uint8) for d in range(4)]
    cap = min(n) // 4 + 1
    begin, ln, ce = ([np.zeros(cap, dtype=np.uint32) for _ in range(2)] for _ in range(3))
    ptrs = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    stats = np.zeros((2, len(TRIM_STATS_FIELDS)), dtype=np.uint64)
    clip = np.zeros((len(CLIP_STATS_FIELDS), 2), dtype=np.uint64)
    ps = np.zeros(6, dtype=np.uint64)
    out_n, used = np.zeros(4, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    recs, bad = C.c_uint64(), C.c_uint64()
    clause = L.pfh_trim_fastq_pair_chunk_clip(src[0].ctypes.data if n[0] else None, n[0], src[1].ctypes.data if n[1] else None, n[1], int(final),
                                              st.ctypes.data if len(st) else None, len(st), int(phred), *pa, int(seed), int(score), int(pair_score),
                                              int(pair_min), int(bool(keep_both)), ptrs(outs), out_n.ctypes.data, used.ctypes.data, ptrs(begin), ptrs(ln),
                                              ptrs(ce), cap, C.byref(recs), stats.ctypes.data, clip.ctypes.data, ps.ctypes.data, C.byref(bad))
    if clause < 0:
        raise ValueError(L.pfh_last_error(None).decode())
    m = recs.value
    return dict(clause=TRIM_PAIR_CLIP_CLAUSES[clause], bad_record=bad.value, out=[outs[d][: int(out_n[d])].tobytes() for d in range(4)],
                bytes_used=[int(v) for v in used], n_records=m, begin=[b[:m].tolist() for b in begin], len=[x[:m].tolist() for x in ln],
                clip_end=[x[:m].tolist() for x in ce], stats=[{f: int(v) for f, v in zip(TRIM_STATS_FIELDS, row)} for row in stats],
                clip={f: [int(v) for v in row] for f, row in zip(CLIP_STATS_FIELDS, clip)}, pairs=_pair_stats_dict(ps))


def _set_adapters(L, adapters, seed, score, pairs=False, pair_score=30, pair_min=8, keep_both=False):
    """`--adapters` of the next trim / run call (pfh_reads_adapters): a path, or None for no clipping; pairs: `--adapter-pairs` and
    its values (pfh_reads_adapter_pairs).  The pair options without adapters, or the values without pairs, are refused as the command
    line refuses them."""
    if adapters is None and (pairs or keep_both or pair_score != 30 or pair_min != 8):
        raise ValueError("adapter_pairs, adapter_pair_score, adapter_pair_min and adapter_keep_both need adapters")
    if not pairs and (keep_both or pair_score != 30 or pair_min != 8):
        raise ValueError("adapter_pair_score, adapter_pair_min and adapter_keep_both need adapter_pairs")
    L.pfh_reads_adapters(None if adapters is None else os.fsencode(adapters), int(seed), int(score))
    if pairs:
        L.pfh_reads_adapter_pairs(int(pair_score), int(pair_min), int(bool(keep_both)))


def clip_pair_report() -> dict:
    """What the last trim / run call of this thread that took adapter_pairs= reported (pfh_reads_adapters_pair_report): pairs (the prefix
    pairs of the file) and the statistics of CLIP_PAIR_STATS_FIELDS -- the tail of the command's `clip:` line."""
    L = load_library()
    q = C.c_uint32()
    ps = np.zeros(6, dtype=np.uint64)
    L.pfh_reads_adapters_pair_report(C.byref(q), ps.ctypes.data)
    return dict(_pair_stats_dict(ps), pairs=q.value)


def clip_report() -> dict:
    """What the last trim / run call of this thread that took adapters= reported (pfh_reads_adapters_report): adapters, skipped and the
    statistics of CLIP_STATS_FIELDS, each [file 1, file 2] -- the command's `clip:` line."""
    L = load_library()
    a, p = C.c_uint32(), C.c_uint32()
    st = np.zeros((len(CLIP_STATS_FIELDS), 2), dtype=np.uint64)
    L.pfh_reads_adapters_report(C.byref(a), C.byref(p), st.ctypes.data)
    out = dict(adapters=a.value, skipped=p.value)
    out.update({f: [int(v) for v in row] for f, row in zip(CLIP_STATS_FIELDS, st)})
    return out


TRIM_TABLE_CLAUSES = MASK_CLAUSES + ("pair_count",)   # pf_mask::Clause, then pf_trimrun::CLAUSE_PAIR_COUNT


def trim_table_chunk(text, steps, phred: int = 33, final: bool = True, text2=None):
    """What `run STEP...` hands on from one chunk of raw FASTQ, by the host's plain restatement (pfh_trim_table_chunk; no device;
    csrc/pf_trimrun_rule.hpp): dict with clause (a name of TRIM_TABLE_CLAUSES), message, bad_record, read_off / read_len (the table of the
    reads handed on: the kept interval of the sequence line of every kept record), n_reads, bytes_used, n_records, stats.  text2: the
    chunk of the second file of a pair (pfh_trim_table_chunk_pair) -- read_off / read_len / bytes_used / stats are then [file 1,
    file 2], a record goes on only when it is kept in both files, and bad_record = 2 * record + file."""
    L = load_library()
    st = trim_parse_steps(steps)
    texts = [np.frombuffer(bytes(x), dtype=np.uint8) for x in ((text,) if text2 is None else (text, text2))]
    n = [len(x) for x in texts]
    cap = min(n) // 4 + 1
    off = [np.zeros(cap, dtype=np.uint64) for _ in texts]
    ln = [np.zeros(cap, dtype=np.uint32) for _ in texts]
    stats = np.zeros((len(texts), len(TRIM_STATS_FIELDS)), dtype=np.uint64)
    n_reads, recs, bad, used = C.c_uint64(), C.c_uint64(), C.c_uint64(), (C.c_uint64 * 2)()
    sp, sn = (st.ctypes.data if len(st) else None), len(st)
    if text2 is None:
        clause = L.pfh_trim_table_chunk(texts[0].ctypes.data if n[0] else None, n[0], int(final), sp, sn, phred, off[0].ctypes.data, ln[0].ctypes.data, cap,
                                        C.byref(n_reads), used, C.byref(recs), stats.ctypes.data, C.byref(bad))
    else:
        off_p = (C.c_void_p * 2)(*[x.ctypes.data for x in off])
        len_p = (C.c_void_p * 2)(*[x.ctypes.data for x in ln])
        clause = L.pfh_trim_table_chunk_pair(texts[0].ctypes.data if n[0] else None, n[0], texts[1].ctypes.data if n[1] else None, n[1], int(final), sp, sn,
                                             phred, off_p, len_p, cap, C.byref(n_reads), used, C.byref(recs), stats.ctypes.data, C.byref(bad))
    if clause < 0:
        raise ValueError(L.pfh_last_error(None).decode())
    m = n_reads.value
    per = [dict(read_off=off[f][:m].tolist(), read_len=ln[f][:m].tolist(), bytes_used=used[f],
                stats={k: int(v) for k, v in zip(TRIM_STATS_FIELDS, stats[f])}) for f in range(len(texts))]
    out = dict(clause=TRIM_TABLE_CLAUSES[clause], message=L.pfh_trim_table_clause_text(clause).decode(), bad_record=bad.value, n_reads=m, n_records=recs.value)
    for key in ("read_off", "read_len", "bytes_used", "stats"):
        out[key] = per[0][key] if text2 is None else [x[key] for x in per]
    return out


def _gz_mode(gz) -> int:
    """gz= of the reads calls: False, True (`--gz`: blocked gzip) or "plain" (`--gz-plain`: any gzip) -> what pfh_reads_gz takes"""
    if isinstance(gz, str):
        if gz != "plain":
            raise ValueError('gz is False, True or "plain"')
        return 2
    return int(bool(gz))


def _set_report(L, report):
    """`--report` of the next trim / run call (pfh_reads_report): a path, or None for no report"""
    L.pfh_reads_report(None if report is None else os.fsencode(report))


QC_TABLE_WORDS, QC_CLIP_WORDS = 9515, 1025   # PF_QC_TABLE_WORDS, PF_QC_CLIP_WORDS (csrc/pf_qc_rule.hpp has the words)


def qc_fastq(paths, report: str, paths2=None, phred: int = 33, gz: bool = False, chunk_bytes: int = 0) -> None:
    """`ploidyfrost qc (-i ... | -1 ... -2 ...) -o report` (pfh_qc_fastq): the read quality report of the FASTQ file(s) `paths` (side 1)
    and `paths2` (side 2, may be None) as they are, accumulated on the device (K-QC) and written to `report` as tab-separated text.  A
    refusal raises RuntimeError by name; nothing is left under the report's name."""
    L = load_library()
    p1, n1 = _paths(paths)
    p2, n2 = _paths([] if paths2 is None else paths2)
    L.pfh_reads_gz(_gz_mode(gz))
    rc = L.pfh_qc_fastq(p1, n1, p2, n2, os.fsencode(report), int(phred), int(chunk_bytes), 0)
    if rc:
        raise (ReadsRefused if gz else RuntimeError)(L.pfh_last_error(None).decode())


def qc_fastq_chunk(text: bytes, tables=None, clip=None, side: int = 1, phred: int = 33, final: bool = True, steps=None, adapters=None, seed: int = 2,
                   score: int = 10) -> dict:
    """The rule of K-QC on one chunk of one file by the host's plain restatement (pfh_qc_fastq_chunk; no device): the whole records of
    `text` added to tables[side - 1][0] (raw) and, with steps (Trimmomatic's words; may be [] beside adapters) the kept ones to
    tables[side - 1][1]; with adapters (the dict of clip_parse_adapters) the clip ends below the read length to clip[side - 1].
    tables: a u64 array [2][2][QC_TABLE_WORDS] to add to (None: a new one of zeros), clip: [2][QC_CLIP_WORDS] likewise.  Returns dict with
    tables, clip, clause (a name of MASK_CLAUSES), bad_record, bytes_used, n_records."""
    L = load_library()
    if tables is None:
        tables = np.zeros((2, 2, QC_TABLE_WORDS), dtype=np.uint64)
    if clip is None:
        clip = np.zeros((2, QC_CLIP_WORDS), dtype=np.uint64)
    trimmed = steps is not None
    st = trim_parse_steps(steps) if trimmed and len(steps) else np.zeros(0, dtype=TRIM_STEP)
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    if adapters is not None:
        bases = np.frombuffer(bytes(adapters["bases"]), dtype=np.uint8)
        off = np.ascontiguousarray(adapters["off"], dtype=np.uint32)
        sd = np.ascontiguousarray(adapters["side"], dtype=np.uint8)
    else:
        bases, off, sd = np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
    used, recs, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
    clause = L.pfh_qc_fastq_chunk(t.ctypes.data if len(t) else None, len(t), int(final), int(phred), int(side), int(trimmed),
                                  st.ctypes.data if len(st) else None, len(st), int(adapters is not None), bases.ctypes.data if len(bases) else None,
                                  off.ctypes.data, sd.ctypes.data if len(sd) else None, len(sd), int(seed), int(score), tables[side - 1, 0].ctypes.data,
                                  tables[side - 1, 1].ctypes.data, clip[side - 1].ctypes.data, C.byref(used), C.byref(recs), C.byref(bad))
    if clause < 0:
        raise ValueError(L.pfh_last_error(None).decode())
    return dict(tables=tables, clip=clip, clause=MASK_CLAUSES[clause], bad_record=bad.value, bytes_used=used.value, n_records=recs.value)


def qc_report_text(tables, clip=None, phred: int = 33) -> bytes:
    """The report as `qc` and `--report` write it (pfh_qc_report_text): a function of the tables [2][2][QC_TABLE_WORDS] and, where a
    clip was open, of clip [2][QC_CLIP_WORDS] alone."""
    L = load_library()
    tables = np.ascontiguousarray(tables, dtype=np.uint64).reshape(2, 2, QC_TABLE_WORDS)
    cp = None if clip is None else np.ascontiguousarray(clip, dtype=np.uint64).reshape(2, QC_CLIP_WORDS)
    n = C.c_uint64()
    if L.pfh_qc_report_text(tables.ctypes.data, None if cp is None else cp.ctypes.data, int(phred), None, 0, C.byref(n)):
        raise ValueError(L.pfh_last_error(None).decode())
    buf = C.create_string_buffer(max(n.value, 1))
    L.pfh_qc_report_text(tables.ctypes.data, None if cp is None else cp.ctypes.data, int(phred), buf, n.value, C.byref(n))
    return buf.raw[: n.value]


def qc_phred_hint(min_byte: int, reads: int) -> int:
    """33, 64 or 0 (undecided) from the smallest quality byte of the raw stage and the number of reads that held one (pfh_qc_phred_hint)"""
    return int(load_library().pfh_qc_phred_hint(int(min_byte), int(reads)))


HETPAIR_STATS_FIELDS = ("kmers", "in_range", "one_partner", "many_partners", "pairs")   # pf_hetpair_stats
SMUDGE_RESULT = np.dtype([(f, "<u8") for f in HETPAIR_STATS_FIELDS] + [(f, "<u4") for f in ("k", "lower", "upper", "clamped", "proposed_p", "proposed_m")] +
                         [("proposed_pairs", "<u8"), ("all_pairs", "<u8")])   # pfh_smudge_result
assert SMUDGE_RESULT.itemsize == 80


def hetpairs_host(kmers, counts, k: int, lo: int, hi: int) -> dict:
    """The rule of K-HETPAIR by the host's plain restatement (pfh_hetpairs_host, csrc/pf_hetpair_rule.hpp; no device): distinct
    canonical k-mers (u64) and their counters (u32) in; "table" (W x W uint64, W = hi - lo + 1), "pair_x", "pair_y", "cov_x", "cov_y" in
    the order of x in kmers and "stats" out -- what hipapi.Device.hetpairs returns.  A refused argument raises ValueError by name."""
    L = load_library()
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    n = len(kmers)
    assert len(counts) == n
    W = int(hi) - int(lo) + 1
    table = np.zeros((W, W), dtype=np.uint64) if 1 <= W <= 4096 else None
    stats = np.zeros(len(HETPAIR_STATS_FIELDS), dtype=np.uint64)
    m = C.c_uint64()
    cap = n // 2 + 1   # a key is in one pair at most
    px, py = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    cx, cy = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
    if L.pfh_hetpairs_host(kmers.ctypes.data if n else None, counts.ctypes.data if n else None, n, int(k), int(lo), int(hi),
                           None if table is None else table.ctypes.data, px.ctypes.data, py.ctypes.data, cx.ctypes.data, cy.ctypes.data, cap, C.byref(m),
                           stats.ctypes.data):
        raise ValueError(L.pfh_last_error(None).decode())
    assert m.value <= cap
    return {"table": table, "pair_x": px[: m.value], "pair_y": py[: m.value], "cov_x": cx[: m.value], "cov_y": cy[: m.value],
            "stats": {f: int(v) for f, v in zip(HETPAIR_STATS_FIELDS, stats)}}


def smudge_report(table, stats, k: int, lo: int, hi: int, n: int = 0) -> bytes:
    """The report as `smudge` and `run --smudge` write it (pfh_smudge_report_text): a function of the table (W x W), the statistics (a
    dict of HETPAIR_STATS_FIELDS), k, the bounds and the haploid coverage n (0: none) alone."""
    L = load_library()
    W = int(hi) - int(lo) + 1
    table = np.ascontiguousarray(table, dtype=np.uint64).reshape(max(W, 1), max(W, 1))
    st = np.array([int(stats[f]) for f in HETPAIR_STATS_FIELDS], dtype=np.uint64)
    ln = C.c_uint64()
    if L.pfh_smudge_report_text(table.ctypes.data, st.ctypes.data, int(k), int(lo), int(hi), int(n), None, 0, C.byref(ln)):
        raise ValueError(L.pfh_last_error(None).decode())
    buf = C.create_string_buffer(max(ln.value, 1))
    L.pfh_smudge_report_text(table.ctypes.data, st.ctypes.data, int(k), int(lo), int(hi), int(n), buf, ln.value, C.byref(ln))
    return buf.raw[: ln.value]


def smudge_of(a: int, b: int, n: int):
    """(p, m, label) of a pair with the coverages a <= b at the haploid coverage n (pfh_smudge_of): p - m letters A, m letters B"""
    L = load_library()
    p, m = C.c_uint32(), C.c_uint32()
    if L.pfh_smudge_of(int(a), int(b), int(n), C.byref(p), C.byref(m)):
        raise ValueError(L.pfh_last_error(None).decode())
    return p.value, m.value, "A" * (p.value - m.value) + "B" * m.value


def _set_smudge(L, smudge, smudge_n, smudge_pairs):
    """`--smudge [--smudge-n N] [--smudge-pairs FILE]` of the next run call (pfh_reads_smudge)"""
    L.pfh_reads_smudge(int(bool(smudge)), -1 if smudge_n is None else int(smudge_n), None if smudge_pairs is None else os.fsencode(smudge_pairs))


def _smudge_result(r) -> dict:
    d = {f: int(r[0][f]) for f in SMUDGE_RESULT.names}
    d["stats"] = {f: d.pop(f) for f in HETPAIR_STATS_FIELDS}
    return d


def smudge(out: str, db=None, inputs=None, lower=None, upper=None, auto: bool = False, q: float = 0.998, n=None, pairs=None, k: int = 25,
           ci: int = 1, cx: int = 10 ** 9, cs: int = 10000, chunk_bytes: int = 0, initial_slots: int = 0, gz: bool = False, fasta: bool = False) -> dict:
    """`ploidyfrost smudge` (pfh_smudge): the k-mer pair report <out>_smudge.tsv from a KMC database (db) or from reads counted first
    (inputs, with k, ci, cx, cs) -- K-HETPAIR over the count table on the device.  lower and upper, or auto=True (what `cutoffL -d` and
    `cutoffU -d q` print); n: the haploid coverage for the summary; pairs: a path for the pairs file.  Returns "stats", the bounds used
    ("lower", "upper", "clamped") and with n the proposed ploidy.  A refusal raises RuntimeError by name; nothing is left under an
    output name."""
    L = load_library()
    if (db is None) == (inputs is None):
        raise ValueError("smudge: either db or inputs")
    if auto == (lower is not None or upper is not None) or (not auto and (lower is None or upper is None)):
        raise ValueError("smudge: either lower=L and upper=U or auto=True")
    if n is not None and int(n) < 1:
        raise ValueError("smudge: n is a haploid coverage of at least 1")
    paths, n_in = _paths(inputs if inputs is not None else [])
    res = np.zeros(1, dtype=SMUDGE_RESULT)
    L.pfh_reads_gz(_gz_mode(gz))
    L.pfh_reads_fasta(int(bool(fasta)))
    rc = L.pfh_smudge(None if db is None else os.fsencode(db), paths, n_in, int(k), int(ci), int(cx), int(cs), 0 if lower is None else int(lower),
                      0 if upper is None else int(upper), int(auto), float(q), 0 if n is None else int(n), None if pairs is None else os.fsencode(pairs),
                      os.fsencode(out), int(chunk_bytes), int(initial_slots), 0, res.ctypes.data)
    if rc:
        raise (ReadsRefused if gz else RuntimeError)(L.pfh_last_error(None).decode())
    return _smudge_result(res)


def smudge_result() -> dict:
    """What the last run_reads(..., smudge=True) of this thread found (pfh_reads_smudge_result)"""
    res = np.zeros(1, dtype=SMUDGE_RESULT)
    load_library().pfh_reads_smudge_result(res.ctypes.data)
    return _smudge_result(res)


DEDUP_STATS_FIELDS = ("units", "unique", "duplicates", "max_copies", "levels", "slots", "growths")   # pf_dedup_stats (levels: 10 words)
DEDUP_STATS = hipapi.DEDUP_STATS


def _dedup_dict(st) -> dict:
    return {f: ([int(v) for v in st[0][f]] if f == "levels" else int(st[0][f])) for f in DEDUP_STATS_FIELDS}


def _set_dedup(L, dedup, dedup_bases, dedup_initial_slots):
    """`--dedup [--dedup-bases N] [--dedup-initial-slots N]` of the next trim / run call (pfh_reads_dedup); the values without the switch
    are refused by name here, as the command line refuses them"""
    if not dedup and dedup_bases:
        raise RuntimeError("--dedup-bases needs --dedup: the bases are read by the duplicate removal alone")
    if not dedup and dedup_initial_slots:
        raise RuntimeError("--dedup-initial-slots needs --dedup: the table is the duplicate removal's alone")
    L.pfh_reads_dedup(int(bool(dedup)), int(dedup_bases), int(dedup_initial_slots))


def dedup_report() -> dict:
    """What the last trim / run call of this thread that ran with dedup=True found (pfh_reads_dedup_report), summed over its units"""
    st = np.zeros(1, dtype=DEDUP_STATS)
    load_library().pfh_reads_dedup_report(st.ctypes.data)
    return _dedup_dict(st)


def dedup_key(seq1, seq2=None, bases: int = 0):
    """The 128-bit key of one unit as K-DEDUP defines it (pfh_dedup_key, csrc/pf_dedup_rule.hpp; no device): (h1, h2) of the read seq1, or
    of the pair (seq1, seq2); bases: 0 = the whole read, else the first 16 .. 4096 bases.  A refusal raises RuntimeError by name."""
    L = load_library()
    key = np.zeros(2, dtype=np.uint64)
    s1 = bytes(seq1)
    s2 = None if seq2 is None else bytes(seq2)
    if L.pfh_dedup_key(s1, len(s1), s2, 0 if s2 is None else len(s2), int(bases), key.ctypes.data):
        raise RuntimeError(L.pfh_last_error(None).decode())
    return int(key[0]), int(key[1])


def dedup_units(keys, participates=None):
    """The decision of K-DEDUP over the keys ([n, 2] u64) of the units of a whole stream in order (pfh_dedup_units; no device):
    (keep, stats) -- keep[i] = 1 for the first unit of its key and for a unit that takes no part (participates[i] == 0), 0 for a later
    copy; stats: DEDUP_STATS_FIELDS (slots and growths 0)."""
    L = load_library()
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, 2)
    n = len(keys)
    part = None if participates is None else np.ascontiguousarray(participates, dtype=np.uint8)
    keep = np.zeros(n, dtype=np.uint8)
    st = np.zeros(1, dtype=DEDUP_STATS)
    if L.pfh_dedup_units(keys.ctypes.data if n else None, None if part is None else part.ctypes.data, n, keep.ctypes.data if n else None, st.ctypes.data):
        raise RuntimeError(L.pfh_last_error(None).decode())
    return keep, _dedup_dict(st)


def trim_fastq_chunk_dedup(text, steps, phred: int = 33, final: bool = True, bases: int = 0, seen_keys=None, text2=None):
    """What Device.trim_fastq (text2 None) / Device.trim_fastq_pair give for one chunk while a dedup is open and no clip, restated on the
    host (pfh_trim_fastq[_pair]_chunk_dedup; no device).  seen_keys: [m, 2] u64, the keys of the units that took part before.  Returns a
    dict: clause, bad_record, n_records, keys ([n_records, 2]; 0 0 = takes no part), and per file (single-ended: the values
    themselves; a pair: lists of two) out / outs (o1 u1 o2 u2), bytes_used, begin, len, stats."""
    L = load_library()
    st = trim_parse_steps(steps) if len(steps) else np.zeros(0, dtype=TRIM_STEP)
    seen = np.zeros((0, 2), dtype=np.uint64) if seen_keys is None else np.ascontiguousarray(seen_keys, dtype=np.uint64).reshape(-1, 2)
    texts = [bytes(text)] + ([] if text2 is None else [bytes(text2)])
    nf = len(texts)
    cap = max(len(t) for t in texts) // 4 + 1
    outs = [np.zeros(len(texts[d // 2 if nf == 2 else 0]) + 1, dtype=np.uint8) for d in range(4 if nf == 2 else 1)]
    begin = [np.zeros(cap, dtype=np.uint32) for _ in range(nf)]
    ln = [np.zeros(cap, dtype=np.uint32) for _ in range(nf)]
    keys = np.zeros((cap, 2), dtype=np.uint64)
    stats = np.zeros((nf, len(TRIM_STATS_FIELDS)), dtype=np.uint64)
    out_n = (C.c_uint64 * 4)()
    used = (C.c_uint64 * 2)()
    recs, bad = C.c_uint64(), C.c_uint64()
    if nf == 1:
        clause = L.pfh_trim_fastq_chunk_dedup(texts[0], len(texts[0]), int(final), st.ctypes.data if len(st) else None, len(st), int(phred), int(bases),
                                              seen.ctypes.data if len(seen) else None, len(seen), outs[0].ctypes.data, out_n, used, begin[0].ctypes.data,
                                              ln[0].ctypes.data, keys.ctypes.data, cap, C.byref(recs), stats.ctypes.data, C.byref(bad))
    else:
        p_out = (C.c_void_p * 4)(*[o.ctypes.data for o in outs])
        p_b = (C.c_void_p * 2)(*[a.ctypes.data for a in begin])
        p_l = (C.c_void_p * 2)(*[a.ctypes.data for a in ln])
        clause = L.pfh_trim_fastq_pair_chunk_dedup(texts[0], len(texts[0]), texts[1], len(texts[1]), int(final), st.ctypes.data if len(st) else None, len(st),
                                                   int(phred), int(bases), seen.ctypes.data if len(seen) else None, len(seen), p_out, out_n, used, p_b, p_l,
                                                   keys.ctypes.data, cap, C.byref(recs), stats.ctypes.data, C.byref(bad))
    if clause < 0:
        raise RuntimeError(L.pfh_last_error(None).decode())
    n = recs.value
    res = dict(clause=clause, bad_record=bad.value, n_records=n, keys=keys[:n].copy())
    sts = [{f: int(v) for f, v in zip(TRIM_STATS_FIELDS, row)} for row in stats]
    if nf == 1:
        res.update(out=outs[0][: out_n[0]].tobytes(), bytes_used=used[0], begin=begin[0][:n], len=ln[0][:n], stats=sts[0])
    else:
        res.update(outs=[outs[d][: out_n[d]].tobytes() for d in range(4)], bytes_used=[used[0], used[1]], begin=[b[:n] for b in begin],
                   len=[a[:n] for a in ln], stats=sts)
    return res


def trim_fastq(inputs, out: str, steps, phred: int = 33, trimlog=None, chunk_bytes: int = 0, gz: bool = False, gz_out: bool = False,
               adapters=None, adapter_seed: int = 2, adapter_score: int = 10, report=None, dedup: bool = False, dedup_bases: int = 0,
               dedup_initial_slots: int = 0) -> dict:
    """`ploidyfrost trim -i ... -o out STEP...` (pfh_trim_fastq): the reads of the FASTQ file(s) `inputs`, one after the other,
    quality-trimmed by `steps` (Trimmomatic's words) into `out`; trimlog: a file with one line per record.  Returns the statistics.  A
    refusal raises RuntimeError (format refusals with the input's path and the 1-based record number); nothing is left under any
    output name.  gz_out (`--gz-out`): `out` is written as blocked gzip, deflated on the device (K-DEFLATE).
    adapters (`--adapters`): the path of an adapter file -- adapter read-through is clipped on the device before the steps (K-CLIP;
    adapter_seed, adapter_score: `--adapter-seed`, `--adapter-score`); steps may then be empty; clip_report() gives the `clip:` line.
    report (`--report`): a path for the read quality report of the reads as they come (raw) and as they are written (kept) (K-QC); every
    other output is what it is without.
    dedup (`--dedup`, with dedup_bases and dedup_initial_slots): every later copy of a kept read is dropped on the device (K-DEDUP; one
    table over all inputs); steps may then be empty, and the returned dict gains "dedup" (DEDUP_STATS_FIELDS)."""
    L = load_library()
    if isinstance(inputs, (str, bytes, os.PathLike)):
        inputs = [inputs]
    st = trim_parse_steps(steps) if len(steps) or (adapters is None and not dedup) else np.zeros(0, dtype=TRIM_STEP)
    paths = (C.c_char_p * max(len(inputs), 1))(*[os.fsencode(p) for p in inputs])
    stats = np.zeros(len(TRIM_STATS_FIELDS), dtype=np.uint64)
    L.pfh_reads_gz(_gz_mode(gz))
    L.pfh_reads_gz_out(int(gz_out))
    _set_dedup(L, dedup, dedup_bases, dedup_initial_slots)
    _set_adapters(L, adapters, adapter_seed, adapter_score)
    _set_report(L, report)
    rc = L.pfh_trim_fastq(paths, len(inputs), os.fsencode(out), st.ctypes.data if len(st) else None, len(st), phred,
                          os.fsencode(trimlog) if trimlog else None, int(chunk_bytes), 0, stats.ctypes.data)
    if rc:
        raise (ReadsRefused if gz else RuntimeError)(L.pfh_last_error(None).decode())
    res = {f: int(v) for f, v in zip(TRIM_STATS_FIELDS, stats)}
    if dedup:
        res["dedup"] = dedup_report()
    return res


def trim_fastq_pair(in1: str, in2: str, outs, steps, phred: int = 33, trimlog=None, chunk_bytes: int = 0, gz: bool = False, gz_out: bool = False,
                    adapters=None, adapter_seed: int = 2, adapter_score: int = 10, adapter_pairs: bool = False, adapter_pair_score: int = 30,
                    adapter_pair_min: int = 8, adapter_keep_both: bool = False, report=None, dedup: bool = False, dedup_bases: int = 0,
                    dedup_initial_slots: int = 0):
    """`ploidyfrost trim -1 in1 -2 in2 -o1 .. -u1 .. -o2 .. -u2 .. STEP...` (pfh_trim_fastq_pair): outs = (o1, u1, o2, u2).  Returns the
    statistics of file 1 and of file 2 (the pair fields are the same in both).  gz_out (`--gz-out`): the four outputs are blocked gzip.
    adapters, adapter_seed, adapter_score: as trim_fastq takes them (names ending in /1 and /2 choose the file).
    adapter_pairs (`--adapter-pairs`, with adapter_pair_score, adapter_pair_min, adapter_keep_both): palindrome mode from the file's
    prefix pairs beside simple mode (K-PALIN); clip_pair_report() gives the tail of the `clip:` line.
    report (`--report`): as trim_fastq takes it; file 1 is side 1 of the report, file 2 side 2.
    dedup, dedup_bases, dedup_initial_slots: as trim_fastq takes them; the unit is the pair, and both dicts gain "dedup"."""
    L = load_library()
    st = trim_parse_steps(steps) if len(steps) or (adapters is None and not dedup) else np.zeros(0, dtype=TRIM_STEP)
    assert len(outs) == 4
    paths = (C.c_char_p * 4)(*[os.fsencode(p) for p in outs])
    stats = np.zeros((2, len(TRIM_STATS_FIELDS)), dtype=np.uint64)
    L.pfh_reads_gz(_gz_mode(gz))
    L.pfh_reads_gz_out(int(gz_out))
    _set_dedup(L, dedup, dedup_bases, dedup_initial_slots)
    _set_adapters(L, adapters, adapter_seed, adapter_score, adapter_pairs, adapter_pair_score, adapter_pair_min, adapter_keep_both)
    _set_report(L, report)
    rc = L.pfh_trim_fastq_pair(os.fsencode(in1), os.fsencode(in2), paths, st.ctypes.data if len(st) else None, len(st), phred,
                               os.fsencode(trimlog) if trimlog else None, int(chunk_bytes), 0, stats.ctypes.data)
    if rc:
        raise (ReadsRefused if gz else RuntimeError)(L.pfh_last_error(None).decode())
    res = [{f: int(v) for f, v in zip(TRIM_STATS_FIELDS, row)} for row in stats]
    if dedup:
        for r in res:
            r["dedup"] = dedup_report()
    return res


COUNT_STATS_FIELDS = ("reads", "bases", "kmers", "kmers_bad", "unique", "below_min", "above_max", "written")   # pf_count_stats
COUNT_CUT_CLAUSES = ("none", "ci_zero", "ci_above_cx", "cs_zero", "too_large", "k", "k_layout")                               # pf_count::CutClause, in its order


def _paths(inputs):
    if isinstance(inputs, (str, bytes, os.PathLike)):
        inputs = [inputs]
    return (C.c_char_p * max(len(inputs), 1))(*[os.fsencode(p) for p in inputs]), len(inputs)


def count_fastq(inputs, out_prefix: str, k: int = 25, ci: int = 2, cx: int = 10 ** 9, cs: int = 255, both_strands: bool = True, hist=None,
                chunk_bytes: int = 0, initial_slots: int = 0, gz: bool = False, fasta: bool = False) -> dict:
    """`ploidyfrost count` (pfh_count_fastq): the k-mers of the FASTQ file(s) `inputs` counted on the device (K-COUNT), those with
    ci <= c <= cx written as min(c, cs) to <out_prefix>.kmc_pre / .kmc_suf in the KMC1 layout; hist: the histogram file of the finished
    counters.  Returns the statistics.  A refusal raises RuntimeError by name (format refusals with the input's path and the 1-based
    record number); nothing is left under the output names.  fasta (`--fasta`): an input whose first byte is '>' is read as FASTA
    (K-FASTA); every other input as before."""
    L = load_library()
    paths, n = _paths(inputs)
    stats = np.zeros(len(COUNT_STATS_FIELDS), dtype=np.uint64)
    L.pfh_reads_gz(_gz_mode(gz))
    L.pfh_reads_fasta(int(bool(fasta)))
    rc = L.pfh_count_fastq(paths, n, os.fsencode(out_prefix), int(k), int(ci), int(cx), int(cs), int(both_strands),
                           None if hist is None else os.fsencode(hist), int(chunk_bytes), int(initial_slots), 0, stats.ctypes.data)
    if rc:
        raise (ReadsRefused if gz else RuntimeError)(L.pfh_last_error(None).decode())
    return {f: int(v) for f, v in zip(COUNT_STATS_FIELDS, stats)}


def mask_fastq_counted(inputs, out: str, k: int = 25, ci: int = 2, cx: int = 10 ** 9, cs: int = 255, both_strands: bool = True, db_out=None,
                       lower=None, upper=None, auto: bool = False, chunk_bytes: int = 0, gz_out: bool = False) -> dict:
    """`ploidyfrost mask -k` (pfh_mask_fastq_counted): mask_fastq without a database -- the inputs are counted first, then masked
    against their own counters; db_out: the database is written as well; gz_out: `out` is blocked gzip."""
    L = load_library()
    if auto == (lower is not None):
        raise ValueError("mask_fastq_counted: either lower=L or auto=True")
    paths, n = _paths(inputs)
    stats = np.zeros(len(MASK_STATS_FIELDS), dtype=np.uint64)
    used = C.c_uint32()
    L.pfh_reads_gz_out(int(gz_out))
    rc = L.pfh_mask_fastq_counted(paths, n, os.fsencode(out), int(k), int(ci), int(cx), int(cs), int(both_strands),
                                  None if db_out is None else os.fsencode(db_out), 0 if lower is None else int(lower),
                                  0xFFFFFFFF if upper is None else int(upper), int(auto), int(chunk_bytes), 0, stats.ctypes.data, C.byref(used))
    if rc:
        raise RuntimeError(L.pfh_last_error(None).decode())
    d = {f: int(v) for f, v in zip(MASK_STATS_FIELDS, stats)}
    d["lower"] = used.value
    return d


def fasta_index(text: bytes, final: bool = True) -> dict:
    """The host rule of K-FASTA on one chunk (pfh_fasta_index, csrc/pf_fasta_rule.hpp; no device): "text" = the compacted text (the
    sequences of the whole records, one directly behind the other), "read_off" / "read_len" = the table into it, "bytes_used",
    "records", "bases".  A text that does not start with '>' raises ValueError with the clause's text."""
    L = load_library()
    src = np.frombuffer(bytes(text), dtype=np.uint8)
    used, n_rec, n_bases = C.c_uint64(), C.c_uint64(), C.c_uint64()
    out = np.zeros(max(len(src), 1), dtype=np.uint8)
    off, ln = np.zeros(max(len(src), 1), dtype=np.uint64), np.zeros(max(len(src), 1), dtype=np.uint32)   # (a record holds at least its '>')
    rc = L.pfh_fasta_index(src.ctypes.data if len(src) else None, len(src), int(final), C.byref(used), C.byref(n_rec), C.byref(n_bases),
                           out.ctypes.data, len(out), off.ctypes.data, ln.ctypes.data, len(off))
    if rc:
        raise ValueError(L.pfh_fasta_clause_text(rc).decode())
    return {"text": out[: n_bases.value].tobytes(), "read_off": off[: n_rec.value].copy(), "read_len": ln[: n_rec.value].copy(),
            "bytes_used": used.value, "records": n_rec.value, "bases": n_bases.value}


def count_reads_host(text: bytes, read_off, read_len, k: int, both_strands: bool = True, ci: int = 2, cx: int = 10 ** 9, cs: int = 255):
    """(kmers u64 sorted, counts u32, stats dict): the rule of `count` on the host (pfh_count_reads_host; no device).  A refusal of the
    options raises ValueError with its name of COUNT_CUT_CLAUSES and its text."""
    L = load_library()
    src = np.frombuffer(bytes(text), dtype=np.uint8)
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    ln = np.ascontiguousarray(read_len, dtype=np.uint32)
    cap = max(int(ln.astype(np.int64).sum()), 1)
    kmers, counts = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
    n = C.c_uint64()
    stats = np.zeros(len(COUNT_STATS_FIELDS), dtype=np.uint64)
    rc = L.pfh_count_reads_host(src.ctypes.data if len(src) else None, off.ctypes.data, ln.ctypes.data, len(off), int(k), int(both_strands), int(ci),
                                int(cx), int(cs), kmers.ctypes.data, counts.ctypes.data, cap, C.byref(n), stats.ctypes.data)
    if rc > 0:
        raise ValueError("%s: %s" % (COUNT_CUT_CLAUSES[rc], L.pfh_count_cut_text(rc).decode()))
    if rc < 0:
        raise OverflowError("a k-mer occurs more than 4294967295 times")
    return kmers[: n.value].copy(), counts[: n.value].copy(), {f: int(v) for f, v in zip(COUNT_STATS_FIELDS, stats)}


def count_encode_kmc1(kmers, counts, k: int, ci: int = 2, cx: int = 10 ** 9, cs: int = 255, both_strands: bool = True):
    """(bytes of .kmc_pre, bytes of .kmc_suf) for sorted distinct k-mers, by the host's restatement (pfh_count_encode_kmc1)"""
    L = load_library()
    km = np.ascontiguousarray(kmers, dtype=np.uint64)
    ct = np.ascontiguousarray(counts, dtype=np.uint32)
    pn, sn = C.c_uint64(), C.c_uint64()
    args = (km.ctypes.data, ct.ctypes.data, len(km), int(k), int(ci), int(cx), int(cs), int(both_strands))
    rc = L.pfh_count_encode_kmc1(*args, None, 0, C.byref(pn), None, 0, C.byref(sn))
    if rc:
        raise ValueError("%s: %s" % (COUNT_CUT_CLAUSES[rc], L.pfh_count_cut_text(rc).decode()))
    pre, suf = np.zeros(pn.value, dtype=np.uint8), np.zeros(sn.value, dtype=np.uint8)
    L.pfh_count_encode_kmc1(*args, pre.ctypes.data, len(pre), C.byref(pn), suf.ctypes.data, len(suf), C.byref(sn))
    return pre.tobytes(), suf.tobytes()


UNITIG_G_DEFAULT = -2 ** 31   # PFH_UNITIG_G_DEFAULT: Bifrost's minimizer length for k (pf_unitig::default_g decides)


def _unitig_g(g) -> int:
    """the g argument of the pfh_ calls: None = the default, any number as it is (0 and below are refused there by name)"""
    return UNITIG_G_DEFAULT if g is None else max(min(int(g), 2 ** 31 - 1), UNITIG_G_DEFAULT + 1)


UNITIG_STATS_FIELDS = ("distinct", "unitigs", "removed", "unitigs_out", "longest", "bytes")   # the first six of pf_unitig_stats
UNITIG_STATS = np.dtype([(f, "<u8") for f in UNITIG_STATS_FIELDS + ("cycles", "rounds", "cycle_rounds")] + [("stage_ms", "<f8", (6,))])   # pf_unitig_stats


def build_graph(inputs, out_prefix: str, k: int = 25, clip_tips: bool = False, del_isolated: bool = False, g=None, chunk_bytes: int = 0,
                initial_slots: int = 0, fasta: bool = False) -> dict:
    """`ploidyfrost build` (pfh_build_fastq): the compacted de Bruijn graph of the FASTQ file(s) `inputs`, counted and compacted on the
    device (K-COUNT, K-UNITIG), written to <out_prefix>.gfa -- `Bifrost build [-i] [-d] -k <k> -r <inputs> -o <out_prefix>`.  Returns
    the statistics of the count and of the graph.  A refusal raises RuntimeError by name; nothing is left under the output name.
    fasta (`--fasta`): an input whose first byte is '>' is read as FASTA (K-FASTA)."""
    L = load_library()
    paths, n = _paths(inputs)
    counted = np.zeros(len(COUNT_STATS_FIELDS), dtype=np.uint64)
    stats = np.zeros(1, dtype=UNITIG_STATS)
    L.pfh_reads_fasta(int(bool(fasta)))
    rc = L.pfh_build_fastq(paths, n, os.fsencode(out_prefix), int(k), _unitig_g(g), int(clip_tips), int(del_isolated), int(chunk_bytes),
                           int(initial_slots), 0, counted.ctypes.data, stats.ctypes.data)
    if rc:
        raise RuntimeError(L.pfh_last_error(None).decode())
    d = {f: int(v) for f, v in zip(COUNT_STATS_FIELDS[:4], counted)}
    d.update({f: int(stats[0][f]) for f in UNITIG_STATS.names if f != "stage_ms"})
    d["stage_ms"] = [float(x) for x in stats[0]["stage_ms"]]
    return d


def run_reads(inputs, out_prefix: str, k: int = 25, ci: int = 1, cx: int = 10 ** 9, cs: int = 10000, q: float = 0.998, mask_upper=None,
              keep_tips: bool = False, keep_isolated: bool = False, g=None, z: int = 8, M: float = 2.0, D: float = -1.0, G: float = -3.0,
              threads: int = 1, model=None, model_only: bool = False, db_out=None, gfa_out=None, chunk_bytes: int = 0,
              initial_slots: int = 0, steps=None, phred: int = 33, pairs=None, gz: bool = False, fasta: bool = False,
              adapters=None, adapter_seed: int = 2, adapter_score: int = 10, adapter_pairs: bool = False, adapter_pair_score: int = 30,
              adapter_pair_min: int = 8, adapter_keep_both: bool = False, report=None, smudge: bool = False, smudge_n=None,
              smudge_pairs=None, dedup: bool = False, dedup_bases: int = 0, dedup_initial_slots: int = 0) -> dict:
    """`ploidyfrost run` (pfh_run_fastq): reads to ploidy estimate in one process -- the FASTQ file(s) `inputs` counted, the thresholds
    derived, the k-mers of the masked reads counted (K-MASKCOUNT), the graph built and the single-sample calling run made on one device
    context; PloidyFrost_output/<out_prefix>_*.txt in the working directory.  model: None, "cov" or "fre".  Returns the fields of the
    command's stderr line ("lower" and "upper" among them).  A refusal raises RuntimeError by name.
    steps (Trimmomatic's words, as trim_fastq takes them): `run STEP...` (pfh_run_fastq_trimmed) -- the inputs are raw reads, trimmed on
    the device on the way into both passes; pairs = [(r1.fq, r2.fq), ...] instead of inputs (None then): the records of a pair go on
    only when both are kept.  The result then has "trim" as well: the statistics of every unit (one dict for all single-ended inputs;
    per pair a list of two, file 1 and file 2), as the command's `trim:` lines give them.
    fasta (`--fasta`): an input whose first byte is '>' (with gz: whose first inflated byte is) is read as FASTA in both passes (K-FASTA);
    refused by name together with steps or pairs.
    adapters (`--adapters`, with adapter_seed and adapter_score): as trim_fastq takes them; they turn the trimming on as steps do, and
    no step is needed beside them, also with pairs.
    adapter_pairs (`--adapter-pairs`, with adapter_pair_score, adapter_pair_min, adapter_keep_both): palindrome mode on pairs, as
    trim_fastq_pair takes it; refused by name without pairs.  Only pairs of which both records are kept go on, so without
    adapter_keep_both a clipped pair is not counted at all.
    report (`--report`): the report `trim_fastq(..., report=)` writes for the same inputs, taken over the first pass; refused by name
    without steps or adapters.
    smudge (`--smudge`, with smudge_n and smudge_pairs): the k-mer pair report PloidyFrost_output/<out_prefix>_smudge.tsv from the table
    of the first pass (K-HETPAIR), every other output being what it is without; the result then has "smudge" (smudge_result()).
    dedup (`--dedup`, with dedup_bases and dedup_initial_slots): as trim_fastq takes them -- one table per unit in both passes (all
    inputs together, each pair on its own); it turns the trimming on as steps do, and the result gains "dedup" (summed over the units)."""
    L = load_library()
    if pairs is not None:
        if inputs is not None:
            raise ValueError("run_reads: either inputs or pairs")
        inputs = [f for p in pairs for f in p]
    st = trim_parse_steps(steps) if steps is not None and (len(steps) or (adapters is None and not dedup)) else np.zeros(0, dtype=TRIM_STEP)   # (adapters or dedup alone: no step)
    paths, n = _paths(inputs)
    o = RunOptions()
    L.pfh_run_defaults(C.byref(o))
    o.k, o.ci, o.cx, o.cs = int(k), int(ci), int(cx), int(cs)
    o.g = _unitig_g(g)
    o.clip_tips, o.del_isolated = int(not keep_tips), int(not keep_isolated)
    o.chunk_bytes, o.initial_slots = int(chunk_bytes), int(initial_slots)
    o.quantile = float(q)
    o.mask_up = 0xFFFFFFFF if mask_upper is None else int(mask_upper)
    o.complex_size, o.match, o.mismatch, o.gap, o.threads = int(z), float(M), float(D), float(G), int(threads)
    if model is not None:
        if model not in ("cov", "fre"):
            raise ValueError("run_reads: model is None, 'cov' or 'fre'")
        o.model_source = 0 if model == "cov" else 1   # PF_MODEL_COV, PF_MODEL_FRE
        o.model_only = int(model_only)
    o.db_out = None if db_out is None else os.fsencode(db_out)
    o.gfa_out = None if gfa_out is None else os.fsencode(gfa_out)
    stats = np.zeros(len(RUN_STATS_FIELDS), dtype=np.uint64)
    if not dedup:
        _set_dedup(L, False, dedup_bases, dedup_initial_slots)   # (the values without the switch are refused)
    if steps is None and pairs is None and adapters is None and not dedup:
        L.pfh_reads_gz(_gz_mode(gz))
        L.pfh_reads_fasta(int(bool(fasta)))
        _set_report(L, report)
        _set_smudge(L, smudge, smudge_n, smudge_pairs)
        rc = L.pfh_run_fastq(paths, n, os.fsencode(out_prefix), C.byref(o), 0, stats.ctypes.data)
        if rc:
            raise (ReadsRefused if gz else RuntimeError)(L.pfh_last_error(None).decode())
        out = {f: int(v) for f, v in zip(RUN_STATS_FIELDS, stats)}
        if smudge:
            out["smudge"] = smudge_result()
        return out
    per = np.zeros((max(n, 1), len(TRIM_STATS_FIELDS)), dtype=np.uint64)
    L.pfh_reads_gz(_gz_mode(gz))
    L.pfh_reads_fasta(int(bool(fasta)))
    _set_adapters(L, adapters, adapter_seed, adapter_score, adapter_pairs, adapter_pair_score, adapter_pair_min, adapter_keep_both)
    _set_report(L, report)
    _set_smudge(L, smudge, smudge_n, smudge_pairs)
    _set_dedup(L, dedup, dedup_bases, dedup_initial_slots)
    rc = L.pfh_run_fastq_trimmed(paths, n, int(pairs is not None), st.ctypes.data if len(st) else None, len(st), int(phred), os.fsencode(out_prefix),
                                 C.byref(o), 0, stats.ctypes.data, per.ctypes.data)
    if rc:
        raise (ReadsRefused if gz else RuntimeError)(L.pfh_last_error(None).decode())
    out = {f: int(v) for f, v in zip(RUN_STATS_FIELDS, stats)}
    rows = [{f: int(v) for f, v in zip(TRIM_STATS_FIELDS, row)} for row in per]
    out["trim"] = [rows[0]] if pairs is None else [[rows[2 * u], rows[2 * u + 1]] for u in range(len(pairs))]
    if smudge:
        out["smudge"] = smudge_result()
    if dedup:
        out["dedup"] = dedup_report()
    return out


def run_multi_reads(samples, out_prefix: str, k: int = 25, ci: int = 1, cx: int = 10 ** 9, cs: int = 10000, q: float = 0.998, mask_upper=None,
                    keep_tips: bool = False, keep_isolated: bool = False, g=None, z: int = 8, M: float = 2.0, D: float = -1.0, G: float = -3.0,
                    threads: int = 1, model=None, model_only: bool = False, filter_multi=None, each_color: bool = False, db_out=None, gfa_out=None,
                    chunk_bytes: int = 0, initial_slots: int = 0, steps=None, phred: int = 33, pairs=None, gz: bool = False,
                    fasta: bool = False, adapters=None, adapter_seed: int = 2, adapter_score: int = 10, adapter_pairs: bool = False,
                    adapter_pair_score: int = 30, adapter_pair_min: int = 8, adapter_keep_both: bool = False, dedup: bool = False,
                    dedup_bases: int = 0, dedup_initial_slots: int = 0) -> dict:
    """`ploidyfrost run-multi` (pfh_run_multi_fastq): reads of several samples to one estimate per sample in one process.  samples: a
    list of (name, file or list of files), a sample a colour in the order given.  Every sample is counted and its thresholds derived,
    the k-mers of its masked reads counted (K-MASKCOUNT), their union taken (K-UNION), the coloured graph built and coloured per
    distinct k-mer (K-COLORSET) and the coloured calling run made on one device context; PloidyFrost_output/<out_prefix>_*.txt in the
    working directory.  model: None, "cov" or "fre", behind filter_multi = the options of filter_multi_opts as a dict.  Returns the
    fields of the command's stderr line (RUN_MULTI_STATS_FIELDS) and under "color" one dict of RUN_MULTI_COLOR_FIELDS per sample.  A
    refusal raises RuntimeError by name.
    steps: `run-multi STEP...` (pfh_run_multi_fastq_trimmed) -- the files are raw reads, trimmed on the way into both passes; pairs: the
    names of the samples whose files are pairs (file 1, file 2, file 1, ...).  The result then has "trim": per sample the statistics of
    its units, as run_reads gives them.
    fasta (`--fasta`): as run_reads takes it; the files of a sample may mix FASTA and FASTQ.
    adapters, adapter_seed, adapter_score: as run_reads takes them; they hold for every sample.
    adapter_pairs, adapter_pair_score, adapter_pair_min, adapter_keep_both: as run_reads takes them; every sample is then a pair sample.
    dedup, dedup_bases, dedup_initial_slots: as run_reads takes them, per sample; the result gains "dedup" (summed over all units)."""
    L = load_library()
    names, counts, flat, paired = [], [], [], []
    for name, files in samples:
        if isinstance(files, (str, bytes, os.PathLike)):
            files = [files]
        names.append(os.fsencode(name))
        counts.append(len(files))
        flat.extend(files)
        paired.append(int(pairs is not None and name in pairs))
    st = trim_parse_steps(steps) if steps is not None and (len(steps) or (adapters is None and not dedup)) else np.zeros(0, dtype=TRIM_STEP)   # (adapters or dedup alone: no step)
    c_names = (C.c_char_p * max(len(names), 1))(*names)
    n_of = np.ascontiguousarray(counts, dtype=np.uint32)
    paths, _ = _paths(flat)
    o = RunOptions()
    L.pfh_run_defaults(C.byref(o))
    o.k, o.ci, o.cx, o.cs = int(k), int(ci), int(cx), int(cs)
    o.g = _unitig_g(g)
    o.clip_tips, o.del_isolated = int(not keep_tips), int(not keep_isolated)
    o.chunk_bytes, o.initial_slots = int(chunk_bytes), int(initial_slots)
    o.quantile = float(q)
    o.mask_up = 0xFFFFFFFF if mask_upper is None else int(mask_upper)
    o.complex_size, o.match, o.mismatch, o.gap, o.threads = int(z), float(M), float(D), float(G), int(threads)
    multi = None
    if model is not None:
        if model not in ("cov", "fre"):
            raise ValueError("run_multi_reads: model is None, 'cov' or 'fre'")
        if filter_multi is None:
            raise ValueError("run_multi_reads: a model stands behind filter_multi (the options of `filter-multi`)")
        o.model_source = 0 if model == "cov" else 1   # PF_MODEL_COV, PF_MODEL_FRE
        o.model_only = int(model_only)
        multi = filter_multi_opts(**filter_multi)
    o.db_out = None if db_out is None else os.fsencode(db_out)
    o.gfa_out = None if gfa_out is None else os.fsencode(gfa_out)
    stats = np.zeros(len(RUN_MULTI_STATS_FIELDS), dtype=np.uint64)
    per = np.zeros((max(len(names), 1), len(RUN_MULTI_COLOR_FIELDS)), dtype=np.uint64)
    trimmed = steps is not None or pairs is not None or adapters is not None or bool(dedup)
    _set_dedup(L, dedup, dedup_bases, dedup_initial_slots)
    per_in = np.zeros((max(len(flat), 1), len(TRIM_STATS_FIELDS)), dtype=np.uint64)
    if trimmed:
        pair_of = np.ascontiguousarray(paired, dtype=np.int32)
        L.pfh_reads_gz(_gz_mode(gz))
        L.pfh_reads_fasta(int(bool(fasta)))
        _set_adapters(L, adapters, adapter_seed, adapter_score, adapter_pairs, adapter_pair_score, adapter_pair_min, adapter_keep_both)
        rc = L.pfh_run_multi_fastq_trimmed(c_names, n_of.ctypes.data if len(names) else None, pair_of.ctypes.data if len(names) else None, len(names), paths,
                                           st.ctypes.data if len(st) else None, len(st), int(phred), os.fsencode(out_prefix), C.byref(o),
                                           C.byref(multi) if multi is not None else None, int(each_color), 0, stats.ctypes.data, per.ctypes.data,
                                           per_in.ctypes.data)
    else:
        L.pfh_reads_gz(_gz_mode(gz))
        L.pfh_reads_fasta(int(bool(fasta)))
        rc = L.pfh_run_multi_fastq(c_names, n_of.ctypes.data if len(names) else None, len(names), paths, os.fsencode(out_prefix), C.byref(o),
                                   C.byref(multi) if multi is not None else None, int(each_color), 0, stats.ctypes.data, per.ctypes.data)
    if rc:
        raise (ReadsRefused if gz else RuntimeError)(L.pfh_last_error(None).decode())
    out = {f: int(v) for f, v in zip(RUN_MULTI_STATS_FIELDS, stats)}
    out["color"] = [{f: int(v) for f, v in zip(RUN_MULTI_COLOR_FIELDS, per[c])} for c in range(len(names))]
    if trimmed:
        rows = [{f: int(v) for f, v in zip(TRIM_STATS_FIELDS, row)} for row in per_in]
        out["trim"], at = [], 0
        for c in range(len(names)):
            out["trim"].append([[rows[at + 2 * u], rows[at + 2 * u + 1]] for u in range(counts[c] // 2)] if paired[c] else [rows[at]])
            at += counts[c]
    if dedup:
        out["dedup"] = dedup_report()
    return out


def union_host(arrays) -> np.ndarray:
    """The sorted distinct union of sorted distinct arrays of 64-bit keys as K-UNION defines it (pfh_union_host, csrc/pf_runmulti_rule.hpp;
    no device): rounds of pairwise merges, an odd set carried.  An array that is not ascending or holds a key twice raises RuntimeError
    by name."""
    L = load_library()
    arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in arrays]
    ns = np.array([len(a) for a in arrs], dtype=np.uint64)
    ptrs = np.array([a.ctypes.data for a in arrs], dtype=np.uint64)
    out = np.zeros(max(int(ns.sum()), 1), dtype=np.uint64)
    n = C.c_uint64()
    if L.pfh_union_host(ptrs.ctypes.data if len(arrs) else None, ns.ctypes.data if len(arrs) else None, len(arrs), out.ctypes.data, C.byref(n)):
        raise RuntimeError(L.pfh_last_error(None).decode())
    return out[: n.value].copy()


def count_masked_host(text: bytes, read_off, read_len, k: int, counters, low: int, up: int = 0xFFFFFFFF):
    """(kmers u64 sorted, counts u32, stats dict): the rule of `run`'s second pass on the host (pfh_count_masked_host,
    csrc/pf_run_rule.hpp; no device) -- every window of the reads that survives the masking with [low, up], counted in canonical form.
    counters: one u32 per byte of the text, the counter of the window that starts there (read at window starts only)."""
    L = load_library()
    src = np.frombuffer(bytes(text), dtype=np.uint8)
    off = np.ascontiguousarray(read_off, dtype=np.uint64)
    ln = np.ascontiguousarray(read_len, dtype=np.uint32)
    cnt = np.ascontiguousarray(counters, dtype=np.uint32)
    if len(cnt) < len(src):
        raise ValueError("count_masked_host: one counter per byte of the text")
    cap = max(int(ln.astype(np.int64).sum()), 1)
    kmers, counts = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
    n = C.c_uint64()
    stats = np.zeros(len(MASKCOUNT_STATS_FIELDS), dtype=np.uint64)
    rc = L.pfh_count_masked_host(src.ctypes.data if len(src) else None, off.ctypes.data, ln.ctypes.data, len(off), int(k),
                                 cnt.ctypes.data if len(cnt) else None, int(low), int(up), kmers.ctypes.data, counts.ctypes.data, cap, C.byref(n),
                                 stats.ctypes.data)
    if rc:
        raise ValueError("count_masked_host: k = %d: k goes from 3 to 31" % k)
    return kmers[: n.value].copy(), counts[: n.value].copy(), {f: int(v) for f, v in zip(MASKCOUNT_STATS_FIELDS, stats)}


def unitig_build_host(kmers, k: int, clip_tips: bool = False, del_isolated: bool = False, g=None):
    """(text of the GFA file as bytes, statistics): the rule of `build` on the host (pfh_unitig_build_host; no device) from canonical
    k-mers in any order"""
    L = load_library()
    km = np.ascontiguousarray(kmers, dtype=np.uint64)
    size, stats = C.c_uint64(), np.zeros(6, dtype=np.uint64)
    text = np.zeros(64 + len(km) * (int(k) + 16), dtype=np.uint8)   # the header, and at most one line (S, tabs, id, k bases, newline) and one base a k-mer
    rc = L.pfh_unitig_build_host(km.ctypes.data if len(km) else None, len(km), int(k), _unitig_g(g), int(clip_tips),
                                 int(del_isolated), text.ctypes.data, len(text), C.byref(size), stats.ctypes.data)
    if rc:
        raise ValueError("unitig_build_host: %s" % ("k goes from 3 to 31" if rc == 1 else "g goes from 1 to k - 2"))
    assert size.value <= len(text)
    return text[: size.value].tobytes(), {f: int(v) for f, v in zip(UNITIG_STATS_FIELDS, stats)}


def unitig_no_room_text(need: int, free_bytes: int, n_kmers: int) -> str:
    return load_library().pfh_unitig_no_room_text(int(need), int(free_bytes), int(n_kmers)).decode()


COLOR_SEEDS = 31   # pf_color::DEFAULT_SEEDS
COLOR_STATS = np.dtype([(f, "<u8") for f in ("colors", "reads", "windows_colored", "windows_unplaced", "windows_bad", "runs", "overflow", "lines",
                                             "table_slots", "plane_words")] + [(f, "<f8") for f in ("table_ms", "mark_ms", "runs_ms")])   # pf_color_stats
COLOR_STATS_FIELDS = ("colors", "windows_colored", "windows_unplaced", "windows_bad", "runs", "overflow")   # what the host's restatement reports
COLOR_TIMES = ("stream_s", "finish_s", "graph_s", "color_s", "serialise_s", "write_s")


def _names(names):
    arr = (C.c_char_p * max(len(names), 1))(*[os.fsencode(n) for n in names])
    return arr


def build_colored_graph(inputs, out_prefix: str, k: int = 25, clip_tips: bool = False, del_isolated: bool = False, g=None, n_seeds: int = 0,
                        chunk_bytes: int = 0, initial_slots: int = 0, fasta: bool = False) -> dict:
    """`ploidyfrost build-multi` (pfh_build_colored_fastq): the coloured graph of the FASTQ files `inputs`, one colour a file in the
    order given -- `Bifrost build -c [-i] [-d] -k <k> -r ... -o <out_prefix>` on the device (K-COUNT, K-UNITIG, K-COLOR): <out_prefix>.gfa
    and <out_prefix>.bfg_colors.  Returns the statistics of the count, the graph and the colouring, "color_bytes" and "times".  A refusal
    raises RuntimeError by name; nothing is left under either output name.  fasta (`--fasta`): a file whose first byte is '>' is
    read as FASTA (K-FASTA); assemblies and read sets may stand side by side."""
    L = load_library()
    paths, n = _paths(inputs)
    counted = np.zeros(len(COUNT_STATS_FIELDS), dtype=np.uint64)
    stats = np.zeros(1, dtype=UNITIG_STATS)
    col = np.zeros(1, dtype=COLOR_STATS)
    nb = C.c_uint64()
    times = np.zeros(6, dtype=np.float64)
    L.pfh_reads_fasta(int(bool(fasta)))
    rc = L.pfh_build_colored_fastq(paths, n, os.fsencode(out_prefix), int(k), _unitig_g(g), int(clip_tips), int(del_isolated), int(n_seeds),
                                   int(chunk_bytes), int(initial_slots), 0, counted.ctypes.data, stats.ctypes.data, col.ctypes.data, C.byref(nb),
                                   times.ctypes.data)
    if rc:
        raise RuntimeError(L.pfh_last_error(None).decode())
    d = {f: int(v) for f, v in zip(COUNT_STATS_FIELDS[:4], counted)}
    d.update({f: int(stats[0][f]) for f in UNITIG_STATS.names if f != "stage_ms"})
    d["stage_ms"] = [float(x) for x in stats[0]["stage_ms"]]
    d.update({f: col[0][f].item() for f in COLOR_STATS.names if f != "reads"})
    d["color_bytes"] = nb.value
    d["times"] = dict(zip(COLOR_TIMES, (float(x) for x in times)))
    return d


def build_colored_host(reads_per_colour, k: int, clip_tips: bool = False, del_isolated: bool = False, g=None, n_seeds: int = COLOR_SEEDS, names=None):
    """(gfa bytes, bfg_colors bytes, statistics): the rule of `build-multi` on the host (pfh_build_colored_host; no device) from the reads
    of every colour; names: the colours' names (default "c0", "c1", ...)"""
    L = load_library()
    flat = [(r if isinstance(r, bytes) else r.encode()) for reads in reads_per_colour for r in reads]
    colour_of = np.array([c for c, reads in enumerate(reads_per_colour) for _ in reads], dtype=np.uint32)
    n_colors = len(reads_per_colour)
    names = ["c%d" % c for c in range(n_colors)] if names is None else list(names)
    assert len(names) == n_colors
    arr = (C.c_char_p * max(len(flat), 1))(*flat)
    gs, cs, gst, cst = C.c_uint64(), C.c_uint64(), np.zeros(6, dtype=np.uint64), np.zeros(6, dtype=np.uint64)
    args = (arr, colour_of.ctypes.data if len(flat) else None, len(flat), n_colors, _names(names), int(k), _unitig_g(g), int(clip_tips), int(del_isolated),
            int(n_seeds))
    rc = L.pfh_build_colored_host(*args, None, 0, C.byref(gs), None, 0, C.byref(cs), None, None)
    if rc:
        raise ValueError("build_colored_host: %s" % {1: "k goes from 3 to 31", 2: "g goes from 1 to k - 2", 3: "n_seeds goes from 1 to 255"}.get(
            rc, "more than 1024 colours, or colours times k-mers of a unitig reach 2^32"))
    gfa, col = np.zeros(max(gs.value, 1), dtype=np.uint8), np.zeros(max(cs.value, 1), dtype=np.uint8)
    L.pfh_build_colored_host(*args, gfa.ctypes.data, len(gfa), C.byref(gs), col.ctypes.data, len(col), C.byref(cs), gst.ctypes.data, cst.ctypes.data)
    st = {f: int(v) for f, v in zip(UNITIG_STATS_FIELDS, gst)}
    st.update({f: int(v) for f, v in zip(COLOR_STATS_FIELDS, cst)})
    return gfa[: gs.value].tobytes(), col[: cs.value].tobytes(), st


def bfg_colors_bytes(fetched: dict, k: int, names, n_seeds: int = COLOR_SEEDS) -> bytes:
    """the bytes of the colour file (pfh_bfg_colors_bytes, csrc/host/pf_bfg_write.hpp) from what hipapi.Device.color_finish fetched"""
    L = load_library()
    heads, m, slot = (np.ascontiguousarray(fetched[f], dtype=t) for f, t in (("heads", np.uint64), ("m", np.uint32), ("slot", np.uint32)))
    run_off, runs = np.ascontiguousarray(fetched["run_off"], dtype=np.uint64), np.ascontiguousarray(fetched["runs"], dtype=np.uint32)
    n = len(heads)
    size = C.c_uint64()
    args = (heads.ctypes.data if n else None, m.ctypes.data if n else None, slot.ctypes.data if n else None, run_off.ctypes.data,
            runs.ctypes.data if len(runs) else None, n, int(k), int(n_seeds), _names(list(names)), len(names))
    if L.pfh_bfg_colors_bytes(*args, None, 0, C.byref(size)):
        raise RuntimeError(L.pfh_last_error(None).decode())
    out = np.zeros(max(size.value, 1), dtype=np.uint8)
    L.pfh_bfg_colors_bytes(*args, out.ctypes.data, len(out), C.byref(size))
    return out[: size.value].tobytes()


def color_no_room_text(need: int, free_bytes: int, n_colors: int, n_kmers: int) -> str:
    return load_library().pfh_color_no_room_text(int(need), int(free_bytes), int(n_colors), int(n_kmers)).decode()


def count_counter_bytes(cx: int, cs: int) -> int:
    return int(load_library().pfh_count_counter_bytes(int(cx), int(cs)))


def count_lut_prefix_len(k: int) -> int:
    return int(load_library().pfh_count_lut_prefix_len(int(k)))


def load_trace(reset: bool = True) -> list:
    """[(step, seconds)] of the loads of this process since the last reset (pfh_load_trace)"""
    L = load_library()
    n = L.pfh_load_trace(None, 0, 0)
    buf = C.create_string_buffer(int(n) + 1)
    L.pfh_load_trace(buf, n + 1, int(reset))
    out = []
    for ln in buf.value.decode().splitlines():
        a, b = ln.rsplit("\t", 1)
        out.append((a, float(b)))
    return out


class Run:
    """CompactedDBG::read + CDBG::CDBG of the reference's main(): graph and count table in HBM."""

    def __init__(self, gfa: str, kmc_prefix: str, z: int = 8, M: float = 2.0, D: float = -1.0, G: float = -3.0,
                 device: int = 0):
        self.L = load_library()
        self.h = self.L.pfh_open(gfa.encode(), kmc_prefix.encode(), z, M, D, G, device)
        if not self.h:
            raise RuntimeError("ploidyfrost host layer: " + self.L.pfh_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.pfh_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise hipapi.DeviceError(st, self.L.pfh_last_error(self.h).decode())

    def set_output_dir(self, d: str):
        self.L.pfh_set_output_dir(self.h, d.encode())

    def set_write_files(self, on: bool):
        self.L.pfh_set_write_files(self.h, int(on))

    def set_threads(self, threads: int):
        self.L.pfh_set_threads(self.h, threads)

    def set_align_pieces(self, n: int):
        self.L.pfh_set_align_pieces(self.h, n)

    def set_reference_threads(self, n: int):
        """n > 1: the text format of the reference's `-t n` run (deterministic row order)"""
        self._check(self.L.pfh_set_reference_threads(self.h, n))

    def set_overlap_output(self, on: bool):
        self.L.pfh_set_overlap_output(self.h, int(on))

    def set_third_tier_on_host(self, on: bool):
        self.L.pfh_set_third_tier_on_host(self.h, int(on))

    def set_batch_bubbles(self, n: int):
        self.L.pfh_set_batch_bubbles(self.h, n)

    def set_unitig_id(self, outpre: str):
        self._check(self.L.pfh_set_unitig_id(self.h, outpre.encode()))

    def find_superbubbles(self, outpre: str):
        self._check(self.L.pfh_find_superbubbles(self.h, outpre.encode()))

    def ploidy_estimation(self, outpre: str, lower: int = 10, upper: int = 1000):
        self._check(self.L.pfh_ploidy_estimation(self.h, outpre.encode(), lower, upper))

    def set_auto_cutoffs(self, q: float | None = 0.998):
        """The thresholds from the run's own database (K-HIST): max(10, cutoffL), cutoffU at quantile q of its k-mer histogram; the
        next ploidy_estimation uses them instead of its arguments.  None: off again."""
        self._check(self.L.pfh_set_auto_cutoffs(self.h, -1.0 if q is None else q))

    def cutoffs(self):
        """(lower, upper) the last ploidy_estimation used (before one: what set_auto_cutoffs derived); a colored run: one pair per
        colour"""
        n = self.L.pfh_cutoffs(self.h, None, None, 0)
        lo, up = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
        self.L.pfh_cutoffs(self.h, lo, up, n)
        pairs = [(lo[c], up[c]) for c in range(n)]
        return pairs if isinstance(self, ColoredRun) else (pairs[0] if pairs else None)

    def set_model(self, source, q: float = 0.0, lo: int = 1, hi: int = 9, m_thre: float = 5.0, n_thre: float = 2.0,
                  max_iter: int = 1000, max_delta: float = 0.01, only: bool = False):
        """The ploidy estimate in the same run: the next ploidy_estimation feeds K-GMM from the result text while it is on the
        device and writes <outpre>_model_result.txt (source "cov": as `model -f <outpre>`, "fre": as `model -g
        <outpre>_allele_frequency.txt`; lo .. hi Gaussians = ploidy lo + 1 .. hi + 1).  only: none of the ten calling files.
        source None switches it off."""
        src = -1 if source is None else MODEL_SOURCES[source]
        self._check(self.L.pfh_set_model(self.h, src, q, lo, hi, m_thre, n_thre, max_iter, max_delta, int(only)))

    def set_filter(self, simple=False, low=0, up=10000, indel=False, snp=False, num=10000, distance=-1, size=10000, frequency=0.05):
        """`ploidyfrost filter`'s row predicates in front of the model of the same run (after set_model): the next
        ploidy_estimation fits what `filter` with these options followed by `model` would read from this run's files, and writes
        no filtered table.  set_filter(None) takes the filter away again, as set_model(None) does."""
        if simple is None:
            self._check(self.L.pfh_set_filter(self.h, None))
            return
        o = filter_opts(simple, low, up, indel, snp, num, distance, size, frequency)
        self._check(self.L.pfh_set_filter(self.h, C.byref(o)))

    def set_density(self, points: int = 512, adjust: float = 1.0):
        """After set_model: the next ploidy_estimation also takes the Gaussian kernel density (ggplot2's geom_density defaults: bw.nrd0,
        `points` abscissae over [min, max]; the exact sum, on the device) of the array every fit reads, right after that fit, and
        writes <outpre>_allele_frequency_density.txt (split by colour: <outpre>_color<c>_allele_frequency_density.txt) beside the
        model result.  points=0 (or None) switches it off, as set_model(None) does."""
        self._check(self.L.pfh_set_density(self.h, int(points or 0), float(adjust)))

    def _density(self, color: int) -> dict:
        n = int(self.L.pfh_model_density_points(self.h, color))
        if n == 0:
            raise KeyError("the last ploidy_estimation took no density" + (" of colour %d" % color if color >= 0 else ""))
        x, den, info = np.zeros(n), np.zeros(n), np.zeros(1, dtype=hipapi.DENSITY_INFO)
        if color < 0:
            rc = self.L.pfh_model_density(self.h, x.ctypes.data, den.ctypes.data, info.ctypes.data)
        else:
            rc = self.L.pfh_model_color_density(self.h, color, x.ctypes.data, den.ctypes.data, info.ctypes.data)
        if rc != 0:
            raise KeyError("the last ploidy_estimation took no density")
        return hipapi.density_dict(x, den, info)

    def model_density(self) -> dict:
        """the density the last ploidy_estimation took (set_density): what Gmm.density returns"""
        return self._density(-1)

    def model_values(self) -> np.ndarray:
        """the array K-GMM fitted in the last ploidy_estimation, copied from the device"""
        n = self.L.pfh_model_values(self.h, None, 0)
        out = np.zeros(n, dtype=np.float64)
        if n and self.L.pfh_model_values(self.h, out.ctypes.data, n) != n:
            raise hipapi.DeviceError(hipapi.PF_ERR_HIP, "pfh_model_values: copy from the device failed")
        return out

    def model_result(self) -> dict:
        """{"fits": {gauss: {weights, means, vars, loglik, aic, iterations}}, "ploidy": last line of the result file, "values": n}"""
        fits = {}
        for g in range(1, 17):
            w, mean, var = (np.zeros(g) for _ in range(3))
            ll, aic, it = C.c_double(), C.c_double(), C.c_uint32()
            if self.L.pfh_model_fit(self.h, g, w.ctypes.data, mean.ctypes.data, var.ctypes.data, C.byref(ll), C.byref(aic), C.byref(it)) == 0:
                fits[g] = {"weights": w, "means": mean, "vars": var, "loglik": ll.value, "aic": aic.value, "iterations": it.value}
        return {"fits": fits, "ploidy": self.L.pfh_model_ploidy(self.h), "values": int(self.L.pfh_model_values(self.h, None, 0))}

    def text_bytes_fetched(self) -> int:
        """bytes of the ten calling streams the last ploidy_estimation copied from the device"""
        return int(self.L.pfh_text_bytes_fetched(self.h))

    def times(self) -> dict:
        t = Times()
        self.L.pfh_get_times(self.h, C.byref(t))
        d = {n: getattr(t, n) for n, _ in Times._fields_ if n != "allele"}
        d["allele"] = list(t.allele)
        return d

    def last_allele_frequency(self) -> np.ndarray:
        """bytes of <outpre>_allele_frequency.txt of the last run (copy)"""
        n = C.c_uint64()
        p = self.L.pfh_last_allele_frequency(self.h, C.byref(n))
        if not n.value:
            return np.zeros(0, dtype=np.uint8)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).copy()

    def device_ctx(self) -> int:
        return self.L.pfh_device_ctx(self.h)

    # ---- one graph over several GPUs (include/ploidyfrost_host.h; the exchange itself lives in ploidyfrost_amd/dist.py) ----
    def find_shard(self, u0: int, u1: int):
        """K-BFS + host walkers of the entrances on unitigs [u0, u1): (records as BFS_RECORD array, pool u32) copies"""
        self._check(self.L.pfh_find_shard(self.h, u0, u1))
        n = C.c_uint64()
        p = self.L.pfh_shard_records(self.h, C.byref(n))
        rec = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value * hipapi.BFS_RECORD.itemsize,)).copy().view(hipapi.BFS_RECORD) \
            if n.value else np.zeros(0, dtype=hipapi.BFS_RECORD)
        p = self.L.pfh_shard_pool(self.h, C.byref(n))
        pool = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.uint32)
        return rec, pool

    def find_replay(self, outpre: str, records: list, pools: list, write_file: bool = True, dev_records: list | None = None,
                    dev_pools: list | None = None):
        """dev_records / dev_pools: device addresses (ints) of the same shards where they already lie in device memory"""
        if records is None:   # device arrays only: (n_records, pool_len) per shard in `pools`
            n = len(pools)
            rp = pp = None
            nr = (C.c_uint64 * n)(*[int(a) for a, _ in pools])
            pl = (C.c_uint64 * n)(*[int(b) for _, b in pools])
        else:
            recs = [np.ascontiguousarray(r) for r in records]
            pls = [np.ascontiguousarray(p, dtype=np.uint32) if len(p) else np.zeros(1, dtype=np.uint32) for p in pools]
            n = len(recs)
            rp = (C.c_void_p * n)(*[r.ctypes.data if len(r) else None for r in recs])
            pp = (C.c_void_p * n)(*[p.ctypes.data for p in pls])
            nr = (C.c_uint64 * n)(*[len(r) for r in recs])
            pl = (C.c_uint64 * n)(*[len(p) for p in pools])
        dr = (C.c_void_p * n)(*[int(a) if a else None for a in dev_records]) if dev_records else None
        dp = (C.c_void_p * n)(*[int(a) if a else None for a in dev_pools]) if dev_pools else None
        self._check(self.L.pfh_find_replay(self.h, outpre.encode(), n, rp, nr, pp, int(write_file), pl, dr, dp))

    def set_write_super_bubble(self, on: bool):
        """several ranks running findSuperBubble on one graph into one directory: off on all but the rank that writes the file"""
        self.L.pfh_set_write_super_bubble(self.h, int(on))

    def set_replay_threads(self, threads: int):
        """host threads of the commit replay: 0 = sequential, -1 = default"""
        self.L.pfh_set_replay_threads(self.h, threads)

    def ploidy_select(self, lower: int, upper: int) -> int:
        n = C.c_uint64()
        self._check(self.L.pfh_ploidy_select(self.h, lower, upper, C.byref(n)))
        return n.value

    def ploidy_align(self, t0: int, t1: int) -> int:
        n = C.c_uint64()
        self._check(self.L.pfh_ploidy_align(self.h, t0, t1, C.byref(n)))
        return n.value

    def ploidy_text(self, var_count_base: int):
        """-> (sizes of the ten slabs, [sites with 2..5 alleles, coreCov, coreNum, bubbles called, bubbles])"""
        sizes = np.zeros(10, dtype=np.uint64)
        counters = np.zeros(8, dtype=np.uint64)
        self._check(self.L.pfh_ploidy_text(self.h, var_count_base, sizes.ctypes.data, counters.ctypes.data))
        return sizes, counters

    def ploidy_write(self, outpre: str, offsets, totals, truncate: bool = True):
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        t = np.ascontiguousarray(totals, dtype=np.uint64)
        self._check(self.L.pfh_ploidy_write(self.h, outpre.encode(), o.ctypes.data, t.ctypes.data, int(truncate)))

    def state(self):
        n = self.times()["unitigs"]
        f = np.empty(n, dtype=np.uint8)
        p = np.empty(n, dtype=np.uint32)
        m = np.empty(n, dtype=np.uint32)
        self.L.pfh_state(self.h, f.ctypes.data, p.ctypes.data, m.ctypes.data)
        return f, p, m


class ColoredRun(Run):
    """ColoredCDBG::read + CCDBG::CCDBG (reference src/Main.cpp:775-795): graph, colour sets, and the count
    databases of all colours joined in one HBM table."""

    def __init__(self, gfa: str, colors: str, db_prefixes: list[str], workdir: str, z: int = 8, M: float = 2.0, D: float = -1.0,
                 G: float = -3.0, threads: int = 1, device: int = 0):
        self.L = load_library()
        lst = os.path.join(workdir, "kmc_databases.txt")
        with open(lst, "w") as f:
            f.write("".join(p + "\n" for p in db_prefixes))
        self.h = self.L.pfh_open_colored(gfa.encode(), colors.encode(), lst.encode(), z, M, D, G, threads, device)
        if not self.h:
            raise RuntimeError("ploidyfrost host layer: " + self.L.pfh_last_error(None).decode())
        self.n_colors = self.L.pfh_num_colors(self.h)

    def ploidy_estimation(self, outpre: str, cutoffs=None):
        """cutoffs: one (lower, upper) per colour, the reference's -C file (None after set_auto_cutoffs: the derived ones)"""
        if cutoffs is None:
            cutoffs = self.cutoffs()
        lo = (C.c_int * self.n_colors)(*[int(c[0]) for c in cutoffs])
        up = (C.c_int * self.n_colors)(*[int(c[1]) for c in cutoffs])
        self._check(self.L.pfh_ploidy_estimation_colored(self.h, outpre.encode(), lo, up, len(cutoffs)))

    def set_filter_multi(self, color=-1, cramer=0.0, each_color=False, **opts):
        """`ploidyfrost filter-multi`'s row predicates in front of the model of the same run (after set_model, which a colored run
        accepts behind this filter only): the next ploidy_estimation fits what `filter-multi` with these options (those of
        Run.set_filter plus color and cramer) followed by `model` would read from this run's files, and writes no filtered table.
        each_color (with color=-1): one fit per colour that keeps a row, <outpre>_color<c>_model_result.txt each; model_values() is
        then the pooled array.  set_filter_multi(None) takes the filter away again, as set_model(None) does."""
        if color is None:
            self._check(self.L.pfh_set_filter_multi(self.h, None, 0))
            return
        o = filter_multi_opts(color, cramer, **opts)
        self._check(self.L.pfh_set_filter_multi(self.h, C.byref(o), int(each_color)))

    def model_colors(self) -> list:
        """the colours the last ploidy_estimation split by colour has a fit for, ascending"""
        return [int(self.L.pfh_model_color_at(self.h, i)) for i in range(self.L.pfh_model_color_count(self.h))]

    def model_values(self, color=None) -> np.ndarray:
        """the array K-GMM fitted in the last ploidy_estimation (split by colour: the pooled one); color=c: that colour's"""
        if color is None:
            return Run.model_values(self)
        n = self.L.pfh_model_color_values(self.h, int(color), None, 0)
        if n == 0xFFFFFFFFFFFFFFFF:
            raise KeyError("colour %d has no fit" % color)
        out = np.zeros(n, dtype=np.float64)
        if n:
            self.L.pfh_model_color_values(self.h, int(color), out.ctypes.data, n)
        return out

    def model_density(self, color=None) -> dict:
        """Run.model_density; color=c: the density of that colour's array after a ploidy_estimation split by colour"""
        return self._density(-1 if color is None else int(color))

    def model_result(self, color=None) -> dict:
        """Run.model_result; color=c: the fits of that colour after a ploidy_estimation split by colour"""
        if color is None:
            return Run.model_result(self)
        if int(color) not in self.model_colors():
            raise KeyError("colour %d has no fit" % color)
        fits = {}
        for g in range(1, 17):
            w, mean, var = (np.zeros(g) for _ in range(3))
            ll, aic, it = C.c_double(), C.c_double(), C.c_uint32()
            if self.L.pfh_model_color_fit(self.h, int(color), g, w.ctypes.data, mean.ctypes.data, var.ctypes.data, C.byref(ll), C.byref(aic), C.byref(it)) == 0:
                fits[g] = {"weights": w, "means": mean, "vars": var, "loglik": ll.value, "aic": aic.value, "iterations": it.value}
        return {"fits": fits, "ploidy": self.L.pfh_model_color_ploidy(self.h, int(color)), "values": len(self.model_values(color))}

    def ploidy_select(self, cutoffs) -> int:
        """scan + sequential pass with one (lower, upper) per colour; then ploidy_align / ploidy_text / ploidy_write as for Run"""
        lo = (C.c_int * len(cutoffs))(*[int(c[0]) for c in cutoffs])
        up = (C.c_int * len(cutoffs))(*[int(c[1]) for c in cutoffs])
        n = C.c_uint64()
        self._check(self.L.pfh_ploidy_select_colored(self.h, C.cast(lo, C.c_void_p), C.cast(up, C.c_void_p), len(cutoffs), C.byref(n)))
        return n.value


class Gmm:
    """`PloidyFrost model` (reference class GmmModel, src/GmmModel.hpp): readers on the host, the EM fit on the GPU."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        L, vp, d = self.L, C.c_void_p, C.c_double
        L.pfh_gmm_open.restype = vp
        L.pfh_gmm_open.argtypes = [C.c_int]
        L.pfh_gmm_close.argtypes = [vp]
        L.pfh_gmm_last_error.restype = C.c_char_p
        L.pfh_gmm_last_error.argtypes = [vp]
        L.pfh_gmm_read_fre.argtypes = [vp, C.c_char_p, d]
        L.pfh_gmm_read_cov.argtypes = [vp, C.c_char_p, d]
        L.pfh_gmm_set_values.argtypes = [vp, vp, C.c_uint64]
        L.pfh_gmm_size.restype = C.c_uint64
        L.pfh_gmm_size.argtypes = [vp]
        L.pfh_gmm_values.argtypes = [vp, vp]
        L.pfh_gmm_fit.argtypes = [vp, C.c_uint32, d, d, C.c_int32, d, vp, vp, vp, C.POINTER(d), C.POINTER(d), C.POINTER(C.c_uint32)]
        L.pfh_gmm_run.argtypes = [vp, C.c_int, C.c_int, d, d, C.c_int32, d, C.c_char_p]
        L.pfh_gmm_kernel_time.argtypes = [vp, C.c_int, C.POINTER(d), C.POINTER(C.c_uint64)]
        L.pfh_gmm_read_column.argtypes = [vp, C.c_char_p]
        L.pfh_gmm_density.argtypes = [vp, C.c_uint32, d, vp, vp, vp]
        L.pfh_gmm_write_density.argtypes = [vp, C.c_char_p, vp, C.c_uint32, vp, vp]
        L.pfh_gmm_density_time.argtypes = [vp, C.POINTER(d), C.POINTER(C.c_uint64)]
        self.h = L.pfh_gmm_open(device)
        if not self.h:
            raise RuntimeError(L.pfh_gmm_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.pfh_gmm_close(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.pfh_gmm_last_error(self.h).decode())

    def read_fre(self, path, min_frequency=0.0):
        self._check(self.L.pfh_gmm_read_fre(self.h, path.encode(), min_frequency))

    def read_cov(self, prefix, min_frequency=0.0):
        self._check(self.L.pfh_gmm_read_cov(self.h, prefix.encode(), min_frequency))

    def read_column(self, path):
        """a plain column of numbers (what script/Drawfreq.R reads): blank lines and lines beginning with '#' are skipped, every
        other line is one finite number or is refused with its line number"""
        self._check(self.L.pfh_gmm_read_column(self.h, str(path).encode()))

    def density(self, points=512, adjust=1.0) -> dict:
        """The Gaussian kernel density of the values, on the GPU: ggplot2's geom_density defaults (bandwidth adjust * bw.nrd0,
        `points` abscissae from min to max), the exact sum in fp64 (R bins onto 1024 cells and convolves by FFT: its numbers differ
        by that binning error).  {"x", "density", "bw", "n", "min", "max", "sd", "q1", "q3", "order"}; order = x(lo), x(lo+1) of
        Q(0.25), then of Q(0.75).  RuntimeError: fewer than two values, a value that is not finite, points or adjust out of range."""
        if not 0 <= int(points) < 2 ** 32:
            raise RuntimeError("density: %d points: the grid holds %d to %d" % (points, hipapi.DENSITY_MIN_POINTS, hipapi.DENSITY_MAX_POINTS))
        n = min(max(int(points), 1), hipapi.DENSITY_MAX_POINTS)
        x, den, info = np.zeros(n), np.zeros(n), np.zeros(1, dtype=hipapi.DENSITY_INFO)
        self._check(self.L.pfh_gmm_density(self.h, int(points), float(adjust), x.ctypes.data, den.ctypes.data, info.ctypes.data))
        return hipapi.density_dict(x, den, info)

    def write_density(self, outprefix, dens: dict) -> str:
        """<outprefix>_allele_frequency_density.txt from what density() returned: "# values N bandwidth BW points P", then P rows
        x<TAB>density, every number %.17g; returns the file's name"""
        x = np.ascontiguousarray(dens["x"], dtype=np.float64)
        den = np.ascontiguousarray(dens["density"], dtype=np.float64)
        if x.shape != den.shape or x.ndim != 1:
            raise ValueError("x and density are two columns of one length")
        info = np.zeros(1, dtype=hipapi.DENSITY_INFO)
        info[0]["n"], info[0]["bw"] = int(dens["n"]), float(dens["bw"])
        self._check(self.L.pfh_gmm_write_density(self.h, str(outprefix).encode(), info.ctypes.data, len(x), x.ctypes.data, den.ctypes.data))
        return str(outprefix) + "_allele_frequency_density.txt"

    def density_time(self):
        """(milliseconds, launches) of the density calls since enable_timing()"""
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.L.pfh_gmm_density_time(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_values(self, v):
        import numpy as np
        v = np.ascontiguousarray(v, dtype=np.float64)
        self._check(self.L.pfh_gmm_set_values(self.h, v.ctypes.data, len(v)))

    def values(self):
        import numpy as np
        out = np.zeros(self.L.pfh_gmm_size(self.h), dtype=np.float64)
        self._check(self.L.pfh_gmm_values(self.h, out.ctypes.data if len(out) else None) if len(out) else 0)
        return out

    def fit(self, gauss, m_thre=5.0, n_thre=2.0, max_iter=1000, max_delta=0.01):
        import numpy as np
        w, mean, var = (np.zeros(gauss) for _ in range(3))
        ll, aic, it = C.c_double(), C.c_double(), C.c_uint32()
        self._check(self.L.pfh_gmm_fit(self.h, gauss, m_thre, n_thre, max_iter, max_delta, w.ctypes.data, mean.ctypes.data,
                                       var.ctypes.data, C.byref(ll), C.byref(aic), C.byref(it)))
        return {"weights": w, "means": mean, "vars": var, "loglik": ll.value, "aic": aic.value, "iterations": it.value}

    def run(self, outprefix, lo=1, hi=9, m_thre=5.0, n_thre=2.0, max_iter=1000, max_delta=0.01):
        self._check(self.L.pfh_gmm_run(self.h, lo, hi, m_thre, n_thre, max_iter, max_delta, outprefix.encode()))

    def enable_timing(self, on=True):
        self._check(self.L.pfh_gmm_kernel_time(self.h, 1 if on else 0, None, None))

    def kernel_time(self):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.L.pfh_gmm_kernel_time(self.h, -1, C.byref(ms), C.byref(n)))
        return ms.value, n.value


# ---- blocked gzip: the rule of K-INFLATE without a device (csrc/pf_inflate_rule.hpp) ----
def _u8(data):
    a = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
    return a, (a.ctypes.data if len(a) else None)


def inflate_clause_text(clause: int) -> str:
    return load_library().pfh_inflate_clause_text(clause).decode()


def inflate_parse_member(data, n=None):
    """pfh_inflate_parse_member: (clause, dict(payload_off, member_len, crc, isize)) of the member header at data[0:]; n: the bytes up to
    the end of the file (default len(data))."""
    a, p = _u8(data)
    f = (C.c_uint32 * 4)()
    clause = load_library().pfh_inflate_parse_member(p, len(a) if n is None else n, f)
    return clause, dict(payload_off=f[0], member_len=f[1], crc=f[2], isize=f[3])


def inflate_member(payload, isize: int, guard: int = 64):
    """pfh_inflate_member: one member's deflate stream -> (clause, the bytes produced, [stored, fixed, dynamic] blocks).  The stream is
    copied to the end of a buffer of its own size and the output gets `guard` bytes behind its isize that must come back untouched."""
    a, _ = _u8(payload)
    src = np.empty(len(a), dtype=np.uint8)
    src[:] = a
    out = np.full(isize + guard, 0xA5, dtype=np.uint8)
    made, blocks = C.c_uint32(), (C.c_uint32 * 3)()
    clause = load_library().pfh_inflate_member(src.ctypes.data if len(src) else None, len(src), out.ctypes.data, isize, C.byref(made), blocks)
    if made.value > isize or not (out[isize:] == 0xA5).all():
        raise AssertionError("pfh_inflate_member wrote outside out[0, isize)")
    return clause, out[: made.value].tobytes(), list(blocks)


def inflate_bgzf_member(data, n=None):
    """pfh_inflate_bgzf_member: a whole member, header to CRC -> (clause, text, [stored, fixed, dynamic])"""
    a, p = _u8(data)
    out = np.zeros(65536, dtype=np.uint8)
    n_out, blocks = C.c_uint32(), (C.c_uint32 * 3)()
    clause = load_library().pfh_inflate_bgzf_member(p, len(a) if n is None else n, out.ctypes.data, C.byref(n_out), blocks)
    return clause, out[: n_out.value].tobytes(), list(blocks)


def inflate_bgzf(data):
    """every member of a blocked-gzip file by the host rule: the text (what Device.inflate_bgzf is held to); ValueError names a refusal"""
    a, _ = _u8(data)
    out, at, m = [], 0, 0
    while at < len(a):
        clause, text, _ = inflate_bgzf_member(a[at:])
        if clause:
            raise ValueError("member %d, byte %d: %s" % (m + 1, at, inflate_clause_text(clause)))
        out.append(text)
        at += inflate_parse_member(a[at:])[1]["member_len"]
        m += 1
    return b"".join(out)


def inflate_crc32(data, n_lanes: int = 0) -> int:
    """pfh_inflate_crc32, or with n_lanes pfh_inflate_crc32_sliced (as the kernel's lanes compute it)"""
    a, p = _u8(data)
    L = load_library()
    return L.pfh_inflate_crc32_sliced(p, len(a), n_lanes) if n_lanes else L.pfh_inflate_crc32(p, len(a))


# ---- blocked-gzip output: the rule of K-DEFLATE without a device (csrc/pf_deflate_rule.hpp) ----
DEFLATE_MEMBER_TEXT = 65280   # pf_deflate::MEMBER_TEXT, bgzip's cut
DEFLATE_EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def deflate_member(text, guard: int = 64):
    """pfh_deflate_member: one BGZF member of text (at most 65 280 bytes) -> (member bytes, (stored, fixed, dynamic), literals, matches).
    The text is copied to a buffer of its own size and the output gets `guard` bytes behind the bound's len(text) + 31 that must come
    back untouched."""
    a, _ = _u8(text)
    if len(a) > DEFLATE_MEMBER_TEXT:
        raise ValueError("a member holds at most %d bytes of text" % DEFLATE_MEMBER_TEXT)
    src = np.empty(len(a), dtype=np.uint8)
    src[:] = a
    cap = len(a) + 31
    out = np.full(cap + guard, 0xA5, dtype=np.uint8)
    res = (C.c_uint32 * 3)()
    size = load_library().pfh_deflate_member(src.ctypes.data if len(src) else None, len(src), out.ctypes.data, cap, res)
    if size < 0 or size > cap or not (out[cap:] == 0xA5).all():
        raise AssertionError("pfh_deflate_member wrote outside out[0, n + 31)")
    return out[:size].tobytes(), tuple(1 if res[0] == k else 0 for k in range(3)), int(res[1]), int(res[2])


def deflate_bgzf(text, member_text: int = DEFLATE_MEMBER_TEXT, eof: bool = True) -> bytes:
    """text cut into members of member_text bytes by the host rule, then the end-of-file marker: the file `--gz-out` writes for it (what
    Device.deflate_bgzf is held to)"""
    if not 1 <= member_text <= DEFLATE_MEMBER_TEXT:
        raise ValueError("member_text is 1 .. %d" % DEFLATE_MEMBER_TEXT)
    a, _ = _u8(text)
    return b"".join(deflate_member(a[at:at + member_text])[0] for at in range(0, len(a), member_text)) + (DEFLATE_EOF_MARKER if eof else b"")


# ---- plain gzip: the rule of K-GUNZIP without a device (csrc/pf_gunzip_rule.hpp) ----
GUNZIP_CLAUSES = ("reserved_flag", "header_past", "cut_block", "cut_trailer", "trailing", "block_too_large", "piece_limit")   # pf_gunzip::Clause, behind INFLATE_CLAUSES
GUNZIP_COUNTERS = ("pieces_found", "pieces_live", "pieces_dead", "markers", "blocks_stored", "blocks_fixed", "blocks_dynamic", "bytes_in", "bytes_out")


def gunzip_clause_text(clause: int) -> str:
    return load_library().pfh_gunzip_clause_text(clause).decode()


def gunzip_header(data, n=None):
    """pfh_gunzip_header: (clause, header length) of the member header at data[0:n]"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    ln = C.c_uint64()
    clause = load_library().pfh_gunzip_header(a.ctypes.data if len(a) else None, len(a) if n is None else n, C.byref(ln))
    return clause, ln.value


def gunzip_file_kind(first, file_size=None):
    """pfh_gunzip_file_kind: (kind, clause): kind 0 plain, 1 blocked gzip, 2 refused by `clause`, 3 gzip for K-GUNZIP"""
    a = np.frombuffer(bytes(first), dtype=np.uint8)
    clause = C.c_int()
    kind = load_library().pfh_gunzip_file_kind(a.ctypes.data if len(a) else None, len(a), len(a) if file_size is None else file_size, C.byref(clause))
    return kind, clause.value


def gunzip_candidate(data, bit: int) -> bool:
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    return bool(load_library().pfh_gunzip_candidate(a.ctypes.data if len(a) else None, len(a), bit))


def gunzip_call(comp, start_bit: int = 0, window=b"", piece_bytes: int = 0, out_cap=None):
    """pfh_gunzip_call: one call of pf_inflate_gzip's algorithm on the host -> (text, result dict, stats dict, new window), as
    Device.inflate_gzip returns them (a refused stream has result["clause"] set and no text; out_cap too small raises OverflowError)"""
    from . import hipapi
    a, w = np.frombuffer(bytes(comp), dtype=np.uint8), np.frombuffer(bytes(window), dtype=np.uint8)
    res, stats, new_w = np.zeros(1, dtype=hipapi.GUNZIP_RESULT), np.zeros(9, dtype=np.uint64), np.zeros(32768, dtype=np.uint8)
    L = load_library()
    call = lambda o, cap: L.pfh_gunzip_call(a.ctypes.data if len(a) else None, len(a), start_bit, w.ctypes.data if len(w) else None, len(w), piece_bytes,   # noqa: E731
                                            o.ctypes.data, cap, new_w.ctypes.data, res.ctypes.data, stats.ctypes.data)
    out = np.zeros(1, dtype=np.uint8)
    rc = call(out, 0 if out_cap is None else out_cap)
    if rc == -1 and out_cap is None:
        out = np.zeros(int(res[0]["out_bytes"]), dtype=np.uint8)
        rc = call(out, len(out))
    if rc == -1:
        raise OverflowError(int(res[0]["out_bytes"]))
    if rc != 0:
        raise ValueError("pfh_gunzip_call: arguments out of range")
    r = {f: int(res[0][f]) for f in hipapi.GUNZIP_RESULT.names}
    n = 0 if r["clause"] else r["out_bytes"]
    return out[:n].tobytes(), r, dict(zip(GUNZIP_COUNTERS, (int(x) for x in stats))), new_w[: r["n_window"]].tobytes()


def gunzip_member(data, piece_bytes: int = 0, block_bytes: int = 0, carry_max: int = 0, stats=None):
    """The host rule of `--gz-plain` over a whole gzip file in memory (pfh_gunzip_file): every member's text, one behind the other.  The
    file goes through the loop the stream seams run, in blocks of block_bytes (0: at once), each call cut into pieces of piece_bytes.
    ValueError names a refusal as the commands do (`member N, byte B: clause`) and carries .clause, .member, .byte.  stats: a dict
    that receives the summed counters."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    L = load_library()
    out_len, member, byte, st = C.c_uint64(), C.c_uint64(), C.c_uint64(), np.zeros(9, dtype=np.uint64)
    out = np.zeros(1, dtype=np.uint8)
    for _ in range(2):
        clause = L.pfh_gunzip_file(a.ctypes.data if len(a) else None, len(a), piece_bytes, block_bytes, carry_max, out.ctypes.data, len(out), C.byref(out_len),
                                   C.byref(member), C.byref(byte), st.ctypes.data)
        if clause or out_len.value <= len(out):
            break
        out = np.zeros(out_len.value, dtype=np.uint8)
    if clause:
        e = ValueError("member %d, byte %d: %s" % (member.value + 1, byte.value, gunzip_clause_text(clause)))
        e.clause, e.member, e.byte = clause, member.value, byte.value
        raise e
    if stats is not None:
        stats.update(zip(GUNZIP_COUNTERS, (int(x) for x in st)))
    return out[: out_len.value].tobytes()


def inflate_file_clause(first, file_size=None):
    """pfh_inflate_file_clause: (kind, clause): kind 0 plain, 1 blocked gzip, 2 refused by `clause`"""
    a, p = _u8(first)
    clause = C.c_int()
    kind = load_library().pfh_inflate_file_clause(p, len(a), len(a) if file_size is None else file_size, C.byref(clause))
    return kind, clause.value
