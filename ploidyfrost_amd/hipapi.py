"""ctypes binding of the gfx950 device layer (include/ploidyfrost_hip.h).

The library is the product; this module is plumbing so that Python callers (bench.py, the
tests, torch.distributed launchers) can drive it.  torch is imported first on purpose: PyTorch
ships its own libamdhip64.so.7, and loading it first makes this library bind to the same HIP
runtime, so torch tensors and torch streams can be handed straight to the C ABI.

There is no CPU fallback: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "csrc", "libploidyfrost_hip.so")

NONE = 0xFFFFFFFF
PF_OK, PF_ERR_ARG, PF_ERR_HIP, PF_ERR_NO_DEVICE, PF_ERR_OVERFLOW, PF_ERR_MISSING_KMER = range(6)
KERNELS = ["k_table_build", "k_adj_insert", "k_adj_probe", "k_cov", "k_bfs", "k_bfs_big", "k_align", "k_align_big",
           "k_strcov", "k_bubble", "k_bubble_big", "k_cov_colored", "k_strcov_colored", "k_gmm", "k_kmc_decode", "k_minz_count", "k_cov_join",
           "k_call_sides", "k_call_prep", "k_call_paths", "k_call_sites", "k_call_format", "k_call_snp", "k_bfs_thread", "k_call_pair", "k_call_stack", "k_cov_join_rest", "copy_text_to_host", "k_call_model"]

K_DENSITY = len(KERNELS)   # PF_K_DENSITY ("k_density"): the kernels of one pf_gmm_density, timed as one launch
K_HIST = K_DENSITY + 1     # PF_K_HIST ("k_hist"): K-HIST, the histogram of decoded counters (pf_count_histogram)
HIST_MAX_BINS = 1 << 20
K_MASK = K_HIST + 1        # PF_K_MASK ("k_mask"): everything one pf_mask_reads / pf_mask_fastq launches; unit: windows
MASK_STATS = np.dtype([(f, "<u8") for f in ("reads", "reads_changed", "bases", "bases_masked", "kmers", "kmers_bad")])   # pf_mask_stats
MASK_NO_UPPER = 0xFFFFFFFF
K_COUNT = K_MASK + 1       # PF_K_COUNT ("k_count"): everything one pf_count_reads / pf_count_fastq launches; unit: windows
COUNT_STATS = np.dtype([(f, "<u8") for f in ("reads", "bases", "kmers", "kmers_bad", "unique", "below_min", "above_max", "written")])   # pf_count_stats
K_TRIM = K_COUNT + 1       # PF_K_TRIM ("k_trim"): everything one pf_trim_fastq / pf_trim_fastq_pair launches; unit: records
TRIM_STEP = np.dtype([("kind", "<u4"), ("a", "<u4"), ("b", "<u4")])   # pf_trim_step
TRIM_STATS = np.dtype([(f, "<u8") for f in ("reads", "kept", "dropped", "bases", "bases_kept", "both", "only1", "only2", "neither")])   # pf_trim_stats
K_UNITIG = K_TRIM + 1      # PF_K_UNITIG ("k_unitig"): everything one pf_unitig_build launches; unit: k-mers
K_MASKCOUNT = K_UNITIG + 1   # PF_K_MASKCOUNT ("k_maskcount"): everything one pf_maskcount_reads / pf_maskcount_fastq launches; unit: windows
MASKCOUNT_STATS = np.dtype([(f, "<u8") for f in ("reads", "bases", "kmers", "kmers_invalid", "kmers_bad", "kmers_kept")])   # pf_maskcount_stats
K_UNION = K_MASKCOUNT + 1    # PF_K_UNION ("k_union"): everything one pf_kmer_union launches; unit: keys given
K_COLORSET = K_UNION + 1     # PF_K_COLORSET ("k_colorset"): the kernel of one pf_color_kmers; unit: keys
K_TRIMCOUNT = K_COLORSET + 1   # PF_K_TRIMCOUNT ("k_trimcount"): everything one pf_*_trimmed / pf_trim_table_* call launches; unit: records
K_INFLATE = K_TRIMCOUNT + 1    # PF_K_INFLATE ("k_inflate"): everything one pf_inflate_bgzf launches; unit: inflated bytes
K_GUNZIP = K_INFLATE + 1       # PF_K_GUNZIP ("k_gunzip"): everything one pf_inflate_gzip launches; unit: inflated bytes
K_FASTA = K_GUNZIP + 1         # PF_K_FASTA ("k_fasta"): everything the index of one pf_fasta_index / pf_*_fasta call launches; unit: bytes of the chunk
K_DEFLATE = K_FASTA + 1        # PF_K_DEFLATE ("k_deflate"): everything one pf_deflate_bgzf launches; unit: bytes of text
K_CLIP = K_DEFLATE + 1         # PF_K_CLIP ("k_clip"): the clipping kernels of one trim / trimmed-count call while a clip is open; unit: records
K_PALIN = K_CLIP + 1           # PF_K_PALIN ("k_palin"): palindrome mode's kernel of one paired trim / trimmed-count call while a clip with prefix pairs is open; unit: pairs
K_QC = K_PALIN + 1             # PF_K_QC ("k_qc"): the report kernel of one qc_fastq call, or of one trim / trimmed-count call per file while a report is open; unit: records
QC_TABLE_WORDS, QC_CLIP_WORDS = 9515, 1025   # PF_QC_TABLE_WORDS, PF_QC_CLIP_WORDS
K_HETPAIR = K_QC + 1           # PF_K_HETPAIR ("k_hetpair"): everything one pf_hetpairs launches (flag, scan, write, table); unit: keys in range
HETPAIR_STATS = np.dtype([(f, "<u8") for f in ("kmers", "in_range", "one_partner", "many_partners", "pairs")])   # pf_hetpair_stats
K_DEDUP = K_HETPAIR + 1         # PF_K_DEDUP ("k_dedup"): the kernels of one trim / trimmed-count call while a dedup is open, or of one dedup_keys; unit: units that take part
DEDUP_STATS = np.dtype([(f, "<u8") for f in ("units", "unique", "duplicates", "max_copies")] + [("levels", "<u8", (10,)), ("slots", "<u8"), ("growths", "<u8")])   # pf_dedup_stats
HETPAIR_MAX_W = 4096           # pf_hetpair::MAX_W: upper - lower + 1 of a table
CLIP_PAIR_STATS = np.dtype([("pairs_clipped", "<u8"), ("pairs_dropped", "<u8"), ("pairs_too_long", "<u8"), ("candidates_scored", "<u8"),
                            ("bases_clipped", "<u8", (2,))])   # pf_clip_pair_stats
CLIP_STATS = np.dtype([(f, "<u8", (2,)) for f in ("reads_clipped", "reads_dropped", "bases_clipped", "candidates_scored")])   # pf_clip_stats
FASTA_TILE = 4096              # PF_FASTA_TILE: bytes of the chunk one block of K-FASTA's compaction kernel takes at a time
GUNZIP_RESULT = np.dtype([("out_bytes", "<u8"), ("end_bit", "<u8"), ("final", "<u4"), ("n_window", "<u4"), ("crc_raw", "<u4"), ("clause", "<u4"),
                          ("clause_bit", "<u8")])   # pf_gunzip_result
GUNZIP_COUNTERS = ("pieces_found", "pieces_live", "pieces_dead", "markers", "blocks_stored", "blocks_fixed", "blocks_dynamic", "bytes_in", "bytes_out")
GUNZIP_STAGES = ("find", "count", "decode", "window", "resolve")
GUNZIP_STATS = np.dtype([(f, "<u8") for f in GUNZIP_COUNTERS] + [("stage_ms", "<f8", (5,))])   # pf_gunzip_stats
INFLATE_STATS = np.dtype([(f, "<u8") for f in ("members", "bytes_in", "bytes_out", "blocks_stored", "blocks_fixed", "blocks_dynamic")])   # pf_inflate_stats
DEFLATE_STATS = np.dtype([(f, "<u8") for f in ("members", "bytes_in", "bytes_out", "blocks_stored", "blocks_fixed", "blocks_dynamic", "literals", "matches")])   # pf_deflate_stats
UNION_TILE = 1024            # pf_runmulti::UNION_TILE: merged positions a block of K-UNION takes
UNION_ITEMS = 4              # pf_runmulti::UNION_ITEMS: ... and a lane
COLOR_KMERS_STATS = np.dtype([(f, "<u8") for f in ("kmers", "kmers_colored", "kmers_unplaced")])   # pf_color_kmers_stats
UNITIG_G_DEFAULT = 0xFFFFFFFF   # PF_UNITIG_G_DEFAULT: Bifrost's default for k
COLOR_SEEDS = 31                # pf_color::DEFAULT_SEEDS: placement rounds of a colour file
COLOR_STATS = np.dtype([(f, "<u8") for f in ("colors", "reads", "windows_colored", "windows_unplaced", "windows_bad", "runs", "overflow", "lines",
                                             "table_slots", "plane_words")] + [(f, "<f8") for f in ("table_ms", "mark_ms", "runs_ms")])   # pf_color_stats
UNITIG_STAGES = ("index", "adjacency", "simplify", "rank", "cycles", "emit")
UNITIG_STATS = np.dtype([(f, "<u8") for f in ("distinct", "unitigs", "removed", "unitigs_out", "longest", "bytes", "cycles", "rounds", "cycle_rounds")] +
                        [("stage_ms", "<f8", (len(UNITIG_STAGES),))])   # pf_unitig_stats
TRIM_KINDS = {"LEADING": 1, "TRAILING": 2, "SLIDINGWINDOW": 3, "MINLEN": 4}   # PF_TRIM_LEADING ..
DENSITY_INFO = np.dtype([("n", "<u8"), ("min", "<f8"), ("max", "<f8"), ("sd", "<f8"), ("q1", "<f8"), ("q3", "<f8"), ("bw", "<f8"),
                         ("order", "<f8", (4,))])   # pf_density_info
assert DENSITY_INFO.itemsize == 88
DENSITY_MIN_POINTS, DENSITY_MAX_POINTS = 2, 4096

BFS_RECORD = np.dtype([("entrance", "<u4"), ("exit", "<u4"), ("n_seen", "<u4"), ("n_list", "<u4"), ("list_off", "<u8"),
                       ("outcome", "u1"), ("flag_cycle", "u1"), ("flag_tip", "u1"), ("strict", "u1"), ("pad", "<u4")])
ALIGN_JOB = np.dtype([("a_off", "<u8"), ("b_off", "<u8"), ("a_len", "<u4"), ("b_len", "<u4")])
ALIGN_HIT = np.dtype([("text_off", "<u8"), ("gap_off", "<u8"), ("len", "<u4"), ("n_gaps", "<u4"), ("score", "<i8"),
                      ("n_pos", "<u4"), ("n_indel", "<u4")])
CALL_SIDE = np.dtype([("u", "<u4"), ("exit_ov", "<u4"), ("err_unitig", "<u4"), ("plus_side", "u1"), ("kind", "u1"), ("aligned", "u1"),
                      ("err", "u1")])
CALL_RESULT = np.dtype([("text_len", "<u8", (10,)), ("allele", "<u8", (4,)), ("core_cov", "<u8"), ("core_num", "<u8"), ("n_called", "<u8"),
                        ("align_jobs", "<u8"), ("site_strings", "<u8"), ("n_branching", "<u8"),
                        ("snp_jobs", "<u8"), ("pair_jobs", "<u8"), ("wave_jobs", "<u8"), ("stack_jobs", "<u8"),
                        ("alignseq_packed_len", "<u8"), ("numeric_packed", "<u8")])
CALL_STREAMS = ["allele_frequency", "alignseq", "bifre", "trifre", "tetrafre", "pentafre", "bicov", "tricov", "tetracov", "pentacov"]
BUBBLE_PATH = np.dtype([("text_off", "<u8"), ("len", "<u4"), ("ov", "<u4")])
BUBBLE_TASK = np.dtype([("path_first", "<u8"), ("n_paths", "<u4"), ("pad", "<u4")])
BUBBLE_SITE = np.dtype([("col", "<u4"), ("is_indel", "u1"), ("maxnum", "u1"), ("pad", "<u2")])
BUBBLE_RESULT = np.dtype([("rows_off", "<u8"), ("site_off", "<u8"), ("group_off", "<u8"), ("ilen_off", "<u8"), ("n_rows", "<u4"),
                          ("n_cols", "<u4"), ("n_sites", "<u4"), ("n_indel_len", "<u4")])
CALL_BUBBLE = np.dtype([("entrance_ov", "<u4"), ("exit_ov", "<u4"), ("strict", "<u4"), ("n_inner", "<u4"), ("inner", "<u4", (4,)),
                        ("cov", "<f8", (4,)), ("core_mean", "<f8"), ("cov_sum", "<f8")])
assert CALL_BUBBLE.itemsize == 80
assert BFS_RECORD.itemsize == 32 and ALIGN_JOB.itemsize == 24 and ALIGN_HIT.itemsize == 40
assert BUBBLE_PATH.itemsize == 16 and BUBBLE_TASK.itemsize == 16 and BUBBLE_SITE.itemsize == 8 and BUBBLE_RESULT.itemsize == 48

_lib = None


class DeviceError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__("ploidyfrost_hip status %d: %s" % (status, msg))
        self.status = status


def load_library() -> C.CDLL:
    """Load libploidyfrost_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the device layer)" % LIB_PATH)
    try:
        import torch  # noqa: F401  (binds libamdhip64.so.7 first, see module docstring)
    except Exception:  # pragma: no cover - torch is optional for pure ctypes use
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    sig = {
        "pf_create": (i, [i, C.POINTER(vp)]),
        "pf_warmup": (i, [i]),
        "pf_destroy": (None, [vp]),
        "pf_last_error": (C.c_char_p, [vp]),
        "pf_set_stream": (i, [vp, vp]),
        "pf_synchronize": (i, [vp]),
        "pf_enable_timing": (i, [vp, i]),
        "pf_kernel_time": (i, [vp, i, C.POINTER(C.c_double), C.POINTER(u64)]),
        "pf_reset_timing": (i, [vp]),
        "pf_device_busy": (i, [vp, vp, vp]),
        "pf_kernel_units": (i, [vp, i, C.POINTER(u64)]),
        "pf_side_components": (i, [vp, i, vp, u64, vp, u64, vp, u64, vp, u64]),
        "pf_bfs_candidates_begin": (i, [vp, C.c_uint32, C.c_uint32, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), vp, vp, u64, C.POINTER(u64)]),
        "pf_bfs_candidates_end": (i, [vp]),
        "pf_bfs_candidates_split": (i, [vp, C.c_uint32, C.c_uint32, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), vp, u64, C.POINTER(u64)]),
        "pf_fetch": (i, [vp, vp, vp, u64]),
        "pf_bfs_candidates_resident": (i, [vp, C.c_uint32, C.c_uint32, C.POINTER(u64), C.POINTER(u64), vp, vp, u64, C.POINTER(u64)]),
        "pf_replay_device": (i, [vp, C.c_uint32, C.c_uint32, C.POINTER(u64), C.POINTER(u64)]),
        "pf_replay_big_fetch": (i, [vp, vp, vp, vp]),
        "pf_replay_set_colours": (i, [vp, C.c_uint32, vp, vp, vp]),
        "pf_replay_finish": (i, [vp, vp, vp, vp, u64]),
        "pf_call_get_state": (i, [vp, vp, vp, vp]),
        "pf_gfa_ingest": (i, [vp, vp, u64, i, i, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "pf_gfa_parse": (i, [vp, vp, u64, i, i, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "pf_gfa_upload": (i, [vp]),
        "pf_gfa_error": (C.c_char_p, [vp]),
        "pf_gfa_segments": (i, [vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]),
        "pf_replay_order": (i, [vp, C.c_uint32, vp, vp, vp]),
        "pf_kernel_name": (C.c_char_p, [i]),
        "pf_upload_graph": (i, [vp, vp, vp, vp, u32, i]),
        "pf_build_adjacency": (i, [vp, vp, vp]),
        "pf_upload_counts": (i, [vp, vp, vp, u64, u32, u64, u64, i]),
        "pf_join_counts": (i, [vp]),
        "pf_join_counts_begin": (i, [vp]),
        "pf_join_counts_end": (i, [vp]),
        "pf_lookup_kmers": (i, [vp, vp, u64, vp, vp]),
        "pf_unitig_cov": (i, [vp, u32, u32, vp, vp, vp]),
        "pf_unitig_cov_probe": (i, [vp, u32, u32, vp, vp, vp]),
        "pf_count_candidates": (i, [vp, u32, u32, C.POINTER(u64)]),
        "pf_bfs_candidates": (i, [vp, u32, u32, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]),
        "pf_align_batch": (i, [vp, vp, u64, vp, u32, C.c_double, C.c_double, C.c_double, vp, vp, vp, u64, vp, u64, vp, u64,
                               C.POINTER(u64)]),
        "pf_align_bubbles": (i, [vp, vp, u64, vp, u64, vp, u32, C.c_double, C.c_double, C.c_double, vp, vp, u64, vp, u64, vp, u64,
                                 vp, u64, C.POINTER(u64)]),
        "pf_string_cov": (i, [vp, vp, vp, u32, u32, u32, vp, vp, vp]),
        "pf_host_alloc": (i, [vp, C.c_size_t, C.POINTER(vp)]),
        "pf_selftest_scan": (i, [vp, u64, C.c_uint32]),
        "pf_call_set_numeric_packed": (i, [vp, i]),
        "pf_call_fetch_text": (i, [vp, i, i, vp, u64]),
        "pf_host_free": (None, [vp, vp]),
        "pf_device_name": (i, [vp, C.c_char_p, C.c_size_t]),
        "pf_device_pci_bus_id": (i, [vp, C.c_char_p, C.c_size_t]),
        "pf_table_capacity": (u64, [vp]),
        "pf_num_kmers": (u64, [vp]),
        "pf_upload_counts_colored": (i, [vp, u32, vp, vp, vp, vp, vp, vp]),
        "pf_num_colors": (u32, [vp]),
        "pf_unitig_cov_colored": (i, [vp, u32, u32, vp, vp, vp, vp]),
        "pf_unitig_cov_colored_probe": (i, [vp, u32, u32, vp, vp, vp, vp]),
        "pf_string_cov_colored": (i, [vp, vp, vp, u32, vp, vp, vp, vp]),
        "pf_unitig_cov_exact": (i, [vp, u32, u32, i, vp, vp, vp]),
        "pf_minimizer_table_slots": (u64, [u64]),
        "pf_minimizer_crowding": (i, [vp, i, u32, vp, vp, vp]),
        "pf_minimizer_replay_inputs": (i, [vp, i, C.c_uint32, vp, vp]),
        "pf_kmc_decode": (i, [vp, vp, u64, u32, u32, vp, u64, u32, u32, vp, vp]),
        "pf_device_free": (None, [vp, vp]),
        "pf_copy_to_host": (i, [vp, vp, vp, C.c_size_t]),
        "pf_gmm_upload": (i, [vp, vp, u64]),
        "pf_gmm_count": (u64, [vp]),
        "pf_gmm_fit": (i, [vp, u32, C.c_double, C.c_double, C.c_int32, C.c_double, vp, vp, vp, vp, vp]),
        "pf_call_set_state": (i, [vp, vp, vp, vp]),
        "pf_call_coverage": (i, [vp]),
        "pf_call_set_format": (i, [vp, i]),
        "pf_superbubble_rows": (i, [vp, i, C.POINTER(u64), C.POINTER(u64)]),
        "pf_superbubble_fetch": (i, [vp, vp, u64]),
        "pf_call_scan": (i, [vp, u32, u32, C.POINTER(u64)]),
        "pf_call_sides": (i, [vp, vp, u64]),
        "pf_call_resolve": (i, [vp, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32)]),
        "pf_call_select": (i, [vp, vp, u64]),
        "pf_call_run": (i, [vp, i, u64, u64, u64, u32, C.c_double, C.c_double, C.c_double, vp]),
        "pf_call_align": (i, [vp, u64, u64, u32, C.c_double, C.c_double, C.c_double, vp]),
        "pf_call_text": (i, [vp, i, u64, vp]),
        "pf_call_set_alignseq_packed": (i, [vp, i]),
        "pf_comm_unique_id": (i, [vp]),
        "pf_comm_init": (i, [vp, vp, i, i]),
        "pf_gather": (i, [vp, vp, C.c_uint32, vp]),
        "pf_comm_destroy": (None, [vp]),
        "pf_call_peek": (i, [vp, i, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp]),
        "pf_call_reserve": (i, [vp, u64, C.c_uint32]),
        "pf_call_reserve_lanes": (i, [vp, u64, C.c_uint32, C.c_int]),
        "pf_timing_select": (i, [vp, u64]),
        "pf_kernel_busy": (i, [vp, u64, C.POINTER(C.c_double)]),
        "pf_call_reserve_text": (i, [vp, u64]),
        "pf_find_reserve": (i, [vp, u64]),
        "pf_call_set_colours": (i, [vp, u32, vp, vp, vp, vp, vp, vp, u64, u64]),
        "pf_call_set_cutoffs": (i, [vp, u32, vp, vp]),
        "pf_call_text_range": (i, [vp, i, u64, u64, u64, vp]),
        "pf_call_align_lane": (i, [vp, i, u64, u64, u32, C.c_double, C.c_double, C.c_double, vp]),
        "pf_call_text_range_lane": (i, [vp, i, i, u64, u64, u64, vp]),
        "pf_call_text_sizes": (i, [vp, i, u64, u64, u64, vp]),
        "pf_bfs_live_deferred": (i, [vp, u64, vp]),
        "pf_bfs_live_count": (i, [vp, vp]),
        "pf_call_fetch": (i, [vp, i, i, vp, u64]),
        "pf_call_fetch_slab": (i, [vp, i, vp, vp]),
        "pf_call_fetch_range": (i, [vp, i, u64, vp, u64, i]),
        "pf_call_fetch_wait": (i, [vp, i]),
        "pf_format_doubles": (i, [vp, vp, u64, vp, vp]),
        "pf_gmm_values": (i, [vp, vp, u64]),
        "pf_call_model_begin": (i, [vp, i, C.c_double]),
        "pf_call_model_take": (i, [vp, i]),
        "pf_call_model_finish": (i, [vp, C.POINTER(u64)]),
        "pf_call_fetched_bytes": (u64, [vp]),
        "pf_call_model_filter": (i, [vp, vp]),
        "pf_call_model_take_text": (i, [vp, i, C.c_char_p, u64]),
        "pf_call_model_filter_multi": (i, [vp, vp, i]),
        "pf_call_model_color_count": (C.c_uint32, [vp]),
        "pf_call_model_color_select": (i, [vp, i, C.POINTER(u64)]),
        "pf_gmm_density": (i, [vp, u32, C.c_double, vp, vp, vp]),
        "pf_count_histogram": (i, [vp, vp, u64, u64, u64, u32, vp]),
        "pf_mask_reads": (i, [vp, vp, u64, vp, vp, u64, u32, u32, vp, vp]),
        "pf_mask_fastq": (i, [vp, vp, u64, i, u32, u32, vp, C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_count_begin": (i, [vp, u32, i, u64]),
        "pf_count_reads": (i, [vp, vp, u64, vp, vp, u64, vp]),
        "pf_count_fastq": (i, [vp, vp, u64, i, C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_count_finish": (i, [vp, u64, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), vp]),
        "pf_count_abort": (i, [vp]),
        "pf_kmc_encode": (i, [vp, vp, vp, u64, u32, u32, u32, vp, vp]),
        "pf_unitig_build": (i, [vp, vp, u64, u32, u32, i, i, vp]),
        "pf_unitig_fetch": (i, [vp, u64, u64, vp]),
        "pf_unitig_release": (i, [vp]),
        "pf_unitig_text": (i, [vp, C.POINTER(vp), C.POINTER(u64)]),
        "pf_maskcount_reads": (i, [vp, vp, u64, vp, vp, u64, u32, u32, vp]),
        "pf_maskcount_fastq": (i, [vp, vp, u64, i, u32, u32, C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_unitig_build_colored": (i, [vp, vp, u64, u32, u32, i, i, u32, vp, C.POINTER(u64)]),
        "pf_color_begin": (i, [vp, u32]),
        "pf_color_reads": (i, [vp, u32, vp, u64, vp, vp, u64, vp]),
        "pf_color_fastq": (i, [vp, u32, vp, u64, i, C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_color_finish": (i, [vp, vp]),
        "pf_color_kmers": (i, [vp, u32, vp, u64, vp]),
        "pf_release_counts": (i, [vp]),
        "pf_kmer_union": (i, [vp, u32, vp, vp, C.POINTER(vp), C.POINTER(u64)]),
        "pf_color_fetch": (i, [vp, vp, vp, vp, vp, vp]),
        "pf_trim_fastq": (i, [vp, vp, u64, i, vp, u32, u32, vp, C.POINTER(u64), C.POINTER(u64), vp, vp, C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_trim_fastq_pair": (i, [vp, vp, u64, vp, u64, i, vp, u32, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(vp), C.POINTER(vp),
                                   C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_device_alloc": (i, [vp, C.c_size_t, C.POINTER(vp)]),
        "pf_copy": (i, [vp, vp, vp, C.c_size_t]),
        "pf_inflate_bgzf": (i, [vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_inflate_gzip": (i, [vp, vp, u64, u64, vp, u32, u32, vp, u64, vp, vp, vp]),
        "pf_deflate_bgzf": (i, [vp, vp, u64, u32, vp, u64, C.POINTER(u64), vp, vp]),
        "pf_fasta_index": (i, [vp, vp, u64, i, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
        "pf_fasta_index_fetch": (i, [vp, vp, u64, i, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, u64, vp, vp, u64]),
        "pf_count_fasta": (i, [vp, vp, u64, i, C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_maskcount_fasta": (i, [vp, vp, u64, i, u32, u32, C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_color_fasta": (i, [vp, u32, vp, u64, i, C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_trim_table_fastq": (i, [vp, vp, u64, i, vp, vp, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, C.POINTER(u64)]),
        "pf_trim_table_fastq_pair": (i, [vp, vp, u64, vp, u64, i, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp,
                                         C.POINTER(u64)]),
        "pf_count_fastq_trimmed": (i, [vp, vp, u64, i, vp, C.POINTER(u64), vp, vp, C.POINTER(u64)]),
        "pf_count_fastq_pair_trimmed": (i, [vp, vp, u64, vp, u64, i, vp, C.POINTER(u64), vp, vp, C.POINTER(u64)]),
        "pf_maskcount_fastq_trimmed": (i, [vp, vp, u64, i, vp, u32, u32, C.POINTER(u64), vp, vp, C.POINTER(u64)]),
        "pf_maskcount_fastq_pair_trimmed": (i, [vp, vp, u64, vp, u64, i, vp, u32, u32, C.POINTER(u64), vp, vp, C.POINTER(u64)]),
        "pf_clip_begin": (i, [vp, vp, vp, vp, u32, u32, u32]),
        "pf_clip_begin_pairs": (i, [vp, vp, vp, vp, u32, vp, vp, u32, u32, u32, u32, u32, i]),
        "pf_clip_pair_stats_get": (i, [vp, vp]),
        "pf_clip_stats_get": (i, [vp, vp]),
        "pf_clip_end": (i, [vp]),
        "pf_clip_last_ends": (i, [vp, i, vp, u64]),
        "pf_qc_begin": (i, [vp, u32]),
        "pf_qc_get": (i, [vp, i, i, vp]),
        "pf_qc_clip_get": (i, [vp, i, vp]),
        "pf_qc_fastq": (i, [vp, i, vp, u64, i, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "pf_qc_end": (i, [vp]),
        "pf_hetpairs": (i, [vp, vp, vp, u64, u32, u32, u32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), vp]),
        "pf_hetpair_table": (i, [vp, vp, vp, u64, u32, u32, vp]),
        "pf_dedup_begin": (i, [vp, u32, u64]),
        "pf_dedup_stats_get": (i, [vp, vp]),
        "pf_dedup_end": (i, [vp]),
        "pf_dedup_keys": (i, [vp, vp, u64, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError = header / library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


DECLARED_SYMBOLS = ["pf_create", "pf_warmup", "pf_destroy", "pf_last_error", "pf_set_stream", "pf_synchronize", "pf_enable_timing",
                    "pf_kernel_time", "pf_reset_timing", "pf_device_busy", "pf_kernel_units", "pf_side_components", "pf_replay_order", "pf_bfs_candidates_begin", "pf_bfs_candidates_end", "pf_fetch", "pf_bfs_candidates_resident", "pf_bfs_live_deferred", "pf_bfs_live_count", "pf_replay_device", "pf_replay_big_fetch", "pf_replay_set_colours", "pf_replay_finish", "pf_call_get_state", "pf_gfa_ingest", "pf_gfa_segments", "pf_gfa_parse", "pf_gfa_upload", "pf_gfa_error", "pf_kernel_name", "pf_upload_graph", "pf_build_adjacency",
                    "pf_upload_counts", "pf_join_counts", "pf_join_counts_begin", "pf_join_counts_end", "pf_lookup_kmers", "pf_unitig_cov", "pf_count_candidates", "pf_bfs_candidates",
                    "pf_align_batch", "pf_align_bubbles", "pf_string_cov", "pf_host_alloc", "pf_host_free", "pf_device_name", "pf_device_pci_bus_id", "pf_table_capacity", "pf_num_kmers",
                    "pf_upload_counts_colored", "pf_num_colors", "pf_unitig_cov_colored", "pf_string_cov_colored",
                    "pf_gmm_upload", "pf_gmm_count", "pf_gmm_fit", "pf_kmc_decode", "pf_device_free", "pf_copy_to_host",
                    "pf_minimizer_table_slots", "pf_minimizer_crowding", "pf_minimizer_replay_inputs", "pf_bfs_candidates_split", "pf_unitig_cov_exact", "pf_unitig_cov_probe", "pf_unitig_cov_colored_probe",
                    "pf_call_set_state", "pf_call_set_format", "pf_superbubble_rows", "pf_superbubble_fetch", "pf_call_coverage", "pf_call_scan", "pf_call_sides", "pf_call_resolve", "pf_call_select", "pf_call_run", "pf_call_align",
                    "pf_call_text", "pf_call_set_alignseq_packed", "pf_comm_unique_id", "pf_comm_init", "pf_gather", "pf_comm_destroy", "pf_call_reserve", "pf_call_reserve_lanes", "pf_timing_select", "pf_kernel_busy", "pf_call_reserve_text", "pf_selftest_scan", "pf_call_set_numeric_packed", "pf_call_fetch_text", "pf_find_reserve", "pf_call_set_colours", "pf_call_set_cutoffs", "pf_call_peek", "pf_call_text_range", "pf_call_align_lane", "pf_call_text_range_lane", "pf_call_text_sizes", "pf_call_fetch", "pf_call_fetch_slab", "pf_call_fetch_range", "pf_call_fetch_wait", "pf_format_doubles",
                    "pf_gmm_values", "pf_call_model_begin", "pf_call_model_take", "pf_call_model_finish", "pf_call_fetched_bytes",
                    "pf_call_model_filter", "pf_call_model_take_text",
                    "pf_call_model_filter_multi", "pf_call_model_color_count", "pf_call_model_color_select",
                    "pf_gmm_density", "pf_count_histogram", "pf_mask_reads", "pf_mask_fastq",
                    "pf_count_begin", "pf_count_reads", "pf_count_fastq", "pf_count_finish", "pf_count_abort", "pf_kmc_encode",
                    "pf_trim_fastq", "pf_trim_fastq_pair", "pf_unitig_build", "pf_unitig_fetch", "pf_unitig_release",
                    "pf_unitig_build_colored", "pf_color_begin", "pf_color_reads", "pf_color_fastq", "pf_color_finish", "pf_color_fetch",
                    "pf_maskcount_reads", "pf_maskcount_fastq", "pf_unitig_text",
                    "pf_kmer_union", "pf_color_kmers", "pf_release_counts",
                    "pf_trim_table_fastq", "pf_trim_table_fastq_pair", "pf_count_fastq_trimmed", "pf_count_fastq_pair_trimmed",
                    "pf_maskcount_fastq_trimmed", "pf_maskcount_fastq_pair_trimmed", "pf_inflate_bgzf", "pf_inflate_gzip", "pf_device_alloc", "pf_copy",
                    "pf_fasta_index", "pf_fasta_index_fetch", "pf_count_fasta", "pf_maskcount_fasta", "pf_color_fasta", "pf_deflate_bgzf",
                    "pf_clip_begin", "pf_clip_stats_get", "pf_clip_end", "pf_clip_last_ends",
                    "pf_clip_begin_pairs", "pf_clip_pair_stats_get",
                    "pf_qc_begin", "pf_qc_get", "pf_qc_clip_get", "pf_qc_fastq", "pf_qc_end",
                    "pf_hetpairs", "pf_hetpair_table",
                    "pf_dedup_begin", "pf_dedup_stats_get", "pf_dedup_end", "pf_dedup_keys"]


class TrimPlan(C.Structure):   # pf_trim_plan
    _fields_ = [("steps", C.c_void_p), ("n_steps", C.c_uint32), ("phred", C.c_uint32)]


def trim_steps(steps) -> np.ndarray:
    """a TRIM_STEP array from Trimmomatic's words ("LEADING:10", "SLIDINGWINDOW:3:20", ...), tuples (kind, a[, b]) or such an array.
    Nothing is checked here: the library refuses bad steps by name."""
    if isinstance(steps, np.ndarray) and steps.dtype == TRIM_STEP:
        return np.ascontiguousarray(steps)
    if isinstance(steps, str):
        steps = steps.split()
    out = np.zeros(len(steps), dtype=TRIM_STEP)
    for j, s in enumerate(steps):
        if isinstance(s, str):
            name, *fields = s.split(":")
            s = (TRIM_KINDS[name],) + tuple(int(x) for x in fields)
        out[j] = tuple(s) + (0,) * (3 - len(s))
    return out


def density_dict(x: np.ndarray, density: np.ndarray, info: np.ndarray) -> dict:
    """grid, curve and pf_density_info record as the dict the Python layers return"""
    r = info[0]
    return {"x": x, "density": density, "bw": float(r["bw"]), "n": int(r["n"]), "min": float(r["min"]), "max": float(r["max"]),
            "sd": float(r["sd"]), "q1": float(r["q1"]), "q3": float(r["q3"]), "order": np.array(r["order"], dtype=np.float64)}


def call_peek(ctx_handle, lane: int = 0):
    """pf_call_peek on a raw pf_ctx (e.g. hostapi.Run.device_ctx()): what pf_call_align left resident, per bubble a dict with
    entrance_ov / exit_ov / strict / inner / cov, and -- when an alignment survived -- rows, sites [(col, is_indel, maxnum, groups,
    ok)], indel_len and, for a branching bubble, site_cov = per site (group coverages, their sum)."""
    L = load_library()
    h = C.c_void_p(ctx_handle)
    used = (C.c_uint64 * 6)()
    st = L.pf_call_peek(h, lane, None, None, None, 0, None, None, None, None, None, None, used)
    if st != PF_OK:
        raise DeviceError(st, L.pf_last_error(h).decode())
    nb = int(used[0])
    if nb == 0:
        return []
    cap = (C.c_uint64 * 5)(*[int(used[x + 1]) for x in range(5)])
    bub = np.zeros(nb, dtype=CALL_BUBBLE)
    res = np.zeros(nb, dtype=BUBBLE_RESULT)
    sv_off = np.zeros(nb, dtype=np.uint64)
    text = np.zeros(max(1, cap[0]), dtype=np.uint8)
    sites = np.zeros(max(1, cap[1]), dtype=BUBBLE_SITE)
    groups = np.zeros(max(1, cap[2]), dtype=np.uint8)
    ilen = np.zeros(max(1, cap[3]), dtype=np.uint32)
    sv = np.zeros(max(1, cap[4]), dtype=np.float64)
    st = L.pf_call_peek(h, lane, bub.ctypes.data, res.ctypes.data, sv_off.ctypes.data, nb, text.ctypes.data, sites.ctypes.data,
                        groups.ctypes.data, ilen.ctypes.data, sv.ctypes.data, cap, used)
    if st != PF_OK:
        raise DeviceError(st, L.pf_last_error(h).decode())
    tb = text.tobytes()
    out = []
    for j in range(nb):
        b, r = bub[j], res[j]
        d = dict(entrance_ov=int(b["entrance_ov"]), exit_ov=int(b["exit_ov"]), strict=bool(b["strict"]),
                 inner=[int(x) for x in b["inner"][: int(b["n_inner"])]], cov=[float(x) for x in b["cov"][: int(b["n_inner"])]],
                 core_mean=float(b["core_mean"]), cov_sum=float(b["cov_sum"]), rows=None)
        R, Lc = int(r["n_rows"]), int(r["n_cols"])
        if R:
            o = int(r["rows_off"])
            d["rows"] = [tb[o + i * Lc: o + (i + 1) * Lc] for i in range(R)]
            d["sites"] = []
            d["site_cov"] = []
            v = int(sv_off[j])
            for i in range(int(r["n_sites"])):
                srec = sites[int(r["site_off"]) + i]
                g0 = int(r["group_off"]) + i * R
                mx = int(srec["maxnum"])
                d["sites"].append((int(srec["col"]), int(srec["is_indel"]), mx, groups[g0: g0 + R].tolist(), int(srec["pad"])))
                if not d["strict"]:
                    d["site_cov"].append((sv[v: v + mx].tolist(), float(sv[v + mx])))
                    v += mx + 1
            d["indel_len"] = ilen[int(r["ilen_off"]): int(r["ilen_off"]) + int(r["n_indel_len"])].tolist()
        out.append(d)
    return out


def pack_unitigs(seqs: list[bytes]):
    """2-bit pack (layout of pf_upload_graph): returns (words u64, off u64[N+1], len u32[N])."""
    n = len(seqs)
    lens = np.fromiter((len(s) for s in seqs), dtype=np.uint32, count=n)
    nwords = (lens.astype(np.uint64) + 31) // 32
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(nwords, out=off[1:])
    total = int(off[-1])
    codes = np.zeros(total * 32, dtype=np.uint8)
    lut = np.zeros(256, dtype=np.uint8)
    for ch, v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
        lut[ch] = v
    for u, s in enumerate(seqs):
        b = int(off[u]) * 32
        codes[b : b + len(s)] = lut[np.frombuffer(s, dtype=np.uint8)]
    c = codes.reshape(total, 32).astype(np.uint64)
    shifts = (np.uint64(62) - np.arange(32, dtype=np.uint64) * np.uint64(2))
    words = (c << shifts).sum(axis=1, dtype=np.uint64) if total else np.zeros(0, dtype=np.uint64)
    return np.ascontiguousarray(words), off, lens


def _ptr(a):
    """Address of a numpy array or a torch tensor (host or device)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data
    return a.data_ptr()  # torch.Tensor


class Device:
    """One pf_ctx: graph + count table resident in the HBM of one MI355X."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        st = self.L.pf_create(device, C.byref(h))
        if st != PF_OK:
            raise DeviceError(st, self.L.pf_last_error(None).decode())
        self.h = h
        self.n = 0
        self.k = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.pf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int, allow=()):
        if st != PF_OK and st not in allow:
            raise DeviceError(st, self.L.pf_last_error(self.h).decode())
        return st

    @property
    def name(self) -> str:
        buf = C.create_string_buffer(256)
        self._check(self.L.pf_device_name(self.h, buf, 256))
        return buf.value.decode()

    def set_stream(self, stream_ptr: int | None):
        self._check(self.L.pf_set_stream(self.h, stream_ptr))

    def synchronize(self):
        self._check(self.L.pf_synchronize(self.h))

    def enable_timing(self, on=True):
        self._check(self.L.pf_enable_timing(self.h, int(on)))

    def reset_timing(self):
        self._check(self.L.pf_reset_timing(self.h))

    def timing_select(self, kernels=None):
        """pf_timing_select: time the launches of these kernels only (names of KERNELS; None = all)"""
        mask = (1 << 64) - 1 if kernels is None else sum(1 << KERNELS.index(k) for k in kernels)
        self._check(self.L.pf_timing_select(self.h, mask))

    def kernel_times(self) -> dict:
        out = {}
        for i, name in enumerate(KERNELS):
            ms, n = C.c_double(), C.c_uint64()
            self._check(self.L.pf_kernel_time(self.h, i, C.byref(ms), C.byref(n)))
            if n.value:
                out[name] = (ms.value, n.value)
        return out

    def format_doubles(self, values: np.ndarray) -> list[bytes]:
        """printf("%g") of every value, formatted on the device (the result rows' number formatting, pf_format_doubles)"""
        v = np.ascontiguousarray(values, dtype=np.float64)
        text = np.zeros((len(v), 32), dtype=np.uint8)
        ln = np.zeros(len(v), dtype=np.uint8)
        self._check(self.L.pf_format_doubles(self.h, _ptr(v), len(v), _ptr(text), _ptr(ln)))
        return [text[i, :ln[i]].tobytes() for i in range(len(v))]

    # ---- uploads
    def upload_graph(self, words, off, lens, k: int):
        self.n = int(len(lens))
        self.k = k
        self._keep = (words, off, lens)
        self._check(self.L.pf_upload_graph(self.h, _ptr(words), _ptr(off), _ptr(lens), self.n, k))

    def build_adjacency(self, want_host=True):
        if want_host:
            succ = np.empty((self.n * 2, 4), dtype=np.uint32)
            pred = np.empty((self.n * 2, 4), dtype=np.uint32)
            self._check(self.L.pf_build_adjacency(self.h, succ.ctypes.data, pred.ctypes.data))
            return succ, pred
        self._check(self.L.pf_build_adjacency(self.h, None, None))
        return None

    def upload_counts(self, kmers, counts, min_count=1, max_count=0xFFFFFFFF, both_strands=True, k=None):
        """k: the database's k-mer length (default: the uploaded graph's) -- the table is addressed by minimizers of its keys"""
        self.both_strands = bool(both_strands)
        n = int(kmers.shape[0])
        k = int(k if k is not None else getattr(self, "k", 0))
        if not k:
            raise ValueError("upload_counts before upload_graph needs k")
        self._check(self.L.pf_upload_counts(self.h, _ptr(kmers), _ptr(counts), n, k, min_count, max_count, int(both_strands)))

    def join_counts(self):
        """pf_join_counts: K-COV-JOIN once more (every graph k-mer looked up in the count table)"""
        self._check(self.L.pf_join_counts(self.h))

    def minimizer_crowding(self, g: int, limit: int = 15, want_table: bool = False):
        """K-MINZ: (max occurrences of a minimizer slot, slots that reached `limit`[, the u32 counter table])."""
        mx, crowded = C.c_uint32(), C.c_uint64()
        table = np.zeros(self.L.pf_minimizer_table_slots(self.L.pf_num_kmers(self.h)), dtype=np.uint32) if want_table else None
        self._check(self.L.pf_minimizer_crowding(self.h, g, limit, C.byref(mx), C.byref(crowded), _ptr(table) if want_table else None))
        return (mx.value, crowded.value, table) if want_table else (mx.value, crowded.value)

    def minimizer_replay_inputs(self, g: int, limit: int = 15):
        """K-MINZ's hand-off to the host replay (pf_minimizer_replay_inputs): (the census as saturating u8 counters, one u8 flag
        per unitig in upload order: 1 when a counted position of it lies in a slot that reached `limit`)."""
        counters8 = np.zeros(self.L.pf_minimizer_table_slots(self.L.pf_num_kmers(self.h)), dtype=np.uint8)
        flags = np.zeros(max(1, self.n), dtype=np.uint8)
        self._check(self.L.pf_minimizer_replay_inputs(self.h, g, limit, _ptr(counters8), _ptr(flags)))
        return counters8, flags[: self.n]

    def kmc_decode(self, records: np.ndarray, n: int, suffix_bytes: int, counter_bytes: int, lut: np.ndarray, p: int, k: int):
        """K-KMC on raw .kmc_suf records (pf_kmc_decode): returns (kmers u64, counts u32) copied back to the host."""
        records = np.ascontiguousarray(records, dtype=np.uint8)
        lut = np.ascontiguousarray(lut, dtype=np.uint64)
        dk, dc = C.c_void_p(), C.c_void_p()
        self._check(self.L.pf_kmc_decode(self.h, _ptr(records), n, suffix_bytes, counter_bytes, _ptr(lut), len(lut) - 1, p, k,
                                         C.byref(dk), C.byref(dc)))
        km, ct = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        try:
            if n:
                self._check(self.L.pf_copy_to_host(self.h, _ptr(km), dk, n * 8))
                self._check(self.L.pf_copy_to_host(self.h, _ptr(ct), dc, n * 4))
        finally:
            self.L.pf_device_free(self.h, dk)
            self.L.pf_device_free(self.h, dc)
        return km, ct

    def count_histogram(self, counts, lo: int, hi: int, n_bins: int, out=None):
        """K-HIST (pf_count_histogram): hist[min(c, n_bins - 1)] += 1 for every counter c with lo <= c <= hi.  counts: u32, a numpy
        array or a device tensor; out: a device tensor of n_bins int64 to fill instead of a new numpy array."""
        if isinstance(counts, np.ndarray):
            counts = np.ascontiguousarray(counts, dtype=np.uint32)
        n = int(counts.shape[0])
        hist = np.zeros(max(int(n_bins), 0), dtype=np.uint64) if out is None else out
        buf = hist if len(hist) else np.zeros(1, dtype=np.uint64)
        self._check(self.L.pf_count_histogram(self.h, _ptr(counts) if n else None, n, lo, hi, n_bins, _ptr(buf)))
        return hist

    def hetpairs(self, kmers, counts, k: int, lo: int, hi: int, want_pairs: bool = True, want_table: bool = True):
        """K-HETPAIR (pf_hetpairs; the rule is csrc/pf_hetpair_rule.hpp): the pairs (x, y), x < y, of distinct canonical k-mers one
        substitution apart, both with a counter in [lo, hi] and neither with another such neighbour, against the resident count table
        (upload_counts of the same arrays, the same k, both strands).  kmers u64 / counts u32: numpy arrays or device tensors.  Returns
        a dict: table (W x W uint64, W = hi - lo + 1, table[a - lo, b - lo] = pairs with the counters a <= b; None unless want_table),
        pair_x, pair_y, cov_x, cov_y (in the order of x in kmers; None unless want_pairs), stats."""
        if isinstance(kmers, np.ndarray):
            kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        if isinstance(counts, np.ndarray):
            counts = np.ascontiguousarray(counts, dtype=np.uint32)
        n = int(kmers.shape[0])
        W = int(hi) - int(lo) + 1
        table = np.zeros((W, W), dtype=np.uint64) if want_table and 1 <= W <= HETPAIR_MAX_W else None
        dummy = np.zeros(1, dtype=np.uint64)   # a refused call never writes it
        px, py, cx, cy, n_pairs = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        stats = np.zeros(1, dtype=HETPAIR_STATS)
        refs = [C.byref(p) if want_pairs else None for p in (px, py, cx, cy)]
        try:
            self._check(self.L.pf_hetpairs(self.h, _ptr(kmers) if n else None, _ptr(counts) if n else None, n, int(k), int(lo), int(hi),
                                           _ptr(table) if table is not None else (_ptr(dummy) if want_table else None), *refs, C.byref(n_pairs),
                                           stats.ctypes.data))
            out = {"table": table, "pair_x": None, "pair_y": None, "cov_x": None, "cov_y": None,
                   "stats": {f: int(stats[0][f]) for f in HETPAIR_STATS.names}}
            if want_pairs:
                m = n_pairs.value
                for name, p, dt in (("pair_x", px, np.uint64), ("pair_y", py, np.uint64), ("cov_x", cx, np.uint32), ("cov_y", cy, np.uint32)):
                    out[name] = np.zeros(m, dtype=dt)
                    if m:
                        self._check(self.L.pf_copy_to_host(self.h, _ptr(out[name]), p, m * out[name].itemsize))
            return out
        finally:
            for p in (px, py, cx, cy):
                if p.value:
                    self.L.pf_device_free(self.h, p)

    def hetpair_table(self, cov_x, cov_y, lo: int, hi: int):
        """The table kernel of K-HETPAIR alone (pf_hetpair_table) over compacted counters in device tensors (int32 / uint32): the
        W x W uint64 table; pairs with a counter outside [lo, hi] add nothing."""
        n = int(cov_x.shape[0])
        W = int(hi) - int(lo) + 1
        table = np.zeros((max(W, 1), max(W, 1)), dtype=np.uint64)
        self._check(self.L.pf_hetpair_table(self.h, _ptr(cov_x) if n else None, _ptr(cov_y) if n else None, n, int(lo), int(hi), _ptr(table)))
        return table

    def kernel_time(self, kernel: int):
        """(ms, launches) of one kernel of the enum by number (K_DENSITY, K_HIST, K_MASK: not in KERNELS)"""
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.L.pf_kernel_time(self.h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_units(self, kernel: int) -> int:
        """work items handed to the timed launches of one kernel of the enum by number (pf_kernel_units)"""
        n = C.c_uint64()
        self._check(self.L.pf_kernel_units(self.h, kernel, C.byref(n)))
        return n.value

    def mask_reads(self, text, read_off, read_len, low: int, up: int = MASK_NO_UPPER, out=None):
        """K-MASK (pf_mask_reads): text with every base of every k-mer whose count lies outside [low, up] replaced by N, for the reads
        text[read_off[i] : read_off[i] + read_len[i]].  text: bytes, a uint8 numpy array or a device tensor; read_off / read_len: numpy
        arrays or device tensors (u64 / u32); out: a device tensor to fill instead of a new numpy array.  Returns (out, stats dict)."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        if isinstance(read_off, (list, tuple, np.ndarray)):
            read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        if isinstance(read_len, (list, tuple, np.ndarray)):
            read_len = np.ascontiguousarray(read_len, dtype=np.uint32)
        n, n_reads = int(text.shape[0]), int(read_off.shape[0])
        if out is None:
            out = np.zeros(n, dtype=np.uint8)
        stats = np.zeros(1, dtype=MASK_STATS)
        self._check(self.L.pf_mask_reads(self.h, _ptr(text) if n else None, n, _ptr(read_off) if n_reads else None,
                                         _ptr(read_len) if n_reads else None, n_reads, low, up, _ptr(out) if n else None, stats.ctypes.data))
        return out, {f: int(stats[0][f]) for f in MASK_STATS.names}

    def mask_fastq(self, text, low: int, up: int = MASK_NO_UPPER, final: bool = True, out=None):
        """K-MASK on one chunk of a FASTQ file (pf_mask_fastq): (out[:bytes_used], bytes_used, stats dict).  A format error raises
        DeviceError with .bad_record = the 0-based record within the chunk."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        if out is None:
            out = np.zeros(n, dtype=np.uint8)
        stats = np.zeros(1, dtype=MASK_STATS)
        used, bad = C.c_uint64(), C.c_uint64()
        st = self.L.pf_mask_fastq(self.h, _ptr(text) if n else None, n, int(final), low, up, _ptr(out) if n else None, C.byref(used),
                                  stats.ctypes.data, C.byref(bad))
        if st != PF_OK:
            e = DeviceError(st, self.L.pf_last_error(self.h).decode())
            e.bad_record = bad.value
            raise e
        return out[: used.value], used.value, {f: int(stats[0][f]) for f in MASK_STATS.names}

    def trim_fastq(self, text, steps, phred: int = 33, final: bool = True, out=None):
        """K-TRIM on one chunk of a FASTQ file (pf_trim_fastq): dict with out (the kept records, trimmed), bytes_used, n_records, begin /
        len (u32 per record, len 0 = dropped) and stats.  steps: trim_steps() of Trimmomatic's words, or a TRIM_STEP array.  text: bytes,
        a uint8 numpy array or a device tensor; out: a device tensor of len(text) + 1 bytes to fill instead of a new numpy array.  A format
        error raises DeviceError with .bad_record = the 0-based record within the chunk."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        steps = trim_steps(steps)
        n = int(text.shape[0])
        if out is None:
            out = np.zeros(n + 1, dtype=np.uint8)
        cap = n // 4 + 1
        begin, ln = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        stats = np.zeros(1, dtype=TRIM_STATS)
        out_n, used, recs, bad = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        st = self.L.pf_trim_fastq(self.h, _ptr(text) if n else None, n, int(final), steps.ctypes.data if len(steps) else None, len(steps), phred,
                                  _ptr(out), C.byref(out_n), C.byref(used), begin.ctypes.data, ln.ctypes.data, C.byref(recs), stats.ctypes.data,
                                  C.byref(bad))
        if st != PF_OK:
            e = DeviceError(st, self.L.pf_last_error(self.h).decode())
            e.bad_record = bad.value
            raise e
        return dict(out=out[: out_n.value], bytes_used=used.value, n_records=recs.value, begin=begin[: recs.value], len=ln[: recs.value],
                    stats={f: int(stats[0][f]) for f in TRIM_STATS.names})

    def clip_begin(self, adapters, seed: int = 2, score: int = 10):
        """K-CLIP (pf_clip_begin): opens a clip on the context -- until clip_end() trim_fastq, trim_fastq_pair, trim_table_fastq[_pair] and
        the *_trimmed count calls clip adapter read-through first and take an empty list of steps.  adapters: a list of (sequence,
        side) pairs (side 0: both files, 1, 2), or the dict of hostapi.clip_parse_adapters.  Refusals raise DeviceError by name."""
        if isinstance(adapters, dict):
            bases, off, side = adapters["bases"], adapters["off"], adapters["side"]
        else:
            seqs = [s.encode() if isinstance(s, str) else bytes(s) for s, _ in adapters]
            bases = b"".join(seqs)
            off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]) if seqs else np.zeros(1)
            side = [sd for _, sd in adapters]
        bases = np.frombuffer(bytes(bases), dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        side = np.ascontiguousarray(side, dtype=np.uint8)
        self._check(self.L.pf_clip_begin(self.h, bases.ctypes.data if len(bases) else None, off.ctypes.data, side.ctypes.data if len(side) else None,
                                         len(side), int(seed), int(score)))

    def clip_begin_pairs(self, adapters, prefix_pairs, seed: int = 2, score: int = 10, pair_score: int = 30, pair_min: int = 8, keep_both: bool = False):
        """K-PALIN (pf_clip_begin_pairs): a clip with prefix pairs -- the paired calls also clip by palindrome mode.  adapters: as
        clip_begin takes them, may be empty; prefix_pairs: a list of (P1, P2), or the dict of hostapi.clip_parse_adapters(pairs=True)
        (then `adapters` may be that dict as well).  Refusals raise DeviceError by name."""
        if isinstance(adapters, dict):
            bases, off, side = adapters["bases"], adapters["off"], adapters["side"]
        else:
            seqs = [s.encode() if isinstance(s, str) else bytes(s) for s, _ in adapters]
            bases = b"".join(seqs)
            off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]) if seqs else np.zeros(1)
            side = [sd for _, sd in adapters]
        if isinstance(prefix_pairs, dict):
            pbases, poff = prefix_pairs["prefix_bases"], prefix_pairs["prefix_off"]
        else:
            halves = [h.encode() if isinstance(h, str) else bytes(h) for pr in prefix_pairs for h in pr]
            pbases = b"".join(halves)
            poff = np.concatenate([[0], np.cumsum([len(h) for h in halves])]) if halves else np.zeros(1)
        bases = np.frombuffer(bytes(bases), dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        side = np.ascontiguousarray(side, dtype=np.uint8)
        pbases = np.frombuffer(bytes(pbases), dtype=np.uint8)
        poff = np.ascontiguousarray(poff, dtype=np.uint32)
        self._check(self.L.pf_clip_begin_pairs(self.h, bases.ctypes.data if len(bases) else None, off.ctypes.data, side.ctypes.data if len(side) else None,
                                               len(side), pbases.ctypes.data if len(pbases) else None, poff.ctypes.data, (len(poff) - 1) // 2, int(seed),
                                               int(score), int(pair_score), int(pair_min), int(bool(keep_both))))

    def clip_pair_stats(self) -> dict:
        """pf_clip_pair_stats_get: what K-PALIN has counted since clip_begin_pairs; bases_clipped is [file 1, file 2]"""
        st = np.zeros(1, dtype=CLIP_PAIR_STATS)
        self._check(self.L.pf_clip_pair_stats_get(self.h, st.ctypes.data))
        return {f: ([int(v) for v in st[0][f]] if f == "bases_clipped" else int(st[0][f])) for f in CLIP_PAIR_STATS.names}

    def clip_stats(self) -> dict:
        """pf_clip_stats_get: what the open clip has counted since clip_begin, each field [file 1 and single-ended calls, file 2]"""
        st = np.zeros(1, dtype=CLIP_STATS)
        self._check(self.L.pf_clip_stats_get(self.h, st.ctypes.data))
        return {f: [int(v) for v in st[0][f]] for f in CLIP_STATS.names}

    def clip_last_ends(self, n_records: int, file: int = 0) -> np.ndarray:
        """pf_clip_last_ends: the clip ends (u32; n untouched, 0 dropped) of the first n_records records of file 0 or 1 of the last call"""
        out = np.zeros(n_records, dtype=np.uint32)
        self._check(self.L.pf_clip_last_ends(self.h, file, out.ctypes.data if n_records else None, n_records))
        return out

    def clip_end(self):
        """pf_clip_end: closes the clip; the trim calls are what they were without one"""
        self._check(self.L.pf_clip_end(self.h))

    def qc_begin(self, phred: int = 33):
        """K-QC (pf_qc_begin): opens a read quality report on the context -- until qc_end() trim_fastq, trim_fastq_pair,
        trim_table_fastq[_pair] and the *_trimmed count calls add every record they take to the report's tables (stage raw, and the kept
        ones with their final interval to stage kept), and qc_fastq adds a chunk to stage raw alone.  Refusals raise DeviceError by name."""
        self._check(self.L.pf_qc_begin(self.h, int(phred)))

    def qc_tables(self) -> np.ndarray:
        """pf_qc_get for both sides and both stages: a u64 array [side][stage][QC_TABLE_WORDS] (the words: csrc/pf_qc_rule.hpp)"""
        t = np.zeros((2, 2, QC_TABLE_WORDS), dtype=np.uint64)
        for side in range(2):
            for stage in range(2):
                self._check(self.L.pf_qc_get(self.h, side, stage, t[side, stage].ctypes.data))
        return t

    def qc_clip_table(self) -> np.ndarray:
        """pf_qc_clip_get for both sides: a u64 array [side][QC_CLIP_WORDS], the clip ends below the read length"""
        t = np.zeros((2, QC_CLIP_WORDS), dtype=np.uint64)
        for side in range(2):
            self._check(self.L.pf_qc_clip_get(self.h, side, t[side].ctypes.data))
        return t

    def qc_fastq(self, text, side: int = 0, final: bool = True):
        """K-QC on one chunk of a FASTQ file (pf_qc_fastq): its whole records into stage raw of `side` (0 or 1); returns (bytes_used,
        n_records).  text: bytes, a uint8 numpy array or a device tensor.  A format error raises DeviceError with .bad_record."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        used, recs, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
        st = self.L.pf_qc_fastq(self.h, int(side), _ptr(text) if n else None, n, int(final), C.byref(used), C.byref(recs), C.byref(bad))
        if st != PF_OK:
            e = DeviceError(st, self.L.pf_last_error(self.h).decode())
            e.bad_record = bad.value
            raise e
        return used.value, recs.value

    def qc_end(self):
        """pf_qc_end: closes the report; the trim calls launch nothing more"""
        self._check(self.L.pf_qc_end(self.h))

    def dedup_begin(self, bases: int = 0, initial_slots: int = 0):
        """K-DEDUP (pf_dedup_begin): opens a dedup on the context -- until dedup_end() trim_fastq, trim_fastq_pair,
        trim_table_fastq[_pair] and the *_trimmed count calls drop every kept unit whose key (the first `bases` bases of its raw
        read(s), 0 = all; csrc/pf_dedup_rule.hpp) an earlier unit of the stream had, and take an empty list of steps.  initial_slots:
        0 = default, rounded up to a power of two, at least 64.  Refusals raise DeviceError by name."""
        self._check(self.L.pf_dedup_begin(self.h, int(bases), int(initial_slots)))

    def dedup_stats(self) -> dict:
        """pf_dedup_stats_get: units, unique, duplicates, max_copies, levels (a list of 10), slots, growths of the open dedup"""
        st = np.zeros(1, dtype=DEDUP_STATS)
        self._check(self.L.pf_dedup_stats_get(self.h, st.ctypes.data))
        return {f: ([int(v) for v in st[0][f]] if f == "levels" else int(st[0][f])) for f in DEDUP_STATS.names}

    def dedup_keys(self, keys, keep=None):
        """pf_dedup_keys: the table by itself -- keys ([n, 2] u64: a numpy array or a device tensor) as the next n units, all taking
        part; returns keep (u8 per key: 1 = not seen before), a numpy array, or the device tensor `keep` filled."""
        if isinstance(keys, np.ndarray):
            keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = int(keys.shape[0])
        if keep is None:
            keep = np.zeros(n, dtype=np.uint8)
        self._check(self.L.pf_dedup_keys(self.h, _ptr(keys) if n else None, n, _ptr(keep) if n else None))
        return keep

    def dedup_end(self):
        """pf_dedup_end: closes the dedup and frees its table; the trim calls are what they were without one"""
        self._check(self.L.pf_dedup_end(self.h))

    def inflate_bgzf(self, comp, member_off, out=None, out_cap=None):
        """K-INFLATE (pf_inflate_bgzf): the BGZF members comp[member_off[m] : member_off[m + 1]] inflated one behind the other; returns
        (text, stats).  comp: bytes, a uint8 numpy array or a device tensor; member_off: n_members + 1 offsets (list, u64 array or device
        tensor); out: an array or device tensor to fill (out_cap bytes of it, default all) instead of a new numpy array of the size
        needed.  A refused member raises DeviceError with .bad_member = the smallest offender; a buffer too small raises it with
        status PF_ERR_OVERFLOW and .needed."""
        if isinstance(comp, (bytes, bytearray)):
            comp = np.frombuffer(bytes(comp), dtype=np.uint8)
        if isinstance(member_off, (list, tuple, np.ndarray)):
            member_off = np.ascontiguousarray(member_off, dtype=np.uint64)
        n, n_members = int(comp.shape[0]), max(int(member_off.shape[0]) - 1, 0)
        stats = np.zeros(1, dtype=INFLATE_STATS)
        out_n, bad = C.c_uint64(), C.c_uint64()
        call = lambda o, cap: self.L.pf_inflate_bgzf(self.h, _ptr(comp) if n else None, n, _ptr(member_off) if n_members else None, n_members,   # noqa: E731
                                                     _ptr(o) if o is not None and cap else None, cap, C.byref(out_n), stats.ctypes.data, C.byref(bad))
        if out is None:   # sized by a first call that writes nothing
            st = call(None, 0)
            if st == PF_ERR_OVERFLOW:
                out = np.zeros(out_n.value, dtype=np.uint8)
                st = call(out, out_n.value)
            else:
                out = np.zeros(0, dtype=np.uint8)
        else:
            st = call(out, int(out.shape[0]) if out_cap is None else out_cap)
        if st != PF_OK:
            e = DeviceError(st, self.L.pf_last_error(self.h).decode())
            e.bad_member = bad.value
            e.needed = out_n.value
            raise e
        return out[: out_n.value], {f: int(stats[0][f]) for f in INFLATE_STATS.names}

    def deflate_bgzf(self, text, member_text: int = 65280, out=None, out_cap=None, member_off=None):
        """K-DEFLATE (pf_deflate_bgzf): text cut into BGZF members of member_text bytes; returns (bytes, member_off, stats): the members one
        behind the other (a uint8 array, or the part of `out` they fill), their n_members + 1 offsets and the counters of
        pf_deflate_stats.  text: bytes, a uint8 numpy array or a device tensor; out: an array or device tensor to fill (out_cap bytes of
        it, default all) instead of a new numpy array of the bound's len(text) + 31 a member; member_off: a device tensor for the offsets
        instead of a new numpy array.  A buffer below the bound raises DeviceError with status PF_ERR_OVERFLOW."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        n_members = (n + member_text - 1) // member_text if member_text > 0 else 0
        if out is None:
            out = np.zeros(n + 31 * n_members, dtype=np.uint8)
        if member_off is None:
            member_off = np.zeros(n_members + 1, dtype=np.uint64)
        stats = np.zeros(1, dtype=DEFLATE_STATS)
        out_n = C.c_uint64()
        st = self.L.pf_deflate_bgzf(self.h, _ptr(text) if n else None, n, member_text, _ptr(out) if int(out.shape[0]) else None,
                                    int(out.shape[0]) if out_cap is None else out_cap, C.byref(out_n), _ptr(member_off), stats.ctypes.data)
        if st != PF_OK:
            raise DeviceError(st, self.L.pf_last_error(self.h).decode())
        return out[: out_n.value], member_off, {f: int(stats[0][f]) for f in DEFLATE_STATS.names}

    def inflate_gzip(self, comp, start_bit: int = 0, window=None, piece_bytes: int = 0, out=None, out_cap=None, new_window=None):
        """K-GUNZIP (pf_inflate_gzip): the deflate stream comp[0:] of a plain gzip member from start_bit (a block start) on, up to a final
        block or the last complete block boundary; returns (text, result, stats, new_window).  comp, window, out, new_window: bytes, uint8
        numpy arrays or device tensors; window: the last <= 32768 bytes of the member's text so far; result: the fields of
        pf_gunzip_result (end_bit, final, n_window, crc_raw, ...); stats: the counters and stage_ms by name.  A refused stream raises
        DeviceError with .clause and .clause_bit; a buffer too small raises it with status PF_ERR_OVERFLOW and .needed."""
        as_arr = lambda b: np.frombuffer(bytes(b), dtype=np.uint8) if isinstance(b, (bytes, bytearray)) else b   # noqa: E731
        comp, window = as_arr(comp), as_arr(window) if window is not None else None
        n, n_window = int(comp.shape[0]), int(window.shape[0]) if window is not None else 0
        if new_window is None:
            new_window = np.zeros(32768, dtype=np.uint8)
        res, stats = np.zeros(1, dtype=GUNZIP_RESULT), np.zeros(1, dtype=GUNZIP_STATS)
        call = lambda o, cap: self.L.pf_inflate_gzip(self.h, _ptr(comp) if n else None, n, start_bit, _ptr(window) if n_window else None, n_window,   # noqa: E731
                                                     piece_bytes, _ptr(o) if o is not None and cap else None, cap, _ptr(new_window), res.ctypes.data,
                                                     stats.ctypes.data)
        if out is None:   # sized by a first call that writes nothing
            st = call(None, 0)
            if st == PF_ERR_OVERFLOW:
                out = np.zeros(int(res[0]["out_bytes"]), dtype=np.uint8)
                st = call(out, int(out.shape[0]))
            else:
                out = np.zeros(0, dtype=np.uint8)
        else:
            st = call(out, int(out.shape[0]) if out_cap is None else out_cap)
        r = {f: int(res[0][f]) for f in GUNZIP_RESULT.names}
        if st != PF_OK:
            e = DeviceError(st, self.L.pf_last_error(self.h).decode())
            e.clause, e.clause_bit, e.needed = r["clause"], r["clause_bit"], r["out_bytes"]
            raise e
        sd = {f: int(stats[0][f]) for f in GUNZIP_COUNTERS}
        sd["stage_ms"] = dict(zip(GUNZIP_STAGES, (float(x) for x in stats[0]["stage_ms"])))
        return out[: r["out_bytes"]], r, sd, new_window[: r["n_window"]]

    def trim_fastq_pair(self, text1, text2, steps, phred: int = 33, final: bool = True, outs=None):
        """K-TRIM on one chunk of each file of a pair (pf_trim_fastq_pair): dict with out = [o1, u1, o2, u2], bytes_used = [file 1,
        file 2], n_records, begin / len = [file 1, file 2], stats = [file 1, file 2].  outs: four arrays or device tensors to fill (o1,
        u1: len(text1) + 1 bytes; o2, u2: len(text2) + 1).  bad_record of a DeviceError: 2 * record + file."""
        texts = [np.frombuffer(bytes(t), dtype=np.uint8) if isinstance(t, (bytes, bytearray)) else t for t in (text1, text2)]
        steps = trim_steps(steps)
        n = [int(t.shape[0]) for t in texts]
        if outs is None:
            outs = [np.zeros(n[d // 2] + 1, dtype=np.uint8) for d in range(4)]
        cap = min(n) // 4 + 1
        begin = [np.zeros(cap, dtype=np.uint32) for _ in range(2)]
        ln = [np.zeros(cap, dtype=np.uint32) for _ in range(2)]
        stats = np.zeros(2, dtype=TRIM_STATS)
        out_p = (C.c_void_p * 4)(*[_ptr(o) for o in outs])
        begin_p = (C.c_void_p * 2)(*[b.ctypes.data for b in begin])
        len_p = (C.c_void_p * 2)(*[x.ctypes.data for x in ln])
        out_n, used, recs, bad = (C.c_uint64 * 4)(), (C.c_uint64 * 2)(), C.c_uint64(), C.c_uint64()
        st = self.L.pf_trim_fastq_pair(self.h, _ptr(texts[0]) if n[0] else None, n[0], _ptr(texts[1]) if n[1] else None, n[1], int(final),
                                       steps.ctypes.data if len(steps) else None, len(steps), phred, out_p, out_n, used, begin_p, len_p,
                                       C.byref(recs), stats.ctypes.data, C.byref(bad))
        if st != PF_OK:
            e = DeviceError(st, self.L.pf_last_error(self.h).decode())
            e.bad_record = bad.value
            raise e
        r = recs.value
        return dict(out=[outs[d][: out_n[d]] for d in range(4)], bytes_used=[used[0], used[1]], n_records=r, begin=[b[:r] for b in begin],
                    len=[x[:r] for x in ln], stats=[{f: int(stats[j][f]) for f in TRIM_STATS.names} for j in range(2)])

    def count_begin(self, k: int, both_strands: bool = True, initial_slots: int = 0):
        """K-COUNT (pf_count_begin): opens a count of k-mers of length k (3 .. 31); both_strands: canonical keys.  initial_slots = 0:
        twice the first call's bytes."""
        self._check(self.L.pf_count_begin(self.h, k, int(both_strands), initial_slots))

    def count_reads(self, text, read_off, read_len):
        """pf_count_reads: counts the reads text[read_off[i] : read_off[i] + read_len[i]] (arguments as mask_reads takes them); returns
        this call's statistics."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        if isinstance(read_off, (list, tuple, np.ndarray)):
            read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        if isinstance(read_len, (list, tuple, np.ndarray)):
            read_len = np.ascontiguousarray(read_len, dtype=np.uint32)
        n, n_reads = int(text.shape[0]), int(read_off.shape[0])
        stats = np.zeros(1, dtype=COUNT_STATS)
        self._check(self.L.pf_count_reads(self.h, _ptr(text) if n else None, n, _ptr(read_off) if n_reads else None,
                                          _ptr(read_len) if n_reads else None, n_reads, stats.ctypes.data))
        return {f: int(stats[0][f]) for f in COUNT_STATS.names}

    def count_fastq(self, text, final: bool = True):
        """pf_count_fastq on one chunk of a FASTQ file: (bytes_used, this call's statistics).  A format error raises DeviceError with
        .bad_record = the 0-based record within the chunk."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        stats = np.zeros(1, dtype=COUNT_STATS)
        used, bad = C.c_uint64(), C.c_uint64()
        st = self.L.pf_count_fastq(self.h, _ptr(text) if n else None, n, int(final), C.byref(used), stats.ctypes.data, C.byref(bad))
        if st != PF_OK:
            e = DeviceError(st, self.L.pf_last_error(self.h).decode())
            e.bad_record = bad.value
            raise e
        return used.value, {f: int(stats[0][f]) for f in COUNT_STATS.names}

    def count_finish(self, ci: int = 2, cx: int = 10 ** 9, cs: int = 255):
        """pf_count_finish: (kmers u64 sorted, counts u32 = min(c, cs), statistics of the whole count) copied back to the host."""
        dk, dc, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        stats = np.zeros(1, dtype=COUNT_STATS)
        self._check(self.L.pf_count_finish(self.h, ci, cx, cs, C.byref(dk), C.byref(dc), C.byref(n), stats.ctypes.data))
        km, ct = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint32)
        try:
            if n.value:
                self._check(self.L.pf_copy_to_host(self.h, _ptr(km), dk, n.value * 8))
                self._check(self.L.pf_copy_to_host(self.h, _ptr(ct), dc, n.value * 4))
        finally:
            self.L.pf_device_free(self.h, dk)
            self.L.pf_device_free(self.h, dc)
        return km, ct, {f: int(stats[0][f]) for f in COUNT_STATS.names}

    def count_abort(self):
        self._check(self.L.pf_count_abort(self.h))

    def maskcount_reads(self, text, read_off, read_len, low: int, up: int = MASK_NO_UPPER):
        """K-MASKCOUNT (pf_maskcount_reads): counts into the open count every window of the reads that survives the masking with
        [low, up] against the resident table -- mask_reads followed by count_reads on its output, without that output.  Arguments as
        count_reads takes them; returns this call's statistics."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        if isinstance(read_off, (list, tuple, np.ndarray)):
            read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        if isinstance(read_len, (list, tuple, np.ndarray)):
            read_len = np.ascontiguousarray(read_len, dtype=np.uint32)
        n, n_reads = int(text.shape[0]), int(read_off.shape[0])
        stats = np.zeros(1, dtype=MASKCOUNT_STATS)
        self._check(self.L.pf_maskcount_reads(self.h, _ptr(text) if n else None, n, _ptr(read_off) if n_reads else None,
                                              _ptr(read_len) if n_reads else None, n_reads, low, up, stats.ctypes.data))
        return {f: int(stats[0][f]) for f in MASKCOUNT_STATS.names}

    def maskcount_fastq(self, text, low: int, up: int = MASK_NO_UPPER, final: bool = True):
        """pf_maskcount_fastq on one chunk of a FASTQ file: (bytes_used, this call's statistics).  A format error raises DeviceError
        with .bad_record = the 0-based record within the chunk."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        stats = np.zeros(1, dtype=MASKCOUNT_STATS)
        used, bad = C.c_uint64(), C.c_uint64()
        st = self.L.pf_maskcount_fastq(self.h, _ptr(text) if n else None, n, int(final), low, up, C.byref(used), stats.ctypes.data, C.byref(bad))
        if st != PF_OK:
            e = DeviceError(st, self.L.pf_last_error(self.h).decode())
            e.bad_record = bad.value
            raise e
        return used.value, {f: int(stats[0][f]) for f in MASKCOUNT_STATS.names}

    # ---- K-FASTA: FASTA chunks to compacted text and table, then the cores (pf_fasta_rule.hpp) ----
    def _fasta_call(self, fn, text, final, stats, head=(), tail=()):   # head: in front of the text (a colour); tail: behind `final` (low, up)
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        used, bad = C.c_uint64(), C.c_uint64()
        st = fn(self.h, *head, _ptr(text) if n else None, n, int(final), *tail, C.byref(used), stats.ctypes.data, C.byref(bad))
        if st != PF_OK:
            e = DeviceError(st, self.L.pf_last_error(self.h).decode())
            e.bad_record = bad.value
            raise e
        return used.value

    def fasta_index(self, text, final: bool = True) -> dict:
        """K-FASTA alone (pf_fasta_index_fetch) on one chunk of FASTA text: "text" = the compacted text (the sequences of the whole
        records, one directly behind the other), "read_off" / "read_len" = the table into it, "bytes_used", "records", "bases" -- what
        hostapi.fasta_index gives for the same chunk.  A chunk that does not start with '>' raises DeviceError."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        used, n_rec, n_bases = C.c_uint64(), C.c_uint64(), C.c_uint64()
        out = np.zeros(max(n, 1), dtype=np.uint8)
        off, ln = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)   # (a record holds at least its '>')
        self._check(self.L.pf_fasta_index_fetch(self.h, _ptr(text) if n else None, n, int(final), C.byref(used), C.byref(n_rec), C.byref(n_bases),
                                                out.ctypes.data, len(out), off.ctypes.data, ln.ctypes.data, len(off)))
        return {"text": out[: n_bases.value].tobytes(), "read_off": off[: n_rec.value].copy(), "read_len": ln[: n_rec.value].copy(),
                "bytes_used": used.value, "records": n_rec.value, "bases": n_bases.value}

    def fasta_index_resident(self, text, final: bool = True) -> dict:
        """K-FASTA alone, the index left on the device (pf_fasta_index): "bytes_used", "records", "bases", and the device addresses
        "text_dev", "read_off_dev", "read_len_dev" (None where empty), which belong to the context until its next K-FASTA call."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        used, n_rec, n_bases = C.c_uint64(), C.c_uint64(), C.c_uint64()
        dt, doff, dlen = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.L.pf_fasta_index(self.h, _ptr(text) if n else None, n, int(final), C.byref(used), C.byref(n_rec), C.byref(n_bases),
                                          C.byref(dt), C.byref(doff), C.byref(dlen)))
        return {"bytes_used": used.value, "records": n_rec.value, "bases": n_bases.value, "text_dev": dt.value, "read_off_dev": doff.value,
                "read_len_dev": dlen.value}

    def count_fasta(self, text, final: bool = True):
        """pf_count_fasta on one chunk of a FASTA file: (bytes_used, this call's statistics), as count_fastq gives them for Q(F)."""
        stats = np.zeros(1, dtype=COUNT_STATS)
        used = self._fasta_call(self.L.pf_count_fasta, text, final, stats)
        return used, {f: int(stats[0][f]) for f in COUNT_STATS.names}

    def maskcount_fasta(self, text, low: int, up: int = MASK_NO_UPPER, final: bool = True):
        """pf_maskcount_fasta on one chunk of a FASTA file: (bytes_used, this call's statistics), as maskcount_fastq gives them for Q(F)."""
        stats = np.zeros(1, dtype=MASKCOUNT_STATS)
        used = self._fasta_call(self.L.pf_maskcount_fasta, text, final, stats, tail=(low, up))
        return used, {f: int(stats[0][f]) for f in MASKCOUNT_STATS.names}

    def color_fasta(self, colour: int, text, final: bool = True):
        """pf_color_fasta on one chunk of a FASTA file of `colour`: (bytes_used, this call's statistics)."""
        stats = np.zeros(1, dtype=COLOR_STATS)
        used = self._fasta_call(self.L.pf_color_fasta, text, final, stats, head=(int(colour),))
        return used, {f: stats[0][f].item() for f in COLOR_STATS.names}

    # ---- K-TRIMCOUNT: K-TRIM folded into K-COUNT / K-MASKCOUNT (pf_trimrun_rule.hpp) ----
    @staticmethod
    def _trim_plan(steps, phred):
        steps = trim_steps(steps)
        return steps, TrimPlan(steps.ctypes.data if len(steps) else None, len(steps), phred)   # (the array is kept alive by the caller)

    def _raise_bad(self, st, bad):
        e = DeviceError(st, self.L.pf_last_error(self.h).decode())
        e.bad_record = bad.value
        raise e

    def trim_table_fastq(self, text, steps, phred: int = 33, final: bool = True, read_off=None, read_len=None):
        """pf_trim_table_fastq on one chunk of raw FASTQ: dict with read_off (u64) / read_len (u32) = the table of the reads handed on
        (sequence bytes [seq_begin + b, seq_begin + e) of every kept record), n_reads, bytes_used, n_records, stats (pf_trim_stats).
        read_off / read_len: device tensors to fill instead of new numpy arrays (one entry per record of the chunk)."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        steps, plan = self._trim_plan(steps, phred)
        n = int(text.shape[0])
        cap = n // 4 + 1
        off = np.zeros(cap, dtype=np.uint64) if read_off is None else read_off
        ln = np.zeros(cap, dtype=np.uint32) if read_len is None else read_len
        stats = np.zeros(1, dtype=TRIM_STATS)
        n_reads, used, recs, bad = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        st = self.L.pf_trim_table_fastq(self.h, _ptr(text) if n else None, n, int(final), C.addressof(plan), _ptr(off), _ptr(ln), C.byref(n_reads),
                                        C.byref(used), C.byref(recs), stats.ctypes.data, C.byref(bad))
        if st != PF_OK:
            self._raise_bad(st, bad)
        return dict(read_off=off[: n_reads.value], read_len=ln[: n_reads.value], n_reads=n_reads.value, bytes_used=used.value, n_records=recs.value,
                    stats={f: int(stats[0][f]) for f in TRIM_STATS.names})

    def trim_table_fastq_pair(self, text1, text2, steps, phred: int = 33, final: bool = True, read_off=None, read_len=None):
        """pf_trim_table_fastq_pair on one chunk of each file of a pair: read_off / read_len = [file 1, file 2] (a record is handed on only
        when the records of both files are kept: both tables have n_reads entries), bytes_used = [file 1, file 2], n_records,
        stats = [file 1, file 2].  bad_record of a DeviceError: 2 * record + file."""
        texts = [np.frombuffer(bytes(t), dtype=np.uint8) if isinstance(t, (bytes, bytearray)) else t for t in (text1, text2)]
        steps, plan = self._trim_plan(steps, phred)
        n = [int(t.shape[0]) for t in texts]
        cap = min(n) // 4 + 1
        off = [np.zeros(cap, dtype=np.uint64) for _ in range(2)] if read_off is None else read_off
        ln = [np.zeros(cap, dtype=np.uint32) for _ in range(2)] if read_len is None else read_len
        off_p = (C.c_void_p * 2)(*[_ptr(x) for x in off])
        len_p = (C.c_void_p * 2)(*[_ptr(x) for x in ln])
        stats = np.zeros(2, dtype=TRIM_STATS)
        n_reads, used, recs, bad = C.c_uint64(), (C.c_uint64 * 2)(), C.c_uint64(), C.c_uint64()
        st = self.L.pf_trim_table_fastq_pair(self.h, _ptr(texts[0]) if n[0] else None, n[0], _ptr(texts[1]) if n[1] else None, n[1], int(final),
                                             C.addressof(plan), off_p, len_p, C.byref(n_reads), used, C.byref(recs), stats.ctypes.data, C.byref(bad))
        if st != PF_OK:
            self._raise_bad(st, bad)
        m = n_reads.value
        return dict(read_off=[x[:m] for x in off], read_len=[x[:m] for x in ln], n_reads=m, bytes_used=[used[0], used[1]], n_records=recs.value,
                    stats=[{f: int(stats[j][f]) for f in TRIM_STATS.names} for j in range(2)])

    def _counted_trimmed(self, masked, texts, steps, phred, final, low, up):
        texts = [np.frombuffer(bytes(t), dtype=np.uint8) if isinstance(t, (bytes, bytearray)) else t for t in texts]
        steps, plan = self._trim_plan(steps, phred)
        n = [int(t.shape[0]) for t in texts]
        pair = len(texts) == 2
        dt = MASKCOUNT_STATS if masked else COUNT_STATS
        tstats, stats = np.zeros(2, dtype=TRIM_STATS), np.zeros(1, dtype=dt)
        used, bad = (C.c_uint64 * 2)(), C.c_uint64()
        args = [self.h]
        for t, m in zip(texts, n):
            args += [_ptr(t) if m else None, m]
        args += [int(final), C.addressof(plan)] + ([low, up] if masked else []) + [used, tstats.ctypes.data, stats.ctypes.data, C.byref(bad)]
        fn = getattr(self.L, "pf_%s_fastq%s_trimmed" % ("maskcount" if masked else "count", "_pair" if pair else ""))
        st = fn(*args)
        if st != PF_OK:
            self._raise_bad(st, bad)
        ts = [{f: int(tstats[j][f]) for f in TRIM_STATS.names} for j in range(2 if pair else 1)]
        return ([used[0], used[1]] if pair else used[0]), (ts if pair else ts[0]), {f: int(stats[0][f]) for f in dt.names}

    def count_fastq_trimmed(self, text, steps, phred: int = 33, final: bool = True):
        """pf_count_fastq_trimmed on one chunk of raw FASTQ: (bytes_used, trimming statistics, this call's counting statistics) -- trim_fastq
        followed by count_fastq on its output, without that output."""
        return self._counted_trimmed(False, [text], steps, phred, final, 0, 0)

    def count_fastq_pair_trimmed(self, text1, text2, steps, phred: int = 33, final: bool = True):
        """pf_count_fastq_pair_trimmed: ([bytes_used 1, 2], [trimming statistics 1, 2], counting statistics): the both-kept records of
        both files are counted (o1 and o2 of trim_fastq_pair)."""
        return self._counted_trimmed(False, [text1, text2], steps, phred, final, 0, 0)

    def maskcount_fastq_trimmed(self, text, steps, low: int, up: int = MASK_NO_UPPER, phred: int = 33, final: bool = True):
        """pf_maskcount_fastq_trimmed: (bytes_used, trimming statistics, K-MASKCOUNT's statistics) on the trimmed reads of the chunk"""
        return self._counted_trimmed(True, [text], steps, phred, final, low, up)

    def maskcount_fastq_pair_trimmed(self, text1, text2, steps, low: int, up: int = MASK_NO_UPPER, phred: int = 33, final: bool = True):
        """pf_maskcount_fastq_pair_trimmed: the pair form of maskcount_fastq_trimmed"""
        return self._counted_trimmed(True, [text1, text2], steps, phred, final, low, up)

    def unitig_text(self):
        """pf_unitig_text: (device address, bytes) of the text a held graph keeps on the device until unitig_release"""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.pf_unitig_text(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def unitig_build(self, kmers, k: int, clip_tips: bool = False, del_isolated: bool = False, g=None):
        """K-UNITIG (pf_unitig_build, pf_unitig_fetch, pf_unitig_release): (the text of the GFA file as bytes, statistics) of the
        compacted de Bruijn graph of `kmers` -- sorted distinct canonical k-mers as count_finish gives them, a numpy array or a device
        tensor.  g: the ML tag of the header, None = Bifrost's default for k."""
        if isinstance(kmers, (list, tuple, np.ndarray)):
            kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        n = int(kmers.shape[0])
        g = UNITIG_G_DEFAULT if g is None else min(max(int(g), 0), UNITIG_G_DEFAULT - 1)   # (0 is refused by name like any other g outside 1 .. k - 2)
        stats = np.zeros(1, dtype=UNITIG_STATS)
        self._check(self.L.pf_unitig_build(self.h, _ptr(kmers) if n else None, n, k, g, int(clip_tips), int(del_isolated), stats.ctypes.data))
        try:
            text = np.zeros(max(int(stats[0]["bytes"]), 1), dtype=np.uint8)
            self._check(self.L.pf_unitig_fetch(self.h, 0, int(stats[0]["bytes"]), _ptr(text)))
        finally:
            self.L.pf_unitig_release(self.h)
        out = {f: int(stats[0][f]) for f in UNITIG_STATS.names if f != "stage_ms"}
        out["stage_ms"] = dict(zip(UNITIG_STAGES, (float(x) for x in stats[0]["stage_ms"])))
        return text[: int(stats[0]["bytes"])].tobytes(), out

    def unitig_build_colored(self, kmers, k: int, clip_tips: bool = False, del_isolated: bool = False, g=None, n_seeds: int = COLOR_SEEDS):
        """pf_unitig_build_colored: unitig_build on the k-mers of all colours' reads together, every S line with its DA tag; returns (the
        text of the GFA file, statistics with "overflow").  The graph stays held for color_begin, color_reads / color_fastq and
        color_finish until unitig_release."""
        if isinstance(kmers, (list, tuple, np.ndarray)):
            kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        n = int(kmers.shape[0])
        g = UNITIG_G_DEFAULT if g is None else min(max(int(g), 0), UNITIG_G_DEFAULT - 1)
        stats = np.zeros(1, dtype=UNITIG_STATS)
        over = C.c_uint64()
        self._check(self.L.pf_unitig_build_colored(self.h, _ptr(kmers) if n else None, n, k, g, int(clip_tips), int(del_isolated), int(n_seeds),
                                                   stats.ctypes.data, C.byref(over)))
        try:
            text = np.zeros(max(int(stats[0]["bytes"]), 1), dtype=np.uint8)
            self._check(self.L.pf_unitig_fetch(self.h, 0, int(stats[0]["bytes"]), _ptr(text)))
        except Exception:
            self.L.pf_unitig_release(self.h)
            raise
        out = {f: int(stats[0][f]) for f in UNITIG_STATS.names if f != "stage_ms"}
        out["stage_ms"] = dict(zip(UNITIG_STAGES, (float(x) for x in stats[0]["stage_ms"])))
        out["overflow"] = over.value
        return text[: int(stats[0]["bytes"])].tobytes(), out

    def unitig_release(self):
        self._check(self.L.pf_unitig_release(self.h))

    def color_begin(self, n_colors: int):
        """K-COLOR (pf_color_begin): the look-up table over the k-mers of the held coloured graph and one cleared bit plane a colour"""
        self._check(self.L.pf_color_begin(self.h, int(n_colors)))

    def color_reads(self, colour: int, text, read_off, read_len):
        """pf_color_reads: colours the k-mers of the reads text[read_off[i] : read_off[i] + read_len[i]] (arguments as count_reads takes
        them) with `colour`; returns this call's statistics."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        if isinstance(read_off, (list, tuple, np.ndarray)):
            read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        if isinstance(read_len, (list, tuple, np.ndarray)):
            read_len = np.ascontiguousarray(read_len, dtype=np.uint32)
        n, n_reads = int(text.shape[0]), int(read_off.shape[0])
        stats = np.zeros(1, dtype=COLOR_STATS)
        self._check(self.L.pf_color_reads(self.h, int(colour), _ptr(text) if n else None, n, _ptr(read_off) if n_reads else None,
                                          _ptr(read_len) if n_reads else None, n_reads, stats.ctypes.data))
        return {f: stats[0][f].item() for f in COLOR_STATS.names}

    def color_fastq(self, colour: int, text, final: bool = True):
        """pf_color_fastq on one chunk of a FASTQ file of `colour`: (bytes_used, this call's statistics).  A format error raises
        DeviceError with .bad_record = the 0-based record within the chunk."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        stats = np.zeros(1, dtype=COLOR_STATS)
        used, bad = C.c_uint64(), C.c_uint64()
        st = self.L.pf_color_fastq(self.h, int(colour), _ptr(text) if n else None, n, int(final), C.byref(used), stats.ctypes.data, C.byref(bad))
        if st != PF_OK:
            e = DeviceError(st, self.L.pf_last_error(self.h).decode())
            e.bad_record = bad.value
            raise e
        return used.value, {f: stats[0][f].item() for f in COLOR_STATS.names}

    def _keys_on_device(self, a):
        """a numpy array of 64-bit keys as a device tensor (a device tensor stays what it is)"""
        if not isinstance(a, (list, tuple, np.ndarray)):
            return a
        import torch
        a = np.ascontiguousarray(a, dtype=np.uint64)
        return torch.from_numpy(a.view(np.int64).copy()).to("cuda")

    def kmer_union(self, arrays):
        """K-UNION (pf_kmer_union): the sorted distinct union (numpy u64) of sorted distinct arrays of 64-bit keys -- numpy arrays, which
        are copied to the device first, or device tensors.  An array that is not ascending or holds a key twice raises DeviceError."""
        dev = [self._keys_on_device(a) for a in arrays]
        ns = np.array([int(d.shape[0]) for d in dev], dtype=np.uint64)
        ptrs = np.array([_ptr(d) if int(d.shape[0]) else 0 for d in dev], dtype=np.uint64)
        out, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.pf_kmer_union(self.h, len(dev), _ptr(ptrs) if len(dev) else None, _ptr(ns) if len(dev) else None, C.byref(out), C.byref(n)))
        res = np.zeros(n.value, dtype=np.uint64)
        try:
            if n.value:
                self._check(self.L.pf_copy_to_host(self.h, _ptr(res), out, n.value * 8))
        finally:
            self.L.pf_device_free(self.h, out)
        return res

    def color_kmers(self, colour: int, kmers):
        """K-COLORSET (pf_color_kmers): colours with `colour` the graph k-mers among `kmers`, the distinct canonical k-mers of that
        colour's reads (a numpy array, copied to the device first, or a device tensor); returns this call's statistics."""
        dev = self._keys_on_device(kmers)
        n = int(dev.shape[0])
        stats = np.zeros(1, dtype=COLOR_KMERS_STATS)
        self._check(self.L.pf_color_kmers(self.h, int(colour), _ptr(dev) if n else None, n, stats.ctypes.data))
        return {f: int(stats[0][f]) for f in COLOR_KMERS_STATS.names}

    def color_finish(self):
        """pf_color_finish and pf_color_fetch: (statistics of the whole colouring, what leaves the device: per line `heads` u64, `m` u32,
        `slot` u32, `run_off` u64 of lines + 1 entries, and `runs` u32 [n, 2] = first id, last id)"""
        stats = np.zeros(1, dtype=COLOR_STATS)
        self._check(self.L.pf_color_finish(self.h, stats.ctypes.data))
        nl, nr = int(stats[0]["lines"]), int(stats[0]["runs"])
        got = dict(heads=np.zeros(nl, dtype=np.uint64), m=np.zeros(nl, dtype=np.uint32), slot=np.zeros(nl, dtype=np.uint32),
                   run_off=np.zeros(nl + 1, dtype=np.uint64), runs=np.zeros((nr, 2), dtype=np.uint32))
        self._check(self.L.pf_color_fetch(self.h, _ptr(got["heads"]) if nl else None, _ptr(got["m"]) if nl else None, _ptr(got["slot"]) if nl else None,
                                          _ptr(got["run_off"]), _ptr(got["runs"]) if nr else None))
        return {f: stats[0][f].item() for f in COLOR_STATS.names}, got

    def kmc_encode(self, kmers, counts, k: int, p: int, counter_bytes: int):
        """pf_kmc_encode, the inverse of kmc_decode: (records u8, lut u64 of 4^p + 1 entries) of sorted distinct k-mers.  kmers / counts:
        numpy arrays or device tensors."""
        if isinstance(kmers, np.ndarray):
            kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        if isinstance(counts, np.ndarray):
            counts = np.ascontiguousarray(counts, dtype=np.uint32)
        n = int(kmers.shape[0])
        rec = np.zeros(max(n * ((k - p) // 4 + counter_bytes), 1), dtype=np.uint8)
        lut = np.zeros(4 ** p + 1, dtype=np.uint64)
        self._check(self.L.pf_kmc_encode(self.h, _ptr(kmers) if n else None, _ptr(counts) if n else None, n, k, p, counter_bytes, _ptr(rec), _ptr(lut)))
        return rec[: n * ((k - p) // 4 + counter_bytes)], lut

    def lookup(self, kmers: np.ndarray):
        n = len(kmers)
        c = np.zeros(n, dtype=np.uint32)
        f = np.zeros(n, dtype=np.uint8)
        self._check(self.L.pf_lookup_kmers(self.h, _ptr(np.ascontiguousarray(kmers, dtype=np.uint64)), n, _ptr(c), _ptr(f)))
        return c, f

    def upload_counts_colored(self, dbs, min_count=1, max_count=0xFFFFFFFF):
        """dbs: list of (kmers u64, counts u32[, both_strands]) per colour -> one joined table (pf_upload_counts_colored)."""
        nc = len(dbs)
        self.n_colors = nc
        km = [np.ascontiguousarray(d[0], dtype=np.uint64) for d in dbs]
        ct = [np.ascontiguousarray(d[1], dtype=np.uint32) for d in dbs]
        pk = (C.c_void_p * nc)(*[a.ctypes.data for a in km])
        pc = (C.c_void_p * nc)(*[a.ctypes.data for a in ct])
        n = np.array([len(a) for a in km], dtype=np.uint64)
        mn = np.full(nc, min_count, dtype=np.uint64)
        mx = np.full(nc, max_count, dtype=np.uint64)
        both = np.array([int(d[2]) if len(d) > 2 else 1 for d in dbs], dtype=np.int32)
        self._check(self.L.pf_upload_counts_colored(self.h, nc, pk, pc, n.ctypes.data, mn.ctypes.data, mx.ctypes.data, both.ctypes.data))

    def unitig_cov_colored(self, u0=0, u1=None, probe=False):
        """(sum, min, max, miss), each [n_colors, u1 - u0]; probe: pf_unitig_cov_colored_probe (table look-ups at call time)"""
        u1 = self.n if u1 is None else u1
        shape = (self.n_colors, u1 - u0)
        s = np.zeros(shape, dtype=np.uint64)
        lo = np.zeros(shape, dtype=np.uint32)
        hi = np.zeros(shape, dtype=np.uint32)
        x = np.zeros(shape, dtype=np.uint8)
        fn = self.L.pf_unitig_cov_colored_probe if probe else self.L.pf_unitig_cov_colored
        self._check(fn(self.h, u0, u1, _ptr(s), _ptr(lo), _ptr(hi), _ptr(x)))
        return s, lo, hi, x

    def string_cov_colored(self, strings: list[bytes], low, up):
        """(sum, ok), each [n_strings, n_colors]; low / up: one cutoff per colour"""
        n = len(strings)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in strings], out=off[1:])
        text = np.frombuffer(b"".join(strings) + b"\0", dtype=np.uint8).copy()
        lo = np.ascontiguousarray(low, dtype=np.uint32)
        hi = np.ascontiguousarray(up, dtype=np.uint32)
        s = np.zeros((n, self.n_colors), dtype=np.uint64)
        ok = np.zeros((n, self.n_colors), dtype=np.uint8)
        self._check(self.L.pf_string_cov_colored(self.h, text.ctypes.data, off.ctypes.data, n, lo.ctypes.data, hi.ctypes.data,
                                                 s.ctypes.data, ok.ctypes.data))
        return s, ok

    # ---- kernels
    def unitig_cov(self, u0=0, u1=None, out=None):
        u1 = self.n if u1 is None else u1
        if out is None:
            s = np.zeros(u1 - u0, dtype=np.uint64)
            m = np.zeros(u1 - u0, dtype=np.uint32)
            x = np.zeros(u1 - u0, dtype=np.uint8)
        else:
            s, m, x = out
        if getattr(self, "both_strands", True):
            st = self._check(self.L.pf_unitig_cov(self.h, u0, u1, _ptr(s), _ptr(m), _ptr(x)), allow=(PF_ERR_MISSING_KMER,))
        else:  # database without canonical counting: the unitigs as stored
            st = self._check(self.L.pf_unitig_cov_exact(self.h, u0, u1, 0, _ptr(s), _ptr(m), _ptr(x)), allow=(PF_ERR_MISSING_KMER,))
        return s, m, x, st

    def unitig_cov_probe(self, u0=0, u1=None):
        """pf_unitig_cov_probe: C1 with every k-mer looked up in the hash table at call time (never the joined SoA)"""
        u1 = self.n if u1 is None else u1
        s = np.zeros(u1 - u0, dtype=np.uint64)
        m = np.zeros(u1 - u0, dtype=np.uint32)
        x = np.zeros(u1 - u0, dtype=np.uint8)
        st = self._check(self.L.pf_unitig_cov_probe(self.h, u0, u1, _ptr(s), _ptr(m), _ptr(x)), allow=(PF_ERR_MISSING_KMER,))
        return s, m, x, st

    def unitig_cov_exact(self, reverse: bool, u0=0, u1=None):
        """pf_unitig_cov_exact: every k-mer looked up as it reads in the given orientation"""
        u1 = self.n if u1 is None else u1
        s = np.zeros(u1 - u0, dtype=np.uint64)
        m = np.zeros(u1 - u0, dtype=np.uint32)
        x = np.zeros(u1 - u0, dtype=np.uint8)
        st = self._check(self.L.pf_unitig_cov_exact(self.h, u0, u1, int(reverse), _ptr(s), _ptr(m), _ptr(x)), allow=(PF_ERR_MISSING_KMER,))
        return s, m, x, st

    def count_candidates(self, u0=0, u1=None) -> int:
        u1 = self.n if u1 is None else u1
        n = C.c_uint64()
        self._check(self.L.pf_count_candidates(self.h, u0, u1, C.byref(n)))
        return n.value

    def bfs(self, u0=0, u1=None, pool_cap=None):
        u1 = self.n if u1 is None else u1
        n = self.count_candidates(u0, u1)
        rec = np.zeros(max(n, 1), dtype=BFS_RECORD)
        pool_cap = pool_cap or max(1024, n * 8)
        while True:
            pool = np.zeros(pool_cap, dtype=np.uint32)
            nr, used = C.c_uint64(), C.c_uint64()
            st = self.L.pf_bfs_candidates(self.h, u0, u1, rec.ctypes.data, len(rec), pool.ctypes.data, pool_cap, C.byref(nr),
                                          C.byref(used))
            if st == PF_ERR_OVERFLOW and used.value > pool_cap:
                pool_cap = int(used.value)
                continue
            self._check(st)
            return rec[: nr.value], pool[: used.value]

    def _bfs_handing_over(self, entry, u0, u1, pool_cap, entrances):
        """pf_bfs_candidates_split / _begin: (records, pool, deferred[, deferred_entrance]) with a pool that is large enough"""
        u1 = self.n if u1 is None else u1
        n = self.count_candidates(u0, u1)
        rec = np.zeros(max(n, 1), dtype=BFS_RECORD)
        deferred = np.zeros(max(n, 1), dtype=np.uint32)
        entrance = (np.zeros(max(n, 1), dtype=np.uint32),) if entrances else ()
        pool_cap = pool_cap or max(1024, n * 8)
        while True:
            pool = np.zeros(pool_cap, dtype=np.uint32)
            nr, used, nd = C.c_uint64(), C.c_uint64(), C.c_uint64()
            st = entry(self.h, u0, u1, rec.ctypes.data, len(rec), pool.ctypes.data, pool_cap, C.byref(nr), C.byref(used),
                       deferred.ctypes.data, *[e.ctypes.data for e in entrance], len(deferred), C.byref(nd))
            if st == PF_ERR_OVERFLOW and used.value > pool_cap:
                pool_cap = int(used.value)
                continue
            self._check(st)
            if entrances:
                self._bfs_pending = (rec, pool)   # written to until bfs_end()
            return (rec[: nr.value], pool[: used.value], deferred[: nd.value]) + tuple(e[: nd.value] for e in entrance)

    def bfs_split(self, u0=0, u1=None, pool_cap=None):
        """(records, pool, deferred): what the wavefront tier gave up is left to the caller -- records[deferred] hold an entrance only"""
        return self._bfs_handing_over(self.L.pf_bfs_candidates_split, u0, u1, pool_cap, entrances=False)

    def bfs_begin(self, u0=0, u1=None, pool_cap=None):
        """(records, pool, deferred, deferred_entrance) like bfs_split; records and pool are still on their way until bfs_end()"""
        return self._bfs_handing_over(self.L.pf_bfs_candidates_begin, u0, u1, pool_cap, entrances=True)

    def bfs_end(self):
        self._check(self.L.pf_bfs_candidates_end(self.h))
        self._bfs_pending = None

    def bfs_resident(self, u0=0, u1=None):
        """(n_records, pool_used, deferred, deferred_entrance): records and pool stay on the device, for side_components(n_records=...)"""
        u1 = self.n if u1 is None else u1
        n = self.count_candidates(u0, u1)
        deferred = np.zeros(max(n, 1), dtype=np.uint32)
        entrance = np.zeros(max(n, 1), dtype=np.uint32)
        nr, used, nd = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.pf_bfs_candidates_resident(self.h, u0, u1, C.byref(nr), C.byref(used), deferred.ctypes.data, entrance.ctypes.data,
                                                      len(deferred), C.byref(nd)))
        return nr.value, used.value, deferred[: nd.value], entrance[: nd.value]

    def side_components(self, records=None, pool=None, n_records=None, reset=True, extra=None, extra_pool=None):
        """K-CC: the records (default: the ones the last bfs() call left on the device) join the union-find over unitig sides"""
        if records is None:
            rp, pp, n, pl = None, None, int(n_records), 0
        else:
            records = np.ascontiguousarray(records)
            pool = np.ascontiguousarray(pool, dtype=np.uint32) if len(pool) else np.zeros(1, dtype=np.uint32)
            rp, pp, n, pl = records.ctypes.data, pool.ctypes.data, len(records), len(pool)
        xr = xp = None
        nx = nxp = 0
        if extra is not None and len(extra):
            extra = np.ascontiguousarray(extra)
            extra_pool = np.ascontiguousarray(extra_pool, dtype=np.uint32) if len(extra_pool) else np.zeros(1, dtype=np.uint32)
            xr, xp, nx, nxp = extra.ctypes.data, extra_pool.ctypes.data, len(extra), len(extra_pool)
        self._check(self.L.pf_side_components(self.h, int(reset), rp, n, pp, pl, xr, nx, xp, nxp))
        self._cc_n = n

    def replay_order(self, n_classes: int = 64):
        """(order, class_off, labels) of the records of the last side_components call"""
        n = self._cc_n
        order = np.zeros(max(n, 1), dtype=np.uint32)
        labels = np.zeros(max(n, 1), dtype=np.uint32)
        off = np.zeros(n_classes + 1, dtype=np.uint32)
        self._check(self.L.pf_replay_order(self.h, n_classes, order.ctypes.data, off.ctypes.data, labels.ctypes.data))
        return order[:n], off, labels[:n]

    def string_cov(self, strings: list[bytes], low: int, up: int):
        n = len(strings)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in strings], out=off[1:])
        text = np.frombuffer(b"".join(strings) + b"\0", dtype=np.uint8).copy()
        s = np.zeros(n, dtype=np.uint64)
        ok = np.zeros(n, dtype=np.uint8)
        miss = np.zeros(n, dtype=np.uint8)
        self._check(self.L.pf_string_cov(self.h, text.ctypes.data, off.ctypes.data, n, low, up, s.ctypes.data, ok.ctypes.data,
                                         miss.ctypes.data))
        return s, ok, miss

    def align_batch(self, pairs: list[tuple[bytes, bytes]], M=2.0, D=-1.0, G=-3.0):
        """Returns, per job, the list of (a_row, b_row, gap_pos, score, n_pos, n_indel)."""
        n = len(pairs)
        jobs = np.zeros(n, dtype=ALIGN_JOB)
        chunks = []
        pos = 0
        for j, (a, b) in enumerate(pairs):
            jobs[j] = (pos, pos + len(a), len(a), len(b))
            chunks += [a, b]
            pos += len(a) + len(b)
        text = np.frombuffer(b"".join(chunks) + b"\0", dtype=np.uint8).copy()
        hit_cap, text_cap, gap_cap = max(64, 4 * n), max(4096, 8 * pos), max(1024, 4 * n * 8)
        while True:
            first = np.zeros(n, dtype=np.uint64)
            count = np.zeros(n, dtype=np.uint32)
            hits = np.zeros(hit_cap, dtype=ALIGN_HIT)
            otext = np.zeros(text_cap, dtype=np.uint8)
            ogap = np.zeros(gap_cap, dtype=np.uint32)
            used = (C.c_uint64 * 3)()
            st = self.L.pf_align_batch(self.h, text.ctypes.data, pos, jobs.ctypes.data, n, M, D, G, first.ctypes.data,
                                       count.ctypes.data, hits.ctypes.data, hit_cap, otext.ctypes.data, text_cap, ogap.ctypes.data, gap_cap, used)
            if st == PF_ERR_OVERFLOW and (used[0] > hit_cap or used[1] > text_cap or used[2] > gap_cap):
                hit_cap, text_cap, gap_cap = max(hit_cap, used[0]), max(text_cap, used[1]), max(gap_cap, used[2])
                continue
            self._check(st)
            break
        out = []
        tb = otext.tobytes()
        for j in range(n):
            lst = []
            for h in hits[int(first[j]) : int(first[j]) + int(count[j])]:
                o, ln = int(h["text_off"]), int(h["len"])
                gp = ogap[int(h["gap_off"]) : int(h["gap_off"]) + int(h["n_gaps"])].copy()
                lst.append((tb[o : o + ln], tb[o + ln : o + 2 * ln], gp, int(h["score"]), int(h["n_pos"]), int(h["n_indel"])))
            out.append(lst)
        return out

    def align_bubbles(self, bubbles: list[list], M=2.0, D=-1.0, G=-3.0):
        """bubbles[t] = list of paths, each either bytes (ASCII) or an int oriented-unitig id.
        Returns per bubble None (no alignment) or dict(rows, sites=[(col, is_indel, groups)], indel_len)."""
        nt = len(bubbles)
        tasks = np.zeros(nt, dtype=BUBBLE_TASK)
        paths = []
        chunks = []
        pos = 0
        lens = self._keep[2]
        for t, b in enumerate(bubbles):
            tasks[t] = (len(paths), len(b), 0)
            for x in b:
                if isinstance(x, (bytes, bytearray)):
                    paths.append((pos, len(x), NONE))
                    chunks.append(bytes(x))
                    pos += len(x)
                else:
                    paths.append((0, int(lens[int(x) >> 1]), int(x)))
        parr = np.array(paths, dtype=BUBBLE_PATH)
        text = np.frombuffer(b"".join(chunks) + b"\0", dtype=np.uint8).copy()
        caps = [max(4096, 4 * int(parr["len"].sum())), max(256, 8 * nt), max(1024, 32 * nt), max(256, 4 * nt)]
        while True:
            res = np.zeros(nt, dtype=BUBBLE_RESULT)
            otext = np.zeros(caps[0], dtype=np.uint8)
            osites = np.zeros(caps[1], dtype=BUBBLE_SITE)
            ogroups = np.zeros(caps[2], dtype=np.uint8)
            oilen = np.zeros(caps[3], dtype=np.uint32)
            used = (C.c_uint64 * 4)()
            st = self.L.pf_align_bubbles(self.h, text.ctypes.data, pos, parr.ctypes.data, len(parr), tasks.ctypes.data, nt, M, D, G,
                                         res.ctypes.data, otext.ctypes.data, caps[0], osites.ctypes.data, caps[1],
                                         ogroups.ctypes.data, caps[2], oilen.ctypes.data, caps[3], used)
            if st == PF_ERR_OVERFLOW and any(used[i] > caps[i] for i in range(4)):
                caps = [max(caps[i], int(used[i])) for i in range(4)]
                continue
            self._check(st)
            break
        out = []
        tb = otext.tobytes()
        for r in res:
            R, L = int(r["n_rows"]), int(r["n_cols"])
            if R == 0:
                out.append(None)
                continue
            o = int(r["rows_off"])
            rows = [tb[o + i * L : o + (i + 1) * L] for i in range(R)]
            sites = []
            for i in range(int(r["n_sites"])):
                srec = osites[int(r["site_off"]) + i]
                g0 = int(r["group_off"]) + i * R
                sites.append((int(srec["col"]), int(srec["is_indel"]), int(srec["maxnum"]), ogroups[g0 : g0 + R].tolist()))
            il = oilen[int(r["ilen_off"]) : int(r["ilen_off"]) + int(r["n_indel_len"])].tolist()
            out.append(dict(rows=rows, sites=sites, indel_len=il))
        return out
