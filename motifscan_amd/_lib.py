"""
motifscan_amd._lib -- ctypes binding of libmotifscan_amd.so (include/motifscan_amd.h).

The shared library is built in-tree by motifscan_amd/csrc/Makefile (hipcc, gfx950).  There is
no CPU implementation behind it: if the library is missing, or no MI355X is visible when a
compute entry point is called, the call raises -- it never falls back.
"""
import contextlib
import ctypes
import importlib.util
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmotifscan_amd.so")

MS_OK, MS_ERR_INVALID, MS_ERR_NOMEM, MS_ERR_RUNTIME = 0, 1, 2, 3
MS_ERR_INTERNAL = 4
MS_SCAN_DEFAULT, MS_SCAN_EXACT_ONLY, MS_SCAN_COUNTS_ONLY = 0, 1, 2
MS_STREAM_DEDUP, MS_STREAM_NO_HITS, MS_STREAM_EXACT_ONLY, MS_STREAM_PACKED, MS_STREAM_HOST_PACK, MS_STREAM_PACKED12 = 1, 2, 4, 8, 16, 32
MS_PROFILE_UNSMOOTHED = 1
MS_SCOREHIST_MAX_BINS, MS_HIST_PER_POSITION = 4096, 1
MS_REPLAY_DONE, MS_REPLAY_WORDS, MS_REPLAY_ATTEMPTS, MS_REPLAY_NO_SIZE, MS_REPLAY_EMPTY_RANGE, MS_REPLAY_WIDE = 0, 1, 2, 3, 4, 5
MS_REPLAY_SIZE_MISSING = -(1 << 63)


class ScanStats(ctypes.Structure):
    _fields_ = [("n_bases", ctypes.c_int64), ("n_windows", ctypes.c_int64), ("n_candidates", ctypes.c_int64),
                ("n_hits", ctypes.c_int64), ("n_pwms", ctypes.c_int32), ("n_pwms_exact", ctypes.c_int32),
                ("n_tiles", ctypes.c_int32), ("n_passes", ctypes.c_int32), ("ms_prefilter", ctypes.c_double),
                ("ms_exact", ctypes.c_double), ("ms_sort", ctypes.c_double), ("ms_finalize", ctypes.c_double),
                ("ms_total", ctypes.c_double), ("lds_bytes_read", ctypes.c_int64),
                ("hbm_bytes_algorithmic", ctypes.c_int64), ("pf_clock_mhz", ctypes.c_double),
                ("mfma_ops", ctypes.c_int64), ("mfma_ops_algorithmic", ctypes.c_int64), ("pf_engine", ctypes.c_int32),
                ("order_overflow_runs", ctypes.c_int32), ("order_bucketed", ctypes.c_int32), ("reserved0", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Span(ctypes.Structure):
    """ms_span: one span of a host-streamed window sweep."""
    _fields_ = [("chrom", ctypes.c_int32), ("reserved", ctypes.c_int32), ("begin", ctypes.c_int64), ("end", ctypes.c_int64),
                ("first_window", ctypes.c_int64), ("n_windows", ctypes.c_int64)]


_lib = None


def build(verbose=False):
    """Compile libmotifscan_amd.so in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.run(cmd, check=True)
    return LIB_PATH


def _preload_hip_runtime():
    """torch wheels carry their own libamdhip64.so (same SONAME as /opt/rocm's).  If torch is
    installed, map ITS copy first so that this library and torch share one HIP runtime in the
    process whichever gets imported first."""
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is not built (run `python -c 'import __graft_entry__ as g; g.build()'` or "
            f"`make -C motifscan_amd/csrc`); motifscan_amd has no CPU fallback")
    _preload_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    c_int, c_i32, c_i64, c_u32, vp = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p
    pd, pi32, pi64 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_i32), ctypes.POINTER(c_i64)
    pi8, pu8, pu32 = ctypes.POINTER(ctypes.c_int8), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(c_u32)
    pvp = ctypes.POINTER(vp)
    sig = {
        "ms_last_error": (ctypes.c_char_p, []),
        "ms_version": (c_int, []),
        "ms_device_count": (c_int, [ctypes.POINTER(c_int)]),
        "ms_set_device": (c_int, [c_int]),
        "ms_device_name": (c_int, [ctypes.c_char_p, c_int]),
        "ms_numa_bind_thread": (c_int, [c_int, ctypes.POINTER(c_int)]),
        "ms_pwmset_create": (c_int, [pd, pi32, pd, c_i32, pvp]),
        "ms_pwmset_set_cutoffs": (c_int, [vp, pd]),
        "ms_pwmset_size": (c_int, [vp, pi32]),
        "ms_pwmset_max_raw": (c_int, [vp, pd]),
        "ms_pwmset_free": (None, [vp]),
        "ms_seqset_create": (c_int, [ctypes.c_char_p, pi64, c_i64, c_int, pvp]),
        "ms_seqset_create_hostpacked": (c_int, [ctypes.c_char_p, pi64, c_i64, c_int, pvp]),
        "ms_debug_host_pack": (c_int, [ctypes.c_char_p, pi64, c_i64, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), pi32, pi32]),
        "ms_seqset_from_device": (c_int, [vp, pi64, c_i64, pvp]),
        "ms_seqset_repack": (c_int, [vp]),
        "ms_seqset_size": (c_int, [vp, pi64, pi64]),
        "ms_seqset_free": (None, [vp]),
        "ms_genome_create": (c_int, [ctypes.c_char_p, pi64, c_i32, pvp]),
        "ms_genome_size": (c_int, [vp, pi32, pi64]),
        "ms_genome_create_packed": (c_int, [pu32, pu32, pi64, c_i32, pvp]),
        "ms_genome_packed_host": (c_int, [vp, pu32, pu32]),
        "ms_pack_bases_host": (c_int, [ctypes.c_char_p, c_i64, c_int, pu32, pu32]),
        "ms_genome_free": (None, [vp]),
        "ms_seqset_from_genome": (c_int, [vp, pi32, pi64, pi64, c_i64, pvp]),
        "ms_genome_base_counts": (c_int, [vp, pi64]),
        "ms_genome_window_filter": (c_int, [vp, pi64, c_i64, c_i32, c_i32, pi64, c_i64, c_i64, pi64, pi64]),
        "ms_randint_replay_host": (c_int, [pu32, c_i64, pi64, c_i64, pi64, pi64, pi64]),
        "ms_genes_create": (c_int, [pi64, c_i32, pi64, pi8, pvp]),
        "ms_genes_free": (None, [vp]),
        "ms_genes_nearest_tss": (c_int, [vp, pi32, pi64, c_i64, c_i64, pi64, pu8]),
        "ms_genes_promoter_overlap": (c_int, [vp, c_i64, c_i64, pi32, pi64, pi64, c_i64, pu8]),
        "ms_control_regions_replay_host": (c_int, [pu32, c_i64, c_i64, pi64, pi64, pi64, pi64, pi64, pu8, pi64, pi8, c_i32, c_i64,
                                                   pi64, pi64, pi64, pi64, pi32, pi64]),
        "ms_scan": (c_int, [vp, vp, c_int, c_u32, pvp]),
        "ms_scan_sweep": (c_int, [vp, vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_int, c_u32, pvp]),
        "ms_scan_regions_once": (c_int, [vp, vp, pi32, pi64, pi64, c_i64, c_int, c_u32, pvp]),
        "ms_result_num_hits": (c_int, [vp, pi64]),
        "ms_result_motif_offsets": (c_int, [vp, pi64]),
        "ms_result_hits": (c_int, [vp, pi64, pi64, pd, pi8]),
        "ms_result_hits_host": (c_int, [vp, ctypes.POINTER(pi64), ctypes.POINTER(pi64), ctypes.POINTER(pd), ctypes.POINTER(pi8)]),
        "ms_result_hits_packed_host": (c_int, [vp, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint64)), ctypes.POINTER(pd)]),
        "ms_result_hits_packed12_host": (c_int, [vp, ctypes.POINTER(pu32), ctypes.POINTER(pd), pi32]),
        "ms_result_packed_form": (c_int, [vp, pi32]),
        "ms_host_alloc": (c_int, [ctypes.c_size_t, pvp]),
        "ms_device_pool_stats": (c_int, [ctypes.POINTER(ctypes.c_uint64)]),
        "ms_host_free": (None, [vp]),
        "ms_host_pool_stats": (c_int, [ctypes.POINTER(ctypes.c_uint64)]),
        "ms_stream_create": (c_int, [vp, c_int, c_u32, c_int, pvp]),
        "ms_stream_submit": (c_int, [vp, vp, pi64, c_i64]),
        "ms_stream_submit_counts_only": (c_int, [vp, vp, pi64, c_i64]),
        "ms_stream_submit_span": (c_int, [vp, vp, c_i64, c_i32, c_i32]),
        "ms_stream_submit_regions": (c_int, [vp, vp, pi32, pi64, pi64, c_i64]),
        "ms_stream_next": (c_int, [vp, pvp]),
        "ms_stream_in_flight": (c_int, [vp, ctypes.POINTER(c_int)]),
        "ms_stream_capacity": (c_int, [vp, ctypes.POINTER(c_int)]),
        "ms_stream_stats": (c_int, [vp, ctypes.POINTER(ctypes.c_double)]),
        "ms_stream_free": (None, [vp]),
        "ms_sweep_spans": (c_int, [pi64, c_i32, c_i32, c_i32, c_i64, ctypes.POINTER(Span), c_i64, pi64]),
        "ms_result_region_counts": (c_int, [vp, pi64]),
        "ms_result_region_counts_device": (c_int, [vp, pvp]),
        "ms_result_stats": (c_int, [vp, ctypes.POINTER(ScanStats)]),
        "ms_result_dedup": (c_int, [vp, vp]),
        "ms_result_site_tables": (c_int, [vp, pi32, pd]),
        "ms_result_free": (None, [vp]),
        "ms_result_from_hits": (c_int, [c_i32, c_i64, pi64, pi64, pi64, pd, pi8, pvp]),
        "ms_result_site_histogram": (c_int, [vp, vp, pi64, c_i64, c_i32, c_i32, pi64, pi64]),
        "ms_result_rank_profile": (c_int, [vp, pi64, pd, pd, c_i32, c_i32, c_int, vp]),
        "ms_result_cooccurrence": (c_int, [vp, c_i32, c_i32, vp]),
        "ms_result_pair_spacing": (c_int, [vp, vp, c_i32, c_i32, c_i32, c_i32, pi64, pi64]),
        "ms_result_site_base_counts": (c_int, [vp, vp, vp, c_i32, c_i32, c_i32, c_u32, vp, vp, vp, pd]),
        "ms_debug_sitestack_dims": (c_int, [pi32]),
        "ms_track_create": (c_int, [vp, pi64, c_i64, pvp]),
        "ms_track_size": (c_int, [vp, pi64, pi64]),
        "ms_track_values_host": (c_int, [vp, c_i64, c_i64, pi32]),
        "ms_track_free": (None, [vp]),
        "ms_result_site_signal": (c_int, [vp, vp, vp, c_i32, c_i32, c_i32, c_u32, vp, vp, vp, vp, pd]),
        "ms_debug_sitesignal_dims": (c_int, [pi32]),
        "ms_debug_pair_lds_bins": (c_int, []),
        "ms_debug_cooc_chunk_regions": (c_int, []),
        "ms_debug_plot_dims": (c_int, [pi32]),
        "ms_debug_pair_lds_pair_limit": (c_int, [c_i64, pi64]),
        "ms_debug_genome_dims": (c_int, [pi32]),
        "ms_debug_seqset_planes": (c_int, [vp, pu32, pu32, pi32, pi32]),
        "ms_debug_score_rank_budget": (c_int, [c_i64, pi64]),
        "ms_score": (c_int, [vp, vp, c_int, pd]),
        "ms_score_ranks": (c_int, [vp, vp, c_int, pi64, c_i32, pd]),
        "ms_dedup_hits": (c_int, [pi64, c_i32, pi32, pi64, pi64, pd, pi8, pu8]),
        "ms_debug_plan_dims": (c_int, [vp, c_int, c_i64, pi32, pi32, pi32, pi32]),
        "ms_debug_plan_rows": (c_int, [vp, pi32, ctypes.POINTER(ctypes.c_int16), pi32, pi32, pi32, pi32, pi32, pi32]),
        "ms_debug_release_scratch": (c_int, []),
        "ms_debug_scan_candidates": (c_int, [vp, vp, c_int, c_u32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), pi64]),
        "ms_debug_scan_from_candidates": (c_int, [vp, vp, c_int, c_u32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64, pvp]),
        "ms_debug_numa_probe": (c_int, [ctypes.c_char_p, ctypes.c_char_p, pi32, pi32, pi32]),
        "ms_scan_variants": (c_int, [vp, vp, pi32, pi64, ctypes.c_char_p, c_i64, c_int, c_u32, pvp]),
        "ms_varscan_num_sites": (c_int, [vp, pi64]),
        "ms_varscan_motif_offsets": (c_int, [vp, pi64]),
        "ms_varscan_sites": (c_int, [vp, pi64, pi64, pi8, pd, pd, pu8]),
        "ms_varscan_ref_codes": (c_int, [vp, pi8]),
        "ms_varscan_motif_counts": (c_int, [vp, pi64, pi64]),
        "ms_varscan_device_ms": (c_int, [vp, pd]),
        "ms_varscan_free": (None, [vp]),
        "ms_debug_varscan_chunk": (c_int, [c_i64, pi64]),
        "ms_debug_varscan_dims": (c_int, [pi32]),
        "ms_debug_bucket_plan": (c_int, [pi64, c_i64, pi32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_i64,
                                 ctypes.POINTER(ctypes.c_uint64), ctypes.c_double, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32,
                                 ctypes.POINTER(ctypes.c_uint64), pi32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "ms_scan_alleles": (c_int, [vp, vp, pi32, pi64, pi32, ctypes.c_char_p, pi64, ctypes.c_char_p, c_i64, c_int, c_u32, pvp]),
        "ms_allelescan_num_sites": (c_int, [vp, pi64]),
        "ms_allelescan_motif_offsets": (c_int, [vp, pi64]),
        "ms_allelescan_sites": (c_int, [vp, pi64, pu8, pi64, pi8, pd]),
        "ms_allelescan_motif_counts": (c_int, [vp, pi64, pi64]),
        "ms_allelescan_ref_mismatch": (c_int, [vp, pu8]),
        "ms_allelescan_device_ms": (c_int, [vp, pd]),
        "ms_allelescan_free": (None, [vp]),
        "ms_scan_alleles_best": (c_int, [vp, vp, pi32, pi64, pi32, ctypes.c_char_p, pi64, ctypes.c_char_p, c_i64, c_int, c_u32, pvp]),
        "ms_allelebest_shape": (c_int, [vp, pi32, pi64]),
        "ms_allelebest_sites": (c_int, [vp, c_i32, c_i32, pd, pi32, pi8, pd, pi32, pi8]),
        "ms_allelebest_sites_device": (c_int, [vp, pvp, pvp, pvp, pvp, pvp, pvp]),
        "ms_allelebest_ref_mismatch": (c_int, [vp, pu8]),
        "ms_allelebest_device_ms": (c_int, [vp, pd]),
        "ms_allelebest_free": (None, [vp]),
        "ms_debug_allelebest_dims": (c_int, [pi32]),
        "ms_scan_best": (c_int, [vp, vp, c_int, c_u32, pvp]),
        "ms_best_shape": (c_int, [vp, pi32, pi64]),
        "ms_best_sites": (c_int, [vp, c_i32, c_i32, pd, pi32, pi8]),
        "ms_best_sites_device": (c_int, [vp, pvp, pvp, pvp]),
        "ms_best_device_ms": (c_int, [vp, pd]),
        "ms_best_free": (None, [vp]),
        "ms_debug_best_segment_windows": (c_int, []),
        "ms_best_rank_sum": (c_int, [vp, pu8, vp, pu8, c_i32, c_i32, c_u32, pi64, ctypes.POINTER(ctypes.c_uint64), pi64, pd]),
        "ms_best_count_passing": (c_int, [vp, pu8, pd, c_i32, c_i32, c_i32, pi64, pd]),
        "ms_debug_ranksum_dims": (c_int, [pi32]),
        "ms_debug_ranksum_budget": (c_int, [c_i64, pi64]),
        "ms_scan_affinity": (c_int, [vp, vp, c_int, ctypes.c_double, c_i32, c_u32, pvp]),
        "ms_affinity_shape": (c_int, [vp, pi32, pi64]),
        "ms_affinity_cells": (c_int, [vp, c_i32, c_i32, pd, pd, pi32, pd]),
        "ms_affinity_cells_device": (c_int, [vp, pvp, pvp, pvp, pvp]),
        "ms_affinity_device_ms": (c_int, [vp, pd]),
        "ms_affinity_free": (None, [vp]),
        "ms_affinity_rank_sum": (c_int, [vp, pu8, vp, pu8, c_i32, c_i32, c_u32, pi64, ctypes.POINTER(ctypes.c_uint64), pi64, pd]),
        "ms_debug_affinity_dims": (c_int, [pi32]),
        "ms_affinity_expected_counts": (c_int, [vp, vp, vp, ctypes.c_double, c_i32, c_i32, c_u32, vp, vp, vp, pd]),
        "ms_debug_expected_dims": (c_int, [pi32]),
        "ms_debug_expected_grid_cap": (c_int, [c_i32]),
        "ms_debug_alloc_fill": (c_int, [c_i32, pi32]),
        "ms_debug_seqset_pad_words": (c_int, [vp, pu32, pu32]),
        "ms_debug_pool_trim": (c_int, [ctypes.POINTER(ctypes.c_uint64)]),
        "ms_debug_key_layout": (c_int, [c_i64, c_i64, c_i64, c_i32, c_i32, pi32, pi32]),
        "ms_scan_score_histogram": (c_int, [vp, vp, c_int, c_u32, pd, pd, c_i32, c_i32, vp, pd]),
        "ms_debug_scorehist_dims": (c_int, [pi32]),
        "ms_genome_apply_alleles": (c_int, [vp, pi32, pi64, pi32, ctypes.c_char_p, pi64, ctypes.c_char_p, c_i64, c_u32, pvp, pvp]),
        "ms_liftmap_shape": (c_int, [vp, pi32, pi64, pi64]),
        "ms_liftmap_status": (c_int, [vp, pu8]),
        "ms_liftmap_ref_mismatch": (c_int, [vp, pu8]),
        "ms_liftmap_chrom_sizes": (c_int, [vp, pi64, pi64]),
        "ms_liftmap_lift": (c_int, [vp, c_int, pi32, pi64, c_i64, pi64, pu8]),
        "ms_liftmap_device_ms": (c_int, [vp, pd]),
        "ms_liftmap_free": (None, [vp]),
        "ms_debug_personal_dims": (c_int, [pi32]),
        "ms_debug_liftmap_stage_ms": (c_int, [vp, pd]),
        "ms_seqset_packed_host": (c_int, [vp, pu32, pu32]),
        "ms_seqset_shuffle": (c_int, [vp, c_int, ctypes.c_uint64, c_i64, c_u32, pvp]),
        "ms_debug_shuffle_dims": (c_int, [pi32]),
        "ms_debug_shuffle_stage_ms": (c_int, [pd]),
        "ms_seqset_kmer_counts": (c_int, [vp, c_i32, c_u32, pu8, vp, vp, pi64, pd]),
        "ms_genome_kmer_counts": (c_int, [vp, c_i32, c_u32, pu8, vp, vp, pi64, pd]),
        "ms_debug_kmer_dims": (c_int, [pi32]),
        "ms_debug_kmer_bitmap_budget": (c_int, [c_i64, pi64]),
        "ms_debug_counts_dims": (c_int, [pi32]),
        "ms_debug_seqset_upload_only": (c_int, [ctypes.c_char_p, pi64, c_i64, pvp]),
        "ms_pwmset_score_distribution": (c_int, [vp, c_int, c_i32, pd, pd, c_i32, pd, pi64, vp, pd]),
        "ms_debug_scoredist_dims": (c_int, [pi32]),
        "ms_debug_scoredist_budget": (c_int, [c_i64, pi64]),
        "ms_debug_scoredist_force_global": (c_int, [c_i32, pi32]),
        "ms_motifs_compare": (c_int, [pd, pi32, c_i32, pd, pi32, c_i32, c_int, c_i32, c_i32, c_int, c_i32, c_i32, pd, pi32, pi32, pi32, pi32, pi8, pd]),
        "ms_debug_compare_dims": (c_int, [pi32]),
        "ms_debug_compare_budget": (c_int, [c_i64, pi64]),
        "ms_debug_compare_null": (c_int, [pd, pi32, c_i32, pd, pi32, c_i32, c_int, c_i32, c_int, c_i32, pu32, pd]),
        "ms_dimodelset_create": (c_int, [pd, pi32, c_i32, pvp]),
        "ms_dimodelset_size": (c_int, [vp, pi32]),
        "ms_dimodelset_max_raw": (c_int, [vp, pd]),
        "ms_dimodelset_free": (None, [vp]),
        "ms_scan_best_dimodels": (c_int, [vp, vp, c_int, c_u32, pvp]),
        "ms_debug_dimodel_dims": (c_int, [pi32]),
        "ms_scan_best_bipartite": (c_int, [vp, pi32, pi32, pu8, pi32, pi32, c_i32, vp, c_int, c_u32, pvp]),
        "ms_best_gaps": (c_int, [vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_int16)]),
        "ms_best_gaps_device": (c_int, [vp, pvp]),
        "ms_debug_bipartite_dims": (c_int, [pi32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def check(rc):
    """Status code -> the exception class the reference raises for that kind of failure
    (MemoryError / RuntimeError: cscore.c:243-268, 411-430; ValueError: scanner.py:51-54)."""
    if rc == MS_OK:
        return
    msg = lib().ms_last_error().decode("utf-8", "replace")
    if rc == MS_ERR_INVALID:
        raise ValueError(msg)
    if rc == MS_ERR_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def ptr(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def device_count():
    n = ctypes.c_int(0)
    rc = lib().ms_device_count(ctypes.byref(n))
    return n.value if rc == MS_OK else 0


def set_device(device):
    check(lib().ms_set_device(int(device)))


def numa_bind_thread(force=False):
    """Bind the calling thread to the NUMA node of the current device (ms_numa_bind_thread): call it on a rank's main thread before it
    allocates its pinned input buffers.  Returns the node, or -1 if nothing was done (policy off / no NUMA information)."""
    node = ctypes.c_int(-1)
    check(lib().ms_numa_bind_thread(1 if force else 0, ctypes.byref(node)))
    return node.value


def device_name():
    buf = ctypes.create_string_buffer(256)
    check(lib().ms_device_name(buf, 256))
    return buf.value.decode()


# --------------------------------------------------------------------------- handles --

class PwmSet:
    """Device-side PWM set (convert_pwm + get_max_raw_score, cscore.c:36-79)."""

    def __init__(self, values, widths, cutoffs=None):
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.widths = np.ascontiguousarray(widths, dtype=np.int32)
        if self.values.size != 4 * int(self.widths.sum()):
            raise ValueError("values must hold 4*width doubles per PWM")
        self.n = len(self.widths)
        cut = None if cutoffs is None else np.ascontiguousarray(cutoffs, dtype=np.float64)
        if cut is not None and cut.size != self.n:
            raise ValueError("need one cutoff per PWM")
        h = ctypes.c_void_p()
        check(lib().ms_pwmset_create(ptr(self.values, ctypes.c_double), ptr(self.widths, ctypes.c_int32),
                                     None if cut is None else ptr(cut, ctypes.c_double), self.n, ctypes.byref(h)))
        self.h = h

    @classmethod
    def from_matrices(cls, matrices, cutoffs=None):
        mats = []
        for m in matrices:
            a = np.asarray(m, dtype=np.float64)
            if a.ndim != 2 or a.shape[0] != 4:
                raise ValueError("each PWM must have exactly 4 rows (A, C, G, T)")
            if a.shape[1] == 0:
                raise ValueError("each PWM needs at least 1 position per row")
            mats.append(np.ascontiguousarray(a))
        widths = np.array([m.shape[1] for m in mats], dtype=np.int32)
        values = np.concatenate([m.ravel() for m in mats]) if mats else np.zeros(0)
        return cls(values, widths, cutoffs)

    def set_cutoffs(self, cutoffs):
        cut = np.ascontiguousarray(cutoffs, dtype=np.float64)
        if cut.size != self.n:
            raise ValueError("need one cutoff per PWM")
        check(lib().ms_pwmset_set_cutoffs(self.h, ptr(cut, ctypes.c_double)))

    def max_raw(self):
        out = np.zeros(self.n, dtype=np.float64)
        check(lib().ms_pwmset_max_raw(self.h, ptr(out, ctypes.c_double)))
        return out

    def plan(self, strand_mask=3, lds_budget=70 * 1024):
        """Host-side view of the pre-filter plan, decoded from the operand image the kernel reads (tests only):
        group_fields [groups][16] motif of the field (-1 empty; both strands: field n = slot n >> 1, even forward, odd reverse;
        one strand: field n = slot n), rows [groups][16][64 columns][4 bases] and bias [groups][16] in units of 1/8,
        group_kb [groups] matrix instructions per row tile, group_cols [groups] columns of the group's fields incl. the bias
        column (16 per instruction; paired rows: 8), group_paired [groups] 0 = plain row, 1 / 2 = field X / Y of a paired row."""
        L = lib()
        nf, ne, nq, nt = (ctypes.c_int32() for _ in range(4))
        check(L.ms_debug_plan_dims(self.h, strand_mask, lds_budget, ctypes.byref(nf), ctypes.byref(ne),
                                   ctypes.byref(nq), ctypes.byref(nt)))
        gf = np.full((nq.value, 16), -1, dtype=np.int32)
        ex = np.zeros(max(ne.value, 1), dtype=np.int32)
        tf = np.zeros(nt.value + 1, dtype=np.int32)
        rows = np.zeros((nq.value, 16, 64, 4), dtype=np.int16)
        bias = np.zeros((nq.value, 16), dtype=np.int32)
        kb = np.zeros(nq.value, dtype=np.int32)
        cols = np.zeros(nq.value, dtype=np.int32)
        paired = np.zeros(nq.value, dtype=np.int32)
        check(L.ms_debug_plan_rows(self.h, ptr(gf, ctypes.c_int32), ptr(rows, ctypes.c_int16), ptr(bias, ctypes.c_int32),
                                   ptr(kb, ctypes.c_int32), ptr(cols, ctypes.c_int32), ptr(paired, ctypes.c_int32),
                                   ptr(ex, ctypes.c_int32), ptr(tf, ctypes.c_int32)))
        return {"n_fast": nf.value, "n_exact": ne.value, "n_tiles": nt.value, "strand_mask": strand_mask, "group_fields": gf,
                "rows": rows, "bias": bias, "group_kb": kb, "group_cols": cols, "group_paired": paired,
                "exact_motifs": ex[:ne.value], "tile_first_group": tf}

    def close(self):
        if getattr(self, "h", None):
            lib().ms_pwmset_free(self.h)
            self.h = None

    __del__ = close


class SeqSet:
    """Device-side packed sequence set (convert_seq, cscore.c:81-114)."""

    def __init__(self, bases, offsets, keep_ascii=False, host_pack_threads=0):
        """host_pack_threads > 0: convert_seq on that many host threads (ms_seqset_create_hostpacked: no kernel is launched) -- the same set."""
        if isinstance(bases, np.ndarray):
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
            buf = bases.ctypes.data_as(ctypes.c_char_p)
            nbytes = bases.size
        else:
            bases = bytes(bases)
            buf = bases
            nbytes = len(bases)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if self.offsets.ndim != 1 or self.offsets.size < 1:
            raise ValueError("offsets must have n_seqs + 1 entries")
        if int(self.offsets[-1]) != nbytes:
            raise ValueError("offsets[-1] must equal the number of bases")
        self.n_seqs = self.offsets.size - 1
        self.n_bases = nbytes
        h = ctypes.c_void_p()
        if host_pack_threads and not keep_ascii:
            check(lib().ms_seqset_create_hostpacked(buf, ptr(self.offsets, ctypes.c_int64), self.n_seqs, int(host_pack_threads), ctypes.byref(h)))
        else:
            check(lib().ms_seqset_create(buf, ptr(self.offsets, ctypes.c_int64), self.n_seqs, int(bool(keep_ascii)),
                                         ctypes.byref(h)))
        self.h = h

    @classmethod
    def from_strings(cls, seqs, keep_ascii=False):
        seqs = seqs if isinstance(seqs, (list, tuple)) else list(seqs)
        offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
        try:
            lens = np.fromiter(map(len, seqs), dtype=np.int64, count=len(seqs))
            if seqs:
                np.cumsum(lens, out=offsets[1:])
            if seqs and lens[0] > 0 and (lens == lens[0]).all():
                # regions of ONE length (the reference's fixed window around the summit, scanner.py:70-79): numpy encodes the list into one
                # fixed-width byte matrix in a single C loop -- 2.6x faster than join + encode for 100 000 x 1 kb
                raw = np.array(seqs, dtype="S%d" % int(lens[0])).view(np.uint8).reshape(-1)
                if raw.size != int(offsets[-1]):
                    raise TypeError("not a flat list of strings")
            else:                                 # ONE join + ONE encode (plain-ASCII strings: a base is a byte)
                raw = "".join(seqs).encode("ascii")
        except (TypeError, ValueError, UnicodeEncodeError):   # bytes among them, or non-ASCII text (every such byte scores as 'N', cscore.c:92-111)
            bs = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in seqs]
            if bs:
                offsets[1:] = np.cumsum([len(b) for b in bs])
            raw = b"".join(bs)
        return cls(raw, offsets, keep_ascii)

    @classmethod
    def from_device(cls, device_ptr, offsets):
        """ASCII already resident in device memory (e.g. a torch uint8 tensor's data_ptr())."""
        self = cls.__new__(cls)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.n_seqs = self.offsets.size - 1
        self.n_bases = int(self.offsets[-1])
        h = ctypes.c_void_p()
        check(lib().ms_seqset_from_device(ctypes.c_void_p(int(device_ptr)), ptr(self.offsets, ctypes.c_int64),
                                          self.n_seqs, ctypes.byref(h)))
        self.h = h
        return self

    def repack(self):
        check(lib().ms_seqset_repack(self.h))

    def _host_offsets(self):
        """int64 [n_seqs + 1]: the set's offsets on the host (a set cut from a genome keeps only its region lengths)."""
        if self.offsets is not None:
            return self.offsets
        lens = getattr(self, "_region_lengths", None)
        if lens is None:
            raise ValueError("the offsets of this set are not known on the host")
        off = np.zeros(lens.size + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        return off

    def packed_host(self):
        """(codes uint32 [2 x units], nmask uint32 [units]) copied back from the device (ms_seqset_packed_host), in host_pack's layout."""
        units = (self.n_bases + 31) // 32
        codes, nmask = np.zeros(2 * units, dtype=np.uint32), np.zeros(units, dtype=np.uint32)
        check(lib().ms_seqset_packed_host(self.h, ptr(codes, ctypes.c_uint32), ptr(nmask, ctypes.c_uint32)))
        return codes, nmask

    def to_strings(self):
        """The sequences as a list of str, from the planes on the device: codes become ACGT, every non-ACGT base N (case and IUPAC
        letters do not survive packing)."""
        codes, nmask = self.packed_host()
        n = self.n_bases
        two = ((codes[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).astype(np.uint8).reshape(-1)[:n]
        isn = np.unpackbits(nmask.view(np.uint8), bitorder="little")[:n].astype(bool)
        text = np.where(isn, np.uint8(ord("N")), np.frombuffer(b"ACGT", dtype=np.uint8)[two]).tobytes().decode("ascii")
        off = self._host_offsets().tolist()
        return [text[off[k]:off[k + 1]] for k in range(self.n_seqs)]

    def shuffled(self, kind, seed, seq_index_base=0):
        """A new SeqSet with the same offsets whose sequences are this set's, shuffled on the device (ms_seqset_shuffle): kind "mono" (1)
        keeps the base composition, "dinuc" (2) every dinucleotide count and both end bases, of every run of ACGT; non-ACGT positions
        stay.  Sequence k is shuffled as sequence seq_index_base + k, so a shard gets the bytes the whole set would.  The result equals
        shuffle.shuffle_host(...) byte for byte."""
        return seqset_shuffled(self, kind, seed, seq_index_base)

    def kmer_counts(self, k, canonical=False, sel=None, nseq=True, out=None, timing=None):
        """The k-mer spectrum of the set's sequences (ms_seqset_kmer_counts) as a kmers.KmerCounts: occ[c] the windows of code c, nseq[c]
        the sequences that hold it at least once (nseq=False: not made), and the four totals.  A window with a non-ACGT base is left
        out; canonical counts a window under min(code, code of its reverse complement).  sel: one flag per sequence, or None for all.
        out: (occ, nseq) -- each an int64 numpy array [4^k], the device pointer of a torch tensor as an int (it is returned in the
        array's place), or None (a new array).  timing: a dict that receives 'device_ms'.  Equals kmers.kmer_counts_host exactly."""
        return _kmer_counts(lib().ms_seqset_kmer_counts, self.h, self.n_seqs, k, canonical, sel, nseq, out, timing)

    def close(self):
        if getattr(self, "h", None):
            lib().ms_seqset_free(self.h)
            self.h = None

    __del__ = close


def seqset_shuffled(seqs, kind, seed, seq_index_base=0):
    """ms_seqset_shuffle of a SeqSet, or of a ResidentGenome (its chromosomes are the sequences): a new SeqSet on the same device."""
    from .shuffle import KINDS
    sq = SeqSet.__new__(SeqSet)
    h = ctypes.c_void_p()
    check(lib().ms_seqset_shuffle(seqs.h, int(KINDS.get(kind, kind)), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), int(seq_index_base), 0, ctypes.byref(h)))
    sq.h = h
    sq.offsets = seqs._host_offsets() if isinstance(seqs, SeqSet) else np.ascontiguousarray(seqs.offsets, dtype=np.int64)
    sq.n_seqs = sq.offsets.size - 1
    sq.n_bases = int(sq.offsets[-1])
    return sq


MS_KMER_MAX_K, MS_KMER_CANONICAL = 12, 1


def _kmer_counts(fn, handle, n_seqs, k, canonical, sel, nseq, out, timing):
    """The call behind SeqSet.kmer_counts and ResidentGenome.kmer_counts.  The library checks k, the flags and the handle."""
    from .kmers import KmerCounts
    k = int(k)
    n_codes = 4 ** k if 1 <= k <= MS_KMER_MAX_K else 1          # (an invalid k: the library refuses it before it writes)
    if sel is not None:
        sel = np.ascontiguousarray(sel)
        if sel.shape != (n_seqs,):
            raise ValueError(f"sel must hold one flag per sequence ({n_seqs}), got shape {sel.shape}")
        sel = np.ascontiguousarray(sel != 0, dtype=np.uint8)
    given = (None, None) if out is None else tuple(out)
    if len(given) != 2:
        raise ValueError("out must be (occ, nseq)")
    dst, kept = [], []
    for a, want in zip(given, (True, bool(nseq))):
        if not want:
            dst.append(None)
            kept.append(None)
            continue
        if isinstance(a, int):
            dst.append(a)
            kept.append(a)
            continue
        if a is None:
            a = np.zeros(n_codes, dtype=np.int64)
        if a.dtype != np.int64 or a.shape != (n_codes,) or not a.flags.c_contiguous:
            raise ValueError("an output must be a C-contiguous int64 array of 4^k entries")
        dst.append(a.ctypes.data)
        kept.append(a)
    totals = np.zeros(4, dtype=np.int64)
    ms = ctypes.c_double()
    check(fn(handle, k, MS_KMER_CANONICAL if canonical else 0, None if sel is None else ptr(sel, ctypes.c_uint8), ctypes.c_void_p(dst[0]),
             ctypes.c_void_p(dst[1]), ptr(totals, ctypes.c_int64), ctypes.byref(ms)))
    if timing is not None:
        timing["device_ms"] = ms.value
    return KmerCounts(k, bool(canonical), kept[0], kept[1], *totals.tolist())


def kmer_dims():
    """ms_debug_kmer_dims: dict(threads, tile_bases, lds_k, sort_windows, sort_seqs_per_block, bitmap_budget_mib) -- the sizes at which
    the k-mer counts change path.  Constants of the build; no device."""
    out = np.zeros(8, dtype=np.int32)
    check(lib().ms_debug_kmer_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("threads", "tile_bases", "lds_k", "sort_windows", "sort_seqs_per_block", "bitmap_budget_mib"), out.tolist()))


def counts_dims():
    """ms_debug_counts_dims: dict(bins, threads, keys_per_block, max_blocks, gate_ratio, sweep_threads, sweep_max_motifs) -- the sizes at
    which the counts-only scan and sweep change path.  Constants of the build; no device."""
    out = np.zeros(8, dtype=np.int32)
    check(lib().ms_debug_counts_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("bins", "threads", "keys_per_block", "max_blocks", "gate_ratio", "sweep_threads", "sweep_max_motifs"), out.tolist()))


def kmer_bitmap_budget(nbytes):
    """ms_debug_kmer_bitmap_budget: the bytes of bitmaps a k-mer count holds at once for the calls that follow (0 = the library's own);
    returns the value before."""
    prev = ctypes.c_int64()
    check(lib().ms_debug_kmer_bitmap_budget(int(nbytes), ctypes.byref(prev)))
    return prev.value


def seqset_upload_only(seqs):
    """ms_debug_seqset_upload_only: a SeqSet of these strings as a batch stream's upload stage leaves it, its planes not packed yet (tests
    of the entry points that refuse such a set)."""
    raw = "".join(seqs).encode("latin-1")
    sq = SeqSet.__new__(SeqSet)
    sq.offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        np.cumsum([len(s) for s in seqs], out=sq.offsets[1:])
    sq.n_seqs, sq.n_bases = len(seqs), len(raw)
    h = ctypes.c_void_p()
    check(lib().ms_debug_seqset_upload_only(raw, ptr(sq.offsets, ctypes.c_int64), sq.n_seqs, ctypes.byref(h)))
    sq.h = h
    return sq


def shuffle_dims():
    """ms_debug_shuffle_dims: the run lengths at which ms_seqset_shuffle changes path, as a dict."""
    out = np.zeros(4, dtype=np.int32)
    check(lib().ms_debug_shuffle_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("lane_run", "lds_run", "block_bases", "reserved"), out.tolist()))


def shuffle_stage_ms():
    """ms_debug_shuffle_stage_ms: [run count, run list, shuffle kernels, region hints] of the last shuffle on this device, in ms."""
    out = np.zeros(4, dtype=np.float64)
    check(lib().ms_debug_shuffle_stage_ms(ptr(out, ctypes.c_double)))
    return out


class Track:
    """A resident signal track (ms_track): one int32 per base of a sequence set, laid out by the same offsets -- what
    ScanResult.site_signal sums over the sites of a scan."""

    def __init__(self, values, offsets):
        """values: an int32 numpy array of offsets[-1] entries, or the device pointer of one (an int, e.g. a torch int32 tensor's
        data_ptr() on the current device); offsets: n_seqs + 1 entries on the host."""
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if self.offsets.ndim != 1 or self.offsets.size < 1:
            raise ValueError("offsets must have n_seqs + 1 entries")
        if isinstance(values, int):
            src = values
        else:
            values = np.ascontiguousarray(values)
            if values.dtype != np.int32 or values.ndim != 1:
                raise ValueError("values must be a flat int32 array (footprint.Track.from_float turns floats into fixed point)")
            if values.size != int(self.offsets[-1]):
                raise ValueError("offsets[-1] must equal the number of values")
            src = values.ctypes.data
        h = ctypes.c_void_p()
        check(lib().ms_track_create(ctypes.c_void_p(src), ptr(self.offsets, ctypes.c_int64), self.offsets.size - 1, ctypes.byref(h)))
        self.h = h
        n_seqs, n_values = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().ms_track_size(self.h, ctypes.byref(n_seqs), ctypes.byref(n_values)))
        self.n_seqs, self.n_values = n_seqs.value, n_values.value

    @classmethod
    def from_values(cls, values, offsets):
        return cls(values, offsets)

    def values(self, first=0, n=None):
        """The values [first, first + n) read back from the device (ms_track_values_host)."""
        n = self.n_values - int(first) if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=np.int32)
        check(lib().ms_track_values_host(self.h, int(first), n, ptr(out, ctypes.c_int32)))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().ms_track_free(self.h)
            self.h = None

    __del__ = close


class ResidentGenome:
    """A genome packed once into HBM; regions are cut out on the device (no per-region host fetch).

    Quacks like the part of `motifscan.genome.Genome` the Scanner reads: `chrom_sizes` and
    `fetch_sequence(chrom, start, end)` (served from a host copy only if keep_host=True)."""

    def __init__(self, chroms, keep_host=False):
        """chroms: dict name -> str/bytes/uint8 array (insertion order = chromosome index)."""
        self.names = list(chroms.keys())
        self.index = {n: i for i, n in enumerate(self.names)}
        raws = [v.encode() if isinstance(v, str) else (v.tobytes() if isinstance(v, np.ndarray) else bytes(v))
                for v in chroms.values()]
        self.chrom_sizes = {n: len(r) for n, r in zip(self.names, raws)}
        self.offsets = np.zeros(len(raws) + 1, dtype=np.int64)
        if raws:
            self.offsets[1:] = np.cumsum([len(r) for r in raws])
        self._host = dict(zip(self.names, raws)) if keep_host else None
        h = ctypes.c_void_p()
        check(lib().ms_genome_create(b"".join(raws), ptr(self.offsets, ctypes.c_int64), len(raws), ctypes.byref(h)))
        self.h = h

    # ---- FASTA -> packed genome file -> resident genome (motifscan_amd/genome.py has the file format) ----
    @classmethod
    def from_packed(cls, packed):
        """The planes of a genome.PackedGenome (arrays or a memory-mapped genome file) uploaded as they are: 0.375 B per base over the
        link, no ASCII, no pack kernel (ms_genome_create_packed).  fetch_sequence is served by the packed host side."""
        g = cls.__new__(cls)
        g.names = list(packed.names)
        g.index = dict(packed.index)
        g.chrom_sizes = dict(packed.chrom_sizes)
        g.offsets = np.ascontiguousarray(packed.offsets, dtype=np.int64)
        g._host = None
        g._packed = packed
        codes = np.ascontiguousarray(packed.codes, dtype=np.uint32)          # (a memory map: read sequentially here, once)
        nmask = np.ascontiguousarray(packed.nmask, dtype=np.uint32)
        h = ctypes.c_void_p()
        check(lib().ms_genome_create_packed(ptr(codes, ctypes.c_uint32), ptr(nmask, ctypes.c_uint32), ptr(g.offsets, ctypes.c_int64),
                                            len(g.names), ctypes.byref(h)))
        g.h = h
        return g

    @classmethod
    def from_fasta(cls, path, n_threads=None):
        """Read a FASTA (plain reader, optional .fai check), pack it on host threads, upload the planes.  To pay the read + pack once
        per genome instead of once per process: ResidentGenome.from_fasta(fa).save(path) -- then ResidentGenome.load(path)."""
        from . import genome as _genome
        return cls.from_packed(_genome.PackedGenome.from_fasta(path, n_threads=n_threads))

    @classmethod
    def load(cls, path, verify=True):
        from . import genome as _genome
        return cls.from_packed(_genome.PackedGenome.load(path, verify=verify))

    def packed(self):
        """The genome as a genome.PackedGenome: the one it was made from, or -- for a genome packed on the device from strings -- its planes
        copied back (ms_genome_packed_host; case and IUPAC letters come from the host copy if one was kept, else they are lost: N / upper case)."""
        if getattr(self, "_packed", None) is not None:
            return self._packed
        from . import genome as _genome
        if self._host is not None:
            return _genome.PackedGenome.from_arrays(self.names, [self._host[n] for n in self.names])
        n = int(self.offsets[-1])
        units = (n + 31) // 32
        codes, nmask = np.zeros(2 * units, dtype=np.uint32), np.zeros(units, dtype=np.uint32)
        check(lib().ms_genome_packed_host(self.h, ptr(codes, ctypes.c_uint32), ptr(nmask, ctypes.c_uint32)))
        return _genome.PackedGenome(self.names, self.offsets, codes, nmask)

    def save(self, path):
        return self.packed().save(path)

    @property
    def chroms(self):
        return sorted(self.names)                        # genome/__init__.py:88-99

    def fetch_sequence(self, chrom, start, end):
        if self._host is not None:
            return self._host[chrom][start:end].decode()
        if getattr(self, "_packed", None) is not None:
            return self._packed.fetch_sequence(chrom, start, end)
        if getattr(self, "_device_made", False):         # made on the device (apply_alleles): the planes are copied back once, ms_genome_packed_host
            self._packed = self.packed()
            return self._packed.fetch_sequence(chrom, start, end)
        raise RuntimeError("ResidentGenome was created without keep_host: sequences live on the device only")

    def extract(self, chrom_idx, starts, ends):
        """SeqSet of the regions (chromosome indices, 0-based half-open, already clipped)."""
        ci = np.ascontiguousarray(chrom_idx, dtype=np.int32)
        st = np.ascontiguousarray(starts, dtype=np.int64)
        en = np.ascontiguousarray(ends, dtype=np.int64)
        if not (len(ci) == len(st) == len(en)):
            raise ValueError("chrom / start / end must have the same length")
        sq = SeqSet.__new__(SeqSet)
        h = ctypes.c_void_p()
        check(lib().ms_seqset_from_genome(self.h, ptr(ci, ctypes.c_int32), ptr(st, ctypes.c_int64), ptr(en, ctypes.c_int64),
                                          len(ci), ctypes.byref(h)))
        sq.h = h
        sq.n_seqs = len(ci)
        sq.offsets = None                         # lives on the device; not needed on the host
        sq._region_lengths = en - st              # (what to_strings / shuffled rebuild the offsets from, if ever asked)
        nb = ctypes.c_int64()
        check(lib().ms_seqset_size(sq.h, None, ctypes.byref(nb)))
        sq.n_bases = nb.value
        return sq

    # ---- the genome-wide jobs of motif --build / genome --install (genome/__init__.py:137-220; motifscan_amd/genome.py) ----
    def base_counts(self):
        """[n_chroms, 4] int64: A, C, G, T of every chromosome (file order), either case; N / IUPAC bytes count for nothing."""
        out = np.zeros((len(self.names), 4), dtype=np.int64)
        check(lib().ms_genome_base_counts(self.h, ptr(out, ctypes.c_int64)))
        return out

    def kmer_counts(self, k, canonical=False, sel=None, nseq=True, out=None, timing=None):
        """SeqSet.kmer_counts over the genome, whose sequences are its chromosomes in file order (ms_genome_kmer_counts): k = 1 without
        canonical is base_counts().sum(0); nseq counts chromosomes; sel: one flag per chromosome."""
        return _kmer_counts(lib().ms_genome_kmer_counts, self.h, len(self.names), k, canonical, sel, nseq, out, timing)

    def _exceptions(self):
        """The ascending genome positions of the non-ACGT bytes that are not N / n: the device planes mark them as N, the reference's
        sampler does not count them, and only the host side knows where they are."""
        if getattr(self, "_packed", None) is not None:
            return self._packed.exc_pos
        if self._host is not None:
            if getattr(self, "_host_exc", None) is None:
                self._host_exc = self.packed().exc_pos
            return self._host_exc
        raise RuntimeError("ResidentGenome was created without keep_host: the positions of its IUPAC letters (which Genome.random_sequences "
                           "does not count as N) live only on the host, so windows cannot be sampled as the reference samples them")

    def random_windows(self, n_times, length, max_n=0, random_seed=None, max_attempts=None):
        """Genome.random_sequences' draws (genome/__init__.py:137-176) as (chrom_idx, start) arrays, chromosome indices in file order;
        numpy's global RandomState ends where the reference leaves it.  See motifscan_amd.genome.sample_windows."""
        from . import genome as _genome
        return _genome.sample_windows(self, self._exceptions(), n_times, length, max_n, random_seed, max_attempts)

    def random_sequences(self, n_times, length, max_n=0, random_seed=None):
        """Genome.random_sequences: the same strings under the same seed, case and IUPAC letters included."""
        ci, st = self.random_windows(n_times, length, max_n, random_seed)
        for c, s in zip(ci.tolist(), st.tolist()):
            yield self.fetch_sequence(self.names[c], s, s + length)

    def close(self):
        if getattr(self, "h", None):
            lib().ms_genome_free(self.h)
            self.h = None

    __del__ = close


def window_filter(genome, gstart, length, max_n, exc_pos, n_want):
    """Candidate indices of the first n_want windows [gstart[k], gstart[k] + length) of a ResidentGenome with at most max_n N / n bytes,
    in candidate order (ms_genome_window_filter)."""
    gstart = np.ascontiguousarray(gstart, dtype=np.int64)
    exc = np.ascontiguousarray(exc_pos, dtype=np.int64)
    n_want = int(n_want)
    taken = np.zeros(max(1, min(n_want, gstart.size)), dtype=np.int64)
    nt = ctypes.c_int64()
    check(lib().ms_genome_window_filter(genome.h, ptr(gstart, ctypes.c_int64), gstart.size, int(length), int(min(max_n, length)),
                                        ptr(exc, ctypes.c_int64), exc.size, n_want, ptr(taken, ctypes.c_int64), ctypes.byref(nt)))
    return taken[:nt.value]


def randint_replay(words, high):
    """ms_randint_replay_host: (start, words_used, n_done) of len(high) sequential legacy randint(high[k]) calls replayed from raw words."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    high = np.ascontiguousarray(high, dtype=np.int64)
    start, used = np.zeros(high.size, dtype=np.int64), np.zeros(high.size, dtype=np.int64)
    done = ctypes.c_int64()
    check(lib().ms_randint_replay_host(ptr(words, ctypes.c_uint32), words.size, ptr(high, ctypes.c_int64), high.size,
                                       ptr(start, ctypes.c_int64), ptr(used, ctypes.c_int64), ctypes.byref(done)))
    return start, used, done.value


class GeneTable:
    """ms_genes: a gene table (chromosome offsets, tss, strand 1 '+' / 2 '-', file order per chromosome).  Made on the host; the device
    copy is made by the first nearest_tss / promoter_overlap call (which need a device, as every compute entry does)."""

    def __init__(self, chrom_offsets, tss, strand):
        self.chrom_offsets = np.ascontiguousarray(chrom_offsets, dtype=np.int64)
        self.tss = np.ascontiguousarray(tss, dtype=np.int64)
        self.strand = np.ascontiguousarray(strand, dtype=np.int8)
        if self.chrom_offsets.ndim != 1 or self.chrom_offsets.size < 1 or not (self.tss.size == self.strand.size == int(self.chrom_offsets[-1])):
            raise ValueError("need chrom_offsets[n_chroms + 1] and chrom_offsets[-1] genes in tss and strand")
        h = ctypes.c_void_p()
        check(lib().ms_genes_create(ptr(self.chrom_offsets, ctypes.c_int64), self.chrom_offsets.size - 1, ptr(self.tss, ctypes.c_int64),
                                    ptr(self.strand, ctypes.c_int8), ctypes.byref(h)))
        self.h = h

    def nearest_tss(self, chrom_idx, start, cutoff=10000):
        """(distance int64, found bool) of dis_to_nearest_gene for every region (ms_genes_nearest_tss)."""
        ci = np.ascontiguousarray(chrom_idx, dtype=np.int32)
        st = np.ascontiguousarray(start, dtype=np.int64)
        if ci.shape != st.shape or ci.ndim != 1:
            raise ValueError("chrom_idx and start must have one entry per region")
        dist, found = np.zeros(ci.size, dtype=np.int64), np.zeros(ci.size, dtype=np.uint8)
        check(lib().ms_genes_nearest_tss(self.h, ptr(ci, ctypes.c_int32), ptr(st, ctypes.c_int64), ci.size, int(cutoff),
                                         ptr(dist, ctypes.c_int64), ptr(found, ctypes.c_uint8)))
        return dist, found.astype(bool)

    def promoter_overlap(self, chrom_idx, start, end, upstream=2000, downstream=2000):
        """bool per region: subset_by_location's overlap with the chromosome's promoters (ms_genes_promoter_overlap)."""
        ci = np.ascontiguousarray(chrom_idx, dtype=np.int32)
        st = np.ascontiguousarray(start, dtype=np.int64)
        en = np.ascontiguousarray(end, dtype=np.int64)
        if not (ci.shape == st.shape == en.shape) or ci.ndim != 1:
            raise ValueError("chrom_idx, start and end must have one entry per region")
        out = np.zeros(ci.size, dtype=np.uint8)
        check(lib().ms_genes_promoter_overlap(self.h, int(upstream), int(downstream), ptr(ci, ctypes.c_int32), ptr(st, ctypes.c_int64),
                                              ptr(en, ctypes.c_int64), ci.size, ptr(out, ctypes.c_uint8)))
        return out.astype(bool)

    def close(self):
        if getattr(self, "h", None):
            lib().ms_genes_free(self.h)
            self.h = None

    __del__ = close


def control_regions_replay(words, chrom_size, length, n_random, max_attempts=1, gene_lo=None, gene_hi=None, distance=None, found=None,
                           tss=None, strand=None):
    """ms_control_regions_replay_host over the regions given: (start [n, n_random], words_used [n], attempts [n], n_done, stop,
    stop_words).  tss=None is the no-annotation path.  No device."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    chrom_size = np.ascontiguousarray(chrom_size, dtype=np.int64)
    length = np.ascontiguousarray(length, dtype=np.int64)
    n, n_random = chrom_size.size, int(n_random)
    if length.size != n:
        raise ValueError("need one chromosome size and one length per region")
    args = [None] * 6
    if tss is not None:
        args = [np.ascontiguousarray(gene_lo, dtype=np.int64), np.ascontiguousarray(gene_hi, dtype=np.int64),
                np.ascontiguousarray(distance, dtype=np.int64), np.ascontiguousarray(found, dtype=np.uint8),
                np.ascontiguousarray(tss, dtype=np.int64), np.ascontiguousarray(strand, dtype=np.int8)]
        if any(a.size != n for a in args[:4]) or args[4].size != args[5].size:
            raise ValueError("need one gene range, distance and found flag per region, and one strand per tss")
        if n and (args[0].min() < 0 or args[1].max() > args[4].size):
            raise ValueError("gene range outside the gene table")
    start = np.zeros((n, max(n_random, 0)), dtype=np.int64)
    used, attempts = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    done, stop, stop_words = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
    cts = (ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint8, ctypes.c_int64, ctypes.c_int8)
    check(lib().ms_control_regions_replay_host(ptr(words, ctypes.c_uint32), words.size, n, ptr(chrom_size, ctypes.c_int64),
                                               ptr(length, ctypes.c_int64), *[None if a is None else ptr(a, ct) for a, ct in zip(args, cts)],
                                               n_random, int(max_attempts), ptr(start, ctypes.c_int64), ptr(used, ctypes.c_int64),
                                               ptr(attempts, ctypes.c_int64), ctypes.byref(done), ctypes.byref(stop), ctypes.byref(stop_words)))
    return start, used, attempts, done.value, stop.value, stop_words.value


def _owned_array(address, ctype, n, dtype, owner):
    """A numpy array over n items of library-owned memory at `address` that keeps `owner` (the ScanResult / pinned block that
    frees the memory) alive for as long as ANY array derived from it lives.  numpy collapses `.base` to the object that owns
    the memory -- np.asarray(view), slices, reshapes all end up referencing the ctypes array below, not an ndarray subclass in
    between -- so the owner hangs on that object (an owner kept on an ndarray subclass was lost by np.asarray)."""
    raw = (ctype * max(int(n), 1)).from_address(int(address))
    raw._owner = owner
    return np.frombuffer(raw, dtype=dtype, count=int(n))


class ScanResult:
    """Hits of one ms_scan call, in the reference's order (cscore.c:336-390, 443-471)."""

    def __init__(self, handle, n_pwms):
        self.h = handle
        self.n_pwms = n_pwms
        n = ctypes.c_int64()
        check(lib().ms_result_num_hits(self.h, ctypes.byref(n)))
        self.n_hits = n.value
        self.motif_offsets = np.zeros(n_pwms + 1, dtype=np.int64)
        check(lib().ms_result_motif_offsets(self.h, ptr(self.motif_offsets, ctypes.c_int64)))
        self._hits = None
        self._hits_owned = True

    def hits(self, copy=True, packed=False, motif=True):
        """dict of numpy arrays: seq_idx, pos, score, strand (1 '+', 2 '-'), motif (motif=False leaves the per-hit motif
        index out: it is motif_offsets expanded, 4 bytes per hit that few callers read).
        copy=False returns views of the library's pinned host buffer; the views keep this result alive.  The result has ONE such
        buffer, which holds one form at a time: the views are invalidated by an explicit close() or dedup() and ALSO by a request
        for another form -- hits(packed=...) or packed_words(), even one that is refused -- which overwrites it; fetch them again
        after such a call.  Arrays of copy=True are the caller's own and never change.  packed=True moves 16 instead of 25 bytes
        per hit over the host link (ms_result_hits_packed_host) and unpacks on the host -- the arrays are then always fresh copies."""
        if packed:
            return self._hits_packed(None if packed is True else int(packed))
        if self._hits is None or (copy and not self._hits_owned):
            n = self.n_hits
            ps, pp = ctypes.POINTER(ctypes.c_int64)(), ctypes.POINTER(ctypes.c_int64)()
            pv, pd_ = ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int8)()
            check(lib().ms_result_hits_host(self.h, ctypes.byref(ps), ctypes.byref(pp), ctypes.byref(pv), ctypes.byref(pd_)))
            if n:
                spec = ((ps, ctypes.c_int64, np.int64), (pp, ctypes.c_int64, np.int64), (pv, ctypes.c_double, np.float64), (pd_, ctypes.c_int8, np.int8))
                arrs = [_owned_array(ctypes.cast(q, ctypes.c_void_p).value, ct, n, dt, self) for q, ct, dt in spec]
                if copy:
                    arrs = [a.copy() for a in arrs]
            else:
                arrs = [np.zeros(0, dtype=t) for t in (np.int64, np.int64, np.float64, np.int8)]
            self._hits = {"seq_idx": arrs[0], "pos": arrs[1], "score": arrs[2], "strand": arrs[3],
                          "motif_offsets": self.motif_offsets}
            self._hits_owned = copy or n == 0
        out = self._hits
        if motif and "motif" not in out:
            out["motif"] = np.repeat(np.arange(self.n_pwms, dtype=np.int32), np.diff(self.motif_offsets))
        if not self._hits_owned:
            self._hits = None                            # the views reference this object: caching them here would be a cycle
        return out

    def packed_form(self):
        """12, 16 or 0: the compact form a batch stream's copy-out left in this result (ms_result_packed_form)."""
        b = ctypes.c_int32()
        check(lib().ms_result_packed_form(self.h, ctypes.byref(b)))
        return b.value

    def hits_pageable(self):
        """The four hit arrays through ms_result_hits: four device copies into buffers of the caller's (here fresh numpy arrays),
        no pinned buffer involved."""
        n = self.n_hits
        seq_idx, pos, score_, strand = (np.zeros(n, dtype=t) for t in (np.int64, np.int64, np.float64, np.int8))
        check(lib().ms_result_hits(self.h, ptr(seq_idx, ctypes.c_int64), ptr(pos, ctypes.c_int64), ptr(score_, ctypes.c_double), ptr(strand, ctypes.c_int8)))
        return {"seq_idx": seq_idx, "pos": pos, "score": score_, "strand": strand, "motif_offsets": self.motif_offsets}

    def packed_words(self, form, copy=True):
        """The compact form as the library hands it over: (coord uint64 [n] for form 16 / uint32 [n] for form 12, score float64 [n],
        shift -- 0 for form 16).  copy=False: views of the pinned buffer, valid until the next request for any form, close() or
        dedup().  ValueError if a hit does not fit the form; the result stays usable."""
        n = self.n_hits
        sh = ctypes.c_int32(0)
        pv = ctypes.POINTER(ctypes.c_double)()
        if int(form) == 12:
            pc = ctypes.POINTER(ctypes.c_uint32)()
            check(lib().ms_result_hits_packed12_host(self.h, ctypes.byref(pc), ctypes.byref(pv), ctypes.byref(sh)))
        elif int(form) == 16:
            pc = ctypes.POINTER(ctypes.c_uint64)()
            check(lib().ms_result_hits_packed_host(self.h, ctypes.byref(pc), ctypes.byref(pv)))
        else:
            raise ValueError("form must be 12 or 16")
        if n == 0:
            return np.zeros(0, dtype=np.uint32 if int(form) == 12 else np.uint64), np.zeros(0, dtype=np.float64), sh.value
        coord, score_ = np.ctypeslib.as_array(pc, shape=(n,)), np.ctypeslib.as_array(pv, shape=(n,))
        return (coord.copy(), score_.copy(), sh.value) if copy else (coord, score_, sh.value)

    def _hits_packed(self, form=None):
        """form: None = whatever the result holds already (a stream's copy-out), else 12 / 16."""
        if form is None:
            form = self.packed_form() or 16
        form = 12 if form == 12 else 16
        coord, score_, shift = self.packed_words(form, copy=False)
        score_ = score_.copy()
        word = coord.dtype.type
        low = word(shift if form == 12 else 32)
        seq_idx = (coord >> low).astype(np.int64)
        pos = ((coord & word((1 << int(low)) - 1)) >> word(1)).astype(np.int64)
        strand = ((coord & word(1)) + word(1)).astype(np.int8)
        motif = np.repeat(np.arange(self.n_pwms, dtype=np.int32), np.diff(self.motif_offsets))
        return {"seq_idx": seq_idx, "pos": pos, "score": score_, "strand": strand, "motif": motif,
                "motif_offsets": self.motif_offsets}

    def dedup(self, pwms):
        """Device-side de-duplication in place (scanner.py:156-193)."""
        check(lib().ms_result_dedup(self.h, pwms.h))
        n = ctypes.c_int64()
        check(lib().ms_result_num_hits(self.h, ctypes.byref(n)))
        self.n_hits = n.value
        check(lib().ms_result_motif_offsets(self.h, ptr(self.motif_offsets, ctypes.c_int64)))
        self._hits = None
        return self

    def site_tables(self, n_seqs):
        """(n_sites int32 [P][R], max_score float64 [P][R], NaN = no site)."""
        n_sites = np.zeros((self.n_pwms, n_seqs), dtype=np.int32)
        max_score = np.full((self.n_pwms, n_seqs), np.nan, dtype=np.float64)
        check(lib().ms_result_site_tables(self.h, ptr(n_sites, ctypes.c_int32), ptr(max_score, ctypes.c_double)))
        return n_sites, max_score

    def region_counts(self):
        out = np.zeros(self.n_pwms, dtype=np.int64)
        check(lib().ms_result_region_counts(self.h, ptr(out, ctypes.c_int64)))
        return out

    def region_counts_device_ptr(self):
        p = ctypes.c_void_p()
        check(lib().ms_result_region_counts_device(self.h, ctypes.byref(p)))
        return p.value

    def stats(self):
        s = ScanStats()
        check(lib().ms_result_stats(self.h, ctypes.byref(s)))
        return s.as_dict()

    def site_histogram(self, pwms, summit_rel, extend, m0=0, m1=None):
        """plot.py:60-70 on the device (ms_result_site_histogram): (counts int64 [m1 - m0][n_bins], n_sites int64 [m1 - m0]) of the
        distance site centre - summit in the bins of np.arange(-extend - 5, extend + 6, 10).  summit_rel [R]: summit - sequence start."""
        m1 = self.n_pwms if m1 is None else int(m1)
        m0, extend = int(m0), int(extend)
        summit_rel = np.ascontiguousarray(summit_rel, dtype=np.int64)
        n_bins = len(np.arange(-extend - 5, extend + 6, 10)) - 1 if extend >= 0 else 0
        counts = np.zeros((max(m1 - m0, 0), max(n_bins, 0)), dtype=np.int64)
        n_sites = np.zeros(max(m1 - m0, 0), dtype=np.int64)
        check(lib().ms_result_site_histogram(self.h, pwms.h, ptr(summit_rel, ctypes.c_int64), extend, m0, m1,
                                             ptr(counts, ctypes.c_int64), ptr(n_sites, ctypes.c_int64)))
        return counts, n_sites

    def rank_profile(self, rank_order, ratio_control, kernel=None, m0=0, m1=None, smoothed=True, out=None):
        """plot.py:120-142 on the device (ms_result_rank_profile): the fold-change profile [m1 - m0][R] over the ranks of rank_order,
        smoothed with the 11 `kernel` weights unless smoothed=False.  ratio_control [m1 - m0], each > 0.  out: a float64 numpy array
        of that shape, or None (a new one); the device pointer of a torch tensor may be passed as an int instead (then it is returned)."""
        m1 = self.n_pwms if m1 is None else int(m1)
        m0 = int(m0)
        rank_order = np.ascontiguousarray(rank_order, dtype=np.int64)
        ratio_control = np.ascontiguousarray(ratio_control, dtype=np.float64)
        if ratio_control.shape != (max(m1 - m0, 0),):
            raise ValueError("need one ratio_control per motif of [m0, m1)")
        k = None if kernel is None else np.ascontiguousarray(kernel, dtype=np.float64)
        if smoothed and (k is None or k.shape != (11,)):
            raise ValueError("smoothing needs 11 kernel weights")
        if isinstance(out, int):
            dst = out
        else:
            if out is None:
                out = np.empty((max(m1 - m0, 0), len(rank_order)), dtype=np.float64)
            if out.dtype != np.float64 or out.shape != (max(m1 - m0, 0), len(rank_order)) or not out.flags.c_contiguous:
                raise ValueError("out must be a C-contiguous float64 array of shape (m1 - m0, R)")
            dst = out.ctypes.data
        check(lib().ms_result_rank_profile(self.h, ptr(rank_order, ctypes.c_int64), ptr(ratio_control, ctypes.c_double),
                                           None if k is None else ptr(k, ctypes.c_double), m0, m1,
                                           0 if smoothed else MS_PROFILE_UNSMOOTHED, ctypes.c_void_p(dst)))
        return out

    def cooccurrence(self, m0=0, m1=None, out=None):
        """ms_result_cooccurrence: int64 [m1 - m0][P], the regions that hold a site of motif m0 + a and a site of motif j.  out: an int64
        numpy array of that shape, or None (a new one); the device pointer of a torch tensor may be passed as an int instead (then it is
        returned)."""
        m1 = self.n_pwms if m1 is None else int(m1)
        m0 = int(m0)
        shape = (max(m1 - m0, 0), self.n_pwms)
        if isinstance(out, int):
            dst = out
        else:
            if out is None:
                out = np.zeros(shape, dtype=np.int64)
            if out.dtype != np.int64 or out.shape != shape or not out.flags.c_contiguous:
                raise ValueError("out must be a C-contiguous int64 array of shape (m1 - m0, P)")
            dst = out.ctypes.data
        check(lib().ms_result_cooccurrence(self.h, m0, m1, ctypes.c_void_p(dst)))
        return out

    def pair_spacing(self, pwms, anchor, max_dist, m0=0, m1=None):
        """ms_result_pair_spacing: (counts int64 [m1 - m0][4][2 * max_dist + 1], n_pairs int64 [m1 - m0]) of the anchor motif's sites against
        those of motifs m0 .. m1 - 1 in the same region: bin = centre-to-centre distance in half base pairs shifted to 0 and halved,
        orientation 2 * (anchor strand - 1) + (partner strand - 1).  The library checks every argument."""
        m1 = self.n_pwms if m1 is None else int(m1)
        m0, anchor, max_dist = int(m0), int(anchor), int(max_dist)
        rows, n_bins = max(m1 - m0, 0), 2 * max_dist + 1
        fits = 0 <= max_dist <= 1 << 20 and rows * 4 * n_bins <= 1 << 31        # what it refuses is refused before it writes
        counts = np.zeros((rows, 4, n_bins) if fits else (1, 4, 1), dtype=np.int64)
        n_pairs = np.zeros(max(rows, 1), dtype=np.int64)
        check(lib().ms_result_pair_spacing(self.h, pwms.h, anchor, m0, m1, max_dist, ptr(counts, ctypes.c_int64), ptr(n_pairs, ctypes.c_int64)))
        return counts, n_pairs[:rows]

    def site_base_counts(self, pwmset, seqset, flank=0, m0=0, m1=None, dinuc=False, out=None, flags=0):
        """ms_result_site_base_counts: (counts int64 [m1 - m0][C][6], dinuc int64 [m1 - m0][C][16] or None, n_sites int64 [m1 - m0]) of
        the sites of motifs m0 .. m1 - 1 over the sequence set the result was made of, C = the set's widest motif + 2 * flank: per
        column of the motif (column flank + c is motif column c) the sites with A, C, G, T there in the motif's orientation, with a
        non-ACGT base (slot 4) and outside the region (slot 5); dinuc[.][j][4 * a + b] the sites with a at column j and b at j + 1.
        out: None, or (counts, dinuc, n_sites), each an int64 numpy array of that shape or None (a new one; dinuc must be None unless
        asked for); the device pointer of a torch tensor may be passed as an int instead (then it is returned).  The call's
        device_ms is left in self.site_base_counts_ms.  The library checks every argument."""
        m1 = self.n_pwms if m1 is None else int(m1)
        m0, flank = int(m0), int(flank)
        rows = max(m1 - m0, 0)
        fits = 0 <= flank <= 64                                  # what the library refuses is refused before it writes
        C = (int(pwmset.widths.max()) if pwmset.n else 0) + 2 * flank if fits else 1
        shapes = ((rows, C, 6), (rows, C, 16), (rows,))
        given = (None, None, None) if out is None else tuple(out)
        if len(given) != 3 or (given[1] is not None and not dinuc):
            raise ValueError("out must be (counts, dinuc, n_sites), dinuc None unless asked for")
        arrs, dst = [], []
        for a, shape, want in zip(given, shapes, (True, bool(dinuc), True)):
            if not want:
                a, p = None, None
            elif isinstance(a, int):
                p = a
            else:
                if a is None:
                    a = np.zeros(shape, dtype=np.int64)
                if a.dtype != np.int64 or a.shape != shape or not a.flags.c_contiguous:
                    raise ValueError("out arrays must be C-contiguous int64 of shapes (m1 - m0, C, 6), (m1 - m0, C, 16) and (m1 - m0,)")
                p = a.ctypes.data
            arrs.append(a)
            dst.append(ctypes.c_void_p(p))
        ms = ctypes.c_double(0.0)
        check(lib().ms_result_site_base_counts(self.h, pwmset.h, seqset.h, flank, m0, m1, int(flags), dst[0], dst[1], dst[2], ctypes.byref(ms)))
        self.site_base_counts_ms = ms.value
        return tuple(arrs)

    def site_signal(self, pwmset, track, flank=0, m0=0, m1=None, profile=True, per_site=False, out=None, flags=0):
        """ms_result_site_signal: (sum int64 [m1 - m0][2][C], cover int64 [m1 - m0][2][C], n_sites int64 [m1 - m0][2], per_site int64
        [n_sel][3]) of the sites of motifs m0 .. m1 - 1 over a Track laid out as the sequence set the result was made of, C = the set's
        widest motif + 2 * flank: per strand ('+' 0, '-' 1) and column of the motif (column flank + c is motif column c, in the motif's
        orientation) the track summed over the sites whose column lies inside the region, and the number of those sites; per selected
        hit, in hit order, the sums over its upstream flank, core and downstream flank.  profile=False leaves sum and cover out (None),
        per_site=False the last.  out: None, or (sum, cover, n_sites, per_site), each an int64 numpy array of that shape, None (a new
        one) or the device pointer of a torch tensor as an int (then it is returned).  The call's device_ms is left in
        self.site_signal_ms.  The library checks every argument."""
        m1 = self.n_pwms if m1 is None else int(m1)
        m0, flank = int(m0), int(flank)
        rows = max(m1 - m0, 0)
        fits = 0 <= flank <= 512                                 # what the library refuses is refused before it writes
        C = (int(pwmset.widths.max()) if pwmset.n else 0) + 2 * flank if fits else 1
        in_range = 0 <= m0 <= m1 <= self.n_pwms
        n_sel = int(self.motif_offsets[m1] - self.motif_offsets[m0]) if in_range and per_site else 0
        shapes = ((rows, 2, C), (rows, 2, C), (rows, 2), (n_sel, 3))
        given = (None, None, None, None) if out is None else tuple(out)
        if len(given) != 4:
            raise ValueError("out must be (sum, cover, n_sites, per_site)")
        arrs, dst = [], []
        for a, shape, want in zip(given, shapes, (bool(profile), bool(profile), True, bool(per_site))):
            if not want:
                if a is not None:
                    raise ValueError("an output array was given for a part that was not asked for")
                p = None
            elif isinstance(a, int):
                p = a
            else:
                if a is None:
                    a = np.zeros(shape, dtype=np.int64)
                if a.dtype != np.int64 or a.shape != shape or not a.flags.c_contiguous:
                    raise ValueError("out arrays must be C-contiguous int64 of shapes (m1 - m0, 2, C), (m1 - m0, 2, C), (m1 - m0, 2) and (n_sel, 3)")
                p = a.ctypes.data
            arrs.append(a)
            dst.append(ctypes.c_void_p(p))
        ms = ctypes.c_double(0.0)
        check(lib().ms_result_site_signal(self.h, pwmset.h, track.h, flank, m0, m1, int(flags), dst[0], dst[1], dst[2], dst[3], ctypes.byref(ms)))
        self.site_signal_ms = ms.value
        return tuple(arrs)

    def close(self):
        if getattr(self, "h", None):
            lib().ms_result_free(self.h)
            self.h = None

    __del__ = close


def result_from_hits(n_pwms, n_regions, motif_offsets, seq_idx, pos, score_, strand):
    """A ScanResult made of host hit arrays in ms_result order (ms_result_from_hits), on the current device."""
    motif_offsets = np.ascontiguousarray(motif_offsets, dtype=np.int64)
    seq_idx = np.ascontiguousarray(seq_idx, dtype=np.int64)
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    score_ = np.ascontiguousarray(score_, dtype=np.float64)
    strand = np.ascontiguousarray(strand, dtype=np.int8)
    n = int(motif_offsets[-1]) if len(motif_offsets) else 0
    if len(motif_offsets) != int(n_pwms) + 1 or not len(seq_idx) == len(pos) == len(score_) == len(strand) == n:
        raise ValueError("need motif_offsets[n_pwms + 1] and motif_offsets[-1] hits in every array")
    h = ctypes.c_void_p()
    check(lib().ms_result_from_hits(int(n_pwms), int(n_regions), ptr(motif_offsets, ctypes.c_int64), ptr(seq_idx, ctypes.c_int64),
                                    ptr(pos, ctypes.c_int64), ptr(score_, ctypes.c_double), ptr(strand, ctypes.c_int8), ctypes.byref(h)))
    return ScanResult(h, int(n_pwms))


def bucket_plan(mu, n_pred, *, gbits, pbits, end_bit, low_bits, offsets=None, widths=None, weights=None, n_pwms=0, n_regions=0, cap_max=None,
                predicted=True, counts_only=False, carry_only=True, sticky_off=False, force=-1):
    """ms_debug_bucket_plan (no device): the host arithmetic of a scan's bucketed hit list.  Either a set (offsets, widths) or the 256 bucket
    weights; returns dict(weights, need, gate, base, cap)."""
    w = np.zeros(256, dtype=np.uint64)
    po = pw = None
    n_seqs = 0
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        po, pw, n_seqs, n_pwms = ptr(offsets, ctypes.c_int64), ptr(widths, ctypes.c_int32), offsets.size - 1, widths.size
    else:
        w[:] = np.asarray(weights, dtype=np.uint64)
    need, gate = ctypes.c_uint64(), ctypes.c_int32()
    base, cap = np.zeros(256, dtype=np.uint64), np.zeros(256, dtype=np.uint64)
    form = (1 if predicted else 0) | (2 if counts_only else 0) | (4 if carry_only else 0) | (8 if sticky_off else 0)
    check(lib().ms_debug_bucket_plan(po, n_seqs, pw, n_pwms, int(gbits), int(pbits), int(end_bit), int(low_bits), int(n_regions), ptr(w, ctypes.c_uint64), float(mu),
                                     int(n_pred), (1 << 64) - 1 if cap_max is None else int(cap_max), form, int(force), ctypes.byref(need),
                                     ctypes.byref(gate), ptr(base, ctypes.c_uint64), ptr(cap, ctypes.c_uint64)))
    return {"weights": w, "need": need.value, "gate": bool(gate.value), "base": base, "cap": cap}


def key_layout(n_bases, n_seqs, max_len, n_pwms, coord_global=False):
    """ms_debug_key_layout (no device): (gbits, pbits) of the hit keys of a scan over a set of these sizes; pbits > 0 = (region, position)
    coordinates, 0 = global base positions."""
    gbits, pbits = ctypes.c_int32(), ctypes.c_int32()
    check(lib().ms_debug_key_layout(int(n_bases), int(n_seqs), int(max_len), int(n_pwms), 1 if coord_global else 0, ctypes.byref(gbits),
                                    ctypes.byref(pbits)))
    return gbits.value, pbits.value


def host_pack(bases, offsets):
    """The host packer alone (ms_debug_host_pack; no device): (codes uint32 [2 x units], nmask uint32 [units], blk2reg int32 [blocks],
    blkinfo int32 [blocks][4]) of a sequence set -- the layout the device's pack / hint kernels write."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = int(offsets[-1])
    units, blocks = (n + 31) // 32, (n + 63) // 64 + 1
    codes, nmask = np.zeros(2 * units, dtype=np.uint32), np.zeros(units, dtype=np.uint32)
    blk, info = np.zeros(blocks, dtype=np.int32), np.zeros((blocks, 4), dtype=np.int32)
    check(lib().ms_debug_host_pack(bases.ctypes.data_as(ctypes.c_char_p), ptr(offsets, ctypes.c_int64), offsets.size - 1,
                                   ptr(codes, ctypes.c_uint32), ptr(nmask, ctypes.c_uint32), ptr(blk, ctypes.c_int32), ptr(info, ctypes.c_int32)))
    return codes, nmask, blk, info


def host_pool_stats():
    """The pinned-block cache (ms_host_pool_stats): dict(hits, misses, driver_frees, ms_in_driver)."""
    out = (ctypes.c_uint64 * 4)()
    check(lib().ms_host_pool_stats(out))
    return {"hits": int(out[0]), "misses": int(out[1]), "driver_frees": int(out[2]), "ms_in_driver": out[3] / 1e6}


def pool_stats():
    """HBM block cache of the calling thread's device (ms_device_pool_stats)."""
    out = (ctypes.c_uint64 * 6)()
    check(lib().ms_device_pool_stats(out))
    return {"hits": int(out[0]), "misses": int(out[1]), "driver_frees": int(out[2]), "driver_ms": out[3] / 1e6,
            "cached_bytes": int(out[4]), "cached_blocks": int(out[5])}


_warned_exact_only = set()


def pool_trim():
    """ms_debug_pool_trim: every cached block of the calling thread's device back to the driver; returns the bytes released.  The
    allocations that follow are misses.  Tests only."""
    n = ctypes.c_uint64()
    check(lib().ms_debug_pool_trim(ctypes.byref(n)))
    return n.value


def _fence_exact_only(res, pwms, flags=0):
    """motifs the pre-filter cannot take -- wider than 63 columns, max_raw <= 0, non-finite entries, a cutoff under the
    quantiser's floor -- are scored in fp64 at EVERY window (exact_tiled_kernel: correct, the reference's arithmetic, the motif's table in LDS --
    and still ~400 x the cost per motif of the matrix-core path; the reference itself has no width limit, cscore.c:50-51).  Never silent:
    one warning per PWM set with the number of such motifs (MS_SCAN_EXACT_ONLY scans -- validation -- are the caller's own choice)."""
    if (flags & MS_SCAN_EXACT_ONLY) or id(pwms) in _warned_exact_only:
        return res
    st = res.stats()
    if st["n_pwms_exact"] > 0 and st["n_pwms_exact"] * st["n_bases"] >= 10_000_000:       # (a handful of short sequences costs nothing either way)
        _warned_exact_only.add(id(pwms))
        import warnings
        warnings.warn(f"{st['n_pwms_exact']} of {st['n_pwms']} PWMs cannot take the matrix-core pre-filter (wider than 63 columns, max_raw <= 0, "
                      f"non-finite entries or a cutoff below the quantiser's floor) and are scored in fp64 at every window: same results, "
                      f"roughly 400 x the device time per such motif (fp64 stage of this scan: {st['ms_exact']:.1f} ms of {st['ms_total']:.1f} ms)", RuntimeWarning, stacklevel=3)
    return res


def scan(pwms, seqs, strand_mask=3, flags=MS_SCAN_DEFAULT):
    h = ctypes.c_void_p()
    check(lib().ms_scan(pwms.h, seqs.h, int(strand_mask), int(flags), ctypes.byref(h)))
    return _fence_exact_only(ScanResult(h, pwms.n), pwms, int(flags))


SCAN_GEOM_FIELDS = ("wide", "dense", "counter_used", "wave_passes", "blocks_per_tile", "n_tiles", "rare_cap", "cand_block", "cand_static",
                    "skip_alln", "pass_windows", "rescore_chunk")


def scan_candidates(pwms, seqs, strand_mask=3, flags=MS_SCAN_DEFAULT):
    """ms_debug_scan_candidates (tests only): the pre-filter of a scan alone.  Returns (records uint64 [n_slots], geom dict, cap): every slot
    of the candidate list the launch used (g << 30 | group << 16 | flags, 0 = empty), the launch's geometry (SCAN_GEOM_FIELDS), and the
    room the records were asked into.  The list is sized by a first call; which wave reserves how many blocks depends on the hand-out, so the
    call is repeated with more room should the second list be longer."""
    L = lib()
    n, geom = ctypes.c_uint64(0), np.zeros(16, dtype=np.int64)
    check(L.ms_debug_scan_candidates(pwms.h, seqs.h, int(strand_mask), int(flags), None, 0, ctypes.byref(n), ptr(geom, ctypes.c_int64)))
    while True:
        cap = int(n.value) + int(n.value) // 4 + 4096
        rec = np.zeros(cap, dtype=np.uint64)
        check(L.ms_debug_scan_candidates(pwms.h, seqs.h, int(strand_mask), int(flags), ptr(rec, ctypes.c_uint64), cap, ctypes.byref(n),
                                         ptr(geom, ctypes.c_int64)))
        if n.value <= cap:
            assert not geom[len(SCAN_GEOM_FIELDS):].any()
            return rec[:n.value], {k: int(v) for k, v in zip(SCAN_GEOM_FIELDS, geom)}, cap


def scan_from_candidates(pwms, seqs, records, strand_mask=3, flags=MS_SCAN_DEFAULT):
    """ms_debug_scan_from_candidates (tests only): the scan with `records` in place of the pre-filter's candidate list."""
    rec = np.ascontiguousarray(records, dtype=np.uint64)
    h = ctypes.c_void_p()
    check(lib().ms_debug_scan_from_candidates(pwms.h, seqs.h, int(strand_mask), int(flags), ptr(rec, ctypes.c_uint64), rec.size, ctypes.byref(h)))
    return ScanResult(h, pwms.n)


def scan_sweep(pwms, genome, chrom, begin, end, window, stride, strand_mask=3, flags=MS_SCAN_DEFAULT):
    """Scan the windows [begin + k*stride, begin + k*stride + window) of one chromosome of a ResidentGenome.  Same
    result as scan() over those windows as separate regions (seq_idx = k), with every base scored once."""
    ci = genome.index[chrom] if isinstance(chrom, str) else int(chrom)
    h = ctypes.c_void_p()
    check(lib().ms_scan_sweep(pwms.h, genome.h, ci, int(begin), int(end), int(window), int(stride), int(strand_mask),
                              int(flags), ctypes.byref(h)))
    return _fence_exact_only(ScanResult(h, pwms.n), pwms, int(flags))


class VariantScan:
    """Records of one ms_scan_variants call: per motif, variant index, window start, '+' before '-' (include/motifscan_amd.h)."""

    def __init__(self, handle, n_pwms, n_variants):
        self.h = handle
        self.n_pwms = n_pwms
        self.n_variants = n_variants
        n = ctypes.c_int64()
        check(lib().ms_varscan_num_sites(self.h, ctypes.byref(n)))
        self.n_sites = n.value
        self.motif_offsets = np.zeros(n_pwms + 1, dtype=np.int64)
        check(lib().ms_varscan_motif_offsets(self.h, ptr(self.motif_offsets, ctypes.c_int64)))

    def sites(self):
        """dict of fresh numpy arrays: variant, start, strand (1 '+', 2 '-'), score_ref, score_alt, state (1 lost, 2 gained, 3 kept),
        motif (motif_offsets expanded) and motif_offsets."""
        n = self.n_sites
        variant, start = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        strand, state = np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.uint8)
        score_ref, score_alt = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        check(lib().ms_varscan_sites(self.h, ptr(variant, ctypes.c_int64), ptr(start, ctypes.c_int64), ptr(strand, ctypes.c_int8),
                                     ptr(score_ref, ctypes.c_double), ptr(score_alt, ctypes.c_double), ptr(state, ctypes.c_uint8)))
        motif = np.repeat(np.arange(self.n_pwms, dtype=np.int32), np.diff(self.motif_offsets))
        return {"variant": variant, "start": start, "strand": strand, "score_ref": score_ref, "score_alt": score_alt, "state": state,
                "motif": motif, "motif_offsets": self.motif_offsets}

    def ref_codes(self):
        """int8 per input variant: the genome's base there, 0..3 = A C G T, -1 = non-ACGT."""
        out = np.zeros(self.n_variants, dtype=np.int8)
        check(lib().ms_varscan_ref_codes(self.h, ptr(out, ctypes.c_int8)))
        return out

    def motif_counts(self):
        """(gained, lost) int64 [P]: variants with at least one gained / lost site of the motif, counted on the device."""
        gained, lost = np.zeros(self.n_pwms, dtype=np.int64), np.zeros(self.n_pwms, dtype=np.int64)
        check(lib().ms_varscan_motif_counts(self.h, ptr(gained, ctypes.c_int64), ptr(lost, ctypes.c_int64)))
        return gained, lost

    def device_ms(self):
        ms = ctypes.c_double()
        check(lib().ms_varscan_device_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "h", None):
            lib().ms_varscan_free(self.h)
            self.h = None

    __del__ = close


def scan_variants(pwms, genome, chrom_idx, pos, alt, strand_mask=3, flags=0):
    """ms_scan_variants: chrom_idx / pos (0-based) / alt (bytes, a str, or a uint8 / S1 array: one byte per variant) against a
    ResidentGenome.  Returns a VariantScan."""
    ci = np.ascontiguousarray(chrom_idx, dtype=np.int32)
    ps = np.ascontiguousarray(pos, dtype=np.int64)
    if isinstance(alt, str):
        alt = alt.encode("latin-1")
    if isinstance(alt, (bytes, bytearray)):
        ab = np.frombuffer(bytes(alt), dtype=np.uint8)
    else:
        ab = np.asarray(alt)
        ab = ab.astype("S1").view(np.uint8) if ab.dtype.kind in "SU" else ab.astype(np.uint8)
    ab = np.ascontiguousarray(ab).reshape(-1)
    if ci.ndim != 1 or not (ci.size == ps.size == ab.size):
        raise ValueError("chrom_idx, pos and alt must have one entry per variant")
    h = ctypes.c_void_p()
    check(lib().ms_scan_variants(pwms.h, genome.h, ptr(ci, ctypes.c_int32), ptr(ps, ctypes.c_int64), ab.ctypes.data_as(ctypes.c_char_p),
                                 ci.size, int(strand_mask), int(flags), ctypes.byref(h)))
    return VariantScan(h, pwms.n, ci.size)


def varscan_chunk(n_variants):
    """ms_debug_varscan_chunk: variants per chunk of scan_variants, scan_alleles and scan_alleles_best for the calls that follow (0 = the library's own); returns the
    value before.  Tests only."""
    prev = ctypes.c_int64()
    check(lib().ms_debug_varscan_chunk(int(n_variants), ctypes.byref(prev)))
    return prev.value


def varscan_dims():
    """ms_debug_varscan_dims: dict(variants=dict(tile, threads, lds_max_width), alleles=dict(...)) -- per scan the variants of one block's
    tile, the threads of that block, the widest motif whose table is staged in LDS.  Constants of the build; no device."""
    out = np.zeros(6, dtype=np.int32)
    check(lib().ms_debug_varscan_dims(ptr(out, ctypes.c_int32)))
    keys = ("tile", "threads", "lds_max_width")
    return {"variants": dict(zip(keys, out[:3].tolist())), "alleles": dict(zip(keys, out[3:].tolist()))}


class AlleleScan:
    """Records of one ms_scan_alleles call: per motif, variant index, allele (ref first), start, '+' before '-' (include/motifscan_amd.h)."""

    def __init__(self, handle, n_pwms, n_variants):
        self.h = handle
        self.n_pwms = n_pwms
        self.n_variants = n_variants
        n = ctypes.c_int64()
        check(lib().ms_allelescan_num_sites(self.h, ctypes.byref(n)))
        self.n_sites = n.value
        self.motif_offsets = np.zeros(n_pwms + 1, dtype=np.int64)
        check(lib().ms_allelescan_motif_offsets(self.h, ptr(self.motif_offsets, ctypes.c_int64)))

    def sites(self):
        """dict of fresh numpy arrays: variant, allele (0 ref, 1 alt), start (in that haplotype's coordinates), strand (1 '+', 2 '-'),
        score, motif (motif_offsets expanded) and motif_offsets."""
        n = self.n_sites
        variant, start = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        strand, allele = np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.uint8)
        score_ = np.zeros(n, dtype=np.float64)
        check(lib().ms_allelescan_sites(self.h, ptr(variant, ctypes.c_int64), ptr(allele, ctypes.c_uint8), ptr(start, ctypes.c_int64),
                                        ptr(strand, ctypes.c_int8), ptr(score_, ctypes.c_double)))
        motif = np.repeat(np.arange(self.n_pwms, dtype=np.int32), np.diff(self.motif_offsets))
        return {"variant": variant, "allele": allele, "start": start, "strand": strand, "score": score_, "motif": motif,
                "motif_offsets": self.motif_offsets}

    def motif_counts(self):
        """(gained, lost) int64 [P]: variants with records of the motif on the alt haplotype only / on the ref haplotype only."""
        gained, lost = np.zeros(self.n_pwms, dtype=np.int64), np.zeros(self.n_pwms, dtype=np.int64)
        check(lib().ms_allelescan_motif_counts(self.h, ptr(gained, ctypes.c_int64), ptr(lost, ctypes.c_int64)))
        return gained, lost

    def ref_mismatch(self):
        """bool per input variant: its REF string is not what the genome holds (all False when no REF strings were given)."""
        out = np.zeros(self.n_variants, dtype=np.uint8)
        check(lib().ms_allelescan_ref_mismatch(self.h, ptr(out, ctypes.c_uint8)))
        return out.astype(bool)

    def device_ms(self):
        ms = ctypes.c_double()
        check(lib().ms_allelescan_device_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "h", None):
            lib().ms_allelescan_free(self.h)
            self.h = None

    __del__ = close


def _rank_sum(fn, a, b, sel_a, sel_b, m0, m1, timing):
    """One rank-sum call (ms_best_rank_sum / ms_affinity_rank_sum: the same signature) on two result objects of one kind."""
    if a.h is None or b.h is None:
        raise ValueError("the result is closed")
    m0, m1 = int(m0), (a.n_pwms if m1 is None else int(m1))
    rows = max(m1 - m0, 0)
    sa, pa = BestSites._selection(sel_a, a.n_seqs)
    sb, pb = BestSites._selection(sel_b, b.n_seqs)
    u2, ties, n, ms = np.zeros(rows, dtype=np.int64), np.zeros((rows, 2), dtype=np.uint64), np.zeros(2, dtype=np.int64), ctypes.c_double()
    check(fn(a.h, pa, b.h, pb, m0, m1, 0, ptr(u2, ctypes.c_int64), ptr(ties, ctypes.c_uint64), ptr(n, ctypes.c_int64), ctypes.byref(ms)))
    if rows == 0:                                          # (the library leaves its outputs alone for an empty range)
        n[:] = (a.n_seqs if sa is None else int(sa.sum()), b.n_seqs if sb is None else int(sb.sum()))
    if timing is not None:
        timing["device_ms"] = ms.value
    return u2, [int(lo) | (int(hi) << 64) for lo, hi in ties.tolist()], int(n[0]), int(n[1])


class BestSites:
    """The result of one ms_scan_best call: the best-scoring window of every (motif, region) cell (include/motifscan_amd.h).
    .score (float64), .pos (int32, relative to the region start) and .strand (int8: 1 '+', 2 '-') are (P, R) numpy arrays, copied from the
    device the first time they are read; a cell without a winner holds NaN / -1 / 0.  The object owns the device arrays until close():
    keep it alive while device_pointers() are in use."""

    def __init__(self, handle):
        self.h = handle
        p, r = ctypes.c_int32(), ctypes.c_int64()
        check(lib().ms_best_shape(self.h, ctypes.byref(p), ctypes.byref(r)))
        self.n_pwms, self.n_seqs = p.value, r.value
        self._full = None

    @property
    def shape(self):
        return (self.n_pwms, self.n_seqs)

    def sites(self, m0=0, m1=None):
        """(score, pos, strand) of motifs m0 <= m < m1 as fresh (m1 - m0, R) arrays."""
        if self.h is None:
            raise ValueError("the result is closed")
        m1 = self.n_pwms if m1 is None else int(m1)
        m0 = int(m0)
        if m0 < 0 or m1 > self.n_pwms or m0 > m1:
            raise ValueError(f"motif range [{m0}, {m1}) outside [0, {self.n_pwms})")
        shape = (m1 - m0, self.n_seqs)
        score, pos, strand = np.zeros(shape, dtype=np.float64), np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int8)
        check(lib().ms_best_sites(self.h, m0, m1, ptr(score, ctypes.c_double), ptr(pos, ctypes.c_int32), ptr(strand, ctypes.c_int8)))
        return score, pos, strand

    def _arrays(self):
        if self._full is None:
            self._full = self.sites()
        return self._full

    score = property(lambda self: self._arrays()[0])
    pos = property(lambda self: self._arrays()[1])
    strand = property(lambda self: self._arrays()[2])

    def device_pointers(self):
        """(score, pos, strand) device addresses of the full (P, R) arrays, valid until close()."""
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(lib().ms_best_sites_device(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def gaps(self, m0=0, m1=None):
        """ms_best_gaps: the winners' gaps of the rows m0 <= m < m1 as a fresh int16 (m1 - m0, R) array, -1 where no placement wins.  Only
        a result of scan_best_bipartite holds them: every other one raises ValueError."""
        if self.h is None:
            raise ValueError("the result is closed")
        m0, m1 = self._motif_range(m0, m1)
        if m0 < 0 or m1 > self.n_pwms or m0 > m1:
            raise ValueError(f"motif range [{m0}, {m1}) outside [0, {self.n_pwms})")
        gap = np.zeros((m1 - m0, self.n_seqs), dtype=np.int16)
        check(lib().ms_best_gaps(self.h, m0, m1, ptr(gap, ctypes.c_int16)))
        return gap

    def gaps_device_pointer(self):
        """ms_best_gaps_device: the device address of the full (P, R) int16 gap plane, valid until close()."""
        a = ctypes.c_void_p()
        check(lib().ms_best_gaps_device(self.h, ctypes.byref(a)))
        return a.value

    def device_ms(self):
        ms = ctypes.c_double()
        check(lib().ms_best_device_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def _motif_range(self, m0, m1):
        m1 = self.n_pwms if m1 is None else int(m1)
        return int(m0), m1

    @staticmethod
    def _selection(sel, n_seqs):
        """A region selection as the uint8 [R] array the library reads (None stays None: every region)."""
        if sel is None:
            return None, None
        sel = np.ascontiguousarray(np.asarray(sel) != 0, dtype=np.uint8)
        if sel.shape != (n_seqs,):
            raise ValueError(f"a selection must hold one flag per region ({n_seqs}), got shape {sel.shape}")
        return sel, ptr(sel, ctypes.c_uint8)

    def rank_sum(self, other, sel=None, sel_other=None, m0=0, m1=None, timing=None):
        """ms_best_rank_sum of this matrix's selected regions (group A) against `other`'s (group B; may be self): (u2 int64 [m1 - m0],
        ties as a list of Python ints, na, nb).  The matrices stay on the device.  timing: a dict that receives 'device_ms'."""
        return _rank_sum(lib().ms_best_rank_sum, self, other, sel, sel_other, m0, m1, timing)

    def count_passing(self, cutoffs, sel=None, m0=0, m1=None, timing=None):
        """ms_best_count_passing: int64 [m1 - m0][K], the selected regions whose best score passes cutoffs[row][k] by ms_scan's hit rule.
        cutoffs: [m1 - m0][K] (a 1-D array is one cutoff per motif)."""
        if self.h is None:
            raise ValueError("the result is closed")
        m0, m1 = self._motif_range(m0, m1)
        rows = max(m1 - m0, 0)
        cutoffs = np.ascontiguousarray(cutoffs, dtype=np.float64)
        if cutoffs.ndim == 1:
            cutoffs = cutoffs.reshape(-1, 1)
        if cutoffs.ndim != 2 or cutoffs.shape[0] != rows:
            raise ValueError(f"cutoffs must be [{rows}][K], got shape {cutoffs.shape}")
        _, ps = self._selection(sel, self.n_seqs)
        counts, ms = np.zeros(cutoffs.shape, dtype=np.int64), ctypes.c_double()
        check(lib().ms_best_count_passing(self.h, ps, ptr(cutoffs, ctypes.c_double), cutoffs.shape[1], m0, m1, ptr(counts, ctypes.c_int64), ctypes.byref(ms)))
        if timing is not None:
            timing["device_ms"] = ms.value
        return counts

    def close(self):
        if getattr(self, "h", None):
            lib().ms_best_free(self.h)
            self.h = None

    __del__ = close


def scan_best(pwms, seqs, strand_mask=3, flags=0):
    """ms_scan_best: the best window of every (motif, region) cell of a PwmSet x SeqSet (the set's cutoffs are not read).  Returns a BestSites."""
    strand_mask = int(strand_mask)
    if strand_mask not in (1, 2, 3):
        raise ValueError(f"invalid strand mask {strand_mask!r} (1 '+', 2 '-', 3 both)")
    if int(flags) != 0:
        raise ValueError(f"unknown best-site scan flags {flags!r}")
    h = ctypes.c_void_p()
    check(lib().ms_scan_best(pwms.h, seqs.h, strand_mask, int(flags), ctypes.byref(h)))
    return BestSites(h)


class DiModelSet:
    """A set of first-order models as the library holds it (ms_dimodelset_create; include/motifscan_amd.h has the definition).  values:
    float64 [sum of W][16], the models' rows one after the other; widths int32 [P].  Needs no device: the scan uploads the tables."""

    def __init__(self, values, widths):
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.widths = np.ascontiguousarray(widths, dtype=np.int32).reshape(-1)
        self.n = len(self.widths)
        if self.n and int(self.widths.min()) >= 1 and self.values.size != 16 * int(self.widths.astype(np.int64).sum()):
            raise ValueError("values must hold 16 * width doubles per model")
        h = ctypes.c_void_p()
        check(lib().ms_dimodelset_create(ptr(self.values, ctypes.c_double), ptr(self.widths, ctypes.c_int32), self.n, ctypes.byref(h)))
        self.h = h

    @classmethod
    def from_models(cls, models):
        """From dimodel.DiModel objects, or a dimodel.DiModelSet."""
        from . import dimodel
        ms = models if isinstance(models, dimodel.DiModelSet) else dimodel.DiModelSet(models)
        return cls(ms.values, ms.widths)

    def __len__(self):
        return self.n

    def max_raw(self):
        out = np.zeros(self.n, dtype=np.float64)
        check(lib().ms_dimodelset_max_raw(self.h, ptr(out, ctypes.c_double)))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().ms_dimodelset_free(self.h)
            self.h = None

    __del__ = close


def scan_best_dimodels(models, seqs, strand_mask=3, flags=0):
    """ms_scan_best_dimodels: the best window of every (first-order model, region) cell of a DiModelSet x SeqSet.  Returns a BestSites:
    rank_sum, count_passing and the device pointers work on it as on ms_scan_best's."""
    strand_mask = int(strand_mask)
    if strand_mask not in (1, 2, 3):
        raise ValueError(f"invalid strand mask {strand_mask!r} (1 '+', 2 '-', 3 both)")
    if int(flags) != 0:
        raise ValueError(f"unknown first-order best-site scan flags {flags!r}")
    h = ctypes.c_void_p()
    check(lib().ms_scan_best_dimodels(models.h, seqs.h, strand_mask, int(flags), ctypes.byref(h)))
    return BestSites(h)


def scan_best_bipartite(pwms, specs, seqs, strand_mask=3, flags=0):
    """ms_scan_best_bipartite: the best site of every (bipartite spec, region) cell of a PwmSet x SeqSet; specs: bipartite.Bipartite objects
    or (a, b, flip, gap_min, gap_max) tuples.  Returns a BestSites whose gaps() holds the fourth plane: rank_sum, count_passing and the
    device pointers work on it as on ms_scan_best's."""
    from . import bipartite
    strand_mask = int(strand_mask)
    if strand_mask not in (1, 2, 3):
        raise ValueError(f"invalid strand mask {strand_mask!r} (1 '+', 2 '-', 3 both)")
    if int(flags) != 0:
        raise ValueError(f"unknown bipartite best-site scan flags {flags!r}")
    a, b, flip, g0, g1 = bipartite.spec_arrays(specs)
    h = ctypes.c_void_p()
    check(lib().ms_scan_best_bipartite(pwms.h, ptr(a, ctypes.c_int32), ptr(b, ctypes.c_int32), ptr(flip, ctypes.c_uint8), ptr(g0, ctypes.c_int32),
                                       ptr(g1, ctypes.c_int32), len(a), seqs.h, strand_mask, int(flags), ctypes.byref(h)))
    return BestSites(h)


def bipartite_dims():
    """ms_debug_bipartite_dims: dict(threads, seg_windows, tile_entries, max_width, max_gap, halo_strips, lds_bytes) -- the sizes at which
    ms_scan_best_bipartite changes segment or tile, and its caps.  Constants of the build; no device."""
    out = np.zeros(8, dtype=np.int32)
    check(lib().ms_debug_bipartite_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("threads", "seg_windows", "tile_entries", "max_width", "max_gap", "halo_strips", "lds_bytes"), (int(v) for v in out[:7])))


def dimodel_dims():
    """ms_debug_dimodel_dims: dict(threads, seg_windows, tile_entries, max_width, strips, word_steps) -- the sizes at which
    ms_scan_best_dimodels changes segment, tile or word.  Constants of the build; no device."""
    out = np.zeros(8, dtype=np.int32)
    check(lib().ms_debug_dimodel_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("threads", "seg_windows", "tile_entries", "max_width", "strips", "word_steps"), (int(v) for v in out[:6])))


class Affinity:
    """The result of one ms_scan_affinity call: the summed likelihood ratio of every (motif, region) cell (include/motifscan_amd.h).
    .peak, .sum, .log_mean (float64) and .n_terms (int32) are (P, R) numpy arrays, copied from the device the first time they are
    read; a cell without a term holds NaN / 0 / NaN / 0.  The object owns the device planes until close(): keep it alive while
    device_pointers() are in use."""

    def __init__(self, handle):
        self.h = handle
        p, r = ctypes.c_int32(), ctypes.c_int64()
        check(lib().ms_affinity_shape(self.h, ctypes.byref(p), ctypes.byref(r)))
        self.n_pwms, self.n_seqs = p.value, r.value
        self._full = None
        self.expected_counts_ms = None                   # device_ms of the last expected_counts call

    @property
    def shape(self):
        return (self.n_pwms, self.n_seqs)

    def cells(self, m0=0, m1=None):
        """(peak, sum, n_terms, log_mean) of motifs m0 <= m < m1 as fresh (m1 - m0, R) arrays."""
        if self.h is None:
            raise ValueError("the result is closed")
        m1 = self.n_pwms if m1 is None else int(m1)
        m0 = int(m0)
        if m0 < 0 or m1 > self.n_pwms or m0 > m1:
            raise ValueError(f"motif range [{m0}, {m1}) outside [0, {self.n_pwms})")
        shape = (m1 - m0, self.n_seqs)
        peak, total, log_mean = (np.zeros(shape, dtype=np.float64) for _ in range(3))
        n_terms = np.zeros(shape, dtype=np.int32)
        check(lib().ms_affinity_cells(self.h, m0, m1, ptr(peak, ctypes.c_double), ptr(total, ctypes.c_double), ptr(n_terms, ctypes.c_int32),
                                      ptr(log_mean, ctypes.c_double)))
        return peak, total, n_terms, log_mean

    def _arrays(self):
        if self._full is None:
            self._full = self.cells()
        return self._full

    peak = property(lambda self: self._arrays()[0])
    sum = property(lambda self: self._arrays()[1])
    n_terms = property(lambda self: self._arrays()[2])
    log_mean = property(lambda self: self._arrays()[3])

    def device_pointers(self):
        """(peak, sum, n_terms, log_mean) device addresses of the full (P, R) planes, valid until close()."""
        a = [ctypes.c_void_p() for _ in range(4)]
        check(lib().ms_affinity_cells_device(self.h, *[ctypes.byref(x) for x in a]))
        return tuple(x.value for x in a)

    def device_ms(self):
        ms = ctypes.c_double()
        check(lib().ms_affinity_device_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def rank_sum(self, other, sel=None, sel_other=None, m0=0, m1=None, timing=None):
        """ms_affinity_rank_sum of this result's selected regions (group A) against `other`'s (group B; may be self), on the log_mean
        planes: (u2 int64 [m1 - m0], ties as a list of Python ints, na, nb) -- BestSites.rank_sum's form.  The planes stay on the device."""
        return _rank_sum(lib().ms_affinity_rank_sum, self, other, sel, sel_other, m0, m1, timing)

    def expected_counts(self, pwms, seqs, prior_logit=math.inf, motifs=slice(None), out=None):
        """ms_affinity_expected_counts on this result, which must come from scan_affinity(pwms, seqs, ...): (counts int64
        [rows][max width][5], total int64 [rows], n_regions int64 [rows]) of the motifs of the slice `motifs` (step 1), in units of
        2^-32 -- em.ExpectedCounts reads them.  prior_logit = log(gamma / (1 - gamma)) of the ZOOPS prior, +inf for OOPS.  out: None, or
        (counts, total, n_regions), each a C-contiguous int64 array of that shape, None (a new one), or the device pointer of a torch
        tensor as an int (then it is returned).  The call's device_ms is left in self.expected_counts_ms.  The library checks the rest."""
        if self.h is None:
            raise ValueError("the result is closed")
        prior_logit = float(prior_logit)
        if math.isnan(prior_logit):
            raise ValueError("prior_logit is NaN")
        if not isinstance(motifs, slice) or motifs.step not in (None, 1):
            raise ValueError("motifs must be a slice of step 1")
        m0, m1, _ = motifs.indices(self.n_pwms)
        m1 = max(m1, m0)
        rows = m1 - m0
        C = int(pwms.widths.max()) if pwms.n else 0
        shapes = ((rows, C, 5), (rows,), (rows,))
        given = (None, None, None) if out is None else tuple(out)
        if len(given) != 3:
            raise ValueError("out must be (counts, total, n_regions)")
        arrs, dst = [], []
        for a, shape in zip(given, shapes):
            if isinstance(a, int):
                p = a
            else:
                if a is None:
                    a = np.zeros(shape, dtype=np.int64)
                if a.dtype != np.int64 or a.shape != shape or not a.flags.c_contiguous:
                    raise ValueError("out arrays must be C-contiguous int64 of shapes (rows, max width, 5), (rows,) and (rows,)")
                p = a.ctypes.data
            arrs.append(a)
            dst.append(ctypes.c_void_p(p))
        ms = ctypes.c_double(0.0)
        check(lib().ms_affinity_expected_counts(self.h, pwms.h, seqs.h, prior_logit, m0, m1, 0, dst[0], dst[1], dst[2], ctypes.byref(ms)))
        self.expected_counts_ms = ms.value
        return tuple(arrs)

    def close(self):
        if getattr(self, "h", None):
            lib().ms_affinity_free(self.h)
            self.h = None

    __del__ = close


def scan_affinity(pwms, seqs, strand_mask=3, scale=1.0, max_n=-1, flags=0):
    """ms_scan_affinity: the summed likelihood ratio of every (motif, region) cell of a PwmSet x SeqSet (the set's cutoffs are not read).
    scale: finite and > 0 (1.0 for natural-log odds); max_n >= 0: only windows of at most max_n non-ACGT bases are terms.
    Returns an Affinity."""
    from .affinity import check_args
    strand_mask = int(strand_mask)
    if strand_mask not in (1, 2, 3):
        raise ValueError(f"invalid strand mask {strand_mask!r} (1 '+', 2 '-', 3 both)")
    if int(flags) != 0:
        raise ValueError(f"unknown affinity scan flags {flags!r}")
    scale, max_n = check_args(scale, max_n)
    h = ctypes.c_void_p()
    check(lib().ms_scan_affinity(pwms.h, seqs.h, strand_mask, scale, max_n, int(flags), ctypes.byref(h)))
    return Affinity(h)


def affinity_dims():
    """ms_debug_affinity_dims: dict(segment_windows, tile_max_width, tile_entries, waves, strips, part_bytes) -- the sizes at which
    ms_scan_affinity changes path.  Constants of the build; no device."""
    out = np.zeros(8, dtype=np.int32)
    check(lib().ms_debug_affinity_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("segment_windows", "tile_max_width", "tile_entries", "waves", "strips", "part_bytes"), out.tolist()))


def expected_dims():
    """ms_debug_expected_dims: dict(segment_windows, max_width, tile_entries, waves, strips, acc_bytes_per_column, grid_cap) -- the sizes
    of ms_affinity_expected_counts' walk.  Constants of the build; no device."""
    out = np.zeros(8, dtype=np.int32)
    check(lib().ms_debug_expected_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("segment_windows", "max_width", "tile_entries", "waves", "strips", "acc_bytes_per_column", "grid_cap"), out.tolist()))


@contextlib.contextmanager
def expected_grid_cap(blocks):
    """ms_debug_expected_grid_cap for the body of a `with`: the blocks per tile of ms_affinity_expected_counts' grid (0 = the library's
    own), given back at the end.  The result does not depend on it.  Tests only."""
    check(lib().ms_debug_expected_grid_cap(int(blocks)))
    try:
        yield
    finally:
        check(lib().ms_debug_expected_grid_cap(0))


@contextlib.contextmanager
def alloc_fill(byte):
    """ms_debug_alloc_fill for the body of a `with`: every device and pinned block the library hands out is filled with `byte` (0..255)
    over its whole size before its caller sees it; -1 turns the fill off.  The value before is put back at the end.  No result depends on
    it.  Tests only."""
    before = ctypes.c_int32(-1)
    check(lib().ms_debug_alloc_fill(int(byte), ctypes.byref(before)))
    try:
        yield before.value
    finally:
        check(lib().ms_debug_alloc_fill(before.value, None))


def histogram_binning(n_pwms, lo, hi, n_bins):
    """(lo [P], inv_width [P]) of a score histogram: scalars broadcast, inv_width = n_bins / (hi - lo) as one float64 division each.
    Pure numpy."""
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (n_pwms,)))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), (n_pwms,))
    with np.errstate(all="ignore"):
        inv_width = np.ascontiguousarray(np.float64(n_bins) / (hi - lo))
    return lo, inv_width


def score_histogram(pwms, seqs, strand_mask, lo, hi, n_bins, per_position=False, max_n=-1, out=None, timing=None):
    """ms_scan_score_histogram: int64 [P][n_bins + 2], per motif the number of windows of the sequence set per score bin -- slot 0
    "below lo", slots 1 .. n_bins the bins of [lo, hi), slot n_bins + 1 "at or above hi" (the exact rule: include/motifscan_amd.h;
    motifscan_amd.scoredist restates it).  lo, hi: per motif, scalars broadcast.  per_position: one count per window start (c_score's
    max over the strands) instead of one per (window, strand).  max_n >= 0: windows with more non-ACGT bases are not counted.  out: an
    int64 numpy array of that shape, or None (a new one); the device pointer of a torch tensor may be passed as an int instead (then it
    is returned).  timing: a dict that receives 'device_ms'.  The library checks every argument."""
    n_bins = int(n_bins)
    lo, inv_width = histogram_binning(pwms.n, lo, hi, n_bins)
    shape = (pwms.n, n_bins + 2)
    if isinstance(out, int):
        dst = out
    else:
        if out is None:
            out = np.zeros(shape, dtype=np.int64)
        if out.dtype != np.int64 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous int64 array of shape (P, n_bins + 2)")
        dst = out.ctypes.data
    ms = ctypes.c_double()
    check(lib().ms_scan_score_histogram(pwms.h, seqs.h, int(strand_mask), MS_HIST_PER_POSITION if per_position else 0, ptr(lo, ctypes.c_double),
                                        ptr(inv_width, ctypes.c_double), n_bins, int(max_n), ctypes.c_void_p(dst), ctypes.byref(ms)))
    if timing is not None:
        timing["device_ms"] = ms.value
    return out


def scorehist_dims():
    """ms_debug_scorehist_dims: dict(segment_windows, tile_max_width, lds_slots, flush_windows) -- the sizes at which
    ms_scan_score_histogram changes path.  Constants of the build; no device."""
    out = np.zeros(4, dtype=np.int32)
    check(lib().ms_debug_scorehist_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("segment_windows", "tile_max_width", "lds_slots", "flush_windows"), out.tolist()))


MS_SCOREDIST_MAX_ORDER, MS_SCOREDIST_MAX_BINS = 5, 1 << 20


def score_distribution(pwms, strand, order, cond, init, n_bins, out=None, timing=None):
    """ms_pwmset_score_distribution: (mass float64 [P][n_bins], step float64 [P], s0 int64 [P]) -- per motif the probability of every
    integer score s0 + i of a window under the Markov background (cond [4^order][4], init [4^order]); the definition is in
    include/motifscan_amd.h and motifscan_amd.pvalues.restate_distribution restates it.  strand: 1 forward, 2 reverse.  out: a float64
    numpy array (P, n_bins), or None (a new one); the device pointer of a torch tensor may be passed as an int instead (then it is
    returned).  timing: a dict that receives 'device_ms'.  The library checks every argument."""
    n_bins, order = int(n_bins), int(order)
    n_ctx = 4 ** order if 0 <= order <= MS_SCOREDIST_MAX_ORDER else 1          # (an invalid order: the library refuses it before it reads)
    cond = np.ascontiguousarray(cond, dtype=np.float64)
    init = np.ascontiguousarray(init, dtype=np.float64)
    if cond.size != 4 * n_ctx or init.size != n_ctx:
        raise ValueError(f"cond must hold {n_ctx} x 4 entries and init {n_ctx}")
    shape = (pwms.n, max(n_bins, 0))
    if isinstance(out, int):
        dst = out
    else:
        if out is None:
            out = np.zeros(shape, dtype=np.float64)
        if out.dtype != np.float64 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of shape (P, n_bins)")
        dst = out.ctypes.data
    step, s0 = np.zeros(pwms.n, dtype=np.float64), np.zeros(pwms.n, dtype=np.int64)
    ms = ctypes.c_double()
    check(lib().ms_pwmset_score_distribution(pwms.h, int(strand), order, ptr(cond, ctypes.c_double), ptr(init, ctypes.c_double), n_bins,
                                             ptr(step, ctypes.c_double), ptr(s0, ctypes.c_int64), ctypes.c_void_p(dst), ctypes.byref(ms)))
    if timing is not None:
        timing["device_ms"] = ms.value
    return out, step, s0


def scoredist_dims():
    """ms_debug_scoredist_dims: dict(threads, tile_bins, lds_elems, budget_mib) -- the sizes at which ms_pwmset_score_distribution changes
    path: the bins per block of the global path, and the largest contexts x bins the LDS path takes.  Constants of the build; no device."""
    out = np.zeros(4, dtype=np.int32)
    check(lib().ms_debug_scoredist_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("threads", "tile_bins", "lds_elems", "budget_mib"), out.tolist()))


def scoredist_budget(nbytes):
    """ms_debug_scoredist_budget: the bytes of ping-pong buffers a score distribution holds at once for the calls that follow (0 = the
    library's own); returns the value before."""
    prev = ctypes.c_int64()
    check(lib().ms_debug_scoredist_budget(int(nbytes), ctypes.byref(prev)))
    return prev.value


def scoredist_force_global(on):
    """ms_debug_scoredist_force_global: the calls that follow take the global path even where the LDS path applies (False gives the
    choice back); returns the value before."""
    prev = ctypes.c_int32()
    check(lib().ms_debug_scoredist_force_global(1 if on else 0, ctypes.byref(prev)))
    return bool(prev.value)


MS_COMPARE_PEARSON, MS_COMPARE_SW, MS_COMPARE_ED = 0, 1, 2
MS_COMPARE_MAX_WIDTH, MS_COMPARE_MAX_BINS = 64, 256
COMPARE_PLANES = (("p_min", np.float64), ("offset", np.int32), ("overlap", np.int32), ("score", np.int32), ("n_offsets", np.int32), ("orient", np.int8))


def _flat_set(values, widths):
    """(values float64 [sum 4 W], widths int32 [n]) contiguous, with the one check the library cannot make: the two agree in size."""
    values = np.ascontiguousarray(values, dtype=np.float64).ravel()
    widths = np.ascontiguousarray(widths, dtype=np.int32).ravel()
    if values.size != 4 * int(widths.astype(np.int64).sum()):
        raise ValueError("values must hold 4 * width doubles per matrix")
    return values, widths


def compare_motifs(q_values, q_widths, t_values, t_widths, metric=MS_COMPARE_PEARSON, bins=100, min_overlap=5, orientations=3, q0=0, q1=None,
                   timing=None):
    """ms_motifs_compare: dict of the six host planes [(q1 - q0)][n_t] -- p_min float64, offset, overlap, score, n_offsets int32, orient
    int8 -- of the queries [q0, q1) against all targets; the definition is in include/motifscan_amd.h and
    motifscan_amd.compare.restate_compare restates it.  values / widths: the matrices concatenated, row-major [4][W] each
    (MotifSet.flat()).  timing: a dict to whose 'device_ms' this call's is ADDED (a caller that tiles the queries gets the sum).  The
    library checks every argument."""
    q_values, q_widths = _flat_set(q_values, q_widths)
    t_values, t_widths = _flat_set(t_values, t_widths)
    n_q, n_t = len(q_widths), len(t_widths)
    q1 = n_q if q1 is None else int(q1)
    rows = max(q1 - int(q0), 0)
    out = {name: np.zeros((rows, n_t), dtype=dt) for name, dt in COMPARE_PLANES}
    ms = ctypes.c_double()
    check(lib().ms_motifs_compare(ptr(q_values, ctypes.c_double), ptr(q_widths, ctypes.c_int32), n_q, ptr(t_values, ctypes.c_double),
                                  ptr(t_widths, ctypes.c_int32), n_t, int(metric), int(bins), int(min_overlap), int(orientations), int(q0), q1,
                                  ptr(out["p_min"], ctypes.c_double), ptr(out["offset"], ctypes.c_int32), ptr(out["overlap"], ctypes.c_int32),
                                  ptr(out["score"], ctypes.c_int32), ptr(out["n_offsets"], ctypes.c_int32), ptr(out["orient"], ctypes.c_int8),
                                  ctypes.byref(ms)))
    if timing is not None:
        timing["device_ms"] = timing.get("device_ms", 0.0) + ms.value
    return out


def compare_dims():
    """ms_debug_compare_dims: dict(threads, hist_tile, align_tile, budget_mib, batch_cap, hist_grid_y, lds_limit) -- the sizes at which
    ms_motifs_compare changes tile or batch (lds_limit 0: the tables have one path).  Constants of the build; no device."""
    out = np.zeros(8, dtype=np.int32)
    check(lib().ms_debug_compare_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("threads", "hist_tile", "align_tile", "budget_mib", "batch_cap", "hist_grid_y", "lds_limit"), out.tolist()))


def compare_budget(nbytes):
    """ms_debug_compare_budget: the bytes of tables a comparison holds at once for the calls that follow (0 = the library's own); returns
    the value before."""
    prev = ctypes.c_int64()
    check(lib().ms_debug_compare_budget(int(nbytes), ctypes.byref(prev)))
    return prev.value


def compare_null(q_values, q_widths, t_values, t_widths, metric, bins, orientations, query):
    """ms_debug_compare_null: (H uint32 [Wq][bins], tail float64 flat: every table of the query in (a ascending, L ascending) order) as
    ms_motifs_compare builds them for query `query`.  Tests only."""
    q_values, q_widths = _flat_set(q_values, q_widths)
    t_values, t_widths = _flat_set(t_values, t_widths)
    query, bins = int(query), int(bins)
    W = int(q_widths[query]) if 0 <= query < len(q_widths) else 1
    if not (1 <= W <= MS_COMPARE_MAX_WIDTH and 2 <= bins <= MS_COMPARE_MAX_BINS):      # (the library refuses these before it writes)
        W, bins_h = 1, 1
    else:
        bins_h = bins
    n_tail = sum((bins_h - 1) * n * (n + 1) // 2 + n for n in range(1, W + 1))
    H, tail = np.zeros((W, bins_h), dtype=np.uint32), np.zeros(n_tail, dtype=np.float64)
    check(lib().ms_debug_compare_null(ptr(q_values, ctypes.c_double), ptr(q_widths, ctypes.c_int32), len(q_widths), ptr(t_values, ctypes.c_double),
                                      ptr(t_widths, ctypes.c_int32), len(t_widths), int(metric), bins, int(orientations), query,
                                      ptr(H, ctypes.c_uint32), ptr(tail, ctypes.c_double)))
    return H, tail


def best_segment_windows():
    """ms_debug_best_segment_windows: window starts per segment of ms_scan_best (tests size a multi-segment region with it)."""
    return int(lib().ms_debug_best_segment_windows())


def ranksum_dims():
    """ms_debug_ranksum_dims: the path constants of ms_best_rank_sum and ms_best_count_passing -- dict(threads, gather_elems, rank_elems,
    count_elems, budget, cut_chunk, segmented_max).  Constants of the build; no device."""
    out = np.zeros(8, dtype=np.int32)
    check(lib().ms_debug_ranksum_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("threads", "gather_elems", "rank_elems", "count_elems", "budget", "cut_chunk", "segmented_max"), out.tolist()))


def ranksum_budget(elems):
    """ms_debug_ranksum_budget: the elements ms_best_rank_sum holds at once for the calls that follow (0 = the library's own); returns the
    value before."""
    prev = ctypes.c_int64()
    check(lib().ms_debug_ranksum_budget(int(elems), ctypes.byref(prev)))
    return prev.value


def pair_lds_bins():
    """ms_debug_pair_lds_bins: the widest 2 * max_dist + 1 that ms_result_pair_spacing bins in LDS."""
    return int(lib().ms_debug_pair_lds_bins())


def sitestack_dims():
    """ms_debug_sitestack_dims: the path constants of ms_result_site_base_counts -- dict(threads, chunk_hits, lds_columns,
    lds_columns_no_dinuc).  Constants of the build; no device."""
    out = np.zeros(4, dtype=np.int32)
    check(lib().ms_debug_sitestack_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("threads", "chunk_hits", "lds_columns", "lds_columns_no_dinuc"), out.tolist()))


def sitesignal_dims():
    """ms_debug_sitesignal_dims: the path constants of ms_result_site_signal -- dict(threads, chunk_sites, panel_columns, max_blocks_x).
    Constants of the build; no device."""
    out = np.zeros(4, dtype=np.int32)
    check(lib().ms_debug_sitesignal_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("threads", "chunk_sites", "panel_columns", "max_blocks_x"), out.tolist()))


def cooc_chunk_regions():
    """ms_debug_cooc_chunk_regions: regions per LDS stage of ms_result_cooccurrence."""
    return int(lib().ms_debug_cooc_chunk_regions())


def plot_dims():
    """ms_debug_plot_dims: the sizes at which the plot-data kernels change path -- dict(hist_lds_bins, hist_hits_per_block,
    hist_max_blocks, scan_threads, prof_tile, half).  Constants of the build; no device."""
    out = np.zeros(6, dtype=np.int32)
    check(lib().ms_debug_plot_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("hist_lds_bins", "hist_hits_per_block", "hist_max_blocks", "scan_threads", "prof_tile", "half"), out.tolist()))


def genome_dims():
    """ms_debug_genome_dims: the sizes at which the kernels either side of the scan change path -- dict(count_tile_bases, lds_chroms,
    filter_threads, pack_block_bases, near_threads, gene_tile, overlap_threads, rank_budget); constants of the build, no GPU."""
    out = np.zeros(8, dtype=np.int32)
    check(lib().ms_debug_genome_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("count_tile_bases", "lds_chroms", "filter_threads", "pack_block_bases", "near_threads", "gene_tile", "overlap_threads",
                     "rank_budget"), out.tolist()))


def seqset_planes(seqs):
    """ms_debug_seqset_planes: (codes, nmask, blk2reg, blkinfo [n, 4]) of a SeqSet or a ResidentGenome as they are on the device, in
    host_pack's layout."""
    n = ctypes.c_int64()
    check(lib().ms_seqset_size(seqs.h, None, ctypes.byref(n)))
    n = n.value
    units, blocks = (n + 31) // 32, (n + 63) // 64 + 1
    codes, nmask = np.zeros(2 * units, dtype=np.uint32), np.zeros(units, dtype=np.uint32)
    blk2reg, blkinfo = np.zeros(blocks, dtype=np.int32), np.zeros((blocks, 4), dtype=np.int32)
    check(lib().ms_debug_seqset_planes(seqs.h, ptr(codes, ctypes.c_uint32), ptr(nmask, ctypes.c_uint32), ptr(blk2reg, ctypes.c_int32),
                                       ptr(blkinfo, ctypes.c_int32)))
    return codes, nmask, blk2reg, blkinfo


def seqset_pad_words(seqs):
    """ms_debug_seqset_pad_words: (codes_pad [16], nmask_pad [16]) -- the words behind the two planes of a SeqSet or a ResidentGenome as
    they are on the device.  Every maker of a set leaves them zero."""
    codes_pad, nmask_pad = np.empty(16, dtype=np.uint32), np.empty(16, dtype=np.uint32)
    check(lib().ms_debug_seqset_pad_words(seqs.h, ptr(codes_pad, ctypes.c_uint32), ptr(nmask_pad, ctypes.c_uint32)))
    return codes_pad, nmask_pad


def score_rank_budget(elems):
    """ms_debug_score_rank_budget: the scores score_ranks holds at once for the calls that follow (0 = the library's own); returns the
    value before."""
    prev = ctypes.c_int64()
    check(lib().ms_debug_score_rank_budget(int(elems), ctypes.byref(prev)))
    return prev.value


def pair_lds_pair_limit(limit):
    """ms_debug_pair_lds_pair_limit: partner hits x anchor hits up to which a block of pair_spacing bins in LDS, for the calls that follow
    (0 = the library's own); returns the value before.  Tests only."""
    prev = ctypes.c_int64()
    check(lib().ms_debug_pair_lds_pair_limit(int(limit), ctypes.byref(prev)))
    return prev.value


def _flatten_alleles(seqs):
    """Sequences of str / bytes -> (their bytes concatenated as a uint8 array, int64 offsets [n + 1])."""
    parts = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    if parts:
        np.cumsum([len(p) for p in parts], out=offsets[1:])
    return np.frombuffer(b"".join(parts), dtype=np.uint8), offsets


def scan_alleles(pwms, genome, chrom_idx, pos, ref_len, alts, refs=None, strand_mask=3, flags=0):
    """ms_scan_alleles: chrom_idx / pos (0-based) / ref_len (reference bases replaced) / alts (a str or bytes per variant, '' for a
    deletion) against a ResidentGenome; refs (a str or bytes per variant, of ref_len bytes) has the library compare them with the genome.
    Returns an AlleleScan."""
    ci = np.ascontiguousarray(chrom_idx, dtype=np.int32)
    ps = np.ascontiguousarray(pos, dtype=np.int64)
    rl = np.ascontiguousarray(ref_len, dtype=np.int32)
    ab, ao = _flatten_alleles(alts)
    if ci.ndim != 1 or not (ci.size == ps.size == rl.size == ao.size - 1):
        raise ValueError("chrom_idx, pos, ref_len and alts must have one entry per variant")
    rb = None
    if refs is not None:
        rb, ro = _flatten_alleles(refs)
        if ro.size - 1 != ci.size or not np.array_equal(np.diff(ro), rl):
            raise ValueError("refs must hold one string of ref_len bytes per variant")
    h = ctypes.c_void_p()
    check(lib().ms_scan_alleles(pwms.h, genome.h, ptr(ci, ctypes.c_int32), ptr(ps, ctypes.c_int64), ptr(rl, ctypes.c_int32),
                                ab.ctypes.data_as(ctypes.c_char_p), ptr(ao, ctypes.c_int64),
                                None if rb is None else rb.ctypes.data_as(ctypes.c_char_p), ci.size, int(strand_mask), int(flags), ctypes.byref(h)))
    return AlleleScan(h, pwms.n, ci.size)


class AlleleBest:
    """The result of one ms_scan_alleles_best call: the best-scoring window of every (motif, variant, haplotype) cell
    (include/motifscan_amd.h).  sites(m0, m1) copies out the six (m1 - m0, V) arrays of a motif range: score (float64), offset (int32,
    winning start - x in that haplotype's coordinates) and strand (int8: 1 '+', 2 '-') for the ref and for the alt haplotype; a cell
    without a winner holds NaN / 0 / 0.  The object owns the device arrays until close(): keep it alive while device_pointers() are in use."""

    FIELDS = ("score_ref", "offset_ref", "strand_ref", "score_alt", "offset_alt", "strand_alt")

    def __init__(self, handle):
        self.h = handle
        p, v = ctypes.c_int32(), ctypes.c_int64()
        check(lib().ms_allelebest_shape(self.h, ctypes.byref(p), ctypes.byref(v)))
        self.n_pwms, self.n_variants = p.value, v.value

    @property
    def shape(self):
        return (self.n_pwms, self.n_variants)

    def sites(self, m0=0, m1=None):
        """dict of fresh (m1 - m0, V) arrays: score_ref, offset_ref, strand_ref, score_alt, offset_alt, strand_alt."""
        if self.h is None:
            raise ValueError("the result is closed")
        m1 = self.n_pwms if m1 is None else int(m1)
        m0 = int(m0)
        if m0 < 0 or m1 > self.n_pwms or m0 > m1:
            raise ValueError(f"motif range [{m0}, {m1}) outside [0, {self.n_pwms})")
        shape = (m1 - m0, self.n_variants)
        out = {}
        for hap in ("ref", "alt"):
            out["score_" + hap] = np.zeros(shape, dtype=np.float64)
            out["offset_" + hap] = np.zeros(shape, dtype=np.int32)
            out["strand_" + hap] = np.zeros(shape, dtype=np.int8)
        check(lib().ms_allelebest_sites(self.h, m0, m1, ptr(out["score_ref"], ctypes.c_double), ptr(out["offset_ref"], ctypes.c_int32),
                                        ptr(out["strand_ref"], ctypes.c_int8), ptr(out["score_alt"], ctypes.c_double),
                                        ptr(out["offset_alt"], ctypes.c_int32), ptr(out["strand_alt"], ctypes.c_int8)))
        return out

    def ref_mismatch(self):
        """bool per input variant: its REF string is not what the genome holds (all False when no REF strings were given)."""
        out = np.zeros(self.n_variants, dtype=np.uint8)
        check(lib().ms_allelebest_ref_mismatch(self.h, ptr(out, ctypes.c_uint8)))
        return out.astype(bool)

    def device_pointers(self):
        """dict of the device addresses of the six full (P, V) arrays, valid until close()."""
        a = [ctypes.c_void_p() for _ in self.FIELDS]
        check(lib().ms_allelebest_sites_device(self.h, *[ctypes.byref(x) for x in a]))
        return {k: x.value for k, x in zip(self.FIELDS, a)}

    def device_ms(self):
        ms = ctypes.c_double()
        check(lib().ms_allelebest_device_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "h", None):
            lib().ms_allelebest_free(self.h)
            self.h = None

    __del__ = close


def scan_alleles_best(pwms, genome, chrom_idx, pos, ref_len, alts, refs=None, strand_mask=3, flags=0):
    """ms_scan_alleles_best: scan_alleles' arguments (the PwmSet's cutoffs are not read); the best window of every (motif, variant,
    haplotype) cell.  Returns an AlleleBest."""
    ci = np.ascontiguousarray(chrom_idx, dtype=np.int32)
    ps = np.ascontiguousarray(pos, dtype=np.int64)
    rl = np.ascontiguousarray(ref_len, dtype=np.int32)
    ab, ao = _flatten_alleles(alts)
    if ci.ndim != 1 or not (ci.size == ps.size == rl.size == ao.size - 1):
        raise ValueError("chrom_idx, pos, ref_len and alts must have one entry per variant")
    rb = None
    if refs is not None:
        rb, ro = _flatten_alleles(refs)
        if ro.size - 1 != ci.size or not np.array_equal(np.diff(ro), rl):
            raise ValueError("refs must hold one string of ref_len bytes per variant")
    h = ctypes.c_void_p()
    check(lib().ms_scan_alleles_best(pwms.h, genome.h, ptr(ci, ctypes.c_int32), ptr(ps, ctypes.c_int64), ptr(rl, ctypes.c_int32),
                                     ab.ctypes.data_as(ctypes.c_char_p), ptr(ao, ctypes.c_int64),
                                     None if rb is None else rb.ctypes.data_as(ctypes.c_char_p), ci.size, int(strand_mask), int(flags), ctypes.byref(h)))
    return AlleleBest(h)


def allelebest_dims():
    """ms_debug_allelebest_dims: dict(tile, long_windows, lds_max_width) -- variants per block tile, the window count above which a cell
    takes the wave path, the widest motif whose table is staged in LDS.  Constants of the build; no device."""
    out = np.zeros(3, dtype=np.int32)
    check(lib().ms_debug_allelebest_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("tile", "long_windows", "lds_max_width"), out.tolist()))


MS_APPLY_SKIP_MISMATCH, MS_LIFT_REF_TO_ALT, MS_LIFT_ALT_TO_REF = 1, 0, 1


class LiftMap:
    """The coordinate map of one ms_genome_apply_alleles call (include/motifscan_amd.h): `status` (uint8 per input variant: 1 applied,
    0 skipped for overlap, 2 skipped for a REF mismatch), `ref_mismatch`, the chromosome lengths of both genomes, and the two lifts --
    to_alt(chrom_idx, pos) / to_ref(chrom_idx, pos) return (positions int64, inside uint8).  It outlives both genomes."""

    def __init__(self, handle):
        self.h = handle
        c, v, n = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        check(lib().ms_liftmap_shape(self.h, ctypes.byref(c), ctypes.byref(v), ctypes.byref(n)))
        self.n_chroms, self.n_variants, self.n_applied = c.value, v.value, n.value
        self.status, self.ref_mismatch = np.zeros(v.value, dtype=np.uint8), np.zeros(v.value, dtype=np.uint8)
        check(lib().ms_liftmap_status(self.h, ptr(self.status, ctypes.c_uint8)))
        check(lib().ms_liftmap_ref_mismatch(self.h, ptr(self.ref_mismatch, ctypes.c_uint8)))
        self.ref_sizes, self.alt_sizes = np.zeros(c.value, dtype=np.int64), np.zeros(c.value, dtype=np.int64)
        check(lib().ms_liftmap_chrom_sizes(self.h, ptr(self.ref_sizes, ctypes.c_int64), ptr(self.alt_sizes, ctypes.c_int64)))

    def _lift(self, direction, chrom_idx, pos):
        if not getattr(self, "h", None):
            raise ValueError("the lift map is closed")
        ps = np.ascontiguousarray(pos, dtype=np.int64)
        ci = np.ascontiguousarray(np.broadcast_to(np.asarray(chrom_idx, dtype=np.int32), ps.shape))
        if ps.ndim != 1:
            raise ValueError("chrom_idx and pos must be one-dimensional, one entry per query")
        out, inside = np.zeros(ps.size, dtype=np.int64), np.zeros(ps.size, dtype=np.uint8)
        check(lib().ms_liftmap_lift(self.h, direction, ptr(ci, ctypes.c_int32), ptr(ps, ctypes.c_int64), ps.size, ptr(out, ctypes.c_int64),
                                    ptr(inside, ctypes.c_uint8)))
        return out, inside

    def to_alt(self, chrom_idx, pos):
        return self._lift(MS_LIFT_REF_TO_ALT, chrom_idx, pos)

    def to_ref(self, chrom_idx, pos):
        return self._lift(MS_LIFT_ALT_TO_REF, chrom_idx, pos)

    def device_ms(self):
        ms = ctypes.c_double()
        check(lib().ms_liftmap_device_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def stage_ms(self):
        """ms_debug_liftmap_stage_ms: dict(prep, order, host, splice) of the call that made the map."""
        out = np.zeros(4)
        check(lib().ms_debug_liftmap_stage_ms(self.h, ptr(out, ctypes.c_double)))
        return dict(zip(("prep", "order", "host", "splice"), out.tolist()))

    def close(self):
        if getattr(self, "h", None):
            lib().ms_liftmap_free(self.h)
            self.h = None

    __del__ = close


def apply_alleles(genome, chrom_idx, pos, ref_len, alts, refs=None, skip_mismatch=False):
    """ms_genome_apply_alleles: scan_alleles' variant arguments applied to a ResidentGenome TOGETHER.  Returns (ResidentGenome, LiftMap):
    the personal haplotype as a new resident genome with the same chromosome names -- Scanner and every region-based entry point take it
    as it is; its packed() and fetch_sequence are served by the planes copied back (N for every non-ACGT base) -- and the map between
    the two coordinate systems.  The header has the overlap rule."""
    ci = np.ascontiguousarray(chrom_idx, dtype=np.int32)
    ps = np.ascontiguousarray(pos, dtype=np.int64)
    rl = np.ascontiguousarray(ref_len, dtype=np.int32)
    ab, ao = _flatten_alleles(alts)
    if ci.ndim != 1 or not (ci.size == ps.size == rl.size == ao.size - 1):
        raise ValueError("chrom_idx, pos, ref_len and alts must have one entry per variant")
    rb = None
    if refs is not None:
        rb, ro = _flatten_alleles(refs)
        if ro.size - 1 != ci.size or not np.array_equal(np.diff(ro), rl):
            raise ValueError("refs must hold one string of ref_len bytes per variant")
    h, hm = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib().ms_genome_apply_alleles(genome.h, ptr(ci, ctypes.c_int32), ptr(ps, ctypes.c_int64), ptr(rl, ctypes.c_int32),
                                        ab.ctypes.data_as(ctypes.c_char_p), ptr(ao, ctypes.c_int64),
                                        None if rb is None else rb.ctypes.data_as(ctypes.c_char_p), ci.size,
                                        MS_APPLY_SKIP_MISMATCH if skip_mismatch else 0, ctypes.byref(h), ctypes.byref(hm)))
    g = ResidentGenome.__new__(ResidentGenome)
    g.h = h
    g.names = list(genome.names)
    g.index = dict(genome.index)
    g._host = None
    g._packed = None
    g._device_made = True
    lm = LiftMap(hm)
    sizes = lm.alt_sizes
    g.offsets = np.zeros(len(g.names) + 1, dtype=np.int64)
    np.cumsum(sizes, out=g.offsets[1:])
    g.chrom_sizes = {n: int(s) for n, s in zip(g.names, sizes)}
    return g, lm


def personal_dims():
    """ms_debug_personal_dims: dict(block_bases, stage_variants, lift_block) -- the output bases of one splice block, the applied variants
    a block stages in LDS, the queries per block of the lift kernel.  Constants of the build; no device."""
    out = np.zeros(4, dtype=np.int32)
    check(lib().ms_debug_personal_dims(ptr(out, ctypes.c_int32)))
    return dict(zip(("block_bases", "stage_variants", "lift_block"), out.tolist()[:3]))


class PinnedBuffer:
    """Page-locked host memory (ms_host_alloc) as a uint8 numpy array: uploads from it run at the full link rate and
    overlap with scans."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        check(lib().ms_host_alloc(int(nbytes), ctypes.byref(p)))
        self.ptr = p
        self.nbytes = int(nbytes)

    @property
    def array(self):
        """uint8 view of the block; every view (and anything numpy derives from it) keeps the block alive.  Made on demand: a
        view stored on the object itself would be a reference cycle and delay the release of the pinned memory to the cycle GC."""
        if not getattr(self, "ptr", None):
            raise ValueError("the pinned buffer is closed")
        return _owned_array(self.ptr.value, ctypes.c_uint8, self.nbytes, np.uint8, self)

    def close(self):
        if getattr(self, "ptr", None):
            lib().ms_host_free(self.ptr)
            self.ptr = None

    __del__ = close


class Stream:
    """ms_stream: batches of regions (or spans of a window sweep) flow through upload + pack | scan | copy-out, the three
    stages of consecutive batches overlapped on one device.  Results come back in submission order."""

    def __init__(self, pwms, strand_mask=3, flags=0, depth=2):
        self.pwms = pwms                               # keep alive
        self.flags = int(flags)
        h = ctypes.c_void_p()
        check(lib().ms_stream_create(pwms.h, int(strand_mask), int(flags), int(depth), ctypes.byref(h)))
        self.h = h
        n = ctypes.c_int()
        check(lib().ms_stream_capacity(self.h, ctypes.byref(n)))
        self.capacity = n.value
        self._keep = []                                # buffers borrowed by batches still in flight

    @property
    def in_flight(self):
        n = ctypes.c_int()
        check(lib().ms_stream_in_flight(self.h, ctypes.byref(n)))
        return n.value

    def submit(self, bases, offsets, counts_only=False):
        bases = np.ascontiguousarray(bases, dtype=np.uint8) if isinstance(bases, np.ndarray) else np.frombuffer(bytes(bases), dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or offsets.size < 1 or int(offsets[0]) != 0 or int(offsets[-1]) != bases.size:
            raise ValueError("offsets must run from 0 to the number of bases")
        fn = lib().ms_stream_submit_counts_only if counts_only else lib().ms_stream_submit
        check(fn(self.h, ctypes.c_void_p(bases.ctypes.data), ptr(offsets, ctypes.c_int64), offsets.size - 1))
        self._keep.append(bases)

    def submit_regions(self, genome, chrom_idx, starts, ends):
        """A batch of regions of a ResidentGenome (chromosome indices, 0-based half-open): cut on the device while the previous
        batch is scanned."""
        ci = np.ascontiguousarray(chrom_idx, dtype=np.int32)
        st = np.ascontiguousarray(starts, dtype=np.int64)
        en = np.ascontiguousarray(ends, dtype=np.int64)
        if not (ci.size == st.size == en.size):
            raise ValueError("chrom_idx, starts and ends must have one entry per region")
        check(lib().ms_stream_submit_regions(self.h, genome.h, ptr(ci, ctypes.c_int32), ptr(st, ctypes.c_int64), ptr(en, ctypes.c_int64), ci.size))
        self._keep.append(genome)

    def submit_span(self, bases, window, stride):
        bases = np.ascontiguousarray(bases, dtype=np.uint8) if isinstance(bases, np.ndarray) else np.frombuffer(bytes(bases), dtype=np.uint8)
        check(lib().ms_stream_submit_span(self.h, ctypes.c_void_p(bases.ctypes.data), bases.size, int(window), int(stride)))
        self._keep.append(bases)

    def next(self):
        """The oldest batch's ScanResult (hits already on the host), or None when nothing is in flight."""
        if self.in_flight == 0:
            self._keep.clear()
            return None
        h = ctypes.c_void_p()
        try:
            check(lib().ms_stream_next(self.h, ctypes.byref(h)))
        finally:
            if self._keep:
                self._keep.pop(0)                      # returned or failed: either way the batch no longer borrows its buffer
        return _fence_exact_only(ScanResult(h, self.pwms.n), self.pwms, MS_SCAN_EXACT_ONLY if self.flags & MS_STREAM_EXACT_ONLY else 0) if h.value else None

    def stats(self):
        """ms_stream_stats: per stage {batches, ms_work, ms_wait_in, ms_wait_out}; the stage that waits least bounds the stream."""
        out = (ctypes.c_double * 12)()
        check(lib().ms_stream_stats(self.h, out))
        return {name: {"batches": int(out[4 * k]), "ms_work": out[4 * k + 1], "ms_wait_in": out[4 * k + 2], "ms_wait_out": out[4 * k + 3]}
                for k, name in enumerate(("upload", "scan", "copy_out"))}

    def close(self):
        if getattr(self, "h", None):
            lib().ms_stream_free(self.h)
            self.h = None
            self._keep = []

    __del__ = close


def merge_hits(parts, n_pwms):
    """Concatenate per-batch hit dicts into the single-call result: parts = [(hits dict, seq_idx offset), ...] in batch
    order.  Within a motif the reference orders hits by sequence index (cscore.c:336-390), so motif p's hits are batch 0's
    hits of p, then batch 1's, ... -- one slice copy per (motif, batch)."""
    offs = np.zeros(n_pwms + 1, dtype=np.int64)
    for h, _ in parts:
        offs[1:] += np.diff(h["motif_offsets"])
    offs = np.concatenate([[0], np.cumsum(offs[1:])]).astype(np.int64)
    n = int(offs[-1])
    out = {"seq_idx": np.empty(n, np.int64), "pos": np.empty(n, np.int64), "score": np.empty(n, np.float64),
           "strand": np.empty(n, np.int8)}
    cur = offs[:-1].copy()
    for h, shift in parts:
        mo = h["motif_offsets"]
        for p in np.nonzero(np.diff(mo))[0].tolist():
            a, b = int(mo[p]), int(mo[p + 1])
            d = int(cur[p])
            out["seq_idx"][d:d + b - a] = h["seq_idx"][a:b] + shift
            out["pos"][d:d + b - a] = h["pos"][a:b]
            out["score"][d:d + b - a] = h["score"][a:b]
            out["strand"][d:d + b - a] = h["strand"][a:b]
            cur[p] += b - a
    out["motif"] = np.repeat(np.arange(n_pwms, dtype=np.int32), np.diff(offs))
    out["motif_offsets"] = offs
    return out


def scan_stream(pwms, batches, strand_mask=3, flags=0, depth=2, packed=False, stage_stats=None, host_pack=False):
    """Generator: push (bases, offsets) batches -- or (ResidentGenome, chrom_idx, starts, ends) batches of a genome that sits in
    HBM -- through a Stream, yield each batch's ScanResult in order (the caller closes them).  Keeps the stream as full as its capacity allows.  stage_stats: a dict that receives Stream.stats() at the end.
    A (bases, offsets, True) batch is COUNTS ONLY (ms_stream_submit_counts_only): its hits stay on the device, only the per-motif
    region counts are read -- what the reference does with the control regions (cli/scan.py:81-89 -> stats.py:29-31).
    host_pack: the upload stage packs the batches on host threads (MS_STREAM_HOST_PACK: no kernel beside the scan).
    packed: True / 16 = the 16-byte compact copy-out, 12 = the 12-byte form for every batch that fits it (MS_STREAM_PACKED12)."""
    st = Stream(pwms, strand_mask, flags | (MS_STREAM_PACKED12 if packed == 12 else (MS_STREAM_PACKED if packed else 0)) | (MS_STREAM_HOST_PACK if host_pack else 0), depth)
    try:
        for batch in batches:                             # (bases, offsets), or (ResidentGenome, chrom_idx, starts, ends)
            while st.in_flight >= st.capacity:
                yield st.next()
            if len(batch) == 4:
                st.submit_regions(*batch)
            else:
                st.submit(*batch)                         # (bases, offsets) or (bases, offsets, counts_only)
        while st.in_flight:
            yield st.next()
        if stage_stats is not None:
            stage_stats.update(st.stats())
    finally:
        st.close()


def sweep_stream(pwms, chroms, window, stride, max_span_bases, strand_mask=3, flags=0, depth=2, spans=None, packed=False,
                 stage_stats=None):
    """Host-streamed window sweep over a whole genome (BASELINE configs[4]): chroms = list of uint8 arrays (host memory,
    ideally pinned); the windows [k*stride, k*stride + window) of every chromosome are cut into spans of at most
    max_span_bases bases (ms_sweep_spans), and the spans flow through a Stream (upload + pack | scan-once + hand-out |
    copy-out).  Yields (span, ScanResult) in order; span = (chrom, begin, end, first_window, n_windows) and the result's
    seq_idx counts windows from the span's first one: add span[3] for the genome-wide window index.  `spans` restricts
    the sweep to a subset (a rank's share)."""
    if spans is None:
        spans = sweep_spans([len(c) for c in chroms], window, stride, max_span_bases)
    st = Stream(pwms, strand_mask, flags | (MS_STREAM_PACKED12 if packed == 12 else (MS_STREAM_PACKED if packed else 0)), depth)
    try:
        pending = []
        for sp in spans:
            while st.in_flight >= st.capacity:
                yield pending.pop(0), st.next()
            st.submit_span(chroms[sp[0]][sp[1]:sp[2]], window, stride)
            pending.append(sp)
        while st.in_flight:
            yield pending.pop(0), st.next()
        if stage_stats is not None:
            stage_stats.update(st.stats())
    finally:
        st.close()


def sweep_spans(chrom_lens, window, stride, max_span_bases):
    """ms_sweep_spans: [(chrom, begin, end, first_window, n_windows), ...] for the windows [k*stride, k*stride + window)
    of every chromosome, in spans of at most max_span_bases bases."""
    lens = np.ascontiguousarray(chrom_lens, dtype=np.int64)
    n = ctypes.c_int64()
    check(lib().ms_sweep_spans(ptr(lens, ctypes.c_int64), len(lens), int(window), int(stride), int(max_span_bases), None, 0,
                               ctypes.byref(n)))
    arr = (Span * max(n.value, 1))()
    check(lib().ms_sweep_spans(ptr(lens, ctypes.c_int64), len(lens), int(window), int(stride), int(max_span_bases), arr, n.value,
                               ctypes.byref(n)))
    return [(a.chrom, a.begin, a.end, a.first_window, a.n_windows) for a in arr[:n.value]]


def scan_regions_once(pwms, genome, chrom_idx, starts, ends, strand_mask=3, flags=MS_SCAN_DEFAULT):
    """ms_scan_regions_once: the regions (chromosome indices, 0-based half-open, clipped; any order, any overlap) of a
    ResidentGenome, with the result of extract() + scan() over them but every base of their union scored once."""
    ci = np.ascontiguousarray(chrom_idx, dtype=np.int32)
    st = np.ascontiguousarray(starts, dtype=np.int64)
    en = np.ascontiguousarray(ends, dtype=np.int64)
    if not (len(ci) == len(st) == len(en)):
        raise ValueError("chrom / start / end must have the same length")
    h = ctypes.c_void_p()
    check(lib().ms_scan_regions_once(pwms.h, genome.h, ptr(ci, ctypes.c_int32), ptr(st, ctypes.c_int64), ptr(en, ctypes.c_int64),
                                     len(ci), int(strand_mask), int(flags), ctypes.byref(h)))
    return _fence_exact_only(ScanResult(h, pwms.n), pwms, int(flags))


def union_bases(chrom_idx, starts, ends):
    """Bases covered by at least one region (the regions' union), by chromosome-wise interval merging."""
    ci = np.asarray(chrom_idx, dtype=np.int64)
    st = np.asarray(starts, dtype=np.int64)
    en = np.asarray(ends, dtype=np.int64)
    if len(ci) == 0:
        return 0
    o = np.lexsort((st, ci))
    c, s, e = ci[o], st[o], en[o]
    big = int(e.max()) + 1
    reach = np.maximum.accumulate(e + c * big) - c * big          # furthest end seen so far on this chromosome
    prev = np.concatenate([[0], reach[:-1]])
    prev[np.concatenate([[True], c[1:] != c[:-1]])] = 0
    return int(np.maximum(e - np.maximum(s, prev), 0).sum())


def score(pwms, seqs, strand_mask=3):
    out = np.zeros((pwms.n, seqs.n_seqs), dtype=np.float64)
    check(lib().ms_score(pwms.h, seqs.h, int(strand_mask), ptr(out, ctypes.c_double)))
    return out


def score_ranks(pwms, seqs, ranks, strand_mask=3):
    """out[p][k] = the score at 0-based rank ranks[k] of PWM p's scores over all sequences, descending."""
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    out = np.zeros((pwms.n, len(ranks)), dtype=np.float64)
    check(lib().ms_score_ranks(pwms.h, seqs.h, int(strand_mask), ptr(ranks, ctypes.c_int64), len(ranks),
                               ptr(out, ctypes.c_double)))
    return out


def release_scratch():
    check(lib().ms_debug_release_scratch())


def dedup_keep(motif_offsets, widths, seq_idx, pos, score_, strand):
    motif_offsets = np.ascontiguousarray(motif_offsets, dtype=np.int64)
    widths = np.ascontiguousarray(widths, dtype=np.int32)
    seq_idx = np.ascontiguousarray(seq_idx, dtype=np.int64)
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    score_ = np.ascontiguousarray(score_, dtype=np.float64)
    strand = np.ascontiguousarray(strand, dtype=np.int8)
    keep = np.ones(len(seq_idx), dtype=np.uint8)
    check(lib().ms_dedup_hits(ptr(motif_offsets, ctypes.c_int64), len(widths), ptr(widths, ctypes.c_int32),
                              ptr(seq_idx, ctypes.c_int64), ptr(pos, ctypes.c_int64), ptr(score_, ctypes.c_double),
                              ptr(strand, ctypes.c_int8), ptr(keep, ctypes.c_uint8)))
    return keep.astype(bool)
