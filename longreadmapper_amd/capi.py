"""ctypes binding of liblrm_accel.so (include/lrm_accel.h, include/lrm_index_host.h).

This is what a Python host would bind: the entry points here, the structs (which mirror the
reference's own: accaln.h / alnmain.h / fmidx.h / lchash.h / histo.h) in records.py.  There is
no fallback: if the library is missing the import of this module fails loudly.
"""
import ctypes as C
import os

from . import _build
from .records import *  # noqa: F401,F403  (every struct, record dtype and constant of the headers: capi.Entry, capi.META_DT, ...)

# every symbol include/*.h declares: (restype, argtypes)
SYMBOLS = {
    "lrm_last_error": (C.c_char_p, []),
    "lrm_free": (None, [C.c_void_p]),
    "lrm_abi_version": (C.c_int, []),
    "lrm_device_count": (C.c_int, []),
    "lrm_index_blob_bytes": (C.c_uint64, [C.c_uint64, C.c_int, C.c_int]),
    "lrm_index_pack_blob": (C.c_int, [C.POINTER(DnaFmi), C.POINTER(LcHash), C.POINTER(SaMem), C.c_void_p,
                                      C.c_uint64, C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_uint64]),
    "lrm_index_upload": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(DnaFmi), C.POINTER(LcHash),
                                   C.POINTER(SaMem), C.c_void_p, C.c_uint64, C.POINTER(MtaEntry), C.c_int, C.c_int]),
    "lrm_index_pack_device": (C.c_int, [C.POINTER(DnaFmi), C.POINTER(LcHash), C.POINTER(SaMem), C.c_void_p,
                                        C.c_uint64, C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_uint64, C.c_int]),
    "lrm_index_options_init": (None, [C.POINTER(IndexOptions)]),
    "lrm_map_options_init": (None, [C.POINTER(MapOptions)]),
    "lrm_index_blob_bytes_opt": (C.c_uint64, [C.c_uint64, C.c_int, C.c_int, C.POINTER(IndexOptions)]),
    "lrm_index_pack_blob_opt": (C.c_int, [C.POINTER(DnaFmi), C.POINTER(LcHash), C.POINTER(SaMem), C.c_void_p,
                                          C.c_uint64, C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_uint64,
                                          C.POINTER(IndexOptions)]),
    "lrm_index_pack_device_opt": (C.c_int, [C.POINTER(DnaFmi), C.POINTER(LcHash), C.POINTER(SaMem), C.c_void_p,
                                            C.c_uint64, C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_uint64, C.c_int,
                                            C.POINTER(IndexOptions)]),
    "lrm_index_upload_opt": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(DnaFmi), C.POINTER(LcHash),
                                       C.POINTER(SaMem), C.c_void_p, C.c_uint64, C.POINTER(MtaEntry), C.c_int,
                                       C.POINTER(C.c_int), C.c_int, C.POINTER(IndexOptions)]),
    "lrm_index_adopt_device_opt": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_int,
                                             C.POINTER(IndexOptions)]),
    "lrm_index_upload_blob_opt": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_int,
                                            C.POINTER(IndexOptions)]),
    "lrm_index_set_map_options": (C.c_int, [C.c_void_p, C.POINTER(MapOptions)]),
    "lrm_index_get_tables": (C.c_int, [C.c_void_p, C.POINTER(IndexTables)]),
    "lrm_map_batch_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, Params, GactParams,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(MapOptions), C.POINTER(C.c_void_p)]),
    "lrm_map_batch_submit_mapq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, Params, GactParams,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(MapOptions), C.c_void_p, C.POINTER(C.c_void_p)]),
    "lrm_map_batch_submit_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, Params, GactParams,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(MapOptions), C.POINTER(BatchExtras), C.POINTER(C.c_void_p)]),
    "lrm_map_batch_submit_ex2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, Params, GactParams,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(MapOptions), C.POINTER(BatchExtras), C.POINTER(BatchDiff), C.POINTER(C.c_void_p)]),
    "lrm_map_batch_submit_ex3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, Params, GactParams,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(MapOptions), C.POINTER(BatchExtras), C.POINTER(BatchDiff), C.POINTER(BatchPileup),
                                           C.POINTER(C.c_void_p)]),
    "lrm_map_batch_wait": (C.c_int, [C.c_void_p]),
    "lrm_aln_diff_offsets_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "lrm_aln_diff_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "lrm_aln_diff_host": (C.c_int64, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]),
    "lrm_md_format": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int]),
    "lrm_pileup_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_uint64]),
    "lrm_pileup_free": (None, [C.c_void_p]),
    "lrm_pileup_bytes": (C.c_uint64, [C.c_void_p]),
    "lrm_pileup_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lrm_pileup_add_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]),
    "lrm_pileup_read_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "lrm_pileup_add_host": (None, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]),
    "lrm_pileup_cols_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]),
    "lrm_pileup_format": (C.c_int64, [C.POINTER(MtaEntry), C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int64]),
    "lrm_pileup_sites_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "lrm_pileup_sites_host": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "lrm_pileup_sites_format": (C.c_int64, [C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64]),
    "lrm_debug_pileup_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "lrm_pileup_create_ins": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32]),
    "lrm_pileup_ins_cols": (C.c_uint32, [C.c_void_p]),
    "lrm_pileup_ins_read_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "lrm_pileup_polish_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "lrm_pileup_site_alleles_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "lrm_pileup_ins_add_host": (None, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]),
    "lrm_pileup_polish_host": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    "lrm_pileup_ins_allele_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "lrm_debug_pileup_ins_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "lrm_pileup_create_replica": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32]),
    "lrm_pileup_merge_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrm_debug_pileup_merge_staged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "lrm_pileup_sites_format_ins": (C.c_int64, [C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64]),
    "lrm_pileup_variants_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "lrm_pileup_variants_host": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    "lrm_pileup_variants_format_vcf": (C.c_int64, [C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64]),
    "lrm_vcf_header": (C.c_int64, [C.POINTER(MtaEntry), C.c_int, C.c_char_p, C.c_void_p, C.c_int64]),
    "lrm_aln_summary_host": (None, [C.c_void_p, C.c_int, C.POINTER(AlnSummary)]),
    "lrm_aln_summary_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_void_p]),
    "lrm_debug_reload_env": (C.c_int, [C.c_void_p]),
    "lrm_debug_set_vote_limits": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "lrm_debug_set_mapq_slots": (C.c_int, [C.c_void_p, C.c_uint32]),
    "lrm_debug_gact_impl": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, GactParams, C.c_int, C.c_void_p,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]),
    "lrm_debug_gact_jobs": (C.c_int, [C.POINTER(GactTable), GactParams, C.c_int, C.c_uint32, C.c_int, C.c_int]),
    "lrm_index_adopt_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_int]),
    "lrm_index_upload_blob": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_int]),
    "lrm_index_free": (None, [C.c_void_p]),
    "lrm_seed_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, Params, C.c_void_p]),
    "lrm_extend_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                   GactParams, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "lrm_map_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, Params, GactParams,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrm_host_alloc": (C.c_void_p, [C.c_uint64]),
    "lrm_host_free": (None, [C.c_void_p]),
    "lrm_host_register": (C.c_int, [C.c_void_p, C.c_uint64]),
    "lrm_host_unregister": (C.c_int, [C.c_void_p]),
    "lrm_pair_end": (C.c_int, [C.c_int, C.c_void_p]),
    "lrm_index_upload_multi": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(DnaFmi), C.POINTER(LcHash),
                                         C.POINTER(SaMem), C.c_void_p, C.c_uint64, C.POINTER(MtaEntry), C.c_int,
                                         C.POINTER(C.c_int), C.c_int]),
    "lrm_index_replicas": (C.c_int, [C.c_void_p]),
    "lrm_index_replica": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lrm_result_flags": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrm_result_flags_mapq": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "lrm_workspace_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                       C.c_uint32]),
    "lrm_workspace_free": (None, [C.c_void_p]),
    "lrm_workspace_bytes": (C.c_uint64, [C.c_void_p]),
    "lrm_seed_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                     C.c_uint32, Params, C.c_void_p, C.c_void_p]),
    "lrm_seed_batch_mapq_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                          C.c_uint32, Params, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrm_extend_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                       C.c_uint32, C.c_void_p, GactParams, C.c_void_p, C.c_uint64, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrm_extend_batch_anchored_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                C.c_uint32, C.c_void_p, GactParams, C.c_void_p, C.c_uint64, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "lrm_extend_batch_clipped_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                               C.c_uint32, C.c_void_p, GactParams, C.c_void_p, C.c_uint64, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                               C.c_uint32, C.c_void_p, C.c_void_p]),
    "lrm_split_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, u64p]),
    "lrm_clip_of_cigar": (C.c_int, [C.POINTER(Cigar), C.c_int, u32p, u32p]),
    "lrm_split_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, Params,
                                      GactParams, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SplitDev), u64p,
                                      C.c_void_p]),
    "lrm_split_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  Params, GactParams, C.POINTER(MapOptions), C.POINTER(SplitOut)]),
    "lrm_rival_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, Params, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                C.c_void_p, C.c_void_p]),
    "lrm_rival_host": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(Entry), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.POINTER(Entry)]),
    "lrm_secondary_plan": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, u64p]),
    "lrm_secondary_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, Params, GactParams, C.POINTER(SecondaryOptions),
                                          C.POINTER(SecondaryDev), u64p, C.c_void_p]),
    "lrm_secondary_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      Params, GactParams, C.POINTER(MapOptions), C.POINTER(SecondaryOptions), C.POINTER(SecondaryOut)]),
    "lrm_accaln_secondary": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, Params, GactParams, C.c_int, C.c_long, u64p, u64p,
                                       C.POINTER(MapOptions), C.POINTER(SecondaryOptions)]),
    "lrm_debug_anchor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(Anchor)]),
    "lrm_workspace_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats), C.c_void_p]),
    "lrm_debug_vote_results": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "lrm_workspace_set_counting": (C.c_int, [C.c_void_p, C.c_int]),
    "lrm_workspace_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "lrm_workspace_timing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrm_kernel_name": (C.c_char_p, [C.c_int]),
    "lrm_debug_seed_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]),
    "lrm_debug_rccl_selftest": (C.c_int, [C.c_int, C.c_uint64]),
    "lrm_debug_gact": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, GactParams, C.c_void_p,
                                 C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]),
    # lrm_index_host.h
    "lrm_cat_from_seqs": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), u64p, C.c_int, C.c_uint64,
                                    C.POINTER(C.c_void_p), u64p, C.POINTER(C.POINTER(MtaEntry))]),
    "lrm_sa_build": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "lrm_host_index_build": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(MtaEntry), C.c_int, C.c_int, C.c_int,
                                       C.POINTER(HostIndex)]),
    "lrm_host_index_free": (None, [C.POINTER(HostIndex)]),
    "lrm_host_index_write": (C.c_int, [C.POINTER(HostIndex), C.c_char_p]),
    "lrm_host_index_read": (C.c_int, [C.c_char_p, C.POINTER(HostIndex)]),
    "lrm_fmi_write": (C.c_int, [C.POINTER(DnaFmi), C.c_char_p]),
    "lrm_fmi_read": (C.c_int, [C.POINTER(DnaFmi), C.c_char_p]),
    "lrm_lc_write": (C.c_int, [C.c_char_p, C.POINTER(LcHash)]),
    "lrm_lc_read": (C.c_int, [C.c_char_p, C.POINTER(LcHash)]),
    "lrm_sa5_write": (C.c_int, [C.c_char_p, C.c_void_p, C.c_uint64]),
    "lrm_sa5_read": (C.c_int64, [C.c_char_p, C.c_void_p, C.c_uint64]),
    "lrm_mta_write": (C.c_int, [C.c_char_p, C.POINTER(MtaEntry), C.c_int]),
    "lrm_mta_read": (C.c_int, [C.c_char_p, C.POINTER(C.POINTER(MtaEntry))]),
    "lrm_mta_free": (None, [C.POINTER(MtaEntry), C.c_int]),
    "lrm_accidx": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_uint64]),
    # lrm_io_host.h
    "lrm_reader_open": (C.c_int, [C.POINTER(C.c_void_p), C.c_char_p]),
    "lrm_reader_next": (C.c_int64, [C.c_void_p, C.c_uint64, C.POINTER(ReadBatch)]),
    "lrm_reader_next_into": (C.c_int64, [C.c_void_p, C.c_uint64, C.POINTER(ReadBatch), C.c_void_p, C.c_uint64]),
    "lrm_read_batch_free": (None, [C.POINTER(ReadBatch)]),
    "lrm_reader_close": (None, [C.c_void_p]),
    "lrm_parse_cigar": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "lrm_sam_header": (C.c_void_p, [C.POINTER(MtaEntry), C.c_int, C.c_long, u64p]),
    "lrm_sam_format": (C.c_void_p, [C.POINTER(ReadBatch), C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint64, u64p]),
    "lrm_sam_format_split": (C.c_void_p, [C.POINTER(ReadBatch), C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(SplitOut), u64p]),
    "lrm_sam_format_mapq": (C.c_void_p, [C.POINTER(ReadBatch), C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(SplitOut), C.c_void_p, u64p]),
    "lrm_sam_format_md": (C.c_void_p, [C.POINTER(ReadBatch), C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(SplitOut), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, u64p]),
    "lrm_sam_format_secondary": (C.c_void_p, [C.POINTER(ReadBatch), C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(SplitOut), C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SecondaryOut), u64p]),
    "lrm_accaln_md": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, Params, GactParams, C.c_int, C.c_long, u64p, u64p,
                                C.POINTER(MapOptions), C.c_int, C.c_int]),
    "lrm_paf_format": (C.c_void_p, [C.POINTER(ReadBatch), C.POINTER(MtaEntry), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, u64p]),
    "lrm_accaln_paf": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, Params, GactParams, C.c_int, u64p, u64p,
                                 C.POINTER(MapOptions), C.c_int]),
    "lrm_accaln": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, Params, GactParams, C.c_int, C.c_long, u64p, u64p]),
    "lrm_accaln_opt": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, Params, GactParams, C.c_int, C.c_long, u64p, u64p,
                                 C.POINTER(MapOptions)]),
    "lrm_accaln_mapq": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, Params, GactParams, C.c_int, C.c_long, u64p, u64p,
                                  C.POINTER(MapOptions), C.c_int]),
    "lrm_accaln_pileup": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, Params, GactParams, C.c_int, C.c_long, u64p, u64p,
                                    C.POINTER(MapOptions), C.c_int, C.POINTER(AccalnPileupOptions)]),
    "lrm_accaln_pileup_vcf": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, Params, GactParams, C.c_int, C.c_long, u64p, u64p,
                                        C.POINTER(MapOptions), C.c_int, C.POINTER(AccalnPileupOptions), C.POINTER(AccalnVcfOptions)]),
}


def _load():
    # torch bundles its own libamdhip64.so.7 (+ HSA runtime).  Two HIP runtimes in one process do
    # not both get the GPU, and the dynamic linker keys on the SONAME: whichever is loaded first
    # serves both.  torch.distributed / torch tensors are this package's device plumbing, so let
    # torch's runtime win: import it before liblrm_accel.so pulls in /opt/rocm's.
    try:
        import torch  # noqa: F401
    except Exception:      # torch absent: the system runtime is the only one
        pass
    path = _build.ACCEL_LIB
    if not os.path.exists(path):
        path = _build.build_accel()
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def index_options(**kw):
    """lrm_index_options with the automatic choices, then the given fields (None = automatic)."""
    o = IndexOptions()
    lib.lrm_index_options_init(C.byref(o))
    for k, v in kw.items():
        if k not in _INDEX_OPTION_NAMES:      # (a ctypes structure takes any attribute: a misspelt option would be dropped)
            raise AttributeError("lrm_index_options has no field %r" % k)
        if v is not None:
            setattr(o, k, v)
    return o


_INDEX_OPTION_NAMES = frozenset(n for n, _ in IndexOptions._fields_) - {"struct_size", "reserved"}


def map_options(**kw):
    o = MapOptions()
    lib.lrm_map_options_init(C.byref(o))
    for k, v in kw.items():
        if v is not None:
            getattr(o, k)             # AttributeError for a field the struct does not have
            setattr(o, k, v)
    return o


class LrmError(RuntimeError):
    pass


def failure(what="", **fields):
    """The LrmError of a call that failed: lrm_last_error() behind `what`; fields (rc, n_seg) become its attributes."""
    e = LrmError("%s: %s" % (what or "liblrm_accel", lib.lrm_last_error().decode(errors="replace")))
    e.__dict__.update(fields)
    return e


def check(rc, what=""):
    if rc < 0:
        raise failure(what)
    return rc
