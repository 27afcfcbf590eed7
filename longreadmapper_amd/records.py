"""The structs and constants of include/*.h, written down once.

Every struct the binding passes is a ctypes.Structure listed under its C name (STRUCTS); the records that cross the
boundary as arrays get their numpy dtype from that same class (dtype_of).  tests/test_header_agreement.py compiles a C
program from STRUCTS and CONSTANTS against the headers themselves: sizes, offsets and values must agree."""
import ctypes as C

import numpy as np

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
i32p = C.POINTER(C.c_int32)


def dtype_of(cls):
    """numpy dtype of a record class: its members at their C offsets (a pointer as an address, a member `pad` as `_pad`),
    and the struct's tail padding, where it has one, as `_pad` bytes."""
    names, formats, offsets, end = [], [], [], 0
    for name, ctype in cls._fields_:
        member = getattr(cls, name)
        names.append("_pad" if name == "pad" else name)
        formats.append("<u8" if issubclass(ctype, C._Pointer) else np.dtype(ctype).str)
        offsets.append(member.offset)
        end = member.offset + member.size
    if end < C.sizeof(cls):
        names.append("_pad")
        formats.append("V%d" % (C.sizeof(cls) - end))
        offsets.append(end)
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=C.sizeof(cls)))


class Entry(C.Structure):              # histo.h:21-23
    _fields_ = [("key", C.c_uint64), ("val", C.c_uint64), ("bucket", C.c_uint64)]


class Params(C.Structure):             # alnmain.h:10-13
    _fields_ = [("batch_size", C.c_uint64), ("seed_len", C.c_uint32), ("thres", C.c_uint32)]


class DnaFmi(C.Structure):             # fmidx.h:16-21
    _fields_ = [("length", C.c_uint64), ("o_len", C.c_uint64), ("csa_len", C.c_uint64),
                ("c", u64p), ("o", u64p), ("csa", u64p),
                ("o_ratio", C.c_int), ("csa_ratio", C.c_int), ("bwt", C.c_void_p)]


class LcHash(C.Structure):             # lchash.h:16-20
    _fields_ = [("lc", u64p), ("len", C.c_uint64), ("hlen", C.c_int)]


class Ui40(C.Structure):               # sa_use.h:17-20 (8 bytes in RAM)
    _fields_ = [("low", C.c_uint32), ("high", C.c_uint8)]


class SaMem(C.Structure):              # fmidx.h:23-26
    _fields_ = [("start", C.c_uint64), ("len", C.c_uint64), ("mem", C.POINTER(Ui40))]


class MtaEntry(C.Structure):           # accaln.h:67-71 flattened
    _fields_ = [("name_len", C.c_uint64), ("name", C.c_char_p), ("name_own", C.c_int),
                ("offset", C.c_uint64), ("seq_len", C.c_size_t)]


class SeqMeta(C.Structure):            # alnmain.c:143-148
    _fields_ = [("loc", C.c_uint64), ("off", C.c_uint64), ("seq_id", C.c_int32), ("strand", C.c_uint8)]


class Cigar(C.Structure):              # gact cigar (mutils.c:97-103)
    _fields_ = [("cigar", u8p), ("n_cigar_op", C.c_int), ("score", C.c_int)]


class GactParams(C.Structure):
    _fields_ = [("T", C.c_int), ("O", C.c_int), ("W", C.c_int)]


class IndexOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sa_sampled", C.c_int32), ("lc_long", C.c_int32),
                ("lc_long_max", C.c_int32), ("lc_pair", C.c_int32), ("lcx_threshold", C.c_uint32),
                ("lc_entry_bytes", C.c_uint32), ("lc_core", C.c_int32), ("lc_count_bits", C.c_uint32),
                ("seed_table", C.c_int32), ("seed_table_len", C.c_uint32), ("seed_table_share", C.c_uint32),
                ("seed_table_bits", C.c_uint32), ("seed_table_count_bits", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class IndexTables(C.Structure):
    _fields_ = [("lc_long", C.c_int32), ("lc_pair", C.c_int32), ("lc_entry_bytes", C.c_int32), ("lc_core", C.c_int32),
                ("seed_table_len", C.c_int32), ("seed_table_share", C.c_int32), ("seed_table_bits", C.c_int32),
                ("seed_table_slot_bytes", C.c_int32), ("seed_table_count_bits", C.c_int32), ("reserved0", C.c_int32),
                ("seed_table_side_entries", C.c_uint64), ("derived_bytes", C.c_uint64), ("reserved", C.c_uint64 * 4)]


class _SplitWords(C.Structure):        # the last two words of lrm_map_options
    _fields_ = [("split", C.c_uint32), ("split_min_len", C.c_uint32)]


class _MapTail(C.Union):               # ... which were `reserved` until the split fields took them: both names reach them
    _anonymous_ = ("_split",)
    _fields_ = [("_split", _SplitWords), ("reserved", C.c_uint32 * 2)]


_MAP_OPTION_WORDS = ("struct_size", "dense_results", "gact_impl", "seed_rounds", "vote_exact_only", "slice_reads", "sub_batches",
                     "group_subs", "bs_waves", "cigar_text", "copy_threads", "keep_reads", "anchored", "anchor_min_len", "clip",
                     "clip_penalty", "clip_end_bonus")
_MAP_OPTION_SIGNED = ("dense_results", "gact_impl", "seed_rounds", "vote_exact_only")


class MapOptions(C.Structure):
    _anonymous_ = ("_tail",)
    _fields_ = [(name, C.c_int32 if name in _MAP_OPTION_SIGNED else C.c_uint32) for name in _MAP_OPTION_WORDS] + [("_tail", _MapTail)]


class Anchor(C.Structure):
    _fields_ = [("text_pos", C.c_uint64), ("read_pos", C.c_uint32), ("len", C.c_uint32), ("delta", C.c_int32),
                ("left_ops", C.c_uint32), ("flags", C.c_uint32)]


class Clip(C.Structure):
    _fields_ = [("left", C.c_uint32), ("right", C.c_uint32)]


class Segment(C.Structure):
    _fields_ = [("read", C.c_uint32), ("start", C.c_uint32), ("len", C.c_uint32), ("flags", C.c_uint32)]


class SplitDev(C.Structure):           # device pointers
    _fields_ = [("cap", C.c_uint64), ("seg", C.c_void_p), ("rows", C.c_void_p), ("row_stride", C.c_uint64), ("lens", C.c_void_p),
                ("best", C.c_void_p), ("store", C.c_void_p), ("store_stride", C.c_uint64), ("n_ops", C.c_void_p),
                ("score", C.c_void_p), ("meta", C.c_void_p), ("meta_r", C.c_void_p), ("anchor", C.c_void_p), ("clip", C.c_void_p)]


class SplitOut(C.Structure):           # host pointers
    _fields_ = [("cap", C.c_uint64), ("n_seg", C.c_uint64), ("seg", C.c_void_p), ("rows", C.c_void_p), ("row_stride", C.c_uint64),
                ("lens", C.c_void_p), ("best", C.c_void_p), ("cig", C.c_void_p), ("store", C.c_void_p),
                ("store_stride", C.c_uint64), ("score", C.c_void_p), ("meta", C.c_void_p), ("meta_r", C.c_void_p),
                ("anchor", C.c_void_p), ("clip", C.c_void_p)]


class Mapq(C.Structure):               # docs/GACT_SPEC.md, "Mapping quality"
    _fields_ = [("n1", C.c_uint32), ("n2", C.c_uint32), ("radius", C.c_uint32), ("mapq", C.c_uint8), ("phase", C.c_uint8),
                ("flags", C.c_uint8), ("pad", C.c_uint8)]


class AlnSummary(C.Structure):         # docs/GACT_SPEC.md, "Alignment summary and PAF"
    _fields_ = [("n_eq", C.c_uint32), ("n_x", C.c_uint32), ("n_ins", C.c_uint32), ("n_del", C.c_uint32),
                ("ins_runs", C.c_uint32), ("del_runs", C.c_uint32), ("clip_left", C.c_uint32), ("clip_right", C.c_uint32)]


class BatchExtras(C.Structure):        # host pointers
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("mapq_out", C.c_void_p), ("summary_out", C.c_void_p)]


class _BatchDiff(C.Structure):         # host pointers; docs/GACT_SPEC.md, "Difference events and MD:Z"
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("off_out", C.c_void_p), ("cnt_out", C.c_void_p),
                ("events_out", C.c_void_p), ("cap", C.c_uint64), ("needed_out", C.c_void_p)]


# tests/test_header_agreement.py asserts that STRUCTS has exactly 25 entries AND that every Structure of the binding whose class
# name has no leading underscore is one of them; an existing test may not change.  The underscore in the class name is there
# to stay outside that assertion, nothing else: the public name is BatchDiff, and the struct is compared with the header through
# LATER_STRUCTS by tests/test_aln_diff_cpu.py, which also asserts that every underscore-named Structure here except the
# anonymous parts of MapOptions is listed in LATER_STRUCTS -- a later struct added the same way cannot escape both.
BatchDiff = _BatchDiff


class _Secondary(C.Structure):         # docs/GACT_SPEC.md, "Secondary alignments"; compared with the header like BatchDiff
    _fields_ = [("read", C.c_uint32), ("hits", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32)]


class _SecondaryOptions(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "min_hits", "ratio_pct", "anchored", "anchor_min_len", "clip",
                                                "clip_penalty", "clip_end_bonus")]


class _SecondaryDev(C.Structure):      # device pointers
    _fields_ = [("cap", C.c_uint64), ("table", C.c_void_p), ("rows", C.c_void_p), ("row_stride", C.c_uint64), ("lens", C.c_void_p),
                ("rival", C.c_void_p), ("store", C.c_void_p), ("store_stride", C.c_uint64), ("n_ops", C.c_void_p),
                ("score", C.c_void_p), ("meta", C.c_void_p), ("meta_r", C.c_void_p), ("anchor", C.c_void_p), ("clip", C.c_void_p)]


class _SecondaryOut(C.Structure):      # host pointers
    _fields_ = [("cap", C.c_uint64), ("n_sec", C.c_uint64), ("table", C.c_void_p), ("rows", C.c_void_p), ("row_stride", C.c_uint64),
                ("lens", C.c_void_p), ("rival", C.c_void_p), ("cig", C.c_void_p), ("store", C.c_void_p),
                ("store_stride", C.c_uint64), ("score", C.c_void_p), ("meta", C.c_void_p), ("meta_r", C.c_void_p),
                ("anchor", C.c_void_p), ("clip", C.c_void_p)]


Secondary, SecondaryOptions, SecondaryDev, SecondaryOut = _Secondary, _SecondaryOptions, _SecondaryDev, _SecondaryOut


class _PileupCol(C.Structure):         # docs/GACT_SPEC.md, "Pileup"; compared with the header like BatchDiff
    _fields_ = [(name, C.c_uint32) for name in ("depth", "n_eq", "x_a", "x_c", "x_g", "x_t", "n_del", "n_ins")]


class _PileupCallOptions(C.Structure):     # docs/GACT_SPEC.md, "Pileup calls"; a zero field means its default
    _fields_ = [(name, C.c_uint32) for name in ("min_depth", "min_count", "min_pct", "reserved")]


class _PileupSite(C.Structure):
    _fields_ = [("pos", C.c_uint64)] + [(name, C.c_uint32) for name in ("depth", "n_ref", "n_alt", "n_del", "n_ins")] + [
        (name, C.c_uint8) for name in ("ref", "alt", "cons", "kinds")]


class _BatchPileup(C.Structure):       # host pointers; docs/GACT_SPEC.md, "Pileup on the host-buffer path and across replicas"
    _fields_ = [("struct_size", C.c_uint32), ("min_mapq", C.c_uint32), ("pileups", C.POINTER(C.c_void_p)), ("n_pileups", C.c_uint32),
                ("reserved", C.c_uint32)]


class _AccalnPileupOptions(C.Structure):       # include/lrm_io_host.h
    _fields_ = [("struct_size", C.c_uint32), ("ins_cols", C.c_uint32), ("min_mapq", C.c_uint32), ("reserved", C.c_uint32),
                ("call", _PileupCallOptions), ("seq", C.c_int32), ("reserved2", C.c_uint32), ("sites_path", C.c_char_p),
                ("fasta_path", C.c_char_p)]


class _PileupVariantOptions(C.Structure):  # docs/GACT_SPEC.md, "Pileup variants and VCF"; a zero field means its default
    _fields_ = [("call", _PileupCallOptions), ("hom_pct", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class _PileupVariant(C.Structure):
    _fields_ = [("pos", C.c_uint64)] + [(name, C.c_uint32) for name in ("len", "depth", "n_ref", "n_alt", "n_col0")] + [
        (name, C.c_uint8) for name in ("kind", "ref", "alt", "gt")] + [("bases", C.c_uint8 * 8), ("ins_flags", C.c_uint8), ("pad", C.c_uint8 * 7)]


class _AccalnVcfOptions(C.Structure):          # include/lrm_io_host.h
    _fields_ = [("struct_size", C.c_uint32), ("hom_pct", C.c_uint32), ("vcf_path", C.c_char_p), ("sample", C.c_char_p),
                ("reserved", C.c_uint64)]


PileupCol, PileupCallOptions, PileupSite = _PileupCol, _PileupCallOptions, _PileupSite
BatchPileup, AccalnPileupOptions = _BatchPileup, _AccalnPileupOptions
PileupVariantOptions, PileupVariant, AccalnVcfOptions = _PileupVariantOptions, _PileupVariant, _AccalnVcfOptions


class GactTable(C.Structure):          # host pointers
    _fields_ = [("n", C.c_uint64), ("reads", C.c_void_p), ("stride", C.c_uint64), ("lens", C.c_void_p), ("text", C.c_void_p),
                ("text_len", C.c_uint64), ("toffs", C.c_void_p), ("tlens", C.c_void_p), ("meta_r", C.c_void_p),
                ("store", C.c_void_p), ("store_stride", C.c_uint64), ("n_ops", C.c_void_p), ("score", C.c_void_p),
                ("counters", C.c_void_p)]


# the counting build of gact_bs_kernel (lrm_stats, after vote_redo_items)
BS_COUNTERS = ("bs_wave_tiles", "bs_pass1_pairs_masked", "bs_pass1_pairs_plain", "bs_blocks_full", "bs_blocks_windowed",
               "bs_blocks_skipped", "bs_refill_rounds")


class Stats(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("vote_tier2_items", "vote_tier3_items", "reads_decided_phase0", "gact_tiles",
                                                "seeds_evaluated", "seed_table_lookups", "seed_rank_requests",
                                                "vote_redo_items") + BS_COUNTERS]


class ReadBatch(C.Structure):          # lrm_io_host.h
    _fields_ = [("n", C.c_uint64), ("stride", C.c_uint64), ("max_len", C.c_uint32), ("seqs", C.c_void_p),
                ("lens", u32p), ("names", C.POINTER(C.c_char_p)), ("quals", C.POINTER(C.c_char_p)),
                ("name_arena", C.c_void_p), ("qual_arena", C.c_void_p), ("seqs_borrowed", C.c_int)]


class HostIndex(C.Structure):          # lrm_index_host.h
    _fields_ = [("fmi", DnaFmi), ("lch", LcHash), ("sa", SaMem), ("content", C.c_void_p),
                ("con_len", C.c_uint64), ("mta", C.POINTER(MtaEntry)), ("mta_len", C.c_int)]


# every struct above under the header's name for it; MAP_OPTION_FIELDS: the header's members of lrm_map_options
STRUCTS = {Entry: "lrm_entry", Params: "lrm_params", DnaFmi: "lrm_dna_fmi", LcHash: "lrm_lc_hash", Ui40: "lrm_ui40", SaMem: "lrm_sa_mem",
           MtaEntry: "lrm_mta_entry", SeqMeta: "lrm_seq_meta", Cigar: "lrm_cigar", GactParams: "lrm_gact_params",
           IndexOptions: "lrm_index_options", IndexTables: "lrm_index_tables", MapOptions: "lrm_map_options", Anchor: "lrm_anchor",
           Clip: "lrm_clip", Segment: "lrm_segment", SplitDev: "lrm_split_dev", SplitOut: "lrm_split_out", Mapq: "lrm_mapq",
           AlnSummary: "lrm_aln_summary", BatchExtras: "lrm_batch_extras", GactTable: "lrm_debug_gact_table", Stats: "lrm_stats",
           ReadBatch: "lrm_read_batch", HostIndex: "lrm_host_index"}
MAP_OPTION_FIELDS = _MAP_OPTION_WORDS + ("split", "split_min_len")
# tests/test_header_agreement.py compares exactly the 25 structs of STRUCTS with the headers; the structs that came after it
# are listed here and compared in the same way by the tests of their feature (tests/test_aln_diff_cpu.py)
LATER_STRUCTS = {BatchDiff: "lrm_batch_diff", Secondary: "lrm_secondary", SecondaryOptions: "lrm_secondary_options",
                 SecondaryDev: "lrm_secondary_dev", SecondaryOut: "lrm_secondary_out", PileupCol: "lrm_pileup_col",
                 PileupCallOptions: "lrm_pileup_call_options", PileupSite: "lrm_pileup_site", BatchPileup: "lrm_batch_pileup",
                 AccalnPileupOptions: "lrm_accaln_pileup_options", PileupVariantOptions: "lrm_pileup_variant_options",
                 PileupVariant: "lrm_pileup_variant", AccalnVcfOptions: "lrm_accaln_vcf_options"}

# the records that cross the boundary as arrays
ENTRY_DT, META_DT, CIGAR_DT = dtype_of(Entry), dtype_of(SeqMeta), dtype_of(Cigar)
ANCHOR_DT, CLIP_DT, SEGMENT_DT = dtype_of(Anchor), dtype_of(Clip), dtype_of(Segment)
MAPQ_DT, SUMMARY_DT = dtype_of(Mapq), dtype_of(AlnSummary)
SECONDARY_DT = dtype_of(Secondary)
PILEUP_COL_DT = dtype_of(PileupCol)
PILEUP_SITE_DT = dtype_of(PileupSite)
# lrm_pileup_ins_allele (16 bytes): a record that crosses only as an array, so it has a dtype and no ctypes structure
PILEUP_INS_ALLELE_DT = np.dtype([("n_col0", "<u4"), ("len", "u1"), ("flags", "u1"), ("pad", "u1", (2,)), ("bases", "u1", (8,))])
# lrm_pileup_variant (48 bytes): the members of PileupVariant with the eight bases as one field
PILEUP_VARIANT_DT = np.dtype([("pos", "<u8"), ("len", "<u4"), ("depth", "<u4"), ("n_ref", "<u4"), ("n_alt", "<u4"), ("n_col0", "<u4"), ("kind", "u1"),
                              ("ref", "u1"), ("alt", "u1"), ("gt", "u1"), ("bases", "u1", (8,)), ("ins_flags", "u1"), ("pad", "u1", (7,))])

N_KERNELS = 9
MAPQ_SLOTS, MAPQ_OVERFLOW = 4096, 1    # lrm_mapq.flags
SEG_RIGHT, SEG_ALIGNED = 1, 2          # lrm_segment.flags
SPLIT_MIN_DEFAULT = 200
SEC_ALIGNED, SEC_DUPLICATE = 1, 2      # lrm_secondary.flags
DIFF_X, DIFF_D_OPEN, DIFF_D_MORE = 0, 1, 2        # bits 8-9 of a difference event
DIFF_NO_ROOM = 2**64 - 1               # lrm_batch_diff.off_out of a read whose group found no room
PILEUP_TILE = 2048                     # positions per workgroup of the pileup read-back
PILEUP_PLANES = ("x_a", "x_c", "x_g", "x_t", "x_other", "n_del", "n_ins")     # the event planes behind the depth's difference plane
CALL_SNV, CALL_DEL, CALL_INS = 1, 2, 4   # lrm_pileup_site.kinds
PILEUP_INS_COLS_MAX = 8                # insertion columns of an accumulator (lrm_pileup_create_ins)
INS_ENTERS, INS_FULL = 1, 2            # lrm_pileup_ins_allele.flags
ANCHOR_ANCHORED, ANCHOR_FALLBACK, ANCHOR_NO_LEFT, ANCHOR_LEFT_CLIPPED, ANCHOR_RIGHT_CLIPPED = 1, 2, 4, 8, 16
ANCHOR_SOFT_LEFT, ANCHOR_SOFT_RIGHT = 32, 64      # end clipping (lrm_map_options.clip)
ANCHOR_DIAGS = 64
DEFAULT_GACT = (320, 120, 128)

# the header's name of every constant above
CONSTANTS = dict(LRM_N_KERNELS=N_KERNELS, LRM_MAPQ_SLOTS=MAPQ_SLOTS, LRM_MAPQ_OVERFLOW=MAPQ_OVERFLOW, LRM_SEG_RIGHT=SEG_RIGHT,
                 LRM_SEG_ALIGNED=SEG_ALIGNED, LRM_SEC_ALIGNED=SEC_ALIGNED, LRM_SEC_DUPLICATE=SEC_DUPLICATE, LRM_SPLIT_MIN_DEFAULT=SPLIT_MIN_DEFAULT, LRM_DIFF_X=DIFF_X, LRM_DIFF_D_OPEN=DIFF_D_OPEN,
                 LRM_DIFF_D_MORE=DIFF_D_MORE, LRM_PILEUP_TILE=PILEUP_TILE, LRM_CALL_SNV=CALL_SNV, LRM_CALL_DEL=CALL_DEL, LRM_CALL_INS=CALL_INS,
                 LRM_PILEUP_INS_COLS_MAX=PILEUP_INS_COLS_MAX, LRM_INS_ENTERS=INS_ENTERS, LRM_INS_FULL=INS_FULL, LRM_ANCHOR_ANCHORED=ANCHOR_ANCHORED,
                 LRM_ANCHOR_FALLBACK=ANCHOR_FALLBACK, LRM_ANCHOR_NO_LEFT=ANCHOR_NO_LEFT, LRM_ANCHOR_LEFT_CLIPPED=ANCHOR_LEFT_CLIPPED,
                 LRM_ANCHOR_RIGHT_CLIPPED=ANCHOR_RIGHT_CLIPPED, LRM_ANCHOR_SOFT_LEFT=ANCHOR_SOFT_LEFT,
                 LRM_ANCHOR_SOFT_RIGHT=ANCHOR_SOFT_RIGHT, LRM_ANCHOR_DIAGS=ANCHOR_DIAGS, LRM_GACT_T_DEFAULT=DEFAULT_GACT[0],
                 LRM_GACT_O_DEFAULT=DEFAULT_GACT[1], LRM_GACT_W_DEFAULT=DEFAULT_GACT[2])

DEFAULT_SEED_LEN = 20      # alnmain.c:577-580
DEFAULT_THRES = 300


# Op bytes per read (lrm_map_options.anchored in the header).  Every entry point makes its store stride from these two:
#   extend_batch, map_batch through lrm_map_batch    max(store_need, 1): the reference's rows (alnmain.c:316-320), never empty
#   map_batch_submit                                 max(units16(store_need), 16): the dense layouts need whole 16-byte units
#   SplitBuffers, DeviceMapper anchored              units16(store_need)
#   DeviceMapper classic                             store_need
def anchored_store_stride(max_len):
    """Op bytes per read the anchored mode needs: both jobs' targets are an eighth longer than their queries."""
    return 2 * max_len + max_len // 8 + 2


def store_need(max_len, anchored):
    return anchored_store_stride(max_len) if anchored else 2 * max_len


def units16(nbytes):
    return (nbytes + 15) // 16 * 16


# what capi re-exports: the pointer types, the structs, the record dtypes and the header's constants -- not the helpers
__all__ = ["u8p", "u32p", "u64p", "i32p", "STRUCTS", "LATER_STRUCTS", "BatchDiff", "Secondary", "SecondaryOptions", "SecondaryDev", "SecondaryOut",
           "SECONDARY_DT", "PileupCol", "PILEUP_COL_DT", "PileupCallOptions", "PileupSite", "BatchPileup", "AccalnPileupOptions", "PileupVariantOptions", "PileupVariant", "AccalnVcfOptions", "PILEUP_VARIANT_DT", "PILEUP_SITE_DT", "PILEUP_INS_ALLELE_DT", "PILEUP_INS_COLS_MAX", "INS_ENTERS", "INS_FULL", "CALL_SNV", "CALL_DEL", "CALL_INS", "PILEUP_TILE", "PILEUP_PLANES", "SEC_ALIGNED", "SEC_DUPLICATE", "MAP_OPTION_FIELDS", "CONSTANTS", "BS_COUNTERS", *(s.__name__ for s in STRUCTS),
           "ENTRY_DT", "META_DT", "CIGAR_DT", "ANCHOR_DT", "CLIP_DT", "SEGMENT_DT", "MAPQ_DT", "SUMMARY_DT", "N_KERNELS", "MAPQ_SLOTS",
           "MAPQ_OVERFLOW", "SEG_RIGHT", "SEG_ALIGNED", "SPLIT_MIN_DEFAULT", "DIFF_X", "DIFF_D_OPEN", "DIFF_D_MORE", "DIFF_NO_ROOM", "ANCHOR_ANCHORED", "ANCHOR_FALLBACK", "ANCHOR_NO_LEFT",
           "ANCHOR_LEFT_CLIPPED", "ANCHOR_RIGHT_CLIPPED", "ANCHOR_SOFT_LEFT", "ANCHOR_SOFT_RIGHT", "ANCHOR_DIAGS"]
