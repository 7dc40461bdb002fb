"""ctypes binding of libfsgpu.so (include/fsgpu.h + include/fshost.h) used by bench.py and the tests.

This is plumbing, not the product: every call goes through the C ABI of the shared library (HIP kernels + C++ host
code).  There is NO CPU fallback -- if the library or a GPU is missing the calls raise.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfsgpu.so")

HIT_DT = np.dtype([("id", np.uint32), ("score", np.int32)])
SWRES_DT = np.dtype([("score", np.int32), ("qEnd", np.int32), ("dbEnd", np.int32), ("word", np.int32)])
RESULT_DT = np.dtype([("dbKey", np.uint32), ("score", np.int32), ("qcov", np.float32), ("dbcov", np.float32),
                      ("seqId", np.float32), ("_pad0", np.uint32), ("eval", np.float64), ("alnLength", np.uint32),
                      ("qStartPos", np.int32), ("qEndPos", np.int32), ("qLen", np.uint32), ("dbStartPos", np.int32),
                      ("dbEndPos", np.int32), ("dbLen", np.uint32), ("backtraceOff", np.uint32),
                      ("backtraceLen", np.uint32), ("_pad1", np.uint32)])


class Params(C.Structure):
    _fields_ = [("maxResListLen", C.c_int), ("minDiagScoreThr", C.c_int), ("compBiasCorrection", C.c_int),
                ("prefCompBiasScale", C.c_float), ("alignmentType", C.c_int), ("alnCompBiasScale", C.c_float),
                ("gapOpen", C.c_int), ("gapExtend", C.c_int), ("evalThr", C.c_double), ("covThr", C.c_float),
                ("covMode", C.c_int), ("addBacktrace", C.c_int), ("maxAccept", C.c_int), ("maxRejected", C.c_int),
                ("seqIdThr", C.c_float), ("alnLenThr", C.c_int), ("seqIdMode", C.c_int), ("altAlignment", C.c_int), ("skipUndefinedDiagonals", C.c_int)]


class KmerIndexParams(C.Structure):
    _fields_ = [("kmerSize", C.c_int32), ("spaced", C.c_int32), ("kmerThr", C.c_int32), ("maskLowerCase", C.c_int32),
                ("maskNrepeats", C.c_int32)]


class KmerSearchParams(C.Structure):
    _fields_ = [("maxResListLen", C.c_int32), ("minDiagScoreThr", C.c_int32), ("bins", C.c_int32), ("kmerScoreOnly", C.c_int32),
                ("maxDbMatches", C.c_int64), ("foundDiagonalsSize", C.c_int64), ("l2CacheSize", C.c_uint64)]


class KmerQuery(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("kmerThr", C.c_void_p), ("profile", C.c_void_p), ("L", C.c_int32),
                ("reserved", C.c_int32), ("identity", C.c_int64)]


class KmerProfileQuery(C.Structure):
    """fsgpu_kmer_profile_query"""
    _fields_ = [("seq", C.c_void_p), ("scores", C.c_void_p), ("profile", C.c_void_p), ("L", C.c_int32), ("kmerThr", C.c_int32),
                ("identity", C.c_int64)]


class GaplessQuery(C.Structure):
    """fsgpu_gapless_query"""
    _fields_ = [("pssm", C.c_void_p), ("L", C.c_int32), ("scoreCap", C.c_int32), ("identityId", C.c_int64)]


KMER_HIT_DT = np.dtype([("id", np.uint32), ("score", np.int32), ("diag", np.uint16), ("pad", np.uint16)])
SW_DT = SWRES_DT      # fsgpu_swres under the name the oracle bindings use
DIAG_PAIR_DT = np.dtype([("query", np.uint32), ("target", np.uint32), ("diagonal", np.int32)])      # fsgpu_diag_pair
DIAG_RES_DT = np.dtype([("score", np.int32), ("startPos", np.int32), ("endPos", np.int32), ("revScore", np.int32), ("diagonalLen", np.int32),
                        ("identicalAA", np.int32), ("status", np.int32), ("reserved", np.int32)])   # fsgpu_diag_res
FSGPU_DIAG_OK, FSGPU_DIAG_NO_OVERLAP, FSGPU_DIAG_UNDEFINED, FSGPU_DIAG_BAD_ID = 0, 1, 2, 3
FSGPU_MAX_SEQ_LEN = 65535      # include/fsgpu.h: the longest query or target an entry takes
FSGPU_E_ARG, FSGPU_E_UNSUPPORTED = -1, -4


class BtQuery(C.Structure):
    """fsgpu_bt_query"""
    _fields_ = [("qAA", C.c_void_p), ("q3Di", C.c_void_p), ("cbAA", C.c_void_p), ("cbSS", C.c_void_p), ("L", C.c_int32), ("reserved", C.c_int32)]


class BtTask(C.Structure):
    """fsgpu_bt_task"""
    _fields_ = [("query", C.c_uint32), ("target", C.c_uint32), ("qEnd", C.c_int32), ("dbEnd", C.c_int32), ("score", C.c_int32)]


class BtRes(C.Structure):
    """fsgpu_bt_res"""
    _fields_ = [("status", C.c_int32), ("qStart", C.c_int32), ("dbStart", C.c_int32), ("identicalAA", C.c_int32), ("btLen", C.c_int32),
                ("blockSizes", C.c_int32), ("btOff", C.c_uint64)]


class PbtQuery(C.Structure):
    """fsgpu_pbt_query"""
    _fields_ = [("pAA", C.c_void_p), ("p3Di", C.c_void_p), ("lettersAA", C.c_void_p), ("L", C.c_int32), ("reserved", C.c_int32)]


class LddtQuery(C.Structure):
    """fsgpu_lddt_query"""
    _fields_ = [("ca", C.c_void_p), ("L", C.c_int32), ("reserved", C.c_int32)]


class LddtTask(C.Structure):
    """fsgpu_lddt_task"""
    _fields_ = [("query", C.c_uint32), ("tLen", C.c_int32), ("tOff", C.c_uint64), ("qStart", C.c_int32), ("dbStart", C.c_int32),
                ("btOff", C.c_uint64), ("btLen", C.c_uint32), ("reserved", C.c_uint32), ("outOff", C.c_uint64)]


class TmTask(C.Structure):
    """fsgpu_tm_task"""
    _fields_ = [("query", C.c_uint32), ("tLen", C.c_int32), ("tOff", C.c_uint64), ("qStart", C.c_int32), ("dbStart", C.c_int32),
                ("btOff", C.c_uint64), ("btLen", C.c_uint32), ("scoreD8", C.c_float), ("d0Std", C.c_float), ("d0", C.c_float),
                ("d0Search", C.c_float), ("reserved", C.c_uint32)]


class TmResult(C.Structure):
    """fsgpu_tm_result"""
    _fields_ = [("nPairs", C.c_int32), ("source", C.c_int32), ("score", C.c_float * 2), ("rms", C.c_float), ("t", C.c_float * 3), ("u", C.c_float * 9)]


TM_SRC_NONE, TM_SRC_KABSCH, TM_SRC_SEARCH1, TM_SRC_SEARCH2, TM_SRC_EXACT = range(5)          # FSGPU_TM_SRC_*


FSGPU_E_ARG, FSGPU_E_HIP, FSGPU_E_NODB, FSGPU_E_UNSUPPORTED, FSGPU_E_NOMEM, FSGPU_E_OUTPUT = -1, -2, -3, -4, -5, -6
SCAN_GUARD = 0xA5A5A5A5          # what Context.sw_scan_c fills its output buffers with before the call


class FsgpuError(RuntimeError):
    pass


_lib = None


def lib():
    """Loads libfsgpu.so; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FsgpuError(f"{LIB_PATH} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, f32, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double
    sig = {
        "fsgpu_create": (i32, [i32, C.POINTER(vp)]),
        "fsgpu_destroy": (None, [vp]),
        "fsgpu_last_error": (C.c_char_p, [vp]),
        "fsgpu_clone": (i32, [vp, C.POINTER(vp)]),
        "fsgpu_device": (i32, [vp]),
        "fsgpu_device_count": (i32, []),
        "fsgpu_live_devices": (i32, []),
        "fsgpu_block_backtrace": (i32, [vp, vp, vp, vp, vp, C.POINTER(BtQuery), i32, C.POINTER(BtTask), i32, i32, i32, C.POINTER(BtRes), C.POINTER(C.c_void_p)]),
        "fsgpu_block_backtrace_footprint": (i32, [vp, i32]),
        "fsgpu_profile_backtrace": (i32, [vp, C.POINTER(PbtQuery), i32, C.POINTER(BtTask), i32, i32, i32, C.POINTER(BtRes), C.POINTER(C.c_void_p)]),
        "fsgpu_profile_backtrace_last": (None, [vp, vp]),
        "fsgpu_lddt_batch": (i32, [vp, C.POINTER(LddtQuery), i32, C.POINTER(LddtTask), i32, vp, u64, vp, u64, vp, vp, u64]),
        "fsgpu_tm_batch": (i32, [vp, C.POINTER(LddtQuery), i32, C.POINTER(TmTask), i32, vp, u64, vp, u64, vp, vp, vp]),
        "fsgpu_tm_superpose_batch": (i32, [vp, C.POINTER(LddtQuery), i32, C.POINTER(TmTask), i32, vp, u64, vp, u64, i32, C.POINTER(TmResult)]),
        "fshost_tm_exact_params": (None, [i32, vp]),
        "fshost_tm_exact_finish": (f64, [i32, f32, f32, vp]),
        "fshost_tm_params": (None, [i32, vp]),
        "fshost_tm_finish": (f64, [i32, f32, f32, i32]),
        "fshost_tm_normalization": (i32, [i32, i32, i32, i32]),
        "fshost_ca_decode": (i32, [vp, C.c_size_t, i32, vp]),
        "fshost_lddt_average": (f64, [vp, i32, C.POINTER(i32)]),
        "fshost_search_bind_ca": (i32, [vp, f32, vp, vp, vp]),
        "fshost_search_set_query_ca": (i32, [vp, i32, vp, vp]),
        "fshost_search_set_tm": (i32, [vp, f32, i32, i32]),
        "fsgpu_gapless_plan_items": (i64, [vp, C.c_uint32, i32, f64, vp, u64, vp]),
        "fsgpu_gapless_item_records": (i64, [vp, u64, vp, vp, C.c_uint32, vp]),
        "fsgpu_gapless_pair_halves": (i32, [vp, i32, vp, vp, vp]),
        "fsgpu_gapless_shape": (i32, [i32, C.POINTER(i32), C.POINTER(i32)]),
        "fsgpu_db_broadcast": (i32, [vp, C.POINTER(vp), i32, C.POINTER(i32)]),
        "fsgpu_rccl_selfcheck": (i32, [vp]),
        "fsgpu_stream": (vp, [vp]),
        "fsgpu_db_load": (i32, [vp, vp, vp, vp, vp, u64, u64]),
        "fsgpu_db_adopt_device": (i32, [vp, vp, vp, vp, vp, u64, u64]),
        "fsgpu_db_check_table": (i64, [vp, vp, u64, u64]),
        "fsgpu_db_size": (u64, [vp]),
        "fsgpu_db_residues": (u64, [vp]),
        "fsgpu_gapless_scan": (i32, [vp, vp, i32, i32, i32, i64, i32, vp, C.POINTER(i32)]),
        "fsgpu_gapless_scores": (i32, [vp, vp]),
        "fsgpu_gapless_launch": (i32, [vp, vp, i32, i32, i32, i64, i32]),
        "fsgpu_gapless_finish": (i32, [vp, vp, C.POINTER(i32)]),
        "fsgpu_sw_batch": (i32, [vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp, vp]),
        "fsgpu_sw_launch": (i32, [vp, vp, vp, vp, vp, i32, vp, i32, i32, i32]),
        "fsgpu_sw_finish": (i32, [vp, vp, vp]),
        "fsgpu_last_kernel_ms": (f64, [vp, i32]),
        "fsgpu_history_counters": (None, [vp, vp]),
        "fsgpu_sw_last_passes": (None, [vp, vp]),
        "fsgpu_sw3_last_plan": (None, [vp, vp]),
        "fsgpu_sw_kernel_counts": (None, [vp, vp]),
        "fsgpu_sw_shape": (i32, [i32, C.POINTER(i32), C.POINTER(i32)]),
        "fsgpu_kmer_index_build": (i32, [vp, vp, vp]),
        "fsgpu_kmer_index_entries": (u64, [vp]),
        "fsgpu_kmer_index_entry_bytes": (i32, [vp]),
        "fsgpu_kmer_index_get_params": (i32, [vp, C.POINTER(KmerIndexParams)]),
        "fsgpu_kmer_search": (i32, [vp, vp, vp, i32, vp, vp, vp, vp]),
        "fsgpu_kmer_index_copy": (i32, [vp, vp, vp, vp]),
        "fsgpu_kmer_row_copy": (i32, [vp, i32, vp, vp]),
        "fsgpu_kmer_last_counts": (None, [vp, vp]),
        "fsgpu_kmer_last_segments": (None, [vp, vp]),
        "fsgpu_kmer_batch_hint": (i32, [vp]),
        "fsgpu_kmer_plan_coarse": (i32, [vp, u64, C.c_uint32, vp, vp, C.c_uint32]),
        "fshost_kmer_query_prepare": (i32, [vp, vp, vp, i32, i32, f32, i32, i32, i32, vp, vp]),
        "fshost_kmer_threshold": (i32, [f32, i32]),
        "fshost_matrix_create": (vp, [i32, f32, f32]),
        "fshost_matrix_from_text": (vp, [C.c_char_p, f32, f32]),
        "fshost_matrix_from_scores": (vp, [vp, i32, vp]),
        "fshost_matrix_free": (None, [vp]),
        "fshost_matrix_size": (i32, [vp]),
        "fshost_matrix_scores": (C.POINTER(C.c_int16), [vp]),
        "fshost_matrix_background": (C.POINTER(C.c_double), [vp]),
        "fshost_matrix_encode": (None, [vp, C.c_char_p, i32, vp]),
        "fshost_matrix_letter": (C.c_char, [vp, i32]),
        "fshost_comp_bias": (None, [vp, vp, i32, f32, vp]),
        "fshost_round_bias": (None, [vp, i32, vp]),
        "fshost_prefilter_profile": (i32, [vp, vp, i32, i32, f32, vp, C.POINTER(i32)]),
        "fshost_align_profiles": (i32, [vp, vp, vp, vp, i32, i32, f32, vp, vp, vp, vp]),
        "fshost_evaluer_create": (vp, [C.c_char_p, u64]),
        "fshost_evaluer_free": (None, [vp]),
        "fshost_predict_mu_lambda": (None, [vp, vp, C.c_uint, i32, C.POINTER(f64), C.POINTER(f64)]),
        "fshost_evalue_corr": (f64, [vp, f64, f64, f64]),
        "fshost_evalue_score_cutoff": (i32, [vp, f64, f64, f64]),
        "fshost_params_default": (None, [C.POINTER(Params)]),
        "fshost_search_create": (vp, [vp, C.POINTER(Params), vp, C.c_char_p, vp, vp, vp, vp]),
        "fshost_search_free": (None, [vp]),
        "fshost_search_error": (C.c_char_p, [vp]),
        "fshost_search_prefilter": (i32, [vp, vp, i32, i64, vp]),
        "fshost_search_align": (i32, [vp, vp, vp, i32, i64, vp, i32, vp]),
        "fshost_search_align_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "fshost_search_exhaustive_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
        "fshost_search_exhaustive_survivors": (i32, [vp, vp, i32]),
        "fsgpu_sw_multi": (i32, [vp, vp, i32, i32, i32, vp, vp]),
        "fsgpu_sw_multi_dir": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "fsgpu_sw_multi_dir_c": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "fsgpu_sw_multi_c": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
        "fsgpu_sw_multi_dir_p": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "fsgpu_sw_multi_p": (i32, [vp, vp, i32, i32, i32, vp, vp]),
        "fshost_profile_decode": (i32, [vp, C.c_size_t, vp, vp, vp, vp, C.c_char_p, C.c_size_t]),
        "fshost_profile_bias": (i32, [vp, i32]),
        "fshost_search_prefilter_profile": (i32, [vp, vp, i32, i64, vp]),
        "fshost_search_prefilter_batch_profile": (i32, [vp, i32, vp, vp, vp, vp, vp]),
        "fshost_search_align_profile": (i32, [vp, vp, i64, vp, i32, vp]),
        "fshost_search_align_batch_profile": (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
        "fsgpu_sw_scan_c": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, u64, vp]),
        "fsgpu_sw_scan_last": (None, [vp, vp]),
        "fshost_search_backtrace": (C.c_char_p, [vp, vp]),
        "fshost_search_stats": (None, [vp, vp]),
        "fshost_search_backtrace_counts": (None, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "fshost_search_last_sw": (None, [vp, C.POINTER(vp), C.POINTER(vp)]),
        "fshost_block_backtrace": (i32, [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32),
                                         C.POINTER(C.c_uint), C.c_char_p, C.c_size_t]),
        "fshost_format_prefilter_hit": (C.c_size_t, [C.c_char_p, C.c_uint32, i32, i32]),
        "fshost_format_result": (C.c_size_t, [C.c_char_p, vp, C.c_char_p, i32]),
        "fsgpu_gapless_scan_multi": (i32, [vp, vp, i32, i32, i32, vp, vp]),
        "fsgpu_gapless_last_batch": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "fsgpu_gapless_scores_multi": (i32, [vp, i32, vp]),
        "fsgpu_sw_batch_seqs": (i32, [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp]),
        "fsgpu_diag_rescore": (i32, [vp, vp, vp, vp, vp, i32, vp, vp, vp, i64, vp]),
        "fshost_search_prefilter_batch": (i32, [vp, i32, vp, vp, vp, vp, vp]),
        "fshost_search_kmer_batch": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "fsgpu_kmer_search_profile": (i32, [vp, vp, vp, i32, vp, vp, vp, vp]),
        "fsgpu_kmer_profile_list_copy": (i32, [vp, i32, i32, vp, C.c_uint32, vp]),
        "fsgpu_kmer_profile_sort_rows": (i32, [vp, i32, vp]),
        "fshost_profile_decode_raw": (i32, [vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_char_p, C.c_size_t]),
        "fshost_kmer_threshold_profile": (i32, [f32, i32, i32]),
        "fshost_kmer_query_prepare_profile": (i32, [vp, C.c_size_t, i32, i32, i32, vp, vp, vp, vp, C.c_char_p, C.c_size_t]),
        "fshost_search_kmer_batch_profile": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "fshost_search_rescore_diagonal_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "fshost_banded_backtrace": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_uint), C.c_char_p, C.c_size_t]),
        "fshost_search_startpos_backtrace": (i32, [vp, vp, vp, i32, C.c_uint32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_uint), C.c_char_p, C.c_size_t]),
        "fshost_set_host_workers": (None, [i32]),
        "fshost_host_workers": (i32, []),
        "fshost_usable_cores": (i32, []),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def exported_symbols():
    return ["fsgpu_create", "fsgpu_destroy", "fsgpu_last_error", "fsgpu_device", "fsgpu_stream", "fsgpu_db_load",
            "fsgpu_db_adopt_device", "fsgpu_db_check_table", "fsgpu_db_size", "fsgpu_db_residues", "fsgpu_gapless_scan", "fsgpu_gapless_scores",
            "fsgpu_gapless_launch", "fsgpu_gapless_finish", "fsgpu_sw_batch", "fsgpu_sw_multi", "fsgpu_sw_multi_dir", "fsgpu_sw_multi_dir_c", "fsgpu_sw_multi_c", "fsgpu_sw_multi_dir_p", "fsgpu_sw_multi_p", "fsgpu_sw_launch", "fsgpu_sw_finish",
            "fsgpu_db_broadcast", "fsgpu_rccl_selfcheck", "fsgpu_device_count", "fsgpu_live_devices", "fsgpu_gapless_plan_items", "fsgpu_gapless_item_records", "fsgpu_gapless_pair_halves", "fsgpu_gapless_shape", "fsgpu_block_backtrace", "fsgpu_block_backtrace_footprint", "fsgpu_profile_backtrace", "fsgpu_profile_backtrace_last",
            "fsgpu_lddt_batch", "fsgpu_tm_batch", "fsgpu_tm_superpose_batch", "fsgpu_last_kernel_ms", "fsgpu_history_counters", "fsgpu_sw_last_passes", "fsgpu_sw3_last_plan", "fsgpu_kmer_index_build", "fsgpu_kmer_index_entries", "fsgpu_kmer_index_entry_bytes", "fsgpu_kmer_index_get_params", "fsgpu_kmer_search",
            "fsgpu_kmer_index_copy", "fsgpu_kmer_row_copy", "fsgpu_kmer_last_counts", "fsgpu_kmer_last_segments", "fsgpu_kmer_plan_coarse", "fsgpu_kmer_batch_hint",
            "fsgpu_kmer_search_profile", "fsgpu_kmer_profile_list_copy", "fsgpu_kmer_profile_sort_rows",
            "fsgpu_diag_rescore", "fsgpu_sw_batch_seqs", "fsgpu_sw_scan_c", "fsgpu_sw_scan_last", "fsgpu_sw_shape", "fsgpu_sw_kernel_counts"]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def db_check_table(offsets, lengths, nbytes):
    """fsgpu_db_check_table (host only): -1 for a table the load entries take, else the index of the first bad entry (len(lengths) for offsets[n])"""
    off = np.ascontiguousarray(offsets, np.uint64)
    ln = np.ascontiguousarray(lengths, np.int32)
    if len(off) != len(ln) + 1:
        raise FsgpuError("offsets must have one entry more than lengths")
    return int(lib().fsgpu_db_check_table(_ptr(off), _ptr(ln), len(ln), int(nbytes)))


def gapless_shape(L):
    """fsgpu_gapless_shape (host only): (row tiles, registers per lane R) of a query of L residues in the gapless scan"""
    n_tiles, R = C.c_int(0), C.c_int(0)
    if lib().fsgpu_gapless_shape(int(L), C.byref(n_tiles), C.byref(R)) != 0:
        raise FsgpuError(f"fsgpu_gapless_shape: no query of {L} residues")
    return n_tiles.value, R.value


SW_R_CLASSES = (1, 2, 3, 4, 6, 8)


def sw_shape(L):
    """fsgpu_sw_shape (host only): (row tiles, register rows per lane R) of a query of L residues in the profile path (k_sw / k_sw2)"""
    n_tiles, R = C.c_int(0), C.c_int(0)
    if lib().fsgpu_sw_shape(int(L), C.byref(n_tiles), C.byref(R)) != 0:
        raise FsgpuError(f"fsgpu_sw_shape: no query of {L} residues")
    return n_tiles.value, R.value


class Matrix:
    """fshost_matrix: bit-scaled substitution matrix (built-in 3Di / BLOSUM62 or user .out text)."""

    def __init__(self, which=None, bit_factor=2.0, score_bias=0.0, text=None):
        L = lib()
        self.h = L.fshost_matrix_from_text(text.encode(), bit_factor, score_bias) if text is not None else \
            L.fshost_matrix_create(which, bit_factor, score_bias)
        if not self.h:
            raise FsgpuError("matrix construction failed")
        self.n = L.fshost_matrix_size(self.h)

    def scores(self):
        return np.ctypeslib.as_array(lib().fshost_matrix_scores(self.h), (self.n * self.n,)).copy().reshape(self.n, self.n)

    def background(self):
        return np.ctypeslib.as_array(lib().fshost_matrix_background(self.h), (self.n,)).copy()

    def encode(self, s):
        out = np.zeros(len(s), np.uint8)
        lib().fshost_matrix_encode(self.h, s.encode(), len(s), _ptr(out))
        return out

    def comp_bias(self, seq, scale):
        seq = np.ascontiguousarray(seq, np.uint8)
        out = np.zeros(len(seq), np.float32)
        lib().fshost_comp_bias(self.h, _ptr(seq), len(seq), scale, _ptr(out))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            lib().fshost_matrix_free(self.h)
            self.h = None


def prefilter_profile(m3di, q3di, comp_bias=True, scale=0.15):
    q = np.ascontiguousarray(q3di, np.uint8)
    pssm = np.zeros((m3di.n, len(q)), np.int8)
    cap = C.c_int(0)
    rc = lib().fshost_prefilter_profile(m3di.h, _ptr(q), len(q), int(comp_bias), scale, _ptr(pssm), C.byref(cap))
    if rc != 0:
        raise FsgpuError(f"fshost_prefilter_profile rc={rc}")
    return pssm, cap.value


def align_profiles(mAA, m3Di, qAA, q3Di, comp_bias=True, scale=0.5):
    qa = np.ascontiguousarray(qAA, np.uint8)
    q3 = np.ascontiguousarray(q3Di, np.uint8)
    n, L_ = m3Di.n, len(q3)
    pAA = np.zeros((n, L_), np.int16)
    p3 = np.zeros((n, L_), np.int16)
    cbA = np.zeros(L_, np.int8)
    cbS = np.zeros(L_, np.int8)
    rc = lib().fshost_align_profiles(mAA.h, m3Di.h, _ptr(qa), _ptr(q3), L_, int(comp_bias), scale, _ptr(pAA), _ptr(p3),
                                     _ptr(cbA), _ptr(cbS))
    if rc != 0:
        raise FsgpuError(f"fshost_align_profiles rc={rc}")
    return pAA, p3, cbA, cbS


def kmer_threshold(sensitivity=9.5, kmer_size=6):
    return lib().fshost_kmer_threshold(sensitivity, kmer_size)


def kmer_query_prepare(m_kmer, m_ungapped, q3di, comp_bias=True, scale=0.15, kmer_thr=78, kmer_size=6, spaced=1):
    """-> (seq, kmerThr[nPos], profile[L,21]) for Context.kmer_search"""
    q = np.ascontiguousarray(q3di, np.uint8)
    L_ = len(q)
    thr = np.zeros(max(L_, 1), np.int16)
    prof = np.zeros((max(L_, 1), 21), np.int8)
    n = lib().fshost_kmer_query_prepare(m_kmer.h, m_ungapped.h, _ptr(q), L_, int(comp_bias), scale, kmer_thr, kmer_size, spaced,
                                        _ptr(thr), _ptr(prof))
    if n < 0:
        raise FsgpuError("fshost_kmer_query_prepare failed")
    return q, thr[:n].copy(), prof[:L_].copy()


class Evaluer:
    def __init__(self, db_residues, nn_path=None):
        self.h = lib().fshost_evaluer_create(nn_path.encode() if nn_path else None, db_residues)
        if not self.h:
            raise FsgpuError("cannot load e-value network")

    def mu_lambda(self, q3di, alphabet=21):
        q = np.ascontiguousarray(q3di, np.uint8)
        lam, mu = C.c_double(), C.c_double()
        lib().fshost_predict_mu_lambda(self.h, _ptr(q), len(q), alphabet, C.byref(lam), C.byref(mu))
        return lam.value, mu.value

    def evalue_corr(self, score, lam, mu):
        return lib().fshost_evalue_corr(self.h, float(score), lam, mu)

    def score_cutoff(self, lam, mu, eval_thr):
        """fshost_evalue_score_cutoff: the smallest integer score in [0, 32767] whose e-value does not exceed eval_thr, 32767 when none does"""
        return int(lib().fshost_evalue_score_cutoff(self.h, float(lam), float(mu), float(eval_thr)))

    def __del__(self):
        if getattr(self, "h", None):
            lib().fshost_evaluer_free(self.h)
            self.h = None


class Context:
    """fsgpu_ctx: one MI355X, one HIP stream, one resident target DB."""

    def __init__(self, device=0, _clone_of=None):
        h = C.c_void_p()
        if _clone_of is not None:
            rc = lib().fsgpu_clone(_clone_of.h, C.byref(h))
        else:
            rc = lib().fsgpu_create(device, C.byref(h))
        if rc != 0:
            raise FsgpuError(f"fsgpu_create({device}) rc={rc}: {lib().fsgpu_last_error(None).decode()}")
        self.h = h
        self._keep = None if _clone_of is None else _clone_of._keep

    def clone(self):
        """second context (own stream + scratch) sharing this context's resident DB"""
        return Context(_clone_of=self)

    def broadcast_db_to(self, others):
        """replicate this context's resident DB into contexts created on other devices (fsgpu_db_broadcast); returns
        True when RCCL carried the broadcast, False for peer copies"""
        arr = (C.c_void_p * len(others))(*[o.h for o in others])
        used = C.c_int(0)
        self._chk(lib().fsgpu_db_broadcast(self.h, arr, len(others), C.byref(used)), "fsgpu_db_broadcast")
        for o in others:
            o._keep = self._keep
        return bool(used.value)

    def rccl_selfcheck(self):
        """librccl on this device alone (one-rank communicator, 1 MiB broadcast in place); raises when it does not run"""
        self._chk(lib().fsgpu_rccl_selfcheck(self.h), "fsgpu_rccl_selfcheck")

    def _chk(self, rc, what):
        if rc != 0:
            raise FsgpuError(f"{what} rc={rc}: {lib().fsgpu_last_error(self.h).decode()}")

    def load_db(self, db):
        """db: foldseek_amd.synth.PaddedDB-like (data3di, dataaa|None, offsets[n+1], lengths[n])."""
        d3 = np.ascontiguousarray(db.data3di, np.uint8)
        da = None if db.dataaa is None else np.ascontiguousarray(db.dataaa, np.uint8)
        off = np.ascontiguousarray(db.offsets, np.uint64)
        ln = np.ascontiguousarray(db.lengths, np.int32)
        self._keep = (d3, da, off, ln)
        self._chk(lib().fsgpu_db_load(self.h, _ptr(d3), _ptr(da), _ptr(off), _ptr(ln), len(ln), d3.size), "fsgpu_db_load")

    def adopt_device_db(self, d3_ptr, da_ptr, off_ptr, len_ptr, n, nbytes):
        self._chk(lib().fsgpu_db_adopt_device(self.h, d3_ptr, da_ptr, off_ptr, len_ptr, n, nbytes), "fsgpu_db_adopt_device")

    @property
    def n(self):
        return lib().fsgpu_db_size(self.h)

    @property
    def residues(self):
        return lib().fsgpu_db_residues(self.h)

    @property
    def stream(self):
        return lib().fsgpu_stream(self.h)

    def gapless_scan(self, pssm, cap, min_score=30, identity=-1, max_res=1000):
        pssm = np.ascontiguousarray(pssm, np.int8)
        out = np.zeros(max_res, HIT_DT)
        nout = C.c_int(0)
        self._chk(lib().fsgpu_gapless_scan(self.h, _ptr(pssm), pssm.shape[1], cap, min_score, identity, max_res, _ptr(out),
                                           C.byref(nout)), "fsgpu_gapless_scan")
        return out[:nout.value]

    def gapless_scan_multi(self, queries, min_score=30, max_res=1000):
        """fsgpu_gapless_scan_multi called directly.  queries: list of (pssm int8 [21, L], cap, identity); a pssm of None goes down as a null
        profile of length 1.  Returns one hit array per query; gapless_scores_multi(i) then reads query i's score vector."""
        nq = len(queries)
        keep, arr = [], (GaplessQuery * max(nq, 1))()
        for i, (pssm, cap, identity) in enumerate(queries):
            p = None if pssm is None else np.ascontiguousarray(pssm, np.int8)
            buf = None if p is None else (p if p.size else np.zeros(1, np.int8))       # L = 0 still carries a pointer: the entry refuses the length
            keep.append(buf)
            arr[i].pssm = None if buf is None else buf.ctypes.data
            arr[i].L, arr[i].scoreCap, arr[i].identityId = (1 if p is None else p.shape[1]), int(cap), int(identity)
        out = np.zeros(max(1, nq * max_res), HIT_DT)
        nout = np.zeros(max(nq, 1), np.int32)
        self._chk(lib().fsgpu_gapless_scan_multi(self.h, C.cast(arr, C.c_void_p), nq, min_score, max_res, _ptr(out), _ptr(nout)),
                  "fsgpu_gapless_scan_multi")
        return [out[i * max_res:i * max_res + nout[i]].copy() for i in range(nq)]

    # ---- k-mer prefilter ------------------------------------------------------------------------------------
    def kmer_index_build(self, kmer_matrix, kmer_thr=78, kmer_size=6, spaced=1, mask_lower_case=1, mask_n_repeats=6):
        """kmer_matrix: Matrix(FSHOST_MAT_3DI, 8.0, -0.2) -- the prefilter's seeding matrix"""
        p = KmerIndexParams(kmer_size, spaced, kmer_thr, mask_lower_case, mask_n_repeats)
        sub = np.ascontiguousarray(kmer_matrix.scores(), np.int16)
        self._kmer_ip = p
        self._chk(lib().fsgpu_kmer_index_build(self.h, C.byref(p), _ptr(sub)), "fsgpu_kmer_index_build")

    @property
    def kmer_index_entries(self):
        return lib().fsgpu_kmer_index_entries(self.h)

    @property
    def kmer_index_entry_bytes(self):
        """4: an index entry is seqId << posBits | position in 32 bits; 8: seqId << 16 | position in 64 (0 before the index is built)"""
        return lib().fsgpu_kmer_index_entry_bytes(self.h)

    def kmer_index_params(self):
        """fsgpu_kmer_index_get_params: the parameters of the resident index as a dict; raises while there is none"""
        p = KmerIndexParams()
        rc = lib().fsgpu_kmer_index_get_params(self.h, C.byref(p))
        if rc != 0:
            raise FsgpuError(f"fsgpu_kmer_index_get_params rc={rc}: no k-mer index")
        return {n: int(getattr(p, n)) for n, _ in KmerIndexParams._fields_}

    def kmer_index_copy(self, nbytes_db):
        off = np.zeros(64000001, np.uint32)
        ent = np.zeros(max(1, self.kmer_index_entries), np.uint64)
        msk = np.zeros(max(1, nbytes_db), np.uint8)
        self._chk(lib().fsgpu_kmer_index_copy(self.h, _ptr(off), _ptr(ent), _ptr(msk)), "fsgpu_kmer_index_copy")
        return off, ent[:self.kmer_index_entries], msk[:nbytes_db]

    def kmer_index_reference_order(self, nbytes_db):
        """(offsets uint64[64e6+1], seqId uint32[], pos uint16[], masked) re-ordered to the reference's k-mer numbering
        (first3 + 8000*last3); the device keeps its table first-3-mer major (kmerDeviceIndex)."""
        off, ent, msk = self.kmer_index_copy(nbytes_db)
        k = np.arange(64000000, dtype=np.int64)
        kdev = (k % 8000) * 8000 + k // 8000
        size_dev = np.diff(off.astype(np.int64))
        size_ref = size_dev[kdev]
        roff = np.zeros(64000001, np.uint64)
        roff[1:] = np.cumsum(size_ref)
        nz = np.nonzero(size_ref)[0]
        starts = off.astype(np.int64)[kdev[nz]]
        lens = size_ref[nz]
        idx = np.repeat(starts - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))
        e = ent[idx]
        return roff, (e >> np.uint64(16)).astype(np.uint32), (e & np.uint64(0xffff)).astype(np.uint16), msk

    def kmer_row(self, row):
        s = np.zeros(8000, np.int16); ix = np.zeros(8000, np.uint16)
        self._chk(lib().fsgpu_kmer_row_copy(self.h, row, _ptr(s), _ptr(ix)), "fsgpu_kmer_row_copy")
        return s, ix

    def kmer_search(self, prepared, identity=None, max_res=1000, min_diag=30, bins=0, max_db_matches=0,
                    found_diagonals_size=0, l2_cache_size=0, want_stats=False, kmer_score_only=False):
        """prepared: list of (seq uint8[L], thr int16[nPos], profile int8[L,21]) from kmer_query_prepare."""
        nq = len(prepared)
        sp = KmerSearchParams(max_res, min_diag, bins, 1 if kmer_score_only else 0, max_db_matches, found_diagonals_size, l2_cache_size)
        qs = (KmerQuery * max(nq, 1))()
        keep = []
        for i, (seq, thr, prof) in enumerate(prepared):
            seq = np.ascontiguousarray(seq, np.uint8); thr = np.ascontiguousarray(thr, np.int16); prof = np.ascontiguousarray(prof, np.int8)
            keep.append((seq, thr, prof))
            qs[i].seq = seq.ctypes.data; qs[i].kmerThr = thr.ctypes.data; qs[i].profile = prof.ctypes.data
            qs[i].L = len(seq); qs[i].reserved = 0
            qs[i].identity = -1 if identity is None else int(identity[i])
        out = np.zeros((max(nq, 1), max_res), KMER_HIT_DT)
        nout = np.zeros(max(nq, 1), np.int32)
        status = np.zeros(max(nq, 1), np.int32)
        stats = np.zeros((max(nq, 1), 4))
        self._chk(lib().fsgpu_kmer_search(self.h, C.byref(sp), C.cast(qs, C.c_void_p), nq, _ptr(out), _ptr(nout), _ptr(status), _ptr(stats)),
                  "fsgpu_kmer_search")
        res = [out[q, :nout[q]].copy() for q in range(nq)]
        return (res, status[:nq], stats[:nq]) if want_stats else (res, status[:nq])

    def kmer_search_profile(self, prepared, identity=None, max_res=1000, min_diag=30, bins=0, max_db_matches=0, found_diagonals_size=0, l2_cache_size=0,
                            want_stats=False, kmer_score_only=False):
        """fsgpu_kmer_search_profile.  prepared: list of (seq uint8[L], scores int8[L,20], profile int8[L,21], kmerThr) from kmer_query_prepare_profile;
        the resident index must have been built with kmer_thr=0."""
        nq = len(prepared)
        sp = KmerSearchParams(max_res, min_diag, bins, 1 if kmer_score_only else 0, max_db_matches, found_diagonals_size, l2_cache_size)
        qs = (KmerProfileQuery * max(nq, 1))()
        keep = []
        for i, (seq, scores, prof, thr) in enumerate(prepared):
            seq = np.ascontiguousarray(seq, np.uint8); scores = np.ascontiguousarray(scores, np.int8).reshape(-1, 20)
            prof = np.ascontiguousarray(prof, np.int8).reshape(-1, 21)
            if len(scores) != len(seq) or len(prof) != len(seq):
                raise FsgpuError("kmer_search_profile: letters, score rows and profile differ in length")
            keep.append((seq, scores, prof))
            qs[i].seq = seq.ctypes.data; qs[i].scores = scores.ctypes.data; qs[i].profile = prof.ctypes.data
            qs[i].L = len(seq); qs[i].kmerThr = int(thr)
            qs[i].identity = -1 if identity is None else int(identity[i])
        out = np.zeros((max(nq, 1), max_res), KMER_HIT_DT)
        nout = np.zeros(max(nq, 1), np.int32)
        status = np.zeros(max(nq, 1), np.int32)
        stats = np.zeros((max(nq, 1), 4))
        self._chk(lib().fsgpu_kmer_search_profile(self.h, C.byref(sp), C.cast(qs, C.c_void_p), nq, _ptr(out), _ptr(nout), _ptr(status), _ptr(stats)),
                  "fsgpu_kmer_search_profile")
        res = [out[q, :nout[q]].copy() for q in range(nq)]
        return (res, status[:nq], stats[:nq]) if want_stats else (res, status[:nq])

    def kmer_profile_list(self, query, pos, cap=None):
        """fsgpu_kmer_profile_list_copy: (K_p, similar k-mers uint32 in emission order, reference numbering) of k-mer start `pos` of query `query` of the
        last device batch, which must have been a profile batch"""
        cnt = C.c_uint32(0)
        self._chk(lib().fsgpu_kmer_profile_list_copy(self.h, int(query), int(pos), None, 0, C.byref(cnt)), "fsgpu_kmer_profile_list_copy")
        n = cnt.value if cap is None else min(cnt.value, int(cap))
        out = np.zeros(max(n, 1), np.uint32)
        if n:
            self._chk(lib().fsgpu_kmer_profile_list_copy(self.h, int(query), int(pos), _ptr(out), n, C.byref(cnt)), "fsgpu_kmer_profile_list_copy")
        return int(cnt.value), out[:n]

    def kmer_counts(self):
        """last batch: similar k-mers probed, index hits, double-diagonal candidates, elements handed to the host"""
        out = np.zeros(4, np.uint64)
        lib().fsgpu_kmer_last_counts(self.h, _ptr(out))
        return out

    def kmer_segments(self):
        """last batch's partition: [1] = [4] (query, chunk, key) runs of the duplicate stage, [3] tiles, [5] coarse keys, [6] ids of the widest key"""
        out = np.zeros(7, np.uint32)
        lib().fsgpu_kmer_last_segments(self.h, _ptr(out))
        return out

    def kmer_stage_ms(self):
        """ms of the last k-mer batch: device total, count, lists, emit, partition, double-diagonal detection, score, walk, select; [9] host tail; [10] k_kmer_lists kernel alone"""
        return [lib().fsgpu_last_kernel_ms(self.h, 2 + i) for i in range(11)]

    def gapless_scores_multi(self, query_index):
        out = np.zeros(self.n, np.uint8)
        self._chk(lib().fsgpu_gapless_scores_multi(self.h, int(query_index), _ptr(out)), "gapless_scores_multi")
        return out

    def gapless_last_batch(self):
        a, b = C.c_int(0), C.c_int(0)
        lib().fsgpu_gapless_last_batch(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def gapless_scores(self):
        s = np.zeros(self.n, np.uint8)
        self._chk(lib().fsgpu_gapless_scores(self.h, _ptr(s)), "fsgpu_gapless_scores")
        return s

    def sw_multi_dir(self, queries, direction, selections=None, gap_open=10, gap_extend=1):
        """queries: list of (pAAf|None, p3f, pAAr|None, p3r, L, target_ids); one direction of the structure SW for the
        selected pairs (fsgpu_sw_multi_dir).  Returns one SWRES array per query (unselected entries stay zero)."""
        class Q(C.Structure):
            _fields_ = [("pAA_fwd", C.c_void_p), ("p3Di_fwd", C.c_void_p), ("pAA_rev", C.c_void_p), ("p3Di_rev", C.c_void_p),
                        ("L", C.c_int32), ("n", C.c_int32), ("targetIds", C.c_void_p)]
        nq = len(queries)
        keep, arr = [], (Q * nq)()
        for i, (paf, p3f, par_, p3r, L, ids) in enumerate(queries):
            bufs = [None if x is None else np.ascontiguousarray(x, np.int16) for x in (paf, p3f, par_, p3r)]
            ids = np.ascontiguousarray(ids, np.uint32)
            keep.append((bufs, ids))
            arr[i].pAA_fwd, arr[i].p3Di_fwd, arr[i].pAA_rev, arr[i].p3Di_rev = [None if b is None else b.ctypes.data for b in bufs]
            arr[i].L, arr[i].n, arr[i].targetIds = int(L), len(ids), ids.ctypes.data
        total = sum(len(k[1]) for k in keep)
        out = np.zeros(max(1, total), SWRES_DT)
        selp = nselp = None
        if selections is not None:
            sels = [np.ascontiguousarray(x, np.int32) for x in selections]
            keep.append(sels)
            selp = (C.c_void_p * nq)(*[x.ctypes.data for x in sels])
            nselp = (C.c_int32 * nq)(*[len(x) for x in sels])
        self._chk(lib().fsgpu_sw_multi_dir(self.h, C.cast(arr, C.c_void_p), nq, gap_open, gap_extend, direction,
                                           None if selp is None else C.cast(selp, C.c_void_p), None if nselp is None else C.cast(nselp, C.c_void_p),
                                           out.ctypes.data), "fsgpu_sw_multi_dir")
        res, b = [], 0
        for k in keep[:nq]:
            res.append(out[b:b + len(k[1])].copy()); b += len(k[1])
        return res

    def sw_multi(self, queries, gap_open=10, gap_extend=1):
        """both directions of every pair (fsgpu_sw_multi); queries as for sw_multi_dir.  Returns (fwd, rev), one SWRES array per query each."""
        class Q(C.Structure):
            _fields_ = [("pAA_fwd", C.c_void_p), ("p3Di_fwd", C.c_void_p), ("pAA_rev", C.c_void_p), ("p3Di_rev", C.c_void_p),
                        ("L", C.c_int32), ("n", C.c_int32), ("targetIds", C.c_void_p)]
        nq = len(queries)
        keep, arr = [], (Q * nq)()
        for i, (paf, p3f, par_, p3r, L, ids) in enumerate(queries):
            bufs = [None if x is None else np.ascontiguousarray(x, np.int16) for x in (paf, p3f, par_, p3r)]
            ids = np.ascontiguousarray(ids, np.uint32)
            keep.append((bufs, ids))
            arr[i].pAA_fwd, arr[i].p3Di_fwd, arr[i].pAA_rev, arr[i].p3Di_rev = [None if b is None else b.ctypes.data for b in bufs]
            arr[i].L, arr[i].n, arr[i].targetIds = int(L), len(ids), ids.ctypes.data
        total = sum(len(k[1]) for k in keep)
        fwd, rev = np.zeros(max(1, total), SWRES_DT), np.zeros(max(1, total), SWRES_DT)
        self._chk(lib().fsgpu_sw_multi(self.h, C.cast(arr, C.c_void_p), nq, gap_open, gap_extend, fwd.ctypes.data, rev.ctypes.data), "fsgpu_sw_multi")
        f, r, b = [], [], 0
        for k in keep:
            f.append(fwd[b:b + len(k[1])].copy()); r.append(rev[b:b + len(k[1])].copy()); b += len(k[1])
        return f, r

    def sw_kernel_counts(self):
        """launches of every k_sw / k_sw2 instantiation by this context since it was created (fsgpu_sw_kernel_counts):
        {(kind, has_aa, R): n}, kind 0 k_sw int16 halves, 1 k_sw int32, 2 k_sw2"""
        o = np.zeros(36, np.uint64)
        lib().fsgpu_sw_kernel_counts(self.h, _ptr(o))
        return {(kind, bool(aa), R): int(o[(kind * 2 + aa) * 6 + c]) for kind in range(3) for aa in (0, 1) for c, R in enumerate(SW_R_CLASSES)}

    def sw_multi_dir_c(self, mat3di, matAA, queries, direction, selections=None, gap_open=10, gap_extend=1):
        """Compact form (fsgpu_sw_multi_dir_c): mat3di / matAA int8 [21, 21] (matAA None = 3Di only); queries: list of
        (qAA|None, q3Di, cbAA_fwd|None, cb3Di_fwd|None, cbAA_rev|None, cb3Di_rev|None, target_ids).  Returns one SWRES array per query."""
        class Q(C.Structure):
            _fields_ = [("qAA", C.c_void_p), ("q3Di", C.c_void_p), ("cbAA_fwd", C.c_void_p), ("cb3Di_fwd", C.c_void_p), ("cbAA_rev", C.c_void_p),
                        ("cb3Di_rev", C.c_void_p), ("L", C.c_int32), ("n", C.c_int32), ("targetIds", C.c_void_p)]
        nq = len(queries)
        m3 = np.ascontiguousarray(mat3di, np.int8)
        mA = None if matAA is None else np.ascontiguousarray(matAA, np.int8)
        keep, arr = [], (Q * nq)()
        for i, (qa, q3, cbaf, cb3f, cbar, cb3r, ids) in enumerate(queries):
            q3 = np.ascontiguousarray(q3, np.uint8)
            qa = None if qa is None else np.ascontiguousarray(qa, np.uint8)
            cbs = [None if x is None else np.ascontiguousarray(x, np.int8) for x in (cbaf, cb3f, cbar, cb3r)]
            ids = np.ascontiguousarray(ids, np.uint32)
            keep.append((ids, q3, qa, cbs))
            arr[i].qAA, arr[i].q3Di = (None if qa is None else qa.ctypes.data), q3.ctypes.data
            arr[i].cbAA_fwd, arr[i].cb3Di_fwd, arr[i].cbAA_rev, arr[i].cb3Di_rev = [None if b is None else b.ctypes.data for b in cbs]
            arr[i].L, arr[i].n, arr[i].targetIds = len(q3), len(ids), ids.ctypes.data
        total = sum(len(k[0]) for k in keep)
        out = np.zeros(max(1, total), SWRES_DT)
        selp = nselp = None
        if selections is not None:
            sels = [np.ascontiguousarray(x, np.int32) for x in selections]
            keep.append(sels)
            selp = (C.c_void_p * nq)(*[x.ctypes.data for x in sels])
            nselp = (C.c_int32 * nq)(*[len(x) for x in sels])
        self._chk(lib().fsgpu_sw_multi_dir_c(self.h, m3.ctypes.data, None if mA is None else mA.ctypes.data, C.cast(arr, C.c_void_p), nq, gap_open, gap_extend,
                                             direction, None if selp is None else C.cast(selp, C.c_void_p), None if nselp is None else C.cast(nselp, C.c_void_p),
                                             out.ctypes.data), "fsgpu_sw_multi_dir_c")
        res, b = [], 0
        for k in keep[:nq]:
            res.append(out[b:b + len(k[0])].copy()); b += len(k[0])
        return res

    def sw_multi_c(self, mat3di, matAA, queries, gap_open=10, gap_extend=1):
        """both directions in one submission (fsgpu_sw_multi_c); queries as in sw_multi_dir_c.  Returns (fwd arrays, rev arrays)."""
        class Q(C.Structure):
            _fields_ = [("qAA", C.c_void_p), ("q3Di", C.c_void_p), ("cbAA_fwd", C.c_void_p), ("cb3Di_fwd", C.c_void_p), ("cbAA_rev", C.c_void_p),
                        ("cb3Di_rev", C.c_void_p), ("L", C.c_int32), ("n", C.c_int32), ("targetIds", C.c_void_p)]
        nq = len(queries)
        m3 = np.ascontiguousarray(mat3di, np.int8)
        mA = None if matAA is None else np.ascontiguousarray(matAA, np.int8)
        keep, arr = [], (Q * nq)()
        for i, (qa, q3, cbaf, cb3f, cbar, cb3r, ids) in enumerate(queries):
            q3 = np.ascontiguousarray(q3, np.uint8)
            qa = None if qa is None else np.ascontiguousarray(qa, np.uint8)
            cbs = [None if x is None else np.ascontiguousarray(x, np.int8) for x in (cbaf, cb3f, cbar, cb3r)]
            ids = np.ascontiguousarray(ids, np.uint32)
            keep.append((ids, q3, qa, cbs))
            arr[i].qAA, arr[i].q3Di = (None if qa is None else qa.ctypes.data), q3.ctypes.data
            arr[i].cbAA_fwd, arr[i].cb3Di_fwd, arr[i].cbAA_rev, arr[i].cb3Di_rev = [None if b is None else b.ctypes.data for b in cbs]
            arr[i].L, arr[i].n, arr[i].targetIds = len(q3), len(ids), ids.ctypes.data
        total = sum(len(k[0]) for k in keep)
        fwd, rev = np.zeros(max(1, total), SWRES_DT), np.zeros(max(1, total), SWRES_DT)
        self._chk(lib().fsgpu_sw_multi_c(self.h, m3.ctypes.data, None if mA is None else mA.ctypes.data, C.cast(arr, C.c_void_p), nq, gap_open, gap_extend,
                                         fwd.ctypes.data, rev.ctypes.data), "fsgpu_sw_multi_c")
        rf, rr, b = [], [], 0
        for k in keep:
            rf.append(fwd[b:b + len(k[0])].copy()); rr.append(rev[b:b + len(k[0])].copy()); b += len(k[0])
        return rf, rr

    def _pqueries(self, queries):
        """fsgpu_sw_pquery array of (pAA_fwd|None, p3Di_fwd, pAA_rev|None, p3Di_rev, target_ids): int8 [21, L] tables"""
        class Q(C.Structure):
            _fields_ = [("pAA_fwd", C.c_void_p), ("p3Di_fwd", C.c_void_p), ("pAA_rev", C.c_void_p), ("p3Di_rev", C.c_void_p),
                        ("L", C.c_int32), ("n", C.c_int32), ("targetIds", C.c_void_p)]
        keep, arr = [], (Q * max(1, len(queries)))()
        for i, (paf, p3f, par_, p3r, ids) in enumerate(queries):
            bufs = [None if x is None else np.ascontiguousarray(x, np.int8).reshape(21, -1) for x in (paf, p3f, par_, p3r)]
            ids = np.ascontiguousarray(ids, np.uint32)
            keep.append((ids, bufs))
            arr[i].pAA_fwd, arr[i].p3Di_fwd, arr[i].pAA_rev, arr[i].p3Di_rev = [None if b is None else b.ctypes.data for b in bufs]
            arr[i].L, arr[i].n, arr[i].targetIds = bufs[1].shape[1], len(ids), ids.ctypes.data
        return keep, arr

    def sw_multi_dir_p(self, queries, direction, selections=None, gap_open=10, gap_extend=1):
        """Profile queries (fsgpu_sw_multi_dir_p): list of (pAA_fwd|None, p3Di_fwd, pAA_rev|None, p3Di_rev, target_ids), each table int8 [21, L] --
        profile_decode's output.  One direction for the selected pairs; returns one SWRES array per query (unselected entries stay zero)."""
        nq = len(queries)
        keep, arr = self._pqueries(queries)
        total = sum(len(k[0]) for k in keep)
        out = np.zeros(max(1, total), SWRES_DT)
        selp = nselp = None
        if selections is not None:
            sels = [np.ascontiguousarray(x, np.int32) for x in selections]
            keep.append(sels)
            selp = (C.c_void_p * nq)(*[x.ctypes.data for x in sels])
            nselp = (C.c_int32 * nq)(*[len(x) for x in sels])
        self._chk(lib().fsgpu_sw_multi_dir_p(self.h, C.cast(arr, C.c_void_p), nq, gap_open, gap_extend, direction,
                                             None if selp is None else C.cast(selp, C.c_void_p), None if nselp is None else C.cast(nselp, C.c_void_p),
                                             out.ctypes.data), "fsgpu_sw_multi_dir_p")
        res, b = [], 0
        for k in keep[:nq]:
            res.append(out[b:b + len(k[0])].copy()); b += len(k[0])
        return res

    def sw_multi_p(self, queries, gap_open=10, gap_extend=1):
        """both directions of profile queries in one submission (fsgpu_sw_multi_p); queries as in sw_multi_dir_p.  Returns (fwd arrays, rev arrays)."""
        keep, arr = self._pqueries(queries)
        total = sum(len(k[0]) for k in keep)
        fwd, rev = np.zeros(max(1, total), SWRES_DT), np.zeros(max(1, total), SWRES_DT)
        self._chk(lib().fsgpu_sw_multi_p(self.h, C.cast(arr, C.c_void_p), len(queries), gap_open, gap_extend, fwd.ctypes.data, rev.ctypes.data), "fsgpu_sw_multi_p")
        rf, rr, b = [], [], 0
        for k in keep:
            rf.append(fwd[b:b + len(k[0])].copy()); rr.append(rev[b:b + len(k[0])].copy()); b += len(k[0])
        return rf, rr

    def sw_scan_c(self, mat3di, matAA, queries, cutoffs, gap_open=10, gap_extend=1, cap=None):
        """Whole-database forward pass with the selection on the device (fsgpu_sw_scan_c).  queries: tuples as for sw_multi_dir_c without the
        target ids (a seventh element is ignored); cutoffs: one score per query.  Returns [(ids, records)] per query: ascending target ids and the
        forward records of the pairs with score >= cutoff.  cap None: the buffers start at 4096 records and the call is repeated once with the
        size FSGPU_E_OUTPUT reported.  cap given: one call with buffers of cap records followed by one guard record, kept with the base array
        and the status as last_scan = (rc, base, ids, records); FSGPU_E_OUTPUT then raises FsgpuError with .rc == FSGPU_E_OUTPUT."""
        class Q(C.Structure):
            _fields_ = [("qAA", C.c_void_p), ("q3Di", C.c_void_p), ("cbAA_fwd", C.c_void_p), ("cb3Di_fwd", C.c_void_p), ("cbAA_rev", C.c_void_p),
                        ("cb3Di_rev", C.c_void_p), ("L", C.c_int32), ("n", C.c_int32), ("targetIds", C.c_void_p)]
        nq = len(queries)
        m3 = np.ascontiguousarray(mat3di, np.int8)
        mA = None if matAA is None else np.ascontiguousarray(matAA, np.int8)
        keep, arr = [], (Q * max(nq, 1))()
        for i, qt in enumerate(queries):
            qa, q3, cbaf, cb3f, cbar, cb3r = qt[:6]
            q3 = np.ascontiguousarray(q3, np.uint8)
            qa = None if qa is None else np.ascontiguousarray(qa, np.uint8)
            cbs = [None if x is None else np.ascontiguousarray(x, np.int8) for x in (cbaf, cb3f, cbar, cb3r)]
            keep.append((q3, qa, cbs))
            arr[i].qAA, arr[i].q3Di = (None if qa is None else qa.ctypes.data), q3.ctypes.data
            arr[i].cbAA_fwd, arr[i].cb3Di_fwd, arr[i].cbAA_rev, arr[i].cb3Di_rev = [None if b is None else b.ctypes.data for b in cbs]
            arr[i].L, arr[i].n, arr[i].targetIds = len(q3), 0, None
        cut = np.ascontiguousarray(cutoffs, np.int32)
        if len(cut) != nq:
            raise ValueError("one cutoff per query")
        base = np.zeros(nq + 1, np.uint64)

        def call(room):
            ids = np.full(room + 1, SCAN_GUARD, np.uint32)
            recs = np.full(room + 1, SCAN_GUARD, np.uint32).repeat(4).view(SWRES_DT)
            rc = lib().fsgpu_sw_scan_c(self.h, m3.ctypes.data, None if mA is None else mA.ctypes.data, C.cast(arr, C.c_void_p), nq, gap_open, gap_extend,
                                       _ptr(cut), _ptr(ids), _ptr(recs), room, _ptr(base))
            return rc, ids, recs
        rc, ids, recs = call(4096 if cap is None else int(cap))
        if cap is None and rc == FSGPU_E_OUTPUT:
            rc, ids, recs = call(int(base[nq]))
        self.last_scan = (rc, base.copy(), ids, recs)
        if rc != 0:
            e = FsgpuError(f"fsgpu_sw_scan_c rc={rc}: {lib().fsgpu_last_error(self.h).decode()}")
            e.rc = rc
            raise e
        return [(ids[int(base[i]):int(base[i + 1])].copy(), recs[int(base[i]):int(base[i + 1])].copy()) for i in range(nq)]

    def sw_scan_last(self):
        """fsgpu_sw_scan_last: sub-batches, records handed to the host, host ms spent planning, survivors, host ms of the whole call"""
        o = np.zeros(8)
        lib().fsgpu_sw_scan_last(self.h, _ptr(o))
        return {"sub_batches": int(o[0]), "device_selected": int(o[1]), "plan_ms": float(o[2]), "survivors": int(o[3]), "call_ms": float(o[4])}

    def sw_batch(self, pAAf, p3f, pAAr, p3r, target_ids, gap_open=10, gap_extend=1):
        p3f = np.ascontiguousarray(p3f, np.int16)
        p3r = np.ascontiguousarray(p3r, np.int16)
        pAAf = None if pAAf is None else np.ascontiguousarray(pAAf, np.int16)
        pAAr = None if pAAr is None else np.ascontiguousarray(pAAr, np.int16)
        t = np.ascontiguousarray(target_ids, np.uint32)
        fwd = np.zeros(len(t), SWRES_DT)
        rev = np.zeros(len(t), SWRES_DT)
        self._chk(lib().fsgpu_sw_batch(self.h, _ptr(pAAf), _ptr(p3f), _ptr(pAAr), _ptr(p3r), p3f.shape[1], _ptr(t), len(t),
                                       gap_open, gap_extend, _ptr(fwd), _ptr(rev)), "fsgpu_sw_batch")
        return fwd, rev

    @staticmethod
    def _pack_seqs(seq_lists, offsets, lengths):
        """code arrays -> one uint8 buffer each, UNPADDED and back to back, + (offsets uint64[n + 1], lengths int32[n]); offsets / lengths given by the
        caller are handed on as they are (the layout checks of the entries are reached that way)"""
        n = len(seq_lists[0])
        ln = np.array([len(s) for s in seq_lists[0]], np.int64)
        bufs = []
        for seqs in seq_lists:
            if seqs is None:
                bufs.append(None)
                continue
            if len(seqs) != n or any(len(s) != l for s, l in zip(seqs, ln)):
                raise FsgpuError("the AA and 3Di sequences differ in number or length")
            parts = [np.ascontiguousarray(s, np.uint8).reshape(-1) for s in seqs]
            bufs.append(np.ascontiguousarray(np.concatenate(parts + [np.zeros(1, np.uint8)])))     # never an empty buffer (NULL would read as "missing")
        off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64) if offsets is None else np.ascontiguousarray(offsets, np.uint64)
        lens = ln.astype(np.int32) if lengths is None else np.ascontiguousarray(lengths, np.int32)
        if len(off) != len(lens) + 1:
            raise FsgpuError("offsets must have one entry more than lengths")
        if int(off[-1]) > int(ln.sum()):                   # the entries copy offsets[n] bytes out of these buffers
            raise FsgpuError("offsets[n] lies beyond the sequence data")
        return bufs, off, lens

    def diag_rescore(self, qAA, q3Di, mat3Di, matAA, pairs, offsets=None, lengths=None):
        """fsgpu_diag_rescore called directly.  qAA / q3Di: lists of code arrays (0..20), one per query; mat3Di / matAA: int16 [21, 21]; pairs: DIAG_PAIR_DT
        array or a list of (query, target, diagonal) with targets of the resident DB.  Returns a DIAG_RES_DT array, one record per pair."""
        (qa, q3), off, lens = self._pack_seqs((qAA, q3Di), offsets, lengths)
        m3 = np.ascontiguousarray(mat3Di, np.int16)
        mA = np.ascontiguousarray(matAA, np.int16)
        if m3.size != 21 * 21 or mA.size != 21 * 21:
            raise FsgpuError("diag_rescore: matrices must be int16 [21, 21]")
        if isinstance(pairs, np.ndarray) and pairs.dtype == DIAG_PAIR_DT:
            p = np.ascontiguousarray(pairs)
        else:
            p = np.zeros(len(pairs), DIAG_PAIR_DT)
            for k, (q, t, d) in enumerate(pairs):
                p[k] = (int(q) & 0xFFFFFFFF, int(t) & 0xFFFFFFFF, int(d))
        out = np.zeros(max(len(p), 1), DIAG_RES_DT)
        out["reserved"] = -1                               # the entry writes every field of every record
        self._chk(lib().fsgpu_diag_rescore(self.h, _ptr(qa), _ptr(q3), _ptr(off), _ptr(lens), len(lens), _ptr(m3), _ptr(mA),
                                           _ptr(p) if len(p) else None, len(p), _ptr(out)), "fsgpu_diag_rescore")
        return out[:len(p)]

    def sw_batch_seqs(self, pAAf, p3f, pAAr, p3r, tAA, t3Di, gap_open=10, gap_extend=1, offsets=None, lengths=None):
        """fsgpu_sw_batch_seqs called directly: both directions of the structure SW of one query against EXPLICIT targets.  tAA (None with pAA* None) /
        t3Di: lists of code arrays (0..20).  Returns (fwd, rev) as SW_DT arrays."""
        p3f = np.ascontiguousarray(p3f, np.int16)
        p3r = np.ascontiguousarray(p3r, np.int16)
        pAAf = None if pAAf is None else np.ascontiguousarray(pAAf, np.int16)
        pAAr = None if pAAr is None else np.ascontiguousarray(pAAr, np.int16)
        (t3, ta), off, lens = self._pack_seqs((t3Di, tAA), offsets, lengths)
        n = len(lens)
        fwd = np.zeros(max(n, 1), SW_DT)
        rev = np.zeros(max(n, 1), SW_DT)
        self._chk(lib().fsgpu_sw_batch_seqs(self.h, _ptr(pAAf), _ptr(p3f), _ptr(pAAr), _ptr(p3r), p3f.shape[1], _ptr(ta), _ptr(t3), _ptr(off), _ptr(lens), n,
                                            gap_open, gap_extend, _ptr(fwd), _ptr(rev)), "fsgpu_sw_batch_seqs")
        return fwd[:n], rev[:n]

    def block_backtrace(self, tblAA, tbl3Di, letAA, let3Di, queries, tasks, gap_open=10, gap_extend=1):
        """fsgpu_block_backtrace called directly: start position + backtrace of accepted hits by the device block aligner, nothing recomputed on the
        host.  tblAA / tbl3Di: int8 [27, 32] letter-indexed tables, letAA / let3Di: uint8 [21] code -> letter - 'A'; queries: list of
        (qAA, q3Di, cbAA, cbSS) (codes 0..20 and the int8 composition bias arrays); tasks: list of (query, target, qEnd, dbEnd, score).
        Returns one dict per task: status (1 answered, 2 SW score not reproduced, 0 handed back), qStart, dbStart, identicalAA, blockSizes and the
        backtrace string, copied out of the context's buffer before the next call can overwrite it."""
        tA, t3 = np.ascontiguousarray(tblAA, np.int8), np.ascontiguousarray(tbl3Di, np.int8)
        lA, l3 = np.ascontiguousarray(letAA, np.uint8), np.ascontiguousarray(let3Di, np.uint8)
        if tA.size != 27 * 32 or t3.size != 27 * 32 or lA.size != 21 or l3.size != 21:
            raise FsgpuError("block_backtrace: tables must be int8 [27, 32], letter maps uint8 [21]")
        nq, nt = len(queries), len(tasks)
        qs, keep = (BtQuery * max(nq, 1))(), []
        for i, (qa, q3, ca, cs) in enumerate(queries):
            bufs = (np.ascontiguousarray(qa, np.uint8), np.ascontiguousarray(q3, np.uint8), np.ascontiguousarray(ca, np.int8), np.ascontiguousarray(cs, np.int8))
            if not (len(bufs[0]) == len(bufs[1]) == len(bufs[2]) == len(bufs[3])):
                raise FsgpuError(f"block_backtrace: query {i}: sequences and bias arrays differ in length")
            keep.append(bufs)
            qs[i].qAA, qs[i].q3Di, qs[i].cbAA, qs[i].cbSS = [b.ctypes.data for b in bufs]
            qs[i].L, qs[i].reserved = len(bufs[0]), 0
        ts = (BtTask * max(nt, 1))()
        for k, (q, t, qe, de, sc) in enumerate(tasks):
            ts[k].query, ts[k].target, ts[k].qEnd, ts[k].dbEnd, ts[k].score = int(q), int(t), int(qe), int(de), int(sc)
        res = (BtRes * max(nt, 1))()
        base = C.c_void_p()
        self._chk(lib().fsgpu_block_backtrace(self.h, _ptr(tA), _ptr(t3), _ptr(lA), _ptr(l3), qs, nq, ts, nt, int(gap_open), int(gap_extend), res,
                                              C.byref(base)), "fsgpu_block_backtrace")
        out = []
        for k in range(nt):
            r = res[k]
            bt = C.string_at(base.value + r.btOff, r.btLen).decode() if r.status == 1 and r.btLen > 0 else ""
            out.append(dict(status=r.status, qStart=r.qStart, dbStart=r.dbStart, identicalAA=r.identicalAA, blockSizes=r.blockSizes, backtrace=bt))
        return out

    def profile_backtrace(self, queries, tasks, gap_open=10, gap_extend=1):
        """fsgpu_profile_backtrace called directly: start cell, identity count and M / I / D string of accepted hits of profile queries.  queries: list of
        (pAA int8 [21, L], p3Di int8 [21, L], lettersAA uint8 [L]) -- the forward alignment profiles; tasks: list of (query, target, qEnd, dbEnd, score)
        with targets of the resident DB.  Returns one dict per task: status (1 answered, 2 reverse pass differs, 3 no path, 0 handed back), qStart,
        dbStart, identicalAA, band (the width the banded pass ended with) and the backtrace, copied out before the next call can overwrite it.  A refusal
        raises FsgpuError with .rc and .res: the result records as the call left them (filled with -7 before it)."""
        nq, nt = len(queries), len(tasks)
        qs, keep = (PbtQuery * max(nq, 1))(), []
        for i, (pa, p3, let) in enumerate(queries):
            bufs = (np.ascontiguousarray(pa, np.int8), np.ascontiguousarray(p3, np.int8), np.ascontiguousarray(let, np.uint8))
            L = len(bufs[2])
            if bufs[0].size != 21 * L or bufs[1].size != 21 * L:
                raise FsgpuError(f"profile_backtrace: query {i}: tables must be int8 [21, L] for L letters")
            keep.append(bufs)
            qs[i].pAA, qs[i].p3Di, qs[i].lettersAA = [b.ctypes.data for b in bufs]
            qs[i].L, qs[i].reserved = L, 0
        ts = (BtTask * max(nt, 1))()
        for k, (q, t, qe, de, sc) in enumerate(tasks):
            ts[k].query, ts[k].target, ts[k].qEnd, ts[k].dbEnd, ts[k].score = int(q) & 0xFFFFFFFF, int(t) & 0xFFFFFFFF, int(qe), int(de), int(sc)
        res = (BtRes * max(nt, 1))()
        C.memset(res, 0xF9, C.sizeof(res))
        base = C.c_void_p()
        rc = lib().fsgpu_profile_backtrace(self.h, qs, nq, ts, nt, int(gap_open), int(gap_extend), res, C.byref(base))
        if rc != 0:
            e = FsgpuError(f"fsgpu_profile_backtrace rc={rc}: {lib().fsgpu_last_error(self.h).decode()}")
            e.rc, e.res = rc, bytes(res)
            raise e
        out = []
        for k in range(nt):
            r = res[k]
            bt = C.string_at(base.value + r.btOff, r.btLen).decode() if r.status == 1 and r.btLen > 0 else ""
            out.append(dict(status=r.status, qStart=r.qStart, dbStart=r.dbStart, identicalAA=r.identicalAA, band=r.blockSizes, backtrace=bt))
        return out

    def profile_backtrace_last(self):
        """fsgpu_profile_backtrace_last: what the last profile_backtrace call of this context did"""
        o = np.zeros(8)
        lib().fsgpu_profile_backtrace_last(self.h, _ptr(o))
        return {"launches": int(o[0]), "status": [int(o[1]), int(o[2]), int(o[3]), int(o[4])], "device_ms": float(o[5]), "scratch_bytes": int(o[6]),
                "band_launches": int(o[7])}

    def lddt_batch(self, queries, targets, tasks):
        """fsgpu_lddt_batch called directly: the reference's per-residue LDDT values of a batch of hits.  queries / targets: lists of float32
        arrays [3, L] (x, y, z rows, what ca_decode returns); tasks: list of (query, target, qStart, dbStart, backtrace string).  Returns one
        (alignLength, float32 array of alignLength per-column values) per task; a NaN marks a column the average skips (lddt_average)."""
        nq, nt = len(queries), len(tasks)
        qs, keep = (LddtQuery * max(nq, 1))(), []
        for i, q in enumerate(queries):
            q = np.ascontiguousarray(q, np.float32)
            if q.ndim != 2 or q.shape[0] != 3:
                raise FsgpuError(f"lddt_batch: query {i}: coordinates must be float32 [3, L]")
            keep.append(q)
            qs[i].ca, qs[i].L, qs[i].reserved = q.ctypes.data, q.shape[1], 0
        tl = [np.ascontiguousarray(t, np.float32) for t in targets]
        toff = np.concatenate([[0], np.cumsum([t.size for t in tl])]).astype(np.int64)
        tc = np.concatenate([t.reshape(-1) for t in tl]) if tl else np.zeros(0, np.float32)
        bts = [str(t[4]).encode() for t in tasks]
        ts = (LddtTask * max(nt, 1))()
        boff = ooff = 0
        for k, (q, t, qs0, ds0, _) in enumerate(tasks):
            ts[k].query, ts[k].tLen, ts[k].tOff, ts[k].qStart, ts[k].dbStart = int(q), tl[int(t)].shape[1], int(toff[int(t)]), int(qs0), int(ds0)
            ts[k].btOff, ts[k].btLen, ts[k].reserved, ts[k].outOff = boff, len(bts[k]), 0, ooff
            boff += len(bts[k])
            ooff += bts[k].count(b"M")
        bt = np.frombuffer(b"".join(bts), np.uint8) if boff else np.zeros(0, np.uint8)
        aln = np.full(max(nt, 1), -1, np.int32)
        out = np.full(max(ooff, 1), -1.0, np.float32)
        self._chk(lib().fsgpu_lddt_batch(self.h, qs, nq, ts, nt, _ptr(tc), tc.size, _ptr(bt), bt.size, _ptr(aln), _ptr(out), ooff), "fsgpu_lddt_batch")
        return [(int(aln[k]), out[ts[k].outOff:ts[k].outOff + max(int(aln[k]), 0)].copy()) for k in range(nt)]

    def tm_batch(self, queries, targets, tasks, params=None):
        """fsgpu_tm_batch called directly: the raw values of the reference's approximate TM-score for a batch of hits.  queries / targets: lists of
        float32 arrays [3, L]; tasks: list of (query, target, qStart, dbStart, backtrace string, normalisation length).  The per-task scalars come from
        fshost_tm_params.  Returns one (pairs, score_max of standard_TMscore's search, score_max of detailed_search_standard's, rmsd) per task, the
        three floats as numpy float32; tm_finish turns them into the TM-score.  params: per task four floats in place of fshost_tm_params' (tests)."""
        nq, nt = len(queries), len(tasks)
        qs, keep = (LddtQuery * max(nq, 1))(), []
        for i, q in enumerate(queries):
            q = np.ascontiguousarray(q, np.float32)
            if q.ndim != 2 or q.shape[0] != 3:
                raise FsgpuError(f"tm_batch: query {i}: coordinates must be float32 [3, L]")
            keep.append(q)
            qs[i].ca, qs[i].L, qs[i].reserved = q.ctypes.data, q.shape[1], 0
        tl = [np.ascontiguousarray(t, np.float32) for t in targets]
        toff = np.concatenate([[0], np.cumsum([t.size for t in tl])]).astype(np.int64)
        tc = np.concatenate([t.reshape(-1) for t in tl]) if tl else np.zeros(0, np.float32)
        bts = [str(t[4]).encode() for t in tasks]
        ts = (TmTask * max(nt, 1))()
        boff, par = 0, {}
        for k, (q, t, qs0, ds0, _, norm_len) in enumerate(tasks):
            ts[k].query, ts[k].tLen, ts[k].tOff, ts[k].qStart, ts[k].dbStart = int(q), tl[int(t)].shape[1], int(toff[int(t)]), int(qs0), int(ds0)
            ts[k].btOff, ts[k].btLen, ts[k].reserved = boff, len(bts[k]), 0
            if norm_len not in par:
                par[norm_len] = tm_params(norm_len)
            ts[k].scoreD8, ts[k].d0Std, ts[k].d0, ts[k].d0Search = (float(v) for v in (params[k] if params is not None else par[norm_len]))
            boff += len(bts[k])
        bt = np.frombuffer(b"".join(bts), np.uint8) if boff else np.zeros(0, np.uint8)
        n = np.full(max(nt, 1), -1, np.int32)
        scores = np.full(2 * max(nt, 1), np.nan, np.float32)
        rmsd = np.full(max(nt, 1), np.nan, np.float32)
        self._chk(lib().fsgpu_tm_batch(self.h, qs, nq, ts, nt, _ptr(tc), tc.size, _ptr(bt), bt.size, _ptr(n), _ptr(scores), _ptr(rmsd)), "fsgpu_tm_batch")
        return [(int(n[k]), scores[k], scores[nt + k], rmsd[k]) for k in range(nt)]

    def tm_superpose_batch(self, queries, targets, tasks, exact=False, params=None):
        """fsgpu_tm_superpose_batch called directly: tm_batch's arguments; exact: the search of --exact-tmscore 1 (the per-task scalars then come from
        fshost_tm_exact_params).  Returns one dict per task: pairs, scores (float32 [2]; exact: [score_max, -1]), rms (the raw float32), source
        (TM_SRC_*), t (float32 [3]), u (float32 [3, 3]).  tm_finish / tm_exact_finish turn the raw values into the TM-score and the rmsd."""
        nq, nt = len(queries), len(tasks)
        qs, keep = (LddtQuery * max(nq, 1))(), []
        for i, q in enumerate(queries):
            q = np.ascontiguousarray(q, np.float32)
            if q.ndim != 2 or q.shape[0] != 3:
                raise FsgpuError(f"tm_superpose_batch: query {i}: coordinates must be float32 [3, L]")
            keep.append(q)
            qs[i].ca, qs[i].L, qs[i].reserved = q.ctypes.data, q.shape[1], 0
        tl = [np.ascontiguousarray(t, np.float32) for t in targets]
        toff = np.concatenate([[0], np.cumsum([t.size for t in tl])]).astype(np.int64)
        tc = np.concatenate([t.reshape(-1) for t in tl]) if tl else np.zeros(0, np.float32)
        bts = [str(t[4]).encode() for t in tasks]
        ts = (TmTask * max(nt, 1))()
        boff, par = 0, {}
        for k, (q, t, qs0, ds0, _, norm_len) in enumerate(tasks):
            ts[k].query, ts[k].tLen, ts[k].tOff, ts[k].qStart, ts[k].dbStart = int(q), tl[int(t)].shape[1], int(toff[int(t)]), int(qs0), int(ds0)
            ts[k].btOff, ts[k].btLen, ts[k].reserved = boff, len(bts[k]), 0
            if norm_len not in par:
                par[norm_len] = tm_exact_params(norm_len) if exact else tm_params(norm_len)
            ts[k].scoreD8, ts[k].d0Std, ts[k].d0, ts[k].d0Search = (float(v) for v in (params[k] if params is not None else par[norm_len]))
            boff += len(bts[k])
        bt = np.frombuffer(b"".join(bts), np.uint8) if boff else np.zeros(0, np.uint8)
        res = (TmResult * max(nt, 1))()
        self._chk(lib().fsgpu_tm_superpose_batch(self.h, qs, nq, ts, nt, _ptr(tc), tc.size, _ptr(bt), bt.size, 1 if exact else 0, res), "fsgpu_tm_superpose_batch")
        return [{"pairs": int(r.nPairs), "source": int(r.source), "scores": np.array(r.score[:], np.float32), "rms": np.float32(r.rms),
                 "t": np.array(r.t[:], np.float32), "u": np.array(r.u[:], np.float32).reshape(3, 3)} for r in res[:nt]]

    def block_backtrace_footprint(self, workgroups_per_cu):
        """workgroups of the block aligner per compute unit for the following block_backtrace calls (0: the default)"""
        self._chk(lib().fsgpu_block_backtrace_footprint(self.h, int(workgroups_per_cu)), "fsgpu_block_backtrace_footprint")

    def kernel_ms(self, which):
        return lib().fsgpu_last_kernel_ms(self.h, which)

    def history_counters(self):
        """fsgpu_history_counters: the choices this context made from what it ran before"""
        o = np.zeros(8, np.uint64)
        lib().fsgpu_history_counters(self.h, _ptr(o))
        o = [int(v) for v in o]
        return {"kmer_count_form": o[0], "kmer_list_form": o[1], "kmer_batches": o[2], "kmer_last_batch_queries": o[3],
                "sw_long_launched": o[4], "sw_long_reused": o[5], "lddt_norm_runs": o[6], "kmer_first_batch_queries": o[7]}

    def sw_last_passes(self):
        """[[ms, cells, pairs, DP wave-instructions] forward, [...] reversed] of the last multi-query SW passes (k_sw2 launches only)"""
        out = np.zeros(8)
        lib().fsgpu_sw_last_passes(self.h, _ptr(out))
        return out.reshape(2, 4)

    def sw3_last_plan(self):
        """what the last compact SW call (sw_multi_dir_c / sw_multi_c) planned and ran (fsgpu_sw3_last_plan): pairs and rows-per-lane classes per
        shape (lanes per target pair -> count / set of R), pairs on the profile path, pairs re-run in int32, images built, launch groups, workgroups"""
        o = np.zeros(12, np.uint32)
        lib().fsgpu_sw3_last_plan(self.h, _ptr(o))
        o = [int(v) for v in o]
        return {"pairs": {16: o[0], 32: o[1], 64: o[2]},
                "classes": {hl: {r for r in range(32) if o[3 + k] >> r & 1} for k, hl in enumerate((16, 32, 64))},
                "profile_pairs": o[6], "rerun_pairs": o[7], "images_built": o[8], "groups": o[9], "workgroups": o[10]}

    def close(self):
        if getattr(self, "h", None):
            lib().fsgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Search:
    """fshost_search: one query at a time through prefilter + structurealign on a Context."""

    def __init__(self, ctx, params=None, keys=None, nn_path=None):
        self.ctx = ctx
        self.par = params if params is not None else default_params()
        d3, da, off, ln = ctx._keep
        self._keys = None if keys is None else np.ascontiguousarray(keys, np.uint32)
        self.h = lib().fshost_search_create(ctx.h, C.byref(self.par), _ptr(self._keys), nn_path.encode() if nn_path else None,
                                            _ptr(d3), _ptr(da), _ptr(off), _ptr(ln))
        err = lib().fshost_search_error(self.h).decode() if self.h else "null"
        if not self.h or err:
            raise FsgpuError(f"fshost_search_create: {err}")

    def prefilter(self, q3di, identity=-1):
        q = np.ascontiguousarray(q3di, np.uint8)
        hits = np.zeros(self.par.maxResListLen, HIT_DT)
        n = lib().fshost_search_prefilter(self.h, _ptr(q), len(q), identity, _ptr(hits))
        if n < 0:
            raise FsgpuError(f"prefilter rc={n}: {lib().fshost_search_error(self.h).decode()}")
        return hits[:n]

    def prefilter_batch(self, q3dis, identity=None):
        """several queries, as few scan launches as their lengths allow (fsgpu_gapless_scan_multi); list of hit arrays"""
        nq = len(q3dis)
        q3 = [np.ascontiguousarray(x, np.uint8) for x in q3dis]
        P = C.c_void_p * max(nq, 1)
        p3 = P(*[x.ctypes.data for x in q3])
        Ls = np.array([len(x) for x in q3], np.int32)
        ident = None if identity is None else np.ascontiguousarray(identity, np.int64)
        K = self.par.maxResListLen
        hits = np.zeros(max(1, nq * K), HIT_DT)
        nh = np.zeros(max(nq, 1), np.int32)
        rc = lib().fshost_search_prefilter_batch(self.h, nq, C.cast(p3, C.c_void_p), _ptr(Ls), _ptr(ident), _ptr(hits), _ptr(nh))
        if rc != 0:
            raise FsgpuError(f"prefilter_batch rc={rc}: {lib().fshost_search_error(self.h).decode()}")
        return [hits[i * K:i * K + nh[i]].copy() for i in range(nq)]

    # ---- profile queries: entries = (AA entry bytes, 3Di entry bytes) of a profile database, decoded here (profile_decode) ----
    class _PQ(C.Structure):
        _fields_ = [("codesAA", C.c_void_p), ("codes3Di", C.c_void_p), ("pAA", C.c_void_p), ("pAArev", C.c_void_p), ("p3Di", C.c_void_p), ("p3Direv", C.c_void_p),
                    ("L", C.c_int32), ("reserved", C.c_int32)]

    def _pqueries(self, entries):
        keep, arr = [], (Search._PQ * max(1, len(entries)))()
        for i, (ea, e3) in enumerate(entries):
            ca, _, aF, aR = profile_decode(ea)
            c3, _, sF, sR = profile_decode(e3)
            if len(ca) != len(c3):
                raise FsgpuError("AA / 3Di profiles do not match")
            keep.append((ca, c3, aF, aR, sF, sR))
            arr[i].codesAA, arr[i].codes3Di, arr[i].pAA, arr[i].pAArev, arr[i].p3Di, arr[i].p3Direv = [x.ctypes.data for x in keep[-1]]
            arr[i].L, arr[i].reserved = len(c3), 0
        return keep, arr

    def prefilter_profile(self, entry_3di, identity=-1):
        """fshost_search_prefilter_profile: the hit list of one profile query (the pssm is its 3Di alignment profile)"""
        _, _, prof, _ = profile_decode(entry_3di)
        hits = np.zeros(self.par.maxResListLen, HIT_DT)
        n = lib().fshost_search_prefilter_profile(self.h, _ptr(prof), prof.shape[1], identity, _ptr(hits))
        if n < 0:
            raise FsgpuError(f"prefilter_profile rc={n}: {lib().fshost_search_error(self.h).decode()}")
        return hits[:n]

    def prefilter_batch_profile(self, entries_3di, identity=None):
        nq = len(entries_3di)
        profs = [profile_decode(e)[2] for e in entries_3di]
        pp = (C.c_void_p * max(nq, 1))(*[x.ctypes.data for x in profs])
        Ls = np.array([x.shape[1] for x in profs], np.int32)
        ident = None if identity is None else np.ascontiguousarray(identity, np.int64)
        K = self.par.maxResListLen
        hits, nh = np.zeros(max(1, nq * K), HIT_DT), np.zeros(max(nq, 1), np.int32)
        rc = lib().fshost_search_prefilter_batch_profile(self.h, nq, C.cast(pp, C.c_void_p), _ptr(Ls), _ptr(ident), _ptr(hits), _ptr(nh))
        if rc != 0:
            raise FsgpuError(f"prefilter_batch_profile rc={rc}: {lib().fshost_search_error(self.h).decode()}")
        return [hits[i * K:i * K + nh[i]].copy() for i in range(nq)]

    def _bts(self, res):
        return [lib().fshost_search_backtrace(self.h, C.c_void_p(res[k:k + 1].ctypes.data)).decode() for k in range(len(res))]

    def align_profile(self, entry_aa, entry_3di, target_ids, identity=-1):
        """fshost_search_align_profile -> (records, backtraces) of one profile query"""
        keep, arr = self._pqueries([(entry_aa, entry_3di)])
        t = np.ascontiguousarray(target_ids, np.uint32)
        res = np.zeros(max(1, len(t)), RESULT_DT)
        n = lib().fshost_search_align_profile(self.h, C.cast(arr, C.c_void_p), identity, _ptr(t), len(t), _ptr(res))
        if n < 0:
            e = FsgpuError(f"align_profile rc={n}: {lib().fshost_search_error(self.h).decode()}")
            e.rc = n
            raise e
        return res[:n], self._bts(res[:n])

    def align_batch_profile(self, entries, target_id_lists, identity=None):
        """fshost_search_align_batch_profile; entries: [(AA entry, 3Di entry)] -> ([records], [backtraces]) per query"""
        nq = len(entries)
        keep, arr = self._pqueries(entries)
        ts = [np.ascontiguousarray(x, np.uint32) for x in target_id_lists]
        res = [np.zeros(max(1, len(t)), RESULT_DT) for t in ts]
        P = C.c_void_p * max(nq, 1)
        pt, pr = P(*[x.ctypes.data for x in ts]), P(*[x.ctypes.data for x in res])
        ns = np.array([len(x) for x in ts], np.int32)
        ident = None if identity is None else np.ascontiguousarray(identity, np.int64)
        nres = np.zeros(max(nq, 1), np.int32)
        rc = lib().fshost_search_align_batch_profile(self.h, nq, C.cast(arr, C.c_void_p), _ptr(ident), C.cast(pt, C.c_void_p), _ptr(ns), C.cast(pr, C.c_void_p), _ptr(nres))
        if rc != 0:
            raise FsgpuError(f"align_batch_profile rc={rc}: {lib().fshost_search_error(self.h).decode()}")
        out = [res[i][:nres[i]] for i in range(nq)]
        return out, [self._bts(o) for o in out]

    def align(self, qAA, q3di, target_ids, identity=-1, with_backtrace=False):
        qa = np.ascontiguousarray(qAA, np.uint8)
        q3 = np.ascontiguousarray(q3di, np.uint8)
        t = np.ascontiguousarray(target_ids, np.uint32)
        res = np.zeros(max(1, len(t) * (1 + max(0, self.par.altAlignment))), RESULT_DT)
        n = lib().fshost_search_align(self.h, _ptr(qa), _ptr(q3), len(q3), identity, _ptr(t), len(t), _ptr(res))
        if n < 0:
            raise FsgpuError(f"align rc={n}: {lib().fshost_search_error(self.h).decode()}")
        res = res[:n]
        if with_backtrace:
            bts = [lib().fshost_search_backtrace(self.h, C.c_void_p(res[i:i + 1].ctypes.data)).decode() for i in range(n)]
            return res, bts
        return res

    def align_batch(self, qAAs, q3dis, target_id_lists, identity=None, with_backtrace=False):
        """several queries, one forward + one reversed device pass (fsgpu_sw_multi_dir); returns a list of result arrays (and backtrace lists)"""
        nq = len(q3dis)
        qa = [np.ascontiguousarray(x, np.uint8) for x in qAAs]
        q3 = [np.ascontiguousarray(x, np.uint8) for x in q3dis]
        ts = [np.ascontiguousarray(x, np.uint32) for x in target_id_lists]
        res = [np.zeros(max(1, len(t) * (1 + max(0, self.par.altAlignment))), RESULT_DT) for t in ts]
        P = C.c_void_p * max(nq, 1)
        pa, p3, pt, pr = P(*[x.ctypes.data for x in qa]), P(*[x.ctypes.data for x in q3]), P(*[x.ctypes.data for x in ts]), P(*[x.ctypes.data for x in res])
        Ls = np.array([len(x) for x in q3], np.int32)
        ns = np.array([len(x) for x in ts], np.int32)
        ident = None if identity is None else np.ascontiguousarray(identity, np.int64)
        nres = np.zeros(max(nq, 1), np.int32)
        rc = lib().fshost_search_align_batch(self.h, nq, C.cast(pa, C.c_void_p), C.cast(p3, C.c_void_p), _ptr(Ls), _ptr(ident), C.cast(pt, C.c_void_p),
                                             _ptr(ns), C.cast(pr, C.c_void_p), _ptr(nres))
        if rc != 0:
            raise FsgpuError(f"align_batch rc={rc}: {lib().fshost_search_error(self.h).decode()}")
        out = [res[i][:nres[i]] for i in range(nq)]
        if with_backtrace:
            bts = [[lib().fshost_search_backtrace(self.h, C.c_void_p(out[i][k:k + 1].ctypes.data)).decode() for k in range(len(out[i]))] for i in range(nq)]
            return out, bts
        return out

    def exhaustive_batch(self, qAAs, q3dis, identity=None, with_backtrace=False):
        """fshost_search_exhaustive_batch: every query against EVERY target of the database (Foldseek's --exhaustive-search 1): the score cutoff of the
        first e-value gate per query, one database-wide forward pass with the selection on the device, the survivors through align_batch's body.
        Returns what align_batch returns over target_id_lists = [range(n)] * nq; last_survivors holds the number of targets that reached the aligner
        per query.  Params.maxRejected other than INT_MAX raises FsgpuError with .rc == FSGPU_E_UNSUPPORTED."""
        nq = len(q3dis)
        qa = [np.ascontiguousarray(x, np.uint8) for x in qAAs]
        q3 = [np.ascontiguousarray(x, np.uint8) for x in q3dis]
        P = C.c_void_p * max(nq, 1)
        pa, p3, pr = P(*[x.ctypes.data for x in qa]), P(*[x.ctypes.data for x in q3]), P()
        Ls = np.array([len(x) for x in q3], np.int32)
        ident = None if identity is None else np.ascontiguousarray(identity, np.int64)
        nres = np.zeros(max(nq, 1), np.int32)
        rc = lib().fshost_search_exhaustive_batch(self.h, nq, C.cast(pa, C.c_void_p), C.cast(p3, C.c_void_p), _ptr(Ls), _ptr(ident), C.cast(pr, C.c_void_p), _ptr(nres))
        if rc != 0:
            e = FsgpuError(f"exhaustive_batch rc={rc}: {lib().fshost_search_error(self.h).decode()}")
            e.rc = rc
            raise e
        surv = np.zeros(max(nq, 1), np.int64)
        lib().fshost_search_exhaustive_survivors(self.h, _ptr(surv), nq)
        self.last_survivors = surv[:nq].tolist()
        views = [np.ctypeslib.as_array(C.cast(pr[i], C.POINTER(C.c_uint8)), shape=(int(nres[i]) * RESULT_DT.itemsize,)).view(RESULT_DT) if nres[i] else np.zeros(0, RESULT_DT)
                 for i in range(nq)]
        bts = None
        if with_backtrace:
            bts = [[lib().fshost_search_backtrace(self.h, C.c_void_p(v[k:k + 1].ctypes.data)).decode() for k in range(len(v))] for v in views]
        out = [v.copy() for v in views]
        return (out, bts) if with_backtrace else out

    def rescore_diagonal_batch(self, qAAs, q3dis, target_id_lists, diagonal_lists, identity=None):
        """fshost_search_rescore_diagonal_batch: structurerescorediagonal's per-query body for several queries in ONE library call.  target_id_lists[q] /
        diagonal_lists[q]: first and third column of query q's prefilter lines in their order (diagonals as the int16 the module reads); identity: per
        query the target index that is the query itself, -1 for none, or None.  The handle's Params decide the gates; Params.skipUndefinedDiagonals = 1
        passes over pairs whose reference result is undefined, 0 refuses them (FsgpuError with .rc == FSGPU_E_UNSUPPORTED).
        Returns (records per query, backtrace strings per query).  Every result buffer has room for n[q] records plus one more and is filled with
        RESCORE_CANARY bytes before the call; last_rescore = (the whole buffers, nres) is kept for tests that look behind nres[q]."""
        nq = len(q3dis)
        qa = [np.ascontiguousarray(x, np.uint8) for x in qAAs]
        q3 = [np.ascontiguousarray(x, np.uint8) for x in q3dis]
        ts = [np.ascontiguousarray(x, np.uint32) for x in target_id_lists]
        ds = [np.ascontiguousarray(x, np.int16) for x in diagonal_lists]
        if not (len(qa) == len(ts) == len(ds) == nq) or any(len(t) != len(d) for t, d in zip(ts, ds)) or any(len(a) != len(b) for a, b in zip(qa, q3)):
            raise ValueError("rescore_diagonal_batch: one AA / 3Di query, one id list and one diagonal list of equal length per query")
        res = [np.frombuffer(bytearray([self.RESCORE_CANARY]) * ((len(t) + 1) * RESULT_DT.itemsize), RESULT_DT) for t in ts]
        P = C.c_void_p * max(nq, 1)
        pa, p3, pt, pd, pr = (P(*[x.ctypes.data for x in v]) for v in (qa, q3, ts, ds, res))
        Ls = np.array([len(x) for x in q3], np.int32)
        ns = np.array([len(x) for x in ts], np.int32)
        ident = None if identity is None else np.ascontiguousarray(identity, np.int64)
        nres = np.full(max(nq, 1), -7, np.int32)
        rc = lib().fshost_search_rescore_diagonal_batch(self.h, nq, C.cast(pa, C.c_void_p), C.cast(p3, C.c_void_p), _ptr(Ls), _ptr(ident), C.cast(pt, C.c_void_p),
                                                        C.cast(pd, C.c_void_p), _ptr(ns), C.cast(pr, C.c_void_p), _ptr(nres))
        self.last_rescore = (res, nres[:nq].copy())
        if rc != 0:
            e = FsgpuError(f"rescore_diagonal_batch rc={rc}: {lib().fshost_search_error(self.h).decode()}")
            e.rc = rc
            raise e
        out = [res[i][:nres[i]] for i in range(nq)]
        bts = [[lib().fshost_search_backtrace(self.h, C.c_void_p(out[i][k:k + 1].ctypes.data)).decode() for k in range(len(out[i]))] for i in range(nq)]
        return out, bts

    RESCORE_CANARY = 0xA5

    def kmer_batch(self, m_kmer, m_ungapped, kmer_thr, spaced, qaa_ptrs, q3_ptrs, lens, pref_identity=None, aln_identity=None, max_res=200, min_diag=30,
                   kmer_score_only=False, rows=None):
        """fshost_search_kmer_batch: k-mer prefilter + coverage pre-filter + structure alignment of a batch of queries in ONE library call (the per-batch
        body of the `search` module).  qaa_ptrs / q3_ptrs: uint64 arrays with the host addresses of the queries' code strings (0..20), lens: their lengths.
        Returns a dict: nhits, status, nkept, nres (int32[nq]), hits [nq, max_res], kept [nq, max_res], results [nq, max_res * (1 + alt)], seconds[4].
        rows: that many rows per output array instead of max(nq, 1) (tests: rows behind the last query that the call must leave alone); the arrays start
        out as bytes of 0xA5 then, not as zeros."""
        nq = len(lens)
        pa = np.ascontiguousarray(qaa_ptrs, np.uint64); p3 = np.ascontiguousarray(q3_ptrs, np.uint64)
        Ls = np.ascontiguousarray(lens, np.int32)
        pi = None if pref_identity is None else np.ascontiguousarray(pref_identity, np.int64)
        ai = None if aln_identity is None else np.ascontiguousarray(aln_identity, np.int64)
        sp = KmerSearchParams(max_res, min_diag, 0, 1 if kmer_score_only else 0, 0, 0, 0)
        rcap = max_res * (1 + max(0, self.par.altAlignment))
        n1 = max(nq, 1) if rows is None else max(nq, 1, int(rows))

        def new(shape, dt):
            a = np.zeros(shape, dt)
            if rows is not None:
                a.view(np.uint8)[...] = 0xA5
            return a
        out = {"hits": new((n1, max_res), KMER_HIT_DT), "nhits": new(n1, np.int32), "status": new(n1, np.int32),
               "kept": new((n1, max_res), np.uint32), "nkept": new(n1, np.int32), "results": new((n1, rcap), RESULT_DT),
               "nres": new(n1, np.int32), "seconds": np.zeros(4)}
        rc = lib().fshost_search_kmer_batch(self.h, m_kmer.h, m_ungapped.h, C.cast(C.byref(sp), C.c_void_p), int(kmer_thr), int(spaced), nq, _ptr(pa), _ptr(p3), _ptr(Ls),
                                            _ptr(pi), _ptr(ai), _ptr(out["hits"]), _ptr(out["nhits"]), _ptr(out["status"]), _ptr(out["kept"]), _ptr(out["nkept"]),
                                            _ptr(out["results"]), _ptr(out["nres"]), _ptr(out["seconds"]))
        if rc != 0:
            raise FsgpuError(f"kmer_batch rc={rc}: {lib().fshost_search_error(self.h).decode()}")
        return out

    def kmer_batch_profile(self, entries, kmer_thr, spaced, pref_identity=None, aln_identity=None, max_res=200, min_diag=30, kmer_score_only=False):
        """fshost_search_kmer_batch_profile: the profile form of kmer_batch.  entries: [(AA entry, 3Di entry)] of the profile databases (bytes without the
        terminator).  Returns the same dict as kmer_batch (results [nq, max_res])."""
        nq = len(entries)
        bufs = [(np.frombuffer(bytes(a), np.uint8).copy(), np.frombuffer(bytes(b), np.uint8).copy()) for a, b in entries]
        pa = np.array([a.ctypes.data for a, _ in bufs] + [0], np.uint64); p3 = np.array([b.ctypes.data for _, b in bufs] + [0], np.uint64)
        la = np.array([len(a) for a, _ in bufs] + [0], np.uint64); l3 = np.array([len(b) for _, b in bufs] + [0], np.uint64)
        assert C.sizeof(C.c_size_t) == 8
        pi = None if pref_identity is None else np.ascontiguousarray(pref_identity, np.int64)
        ai = None if aln_identity is None else np.ascontiguousarray(aln_identity, np.int64)
        sp = KmerSearchParams(max_res, min_diag, 0, 1 if kmer_score_only else 0, 0, 0, 0)
        n1 = max(nq, 1)
        out = {"hits": np.zeros((n1, max_res), KMER_HIT_DT), "nhits": np.zeros(n1, np.int32), "status": np.zeros(n1, np.int32),
               "kept": np.zeros((n1, max_res), np.uint32), "nkept": np.zeros(n1, np.int32), "results": np.zeros((n1, max_res), RESULT_DT),
               "nres": np.zeros(n1, np.int32), "seconds": np.zeros(4)}
        rc = lib().fshost_search_kmer_batch_profile(self.h, C.cast(C.byref(sp), C.c_void_p), int(kmer_thr), int(spaced), nq, _ptr(pa), _ptr(la), _ptr(p3), _ptr(l3),
                                                    _ptr(pi), _ptr(ai), _ptr(out["hits"]), _ptr(out["nhits"]), _ptr(out["status"]), _ptr(out["kept"]),
                                                    _ptr(out["nkept"]), _ptr(out["results"]), _ptr(out["nres"]), _ptr(out["seconds"]))
        if rc != 0:
            raise FsgpuError(f"kmer_batch_profile rc={rc}: {lib().fshost_search_error(self.h).decode()}")
        return out

    def set_tm(self, tm_thr=0.0, mode=0, structure_bits=False):
        """fshost_search_set_tm: --tmscore-threshold, --tmscore-threshold-mode (0 alignment, 1 query, 2 target), --sort-by-structure-bits; call it before
        bind_ca"""
        rc = lib().fshost_search_set_tm(self.h, float(tm_thr), int(mode), 1 if structure_bits else 0)
        if rc != 0:
            raise FsgpuError(f"set_tm rc={rc}: mode {mode} is none of 0, 1, 2")

    def bind_ca(self, lddt_thr, entries):
        """fshost_search_bind_ca: --lddt-threshold and the targets' <db>_ca entries (bytes as stored), entries[i] for target INDEX i; entries None unbinds.
        The packed entries stay alive with this object."""
        if entries is None:
            self._ca = None
            rc = lib().fshost_search_bind_ca(self.h, 0.0, None, None, None)
        else:
            lens = np.array([len(e) for e in entries], np.uint32)
            off = np.zeros(len(entries), np.uint64)
            off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
            base = np.frombuffer(b"".join(bytes(e) for e in entries) + b"\0", np.uint8).copy()
            self._ca = (base, off, lens)
            rc = lib().fshost_search_bind_ca(self.h, float(lddt_thr), _ptr(base), _ptr(off), _ptr(lens))
        if rc != 0:
            raise FsgpuError(f"bind_ca rc={rc}: {lib().fshost_search_error(self.h).decode()}")

    def set_query_ca(self, entries):
        """fshost_search_set_query_ca: the <db>_ca entries of the queries of the NEXT align / align_batch / kmer_batch call, in their order (consumed by it)"""
        self._qca = [np.frombuffer(bytes(e) + b"\0", np.uint8).copy() for e in entries]
        lens = np.array([len(e) for e in entries], np.uint32)
        P = C.c_void_p * max(len(entries), 1)
        ptrs = P(*[x.ctypes.data for x in self._qca])
        rc = lib().fshost_search_set_query_ca(self.h, len(entries), C.cast(ptrs, C.c_void_p), _ptr(lens))
        if rc != 0:
            raise FsgpuError(f"set_query_ca rc={rc}")

    def startpos_backtrace(self, qAA, q3di, target_id, q_end, db_end, score):
        """alignStartPosBacktrace (SSW-style start + CIGAR: device reverse pass + host banded trace-back); (ok, qStart, dbStart, ids, cigar)"""
        qa, q3 = np.ascontiguousarray(qAA, np.uint8), np.ascontiguousarray(q3di, np.uint8)
        qs, ds, ident = C.c_int(), C.c_int(), C.c_uint()
        buf = C.create_string_buffer(len(q3) + 70000)
        rc = lib().fshost_search_startpos_backtrace(self.h, _ptr(qa), _ptr(q3), len(q3), int(target_id), int(q_end), int(db_end), int(score),
                                                    C.byref(qs), C.byref(ds), C.byref(ident), buf, len(buf))
        if rc < 0:
            raise FsgpuError(f"startpos_backtrace rc={rc}: {lib().fshost_search_error(self.h).decode()}")
        return rc == 1, qs.value, ds.value, ident.value, buf.value.decode()

    def backtrace_counts(self):
        """last align_batch: (accepted hits answered by the device block aligner, all accepted hits)"""
        a, b = C.c_int64(0), C.c_int64(0)
        lib().fshost_search_backtrace_counts(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def stats(self):
        out = np.zeros(8)
        lib().fshost_search_stats(self.h, _ptr(out))
        return out

    def last_sw(self, n):
        f, r = C.c_void_p(), C.c_void_p()
        lib().fshost_search_last_sw(self.h, C.byref(f), C.byref(r))
        fa = np.ctypeslib.as_array(C.cast(f, C.POINTER(C.c_int32)), (n * 4,)).copy().view(SWRES_DT)
        ra = np.ctypeslib.as_array(C.cast(r, C.POINTER(C.c_int32)), (n * 4,)).copy().view(SWRES_DT)
        return fa, ra

    def format_result(self, r, backtrace=None, add_backtrace=False):
        buf = C.create_string_buffer(1024 + 65536 * 2)
        n = lib().fshost_format_result(buf, C.c_void_p(r.ctypes.data), backtrace.encode() if backtrace else None, int(add_backtrace))
        return buf.raw[:n].decode()

    def close(self):
        if getattr(self, "h", None):
            lib().fshost_search_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def block_backtrace(mAA, m3Di, qAA, q3Di, cbAA, cbSS, tAA, t3Di, q_end, db_end, score, gap_open=10, gap_extend=1):
    """host start position + backtrace of one hit; returns (ok, qStart, dbStart, identicalAA, backtrace)"""
    qa, q3 = np.ascontiguousarray(qAA, np.uint8), np.ascontiguousarray(q3Di, np.uint8)
    ta, t3 = np.ascontiguousarray(tAA, np.uint8), np.ascontiguousarray(t3Di, np.uint8)
    ca, cs = np.ascontiguousarray(cbAA, np.int8), np.ascontiguousarray(cbSS, np.int8)
    qs, ds, ident = C.c_int(), C.c_int(), C.c_uint()
    buf = C.create_string_buffer(len(qa) + len(ta) + 8)
    ok = lib().fshost_block_backtrace(mAA.h, m3Di.h, _ptr(qa), _ptr(q3), _ptr(ca), _ptr(cs), len(qa), _ptr(ta), _ptr(t3), len(ta),
                                      int(q_end), int(db_end), int(score), gap_open, gap_extend, C.byref(qs), C.byref(ds), C.byref(ident),
                                      buf, len(buf))
    return bool(ok), qs.value, ds.value, ident.value, buf.value.decode()


def banded_backtrace(mAA, m3Di, qAA, q3Di, cbAA, cbSS, tAA, t3Di, q_start, q_end, db_start, db_end, score, gap_open=10, gap_extend=1):
    """host banded_sw + computerBacktrace of a pair with known start and end cells; returns (ok, identicalAA, backtrace)"""
    qa, q3 = np.ascontiguousarray(qAA, np.uint8), np.ascontiguousarray(q3Di, np.uint8)
    ta, t3 = np.ascontiguousarray(tAA, np.uint8), np.ascontiguousarray(t3Di, np.uint8)
    ca, cs = np.ascontiguousarray(cbAA, np.int8), np.ascontiguousarray(cbSS, np.int8)
    ident = C.c_uint()
    buf = C.create_string_buffer(len(qa) + len(ta) + 8)
    ok = lib().fshost_banded_backtrace(mAA.h, m3Di.h, _ptr(qa), _ptr(q3), _ptr(ca), _ptr(cs), _ptr(ta), _ptr(t3), int(q_start), int(q_end), int(db_start),
                                       int(db_end), int(score), gap_open, gap_extend, C.byref(ident), buf, len(buf))
    return ok == 1, ident.value, buf.value.decode()


def set_host_workers(n):
    """size of the process-wide host pool that computes the per-hit backtraces (0: the calling threads do it themselves)"""
    lib().fshost_set_host_workers(int(n))


def host_workers():
    return int(lib().fshost_host_workers())


def default_params():
    p = Params()
    lib().fshost_params_default(C.byref(p))
    return p


def format_prefilter_hit(key, score, diagonal=0):
    buf = C.create_string_buffer(64)
    n = lib().fshost_format_prefilter_hit(buf, key, score, diagonal)
    return buf.raw[:n].decode()


def ca_decode(entry, L):
    """fshost_ca_decode (Coordinate16::read): a <db>_ca entry (bytes, as stored: terminator included or not) of a chain of L residues ->
    float32 [3, L] (x, y, z rows)"""
    buf = np.frombuffer(bytes(entry), np.uint8)
    out = np.zeros((3, int(L)), np.float32)
    if lib().fshost_ca_decode(_ptr(buf), len(buf), int(L), _ptr(out)) != 0:
        raise FsgpuError(f"ca_decode: an entry of {len(buf)} bytes is too short for {L} residues")
    return out


def profile_decode(entry):
    """fshost_profile_decode (Sequence::mapProfile): the bytes of a profile entry without its terminator -> (codes uint8 [L], consensus uint8 [L],
    profile int8 [21, L], reversed profile int8 [21, L]).  A damaged entry raises FsgpuError with the library's reason."""
    buf = np.frombuffer(bytes(entry), np.uint8)
    err = C.create_string_buffer(256)
    L = lib().fshost_profile_decode(_ptr(buf) if len(buf) else None, len(buf), None, None, None, None, err, len(err))
    if L < 0:
        raise FsgpuError(err.value.decode())
    codes, cons = np.zeros(L, np.uint8), np.zeros(L, np.uint8)
    prof, rev = np.zeros((21, L), np.int8), np.zeros((21, L), np.int8)
    if L and lib().fshost_profile_decode(_ptr(buf), len(buf), _ptr(codes), _ptr(cons), _ptr(prof), _ptr(rev), err, len(err)) != L:
        raise FsgpuError(err.value.decode())
    return codes, cons, prof, rev


def profile_decode_raw(entry):
    """fshost_profile_decode_raw: profile_decode's four arrays and the raw score rows int8 [L, 20] the k-mer generator reads"""
    buf = np.frombuffer(bytes(entry), np.uint8)
    err = C.create_string_buffer(256)
    L = lib().fshost_profile_decode_raw(_ptr(buf) if len(buf) else None, len(buf), None, None, None, None, None, err, len(err))
    if L < 0:
        raise FsgpuError(f"profile_decode_raw rc={L}: {err.value.decode()}")
    codes = np.zeros(L, np.uint8); cons = np.zeros(L, np.uint8); prof = np.zeros((21, L), np.int8); rev = np.zeros((21, L), np.int8)
    raw = np.zeros((L, 20), np.int8)
    if L and lib().fshost_profile_decode_raw(_ptr(buf), len(buf), _ptr(codes), _ptr(cons), _ptr(prof), _ptr(rev), _ptr(raw), err, len(err)) != L:
        raise FsgpuError("profile_decode_raw: inconsistent length")
    return codes, cons, prof, rev, raw


def kmer_threshold_profile(sensitivity=9.5, kmer_size=6, context_pseudo_counts=True):
    """fshost_kmer_threshold_profile: Prefiltering::getKmerThreshold for a profile query"""
    return lib().fshost_kmer_threshold_profile(sensitivity, kmer_size, 1 if context_pseudo_counts else 0)


def kmer_query_prepare_profile(entry_3di, kmer_thr, kmer_size=6, spaced=1):
    """fshost_kmer_query_prepare_profile -> (seq uint8[L], scores int8[L,20], profile int8[L,21], threshold) for Context.kmer_search_profile"""
    buf = np.frombuffer(bytes(entry_3di), np.uint8)
    err = C.create_string_buffer(256)
    if len(buf) % 25:
        raise FsgpuError("kmer_query_prepare_profile: the entry is no multiple of the record size")
    L = len(buf) // 25
    codes = np.zeros(L, np.uint8); raw = np.zeros((L, 20), np.int8); prof = np.zeros((L, 21), np.int8)
    thr = C.c_int32(0)
    n = lib().fshost_kmer_query_prepare_profile(_ptr(buf) if L else None, len(buf), int(kmer_thr), int(kmer_size), int(spaced), _ptr(codes), _ptr(raw), _ptr(prof),
                                                C.cast(C.byref(thr), C.c_void_p), err, len(err))
    if n < 0:
        raise FsgpuError(f"kmer_query_prepare_profile rc={n}: {err.value.decode()}")
    return codes, raw, prof, int(thr.value)


def kmer_profile_sort_rows(scores):
    """fsgpu_kmer_profile_sort_rows (host only): int8 [L, 20] -> (sorted scores int16 [L, 20], letters uint8 [L, 20]) as the device reads the rows"""
    sc = np.ascontiguousarray(scores, np.int8).reshape(-1, 20)
    rows = np.zeros((len(sc), 20), np.uint16)
    rc = lib().fsgpu_kmer_profile_sort_rows(_ptr(sc), len(sc), _ptr(rows))
    if rc != 0:
        raise FsgpuError(f"fsgpu_kmer_profile_sort_rows rc={rc}")
    return (rows.view(np.int16) >> 8).astype(np.int16), (rows & 0xff).astype(np.uint8)


def profile_bias(profile):
    """fshost_profile_bias: the bias of ssw_init's profile branch for an int8 [21, L] alignment profile; the gapless scan's cap is 255 - bias"""
    p = np.ascontiguousarray(profile, np.int8).reshape(21, -1)
    return lib().fshost_profile_bias(_ptr(p), p.shape[1])


def lddt_average(cols):
    """fshost_lddt_average (LDDTScoreResult, LDDT.h:102-119): (avgLddtScore, scoreLength) of the per-column values of one hit"""
    c = np.ascontiguousarray(cols, np.float32)
    n = C.c_int(0)
    avg = lib().fshost_lddt_average(_ptr(c), len(c), C.byref(n))
    return avg, n.value


def tm_params(norm_len):
    """fshost_tm_params: (score_d8, d0 of standard_TMscore, d0, d0_search) for a normalisation length, float32 [4]"""
    out = np.zeros(4, np.float32)
    lib().fshost_tm_params(int(norm_len), _ptr(out))
    return out


def tm_exact_params(norm_len):
    """fshost_tm_exact_params: (score_d8, Lnorm, d0, d0_search) of the exact mode for a normalisation length, float32 [4]"""
    out = np.zeros(4, np.float32)
    lib().fshost_tm_exact_params(int(norm_len), _ptr(out))
    return out


def tm_exact_finish(pairs, score, raw_rms):
    """fshost_tm_exact_finish: (TM-score as a double, rmsd as numpy float32) from the raw values of an exact-mode task"""
    rmsd = np.zeros(1, np.float32)
    tm = lib().fshost_tm_exact_finish(int(pairs), float(np.float32(score)), float(np.float32(raw_rms)), _ptr(rmsd))
    return tm, rmsd[0]


def tm_finish(pairs, s1, s2, norm_len):
    """fshost_tm_finish: the TM-score (a double) from the raw values Context.tm_batch returns"""
    return lib().fshost_tm_finish(int(pairs), float(np.float32(s1)), float(np.float32(s2)), int(norm_len))


def tm_normalization(mode, alignment_len, query_len, target_len):
    """fshost_tm_normalization (TMaligner::normalization)"""
    return lib().fshost_tm_normalization(int(mode), int(alignment_len), int(query_len), int(target_len))
