"""ctypes binding of lib/libdctzhip.so (include/dctz_hip.h).

torch is used only for device buffers and the stream; every compute call goes
through the C ABI.  No fallback: a missing library or GPU raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64 = 0, 1
EC, QT = 0, 1
OK, E_ARG, E_BOUND, E_HIP, E_INTERNAL, E_SPACE = 0, -1, -2, -3, -4, -5      # DCTZHIP_OK / DCTZHIP_E_*


class DctzHipError(RuntimeError):
    pass


def lib_path():
    return os.environ.get("DCTZHIP_LIBRARY") or os.path.join(_HERE, "lib", "libdctzhip.so")   # override: A/B builds of the library


MISS_NAN, MISS_INF, MISS_VALUE, MISS_ABS_GE = 1, 2, 4, 8      # DCTZHIP_MISS_*


class Missing(C.Structure):          # dctzhip_missing
    _fields_ = [("flags", C.c_uint), ("value", C.c_double), ("limit", C.c_double)]


class CompressInfo(C.Structure):
    _fields_ = [("sf", C.c_double), ("mean", C.c_double), ("max_abs", C.c_double),
                ("min_abs", C.c_double), ("cnt", C.c_uint32), ("nblk", C.c_uint32),
                ("qtable", C.c_double * 64), ("qtable_raw", C.c_double * 64),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


INFO_STATS_FUSED = 1   # sampled guess of sf verified: the separate statistics pass was saved
INFO_RESPUN = 2        # guess wrong: the compress kernels ran a second time with the true statistics
INFO_SPLIT = 8         # the compress kernel was k_compress_eo (a block over two lanes)
INFO_SINGLE_PASS = 16  # ... and AC_exact was placed by that kernel itself (no k_compact_ac)
INFO_LB_FALLBACK = 32  # ... whose look-back gave up: the pass ran again through the lists
INFO_ONE_LAUNCH = 4    # the whole call was one kernel (arrays whose tiles are all resident at once: dctz_kernels_one.hip)


class Timings(C.Structure):
    _fields_ = [("stats_ms", C.c_float), ("main_ms", C.c_float), ("tail_ms", C.c_float),
                ("total_ms", C.c_float)]


class BatchCItem(C.Structure):       # dctzhip_batch_citem
    _fields_ = [("d_in", C.c_void_p), ("n", C.c_size_t), ("dtype", C.c_int), ("error_bound", C.c_double),
                ("d_bin_index", C.c_void_p), ("d_dc", C.c_void_p), ("d_ac_exact", C.c_void_p), ("d_scaled", C.c_void_p)]


class BatchDItem(C.Structure):       # dctzhip_batch_ditem
    _fields_ = [("d_bin_index", C.c_void_p), ("d_dc", C.c_void_p), ("d_ac_exact", C.c_void_p), ("ac_count", C.c_uint32),
                ("qtable_host", C.c_void_p), ("n", C.c_size_t), ("dtype", C.c_int), ("error_bound", C.c_double),
                ("sf", C.c_double), ("d_out", C.c_void_p)]


class RdPoint(C.Structure):          # dctzhip_rd_point
    _fields_ = [("error_bound", C.c_double), ("cnt", C.c_uint64), ("sse", C.c_double), ("psnr", C.c_double),
                ("raw_bytes", C.c_uint64)]


BOX_MAXDIM = 4                       # DCTZHIP_BOX_MAXDIM
BOXES_MAX = 4096                     # DCTZHIP_BOXES_MAX: boxes per dctzhip_decompress_boxes call


class BoxItem(C.Structure):          # dctzhip_box_item
    _fields_ = [("lo", C.c_size_t * BOX_MAXDIM), ("hi", C.c_size_t * BOX_MAXDIM), ("d_out", C.c_void_p)]


class TileSummary(C.Structure):      # dctzhip_tile_summary_t: one record per 4096-element tile, or the records joined
    _fields_ = [("rmin", C.c_double), ("rmax", C.c_double), ("rsum", C.c_double), ("rsq", C.c_double),
                ("xmin", C.c_double), ("xmax", C.c_double), ("emax", C.c_double), ("esq", C.c_double)]

    def psnr(self, n):
        """calc_psnr (util.c:54-104) of a total taken with the original: 20 log10((xmax - xmin) / sqrt(esq / n))."""
        return 20.0 * float(np.log10((self.xmax - self.xmin) / np.sqrt(self.esq / n)))


RD_MAXK = 16                         # DCTZHIP_RD_MAXK: bounds per dctzhip_rd_probe call


def psnr_grid():
    """The candidate bounds of dctzhip_compress_psnr, ascending (include/dctz_hip.h): m * 10^e for e = -6 .. -1, then 1."""
    return [float(f"{m}e{e}") for e in range(-6, 0) for m in ("1", "1.25", "1.5", "2", "2.5", "3", "4", "5", "6", "8")] + [1.0]


_lib = None

_PROTOS = {
    "dctzhip_device_count": (C.c_int, []),
    "dctzhip_ctx_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "dctzhip_ctx_destroy": (None, [C.c_void_p]),
    "dctzhip_last_error": (C.c_char_p, [C.c_void_p]),
    "dctzhip_reserve": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    "dctzhip_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dctzhip_use_own_stream": (C.c_int, [C.c_void_p]),
    "dctzhip_get_stream": (C.c_void_p, [C.c_void_p]),
    "dctzhip_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "dctzhip_last_timings": (C.c_int, [C.c_void_p, C.POINTER(Timings)]),
    "dctzhip_set_speculation": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t]),
    "dctzhip_set_spec_memory": (C.c_int, [C.c_void_p, C.c_int]),
    "dctzhip_set_one_launch": (C.c_int, [C.c_void_p, C.c_int]),
    "dctzhip_set_split": (C.c_int, [C.c_void_p, C.c_int]),
    "dctzhip_set_decode_memo": (C.c_int, [C.c_void_p, C.c_int]),
    "dctzhip_debug_counter": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]),
    "dctzhip_debug_knob": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "dctzhip_debug_last_kernel": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]),
    "dctzhip_malloc": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]),
    "dctzhip_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dctzhip_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dctzhip_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "dctzhip_sync": (C.c_int, [C.c_void_p]),
    "dctzhip_host_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "dctzhip_host_unregister": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dctzhip_compress": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(CompressInfo)]),
    "dctzhip_decompress": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int,
                                     C.c_void_p]),
    "dctzhip_ac_index_len": (C.c_size_t, [C.c_size_t]),
    "dctzhip_ac_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32)]),
    "dctzhip_decompress_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_size_t,
                                           C.c_size_t, C.c_void_p]),
    "dctzhip_decompress_box": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]),
    "dctzhip_decompress_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                           C.POINTER(C.c_size_t), C.c_int, C.c_void_p]),
    "dctzhip_set_blocking": (C.c_int, [C.c_void_p, C.c_int]),
    "dctzhip_compress_batch": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(BatchCItem), C.c_int, C.POINTER(CompressInfo)]),
    "dctzhip_decompress_batch": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(BatchDItem), C.c_int, C.POINTER(C.c_int)]),
    "dctzhip_last_batch_timings": (C.c_int, [C.c_void_p, C.POINTER(Timings)]),
    "dctzhip_nd_blocks": (C.c_size_t, [C.c_int, C.POINTER(C.c_size_t)]),
    "dctzhip_compress_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CompressInfo)]),
    "dctzhip_decompress_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]),
    "dctzhip_decompress_box_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_double, C.c_int,
                                            C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]),
    "dctzhip_decompress_boxes_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_double, C.c_int,
                                              C.c_int, C.c_void_p]),
    "dctzhip_coarse_len": (C.c_size_t, [C.c_size_t, C.c_int]),
    "dctzhip_decompress_coarse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]),
    "dctzhip_decompress_coarse_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                               C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                               C.c_void_p]),
    "dctzhip_decompress_coarse_box_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                   C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                                   C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]),
    "dctzhip_decompress_coarse_boxes_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                     C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                                     C.c_int, C.c_void_p]),
    "dctzhip_summary_tiles": (C.c_size_t, [C.c_size_t]),
    "dctzhip_tile_summary": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                       C.POINTER(TileSummary)]),
    "dctzhip_tile_summary_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p,
                                          C.c_void_p, C.POINTER(TileSummary)]),
    "dctzhip_fixup_tiles": (C.c_size_t, [C.c_size_t]),
    "dctzhip_fixup_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_double, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "dctzhip_fixup_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_int, C.c_int,
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]),
    "dctzhip_fixup_build_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p,
                                         C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "dctzhip_fixup_apply_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                         C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]),
    "dctzhip_mask_words": (C.c_size_t, [C.c_size_t]),
    "dctzhip_mask_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Missing), C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_uint64)]),
    "dctzhip_mask_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_size_t),
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]),
    "dctzhip_compress_masked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int, C.POINTER(Missing),
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CompressInfo),
                                          C.POINTER(C.c_uint64)]),
    "dctzhip_mask_build_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.c_int, C.POINTER(Missing),
                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "dctzhip_compress_masked_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_int,
                                             C.POINTER(Missing), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(CompressInfo), C.POINTER(C.c_uint64)]),
    "dctzhip_dct_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    "dctzhip_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(CompressInfo)]),
    "dctzhip_serial_mean_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "dctzhip_serial_mean_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "dctzhip_scale_inplace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double]),
    "dctzhip_debug_divide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_void_p,
                                       C.c_void_p]),
    "dctzhip_psnr_terms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "dctzhip_rd_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double),
                                   C.POINTER(RdPoint), C.POINTER(C.c_double)]),
    "dctzhip_compress_psnr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(CompressInfo), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dctzhip_rd_probe_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_int,
                                      C.POINTER(C.c_double), C.POINTER(RdPoint), C.POINTER(C.c_double)]),
    "dctzhip_compress_psnr_nd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_double, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.POINTER(CompressInfo), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]),
    "dctzhip_deflate_bound": (C.c_size_t, [C.c_size_t]),
    "dctzhip_deflate_chunk_bytes": (C.c_size_t, []),
    "dctzhip_deflate_ex": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_uint)]),
    "dctzhip_inflate": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "dctzhip_deflate": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p)]),
    "dctzhip_comm_unique_id": (C.c_int, [C.c_void_p]),
    "dctzhip_comm_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dctzhip_comm_destroy": (C.c_int, [C.c_void_p]),
    "dctzhip_comm_sizes": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "dctzhip_comm_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "dctzhip_compress_part": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dctzhip_h2d_pipe_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]),
    "dctzhip_h2d_pipe_wait": (C.c_int, [C.c_void_p, C.c_size_t]),
    "dctzhip_h2d_pipe_landed": (C.c_int, [C.c_void_p, C.c_size_t]),
    "dctzhip_h2d_pipe_end": (C.c_int, [C.c_void_p, C.c_int]),
    "dctzhip_version": (C.c_char_p, []),
}


def load_library():
    """Loads libdctzhip.so; raises DctzHipError if it has not been built."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise DctzHipError(f"{p} is missing: run `make -C dctz_amd` (or __graft_entry__.build()); "
                               "there is no CPU fallback")
        lib = C.CDLL(p)
        for name, (res, args) in _PROTOS.items():
            try:
                fn = getattr(lib, name)      # AttributeError if the ABI lost a symbol
            except AttributeError:
                if os.environ.get("DCTZHIP_LIBRARY"):      # an older A/B build of the library: that entry point is just absent
                    continue
                raise
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _dt(torch_dtype):
    import torch
    if torch_dtype == torch.float64:
        return F64
    if torch_dtype == torch.float32:
        return F32
    raise TypeError(f"unsupported dtype {torch_dtype}")


def _host_ptr(a):
    """A numpy array (or None) as a const void* argument; the caller keeps the array alive over the call."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """One dctzhip context on a GPU; kernels run on torch's current stream (bound before every call: the raw
    handle, where 0 = the legacy default stream, goes to dctzhip_set_stream as is).  When the current stream is another
    one than the last call ran on, the new stream first waits for the old one (include/dctz_hip.h, dctzhip_set_stream:
    the context's scratch and control blocks are ordered by the stream it ran on)."""

    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise DctzHipError("no GPU visible: the DCTZ hot path has no CPU fallback")
        self.lib = load_library()
        self.torch = torch
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        rc = self.lib.dctzhip_ctx_create(C.byref(h), device)
        if rc != 0:
            raise DctzHipError(f"dctzhip_ctx_create: {self.lib.dctzhip_last_error(None).decode()}")
        self.h = h
        self._bound = object()            # nothing bound yet
        self._stream = None               # the torch Stream that was bound (kept alive: the next hop waits for it)
        self._bind_stream()

    def _bind_stream(self):
        # the raw handle of torch's current stream on this device (the private accessor skips the
        # Stream object; fall back to the public API if it is not there)
        try:
            s = self.torch._C._cuda_getCurrentRawStream(self.device.index)
        except AttributeError:
            s = self.torch.cuda.current_stream(self.device).cuda_stream
        if s != self._bound:
            cur = self.torch.cuda.current_stream(self.device)
            if self._stream is not None:
                cur.wait_stream(self._stream)             # the last call's tail kernels still use the context's scratch
            self.lib.dctzhip_set_stream(self.h, C.c_void_p(s))
            self._bound, self._stream = s, cur

    def close(self):
        if getattr(self, "h", None):
            self.lib.dctzhip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise DctzHipError(f"{what} failed ({rc}): {self.lib.dctzhip_last_error(self.h).decode()}")

    def set_profiling(self, on=True):
        self._check(self.lib.dctzhip_set_profiling(self.h, int(on)), "set_profiling")

    def set_speculation(self, on=True, min_elements=0):
        """Fused statistics behind a sampled guess of sf (include/dctz_hip.h, DCTZHIP_INFO_*)."""
        self._check(self.lib.dctzhip_set_speculation(self.h, int(on), int(min_elements)), "set_speculation")

    def set_spec_memory(self, on=True):
        """The sf guess from the last verified statistics of the same input instead of a sample (include/dctz_hip.h); counters 18 / 19."""
        self._check(self.lib.dctzhip_set_spec_memory(self.h, int(on)), "set_spec_memory")

    def set_one_launch(self, on=True):
        """One kernel per call for arrays whose tiles are all resident at once (include/dctz_hip.h); off: the chain of kernels."""
        self._check(self.lib.dctzhip_set_one_launch(self.h, int(on)), "set_one_launch")

    def set_split(self, on=True):
        """k_compress_eo (a block over two lanes) for flat fp64 arrays on the chain of kernels (include/dctz_hip.h)."""
        self._check(self.lib.dctzhip_set_split(self.h, int(on)), "set_split")

    def set_decode_memo(self, on=True):
        """A decode of the streams the last compress call wrote takes that call's tile counts, checked in the kernel (include/dctz_hip.h)."""
        self._check(self.lib.dctzhip_set_decode_memo(self.h, int(on)), "set_decode_memo")

    def counter(self, which):
        """dctzhip_debug_counter (include/dctz_hip.h): 0 one-launch calls, 1 launches that gave up, 2 cooldown, 3 split calls, ...,
        20 fast_sf | fast_bw << 8 of the last verified pass of the last compress / compress_nd call (which division and
        binning variant the kernels ran)."""
        v = C.c_ulonglong(0)
        self._check(self.lib.dctzhip_debug_counter(self.h, int(which), C.byref(v)), "debug_counter")
        return int(v.value)

    def last_kernel(self, which):
        """The name rocprofv3 lists the big kernel of the last call under (0 compress, 1 decompress, 2-5 batches)."""
        buf = C.create_string_buffer(128)
        self._check(self.lib.dctzhip_debug_last_kernel(self.h, int(which), buf, 128), "debug_last_kernel")
        return buf.value.decode()

    def knob(self, key, value):
        """dctzhip_debug_knob (include/dctz_hip.h): 0 withhold a granule, 1 a look-back gives up, 2 the one-launch cooldown,
        3 the divisor of predicted SSEs, 4 the tag of the last one-launch kernel (its 32 bits: 2**32 - 3 and -3 are the same)."""
        value = int(value)
        if key == 4:
            value = ((value & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000      # the 32 bits as the C int that carries them
        self._check(self.lib.dctzhip_debug_knob(self.h, int(key), int(value)), "debug_knob")

    def set_blocking(self, on=True):
        """Calls return only when their outputs are complete for any observer (default: complete in stream order)."""
        self._check(self.lib.dctzhip_set_blocking(self.h, int(on)), "set_blocking")

    def timings(self):
        t = Timings()
        self._check(self.lib.dctzhip_last_timings(self.h, C.byref(t)), "last_timings")
        return {"stats_ms": t.stats_ms, "main_ms": t.main_ms, "tail_ms": t.tail_ms, "total_ms": t.total_ms}

    def reserve(self, n, dtype, mode):
        self._check(self.lib.dctzhip_reserve(self.h, n, _dt(dtype), mode), "reserve")

    def alloc_outputs(self, n, dtype=None):
        t = self.torch
        nblk = (n + 63) // 64
        return {"bin_index": t.empty(n, dtype=t.uint8, device=self.device),
                "dc": t.empty(nblk, dtype=t.float32, device=self.device),
                "ac_exact": t.empty(n, dtype=t.float32, device=self.device)}

    def compress(self, x, eb, mode=EC, out=None, scaled=None, coef=None):
        """x: 1-D contiguous CUDA tensor (float32|float64).  Returns (out, info)."""
        assert x.is_cuda and x.is_contiguous() and x.dim() == 1
        self._bind_stream()
        n = x.numel()
        if out is None:
            out = self.alloc_outputs(n, x.dtype)
        info = CompressInfo()
        rc = self.lib.dctzhip_compress(
            self.h, x.data_ptr(), n, _dt(x.dtype), float(eb), mode, out["bin_index"].data_ptr(),
            out["dc"].data_ptr(), out["ac_exact"].data_ptr(),
            scaled.data_ptr() if scaled is not None else None,
            coef.data_ptr() if coef is not None else None, C.byref(info))
        self._check(rc, "dctzhip_compress")
        return out, info

    # ---- the same two calls on fixed buffers, their arguments converted once (timing loops: what a C caller's loop costs,
    # without a dozen tensor-attribute look-ups and a fresh 1 KiB info structure per call on the Python side)
    def prepare_pair(self, x, out, dst, eb, mode=EC):
        assert x.is_cuda and x.is_contiguous() and x.dim() == 1 and dst.numel() == x.numel() and dst.dtype == x.dtype
        self._bind_stream()
        info = CompressInfo()
        vp, n, dt = C.c_void_p, x.numel(), _dt(x.dtype)
        b, d, a = vp(out["bin_index"].data_ptr()), vp(out["dc"].data_ptr()), vp(out["ac_exact"].data_ptr())
        cargs = (self.h, vp(x.data_ptr()), C.c_size_t(n), C.c_int(dt), C.c_double(float(eb)), C.c_int(mode), b, d, a, None, None, C.byref(info))
        qtab = None
        if mode == QT:                                   # the call's table in the element type, refreshed from info per call
            qtab = (C.c_double * 64)() if x.dtype == self.torch.float64 else (C.c_float * 64)()
        dhead = (self.h, b, d, a)
        dtail = (C.c_size_t(n), C.c_int(dt), C.c_double(float(eb)))
        return {"info": info, "cargs": cargs, "dhead": dhead, "dtail": dtail, "qtab": qtab, "mode": C.c_int(mode), "dst": vp(dst.data_ptr()),
                "keep": (x, out, dst)}

    def compress_prepared(self, pp):
        rc = self.lib.dctzhip_compress(*pp["cargs"])
        if rc:
            self._check(rc, "dctzhip_compress")
        return pp["info"]

    def decompress_prepared(self, pp):
        info, q = pp["info"], pp["qtab"]
        if q is not None:
            q[:] = info.qtable[:]
        rc = self.lib.dctzhip_decompress(*pp["dhead"], info.cnt, q, *pp["dtail"], info.sf, pp["mode"], pp["dst"])
        if rc:
            self._check(rc, "dctzhip_decompress")

    def compress_part(self, x, eb, max_abs, min_abs, out, lo, ac_at):
        """Elements of one part of an array (x: the part, a 1-D CUDA tensor that starts on a block boundary `lo` of the
        array) with the ARRAY's max|x| / min|x|: its streams go to their places in `out` (the array's outputs), the exact
        coefficients at ac_at.  Returns (cnt, (max|x|, min|x|, sum from the second element on), sf)."""
        assert x.is_cuda and x.is_contiguous() and x.dim() == 1 and lo % 64 == 0
        self._bind_stream()
        cnt, st, sf = C.c_uint32(0), (C.c_double * 3)(), C.c_double(0.0)
        rc = self.lib.dctzhip_compress_part(
            self.h, x.data_ptr(), x.numel(), _dt(x.dtype), float(eb), float(max_abs), float(min_abs),
            out["bin_index"].data_ptr() + lo, out["dc"].data_ptr() + 4 * (lo // 64), out["ac_exact"].data_ptr() + 4 * int(ac_at),
            C.byref(cnt), st, C.byref(sf))
        self._check(rc, "dctzhip_compress_part")
        return cnt.value, (st[0], st[1], st[2]), sf.value

    def decompress(self, out, cnt, n, dtype, eb, sf, mode=EC, qtable=None, dst=None):
        t = self.torch
        self._bind_stream()
        if dst is None:
            dst = t.empty(n, dtype=dtype, device=self.device)
        q = self._qtable(mode, qtable, dtype)
        rc = self.lib.dctzhip_decompress(
            self.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(),
            int(cnt), _host_ptr(q), n, _dt(dtype),
            float(eb), float(sf), mode, dst.data_ptr())
        self._check(rc, "dctzhip_decompress")
        return dst

    # ---- random access on decode (include/dctz_hip.h: dctzhip_ac_index / dctzhip_decompress_range) ----
    def ac_index(self, out, n):
        """Exception index of the streams `out` (their bin_index) of an n-element array: (index, total), index an int32
        CUDA tensor of ceil(n / 4096) + 1 entries (idx[i] = exact coefficients in front of element 4096 i), total = idx[-1]."""
        self._bind_stream()
        idx = self.torch.empty(int(self.lib.dctzhip_ac_index_len(n)), dtype=self.torch.int32, device=self.device)
        tot = C.c_uint32(0)
        rc = self.lib.dctzhip_ac_index(self.h, out["bin_index"].data_ptr(), n, idx.data_ptr(), C.byref(tot))
        self._check(rc, "dctzhip_ac_index")
        return idx, tot.value

    def decompress_range(self, out, cnt, n, dtype, eb, sf, lo, hi, index, mode=EC, qtable=None, dst=None):
        """Elements [lo, hi) of what decompress() rebuilds from the same arguments, bit for bit; `index` from ac_index().
        Returns dst (hi - lo elements)."""
        t = self.torch
        self._bind_stream()
        if dst is None:
            dst = t.empty(max(int(hi) - int(lo), 0), dtype=dtype, device=self.device)
        q = self._qtable(mode, qtable, dtype)
        rc = self.lib.dctzhip_decompress_range(
            self.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(), int(cnt),
            index.data_ptr(), _host_ptr(q), n, _dt(dtype), float(eb), float(sf),
            mode, int(lo), int(hi), dst.data_ptr())
        self._check(rc, "dctzhip_decompress_range")
        return dst

    # flat and tiled boxes through one body per operation.  What differs is where the C call takes its geometry: a flat call
    # has n in front of (dtype, eb, sf, mode) and the shape behind them, a tiled call the shape in front.
    def _decompress_box(self, flat, out, cnt, dims, dtype, eb, sf, lo, hi, index, mode, qtable, dst):
        t = self.torch
        self._bind_stream()
        dims, lo, hi = [int(v) for v in dims], [int(v) for v in lo], [int(v) for v in hi]
        nd = len(dims)
        assert len(lo) == nd and len(hi) == nd
        ext = [max(h - l, 0) for l, h in zip(lo, hi)]
        if dst is None:
            dst = t.empty(ext, dtype=dtype, device=self.device)
        q = self._qtable(mode, qtable, dtype)
        arr = C.c_size_t * max(nd, 1)
        b, d, a, ix, qp = out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(), index.data_ptr(), _host_ptr(q)
        if flat:
            name = "dctzhip_decompress_box"
            n = int(np.prod(dims, dtype=np.int64)) if nd else 0
            rc = self.lib.dctzhip_decompress_box(self.h, b, d, a, int(cnt), ix, qp, n, _dt(dtype), float(eb), float(sf),
                                                 mode, nd, arr(*dims), arr(*lo), arr(*hi), dst.data_ptr())
        else:
            name = "dctzhip_decompress_box_nd"
            rc = self.lib.dctzhip_decompress_box_nd(self.h, b, d, a, int(cnt), ix, qp, nd, arr(*dims), _dt(dtype),
                                                    float(eb), float(sf), mode, arr(*lo), arr(*hi), dst.data_ptr())
        self._check(rc, name)
        return dst.view(ext)

    def _box_items(self, nd, boxes, dtype, dsts):
        """The host table of a list call: (items, dsts, extents) of the boxes (lo, hi); `dsts` None: allocated."""
        t = self.torch
        boxes = [([int(v) for v in lo], [int(v) for v in hi]) for lo, hi in boxes]
        exts = []
        for lo, hi in boxes:
            assert len(lo) == nd and len(hi) == nd
            exts.append([max(h - l, 0) for l, h in zip(lo, hi)])
        if dsts is None:
            dsts = [t.empty(e, dtype=dtype, device=self.device) for e in exts]
        assert len(dsts) == len(boxes)
        items = (BoxItem * max(len(boxes), 1))()
        for it, (lo, hi), d in zip(items, boxes, dsts):
            for i in range(min(nd, BOX_MAXDIM)):
                it.lo[i], it.hi[i] = lo[i], hi[i]
            it.d_out = d.data_ptr()
        return items, dsts, exts

    def _decompress_boxes(self, flat, out, cnt, dims, dtype, eb, sf, boxes, index, mode, qtable, dsts):
        self._bind_stream()
        dims = [int(v) for v in dims]
        nd = len(dims)
        items, dsts, exts = self._box_items(nd, boxes, dtype, dsts)
        q = self._qtable(mode, qtable, dtype)
        arr = C.c_size_t * max(nd, 1)
        b, d, a, ix, qp = out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(), index.data_ptr(), _host_ptr(q)
        if flat:
            name = "dctzhip_decompress_boxes"
            n = int(np.prod(dims, dtype=np.int64)) if nd else 0
            rc = self.lib.dctzhip_decompress_boxes(self.h, b, d, a, int(cnt), ix, qp, n, _dt(dtype), float(eb), float(sf),
                                                   mode, nd, arr(*dims), len(dsts), C.cast(items, C.c_void_p))
        else:
            name = "dctzhip_decompress_boxes_nd"
            rc = self.lib.dctzhip_decompress_boxes_nd(self.h, b, d, a, int(cnt), ix, qp, nd, arr(*dims), _dt(dtype),
                                                      float(eb), float(sf), mode, len(dsts), C.cast(items, C.c_void_p))
        self._check(rc, name)
        return [d.view(e) for d, e in zip(dsts, exts)]

    def decompress_box(self, out, cnt, dims, dtype, eb, sf, lo, hi, index, mode=EC, qtable=None, dst=None):
        """The box lo[i] <= c[i] < hi[i] of what decompress() rebuilds from the same arguments, seen as an array of shape
        `dims` in C order (1 to 4 dimensions), bit for bit; `index` from ac_index().  Returns dst shaped hi - lo."""
        return self._decompress_box(True, out, cnt, dims, dtype, eb, sf, lo, hi, index, mode, qtable, dst)

    def decompress_boxes(self, out, cnt, dims, dtype, eb, sf, boxes, index, mode=EC, qtable=None, dsts=None):
        """The boxes (lo, hi) of `boxes`, each what decompress_box() gives for it, in ONE call (one work list of the hit tiles
        of all boxes, one decode launch, one synchronisation).  Boxes may overlap or repeat.  Returns the list of tensors
        shaped hi - lo; `dsts` (or None: allocated) are the outputs, one per box."""
        return self._decompress_boxes(True, out, cnt, dims, dtype, eb, sf, boxes, index, mode, qtable, dsts)

    # ---- batches of arrays (include/dctz_hip.h: dctzhip_compress_batch / dctzhip_decompress_batch) ----
    def compress_batch(self, xs, ebs, mode=EC, outs=None, scaled=None, prepared=None):
        """k arrays (1-D contiguous CUDA tensors, float32 | float64 each) through one launch sequence per element type.
        ebs: one bound or one per array.  Returns (outs, infos, prepared); pass `prepared` back in to repeat the very
        same call without rebuilding the argument table."""
        self._bind_stream()
        if prepared is None:
            k = len(xs)
            ebs = [float(ebs)] * k if not hasattr(ebs, "__len__") else [float(e) for e in ebs]
            if outs is None:
                outs = [self.alloc_outputs(x.numel(), x.dtype) for x in xs]
            items = (BatchCItem * max(k, 1))()
            for i, x in enumerate(xs):
                assert x.is_cuda and x.is_contiguous() and x.dim() == 1
                it = items[i]
                it.d_in, it.n, it.dtype, it.error_bound = x.data_ptr(), x.numel(), _dt(x.dtype), ebs[i]
                it.d_bin_index, it.d_dc, it.d_ac_exact = outs[i]["bin_index"].data_ptr(), outs[i]["dc"].data_ptr(), outs[i]["ac_exact"].data_ptr()
                it.d_scaled = scaled[i].data_ptr() if (scaled is not None and scaled[i] is not None) else None
            prepared = (k, items, (CompressInfo * max(k, 1))(), outs, (xs, scaled))       # (keeps the tensors alive)
        k, items, infos, outs, _ = prepared
        self._check(self.lib.dctzhip_compress_batch(self.h, k, items, mode, infos), "dctzhip_compress_batch")
        return outs, [infos[i] for i in range(k)], prepared

    def decompress_batch(self, outs, cnts, ns, dtypes, ebs, sfs, mode=EC, qtables=None, dsts=None, prepared=None, check=True):
        """The decode side of a batch.  Returns (dsts, status, prepared); raises on an under-run unless check=False."""
        t = self.torch
        self._bind_stream()
        if prepared is None:
            k = len(outs)
            ebs = [float(ebs)] * k if not hasattr(ebs, "__len__") else [float(e) for e in ebs]
            if dsts is None:
                dsts = [t.empty(int(ns[i]), dtype=dtypes[i], device=self.device) for i in range(k)]
            items = (BatchDItem * max(k, 1))()
            keep = []
            for i in range(k):
                it = items[i]
                it.d_bin_index, it.d_dc, it.d_ac_exact = outs[i]["bin_index"].data_ptr(), outs[i]["dc"].data_ptr(), outs[i]["ac_exact"].data_ptr()
                it.ac_count, it.n, it.dtype, it.error_bound, it.sf = int(cnts[i]), int(ns[i]), _dt(dtypes[i]), ebs[i], float(sfs[i])
                it.d_out = dsts[i].data_ptr()
                if mode == QT:
                    q = np.ascontiguousarray(qtables[i], dtype=np.float64 if dtypes[i] == t.float64 else np.float32)
                    assert q.size == 64
                    keep.append(q)
                    it.qtable_host = q.ctypes.data
            prepared = (k, items, (C.c_int * max(k, 1))(), dsts, (outs, keep))
        k, items, status, dsts, _ = prepared
        rc = self.lib.dctzhip_decompress_batch(self.h, k, items, mode, status)
        if check:
            self._check(rc, "dctzhip_decompress_batch")
        return dsts, [status[i] for i in range(k)], prepared

    def batch_timings(self):
        """Device time of the last batch call per element-type sequence: {"f32": {...}, "f64": {...}} (profiling on)."""
        tt = (Timings * 2)()
        self._check(self.lib.dctzhip_last_batch_timings(self.h, tt), "last_batch_timings")
        return {name: {"stats_ms": tt[i].stats_ms, "main_ms": tt[i].main_ms, "tail_ms": tt[i].tail_ms, "total_ms": tt[i].total_ms}
                for i, name in ((F32, "f32"), (F64, "f64"))}

    # ---- multi-dimensional blocks (include/dctz_hip.h: 8 x 8 tiles of a 2-D array, 4 x 4 x 4 tiles of a 3-D array) ----
    def nd_blocks(self, shape):
        dims = (C.c_size_t * len(shape))(*shape)
        nblk = self.lib.dctzhip_nd_blocks(len(shape), dims)
        if nblk == 0:
            raise DctzHipError(f"multi-dimensional blocks: bad shape {tuple(shape)}")
        return nblk

    def compress_nd(self, x, eb, mode=EC, out=None, scaled=None):
        """x: contiguous 2-D or 3-D CUDA tensor.  The streams cover nblk * 64 positions (edge tiles are padded)."""
        assert x.is_cuda and x.is_contiguous() and x.dim() in (2, 3)
        self._bind_stream()
        shape = tuple(x.shape)
        if out is None:
            out = self.alloc_outputs(self.nd_blocks(shape) * 64, x.dtype)
        dims = (C.c_size_t * len(shape))(*shape)
        info = CompressInfo()
        rc = self.lib.dctzhip_compress_nd(
            self.h, x.data_ptr(), len(shape), dims, _dt(x.dtype), float(eb), mode, out["bin_index"].data_ptr(),
            out["dc"].data_ptr(), out["ac_exact"].data_ptr(), scaled.data_ptr() if scaled is not None else None,
            C.byref(info))
        self._check(rc, "dctzhip_compress_nd")
        return out, info

    def decompress_nd(self, out, cnt, shape, dtype, eb, sf, mode=EC, qtable=None, dst=None):
        t = self.torch
        self._bind_stream()
        shape = tuple(shape)
        if dst is None:
            dst = t.empty(shape, dtype=dtype, device=self.device)
        q = self._qtable(mode, qtable, dtype)
        dims = (C.c_size_t * len(shape))(*shape)
        rc = self.lib.dctzhip_decompress_nd(
            self.h, out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(), int(cnt),
            _host_ptr(q), len(shape), dims, _dt(dtype), float(eb), float(sf),
            mode, dst.data_ptr())
        self._check(rc, "dctzhip_decompress_nd")
        return dst

    def decompress_box_nd(self, out, cnt, shape, dtype, eb, sf, lo, hi, index, mode=EC, qtable=None, dst=None):
        """The box lo[i] <= c[i] < hi[i] of what decompress_nd() rebuilds from the same arguments, bit for bit; `index` from
        ac_index(out, 64 * nd_blocks(shape)).  Returns dst shaped hi - lo."""
        return self._decompress_box(False, out, cnt, shape, dtype, eb, sf, lo, hi, index, mode, qtable, dst)

    def decompress_boxes_nd(self, out, cnt, shape, dtype, eb, sf, boxes, index, mode=EC, qtable=None, dsts=None):
        """The boxes (lo, hi) of `boxes`, each what decompress_box_nd() gives for it, in ONE call (one work list of the hit
        stream tiles of all boxes, one decode launch, one synchronisation).  Boxes may overlap or repeat.  Returns the list
        of tensors shaped hi - lo; `dsts` (or None: allocated) are the outputs, one per box."""
        return self._decompress_boxes(False, out, cnt, shape, dtype, eb, sf, boxes, index, mode, qtable, dsts)

    def _qtable(self, mode, qtable, dtype):
        """The QT table as a decode call passes it: 64 entries of the data type in host memory (QT mode), else None."""
        if mode != QT:
            return None
        q = np.ascontiguousarray(qtable, dtype=np.float64 if dtype == self.torch.float64 else np.float32)
        assert q.size == 64
        return q

    def _stream_args(self, out, index, mode, qtable, dtype):
        """The streams, the index and the QT table as the coarse, summary and correction-list calls pass them: a stream or an
        index that is missing is a null pointer, for the C side to accept or refuse."""
        ptr = lambda v: v.data_ptr() if v is not None else None
        return (ptr(out.get("bin_index")), ptr(out.get("dc")), ptr(out.get("ac_exact"))), ptr(index), self._qtable(mode, qtable, dtype)

    # ---- coarse decode (include/dctz_hip.h: the whole array at 1 / factor of its resolution) ----
    def decompress_coarse(self, out, cnt, n, dtype, eb, sf, factor, index=None, mode=EC, qtable=None, dst=None):
        """The n-element array of decompress() at 1 / factor of its resolution (factor 2 .. 64): ceil(n / factor) values, K =
        64 / factor per block from its K lowest coefficients.  `index` from ac_index(); with factor 64 and n % 64 == 0 only
        out["dc"] is read (bin_index, ac_exact and index may be missing / None).  Returns dst."""
        t = self.torch
        self._bind_stream()
        if dst is None:
            dst = t.empty(int(self.lib.dctzhip_coarse_len(n, int(factor))), dtype=dtype, device=self.device)
        (b, d, a), ix, q = self._stream_args(out, index, mode, qtable, dtype)
        rc = self.lib.dctzhip_decompress_coarse(
            self.h, b, d, a, int(cnt), ix, _host_ptr(q), n, _dt(dtype), float(eb),
            float(sf), mode, int(factor), dst.data_ptr())
        self._check(rc, "dctzhip_decompress_coarse")
        return dst

    def decompress_coarse_nd(self, out, cnt, shape, dtype, eb, sf, factor, index=None, mode=EC, qtable=None, dst=None):
        """The array of decompress_nd() at 1 / factor of its resolution along every axis (2-D: factor 2, 4, 8; 3-D: 2, 4):
        shape ceil(shape[i] / factor).  `index` from ac_index(out, 64 * nd_blocks(shape)); with factor == tile edge only
        out["dc"] is read.  Returns dst."""
        t = self.torch
        self._bind_stream()
        shape = [int(v) for v in shape]
        f = max(int(factor), 1)
        ext = [(v + f - 1) // f for v in shape]
        if dst is None:
            dst = t.empty(ext, dtype=dtype, device=self.device)
        (b, d, a), ix, q = self._stream_args(out, index, mode, qtable, dtype)
        arr = C.c_size_t * max(len(shape), 1)
        rc = self.lib.dctzhip_decompress_coarse_nd(
            self.h, b, d, a, int(cnt), ix, _host_ptr(q), len(shape), arr(*shape),
            _dt(dtype), float(eb), float(sf), mode, int(factor), dst.data_ptr())
        self._check(rc, "dctzhip_decompress_coarse_nd")
        return dst.view(ext)

    def decompress_coarse_box_nd(self, out, cnt, shape, dtype, eb, sf, factor, lo, hi, index=None, mode=EC, qtable=None, dst=None):
        """The box lo[i] <= c[i] < hi[i], in COARSE coordinates, of what decompress_coarse_nd() gives for the same arguments, bit
        for bit; only the stream tiles that hold cells of the box are read.  With factor == tile edge only out["dc"] is
        read.  Returns dst shaped hi - lo."""
        t = self.torch
        self._bind_stream()
        shape, lo, hi = [int(v) for v in shape], [int(v) for v in lo], [int(v) for v in hi]
        nd = len(shape)
        assert len(lo) == nd and len(hi) == nd
        ext = [max(h - l, 0) for l, h in zip(lo, hi)]
        if dst is None:
            dst = t.empty(ext, dtype=dtype, device=self.device)
        (b, d, a), ix, q = self._stream_args(out, index, mode, qtable, dtype)
        arr = C.c_size_t * max(nd, 1)
        rc = self.lib.dctzhip_decompress_coarse_box_nd(
            self.h, b, d, a, int(cnt), ix, _host_ptr(q), nd, arr(*shape),
            _dt(dtype), float(eb), float(sf), mode, int(factor), arr(*lo), arr(*hi), dst.data_ptr())
        self._check(rc, "dctzhip_decompress_coarse_box_nd")
        return dst.view(ext)

    def decompress_coarse_boxes_nd(self, out, cnt, shape, dtype, eb, sf, factor, boxes, index=None, mode=EC, qtable=None, dsts=None):
        """The boxes (lo, hi) of `boxes`, in COARSE coordinates at ONE factor, each what decompress_coarse_box_nd() gives for
        it, in ONE call (one work list of the hit stream tiles of all boxes, one decode launch, one synchronisation; with
        factor == tile edge one gather from out["dc"] alone).  Boxes may overlap or repeat.  Returns the list of tensors
        shaped hi - lo; `dsts` (or None: allocated) are the outputs, one per box."""
        self._bind_stream()
        shape = [int(v) for v in shape]
        nd = len(shape)
        items, dsts, exts = self._box_items(nd, boxes, dtype, dsts)
        (b, d, a), ix, q = self._stream_args(out, index, mode, qtable, dtype)
        arr = C.c_size_t * max(nd, 1)
        rc = self.lib.dctzhip_decompress_coarse_boxes_nd(
            self.h, b, d, a, int(cnt), ix, _host_ptr(q), nd, arr(*shape),
            _dt(dtype), float(eb), float(sf), mode, int(factor), len(dsts), C.cast(items, C.c_void_p))
        self._check(rc, "dctzhip_decompress_coarse_boxes_nd")
        return [d.view(e) for d, e in zip(dsts, exts)]

    # ---- flat and tiled streams through one body per operation ----
    # What a public method makes of its geometry argument: the geometry arguments of the C call (in the flat call's place of n),
    # the positions the streams cover, and whether a tensor is the array's original.
    @staticmethod
    def _geo_flat(n):
        return (n,), n, lambda v: v.numel() == n

    def _geo_nd(self, shape):
        shape = [int(v) for v in shape]
        dims = (C.c_size_t * len(shape))(*shape)
        return (len(shape), dims), self.nd_blocks(shape) * 64, lambda v: list(v.shape) == shape

    # ---- tile summaries (include/dctz_hip.h: verify and survey without writing the decode) ----
    def _tile_summary(self, name, geo, out, cnt, dtype, eb, sf, index, mode, qtable, ref):
        t = self.torch
        self._bind_stream()
        gargs, n_lin, is_original = geo
        if index is None:
            index, _ = self.ac_index(out, n_lin)
        if ref is not None:
            assert ref.is_cuda and ref.is_contiguous() and ref.dtype == dtype and is_original(ref)
        recs = t.empty((int(self.lib.dctzhip_summary_tiles(n_lin)), 8), dtype=t.float64, device=self.device)
        total = TileSummary()
        (b, d, a), ix, q = self._stream_args(out, index, mode, qtable, dtype)
        rc = getattr(self.lib, name)(
            self.h, b, d, a, int(cnt), ix, _host_ptr(q), *gargs, _dt(dtype), float(eb),
            float(sf), mode, ref.data_ptr() if ref is not None else None, recs.data_ptr(), C.byref(total))
        self._check(rc, name)
        return recs, total

    def tile_summary(self, out, cnt, n, dtype, eb, sf, index=None, mode=EC, qtable=None, ref=None):
        """One record per 4096-element tile of what decompress() rebuilds from the same arguments -- min, max, sum and sum of
        squares -- and, with `ref` (the original, a CUDA tensor of n elements), min and max of the original, max |x - r| and
        sum (x - r)^2; the reconstruction is never written.  index=None builds the exception index.  Returns (records, total):
        records a (tiles, 8) float64 CUDA tensor in TileSummary's field order, total a TileSummary of the records joined."""
        return self._tile_summary("dctzhip_tile_summary", self._geo_flat(n), out, cnt, dtype, eb, sf, index, mode, qtable, ref)

    def tile_summary_nd(self, out, cnt, shape, dtype, eb, sf, index=None, mode=EC, qtable=None, ref=None):
        """tile_summary() for the streams of compress_nd(): one record per stream tile (64 blocks of 8 x 8 / 4 x 4 x 4) of what
        decompress_nd() rebuilds from the same arguments, over the array's own elements -- the edge padding of the streams
        enters no field.  `ref`: the original, a contiguous 2-D or 3-D CUDA tensor of `shape` (it may be a slice of a larger
        buffer; only element alignment is asked).  index=None builds the index over 64 * nd_blocks(shape).  Returns
        (records, total) as tile_summary() does."""
        return self._tile_summary("dctzhip_tile_summary_nd", self._geo_nd(shape), out, cnt, dtype, eb, sf, index, mode, qtable, ref)

    # ---- point-wise error bound (include/dctz_hip.h: a correction list beside the streams) ----
    def _fixup_build(self, name, geo, out, cnt, dtype, eb, sf, ref, bound, index, mode, qtable, capacity):
        t = self.torch
        self._bind_stream()
        gargs, n_lin, is_original = geo
        if index is None:
            index, _ = self.ac_index(out, n_lin)
        assert ref.is_cuda and ref.is_contiguous() and ref.dtype == dtype and is_original(ref)
        start = t.empty(int(self.lib.dctzhip_fixup_tiles(n_lin)) + 1, dtype=t.int32, device=self.device)
        (b, d, a), ix, q = self._stream_args(out, index, mode, qtable, dtype)
        qp = _host_ptr(q)
        count = C.c_uint32(0)

        def call(off, val, cap):
            return getattr(self.lib, name)(
                self.h, b, d, a, int(cnt), ix, qp, *gargs, _dt(dtype), float(eb), float(sf), mode, ref.data_ptr(), float(bound),
                start.data_ptr(), off.data_ptr() if off is not None else None, val.data_ptr() if val is not None else None,
                int(cap), C.byref(count))

        if capacity is None or capacity == 0:
            self._check(call(None, None, 0), name)
            if capacity == 0:
                return start, None, None, int(count.value)
            capacity = int(count.value)
        off = t.empty(max(int(capacity), 1), dtype=t.int16, device=self.device)
        val = t.empty(max(int(capacity), 1), dtype=dtype, device=self.device)
        rc = call(off, val, capacity)
        if rc == E_SPACE:
            err = DctzHipError(f"{name} failed ({rc}): {self.lib.dctzhip_last_error(self.h).decode()}")
            err.count = int(count.value)
            raise err
        self._check(rc, name)
        k = int(count.value)
        return start, off[:k], val[:k], k

    def fixup_build(self, out, cnt, n, dtype, eb, sf, ref, bound, index=None, mode=EC, qtable=None, capacity=None):
        """The correction list of the streams against `ref` (the original, a CUDA tensor of n elements) for the absolute bound
        `bound`: every element i with not |ref[i] - r[i]| <= bound, r what decompress() rebuilds from the same arguments.
        Returns (fix_start, fix_off, fix_val, count): fix_start an int32 tensor of tiles + 1 entries, fix_off int16 offsets in
        the tile (their bits are uint16), fix_val the originals of the listed elements.  capacity=None counts first and sizes
        the list from the count; capacity=0 is the count-only call (fix_off and fix_val are None); a list that does not fit
        the capacity raises DctzHipError, its .count says how many entries there are."""
        return self._fixup_build("dctzhip_fixup_build", self._geo_flat(n), out, cnt, dtype, eb, sf, ref, bound, index, mode, qtable,
                                 capacity)

    def fixup_build_nd(self, out, cnt, shape, dtype, eb, sf, ref, bound, index=None, mode=EC, qtable=None, capacity=None):
        """fixup_build() for the streams of compress_nd(): the correction list against `ref` (the original, a contiguous 2-D or
        3-D CUDA tensor of `shape`) over the 64 * nd_blocks(shape) stream positions; r is what decompress_nd() rebuilds from
        the same arguments, the edge padding is never listed.  Return value and capacity conventions are fixup_build's."""
        return self._fixup_build("dctzhip_fixup_build_nd", self._geo_nd(shape), out, cnt, dtype, eb, sf, ref, bound, index, mode,
                                 qtable, capacity)

    def _fixup_apply(self, name, fix, dtype, dst, lo, hi, before_dtype, after_dtype):
        """before_dtype / after_dtype: the C call's geometry arguments on either side of its dtype."""
        self._bind_stream()
        start, off, val, count = fix
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        nd = len(lo)
        assert len(hi) == nd and dst.is_cuda and dst.is_contiguous() and dst.dtype == dtype
        assert dst.numel() == int(np.prod([max(h - l, 0) for l, h in zip(lo, hi)], dtype=np.int64))
        arr = C.c_size_t * max(nd, 1)
        rc = getattr(self.lib, name)(
            self.h, start.data_ptr(), off.data_ptr() if off is not None and count else None,
            val.data_ptr() if val is not None and count else None, int(count), *before_dtype, _dt(dtype), *after_dtype,
            arr(*lo), arr(*hi), dst.data_ptr())
        self._check(rc, name)
        return dst

    def fixup_apply(self, fix, n, dtype, dst, dims=None, lo=None, hi=None):
        """Applies the list `fix` (fixup_build's result) to dst: the dense box lo <= c < hi of the n-element array seen with
        shape `dims` -- what decompress_box() wrote; dims=None: the range [lo, hi) of the flat array (what decompress_range()
        wrote), by default all of it.  Returns dst."""
        if dims is None:
            dims, lo, hi = [n], [0 if lo is None else lo], [n if hi is None else hi]
        dims = [int(v) for v in dims]
        assert len(lo) == len(dims)
        return self._fixup_apply("dctzhip_fixup_apply", fix, dtype, dst, lo, hi, (n,),
                                 (len(dims), (C.c_size_t * max(len(dims), 1))(*dims)))

    def fixup_apply_nd(self, fix, shape, dtype, dst, lo=None, hi=None):
        """Applies the list `fix` (fixup_build_nd's result) to dst: the dense box lo <= c < hi of the array of `shape` -- what
        decompress_box_nd() wrote, by default the whole array (what decompress_nd() wrote).  Returns dst."""
        shape = [int(v) for v in shape]
        lo, hi = [0] * len(shape) if lo is None else lo, list(shape) if hi is None else hi
        assert len(lo) == len(shape)
        return self._fixup_apply("dctzhip_fixup_apply_nd", fix, dtype, dst, lo, hi,
                                 (len(shape), (C.c_size_t * max(len(shape), 1))(*shape)), ())

    # ---- missing values (include/dctz_hip.h: a mask beside the streams, the holes filled on compress) ----
    @staticmethod
    def _missing(flags, value=0.0, limit=0.0):
        return flags if isinstance(flags, Missing) else Missing(int(flags), float(value), float(limit))

    def mask_build(self, x, flags, value=0.0, limit=0.0, filled=None, mask=None):
        """The mask of x (a 1-D CUDA tensor) under the tests `flags` (MISS_*), the count of missing elements, and the filled
        copy: filled=None makes a new tensor, filled=x fills in place, filled=False asks for the mask and the count only.
        Returns (mask, count, filled): mask an int64 tensor of ceil(n / 64) words (their bits are uint64)."""
        t = self.torch
        assert x.is_cuda and x.is_contiguous() and x.dim() == 1
        self._bind_stream()
        n = x.numel()
        if mask is None:
            mask = t.empty(int(self.lib.dctzhip_mask_words(n)), dtype=t.int64, device=self.device)
        if filled is None:
            filled = t.empty_like(x)
        elif filled is False:
            filled = None
        m = self._missing(flags, value, limit)
        count = C.c_uint64(0)
        rc = self.lib.dctzhip_mask_build(self.h, x.data_ptr(), n, _dt(x.dtype), C.byref(m), mask.data_ptr(),
                                         filled.data_ptr() if filled is not None else None, C.byref(count))
        self._check(rc, "dctzhip_mask_build")
        return mask, int(count.value), filled

    def mask_apply(self, mask, n, fill, dst, dims=None, lo=None, hi=None):
        """Writes `fill` into every element of dst whose bit is set in `mask` (mask_build's); dst and its geometry are
        fixup_apply's: the dense box lo <= c < hi of the n-element array seen with shape `dims`, or with dims=None the range
        [lo, hi) of the flat array, by default all of it.  Returns dst."""
        self._bind_stream()
        if dims is None:
            dims, lo, hi = [n], [0 if lo is None else lo], [n if hi is None else hi]
        dims, lo, hi = [int(v) for v in dims], [int(v) for v in lo], [int(v) for v in hi]
        nd = len(dims)
        assert len(lo) == nd and len(hi) == nd and dst.is_cuda and dst.is_contiguous()
        assert dst.numel() == int(np.prod([max(h - l, 0) for l, h in zip(lo, hi)], dtype=np.int64))
        arr = C.c_size_t * max(nd, 1)
        rc = self.lib.dctzhip_mask_apply(self.h, mask.data_ptr(), n, _dt(dst.dtype), float(fill), nd, arr(*dims), arr(*lo), arr(*hi),
                                         dst.data_ptr())
        self._check(rc, "dctzhip_mask_apply")
        return dst

    def compress_masked(self, x, eb, flags, value=0.0, limit=0.0, mode=EC, out=None, filled=None, mask=None):
        """mask_build followed by compress of the filled array, in one call; x is not modified.  filled: a tensor like x that
        receives the filled array (the reference for tile_summary and fixup_build), or None: the context keeps it.
        Returns (out, info, mask, count)."""
        t = self.torch
        assert x.is_cuda and x.is_contiguous() and x.dim() == 1
        self._bind_stream()
        n = x.numel()
        if out is None:
            out = self.alloc_outputs(n, x.dtype)
        if mask is None:
            mask = t.empty(int(self.lib.dctzhip_mask_words(n)), dtype=t.int64, device=self.device)
        m = self._missing(flags, value, limit)
        info, count = CompressInfo(), C.c_uint64(0)
        rc = self.lib.dctzhip_compress_masked(
            self.h, x.data_ptr(), n, _dt(x.dtype), float(eb), mode, C.byref(m), out["bin_index"].data_ptr(), out["dc"].data_ptr(),
            out["ac_exact"].data_ptr(), mask.data_ptr(), filled.data_ptr() if filled is not None else None, C.byref(info),
            C.byref(count))
        self._check(rc, "dctzhip_compress_masked")
        return out, info, mask, int(count.value)

    def mask_build_nd(self, x, flags, value=0.0, limit=0.0, filled=None, mask=None):
        """mask_build for a contiguous 2-D or 3-D CUDA tensor that compress_nd() will take: the same mask, over x in C element
        order, and the holes filled inside each 8 x 8 / 4 x 4 x 4 tile.  Returns (mask, count, filled), filled shaped like x."""
        t = self.torch
        assert x.is_cuda and x.is_contiguous() and x.dim() in (2, 3)
        self._bind_stream()
        shape = tuple(x.shape)
        if mask is None:
            mask = t.empty(int(self.lib.dctzhip_mask_words(x.numel())), dtype=t.int64, device=self.device)
        if filled is None:
            filled = t.empty_like(x)
        elif filled is False:
            filled = None
        m = self._missing(flags, value, limit)
        count = C.c_uint64(0)
        rc = self.lib.dctzhip_mask_build_nd(self.h, x.data_ptr(), len(shape), (C.c_size_t * len(shape))(*shape), _dt(x.dtype),
                                            C.byref(m), mask.data_ptr(), filled.data_ptr() if filled is not None else None,
                                            C.byref(count))
        self._check(rc, "dctzhip_mask_build_nd")
        return mask, int(count.value), filled

    def compress_masked_nd(self, x, eb, flags, value=0.0, limit=0.0, mode=EC, out=None, filled=None, mask=None):
        """mask_build_nd followed by compress_nd of the filled array, in one call; x is not modified.  filled: a tensor like x
        that receives the filled array (the reference for fixup_build_nd), or None: the context keeps it.
        Returns (out, info, mask, count)."""
        t = self.torch
        assert x.is_cuda and x.is_contiguous() and x.dim() in (2, 3)
        self._bind_stream()
        shape = tuple(x.shape)
        if out is None:
            out = self.alloc_outputs(self.nd_blocks(shape) * 64, x.dtype)
        if mask is None:
            mask = t.empty(int(self.lib.dctzhip_mask_words(x.numel())), dtype=t.int64, device=self.device)
        m = self._missing(flags, value, limit)
        info, count = CompressInfo(), C.c_uint64(0)
        rc = self.lib.dctzhip_compress_masked_nd(
            self.h, x.data_ptr(), len(shape), (C.c_size_t * len(shape))(*shape), _dt(x.dtype), float(eb), mode, C.byref(m),
            out["bin_index"].data_ptr(), out["dc"].data_ptr(), out["ac_exact"].data_ptr(), mask.data_ptr(),
            filled.data_ptr() if filled is not None else None, C.byref(info), C.byref(count))
        self._check(rc, "dctzhip_compress_masked_nd")
        return out, info, mask, int(count.value)

    def psnr_terms(self, x, r):
        """calc_psnr's reductions (util.c:54-104) on the GPU: (min x, max x, max |x - r|, sum (x - r)^2)."""
        assert x.is_cuda and r.is_cuda and x.dtype == r.dtype and x.numel() == r.numel()
        self._bind_stream()
        out = (C.c_double * 4)()
        rc = self.lib.dctzhip_psnr_terms(self.h, x.data_ptr(), r.data_ptr(), x.numel(), _dt(x.dtype), out)
        self._check(rc, "dctzhip_psnr_terms")
        return tuple(out)

    def rd_probe(self, x, ebs):
        """Rate-distortion probe (dctzhip_rd_probe): one read of x, up to RD_MAXK error bounds.  Returns (points, (min x, max x)),
        points[i] a dict {error_bound, cnt, sse, psnr, raw_bytes} for ebs[i]: exact count, predicted SSE / PSNR."""
        assert x.is_cuda and x.is_contiguous() and x.dim() == 1
        self._bind_stream()
        k = len(ebs)
        e = (C.c_double * max(k, 1))(*[float(v) for v in ebs])
        pts = (RdPoint * max(k, 1))()
        rng = (C.c_double * 2)()
        rc = self.lib.dctzhip_rd_probe(self.h, x.data_ptr(), x.numel(), _dt(x.dtype), k, e, pts, rng)
        self._check(rc, "dctzhip_rd_probe")
        return [{f: getattr(pts[i], f) for f, _ in RdPoint._fields_} for i in range(k)], (rng[0], rng[1])

    def compress_psnr(self, x, target, out=None):
        """EC compression at the largest bound of psnr_grid() whose measured PSNR reaches `target` dB
        (dctzhip_compress_psnr).  Returns (out, info, eb, psnr): the streams are those of compress(x, eb)."""
        assert x.is_cuda and x.is_contiguous() and x.dim() == 1
        self._bind_stream()
        n = x.numel()
        if out is None:
            out = self.alloc_outputs(n, x.dtype)
        info, eb, ps = CompressInfo(), C.c_double(0.0), C.c_double(0.0)
        rc = self.lib.dctzhip_compress_psnr(self.h, x.data_ptr(), n, _dt(x.dtype), float(target), out["bin_index"].data_ptr(),
                                            out["dc"].data_ptr(), out["ac_exact"].data_ptr(), C.byref(info), C.byref(eb), C.byref(ps))
        self._check(rc, "dctzhip_compress_psnr")
        return out, info, eb.value, ps.value

    def rd_probe_nd(self, x, ebs):
        """rd_probe() for a contiguous 2-D or 3-D CUDA tensor compressed in 8 x 8 / 4 x 4 x 4 tiles (dctzhip_rd_probe_nd): the
        counts are compress_nd's, the predicted SSE / PSNR cover the array's own elements (no edge padding)."""
        assert x.is_cuda and x.is_contiguous() and x.dim() in (2, 3)
        self._bind_stream()
        k = len(ebs)
        shape = tuple(x.shape)
        e = (C.c_double * max(k, 1))(*[float(v) for v in ebs])
        pts = (RdPoint * max(k, 1))()
        rng = (C.c_double * 2)()
        rc = self.lib.dctzhip_rd_probe_nd(self.h, x.data_ptr(), len(shape), (C.c_size_t * len(shape))(*shape), _dt(x.dtype), k, e, pts, rng)
        self._check(rc, "dctzhip_rd_probe_nd")
        return [{f: getattr(pts[i], f) for f, _ in RdPoint._fields_} for i in range(k)], (rng[0], rng[1])

    def compress_psnr_nd(self, x, target, out=None):
        """compress_psnr() for a contiguous 2-D or 3-D CUDA tensor in tiles (dctzhip_compress_psnr_nd).  Returns
        (out, info, eb, psnr): the streams are those of compress_nd(x, eb)."""
        assert x.is_cuda and x.is_contiguous() and x.dim() in (2, 3)
        self._bind_stream()
        shape = tuple(x.shape)
        if out is None:
            out = self.alloc_outputs(self.nd_blocks(shape) * 64, x.dtype)
        info, eb, ps = CompressInfo(), C.c_double(0.0), C.c_double(0.0)
        rc = self.lib.dctzhip_compress_psnr_nd(self.h, x.data_ptr(), len(shape), (C.c_size_t * len(shape))(*shape), _dt(x.dtype),
                                               float(target), out["bin_index"].data_ptr(), out["dc"].data_ptr(),
                                               out["ac_exact"].data_ptr(), C.byref(info), C.byref(eb), C.byref(ps))
        self._check(rc, "dctzhip_compress_psnr_nd")
        return out, info, eb.value, ps.value

    def deflate(self, sections, want_index=False, literals=None):
        """zlib streams of byte sections, made on the GPU (dctzhip_deflate).  sections: device tensors (any dtype,
        contiguous); returns a list of uint8 device tensors holding one zlib stream each -- with want_index also the
        list of per-chunk compressed sizes (numpy uint32) of every section.  literals: per section, True = no match search
        (DCTZHIP_DEFLATE_LITERALS: bytes of floats)."""
        import torch
        self._bind_stream()
        k = len(sections)
        nbytes = [t.numel() * t.element_size() for t in sections]
        outs = [torch.empty(int(self.lib.dctzhip_deflate_bound(nb)), dtype=torch.uint8, device=sections[0].device if k else "cuda")
                for nb in nbytes]
        src = (C.c_void_p * max(k, 1))(*[t.data_ptr() if nb else None for t, nb in zip(sections, nbytes)])
        dst = (C.c_void_p * max(k, 1))(*[o.data_ptr() for o in outs])
        n = (C.c_size_t * max(k, 1))(*nbytes)
        cap = (C.c_size_t * max(k, 1))(*[o.numel() for o in outs])
        ln = (C.c_size_t * max(k, 1))()
        chunk = int(self.lib.dctzhip_deflate_chunk_bytes())
        idx = [np.zeros(max(1, (nb + chunk - 1) // chunk), np.uint32) for nb in nbytes]
        ix = (C.c_void_p * max(k, 1))(*[a.ctypes.data for a in idx])
        fl = (C.c_uint * max(k, 1))(*[1 if (literals and literals[i]) else 0 for i in range(k)])
        rc = self.lib.dctzhip_deflate_ex(self.h, k, src, n, dst, cap, ln, ix if want_index else None, fl)
        self._check(rc, "dctzhip_deflate")
        zs = [o[:int(l)] for o, l in zip(outs, ln)]
        if want_index:
            return zs, [a[:(nb + chunk - 1) // chunk] for a, nb in zip(idx, nbytes)]
        return zs

    def inflate(self, streams, index, raw_bytes):
        """Sections made by deflate() back to bytes on the GPU (dctzhip_inflate).  streams: uint8 device tensors; index:
        per-chunk compressed sizes (numpy uint32) per section; raw_bytes: inflated sizes.  Returns (list of uint8 device
        tensors, ok)."""
        import torch
        self._bind_stream()
        k = len(streams)
        outs = [torch.empty(max(int(nb), 1), dtype=torch.uint8, device=self.device) for nb in raw_bytes]
        idx = [np.ascontiguousarray(a, dtype=np.uint32) for a in index]
        z = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in streams])
        zl = (C.c_size_t * max(k, 1))(*[t.numel() for t in streams])
        ix = (C.c_void_p * max(k, 1))(*[a.ctypes.data if a.size else None for a in idx])
        raw = (C.c_size_t * max(k, 1))(*[int(nb) for nb in raw_bytes])
        dst = (C.c_void_p * max(k, 1))(*[o.data_ptr() for o in outs])
        ok = C.c_int(0)
        rc = self.lib.dctzhip_inflate(self.h, k, z, zl, ix, raw, dst, C.byref(ok))
        self._check(rc, "dctzhip_inflate")
        return [o[:int(nb)] for o, nb in zip(outs, raw_bytes)], bool(ok.value)

    # ---- multi-GPU gather of the pre-zlib streams over RCCL (include/dctz_hip.h, dctzhip_comm_*) ----
    @staticmethod
    def comm_unique_id():
        """Rank 0 makes the 128-byte id; the caller hands it to the other ranks."""
        lib = load_library()
        buf = C.create_string_buffer(128)
        if lib.dctzhip_comm_unique_id(buf) != 0:
            raise DctzHipError(f"dctzhip_comm_unique_id: {lib.dctzhip_last_error(None).decode()}")
        return buf.raw

    def comm_create(self, rank, world, unique_id):
        assert len(unique_id) == 128
        self._bind_stream()
        self._check(self.lib.dctzhip_comm_create(self.h, int(rank), int(world), C.c_char_p(unique_id)), "dctzhip_comm_create")
        self.comm = (int(rank), int(world))

    def comm_gather(self, out, cnt, n, root=0):
        """Collective.  Returns on `root` a dict of the concatenated streams of all ranks (device tensors) plus
        "sizes" = [(n, nblk, cnt)] per rank; None elsewhere."""
        t = self.torch
        rank, world = self.comm
        self._bind_stream()
        sizes = (C.c_uint64 * (3 * world))()
        self._check(self.lib.dctzhip_comm_sizes(self.h, int(n), int(cnt), sizes), "dctzhip_comm_sizes")
        sz = [(sizes[3 * r], sizes[3 * r + 1], sizes[3 * r + 2]) for r in range(world)]
        res = None
        ptrs = (None, None, None)
        if rank == root:
            # the receive buffers are kept between calls (the same shards every step: 1.3 GB of torch.empty per gather
            # otherwise) and only grow; the views handed back are valid until the next gather of this context
            need = (sum(s[0] for s in sz), sum(s[1] for s in sz), max(1, sum(s[2] for s in sz)))
            keep = getattr(self, "_gather_bufs", None)
            if keep is None or any(k.numel() < n_ for k, n_ in zip(keep, need)):
                keep = (t.empty(need[0], dtype=t.uint8, device=self.device), t.empty(need[1], dtype=t.float32, device=self.device),
                        t.empty(need[2], dtype=t.float32, device=self.device))
                self._gather_bufs = keep
            res = {"bin_index": keep[0][:need[0]], "dc": keep[1][:need[1]], "ac_exact": keep[2][:need[2]], "sizes": sz}
            ptrs = (keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr())
        self._check(self.lib.dctzhip_comm_gather(self.h, int(root), out["bin_index"].data_ptr(), out["dc"].data_ptr(),
                                                 out["ac_exact"].data_ptr(), sizes, *ptrs), "dctzhip_comm_gather")
        return res

    def debug_divide(self, x, divisor):
        self._bind_stream()
        fast, ref = self.torch.empty_like(x), self.torch.empty_like(x)
        rc = self.lib.dctzhip_debug_divide(self.h, x.data_ptr(), x.numel(), _dt(x.dtype), float(divisor),
                                           fast.data_ptr(), ref.data_ptr())
        self._check(rc, "dctzhip_debug_divide")
        return fast, ref

    def dct_blocks(self, x, inverse=False):
        self._bind_stream()
        y = self.torch.empty_like(x)
        rc = self.lib.dctzhip_dct_blocks(self.h, x.data_ptr(), y.data_ptr(), x.numel(), _dt(x.dtype), int(inverse))
        self._check(rc, "dctzhip_dct_blocks")
        return y
