"""ctypes binding of libwaverange_amd.so (include/waverange_amd.h).

Host-side mirror of the reference's codec interface (src/core/wrappers.h): the module-level
``setup_wr`` / ``encoding_wrap`` / ``decoding_wrap`` take numpy arrays and return the same
quantities the reference writes through its reference parameters.  ``Context`` exposes the
device-resident entry points used by the parity tests and bench.py.

There is no CPU fallback: loading fails loudly when the HIP library has not been built, and
every compute call fails loudly when no GPU is usable.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# WAVERANGE_AMD_LIB points at another build of the library (A/B runs of experimental builds)
LIB_PATH = os.environ.get("WAVERANGE_AMD_LIB") or os.path.join(HERE, "libwaverange_amd.so")
NLAYMAX = 8

_vp = C.c_void_p
_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_ubyte)
_ulp = C.POINTER(C.c_ulong)


class EncInfo(C.Structure):
    """wr_enc_info: the per-field header record (reference .wrh fields)."""
    _fields_ = [("tolabs", C.c_double), ("midval", C.c_double), ("halfspanval", C.c_double),
                ("wlev", C.c_ubyte), ("nlay", C.c_ubyte), ("ntot_enc", C.c_ulong),
                ("deps_vec", C.c_double * NLAYMAX), ("minval_vec", C.c_double * NLAYMAX),
                ("len_enc_vec", C.c_ulong * NLAYMAX)]

    def as_dict(self):
        L = self.nlay
        return dict(tolabs=self.tolabs, midval=self.midval, halfspanval=self.halfspanval,
                    wlev=self.wlev, nlay=L, ntot_enc=self.ntot_enc,
                    deps_vec=np.array(self.deps_vec[:L]), minval_vec=np.array(self.minval_vec[:L]),
                    len_enc_vec=[int(v) for v in self.len_enc_vec[:L]])

    @classmethod
    def from_dict(cls, d):
        s = cls()
        s.tolabs, s.midval, s.halfspanval = d.get("tolabs", 0.0), d["midval"], d.get("halfspanval", 0.0)
        s.wlev, s.nlay, s.ntot_enc = d["wlev"], d["nlay"], d["ntot_enc"]
        for i in range(d["nlay"]):
            s.deps_vec[i] = d["deps_vec"][i]
            s.minval_vec[i] = d["minval_vec"][i]
            s.len_enc_vec[i] = d["len_enc_vec"][i]
        return s


class Timings(C.Structure):
    _fields_ = [("total", C.c_double), ("gpu", C.c_double), ("transfer", C.c_double),
                ("rangecoder", C.c_double), ("transform_ms", C.c_float), ("quant_ms", C.c_float),
                ("minmax_ms", C.c_float), ("wait", C.c_double), ("h2d_ms", C.c_float), ("d2h_ms", C.c_float),
                ("plane_coder_s", C.c_double * NLAYMAX)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k == "plane_coder_s" else getattr(self, k)) for k, _ in self._fields_}


class BudgetResult(C.Structure):
    """wr_budget_result"""
    _fields_ = [("g", C.c_int), ("tolrel", C.c_double), ("bound", C.c_size_t), ("probe_passes", C.c_int)]


class BoundedResult(C.Structure):
    """wr_bounded_result"""
    _fields_ = [("g", C.c_int), ("tolrel", C.c_double), ("err", C.c_double), ("trials", C.c_int)]


class QualityResult(C.Structure):
    """wr_quality_result"""
    _fields_ = [("g", C.c_int), ("tolrel", C.c_double), ("max_abs", C.c_double), ("rms", C.c_double), ("sumsq", C.c_double),
                ("range", C.c_double), ("psnr", C.c_double), ("max_rms", C.c_double), ("trials", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ErrorStats(C.Structure):
    """wr_error_stats"""
    _fields_ = [("max_abs", C.c_double), ("sumsq", C.c_double), ("rms", C.c_double), ("lo", C.c_double), ("hi", C.c_double),
                ("psnr", C.c_double), ("nonfinite", C.c_ulonglong)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MaskResult(C.Structure):
    """wr_mask_result"""
    _fields_ = [("undefined", C.c_ulonglong), ("pad", C.c_double), ("mask_len", C.c_size_t), ("split_ms", C.c_float), ("fill_ms", C.c_float),
                ("mask_coder_ms", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FusedLevel(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("tiles_x", "tiles_y", "zps", "zsegs", "zlast")]


class FusedPlan(C.Structure):
    """wr_fused_plan_t"""
    _fields_ = [("levels", C.c_int), ("used", C.c_int), ("level", FusedLevel * 4)]


class Box(C.Structure):
    """wr_box: the half-open box [x0, x1) x [y0, y1) x [z0, z1)"""
    _fields_ = [(k, C.c_int) for k in ("x0", "y0", "z0", "x1", "y1", "z1")]


class RoiPlanBox(C.Structure):
    _fields_ = [("src", C.c_int * 3), ("dst", C.c_int * 3), ("len", C.c_int * 3), ("wide", C.c_int)]


class RoiPlan(C.Structure):
    """wr_roi_plan_t"""
    _fields_ = [("win", Box), ("inverse", C.c_int), ("fused", C.c_int), ("fused_levels", C.c_int), ("nbox", C.c_int),
                ("box", RoiPlanBox * 29)]


class ReorderPlanBox(C.Structure):
    _fields_ = [("origin", C.c_int * 3), ("extent", C.c_int * 3), ("bricks", C.c_int * 3), ("first", C.c_uint32), ("first_brick", C.c_uint32),
                ("start", C.c_uint64), ("wide", C.c_int)]


class ReorderPlan(C.Structure):
    """wr_reorder_plan_t"""
    _fields_ = [("group", C.c_int), ("items", C.c_uint32), ("nbricks", C.c_uint32), ("nbox", C.c_int), ("box", ReorderPlanBox * 29)]


class WaveRangeError(RuntimeError):
    pass


_lib = None


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WaveRangeError(
            "%s is missing: build it with `python -m waverange_amd.build` (hipcc, gfx950); "
            "there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.wr_last_error.restype = C.c_char_p
    L.wr_ctx_create.argtypes = [C.POINTER(_vp), C.c_int, _vp]
    L.wr_ctx_destroy.argtypes = [_vp]
    L.wr_ctx_sync.argtypes = [_vp]
    L.wr_ctx_set_keep_residual.argtypes = [_vp, C.c_int]
    L.wr_dev_alloc.argtypes = [_vp, C.POINTER(_vp), C.c_size_t]
    L.wr_dev_free.argtypes = [_vp, _vp]
    L.wr_dev_upload.argtypes = [_vp, _vp, _vp, C.c_size_t]
    L.wr_dev_download.argtypes = [_vp, _vp, _vp, C.c_size_t]
    L.wr_dev_copy.argtypes = [_vp, _vp, _vp, C.c_size_t]
    L.wr_dev_copy_kernel.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int]
    L.wr_dev_linf.argtypes = [_vp, _vp, _vp, C.c_size_t, _dp, _dp]
    L.wr_dev_transform.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.wr_dev_minmax.argtypes = [_vp, _vp, C.c_size_t, _dp, _dp]
    L.wr_dev_quantize_plane.argtypes = [_vp, _vp, C.c_size_t, C.c_double, C.c_double, _vp, _dp, _dp]
    L.wr_dev_dequant_accum.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.POINTER(_vp), _dp, _dp]
    L.wr_dev_synth_field.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_ulonglong]
    L.wr_plane_pitch.restype = C.c_size_t
    L.wr_plane_pitch.argtypes = [C.c_size_t]
    L.wr_dev_encode_planes.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _vp,
                                       C.POINTER(EncInfo)]
    L.wr_dev_decode_planes.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(EncInfo)]
    L.wr_encode_device.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                   C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings)]
    L.wr_encode_device_local.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp,
                                         C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings)]
    L.wr_decode_device.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(EncInfo), _vp, C.c_size_t,
                                   C.POINTER(Timings)]
    L.wr_encode_host.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp,
                                 C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings)]
    L.wr_decode_host.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(EncInfo), _vp, C.c_size_t,
                                 C.POINTER(Timings)]
    L.wr_transform_host.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.wr_encode_host_f32.argtypes = L.wr_encode_host.argtypes
    L.wr_decode_host_f32.argtypes = L.wr_decode_host.argtypes
    L.wr_decode_finish_host_f32.argtypes = [_vp, _vp, C.POINTER(Timings)]
    L.wr_decode_begin.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings)]
    L.wr_decode_finish_host.argtypes = [_vp, _vp, C.POINTER(Timings)]
    L.wr_decode_finish_device.argtypes = [_vp, _vp, C.POINTER(Timings)]
    L.wr_host_alloc.argtypes = [C.POINTER(_vp), C.c_size_t]
    L.wr_host_free.argtypes = [_vp]
    L.wr_host_register.argtypes = [_vp, C.c_size_t]
    L.wr_autotune_batch.argtypes = [C.c_size_t, C.c_int]
    L.wr_test_stale_window.argtypes = [_vp, C.c_size_t]
    L.wr_host_unregister.argtypes = [_vp]
    L.wr_set_device_slots.argtypes = [C.c_int, C.c_int]
    L.wr_set_writeback_residual.argtypes = [C.c_int]
    L.wr_set_coder_pool.argtypes = [C.c_int, C.c_int]
    L.wr_stat.restype = C.c_ulong
    L.wr_stat.argtypes = [C.c_int]
    L.wr_pool_loop_stats.restype = None
    L.wr_pool_loop_stats.argtypes = [_vp, _vp]
    L.wr_range_encode_bound.restype = C.c_size_t
    L.wr_range_encode_bound.argtypes = [C.c_size_t]
    L.wr_range_encode.restype = C.c_size_t
    L.wr_range_encode.argtypes = [_vp, C.c_size_t, _vp]
    L.wr_range_decode.restype = C.c_size_t
    L.wr_range_decode.argtypes = [_vp, C.c_size_t, _vp, C.c_size_t]
    L.wr_range_encode_multi.restype = None
    L.wr_range_encode_multi.argtypes = [C.c_int, _vp, C.c_size_t, _vp, _vp]
    L.wr_ctx_trim.restype = C.c_int
    L.wr_ctx_trim.argtypes = [C.c_void_p]
    L.wr_range_decode_multi.restype = None
    L.wr_range_decode_multi.argtypes = [C.c_int, _vp, _vp, _vp, C.c_size_t, _vp]
    L.wr_range_encode_pool.argtypes = [C.c_int, _vp, _vp, _vp, _vp]
    L.wr_range_decode_pool.argtypes = [C.c_int, _vp, _vp, _vp, _vp, _vp]
    L.wr_range_decode_vec.argtypes = [C.c_int, _vp, _vp, _vp, _vp, _vp]
    L.wr_range_encode_vec.argtypes = [C.c_int, _vp, _vp, _vp, _vp]
    L.wr_range_encode_windowed.argtypes = [C.c_int, C.c_int, _vp, C.c_size_t, C.c_size_t, _vp, _vp]
    L.wr_range_decode_windowed.argtypes = [C.c_int, C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp]
    L.wr_seg_bound.restype = C.c_size_t
    L.wr_seg_bound.argtypes = [C.c_size_t, C.c_uint]
    L.wr_seg_encode_host_ref.restype = C.c_size_t
    L.wr_seg_encode_host_ref.argtypes = [_vp, C.c_size_t, C.c_uint, _vp]
    L.wr_seg_decode_host_ref.argtypes = [_vp, C.c_size_t, _vp, C.c_size_t]
    L.wr_dev_seg_encode.argtypes = [_vp, _vp, C.c_size_t, C.c_uint, _vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.wr_dev_seg_decode.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.wr_encode_host_seg.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_uint,
                                     C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings)]
    L.wr_encode_host_seg_f32.argtypes = L.wr_encode_host_seg.argtypes
    # an encode to a byte budget: the grid, the size bound, the stage calls and the drivers
    L.wr_budget_tol.restype = C.c_double
    L.wr_budget_tol.argtypes = [C.c_int]
    L.wr_budget_index.argtypes = [C.c_double]
    L.wr_seg_size_bound_host_ref.restype = C.c_size_t
    L.wr_seg_size_bound_host_ref.argtypes = [_vp, C.c_size_t, C.c_uint]
    L.wr_dev_plane_size_bound.argtypes = [_vp, _vp, C.c_size_t, C.c_uint, C.POINTER(C.c_size_t)]
    L.wr_dev_quant_size_probe.argtypes = [_vp, _vp, C.c_size_t, C.c_double, C.c_int, _dp, C.c_uint, C.POINTER(C.c_size_t)]
    L.wr_encode_host_seg_budget.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_double,
                                            C.c_uint, C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings), C.POINTER(BudgetResult)]
    L.wr_encode_host_seg_budget_f32.argtypes = L.wr_encode_host_seg_budget.argtypes
    L.wr_encode_device_seg_budget.argtypes = L.wr_encode_host_seg_budget.argtypes
    # an encode to an error bound: the start point, the stage call, the drivers and the measuring half
    L.wr_bounded_start.argtypes = [C.c_double, C.c_double]
    L.wr_dev_requant_accum.argtypes = [_vp, _vp, C.c_size_t, C.c_int, _dp, _dp, _vp]
    L.wr_encode_host_seg_bounded.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                             C.c_uint, C.c_uint, C.c_uint, C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings),
                                             C.POINTER(BoundedResult)]
    L.wr_encode_host_seg_bounded_f32.argtypes = L.wr_encode_host_seg_bounded.argtypes
    L.wr_encode_device_seg_bounded.argtypes = L.wr_encode_host_seg_bounded.argtypes
    L.wr_seg_error_host.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(EncInfo), _vp, C.c_size_t, _dp]
    L.wr_seg_error_host_f32.argtypes = L.wr_seg_error_host.argtypes
    L.wr_ctx_bounded_trial_ms.argtypes = [_vp, _dp, _dp, _dp]
    # an encode to an RMS / PSNR target, its measuring half and the compare alone
    L.wr_psnr_rms.argtypes = [C.c_double, C.c_double, C.c_double]
    L.wr_psnr_rms.restype = C.c_double
    L.wr_encode_host_seg_quality.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                             C.c_uint, C.c_uint, C.c_uint, C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings),
                                             C.POINTER(QualityResult)]
    L.wr_encode_host_seg_quality_f32.argtypes = L.wr_encode_host_seg_quality.argtypes
    L.wr_encode_device_seg_quality.argtypes = L.wr_encode_host_seg_quality.argtypes
    L.wr_seg_error_stats_host.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(ErrorStats)]
    L.wr_seg_error_stats_host_f32.argtypes = L.wr_seg_error_stats_host.argtypes
    L.wr_dev_err_stats.argtypes = [_vp, _vp, _vp, C.c_size_t, C.POINTER(ErrorStats)]
    L.wr_dev_err_stats_f32.argtypes = L.wr_dev_err_stats.argtypes
    # masked fields: the blob on the host, the stage calls and the drivers
    L.wr_mask_bound.restype = C.c_size_t
    L.wr_mask_bound.argtypes = [C.c_size_t, C.c_uint]
    L.wr_mask_blob_host_ref.restype = C.c_size_t
    L.wr_mask_blob_host_ref.argtypes = [_vp, C.c_size_t, C.c_uint, C.c_double, _vp]
    L.wr_mask_parse_host_ref.argtypes = [_vp, C.c_size_t, C.c_size_t, _vp, C.POINTER(C.c_ulonglong), _dp]
    L.wr_mask_sniff.argtypes = [_vp, C.c_size_t]
    L.wr_dev_mask_split.argtypes = [_vp, _vp, C.c_size_t, C.c_double, _vp, C.POINTER(C.c_ulonglong), _dp]
    L.wr_dev_mask_split_f32.argtypes = L.wr_dev_mask_split.argtypes
    L.wr_dev_mask_fill.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_double]
    L.wr_dev_mask_fill_f32.argtypes = L.wr_dev_mask_fill.argtypes
    L.wr_dev_mask_restore.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_double, C.POINTER(C.c_ulonglong)]
    L.wr_dev_mask_restore_f32.argtypes = L.wr_dev_mask_restore.argtypes
    L.wr_encode_host_seg_masked.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_uint, C.c_uint, C.c_uint,
                                            C.c_double, C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings), C.POINTER(MaskResult)]
    L.wr_encode_host_seg_masked_f32.argtypes = L.wr_encode_host_seg_masked.argtypes
    L.wr_encode_device_seg_masked.argtypes = L.wr_encode_host_seg_masked.argtypes
    L.wr_decode_host_seg_masked.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(EncInfo), _vp, C.c_size_t, C.c_double,
                                            C.POINTER(Timings), C.POINTER(MaskResult)]
    L.wr_decode_host_seg_masked_f32.argtypes = L.wr_decode_host_seg_masked.argtypes
    L.wr_decode_device_seg_masked.argtypes = L.wr_decode_host_seg_masked.argtypes
    # masked fields in the tolerance searches: the quality and budget calls, the measuring half and the masked compare alone
    L.wr_encode_host_seg_quality_masked.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                                    C.c_double, C.c_uint, C.c_uint, C.c_uint, C.c_double, C.POINTER(EncInfo), _vp, C.c_size_t,
                                                    C.POINTER(Timings), C.POINTER(QualityResult), C.POINTER(MaskResult)]
    L.wr_encode_host_seg_quality_masked_f32.argtypes = L.wr_encode_host_seg_quality_masked.argtypes
    L.wr_encode_device_seg_quality_masked.argtypes = L.wr_encode_host_seg_quality_masked.argtypes
    L.wr_encode_host_seg_budget_masked.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_double,
                                                   C.c_uint, C.c_double, C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings),
                                                   C.POINTER(BudgetResult), C.POINTER(MaskResult)]
    L.wr_encode_host_seg_budget_masked_f32.argtypes = L.wr_encode_host_seg_budget_masked.argtypes
    L.wr_encode_device_seg_budget_masked.argtypes = L.wr_encode_host_seg_budget_masked.argtypes
    L.wr_seg_error_stats_host_masked.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(ErrorStats),
                                                 C.POINTER(C.c_ulonglong)]
    L.wr_seg_error_stats_host_masked_f32.argtypes = L.wr_seg_error_stats_host_masked.argtypes
    L.wr_dev_err_stats_masked.argtypes = [_vp, _vp, _vp, C.c_size_t, _vp, C.POINTER(ErrorStats), C.POINTER(C.c_ulonglong)]
    L.wr_dev_err_stats_masked_f32.argtypes = L.wr_dev_err_stats_masked.argtypes
    # masked region and low-resolution decode (a NULL region: the whole box of the level)
    L.wr_mask_roi_segments.restype = C.c_size_t
    L.wr_mask_roi_segments.argtypes = [C.c_int] * 4 + [C.POINTER(Box), C.c_uint, _vp, C.c_size_t]
    L.wr_dev_mask_restore_box.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Box), _vp, C.c_double, C.POINTER(C.c_ulonglong)]
    L.wr_dev_mask_restore_box_f32.argtypes = L.wr_dev_mask_restore_box.argtypes
    L.wr_decode_host_seg_roi_masked.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Box), C.POINTER(EncInfo), _vp, C.c_size_t,
                                                C.c_double, C.POINTER(Timings), C.POINTER(MaskResult)]
    L.wr_decode_host_seg_roi_masked_f32.argtypes = L.wr_decode_host_seg_roi_masked.argtypes
    L.wr_decode_device_seg_roi_masked.argtypes = L.wr_decode_host_seg_roi_masked.argtypes
    L.wr_encode_device_seg.argtypes = L.wr_encode_host_seg.argtypes
    L.wr_decode_host_seg.argtypes = L.wr_decode_host.argtypes
    L.wr_decode_host_seg_f32.argtypes = L.wr_decode_host.argtypes
    L.wr_decode_device_seg.argtypes = L.wr_decode_host.argtypes
    L.wr_encode_host_seg_blocked.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_uint, C.c_uint,
                                             C.POINTER(EncInfo), _vp, C.c_size_t, C.POINTER(Timings)]
    L.wr_encode_host_seg_blocked_f32.argtypes = L.wr_encode_host_seg_blocked.argtypes
    L.wr_encode_device_seg_blocked.argtypes = L.wr_encode_host_seg_blocked.argtypes
    L.wr_blocked_order.argtypes = [C.c_int] * 4 + [C.c_uint, _vp]
    L.wr_seg_bound_strands.restype = C.c_size_t
    L.wr_seg_bound_strands.argtypes = [C.c_size_t, C.c_uint, C.c_uint]
    L.wr_seg_encode_host_ref_strands.restype = C.c_size_t
    L.wr_seg_encode_host_ref_strands.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_uint, _vp]
    L.wr_dev_seg_encode_strands.argtypes = [_vp, _vp, C.c_size_t, C.c_uint, C.c_uint, _vp, C.c_size_t, C.POINTER(C.c_size_t)]
    a = list(L.wr_encode_host_seg_blocked.argtypes)
    L.wr_encode_host_seg_strands.argtypes = a[:12] + [C.c_uint] + a[12:]
    L.wr_encode_host_seg_strands_f32.argtypes = L.wr_encode_host_seg_strands.argtypes
    L.wr_encode_device_seg_strands.argtypes = L.wr_encode_host_seg_strands.argtypes
    L.wr_seg_batch_device_bytes.restype = C.c_size_t
    L.wr_seg_batch_device_bytes.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_uint, C.c_uint, C.c_int]
    L.wr_seg_batch_locate.argtypes = [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.wr_dev_seg_encode_batch.argtypes = [_vp, C.c_int, _vp, C.c_size_t, C.c_uint, _vp, _vp, _vp]
    L.wr_dev_seg_decode_batch.argtypes = [_vp, C.c_int, _vp, _vp, _vp, C.c_size_t, _vp]
    L.wr_encode_host_seg_batch.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_uint, C.c_uint,
                                           _vp, _vp, _vp, C.POINTER(Timings)]
    L.wr_encode_host_seg_batch_f32.argtypes = L.wr_encode_host_seg_batch.argtypes
    L.wr_encode_device_seg_batch.argtypes = L.wr_encode_host_seg_batch.argtypes
    L.wr_decode_host_seg_batch.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.POINTER(Timings)]
    L.wr_decode_host_seg_batch_f32.argtypes = L.wr_decode_host_seg_batch.argtypes
    L.wr_decode_device_seg_batch.argtypes = L.wr_decode_host_seg_batch.argtypes
    L.wr_seg_batch_device_bytes_strands.restype = C.c_size_t
    L.wr_seg_batch_device_bytes_strands.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_int]
    L.wr_seg_batch_strand_lane.argtypes = [_vp, C.c_uint32, C.c_uint, C.c_ulonglong, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.wr_dev_seg_encode_batch_strands.argtypes = [_vp, C.c_int, _vp, C.c_size_t, C.c_uint, C.c_uint, _vp, _vp, _vp]
    L.wr_dev_seg_decode_batch_mixed.argtypes = L.wr_dev_seg_decode_batch.argtypes
    a = L.wr_encode_host_seg_batch.argtypes
    L.wr_encode_host_seg_batch_strands.argtypes = a[:13] + [C.c_uint] + a[13:]
    L.wr_encode_host_seg_batch_strands_f32.argtypes = L.wr_encode_host_seg_batch_strands.argtypes
    L.wr_encode_device_seg_batch_strands.argtypes = L.wr_encode_host_seg_batch_strands.argtypes
    L.wr_decode_host_seg_batch_mixed.argtypes = L.wr_decode_host_seg_batch.argtypes
    L.wr_decode_host_seg_batch_mixed_f32.argtypes = L.wr_decode_host_seg_batch.argtypes
    L.wr_decode_device_seg_batch_mixed.argtypes = L.wr_decode_host_seg_batch.argtypes
    a = L.wr_encode_host_seg_batch_strands.argtypes
    L.wr_encode_host_seg_batch_masked.argtypes = a[:14] + [C.c_double] + a[14:] + [_vp]
    L.wr_encode_host_seg_batch_masked_f32.argtypes = L.wr_encode_host_seg_batch_masked.argtypes
    L.wr_encode_device_seg_batch_masked.argtypes = L.wr_encode_host_seg_batch_masked.argtypes
    a = L.wr_decode_host_seg_batch.argtypes
    L.wr_decode_host_seg_batch_masked.argtypes = a[:9] + [C.c_double] + a[9:] + [_vp]
    L.wr_decode_host_seg_batch_masked_f32.argtypes = L.wr_decode_host_seg_batch_masked.argtypes
    L.wr_decode_device_seg_batch_masked.argtypes = L.wr_decode_host_seg_batch_masked.argtypes
    L.wr_seg_batch_device_bytes_masked.restype = C.c_size_t
    L.wr_seg_batch_device_bytes_masked.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_int]
    L.wr_dev_mask_split_batch.argtypes = [_vp, C.c_int, _vp, C.c_size_t, C.c_double, _vp, _vp, _vp]
    L.wr_dev_mask_split_batch_f32.argtypes = L.wr_dev_mask_split_batch.argtypes
    L.wr_dev_mask_fill_batch.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, _vp]
    L.wr_dev_mask_fill_batch_f32.argtypes = L.wr_dev_mask_fill_batch.argtypes
    L.wr_dev_mask_check_batch.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, _vp]
    L.wr_seg_bound_blocked.restype = C.c_size_t
    L.wr_seg_bound_blocked.argtypes = [C.c_size_t, C.c_uint]
    L.wr_seg_lowres_segments_blocked.restype = C.c_size_t
    L.wr_seg_lowres_segments_blocked.argtypes = [C.c_int] * 5 + [C.c_uint, C.c_uint, _vp, C.c_size_t]
    L.wr_seg_roi_segments_blocked.restype = C.c_size_t
    L.wr_seg_roi_segments_blocked.argtypes = [C.c_int] * 5 + [C.POINTER(Box), C.c_uint, C.c_uint, _vp, C.c_size_t]
    L.wr_dev_plane_reorder.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int]
    L.wr_dev_plane_reorder_list.argtypes = L.wr_dev_plane_reorder.argtypes + [_vp, C.c_size_t]
    L.wr_reorder_plan.argtypes = [C.c_int] * 4 + [C.c_uint, C.c_int, C.POINTER(ReorderPlan)]
    L.wr_seg_encode_host_ref_blocked.restype = C.c_size_t
    L.wr_seg_encode_host_ref_blocked.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, _vp]
    L.wr_seg_decode_host_ref_blocked.argtypes = [_vp, C.c_size_t, _vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.wr_lowres_dims.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)] * 3
    L.wr_lowres_scale.restype = C.c_double
    L.wr_lowres_scale.argtypes = [C.c_int] * 4
    L.wr_seg_lowres_segments.restype = C.c_size_t
    L.wr_seg_lowres_segments.argtypes = [C.c_int] * 4 + [C.c_uint, _vp, C.c_size_t]
    L.wr_dev_decode_planes_lowres.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(EncInfo)]
    L.wr_decode_host_seg_lowres.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncInfo), _vp, C.c_size_t,
                                            C.POINTER(Timings)]
    L.wr_decode_host_seg_lowres_f32.argtypes = L.wr_decode_host_seg_lowres.argtypes
    L.wr_decode_device_seg_lowres.argtypes = L.wr_decode_host_seg_lowres.argtypes
    L.wr_roi_window.argtypes = [C.c_int] * 5 + [C.POINTER(Box), C.POINTER(Box)]
    L.wr_roi_plan.argtypes = [C.c_int] * 5 + [C.POINTER(Box), C.POINTER(RoiPlan)]
    L.wr_seg_roi_segments.restype = C.c_size_t
    L.wr_seg_roi_segments.argtypes = [C.c_int] * 5 + [C.POINTER(Box), C.c_uint, _vp, C.c_size_t]
    L.wr_dev_decode_planes_roi.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Box), _vp, C.POINTER(EncInfo)]
    L.wr_decode_host_seg_roi.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Box), C.POINTER(EncInfo), _vp, C.c_size_t,
                                         C.POINTER(Timings)]
    L.wr_decode_host_seg_roi_f32.argtypes = L.wr_decode_host_seg_roi.argtypes
    L.wr_decode_device_seg_roi.argtypes = L.wr_decode_host_seg_roi.argtypes
    L.wr_roi_multi_elems.restype = C.c_size_t
    L.wr_roi_multi_elems.argtypes = [C.c_int] * 4 + [_vp, C.c_int, _vp]
    L.wr_seg_roi_segments_multi.restype = C.c_size_t
    L.wr_seg_roi_segments_multi.argtypes = [C.c_int] * 5 + [_vp, C.c_int, C.c_uint, C.c_uint, _vp, C.c_size_t]
    L.wr_dev_decode_planes_roi_multi.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.POINTER(EncInfo)]
    L.wr_dev_seg_decode_lists.argtypes = [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    L.wr_decode_host_seg_roi_multi.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.POINTER(EncInfo), _vp, C.c_size_t,
                                               C.POINTER(Timings)]
    L.wr_decode_host_seg_roi_multi_f32.argtypes = L.wr_decode_host_seg_roi_multi.argtypes
    L.wr_decode_device_seg_roi_multi.argtypes = L.wr_decode_host_seg_roi_multi.argtypes
    L.wr_seg_roi_batch_device_bytes.restype = C.c_size_t
    L.wr_seg_roi_batch_device_bytes.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_size_t]
    L.wr_ctx_device_free_bytes.restype = C.c_size_t
    L.wr_ctx_device_free_bytes.argtypes = [_vp]
    L.wr_seg_lists_lanes.restype = C.c_size_t
    L.wr_seg_lists_lanes.argtypes = [C.c_int, _vp, _vp, _vp]
    L.wr_dev_seg_decode_lists_mixed.argtypes = L.wr_dev_seg_decode_lists.argtypes
    L.wr_decode_host_seg_roi_batch.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp,
                                               C.POINTER(Timings)]
    L.wr_decode_host_seg_roi_batch_f32.argtypes = L.wr_decode_host_seg_roi_batch.argtypes
    L.wr_decode_device_seg_roi_batch.argtypes = L.wr_decode_host_seg_roi_batch.argtypes
    # masked region decode across a batch of fields
    L.wr_decode_host_seg_roi_batch_masked.argtypes = L.wr_decode_host_seg_roi_batch.argtypes[:13] + [C.c_double, C.POINTER(Timings), _vp]
    L.wr_decode_host_seg_roi_batch_masked_f32.argtypes = L.wr_decode_host_seg_roi_batch_masked.argtypes
    L.wr_decode_device_seg_roi_batch_masked.argtypes = L.wr_decode_host_seg_roi_batch_masked.argtypes
    L.wr_seg_roi_batch_device_bytes_masked.restype = C.c_size_t
    L.wr_seg_roi_batch_device_bytes_masked.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_size_t]
    L.wr_mask_roi_segments_multi.restype = C.c_size_t
    L.wr_mask_roi_segments_multi.argtypes = [C.c_int] * 4 + [_vp, C.c_int, C.c_uint, _vp, C.c_size_t]
    L.wr_mask_boxes_turns.restype = C.c_size_t
    L.wr_mask_boxes_turns.argtypes = [C.c_int] * 4 + [_vp, C.c_int, _vp]
    L.wr_dev_mask_restore_boxes.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_double, _vp]
    L.wr_dev_mask_restore_boxes_f32.argtypes = L.wr_dev_mask_restore_boxes.argtypes
    L.wr_fused_plan.argtypes = [C.c_int] * 4 + [C.POINTER(FusedPlan)]
    L.wr_bench_transform.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp]
    # drop-in symbols (reference src/core/wrappers.h:53,70,75)
    L.setup_wr.argtypes = [C.c_int] * 3 + [_u8p, _ulp]
    L.encoding_wrap.argtypes = [C.c_int] * 3 + [_dp] + [C.c_int] * 4 + [_dp] + [_dp] * 3 + [
        _u8p, _u8p, _ulp, _dp, _dp, _ulp, _u8p]
    L.decoding_wrap.argtypes = [C.c_int] * 3 + [_dp] + [_dp] * 3 + [_u8p, _u8p, _ulp, _dp, _dp, _ulp, _u8p]
    L.waveletcdf97_3d.argtypes = [C.c_int] * 4 + [_dp]
    _up = C.POINTER(C.c_uint)
    L.wr_stream_format_parse.argtypes = [C.c_char_p, C.POINTER(C.c_int), _up, _up, _up]
    L.wr_set_stream_format.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_uint]
    L.wr_get_stream_format.argtypes = [C.POINTER(C.c_int), _up, _up, _up]
    L.wr_stream_sniff.argtypes = [_vp, C.c_size_t]
    L.wr_transcode_bound.restype = C.c_size_t
    L.wr_transcode_bound.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_uint]
    _tc = [C.c_int] * 3 + [C.POINTER(EncInfo), _vp, C.c_size_t, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.POINTER(EncInfo), _vp, C.c_size_t]
    L.wr_transcode_host.argtypes = [_vp] + _tc + [C.POINTER(Timings)]
    L.wr_transcode_host_ref.argtypes = _tc
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise WaveRangeError("libwaverange_amd error %d: %s" % (rc, lib().wr_last_error().decode()))


def device_count():
    return lib().wr_device_count()


def set_verbosity(level):
    lib().wr_set_verbosity(int(level))


def set_threads(n, encoder=0):
    """coder threads per call; `encoder` > 0 gives the encoder its own count"""
    lib().wr_set_threads(int(n))
    lib().wr_set_encoder_threads(int(encoder))


def set_coder_pool(nthreads, decoder_streams=0):
    """process-wide coder pool (wr_set_coder_pool): nthreads workers code the planes of all concurrent calls;
    0 stops it"""
    lib().wr_set_coder_pool(int(nthreads), int(decoder_streams))


def set_device_slots(device, nslots):
    _check(lib().wr_set_device_slots(int(device), int(nslots)))


STAT_EARLY_DECODES, STAT_SLOTS_POPULATED, STAT_DEVICE_PLANE_BYTES, STAT_POOL_IDLE_MS, STAT_POOL_STREAMS_MOVED = 0, 1, 2, 3, 4
STAT_POOL_QUEUE_MS, STAT_PLANE_WAIT_MS, STAT_HANDOVER_ERRORS, STAT_CLOCK_WARMUP_MS, STAT_DECODE_GATE_MS = 5, 6, 7, 8, 9
STAT_WINDOW_WAIT_MS = 10
STAT_LOWRES_SEGMENTS, STAT_LOWRES_BYTES_UP = 11, 12
STAT_ROI_SEGMENTS, STAT_ROI_BYTES_UP = 13, 14
STAT_ROI_CODER_LAUNCHES = 15
STAT_BUDGET_CODER_RUNS = 16
STAT_BOUNDED_CODER_RUNS = 17
STAT_QUALITY_CODER_RUNS = 19
STAT_MASK_ROI_SEGMENTS, STAT_MASK_ROI_BYTES_UP = 20, 21


def stat(what):
    return lib().wr_stat(int(what))


def pool_loop_stats():
    """{loop kind: (worker seconds in block steps, stream-blocks advanced)} since the process started."""
    sec, blk = (C.c_double * 4)(), (C.c_double * 4)()
    lib().wr_pool_loop_stats(sec, blk)
    return {k: (sec[i], blk[i]) for i, k in enumerate(("scalar_encoder", "scalar_decoder", "vector_decoder", "vector_encoder"))}


def set_writeback_residual(on):
    lib().wr_set_writeback_residual(int(on))


class _Pinned:
    def __init__(self, nbytes):
        p = _vp()
        _check(lib().wr_host_alloc(C.byref(p), nbytes))
        self.ptr, self.nbytes = p.value, nbytes

    def __del__(self):
        if self.ptr and _lib is not None:
            _lib.wr_host_free(self.ptr)
            self.ptr = None


def pinned_array(shape, dtype=np.float64):
    """numpy array on pinned host memory (wr_host_alloc): moves over PCIe by DMA without a staging copy.
    The memory is released when the last view of the array is gone."""
    dt = np.dtype(dtype)
    count = int(np.prod(shape))
    owner = _Pinned(max(16, count * dt.itemsize))
    buf = (C.c_ubyte * owner.nbytes).from_address(owner.ptr)
    buf._owner = owner  # keeps the allocation alive as long as the ctypes buffer (numpy's base)
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


class registered:
    """`with api.registered(arr):` pins a numpy array the caller owns for the duration of the block (wr_host_register)."""

    def __init__(self, arr):
        self.arr = arr

    def __enter__(self):
        _check(lib().wr_host_register(self.arr.ctypes.data, self.arr.nbytes))
        return self.arr

    def __exit__(self, *exc):
        _check(lib().wr_host_unregister(self.arr.ctypes.data))
        return False


def range_encode_windowed(planes, chunk, mode=0):
    """Equally long planes coded through windows of `chunk` symbols (test hook of the device-resident plane path).
    mode 0: interleaved loops on this thread, 1: the coder pool, 2: the 16-lane loops."""
    ps = [np.ascontiguousarray(p, dtype=np.uint8).ravel() for p in planes]
    k, n = len(ps), ps[0].size
    assert all(p.size == n for p in ps)
    outs = [np.empty(lib().wr_range_encode_bound(n), dtype=np.uint8) for _ in ps]
    lens = (C.c_size_t * k)()
    _check(lib().wr_range_encode_windowed(mode, k, (C.c_void_p * k)(*[p.ctypes.data for p in ps]), n, chunk,
                                          (C.c_void_p * k)(*[o.ctypes.data for o in outs]), lens))
    return [o[:lens[i]].copy() for i, o in enumerate(outs)]


def range_decode_windowed(streams, n, chunk, mode=0):
    ss = [np.ascontiguousarray(s, dtype=np.uint8).ravel() for s in streams]
    k = len(ss)
    outs = [np.zeros(max(n, 1), dtype=np.uint8) for _ in ss]
    got = (C.c_size_t * k)()
    _check(lib().wr_range_decode_windowed(mode, k, (C.c_void_p * k)(*[s.ctypes.data for s in ss]), (C.c_size_t * k)(*[s.size for s in ss]),
                                          (C.c_void_p * k)(*[o.ctypes.data for o in outs]), n, chunk, got))
    return [o[:n] for o in outs], [got[i] for i in range(k)]


# ---------------------------------------------------------------------------------------
# host range coder (product code, runs without a GPU)
# ---------------------------------------------------------------------------------------
def range_encode(plane):
    p = np.ascontiguousarray(plane, dtype=np.uint8).ravel()
    out = np.empty(lib().wr_range_encode_bound(p.size), dtype=np.uint8)
    n = lib().wr_range_encode(p.ctypes.data, p.size, out.ctypes.data)
    return out[:n].copy()


def range_encode_bound_hist(plane):
    """wr_range_encode_bound_hist on the plane's own per-block histograms (counted here with numpy)."""
    p = np.ascontiguousarray(plane, dtype=np.uint8).ravel()
    nb = p.size // 60000 + 1
    hist = np.zeros((nb, 256), dtype=np.uint16)
    for b in range(nb):
        hist[b] = np.bincount(p[b * 60000:(b + 1) * 60000], minlength=256)
    lib().wr_range_encode_bound_hist.restype = C.c_size_t
    lib().wr_range_encode_bound_hist.argtypes = [C.c_void_p, C.c_size_t]
    return int(lib().wr_range_encode_bound_hist(hist.ctypes.data, p.size))


def range_decode(stream, n):
    s = np.ascontiguousarray(stream, dtype=np.uint8).ravel()
    out = np.zeros(max(n, 1), dtype=np.uint8)
    got = lib().wr_range_decode(s.ctypes.data, s.size, out.ctypes.data, n)
    return out[:n], got


SEG_DEFAULT = 59904  # WR_SEG_DEFAULT


# ---- an encode to a byte budget (include/waverange_amd.h): the tolerance grid and the size bound of a plane, on the host
BUDGET_GMAX = 3840
BUDGET_PROBE_MAX = 8
ERR_BUDGET = -6
ERR_BOUND = -7
NORM_MAX, NORM_RMS, NORM_PSNR = 1, 2, 3


def budget_tol(g):
    """t(g) = ldexp(64 + (g & 63), (g >> 6) - 66), g clamped to [0, BUDGET_GMAX] (wr_budget_tol)."""
    return float(lib().wr_budget_tol(int(g)))


def budget_index(tolrel):
    """The smallest g with budget_tol(g) >= tolrel, clamped to the grid (wr_budget_index)."""
    return int(lib().wr_budget_index(float(tolrel)))


def bounded_start(max_abs_err, absmax):
    """The largest g with budget_tol(g) * absmax <= max_abs_err, clamped to the grid; -1 when even budget_tol(0) is too coarse
    or an argument is not a positive finite number (wr_bounded_start)."""
    return int(lib().wr_bounded_start(float(max_abs_err), float(absmax)))


def psnr_rms(db, lo, hi):
    """The RMS error that a PSNR of `db` over the range hi - lo means, (hi - lo) * 10 ** (-db / 20); NaN unless db is finite and
    the range a positive finite number (wr_psnr_rms)."""
    return float(lib().wr_psnr_rms(float(db), float(lo), float(hi)))


def seg_size_bound_host_ref(plane, seg=0):
    """An upper bound on len(seg_encode_host_ref(plane, seg)) from the segments' histograms alone (wr_seg_size_bound_host_ref)."""
    p = np.ascontiguousarray(plane, dtype=np.uint8).ravel()
    src = p if p.size else np.zeros(1, np.uint8)
    b = int(lib().wr_seg_size_bound_host_ref(src.ctypes.data, p.size, seg))
    if not b:
        raise WaveRangeError(_BAD_SEG)
    return b


def seg_bound(n, seg=0):
    """Worst-case bytes of one plane's segmented blob (0 if `seg` is refused)."""
    return int(lib().wr_seg_bound(n, seg))


def seg_encode_host_ref(plane, seg=0):
    """The segmented blob of a plane, coded on the calling thread: the definition of the format (wr_seg_encode_host_ref)."""
    p = np.ascontiguousarray(plane, dtype=np.uint8).ravel()
    bound = seg_bound(p.size, seg)
    if not bound:
        raise WaveRangeError("segment length must be a multiple of 16 in [16, 59999]")
    out = np.empty(bound, dtype=np.uint8)
    src = p if p.size else np.zeros(1, dtype=np.uint8)
    n = lib().wr_seg_encode_host_ref(src.ctypes.data, p.size, seg, out.ctypes.data)
    if not n:
        raise WaveRangeError(lib().wr_last_error().decode())
    return out[:n].copy()


def seg_decode_host_ref(blob, n):
    """The n symbols of a segmented blob, decoded on the calling thread; raises WaveRangeError for a malformed blob."""
    b = np.ascontiguousarray(blob, dtype=np.uint8).ravel()
    src = b if b.size else np.zeros(1, dtype=np.uint8)
    out = np.zeros(max(n, 1), dtype=np.uint8)
    _check(lib().wr_seg_decode_host_ref(src.ctypes.data, b.size, out.ctypes.data, n))
    return out[:n]


MASK_HEADER_BYTES = 32  # 'W','R','M','1' | u32 0 | u64 n | u64 undefined | f64 pad


def mask_bound(n, seg=0):
    """Worst-case bytes of the mask blob of a field of n samples (0 if `seg` is refused) (wr_mask_bound)."""
    return int(lib().wr_mask_bound(n, seg))


def mask_sniff(data):
    """True if `data` starts like a mask blob ("WRM1")."""
    b = np.ascontiguousarray(data, dtype=np.uint8).ravel()
    return bool(b.size and lib().wr_mask_sniff(b.ctypes.data, b.size))


def mask_blob_host_ref(flags, seg=0, pad=0.0):
    """The mask blob of a field whose sample j is undefined iff flags[j] is nonzero, made on the calling thread: the definition
    of the format (wr_mask_blob_host_ref)."""
    f = np.ascontiguousarray(np.asarray(flags) != 0, dtype=np.uint8).ravel()
    bound = mask_bound(f.size, seg)
    if not bound:
        raise WaveRangeError(_BAD_SEG)
    out = np.empty(bound, dtype=np.uint8)
    src = f if f.size else np.zeros(1, dtype=np.uint8)
    n = lib().wr_mask_blob_host_ref(src.ctypes.data, f.size, seg, float(pad), out.ctypes.data)
    if not n:
        raise WaveRangeError(lib().wr_last_error().decode())
    return out[:n].copy()


def mask_parse_host_ref(blob, n):
    """(flags, undefined, pad) of a mask blob for a field of n samples, parsed on the calling thread; raises WaveRangeError
    (WR_ERR_STREAM) for every blob a decoder refuses (wr_mask_parse_host_ref)."""
    b = np.ascontiguousarray(blob, dtype=np.uint8).ravel()
    src = b if b.size else np.zeros(1, dtype=np.uint8)
    flags = np.zeros(max(n, 1), dtype=np.uint8)
    undefined, pad = C.c_ulonglong(0), C.c_double(0)
    _check(lib().wr_mask_parse_host_ref(src.ctypes.data, b.size, n, flags.ctypes.data, C.byref(undefined), C.byref(pad)))
    return flags[:n].astype(bool), int(undefined.value), pad.value


BRICK_DEFAULT = 32  # WR_BRICK_DEFAULT


def seg_bound_blocked(n, seg=0):
    """Worst-case bytes of one plane's blocked ("WRS2") blob (0 if `seg` is refused)."""
    return int(lib().wr_seg_bound_blocked(n, seg))


def blocked_order(shape, wlev=4, brick=0):
    """pi (uint64, nz*ny*nx entries): stream position -> coefficient index x + nx * (y + ny * z) of the blocked order of a field
    shaped (nz, ny, nx) (wr_blocked_order; brick = 0: BRICK_DEFAULT).  blocked = plane.ravel()[pi]."""
    nz, ny, nx = shape
    pi = np.empty(nx * ny * nz, dtype=np.uint64)
    _check(lib().wr_blocked_order(nx, ny, nz, wlev, brick, pi.ctypes.data))
    return pi


def reorder_plan(shape, wlev=4, brick=0, list=False):
    """How the reorder kernel walks a plane of a field shaped (nz, ny, nx) (wr_reorder_plan; host only, needs no GPU):
    dict(group, items, nbricks, boxes), boxes = one dict(origin, extent, bricks, first, first_brick, start, wide) per box in
    stream order, origin / extent / bricks as (x, y, z).  list: the plan of a launch over a brick list."""
    nz, ny, nx = shape
    p = ReorderPlan()
    _check(lib().wr_reorder_plan(nx, ny, nz, wlev, brick, int(bool(list)), C.byref(p)))
    return dict(group=p.group, items=p.items, nbricks=p.nbricks,
                boxes=[dict(origin=tuple(b.origin), extent=tuple(b.extent), bricks=tuple(b.bricks), first=b.first, first_brick=b.first_brick,
                            start=b.start, wide=bool(b.wide)) for b in p.box[:p.nbox]])


def seg_encode_host_ref_blocked(plane, shape, wlev=4, brick=0, seg=0):
    """The WRS2 blob of a plane given in natural order, permuted and coded on the calling thread: the definition of the format."""
    nz, ny, nx = shape
    p = np.ascontiguousarray(plane, dtype=np.uint8).ravel()
    assert p.size == nx * ny * nz
    bound = seg_bound_blocked(p.size, seg)
    if not bound:
        raise WaveRangeError("segment length must be a multiple of 16 in [16, 59999]")
    out = np.empty(bound, dtype=np.uint8)
    n = lib().wr_seg_encode_host_ref_blocked(p.ctypes.data, nx, ny, nz, wlev, brick, seg, out.ctypes.data)
    if not n:
        raise WaveRangeError(lib().wr_last_error().decode())
    return out[:n].copy()


def seg_decode_host_ref_blocked(blob, shape, wlev=4):
    """The plane (natural order, nz*ny*nx symbols) of a WRS2 or WRS1 blob, decoded on the calling thread."""
    nz, ny, nx = shape
    b = np.ascontiguousarray(blob, dtype=np.uint8).ravel()
    src = b if b.size else np.zeros(1, dtype=np.uint8)
    out = np.zeros(nx * ny * nz, dtype=np.uint8)
    _check(lib().wr_seg_decode_host_ref_blocked(src.ctypes.data, b.size, out.ctypes.data, nx, ny, nz, wlev))
    return out


def seg_lowres_segments_blocked(shape, level, seg=0, wlev=4, brick=0):
    """seg_lowres_segments for a plane in the blocked order: the prefix 0 .. ceil(bx*by*bz / seg) - 1."""
    nz, ny, nx = shape
    count = lib().wr_seg_lowres_segments_blocked(nx, ny, nz, level, wlev, brick, seg, None, 0)
    if not count:
        raise WaveRangeError(lib().wr_last_error().decode())
    ids = np.empty(count, dtype=np.uint32)
    got = lib().wr_seg_lowres_segments_blocked(nx, ny, nz, level, wlev, brick, seg, ids.ctypes.data, ids.size)
    assert got == count
    return ids


def seg_roi_segments_blocked(shape, level, roi, seg=0, wlev=4, brick=0):
    """seg_roi_segments for a plane in the blocked order."""
    nz, ny, nx = shape
    r = _box(roi)
    count = lib().wr_seg_roi_segments_blocked(nx, ny, nz, level, wlev, C.byref(r), brick, seg, None, 0)
    if not count:
        raise WaveRangeError(lib().wr_last_error().decode())
    ids = np.empty(count, dtype=np.uint32)
    got = lib().wr_seg_roi_segments_blocked(nx, ny, nz, level, wlev, C.byref(r), brick, seg, ids.ctypes.data, ids.size)
    assert got == count
    return ids


STRANDS_DEFAULT = 8  # WR_STRANDS_DEFAULT
_BAD_SEG = "segment length must be a multiple of 16 in [16, 59999]"
_BAD_SEG_STRANDS = _BAD_SEG + ", strands one of 1, 2, 4, 8, 16, 32 with 16 * strands <= seg"


def seg_bound_strands(n, seg=0, strands=0):
    """Worst-case bytes of one plane's stranded ("WRS3") blob (0 if `seg` or `strands` is refused)."""
    return int(lib().wr_seg_bound_strands(n, seg, strands))


def seg_encode_host_ref_strands(plane, shape=None, wlev=4, brick=0, seg=0, strands=0):
    """The WRS3 blob of a plane given in natural order, coded on the calling thread: the definition of the format.  brick = 0:
    the natural order (shape may be None); otherwise the blocked order of a field shaped (nz, ny, nx) with that brick edge."""
    p = np.ascontiguousarray(plane, dtype=np.uint8).ravel()
    nz, ny, nx = (1, 1, p.size) if shape is None else shape
    assert p.size == nx * ny * nz
    bound = seg_bound_strands(p.size, seg, strands)
    if not bound:
        raise WaveRangeError(_BAD_SEG_STRANDS)
    out = np.empty(bound, dtype=np.uint8)
    src = p if p.size else np.zeros(1, dtype=np.uint8)
    n = lib().wr_seg_encode_host_ref_strands(src.ctypes.data, nx, ny, nz, wlev, brick, seg, strands, out.ctypes.data)
    if not n:
        raise WaveRangeError(lib().wr_last_error().decode())
    return out[:n].copy()


SEG_BATCH_MAX = 1024  # WR_SEG_BATCH_MAX


def seg_batch_device_bytes(nfields, n, nlay, seg=0, brick=0, decode=False):
    """Device memory a batch of `nfields` fields of n samples and nlay planes each takes beside the work-space slot
    (wr_seg_batch_device_bytes; brick = 0: WRS1); 0 for a refused argument."""
    return int(lib().wr_seg_batch_device_bytes(nfields, n, nlay, seg, brick, 1 if decode else 0))


def seg_batch_locate(first, g):
    """(job, segment) of lane g of a batched coder launch; first: the exclusive prefix of the jobs' segment counts,
    njobs + 1 entries (wr_seg_batch_locate)."""
    f = np.ascontiguousarray(first, dtype=np.uint32)
    job, k = C.c_uint32(0), C.c_uint32(0)
    _check(lib().wr_seg_batch_locate(f.ctypes.data, max(f.size, 1) - 1, g, C.byref(job), C.byref(k)))
    return int(job.value), int(k.value)


def seg_batch_device_bytes_strands(nfields, n, nlay, seg=0, brick=0, strands=0, decode=False):
    """seg_batch_device_bytes for the WRS3 batch calls (wr_seg_batch_device_bytes_strands; strands = 0: STRANDS_DEFAULT;
    decode: the mixed decode of such fields); 0 for a refused argument."""
    return int(lib().wr_seg_batch_device_bytes_strands(nfields, n, nlay, seg, brick, strands, 1 if decode else 0))


def seg_batch_device_bytes_masked(nfields, nmasked, n, nlay, seg=0, brick=0, strands=0, decode=False):
    """Device bytes of the masked batch calls: seg_batch_device_bytes_strands (an encode with strands = 0:
    seg_batch_device_bytes) plus, per masked field, the bit plane and the blob, and once the masks' launch
    (wr_seg_batch_device_bytes_masked); an encode passes nmasked = nfields; 0 for a refused argument."""
    return int(lib().wr_seg_batch_device_bytes_masked(nfields, nmasked, n, nlay, seg, brick, strands, 1 if decode else 0))


def seg_batch_strand_lane(first, strands, g):
    """(job, segment, strand) of lane g of a batched strand-encoder launch, or None for a lane past the end; first: the
    exclusive prefix of the jobs' segment counts, njobs + 1 entries (wr_seg_batch_strand_lane).  Refused arguments raise."""
    f = np.ascontiguousarray(first, dtype=np.uint32)
    job, k, j = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    rc = lib().wr_seg_batch_strand_lane(f.ctypes.data, max(f.size, 1) - 1, strands, g, C.byref(job), C.byref(k), C.byref(j))
    if rc < 0:
        _check(rc)
    return (job.value, k.value, j.value) if rc else None


def seg_split_strands(blob):
    """(seg, brick, K, [(T, [S_0, ..., S_{K-1}]), ...]) of a WRS3 blob whose index and length words are well formed (ValueError
    otherwise); the strands past a record's last non-empty one are b""."""
    b = np.ascontiguousarray(blob, dtype=np.uint8).ravel()
    if b.size < 20 or bytes(b[:4]) != b"WRS3":
        raise ValueError("not a WRS3 blob")
    seg, nseg, brick, K = (int(v) for v in b[4:20].view("<u4"))
    if 20 + 4 * nseg > b.size:
        raise ValueError("index longer than the blob")
    lens = b[20:20 + 4 * nseg].view("<u4").astype(np.int64)
    at = 20 + 4 * nseg
    if at + int(lens.sum()) != b.size:
        raise ValueError("segment lengths do not add up to the blob")
    out = []
    for ln in lens:
        ln = int(ln)
        if ln < 4 * (K + 1) or ln % 4:
            raise ValueError("a record shorter than its length words")
        words = [int(v) for v in b[at:at + 4 * (K + 1)].view("<u4")]
        if (4 * (K + 1) + sum(words) + 3) // 4 * 4 != ln:
            raise ValueError("a record's lengths do not add up to the record")
        p = at + 4 * (K + 1)
        pieces = []
        for w in words:
            pieces.append(bytes(b[p:p + w]))
            p += w
        out.append((pieces[0], pieces[1:]))
        at += ln
    return seg, brick, K, out


def seg_split(blob):
    """(seg, [segment stream bytes, ...]) of a segmented blob whose index is well formed (ValueError otherwise)."""
    b = np.ascontiguousarray(blob, dtype=np.uint8).ravel()
    if b.size < 12 or bytes(b[:4]) != b"WRS1":
        raise ValueError("not a WRS1 blob")
    seg, nseg = (int(v) for v in b[4:12].view("<u4"))
    if 12 + 4 * nseg > b.size:
        raise ValueError("index longer than the blob")
    lens = b[12:12 + 4 * nseg].view("<u4").astype(np.int64)
    at = 12 + 4 * nseg
    if at + int(lens.sum()) != b.size:
        raise ValueError("segment lengths do not add up to the blob")
    out = []
    for ln in lens:
        out.append(bytes(b[at:at + int(ln)]))
        at += int(ln)
    return seg, out


def lowres_shape(shape, level):
    """(bz, by, bx): the box that a low-resolution decode of a field shaped (nz, ny, nx) returns at `level` (wr_lowres_dims)."""
    nz, ny, nx = shape
    bx, by, bz = C.c_int(), C.c_int(), C.c_int()
    _check(lib().wr_lowres_dims(nx, ny, nz, level, C.byref(bx), C.byref(by), C.byref(bz)))
    return bz.value, by.value, bx.value


def fused_plan(shape, inverse=False):
    """Which kernels a four-level transform of a field shaped (nz, ny, nx) runs on (wr_fused_plan; host only, needs no GPU):
    dict(levels, used, grid), grid = one (tiles_x, tiles_y, zps, zsegs, zlast) per fused level, finest first."""
    nz, ny, nx = shape
    p = FusedPlan()
    _check(lib().wr_fused_plan(nx, ny, nz, int(bool(inverse)), C.byref(p)))
    return dict(levels=p.levels, used=bool(p.used),
                grid=[tuple(getattr(p.level[l], k) for k, _ in FusedLevel._fields_) for l in range(p.levels)])


def lowres_scale(shape, level):
    """The factor 2^(-e/2) that takes the gain of `level` transform levels out of the box (wr_lowres_scale)."""
    nz, ny, nx = shape
    s = lib().wr_lowres_scale(nx, ny, nz, level)
    if s == 0.0:
        raise WaveRangeError(lib().wr_last_error().decode())
    return s


def seg_lowres_segments(shape, level, seg=0):
    """Ascending ids (uint32) of the segments of a plane cut at `seg` that a decode at `level` needs (seg = 0: SEG_DEFAULT)."""
    nz, ny, nx = shape
    count = lib().wr_seg_lowres_segments(nx, ny, nz, level, seg, None, 0)
    if not count:
        raise WaveRangeError(lib().wr_last_error().decode())
    ids = np.empty(count, dtype=np.uint32)
    got = lib().wr_seg_lowres_segments(nx, ny, nz, level, seg, ids.ctypes.data, ids.size)
    assert got == count
    return ids


def _box(roi):
    """wr_box of a region given as ((z0, z1), (y0, y1), (x0, x1))"""
    (z0, z1), (y0, y1), (x0, x1) = roi
    return Box(int(x0), int(y0), int(z0), int(x1), int(y1), int(z1))


def roi_shape(roi):
    """(cz, cy, cx): the shape of the array a region decode of `roi` returns."""
    return tuple(int(hi) - int(lo) for lo, hi in roi)


def roi_window(shape, level, roi, wlev=4):
    """((a, b) for z, y, x): the window of the box of `level` that a region decode of `roi` inverts (wr_roi_window); shape is
    the coded field's (nz, ny, nx), roi is ((z0, z1), (y0, y1), (x0, x1)) in the coordinates of that box."""
    nz, ny, nx = shape
    r, w = _box(roi), Box()
    _check(lib().wr_roi_window(nx, ny, nz, level, wlev, C.byref(r), C.byref(w)))
    return (w.z0, w.z1), (w.y0, w.y1), (w.x0, w.x1)


def roi_plan(shape, level, roi, wlev=4):
    """Which kernels a region decode of `roi` runs (wr_roi_plan; host only, needs no GPU): dict(box = lowres_shape(shape, level),
    win = ((a, b) for z, y, x), inverse, fused, fused_levels, boxes), boxes = one dict(src, dst, len, wide) per source box of
    the gather in launch order, src / dst / len as (x, y, z).  Arguments as roi_window."""
    nz, ny, nx = shape
    r, p = _box(roi), RoiPlan()
    _check(lib().wr_roi_plan(nx, ny, nz, level, wlev, C.byref(r), C.byref(p)))
    w = p.win
    return dict(box=lowres_shape(shape, level), win=((w.z0, w.z1), (w.y0, w.y1), (w.x0, w.x1)), inverse=p.inverse, fused=bool(p.fused), fused_levels=p.fused_levels,
                boxes=[dict(src=tuple(b.src), dst=tuple(b.dst), len=tuple(b.len), wide=bool(b.wide)) for b in p.box[:p.nbox]])


def seg_roi_segments(shape, level, roi, seg=0, wlev=4):
    """Ascending ids (uint32) of the segments of a plane cut at `seg` that a region decode needs (seg = 0: SEG_DEFAULT)."""
    nz, ny, nx = shape
    r = _box(roi)
    count = lib().wr_seg_roi_segments(nx, ny, nz, level, wlev, C.byref(r), seg, None, 0)
    if not count:
        raise WaveRangeError(lib().wr_last_error().decode())
    ids = np.empty(count, dtype=np.uint32)
    got = lib().wr_seg_roi_segments(nx, ny, nz, level, wlev, C.byref(r), seg, ids.ctypes.data, ids.size)
    assert got == count
    return ids


def mask_roi_segments(shape, level, roi, seg=0):
    """Ascending ids (uint32) of the segments of the MASK plane of a masked record, cut at `seg` symbols of 8 mask bits, that
    hold a bit of the region `roi` of the box of `level` (roi = None: the whole box); host only (wr_mask_roi_segments).  An
    empty array for a refused argument."""
    nz, ny, nx = shape
    r = C.byref(_box(roi)) if roi is not None else None
    count = lib().wr_mask_roi_segments(nx, ny, nz, level, r, seg, None, 0)
    ids = np.empty(count, dtype=np.uint32)
    if count:
        got = lib().wr_mask_roi_segments(nx, ny, nz, level, r, seg, ids.ctypes.data, ids.size)
        assert got == count
    return ids


ROI_MULTI_MAX = 1024  # WR_ROI_MULTI_MAX


def _boxes(rois):
    """a wr_box array of regions given as ((z0, z1), (y0, y1), (x0, x1)) each (at least one entry, so that it has an address)"""
    arr = (Box * max(len(rois), 1))()
    for i, r in enumerate(rois):
        arr[i] = _box(r)
    return arr


def roi_multi_offsets(shape, level, rois):
    """offs (int64, len(rois) + 1): region i of a multi-region decode lies at elements [offs[i], offs[i + 1]) of the output
    (wr_roi_multi_elems); shape is the coded field's (nz, ny, nx)."""
    nz, ny, nx = shape
    offs = (C.c_size_t * (len(rois) + 1))()
    total = lib().wr_roi_multi_elems(nx, ny, nz, level, _boxes(rois), len(rois), offs)
    if not total:
        raise WaveRangeError(lib().wr_last_error().decode())
    return np.array(list(offs), dtype=np.int64)


def seg_roi_segments_multi(shape, level, rois, seg=0, wlev=4, brick=None):
    """Ascending ids (uint32) of the segments of a plane cut at `seg` that any of the regions needs: the union of
    seg_roi_segments (brick is None) or seg_roi_segments_blocked (0: BRICK_DEFAULT) over `rois`."""
    nz, ny, nx = shape
    b = 0 if brick is None else (brick or BRICK_DEFAULT)
    arr = _boxes(rois)
    count = lib().wr_seg_roi_segments_multi(nx, ny, nz, level, wlev, arr, len(rois), b, seg, None, 0)
    if not count:
        raise WaveRangeError(lib().wr_last_error().decode())
    ids = np.empty(count, dtype=np.uint32)
    got = lib().wr_seg_roi_segments_multi(nx, ny, nz, level, wlev, arr, len(rois), b, seg, ids.ctypes.data, ids.size)
    assert got == count
    return ids


def seg_lists_lanes(nlist, strands=None):
    """(lanes, first) of a coder launch over lists (wr_seg_lists_lanes): job j decodes nlist[j] segments with strands[j]
    lanes each (0: a WRS1 / WRS2 job, one lane per segment and no padding; K: a WRS3 job, rounded up to whole waves).
    first (uint32, len(nlist) + 1) is the exclusive prefix of the jobs' lanes, as seg_batch_locate takes it.  A refused
    argument raises; lanes == 0 with first all zeros: every list is empty."""
    nl = (C.c_size_t * max(len(nlist), 1))(*[int(v) for v in nlist])
    st = None if strands is None else (C.c_uint * max(len(strands), 1))(*[int(v) for v in strands])
    assert strands is None or len(strands) == len(nlist)
    first = np.full(len(nlist) + 1, 0xFFFFFFFF, dtype=np.uint32)
    lanes = int(lib().wr_seg_lists_lanes(len(nlist), nl, st, first.ctypes.data))
    if not lanes and (len(nlist) < 1 or first.any()):
        raise WaveRangeError("libwaverange_amd error -1: %s" % lib().wr_last_error().decode())
    return lanes, first


def seg_roi_batch_device_bytes(nfields, n, planes, seg=0, brick=0, strands=0, out_elems=0):
    """An upper bound of the device memory a region decode over `nfields` fields of n samples with `planes` used planes each
    takes beside the work-space slot (wr_seg_roi_batch_device_bytes; brick = 0 and strands = 0: WRS1; out_elems: the
    elements per field a host caller receives); 0 for a refused argument."""
    return int(lib().wr_seg_roi_batch_device_bytes(nfields, n, planes, seg, brick, strands, out_elems))


def roi_batch_groups(nfields, n, planes, budget, seg=0, brick=0, strands=0, out_elems=0):
    """Cuts range(nfields) into consecutive groups for Context.decode_host_seg_rois_batch: every group's
    seg_roi_batch_device_bytes is within `budget` bytes and its jobs (fields times planes) within SEG_BATCH_MAX.  planes:
    the used planes per field, one number or one per field (the largest of a group sizes it).  Returns (groups, alone):
    groups is a list of ranges that cover range(nfields) in order; alone lists the fields that exceed the budget even as a
    group of one -- each of them is a group of its own, for the caller to decode another way or to let fail."""
    pl = [int(planes)] * nfields if np.isscalar(planes) else [int(p) for p in planes]
    assert len(pl) == nfields
    groups, alone = [], []
    a = 0
    while a < nfields:
        b, most = a, 0
        while b < nfields:
            m = max(most, pl[b])
            size = seg_roi_batch_device_bytes(b + 1 - a, n, m, seg, brick, strands, out_elems)
            if not size or size > budget:  # (0: the jobs exceed SEG_BATCH_MAX, or an argument no group size mends)
                break
            b, most = b + 1, m
        if b == a:
            alone.append(a)
            b = a + 1
        groups.append(range(a, b))
        a = b
    return groups, alone


def mask_roi_segments_multi(shape, level, rois, seg=0):
    """Ascending ids (uint32) of the segments of the MASK plane, cut at `seg` symbols, that hold a bit of any of the regions:
    the union of mask_roi_segments over `rois` (wr_mask_roi_segments_multi); host only.  A refused argument raises."""
    nz, ny, nx = shape
    arr = _boxes(rois)
    count = lib().wr_mask_roi_segments_multi(nx, ny, nz, level, arr, len(rois), seg, None, 0)
    if not count:
        raise WaveRangeError(lib().wr_last_error().decode())
    ids = np.empty(count, dtype=np.uint32)
    got = lib().wr_mask_roi_segments_multi(nx, ny, nz, level, arr, len(rois), seg, ids.ctypes.data, ids.size)
    assert got == count
    return ids


def mask_boxes_turns(shape, level, rois):
    """(turns, first) of the restore launch of the masked batch call for ONE field's regions (wr_mask_boxes_turns): a turn is
    64 consecutive x of one region row; first (uint32, len(rois) + 1) is the exclusive prefix of the regions' turns.  A
    refused argument raises."""
    nz, ny, nx = shape
    first = np.zeros(len(rois) + 1, dtype=np.uint32)
    turns = int(lib().wr_mask_boxes_turns(nx, ny, nz, level, _boxes(rois), len(rois), first.ctypes.data))
    if not turns:
        raise WaveRangeError(lib().wr_last_error().decode())
    return turns, first


def seg_roi_batch_device_bytes_masked(nfields, nmasked, n, planes, seg=0, brick=0, strands=0, mask_seg=0, out_elems=0):
    """seg_roi_batch_device_bytes for a call of which `nmasked` fields carry a mask blob cut at mask_seg
    (wr_seg_roi_batch_device_bytes_masked); 0 for a refused argument."""
    return int(lib().wr_seg_roi_batch_device_bytes_masked(nfields, nmasked, n, planes, seg, brick, strands, mask_seg, out_elems))


def roi_batch_groups_masked(nfields, n, planes, budget, masked=True, seg=0, brick=0, strands=0, mask_seg=0, out_elems=0):
    """roi_batch_groups for Context.decode_host_seg_rois_batch_masked: the groups are cut by
    seg_roi_batch_device_bytes_masked.  masked: whether a field carries a mask blob, one flag or one per field."""
    pl = [int(planes)] * nfields if np.isscalar(planes) else [int(p) for p in planes]
    mk = [bool(masked)] * nfields if np.isscalar(masked) else [bool(m) for m in masked]
    assert len(pl) == nfields and len(mk) == nfields
    groups, alone = [], []
    a = 0
    while a < nfields:
        b, most, nm = a, 0, 0
        while b < nfields:
            m, k = max(most, pl[b]), nm + mk[b]
            size = seg_roi_batch_device_bytes_masked(b + 1 - a, k, n, m, seg, brick, strands, mask_seg, out_elems)
            if not size or size > budget:
                break
            b, most, nm = b + 1, m, k
        if b == a:
            alone.append(a)
            b = a + 1
        groups.append(range(a, b))
        a = b
    return groups, alone


def range_encode_multi(planes):
    """Code several equally long planes on this thread with interleaved symbol loops (wr_range_encode_multi)."""
    ps = [np.ascontiguousarray(p, dtype=np.uint8).ravel() for p in planes]
    n, k = ps[0].size, len(ps)
    assert all(p.size == n for p in ps)
    outs = [np.empty(lib().wr_range_encode_bound(n), dtype=np.uint8) for _ in ps]
    lens = (C.c_size_t * k)()
    lib().wr_range_encode_multi(k, (C.c_void_p * k)(*[p.ctypes.data for p in ps]), n,
                                (C.c_void_p * k)(*[o.ctypes.data for o in outs]), lens)
    return [o[:lens[i]].copy() for i, o in enumerate(outs)]


def range_decode_multi(streams, n):
    ss = [np.ascontiguousarray(s, dtype=np.uint8).ravel() for s in streams]
    k = len(ss)
    outs = [np.zeros(max(n, 1), dtype=np.uint8) for _ in ss]
    got = (C.c_size_t * k)()
    lib().wr_range_decode_multi(k, (C.c_void_p * k)(*[s.ctypes.data for s in ss]), (C.c_size_t * k)(*[s.size for s in ss]),
                                (C.c_void_p * k)(*[o.ctypes.data for o in outs]), n, got)
    return [o[:n] for o in outs], [got[i] for i in range(k)]


def range_encode_pool(planes):
    """Planes of any lengths through the coder pool (set_coder_pool first)."""
    ps = [np.ascontiguousarray(p, dtype=np.uint8).ravel() for p in planes]
    k = len(ps)
    outs = [np.empty(lib().wr_range_encode_bound(p.size), dtype=np.uint8) for p in ps]
    lens = (C.c_size_t * k)()
    _check(lib().wr_range_encode_pool(k, (C.c_void_p * k)(*[p.ctypes.data for p in ps]), (C.c_size_t * k)(*[p.size for p in ps]),
                                      (C.c_void_p * k)(*[o.ctypes.data for o in outs]), lens))
    return [o[:lens[i]].copy() for i, o in enumerate(outs)]


def range_decode_pool(streams, ns):
    ss = [np.ascontiguousarray(s, dtype=np.uint8).ravel() for s in streams]
    k = len(ss)
    outs = [np.zeros(max(n, 1), dtype=np.uint8) for n in ns]
    got = (C.c_size_t * k)()
    _check(lib().wr_range_decode_pool(k, (C.c_void_p * k)(*[s.ctypes.data for s in ss]), (C.c_size_t * k)(*[s.size for s in ss]),
                                      (C.c_void_p * k)(*[o.ctypes.data for o in outs]), (C.c_size_t * k)(*ns), got))
    return [o[:n] for o, n in zip(outs, ns)], [got[i] for i in range(k)]


def range_encode_vec(planes):
    """Planes of any kind and length through the 16-lane AVX-512 encoder loop on this thread."""
    ps = [np.ascontiguousarray(p, dtype=np.uint8).ravel() for p in planes]
    k = len(ps)
    outs = [np.empty(lib().wr_range_encode_bound(p.size), dtype=np.uint8) for p in ps]
    lens = (C.c_size_t * k)()
    _check(lib().wr_range_encode_vec(k, (C.c_void_p * k)(*[p.ctypes.data for p in ps]), (C.c_size_t * k)(*[p.size for p in ps]),
                                     (C.c_void_p * k)(*[o.ctypes.data for o in outs]), lens))
    return [o[:lens[i]].copy() for i, o in enumerate(outs)]


def range_decode_vec(streams, ns):
    """Planes through the 16-lane AVX-512 decoder loop on this thread (raises on CPUs without AVX-512)."""
    ss = [np.ascontiguousarray(s, dtype=np.uint8).ravel() for s in streams]
    k = len(ss)
    outs = [np.zeros(max(n, 1), dtype=np.uint8) for n in ns]
    got = (C.c_size_t * k)()
    _check(lib().wr_range_decode_vec(k, (C.c_void_p * k)(*[s.ctypes.data for s in ss]), (C.c_size_t * k)(*[s.size for s in ss]),
                                     (C.c_void_p * k)(*[o.ctypes.data for o in outs]), (C.c_size_t * k)(*ns), got))
    return [o[:n] for o, n in zip(outs, ns)], [got[i] for i in range(k)]


# ---------------------------------------------------------------------------------------
# drop-in interface on host arrays (reference src/core/wrappers.h)
# ---------------------------------------------------------------------------------------
def setup_wr(nx, ny, nz):
    nl, cap = C.c_ubyte(), C.c_ulong()
    lib().setup_wr(nx, ny, nz, C.byref(nl), C.byref(cap))
    return nl.value, cap.value


def encoding_wrap(fld, tolrel, wtflag=1):
    """fld: float64 array shaped (nz, ny, nx).  Returns the reference's outputs as a dict
    (tolabs, midval, halfspanval, wlev, nlay, ntot_enc, deps_vec, minval_vec, len_enc_vec, data)."""
    fld = np.ascontiguousarray(fld, dtype=np.float64)
    nz, ny, nx = fld.shape
    work = fld.copy()
    _, cap = setup_wr(nx, ny, nz)
    data = np.empty(cap, dtype=np.uint8)
    cut = np.array([tolrel], dtype=np.float64)
    tolabs, midval, halfspan = C.c_double(), C.c_double(), C.c_double()
    wlev, nlay, ntot_enc = C.c_ubyte(), C.c_ubyte(), C.c_ulong()
    deps, mins = np.zeros(NLAYMAX), np.zeros(NLAYMAX)
    lens = np.zeros(NLAYMAX, dtype=np.uint64)
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    lib().encoding_wrap(nx, ny, nz, p(work, _dp), wtflag, 1, 1, 1, p(cut, _dp), C.byref(tolabs),
                        C.byref(midval), C.byref(halfspan), C.byref(wlev), C.byref(nlay),
                        C.byref(ntot_enc), p(deps, _dp), p(mins, _dp), p(lens, _ulp), p(data, _u8p))
    L = nlay.value
    return dict(tolabs=tolabs.value, midval=midval.value, halfspanval=halfspan.value, wlev=wlev.value,
                nlay=L, ntot_enc=ntot_enc.value, deps_vec=deps[:L].copy(), minval_vec=mins[:L].copy(),
                len_enc_vec=[int(v) for v in lens[:L]], data=data[:ntot_enc.value].copy(), residual=work)


def decoding_wrap(enc, shape):
    nz, ny, nx = shape
    out = np.empty(nz * ny * nx, dtype=np.float64)
    deps, mins = np.zeros(NLAYMAX), np.zeros(NLAYMAX)
    lens = np.zeros(NLAYMAX, dtype=np.uint64)
    L = enc["nlay"]
    deps[:L], mins[:L], lens[:L] = enc["deps_vec"], enc["minval_vec"], enc["len_enc_vec"]
    data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
    if data.size == 0:
        data = np.zeros(1, dtype=np.uint8)
    tolabs, midval, halfspan = C.c_double(enc.get("tolabs", 0.0)), C.c_double(enc["midval"]), \
        C.c_double(enc.get("halfspanval", 0.0))
    wlev, nlay, ntot_enc = C.c_ubyte(enc["wlev"]), C.c_ubyte(L), C.c_ulong(enc["ntot_enc"])
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    lib().decoding_wrap(nx, ny, nz, p(out, _dp), C.byref(tolabs), C.byref(midval), C.byref(halfspan),
                        C.byref(wlev), C.byref(nlay), C.byref(ntot_enc), p(deps, _dp), p(mins, _dp),
                        p(lens, _ulp), p(data, _u8p))
    return out.reshape(shape)


# the stream format the drop-in encoders write (wr_set_stream_format; the decoders read what the bytes say)
FORMAT_REF, FORMAT_WRS1, FORMAT_WRS2, FORMAT_WRS3 = 0, 1, 2, 3


def stream_format_parse(text):
    """(format, seg, brick, strands) of "ref" | "wrs1" | "wrs2" | "wrs3" [":seg=N"] [":brick=B"] [":strands=K"], defaults filled
    in; WaveRangeError (error -1, the message quotes the offending token) for anything else."""
    f, seg, brick, strands = C.c_int(), C.c_uint(), C.c_uint(), C.c_uint()
    _check(lib().wr_stream_format_parse(text.encode(), C.byref(f), C.byref(seg), C.byref(brick), C.byref(strands)))
    return f.value, seg.value, brick.value, strands.value


def set_stream_format(text):
    """What encoding_wrap (and every other implicit-context encoder of the library) writes from now on, process-wide; None:
    the reference's stream.  Overrides WR_STREAM_FORMAT."""
    _check(lib().wr_set_stream_format(*(stream_format_parse(text) if text is not None else (FORMAT_REF, 0, 0, 0))))


def stream_format():
    """(format, seg, brick, strands) in force: the last set_stream_format, else WR_STREAM_FORMAT, else the reference's stream."""
    f, seg, brick, strands = C.c_int(), C.c_uint(), C.c_uint(), C.c_uint()
    _check(lib().wr_get_stream_format(C.byref(f), C.byref(seg), C.byref(brick), C.byref(strands)))
    return f.value, seg.value, brick.value, strands.value


def stream_sniff(buf):
    """FORMAT_* of a coded field's first bytes (bytes or a uint8 array); -1: neither a reference stream nor a segmented one."""
    b = np.frombuffer(bytes(buf[:4]), dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.ascontiguousarray(buf, dtype=np.uint8).ravel()[:4]
    return int(lib().wr_stream_sniff(b.ctypes.data if b.size else None, b.size))


def _format_args(format):
    """(format, seg, brick, strands) of a format text, or of such a tuple as it stands (0 = the format's default)"""
    return stream_format_parse(format) if isinstance(format, str) else tuple(int(v) for v in format)


def transcode_bound(n, nlay, format):
    """Bytes that hold any transcode of nlay planes of n symbols into `format` (text, or a (format, seg, brick, strands) tuple):
    nlay times the per-plane bound of the target; 0 if an argument is refused."""
    return int(lib().wr_transcode_bound(n, nlay, *_format_args(format)))


def _transcode(call, shape, info, data, format, cap, out=None):
    nz, ny, nx = shape
    fmt = _format_args(format)
    src = np.ascontiguousarray(data, dtype=np.uint8).ravel()
    i_in, i_out = EncInfo.from_dict(info), EncInfo()
    if cap is None:
        cap = out.size if out is not None else transcode_bound(nx * ny * nz, i_in.nlay, fmt)
    if out is None:
        out = np.empty(max(int(cap), 1), dtype=np.uint8)
    assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= cap
    _check(call(nx, ny, nz, C.byref(i_in), src.ctypes.data if src.size else None, src.size, *fmt, C.byref(i_out), out.ctypes.data, int(cap)))
    d = i_out.as_dict()
    d["data"] = out[:i_out.ntot_enc]
    return d["data"], d


def transcode_host_ref(shape, info, data, format, cap=None, out=None):
    """The definition of Context.transcode on the calling thread (no context, no GPU): the coded field `data` with the header
    record `info` (the dict an encode returns; its "data" entry is not looked at) of a field shaped (nz, ny, nx), in the stream
    format `format`.  Returns (data_out, info_out); info_out is info with the new lengths and carries data_out as "data".  cap: the
    bytes the output may take (default: transcode_bound); out: a uint8 array to code into (e.g. a pinned one)."""
    return _transcode(lib().wr_transcode_host_ref, shape, info, data, format, cap, out)


def waveletcdf97_3d(x, lvl):
    y = np.ascontiguousarray(x, dtype=np.float64).copy()
    nz, ny, nx = y.shape
    lib().waveletcdf97_3d(nx, ny, nz, lvl, y.ctypes.data_as(_dp))
    return y


# ---------------------------------------------------------------------------------------
# device-resident interface
# ---------------------------------------------------------------------------------------
class DeviceBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        p = _vp()
        _check(lib().wr_dev_alloc(ctx.h, C.byref(p), nbytes))
        self.ptr = p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        _check(lib().wr_dev_upload(self.ctx.h, self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self, dtype, count, offset=0):
        out = np.empty(count, dtype=dtype)
        _check(lib().wr_dev_download(self.ctx.h, out.ctypes.data, self.ptr + offset, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().wr_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """One GPU context (device + stream + work space): wr_ctx of include/waverange_amd.h."""

    def __init__(self, device=0, stream=None):
        h = _vp()
        _check(lib().wr_ctx_create(C.byref(h), device, stream))
        self.h = h

    def close(self):
        if self.h:
            lib().wr_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, a):
        a = np.ascontiguousarray(a)
        return self.alloc(max(a.nbytes, 16)).upload(a)

    def sync(self):
        _check(lib().wr_ctx_sync(self.h))

    def trim(self):
        """idle buffers of the device's plane pool go back to the device (wr_ctx_trim)"""
        _check(lib().wr_ctx_trim(self.h))

    def set_keep_residual(self, keep):
        lib().wr_ctx_set_keep_residual(self.h, int(keep))

    def copy(self, dst, src, nbytes):
        _check(lib().wr_dev_copy(self.h, dst.ptr, src.ptr, nbytes))

    def linf(self, a, b, n):
        """(max|a-b|, max|a|) over n doubles."""
        d, m = C.c_double(), C.c_double()
        _check(lib().wr_dev_linf(self.h, a.ptr, b.ptr, n, C.byref(d), C.byref(m)))
        return d.value, m.value

    def transform(self, buf, shape, lvl):
        nz, ny, nx = shape
        _check(lib().wr_dev_transform(self.h, buf.ptr, nx, ny, nz, lvl))

    def minmax(self, buf, n):
        a, b = C.c_double(), C.c_double()
        _check(lib().wr_dev_minmax(self.h, buf.ptr, n, C.byref(a), C.byref(b)))
        return a.value, b.value

    def quantize_plane(self, buf, n, deps, minval, qbuf):
        a, b = C.c_double(), C.c_double()
        _check(lib().wr_dev_quantize_plane(self.h, buf.ptr, n, deps, minval, qbuf.ptr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def dequant_accum(self, acc, n, planes, deps, minval):
        arr = (_vp * len(planes))(*[p if isinstance(p, int) else p.ptr for p in planes])
        d = np.ascontiguousarray(deps, dtype=np.float64)
        m = np.ascontiguousarray(minval, dtype=np.float64)
        _check(lib().wr_dev_dequant_accum(self.h, acc.ptr, n, len(planes), arr, d.ctypes.data_as(_dp),
                                          m.ctypes.data_as(_dp)))

    def synth_field(self, buf, nx, ny, nz, seed):
        _check(lib().wr_dev_synth_field(self.h, buf.ptr, nx, ny, nz, seed))

    def encode_planes(self, buf, shape, tolrel, planes, wtflag=1):
        nz, ny, nx = shape
        info = EncInfo()
        _check(lib().wr_dev_encode_planes(self.h, buf.ptr, nx, ny, nz, wtflag, tolrel, planes.ptr, C.byref(info)))
        return info

    def decode_planes(self, buf, shape, planes, info):
        nz, ny, nx = shape
        _check(lib().wr_dev_decode_planes(self.h, buf.ptr, nx, ny, nz, planes.ptr, C.byref(info)))

    def encode(self, buf, shape, tolrel, wtflag=1, out=None):
        """Whole encode with the field resident on the device.  `buf` is consumed: it holds the residual in wavelet space
        afterwards if set_keep_residual(True) was called on the context, otherwise its contents are unspecified.  Returns
        (info dict incl. data, timings)."""
        nz, ny, nx = shape
        _, cap = setup_wr(nx, ny, nz)
        data = out if out is not None else np.empty(cap, dtype=np.uint8)
        info, tm = EncInfo(), Timings()
        _check(lib().wr_encode_device(self.h, buf.ptr, nx, ny, nz, wtflag, tolrel, C.byref(info),
                                      data.ctypes.data, data.size, C.byref(tm)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc]
        return d, tm.as_dict()

    def encode_local(self, buf, shape, cutoff, m, wtflag=1):
        """Encode with the reference's non-uniform cutoff: cutoff has mx*my*mz entries, m = (mx, my, mz)."""
        nz, ny, nx = shape
        _, cap = setup_wr(nx, ny, nz)
        data = np.empty(cap, dtype=np.uint8)
        cut = np.ascontiguousarray(cutoff, dtype=np.float64)
        info, tm = EncInfo(), Timings()
        _check(lib().wr_encode_device_local(self.h, buf.ptr, nx, ny, nz, wtflag, m[0], m[1], m[2],
                                            cut.ctypes.data_as(_dp), C.byref(info), data.ctypes.data, data.size,
                                            C.byref(tm)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc].copy()
        return d, tm.as_dict()

    def decode(self, buf, shape, enc):
        nz, ny, nx = shape
        info = EncInfo.from_dict(enc)
        tm = Timings()
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        _check(lib().wr_decode_device(self.h, buf.ptr, nx, ny, nz, C.byref(info), data.ctypes.data, data.size,
                                      C.byref(tm)))
        return tm.as_dict()

    # ---- host buffer to host buffer (what encoding_wrap / decoding_wrap run on)
    def encode_host(self, fld, tolrel, wtflag=1, out=None, cutoff=None, m=(1, 1, 1)):
        """fld: C-contiguous float64 array shaped (nz, ny, nx), pinned (pinned_array) or pageable; left
        untouched unless set_keep_residual(True).  Returns (info dict incl. data, timings)."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        nz, ny, nx = fld.shape
        _, cap = setup_wr(nx, ny, nz)
        data = out if out is not None else np.empty(cap, dtype=np.uint8)
        cut = np.ascontiguousarray([tolrel] if cutoff is None else cutoff, dtype=np.float64)
        info, tm = EncInfo(), Timings()
        _check(lib().wr_encode_host(self.h, fld.ctypes.data, nx, ny, nz, wtflag, m[0], m[1], m[2],
                                    cut.ctypes.data_as(_dp), C.byref(info), data.ctypes.data, data.size, C.byref(tm)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc]
        return d, tm.as_dict()

    def decode_host(self, out, enc):
        """out: C-contiguous float64 array shaped (nz, ny, nx) that receives the reconstruction."""
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"]
        nz, ny, nx = out.shape
        info = EncInfo.from_dict(enc)
        tm = Timings()
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        _check(lib().wr_decode_host(self.h, out.ctypes.data, nx, ny, nz, C.byref(info), data.ctypes.data, data.size,
                                    C.byref(tm)))
        return tm.as_dict()

    def encode_host_f32(self, fld, tolrel, wtflag=1, out=None, cutoff=None, m=(1, 1, 1)):
        """encode_host for a C-contiguous float32 field (pinned or pageable), never written: the coded stream of the field
        widened to float64, with 4 bytes per sample crossing the bus."""
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("encode_host_f32: a C-contiguous float32 array is required")
        nz, ny, nx = fld.shape
        _, cap = setup_wr(nx, ny, nz)
        data = out if out is not None else np.empty(cap, dtype=np.uint8)
        cut = np.ascontiguousarray([tolrel] if cutoff is None else cutoff, dtype=np.float64)
        info, tm = EncInfo(), Timings()
        _check(lib().wr_encode_host_f32(self.h, fld.ctypes.data, nx, ny, nz, wtflag, m[0], m[1], m[2],
                                        cut.ctypes.data_as(_dp), C.byref(info), data.ctypes.data, data.size, C.byref(tm)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc]
        return d, tm.as_dict()

    def decode_host_f32(self, out, enc):
        """out: C-contiguous float32 array shaped (nz, ny, nx); receives (float) of decode_host's reconstruction."""
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]):
            raise TypeError("decode_host_f32: a C-contiguous float32 array is required")
        nz, ny, nx = out.shape
        info = EncInfo.from_dict(enc)
        tm = Timings()
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        _check(lib().wr_decode_host_f32(self.h, out.ctypes.data, nx, ny, nz, C.byref(info), data.ctypes.data, data.size,
                                        C.byref(tm)))
        return tm.as_dict()

    # ---- segmented plane streams ("WRS1"): the planes are coded and decoded by the GPU; not readable by the reference's tools
    def _seg_cap(self, shape, seg, brick=None, strands=None):
        nz, ny, nx = shape
        _, cap = setup_wr(nx, ny, nz)
        n = nx * ny * nz
        bound = seg_bound_strands(n, seg, strands) if strands is not None else seg_bound(n, seg) if brick is None else seg_bound_blocked(n, seg)
        return cap + NLAYMAX * max(bound - n, 0)

    def _encode_seg(self, fn, ptr, shape, tolrel, wtflag, seg, out, cutoff, m, brick=None, strands=None):
        """brick is None: `fn` is a WRS1 encoder; otherwise its _blocked form (brick = 0: BRICK_DEFAULT).  strands is not None:
        `fn` is the _strands form (WRS3; strands = 0: STRANDS_DEFAULT; brick None or 0: the natural order)"""
        nz, ny, nx = shape
        data = out if out is not None else np.empty(self._seg_cap(shape, seg, brick, strands), dtype=np.uint8)
        cut = np.ascontiguousarray([tolrel] if cutoff is None else cutoff, dtype=np.float64)
        info, tm = EncInfo(), Timings()
        fmt = (seg, brick or 0, strands) if strands is not None else (seg,) if brick is None else (seg, brick)
        _check(fn(self.h, ptr, nx, ny, nz, wtflag, m[0], m[1], m[2], cut.ctypes.data_as(_dp), *fmt, C.byref(info),
                  data.ctypes.data, data.size, C.byref(tm)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc]
        return d, tm.as_dict()

    def _decode_seg(self, fn, ptr, shape, enc):
        nz, ny, nx = shape
        info = EncInfo.from_dict(enc)
        tm = Timings()
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        _check(fn(self.h, ptr, nx, ny, nz, C.byref(info), data.ctypes.data, data.size, C.byref(tm)))
        return tm.as_dict()

    def encode_host_seg(self, fld, tolrel, wtflag=1, seg=0, out=None, cutoff=None, m=(1, 1, 1), brick=None, strands=None):
        """encode_host with every plane as a segmented blob (seg = 0: SEG_DEFAULT); header scalars as encode_host's.  brick is
        None: WRS1; otherwise the blocked order ("WRS2") with that brick edge (0: BRICK_DEFAULT).  strands is not None: stranded
        segments ("WRS3") with that many strands (0: STRANDS_DEFAULT), in the natural order (brick None or 0) or the blocked
        order with the brick edge `brick`.  The decoders read all three."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        fn = lib().wr_encode_host_seg_strands if strands is not None else lib().wr_encode_host_seg if brick is None else lib().wr_encode_host_seg_blocked
        return self._encode_seg(fn, fld.ctypes.data, fld.shape, tolrel, wtflag, seg, out, cutoff, m, brick, strands)

    def decode_host_seg(self, out, enc):
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"]
        return self._decode_seg(lib().wr_decode_host_seg, out.ctypes.data, out.shape, enc)

    def encode_host_seg_f32(self, fld, tolrel, wtflag=1, seg=0, out=None, cutoff=None, m=(1, 1, 1), brick=None, strands=None):
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("encode_host_seg_f32: a C-contiguous float32 array is required")
        fn = (lib().wr_encode_host_seg_strands_f32 if strands is not None else
              lib().wr_encode_host_seg_f32 if brick is None else lib().wr_encode_host_seg_blocked_f32)
        return self._encode_seg(fn, fld.ctypes.data, fld.shape, tolrel, wtflag, seg, out, cutoff, m, brick, strands)

    def decode_host_seg_f32(self, out, enc):
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]):
            raise TypeError("decode_host_seg_f32: a C-contiguous float32 array is required")
        return self._decode_seg(lib().wr_decode_host_seg_f32, out.ctypes.data, out.shape, enc)

    def encode_seg(self, buf, shape, tolrel, wtflag=1, seg=0, out=None, cutoff=None, m=(1, 1, 1), brick=None, strands=None):
        """encode_host_seg with the field resident on the device (`buf` is consumed, as by encode)."""
        fn = lib().wr_encode_device_seg_strands if strands is not None else lib().wr_encode_device_seg if brick is None else lib().wr_encode_device_seg_blocked
        return self._encode_seg(fn, buf.ptr, shape, tolrel, wtflag, seg, out, cutoff, m, brick, strands)

    # ---- masked fields: undefined samples (not finite, or below `below`) travel as a bit mask behind the field's planes
    def _encode_seg_masked(self, fn, ptr, shape, tolrel, below, wtflag, seg, brick, strands, out, cutoff, m):
        nz, ny, nx = shape
        cap = self._seg_cap(shape, seg, brick if brick else None, strands if strands else None) + mask_bound(nx * ny * nz, seg)
        data = out if out is not None else np.empty(cap, dtype=np.uint8)
        cut = np.ascontiguousarray([tolrel] if cutoff is None else cutoff, dtype=np.float64)
        info, tm, res = EncInfo(), Timings(), MaskResult()
        _check(fn(self.h, ptr, nx, ny, nz, wtflag, m[0], m[1], m[2], cut.ctypes.data_as(_dp), seg, brick, strands, float(below), C.byref(info),
                  data.ctypes.data, data.size, C.byref(tm), C.byref(res)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc + res.mask_len]
        d["mask"] = res.as_dict()
        return d, tm.as_dict()

    def encode_host_seg_masked(self, fld, tolrel, below=-np.inf, wtflag=1, seg=0, brick=0, strands=0, out=None, cutoff=None, m=(1, 1, 1)):
        """encode_host_seg of `fld` with its undefined samples -- not finite, or < below -- replaced by the mean of the defined
        ones, and the mask blob behind the planes (wr_encode_host_seg_masked).  brick = 0, strands = 0: WRS1; brick > 0: WRS2;
        strands > 0: WRS3.  The record's "data" holds ntot_enc bytes of planes, then mask["mask_len"] bytes of mask blob;
        "mask" = {"undefined", "pad", "mask_len", ...}.  data[:ntot_enc] is what every other decoder reads."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        return self._encode_seg_masked(lib().wr_encode_host_seg_masked, fld.ctypes.data, fld.shape, tolrel, below, wtflag, seg, brick, strands, out, cutoff, m)

    def encode_host_seg_masked_f32(self, fld, tolrel, below=-np.inf, wtflag=1, seg=0, brick=0, strands=0, out=None, cutoff=None, m=(1, 1, 1)):
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("encode_host_seg_masked_f32: a C-contiguous float32 array is required")
        return self._encode_seg_masked(lib().wr_encode_host_seg_masked_f32, fld.ctypes.data, fld.shape, tolrel, below, wtflag, seg, brick, strands, out, cutoff, m)

    def encode_seg_masked(self, buf, shape, tolrel, below=-np.inf, wtflag=1, seg=0, brick=0, strands=0, out=None, cutoff=None, m=(1, 1, 1)):
        """encode_host_seg_masked with the field resident on the device (`buf` is consumed, as by encode)."""
        return self._encode_seg_masked(lib().wr_encode_device_seg_masked, buf.ptr, shape, tolrel, below, wtflag, seg, brick, strands, out, cutoff, m)

    def _decode_seg_masked(self, fn, ptr, shape, enc, fill):
        nz, ny, nx = shape
        info = EncInfo.from_dict(enc)
        tm, res = Timings(), MaskResult()
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        src = data if data.size else np.zeros(1, dtype=np.uint8)
        _check(fn(self.h, ptr, nx, ny, nz, C.byref(info), src.ctypes.data, data.size, float(fill), C.byref(tm), C.byref(res)))
        return res.as_dict(), tm.as_dict()

    def decode_host_seg_masked(self, out, enc, fill=np.nan):
        """decode_host_seg of a masked record (enc["data"]: planes, then the mask blob), the undefined samples set to `fill`; a
        record without a mask blob decodes as decode_host_seg.  Returns (mask, timings)."""
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"]
        return self._decode_seg_masked(lib().wr_decode_host_seg_masked, out.ctypes.data, out.shape, enc, fill)

    def decode_host_seg_masked_f32(self, out, enc, fill=np.nan):
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]):
            raise TypeError("decode_host_seg_masked_f32: a C-contiguous float32 array is required")
        return self._decode_seg_masked(lib().wr_decode_host_seg_masked_f32, out.ctypes.data, out.shape, enc, fill)

    def decode_seg_masked(self, buf, shape, enc, fill=np.nan):
        """decode_host_seg_masked into a field resident on the device."""
        return self._decode_seg_masked(lib().wr_decode_device_seg_masked, buf.ptr, shape, enc, fill)

    # ---- masked region / low-resolution decode: roi = ((z0, z1), (y0, y1), (x0, x1)) in the box of `level`, None: the whole box
    def _decode_seg_roi_masked(self, fn, ptr, shape, level, roi, enc, fill, max_planes):
        nz, ny, nx = shape
        info = EncInfo.from_dict(enc)
        tm, res = Timings(), MaskResult()
        r = C.byref(_box(roi)) if roi is not None else None
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        src = data if data.size else np.zeros(1, dtype=np.uint8)
        _check(fn(self.h, ptr, nx, ny, nz, level, max_planes, r, C.byref(info), src.ctypes.data, data.size, float(fill), C.byref(tm), C.byref(res)))
        return res.as_dict(), tm.as_dict()

    def decode_host_seg_roi_masked(self, out, shape, level, roi, enc, fill=np.nan, max_planes=0):
        """decode_host_seg_roi (roi = None: decode_host_seg_lowres) of a masked record, `fill` where the coarse mask says
        undefined; only the mask segments of the region are decoded.  mask["undefined"] counts inside the returned box.
        Returns (mask, timings) (wr_decode_host_seg_roi_masked)."""
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"]
        assert tuple(out.shape) == (roi_shape(roi) if roi is not None else lowres_shape(shape, level))
        return self._decode_seg_roi_masked(lib().wr_decode_host_seg_roi_masked, out.ctypes.data, shape, level, roi, enc, fill, max_planes)

    def decode_host_seg_roi_masked_f32(self, out, shape, level, roi, enc, fill=np.nan, max_planes=0):
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]):
            raise TypeError("decode_host_seg_roi_masked_f32: a C-contiguous float32 array is required")
        assert tuple(out.shape) == (roi_shape(roi) if roi is not None else lowres_shape(shape, level))
        return self._decode_seg_roi_masked(lib().wr_decode_host_seg_roi_masked_f32, out.ctypes.data, shape, level, roi, enc, fill, max_planes)

    def decode_seg_roi_masked(self, buf, shape, level, roi, enc, fill=np.nan, max_planes=0):
        """decode_host_seg_roi_masked into device memory: `buf` holds the region's elements as float64."""
        return self._decode_seg_roi_masked(lib().wr_decode_device_seg_roi_masked, buf.ptr, shape, level, roi, enc, fill, max_planes)

    def mask_restore_box(self, buf, shape, level, roi, bits, fill=np.nan, dtype=np.float64, offset=0, bits_offset=0):
        """Stage level: `fill` into the region `roi` of the box of `level` held contiguously in the device buffer `buf` (from
        ELEMENT `offset`), where the mask plane `bits` (from byte bits_offset) of the field `shape` says undefined; returns the
        count of those samples (wr_dev_mask_restore_box, _f32)."""
        dt = self._mask_dtype("mask_restore_box", dtype)
        fn = lib().wr_dev_mask_restore_box if dt == np.float64 else lib().wr_dev_mask_restore_box_f32
        nz, ny, nx = shape
        r = C.byref(_box(roi)) if roi is not None else None
        undefined = C.c_ulonglong(0)
        _check(fn(self.h, buf.ptr + offset * dt.itemsize, nx, ny, nz, level, r, bits.ptr + bits_offset, float(fill), C.byref(undefined)))
        return int(undefined.value)

    @staticmethod
    def _mask_dtype(who, dtype):
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError(who + ": float64 or float32")
        return dt

    def mask_split(self, fld, n, bits, below=-np.inf, dtype=np.float64, offset=0, bits_offset=0):
        """Stage level: the mask of n samples of the device buffer `fld`, starting `offset` ELEMENTS into it, into the device
        buffer `bits` (ceil(n / 8) bytes from byte bits_offset): (undefined, pad) (wr_dev_mask_split, wr_dev_mask_split_f32)."""
        dt = self._mask_dtype("mask_split", dtype)
        fn = lib().wr_dev_mask_split if dt == np.float64 else lib().wr_dev_mask_split_f32
        undefined, pad = C.c_ulonglong(0), C.c_double(0)
        _check(fn(self.h, fld.ptr + offset * dt.itemsize, int(n), float(below), bits.ptr + bits_offset, C.byref(undefined), C.byref(pad)))
        return int(undefined.value), pad.value

    def mask_fill(self, fld, n, bits, value, dtype=np.float64, offset=0, bits_offset=0):
        """Stage level: `value` into the samples of `fld` whose mask bit is set (wr_dev_mask_fill, wr_dev_mask_fill_f32)."""
        dt = self._mask_dtype("mask_fill", dtype)
        fn = lib().wr_dev_mask_fill if dt == np.float64 else lib().wr_dev_mask_fill_f32
        _check(fn(self.h, fld.ptr + offset * dt.itemsize, int(n), bits.ptr + bits_offset, float(value)))

    def mask_restore(self, fld, n, bits, fill=np.nan, dtype=np.float64, offset=0, bits_offset=0):
        """Stage level: mask_fill with the mask checked; returns the count of its set bits (wr_dev_mask_restore, _f32)."""
        dt = self._mask_dtype("mask_restore", dtype)
        fn = lib().wr_dev_mask_restore if dt == np.float64 else lib().wr_dev_mask_restore_f32
        undefined = C.c_ulonglong(0)
        _check(fn(self.h, fld.ptr + offset * dt.itemsize, int(n), bits.ptr + bits_offset, float(fill), C.byref(undefined)))
        return int(undefined.value)

    # ---- encode to a byte budget: the library picks the tolerance on the grid budget_tol(g), every plane is coded once
    def _encode_seg_budget(self, fn, ptr, shape, max_bytes, tol_min, wtflag, seg, out, m):
        nz, ny, nx = shape
        data = out if out is not None else np.empty(self._seg_cap(shape, seg), dtype=np.uint8)
        info, tm, res = EncInfo(), Timings(), BudgetResult()
        _check(fn(self.h, ptr, nx, ny, nz, wtflag, m[0], m[1], m[2], int(max_bytes), float(tol_min), seg, C.byref(info),
                  data.ctypes.data, data.size, C.byref(tm), C.byref(res)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc]
        return d, d["data"], {"g": res.g, "tolrel": res.tolrel, "bound": res.bound, "probe_passes": res.probe_passes, "timings": tm.as_dict()}

    def encode_host_seg_budget(self, fld, max_bytes, tol_min=2.0 ** -60, wtflag=1, seg=0, out=None, m=(1, 1, 1)):
        """The WRS1 stream of `fld` at the finest tolerance of the grid, not below tol_min, whose size bound fits max_bytes
        (wr_encode_host_seg_budget).  Returns (info, data, result): info as encode_host_seg gives it for
        tolrel = result["tolrel"] = budget_tol(result["g"]), data = info["data"], result["bound"] >= len(data)."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        return self._encode_seg_budget(lib().wr_encode_host_seg_budget, fld.ctypes.data, fld.shape, max_bytes, tol_min, wtflag, seg, out, m)

    def encode_host_seg_budget_f32(self, fld, max_bytes, tol_min=2.0 ** -60, wtflag=1, seg=0, out=None, m=(1, 1, 1)):
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("encode_host_seg_budget_f32: a C-contiguous float32 array is required")
        return self._encode_seg_budget(lib().wr_encode_host_seg_budget_f32, fld.ctypes.data, fld.shape, max_bytes, tol_min, wtflag, seg, out, m)

    def encode_seg_budget(self, buf, shape, max_bytes, tol_min=2.0 ** -60, wtflag=1, seg=0, out=None, m=(1, 1, 1)):
        """encode_host_seg_budget with the field resident on the device (`buf` is consumed, as by encode)."""
        return self._encode_seg_budget(lib().wr_encode_device_seg_budget, buf.ptr, shape, max_bytes, tol_min, wtflag, seg, out, m)

    # ---- encode to a pointwise error bound: the library picks the tolerance on the grid budget_tol(g), every plane is coded once
    def _encode_seg_bounded(self, fn, ptr, shape, max_abs_err, tol_min, wtflag, seg, brick, strands, out, m):
        nz, ny, nx = shape
        cap = self._seg_cap(shape, seg, brick if brick else None, strands if strands else None)
        data = out if out is not None else np.empty(cap, dtype=np.uint8)
        info, tm, res = EncInfo(), Timings(), BoundedResult()
        _check(fn(self.h, ptr, nx, ny, nz, wtflag, m[0], m[1], m[2], float(max_abs_err), float(tol_min), seg, brick, strands, C.byref(info),
                  data.ctypes.data, data.size, C.byref(tm), C.byref(res)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc]
        return d, d["data"], {"g": res.g, "tolrel": res.tolrel, "err": res.err, "trials": res.trials, "timings": tm.as_dict()}

    def encode_host_seg_bounded(self, fld, max_abs_err, tol_min=2.0 ** -60, seg=0, brick=0, strands=0, wtflag=1, out=None, m=(1, 1, 1)):
        """The segmented stream of `fld` at a tolerance of the grid, not below tol_min, whose reconstruction is within
        max_abs_err of `fld` at every sample while the next coarser point's is not (wr_encode_host_seg_bounded).  brick = 0,
        strands = 0: WRS1; brick > 0: WRS2; strands > 0: WRS3.  Returns (info, data, result): info as encode_host_seg gives it for
        tolrel = result["tolrel"] = budget_tol(result["g"]), data = info["data"], result["err"] the error reached."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        return self._encode_seg_bounded(lib().wr_encode_host_seg_bounded, fld.ctypes.data, fld.shape, max_abs_err, tol_min, wtflag, seg, brick, strands, out, m)

    def encode_host_seg_bounded_f32(self, fld, max_abs_err, tol_min=2.0 ** -60, seg=0, brick=0, strands=0, wtflag=1, out=None, m=(1, 1, 1)):
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("encode_host_seg_bounded_f32: a C-contiguous float32 array is required")
        return self._encode_seg_bounded(lib().wr_encode_host_seg_bounded_f32, fld.ctypes.data, fld.shape, max_abs_err, tol_min, wtflag, seg, brick, strands, out, m)

    def encode_seg_bounded(self, buf, shape, max_abs_err, tol_min=2.0 ** -60, seg=0, brick=0, strands=0, wtflag=1, out=None, m=(1, 1, 1)):
        """encode_host_seg_bounded with the field resident on the device (`buf` is consumed, as by encode)."""
        return self._encode_seg_bounded(lib().wr_encode_device_seg_bounded, buf.ptr, shape, max_abs_err, tol_min, wtflag, seg, brick, strands, out, m)

    # ---- encode to an RMS error or a PSNR target: the same search in the L2 norm
    def _encode_seg_quality(self, fn, ptr, shape, norm, target, tol_min, wtflag, seg, brick, strands, out, m):
        nz, ny, nx = shape
        cap = self._seg_cap(shape, seg, brick if brick else None, strands if strands else None)
        data = out if out is not None else np.empty(cap, dtype=np.uint8)
        info, tm, res = EncInfo(), Timings(), QualityResult()
        _check(fn(self.h, ptr, nx, ny, nz, wtflag, m[0], m[1], m[2], int(norm), float(target), float(tol_min), seg, brick, strands, C.byref(info),
                  data.ctypes.data, data.size, C.byref(tm), C.byref(res)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc]
        r = res.as_dict()
        r["timings"] = tm.as_dict()
        return d, d["data"], r

    def encode_host_seg_quality(self, fld, norm, target, tol_min=2.0 ** -60, seg=0, brick=0, strands=0, wtflag=1, out=None, m=(1, 1, 1)):
        """The segmented stream of `fld` at the coarsest tolerance of the grid, not below tol_min, that holds the target while the
        next coarser point does not (wr_encode_host_seg_quality).  norm = NORM_RMS: target is the RMS error allowed, in the
        field's units; NORM_PSNR: target is in dB over the field's range and result["max_rms"] is what it was converted to;
        NORM_MAX: target is the pointwise bound of encode_host_seg_bounded.  Returns (info, data, result): result holds g, tolrel,
        max_abs, rms, sumsq, range, psnr, max_rms, trials (QualityResult)."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        return self._encode_seg_quality(lib().wr_encode_host_seg_quality, fld.ctypes.data, fld.shape, norm, target, tol_min, wtflag, seg, brick, strands, out, m)

    def encode_host_seg_quality_f32(self, fld, norm, target, tol_min=2.0 ** -60, seg=0, brick=0, strands=0, wtflag=1, out=None, m=(1, 1, 1)):
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("encode_host_seg_quality_f32: a C-contiguous float32 array is required")
        return self._encode_seg_quality(lib().wr_encode_host_seg_quality_f32, fld.ctypes.data, fld.shape, norm, target, tol_min, wtflag, seg, brick, strands, out, m)

    def encode_seg_quality(self, buf, shape, norm, target, tol_min=2.0 ** -60, seg=0, brick=0, strands=0, wtflag=1, out=None, m=(1, 1, 1)):
        """encode_host_seg_quality with the field resident on the device (`buf` is consumed, as by encode)."""
        return self._encode_seg_quality(lib().wr_encode_device_seg_quality, buf.ptr, shape, norm, target, tol_min, wtflag, seg, brick, strands, out, m)

    def _seg_error_stats(self, fn, fld, enc):
        nz, ny, nx = fld.shape
        info = EncInfo.from_dict(enc)
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        st = ErrorStats()
        rc = fn(self.h, fld.ctypes.data, nx, ny, nz, C.byref(info), data.ctypes.data, data.size, C.byref(st))
        return rc, st.as_dict()

    def seg_error_stats_host(self, fld, enc, allow_nonfinite=False):
        """max |d|, the sum of squares S, the RMS error R, the field's lo and hi, the PSNR and the count of non-finite differences
        of `fld` against the reconstruction of the segmented stream `enc`, formed and compared on the device
        (wr_seg_error_stats_host).  Differences that are not finite raise unless allow_nonfinite, which returns the record."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        rc, st = self._seg_error_stats(lib().wr_seg_error_stats_host, fld, enc)
        if not (allow_nonfinite and st["nonfinite"] > 0):
            _check(rc)
        return st

    def seg_error_stats_host_f32(self, fld, enc, allow_nonfinite=False):
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("seg_error_stats_host_f32: a C-contiguous float32 array is required")
        rc, st = self._seg_error_stats(lib().wr_seg_error_stats_host_f32, fld, enc)
        if not (allow_nonfinite and st["nonfinite"] > 0):
            _check(rc)
        return st

    def err_stats(self, a, b, n, dtype=np.float64, a_off=0, b_off=0):
        """Stage level: the compare alone on n samples of two device buffers, starting a_off / b_off ELEMENTS into them (any
        alignment): {"max_abs", "sumsq", "rms", "nonfinite", ...} (wr_dev_err_stats, wr_dev_err_stats_f32)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("err_stats: float64 or float32")
        fn = lib().wr_dev_err_stats if dt == np.float64 else lib().wr_dev_err_stats_f32
        st = ErrorStats()
        _check(fn(self.h, a.ptr + a_off * dt.itemsize, b.ptr + b_off * dt.itemsize, int(n), C.byref(st)))
        return st.as_dict()

    # ---- masked fields in the tolerance searches: the error is taken over the defined samples only
    def _encode_seg_quality_masked(self, fn, ptr, shape, norm, target, below, tol_min, wtflag, seg, brick, strands, out, m):
        nz, ny, nx = shape
        cap = self._seg_cap(shape, seg, brick if brick else None, strands if strands else None) + mask_bound(nx * ny * nz, seg)
        data = out if out is not None else np.empty(cap, dtype=np.uint8)
        info, tm, res, mres = EncInfo(), Timings(), QualityResult(), MaskResult()
        _check(fn(self.h, ptr, nx, ny, nz, wtflag, m[0], m[1], m[2], int(norm), float(target), float(tol_min), seg, brick, strands, float(below),
                  C.byref(info), data.ctypes.data, data.size, C.byref(tm), C.byref(res), C.byref(mres)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc + mres.mask_len]
        d["mask"] = mres.as_dict()
        r = res.as_dict()
        r["timings"] = tm.as_dict()
        return d, d["data"], r

    def encode_host_seg_quality_masked(self, fld, norm, target, below=-np.inf, tol_min=2.0 ** -60, seg=0, brick=0, strands=0, wtflag=1, out=None,
                                       m=(1, 1, 1)):
        """encode_host_seg_quality of a masked field: the samples that are not finite or < below are undefined, and max_abs, rms,
        sumsq and psnr are taken over the defined samples only, rms dividing by their count (wr_encode_host_seg_quality_masked).
        norm = NORM_MAX is the masked pointwise bound.  Returns (info, data, result): the record of encode_host_seg_masked at
        tolrel = result["tolrel"] -- info["data"] holds ntot_enc bytes of planes, then info["mask"]["mask_len"] bytes of mask blob --
        and the QualityResult of encode_host_seg_quality."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        return self._encode_seg_quality_masked(lib().wr_encode_host_seg_quality_masked, fld.ctypes.data, fld.shape, norm, target, below, tol_min, wtflag,
                                               seg, brick, strands, out, m)

    def encode_host_seg_quality_masked_f32(self, fld, norm, target, below=-np.inf, tol_min=2.0 ** -60, seg=0, brick=0, strands=0, wtflag=1, out=None,
                                           m=(1, 1, 1)):
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("encode_host_seg_quality_masked_f32: a C-contiguous float32 array is required")
        return self._encode_seg_quality_masked(lib().wr_encode_host_seg_quality_masked_f32, fld.ctypes.data, fld.shape, norm, target, below, tol_min,
                                               wtflag, seg, brick, strands, out, m)

    def encode_seg_quality_masked(self, buf, shape, norm, target, below=-np.inf, tol_min=2.0 ** -60, seg=0, brick=0, strands=0, wtflag=1, out=None,
                                  m=(1, 1, 1)):
        """encode_host_seg_quality_masked with the field resident on the device (`buf` is consumed, as by encode)."""
        return self._encode_seg_quality_masked(lib().wr_encode_device_seg_quality_masked, buf.ptr, shape, norm, target, below, tol_min, wtflag, seg,
                                               brick, strands, out, m)

    def _encode_seg_budget_masked(self, fn, ptr, shape, max_bytes, below, tol_min, wtflag, seg, out, m):
        nz, ny, nx = shape
        data = out if out is not None else np.empty(self._seg_cap(shape, seg) + mask_bound(nx * ny * nz, seg), dtype=np.uint8)
        info, tm, res, mres = EncInfo(), Timings(), BudgetResult(), MaskResult()
        _check(fn(self.h, ptr, nx, ny, nz, wtflag, m[0], m[1], m[2], int(max_bytes), float(tol_min), seg, float(below), C.byref(info),
                  data.ctypes.data, data.size, C.byref(tm), C.byref(res), C.byref(mres)))
        d = info.as_dict()
        d["data"] = data[:info.ntot_enc + mres.mask_len]
        d["mask"] = mres.as_dict()
        return d, d["data"], {"g": res.g, "tolrel": res.tolrel, "bound": res.bound, "probe_passes": res.probe_passes, "timings": tm.as_dict()}

    def encode_host_seg_budget_masked(self, fld, max_bytes, below=-np.inf, tol_min=2.0 ** -60, wtflag=1, seg=0, out=None, m=(1, 1, 1)):
        """encode_host_seg_budget of a masked field: the planes and the mask blob together fit max_bytes,
        result["bound"] + info["mask"]["mask_len"] <= max_bytes (wr_encode_host_seg_budget_masked).  Returns (info, data, result):
        the record of encode_host_seg_masked at tolrel = result["tolrel"], and the result of encode_host_seg_budget."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        return self._encode_seg_budget_masked(lib().wr_encode_host_seg_budget_masked, fld.ctypes.data, fld.shape, max_bytes, below, tol_min, wtflag, seg, out, m)

    def encode_host_seg_budget_masked_f32(self, fld, max_bytes, below=-np.inf, tol_min=2.0 ** -60, wtflag=1, seg=0, out=None, m=(1, 1, 1)):
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("encode_host_seg_budget_masked_f32: a C-contiguous float32 array is required")
        return self._encode_seg_budget_masked(lib().wr_encode_host_seg_budget_masked_f32, fld.ctypes.data, fld.shape, max_bytes, below, tol_min, wtflag, seg,
                                              out, m)

    def encode_seg_budget_masked(self, buf, shape, max_bytes, below=-np.inf, tol_min=2.0 ** -60, wtflag=1, seg=0, out=None, m=(1, 1, 1)):
        """encode_host_seg_budget_masked with the field resident on the device (`buf` is consumed, as by encode)."""
        return self._encode_seg_budget_masked(lib().wr_encode_device_seg_budget_masked, buf.ptr, shape, max_bytes, below, tol_min, wtflag, seg, out, m)

    def _seg_error_stats_masked(self, fn, fld, enc, allow_nonfinite):
        nz, ny, nx = fld.shape
        info = EncInfo.from_dict(enc)
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        st, defined = ErrorStats(), C.c_ulonglong(0)
        rc = fn(self.h, fld.ctypes.data, nx, ny, nz, C.byref(info), data.ctypes.data, np.ascontiguousarray(enc["data"]).size, C.byref(st), C.byref(defined))
        d = st.as_dict()
        d["defined"] = int(defined.value)
        if not (allow_nonfinite and d["nonfinite"] > 0):
            _check(rc)
        return d

    def seg_error_stats_host_masked(self, fld, enc, allow_nonfinite=False):
        """seg_error_stats_host of a masked record (enc["data"]: planes, then the mask blob) over the record's defined samples:
        the ErrorStats record with "defined", their count; lo and hi are those of the defined samples.  Whatever `fld` holds at an
        undefined position is never looked at (wr_seg_error_stats_host_masked)."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        return self._seg_error_stats_masked(lib().wr_seg_error_stats_host_masked, fld, enc, allow_nonfinite)

    def seg_error_stats_host_masked_f32(self, fld, enc, allow_nonfinite=False):
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("seg_error_stats_host_masked_f32: a C-contiguous float32 array is required")
        return self._seg_error_stats_masked(lib().wr_seg_error_stats_host_masked_f32, fld, enc, allow_nonfinite)

    def err_stats_masked(self, a, b, n, bits, dtype=np.float64, a_off=0, b_off=0, bits_offset=0):
        """Stage level: err_stats over the samples whose bit of the packed mask in the device buffer `bits` (from byte
        bits_offset) is clear; nothing is read where a bit is set.  The record of err_stats with "defined", the count of samples
        compared, and rms = sqrt(sumsq / defined) (wr_dev_err_stats_masked, wr_dev_err_stats_masked_f32)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("err_stats_masked: float64 or float32")
        fn = lib().wr_dev_err_stats_masked if dt == np.float64 else lib().wr_dev_err_stats_masked_f32
        st, defined = ErrorStats(), C.c_ulonglong(0)
        _check(fn(self.h, a.ptr + a_off * dt.itemsize, b.ptr + b_off * dt.itemsize, int(n), bits.ptr + bits_offset, C.byref(st), C.byref(defined)))
        d = st.as_dict()
        d["defined"] = int(defined.value)
        return d

    def bounded_trial_ms(self):
        """(requantize, inverse, compare) milliseconds summed over the trials of the last bounded encode on this context."""
        a, b, d = C.c_double(0), C.c_double(0), C.c_double(0)
        _check(lib().wr_ctx_bounded_trial_ms(self.h, C.byref(a), C.byref(b), C.byref(d)))
        return float(a.value), float(b.value), float(d.value)

    def _seg_error(self, fn, fld, enc):
        nz, ny, nx = fld.shape
        info = EncInfo.from_dict(enc)
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        err = C.c_double(0)
        _check(fn(self.h, fld.ctypes.data, nx, ny, nz, C.byref(info), data.ctypes.data, data.size, C.byref(err)))
        return float(err.value)

    def seg_error_host(self, fld, enc):
        """max |fld - reconstruction| of the segmented stream `enc`, formed and compared on the device (wr_seg_error_host)."""
        assert fld.dtype == np.float64 and fld.flags["C_CONTIGUOUS"]
        return self._seg_error(lib().wr_seg_error_host, fld, enc)

    def seg_error_host_f32(self, fld, enc):
        if not (isinstance(fld, np.ndarray) and fld.dtype == np.float32 and fld.flags["C_CONTIGUOUS"]):
            raise TypeError("seg_error_host_f32: a C-contiguous float32 array is required")
        return self._seg_error(lib().wr_seg_error_host_f32, fld, enc)

    def requant_accum(self, coef, deps, minval, offset=0):
        """Stage level: the decoder's coefficient sum of the len(deps) planes the quantizer loop cuts from `coef` (float64) with
        those steps and offsets; no plane is written (wr_dev_requant_accum).  offset: bytes the coefficient array is moved off
        its 16-byte alignment on the device (a multiple of 8)."""
        x = np.ascontiguousarray(coef, dtype=np.float64).ravel()
        dv = np.ascontiguousarray(deps, dtype=np.float64).ravel()
        mv = np.ascontiguousarray(minval, dtype=np.float64).ravel()
        assert dv.size == mv.size and offset % 8 == 0
        d_x, d_acc = self.alloc(max(x.nbytes, 16) + offset), self.alloc(max(x.nbytes, 16))
        try:
            if x.size:
                _check(lib().wr_dev_upload(self.h, d_x.ptr + offset, x.ctypes.data, x.nbytes))
            dd = dv if dv.size else np.zeros(1)
            mm = mv if mv.size else np.zeros(1)
            _check(lib().wr_dev_requant_accum(self.h, d_x.ptr + offset, x.size, int(dv.size), dd.ctypes.data_as(_dp), mm.ctypes.data_as(_dp), d_acc.ptr))
            return d_acc.download(np.float64, x.size)
        finally:
            d_x.free()
            d_acc.free()

    def plane_size_bound(self, plane, seg=0):
        """Stage level: the size bound of a plane of symbols, computed on the device (wr_dev_plane_size_bound)."""
        p = np.ascontiguousarray(plane, dtype=np.uint8).ravel()
        d_sym = self.alloc(max(p.size, 16))
        try:
            if p.size:
                d_sym.upload(p)
            got = C.c_size_t(0)
            _check(lib().wr_dev_plane_size_bound(self.h, d_sym.ptr, p.size, seg, C.byref(got)))
            return int(got.value)
        finally:
            d_sym.free()

    def quant_size_probe(self, resid, minval, deps, seg=0):
        """Stage level: the size bounds of the planes the steps `deps` would cut from the residual array `resid` (float64),
        one pass, nothing written (wr_dev_quant_size_probe).  Returns a list of len(deps) integers."""
        r = np.ascontiguousarray(resid, dtype=np.float64).ravel()
        dv = np.ascontiguousarray(deps, dtype=np.float64).ravel()
        d_res = self.to_device(r)
        try:
            got = (C.c_size_t * max(dv.size, 1))()
            _check(lib().wr_dev_quant_size_probe(self.h, d_res.ptr, r.size, float(minval), int(dv.size), dv.ctypes.data_as(_dp), seg, got))
            return [int(got[k]) for k in range(dv.size)]
        finally:
            d_res.free()

    def plane_reorder(self, plane, shape, wlev=4, brick=0, inverse=False):
        """Stage level: a plane (uint8, nz*ny*nx symbols) through the reorder kernel (wr_dev_plane_reorder).  Forward: natural
        order in, blocked order out (plane.ravel()[blocked_order(...)]); inverse: the other way."""
        nz, ny, nx = shape
        p = np.ascontiguousarray(plane, dtype=np.uint8).ravel()
        assert p.size == nx * ny * nz
        d_src, d_dst = self.to_device(p), self.alloc(p.size)
        try:
            _check(lib().wr_dev_plane_reorder(self.h, d_dst.ptr, d_src.ptr, nx, ny, nz, wlev, brick, int(bool(inverse))))
            return d_dst.download(np.uint8, p.size)
        finally:
            d_src.free()
            d_dst.free()

    def plane_reorder_list(self, plane, shape, wlev, brick, ids, inverse=False, fill=None):
        """Stage level: the bricks `ids` (ascending brick ids, reorder_plan's numbering) of a plane through the reorder kernel
        (wr_dev_plane_reorder_list).  The destination first receives `fill` (uint8, nz*ny*nx bytes; None: zeros) and is
        returned: outside the listed bricks it still holds it."""
        nz, ny, nx = shape
        p = np.ascontiguousarray(plane, dtype=np.uint8).ravel()
        f = np.zeros(p.size, dtype=np.uint8) if fill is None else np.ascontiguousarray(fill, dtype=np.uint8).ravel()
        assert p.size == f.size == nx * ny * nz
        v = np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        d_src, d_dst = self.to_device(p), self.to_device(f)
        try:
            _check(lib().wr_dev_plane_reorder_list(self.h, d_dst.ptr, d_src.ptr, nx, ny, nz, wlev, brick, int(bool(inverse)),
                                                   v.ctypes.data if v.size else None, v.size))
            return d_dst.download(np.uint8, p.size)
        finally:
            d_src.free()
            d_dst.free()

    def decode_seg(self, buf, shape, enc):
        return self._decode_seg(lib().wr_decode_device_seg, buf.ptr, shape, enc)

    # ---- low-resolution decode: the box of `level` (lowres_shape) out of the first max_planes planes (0: all of them)
    def decode_planes_lowres(self, buf, shape, level, planes, info, max_planes=0):
        """Stage level: `planes` as encode_planes left them; `buf` receives the box as float64."""
        nz, ny, nx = shape
        _check(lib().wr_dev_decode_planes_lowres(self.h, buf.ptr, nx, ny, nz, level, max_planes, planes.ptr, C.byref(info)))

    def _decode_seg_lowres(self, fn, ptr, shape, level, enc, max_planes):
        nz, ny, nx = shape
        info = EncInfo.from_dict(enc)
        tm = Timings()
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        _check(fn(self.h, ptr, nx, ny, nz, level, max_planes, C.byref(info), data.ctypes.data, data.size, C.byref(tm)))
        return tm.as_dict()

    def decode_host_seg_lowres(self, out, shape, level, enc, max_planes=0):
        """out: C-contiguous float64 array shaped lowres_shape(shape, level); shape: the coded field's (nz, ny, nx)."""
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and tuple(out.shape) == lowres_shape(shape, level)
        return self._decode_seg_lowres(lib().wr_decode_host_seg_lowres, out.ctypes.data, shape, level, enc, max_planes)

    def decode_host_seg_lowres_f32(self, out, shape, level, enc, max_planes=0):
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]):
            raise TypeError("decode_host_seg_lowres_f32: a C-contiguous float32 array is required")
        assert tuple(out.shape) == lowres_shape(shape, level)
        return self._decode_seg_lowres(lib().wr_decode_host_seg_lowres_f32, out.ctypes.data, shape, level, enc, max_planes)

    def decode_seg_lowres(self, buf, shape, level, enc, max_planes=0):
        """decode_host_seg_lowres into device memory: `buf` holds the box's elements as float64."""
        return self._decode_seg_lowres(lib().wr_decode_device_seg_lowres, buf.ptr, shape, level, enc, max_planes)

    # ---- region decode: the sub-box `roi` = ((z0, z1), (y0, y1), (x0, x1)) of the box of `level`, out of the first max_planes planes
    def decode_planes_roi(self, buf, shape, level, roi, planes, info, max_planes=0):
        """Stage level: `planes` as encode_planes left them; `buf` receives the region as float64."""
        nz, ny, nx = shape
        r = _box(roi)
        _check(lib().wr_dev_decode_planes_roi(self.h, buf.ptr, nx, ny, nz, level, max_planes, C.byref(r), planes.ptr, C.byref(info)))

    def _decode_seg_roi(self, fn, ptr, shape, level, roi, enc, max_planes):
        nz, ny, nx = shape
        info = EncInfo.from_dict(enc)
        tm = Timings()
        r = _box(roi)
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        _check(fn(self.h, ptr, nx, ny, nz, level, max_planes, C.byref(r), C.byref(info), data.ctypes.data, data.size, C.byref(tm)))
        return tm.as_dict()

    def decode_host_seg_roi(self, out, shape, level, roi, enc, max_planes=0):
        """out: C-contiguous float64 array shaped roi_shape(roi); shape: the coded field's (nz, ny, nx)."""
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and tuple(out.shape) == roi_shape(roi)
        return self._decode_seg_roi(lib().wr_decode_host_seg_roi, out.ctypes.data, shape, level, roi, enc, max_planes)

    def decode_host_seg_roi_f32(self, out, shape, level, roi, enc, max_planes=0):
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]):
            raise TypeError("decode_host_seg_roi_f32: a C-contiguous float32 array is required")
        assert tuple(out.shape) == roi_shape(roi)
        return self._decode_seg_roi(lib().wr_decode_host_seg_roi_f32, out.ctypes.data, shape, level, roi, enc, max_planes)

    def decode_seg_roi(self, buf, shape, level, roi, enc, max_planes=0):
        """decode_host_seg_roi into device memory: `buf` holds the region's elements as float64."""
        return self._decode_seg_roi(lib().wr_decode_device_seg_roi, buf.ptr, shape, level, roi, enc, max_planes)

    # ---- region decode, many regions per call: the union of the regions' segments decoded once, all used planes in one launch
    def decode_planes_rois(self, buf, shape, level, rois, planes, info, max_planes=0):
        """Stage level: `planes` as encode_planes left them; `buf` receives the regions as float64, region i at element
        roi_multi_offsets(shape, level, rois)[i]."""
        nz, ny, nx = shape
        _check(lib().wr_dev_decode_planes_roi_multi(self.h, buf.ptr, nx, ny, nz, level, max_planes, _boxes(rois), len(rois), planes.ptr, C.byref(info)))

    def _decode_seg_rois(self, fn, ptr, shape, level, rois, enc, max_planes):
        nz, ny, nx = shape
        info = EncInfo.from_dict(enc)
        tm = Timings()
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        _check(fn(self.h, ptr, nx, ny, nz, level, max_planes, _boxes(rois), len(rois), C.byref(info), data.ctypes.data, data.size, C.byref(tm)))
        return tm.as_dict()

    def decode_host_seg_rois(self, shape, level, rois, enc, max_planes=0, dtype=np.float64, timings=None):
        """The regions `rois` (each ((z0, z1), (y0, y1), (x0, x1)) in the box of `level`) of a segmented stream in one call:
        a list of arrays, views of one buffer, each shaped roi_shape(roi) and bit for bit what decode_host_seg_roi (float32:
        decode_host_seg_roi_f32) gives for that region alone.  shape: the coded field's (nz, ny, nx).  timings: a dict that
        receives the call's wr_timings."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("decode_host_seg_rois: dtype must be float64 or float32")
        try:
            offs = roi_multi_offsets(shape, level, rois)
        except WaveRangeError as e:  # (there is no buffer to size: what the call itself would refuse with, WR_ERR_ARG)
            raise WaveRangeError("libwaverange_amd error -1: %s" % e) from None
        out = np.empty(int(offs[-1]), dtype=dt)
        fn = lib().wr_decode_host_seg_roi_multi if dt == np.dtype(np.float64) else lib().wr_decode_host_seg_roi_multi_f32
        tm = self._decode_seg_rois(fn, out.ctypes.data, shape, level, rois, enc, max_planes)
        if timings is not None:
            timings.update(tm)
        return [out[offs[i]:offs[i + 1]].reshape(roi_shape(r)) for i, r in enumerate(rois)]

    def decode_seg_rois(self, buf, shape, level, rois, enc, max_planes=0):
        """decode_host_seg_rois into device memory: `buf` holds roi_multi_offsets(...)[-1] float64 elements, region i at
        element offset [i].  Returns the timings."""
        return self._decode_seg_rois(lib().wr_decode_device_seg_roi_multi, buf.ptr, shape, level, rois, enc, max_planes)

    def seg_decode_lists(self, blobs, ns, lists):
        """Stage level: WRS1 / WRS2 blobs of planes of ns[j] symbols; the segments lists[j] (ascending ids) of every one are
        decoded by ONE launch into planes prefilled with 0xEE.  Returns ([symbols], [bad segments])."""
        return self._seg_decode_lists(lib().wr_dev_seg_decode_lists, blobs, ns, lists)

    def _seg_decode_lists(self, fn, blobs, ns, lists):
        bs = [np.ascontiguousarray(b, dtype=np.uint8).ravel() for b in blobs]
        ls = [np.ascontiguousarray(l, dtype=np.uint32).ravel() for l in lists]
        nj = len(bs)
        assert len(ns) == nj and len(ls) == nj
        d_blob, d_sym = [self.alloc(max(b.size, 16)) for b in bs], [self.alloc(max(int(n), 16)) for n in ns]
        try:
            for d, b in zip(d_blob, bs):
                if b.size:
                    d.upload(b)
            for d, n in zip(d_sym, ns):
                d.upload(np.full(max(int(n), 16), 0xEE, dtype=np.uint8))
            bp = (C.c_void_p * max(nj, 1))(*[d.ptr for d in d_blob])
            sp = (C.c_void_p * max(nj, 1))(*[d.ptr for d in d_sym])
            ln = (C.c_size_t * max(nj, 1))(*[b.size for b in bs])
            nn = (C.c_size_t * max(nj, 1))(*[int(n) for n in ns])
            ip = (C.c_void_p * max(nj, 1))(*[l.ctypes.data if l.size else None for l in ls])
            il = (C.c_size_t * max(nj, 1))(*[l.size for l in ls])
            bad = (C.c_size_t * max(nj, 1))()
            _check(fn(self.h, nj, bp, ln, sp, nn, ip, il, bad))
            return [d.download(np.uint8, int(n)) if n else np.zeros(0, np.uint8) for d, n in zip(d_sym, ns)], [int(bad[j]) for j in range(nj)]
        finally:
            for d in d_blob + d_sym:
                d.free()

    def device_free_bytes(self):
        """The free memory of the context's device (wr_ctx_device_free_bytes): the budget of roi_batch_groups."""
        return int(lib().wr_ctx_device_free_bytes(self.h))

    def seg_decode_lists_mixed(self, blobs, ns, lists):
        """seg_decode_lists that also takes WRS3 blobs (wr_dev_seg_decode_lists_mixed): the WRS1 / WRS2 jobs go through one
        launch, the WRS3 jobs through a second one.  A WRS3 blob's symbols come out in stream order."""
        return self._seg_decode_lists(lib().wr_dev_seg_decode_lists_mixed, blobs, ns, lists)

    def _decode_seg_rois_batch(self, fn, ptr, shape, level, rois, encs, max_planes):
        nz, ny, nx = shape
        nf = len(encs)
        infos = (EncInfo * max(nf, 1))(*[EncInfo.from_dict(e) for e in encs])
        datas = [np.ascontiguousarray(e["data"], dtype=np.uint8) for e in encs]
        datas = [d if d.size else np.zeros(1, dtype=np.uint8) for d in datas]
        ptrs = (C.c_void_p * max(nf, 1))(*[d.ctypes.data for d in datas])
        lens = (C.c_size_t * max(nf, 1))(*[d.size for d in datas])
        tm = Timings()
        _check(fn(self.h, ptr, nf, nx, ny, nz, level, max_planes, _boxes(rois), len(rois), infos, ptrs, lens, C.byref(tm)))
        return tm.as_dict()

    def decode_host_seg_rois_batch(self, shape, level, rois, encs, max_planes=0, dtype=np.float64, timings=None, out=None):
        """The regions `rois` of every coded field of `encs` (same shape; WRS1, WRS2 and WRS3 may be mixed) with at most two
        coder launches for the whole call: a list per field of the list of region arrays -- views of one buffer of
        len(encs) * T elements -- each bit for bit what decode_host_seg_rois gives for that field alone.  out: a flat array
        of that size and dtype to decode into (a pinned one, for instance)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("decode_host_seg_rois_batch: dtype must be float64 or float32")
        try:
            offs = roi_multi_offsets(shape, level, rois)
        except WaveRangeError as e:  # (there is no buffer to size: what the call itself would refuse with, WR_ERR_ARG)
            raise WaveRangeError("libwaverange_amd error -1: %s" % e) from None
        T = int(offs[-1])
        if out is None:
            out = np.empty(max(len(encs), 1) * T, dtype=dt)
        assert out.dtype == dt and out.size >= len(encs) * T and out.flags.c_contiguous
        fn = lib().wr_decode_host_seg_roi_batch if dt == np.dtype(np.float64) else lib().wr_decode_host_seg_roi_batch_f32
        tm = self._decode_seg_rois_batch(fn, out.ctypes.data, shape, level, rois, encs, max_planes)
        if timings is not None:
            timings.update(tm)
        flat = out.reshape(-1)
        return [[flat[f * T + offs[i]:f * T + offs[i + 1]].reshape(roi_shape(r)) for i, r in enumerate(rois)] for f in range(len(encs))]

    def decode_seg_rois_batch(self, buf, shape, level, rois, encs, max_planes=0):
        """decode_host_seg_rois_batch into device memory: `buf` holds len(encs) * roi_multi_offsets(...)[-1] float64 elements,
        region i of field f at element f * T + offset [i].  Returns the timings."""
        return self._decode_seg_rois_batch(lib().wr_decode_device_seg_roi_batch, buf.ptr, shape, level, rois, encs, max_planes)

    # ---- masked region decode across a batch of fields: enc["data"] is a record's planes and, behind them, its mask blob
    def _decode_seg_rois_batch_masked(self, fn, ptr, shape, level, rois, encs, fill, max_planes):
        nz, ny, nx = shape
        nf = len(encs)
        infos = (EncInfo * max(nf, 1))(*[EncInfo.from_dict(e) for e in encs])
        datas = [np.ascontiguousarray(e["data"], dtype=np.uint8) for e in encs]
        keep = [d if d.size else np.zeros(1, dtype=np.uint8) for d in datas]
        ptrs = (C.c_void_p * max(nf, 1))(*[d.ctypes.data for d in keep])
        lens = (C.c_size_t * max(nf, 1))(*[d.size for d in datas])
        tm = Timings()
        res = (MaskResult * max(nf, 1))()
        _check(fn(self.h, ptr, nf, nx, ny, nz, level, max_planes, _boxes(rois), len(rois), infos, ptrs, lens, float(fill), C.byref(tm), res))
        return [res[f].as_dict() for f in range(nf)], tm.as_dict()

    def decode_host_seg_rois_batch_masked(self, shape, level, rois, encs, fill=np.nan, max_planes=0, dtype=np.float64, timings=None, out=None, masks=None):
        """decode_host_seg_rois_batch on records that may carry a mask blob: region i of field f is bit for bit what
        decode_host_seg_roi_masked gives for rois[i] of that record alone, `fill` where the coarse mask says undefined; the
        masks ride in the call's coder launches and one launch restores every region of every field
        (wr_decode_host_seg_roi_batch_masked, _f32).  masks: a list that receives one wr_mask_result dict per field."""
        dt = self._mask_dtype("decode_host_seg_rois_batch_masked", dtype)
        try:
            offs = roi_multi_offsets(shape, level, rois)
        except WaveRangeError as e:
            raise WaveRangeError("libwaverange_amd error -1: %s" % e) from None
        T = int(offs[-1])
        if out is None:
            out = np.empty(max(len(encs), 1) * T, dtype=dt)
        assert out.dtype == dt and out.size >= len(encs) * T and out.flags.c_contiguous
        fn = lib().wr_decode_host_seg_roi_batch_masked if dt == np.dtype(np.float64) else lib().wr_decode_host_seg_roi_batch_masked_f32
        res, tm = self._decode_seg_rois_batch_masked(fn, out.ctypes.data, shape, level, rois, encs, fill, max_planes)
        if timings is not None:
            timings.update(tm)
        if masks is not None:
            masks[:] = res
        flat = out.reshape(-1)
        return [[flat[f * T + offs[i]:f * T + offs[i + 1]].reshape(roi_shape(r)) for i, r in enumerate(rois)] for f in range(len(encs))]

    def decode_host_seg_rois_batch_masked_f32(self, shape, level, rois, encs, fill=np.nan, max_planes=0, timings=None, out=None, masks=None):
        return self.decode_host_seg_rois_batch_masked(shape, level, rois, encs, fill, max_planes, np.float32, timings, out, masks)

    def decode_seg_rois_batch_masked(self, buf, shape, level, rois, encs, fill=np.nan, max_planes=0):
        """decode_host_seg_rois_batch_masked into device memory (float64, the layout of decode_seg_rois_batch).  Returns
        (masks, timings)."""
        return self._decode_seg_rois_batch_masked(lib().wr_decode_device_seg_roi_batch_masked, buf.ptr, shape, level, rois, encs, fill, max_planes)

    def mask_restore_boxes(self, buf, nfields, shape, level, rois, bits, fill=np.nan, dtype=np.float64, offset=0, bits_offset=0, byte_offset=0):
        """Stage level: `fill` into every region of every field that has a mask plane, in one launch.  `buf` holds nfields
        parts of T = roi_multi_offsets(...)[-1] elements from ELEMENT `offset` behind BYTE byte_offset (the pointers may have
        any alignment); bits[f] is field f's mask plane (a device buffer, read from byte bits_offset) or None.  Returns the
        per-field counts (wr_dev_mask_restore_boxes, _f32)."""
        dt = self._mask_dtype("mask_restore_boxes", dtype)
        fn = lib().wr_dev_mask_restore_boxes if dt == np.float64 else lib().wr_dev_mask_restore_boxes_f32
        nz, ny, nx = shape
        assert len(bits) == nfields
        ptrs = (C.c_void_p * max(nfields, 1))(*[None if b is None else b.ptr + bits_offset for b in bits])
        counts = (C.c_ulonglong * max(nfields, 1))()
        _check(fn(self.h, buf.ptr + byte_offset + offset * dt.itemsize, nfields, nx, ny, nz, level, _boxes(rois), len(rois), ptrs, float(fill), counts))
        return [int(counts[f]) for f in range(nfields)]

    def seg_encode_plane(self, plane, seg=0, strands=None):
        """Stage level: one plane of symbols (a numpy uint8 array) through the coder kernels; returns the blob (WRS1, or with
        strands not None WRS3 in the natural order)."""
        p = np.ascontiguousarray(plane, dtype=np.uint8).ravel()
        bound = seg_bound(p.size, seg) if strands is None else seg_bound_strands(p.size, seg, strands)
        if not bound:
            raise WaveRangeError(_BAD_SEG if strands is None else _BAD_SEG_STRANDS)
        d_sym, d_blob = self.alloc(max(p.size, 16)), self.alloc(bound)
        try:
            if p.size:
                d_sym.upload(p)
            got = C.c_size_t(0)
            if strands is None:
                _check(lib().wr_dev_seg_encode(self.h, d_sym.ptr, p.size, seg, d_blob.ptr, bound, C.byref(got)))
            else:
                _check(lib().wr_dev_seg_encode_strands(self.h, d_sym.ptr, p.size, seg, strands, d_blob.ptr, bound, C.byref(got)))
            return d_blob.download(np.uint8, got.value)
        finally:
            d_sym.free()
            d_blob.free()

    def seg_decode_plane(self, blob, n):
        """Stage level: a blob through the decoder kernel; returns (symbols, bad_segments).  Raises for a malformed index
        or a segment that does not decode."""
        b = np.ascontiguousarray(blob, dtype=np.uint8).ravel()
        d_blob, d_sym = self.alloc(max(b.size, 16)), self.alloc(max(n, 16))
        try:
            if b.size:
                d_blob.upload(b)
            bad = C.c_size_t(0)
            _check(lib().wr_dev_seg_decode(self.h, d_blob.ptr, b.size, d_sym.ptr, n, C.byref(bad)))
            return (d_sym.download(np.uint8, n) if n else np.zeros(0, np.uint8)), int(bad.value)
        finally:
            d_blob.free()
            d_sym.free()

    # ---- batched segmented streams: plane l of all fields of a batch in one coder launch; every field's stream is the single call's
    def _encode_seg_batch(self, fn, ptrs, shape, tolrels, wtflag, seg, brick, cutoffs, m, caps=None, strands=None, outs=None, stranded=False):
        """stranded: `fn` is a _batch_strands entry point (strands = 0 or None: STRANDS_DEFAULT; brick None or 0: the natural order)"""
        if strands is not None and not stranded:  # (these C entry points have no such argument: WR_ERR_UNSUPPORTED, as a WRS3 field in their decode batch)
            raise WaveRangeError("libwaverange_amd error -3: stranded segments (WRS3) are not coded in a batch (the _batch_strands calls code them)")
        nz, ny, nx = shape
        nf = len(ptrs)
        b = (brick or 0) if stranded else 0 if brick is None else (brick or BRICK_DEFAULT)
        if cutoffs is None:
            tol = [tolrels] * nf if np.isscalar(tolrels) else list(tolrels)
            cutoffs = [[t] for t in tol]
        cuts = [np.ascontiguousarray(cv, dtype=np.float64) for cv in cutoffs]
        cap = 0 if not nf else self._seg_cap(shape, seg, b, strands or 0) if stranded else self._seg_cap(shape, seg, None if brick is None else b)
        datas = list(outs) if outs is not None else [np.empty(cap if caps is None else caps[i], dtype=np.uint8) for i in range(nf)]
        infos, tm = (EncInfo * max(nf, 1))(), Timings()
        fp = (C.c_void_p * max(nf, 1))(*ptrs)
        cp = (C.c_void_p * max(nf, 1))(*[cv.ctypes.data for cv in cuts])
        dp = (C.c_void_p * max(nf, 1))(*[d.ctypes.data for d in datas])
        sz = (C.c_size_t * max(nf, 1))(*[d.size for d in datas])
        fmt = (seg, b, strands or 0) if stranded else (seg, b)
        _check(fn(self.h, nf, fp, nx, ny, nz, wtflag, m[0], m[1], m[2], cp, *fmt, infos, dp, sz, C.byref(tm)))
        encs = []
        for i in range(nf):
            d = infos[i].as_dict()
            d["data"] = datas[i][:infos[i].ntot_enc]
            encs.append(d)
        return encs, tm.as_dict()

    def _decode_seg_batch(self, fn, ptrs, shape, encs):
        nz, ny, nx = shape
        nf = len(ptrs)
        infos, tm = (EncInfo * max(nf, 1))(), Timings()
        datas = []
        for i, enc in enumerate(encs):
            infos[i] = EncInfo.from_dict(enc)
            d = np.ascontiguousarray(enc["data"], dtype=np.uint8)
            datas.append(d if d.size else np.zeros(1, dtype=np.uint8))
        fp = (C.c_void_p * max(nf, 1))(*ptrs)
        dp = (C.c_void_p * max(nf, 1))(*[d.ctypes.data for d in datas])
        sz = (C.c_size_t * max(nf, 1))(*[d.size for d in datas])
        _check(fn(self.h, nf, fp, nx, ny, nz, infos, dp, sz, C.byref(tm)))
        return tm.as_dict()

    def encode_host_seg_batch(self, fields, tolrels, wtflag=1, seg=0, brick=None, cutoffs=None, m=(1, 1, 1), caps=None, strands=None, outs=None):
        """encode_host_seg for a list of same-shaped float64 fields, plane l of all of them in one coder launch.  tolrels: one
        tolerance or one per field; cutoffs: a local cutoff vector per field instead.  brick is None: WRS1; otherwise WRS2
        (0: BRICK_DEFAULT).  outs: a uint8 array per field for its coded bytes (caps: their sizes, if they are to be allocated
        here).  Returns ([enc dict per field], timings): every enc is what encode_host_seg returns for that field."""
        assert all(f.dtype == np.float64 and f.flags["C_CONTIGUOUS"] and f.shape == fields[0].shape for f in fields)
        shape = fields[0].shape if len(fields) else (1, 1, 1)
        return self._encode_seg_batch(lib().wr_encode_host_seg_batch, [f.ctypes.data for f in fields], shape, tolrels, wtflag, seg, brick, cutoffs, m, caps, strands, outs)

    def decode_host_seg_batch(self, outs, encs):
        """decode_host_seg for a list of streams (WRS1 and WRS2 may be mixed) into the same-shaped float64 arrays `outs`."""
        assert len(outs) == len(encs) and all(o.dtype == np.float64 and o.flags["C_CONTIGUOUS"] and o.shape == outs[0].shape for o in outs)
        shape = outs[0].shape if len(outs) else (1, 1, 1)
        return self._decode_seg_batch(lib().wr_decode_host_seg_batch, [o.ctypes.data for o in outs], shape, encs)

    def encode_host_seg_batch_f32(self, fields, tolrels, wtflag=1, seg=0, brick=None, cutoffs=None, m=(1, 1, 1), caps=None, strands=None, outs=None):
        if not all(isinstance(f, np.ndarray) and f.dtype == np.float32 and f.flags["C_CONTIGUOUS"] and f.shape == fields[0].shape for f in fields):
            raise TypeError("encode_host_seg_batch_f32: C-contiguous float32 arrays of one shape are required")
        shape = fields[0].shape if len(fields) else (1, 1, 1)
        return self._encode_seg_batch(lib().wr_encode_host_seg_batch_f32, [f.ctypes.data for f in fields], shape, tolrels, wtflag, seg, brick, cutoffs, m, caps, strands, outs)

    def decode_host_seg_batch_f32(self, outs, encs):
        if not (len(outs) == len(encs) and all(isinstance(o, np.ndarray) and o.dtype == np.float32 and o.flags["C_CONTIGUOUS"] and o.shape == outs[0].shape for o in outs)):
            raise TypeError("decode_host_seg_batch_f32: C-contiguous float32 arrays of one shape are required")
        shape = outs[0].shape if len(outs) else (1, 1, 1)
        return self._decode_seg_batch(lib().wr_decode_host_seg_batch_f32, [o.ctypes.data for o in outs], shape, encs)

    def encode_seg_batch(self, bufs, shape, tolrels, wtflag=1, seg=0, brick=None, cutoffs=None, m=(1, 1, 1), caps=None, strands=None, outs=None):
        """encode_host_seg_batch with the fields resident on the device (the buffers are consumed, as by encode_seg)."""
        return self._encode_seg_batch(lib().wr_encode_device_seg_batch, [b.ptr for b in bufs], shape, tolrels, wtflag, seg, brick, cutoffs, m, caps, strands, outs)

    def decode_seg_batch(self, bufs, shape, encs):
        assert len(bufs) == len(encs)
        return self._decode_seg_batch(lib().wr_decode_device_seg_batch, [b.ptr for b in bufs], shape, encs)

    # ---- the batch calls for WRS3: the encoders with strands, the decoders that take any mix of WRS1, WRS2 and WRS3 fields
    def encode_host_seg_batch_strands(self, fields, tolrels, wtflag=1, seg=0, brick=0, strands=0, cutoffs=None, m=(1, 1, 1), caps=None, outs=None):
        """encode_host_seg(..., strands=strands) for a list of same-shaped float64 fields, plane l of all of them in one coder
        launch (wr_encode_host_seg_batch_strands).  strands = 0: STRANDS_DEFAULT; brick 0 or None: the natural order.  Returns
        ([enc dict per field], timings): every enc is what encode_host_seg returns for that field with the same parameters."""
        assert all(f.dtype == np.float64 and f.flags["C_CONTIGUOUS"] and f.shape == fields[0].shape for f in fields)
        shape = fields[0].shape if len(fields) else (1, 1, 1)
        return self._encode_seg_batch(lib().wr_encode_host_seg_batch_strands, [f.ctypes.data for f in fields], shape, tolrels, wtflag, seg, brick, cutoffs, m, caps,
                                      strands, outs, True)

    def encode_host_seg_batch_strands_f32(self, fields, tolrels, wtflag=1, seg=0, brick=0, strands=0, cutoffs=None, m=(1, 1, 1), caps=None, outs=None):
        if not all(isinstance(f, np.ndarray) and f.dtype == np.float32 and f.flags["C_CONTIGUOUS"] and f.shape == fields[0].shape for f in fields):
            raise TypeError("encode_host_seg_batch_strands_f32: C-contiguous float32 arrays of one shape are required")
        shape = fields[0].shape if len(fields) else (1, 1, 1)
        return self._encode_seg_batch(lib().wr_encode_host_seg_batch_strands_f32, [f.ctypes.data for f in fields], shape, tolrels, wtflag, seg, brick, cutoffs, m,
                                      caps, strands, outs, True)

    def encode_seg_batch_strands(self, bufs, shape, tolrels, wtflag=1, seg=0, brick=0, strands=0, cutoffs=None, m=(1, 1, 1), caps=None, outs=None):
        """encode_host_seg_batch_strands with the fields resident on the device (the buffers are consumed, as by encode_seg)."""
        return self._encode_seg_batch(lib().wr_encode_device_seg_batch_strands, [b.ptr for b in bufs], shape, tolrels, wtflag, seg, brick, cutoffs, m, caps, strands,
                                      outs, True)

    def decode_host_seg_batch_mixed(self, outs, encs):
        """decode_host_seg for a list of streams -- WRS1, WRS2 and WRS3 mixed freely, each with its own seg, brick edge and strand
        count -- into the same-shaped float64 arrays `outs`: every (field, plane) is a job, the plain jobs go into one coder
        launch and the stranded ones into another (wr_decode_host_seg_batch_mixed)."""
        assert len(outs) == len(encs) and all(o.dtype == np.float64 and o.flags["C_CONTIGUOUS"] and o.shape == outs[0].shape for o in outs)
        shape = outs[0].shape if len(outs) else (1, 1, 1)
        return self._decode_seg_batch(lib().wr_decode_host_seg_batch_mixed, [o.ctypes.data for o in outs], shape, encs)

    def decode_host_seg_batch_mixed_f32(self, outs, encs):
        if not (len(outs) == len(encs) and all(isinstance(o, np.ndarray) and o.dtype == np.float32 and o.flags["C_CONTIGUOUS"] and o.shape == outs[0].shape for o in outs)):
            raise TypeError("decode_host_seg_batch_mixed_f32: C-contiguous float32 arrays of one shape are required")
        shape = outs[0].shape if len(outs) else (1, 1, 1)
        return self._decode_seg_batch(lib().wr_decode_host_seg_batch_mixed_f32, [o.ctypes.data for o in outs], shape, encs)

    def decode_seg_batch_mixed(self, bufs, shape, encs):
        assert len(bufs) == len(encs)
        return self._decode_seg_batch(lib().wr_decode_device_seg_batch_mixed, [b.ptr for b in bufs], shape, encs)

    # ---- masked batch encode and decode: N masked fields per call, their masks in one coder launch
    def _encode_seg_batch_masked(self, fn, ptrs, shape, tolrels, below, wtflag, seg, brick, strands, cutoffs, m, caps, outs):
        nz, ny, nx = shape
        nf = len(ptrs)
        if cutoffs is None:
            tol = [tolrels] * nf if np.isscalar(tolrels) else list(tolrels)
            cutoffs = [[t] for t in tol]
        cuts = [np.ascontiguousarray(cv, dtype=np.float64) for cv in cutoffs]
        cap = self._seg_cap(shape, seg, brick if brick else None, strands if strands else None) + mask_bound(nx * ny * nz, seg) if nf else 0
        datas = list(outs) if outs is not None else [np.empty(cap if caps is None else caps[i], dtype=np.uint8) for i in range(nf)]
        infos, tm = (EncInfo * max(nf, 1))(), Timings()
        res = (MaskResult * max(nf, 1))()
        fp = (C.c_void_p * max(nf, 1))(*ptrs)
        cp = (C.c_void_p * max(nf, 1))(*[cv.ctypes.data for cv in cuts])
        dp = (C.c_void_p * max(nf, 1))(*[d.ctypes.data for d in datas])
        sz = (C.c_size_t * max(nf, 1))(*[d.size for d in datas])
        _check(fn(self.h, nf, fp, nx, ny, nz, wtflag, m[0], m[1], m[2], cp, seg, brick, strands, float(below), infos, dp, sz, C.byref(tm), res))
        encs = []
        for i in range(nf):
            d = infos[i].as_dict()
            d["data"] = datas[i][:infos[i].ntot_enc + res[i].mask_len]
            d["mask"] = res[i].as_dict()
            encs.append(d)
        return encs, tm.as_dict()

    def encode_host_seg_batch_masked(self, fields, tolrels, below=-np.inf, wtflag=1, seg=0, brick=0, strands=0, cutoffs=None, m=(1, 1, 1), caps=None, outs=None):
        """encode_host_seg_masked for a list of same-shaped float64 fields: plane l of all of them in one coder launch and all
        their masks in one launch more (wr_encode_host_seg_batch_masked).  brick = 0, strands = 0: WRS1; brick > 0: WRS2;
        strands > 0: WRS3.  Returns ([record per field], timings): every record is encode_host_seg_masked's for that field."""
        assert all(f.dtype == np.float64 and f.flags["C_CONTIGUOUS"] and f.shape == fields[0].shape for f in fields)
        shape = fields[0].shape if len(fields) else (1, 1, 1)
        return self._encode_seg_batch_masked(lib().wr_encode_host_seg_batch_masked, [f.ctypes.data for f in fields], shape, tolrels, below, wtflag, seg, brick,
                                             strands, cutoffs, m, caps, outs)

    def encode_host_seg_batch_masked_f32(self, fields, tolrels, below=-np.inf, wtflag=1, seg=0, brick=0, strands=0, cutoffs=None, m=(1, 1, 1), caps=None, outs=None):
        if not all(isinstance(f, np.ndarray) and f.dtype == np.float32 and f.flags["C_CONTIGUOUS"] and f.shape == fields[0].shape for f in fields):
            raise TypeError("encode_host_seg_batch_masked_f32: C-contiguous float32 arrays of one shape are required")
        shape = fields[0].shape if len(fields) else (1, 1, 1)
        return self._encode_seg_batch_masked(lib().wr_encode_host_seg_batch_masked_f32, [f.ctypes.data for f in fields], shape, tolrels, below, wtflag, seg, brick,
                                             strands, cutoffs, m, caps, outs)

    def encode_seg_batch_masked(self, bufs, shape, tolrels, below=-np.inf, wtflag=1, seg=0, brick=0, strands=0, cutoffs=None, m=(1, 1, 1), caps=None, outs=None):
        """encode_host_seg_batch_masked with the fields resident on the device (the buffers are consumed): one launch splits
        all of them and one fills them."""
        return self._encode_seg_batch_masked(lib().wr_encode_device_seg_batch_masked, [b.ptr for b in bufs], shape, tolrels, below, wtflag, seg, brick, strands,
                                             cutoffs, m, caps, outs)

    def _decode_seg_batch_masked(self, fn, ptrs, shape, encs, fill):
        nz, ny, nx = shape
        nf = len(ptrs)
        infos, tm = (EncInfo * max(nf, 1))(), Timings()
        res = (MaskResult * max(nf, 1))()
        datas = [np.ascontiguousarray(e["data"], dtype=np.uint8) for e in encs]
        keep = [d if d.size else np.zeros(1, dtype=np.uint8) for d in datas]
        for i, enc in enumerate(encs):
            infos[i] = EncInfo.from_dict(enc)
        fp = (C.c_void_p * max(nf, 1))(*ptrs)
        dp = (C.c_void_p * max(nf, 1))(*[d.ctypes.data for d in keep])
        sz = (C.c_size_t * max(nf, 1))(*[d.size for d in datas])
        _check(fn(self.h, nf, fp, nx, ny, nz, infos, dp, sz, float(fill), C.byref(tm), res))
        return [res[i].as_dict() for i in range(nf)], tm.as_dict()

    def decode_host_seg_batch_masked(self, outs, encs, fill=np.nan):
        """decode_host_seg_masked for a list of records -- WRS1, WRS2 and WRS3, masked, unmasked and constant mixed freely --
        into the same-shaped float64 arrays `outs`: the masks ride in the call's plain coder launch
        (wr_decode_host_seg_batch_masked).  Returns ([mask per field], timings)."""
        assert len(outs) == len(encs) and all(o.dtype == np.float64 and o.flags["C_CONTIGUOUS"] and o.shape == outs[0].shape for o in outs)
        shape = outs[0].shape if len(outs) else (1, 1, 1)
        return self._decode_seg_batch_masked(lib().wr_decode_host_seg_batch_masked, [o.ctypes.data for o in outs], shape, encs, fill)

    def decode_host_seg_batch_masked_f32(self, outs, encs, fill=np.nan):
        if not (len(outs) == len(encs) and all(isinstance(o, np.ndarray) and o.dtype == np.float32 and o.flags["C_CONTIGUOUS"] and o.shape == outs[0].shape for o in outs)):
            raise TypeError("decode_host_seg_batch_masked_f32: C-contiguous float32 arrays of one shape are required")
        shape = outs[0].shape if len(outs) else (1, 1, 1)
        return self._decode_seg_batch_masked(lib().wr_decode_host_seg_batch_masked_f32, [o.ctypes.data for o in outs], shape, encs, fill)

    def decode_seg_batch_masked(self, bufs, shape, encs, fill=np.nan):
        """decode_host_seg_batch_masked into fields resident on the device."""
        assert len(bufs) == len(encs)
        return self._decode_seg_batch_masked(lib().wr_decode_device_seg_batch_masked, [b.ptr for b in bufs], shape, encs, fill)

    def mask_split_batch(self, flds, n, bits, below=-np.inf, dtype=np.float64, offsets=None, bits_offsets=None):
        """Stage level: mask_split of every device buffer of `flds` (n samples from ELEMENT offsets[f]) into the device buffer
        bits[f] (from byte bits_offsets[f]) in one launch: [(undefined, pad) per field], each bit for bit mask_split's
        (wr_dev_mask_split_batch, _f32)."""
        dt = self._mask_dtype("mask_split_batch", dtype)
        fn = lib().wr_dev_mask_split_batch if dt == np.float64 else lib().wr_dev_mask_split_batch_f32
        nf = len(flds)
        off = offsets if offsets is not None else [0] * nf
        boff = bits_offsets if bits_offsets is not None else [0] * nf
        fp = (C.c_void_p * max(nf, 1))(*[f.ptr + o * dt.itemsize for f, o in zip(flds, off)])
        bp = (C.c_void_p * max(nf, 1))(*[b.ptr + o for b, o in zip(bits, boff)])
        undefined, pad = (C.c_ulonglong * max(nf, 1))(), (C.c_double * max(nf, 1))()
        _check(fn(self.h, nf, fp, int(n), float(below), bp, undefined, pad))
        return [(int(undefined[f]), pad[f]) for f in range(nf)]

    def mask_fill_batch(self, flds, n, bits, values, dtype=np.float64, offsets=None, bits_offsets=None):
        """Stage level: mask_fill of every field with its own value in one launch; a None field is skipped
        (wr_dev_mask_fill_batch, _f32)."""
        dt = self._mask_dtype("mask_fill_batch", dtype)
        fn = lib().wr_dev_mask_fill_batch if dt == np.float64 else lib().wr_dev_mask_fill_batch_f32
        nf = len(flds)
        off = offsets if offsets is not None else [0] * nf
        boff = bits_offsets if bits_offsets is not None else [0] * nf
        fp = (C.c_void_p * max(nf, 1))(*[None if f is None else f.ptr + o * dt.itemsize for f, o in zip(flds, off)])
        bp = (C.c_void_p * max(nf, 1))(*[None if b is None else b.ptr + o for b, o in zip(bits, boff)])
        vals = (C.c_double * max(nf, 1))(*[float(v) for v in values])
        _check(fn(self.h, nf, fp, int(n), bp, vals))

    def mask_check_batch(self, bits, n, bits_offsets=None):
        """Stage level: per mask plane of n bits (count of its set bits, whether one lies at or beyond n), one launch, no field
        read (wr_dev_mask_check_batch)."""
        nm = len(bits)
        boff = bits_offsets if bits_offsets is not None else [0] * nm
        bp = (C.c_void_p * max(nm, 1))(*[b.ptr + o for b, o in zip(bits, boff)])
        undefined, beyond = (C.c_ulonglong * max(nm, 1))(), (C.c_ubyte * max(nm, 1))()
        _check(lib().wr_dev_mask_check_batch(self.h, nm, bp, int(n), undefined, beyond))
        return [(int(undefined[k]), bool(beyond[k])) for k in range(nm)]

    def seg_encode_planes_batch_strands(self, planes, seg=0, strands=0):
        """Stage level: planes of one size through ONE batched strand-coder launch sequence; returns the WRS3 blob (natural
        order) of each, byte for byte seg_encode_plane(p, seg, strands=strands)'s."""
        return self.seg_encode_planes_batch(planes, seg, strands)

    def seg_encode_planes_batch(self, planes, seg=0, _strands=None):
        """Stage level: planes of one size (numpy uint8 arrays) through ONE batched coder launch sequence; returns the WRS1
        blob of each, byte for byte seg_encode_plane's."""
        ps = [np.ascontiguousarray(p, dtype=np.uint8).ravel() for p in planes]
        n = ps[0].size if ps else 0
        assert all(p.size == n for p in ps)
        bound = seg_bound(n, seg) if _strands is None else seg_bound_strands(n, seg, _strands)
        if not bound:
            raise WaveRangeError(_BAD_SEG if _strands is None else _BAD_SEG_STRANDS)
        nj = len(ps)
        d_sym, d_blob = [self.alloc(max(n, 16)) for _ in ps], [self.alloc(bound) for _ in ps]
        try:
            for d, p in zip(d_sym, ps):
                if n:
                    d.upload(p)
            sp = (C.c_void_p * max(nj, 1))(*[d.ptr for d in d_sym])
            bp = (C.c_void_p * max(nj, 1))(*[d.ptr for d in d_blob])
            cap = (C.c_size_t * max(nj, 1))(*([bound] * nj))
            got = (C.c_size_t * max(nj, 1))()
            if _strands is None:
                _check(lib().wr_dev_seg_encode_batch(self.h, nj, sp, n, seg, bp, cap, got))
            else:
                _check(lib().wr_dev_seg_encode_batch_strands(self.h, nj, sp, n, seg, _strands, bp, cap, got))
            return [d_blob[j].download(np.uint8, got[j]) for j in range(nj)]
        finally:
            for d in d_sym + d_blob:
                d.free()

    def seg_decode_planes_batch(self, blobs, n):
        """Stage level: WRS1 blobs of planes of n symbols through ONE batched decoder launch; returns ([symbols], [bad segments])."""
        return self._seg_decode_planes_batch(lib().wr_dev_seg_decode_batch, blobs, n, True)

    def seg_decode_planes_batch_mixed(self, blobs, n, check=True):
        """Stage level: WRS1, WRS2 and WRS3 blobs of planes of n symbols, the plain ones through one batched decoder launch and
        the stranded ones through another (wr_dev_seg_decode_batch_mixed); the symbols come out in stream order.  Returns
        ([symbols], [bad segments]).  check = False: segments that do not decode on the device are only counted (the call's
        WR_ERR_STREAM is not raised if some count is non-zero); a header or index refused on the host raises all the same."""
        return self._seg_decode_planes_batch(lib().wr_dev_seg_decode_batch_mixed, blobs, n, check)

    def _seg_decode_planes_batch(self, fn, blobs, n, check):
        bs = [np.ascontiguousarray(b, dtype=np.uint8).ravel() for b in blobs]
        nj = len(bs)
        d_blob, d_sym = [self.alloc(max(b.size, 16)) for b in bs], [self.alloc(max(n, 16)) for _ in bs]
        try:
            for d, b in zip(d_blob, bs):
                if b.size:
                    d.upload(b)
            bp = (C.c_void_p * max(nj, 1))(*[d.ptr for d in d_blob])
            sp = (C.c_void_p * max(nj, 1))(*[d.ptr for d in d_sym])
            ln = (C.c_size_t * max(nj, 1))(*[b.size for b in bs])
            bad = (C.c_size_t * max(nj, 1))()
            rc = fn(self.h, nj, bp, ln, sp, n, bad)
            if check or rc != -4 or not any(bad[j] for j in range(nj)):
                _check(rc)
            return [d.download(np.uint8, n) if n else np.zeros(0, np.uint8) for d in d_sym], [int(bad[j]) for j in range(nj)]
        finally:
            for d in d_blob + d_sym:
                d.free()

    def transcode(self, info, data, format="wrs3", shape=None, cap=None, timings=None, out=None):
        """The coded field `data` with the header record `info` from whatever format it is in to `format` ("ref" | "wrs1" |
        "wrs2" | "wrs3" [":seg=N"] [":brick=B"] [":strands=K"]) on its planes: no transform, no quantizer, byte for byte what
        the target's encoder returns for the original field.  shape: (nz, ny, nx) of the field (or info["shape"]).  Returns
        (data_out, info_out) as transcode_host_ref; timings: a dict that receives the call's wr_timings."""
        if shape is None:
            shape = info["shape"]
        tm = Timings()
        h = self.h
        r = _transcode(lambda *a: lib().wr_transcode_host(h, *a, C.byref(tm)), shape, info, data, format, cap, out)
        if timings is not None:
            timings.update(tm.as_dict())
        return r

    def decode_begin(self, shape, enc):
        """Host half of a decode (range decoding into the context's staging); no output buffer needed yet."""
        nz, ny, nx = shape
        info = EncInfo.from_dict(enc)
        tm = Timings()
        data = np.ascontiguousarray(enc["data"], dtype=np.uint8)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
        _check(lib().wr_decode_begin(self.h, nx, ny, nz, C.byref(info), data.ctypes.data, data.size, C.byref(tm)))
        return tm.as_dict()

    def decode_finish_host(self, out):
        """Device half of the decode begun on this context: upload, kernels, download into `out`."""
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"]
        tm = Timings()
        _check(lib().wr_decode_finish_host(self.h, out.ctypes.data, C.byref(tm)))
        return tm.as_dict()

    def decode_finish_host_f32(self, out):
        """decode_finish_host into a C-contiguous float32 array."""
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]):
            raise TypeError("decode_finish_host_f32: a C-contiguous float32 array is required")
        tm = Timings()
        _check(lib().wr_decode_finish_host_f32(self.h, out.ctypes.data, C.byref(tm)))
        return tm.as_dict()

    def decode_finish(self, buf):
        tm = Timings()
        _check(lib().wr_decode_finish_device(self.h, buf.ptr, C.byref(tm)))
        return tm.as_dict()

    def burn(self, ms, mode=0, workgroups=1024):
        lib().wr_dev_burn.argtypes = [_vp, C.c_double, C.c_int, C.c_int]
        _check(lib().wr_dev_burn(self.h, ms, mode, workgroups))

    def test_stale_window(self, n):
        """Test hook: the window handle of a finished call against the plane of the next one (must be refused)."""
        _check(lib().wr_test_stale_window(self.h, n))

    def transform_host(self, fld, lvl):
        nz, ny, nx = fld.shape
        _check(lib().wr_transform_host(self.h, fld.ctypes.data, nx, ny, nz, lvl))

    def bench_transform(self, buf, shape, lvl, reps=1):
        nz, ny, nx = shape
        ms = C.c_double()
        _check(lib().wr_bench_transform(self.h, buf.ptr, nx, ny, nz, lvl, reps, C.byref(ms)))
        return ms.value
