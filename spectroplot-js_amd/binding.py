"""ctypes binding of include/spectroplot_hip.h.  No compute happens in Python."""
import ctypes as C
import math
import os
import weakref
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

SP_CB_HIST_SIZE = 1000
FORMATS = ["CU4", "CS4", "CU8", "CS8", "CU12", "CS12", "CU16", "CS16", "CU32", "CS32", "CU64", "CS64", "CF32", "CF64"]

SP_ERR_NOT_POW2 = -2
SP_ERR_BYTE_LENGTH = -3
SP_ERR_UNSUPPORTED = -4
SP_ERR_NO_DEVICE = -5
SP_ERR_INVALID_ARG = -1

DETECTORS = {"sample": 0, "peak": 1}       # enum sp_detector


def detector_id(detector):
    """enum sp_detector of "sample" / "peak"; anything else is an error here, never a different image."""
    if detector not in DETECTORS:
        raise SpectroplotError(SP_ERR_INVALID_ARG, "detector must be 'sample' or 'peak', not %r" % (detector,))
    return DETECTORS[detector]


class SpectroplotError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s (status %d)" % (message, status))
        self.status = status


class _Request(C.Structure):
    _fields_ = [("format", C.c_int32), ("n", C.c_int32), ("channel_mode", C.c_int32), ("waterfall", C.c_int32),
                ("lut_len", C.c_int32), ("detector", C.c_int32), ("block_norm", C.c_double), ("gain", C.c_double),
                ("range", C.c_double), ("windowc", C.c_void_p), ("lut_rgb", C.c_void_p)]


class _NamedRequest(C.Structure):
    _fields_ = [("format", C.c_char_p), ("window", C.c_char_p), ("cmap", C.c_char_p), ("n", C.c_int32), ("channel_mode", C.c_int32),
                ("waterfall", C.c_int32), ("gain", C.c_double), ("range", C.c_double)]


class _Reply(C.Structure):
    _fields_ = [("rgba", C.c_void_p), ("gauge_mins", C.c_void_p), ("gauge_maxs", C.c_void_p), ("gauge_amps", C.c_void_p),
                ("c_hist", C.c_void_p), ("cb_hist", C.c_void_p), ("dbfs_minmax", C.c_void_p)]


class _BatchItem(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("nbytes", C.c_size_t), ("width", C.c_int32), ("reserved", C.c_int32), ("reply", _Reply)]


def lib_path():
    # Kernel experiments only (tools/build_variant.sh, tools/ab_variants.sh): with SP_EXPERIMENT_KNOBS=1 in the environment,
    # SP_LIB_VARIANT=<name> loads lib/variants/<name>.so, a copy of the library built with other compile-time options.
    v = os.environ.get("SP_LIB_VARIANT") if os.environ.get("SP_EXPERIMENT_KNOBS") == "1" else None
    if v:
        return os.path.join(_HERE, "lib", "variants", v + ".so")
    return os.path.join(_HERE, "lib", "libspectroplot_hip.so")


def build_library(force=False):
    """Compiles the HIP library in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    target = lib_path()
    if force:
        subprocess.check_call(["make", "-s", "-C", _HERE, "clean"])
    subprocess.check_call(["make", "-s", "-C", _HERE])
    return target


class Library:
    """The loaded shared library.  Fails loudly when it has not been built: there is no fallback path."""
    _instance = None

    def __init__(self, path=None):
        path = path or lib_path()
        if not os.path.exists(path):
            raise SpectroplotError(SP_ERR_NO_DEVICE, "HIP library %s is missing: run __graft_entry__.build() first" % path)
        L = self.L = C.CDLL(path)
        self.path = path
        vp, i32, sz, dbl = C.c_void_p, C.c_int32, C.c_size_t, C.c_double
        L.sp_version.restype = C.c_int
        L.sp_status_string.restype = C.c_char_p
        L.sp_status_string.argtypes = [C.c_int]
        L.sp_last_error.restype = C.c_char_p
        L.sp_last_error.argtypes = [vp]
        L.sp_format_parse.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(i32)]
        L.sp_format_element_size.argtypes = [i32]
        L.sp_slice_bounds.argtypes = [sz, i32, i32, i32, C.POINTER(sz), C.POINTER(sz)]
        L.sp_window.argtypes = [C.c_char_p, i32, vp, C.POINTER(dbl)]
        L.sp_twiddles.argtypes = [i32, vp, vp]
        L.sp_js_log10.restype = dbl
        L.sp_js_log10.argtypes = [dbl]
        L.sp_cmap_count.restype = C.c_int
        L.sp_cmap_key.restype = C.c_char_p
        L.sp_cmap_key.argtypes = [i32]
        L.sp_cmap.argtypes = [C.c_char_p, vp, i32, C.POINTER(i32)]
        L.sp_cmap_generate.argtypes = [C.c_char_p, i32, vp]
        L.sp_plan_execute_from_host.argtypes = [vp, vp, sz, i32, C.POINTER(_Reply)]
        L.sp_device_count.argtypes = [C.POINTER(i32)]
        L.sp_context_create.argtypes = [i32, C.POINTER(vp)]
        L.sp_context_destroy.argtypes = [vp]
        L.sp_context_destroy.restype = None
        L.sp_context_set_stream.argtypes = [vp, vp]
        L.sp_context_synchronize.argtypes = [vp]
        L.sp_render.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, C.POINTER(_Reply)]
        L.sp_render_named.argtypes = [vp, C.POINTER(_NamedRequest), vp, sz, i32, C.POINTER(_Reply)]
        L.sp_named_resolve.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(i32)]
        L.sp_context_plan_creations.argtypes = [vp, C.POINTER(C.c_int64)]
        L.sp_plan_create.argtypes = [vp, C.POINTER(_Request), C.POINTER(vp)]
        L.sp_plan_destroy.argtypes = [vp]
        L.sp_plan_destroy.restype = None
        L.sp_plan_execute.argtypes = [vp, vp, sz, i32, C.POINTER(_Reply)]
        L.sp_plan_kernel_name.restype = C.c_char_p
        L.sp_plan_kernel_name.argtypes = [vp]
        L.sp_plan_force_kernel.argtypes = [vp, i32]
        L.sp_device_alloc.argtypes = [vp, sz, C.POINTER(vp)]
        L.sp_device_free.argtypes = [vp, vp]
        L.sp_device_upload.argtypes = [vp, vp, vp, sz]
        L.sp_device_download.argtypes = [vp, vp, vp, sz]
        L.sp_device_memset.argtypes = [vp, vp, C.c_int, sz]
        L.sp_synth_trinoise.argtypes = [vp, vp, i32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, dbl, dbl]
        L.sp_context_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.sp_context_enable_timing.argtypes = [vp, i32]
        L.sp_merge_replies.argtypes = [vp, vp, i32, i32, vp, vp, vp]
        L.sp_merge_replies_batch.argtypes = [vp, vp, i32, i32, i32, vp]
        L.sp_context_event_pair_overhead_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.sp_place_strips.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32]
        if not hasattr(L, "sp_group_create"):
            return          # (an older build loaded as an experiment variant, tools/ab_variants.sh: everything above is all it has)
        L.sp_group_create.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]
        L.sp_group_destroy.argtypes = [vp]
        L.sp_group_destroy.restype = None
        L.sp_group_size.argtypes = [vp]
        L.sp_group_render.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, C.POINTER(_Reply)]
        L.sp_group_transport.restype = C.c_char_p
        L.sp_group_transport.argtypes = [vp]
        L.sp_group_last_error.restype = C.c_char_p
        L.sp_group_last_error.argtypes = [vp]
        if hasattr(L, "sp_group_render_ex"):
            L.sp_group_render_ex.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, C.POINTER(_Reply), i32]
            L.sp_group_transport_note.restype = C.c_char_p
            L.sp_group_transport_note.argtypes = [vp]
            L.sp_group_last_timings.argtypes = [vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)]
            L.sp_group_root_bytes.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
            if hasattr(L, "sp_group_rccl_info"):
                L.sp_group_rccl_info.argtypes = [vp, C.c_char_p, sz]
            L.sp_render_strip.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, C.POINTER(_Reply), i32]
        if hasattr(L, "sp_context_last_upload_bytes"):
            L.sp_context_last_upload_bytes.argtypes = [vp, C.POINTER(sz)]
        L.sp_context_get_stream.argtypes = [vp, C.POINTER(vp)]
        L.sp_plan_execute_batch.argtypes = [vp, C.POINTER(_BatchItem), i32]
        L.sp_render_batch.argtypes = [vp, C.POINTER(_Request), C.POINTER(_BatchItem), i32]
        L.sp_debug_batch_plan.argtypes = [i32, i32, i32, i32, vp, vp, i32, vp, sz, C.POINTER(sz)]
        L.sp_peak_subframes.argtypes = [i32, i32, sz, i32, C.POINTER(i32), C.POINTER(i32)]
        L.sp_render_named_ex.argtypes = [vp, C.POINTER(_NamedRequest), i32, vp, sz, i32, C.POINTER(_Reply)]
        L.sp_plan_kernel_name_for.restype = C.c_char_p
        L.sp_plan_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_plan_debug_launch.argtypes = [vp, sz, i32, vp, vp, sz, C.POINTER(sz)]
        L.sp_debug_frames_launch.argtypes = [i32, i32, C.c_int64, i32, i32, vp, sz, C.POINTER(sz)]
        L.sp_plan_execute_traces.argtypes = [vp, vp, sz, i32, vp, vp]
        L.sp_render_traces.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, vp, vp]
        L.sp_plan_traces_kernel_name_for.restype = C.c_char_p
        L.sp_plan_traces_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_plan_execute_power.argtypes = [vp, vp, sz, i32, vp]
        L.sp_plan_power_to_db.argtypes = [vp, vp, sz, vp]
        L.sp_render_power.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, i32, vp]
        L.sp_plan_power_kernel_name_for.restype = C.c_char_p
        L.sp_plan_power_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_power_mean.argtypes = [vp, vp, i32, i32, vp]
        L.sp_plan_execute_mean.argtypes = [vp, vp, sz, i32, vp]
        L.sp_render_mean.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, i32, vp]
        L.sp_context_set_mean_window.argtypes = [vp, sz]
        L.sp_debug_exact_sum.argtypes = [vp, sz, C.POINTER(dbl)]
        L.sp_plan_mean_kernel_name_for.restype = C.c_char_p
        L.sp_plan_mean_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_power_variance.argtypes = [vp, vp, i32, i32, vp]
        L.sp_plan_execute_variance.argtypes = [vp, vp, sz, i32, vp]
        L.sp_render_variance.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, vp]
        L.sp_debug_variance_sums.argtypes = [vp, sz, vp]
        L.sp_debug_variance_launch.argtypes = [i32, C.c_int64, i32, vp, sz, C.POINTER(sz)]
        L.sp_plan_variance_kernel_name_for.restype = C.c_char_p
        L.sp_plan_variance_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_series_lagcov.argtypes = [vp, vp, i32, i32, vp, i32, i32, vp]
        L.sp_power_lagcov.argtypes = [vp, vp, i32, i32, vp, i32, vp, i32, i32, vp]
        L.sp_plan_execute_lagcov.argtypes = [vp, vp, sz, i32, vp, i32, vp, i32, i32, vp]
        L.sp_render_lagcov.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, vp, i32, vp, i32, i32, vp]
        L.sp_plan_lagcov_kernel_name_for.restype = C.c_char_p
        L.sp_plan_lagcov_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_debug_lagcov.argtypes = [vp, vp, i32, i32, vp]
        L.sp_debug_lagcov_launch.argtypes = [i32, i32, C.c_int64, i32, vp, sz, C.POINTER(sz)]
        L.sp_band_rows.argtypes = [i32, dbl, dbl, C.POINTER(i32), C.POINTER(i32)]
        L.sp_power_bands.argtypes = [vp, vp, i32, i32, vp, i32, vp]
        L.sp_plan_execute_bandpower.argtypes = [vp, vp, sz, i32, vp, i32, vp]
        L.sp_render_bandpower.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, vp, i32, i32, vp]
        L.sp_plan_bandpower_kernel_name_for.restype = C.c_char_p
        L.sp_plan_bandpower_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_power_moments.argtypes = [vp, vp, i32, i32, vp, i32, i32, vp]
        L.sp_plan_execute_moments.argtypes = [vp, vp, sz, i32, vp, i32, i32, vp]
        L.sp_render_moments.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, vp, i32, i32, i32, vp]
        L.sp_debug_moment_sum.argtypes = [vp, sz, i32, vp]
        L.sp_plan_moments_kernel_name_for.restype = C.c_char_p
        L.sp_plan_moments_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_power_tracks.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
        L.sp_plan_execute_track.argtypes = [vp, vp, sz, i32, vp, i32, vp, vp]
        L.sp_render_track.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, vp, i32, i32, vp, vp]
        L.sp_plan_track_kernel_name_for.restype = C.c_char_p
        L.sp_plan_track_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_debug_band_peak.argtypes = [vp, i32, i32, i32, C.POINTER(i32), C.POINTER(dbl)]
        L.sp_power_occupancy.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp]
        L.sp_plan_execute_occupancy.argtypes = [vp, vp, sz, i32, vp, vp, i32, vp, vp]
        L.sp_render_occupancy.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, vp, vp, i32, vp, vp]
        L.sp_plan_occupancy_kernel_name_for.restype = C.c_char_p
        L.sp_plan_occupancy_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_debug_occupancy.argtypes = [vp, vp, i32, i32, i32, C.POINTER(C.c_uint32)]
        L.sp_power_quantile.argtypes = [vp, vp, i32, i32, vp, i32, vp]
        L.sp_plan_execute_quantile.argtypes = [vp, vp, sz, i32, vp, i32, vp]
        L.sp_render_quantile.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, i32, vp, i32, vp]
        L.sp_plan_quantile_kernel_name_for.restype = C.c_char_p
        L.sp_plan_quantile_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_quantile_rank.restype = i32
        L.sp_quantile_rank.argtypes = [i32, dbl]
        L.sp_debug_quantile.argtypes = [vp, i32, i32, C.POINTER(dbl)]
        L.sp_plan_execute_bursts.argtypes = [vp, vp, sz, i32, vp, i32, vp, vp, i32, vp, vp]
        L.sp_power_bursts.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, i32, vp, vp]
        L.sp_series_bursts.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp]
        L.sp_render_bursts.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, vp, i32, vp, vp, i32, vp, vp]
        L.sp_plan_bursts_kernel_name_for.restype = C.c_char_p
        L.sp_plan_bursts_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_debug_bursts.argtypes = [vp, i32, dbl, dbl, i32, C.POINTER(C.c_uint32), vp]
        L.sp_plan_execute_pulses.argtypes = [vp, vp, sz, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]
        L.sp_power_pulses.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]
        L.sp_series_pulses.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]
        L.sp_render_pulses.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]
        L.sp_plan_pulses_kernel_name_for.restype = C.c_char_p
        L.sp_plan_pulses_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_debug_pulses.argtypes = [vp, i32, dbl, dbl, i32, C.POINTER(C.c_uint32), vp, vp, vp, vp]
        L.sp_plan_execute_index.argtypes = [vp, vp, sz, i32, C.POINTER(_Reply), vp]
        L.sp_render_index.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, C.POINTER(_Reply), vp]
        L.sp_index_to_rgba.argtypes = [vp, vp, sz, vp, i32, vp]
        L.sp_plan_index_kernel_name_for.restype = C.c_char_p
        L.sp_plan_index_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_plan_debug_index_launch.argtypes = [vp, sz, i32, vp, vp, sz, C.POINTER(sz)]
        L.sp_density_from_index.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32]
        L.sp_plan_execute_density.argtypes = [vp, vp, sz, i32, vp, i32]
        L.sp_render_density.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, vp]
        L.sp_debug_density_launch.argtypes = [i32, i32, i32, i32, i32, vp, sz, C.POINTER(sz)]
        L.sp_debug_scratch_launch.argtypes = [i32, i32, i32, i32, vp, sz, C.POINTER(sz)]
        L.sp_context_debug_set_cu_count.argtypes = [vp, i32]
        L.sp_debug_mean_launch.argtypes = [i32, C.c_int64, i32, vp, sz, C.POINTER(sz)]
        L.sp_blockmean_columns.restype = i32
        L.sp_blockmean_columns.argtypes = [i32, i32]
        L.sp_power_blockmean.argtypes = [vp, vp, i32, i32, i32, vp]
        L.sp_plan_execute_blockmean.argtypes = [vp, vp, sz, i32, i32, vp]
        L.sp_render_blockmean.argtypes = [vp, C.POINTER(_Request), vp, sz, i32, i32, i32, vp]
        L.sp_plan_blockmean_kernel_name_for.restype = C.c_char_p
        L.sp_plan_blockmean_kernel_name_for.argtypes = [vp, sz, i32]
        L.sp_context_set_blockmean_direct_max.argtypes = [vp, i32]
        L.sp_debug_blockmean.argtypes = [vp, i32, i32, i32, vp]
        L.sp_debug_blockmean_split.argtypes = [C.c_int64, C.c_int64, i32, i32, i32, vp, sz, C.POINTER(sz)]
        L.sp_plan_power_to_index.argtypes = [vp, vp, i32, vp]
        L.sp_debug_blockmean_launch.argtypes = [i32, C.c_int64, i32, i32, vp, sz, C.POINTER(sz)]
        L.sp_debug_gray_index.argtypes = [dbl, dbl, dbl, i32, vp, sz, vp]

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = Library()
        return cls._instance

    def check(self, status, ctx=None):
        if status == 0:
            return
        msg = self.L.sp_last_error(ctx).decode() if ctx else ""
        raise SpectroplotError(status, msg or self.L.sp_status_string(status).decode())

    def device_count(self):
        n = C.c_int32(0)
        self.L.sp_device_count(C.byref(n))
        return n.value

    def debug_density_launch(self, n, width, waterfall=False, x_begin=0, x_end=None):
        """The counting kernel's decomposition for the frames [x_begin, x_end) of an index image of n rows and `width` frames
        (sp_debug_density_launch; no device needed): a dict of DENSITY_LAUNCH_FIELDS plus "rects", an int64 array of one
        (first row, end row, first frame, end frame) per workgroup."""
        x_end = int(width) if x_end is None else int(x_end)
        used = C.c_size_t()
        self.L.sp_debug_density_launch(int(n), int(width), int(bool(waterfall)), int(x_begin), x_end, None, 0, C.byref(used))
        out = np.zeros(max(used.value, 1), np.int64)
        self.check(self.L.sp_debug_density_launch(int(n), int(width), int(bool(waterfall)), int(x_begin), x_end,
                                                  out.ctypes.data_as(C.c_void_p), len(out), C.byref(used)))
        d = dict(zip(DENSITY_LAUNCH_FIELDS, (int(v) for v in out[:6])))
        d["rects"] = out[6:used.value].reshape(-1, 4)
        return d


def exact_sum(values):
    """sp_debug_exact_sum: the correctly rounded sum of non-negative doubles (math.fsum's) through the host side of the code the mean
    kernels run; any NaN gives NaN, else any +inf gives +inf, a sum that rounds past DBL_MAX gives +inf.  No device needed."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    out = C.c_double()
    lib = Library.get()
    lib.check(lib.L.sp_debug_exact_sum(v.ctypes.data_as(C.c_void_p) if v.size else None, v.size, C.byref(out)))
    return out.value


def variance_sums(values):
    """sp_debug_variance_sums: f64 [3] of one row of non-negative doubles over W = len(values) frames, through the host side of the code
    the variance kernels run: the correctly rounded sum, the correctly rounded sum of the exact squares, and the correctly rounded
    W * sum of squares - sum**2 (W**2 times the population variance; +0.0 exactly for a constant row, never negative).  Any NaN gives
    NaN in all three, else any +inf gives +inf in all three; a result that rounds past DBL_MAX gives +inf.  No device needed."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    out = np.zeros(3, np.float64)
    lib = Library.get()
    lib.check(lib.L.sp_debug_variance_sums(v.ctypes.data_as(C.c_void_p) if v.size else None, v.size, out.ctypes.data_as(C.c_void_p)))
    return out


def variance_of(sums, width, ddof=0):
    """The variance of every row from a variance reply `sums` ([3, n]) over `width` frames: sums[2] / (width * (width - ddof)), the
    population variance with ddof=0 and the sample variance with ddof=1.  The subtraction was done exactly on the device: this form
    contains no cancellation.  NaN by 0 / 0 where width * (width - ddof) is 0.  Plain numpy, no device needed."""
    sums = np.asarray(sums, np.float64)
    with np.errstate(all="ignore"):
        return sums[2] / np.float64(int(width) * (int(width) - int(ddof)))


def spectral_kurtosis(sums, width):
    """The spectral kurtosis of every row from a variance reply `sums` ([3, n]) over `width` frames:
    (width + 1) / (width - 1) * sums[2] / sums[0]**2 - about 1 for Gaussian noise, below 1 (0 exactly for a constant row) for a steady
    carrier, above 1 for bursts.  No cancellation.  NaN where a row holds no power or width is 0; width 1 divides by zero.  Plain
    numpy, no device needed."""
    sums = np.asarray(sums, np.float64)
    w = np.float64(int(width))
    with np.errstate(all="ignore"):
        return (w + 1.0) / (w - 1.0) * sums[2] / (sums[0] * sums[0])


SP_MAX_LAG_PAIRS = 16
SP_MAX_LAGS = 1024


def lagcov_terms(width, lags):
    """The terms N every lag of a lagged-covariance request over `width` frames and `lags` lags has: width - lags + 1, 0 where that is
    below 1 (the fixed window: every lag sees equally many frames).  Pure host arithmetic."""
    return max(int(width) - int(lags) + 1, 0)


def lagcov_sums(a, b, lags):
    """sp_debug_lagcov: f64 [3, lags] of two series of non-negative doubles, equally long, through the host side of the code the
    lagged-covariance kernels run.  With N = lagcov_terms(len(a), lags) and per lag l: the correctly rounded sum of a[x] * b[x + l] over
    x < N; the correctly rounded N * that sum - sum(a[:N]) * sum(b[l:l + N]), SIGNED, the subtraction done exactly (N**2 times the
    covariance at lag l; +0.0 exactly for a constant series); and the correctly rounded sum(b[l:l + N]).  A NaN in either window gives
    NaN in all three of that lag, else a +inf gives +inf.  No device needed."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    if a.size != b.size:
        raise SpectroplotError(SP_ERR_INVALID_ARG, "lagcov_sums: a and b must be equally long")
    out = np.zeros((3, max(int(lags), 0)), np.float64)
    lib = Library.get()
    lib.check(lib.L.sp_debug_lagcov(_p(a) if a.size else None, _p(b) if b.size else None, a.size, int(lags), _p(out) if out.size else None))
    return out


def lag_correlation(cov_ab, cov_aa0, cov_bb0):
    """The usual correlation coefficient per lag from lagged-covariance replies: cov_ab / sqrt(cov_aa0 * cov_bb0), where cov_ab is
    out[1] of the pair (a, b) over the lags and cov_aa0, cov_bb0 are out[1] at lag 0 of the auto pairs (a, a) and (b, b) of the same
    request (the common factor N**2 cancels).  THE NORMALISATION IS BY THE LAG-0 AUTOCOVARIANCES, the variances of a[0 .. N) and
    b[0 .. N); it is NOT the per-window one, which would take the variance of b[l .. l + N) for every lag, so a value may pass 1 in
    magnitude where b's later frames vary more than its first N.  Where a variance is 0 the division is by zero: NaN for a covariance
    of 0, an infinity otherwise.  Plain numpy, no device needed."""
    with np.errstate(all="ignore"):
        return np.asarray(cov_ab, np.float64) / np.sqrt(np.float64(cov_aa0) * np.float64(cov_bb0))


def blockmean_columns(width, group):
    """sp_blockmean_columns: the columns of an averaged spectrogram of `width` frames, `group` frames per column: ceil(width / group),
    0 where width <= 0 or group < 1.  Pure host arithmetic."""
    return int(Library.get().L.sp_blockmean_columns(int(width), int(group)))


def blockmean(values, group):
    """sp_debug_blockmean: the block means of a frame-major plane f64 [width, n] through the host side of the code the kernels run:
    f64 [columns, n], per column of `group` frames and per row the correctly rounded sum divided by the column's frames, with the mean's
    NaN and inf rule.  No device needed."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    width, n = v.shape
    out = np.empty((blockmean_columns(width, group), n), np.float64)
    lib = Library.get()
    lib.check(lib.L.sp_debug_blockmean(v.ctypes.data_as(C.c_void_p) if v.size else None, int(n), int(width), int(group),
                                       out.ctypes.data_as(C.c_void_p) if out.size else None))
    return out


BLOCKMEAN_SPLIT_FIELDS = ("head", "body", "tail", "body_column", "body_columns", "direct")


def blockmean_split(x_base, frames, width, group, direct_max=0):
    """sp_debug_blockmean_split: what becomes of the run [x_base, x_base + frames) of a block-mean request of `width` frames: a dict of
    BLOCKMEAN_SPLIT_FIELDS - the frames of the head (continues an open column), of the body (whole columns) and of the tail (opens a
    column), the body's first column and its columns, and whether the body takes the direct kernel (direct_max 0: the built default).
    No device needed."""
    out = np.zeros(len(BLOCKMEAN_SPLIT_FIELDS), np.int64)
    used = C.c_size_t()
    lib = Library.get()
    lib.check(lib.L.sp_debug_blockmean_split(int(x_base), int(frames), int(width), int(group), int(direct_max),
                                             out.ctypes.data_as(C.c_void_p), len(out), C.byref(used)))
    return dict(zip(BLOCKMEAN_SPLIT_FIELDS, (int(x) for x in out)))


def debug_blockmean_launch(n, frames, group, cu_count):
    """The grid of the direct block-mean kernel alone (sp_debug_blockmean_launch): (bands of 64 rows, pieces of the columns, columns per
    piece)."""
    lib = Library.get()
    out = np.zeros(3, np.int64)
    used = C.c_size_t()
    lib.check(lib.L.sp_debug_blockmean_launch(int(n), int(frames), int(group), int(cu_count), out.ctypes.data_as(C.c_void_p), 3, C.byref(used)))
    return tuple(int(v) for v in out)


def gray_index(block_norm, gain, rng, lut_len, values):
    """sp_debug_gray_index: the colour index Plan.power_to_index gives each of `values` under a plan of these parameters, u8 of the
    values' shape, through the host side of the code the kernel runs.  No device needed."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    out = np.empty(v.shape, np.uint8)
    lib = Library.get()
    lib.check(lib.L.sp_debug_gray_index(float(block_norm), float(gain), float(rng), int(lut_len),
                                        v.ctypes.data_as(C.c_void_p) if v.size else None, v.size,
                                        out.ctypes.data_as(C.c_void_p) if v.size else None))
    return out


SP_MAX_BANDS = 64


def band_rows(n, f_lo, f_hi):
    """sp_band_rows: the image rows (y0, y1) - a half-open range - whose centre frequency f(y) = (n/2 - y) / n lies in [f_lo, f_hi],
    in cycles per sample (row 0 is +1/2, row n/2 is DC).  For I/Q plans; pure host arithmetic, no device needed."""
    y0, y1 = C.c_int32(), C.c_int32()
    lib = Library.get()
    lib.check(lib.L.sp_band_rows(int(n), float(f_lo), float(f_hi), C.byref(y0), C.byref(y1)))
    return y0.value, y1.value


def moment_sum(values, order=2):
    """sp_debug_moment_sum: f64 [order + 1], out[k] = the correctly rounded sum of r**k * values[r] over one column of non-negative
    doubles with the weights r = 0 .. len - 1 (0**0 = 1), through the host side of the code the moment kernel runs; any NaN gives NaN
    in every moment, else any +inf gives +inf in every moment, a sum that rounds past DBL_MAX gives +inf.  No device needed."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    out = np.zeros(max(int(order), 0) + 1, np.float64)
    lib = Library.get()
    lib.check(lib.L.sp_debug_moment_sum(v.ctypes.data_as(C.c_void_p) if v.size else None, v.size, int(order), out.ctypes.data_as(C.c_void_p)))
    return out


def centroid_freq(n, bands, m0, m1):
    """The centroid frequency of every band and frame in cycles per sample, f64 [count, width], from the moments m0 and m1
    ([count, width] each) of the bands (y0, y1) of an I/Q plan of n rows: (n/2 - y0 - m1 / m0) / n, row y being centred on
    (n/2 - y) / n.  NaN where a band holds no power (0 / 0) or a special value.  Plain numpy, no device needed."""
    b, count = _band_array(bands)
    m0, m1 = np.asarray(m0, np.float64).reshape(count, -1), np.asarray(m1, np.float64).reshape(count, -1)
    with np.errstate(all="ignore"):
        return (float(n // 2) - b[:, :1].astype(np.float64) - m1 / m0) / float(n)


def band_peak(values, y0, y1):
    """sp_debug_band_peak: (row, peak) of the rows [y0, y1) of one frame's values - the strongest row that is not a NaN, the smallest
    among equal ones, and its value bit for bit; (-1, nan) for an empty or all-NaN band - through the host side of the code the track
    kernel runs.  No device needed."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    row, peak = C.c_int32(), C.c_double()
    lib = Library.get()
    lib.check(lib.L.sp_debug_band_peak(v.ctypes.data_as(C.c_void_p) if v.size else None, v.size, int(y0), int(y1), C.byref(row),
                                       C.byref(peak)))
    return row.value, peak.value


def occupancy_count(values, thresholds, y0, y1):
    """sp_debug_occupancy: the number of rows y in [y0, y1) of one frame's values with values[y] >= thresholds[y] (numpy's >=: a NaN
    on either side is no hit; the values are not negative) through the host side of the code the occupancy kernel runs.  No device
    needed."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    t = np.ascontiguousarray(thresholds, dtype=np.float64)
    if t.shape != v.shape:
        raise ValueError("occupancy_count: one threshold per value")
    count = C.c_uint32()
    lib = Library.get()
    lib.check(lib.L.sp_debug_occupancy(v.ctypes.data_as(C.c_void_p) if v.size else None, t.ctypes.data_as(C.c_void_p) if t.size else None,
                                       v.size, int(y0), int(y1), C.byref(count)))
    return count.value


def _threshold_array(threshold, n):
    """f64[n] of a scalar (every row's threshold) or of n values; another length is refused here: the library cannot see it."""
    t = np.asarray(threshold, dtype=np.float64)
    if t.ndim == 0:
        return np.full(int(n), float(t), np.float64)
    t = np.ascontiguousarray(t.reshape(-1))
    if t.size != int(n):
        raise ValueError("threshold must be a number or %d values, one per image row" % int(n))
    return t


SP_MAX_RANKS = 16
SP_QUANTILE_LDS_VALUES = 16384


def quantile_rank(width, q):
    """sp_quantile_rank: the rank of quantile q of `width` values, floor(q * (width - 1)) - numpy's method='lower', the lower median of
    an even width - or -1 for width < 1 or a q outside [0, 1] (a NaN included).  The one place a q becomes a rank; no device needed."""
    return int(Library.get().L.sp_quantile_rank(int(width), float(q)))


def quantile_select(values, rank):
    """sp_debug_quantile: element `rank` of the values sorted ascending - every NaN behind +inf, the reply the value without its sign
    bit or the one NaN - through the host side of the code the percentile kernel runs.  No device needed."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    out = C.c_double()
    lib = Library.get()
    lib.check(lib.L.sp_debug_quantile(v.ctypes.data_as(C.c_void_p) if v.size else None, v.size, int(rank), C.byref(out)))
    return out.value


def _rank_array(width, q, ranks):
    """(int32 [count] host array, count): `ranks` as given - nothing is refused here, the library refuses - or, where ranks is None,
    the ranks of the quantiles q (a number or a sequence) through quantile_rank; a q without a rank is refused here."""
    if ranks is None:
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64)).reshape(-1)
        ranks = [quantile_rank(width, v) for v in qs] if int(width) > 0 else [0] * qs.size
        if any(k < 0 for k in ranks):
            raise SpectroplotError(SP_ERR_INVALID_ARG, "a quantile must lie in [0, 1]")
    # (a rank that is no int32 becomes one the library refuses - -1, or 2^31 - 1, which no width is above - and never wraps into range)
    r = np.ascontiguousarray(np.clip(np.asarray(ranks, dtype=np.int64).reshape(-1), -1, 2 ** 31 - 1).astype(np.int32))
    return r, r.size


SP_BURST_SEGMENT_FRAMES = 2048


def burst_scan(values, hi, lo, max_bursts):
    """sp_debug_bursts: the bursts of one series through the host side of the code the burst kernels run - a Schmitt trigger that
    starts OFF, sets where values[x] >= hi, resets where values[x] < lo (numpy's compares: a NaN does neither) - as (the total,
    edges int32 [max_bursts, 2]): start and end of the first max_bursts bursts, -1 behind them; a burst open at the end ends at
    len(values).  No device needed."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    m = int(max_bursts)
    edges = np.zeros((max(m, 0), 2), np.int32)
    total = C.c_uint32()
    lib = Library.get()
    lib.check(lib.L.sp_debug_bursts(_p(v) if v.size else None, v.size, float(hi), float(lo), m, C.byref(total),
                                    _p(edges) if edges.size else None))
    return total.value, edges


def pulse_scan(values, hi, lo, max_bursts):
    """sp_debug_pulses: the bursts of one series as burst_scan() gives them and their measurements, through the host side of the code
    the kernels run: (the total, edges int32 [max_bursts, 2], energy float64 [max_bursts], peak float64 [max_bursts], peak_at int32
    [max_bursts]).  energy is math.fsum of the burst's frames (any NaN frame: NaN; otherwise any +inf: +inf), peak the largest frame
    that is no NaN and peak_at the earliest frame that holds it; behind the listed bursts -1 and the all-ones NaN.  No device needed."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    m = int(max_bursts)
    edges = np.zeros((max(m, 0), 2), np.int32)
    energy, peak = np.zeros(max(m, 0), np.float64), np.zeros(max(m, 0), np.float64)
    peak_at = np.zeros(max(m, 0), np.int32)
    total = C.c_uint32()
    lib = Library.get()
    some = edges.size > 0
    lib.check(lib.L.sp_debug_pulses(_p(v) if v.size else None, v.size, float(hi), float(lo), m, C.byref(total), _p(edges) if some else None,
                                    _p(energy) if some else None, _p(peak) if some else None, _p(peak_at) if some else None))
    return total.value, edges, energy, peak, peak_at


def burst_pulses(edges_row, total):
    """What a pulse analyser prints of one band's burst list (edges int32 [max_bursts, 2] or flat, and the band's total count): (the
    widths end - start of the listed bursts, the gaps start[i + 1] - end[i] between them), two int64 arrays in frames, the second one
    shorter by one.  Only min(total, max_bursts) bursts are listed."""
    e = np.asarray(edges_row, dtype=np.int64).reshape(-1, 2)
    e = e[:min(int(total), e.shape[0])]
    return e[:, 1] - e[:, 0], e[1:, 0] - e[:-1, 1]


def _burst_thresholds(hi, lo, count):
    """(hi, lo) as two float64 [count] host arrays: a number for every band, or count values; nothing else is checked here."""
    out = []
    for name, t in (("hi", hi), ("lo", lo)):
        a = np.asarray(t, dtype=np.float64)
        a = np.full(count, float(a), np.float64) if a.ndim == 0 else np.ascontiguousarray(a.reshape(-1))
        if a.size != count:
            raise SpectroplotError(SP_ERR_INVALID_ARG, "%s must be a number or one value per band" % name)
        out.append(a)
    return out


def row_freq(n, row):
    """The centre frequency of image row `row` of an n-point spectrum in cycles per sample, (n/2 - row) / n: row 0 is +1/2, row n/2 is
    DC; NaN for row -1, a track's "no value".  The inverse of band_rows for a single row, and like it for I/Q plans (in channel mode
    the rows are the L/R split's, not one frequency axis).  Pure Python."""
    return math.nan if row < 0 else (n // 2 - row) / n


def _pair_array(pairs):
    """(int32 [npairs, 2] host array, npairs) of a sequence of (ia, ib) band indices; nothing is checked here - the library refuses."""
    p = np.ascontiguousarray(np.clip(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), -1, 2 ** 31 - 1).astype(np.int32))
    return p, p.shape[0]


def _band_array(bands):
    """(int32 [count, 2] host array, count) of a sequence of (y0, y1) rows ranges; nothing is checked here - the library refuses."""
    b = np.ascontiguousarray(np.asarray(bands, dtype=np.int64).reshape(-1, 2).astype(np.int32))
    return b, b.shape[0]


def parse_format(name):
    """(format id, bytes per complex sample) for a reference format name (lib/samples.js:22-162)."""
    f, w = C.c_int32(), C.c_int32()
    Library.get().L.sp_format_parse(str(name).encode(), C.byref(f), C.byref(w))
    return f.value, w.value


def slice_bounds(nbytes, sample_width, index, count):
    b, e = C.c_size_t(), C.c_size_t()
    lib = Library.get()
    lib.check(lib.L.sp_slice_bounds(nbytes, sample_width, index, count, C.byref(b), C.byref(e)))
    return b.value, e.value


def window(name, n):
    lib = Library.get()
    out = np.empty(n, dtype=np.float64)
    w = C.c_double()
    lib.check(lib.L.sp_window(name.encode(), n, out.ctypes.data_as(C.c_void_p), C.byref(w)))
    return out, w.value


def twiddles(n):
    lib = Library.get()
    c = np.empty(max(n // 2, 1), dtype=np.float64)
    s = np.empty(max(n // 2, 1), dtype=np.float64)
    lib.check(lib.L.sp_twiddles(n, c.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)))
    return c[:n // 2], s[:n // 2]


def debug_batch_plan(fmt, n, lut_len, cu_count, nbytes, widths):
    """The work list of a batch (sp_debug_batch_plan): (frames per group, (grid0, grid1), (groups0, groups1), per-item rows of
    (launch, first group, group count)).  Launch: 0 prefetching loader, 1 generic loaders, 2 one by one, 3 nothing to render."""
    lib = Library.get()
    fid = parse_format(fmt)[0] if isinstance(fmt, str) else int(fmt)
    nb = np.ascontiguousarray(nbytes, dtype=np.uint64)
    wd = np.ascontiguousarray(widths, dtype=np.int32)
    cap = 5 + 3 * len(wd)
    out = np.zeros(cap, np.int64)
    used = C.c_size_t()
    lib.check(lib.L.sp_debug_batch_plan(fid, int(n), int(lut_len), int(cu_count), nb.ctypes.data_as(C.c_void_p),
                                        wd.ctypes.data_as(C.c_void_p), len(wd), out.ctypes.data_as(C.c_void_p), cap, C.byref(used)))
    return int(out[0]), (int(out[1]), int(out[2])), (int(out[3]), int(out[4])), out[5:used.value].reshape(-1, 3)


def debug_frames_launch(n, lut_len, count, cu_count, gf_fixed=0):
    """The frame-loop kernels' launch rule alone (sp_debug_frames_launch): (frames per group, groups, workgroups, LDS bytes) for `count`
    frames, or for `count` groups of gf_fixed frames; None where the rule refuses the shape."""
    lib = Library.get()
    out = np.zeros(4, np.int64)
    used = C.c_size_t()
    rc = lib.L.sp_debug_frames_launch(int(n), int(lut_len), int(count), int(cu_count), int(gf_fixed), out.ctypes.data_as(C.c_void_p), 4,
                                      C.byref(used))
    if rc == SP_ERR_UNSUPPORTED:
        return None
    lib.check(rc)
    return tuple(int(v) for v in out)


def debug_scratch_launch(n, slabs, frames, cu_count):
    """The scratch kernels' launch shape alone (sp_debug_scratch_launch): (workgroups, whether the kernel is the four-stage variant)
    of one launch over `frames` frames whose workgroups own `slabs` slabs of n doubles each."""
    lib = Library.get()
    out = np.zeros(2, np.int64)
    used = C.c_size_t()
    lib.check(lib.L.sp_debug_scratch_launch(int(n), int(slabs), int(frames), int(cu_count), out.ctypes.data_as(C.c_void_p), 2, C.byref(used)))
    return int(out[0]), bool(out[1])


def debug_mean_launch(n, frames, cu_count):
    """The grid of a mean's accumulation alone (sp_debug_mean_launch): (bands of 64 rows, pieces of the frames, frames per piece)."""
    lib = Library.get()
    out = np.zeros(3, np.int64)
    used = C.c_size_t()
    lib.check(lib.L.sp_debug_mean_launch(int(n), int(frames), int(cu_count), out.ctypes.data_as(C.c_void_p), 3, C.byref(used)))
    return tuple(int(v) for v in out)


def debug_variance_launch(n, frames, cu_count):
    """The grid of a variance request's accumulation alone (sp_debug_variance_launch): (bands of 32 rows, pieces of the frames, frames
    per piece)."""
    lib = Library.get()
    out = np.zeros(3, np.int64)
    used = C.c_size_t()
    lib.check(lib.L.sp_debug_variance_launch(int(n), int(frames), int(cu_count), out.ctypes.data_as(C.c_void_p), 3, C.byref(used)))
    return tuple(int(v) for v in out)


def debug_lagcov_launch(npairs, lags, terms, cu_count):
    """The grid of a lagged-covariance request's accumulation alone (sp_debug_lagcov_launch): (pairs times bands of 32 lags, pieces of
    the terms, terms per piece)."""
    lib = Library.get()
    out = np.zeros(3, np.int64)
    used = C.c_size_t()
    lib.check(lib.L.sp_debug_lagcov_launch(int(npairs), int(lags), int(terms), int(cu_count), out.ctypes.data_as(C.c_void_p), 3,
                                           C.byref(used)))
    return tuple(int(v) for v in out)


DENSITY_LAUNCH_FIELDS = ("workgroups", "rows", "frames", "lds_bytes", "bands", "pieces")
LAUNCH_FIELDS = ("kernel", "log2n", "channel_mode", "prefetch", "gf", "groups", "grid", "lds_bytes", "rgba_fast", "peak_m", "cu_count")
KERNELS = {0: "none", 1: "scratch_radix2", 3: "frames", 4: "frames_peak"}      # enum Kernel (sp_api.hip)


def peak_subframes(fmt, n, nbytes, width):
    """The peak detector's sub-frame rule for a request of this shape (sp_peak_subframes): (M sub-frames per column, how many of them
    the last column has).  M == 1: the request is the sample detector's."""
    lib = Library.get()
    fid = parse_format(fmt)[0] if isinstance(fmt, str) else int(fmt)
    m, last = C.c_int32(), C.c_int32()
    lib.check(lib.L.sp_peak_subframes(fid, int(n), int(nbytes), int(width), C.byref(m), C.byref(last)))
    return m.value, last.value


def named_resolve(window, cmap):
    """(taper name as sp_window takes it, colour-map key, entry count) for two option names, defaults included
    (lib/spectroplot.js:238-264, lib/utils.js:25-40)."""
    w, k, n = C.c_char_p(), C.c_char_p(), C.c_int32()
    lib = Library.get()
    lib.check(lib.L.sp_named_resolve(str(window).encode(), str(cmap).encode(), C.byref(w), C.byref(k), C.byref(n)))
    return w.value.decode(), k.value.decode(), n.value


def _make_request(fmt_id, n, windowc, block_norm, gain, rng, lut, channel_mode, waterfall, detector="sample"):
    windowc = np.ascontiguousarray(windowc, dtype=np.float64)
    lut = np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1, 3)
    req = _Request(fmt_id, int(n), int(bool(channel_mode)), int(bool(waterfall)), len(lut), detector_id(detector), float(block_norm), float(gain),
                   float(rng), windowc.ctypes.data_as(C.c_void_p), lut.ctypes.data_as(C.c_void_p))
    return req, (windowc, lut)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_reply(width, n, lut_len, image="rgba", px=4, fill=None):
    """The reply of a host-fed request in numpy arrays: (dict with the picture under `image` at px bytes per pixel, the dBfs
    [min, max] array, the _Reply over both - an "index" picture is not part of it).  fill: a byte every output holds before the call."""
    W, f = max(int(width), 0), 0 if fill is None else int(fill)
    out = {image: np.full(px * W * n, f, np.uint8), "gauge_mins": np.full(W, f, np.uint8), "gauge_maxs": np.full(W, f, np.uint8),
           "gauge_amps": np.full(W, f, np.uint8), "c_hist": np.full(lut_len, f, np.uint64), "cB_hist": np.full(SP_CB_HIST_SIZE, f, np.uint64)}
    mm = np.array([0.0, -200.0]) if fill is None else np.array([float(f), float(f)])
    rep = _Reply(_p(out[image]) if image == "rgba" else None, _p(out["gauge_mins"]), _p(out["gauge_maxs"]), _p(out["gauge_amps"]),
                 _p(out["c_hist"]), _p(out["cB_hist"]), _p(mm))
    return out, mm, rep


def _device_reply(rgba=0, gauge_mins=0, gauge_maxs=0, gauge_amps=0, c_hist=0, cb_hist=0, dbfs_minmax=0):
    """The _Reply of device addresses (ints); 0 or None skips that output."""
    return _Reply(*[a or None for a in (rgba, gauge_mins, gauge_maxs, gauge_amps, c_hist, cb_hist, dbfs_minmax)])


def _no_picture_lut(lut):
    """The colour map of a request that renders no picture: the caller's, or two grey entries (it only takes part in the plan-cache key)."""
    return np.array([[0, 0, 0], [255, 255, 255]], np.uint8) if lut is None else lut


def _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode):
    """How a host-fed request that renders no picture begins: (the capture as contiguous bytes, the request, the arrays it points into)."""
    fid, _ = parse_format(fmt)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    req, keep = _make_request(fid, n, windowc, block_norm, gain, rng, _no_picture_lut(lut), channel_mode, False)
    return data, req, keep


def _filled(shape, dtype, fill, bytewise=True):
    """An output array of zeros, or one that holds `fill` before the call (tests): in every byte, or as every element's value."""
    out = np.zeros(shape, dtype)
    if fill is not None:
        (out.view(np.uint8) if bytewise else out)[...] = fill
    return out


def _launch_dict(words):
    """sp_plan_debug_launch's words as a dict of LAUNCH_FIELDS, "kernel" as a name (5: k_frames_index)."""
    d = dict(zip(LAUNCH_FIELDS, (int(v) for v in words)))
    d["kernel"] = "frames_index" if d["kernel"] == 5 else KERNELS[d["kernel"]]
    return d


class Context:
    """One device + stream; the analogue of one reference Worker instance."""

    def __init__(self, device=0):
        self.lib = Library.get()
        h = C.c_void_p()
        self.lib.check(self.lib.L.sp_context_create(device, C.byref(h)))
        self.h = h
        self.device = device
        self._plans = weakref.WeakSet()   # live Plan objects of this context

    def close(self):
        if self.h:
            # plans hold a pointer to their context: they go first (a Plan object that outlives this call is inert)
            for p in list(self._plans):
                p.close()
            self.lib.L.sp_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, status):
        self.lib.check(status, self.h)

    def set_stream(self, stream_handle):
        self._chk(self.lib.L.sp_context_set_stream(self.h, C.c_void_p(stream_handle)))

    def get_stream(self):
        """The stream handle bound with set_stream (0 while the context uses its own): what set_stream takes to restore it."""
        s = C.c_void_p()
        self._chk(self.lib.L.sp_context_get_stream(self.h, C.byref(s)))
        return s.value or 0

    def synchronize(self):
        self._chk(self.lib.L.sp_context_synchronize(self.h))

    def last_upload_bytes(self):
        """Bytes of samples the last render() sent over the host link (a sparse request - stride > n - sends its frames only)."""
        v = C.c_size_t()
        self._chk(self.lib.L.sp_context_last_upload_bytes(self.h, C.byref(v)))
        return v.value

    def last_chunks(self):
        """In how many chunks of frames the last host-fed request was carried out (sp_context_last_chunks)."""
        v = C.c_int32()
        self._chk(self.lib.L.sp_context_last_chunks(self.h, C.byref(v)))
        return v.value

    def enable_timing(self, on=True):
        self._chk(self.lib.L.sp_context_enable_timing(self.h, int(on)))

    def merge_replies(self, d_records, count, lut_len, d_c_hist=0, d_cb_hist=0, d_minmax=0):
        """Device-side merge of `count` slice records [c_hist | cB_hist | dBfs_min, dBfs_max] (the caller's merge, spectroplot.js:1229-1238)."""
        self._chk(self.lib.L.sp_merge_replies(self.h, C.c_void_p(d_records), int(count), int(lut_len), C.c_void_p(d_c_hist or None),
                                              C.c_void_p(d_cb_hist or None), C.c_void_p(d_minmax or None)))

    def merge_replies_batch(self, d_gathered, ranks, renders, lut_len, d_merged):
        """The same merge for a batch of renders in ONE launch: d_gathered = [rank][render][record] as an all-gather of the ranks' batches
        delivers it, d_merged = `renders` merged records end to end (sp_merge_replies_batch)."""
        self._chk(self.lib.L.sp_merge_replies_batch(self.h, C.c_void_p(d_gathered), int(ranks), int(renders), int(lut_len), C.c_void_p(d_merged)))

    def place_strips(self, d_image, d_strips, count, n, width, slice_width, waterfall=False):
        """Device-side putImageData of `count` gathered strips (laid end to end at d_strips) into the merged image (spectroplot.js:1241-1244)."""
        self._chk(self.lib.L.sp_place_strips(self.h, C.c_void_p(d_image), C.c_void_p(d_strips), int(count), int(n), int(width),
                                             int(slice_width), int(bool(waterfall))))

    def event_pair_overhead_ms(self):
        ms = C.c_float()
        self._chk(self.lib.L.sp_context_event_pair_overhead_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def last_kernel_ms(self):
        ms = C.c_float()
        self._chk(self.lib.L.sp_context_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    # -- device memory -----------------------------------------------------------------------------
    def alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.lib.L.sp_device_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, ptr):
        self._chk(self.lib.L.sp_device_free(self.h, C.c_void_p(ptr)))

    def upload(self, d_ptr, array):
        a = np.ascontiguousarray(array)
        self._chk(self.lib.L.sp_device_upload(self.h, C.c_void_p(d_ptr), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def download(self, d_ptr, nbytes, dtype=np.uint8):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        self._chk(self.lib.L.sp_device_download(self.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(d_ptr), out.nbytes))
        return out

    def memset(self, d_ptr, value, nbytes):
        self._chk(self.lib.L.sp_device_memset(self.h, C.c_void_p(d_ptr), value, nbytes))

    def synth_trinoise(self, d_ptr, fmt, t0, count, seed, step, gshift, amp, namp):
        fid = parse_format(fmt)[0]
        self._chk(self.lib.L.sp_synth_trinoise(self.h, C.c_void_p(d_ptr), fid, t0, count, seed, step, gshift, amp, namp))

    # -- renderFft on host buffers -------------------------------------------------------------------
    def render(self, fmt, data, n, windowc, block_norm, gain, rng, lut, width, channel_mode=False, waterfall=False, detector="sample"):
        """Same argument meaning as the reference message; returns the reply fields as numpy arrays.  detector: "sample" (the
        reference) or "peak" (max hold over the sub-frames between two columns, include/spectroplot_hip.h enum sp_detector)."""
        fid, _ = parse_format(fmt)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        req, keep = _make_request(fid, n, windowc, block_norm, gain, rng, lut, channel_mode, waterfall, detector)
        W = int(width)
        L = len(keep[1])
        out, mm, rep = _host_reply(W, n, L)
        self._chk(self.lib.L.sp_render(self.h, C.byref(req), _p(data), data.size, W, C.byref(rep)))
        out["dBfs_min"], out["dBfs_max"] = float(mm[0]), float(mm[1])
        return out

    def render_batch(self, fmt, datas, n, windowc, block_norm, gain, rng, lut, widths, channel_mode=False, waterfall=False,
                     detector="sample"):
        """sp_render_batch: every capture of `datas` (one width each) rendered with ONE plan; a list of dicts shaped as render()'s,
        each byte for byte what render() of that capture alone returns."""
        fid, _ = parse_format(fmt)
        datas = [np.ascontiguousarray(d, dtype=np.uint8) for d in datas]
        if len(widths) != len(datas):
            raise ValueError("one width per capture")
        req, keep = _make_request(fid, n, windowc, block_norm, gain, rng, lut, channel_mode, waterfall, detector)   # (peak: refused)
        L = len(keep[1])
        outs, mms = [], []
        items = (_BatchItem * max(len(datas), 1))()
        for k, (d, w) in enumerate(zip(datas, widths)):
            out, mm, items[k].reply = _host_reply(w, n, L)
            items[k].bytes = d.ctypes.data
            items[k].nbytes = d.size
            items[k].width = int(w)
            outs.append(out)
            mms.append(mm)
        self._chk(self.lib.L.sp_render_batch(self.h, C.byref(req), items, len(datas)))
        for out, mm in zip(outs, mms):
            out["dBfs_min"], out["dBfs_max"] = float(mm[0]), float(mm[1])
        return outs

    def render_named(self, fmt, data, n, window, cmap, gain, rng, width, channel_mode=False, waterfall=False, detector="sample"):
        """The request by option names, as the reference's caller assembles its message (lib/spectroplot.js:1113-1146): the library
        evaluates taper, block_norm and colour map (ends forced) itself and keeps the plan while names and numbers repeat."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        W = int(width)
        L = named_resolve(window, cmap)[2]
        req = _NamedRequest(str(fmt).encode(), str(window).encode(), str(cmap).encode(), int(n), int(bool(channel_mode)),
                            int(bool(waterfall)), float(gain), float(rng))
        out, mm, rep = _host_reply(W, n, L)
        self._chk(self.lib.L.sp_render_named_ex(self.h, C.byref(req), detector_id(detector), _p(data), data.size, W, C.byref(rep)))
        out["dBfs_min"], out["dBfs_max"] = float(mm[0]), float(mm[1])
        return out

    def render_traces(self, fmt, data, n, windowc, block_norm, gain, rng, width, channel_mode=False, lut=None, fill=None):
        """sp_render_traces: the per-bin min-hold / max-hold traces of the request, {"trace_min": f64[n], "trace_max": f64[n]} in image
        row order.  No image is rendered; `lut` only takes part in the plan-cache key (default: two grey entries).  fill: a value the
        output arrays hold before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        tmin, tmax = _filled(n, np.float64, fill, False), _filled(n, np.float64, fill, False)
        self._chk(self.lib.L.sp_render_traces(self.h, C.byref(req), _p(data), data.size, int(width), _p(tmin), _p(tmax)))
        return {"trace_min": tmin, "trace_max": tmax}

    def render_power(self, fmt, data, n, windowc, block_norm, gain, rng, width, channel_mode=False, db=False, lut=None, fill=None):
        """sp_render_power: the numeric spectrogram of the request, f64 [width, n]: |X|^2 of frame x at image row y in [x, y], or with
        db=True its dB plane.  No image is rendered; `lut` only takes part in the plan-cache key (default: two grey entries).  fill: a
        byte the output array holds before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        power = _filled((max(int(width), 0), int(n)), np.float64, fill)
        self._chk(self.lib.L.sp_render_power(self.h, C.byref(req), _p(data), data.size, int(width), 1 if db else 0, _p(power)))
        return power

    def render_mean(self, fmt, data, n, windowc, block_norm, gain, rng, width, channel_mode=False, db=False, lut=None, fill=None):
        """sp_render_mean: the exact mean-power trace of the request, f64[n] in image row order: the correctly rounded sum of |X|^2 over
        the frames divided by width, or with db=True the dB of it.  No image is rendered; `lut` only takes part in the plan-cache key
        (default: two grey entries).  fill: a byte the output array holds before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        mean = _filled(int(n), np.float64, fill)
        self._chk(self.lib.L.sp_render_mean(self.h, C.byref(req), _p(data), data.size, int(width), 1 if db else 0, _p(mean)))
        return mean

    def power_mean(self, d_power, n, width, d_mean):
        """sp_power_mean: the exact mean over the frames of the f64 [width, n] plane at device address d_power into f64[n] at d_mean.
        Asynchronous on the context's stream."""
        self._chk(self.lib.L.sp_power_mean(self.h, C.c_void_p(d_power or None), int(n), int(width), C.c_void_p(d_mean or None)))

    def render_variance(self, fmt, data, n, windowc, block_norm, gain, rng, width, channel_mode=False, lut=None, fill=None):
        """sp_render_variance: the exact variance sums of the request, f64 [3, n] in image row order: per row the correctly rounded sum
        of |X|^2 over the frames, the correctly rounded sum of its exact squares, and the correctly rounded width * sum of squares -
        sum**2 (variance_of and spectral_kurtosis take it from there).  No dB form.  No image is rendered; `lut` only takes part in the
        plan-cache key.  fill: a byte the output array holds before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        out = _filled((3, int(n)), np.float64, fill)
        self._chk(self.lib.L.sp_render_variance(self.h, C.byref(req), _p(data), data.size, int(width), _p(out)))
        return out

    def power_variance(self, d_power, n, width, d_out):
        """sp_power_variance: the exact variance sums over the frames of the f64 [width, n] plane at device address d_power into
        f64 [3, n] at d_out.  Asynchronous on the context's stream."""
        self._chk(self.lib.L.sp_power_variance(self.h, C.c_void_p(d_power or None), int(n), int(width), C.c_void_p(d_out or None)))

    def render_blockmean(self, fmt, data, n, windowc, block_norm, gain, rng, width, group, channel_mode=False, db=False, lut=None,
                         fill=None):
        """sp_render_blockmean: the averaged spectrogram of the request, f64 [columns, n]: per column of `group` frames and per image
        row the correctly rounded sum of |X|^2 over the column's frames divided by their number, or with db=True the dB of it.  No
        image is rendered; `lut` only takes part in the plan-cache key (default: two grey entries).  fill: a byte the output array holds
        before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        out = _filled((blockmean_columns(width, group), int(n)), np.float64, fill)
        self._chk(self.lib.L.sp_render_blockmean(self.h, C.byref(req), _p(data), data.size, int(width), int(group), 1 if db else 0,
                                                 _p(out) if out.size else None))
        return out

    def power_blockmean(self, d_power, n, width, group, d_out):
        """sp_power_blockmean: the block means over `group` frames at a time of the f64 [width, n] plane at device address d_power into
        f64 [columns, n] at d_out.  Asynchronous on the context's stream."""
        self._chk(self.lib.L.sp_power_blockmean(self.h, C.c_void_p(d_power or None), int(n), int(width), int(group),
                                                C.c_void_p(d_out or None)))

    def set_blockmean_direct_max(self, frames=0):
        """sp_context_set_blockmean_direct_max: the largest group whose whole columns take the direct kernel (0: the built default).
        The result does not depend on it (tests)."""
        self._chk(self.lib.L.sp_context_set_blockmean_direct_max(self.h, int(frames)))

    def render_bandpower(self, fmt, data, n, windowc, block_norm, gain, rng, width, bands, channel_mode=False, db=False, lut=None,
                         fill=None):
        """sp_render_bandpower: the exact band-power series of the request, f64 [count, width]: per band (y0, y1) of image rows and
        per frame the correctly rounded sum of |X|^2 over the band's rows, or with db=True the dB of it.  No image is rendered; `lut`
        only takes part in the plan-cache key (default: two grey entries).  fill: a byte the output array holds before the call
        (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        b, count = _band_array(bands)
        out = _filled((count, max(int(width), 0)), np.float64, fill)
        self._chk(self.lib.L.sp_render_bandpower(self.h, C.byref(req), _p(data), data.size, int(width), _p(b) if count else None, count,
                                                 1 if db else 0, _p(out) if out.size else None))
        return out

    def power_bands(self, d_power, n, width, bands, d_band):
        """sp_power_bands: the exact sums over the bands (y0, y1) of rows of every frame of the f64 [width, n] plane at device address
        d_power into f64 [count, width] at d_band.  Asynchronous on the context's stream; the bands are read before it returns."""
        b, count = _band_array(bands)
        self._chk(self.lib.L.sp_power_bands(self.h, C.c_void_p(d_power or None), int(n), int(width), _p(b) if count else None, count,
                                            C.c_void_p(d_band or None)))

    def render_moments(self, fmt, data, n, windowc, block_norm, gain, rng, width, bands, order=1, channel_mode=False, db=False, lut=None,
                       fill=None):
        """sp_render_moments: the exact spectral moments of the request, f64 [order + 1, count, width]: per band (y0, y1) of image rows
        and per frame the correctly rounded sums of (y - y0)**k * |X|^2 over the band's rows, k = 0 .. order.  db=True converts m[0]
        only: the higher moments have no dB form.  No image is rendered; `lut` only takes part in the plan-cache key.  fill: a byte the
        output array holds before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        b, count = _band_array(bands)
        out = _filled((max(int(order), 0) + 1, count, max(int(width), 0)), np.float64, fill)
        self._chk(self.lib.L.sp_render_moments(self.h, C.byref(req), _p(data), data.size, int(width), _p(b) if count else None, count,
                                               int(order), 1 if db else 0, _p(out) if out.size else None))
        return out

    def power_moments(self, d_power, n, width, bands, order, d_out):
        """sp_power_moments: the exact moments k = 0 .. order over the bands (y0, y1) of rows of every frame of the f64 [width, n] plane
        at device address d_power into f64 [order + 1, count, width] at d_out.  Asynchronous on the context's stream; the bands are
        read before it returns."""
        b, count = _band_array(bands)
        self._chk(self.lib.L.sp_power_moments(self.h, C.c_void_p(d_power or None), int(n), int(width), _p(b) if count else None, count,
                                              int(order), C.c_void_p(d_out or None)))

    def render_track(self, fmt, data, n, windowc, block_norm, gain, rng, width, bands, channel_mode=False, db=False, lut=None,
                     fill=None):
        """sp_render_track: the peak track of the request, (rows int32 [count, width], peaks f64 [count, width]): per band (y0, y1) of
        image rows and per frame the strongest row that is not a NaN (the smallest among equal ones; -1 where there is none) and its
        |X|^2 bit for bit (NaN where there is none), or with db=True the dB of it.  No image is rendered; `lut` only takes part in the
        plan-cache key (default: two grey entries).  fill: a byte the output arrays hold before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        b, count = _band_array(bands)
        rows = _filled((count, max(int(width), 0)), np.int32, fill)
        peaks = _filled((count, max(int(width), 0)), np.float64, fill)
        self._chk(self.lib.L.sp_render_track(self.h, C.byref(req), _p(data), data.size, int(width), _p(b) if count else None, count,
                                             1 if db else 0, _p(rows) if rows.size else None, _p(peaks) if peaks.size else None))
        return rows, peaks

    def power_tracks(self, d_power, n, width, bands, d_row, d_peak):
        """sp_power_tracks: the strongest row of the bands (y0, y1) of rows of every frame of the f64 [width, n] plane at device address
        d_power into int32 [count, width] at d_row, and its value into f64 [count, width] at d_peak (either address may be 0: not
        written).  Asynchronous on the context's stream; the bands are read before it returns."""
        b, count = _band_array(bands)
        self._chk(self.lib.L.sp_power_tracks(self.h, C.c_void_p(d_power or None), int(n), int(width), _p(b) if count else None, count,
                                             C.c_void_p(d_row or None), C.c_void_p(d_peak or None)))

    def render_occupancy(self, fmt, data, n, windowc, block_norm, gain, rng, width, threshold, bands=(), channel_mode=False, lut=None,
                         fill=None):
        """sp_render_occupancy: the occupancy counts of the request, (rows uint32 [n], frames uint32 [count, width]): rows[y] is the
        number of frames whose |X|^2 at image row y is >= threshold[y], frames[b, x] the number of rows of band (y0, y1) that reach
        theirs in frame x (a NaN on either side is no hit).  threshold: a number, for every row, or n values.  No image is rendered;
        `lut` only takes part in the plan-cache key (default: two grey entries).  fill: a byte the output arrays hold before the call
        (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        b, count = _band_array(bands)
        t = _threshold_array(threshold, n)
        rows = _filled(int(n), np.uint32, fill)
        frames = _filled((count, max(int(width), 0)), np.uint32, fill)
        self._chk(self.lib.L.sp_render_occupancy(self.h, C.byref(req), _p(data), data.size, int(width), _p(t), _p(b) if count else None,
                                                 count, _p(rows), _p(frames) if frames.size else None))
        return rows, frames

    def power_occupancy(self, d_power, n, width, d_threshold, bands, d_rows, d_frames):
        """sp_power_occupancy: the threshold crossings of the f64 [width, n] plane at device address d_power against the f64[n]
        thresholds at d_threshold: per row over the frames into uint32[n] at d_rows, per band (y0, y1) of rows and frame into uint32
        [count, width] at d_frames (either address may be 0: not written).  Asynchronous on the context's stream; the bands are read
        before it returns."""
        b, count = _band_array(bands)
        self._chk(self.lib.L.sp_power_occupancy(self.h, C.c_void_p(d_power or None), int(n), int(width), C.c_void_p(d_threshold or None),
                                                _p(b) if count else None, count, C.c_void_p(d_rows or None), C.c_void_p(d_frames or None)))

    def render_quantile(self, fmt, data, n, windowc, block_norm, gain, rng, width, q=(0.5,), ranks=None, channel_mode=False, db=False,
                        lut=None, fill=None):
        """sp_render_quantile: the percentile traces of the request, f64 [count, n] rank-major: per rank k and image row y element k
        of the row's `width` values of |X|^2 sorted ascending (np.sort(plane[:, y])[k]; a NaN where that element is one), or with
        db=True the dB of it.  ranks: the ranks themselves, or None: those of the quantiles `q` by quantile_rank (method='lower').  No
        image is rendered; `lut` only takes part in the plan-cache key.  fill: a byte the output array holds before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        r, count = _rank_array(width, q, ranks)
        out = _filled((count, int(n)), np.float64, fill)
        self._chk(self.lib.L.sp_render_quantile(self.h, C.byref(req), _p(data), data.size, int(width), 1 if db else 0,
                                                _p(r) if count else None, count, _p(out) if out.size else None))
        return out

    def power_quantile(self, d_power, n, width, ranks, d_out):
        """sp_power_quantile: per rank and row the element of that rank of the row's values over the frames of the f64 [width, n] plane
        at device address d_power, into f64 [count, n] at d_out.  Asynchronous on the context's stream; the ranks are read before it
        returns.  The context keeps 8 * n * width bytes of workspace."""
        r, count = _rank_array(width, None, ranks)
        self._chk(self.lib.L.sp_power_quantile(self.h, C.c_void_p(d_power or None), int(n), int(width), _p(r) if count else None, count,
                                               C.c_void_p(d_out or None)))

    def render_bursts(self, fmt, data, n, windowc, block_norm, gain, rng, width, bands, hi, lo, max_bursts, channel_mode=False, lut=None,
                      fill=None):
        """sp_render_bursts: the burst lists of the request, (counts uint32 [count], edges int32 [count, max_bursts, 2]): per band
        (y0, y1) of image rows a Schmitt trigger along the frames of its exact band sum - ON from a frame with sum >= hi, OFF from
        one with sum < lo, OFF in front of frame 0 - the total number of its bursts and start and end of the first max_bursts of
        them, -1 behind those.  hi, lo: a number for every band, or `count` values.  No image is rendered; `lut` only takes part in
        the plan-cache key.  fill: a byte the output arrays hold before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        b, count = _band_array(bands)
        h, l = _burst_thresholds(hi, lo, count)
        counts = _filled(count, np.uint32, fill)
        edges = _filled((count, max(int(max_bursts), 0), 2), np.int32, fill)
        self._chk(self.lib.L.sp_render_bursts(self.h, C.byref(req), _p(data), data.size, int(width), _p(b) if count else None, count,
                                              _p(h) if count else None, _p(l) if count else None, int(max_bursts), _p(counts),
                                              _p(edges) if edges.size else None))
        return counts, edges

    def power_bursts(self, d_power, n, width, bands, hi, lo, max_bursts, d_counts, d_edges):
        """sp_power_bursts: the burst lists of the f64 [width, n] plane at device address d_power: per band the total into uint32
        [count] at d_counts and the edges into int32 [count, max_bursts, 2] at d_edges (either address may be 0: not written).
        Asynchronous on the context's stream; bands, hi and lo are read before it returns."""
        b, count = _band_array(bands)
        h, l = _burst_thresholds(hi, lo, count)
        self._chk(self.lib.L.sp_power_bursts(self.h, C.c_void_p(d_power or None), int(n), int(width), _p(b) if count else None, count,
                                             _p(h) if count else None, _p(l) if count else None, int(max_bursts),
                                             C.c_void_p(d_counts or None), C.c_void_p(d_edges or None)))

    def series_bursts(self, d_series, count, width, hi, lo, max_bursts, d_counts, d_edges):
        """sp_series_bursts: the burst lists of the band-major f64 [count, width] series at device address d_series - power_bands'
        reply, for example - into d_counts and d_edges as for power_bursts.  Asynchronous on the context's stream."""
        count = int(count)
        h, l = _burst_thresholds(hi, lo, max(count, 0))
        self._chk(self.lib.L.sp_series_bursts(self.h, C.c_void_p(d_series or None), count, int(width), _p(h) if count > 0 else None,
                                              _p(l) if count > 0 else None, int(max_bursts), C.c_void_p(d_counts or None),
                                              C.c_void_p(d_edges or None)))

    def render_lagcov(self, fmt, data, n, windowc, block_norm, gain, rng, width, bands, pairs, lags, channel_mode=False, lut=None,
                      fill=None):
        """sp_render_lagcov: the exact lagged covariance sums of the request, f64 [3, npairs, lags]: per pair (ia, ib) of the bands
        (y0, y1) of image rows and per lag l, over the N = lagcov_terms(width, lags) terms, the correctly rounded sum of
        a[x] * b[x + l], the correctly rounded N * that sum - sum(a) * sum(b window) (signed; N**2 times the covariance) and the
        correctly rounded sum of b's window, a and b the exact band sums per frame.  No dB form.  No image is rendered; `lut` only takes
        part in the plan-cache key.  fill: a byte the output array holds before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        b, count = _band_array(bands)
        p, npairs = _pair_array(pairs)
        out = _filled((3, npairs, max(int(lags), 0)), np.float64, fill)
        self._chk(self.lib.L.sp_render_lagcov(self.h, C.byref(req), _p(data), data.size, int(width), _p(b) if count else None, count,
                                              _p(p) if npairs else None, npairs, int(lags), _p(out) if out.size else None))
        return out

    def power_lagcov(self, d_power, n, width, bands, pairs, lags, d_out):
        """sp_power_lagcov: the lagged covariance sums of the bands of the f64 [width, n] plane at device address d_power into f64
        [3, npairs, lags] at d_out.  Asynchronous on the context's stream; bands and pairs are read before it returns."""
        b, count = _band_array(bands)
        p, npairs = _pair_array(pairs)
        self._chk(self.lib.L.sp_power_lagcov(self.h, C.c_void_p(d_power or None), int(n), int(width), _p(b) if count else None, count,
                                             _p(p) if npairs else None, npairs, int(lags), C.c_void_p(d_out or None)))

    def series_lagcov(self, d_series, count, width, pairs, lags, d_out):
        """sp_series_lagcov: the lagged covariance sums of the band-major f64 [count, width] series at device address d_series -
        power_bands' reply, for example - into f64 [3, npairs, lags] at d_out.  Asynchronous on the context's stream."""
        p, npairs = _pair_array(pairs)
        self._chk(self.lib.L.sp_series_lagcov(self.h, C.c_void_p(d_series or None), int(count), int(width), _p(p) if npairs else None,
                                              npairs, int(lags), C.c_void_p(d_out or None)))

    def render_pulses(self, fmt, data, n, windowc, block_norm, gain, rng, width, bands, hi, lo, max_bursts, channel_mode=False, lut=None,
                      fill=None):
        """sp_render_pulses: the burst lists of the request as render_bursts() gives them and the measurements of every listed burst,
        (counts uint32 [count], edges int32 [count, max_bursts, 2], energy float64 [count, max_bursts], peak float64 [count,
        max_bursts], peak_at int32 [count, max_bursts]): energy is the exact sum of the burst's frames of the band sum rounded once
        (math.fsum), peak the largest of them and peak_at the earliest frame that holds it; behind the listed bursts -1 and the
        all-ones NaN.  fill: a byte the output arrays hold before the call (tests)."""
        data, req, keep = _no_picture_request(fmt, data, n, windowc, block_norm, gain, rng, lut, channel_mode)
        b, count = _band_array(bands)
        h, l = _burst_thresholds(hi, lo, count)
        m = max(int(max_bursts), 0)
        counts = _filled(count, np.uint32, fill)
        edges = _filled((count, m, 2), np.int32, fill)
        energy, peak = _filled((count, m), np.float64, fill), _filled((count, m), np.float64, fill)
        peak_at = _filled((count, m), np.int32, fill)
        some = edges.size > 0
        self._chk(self.lib.L.sp_render_pulses(self.h, C.byref(req), _p(data), data.size, int(width), _p(b) if count else None, count,
                                              _p(h) if count else None, _p(l) if count else None, int(max_bursts), _p(counts),
                                              _p(edges) if some else None, _p(energy) if some else None, _p(peak) if some else None,
                                              _p(peak_at) if some else None))
        return counts, edges, energy, peak, peak_at

    def power_pulses(self, d_power, n, width, bands, hi, lo, max_bursts, d_counts, d_edges, d_energy, d_peak, d_peak_at):
        """sp_power_pulses: power_bursts() and the measurements of the listed bursts of the f64 [width, n] plane at device address
        d_power: energy and peak into f64 [count, max_bursts] at d_energy and d_peak, the peak's frame into int32 [count, max_bursts]
        at d_peak_at (any address may be 0: not written).  Asynchronous on the context's stream."""
        b, count = _band_array(bands)
        h, l = _burst_thresholds(hi, lo, count)
        self._chk(self.lib.L.sp_power_pulses(self.h, C.c_void_p(d_power or None), int(n), int(width), _p(b) if count else None, count,
                                             _p(h) if count else None, _p(l) if count else None, int(max_bursts),
                                             C.c_void_p(d_counts or None), C.c_void_p(d_edges or None), C.c_void_p(d_energy or None),
                                             C.c_void_p(d_peak or None), C.c_void_p(d_peak_at or None)))

    def series_pulses(self, d_series, count, width, hi, lo, max_bursts, d_counts, d_edges, d_energy, d_peak, d_peak_at):
        """sp_series_pulses: series_bursts() and the measurements of the listed bursts of the band-major f64 [count, width] series at
        device address d_series, into the device arrays as for power_pulses.  Asynchronous on the context's stream.  The context
        keeps 552 bytes per band and slot of max_bursts."""
        count = int(count)
        h, l = _burst_thresholds(hi, lo, max(count, 0))
        self._chk(self.lib.L.sp_series_pulses(self.h, C.c_void_p(d_series or None), count, int(width), _p(h) if count > 0 else None,
                                              _p(l) if count > 0 else None, int(max_bursts), C.c_void_p(d_counts or None),
                                              C.c_void_p(d_edges or None), C.c_void_p(d_energy or None), C.c_void_p(d_peak or None),
                                              C.c_void_p(d_peak_at or None)))

    def set_mean_window(self, nbytes=0):
        """sp_context_set_mean_window: the bytes of plane a mean request renders before it accumulates them (0: the default, 64 MiB).
        The result does not depend on it (tests)."""
        self._chk(self.lib.L.sp_context_set_mean_window(self.h, int(nbytes)))

    def set_cu_count(self, cu=0):
        """sp_context_debug_set_cu_count: the CU count every launch on this context is shaped by from the next call on, 1 ... the
        device's own (0: the device's own again; anything else is refused).  The result does not depend on it (tests)."""
        self._chk(self.lib.L.sp_context_debug_set_cu_count(self.h, int(cu)))

    def render_index(self, fmt, data, n, windowc, block_norm, gain, rng, lut, width, channel_mode=False, waterfall=False,
                     detector="sample", want_index=True, fill=None):
        """sp_render_index: render()'s reply with "index" - one colour-index byte per pixel, u8[width * n] in the RGBA image's pixel
        order - in place of "rgba".  want_index=False asks for the side outputs only; fill: a byte every output holds before the call
        (tests)."""
        fid, _ = parse_format(fmt)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        req, keep = _make_request(fid, n, windowc, block_norm, gain, rng, lut, channel_mode, waterfall, detector)
        W = int(width)
        L = len(keep[1])
        out, mm, rep = _host_reply(W, n, L, "index", 1, fill)
        self._chk(self.lib.L.sp_render_index(self.h, C.byref(req), _p(data), data.size, W, C.byref(rep),
                                             _p(out["index"]) if want_index else None))
        out["dBfs_min"], out["dBfs_max"] = float(mm[0]), float(mm[1])
        return out

    def index_to_rgba(self, d_index, pixels, lut, d_rgba):
        """sp_index_to_rgba: the RGBA image of an index image on the device (addresses) through `lut` (u8[lut_len][3], a host array);
        an index the map does not have becomes (0, 0, 0, 255).  Asynchronous on the context's stream."""
        lut = np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1, 3)
        self._chk(self.lib.L.sp_index_to_rgba(self.h, C.c_void_p(d_index or None), int(pixels), lut.ctypes.data_as(C.c_void_p), len(lut),
                                              C.c_void_p(d_rgba or None)))

    def render_density(self, fmt, data, n, windowc, block_norm, gain, rng, lut, width, channel_mode=False, waterfall=False,
                       detector="sample", fill=None):
        """sp_render_density: the persistence spectrum of the request, np.uint32 [n, lut_len]: how many of the `width` frames showed
        colour index g in image row y.  fill: a value the array holds before the call (tests)."""
        fid, _ = parse_format(fmt)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        req, keep = _make_request(fid, n, windowc, block_norm, gain, rng, lut, channel_mode, waterfall, detector)
        out = np.full((int(n), len(keep[1])), 0 if fill is None else int(fill), np.uint32)
        self._chk(self.lib.L.sp_render_density(self.h, C.byref(req), data.ctypes.data_as(C.c_void_p), data.size, int(width),
                                               out.ctypes.data_as(C.c_void_p)))
        return out

    def density_from_index(self, d_index, n, width, waterfall, lut_len, d_density, accumulate=False):
        """sp_density_from_index: the per-row counts of an index image on the device (addresses; the layout `waterfall` names) into
        u32[n * lut_len] at d_density - overwritten, or added to with accumulate.  Asynchronous on the context's stream."""
        self._chk(self.lib.L.sp_density_from_index(self.h, C.c_void_p(d_index or None), int(n), int(width), int(bool(waterfall)),
                                                   int(lut_len), C.c_void_p(d_density or None), int(bool(accumulate))))

    def plan_creations(self):
        n = C.c_int64()
        self._chk(self.lib.L.sp_context_plan_creations(self.h, C.byref(n)))
        return n.value

    def plan(self, fmt, n, windowc, block_norm, gain, rng, lut, channel_mode=False, waterfall=False, detector="sample"):
        return Plan(self, fmt, n, windowc, block_norm, gain, rng, lut, channel_mode, waterfall, detector)


class Plan:
    """Request constants resident on the device; execute() runs the frame loop on device-resident operands."""

    def __init__(self, ctx, fmt, n, windowc, block_norm, gain, rng, lut, channel_mode=False, waterfall=False, detector="sample"):
        self.ctx = ctx
        self.detector = detector
        self.n = int(n)
        self.waterfall = bool(waterfall)
        self.fid, self.sample_width = parse_format(fmt)
        req, keep = _make_request(self.fid, n, windowc, block_norm, gain, rng, lut, channel_mode, waterfall, detector)
        self.lut_len = len(keep[1])
        h = C.c_void_p()
        ctx._chk(ctx.lib.L.sp_plan_create(ctx.h, C.byref(req), C.byref(h)))
        self.h = h
        ctx._plans.add(self)

    def close(self):
        if self.h:
            self.ctx.lib.L.sp_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kernel_name(self, nbytes=None, width=None):
        """The kernel execute() launches; with a request's shape, the one that request takes (a peak plan renders requests with one
        sub-frame per column through the sample detector's kernels)."""
        if nbytes is None:
            return self.ctx.lib.L.sp_plan_kernel_name(self.h).decode()
        return self.ctx.lib.L.sp_plan_kernel_name_for(self.h, int(nbytes), int(width)).decode()

    def debug_launch(self, nbytes, width, rgba=0):
        """What execute() would launch for a request of this shape whose image is at device address `rgba` (sp_plan_debug_launch): a
        dict of LAUNCH_FIELDS, "kernel" as a name of KERNELS."""
        out = np.zeros(len(LAUNCH_FIELDS), np.int64)
        used = C.c_size_t()
        self.ctx._chk(self.ctx.lib.L.sp_plan_debug_launch(self.h, int(nbytes), int(width), C.c_void_p(rgba or None),
                                                          out.ctypes.data_as(C.c_void_p), len(out), C.byref(used)))
        return _launch_dict(out)

    def force_kernel(self, which):
        self.ctx._chk(self.ctx.lib.L.sp_plan_force_kernel(self.h, {"auto": 0, "scratch": 1, "frames": 3}[which]))

    def execute(self, d_bytes, nbytes, width, rgba=0, gauge_mins=0, gauge_maxs=0, gauge_amps=0, c_hist=0, cb_hist=0, dbfs_minmax=0):
        """All pointer arguments are device addresses (ints); 0 skips that output. Asynchronous on the context's stream."""
        rep = _device_reply(rgba, gauge_mins, gauge_maxs, gauge_amps, c_hist, cb_hist, dbfs_minmax)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute(self.h, C.c_void_p(d_bytes), nbytes, int(width), C.byref(rep)))

    def _kernel_name_for(self, kind, nbytes, width):
        """sp_plan_<kind>_kernel_name_for: what that kind's execute runs for a request of this shape."""
        return getattr(self.ctx.lib.L, "sp_plan_%s_kernel_name_for" % kind)(self.h, int(nbytes), int(width)).decode()

    def traces_kernel_name_for(self, nbytes, width):
        """The frame loop execute_traces() launches for a request of this shape: "frames_traces" or "scratch_traces"."""
        return self._kernel_name_for("traces", nbytes, width)

    def execute_traces(self, d_bytes, nbytes, width, trace_min=0, trace_max=0):
        """sp_plan_execute_traces: the per-bin min / max traces of the request into two f64[n] device arrays (addresses; 0 skips one).
        Asynchronous on the context's stream."""
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_traces(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                            C.c_void_p(trace_min or None), C.c_void_p(trace_max or None)))

    def power_kernel_name_for(self, nbytes, width):
        """The frame loop execute_power() launches for a request of this shape: "frames_power" or "scratch_power"."""
        return self._kernel_name_for("power", nbytes, width)

    def execute_power(self, d_bytes, nbytes, width, d_power):
        """sp_plan_execute_power: |X|^2 of every frame and bin into the f64 [width, n] device array at address d_power (frame-major,
        image row order within a frame).  One launch, asynchronous on the context's stream."""
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_power(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                           C.c_void_p(d_power or None)))

    def mean_kernel_name_for(self, nbytes, width):
        """What execute_mean() launches for a request of this shape: "frames_power+mean" or "scratch_power+mean"."""
        return self._kernel_name_for("mean", nbytes, width)

    def execute_mean(self, d_bytes, nbytes, width, d_mean):
        """sp_plan_execute_mean: the exact mean of |X|^2 over the request's frames into the f64[n] device array at address d_mean
        (image row order).  Asynchronous on the context's stream."""
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_mean(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                          C.c_void_p(d_mean or None)))

    def variance_kernel_name_for(self, nbytes, width):
        """What execute_variance() launches for a request of this shape: "frames_power+variance" or "scratch_power+variance"."""
        return self._kernel_name_for("variance", nbytes, width)

    def execute_variance(self, d_bytes, nbytes, width, d_out):
        """sp_plan_execute_variance: per image row the exact sum of |X|^2 over the request's frames, the exact sum of its squares and
        width * sum of squares - sum**2, each rounded once, into the f64 [3, n] device array at address d_out.  Asynchronous on the
        context's stream."""
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_variance(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                              C.c_void_p(d_out or None)))

    def lagcov_kernel_name_for(self, nbytes, width):
        """What execute_lagcov() launches for a request of this shape: "frames_power+lagcov" or "scratch_power+lagcov"."""
        return self._kernel_name_for("lagcov", nbytes, width)

    def execute_lagcov(self, d_bytes, nbytes, width, bands, pairs, lags, d_out):
        """sp_plan_execute_lagcov: per pair (ia, ib) of the bands (y0, y1) of image rows and per lag the exact lagged covariance sums of
        their band-power series, each rounded once, into the f64 [3, npairs, lags] device array at address d_out.  Asynchronous on the
        context's stream; bands and pairs are read before it returns."""
        b, count = _band_array(bands)
        p, npairs = _pair_array(pairs)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_lagcov(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                            _p(b) if count else None, count, _p(p) if npairs else None, npairs, int(lags),
                                                            C.c_void_p(d_out or None)))

    def blockmean_kernel_name_for(self, nbytes, width):
        """What execute_blockmean() launches for a request of this shape: "frames_power+blockmean" or "scratch_power+blockmean"."""
        return self._kernel_name_for("blockmean", nbytes, width)

    def execute_blockmean(self, d_bytes, nbytes, width, group, d_out):
        """sp_plan_execute_blockmean: the exact means of |X|^2 over `group` frames at a time into the f64 [columns, n] device array at
        address d_out (frame-major, image row order).  Asynchronous on the context's stream."""
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_blockmean(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width), int(group),
                                                               C.c_void_p(d_out or None)))

    def power_to_index(self, d_power, width, d_index):
        """sp_plan_power_to_index: the colour index of every value of the f64 [width, n] plane at device address d_power, with the plan's
        gain, range and LUT length, into the u8 index image at d_index in the plan's layout.  Asynchronous on the context's stream."""
        self.ctx._chk(self.ctx.lib.L.sp_plan_power_to_index(self.h, C.c_void_p(d_power or None), int(width), C.c_void_p(d_index or None)))

    def bandpower_kernel_name_for(self, nbytes, width):
        """What execute_bandpower() launches for a request of this shape: "frames_power+bands" or "scratch_power+bands"."""
        return self._kernel_name_for("bandpower", nbytes, width)

    def execute_bandpower(self, d_bytes, nbytes, width, bands, d_band):
        """sp_plan_execute_bandpower: the exact sums of |X|^2 over the bands (y0, y1) of image rows, per frame, into the f64
        [count, width] device array at address d_band.  Asynchronous on the context's stream; the bands are read before it returns."""
        b, count = _band_array(bands)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_bandpower(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                               _p(b) if count else None, count, C.c_void_p(d_band or None)))

    def moments_kernel_name_for(self, nbytes, width):
        """What execute_moments() launches for a request of this shape: "frames_power+moments" or "scratch_power+moments"."""
        return self._kernel_name_for("moments", nbytes, width)

    def execute_moments(self, d_bytes, nbytes, width, bands, order, d_out):
        """sp_plan_execute_moments: the exact sums of (y - y0)**k * |X|^2 over the bands (y0, y1) of image rows, per frame and for
        k = 0 .. order, into the f64 [order + 1, count, width] device array at address d_out.  Asynchronous on the context's stream;
        the bands are read before it returns."""
        b, count = _band_array(bands)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_moments(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                             _p(b) if count else None, count, int(order), C.c_void_p(d_out or None)))

    def track_kernel_name_for(self, nbytes, width):
        """What execute_track() launches for a request of this shape: "frames_power+track" or "scratch_power+track"."""
        return self._kernel_name_for("track", nbytes, width)

    def execute_track(self, d_bytes, nbytes, width, bands, d_row, d_peak):
        """sp_plan_execute_track: per band (y0, y1) of image rows and per frame the strongest row into the int32 [count, width] device
        array at address d_row and its |X|^2 into the f64 [count, width] device array at d_peak (either may be 0: not written).
        Asynchronous on the context's stream; the bands are read before it returns."""
        b, count = _band_array(bands)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_track(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                           _p(b) if count else None, count, C.c_void_p(d_row or None),
                                                           C.c_void_p(d_peak or None)))

    def occupancy_kernel_name_for(self, nbytes, width):
        """What execute_occupancy() launches for a request of this shape: "frames_power+occupancy" or "scratch_power+occupancy"."""
        return self._kernel_name_for("occupancy", nbytes, width)

    def execute_occupancy(self, d_bytes, nbytes, width, d_threshold, bands, d_rows, d_frames):
        """sp_plan_execute_occupancy: the frames whose |X|^2 reaches the f64[n] thresholds at device address d_threshold, per image
        row, into the uint32[n] device array at d_rows, and per band (y0, y1) of image rows and frame the rows that reach theirs into the
        uint32 [count, width] device array at d_frames (either may be 0: not written).  Asynchronous on the context's stream; the
        bands are read before it returns."""
        b, count = _band_array(bands)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_occupancy(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                               C.c_void_p(d_threshold or None), _p(b) if count else None, count,
                                                               C.c_void_p(d_rows or None), C.c_void_p(d_frames or None)))

    def quantile_kernel_name_for(self, nbytes, width):
        """What execute_quantile() launches for a request of this shape: "frames_power+quantile" or "scratch_power+quantile"."""
        return self._kernel_name_for("quantile", nbytes, width)

    def execute_quantile(self, d_bytes, nbytes, width, ranks, d_out):
        """sp_plan_execute_quantile: per rank k of `ranks` and image row y element k of the row's `width` values of |X|^2 sorted
        ascending, into the f64 [count, n] device array at d_out, rank-major.  Asynchronous on the context's stream; the ranks are read
        before it returns.  The context keeps the request's plane as keys: 8 * n * width bytes."""
        r, count = _rank_array(width, None, ranks)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_quantile(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                              _p(r) if count else None, count, C.c_void_p(d_out or None)))

    def bursts_kernel_name_for(self, nbytes, width):
        """What execute_bursts() launches for a request of this shape: "frames_power+bursts" or "scratch_power+bursts"."""
        return self._kernel_name_for("bursts", nbytes, width)

    def execute_bursts(self, d_bytes, nbytes, width, bands, hi, lo, max_bursts, d_counts, d_edges):
        """sp_plan_execute_bursts: per band (y0, y1) of image rows the bursts of a Schmitt trigger along the frames of its exact band
        sum (hi, lo: a number for every band, or `count` values): the total into the uint32 [count] device array at d_counts, start
        and end of the first max_bursts into the int32 [count, max_bursts, 2] device array at d_edges, -1 behind them (either may be
        0: not written).  Asynchronous on the context's stream; bands, hi and lo are read before it returns.  The context keeps the
        band series, 8 * count * width bytes."""
        b, count = _band_array(bands)
        h, l = _burst_thresholds(hi, lo, count)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_bursts(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                            _p(b) if count else None, count, _p(h) if count else None,
                                                            _p(l) if count else None, int(max_bursts), C.c_void_p(d_counts or None),
                                                            C.c_void_p(d_edges or None)))

    def pulses_kernel_name_for(self, nbytes, width):
        """What execute_pulses() launches for a request of this shape: "frames_power+pulses" or "scratch_power+pulses"."""
        return self._kernel_name_for("pulses", nbytes, width)

    def execute_pulses(self, d_bytes, nbytes, width, bands, hi, lo, max_bursts, d_counts, d_edges, d_energy, d_peak, d_peak_at):
        """sp_plan_execute_pulses: execute_bursts() and, for every listed burst, its exact energy and its peak into the f64 [count,
        max_bursts] device arrays at d_energy and d_peak and the earliest frame of the peak into the int32 [count, max_bursts] device
        array at d_peak_at; -1 and the all-ones NaN behind the listed bursts (any address may be 0: not written).  Asynchronous on the
        context's stream; bands, hi and lo are read before it returns.  Beside the band series the context keeps 552 bytes per band
        and slot of max_bursts."""
        b, count = _band_array(bands)
        h, l = _burst_thresholds(hi, lo, count)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_pulses(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                            _p(b) if count else None, count, _p(h) if count else None,
                                                            _p(l) if count else None, int(max_bursts), C.c_void_p(d_counts or None),
                                                            C.c_void_p(d_edges or None), C.c_void_p(d_energy or None),
                                                            C.c_void_p(d_peak or None), C.c_void_p(d_peak_at or None)))

    def power_to_db(self, d_power, count, d_db):
        """sp_plan_power_to_db: d_db[k] = (5 * log10(d_power[k]) + block_norm_db + gain) - gain for k < count (device addresses; in place
        where they are equal).  Asynchronous on the context's stream."""
        self.ctx._chk(self.ctx.lib.L.sp_plan_power_to_db(self.h, C.c_void_p(d_power or None), int(count), C.c_void_p(d_db or None)))

    def index_kernel_name_for(self, nbytes, width):
        """What execute_index() runs for a request of this shape: "frames_index" or "render_extract"."""
        return self._kernel_name_for("index", nbytes, width)

    def debug_index_launch(self, nbytes, width, index=0):
        """debug_launch() for execute_index() with the index image at device address `index` (sp_plan_debug_index_launch); "kernel" is
        "frames_index" where k_frames_index runs, "rgba_fast" then tells whether its write-out stores 16-byte pieces."""
        out = np.zeros(len(LAUNCH_FIELDS), np.int64)
        used = C.c_size_t()
        self.ctx._chk(self.ctx.lib.L.sp_plan_debug_index_launch(self.h, int(nbytes), int(width), C.c_void_p(index or None),
                                                                out.ctypes.data_as(C.c_void_p), len(out), C.byref(used)))
        return _launch_dict(out)

    def execute_index(self, d_bytes, nbytes, width, index=0, rgba=0, gauge_mins=0, gauge_maxs=0, gauge_amps=0, c_hist=0, cb_hist=0,
                      dbfs_minmax=0):
        """sp_plan_execute_index: execute() with the picture as one colour-index byte per pixel at device address `index` (0: side
        outputs only); `rgba` must stay 0 (the library refuses anything else)."""
        rep = _device_reply(rgba, gauge_mins, gauge_maxs, gauge_amps, c_hist, cb_hist, dbfs_minmax)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_index(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width), C.byref(rep),
                                                           C.c_void_p(index or None)))

    def execute_density(self, d_bytes, nbytes, width, d_density, accumulate=False):
        """sp_plan_execute_density: the request's persistence spectrum into u32[n * lut_len] at device address d_density (overwritten,
        or added to with accumulate).  The index image lives in a workspace of the context (width * n bytes).  Asynchronous."""
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_density(self.h, C.c_void_p(d_bytes or None), int(nbytes), int(width),
                                                             C.c_void_p(d_density or None), int(bool(accumulate))))

    def execute_batch(self, items):
        """sp_plan_execute_batch: `items` = [(d_bytes, nbytes, width, {"rgba": addr, "gauge_mins": ..., "c_hist": ..., "cb_hist": ...,
        "dbfs_minmax": ...}), ...], every address on the device (missing keys: output skipped).  Asynchronous on the context's stream."""
        arr = (_BatchItem * max(len(items), 1))()
        keys = ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps", "c_hist", "cb_hist", "dbfs_minmax")
        for k, (d_bytes, nbytes, width, outs) in enumerate(items):
            arr[k].bytes = d_bytes or None
            arr[k].nbytes = int(nbytes)
            arr[k].width = int(width)
            arr[k].reply = _device_reply(*[outs.get(key) for key in keys])
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_batch(self.h, arr, len(items)))

    def execute_from_host(self, data, width, rgba=0, gauge_mins=0, gauge_maxs=0, gauge_amps=0, c_hist=0, cb_hist=0, dbfs_minmax=0):
        """sp_plan_execute_from_host: `data` is the capture in HOST memory (numpy uint8; it must stay alive until the context has been
        synchronised), the outputs are device addresses as for execute().  The samples travel in chunks under the renders; a sparse
        request uploads only what its frames read (ctx.last_upload_bytes())."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        rep = _device_reply(rgba, gauge_mins, gauge_maxs, gauge_amps, c_hist, cb_hist, dbfs_minmax)
        self.ctx._chk(self.ctx.lib.L.sp_plan_execute_from_host(self.h, data.ctypes.data_as(C.c_void_p), data.size, int(width), C.byref(rep)))
        return data


class Group:
    """The caller's sliced render from one process (sp_group_*): one member context per listed device, slice r rendered on member r,
    strips gathered device to device (RCCL or peer copies) and merged on the root (lib/spectroplot.js:1206-1244)."""

    def __init__(self, devices):
        self.lib = Library.get()
        arr = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        self.lib.check(self.lib.L.sp_group_create(arr, len(devices), C.byref(h)))
        self.h = h
        self.size = len(devices)

    def close(self):
        if self.h:
            self.lib.L.sp_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transport(self):
        return self.lib.L.sp_group_transport(self.h).decode()

    def transport_note(self):
        """Why the last transport was chosen when it was not the first choice (RCCL failures, peer access that could not be enabled)."""
        return self.lib.L.sp_group_transport_note(self.h).decode()

    def rccl_info(self):
        """Which RCCL the group has loaded (library path, version code, communicators); '' while none is."""
        buf = C.create_string_buffer(512)
        self.lib.L.sp_group_rccl_info(self.h, buf, len(buf))
        return buf.value.decode()

    def timings(self):
        """Milliseconds of the last render's phases: (upload + render of the slowest member, gather on the root, download)."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self.lib.L.sp_group_last_timings(self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def root_bytes(self):
        """(image bytes, staging bytes) the root member holds on its device for the gather."""
        a, b = C.c_size_t(), C.c_size_t()
        self.lib.L.sp_group_root_bytes(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def render(self, fmt, data, n, windowc, block_norm, gain, rng, lut, width, channel_mode=False, waterfall=False, gather="device",
               dirty=None, detector="sample"):
        """Same argument meaning as Context.render; the reply is the caller's MERGED result (`rgba` the whole image, histograms and
        dBfs range over all slices, gauges with slice r's at [r * slice_width, (r + 1) * slice_width)).  gather: "device" (strips meet
        in the root's HBM: RCCL / peer copies) or "host" (every member writes its band of the host image over its own link).
        dirty: a byte value the output buffers are pre-filled with (tests: what no slice draws must come back cleared)."""
        fid, _ = parse_format(fmt)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        req, keep = _make_request(fid, n, windowc, block_norm, gain, rng, lut, channel_mode, waterfall, detector)   # (peak: refused)
        W = int(width)
        L = len(keep[1])
        out, mm, rep = _host_reply(W, n, L)
        if dirty is not None:
            for k in ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps"):
                out[k][:] = dirty
        mode = {"device": 0, "host": 1}[gather]
        status = self.lib.L.sp_group_render_ex(self.h, C.byref(req), _p(data), data.size, W, C.byref(rep), mode)
        if status:
            raise SpectroplotError(status, self.lib.L.sp_group_last_error(self.h).decode() or self.lib.L.sp_status_string(status).decode())
        out["dBfs_min"], out["dBfs_max"] = float(mm[0]), float(mm[1])
        out["slice_width"] = W // self.size
        return out
