"""ctypes binding of include/oip_c.h.  No arithmetic here -- every method forwards device
pointers to liboipgpu.so.  Anything that cannot reach the HIP library raises."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
_LIB = None

STATUS_NAMES = {0: "OK", 1: "INVALID", 2: "RUNTIME", 3: "IO", 4: "DEVICE", 5: "NOMEM", 6: "UNSUPPORTED"}
# the exception classes the reference throws for each status (main.cpp:320-343 exit codes)
_STATUS_EXC = {1: ValueError, 2: RuntimeError, 3: OSError, 4: RuntimeError, 5: MemoryError, 6: NotImplementedError}


class OipError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("oip status %s: %s" % (STATUS_NAMES.get(status, status), msg))
        self.status = status


def library_path() -> str:
    # OIP_LIBRARY: another build of the same library (A/B experiments on one box: profiles/experiments/*.sh)
    return os.environ.get("OIP_LIBRARY") or os.path.join(_PKG, "lib", "liboipgpu.so")


def build(jobs: int = 8, quiet: bool = True) -> None:
    """Compile liboipgpu.so (+ the oip CLI) for gfx950 with hipcc."""
    subprocess.run(["make", "-C", os.path.join(_PKG, "csrc"), "-j%d" % jobs], check=True,
                   stdout=subprocess.DEVNULL if quiet else None)


def declared_symbols():
    """Every function name include/oip_c.h declares."""
    text = open(os.path.join(_ROOT, "include", "oip_c.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(oip_[a-z0-9_]+)\s*\(", text)))


_vp, _i, _l, _d, _sz = C.c_void_p, C.c_int, C.c_long, C.c_double, C.c_size_t
_dp, _lp, _cp = C.POINTER(C.c_double), C.POINTER(C.c_long), C.c_char_p
_SIGS = {
    "oip_version": ([], _i),
    "oip_create": ([_i, C.POINTER(_vp)], _i),
    "oip_destroy": ([_vp], None),
    "oip_last_error": ([_vp], _cp),
    "oip_set_stream": ([_vp, _vp], _i),
    "oip_get_stream": ([_vp], _vp),
    "oip_sync": ([_vp], _i),
    "oip_malloc": ([_vp, C.POINTER(_vp), _sz], _i),
    "oip_free": ([_vp, _vp], _i),
    "oip_memset": ([_vp, _vp, _i, _sz], _i),
    "oip_memcpy_h2d": ([_vp, _vp, _vp, _sz], _i),
    "oip_memcpy_d2h": ([_vp, _vp, _vp, _sz], _i),
    "oip_host_alloc": ([_vp, C.POINTER(_vp), _sz], _i),
    "oip_host_free": ([_vp, _vp], _i),
    "oip_load_rrc_param_file": ([_cp, _i, _dp, _cp, _i], _i),
    "oip_rrc_u16": ([_vp, _vp, _vp, _i, _l, _vp], _i),
    "oip_rrc_u16_window": ([_vp, _vp, _l, _vp, _l, _i, _l, _vp], _i),
    "oip_rrc_u16_host": ([_vp, _vp, _i, _l, _dp], _i),
    "oip_colstats_u16": ([_vp, _vp, _l, _i, _l, _i, _i, _vp], _i),
    "oip_rrc_fit_columns": ([C.POINTER(C.c_uint64), _i, _i, _i, C.c_uint64, _dp, C.POINTER(_i), _dp, _cp, _i], _i),
    "oip_write_rrc_param_file": ([_cp, _dp, _i, _cp, _i], _i),
    "oip_rrc_dead_columns": ([C.POINTER(C.c_uint64), _i, _i, C.c_uint64, C.POINTER(_i), C.POINTER(_i)], _i),
    "oip_decimate_box_u16": ([_vp, _vp, _l, _i, _l, _i, _i, _vp, _l, _sz], _i),
    "oip_histogram_u16": ([_vp, _vp, _l, _i, _l, _vp], _i),
    "oip_apply_lut_u8": ([_vp, C.POINTER(_vp), _l, _i, _l, _i, _vp, _vp], _i),
    "oip_stretch_limits": ([C.POINTER(C.c_uint64), _i, _i, _d, _d, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_uint64)], _i),
    "oip_stretch_lut_u8": ([_i, _i, C.POINTER(C.c_uint8)], _i),
    "oip_write_tiff_u8": ([_cp, _vp, _i, _l, _i, _cp, _i], _i),
    "oip_read_file_to_device": ([_vp, _cp, _sz, _sz, _vp, C.POINTER(_sz), _lp], _i),
    "oip_write_device_to_file": ([_vp, _vp, _sz, _cp, _i], _i),
    "oip_write_device_to_file_at": ([_vp, _vp, _sz, _cp, _sz, _l], _i),
    "oip_file_sink_open": ([_vp, _cp, _sz, C.POINTER(_vp)], _i),
    "oip_file_sink_write": ([_vp, _vp, _sz, _vp, _sz, _l], _i),
    "oip_file_sink_close": ([_vp, _vp], _i),
    "oip_compute_mark": ([_vp, _lp], _i),
    "oip_compute_mark_sync": ([_vp, _l], _i),
    "oip_download_staged_after": ([_vp, _vp, _vp, _sz, _l], _i),
    "oip_permute_u16x4": ([_vp, _vp, _sz, C.POINTER(_i)], _i),
    "oip_tiff_lzw_worst_bytes": ([_l, _i, _i, _l], _sz),
    "oip_tiff_lzw_scratch_bytes": ([_l, _i, _i, _l], _sz),
    "oip_tiff_lzw_decode_u16": ([_vp, _vp, _sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _l, _l, _i, _i, _l, _i, _vp], _i),
    "oip_tiff_deflate_decode_u16": ([_vp, _vp, _sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _l, _l, _i, _i, _l, _i, _vp], _i),
    "oip_tiff_lzw_strips_u16": ([_vp, _vp, _l, _i, _i, _l, _vp, _sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_sz), _vp, _sz], _i),
    "oip_tiff_deflate_worst_bytes": ([_l, _i, _i, _l], _sz),
    "oip_tiff_deflate_scratch_bytes": ([_l, _i, _i, _l], _sz),
    "oip_tiff_deflate_strips_u16": ([_vp, _vp, _l, _i, _i, _l, _vp, _sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_sz), _vp, _sz], _i),
    "oip_deflate_stream_host": ([_vp, _sz, _vp, _sz], _sz),
    "oip_jpeg_worst_bytes": ([_i, _l, _i], _sz),
    "oip_jpeg_scratch_bytes": ([_i, _l, _i], _sz),
    "oip_jpeg_scan_u8": ([_vp, _vp, _l, _i, _l, _i, _i, _vp, _sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_sz), _vp, _sz], _i),
    "oip_jpeg_interval_host": ([_vp, _l, _i, _l, _i, _i, _l, _vp, _sz], _sz),
    "oip_write_jpeg_u8": ([_cp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _i, _l, _i, _i, _cp, _i], _i),
    "oip_upload_staged": ([_vp, _vp, _vp, _sz, _lp], _i),
    "oip_upload_staged_2d": ([_vp, _vp, _sz, _vp, _sz, _sz, _sz, _lp], _i),
    "oip_download_staged": ([_vp, _vp, _vp, _sz], _i),
    "oip_stage_wait": ([_vp, _l], _i),
    "oip_stage_sync": ([_vp], _i),
    "oip_stage_order_after_compute": ([_vp], _i),
    "oip_stage_threads": ([], _i),
    "oip_stage_stats": ([_vp, _dp, _i], _i),
    "oip_mss_split_rrc_u16": ([_vp, _vp, _vp, _sz, _i, _l, _vp], _i),
    "oip_phase_correlate_f32": ([_vp, _vp, _vp, _i, _i, _dp, _dp, _dp], _i),
    "oip_window_u16_to_f32": ([_vp, _vp, _sz, _l, _i, _i, _i, _vp], _i),
    "oip_resize_cubic_f32": ([_vp, _vp, _i, _i, _vp, _i, _i], _i),
    "oip_stt_correlate": ([_vp, _vp, _vp, _i, _l, _l, _l, _i, _i, _i, _i, _dp], _i),
    "oip_stt_correlate_windows": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _dp], _i),
    "oip_interband_correlate_units": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _dp], _i),
    "oip_interband_correlate": ([_vp, _vp, _l, _l, _l, _vp, _sz, _l, _l, _i, _i, _i, _i, _dp], _i),
    "oip_peak_prune_stats": ([_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)], _i),
    "oip_rows_window_stats": ([_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)], _i),
    "oip_rows_window_geometry": ([_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)], _i),
    "oip_filter_and_fit": ([_dp, _i, _d, _i, _dp, _dp, _cp, _i], _i),
    "oip_filter_and_fit_mode": ([_dp, _i, _d, _i, _i, _dp, _dp, _cp, _i], _i),
    "oip_polyfit": ([_dp, _dp, _i, _i, _dp], _i),
    "oip_polyfit_reference": ([_dp, _dp, _i, _i, _dp], _i),
    "oip_stt_mean": ([_dp, _i, _d, _d, _dp, _dp, _dp, C.POINTER(_i)], _i),
    "oip_upsample_operator": ([_i, C.POINTER(C.c_float)], _i),
    "oip_fft_plan_describe": ([_i, _i, _cp, _i], _i),
    "oip_corr_route_describe": ([_i, _i, _i, _cp, _i], _i),
    "oip_remap_shift_bicubic_u16": ([_vp, _vp, _l, _l, _vp, _l, _l, _i, _l, _d, _d, _i, _i], _i),
    "oip_remap_shift_bicubic_u16_f16acc": ([_vp, _vp, _l, _l, _vp, _l, _l, _i, _l, _d, _d, _i, _i], _i),
    "oip_remap_shift_bicubic_u16_window": ([_vp, _vp, _l, _l, _vp, _l, _i, _l, _l, _l, _i, _l, _d, _d, _i, _i, _i], _i),
    "oip_remap_shift_rrc_bicubic_u16_window": ([_vp, _vp, _l, _l, _vp, _vp, _l, _i, _l, _l, _l, _i, _l, _d, _d, _i, _i, _i], _i),
    "oip_remap_shift_src_range": ([_l, _l, _l, _d, _i, _lp, _lp], _i),
    "oip_align_mss_bicubic_u16x4": ([_vp, _vp, _sz, _l, _l, _vp, _l, _l, _i, _l, _dp, _dp, _i, _i, _i, _i, _i, _lp], _i),
    "oip_align_mss_src_range": ([_l, _l, _l, _dp, _i, _i, _i, _i, _i, _i, _lp, _lp], _i),
    "oip_stitch_rows_u16": ([_vp, _vp, _vp, _vp, _i, _l, _i], _i),
    "oip_seam_moments_u16": ([_vp, _vp, _vp, _i, _l, _i, _i, _i, _i, _vp], _i),
    "oip_seam_fit": ([C.POINTER(C.c_uint64), _i, _i, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, C.POINTER(_i), _cp, _i], _i),
    "oip_stitch_balanced_u16": ([_vp, _vp, _vp, _vp, _i, _l, _i, _i, _vp, _vp, _i, _i], _i),
    "oip_seam_moments_blocks_u16": ([_vp, _vp, _vp, _i, _l, _i, _i, _i, _i, _l, _vp], _i),
    "oip_seam_fit_blocks": ([C.POINTER(C.c_uint64), _l, _i, _i, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_i),
                             C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_i), _dp, _cp, _i], _i),
    "oip_seam_line_tables": ([C.POINTER(C.c_int32), C.POINTER(C.c_int32), _l, _i, _l, _l, C.POINTER(C.c_int32), C.POINTER(C.c_int32)], _i),
    "oip_stitch_balanced_lines_u16": ([_vp, _vp, _vp, _vp, _i, _l, _i, _i, _vp, _vp, _i, _i], _i),
    "oip_convolve_u16": ([_vp, _vp, _l, _l, _vp, _l, _l, _i, _l, _i, C.POINTER(C.c_int32), _i, _i, _i], _i),
    "oip_mtfc_quantise": ([_dp, _i, _i, C.POINTER(C.c_int32), _cp, _i], _i),
    "oip_mtfc_design3": ([_d, _d, _d, _dp], _i),
    "oip_mtfc_load_kernel": ([_cp, _dp, C.POINTER(_i), C.POINTER(_i), _cp, _i], _i),
    "oip_despike_u16": ([_vp, _vp, _l, _l, _vp, _l, _l, _i, _l, _i, _i, _vp, _i, _i, _i, _vp], _i),
    "oip_load_column_list": ([_cp, _i, C.POINTER(_i), _i, C.POINTER(_i), _cp, _i], _i),
    "oip_write_column_list": ([_cp, C.POINTER(_i), _i, _cp, _cp, _i], _i),
    "oip_despike_column_table": ([C.POINTER(_i), _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(_i), _cp, _i], _i),
    "oip_noise_blocks_u16": ([_vp, _vp, _l, _i, _l, _i, _i, _i, _i, _i, _vp, _l, _sz], _i),
    "oip_noise_levels": ([C.POINTER(C.c_uint64), C.c_uint64, _dp, C.POINTER(C.c_uint64), C.POINTER(_i)], _i),
    "oip_noise_fit": ([_dp, C.POINTER(C.c_uint64), _i, _dp, _dp, _dp, _cp, _i], _i),
    "oip_noise_despike_threshold": ([_d, _d, _d, _d, C.POINTER(_i), C.POINTER(_i), _cp, _i], _i),
    "oip_sigma_filter_u16": ([_vp, _vp, _l, _l, _vp, _l, _l, _i, _l, _i, _i, _vp, _i, _i, _vp], _i),
    "oip_denoise_thresholds": ([_d, _d, _d, C.POINTER(C.c_uint16), _cp, _i], _i),
    "oip_mask_cells_u16": ([_vp, _vp, _l, _i, _l, _i, _i, _i, _i, _i, C.POINTER(_i), _i, _i, _i, _i, _vp, _l, _vp], _i),
    "oip_mask_morph_u8": ([_vp, _vp, _l, _i, _l, _i, _i, _vp], _i),
    "oip_mask_grid": ([_i, _l, _i, C.POINTER(_i), _lp], _i),
    "oip_mask_tile_flag": ([C.POINTER(C.c_uint8), _l, _i, _l, _i, _l, _l, _l, _l, _i], _i),
    "oip_block_moments_u16": ([_vp, _vp, _l, _i, _l, _i, _i, _i, _i, _vp, _l, _sz], _i),
    "oip_wallis_grid": ([_i, _l, _i, C.POINTER(_i), _lp], _i),
    "oip_wallis_fit": ([C.POINTER(C.c_uint64), _l, _sz, _i, _l, _i, _d, _d, _d, _d, C.c_uint64, _dp, _dp, C.POINTER(C.c_int32),
                        C.POINTER(C.c_int32), C.POINTER(_i), _dp, _cp, _i], _i),
    "oip_wallis_apply_u16": ([_vp, _vp, _vp, _l, _l, _i, _l, _i, _i, _vp, _vp, _i, _l, _i, _i, _i, _vp], _i),
    "oip_mtf_tiles_u16": ([_vp, _vp, _l, _i, _l, _i, _i, _i, _i, _i, _i, _vp, _l, _sz], _i),
    "oip_mtf_esf_u16": ([_vp, _vp, _l, _i, _l, _i, _i, _i, _i, _i, _i, _vp, _l, _vp, _vp], _i),
    "oip_mtf_tile": ([_i, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _dp], _i),
    "oip_mtf_summary": ([_dp, _l, _dp, _dp, _dp], _i),
    "oip_mtf_tv_slack": ([_d], _i),
    "oip_halve_u16": ([_vp, _vp, _l, _i, _l, _i, _i, _vp, _l], _i),
    "oip_overview_levels": ([_i, _l], _i),
    "oip_retile_u16": ([_vp, _vp, _l, _i, _l, _i, _i, _l, _l, _vp], _i),
    "oip_untile_u16": ([_vp, _vp, _i, _l, _i, _i, _l, _l, _vp, _l], _i),
    "oip_rescale_taps": ([_i, _l, _l, C.POINTER(_i), C.POINTER(C.c_int16), _sz, C.POINTER(_i), _cp, _i], _i),
    "oip_rescale_size": ([_l, _l, _l, _lp], _i),
    "oip_rescale_src_range": ([_l, _l, _i, _l, _l, _lp, _lp], _i),
    "oip_rescale_u16": ([_vp, _vp, _l, _l, _i, _l, _i, _vp, _l, _l, _i, _l, _vp, _vp, _i, _vp, _vp, _i, _i], _i),
    "oip_match_tiles_u16": ([_vp, _vp, _l, _i, _vp, _l, _i, _i, _l, _i, _i, _i, _l, _i, _l, _i, _l, _i, _i, _vp, _vp], _i),
    "oip_match_grid": ([_i, _l, _i, _i, _i, C.POINTER(_i), _lp, C.POINTER(_i), _lp], _i),
    "oip_match_peak": ([C.POINTER(C.c_uint64), _i, _i, _d, _dp, _dp, _dp, C.POINTER(_i)], _i),
    "oip_match_summary": ([_dp, _dp, C.POINTER(_i), _l, _dp], _i),
    "oip_warp_grid_bicubic_u16": ([_vp, _vp, _l, _l, _vp, _l, _l, _i, _l, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _i, _l, _l, _i, _i], _i),
    "oip_warp_grid_src_range": ([_l, _l, _l, C.POINTER(C.c_int32), _i, _i, _l, _i, _i, _lp, _lp], _i),
    "oip_regfix_load_report": ([_cp, _l, _l, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _l, _lp, _cp, _i], _i),
    "oip_regfix_fill": ([C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), _i, _i], _i),
    "oip_regfix_smooth": ([C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _i, _i], _i),
    "oip_pansharpen_sfim_u16": ([_vp, _vp, _l, _vp, _l, _vp, _l, _i, _l, _vp, _l, _l, _l, _i, _vp], _i),
    "oip_pansharpen_geometry": ([_l, _l, _l, _l, _l, _lp, _lp, _lp], _i),
    "oip_merge_subimages_be16": ([_vp, _vp, _vp, _i, _i, _i, _i], _i),
    "oip_profile_enable": ([_vp, _i], _i),
    "oip_profile_reset": ([_vp], _i),
    "oip_profile_filter": ([_vp, _cp], _i),
    "oip_profile_count": ([_vp], _i),
    "oip_profile_get": ([_vp, _i, _cp, _i, _dp, _lp], _i),
}


def load_library() -> C.CDLL:
    """dlopen liboipgpu.so (in-tree).  Raises if it has not been built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise OSError("liboipgpu.so not built at %s -- run __graft_entry__.build() "
                          "(there is no CPU fallback)" % path)
        # torch wheels bundle their own ROCm runtime; whichever HIP runtime is loaded first
        # in a process must be torch's, or the second one finds no devices.  (The oip CLI
        # links the system runtime and never meets torch.)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(path)
        for name, (args, res) in _SIGS.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is missing
            fn.argtypes = args
            fn.restype = res
        _LIB = lib
    return _LIB


def _ptr(t):
    """device pointer of a torch tensor / raw int"""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _dbl(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if n is not None:
        assert a.size == n, (a.size, n)
    return a


# ---- host-only entry points ---------------------------------------------------------------
def load_rrc_param_file(path: str, expected: int) -> np.ndarray:
    lib = load_library()
    out = np.zeros((expected, 2), np.float64)
    err = C.create_string_buffer(2048)
    rc = lib.oip_load_rrc_param_file(os.fsencode(path), expected, out.ctypes.data_as(_dp), err, 2048)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return out


RRCFIT_MODES = {"moments": 0, "gain": 1}


def rrc_fit_columns(acc, groups: int = 1, mode="moments", min_count: int = 0):
    """(k, b) per column from the (3, w) uint64 totals of Context.colstats_u16 (include/oip_c.h: oip_rrc_fit_columns).
    Returns (kb (w, 2), dead columns per group (groups,), (mu_ref, sigma_ref) per group (groups, 2))."""
    lib = load_library()
    a = np.ascontiguousarray(acc, dtype=np.uint64)
    assert a.ndim == 2 and a.shape[0] == 3, a.shape
    w = a.shape[1]
    kb, dead, ref = np.zeros((w, 2)), np.zeros(max(groups, 1), np.int32), np.zeros((max(groups, 1), 2))
    err = C.create_string_buffer(1024)
    rc = lib.oip_rrc_fit_columns(a.ctypes.data_as(C.POINTER(C.c_uint64)), w, groups, RRCFIT_MODES.get(mode, mode), min_count,
                                 kb.ctypes.data_as(_dp), dead.ctypes.data_as(C.POINTER(_i)), ref.ctypes.data_as(_dp), err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return kb, dead, ref


def write_rrc_param_file(path: str, kb) -> None:
    """RRCParam[n] in the format load_rrc_param_file (IMO::LoadRRCParamFile) reads; the doubles load back bit for bit"""
    lib = load_library()
    kb = _dbl(kb).reshape(-1, 2)
    err = C.create_string_buffer(2048)
    rc = lib.oip_write_rrc_param_file(os.fsencode(path), kb.ctypes.data_as(_dp), kb.shape[0], err, 2048)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())


def rrc_dead_columns(acc, mode="moments", min_count: int = 0) -> np.ndarray:
    """the columns of the (3, w) uint64 totals that rrc_fit_columns treats as not usable, ascending
    (include/oip_c.h: oip_rrc_dead_columns)"""
    lib = load_library()
    a = np.ascontiguousarray(acc, dtype=np.uint64)
    assert a.ndim == 2 and a.shape[0] == 3, a.shape
    w = a.shape[1]
    cols, n = np.zeros(w, np.int32), _i()
    rc = lib.oip_rrc_dead_columns(a.ctypes.data_as(C.POINTER(C.c_uint64)), w, RRCFIT_MODES.get(mode, mode), min_count,
                                  cols.ctypes.data_as(C.POINTER(_i)), C.byref(n))
    if rc:
        raise ValueError("oip_rrc_dead_columns: bad argument")
    return cols[:n.value].copy()


def load_column_list(path: str, w: int, cap: int = None) -> np.ndarray:
    """the sorted, unique 0-based columns of a bad-column text file for a w-sample line (include/oip_c.h: oip_load_column_list)"""
    lib = load_library()
    cap = w if cap is None else cap
    cols, n = np.zeros(max(cap, 1), np.int32), _i()
    err = C.create_string_buffer(2048)
    rc = lib.oip_load_column_list(os.fsencode(path), w, cols.ctypes.data_as(C.POINTER(_i)), cap, C.byref(n), err, 2048)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return cols[:n.value].copy()


def write_column_list(path: str, cols, comment: str = "") -> None:
    """`# comment`, then one column index per line (include/oip_c.h: oip_write_column_list)"""
    lib = load_library()
    c = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
    err = C.create_string_buffer(2048)
    rc = lib.oip_write_column_list(os.fsencode(path), c.ctypes.data_as(C.POINTER(_i)), c.size, comment.encode(), err, 2048)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())


def despike_column_table(bad, w: int, groups: int = 1):
    """((w, 2) int32 table of (Lx, Rx) per column, longest run of adjacent listed columns) for Context.despike_u16
    (include/oip_c.h: oip_despike_column_table)"""
    lib = load_library()
    b = np.ascontiguousarray(bad, dtype=np.int32).reshape(-1)
    tab, run = np.zeros((max(w, 1), 2), np.int32), _i()
    err = C.create_string_buffer(1024)
    rc = lib.oip_despike_column_table(b.ctypes.data_as(C.POINTER(_i)), b.size, w, groups, tab.ctypes.data_as(C.POINTER(C.c_int32)),
                                      C.byref(run), err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return tab, run.value


MASK_NODATA, MASK_SATURATED, MASK_CLOUD, MASK_BUFFER, MASK_CANDIDATE = 1, 2, 4, 8, 16
MASK_COUNTERS = ("cells", "nodata_cells", "saturated_cells", "tested_cells", "candidate_cells", "cloud_cells", "buffer_cells",
                 "saturated_pixels")


def mask_grid(w: int, h: int, cell: int):
    """(gw, gh) = (ceil(w / cell), ceil(h / cell)) of the mask of a w x h raster (include/oip_c.h: oip_mask_grid)"""
    gw, gh = _i(), _l()
    if load_library().oip_mask_grid(w, h, cell, C.byref(gw), C.byref(gh)):
        raise ValueError("oip_mask_grid: cell 4, 8 or 16 and w, h >= 0 expected")
    return gw.value, gh.value


def mask_tile_flag(flags, cell: int, x: int, y: int, tw: int, th: int, bits: int = MASK_CLOUD | MASK_BUFFER) -> bool:
    """whether a cell of the (gh, gw) uint8 mask that intersects the pixel rectangle [x, x + tw) x [y, y + th) has a bit of
    `bits` set (include/oip_c.h: oip_mask_tile_flag)"""
    f = np.asarray(flags)
    if f.dtype != np.uint8 or f.ndim != 2 or (f.size and f.strides[1] != 1) or f.strides[0] < f.shape[1]:
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        if f.ndim != 2:
            raise ValueError("mask_tile_flag: a (gh, gw) uint8 mask expected")
    pitch = f.strides[0] if f.shape[0] > 1 else max(f.shape[1], 1)
    return bool(load_library().oip_mask_tile_flag(f.ctypes.data_as(C.POINTER(C.c_uint8)), pitch, f.shape[1], f.shape[0], cell, x, y, tw, th, bits))


WALLIS_REPORT = ("samples", "mean", "std", "target_mean", "target_std", "nodes", "substituted_nodes", "min_gain_q16", "max_gain_q16")


def wallis_grid(w: int, h: int, block: int):
    """(gw, gh) = (ceil(w / block), ceil(h / block)) of the Wallis nodes of a w x h raster (include/oip_c.h: oip_wallis_grid)"""
    gw, gh = _i(), _l()
    if load_library().oip_wallis_grid(w, h, block, C.byref(gw), C.byref(gh)):
        raise ValueError("oip_wallis_grid: block 32, 64, 128 or 256 and w, h >= 0 expected")
    return gw.value, gh.value


def wallis_fit(acc, contrast: float = 0.8, brightness: float = 0.6, g_min: float = 0.25, g_max: float = 4.0, min_count: int = 0,
               target_mean=None, target_std=None):
    """node gains and offsets from the (3, spp, gh, gw) uint64 block moments of Context.block_moments_u16
    (include/oip_c.h: oip_wallis_fit).  target_mean / target_std: None, or spp values with NaN for the image's own.  Returns
    (gain_q16 (gh, gw, spp) int32, offset_q8 (gh, gw, spp) int32, substituted (gh, gw, spp) int32, report (spp, 9))."""
    a = np.ascontiguousarray(acc, dtype=np.uint64)
    if a.ndim != 4 or a.shape[0] != 3:
        raise ValueError("wallis_fit: (3, spp, gh, gw) moments expected")
    spp, gh, gw = a.shape[1:]
    i32 = C.POINTER(C.c_int32)
    gain, offset, sub = (np.zeros((gh, gw, spp), np.int32) for _ in range(3))
    report = np.zeros((spp, 9))
    tm = None if target_mean is None else _dbl(target_mean, spp)
    ts = None if target_std is None else _dbl(target_std, spp)
    err = C.create_string_buffer(1024)
    rc = load_library().oip_wallis_fit(a.ctypes.data_as(C.POINTER(C.c_uint64)), gw, gh * gw, gw, gh, spp, contrast, brightness, g_min, g_max,
                                       min_count, None if tm is None else tm.ctypes.data_as(_dp), None if ts is None else ts.ctypes.data_as(_dp),
                                       gain.ctypes.data_as(i32), offset.ctypes.data_as(i32), sub.ctypes.data_as(C.POINTER(_i)),
                                       report.ctypes.data_as(_dp), err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return gain, offset, sub, report


def noise_levels(hist, min_blocks: int = 100):
    """(sigma (256,) float64 with -1 for a level that is not usable, blocks (256,) uint64, usable levels) from the (65536,)
    uint64 histogram of a key plane of Context.noise_blocks_u16 (include/oip_c.h: oip_noise_levels)"""
    lib = load_library()
    h = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    assert h.size == 65536, h.size
    sigma, blocks, n = np.zeros(256), np.zeros(256, np.uint64), _i()
    rc = lib.oip_noise_levels(h.ctypes.data_as(C.POINTER(C.c_uint64)), min_blocks, sigma.ctypes.data_as(_dp),
                              blocks.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n))
    if rc:
        raise ValueError("oip_noise_levels: bad argument")
    return sigma, blocks, n.value


def noise_fit(sigma, blocks, level_shift: int):
    """(a, b, mu_ref) of sigma^2 = a + b mu over the usable levels of noise_levels (include/oip_c.h: oip_noise_fit)"""
    lib = load_library()
    s = _dbl(sigma, 256)
    n = np.ascontiguousarray(blocks, dtype=np.uint64).reshape(-1)
    assert n.size == 256, n.size
    a, b, mu = _d(), _d(), _d()
    err = C.create_string_buffer(1024)
    rc = lib.oip_noise_fit(s.ctypes.data_as(_dp), n.ctypes.data_as(C.POINTER(C.c_uint64)), level_shift, C.byref(a), C.byref(b), C.byref(mu), err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return a.value, b.value, mu.value


def noise_despike_threshold(a: float, b: float, mu_ref: float, k: float = 5.0):
    """(thr_abs, thr_rel_q8) of Context.despike_u16 from a noise model: the tangent at mu_ref to k sqrt(a + b mu)
    (include/oip_c.h: oip_noise_despike_threshold)"""
    lib = load_library()
    ta, q8 = _i(), _i()
    err = C.create_string_buffer(1024)
    rc = lib.oip_noise_despike_threshold(a, b, mu_ref, k, C.byref(ta), C.byref(q8), err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return ta.value, q8.value


def denoise_thresholds(a: float, b: float, k: float = 2.0):
    """the 256 uint16 thresholds of one band of Context.sigma_filter_u16 from its noise model: ceil(k sqrt(a + b level)) at the
    middle of every level, cut at 65535 (include/oip_c.h: oip_denoise_thresholds)"""
    lib = load_library()
    thr = np.zeros(256, dtype=np.uint16)
    err = C.create_string_buffer(1024)
    rc = lib.oip_denoise_thresholds(a, b, k, thr.ctypes.data_as(C.POINTER(C.c_uint16)), err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return thr


MTF_NO_VALUE = 16
MTF_AXES = {"x": 0, "y": 1}


def mtf_tile(s: int, sums, cnts):
    """the MTF at Nyquist of a tile from its polarity and its 64 edge-spread sums and counts (Context.mtf_esf_u16), or None for
    a tile without a value (include/oip_c.h: oip_mtf_tile)"""
    lib = load_library()
    a = np.ascontiguousarray(sums, dtype=np.uint32).reshape(-1)
    c = np.ascontiguousarray(cnts, dtype=np.uint32).reshape(-1)
    assert a.size == 64 and c.size == 64, (a.size, c.size)
    m = _d()
    rc = lib.oip_mtf_tile(int(s), a.ctypes.data_as(C.POINTER(C.c_uint32)), c.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(m))
    if rc == MTF_NO_VALUE:
        return None
    if rc:
        raise ValueError("oip_mtf_tile: bad argument")
    return m.value


def mtf_summary(values):
    """(median, p75, p90) of the tile values of a band and axis (include/oip_c.h: oip_mtf_summary)"""
    lib = load_library()
    v = _dbl(values).reshape(-1)
    med, p75, p90 = _d(), _d(), _d()
    if lib.oip_mtf_summary(v.ctypes.data_as(_dp), v.size, C.byref(med), C.byref(p75), C.byref(p90)):
        raise ValueError("oip_mtf_summary: bad argument")
    return med.value, p75.value, p90.value


def mtf_tv_slack(sigma_ref: float) -> int:
    """the --tv-slack that fits noise of sigma_ref DN (include/oip_c.h: oip_mtf_tv_slack)"""
    t = load_library().oip_mtf_tv_slack(sigma_ref)
    if t < 0:
        raise ValueError("oip_mtf_tv_slack: bad argument")
    return t


SEAM_MODES = {"moments": 0, "gain": 1, "offset": 2}


def seam_fit(acc, mode="moments", min_count: int = 0):
    """gain and offset (Q16) of image 2 relative to image 1 from the (6, spp) uint64 totals of Context.seam_moments_u16
    (include/oip_c.h: oip_seam_fit).  Returns (gain_q16 (spp,) int32, offset_q16 (spp,) int32, identity (spp,) int32,
    report (spp, 6): n, mean_a, mean_b, sigma_a, sigma_b, r)."""
    lib = load_library()
    m = SEAM_MODES.get(mode, mode)
    if not isinstance(m, int):
        raise ValueError("seam_fit: moments, gain or offset expected")
    a = np.ascontiguousarray(acc, dtype=np.uint64)
    assert a.ndim == 2 and a.shape[0] == 6, a.shape
    spp = a.shape[1]
    gain, offset, ident, report = np.zeros(spp, np.int32), np.zeros(spp, np.int32), np.zeros(spp, np.int32), np.zeros((spp, 6))
    err = C.create_string_buffer(1024)
    rc = lib.oip_seam_fit(a.ctypes.data_as(C.POINTER(C.c_uint64)), spp, m, min_count,
                          gain.ctypes.data_as(C.POINTER(C.c_int32)), offset.ctypes.data_as(C.POINTER(C.c_int32)), report.ctypes.data_as(_dp),
                          ident.ctypes.data_as(C.POINTER(_i)), err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return gain, offset, ident, report


def seam_fit_blocks(acc, mode="moments", min_count: int = 0):
    """a fit per block of lines from the (nb, 6, spp) uint64 totals of Context.seam_moments_blocks_u16, a block channel
    without a usable fit of its own taking the whole strip's (include/oip_c.h: oip_seam_fit_blocks).  Returns (gain_q16
    (nb, spp) int32, offset_q16 (nb, spp) int32, substituted (nb, spp) int32, gain0_q16 (spp,), offset0_q16 (spp,), identity0
    (spp,), report (nb, spp, 6))."""
    lib = load_library()
    m = SEAM_MODES.get(mode, mode)
    if not isinstance(m, int):
        raise ValueError("seam_fit_blocks: moments, gain or offset expected")
    a = np.ascontiguousarray(acc, dtype=np.uint64)
    assert a.ndim == 3 and a.shape[1] == 6, a.shape
    nb, spp = a.shape[0], a.shape[2]
    i32 = C.POINTER(C.c_int32)
    gain, offset, sub = (np.zeros((nb, spp), np.int32) for _ in range(3))
    gain0, offset0, ident0 = (np.zeros(spp, np.int32) for _ in range(3))
    report = np.zeros((nb, spp, 6))
    err = C.create_string_buffer(1024)
    rc = lib.oip_seam_fit_blocks(a.ctypes.data_as(C.POINTER(C.c_uint64)), nb, spp, m, min_count, gain.ctypes.data_as(i32),
                                 offset.ctypes.data_as(i32), sub.ctypes.data_as(C.POINTER(_i)), gain0.ctypes.data_as(i32),
                                 offset0.ctypes.data_as(i32), ident0.ctypes.data_as(C.POINTER(_i)), report.ctypes.data_as(_dp), err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return gain, offset, sub, gain0, offset0, ident0, report


def seam_line_tables(gain_q16, offset_q16, L: int, block_lines: int):
    """the (nb, spp) block values as nodes, interpolated to (L, spp) int32 tables of gain and offset per line
    (include/oip_c.h: oip_seam_line_tables); nb must be max(1, L // block_lines)"""
    lib = load_library()
    g = np.ascontiguousarray(gain_q16, dtype=np.int32)
    o = np.ascontiguousarray(offset_q16, dtype=np.int32)
    assert g.ndim == 2 and g.shape == o.shape, (g.shape, o.shape)
    nb, spp = g.shape
    i32 = C.POINTER(C.c_int32)
    lg, lo = np.zeros((max(L, 0), spp), np.int32), np.zeros((max(L, 0), spp), np.int32)
    rc = lib.oip_seam_line_tables(g.ctypes.data_as(i32), o.ctypes.data_as(i32), nb, spp, L, block_lines, lg.ctypes.data_as(i32),
                                  lo.ctypes.data_as(i32))
    if rc:
        raise ValueError("oip_seam_line_tables: bad argument")
    return lg, lo


def mtfc_quantise(c) -> np.ndarray:
    """(ky, kx) coefficients summing to 1 -> Q12 int32 taps with DC gain exactly 1 (include/oip_c.h: oip_mtfc_quantise);
    ValueError for a sum away from 1, an even or too large size, or sum |taps| above 32767"""
    lib = load_library()
    a = _dbl(c)
    if a.ndim != 2:
        raise ValueError("mtfc_quantise: a (ky, kx) array expected")
    taps = np.zeros(a.shape, np.int32)
    err = C.create_string_buffer(1024)
    rc = lib.oip_mtfc_quantise(a.ctypes.data_as(_dp), a.shape[0], a.shape[1], taps.ctypes.data_as(C.POINTER(C.c_int32)), err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return taps


def mtfc_design3(mtf_x: float, mtf_y: float, max_gain: float = 2.0) -> np.ndarray:
    """the separable 3 x 3 MTF-compensation coefficients (fp64) for the MTF at Nyquist of either axis
    (include/oip_c.h: oip_mtfc_design3)"""
    lib = load_library()
    c = np.zeros((3, 3))
    if lib.oip_mtfc_design3(mtf_x, mtf_y, max_gain, c.ctypes.data_as(_dp)):
        raise ValueError("oip_mtfc_design3: 0 < mtf <= 1 and max_gain >= 1 expected")
    return c


def mtfc_load_kernel(path: str) -> np.ndarray:
    """the (ky, kx) coefficients of a kernel text file (include/oip_c.h: oip_mtfc_load_kernel)"""
    lib = load_library()
    c = np.zeros(81)
    ky, kx = _i(), _i()
    err = C.create_string_buffer(2048)
    rc = lib.oip_mtfc_load_kernel(os.fsencode(path), c.ctypes.data_as(_dp), C.byref(ky), C.byref(kx), err, 2048)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return c[:ky.value * kx.value].reshape(ky.value, kx.value).copy()


def stretch_limits(hist, valid_min=1, valid_max=65535, p_lo=2.0, p_hi=98.0):
    """(lo, hi, n_valid) of a 65536-bin histogram: the values at the p_lo / p_hi percentile ranks among the samples with
    valid_min <= v <= valid_max (include/oip_c.h: oip_stretch_limits)"""
    lib = load_library()
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    assert h.shape == (65536,), h.shape
    lo, hi, n = _i(), _i(), C.c_uint64()
    rc = lib.oip_stretch_limits(h.ctypes.data_as(C.POINTER(C.c_uint64)), valid_min, valid_max, p_lo, p_hi, C.byref(lo), C.byref(hi), C.byref(n))
    if rc:
        raise ValueError("oip_stretch_limits: bad argument")
    return lo.value, hi.value, n.value


def stretch_lut_u8(lo: int, hi: int) -> np.ndarray:
    """the 65536-entry table of the linear stretch lo..hi -> 0..255 (include/oip_c.h: oip_stretch_lut_u8)"""
    lib = load_library()
    lut = np.zeros(65536, np.uint8)
    rc = lib.oip_stretch_lut_u8(lo, hi, lut.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc:
        raise ValueError("oip_stretch_lut_u8: bad argument")
    return lut


def write_tiff_u8(path: str, img) -> None:
    """(rows, w) or (rows, w, 3) uint8 as an uncompressed baseline TIFF (include/oip_c.h: oip_write_tiff_u8)"""
    lib = load_library()
    a = np.ascontiguousarray(img, dtype=np.uint8)
    assert a.ndim in (2, 3), a.shape
    err = C.create_string_buffer(1024)
    rc = lib.oip_write_tiff_u8(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0], 1 if a.ndim == 2 else a.shape[2], err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())


RESCALE_KERNELS = {"lanczos": 0, "cubic": 1, "linear": 2}


def rescale_taps(kind, n_in: int, n_out: int):
    """(first (n_out,) int32, taps (n_out, K) int16 in Q14, every row summing to 16384) of an axis that goes from n_in to n_out
    samples; kind is "lanczos", "cubic", "linear" or its number (include/oip_c.h: oip_rescale_taps)"""
    lib = load_library()
    kind = RESCALE_KERNELS.get(kind, kind)
    err = C.create_string_buffer(512)
    K = _i()
    rc = lib.oip_rescale_taps(kind, n_in, n_out, None, None, 0, C.byref(K), err, 512)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    first = np.zeros(n_out, np.int32)
    taps = np.zeros((n_out, K.value), np.int16)
    rc = lib.oip_rescale_taps(kind, n_in, n_out, first.ctypes.data_as(C.POINTER(_i)), taps.ctypes.data_as(C.POINTER(C.c_int16)), taps.size,
                              C.byref(K), err, 512)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return first, taps


def rescale_size(n_in: int, p: int, q: int) -> int:
    """floor(n_in p / q + 1/2) in exact integers (include/oip_c.h: oip_rescale_size)"""
    n = _l()
    if load_library().oip_rescale_size(n_in, p, q, C.byref(n)):
        raise ValueError("oip_rescale_size: n_in, p, q >= 1 and a result below 2^31 expected")
    return n.value


def rescale_src_range(n_in: int, n_out: int, K: int, out0: int, outs: int):
    """(src0, srcs): the source samples that outputs [out0, out0 + outs) of an axis read (include/oip_c.h: oip_rescale_src_range)"""
    a, b = _l(), _l()
    if load_library().oip_rescale_src_range(n_in, n_out, K, out0, outs, C.byref(a), C.byref(b)):
        raise ValueError("oip_rescale_src_range: bad argument")
    return a.value, b.value


def overview_levels(w: int, h: int) -> int:
    """the default level count of the pyramid of a w x h image (include/oip_c.h: oip_overview_levels)"""
    return load_library().oip_overview_levels(w, h)


def deflate_stored_bound(n: int) -> int:
    """the most a zlib stream of the project's encoder takes for n bytes: all of it in stored blocks (include/oip_c.h)"""
    return n + 5 * ((n + 65534) // 65535) + 6 if n else 11


def deflate_stream_host(data, cap: int = None) -> bytes:
    """`data` as one zlib stream by the host instantiation of the Deflate encoder (include/oip_c.h: oip_deflate_stream_host);
    cap: the room it is given (default: the stored bound).  b"" where it does not fit."""
    data = bytes(data)
    cap = deflate_stored_bound(len(data)) if cap is None else cap
    src = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    dst = (C.c_uint8 * max(cap, 1))()
    size = load_library().oip_deflate_stream_host(src, len(data), dst, cap)
    return bytes(dst[:size])


def jpeg_worst_bytes(w: int, h: int, nch: int) -> int:
    """the payload capacity oip_jpeg_scan_u8 asks for: 416 bytes a block (include/oip_c.h); 0 for a geometry it refuses"""
    return int(load_library().oip_jpeg_worst_bytes(w, h, nch))


def jpeg_interval_host(img, quality: int, interval: int, cap: int = None) -> bytes:
    """interval `interval` of a (h, w) or (h, w, 3) uint8 image by the host instantiation of the JPEG coder (include/oip_c.h:
    oip_jpeg_interval_host); cap: the room it is given (default: the bound).  b"" where it does not fit or is refused."""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    h, w, nch = a.shape[0], a.shape[1], 1 if a.ndim == 2 else a.shape[2]
    cap = (w + 7) // 8 * nch * 416 if cap is None else cap
    dst = (C.c_uint8 * max(cap, 1))()
    size = load_library().oip_jpeg_interval_host(a.ctypes.data, w * nch, w, h, nch, quality, interval, dst, cap)
    return bytes(dst[:size])


def write_jpeg_u8(path: str, payload, interval_off, interval_len, w: int, h: int, nch: int, quality: int) -> None:
    """the JFIF file of a scan (include/oip_c.h: oip_write_jpeg_u8); payload: host bytes or a uint8 array"""
    a = np.ascontiguousarray(np.frombuffer(payload, dtype=np.uint8) if isinstance(payload, (bytes, bytearray)) else payload, dtype=np.uint8)
    n = len(interval_off)
    off = (C.c_uint64 * n)(*[int(v) for v in interval_off])
    ln = (C.c_uint64 * n)(*[int(v) for v in interval_len])
    err = C.create_string_buffer(1024)
    rc = load_library().oip_write_jpeg_u8(os.fsencode(path), a.ctypes.data, off, ln, w, h, nch, quality, err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())


MATCH_RECORD_WORDS = 20
MATCH_NODATA, MATCH_FLAT, MATCH_EDGE, MATCH_WEAK = 1, 2, 4, 8


def match_grid(w: int, rows: int, T: int, S: int, step: int):
    """(x0, y0, nx, ny) of the regcheck grid of step `step` whose search windows lie inside w x rows (include/oip_c.h:
    oip_match_grid); ValueError for sizes out of range or an image that holds no tile"""
    x0, y0, nx, ny = _i(), _l(), _i(), _l()
    if load_library().oip_match_grid(w, rows, T, S, step, C.byref(x0), C.byref(y0), C.byref(nx), C.byref(ny)):
        raise ValueError("oip_match_grid: T a multiple of 8 in 8..128, 1 <= S <= 16, step >= 1 and an image of at least T + 2S expected")
    return x0.value, y0.value, nx.value, ny.value


def match_peak(record, T: int, S: int, min_score: float = 0.5):
    """(dx, dy, score, flags) of one 20-word record of Context.match_tiles_u16 (include/oip_c.h: oip_match_peak)"""
    r = np.ascontiguousarray(record, dtype=np.uint64).reshape(-1)
    assert r.size == MATCH_RECORD_WORDS, r.size
    dx, dy, sc, fl = _d(), _d(), _d(), _i()
    if load_library().oip_match_peak(r.ctypes.data_as(C.POINTER(C.c_uint64)), T, S, min_score, C.byref(dx), C.byref(dy), C.byref(sc), C.byref(fl)):
        raise ValueError("oip_match_peak: bad T, S or peak index")
    return dx.value, dy.value, sc.value, fl.value


def match_summary(dx, dy, flags) -> np.ndarray:
    """(count, mean dx, mean dy, std dx, std dy, rms, ce90, max) over the tiles whose flags are 0 (include/oip_c.h:
    oip_match_summary)"""
    x, y = _dbl(dx).reshape(-1), _dbl(dy).reshape(-1)
    f = np.ascontiguousarray(flags, dtype=np.int32).reshape(-1)
    assert x.size == y.size == f.size
    out = np.zeros(8)
    if load_library().oip_match_summary(x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), f.ctypes.data_as(C.POINTER(_i)), x.size, out.ctypes.data_as(_dp)):
        raise ValueError("oip_match_summary: bad argument")
    return out


_i32p = C.POINTER(C.c_int32)


def _nodes(nodes_x, nodes_y):
    """the two (ny, nx) int32 node arrays of a warp field, contiguous"""
    x, y = np.ascontiguousarray(nodes_x, dtype=np.int32), np.ascontiguousarray(nodes_y, dtype=np.int32)
    if x.ndim != 2 or x.shape != y.shape or x.size == 0:
        raise ValueError("warp field: two (ny, nx) node arrays of one shape expected")
    return x, y


def warp_grid_src_range(out_row0: int, out_rows: int, L: int, nodes_y, gy0: int, sy: int, include_output: bool = False):
    """source lines [first, last) that output lines [out_row0, out_row0 + out_rows) of Context.warp_grid_bicubic_u16 read
    (include/oip_c.h: oip_warp_grid_src_range)"""
    y = np.ascontiguousarray(nodes_y, dtype=np.int32)
    if y.ndim != 2 or y.size == 0:
        raise ValueError("warp field: a (ny, nx) node array expected")
    first, last = _l(), _l()
    if load_library().oip_warp_grid_src_range(out_row0, out_rows, L, y.ctypes.data_as(_i32p), y.shape[1], y.shape[0], gy0, sy, int(include_output),
                                              C.byref(first), C.byref(last)):
        raise ValueError("oip_warp_grid_src_range: bad argument")
    return first.value, last.value


def regfix_load_report(path: str, w: int = 0, h: int = 0, cap: int = 1 << 22):
    """the field of a regcheck report: (nodes_x, nodes_y (ny, nx) int32 Q10, dict(gx0, gy0, sx, sy, band2, used)); w, h: the image
    it is for, 0: not checked (include/oip_c.h: oip_regfix_load_report)"""
    x, y = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    geom = (C.c_long * 8)()
    err = C.create_string_buffer(1024)
    rc = load_library().oip_regfix_load_report(os.fsencode(path), w, h, x.ctypes.data_as(_i32p), y.ctypes.data_as(_i32p), cap, geom, err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode(errors="replace"))
    nx, ny = geom[0], geom[1]
    return (x[:nx * ny].reshape(ny, nx).copy(), y[:nx * ny].reshape(ny, nx).copy(),
            dict(gx0=geom[2], gy0=geom[3], sx=geom[4], sy=geom[5], band2=geom[6], used=geom[7]))


def regfix_fill(nodes_x, nodes_y, is_set):
    """the nodes where is_set is false filled from their set 4-neighbours in passes (include/oip_c.h: oip_regfix_fill)"""
    x, y = _nodes(nodes_x, nodes_y)
    x, y = x.copy(), y.copy()
    m = np.ascontiguousarray(is_set, dtype=np.uint8)
    if m.shape != x.shape:
        raise ValueError("regfix_fill: a mask of the nodes' shape expected")
    if load_library().oip_regfix_fill(x.ctypes.data_as(_i32p), y.ctypes.data_as(_i32p), m.ctypes.data_as(C.POINTER(C.c_uint8)), x.shape[1], x.shape[0]):
        raise ValueError("oip_regfix_fill: no node is set, or a value above 64 px")
    return x, y


def regfix_smooth(nodes_x, nodes_y, passes: int):
    """`passes` times [1 2 1] along and across the node lines, replicated edges (include/oip_c.h: oip_regfix_smooth)"""
    x, y = _nodes(nodes_x, nodes_y)
    x, y = x.copy(), y.copy()
    if load_library().oip_regfix_smooth(x.ctypes.data_as(_i32p), y.ctypes.data_as(_i32p), x.shape[1], x.shape[0], passes):
        raise ValueError("oip_regfix_smooth: 0 <= passes <= 16 and values within 64 px expected")
    return x, y


def pansharpen_geometry(W: int, Hp: int, w: int, h: int, line_offset: int = 0):
    """(out_w, out_h, mss_lines) of `oip pansharpen` for a W x Hp PAN raster used from line_offset on and a w x h MSS product
    (include/oip_c.h: oip_pansharpen_geometry)"""
    ow, oh, ml = _l(), _l(), _l()
    if load_library().oip_pansharpen_geometry(W, Hp, w, h, line_offset, C.byref(ow), C.byref(oh), C.byref(ml)):
        raise ValueError("oip_pansharpen_geometry: W = 4 w, w, h >= 1, line_offset >= 0 and 4 PAN lines from it on expected")
    return ow.value, oh.value, ml.value


FIT_MODES = {"reference": 0, "lstsq": 1}


def polyfit(x, y, deg: int, fit: str = "reference") -> np.ndarray:
    """fit="reference": NumCpp's operation order as the reference calls it (the product default);
    fit="lstsq": Householder QR on a scaled abscissa"""
    lib = load_library()
    x, y = _dbl(x), _dbl(y)
    out = np.zeros(deg + 1)
    fn = lib.oip_polyfit if FIT_MODES[fit] else lib.oip_polyfit_reference
    rc = fn(x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), x.size, deg, out.ctypes.data_as(_dp))
    if rc:
        raise _STATUS_EXC.get(rc, OipError)("oip_polyfit failed (%s)" % STATUS_NAMES.get(rc))
    return out


def filter_and_fit(shifts, threshold=0.4, min_count=5, fit: str = "reference"):
    lib = load_library()
    s = _dbl(shifts)
    assert s.ndim == 3 and s.shape[0] == 4 and s.shape[2] == 4
    cx, cy = np.zeros((4, 2)), np.zeros((4, 3))
    err = C.create_string_buffer(1024)
    rc = lib.oip_filter_and_fit_mode(s.ctypes.data_as(_dp), s.shape[1], threshold, min_count, FIT_MODES[fit],
                                     cx.ctypes.data_as(_dp), cy.ctypes.data_as(_dp), err, 1024)
    if rc:
        raise _STATUS_EXC.get(rc, OipError)(err.value.decode())
    return cx, cy


def stt_mean(table, threshold=0.4, max_delta_y=0.0):
    """stitcher.h:181-198 on an (S, 3) table -> (dx, dy, response, valid)"""
    lib = load_library()
    t = _dbl(table)
    dx, dy, r, v = _d(), _d(), _d(), _i()
    rc = lib.oip_stt_mean(t.ctypes.data_as(_dp), t.shape[0], threshold, max_delta_y, C.byref(dx), C.byref(dy), C.byref(r), C.byref(v))
    if rc == 2:
        raise RuntimeError("No valid delta value found for stitching parameter calculating")
    if rc:
        raise ValueError("oip_stt_mean: bad argument")
    return dx.value, dy.value, r.value, v.value


def upsample_operator(n):
    """H, G_0..G_3 of the x4 cubic up-sampling n -> 4 n as an operator on spectra (include/oip_c.h): complex64 (5, 4 n)"""
    lib = load_library()
    out = np.zeros((5, 4 * n, 2), np.float32)
    rc = lib.oip_upsample_operator(n, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise ValueError("oip_upsample_operator: unsupported length %d" % n)
    return out[..., 0] + 1j * out[..., 1]


def fft_plan_describe(M, N):
    """the FFT plan of an M x N correlation, from the planner (include/oip_c.h): one dict per pass in forward order, with
    axis ('y' | 'x'), F, mode, kind ('ct' | 'generic'), vshift, Vp, radix (a tuple) and lds; ValueError with the planner's
    own text where it refuses the size"""
    lib = load_library()
    buf = C.create_string_buffer(4096)
    rc = lib.oip_fft_plan_describe(int(M), int(N), buf, len(buf))
    if rc:
        raise ValueError(buf.value.decode() or "oip_fft_plan_describe: bad argument")
    passes = []
    for line in buf.value.decode().splitlines():
        f = dict(kv.split("=", 1) for kv in line.split())
        passes.append({k: v if k in ("axis", "kind") else tuple(int(r) for r in v.split(",") if r) if k == "radix" else int(v)
                       for k, v in f.items()})
    return passes


def corr_route_describe(rows, cols, cu_count=256):
    """the plan of an inter-band correlation call on rows x cols units, from its planner with the environment's switches
    (include/oip_c.h): a dict with route ('image' | 'H' | 'HV' | 'V'), row_kernel, pack_kernel, window, regions, ...;
    ValueError with the planner's own text where it refuses the geometry"""
    import json
    lib = load_library()
    buf = C.create_string_buffer(8192)
    rc = lib.oip_corr_route_describe(int(rows), int(cols), int(cu_count), buf, len(buf))
    if not buf.value:
        raise ValueError("oip_corr_route_describe: bad argument")
    d = json.loads(buf.value.decode())
    if rc:
        raise ValueError(d["refused"])
    return d


def remap_shift_src_range(out_row0, out_rows, L, dy, section_rows=30000):
    lib = load_library()
    a, b = C.c_long(), C.c_long()
    rc = lib.oip_remap_shift_src_range(out_row0, out_rows, L, dy, section_rows, C.byref(a), C.byref(b))
    if rc:
        raise ValueError("oip_remap_shift_src_range: bad argument")
    return a.value, b.value


def align_mss_src_range(out_row0, out_rows, Lm, cy, Wb, lines_per_section=20000, line_offset=0,
                        overlap=520, keep_leading=False, min_lines=1500):
    lib = load_library()
    cy = _dbl(cy, 12)
    a, b = C.c_long(), C.c_long()
    rc = lib.oip_align_mss_src_range(out_row0, out_rows, Lm, cy.ctypes.data_as(_dp), Wb, lines_per_section,
                                     line_offset, overlap, int(keep_leading), min_lines, C.byref(a), C.byref(b))
    if rc:
        raise ValueError("oip_align_mss_src_range: bad argument")
    return a.value, b.value


# ---- device context -------------------------------------------------------------------------
class Context:
    """One oip_ctx (one GPU).  Methods take torch CUDA tensors (or raw device pointers)."""

    def __init__(self, device: int = 0, stream=None):
        self.lib = load_library()
        h = _vp()
        rc = self.lib.oip_create(device, C.byref(h))
        if rc:
            raise OipError(rc, "oip_create(%d) failed: no gfx950 device (no CPU fallback)" % device)
        self.h = h
        self.device = device
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "h", None):
            self.lib.oip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            msg = self.lib.oip_last_error(self.h).decode()
            exc = _STATUS_EXC.get(rc, OipError)
            raise exc(msg) if exc is not OipError else OipError(rc, msg)

    def set_stream(self, stream):
        """stream: torch.cuda.Stream, raw hipStream_t int, or None for the context's own."""
        s = getattr(stream, "cuda_stream", stream)
        self._ck(self.lib.oip_set_stream(self.h, s))

    def get_stream(self):
        """the hipStream_t the context's kernels run on, as an integer"""
        return self.lib.oip_get_stream(self.h) or 0

    def sync(self):
        self._ck(self.lib.oip_sync(self.h))

    # -- RRC
    def upload_kb(self, kb):
        import torch
        kb = _dbl(kb)
        return torch.from_numpy(kb.reshape(-1, 2)).to("cuda:%d" % self.device)

    def rrc_u16(self, src, dst, w, h, d_kb):
        self._ck(self.lib.oip_rrc_u16(self.h, _ptr(src), _ptr(dst), w, h, _ptr(d_kb)))

    def rrc_u16_window(self, src, src_pitch, dst, dst_pitch, w, h, d_kb):
        """RRC of columns [0, w) of h lines (pitches in pixels): e.g. straight into the left half of a stitched raster"""
        self._ck(self.lib.oip_rrc_u16_window(self.h, _ptr(src), src_pitch, _ptr(dst), dst_pitch, w, h, _ptr(d_kb)))

    def colstats_u16(self, img, pitch, w, rows, acc, valid_min=0, valid_max=65535):
        """per-column count / sum / sum of squares of rows x w u16 (lines `pitch` pixels apart) ADDED into acc: (3, w) uint64
        on the device, zeroed by the caller before the first call"""
        self._ck(self.lib.oip_colstats_u16(self.h, _ptr(img), pitch, w, rows, valid_min, valid_max, _ptr(acc)))

    # -- quick look
    def decimate_box_u16(self, src, pitch, w, rows, spp, factor, dst, dst_pitch, dst_plane_stride=0):
        """factor x factor box means of rows x w pixels of spp samples (lines `pitch` samples apart) into one plane per channel,
        ceil(w / factor) x ceil(rows / factor) each (include/oip_c.h: oip_decimate_box_u16)"""
        self._ck(self.lib.oip_decimate_box_u16(self.h, _ptr(src), pitch, w, rows, spp, factor, _ptr(dst), dst_pitch, dst_plane_stride))

    def halve_u16(self, src, src_pitch, w, rows, spp, valid_min, dst, dst_pitch):
        """one pyramid level: 2 x 2 means, skipping samples below valid_min, of rows x w pixels of spp samples (lines src_pitch
        samples apart) into ceil(rows / 2) lines of ceil(w / 2) pixels, dst_pitch samples apart (include/oip_c.h: oip_halve_u16)"""
        self._ck(self.lib.oip_halve_u16(self.h, _ptr(src), src_pitch, w, rows, spp, valid_min, _ptr(dst), dst_pitch))

    def retile_u16(self, img, src_pitch, w, h, spp, T, tile_row0, tile_rows, tiles):
        """tile rows [tile_row0, tile_row0 + tile_rows) of the tile-major form (T x T tiles, edge tiles replicating the last column
        and line) of the w x h x spp image whose lines are src_pitch samples apart (include/oip_c.h: oip_retile_u16)"""
        self._ck(self.lib.oip_retile_u16(self.h, _ptr(img), src_pitch, w, h, spp, T, tile_row0, tile_rows, _ptr(tiles)))

    def untile_u16(self, tiles, w, h, spp, T, tile_row0, tile_rows, img, dst_pitch):
        """the inverse: the image samples of those tile rows from the tile-major buffer, whatever its padding holds
        (include/oip_c.h: oip_untile_u16)"""
        self._ck(self.lib.oip_untile_u16(self.h, _ptr(tiles), w, h, spp, T, tile_row0, tile_rows, _ptr(img), dst_pitch))

    def rescale_u16(self, src, src_row0, src_rows, W, L, spp, dst, out_row0, out_rows, Wo, Lo, first_x, taps_x, Kx, first_y, taps_y, Ky, valid_min=0):
        """output lines [out_row0, out_row0 + out_rows) of the W x L x spp raster resampled to Wo x Lo with the int32 first / int16
        Q14 tap tables of rescale_taps on the device; src holds the source lines [src_row0, src_row0 + src_rows), which must
        cover rescale_src_range(L, Lo, Ky, out_row0, out_rows) (include/oip_c.h: oip_rescale_u16)"""
        self._ck(self.lib.oip_rescale_u16(self.h, _ptr(src), src_row0, src_rows, W, L, spp, _ptr(dst), out_row0, out_rows, Wo, Lo, _ptr(first_x),
                                          _ptr(taps_x), Kx, _ptr(first_y), _ptr(taps_y), Ky, valid_min))

    def match_tiles_u16(self, a, pitch_a, stride_a, b, pitch_b, stride_b, w, rows, T, S, x0, y0, step_x, step_y, nx, ny, valid_min, valid_max,
                        records, sums=None):
        """regcheck: per tile of the nx x ny grid the 20-word record of the T x T template of plane a matched in plane b over
        offsets [-S, S]^2, and (sums not None) the three sums of every offset (include/oip_c.h: oip_match_tiles_u16)"""
        self._ck(self.lib.oip_match_tiles_u16(self.h, _ptr(a), pitch_a, stride_a, _ptr(b), pitch_b, stride_b, w, rows, T, S, x0, y0, step_x, step_y,
                                              nx, ny, valid_min, valid_max, _ptr(records), _ptr(sums)))

    def histogram_u16(self, img, pitch, w, rows, hist):
        """counts of rows x w u16 (lines `pitch` samples apart) ADDED into hist: 65536 uint64 on the device, zeroed by the caller"""
        self._ck(self.lib.oip_histogram_u16(self.h, _ptr(img), pitch, w, rows, _ptr(hist)))

    def apply_lut_u8(self, planes, pitch, w, rows, luts, out):
        """1 or 3 u16 planes through luts (nch x 65536 uint8 on the device) into out: rows x w x nch uint8, interleaved"""
        n = len(planes)
        pp = (C.c_void_p * n)(*[_ptr(p) for p in planes])
        self._ck(self.lib.oip_apply_lut_u8(self.h, pp, pitch, w, rows, n, _ptr(luts), _ptr(out)))

    def rrc_u16_host(self, buff: np.ndarray, kb):
        assert buff.dtype == np.uint16 and buff.flags.c_contiguous and buff.ndim == 2
        kb = _dbl(kb, buff.shape[1] * 2)
        self._ck(self.lib.oip_rrc_u16_host(self.h, buff.ctypes.data, buff.shape[1], buff.shape[0],
                                           kb.ctypes.data_as(_dp)))

    # -- raster I/O staging
    def read_file_to_device(self, path, d_dst, offset=0, nbytes=0, want_ticket=False):
        got, t = C.c_size_t(), C.c_long()
        self._ck(self.lib.oip_read_file_to_device(self.h, os.fsencode(path), offset, nbytes, _ptr(d_dst), C.byref(got),
                                                  C.byref(t) if want_ticket else None))
        return (got.value, t.value) if want_ticket else got.value

    def write_device_to_file(self, d_src, nbytes, path, append=False):
        self._ck(self.lib.oip_write_device_to_file(self.h, _ptr(d_src), nbytes, os.fsencode(path), int(append)))

    def write_device_to_file_at(self, d_src, nbytes, path, file_offset, mark=0, byte_offset=0):
        self._ck(self.lib.oip_write_device_to_file_at(self.h, _ptr(d_src) + byte_offset, nbytes, os.fsencode(path), file_offset, mark))

    def file_sink_open(self, path, nbytes):
        h = C.c_void_p()
        self._ck(self.lib.oip_file_sink_open(self.h, os.fsencode(path), nbytes, C.byref(h)))
        return h

    def file_sink_write(self, sink, file_offset, d_src, nbytes, mark=0, byte_offset=0):
        self._ck(self.lib.oip_file_sink_write(self.h, sink, file_offset, _ptr(d_src) + byte_offset, nbytes, mark))

    def file_sink_close(self, sink):
        self._ck(self.lib.oip_file_sink_close(self.h, sink))

    def compute_mark(self):
        m = C.c_long()
        self._ck(self.lib.oip_compute_mark(self.h, C.byref(m)))
        return m.value

    def compute_mark_sync(self, mark):
        self._ck(self.lib.oip_compute_mark_sync(self.h, mark))

    def permute_u16x4(self, img, npixels, order):
        o = (C.c_int * 4)(*[int(v) for v in order])
        self._ck(self.lib.oip_permute_u16x4(self.h, _ptr(img), npixels, o))

    def _tiff_strips(self, entry, img, rows, width, spp, rows_per_strip, payload, scratch, payload_cap, scratch_bytes):
        """one device strip encoder (include/oip_c.h: LZW's and Deflate's take the same arguments); returns (offsets, lengths,
        payload_bytes).  payload_cap / scratch_bytes: what the call is told the buffers hold, where that is not all of them"""
        n = (rows + rows_per_strip - 1) // max(rows_per_strip, 1) if rows > 0 else 1
        off = (C.c_uint64 * max(n, 1))()
        ln = (C.c_uint64 * max(n, 1))()
        total = C.c_size_t()
        if payload_cap is None:
            payload_cap = payload.numel() * payload.element_size()
        if scratch_bytes is None:
            scratch_bytes = scratch.numel() * scratch.element_size() if scratch is not None else 0
        self._ck(entry(self.h, _ptr(img), rows, width, spp, rows_per_strip, _ptr(payload), payload_cap, off, ln, C.byref(total),
                       _ptr(scratch) if scratch is not None else None, scratch_bytes))
        return np.array(off[:], dtype=np.uint64), np.array(ln[:], dtype=np.uint64), total.value

    def _tiff_decode(self, entry, d_file, strip_off, strip_len, rows, width, spp, rows_per_strip, predictor, d_img):
        """one device stream decoder: the streams in `d_file` (device, uint8; offsets relative to it) into d_img (device, rows x width x spp u16)"""
        n = len(strip_off)
        off = (C.c_uint64 * n)(*[int(v) for v in strip_off])
        ln = (C.c_uint64 * n)(*[int(v) for v in strip_len])
        self._ck(entry(self.h, _ptr(d_file), d_file.numel() * d_file.element_size(), off, ln, n, rows, width, spp, rows_per_strip, predictor, _ptr(d_img)))

    def tiff_lzw_strips(self, img, rows, width, spp, rows_per_strip, payload, scratch=None, payload_cap=None, scratch_bytes=None):
        """LZW strips (predictor 2) of a device image into `payload` (device, uint8)"""
        return self._tiff_strips(self.lib.oip_tiff_lzw_strips_u16, img, rows, width, spp, rows_per_strip, payload, scratch, payload_cap, scratch_bytes)

    def tiff_deflate_strips(self, img, rows, width, spp, rows_per_strip, payload, scratch=None, payload_cap=None, scratch_bytes=None):
        """Deflate strips (zlib streams, predictor 2) of a device image into `payload` (device, uint8)"""
        return self._tiff_strips(self.lib.oip_tiff_deflate_strips_u16, img, rows, width, spp, rows_per_strip, payload, scratch, payload_cap, scratch_bytes)

    def tiff_lzw_decode(self, d_file, strip_off, strip_len, rows, width, spp, rows_per_strip, predictor, d_img):
        """LZW strips decoded on the device"""
        self._tiff_decode(self.lib.oip_tiff_lzw_decode_u16, d_file, strip_off, strip_len, rows, width, spp, rows_per_strip, predictor, d_img)

    def tiff_deflate_decode(self, d_file, strip_off, strip_len, rows, width, spp, rows_per_strip, predictor, d_img):
        """Deflate (zlib) strips inflated on the device"""
        self._tiff_decode(self.lib.oip_tiff_deflate_decode_u16, d_file, strip_off, strip_len, rows, width, spp, rows_per_strip, predictor, d_img)

    def tiff_deflate_scratch_bytes(self, rows, width, spp, rows_per_strip):
        return int(self.lib.oip_tiff_deflate_scratch_bytes(rows, width, spp, rows_per_strip))

    def tiff_deflate_worst_bytes(self, rows, width, spp, rows_per_strip):
        return int(self.lib.oip_tiff_deflate_worst_bytes(rows, width, spp, rows_per_strip))

    def jpeg_scan(self, img, pitch_bytes, w, h, nch, quality, payload, scratch=None, payload_cap=None, scratch_bytes=None, byte_offset=0):
        """the scan of a baseline JPEG of a device image (uint8, from `byte_offset` on) into `payload` (device, uint8), an interval per
        row of 8 x 8 blocks (include/oip_c.h: oip_jpeg_scan_u8); returns (offsets, lengths, payload_bytes)"""
        n = max((h + 7) // 8, 1)
        off = (C.c_uint64 * n)()
        ln = (C.c_uint64 * n)()
        total = C.c_size_t()
        if payload_cap is None:
            payload_cap = payload.numel() * payload.element_size()
        if scratch_bytes is None:
            scratch_bytes = scratch.numel() * scratch.element_size() if scratch is not None else 0
        self._ck(self.lib.oip_jpeg_scan_u8(self.h, _ptr(img) + byte_offset if img is not None else None, pitch_bytes, w, h, nch, quality, _ptr(payload), payload_cap, off, ln,
                                           C.byref(total), _ptr(scratch) if scratch is not None else None, scratch_bytes))
        return np.array(off[:], dtype=np.uint64), np.array(ln[:], dtype=np.uint64), total.value

    def jpeg_scratch_bytes(self, w, h, nch):
        return int(self.lib.oip_jpeg_scratch_bytes(w, h, nch))

    def jpeg_worst_bytes(self, w, h, nch):
        return int(self.lib.oip_jpeg_worst_bytes(w, h, nch))

    def tiff_lzw_scratch_bytes(self, rows, width, spp, rows_per_strip):
        return int(self.lib.oip_tiff_lzw_scratch_bytes(rows, width, spp, rows_per_strip))

    def tiff_lzw_worst_bytes(self, rows, width, spp, rows_per_strip):
        return int(self.lib.oip_tiff_lzw_worst_bytes(rows, width, spp, rows_per_strip))

    def upload_staged(self, d_dst, host: np.ndarray, want_ticket=False, byte_offset=0):
        assert host.flags.c_contiguous
        t = C.c_long()
        self._ck(self.lib.oip_upload_staged(self.h, _ptr(d_dst) + byte_offset, host.ctypes.data, host.nbytes,
                                            C.byref(t) if want_ticket else None))
        return t.value if want_ticket else None

    def upload_staged_2d(self, d_dst, dst_pitch_bytes, host: np.ndarray, want_ticket=False, byte_offset=0):
        """a 2-D host view (rows contiguous, any row stride) into device rows dst_pitch_bytes apart"""
        assert host.ndim == 2 and host.strides[1] == host.itemsize and host.strides[0] >= host.shape[1] * host.itemsize
        t = C.c_long()
        self._ck(self.lib.oip_upload_staged_2d(self.h, _ptr(d_dst) + byte_offset, dst_pitch_bytes, host.ctypes.data, host.strides[0],
                                               host.shape[1] * host.itemsize, host.shape[0], C.byref(t) if want_ticket else None))
        return t.value if want_ticket else None

    def download_staged(self, host: np.ndarray, d_src, byte_offset=0, mark=0):
        assert host.flags.c_contiguous and host.flags.writeable
        self._ck(self.lib.oip_download_staged_after(self.h, host.ctypes.data, _ptr(d_src) + byte_offset, host.nbytes, mark))

    def stage_wait(self, ticket):
        self._ck(self.lib.oip_stage_wait(self.h, ticket))

    def stage_stats(self, reset=False):
        """(seconds in pageable -> pinned copies, seconds waiting for a ring slot, bytes, calls) of the upload lane"""
        out = (C.c_double * 4)()
        self._ck(self.lib.oip_stage_stats(self.h, out, 1 if reset else 0))
        return tuple(out)

    def stage_order_after_compute(self):
        self._ck(self.lib.oip_stage_order_after_compute(self.h))

    def stage_sync(self):
        self._ck(self.lib.oip_stage_sync(self.h))

    def mss_split_rrc_u16(self, bil, planes, plane_stride, w, lines, d_kb4):
        self._ck(self.lib.oip_mss_split_rrc_u16(self.h, _ptr(bil), _ptr(planes), plane_stride, w, lines, _ptr(d_kb4)))

    # -- correlation
    def phase_correlate_f32(self, a, b, rows, cols):
        dx, dy, r = _d(), _d(), _d()
        self._ck(self.lib.oip_phase_correlate_f32(self.h, _ptr(a), _ptr(b), rows, cols, C.byref(dx), C.byref(dy), C.byref(r)))
        return (dx.value, dy.value), r.value

    def window_u16_to_f32(self, img, pitch, row0, col0, rows, cols, out):
        self._ck(self.lib.oip_window_u16_to_f32(self.h, _ptr(img), pitch, row0, col0, rows, cols, _ptr(out)))

    def resize_cubic_f32(self, src, sw, sh, dst, dw, dh):
        self._ck(self.lib.oip_resize_cubic_f32(self.h, _ptr(src), sw, sh, _ptr(dst), dw, dh))

    def stt_correlate(self, pan1, pan2, W, L, row0, nrows, sections=10, lines_per_section=16000,
                      overlap_cols=200, edge_cols=0):
        out = np.zeros((sections, 3))
        self._ck(self.lib.oip_stt_correlate(self.h, _ptr(pan1), _ptr(pan2), W, L, row0, nrows, sections,
                                            lines_per_section, overlap_cols, edge_cols, out.ctypes.data_as(_dp)))
        return out

    def interband_correlate(self, pan, Lp, prow0, pn, planes, plane_stride, mrow0, mn, W, slices=10,
                            sections=5, corr_lines=16000):
        out = np.zeros((4, sections * slices, 4))
        self._ck(self.lib.oip_interband_correlate(self.h, _ptr(pan), Lp, prow0, pn, _ptr(planes), plane_stride,
                                                  mrow0, mn, W, slices, sections, corr_lines,
                                                  out.ctypes.data_as(_dp)))
        return out

    def stt_correlate_windows(self, a_ptrs, a_pitch, b_ptrs, b_pitch, rows, cols):
        """n explicit CCD window pairs (device pointers + element pitches) -> (n, 3) dx, dy, response"""
        n = len(a_ptrs)
        out = np.zeros((n, 3))
        if n == 0:
            return out
        pa = (C.c_void_p * n)(*[_ptr(p) for p in a_ptrs]); pb = (C.c_void_p * n)(*[_ptr(p) for p in b_ptrs])
        qa = (C.c_size_t * n)(*a_pitch); qb = (C.c_size_t * n)(*b_pitch)
        self._ck(self.lib.oip_stt_correlate_windows(self.h, pa, qa, pb, qb, n, rows, cols, out.ctypes.data_as(_dp)))
        return out

    def interband_correlate_units(self, pan_ptrs, pan_pitch, band_ptrs, band_pitch, rows, cols):
        """n explicit (section, slice) units; band_ptrs is n x 4 device pointers -> (n, 4, 3) dx, dy, rs"""
        n = len(pan_ptrs)
        out = np.zeros((n, 4, 3))
        if n == 0:
            return out
        pp = (C.c_void_p * n)(*[_ptr(p) for p in pan_ptrs])
        bp = (C.c_void_p * (4 * n))(*[_ptr(p) for u in band_ptrs for p in u])
        qp = (C.c_size_t * n)(*pan_pitch); qb = (C.c_size_t * n)(*band_pitch)
        self._ck(self.lib.oip_interband_correlate_units(self.h, pp, qp, bp, qb, n, rows, cols, out.ctypes.data_as(_dp)))
        return out

    def peak_prune_stats(self):
        """(tiles searched, tiles in all) of the spectral route's peak search since the previous call; starts the count again"""
        s, t = C.c_longlong(0), C.c_longlong(0)
        self._ck(self.lib.oip_peak_prune_stats(self.h, C.byref(s), C.byref(t)))
        return s.value, t.value

    def rows_window_stats(self):
        """(pairs of units correlated with the row stage's stored window, pairs run again with every column stored) since
        the previous call; starts the count again"""
        p, r = C.c_longlong(0), C.c_longlong(0)
        self._ck(self.lib.oip_rows_window_stats(self.h, C.byref(p), C.byref(r)))
        return p.value, r.value

    def rows_window_geometry(self):
        """(tile width in columns, tiles, radius R in tiles or -1 when every column was stored) of the latest correlation
        call: tiles 0 .. R and tiles - R .. tiles - 1 were stored"""
        v, t, r = C.c_int(0), C.c_int(0), C.c_int(-1)
        self._ck(self.lib.oip_rows_window_geometry(self.h, C.byref(v), C.byref(t), C.byref(r)))
        return v.value, t.value, r.value

    # -- resampling
    def remap_shift_bicubic_u16(self, src, dst, W, L, dx, dy, section_rows=30000, row_guard=32767,
                                src_row0=0, src_rows=None, out_row0=0, out_rows=None, f16acc=False):
        """f16acc=True: the fp16-accumulate variant (not the parity mode; tolerance in include/oip_c.h)"""
        src_rows = L if src_rows is None else src_rows
        out_rows = L if out_rows is None else out_rows
        fn = self.lib.oip_remap_shift_bicubic_u16_f16acc if f16acc else self.lib.oip_remap_shift_bicubic_u16
        self._ck(fn(self.h, _ptr(src), src_row0, src_rows, _ptr(dst), out_row0, out_rows, W, L, dx, dy,
                    section_rows, row_guard))

    def remap_shift_bicubic_u16_window(self, src, dst, dst_pitch, dst_col0, dst_col_off, W, L, dx, dy, section_rows=30000,
                                       row_guard=32767, src_row0=0, src_rows=None, out_row0=0, out_rows=None, f16acc=False):
        """the same resampling written into a window of another raster (columns >= dst_col0 only; see include/oip_c.h)"""
        src_rows = L if src_rows is None else src_rows
        out_rows = L if out_rows is None else out_rows
        self._ck(self.lib.oip_remap_shift_bicubic_u16_window(self.h, _ptr(src), src_row0, src_rows, _ptr(dst), dst_pitch, dst_col0,
                                                             dst_col_off, out_row0, out_rows, W, L, dx, dy, section_rows, row_guard,
                                                             1 if f16acc else 0))

    def remap_shift_rrc_bicubic_u16_window(self, src_raw, d_kb, dst, dst_pitch, dst_col0, dst_col_off, W, L, dx, dy, section_rows=30000,
                                           row_guard=32767, src_row0=0, src_rows=None, out_row0=0, out_rows=None, f16acc=False):
        """the windowed resampling with the RAW strip as source: RRC applied on load (see include/oip_c.h)"""
        src_rows = L if src_rows is None else src_rows
        out_rows = L if out_rows is None else out_rows
        self._ck(self.lib.oip_remap_shift_rrc_bicubic_u16_window(self.h, _ptr(src_raw), src_row0, src_rows, _ptr(d_kb), _ptr(dst), dst_pitch,
                                                                 dst_col0, dst_col_off, out_row0, out_rows, W, L, dx, dy, section_rows,
                                                                 row_guard, 1 if f16acc else 0))

    def align_mss_bicubic_u16x4(self, planes, plane_stride, dst, Wb, Lm, cx, cy, lines_per_section=20000,
                                line_offset=0, overlap=520, keep_leading=False, min_lines=1500,
                                src_row0=0, src_rows=None, out_row0=0, out_rows=None):
        cx, cy = _dbl(cx, 8), _dbl(cy, 12)
        src_rows = Lm if src_rows is None else src_rows
        total = Lm - line_offset - (0 if keep_leading else overlap)
        out_rows = total if out_rows is None else out_rows
        valid = C.c_long()
        self._ck(self.lib.oip_align_mss_bicubic_u16x4(self.h, _ptr(planes), plane_stride, src_row0, src_rows,
                                                      _ptr(dst), out_row0, out_rows, Wb, Lm,
                                                      cx.ctypes.data_as(_dp), cy.ctypes.data_as(_dp),
                                                      lines_per_section, line_offset, overlap, int(keep_leading),
                                                      min_lines, C.byref(valid)))
        return valid.value

    def stitch_rows_u16(self, left, right, out, W, L, fold):
        self._ck(self.lib.oip_stitch_rows_u16(self.h, _ptr(left), _ptr(right), _ptr(out), W, L, fold))

    # -- seam balancing and feathering
    def seam_moments_u16(self, left, right, Ws, L, fs, spp, acc, valid_min=0, valid_max=65535):
        """overlap totals n, Sa, Sb, Saa, Sbb, Sab per channel ADDED into acc: (6, spp) uint64 on the device, zeroed by the
        caller before the first call (include/oip_c.h: oip_seam_moments_u16; Ws, fs in samples)"""
        self._ck(self.lib.oip_seam_moments_u16(self.h, _ptr(left), _ptr(right), Ws, L, fs, spp, valid_min, valid_max, _ptr(acc)))

    def stitch_balanced_u16(self, left, right, out, Ws, L, fs, spp, gain_q16, offset_q16, feather=0, valid_min=1):
        """the stitch with image 2 balanced by gain_q16 / offset_q16 (spp int32 each, on the device) and blended over
        `feather` pixels either side of the seam (include/oip_c.h: oip_stitch_balanced_u16)"""
        self._ck(self.lib.oip_stitch_balanced_u16(self.h, _ptr(left), _ptr(right), _ptr(out), Ws, L, fs, spp, _ptr(gain_q16), _ptr(offset_q16),
                                                  feather, valid_min))

    def seam_moments_blocks_u16(self, left, right, Ws, L, fs, spp, block_lines, acc, valid_min=0, valid_max=65535):
        """seam_moments_u16 per block of block_lines lines in one launch: the totals of block k ADDED into plane k of acc,
        (max(1, L // block_lines), 6, spp) uint64 on the device, zeroed by the caller (include/oip_c.h:
        oip_seam_moments_blocks_u16)"""
        self._ck(self.lib.oip_seam_moments_blocks_u16(self.h, _ptr(left), _ptr(right), Ws, L, fs, spp, valid_min, valid_max, block_lines,
                                                      _ptr(acc)))

    def stitch_balanced_lines_u16(self, left, right, out, Ws, L, fs, spp, line_gain_q16, line_offset_q16, feather=0, valid_min=1):
        """stitch_balanced_u16 with a gain and an offset per line and channel: (L, spp) int32 tables on the device
        (include/oip_c.h: oip_stitch_balanced_lines_u16)"""
        self._ck(self.lib.oip_stitch_balanced_lines_u16(self.h, _ptr(left), _ptr(right), _ptr(out), Ws, L, fs, spp, _ptr(line_gain_q16),
                                                        _ptr(line_offset_q16), feather, valid_min))

    # -- MTF compensation
    def convolve_u16(self, src, dst, W, L, spp, taps, valid_min=1, src_row0=0, src_rows=None, out_row0=0, out_rows=None):
        """the (ky, kx) Q12 integer taps (host) applied to lines [out_row0, out_row0 + out_rows) of the W x L x spp raster
        whose lines [src_row0, src_row0 + src_rows) are at src; not in place (include/oip_c.h: oip_convolve_u16)"""
        t = np.ascontiguousarray(taps, dtype=np.int32)
        if t.ndim != 2:
            raise ValueError("convolve_u16: a (ky, kx) tap array expected")
        src_rows = L if src_rows is None else src_rows
        out_rows = L if out_rows is None else out_rows
        self._ck(self.lib.oip_convolve_u16(self.h, _ptr(src), src_row0, src_rows, _ptr(dst), out_row0, out_rows, W, L, spp,
                                           t.ctypes.data_as(C.POINTER(C.c_int32)), t.shape[0], t.shape[1], valid_min))

    # -- regfix
    def warp_grid_bicubic_u16(self, src, dst, W, L, spp, nodes_x, nodes_y, gx0, gy0, sx, sy, band_mask=None, src_row0=0, src_rows=None,
                              out_row0=0, out_rows=None):
        """lines [out_row0, out_row0 + out_rows) of the W x L x spp raster whose lines [src_row0, src_row0 + src_rows) are at src,
        resampled (OpenCV-exact bicubic) by the field of the (ny, nx) int32 Q10 node arrays (host) at (gx0 + i sx, gy0 + j sy);
        band_mask: the channels resampled (default: all), the others are copied; not in place (include/oip_c.h:
        oip_warp_grid_bicubic_u16)"""
        x, y = _nodes(nodes_x, nodes_y)
        src_rows = L if src_rows is None else src_rows
        out_rows = L if out_rows is None else out_rows
        band_mask = (1 << spp) - 1 if band_mask is None else band_mask
        self._ck(self.lib.oip_warp_grid_bicubic_u16(self.h, _ptr(src), src_row0, src_rows, _ptr(dst), out_row0, out_rows, W, L, spp, band_mask,
                                                    x.ctypes.data_as(_i32p), y.ctypes.data_as(_i32p), x.shape[1], x.shape[0], gx0, gy0, sx, sy))

    # -- pansharpen
    def pansharpen_sfim_u16(self, pan, mss, low, w, h, dst, max_gain=4, stats=None, out_row0=0, out_rows=None, pan_pitch=None, mss_pitch=None,
                            low_pitch=None, dst_pitch=None):
        """lines [out_row0, out_row0 + out_rows) of the 4 w x 4 h x 4 product fused from the PAN lines under them (pan: the first of
        them), the whole w x h x 4 MSS product and the whole w x h low-resolution PAN (decimate_box_u16, factor 4); dst: the first
        of the lines; stats: None or two uint64 on the device that the counters (UL == 0, gain cut) are added to; pitches in
        samples (include/oip_c.h: oip_pansharpen_sfim_u16)"""
        out_rows = 4 * h - out_row0 if out_rows is None else out_rows
        self._ck(self.lib.oip_pansharpen_sfim_u16(self.h, _ptr(pan), 4 * w if pan_pitch is None else pan_pitch, _ptr(mss),
                                                  4 * w if mss_pitch is None else mss_pitch, _ptr(low), w if low_pitch is None else low_pitch, w, h,
                                                  _ptr(dst), 16 * w if dst_pitch is None else dst_pitch, out_row0, out_rows, max_gain, _ptr(stats)))

    # -- despike
    def despike_u16(self, src, dst, W, L, spp, thr_abs, thr_rel_q8=0, valid_min=1, groups=1, coltab=None, count=None,
                    src_row0=0, src_rows=None, out_row0=0, out_rows=None):
        """column repair (coltab: (W, 2) int32 on the device, or None) and the conditional 3 x 3 median of lines
        [out_row0, out_row0 + out_rows) of the W x L x spp raster whose lines [src_row0, src_row0 + src_rows) are at src; the
        replacements per sample column are ADDED into count ((W * spp,) uint64 on the device, or None); not in place
        (include/oip_c.h: oip_despike_u16)"""
        src_rows = L if src_rows is None else src_rows
        out_rows = L if out_rows is None else out_rows
        self._ck(self.lib.oip_despike_u16(self.h, _ptr(src), src_row0, src_rows, _ptr(dst), out_row0, out_rows, W, L, spp, groups,
                                          _ptr(coltab), thr_abs, thr_rel_q8, valid_min, _ptr(count)))

    # -- denoise
    def sigma_filter_u16(self, src, dst, W, L, spp, radius, thr, min_members=None, valid_min=1, stats=None,
                         src_row0=0, src_rows=None, out_row0=0, out_rows=None):
        """Lee's sigma filter with a pilot estimate over (2 radius + 1)^2 on lines [out_row0, out_row0 + out_rows) of the
        W x L x spp raster whose lines [src_row0, src_row0 + src_rows) are at src; thr: (spp, 256) uint16 on the device, the
        half width of the range per channel and level (value >> 8); min_members defaults to 2 radius + 1; the four counters
        (valid, left alone, members, changed) are ADDED into stats ((4,) uint64 on the device, or None); not in place
        (include/oip_c.h: oip_sigma_filter_u16)"""
        src_rows = L if src_rows is None else src_rows
        out_rows = L if out_rows is None else out_rows
        min_members = 2 * radius + 1 if min_members is None else min_members
        self._ck(self.lib.oip_sigma_filter_u16(self.h, _ptr(src), src_row0, src_rows, _ptr(dst), out_row0, out_rows, W, L, spp, radius,
                                               _ptr(thr), min_members, valid_min, _ptr(stats)))

    # -- noise
    def noise_blocks_u16(self, src, pitch, w, rows, spp, block, level_shift, keys, key_pitch, key_plane_stride=0, valid_min=1,
                         valid_max=65535):
        """one u16 key per block x block block and channel of rows lines of w pixels of spp samples (lines `pitch` samples
        apart) into spp planes of key lines key_pitch keys apart (include/oip_c.h: oip_noise_blocks_u16)"""
        self._ck(self.lib.oip_noise_blocks_u16(self.h, _ptr(src), pitch, w, rows, spp, block, level_shift, valid_min, valid_max, _ptr(keys),
                                               key_pitch, key_plane_stride))

    # -- mask
    def mask_cells_u16(self, src, pitch, w, rows, spp, cell, flags, flag_pitch, counts=None, valid_min=1, sat_level=4095, full_scale=4095,
                       band=(2, 1, 0, 3), bright_q8=77, white_q8=38, hot_q8=20, ndvi_q8=51):
        """one flag byte (NODATA 1, SATURATED 2, CANDIDATE 16) per cell x cell cell of rows lines of w pixels of spp samples
        (lines `pitch` samples apart) into flag lines flag_pitch bytes apart; band: the channel of (blue, green, red, nir); a
        q8 of -1 disables its test; the counters are ADDED into counts ((8,) uint64 on the device, or None)
        (include/oip_c.h: oip_mask_cells_u16)"""
        b = (_i * 4)(*[int(v) for v in band]) if band is not None else None
        self._ck(self.lib.oip_mask_cells_u16(self.h, _ptr(src), pitch, w, rows, spp, cell, valid_min, sat_level, full_scale, b, bright_q8,
                                             white_q8, hot_q8, ndvi_q8, _ptr(flags), flag_pitch, _ptr(counts)))

    def mask_morph_u8(self, flags, flag_pitch, gw, gh, open_radius=1, buffer_radius=2, counts=None):
        """CLOUD 4 = the opening of the CANDIDATE cells by open_radius, BUFFER 8 = what lies within buffer_radius of it, in
        place on the gw x gh grid of flag bytes; counts[5], counts[6] are ADDED into (include/oip_c.h: oip_mask_morph_u8)"""
        self._ck(self.lib.oip_mask_morph_u8(self.h, _ptr(flags), flag_pitch, gw, gh, open_radius, buffer_radius, _ptr(counts)))

    # -- wallis
    def block_moments_u16(self, src, pitch, w, rows, spp, block, acc, acc_pitch, acc_plane_stride, valid_min=1, valid_max=65535):
        """n, S1, S2 of every block x block block and channel of rows lines of w pixels of spp samples (lines `pitch` samples
        apart), STORED into the 3 * spp uint64 planes of acc: entry [(m * spp + c) * acc_plane_stride + j * acc_pitch + i]
        (include/oip_c.h: oip_block_moments_u16)"""
        self._ck(self.lib.oip_block_moments_u16(self.h, _ptr(src), pitch, w, rows, spp, block, valid_min, valid_max, _ptr(acc), acc_pitch,
                                                acc_plane_stride))

    def wallis_apply_u16(self, src, dst, row0, rows, W, L, spp, block, gain_q16, offset_q8, gw, gh, valid_min=1, valid_max=65535, clamp_max=65535,
                         stats=None):
        """the lines [row0, row0 + rows) of a W x L x spp raster through out = clamp((G v + 256 O + 32768) >> 16), G and O
        interpolated between the (gh, gw, spp) int32 nodes on the device; dst may be src; the three counters are ADDED into
        stats ((3,) uint64 on the device, or None) (include/oip_c.h: oip_wallis_apply_u16)"""
        self._ck(self.lib.oip_wallis_apply_u16(self.h, _ptr(src), _ptr(dst), row0, rows, W, L, spp, block, _ptr(gain_q16), _ptr(offset_q8), gw, gh,
                                               valid_min, valid_max, clamp_max, _ptr(stats)))

    # -- mtf
    def mtf_tiles_u16(self, src, pitch, w, rows, spp, axis, rec, rec_pitch, rec_plane_stride=0, contrast_min=200, tv_slack=256, valid_min=1,
                      valid_max=65535):
        """the {status, s, Sc, Num} int32 record of every whole slanted-edge tile and channel of rows lines of w pixels of spp
        samples (lines `pitch` samples apart); axis "x" / 0 or "y" / 1; pitch and plane stride of the records count records
        (include/oip_c.h: oip_mtf_tiles_u16)"""
        self._ck(self.lib.oip_mtf_tiles_u16(self.h, _ptr(src), pitch, w, rows, spp, MTF_AXES.get(axis, axis), contrast_min, tv_slack, valid_min,
                                            valid_max, _ptr(rec), rec_pitch, rec_plane_stride))

    def mtf_esf_u16(self, src, pitch, w, rows, spp, axis, entries, n, esf, s0=None, contrast_min=200, tv_slack=256, valid_min=1, valid_max=65535):
        """the 64 edge-spread sums and 64 counts (uint32) of the n tiles {channel, ty, tx} (int32, on the device) of the same
        window; s0: None or n int32 on the device for sum S0_r (include/oip_c.h: oip_mtf_esf_u16)"""
        self._ck(self.lib.oip_mtf_esf_u16(self.h, _ptr(src), pitch, w, rows, spp, MTF_AXES.get(axis, axis), contrast_min, tv_slack, valid_min,
                                          valid_max, _ptr(entries), n, _ptr(esf), _ptr(s0)))

    # -- instrumentation
    def merge_subimages_be16(self, tiles, out, vparts, hparts, sub_lines, sub_cols):
        """aux_separator.h:341-393 for uncompressed frames: big-endian sub-images -> little-endian stripes"""
        self._ck(self.lib.oip_merge_subimages_be16(self.h, _ptr(tiles), _ptr(out), vparts, hparts, sub_lines, sub_cols))

    def profile_enable(self, on=True):
        self._ck(self.lib.oip_profile_enable(self.h, int(on)))

    def profile_filter(self, name=None):
        """time only the kernels profiled under `name` (None: all)"""
        self._ck(self.lib.oip_profile_filter(self.h, name.encode() if name else None))

    def profile_reset(self):
        self._ck(self.lib.oip_profile_reset(self.h))

    def profile(self):
        out = {}
        n = self.lib.oip_profile_count(self.h)
        for i in range(n):
            name = C.create_string_buffer(128)
            ms, cnt = _d(), _l()
            self._ck(self.lib.oip_profile_get(self.h, i, name, 128, C.byref(ms), C.byref(cnt)))
            out[name.value.decode()] = (ms.value, cnt.value)
        return out
