"""opticalimageprocessor_amd -- MI355X (gfx950) implementation of the
arloan/OpticalImageProcessor hot path (RRC, phase-correlation alignment, bicubic
resampling, strip stitching).

The product is ``lib/liboipgpu.so`` (hand-written HIP kernels behind the C ABI declared in
``include/oip_c.h``) plus the ``oip`` CLI built from ``csrc/oip_main.cpp``.  This Python
package is only a ctypes binding of that C ABI for tests and ``bench.py``; torch is used for
device allocations and ``torch.distributed``, never for arithmetic.  There is no CPU
fallback: loading fails loudly when the library is missing, and ``Context()`` fails when no
gfx950 device is present.
"""
from .capi import (  # noqa: F401
    Context,
    OipError,
    STATUS_NAMES,
    build,
    declared_symbols,
    denoise_thresholds,
    despike_column_table,
    fft_plan_describe,
    corr_route_describe,
    filter_and_fit,
    library_path,
    load_column_list,
    load_library,
    load_rrc_param_file,
    match_grid,
    match_peak,
    match_summary,
    mtf_summary,
    mtf_tile,
    mtf_tv_slack,
    mtfc_design3,
    mtfc_load_kernel,
    mtfc_quantise,
    noise_despike_threshold,
    noise_fit,
    noise_levels,
    overview_levels,
    deflate_stored_bound,
    deflate_stream_host,
    jpeg_interval_host,
    jpeg_worst_bytes,
    pansharpen_geometry,
    polyfit,
    regfix_fill,
    regfix_load_report,
    regfix_smooth,
    remap_shift_src_range,
    rrc_dead_columns,
    rrc_fit_columns,
    seam_fit,
    seam_fit_blocks,
    seam_line_tables,
    stretch_limits,
    stretch_lut_u8,
    stt_mean,
    upsample_operator,
    warp_grid_src_range,
    write_column_list,
    write_rrc_param_file,
    write_jpeg_u8,
    write_tiff_u8,
    align_mss_src_range,
)

__version__ = "1.1"
