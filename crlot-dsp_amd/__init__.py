"""crlot-dsp_amd -- MI355X-native batched STFT -> iSTFT -> OLA engine (Python host binding).

Thin ctypes layer over the C ABI in include/crlot_dsp.h (libcrlot_dsp.so, built
in-tree by __graft_entry__.build()).  PyTorch is used only for device memory and
the current HIP stream.  Names and argument meanings follow the reference's
C++ API (dsp::Framer / WindowLUT / fft::IFftPlan / OLAAccumulator); error codes
map to the reference's exception types: CRLOT_EINVAL -> ValueError
(std::invalid_argument), CRLOT_ERUNTIME / CRLOT_EHIP -> RuntimeError
(std::runtime_error), CRLOT_ENOMEM -> MemoryError (std::bad_alloc),
CRLOT_EUNSUPPORTED -> NotImplementedError.

There is no CPU fallback: if the library cannot be loaded, every entry raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CRLOT_LIB") or os.path.join(HERE, "libcrlot_dsp.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "crlot_dsp.h")

# dsp::WindowType / NormalizationType / BoundaryMode ordinals
HANN, HAMMING, BLACKMAN, RECT, BLACKMAN_HARRIS = range(5)
NORM_NONE, NORM_SUM_TO_ONE, NORM_L2, NORM_OLA_UNITY_GAIN, NORM_OLA_SUM_WSQ = range(5)
ZERO_PAD, DROP, FRAMEQUEUE = 0, 1, 2
# dsp::PadMode (FrameQueue.h:8-12)
PAD_CONSTANT, PAD_REFLECT, PAD_EDGE = 0, 1, 2
# dsp::fft::FftDomain
FFT_REAL, FFT_COMPLEX = 0, 1

# spectrogram features (crlot_features_desc) and the mel scales
FEAT_POWER, FEAT_MAGNITUDE = 0, 1
FEAT_LIN, FEAT_LN, FEAT_LOG10, FEAT_DB = 0, 1, 2, 3
MEL_HTK, MEL_SLANEY = 0, 1

OK, EINVAL, EUNSUPPORTED, EHIP, ENOMEM, ERUNTIME, ERANGE = 0, -1, -2, -3, -4, -5, -6


class PlanDesc(C.Structure):
    """crlot_plan_desc (include/crlot_dsp.h)."""
    _fields_ = [
        ("frame_size", C.c_int32),
        ("hop_size", C.c_int32),
        ("window_type", C.c_int32),
        ("periodic", C.c_int32),
        ("window_norm", C.c_int32),
        ("boundary_mode", C.c_int32),
        ("analysis_window", C.c_int32),
        ("apply_window_inside", C.c_int32),
        ("eps", C.c_float),
        ("ola_gain", C.c_float),
        ("ring_len", C.c_int32),
        ("device", C.c_int32),
        ("center", C.c_int32),
        ("pad_mode", C.c_int32),
    ]


class LaunchInfo(C.Structure):
    """crlot_launch_info (include/crlot_dsp.h): what a plan's last call on a stream launched."""
    _fields_ = [
        ("n_kernels", C.c_int32),
        ("kernels", C.c_int32 * 8),
        ("grid", C.c_int64 * 8),
        ("n_chunks", C.c_int32),
        ("reserved", C.c_int32),
    ]


class OlaConfigC(C.Structure):
    """crlot_ola_config (include/crlot_dsp.h) = dsp::OLAConfig + device."""
    _fields_ = [
        ("sample_rate", C.c_int32),
        ("frame_size", C.c_int64),
        ("hop_size", C.c_int64),
        ("channels", C.c_int64),
        ("eps", C.c_float),
        ("apply_window_inside", C.c_int32),
        ("shadow_ring", C.c_int32),
        ("device", C.c_int32),
    ]


class FeaturesDesc(C.Structure):
    """crlot_features_desc (include/crlot_dsp.h)."""
    _fields_ = [("kind", C.c_int32), ("n_bands", C.c_int32), ("log", C.c_int32), ("floor", C.c_float)]


class ResamplerDesc(C.Structure):
    """crlot_resampler_desc (include/crlot_dsp.h)."""
    _fields_ = [("up", C.c_int32), ("down", C.c_int32), ("zeros", C.c_int32), ("window", C.c_int32),
                ("rolloff", C.c_double), ("beta", C.c_double), ("device", C.c_int32), ("reserved", C.c_int32)]


class ResamplerGeometry(C.Structure):
    """crlot_resampler_geometry (include/crlot_dsp.h)."""
    _fields_ = [("up", C.c_int32), ("down", C.c_int32), ("half_width", C.c_int32), ("taps", C.c_int32),
                ("phase_ok", C.c_int32), ("device", C.c_int32)]


class ResampleLaunch(C.Structure):
    """crlot_resample_launch (include/crlot_dsp.h): a resampler's last launch."""
    _fields_ = [("kernel", C.c_int32), ("threads", C.c_int32), ("grid", C.c_int64), ("tile_outputs", C.c_int64),
                ("tile", C.c_int32), ("groups", C.c_int32), ("taps_padded", C.c_int32), ("lds_table", C.c_int32),
                ("lds_bytes", C.c_int64)]


class HpssDesc(C.Structure):
    """crlot_hpss_desc (include/crlot_dsp.h)."""
    _fields_ = [("win_harm", C.c_int32), ("win_perc", C.c_int32), ("power", C.c_int32), ("reserved", C.c_int32),
                ("margin_harm", C.c_double), ("margin_perc", C.c_double)]


class ConvolverDesc(C.Structure):
    """crlot_convolver_desc (include/crlot_dsp.h)."""
    _fields_ = [("block", C.c_int32), ("n_filters", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32)]


class ConvolverLaunch(C.Structure):
    """crlot_convolver_launch (include/crlot_dsp.h): a convolver's last delay-line launch."""
    _fields_ = [("kernel", C.c_int32), ("threads", C.c_int32), ("grid", C.c_int64), ("n_chunks", C.c_int32),
                ("chunk", C.c_int32), ("tile", C.c_int32), ("reserved", C.c_int32)]


class SconvLaunch(C.Structure):
    """crlot_sconv_launch (include/crlot_dsp.h): what a streaming convolver's last hop launched."""
    _fields_ = [("head_kernel", C.c_int32), ("tail_kernel", C.c_int32), ("head_grid", C.c_int64),
                ("tail_grid", C.c_int64), ("route", C.c_int32), ("tail_pending", C.c_int32)]


class FdafLaunch(C.Structure):
    """crlot_fdaf_launch (include/crlot_dsp.h): what an adaptive filter's last hop launched."""
    _fields_ = [("hop_kernel", C.c_int32), ("update_kernel", C.c_int32), ("constrain_kernel", C.c_int32),
                ("reserved", C.c_int32), ("hop_grid", C.c_int64), ("update_grid", C.c_int64),
                ("constrain_grid", C.c_int64)]


class DenoiseDesc(C.Structure):
    """crlot_denoise_desc (include/crlot_dsp.h)."""
    _fields_ = [("alpha_s", C.c_double), ("alpha_p", C.c_double), ("alpha_d", C.c_double), ("delta", C.c_double),
                ("alpha_dd", C.c_double), ("g_min", C.c_double), ("window", C.c_int32), ("reserved", C.c_int32)]


class DenoiseLaunch(C.Structure):
    """crlot_denoise_launch (include/crlot_dsp.h): what a noise suppressor's last call launched."""
    _fields_ = [("route", C.c_int32), ("n_kernels", C.c_int32), ("kernel", C.c_int32 * 3), ("reserved", C.c_int32),
                ("grid", C.c_int64 * 3)]


class XspecLaunch(C.Structure):
    """crlot_xspec_launch (include/crlot_dsp.h): what a cross-spectrum object's last call launched."""
    _fields_ = [("n_kernels", C.c_int32), ("kernel", C.c_int32 * 3), ("reserved", C.c_int32 * 2),
                ("grid", C.c_int64 * 3)]


class BeamformDesc(C.Structure):
    """crlot_beamform_desc (include/crlot_dsp.h)."""
    _fields_ = [("mics", C.c_int32), ("ref", C.c_int32), ("mode", C.c_int32), ("update_every", C.c_int32),
                ("alpha", C.c_double), ("loading", C.c_double)]


class BeamformLaunch(C.Structure):
    """crlot_beamform_launch (include/crlot_dsp.h): what a beamformer's last call launched."""
    _fields_ = [("n_kernels", C.c_int32), ("kernel", C.c_int32 * 3), ("reserved", C.c_int32 * 2),
                ("grid", C.c_int64 * 3)]


class WpeDesc(C.Structure):
    """crlot_wpe_desc (include/crlot_dsp.h)."""
    _fields_ = [("mics", C.c_int32), ("taps", C.c_int32), ("delay", C.c_int32), ("iterations", C.c_int32),
                ("alpha", C.c_double), ("loading", C.c_double), ("floor", C.c_double)]


class WpeLaunch(C.Structure):
    """crlot_wpe_launch (include/crlot_dsp.h): what a dereverberator's last call launched."""
    _fields_ = [("n_kernels", C.c_int32), ("kernel", C.c_int32 * 4), ("reserved", C.c_int32),
                ("grid", C.c_int64 * 4)]


class FftDesc(C.Structure):
    """crlot_fft_desc (include/crlot_dsp.h)."""
    _fields_ = [("domain", C.c_int32), ("nfft", C.c_int32), ("device", C.c_int32)]


_lib = None


def lib():
    """Load libcrlot_dsp.so (raises if it is missing: no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built; run __graft_entry__.build()")
    # torch ships its own libamdhip64.so.7 and loads it by path; if this library
    # bound /opt/rocm's copy first, the process would hold two HIP runtimes
    # that do not share devices, streams or allocations.  Load torch's first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    fp = C.POINTER(C.c_float)
    sig = {
        "crlot_last_error": ([], C.c_char_p),
        "crlot_abi_version": ([], C.c_int),
        "crlot_build_info": ([], C.c_char_p),
        "crlot_plan_create": ([C.POINTER(PlanDesc), C.POINTER(vp)], C.c_int),
        "crlot_plan_destroy": ([vp], None),
        "crlot_plan_upload_tables": ([vp, vp, vp], C.c_int),
        "crlot_plan_set_spectral_gain": ([vp, vp], C.c_int),
        "crlot_plan_upload_tables_async": ([vp, vp, vp, vp], C.c_int),
        "crlot_plan_set_spectral_gain_async": ([vp, vp, vp], C.c_int),
        "crlot_plan_set_frame_pairing": ([vp, i32], C.c_int),
        "crlot_plan_set_chunks": ([vp, i32], C.c_int),
        "crlot_set_call_speculation": ([i32], C.c_int),
        "crlot_call_speculation_stats": ([C.POINTER(i64)], C.c_int),
        "crlot_call_speculation_stats_ex": ([C.POINTER(i64), i32], C.c_int),
        "crlot_call_batch_capacity": ([C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "crlot_test_inject": ([i32, i32], C.c_int),
        "crlot_plan_last_launch": ([vp, vp, C.POINTER(LaunchInfo)], C.c_int),
        "crlot_kernel_name": ([i32], C.c_char_p),
        "crlot_plan_info": ([vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)], C.c_int),
        "crlot_frame_count": ([vp, i64], i64),
        "crlot_output_length": ([vp, i64], i64),
        "crlot_workspace_bytes": ([vp, i32, i64], i64),
        "crlot_plan_reserve": ([vp, i64], C.c_int),
        "crlot_roundtrip": ([vp, vp, vp, i32, i64, i64, i64, vp], C.c_int),
        "crlot_roundtrip_stages": ([vp, vp, i32, i64, i64, vp, vp, vp], C.c_int),
        "crlot_ola_gather": ([vp, vp, vp, i32, i64, i64, i64, vp], C.c_int),
        "crlot_rfft_batched": ([vp, vp, vp, i32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_irfft_batched": ([vp, vp, vp, i32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_plan_set_spectral_mask": ([vp, vp, i64, i64], C.c_int),
        "crlot_stft": ([vp, vp, vp, i32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_istft_ola": ([vp, vp, vp, i32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_stretch_frame_count": ([i64, C.c_double], i64),
        "crlot_stretch_output_length": ([vp, i64, C.c_double], i64),
        "crlot_phase_vocoder": ([vp, vp, vp, i32, i64, C.c_double, i64, i64, i64, i64, vp], C.c_int),
        "crlot_time_stretch": ([vp, vp, vp, i32, i64, C.c_double, i64, i64, vp], C.c_int),
        "crlot_gl_project": ([vp, vp, vp, vp, vp, i32, i64, C.c_double, i64, i64, i64, i64, i64, i64, i64, i64, vp],
                             C.c_int),
        "crlot_griffin_lim": ([vp, vp, i64, i64, vp, i64, i64, vp, i64, i32, i64, i32, C.c_double, vp], C.c_int),
        "crlot_hpss_masks": ([vp, C.POINTER(HpssDesc), vp, vp, vp, i32, i64, i64, i64, i64, i64, i64, i64, vp], C.c_int),
        "crlot_hpss": ([vp, C.POINTER(HpssDesc), vp, vp, vp, i32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_convolver_create": ([C.POINTER(ConvolverDesc), fp, i64, i64, C.POINTER(vp)], C.c_int),
        "crlot_convolver_destroy": ([vp], None),
        "crlot_convolver_info": ([vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i32)], C.c_int),
        "crlot_convolver_prepare": ([vp], C.c_int),
        "crlot_convolver_spectra": ([vp, fp], C.c_int),
        "crlot_convolver_plan": ([vp], vp),
        "crlot_convolve_output_length": ([vp, i64], i64),
        "crlot_convolver_set_chunks": ([vp, i32], C.c_int),
        "crlot_convolver_last_launch": ([vp, C.POINTER(ConvolverLaunch)], C.c_int),
        "crlot_fdl_mac": ([vp, vp, vp, i32, i64, i64, i64, i64, i64, i64, vp], C.c_int),
        "crlot_convolve": ([vp, vp, vp, i32, i64, i64, i64, vp], C.c_int),
        "crlot_stream_convolver_create": ([vp, i32, C.POINTER(vp)], C.c_int),
        "crlot_stream_convolver_destroy": ([vp], None),
        "crlot_stream_convolver_prepare": ([vp], C.c_int),
        "crlot_stream_convolver_state_bytes": ([vp], i64),
        "crlot_stream_convolver_reset": ([vp], C.c_int),
        "crlot_stream_convolver_set_layout": ([vp, i32], C.c_int),
        "crlot_stream_convolver_set_route": ([vp, i32], C.c_int),
        "crlot_stream_convolver_set_prefetch": ([vp, i32], C.c_int),
        "crlot_stream_convolver_info": ([vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)], C.c_int),
        "crlot_stream_convolver_last_launch": ([vp, C.POINTER(SconvLaunch)], C.c_int),
        "crlot_stream_convolve_hop": ([vp, vp, vp, vp], C.c_int),
        "crlot_stream_convolve_prefetch": ([vp, vp], C.c_int),
        "crlot_fdaf_create": ([i32, i64, i32, C.POINTER(vp)], C.c_int),
        "crlot_fdaf_destroy": ([vp], None),
        "crlot_fdaf_prepare": ([vp], C.c_int),
        "crlot_fdaf_state_bytes": ([vp], i64),
        "crlot_fdaf_reset": ([vp], C.c_int),
        "crlot_fdaf_set_layout": ([vp, i32], C.c_int),
        "crlot_fdaf_info": ([vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i32), C.POINTER(i64)],
                            C.c_int),
        "crlot_fdaf_last_launch": ([vp, C.POINTER(FdafLaunch)], C.c_int),
        "crlot_fdaf_set_step": ([vp, C.c_double, C.c_double, C.c_double], C.c_int),
        "crlot_fdaf_set_constraint": ([vp, i32], C.c_int),
        "crlot_fdaf_set_adapt": ([vp, i32], C.c_int),
        "crlot_fdaf_set_taps": ([vp, fp, i32, i64], C.c_int),
        "crlot_fdaf_get_taps": ([vp, fp, i64], C.c_int),
        "crlot_fdaf_state": ([vp] + [C.POINTER(vp)] * 6, C.c_int),
        "crlot_fdaf_hop": ([vp, vp, vp, vp, vp, vp], C.c_int),
        "crlot_fdaf_constrain": ([vp, i32, vp], C.c_int),
        "crlot_denoise_desc_default": ([C.POINTER(DenoiseDesc)], C.c_int),
        "crlot_denoiser_create": ([vp, C.POINTER(DenoiseDesc), i32, C.POINTER(vp)], C.c_int),
        "crlot_denoiser_destroy": ([vp], None),
        "crlot_denoiser_prepare": ([vp], C.c_int),
        "crlot_denoiser_reset": ([vp], C.c_int),
        "crlot_denoiser_info": ([vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)],
                                C.c_int),
        "crlot_denoiser_state": ([vp, C.POINTER(vp)], C.c_int),
        "crlot_denoiser_set_route": ([vp, i32], C.c_int),
        "crlot_denoiser_last_launch": ([vp, C.POINTER(DenoiseLaunch)], C.c_int),
        "crlot_denoise_gains": ([vp, vp, vp, i32, i64, i64, i64, i64, i64, i32, vp], C.c_int),
        "crlot_denoise": ([vp, vp, vp, i32, i64, i64, i64, vp], C.c_int),
        "crlot_stream_denoise_hop": ([vp, vp, vp, vp, C.POINTER(i32), vp], C.c_int),
        "crlot_xspec_create": ([vp, i32, C.c_double, C.POINTER(vp)], C.c_int),
        "crlot_xspec_destroy": ([vp], None),
        "crlot_xspec_prepare": ([vp], C.c_int),
        "crlot_xspec_reset": ([vp], C.c_int),
        "crlot_xspec_info": ([vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), fp, fp], C.c_int),
        "crlot_xspec_state": ([vp, C.POINTER(vp)], C.c_int),
        "crlot_xspec_last_launch": ([vp, C.POINTER(XspecLaunch)], C.c_int),
        "crlot_xspec_accumulate": ([vp, vp, vp, i32, i64, i64, i64, i64, i64, i32, vp, vp], C.c_int),
        "crlot_xspec_derive": ([vp, vp, i32, i32, vp, i64, vp, i64, vp, i64, vp], C.c_int),
        "crlot_xspec_peak": ([vp, vp, i64, i32, i32, vp, i64, vp], C.c_int),
        "crlot_xspec_estimate": ([vp, vp, vp, i32, i64, i64, i64, i32, vp, vp], C.c_int),
        "crlot_xspec_delay": ([vp, vp, i32, i32, i32, vp, i64, vp], C.c_int),
        "crlot_beamform_desc_default": ([C.POINTER(BeamformDesc)], C.c_int),
        "crlot_beamformer_create": ([vp, C.POINTER(BeamformDesc), i32, C.POINTER(vp)], C.c_int),
        "crlot_beamformer_destroy": ([vp], None),
        "crlot_beamformer_prepare": ([vp], C.c_int),
        "crlot_beamformer_reset": ([vp], C.c_int),
        "crlot_beamformer_info": ([vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), fp, fp, fp],
                                  C.c_int),
        "crlot_beamformer_state": ([vp, C.POINTER(vp)], C.c_int),
        "crlot_beamformer_weights": ([vp, C.POINTER(vp)], C.c_int),
        "crlot_beamformer_steering": ([vp, C.POINTER(vp)], C.c_int),
        "crlot_beamformer_last_launch": ([vp, C.POINTER(BeamformLaunch)], C.c_int),
        "crlot_beamform_accumulate": ([vp, vp, i64, i64, vp, i64, i64, i32, i64, i32, i32, vp, vp], C.c_int),
        "crlot_beamform_solve": ([vp, vp, vp, i32, vp, vp], C.c_int),
        "crlot_beamform_apply": ([vp, vp, i64, i64, vp, i32, i64, vp, i64, i64, vp], C.c_int),
        "crlot_beamform": ([vp, vp, i64, vp, i64, i64, vp, i64, i32, i64, vp], C.c_int),
        "crlot_stream_beamform_hop": ([vp, vp, vp, vp, vp, i64, vp, C.POINTER(i32), vp], C.c_int),
        "crlot_wpe_desc_default": ([C.POINTER(WpeDesc)], C.c_int),
        "crlot_wpe_create": ([vp, C.POINTER(WpeDesc), i32, C.POINTER(vp)], C.c_int),
        "crlot_wpe_destroy": ([vp], None),
        "crlot_wpe_prepare": ([vp], C.c_int),
        "crlot_wpe_reset": ([vp], C.c_int),
        "crlot_wpe_info": ([vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32),
                            C.POINTER(i32), C.POINTER(i64), fp, fp, fp], C.c_int),
        "crlot_wpe_state": ([vp, C.POINTER(vp)], C.c_int),
        "crlot_wpe_inv_cov": ([vp, C.POINTER(vp)], C.c_int),
        "crlot_wpe_taps": ([vp, C.POINTER(vp)], C.c_int),
        "crlot_wpe_last_launch": ([vp, C.POINTER(WpeLaunch)], C.c_int),
        "crlot_wpe_power": ([vp, vp, i64, i64, i32, i64, i64, vp, i64, i64, vp], C.c_int),
        "crlot_wpe_accumulate": ([vp, vp, i64, i64, vp, i64, i64, i32, i64, i64, i32, vp, vp], C.c_int),
        "crlot_wpe_solve": ([vp, vp, i32, vp, vp], C.c_int),
        "crlot_wpe_filter": ([vp, vp, i64, i64, vp, i32, i64, i64, vp, i64, i64, vp], C.c_int),
        "crlot_wpe_rls": ([vp, vp, i64, i64, i64, i64, vp, i64, i64, vp], C.c_int),
        "crlot_wpe": ([vp, vp, i64, vp, i64, i32, i64, vp], C.c_int),
        "crlot_stream_wpe_hop": ([vp, vp, vp, vp, vp, C.POINTER(i32), vp], C.c_int),
        "crlot_resample_geometry": ([C.POINTER(ResamplerDesc), C.POINTER(ResamplerGeometry)], C.c_int),
        "crlot_resample_table_host": ([C.POINTER(ResamplerDesc), fp], C.c_int),
        "crlot_rational_approx": ([C.c_double, i32, C.POINTER(i32), C.POINTER(i32)], C.c_int),
        "crlot_resampler_create": ([C.POINTER(ResamplerDesc), C.POINTER(vp)], C.c_int),
        "crlot_resampler_destroy": ([vp], None),
        "crlot_resampler_info": ([vp, C.POINTER(ResamplerGeometry)], C.c_int),
        "crlot_resampler_table": ([vp, fp], C.c_int),
        "crlot_resampler_prepare": ([vp], C.c_int),
        "crlot_resample_output_length": ([vp, i64], i64),
        "crlot_resampler_set_route": ([vp, i32], C.c_int),
        "crlot_resampler_set_tile": ([vp, i32], C.c_int),
        "crlot_resampler_last_launch": ([vp, C.POINTER(ResampleLaunch)], C.c_int),
        "crlot_resample": ([vp, vp, vp, i32, i64, i64, i64, vp], C.c_int),
        "crlot_pitch_shift": ([vp, vp, vp, vp, i32, i64, i64, i64, vp], C.c_int),
        "crlot_features_create": ([vp, C.POINTER(FeaturesDesc), vp, C.POINTER(vp)], C.c_int),
        "crlot_features_destroy": ([vp], None),
        "crlot_features_info": ([vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)], C.c_int),
        "crlot_spectrogram": ([vp, vp, vp, i32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_mel_filterbank": ([i32, i32, C.c_double, C.c_double, C.c_double, i32, i32, fp], C.c_int),
        "crlot_filterbank_spans": ([fp, i32, i32, C.POINTER(i32), C.POINTER(i32)], C.c_int),
        "crlot_fft_plan_create": ([C.POINTER(FftDesc), C.POINTER(vp)], C.c_int),
        "crlot_fft_plan_destroy": ([vp], None),
        "crlot_fft_plan_info": ([vp, C.POINTER(i32), C.POINTER(i32)], C.c_int),
        "crlot_fft_forward": ([vp, vp, vp, i32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_fft_inverse": ([vp, vp, vp, i32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_fft_forward_complex": ([vp, vp, vp, i32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_fft_inverse_complex": ([vp, vp, vp, i32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_roundtrip_interleaved": ([vp, vp, vp, i32, i32, i64, i64, i64, vp], C.c_int),
        "crlot_stream_create": ([vp, i32, C.POINTER(vp)], C.c_int),
        "crlot_stream_destroy": ([vp], None),
        "crlot_stream_reset": ([vp], C.c_int),
        "crlot_stream_push_hop": ([vp, vp, vp, C.POINTER(i32), vp], C.c_int),
        "crlot_stream_stft_hop": ([vp, vp, vp, i64, C.POINTER(i32), vp], C.c_int),
        "crlot_stream_istft_hop": ([vp, vp, i64, vp, i64, vp, vp], C.c_int),
        "crlot_stream_push_hop_masked": ([vp, vp, vp, i64, vp, C.POINTER(i32), vp], C.c_int),
        "crlot_stream_features_hop": ([vp, vp, vp, vp, i64, vp, i64, C.POINTER(i32), vp], C.c_int),
        "crlot_stream_set_layout": ([vp, i32], C.c_int),
        "crlot_stream_rt_create": ([vp, i32, i32, i32, C.POINTER(vp)], C.c_int),
        "crlot_stream_rt_destroy": ([vp], None),
        "crlot_stream_rt_reset": ([vp], C.c_int),
        "crlot_stream_rt_push_hop": ([vp, vp, vp, C.POINTER(i32)], C.c_int),
        "crlot_stream_rt_input_slot": ([vp], vp),
        "crlot_stream_rt_submit": ([vp, C.POINTER(i64)], C.c_int),
        "crlot_stream_rt_wait": ([vp, i64, C.POINTER(vp), C.POINTER(i32)], C.c_int),
        "crlot_stream_rt_info": ([vp, C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(i32)], C.c_int),
        "crlot_stream_rt_set_idle_timeout": ([vp, C.c_double, C.c_double], C.c_int),
        "crlot_wav_reader_open": ([C.c_char_p, C.POINTER(vp)], C.c_int),
        "crlot_wav_reader_close": ([vp], None),
        "crlot_wav_reader_info": ([vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(i32)],
                                  C.c_int),
        "crlot_wav_reader_read": ([vp, fp, C.c_uint64, C.POINTER(C.c_uint64)], C.c_int),
        "crlot_wav_writer_open": ([C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, i32,
                                   C.POINTER(vp)], C.c_int),
        "crlot_wav_writer_write": ([vp, fp, C.c_uint64, C.POINTER(C.c_uint64)], C.c_int),
        "crlot_wav_writer_close": ([vp], C.c_int),
        "crlot_framer_create": ([C.POINTER(vp)], C.c_int),
        "crlot_framer_destroy": ([vp], None),
        "crlot_framer_set_params": ([vp, i64, i64, i64, i32], C.c_int),
        "crlot_framer_push": ([vp, vp, i64], C.c_int),
        "crlot_framer_pop": ([vp, vp], C.c_int),
        "crlot_framer_available": ([vp], i64),
        "crlot_framer_reset": ([vp], C.c_int),
        "crlot_framer_info": ([vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32),
                               C.POINTER(i64)], C.c_int),
        "crlot_ola_create": ([C.POINTER(OlaConfigC), C.POINTER(vp)], C.c_int),
        "crlot_ola_destroy": ([vp], None),
        "crlot_ola_set_window": ([vp, vp, i32], C.c_int),
        "crlot_ola_add_frame_soa": ([vp, vp, vp, i64, i64, i64, f32], C.c_int),
        "crlot_ola_push_frame_aos": ([vp, vp, vp, i64, i64, i64, f32], C.c_int),
        "crlot_ola_produce": ([vp, vp, i64, C.POINTER(i64)], C.c_int),
        "crlot_ola_add_frame_soa_device": ([vp, vp, i64, vp, i64, i64, i64, f32, vp], C.c_int),
        "crlot_ola_push_frame_aos_device": ([vp, vp, vp, i64, i64, i64, f32, vp], C.c_int),
        "crlot_ola_produce_device": ([vp, vp, i64, i64, C.POINTER(i64), vp], C.c_int),
        "crlot_ola_flush": ([vp], C.c_int),
        "crlot_ola_reset": ([vp], C.c_int),
        "crlot_ola_info": ([vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)],
                           C.c_int),
        "crlot_ola_meter_peak": ([vp, C.POINTER(f32)], C.c_int),
        "crlot_ola_norm_table": ([vp, fp], C.c_int),
        "crlot_ola_synchronize": ([vp], C.c_int),
        "crlot_fft_forward_host": ([vp, vp, vp, i32, i64, i64, i64, i64], C.c_int),
        "crlot_fft_inverse_host": ([vp, vp, vp, i32, i64, i64, i64, i64], C.c_int),
        "crlot_fft_forward_complex_host": ([vp, vp, vp, i32, i64, i64, i64, i64], C.c_int),
        "crlot_fft_inverse_complex_host": ([vp, vp, vp, i32, i64, i64, i64, i64], C.c_int),
        "crlot_axpy": ([vp, vp, f32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_axpy_windowed": ([vp, vp, vp, f32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_normalize_and_clear": ([vp, vp, vp, f32, i64, i64, i64, i64, vp], C.c_int),
        "crlot_call_axpy": ([vp, vp, f32, i64], C.c_int),
        "crlot_call_axpy_windowed": ([vp, vp, vp, f32, i64], C.c_int),
        "crlot_call_normalize_and_clear": ([vp, vp, vp, f32, i64], C.c_int),
        "crlot_framequeue_count": ([i64, i64, i64, i32], i64),
        "crlot_framequeue_frames": ([vp, i32, i64, i64, i64, i64, i32, i32, vp, vp], C.c_int),
        "crlot_framequeue_create": ([vp, i64, i64, i64, i32, i32, i32, C.POINTER(vp)], C.c_int),
        "crlot_framequeue_destroy": ([vp], None),
        "crlot_framequeue_info": ([vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "crlot_framequeue_frame": ([vp, i64], vp),
        "crlot_framequeue_copy_frame": ([vp, i64, vp], C.c_int),
        "crlot_framequeue_all_frames": ([vp], vp),
        "crlot_framequeue_device_frames": ([vp], vp),
        "crlot_plan_reserve_stream": ([vp, i32, i64, i32, vp], C.c_int),
        "crlot_window_table": ([i32, i64, i32, i32, fp], C.c_int),
        "crlot_ring_len": ([i64, i64], i64),
        "crlot_norm_table": ([fp, i64, i64, i64, i32, f32, fp], C.c_int),
    }
    for name, (argt, rest) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = argt
        fn.restype = rest
    _lib = L
    return L


def build_info() -> dict:
    """What the loaded library was built from (crlot_build_info): {"src": the
    source hash baked in at build time, "arch": ...}."""
    parts = dict(p.split(":", 1) for p in lib().crlot_build_info().decode().split())
    return {"src": parts.get("src"), "arch": parts.get("arch"), "path": LIB_PATH}


def set_call_speculation(mode: int):
    """1: per-call speculation of the call kernel only; 2 (default): the whole
    per-frame drop-in loop batched on the device as well (crlot_set_call_speculation)."""
    _check(lib().crlot_set_call_speculation(int(mode)), "crlot_set_call_speculation")


def call_speculation_stats() -> dict:
    """Process-wide counters of the batched speculation (crlot_call_speculation_stats)."""
    v = (C.c_int64 * 6)()
    _check(lib().crlot_call_speculation_stats(v), "crlot_call_speculation_stats")
    return dict(zip(("batches", "forwards", "inverses", "pushes", "produces", "rebuilds"), list(v)))


SPEC_STATS = ("batches", "forwards", "inverses", "pushes", "produces", "rebuilds", "frames", "windows", "declined",
              "gains", "gain_backoffs")


def call_speculation_stats_ex() -> dict:
    """All counters of the batched speculation (crlot_call_speculation_stats_ex):
    the six above plus frames transformed by batch chains, window continuations and
    declined speculations."""
    v = (C.c_int64 * len(SPEC_STATS))()
    _check(lib().crlot_call_speculation_stats_ex(v, len(SPEC_STATS)), "crlot_call_speculation_stats_ex")
    return dict(zip(SPEC_STATS, list(v)))


def call_batch_capacity() -> dict:
    """Bounds of the batched speculation (crlot_call_batch_capacity): frames per
    window, device / pinned bytes held now, pinned peak since load."""
    v = [C.c_int64() for _ in range(4)]
    _check(lib().crlot_call_batch_capacity(*[C.byref(x) for x in v]), "crlot_call_batch_capacity")
    return dict(zip(("window_frames", "device_bytes", "pinned_bytes", "pinned_peak"), [x.value for x in v]))


INJECT_BATCH_ALLOC = 1
INJECT_CALL_TIMEOUT = 2


def test_inject(what: int, count: int):
    """Test-only fault injection (crlot_test_inject): INJECT_BATCH_ALLOC fails the
    next `count` buffer allocations of the batched speculation."""
    _check(lib().crlot_test_inject(int(what), int(count)), "crlot_test_inject")


def kernel_name(kernel_id: int) -> str:
    """Name of a CRLOT_K_* launch-record id (crlot_kernel_name)."""
    return lib().crlot_kernel_name(int(kernel_id)).decode()


def _check(rc: int, what: str = "") -> int:
    if rc >= 0:
        return rc
    msg = lib().crlot_last_error().decode(errors="replace")
    msg = f"{what}: {msg}" if what else msg
    if rc == EINVAL:
        raise ValueError(msg)
    if rc == EUNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == ENOMEM:
        raise MemoryError(msg)
    if rc == ERANGE:
        raise IndexError(msg)
    raise RuntimeError(msg)


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ----------------------------------------------------------------- host tables
def window_table(wtype: int, n: int, periodic: bool = False, norm: int = NORM_NONE) -> np.ndarray:
    """WindowLUT(n, type, periodic, norm).data() (WindowLUT.cc:215-388)."""
    out = np.zeros(max(n, 1), np.float32)
    _check(lib().crlot_window_table(wtype, n, int(periodic), norm, _fptr(out)), "window")
    return out[:n]


def ring_len(frame_size: int, hop: int) -> int:
    return _check(int(lib().crlot_ring_len(frame_size, hop)), "ring_len")


def norm_table(window, frame_size: int, hop: int, ring: int | None = None,
               apply_window_inside: bool = True, eps: float = 1e-8) -> np.ndarray:
    ring = ring_len(frame_size, hop) if ring is None else ring
    out = np.zeros(ring, np.float32)
    w = None if window is None else np.ascontiguousarray(window, np.float32)
    _check(lib().crlot_norm_table(None if w is None else _fptr(w), frame_size, hop, ring,
                                  int(apply_window_inside), eps, _fptr(out)), "norm")
    return out


def header_symbols() -> list[str]:
    """Every function the C header declares (for the ABI-surface test)."""
    import re
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(crlot_[a-z0-9_]+)\s*\(", txt)))


# ----------------------------------------------------------------- device plan
def _torch():
    import torch
    return torch


def _ld(t, dim: int, minimum: int) -> int:
    """Leading dimension of `t` along `dim`; a size-1 dim's stride is meaningless
    (numpy/torch may report 0), so use the dense value there."""
    return int(t.stride(dim)) if t.shape[dim] > 1 else int(minimum)


def mask_layout(shape, strides, dtype: str, device_index, plan_device: int, bins: int):
    """Validate a spectral mask from its plain description -- shape and strides (in
    elements) as tuples, dtype name, device index (None: not a device tensor) -- for a
    plan on `plan_device` with `bins` = N/2+1.  Returns (ld_frame, ld_stream,
    (S_mask or None, F_mask)): the leading dimensions the kernels index with and the
    extent later calls are checked against.  S_mask is None when one set of rows
    serves every stream: a (F, bins) mask, or (1, F, bins), whose stream stride is 0.
    Everything the kernels would read out of bounds is refused here."""
    shape, strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
    if len(shape) not in (2, 3) or len(strides) != len(shape) or shape[-1] != bins or strides[-1] != 1:
        raise ValueError("mask must be a (S, F, N/2+1) or (F, N/2+1) device tensor with contiguous rows")
    if dtype != "float32":
        raise ValueError(f"mask must be float32, not {dtype}")
    if device_index is None or int(device_index) != int(plan_device):
        raise ValueError(f"mask must live on the plan's device {plan_device}, not "
                         f"{'the host' if device_index is None else device_index}")
    if min(shape) < 1:
        raise ValueError("mask has an empty dimension")
    F_mask = shape[-2]
    # a size-1 dim's stride is meaningless: the dense value there
    ld_frame = strides[-2] if F_mask > 1 else bins
    if ld_frame < 0 or strides[0] < 0:
        raise ValueError("mask strides must not be negative")
    if len(shape) == 2 or shape[0] == 1:
        return ld_frame, 0, (None, F_mask)
    return ld_frame, strides[0], (shape[0], F_mask)


def check_mask_extent(extent, n_streams: int, n_frames: int, what: str = "call"):
    """Raise ValueError when the stored mask (extent = (S_mask or None, F_mask) from
    mask_layout, None: no mask) has fewer frames or streams than a call of
    n_streams x n_frames reads."""
    if extent is None:
        return
    s_mask, f_mask = extent
    if n_frames > f_mask:
        raise ValueError(f"{what}: the spectral mask has {f_mask} frames, the call has {n_frames}")
    if s_mask is not None and n_streams > s_mask:
        raise ValueError(f"{what}: the spectral mask has {s_mask} streams, the call has {n_streams}")


def stretch_frame_count(F: int, rate: float) -> int:
    """Frames a phase-vocoder stretch of F frames at `rate` gives: the number of
    t >= 0 with t * rate < F (crlot_stretch_frame_count; rate in [1/64, 64])."""
    return _check(int(lib().crlot_stretch_frame_count(int(F), float(rate))), "crlot_stretch_frame_count")


def _stretch_spec_layout(shape, strides, dtype: str, device_index, plan_device: int, bins: int, what: str = "spec",
                         expect=None):
    """Validate a spectra tensor of Plan.phase_vocoder from its plain description
    (shape and strides in complex elements as tuples, dtype name, device index or
    None for a host tensor): (S, F, bins) complex64 on the plan's device, rows
    contiguous and at least `bins` elements (N+2 floats) apart; `expect`: the exact
    shape an output must have.  Returns (ld_spec, ld_frame) in floats."""
    shape, strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
    if len(shape) != 3 or len(strides) != 3 or shape[2] != bins:
        raise ValueError(f"{what} must be (S, F, N/2+1) or (F, N/2+1) complex64")
    if expect is not None and shape != tuple(expect):
        raise ValueError(f"{what} must be {tuple(expect)}, not {shape}")
    if dtype != "complex64":
        raise ValueError(f"{what} must be complex64, not {dtype}")
    if device_index is None or int(device_index) != int(plan_device):
        raise ValueError(f"{what} must live on the plan's device {plan_device}, not "
                         f"{'the host' if device_index is None else device_index}")
    if strides[2] != 1:
        raise ValueError(f"{what} must have contiguous rows")
    S, F = shape[0], shape[1]
    # a size-1 dim's stride is meaningless: the dense value there
    ld_frame = strides[1] if F > 1 else bins
    ld_spec = strides[0] if S > 1 else max(F, 1) * ld_frame
    if ld_frame < bins:
        raise ValueError(f"{what} rows overlap: ld_frame < N+2 floats")
    if S > 1 and ld_spec < (F - 1) * ld_frame + bins:
        raise ValueError(f"{what} streams overlap: ld_spec too small")
    return 2 * ld_spec, 2 * ld_frame


def _gl_mag_layout(shape, strides, dtype: str, device_index, plan_device: int, bins: int, what: str = "mag",
                   expect=None):
    """Validate a magnitude tensor of Plan.gl_project / Plan.griffin_lim from its
    plain description (shape and strides in elements as tuples, dtype name, device
    index or None for a host tensor): (S, F, bins) float32 on the plan's device, rows
    contiguous and at least `bins` apart, streams not overlapping; `expect`: the
    (S, F, bins) it must have.  Returns (S, F, ld_mag, ld_frame)."""
    shape, strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
    if len(shape) != 3 or len(strides) != 3 or shape[2] != bins:
        raise ValueError(f"{what} must be (S, F, N/2+1) or (F, N/2+1) float32")
    if expect is not None and shape != tuple(expect):
        raise ValueError(f"{what} must be {tuple(expect)}, not {shape}")
    if dtype != "float32":
        raise ValueError(f"{what} must be float32, not {dtype}")
    if device_index is None or int(device_index) != int(plan_device):
        raise ValueError(f"{what} must live on the plan's device {plan_device}, not "
                         f"{'the host' if device_index is None else device_index}")
    if strides[2] != 1:
        raise ValueError(f"{what} must have contiguous rows")
    S, F = shape[0], shape[1]
    # a size-1 dim's stride is meaningless: the dense value there
    ld_frame = strides[1] if F > 1 else bins
    ld_mag = strides[0] if S > 1 else max(F, 1) * ld_frame
    if ld_frame < bins:
        raise ValueError(f"{what} rows overlap: ld_frame < N/2+1")
    if S > 1 and ld_mag < (F - 1) * ld_frame + bins:
        raise ValueError(f"{what} streams overlap: the stream stride is too small")
    return S, F, ld_mag, ld_frame


def _gl_y_layout(shape, strides, dtype: str, device_index, plan_device: int, S: int, L: int):
    """The same for Plan.griffin_lim's output: (S, >= L) float32 on the plan's
    device, rows contiguous and not overlapping.  Returns ld_y."""
    shape, strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
    if len(shape) != 2 or len(strides) != 2 or shape[0] != S or shape[1] < L:
        raise ValueError(f"y must be ({S}, >= {L})")
    if dtype != "float32":
        raise ValueError(f"y must be float32, not {dtype}")
    if device_index is None or int(device_index) != int(plan_device):
        raise ValueError(f"y must live on the plan's device {plan_device}, not "
                         f"{'the host' if device_index is None else device_index}")
    if shape[1] > 1 and strides[1] != 1:
        raise ValueError("y must have contiguous rows")
    ld_y = strides[0] if S > 1 else max(L, 1)
    if S > 1 and ld_y < L:
        raise ValueError("y rows overlap: the stream stride is below F * H")
    return ld_y


def _gl_scalars(n_iter: int, momentum: float):
    """n_iter in [0, 65536] and a finite momentum in [0, 1), else ValueError."""
    if int(n_iter) != n_iter or not 0 <= int(n_iter) <= 65536:
        raise ValueError("n_iter must be an integer in [0, 65536]")
    m = float(momentum)
    if not (m == m and 0.0 <= m < 1.0):
        raise ValueError("momentum must be finite and in [0, 1)")
    return int(n_iter), m


HPSS_HARD = -1  # crlot_hpss_desc.power: the hard masks (librosa's power = inf)


def _hpss_desc(kernel_size=31, power=2, margin=1.0) -> HpssDesc:
    """Plan.hpss / Plan.hpss_masks's scalars as a crlot_hpss_desc: kernel_size and
    margin a scalar or a (harm, perc) pair as in librosa; windows odd in [1, 63];
    power 1, 2 or inf (HPSS_HARD); margins finite and >= 1.  ValueError otherwise."""
    def pair(v, what):
        if isinstance(v, (tuple, list)):
            if len(v) != 2:
                raise ValueError(f"{what} must be a scalar or a (harm, perc) pair")
            return v[0], v[1]
        return v, v
    wins = pair(kernel_size, "kernel_size")
    for w in wins:
        if isinstance(w, bool) or int(w) != w or not 1 <= int(w) <= 63 or int(w) % 2 == 0:
            raise ValueError("kernel_size must be odd and in [1, 63]")
    margins = tuple(float(m) for m in pair(margin, "margin"))
    for m in margins:
        if not (m == m and 1.0 <= m < float("inf")):
            raise ValueError("margin must be finite and >= 1")
    if power == float("inf") or power == HPSS_HARD:
        pw = HPSS_HARD
    elif power in (1, 2):
        pw = int(power)
    else:
        raise ValueError("power must be 1, 2 or inf")
    return HpssDesc(int(wins[0]), int(wins[1]), pw, 0, margins[0], margins[1])


def _tensors_overlap(a, b) -> bool:
    """Do the address ranges of two tensors (first to last element) intersect."""
    def span(t):
        last = sum((int(n) - 1) * int(st) for n, st in zip(t.shape, t.stride()))
        return int(t.data_ptr()), int(t.data_ptr()) + (last + 1) * int(t.element_size())
    if a.numel() == 0 or b.numel() == 0:
        return False
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def _stream_handle(tensor) -> int:
    torch = _torch()
    return int(torch.cuda.current_stream(tensor.device).cuda_stream)


@dataclass
class PlanConfig:
    frame_size: int = 1024
    hop_size: int = 256
    window_type: int = HANN
    periodic: bool = False
    window_norm: int = NORM_NONE
    boundary_mode: int = ZERO_PAD
    analysis_window: bool = True
    apply_window_inside: bool = True
    eps: float = 1e-8
    ola_gain: float = 1.0
    ring_len: int = 0
    device: int = -1
    center: bool = True          # boundary_mode == FRAMEQUEUE only (FrameQueue default)
    pad_mode: int = PAD_CONSTANT
    frame_pairing: bool = True   # crlot_plan_set_frame_pairing (N = 1024 fused path)


class Plan:
    """A device plan: tables resident in HBM, kernels dispatched per call.

    The default configuration is the reference harness's round trip
    (bench/e2e_benchmark.cc:42-76): symmetric Hann analysis window applied by the
    caller, window applied again inside the OLA, ZERO_PAD whole-stream framing.
    """

    def __init__(self, cfg: PlanConfig | None = None, **kw):
        cfg = cfg or PlanConfig(**kw)
        self.cfg = cfg
        d = PlanDesc(cfg.frame_size, cfg.hop_size, cfg.window_type, int(cfg.periodic),
                     cfg.window_norm, cfg.boundary_mode, int(cfg.analysis_window),
                     int(cfg.apply_window_inside), cfg.eps, cfg.ola_gain, cfg.ring_len,
                     cfg.device, int(cfg.center), cfg.pad_mode)
        h = C.c_void_p()
        _check(lib().crlot_plan_create(C.byref(d), C.byref(h)), "crlot_plan_create")
        self._h = h
        self._mask, self._mask_extent = None, None
        n, hop, ring = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().crlot_plan_info(self._h, C.byref(n), C.byref(hop), C.byref(ring)))
        self.frame_size, self.hop_size, self.ring_len = n.value, hop.value, ring.value
        self.set_frame_pairing(cfg.frame_pairing)

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    # -- sizes
    def frame_count(self, T: int) -> int:
        return _check(int(lib().crlot_frame_count(self._h, T)))

    def output_length(self, T: int) -> int:
        return _check(int(lib().crlot_output_length(self._h, T)))

    def workspace_bytes(self, n_streams: int, T: int) -> int:
        return _check(int(lib().crlot_workspace_bytes(self._h, n_streams, T)))

    def reserve(self, nbytes: int):
        _check(lib().crlot_plan_reserve(self._h, nbytes))

    def reserve_stream(self, n_streams: int, T: int, channels: int = 1, stream: int | None = None):
        """Grow `stream`'s scratch slot (default: the current torch stream) for
        round trips of this shape, so those launches never allocate."""
        s = self._cur_stream() if stream is None else stream
        _check(lib().crlot_plan_reserve_stream(self._h, n_streams, T, channels, s), "reserve_stream")

    def _device_index(self) -> int:
        return self.cfg.device if self.cfg.device >= 0 else _torch().cuda.current_device()

    def _cur_stream(self) -> int:
        return int(_torch().cuda.current_stream(self._device_index()).cuda_stream)

    def _require_mask_covers(self, n_streams: int, n_frames: int, what: str):
        check_mask_extent(getattr(self, "_mask_extent", None), n_streams, n_frames, what)

    def upload_tables(self, window=None, norm=None):
        """Replace window / norm, ordered on the current torch stream."""
        w = None if window is None else np.ascontiguousarray(window, np.float32)
        nm = None if norm is None else np.ascontiguousarray(norm, np.float32)
        _check(lib().crlot_plan_upload_tables_async(self._h, None if w is None else w.ctypes.data,
                                                    None if nm is None else nm.ctypes.data,
                                                    self._cur_stream()))

    def set_frame_pairing(self, enable: bool = True):
        """Two frames per complex transform on the fused round trip (default);
        False selects the per-frame kernels, bit-identical to stages + ola_gather;
        2 pairs through the two-regime walkers only (hot walkers off, same bits)."""
        _check(lib().crlot_plan_set_frame_pairing(self._h, 2 if enable == 2 else int(bool(enable))))

    def set_chunks(self, chunks_per_stream: int = 0):
        """Force the chunked walkers to split every stream into this many chunks
        (min(n, F); 0 restores the library's choice).  Output bits never depend
        on it; parity tests use it to move the chunk seams (crlot_plan_set_chunks)."""
        _check(lib().crlot_plan_set_chunks(self._h, int(chunks_per_stream)), "crlot_plan_set_chunks")

    def last_launch(self, stream: int | None = None) -> dict:
        """What the last call on `stream` (default: the current torch stream)
        launched: {"kernels": [names in launch order], "grid": [...],
        "n_chunks": chunks per stream, "n_kernels": count} (crlot_plan_last_launch)."""
        s = self._cur_stream() if stream is None else stream
        info = LaunchInfo()
        _check(lib().crlot_plan_last_launch(self._h, s, C.byref(info)), "crlot_plan_last_launch")
        k = min(info.n_kernels, 8)
        return {"n_kernels": info.n_kernels,
                "kernels": [kernel_name(info.kernels[i]) for i in range(k)],
                "grid": [int(info.grid[i]) for i in range(k)],
                "n_chunks": info.n_chunks}

    def set_spectral_gain(self, gain=None):
        g = None if gain is None else np.ascontiguousarray(gain, np.float32)
        if g is not None and g.size != self.frame_size // 2 + 1:
            raise ValueError("gain needs N/2+1 bins")
        _check(lib().crlot_plan_set_spectral_gain_async(self._h, None if g is None else g.ctypes.data,
                                                        self._cur_stream()))

    def set_spectral_mask(self, mask=None):
        """Time-varying spectral step (crlot_plan_set_spectral_mask): mask is a
        float32 tensor on the plan's device, (S, F, N/2+1) -- one real row per stream
        and frame -- or (F, N/2+1) / (1, F, N/2+1), one row per frame shared by every
        stream; None clears it.  The plan keeps a reference to the tensor until it is
        replaced, and a later call with more frames or streams than the mask has
        raises ValueError before anything is launched."""
        if mask is None:
            self._mask, self._mask_extent = None, None
            _check(lib().crlot_plan_set_spectral_mask(self._h, None, 0, 0), "crlot_plan_set_spectral_mask")
            return
        ld_frame, ld_stream, extent = mask_layout(
            tuple(mask.shape), tuple(mask.stride()), str(mask.dtype).replace("torch.", ""),
            mask.device.index if mask.is_cuda else None, self._device_index(), self.frame_size // 2 + 1)
        self._mask, self._mask_extent = mask, extent
        _check(lib().crlot_plan_set_spectral_mask(self._h, mask.data_ptr(), ld_frame, ld_stream),
               "crlot_plan_set_spectral_mask")

    def stft(self, x, spec=None, stream: int | None = None):
        """x: (S, T) float32 device tensor -> spec: (S, F, N/2+1) complex64, frame *
        analysis window then IFftPlan::forward per frame (crlot_stft)."""
        torch = _torch()
        if x.dim() == 1:
            return self.stft(x[None], None if spec is None else spec[None], stream)[0]
        S, T = x.shape
        if x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1:
            raise ValueError("x must be a float32 device tensor with contiguous rows")
        F, bins = self.frame_count(T), self.frame_size // 2 + 1
        if spec is None:
            spec = torch.empty((S, F, bins), dtype=torch.complex64, device=x.device)
        if spec.dtype != torch.complex64 or spec.shape != (S, F, bins) or spec.stride(2) != 1:
            raise ValueError("spec must be (S, F, N/2+1) complex64 with contiguous rows")
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_stft(self._h, x.data_ptr(), spec.data_ptr(), S, T, _ld(x, 0, T),
                                2 * _ld(spec, 0, F * bins), 2 * _ld(spec, 1, bins), s), "crlot_stft")
        return spec

    def istft_ola(self, spec, y=None, stream: int | None = None):
        """spec: (S, F, N/2+1) complex64 device tensor -> y: (S, F*H): the spectral
        step, IFftPlan::inverse, overlap-add and produce (crlot_istft_ola)."""
        torch = _torch()
        if spec.dim() == 2:
            return self.istft_ola(spec[None], None if y is None else y[None], stream)[0]
        S, F, bins = spec.shape
        if spec.dtype != torch.complex64 or not spec.is_cuda or bins != self.frame_size // 2 + 1 or \
                spec.stride(2) != 1:
            raise ValueError("spec must be (S, F, N/2+1) complex64 with contiguous rows")
        self._require_mask_covers(S, F, "istft_ola")
        L = F * self.hop_size
        if y is None:
            y = torch.empty((S, L), dtype=torch.float32, device=spec.device)
        if y.shape[0] != S or y.shape[1] < L or y.stride(1) != 1:
            raise ValueError("bad y shape")
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_istft_ola(self._h, spec.data_ptr(), y.data_ptr(), S, F, 2 * _ld(spec, 0, F * bins),
                                     2 * _ld(spec, 1, bins), _ld(y, 0, L), s), "crlot_istft_ola")
        return y

    def stretch_output_length(self, T: int, rate: float) -> int:
        return _check(int(lib().crlot_stretch_output_length(self._h, int(T), float(rate))),
                      "crlot_stretch_output_length")

    def phase_vocoder(self, spec, rate: float, out=None, stream: int | None = None):
        """spec: (S, F, N/2+1) or (F, N/2+1) complex64 device tensor -> (S, F', N/2+1):
        the spectra stretched in time by 1 / rate, F' = stretch_frame_count(F, rate)
        (crlot_phase_vocoder; librosa / torchaudio phase_vocoder's recurrence)."""
        if len(spec.shape) == 2:
            return self.phase_vocoder(spec[None], rate, None if out is None else out[None], stream)[0]
        bins = self.frame_size // 2 + 1
        ld_in, ldf_in = _stretch_spec_layout(*_tensor_layout(spec), self._device_index(), bins)
        S, F = int(spec.shape[0]), int(spec.shape[1])
        Fp = stretch_frame_count(F, rate)
        if out is None:
            out = _torch().empty((S, Fp, bins), dtype=spec.dtype, device=spec.device)
        ld_out, ldf_out = _stretch_spec_layout(*_tensor_layout(out), self._device_index(), bins, "out", (S, Fp, bins))
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_phase_vocoder(self._h, spec.data_ptr(), out.data_ptr(), S, F, float(rate), ld_in, ldf_in,
                                         ld_out, ldf_out, s), "crlot_phase_vocoder")
        return out

    def time_stretch(self, x, rate: float, y=None, stream: int | None = None):
        """x: (S, T) or (T,) float32 device tensor -> y: (S, F' * H), the signal
        stretched by 1 / rate at its pitch: istft_ola(phase_vocoder(stft(x), rate)),
        bit for bit, with the spectra in the plan's scratch (crlot_time_stretch)."""
        if x.dim() == 1:
            return self.time_stretch(x[None], rate, None if y is None else y[None], stream)[0]
        S, T = _spectrogram_x_layout(*_tensor_layout(x))
        Fp = stretch_frame_count(self.frame_count(T), rate)
        self._require_mask_covers(S, Fp, "time_stretch")
        L = Fp * self.hop_size
        if y is None:
            y = _torch().empty((S, L), dtype=x.dtype, device=x.device)
        if str(y.dtype) != "torch.float32" or not y.is_cuda or y.dim() != 2 or y.shape[0] != S or y.shape[1] < L or \
                (y.shape[1] > 1 and y.stride(1) != 1):
            raise ValueError(f"y must be a float32 device tensor of ({S}, >= {L}) with contiguous rows")
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_time_stretch(self._h, x.data_ptr(), y.data_ptr(), S, T, float(rate), _ld(x, 0, T),
                                        _ld(y, 0, L), s), "crlot_time_stretch")
        return y

    def gl_project(self, spec, mag, tprev=None, momentum: float = 0.0, out=None, stream: int | None = None):
        """The Griffin-Lim projection (crlot_gl_project): spec, tprev (optional, the
        previous rebuilt spectra), out: (S, F, N/2+1) or (F, N/2+1) complex64, mag the
        same shape in float32 -> out = mag * c / (|c| + 1e-16), c = spec - tprev *
        momentum / (1 + momentum).  out may be spec itself (in place)."""
        if len(spec.shape) == 2:
            return self.gl_project(spec[None], mag[None] if len(mag.shape) == 2 else mag,
                                   None if tprev is None else tprev[None], momentum,
                                   None if out is None else out[None], stream)[0]
        _, m = _gl_scalars(0, momentum)
        bins, dev = self.frame_size // 2 + 1, self._device_index()
        ld_s, ldf_s = _stretch_spec_layout(*_tensor_layout(spec), dev, bins)
        S, F = int(spec.shape[0]), int(spec.shape[1])
        _, _, ld_m, ldf_m = _gl_mag_layout(*_tensor_layout(mag), dev, bins, "mag", (S, F, bins))
        ld_t = ldf_t = 0
        if tprev is not None:
            ld_t, ldf_t = _stretch_spec_layout(*_tensor_layout(tprev), dev, bins, "tprev", (S, F, bins))
        if out is None:
            out = _torch().empty((S, F, bins), dtype=spec.dtype, device=spec.device)
        ld_o, ldf_o = _stretch_spec_layout(*_tensor_layout(out), dev, bins, "out", (S, F, bins))
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_gl_project(self._h, spec.data_ptr(), None if tprev is None else tprev.data_ptr(),
                                      mag.data_ptr(), out.data_ptr(), S, F, m, ld_s, ldf_s, ld_t, ldf_t, ld_m, ldf_m,
                                      ld_o, ldf_o, s), "crlot_gl_project")
        return out

    def griffin_lim(self, mag, n_iter: int = 32, momentum: float = 0.99, init=None, y=None,
                    stream: int | None = None):
        """mag: (S, F, N/2+1) or (F, N/2+1) float32 device tensor of target magnitudes
        -> y: (S, F * H), the signal whose STFT magnitudes approach mag after n_iter
        fast Griffin-Lim iterations (crlot_griffin_lim; librosa / torchaudio
        GriffinLim).  init: optional complex64 spectra of the same shape giving the
        starting phases (default: zero phase).  The plan must use ZERO_PAD framing
        and have no spectral gain or mask.  On a default plan, whose norm table is
        the sum of the window, the magnitudes of y settle at sum(w^2) / sum(w) times
        mag (the phases are reconstructed, the level is not); for magnitudes that
        approach mag, upload_tables(norm=sum of w^2 per sample, ring_len floats)
        first (include/crlot_dsp.h, "What it converges to")."""
        if len(mag.shape) == 2:
            return self.griffin_lim(mag[None], n_iter, momentum, None if init is None else init[None],
                                    None if y is None else y[None], stream)[0]
        n_iter, m = _gl_scalars(n_iter, momentum)
        bins, dev = self.frame_size // 2 + 1, self._device_index()
        S, F, ld_m, ldf_m = _gl_mag_layout(*_tensor_layout(mag), dev, bins)
        ld_i = ldf_i = 0
        if init is not None:
            ld_i, ldf_i = _stretch_spec_layout(*_tensor_layout(init), dev, bins, "init", (S, F, bins))
        L = F * self.hop_size
        if y is None:
            y = _torch().empty((S, L), dtype=mag.dtype, device=mag.device)
        ld_y = _gl_y_layout(*_tensor_layout(y), dev, S, L)
        s = _stream_handle(mag) if stream is None else stream
        _check(lib().crlot_griffin_lim(self._h, mag.data_ptr(), ld_m, ldf_m, None if init is None else init.data_ptr(),
                                       ld_i, ldf_i, y.data_ptr(), ld_y, S, F, n_iter, m, s), "crlot_griffin_lim")
        return y

    def hpss_masks(self, spec, kernel_size=31, power=2, margin=1.0, mask_h=None, mask_p=None,
                   stream: int | None = None):
        """spec: (S, F, N/2+1) or (F, N/2+1) complex64 device tensor -> (mask_h, mask_p),
        float32 of the same shape: the harmonic and percussive soft masks of
        librosa.decompose.hpss(mask=True) (crlot_hpss_masks): medians of |spec| over
        kernel_size frames and bins, margins and power as in librosa (power 1, 2 or
        inf).  Pass mask_h=False or mask_p=False to skip that mask (None is returned
        in its place); a tensor is written in place (rows may be padded).  The masks
        are what Plan.set_spectral_mask takes."""
        if len(spec.shape) == 2:
            up = lambda m: m[None] if m is not None and m is not False else m  # noqa: E731
            mh, mp = self.hpss_masks(spec[None], kernel_size, power, margin, up(mask_h), up(mask_p), stream)
            return (None if mh is None else mh[0]), (None if mp is None else mp[0])
        desc = _hpss_desc(kernel_size, power, margin)
        if mask_h is False and mask_p is False:
            raise ValueError("at least one of mask_h and mask_p must be computed")
        bins, dev = self.frame_size // 2 + 1, self._device_index()
        ld_s, ldf_s = _stretch_spec_layout(*_tensor_layout(spec), dev, bins)
        S, F = int(spec.shape[0]), int(spec.shape[1])
        outs, lds = [], []
        for m, what in ((mask_h, "mask_h"), (mask_p, "mask_p")):
            if m is False:
                outs.append(None)
                lds.append((0, 0))
                continue
            if m is None:
                m = _torch().empty((S, F, bins), dtype=_torch().float32, device=spec.device)
            _, _, ld_m, ldf_m = _gl_mag_layout(*_tensor_layout(m), dev, bins, what, (S, F, bins))
            if _tensors_overlap(m, spec) or any(o is not None and _tensors_overlap(m, o) for o in outs):
                raise ValueError(f"{what} overlaps spec or the other mask")
            outs.append(m)
            lds.append((ld_m, ldf_m))
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_hpss_masks(self._h, C.byref(desc), spec.data_ptr(),
                                      None if outs[0] is None else outs[0].data_ptr(),
                                      None if outs[1] is None else outs[1].data_ptr(), S, F, ld_s, ldf_s,
                                      lds[0][0], lds[0][1], lds[1][0], lds[1][1], s), "crlot_hpss_masks")
        return outs[0], outs[1]

    def hpss(self, x, kernel_size=31, power=2, margin=1.0, y_h=None, y_p=None, stream: int | None = None):
        """x: (S, T) or (T,) float32 device tensor -> (y_h, y_p), each (S, F * H): the
        harmonic and the percussive part of x (crlot_hpss; librosa.effects.hpss):
        istft_ola of stft(x) under each of hpss_masks' masks, bit for bit, with the
        spectra and the masks in the plan's scratch.  Pass y_h=False or y_p=False to
        skip that part (None is returned in its place).  The plan must have no
        stored spectral mask."""
        if x.dim() == 1:
            up = lambda y: y[None] if y is not None and y is not False else y  # noqa: E731
            yh, yp = self.hpss(x[None], kernel_size, power, margin, up(y_h), up(y_p), stream)
            return (None if yh is None else yh[0]), (None if yp is None else yp[0])
        desc = _hpss_desc(kernel_size, power, margin)
        if y_h is False and y_p is False:
            raise ValueError("at least one of y_h and y_p must be computed")
        S, T = _spectrogram_x_layout(*_tensor_layout(x))
        if getattr(self, "_mask", None) is not None:
            raise ValueError("hpss: the plan has a stored spectral mask; clear it first")
        dev = self._device_index()
        L = self.frame_count(T) * self.hop_size
        outs, lds = [], []
        for y in (y_h, y_p):
            if y is False:
                outs.append(None)
                lds.append(0)
                continue
            if y is None:
                y = _torch().empty((S, L), dtype=x.dtype, device=x.device)
            lds.append(_gl_y_layout(*_tensor_layout(y), dev, S, L))
            if _tensors_overlap(y, x) or any(o is not None and _tensors_overlap(y, o) for o in outs):
                raise ValueError("an output overlaps x or the other output")
            outs.append(y)
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_hpss(self._h, C.byref(desc), x.data_ptr(), None if outs[0] is None else outs[0].data_ptr(),
                                None if outs[1] is None else outs[1].data_ptr(), S, T, _ld(x, 0, T), lds[0], lds[1],
                                s), "crlot_hpss")
        return outs[0], outs[1]

    def pitch_shift(self, x, resampler=None, semitones: float | None = None, max_den: int = 256, y=None,
                    stream: int | None = None):
        """x: (S, T) or (T,) float32 device tensor -> y: (S, T), the pitch multiplied
        by D / U of `resampler` (a Resampler(U, D, ...) on the plan's device) at the
        same length: resample(time_stretch(x, U / D)) cropped or zero-filled to T, bit
        for bit (crlot_pitch_shift).  semitones instead of a resampler: the ratio
        2 ** (semitones / 12) through rational_approx(., max_den) and a Resampler with
        the default filter, cached on the plan."""
        if (resampler is None) == (semitones is None):
            raise ValueError("give either a resampler or semitones")
        if resampler is None:
            num, den = rational_approx(2.0 ** (float(semitones) / 12.0), max_den)
            cache = self.__dict__.setdefault("_pitch_resamplers", {})
            resampler = cache.get((den, num))
            if resampler is None:  # (pitch * num / den: D = num, U = den)
                resampler = cache[(den, num)] = Resampler(den, num, device=self._device_index())
        if x.dim() == 1:
            return self.pitch_shift(x[None], resampler, None, max_den, None if y is None else y[None], stream)[0]
        S, T = _spectrogram_x_layout(*_tensor_layout(x))
        if resampler.device != self._device_index():
            raise ValueError(f"the resampler is on device {resampler.device}, the plan on {self._device_index()}")
        rate = resampler.up / resampler.down
        if T > 0 and self.frame_count(T) > 0:
            self._require_mask_covers(S, stretch_frame_count(self.frame_count(T), rate), "pitch_shift")
        if y is None:
            y = _torch().empty((S, T), dtype=x.dtype, device=x.device)
        ld_y = _resample_y_layout(*_tensor_layout(y), S, T)
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_pitch_shift(self._h, resampler._h, x.data_ptr(), y.data_ptr(), S, T, _ld(x, 0, T), ld_y, s),
               "crlot_pitch_shift")
        return y

    # -- hot path
    def roundtrip(self, x, y=None, stream: int | None = None):
        """x: (S, T) float32 CUDA tensor -> y: (S, F*H)."""
        torch = _torch()
        if x.dim() == 1:
            return self.roundtrip(x[None], None if y is None else y[None], stream)[0]
        if x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError("x must be a float32 device tensor")
        S, T = x.shape
        if x.stride(1) != 1:
            raise ValueError("x rows must be contiguous")
        L = self.output_length(T)
        self._require_mask_covers(S, self.frame_count(T), "roundtrip")
        if y is None:
            y = torch.empty((S, L), dtype=torch.float32, device=x.device)
        if y.shape[0] != S or y.shape[1] < L or y.stride(1) != 1:
            raise ValueError("bad y shape")
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_roundtrip(self._h, x.data_ptr(), y.data_ptr(), S, T, _ld(x, 0, T),
                                     _ld(y, 0, L), s), "crlot_roundtrip")
        return y

    def roundtrip_interleaved(self, x, y=None, stream: int | None = None):
        """x: (G, T, C) float32 CUDA tensor of G groups of C interleaved channels ->
        y: (G, F*H, C), each channel an independent stream (crlot_roundtrip_interleaved)."""
        torch = _torch()
        G, T, Cc = x.shape
        if x.stride(2) != 1 or x.stride(1) != Cc:
            raise ValueError("x must be (G, T, C) with contiguous rows of C samples")
        L = self.output_length(T)
        # every channel is a stream of its own: the mask is read for G * C streams
        self._require_mask_covers(G * Cc, self.frame_count(T), "roundtrip_interleaved")
        if y is None:
            y = torch.empty((G, L, Cc), dtype=torch.float32, device=x.device)
        s = _stream_handle(x) if stream is None else stream
        ldx = x.stride(0) if G > 1 else T * Cc
        ldy = y.stride(0) if G > 1 else L * Cc
        _check(lib().crlot_roundtrip_interleaved(self._h, x.data_ptr(), y.data_ptr(), G, Cc, T, ldx, ldy, s),
               "crlot_roundtrip_interleaved")
        return y

    def stages(self, x, want_spec=True):
        """Per-stage outputs: frames (S, F, N) push_frame_AoS inputs, spec (S, F, N/2+1)."""
        torch = _torch()
        S, T = x.shape
        F = self.frame_count(T)
        n = self.frame_size
        frames = torch.empty((S, F, n), dtype=torch.float32, device=x.device)
        spec = (torch.empty((S, F, n // 2 + 1), dtype=torch.complex64, device=x.device)
                if want_spec else None)
        _check(lib().crlot_roundtrip_stages(self._h, x.data_ptr(), S, T, _ld(x, 0, T),
                                            frames.data_ptr(),
                                            None if spec is None else spec.data_ptr(),
                                            _stream_handle(x)), "crlot_roundtrip_stages")
        return frames, spec

    def ola_gather(self, frames, y=None):
        """frames (S, F, N) -> y (S, F*H) through the bit-exact OLA kernel."""
        torch = _torch()
        S, F, n = frames.shape
        if n != self.frame_size or frames.stride(2) != 1 or (
                S > 1 and frames.stride(0) != F * _ld(frames, 1, n)):
            raise ValueError("frames must be (S, F, N) with contiguous (F, N) blocks")
        L = F * self.hop_size
        if y is None:
            y = torch.empty((S, L), dtype=torch.float32, device=frames.device)
        _check(lib().crlot_ola_gather(self._h, frames.data_ptr(), y.data_ptr(), S, F,
                                      _ld(frames, 1, n), _ld(y, 0, L), _stream_handle(frames)),
               "crlot_ola_gather")
        return y

    def rfft(self, x):
        """(B, N) real -> (B, N/2+1) complex, KissFftPlan::forward semantics."""
        torch = _torch()
        B, n = x.shape
        out = torch.empty((B, n // 2 + 1), dtype=torch.complex64, device=x.device)
        _check(lib().crlot_rfft_batched(self._h, x.data_ptr(), out.data_ptr(), B, _ld(x, 0, n),
                                        x.stride(1), 2 * (n // 2 + 1), 1, _stream_handle(x)),
               "crlot_rfft_batched")
        return out

    def irfft(self, X):
        """(B, N/2+1) complex -> (B, N) real, KissFftPlan::inverse semantics."""
        torch = _torch()
        B, bins = X.shape
        n = self.frame_size
        X = X.contiguous()
        out = torch.empty((B, n), dtype=torch.float32, device=X.device)
        _check(lib().crlot_irfft_batched(self._h, X.data_ptr(), out.data_ptr(), B, 2 * bins,
                                         1, n, 1, _stream_handle(X)),
               "crlot_irfft_batched")
        return out


def mel_filterbank(n_mels: int, nfft: int, sample_rate: float, fmin: float = 0.0, fmax: float | None = None,
                   scale: int = MEL_HTK, slaney_norm: bool = False) -> np.ndarray:
    """(n_mels, nfft/2+1) float32 triangular mel weights (crlot_mel_filterbank):
    computed in double, rounded once; fmax None: sample_rate / 2."""
    out = np.zeros((max(int(n_mels), 1), max(int(nfft), 0) // 2 + 1), np.float32)
    _check(lib().crlot_mel_filterbank(int(n_mels), int(nfft), float(sample_rate), float(fmin),
                                      0.0 if fmax is None else float(fmax), int(scale), int(bool(slaney_norm)),
                                      _fptr(out)), "crlot_mel_filterbank")
    return out


def filterbank_spans(weights) -> tuple[np.ndarray, np.ndarray]:
    """(lo, hi) of every row of a (n_bands, bins) filterbank: the first to one past
    the last non-zero weight, (0, 0) for an all-zero row (crlot_filterbank_spans)."""
    w = np.ascontiguousarray(weights, np.float32)
    if w.ndim != 2 or w.shape[1] < 1:
        raise ValueError("weights must be (n_bands, bins)")
    lo, hi = np.zeros(w.shape[0], np.int32), np.zeros(w.shape[0], np.int32)
    i32p = C.POINTER(C.c_int32)
    _check(lib().crlot_filterbank_spans(_fptr(w), w.shape[0], w.shape[1], lo.ctypes.data_as(i32p),
                                        hi.ctypes.data_as(i32p)), "crlot_filterbank_spans")
    return lo, hi


def _spectrogram_x_layout(shape, strides, dtype: str, device_index):
    """Validate Features.spectrogram's input from its plain description (shape and
    strides in elements as tuples, dtype name, device index or None for a host
    tensor), as Plan.stft validates its own x.  Returns (S, T)."""
    if len(shape) != 2 or len(strides) != 2:
        raise ValueError("x must be (S, T) or (T,)")
    if dtype != "float32":
        raise ValueError(f"x must be float32, not {dtype}")
    if device_index is None:
        raise ValueError("x must be a device tensor")
    if int(shape[1]) > 1 and int(strides[1]) != 1:
        raise ValueError("x must have contiguous rows")
    return int(shape[0]), int(shape[1])


def _spectrogram_out_layout(shape, strides, dtype: str, device_index, S: int, F: int, n_out: int):
    """The same for a caller's output tensor: (S, F, n_out) float32 on the device,
    rows contiguous and at least n_out apart.  Returns (ld_out, ld_frame)."""
    if dtype != "float32" or device_index is None:
        raise ValueError("out must be a float32 device tensor")
    if tuple(int(v) for v in shape) != (S, F, n_out) or len(strides) != 3:
        raise ValueError(f"out must be ({S}, {F}, {n_out})")
    if n_out > 1 and int(strides[2]) != 1:
        raise ValueError("out must have contiguous rows")
    # a size-1 dim's stride is meaningless: the dense value there
    ld_frame = int(strides[1]) if F > 1 else n_out
    ld_out = int(strides[0]) if S > 1 else F * n_out
    if ld_frame < n_out or ld_out < 0:
        raise ValueError("out rows overlap: ld_frame < n_out")
    return ld_out, ld_frame


def _features_hop_out_layout(shape, strides, dtype: str, device_index, channels: int, n_out: int,
                             same_plan: bool = True):
    """The same for Stream.features_hop's output: (channels, n_out) float32 on the
    device, rows contiguous and at least n_out apart, the features object built on
    the stream's plan (same_plan).  Returns ld_feat."""
    if not same_plan:
        raise ValueError("features was created on another plan than the stream's")
    if dtype != "float32":
        raise ValueError(f"out must be float32, not {dtype}")
    if device_index is None:
        raise ValueError("out must be a device tensor")
    if tuple(int(v) for v in shape) != (channels, n_out) or len(strides) != 2:
        raise ValueError(f"out must be ({channels}, {n_out})")
    if n_out > 1 and int(strides[1]) != 1:
        raise ValueError("out must have contiguous rows")
    ld_feat = int(strides[0]) if channels > 1 else n_out  # (a size-1 dim's stride is meaningless)
    if ld_feat < n_out:
        raise ValueError("out rows overlap: ld_feat < n_out")
    return ld_feat


def _tensor_layout(t):
    return (tuple(t.shape), tuple(t.stride()), str(t.dtype).replace("torch.", ""),
            (t.device.index if t.device.index is not None else 0) if t.is_cuda else None)


class Features:
    """Spectrogram features of a plan's STFT, computed where the spectrum would be
    stored (crlot_features_create / crlot_spectrogram): per bin |X|^2 or |X|
    (weights None), or the rows of a (n_bands, N/2+1) filterbank applied to them,
    optionally logged (log FEAT_LN / FEAT_LOG10 / FEAT_DB of max(value, floor)).
    Keeps a reference to the plan, which must outlive it."""

    def __init__(self, plan: Plan, kind: int = FEAT_POWER, weights=None, log: int = FEAT_LIN, floor: float = 0.0):
        self._h = None
        bins = plan.frame_size // 2 + 1
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, np.float32)
            if w.ndim != 2 or w.shape[1] != bins or w.shape[0] < 1:
                raise ValueError("weights must be (n_bands, N/2+1)")
        d = FeaturesDesc(int(kind), 0 if w is None else w.shape[0], int(log), float(floor))
        h = C.c_void_p()
        _check(lib().crlot_features_create(plan._h, C.byref(d), None if w is None else w.ctypes.data, C.byref(h)),
               "crlot_features_create")
        self._h, self.plan = h, plan
        n_out, k, lg, widest = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().crlot_features_info(self._h, C.byref(n_out), C.byref(k), C.byref(lg), C.byref(widest)))
        self.n_out, self.kind, self.log, self.widest_band = n_out.value, k.value, lg.value, widest.value

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_features_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def spectrogram(self, x, out=None, stream: int | None = None):
        """x: (S, T) or (T,) float32 device tensor -> (S, F, n_out) float32: frame k of
        stream s framed, windowed and transformed exactly as Plan.stft, then the
        feature (crlot_spectrogram)."""
        if x.dim() == 1:
            return self.spectrogram(x[None], None if out is None else out[None], stream)[0]
        S, T = _spectrogram_x_layout(*_tensor_layout(x))
        F = self.plan.frame_count(T)
        if out is None:
            out = _torch().empty((S, F, self.n_out), dtype=x.dtype, device=x.device)
        ld_out, ld_frame = _spectrogram_out_layout(*_tensor_layout(out), S, F, self.n_out)
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_spectrogram(self._h, x.data_ptr(), out.data_ptr(), S, T, _ld(x, 0, T), ld_out, ld_frame,
                                       s), "crlot_spectrogram")
        return out


# ----------------------------------------------------------------- resampler
RESAMPLE_HANN, RESAMPLE_KAISER = 0, 1
RESAMPLE_AUTO, RESAMPLE_PHASE, RESAMPLE_ANY = 0, 1, 2
_RESAMPLE_WINDOWS = {"hann": RESAMPLE_HANN, "kaiser": RESAMPLE_KAISER}
_RESAMPLE_ROUTES = {"auto": RESAMPLE_AUTO, "phase": RESAMPLE_PHASE, "any": RESAMPLE_ANY}


def rational_approx(ratio: float, max_den: int) -> tuple[int, int]:
    """The best rational (num, den) to `ratio` with den <= max_den: exactly
    fractions.Fraction(ratio).limit_denominator(max_den) (crlot_rational_approx)."""
    num, den = C.c_int32(), C.c_int32()
    _check(lib().crlot_rational_approx(float(ratio), int(max_den), C.byref(num), C.byref(den)),
           "crlot_rational_approx")
    return num.value, den.value


def _resampler_desc(up, down, zeros=16, rolloff=0.95, window="hann", beta=8.6, device=0) -> ResamplerDesc:
    if isinstance(window, str):
        if window not in _RESAMPLE_WINDOWS:
            raise ValueError(f"window must be one of {sorted(_RESAMPLE_WINDOWS)}")
        window = _RESAMPLE_WINDOWS[window]
    return ResamplerDesc(int(up), int(down), int(zeros), int(window), float(rolloff), float(beta), int(device), 0)


def resample_geometry(up, down, zeros=16, rolloff=0.95, window="hann", beta=8.6, device=0) -> dict:
    """The reduced rates and filter geometry of a descriptor, on the host
    (crlot_resample_geometry): up, down, half_width W, taps K, phase_ok."""
    d, g = _resampler_desc(up, down, zeros, rolloff, window, beta, device), ResamplerGeometry()
    _check(lib().crlot_resample_geometry(C.byref(d), C.byref(g)), "crlot_resample_geometry")
    return {k: getattr(g, k) for k, _ in ResamplerGeometry._fields_}


def resample_table_host(up, down, zeros=16, rolloff=0.95, window="hann", beta=8.6) -> np.ndarray:
    """The (U, K) float32 filter table of a descriptor, built on the host
    (crlot_resample_table_host)."""
    g = resample_geometry(up, down, zeros, rolloff, window, beta)
    d = _resampler_desc(up, down, zeros, rolloff, window, beta)
    out = np.zeros((g["up"], g["taps"]), np.float32)
    _check(lib().crlot_resample_table_host(C.byref(d), _fptr(out)), "crlot_resample_table_host")
    return out


def _resample_y_layout(shape, strides, dtype: str, device_index, S: int, L: int, what: str = "y"):
    """Validate a resampler output from its plain description: (S, >= L) float32 on
    the device with contiguous rows.  Returns ld_y."""
    if dtype != "float32" or device_index is None:
        raise ValueError(f"{what} must be a float32 device tensor")
    if len(shape) != 2 or len(strides) != 2 or int(shape[0]) != S or int(shape[1]) < L:
        raise ValueError(f"{what} must be ({S}, >= {L})")
    if int(shape[1]) > 1 and int(strides[1]) != 1:
        raise ValueError(f"{what} must have contiguous rows")
    ld = int(strides[0]) if S > 1 else max(int(shape[1]), L)  # (a size-1 dim's stride is meaningless)
    if S > 1 and ld < L:
        raise ValueError(f"{what} rows overlap: ld_y < {L}")
    return ld


class Resampler:
    """A band-limited rational resampler from rate `down` to rate `up`
    (crlot_resampler_create / crlot_resample): the polyphase windowed-sinc filter of
    torchaudio.functional.resample, `zeros` zero crossings wide, Hann or Kaiser
    windowed.  Needs no plan; the table is uploaded by the first call."""

    def __init__(self, up: int, down: int, zeros: int = 16, rolloff: float = 0.95, window="hann", beta: float = 8.6,
                 device: int = 0):
        self._h = None
        d = _resampler_desc(up, down, zeros, rolloff, window, beta, device)
        h = C.c_void_p()
        _check(lib().crlot_resampler_create(C.byref(d), C.byref(h)), "crlot_resampler_create")
        self._h = h
        g = ResamplerGeometry()
        _check(lib().crlot_resampler_info(self._h, C.byref(g)), "crlot_resampler_info")
        self.info = {k: getattr(g, k) for k, _ in ResamplerGeometry._fields_}
        self.up, self.down, self.half_width, self.taps, self.device = g.up, g.down, g.half_width, g.taps, g.device

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_resampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def output_length(self, T: int) -> int:
        return _check(int(lib().crlot_resample_output_length(self._h, int(T))), "crlot_resample_output_length")

    def table(self) -> np.ndarray:
        out = np.zeros((self.up, self.taps), np.float32)
        _check(lib().crlot_resampler_table(self._h, _fptr(out)), "crlot_resampler_table")
        return out

    def prepare(self):
        _check(lib().crlot_resampler_prepare(self._h), "crlot_resampler_prepare")

    def set_route(self, route):
        """"auto", "phase" or "any" (RESAMPLE_*): a test knob; "phase" on a shape the
        phase kernel cannot take raises NotImplementedError."""
        route = _RESAMPLE_ROUTES[route] if isinstance(route, str) else int(route)
        _check(lib().crlot_resampler_set_route(self._h, route), "crlot_resampler_set_route")

    def set_tile(self, n_blocks: int):
        """Force n output blocks of U outputs per tile (0: the library's choice)."""
        _check(lib().crlot_resampler_set_tile(self._h, int(n_blocks)), "crlot_resampler_set_tile")

    def last_launch(self) -> dict:
        r = ResampleLaunch()
        _check(lib().crlot_resampler_last_launch(self._h, C.byref(r)), "crlot_resampler_last_launch")
        d = {k: getattr(r, k) for k, _ in ResampleLaunch._fields_}
        d["name"] = kernel_name(r.kernel) if r.kernel else None
        return d

    def resample(self, x, y=None, stream: int | None = None):
        """x: (S, T) or (T,) float32 device tensor -> y: (S, L), L = output_length(T)
        (crlot_resample)."""
        if x.dim() == 1:
            return self.resample(x[None], None if y is None else y[None], stream)[0]
        S, T = _spectrogram_x_layout(*_tensor_layout(x))
        if (x.device.index or 0) != self.device:
            raise ValueError(f"x must live on the resampler's device {self.device}")
        L = self.output_length(T)
        if y is None:
            y = _torch().empty((S, L), dtype=x.dtype, device=x.device)
        ld_y = _resample_y_layout(*_tensor_layout(y), S, L)
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_resample(self._h, x.data_ptr(), y.data_ptr(), S, T, _ld(x, 0, T), ld_y, s),
               "crlot_resample")
        return y


# ----------------------------------------------------------------- partitioned FFT convolution
def _convolve_layouts(x_layout, y_layout, device: int, K: int):
    """Validate Convolver.convolve's tensors from their plain descriptions (shape,
    strides in elements, dtype name, device index or None for a host tensor; y_layout
    None: the call allocates y): x (S, T) float32 and y (S, >= T + K - 1) float32 on
    `device`, rows contiguous and not overlapping.  Returns (S, T, L, ld_x, ld_y)."""
    S, T = _spectrogram_x_layout(*x_layout)
    if int(x_layout[3]) != int(device):
        raise ValueError(f"x must live on the convolver's device {device}, not {x_layout[3]}")
    L = 0 if T == 0 else T + int(K) - 1
    ld_x = int(x_layout[1][0]) if S > 1 else max(T, 1)
    if S > 1 and ld_x < T:
        raise ValueError("x rows overlap: the stream stride is below T")
    ld_y = max(L, 1) if y_layout is None else _gl_y_layout(*y_layout, device, S, L)
    return S, T, L, ld_x, ld_y


def _fdl_layouts(spec_layout, out_layout, device: int, bins: int, P: int, F_out=None):
    """The same for Convolver.fdl_mac: spec (S, F_in, bins) complex64 and out
    (S, F_out, bins) complex64 on `device` (_stretch_spec_layout's rules); F_out
    defaults to F_in + P - 1.  Returns (S, F_in, F_out, ld_in, ldf_in, ld_out, ldf_out),
    the last two None when the call allocates out."""
    ld_in, ldf_in = _stretch_spec_layout(*spec_layout, device, bins)
    S, F_in = int(spec_layout[0][0]), int(spec_layout[0][1])
    if F_out is None:
        F_out = F_in + int(P) - 1 if F_in > 0 else 0
    if isinstance(F_out, bool) or int(F_out) != F_out or int(F_out) < 0:
        raise ValueError("F_out must be a non-negative integer")
    F_out = int(F_out)
    if out_layout is None:
        return S, F_in, F_out, ld_in, ldf_in, None, None
    ld_out, ldf_out = _stretch_spec_layout(*out_layout, device, bins, "out", (S, F_out, bins))
    return S, F_in, F_out, ld_in, ldf_in, ld_out, ldf_out


class _BorrowedPlan(Plan):
    """A Plan over a handle another object owns (Convolver.plan): closing it forgets
    the handle and destroys nothing; it keeps its owner alive."""

    def __init__(self, handle, owner, cfg: PlanConfig):
        self.cfg, self._h, self._owner = cfg, handle, owner
        self._mask, self._mask_extent = None, None
        n, hop, ring = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().crlot_plan_info(self._h, C.byref(n), C.byref(hop), C.byref(ring)))
        self.frame_size, self.hop_size, self.ring_len = n.value, hop.value, ring.value

    def close(self):
        self._h, self._owner = None, None


class Convolver:
    """Full linear convolution of every stream with a long FIR as uniformly
    partitioned overlap-add (crlot_convolver_create / crlot_convolve; the numbers of
    torchaudio.functional.fftconvolve).  h: (K,) or (n_filters, K) float32 taps on
    the host, stream s uses filter s mod n_filters; block: the partition size B (the
    engine plan has N = 2B, H = B).  Creation touches no device: the plan and the
    filter spectra are made by prepare(), .plan or the first device call."""

    def __init__(self, h, block: int = 512, device: int | None = None):
        self._h, self._plan = None, None
        taps = np.ascontiguousarray(np.asarray(h.cpu() if hasattr(h, "cpu") else h), np.float32)
        if taps.ndim == 1:
            taps = taps[None]
        if taps.ndim != 2 or taps.shape[1] < 1:
            raise ValueError("h must be (K,) or (n_filters, K) with K >= 1")
        self._device = None if device is None else int(device)
        d = ConvolverDesc(int(block), int(taps.shape[0]), -1 if device is None else int(device), 0)
        hd = C.c_void_p()
        _check(lib().crlot_convolver_create(C.byref(d), _fptr(taps), taps.shape[1], taps.shape[1], C.byref(hd)),
               "crlot_convolver_create")
        self._h = hd
        b, nf, k, p = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        _check(lib().crlot_convolver_info(self._h, C.byref(b), C.byref(nf), C.byref(k), C.byref(p)),
               "crlot_convolver_info")
        self.block, self.n_filters, self.taps, self.partitions = b.value, nf.value, k.value, p.value
        self.frame_size, self.bins = 2 * b.value, b.value + 1

    def close(self):
        if getattr(self, "_plan", None) is not None:
            self._plan.close()
            self._plan = None
        if getattr(self, "_h", None):
            lib().crlot_convolver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    @property
    def device(self) -> int:
        """The device index (device=None: the current device at the first use)."""
        if self._device is None:
            self._device = int(_torch().cuda.current_device())
        return self._device

    def prepare(self):
        """Create the engine plan, upload and transform the filter now."""
        dev = self.device
        with _torch().cuda.device(dev):
            _check(lib().crlot_convolver_prepare(self._h), "crlot_convolver_prepare")

    @property
    def plan(self) -> Plan:
        """The engine plan (N = 2B, H = B, ZERO_PAD, a window of B ones and B zeros,
        unit norm), borrowed: use its stft / istft_ola / set_frame_pairing /
        set_chunks / last_launch; do not replace its tables, gain or mask."""
        if self._plan is None:
            self.prepare()
            h = lib().crlot_convolver_plan(self._h)
            if not h:
                _check(EHIP, "crlot_convolver_plan")
            cfg = PlanConfig(frame_size=self.frame_size, hop_size=self.block, window_type=RECT,
                             boundary_mode=ZERO_PAD, analysis_window=True, apply_window_inside=False,
                             device=self.device)
            self._plan = _BorrowedPlan(C.c_void_p(h), self, cfg)
        return self._plan

    def output_length(self, T: int) -> int:
        return _check(int(lib().crlot_convolve_output_length(self._h, int(T))), "crlot_convolve_output_length")

    def spectra(self) -> np.ndarray:
        """The filter spectra H, (n_filters, P, N/2+1) complex64, from the device."""
        self.prepare()
        out = np.zeros((self.n_filters, self.partitions, 2 * self.bins), np.float32)
        _check(lib().crlot_convolver_spectra(self._h, _fptr(out)), "crlot_convolver_spectra")
        return out.view(np.complex64)

    def set_chunks(self, n: int = 0):
        """Force the delay line to split every stream's output frames into min(n, F_out)
        chunks (0: the library's choice).  Output bits never depend on it."""
        _check(lib().crlot_convolver_set_chunks(self._h, int(n)), "crlot_convolver_set_chunks")

    def last_launch(self) -> dict:
        r = ConvolverLaunch()
        _check(lib().crlot_convolver_last_launch(self._h, C.byref(r)), "crlot_convolver_last_launch")
        d = {k: getattr(r, k) for k, _ in ConvolverLaunch._fields_ if k != "reserved"}
        d["name"] = kernel_name(r.kernel) if r.kernel else None
        return d

    def fdl_mac(self, spec, out=None, F_out: int | None = None, stream: int | None = None):
        """spec: (S, F_in, N/2+1) or (F_in, N/2+1) complex64 device tensor -> out:
        (S, F_out, N/2+1), F_out = F_in + P - 1 by default: per bin the complex FIR of
        the filter's partition spectra along the frame axis (crlot_fdl_mac)."""
        if len(spec.shape) == 2:
            return self.fdl_mac(spec[None], None if out is None else out[None], F_out, stream)[0]
        S, F_in, F_out, ld_in, ldf_in, ld_out, ldf_out = _fdl_layouts(
            _tensor_layout(spec), None if out is None else _tensor_layout(out), self.device, self.bins,
            self.partitions, F_out)
        if out is None:
            out = _torch().empty((S, F_out, self.bins), dtype=spec.dtype, device=spec.device)
            ld_out, ldf_out = 2 * F_out * self.bins, 2 * self.bins
        elif _tensors_overlap(spec, out):
            raise ValueError("out overlaps spec")
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_fdl_mac(self._h, spec.data_ptr(), out.data_ptr(), S, F_in, F_out, ld_in, ldf_in, ld_out,
                                   ldf_out, s), "crlot_fdl_mac")
        return out

    def convolve(self, x, y=None, stream: int | None = None):
        """x: (S, T) or (T,) float32 device tensor -> y: (S, T + K - 1), the full
        convolution of stream s with filter s mod n_filters (crlot_convolve).  A wider
        y keeps its samples from T + K - 1 on."""
        if x.dim() == 1:
            return self.convolve(x[None], None if y is None else y[None], stream)[0]
        S, T, L, ld_x, ld_y = _convolve_layouts(_tensor_layout(x), None if y is None else _tensor_layout(y),
                                                self.device, self.taps)
        if y is None:
            y = _torch().empty((S, L), dtype=x.dtype, device=x.device)
        elif _tensors_overlap(x, y):
            raise ValueError("y overlaps x")
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_convolve(self._h, x.data_ptr(), y.data_ptr(), S, T, ld_x, ld_y, s), "crlot_convolve")
        return y


# ----------------------------------------------------------------- streaming convolution
def _sconv_hop_layout(layout, device: int, channels: int, block: int, interleaved: bool, what: str = "block"):
    """Validate one block of StreamConvolver.push from its plain description (shape,
    strides in elements, dtype name, device index or None for a host tensor): a dense
    float32 (channels, B) tensor, (B, channels) when interleaved, on `device`."""
    shape, strides, dtype, dev = layout
    want = (int(block), int(channels)) if interleaved else (int(channels), int(block))
    if dtype != "float32":
        raise ValueError(f"{what} must be float32, not {dtype}")
    if dev is None:
        raise ValueError(f"{what} must be a device tensor")
    if int(dev) != int(device):
        raise ValueError(f"{what} must live on the convolver's device {device}, not {dev}")
    if tuple(int(v) for v in shape) != want:
        raise ValueError(f"{what} must have shape {want}, not {tuple(shape)}")
    # (the stride of a dimension of one element addresses nothing)
    if any(n > 1 and int(st) != d for n, st, d in zip(want, strides, (want[1], 1))):
        raise ValueError(f"{what} must be contiguous")
    return want


class StreamConvolver:
    """crlot_convolve per hop with a carried delay line (crlot_stream_convolver_create /
    crlot_stream_convolve_hop): push(block) takes B samples per channel and returns
    block k of the full convolution of everything pushed so far, channel c with filter
    c mod n_filters, bit for bit Convolver.convolve's samples with frame pairing off.
    Blocks are (channels, B) float32 device tensors, (B, channels) when interleaved.
    Keeps `conv` alive; creation touches no device."""

    def __init__(self, conv: Convolver, channels: int, interleaved: bool = False):
        self._h = None
        if not isinstance(conv, Convolver):
            raise ValueError("conv must be a Convolver")
        self.conv, self.channels, self.interleaved = conv, int(channels), bool(interleaved)
        h = C.c_void_p()
        _check(lib().crlot_stream_convolver_create(conv._h, int(channels), C.byref(h)),
               "crlot_stream_convolver_create")
        self._h = h
        _check(lib().crlot_stream_convolver_set_layout(self._h, int(self.interleaved)))
        self.block, self.partitions = conv.block, conv.partitions

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_stream_convolver_destroy(self._h)
            self._h = None
        self.conv = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def prepare(self):
        """Prepare the convolver and allocate and zero the state now."""
        with _torch().cuda.device(self.conv.device):
            _check(lib().crlot_stream_convolver_prepare(self._h), "crlot_stream_convolver_prepare")

    @property
    def state_bytes(self) -> int:
        return _check(int(lib().crlot_stream_convolver_state_bytes(self._h)), "crlot_stream_convolver_state_bytes")

    @property
    def hops(self) -> int:
        n = C.c_int64()
        _check(lib().crlot_stream_convolver_info(self._h, None, None, None, C.byref(n)), "crlot_stream_convolver_info")
        return n.value

    def reset(self):
        _check(lib().crlot_stream_convolver_reset(self._h), "crlot_stream_convolver_reset")

    def set_route(self, route: int = 0):
        """0: the library's choice; 1: one launch per hop; 2: head + tail.  At hop 0 only."""
        _check(lib().crlot_stream_convolver_set_route(self._h, int(route)), "crlot_stream_convolver_set_route")

    def set_prefetch(self, automatic: bool = True):
        _check(lib().crlot_stream_convolver_set_prefetch(self._h, int(bool(automatic))),
               "crlot_stream_convolver_set_prefetch")

    def last_launch(self) -> dict:
        r = SconvLaunch()
        _check(lib().crlot_stream_convolver_last_launch(self._h, C.byref(r)), "crlot_stream_convolver_last_launch")
        d = {k: getattr(r, k) for k, _ in SconvLaunch._fields_}
        d["head_name"] = kernel_name(r.head_kernel) if r.head_kernel else None
        d["tail_name"] = kernel_name(r.tail_kernel) if r.tail_kernel else None
        return d

    def push(self, block, out=None, stream: int | None = None):
        """block: one hop, or None for a block of zeros (a flush or a gap) -> out, output block k."""
        torch = _torch()
        dev = self.conv.device
        shape = (self.block, self.channels) if self.interleaved else (self.channels, self.block)
        if block is not None:
            if not torch.is_tensor(block):
                raise ValueError("block must be a float32 device tensor or None")
            _sconv_hop_layout(_tensor_layout(block), dev, self.channels, self.block, self.interleaved)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=f"cuda:{dev}")
        else:
            if not torch.is_tensor(out):
                raise ValueError("out must be a float32 device tensor")
            _sconv_hop_layout(_tensor_layout(out), dev, self.channels, self.block, self.interleaved, "out")
            if block is not None and _tensors_overlap(block, out):
                raise ValueError("out overlaps block")
        s = _stream_handle(out) if stream is None else stream
        _check(lib().crlot_stream_convolve_hop(self._h, None if block is None else block.data_ptr(), out.data_ptr(),
                                               s), "crlot_stream_convolve_hop")
        return out

    def prefetch(self, stream: int | None = None):
        """Manual prefetch: enqueue the tail of the last hop (nothing when none is pending)."""
        if stream is None:
            stream = _torch().cuda.current_stream(self.conv.device).cuda_stream
        _check(lib().crlot_stream_convolve_prefetch(self._h, stream), "crlot_stream_convolve_prefetch")


# ----------------------------------------------------------------- adaptive filter
class _DeviceFloats:
    """A float32 array in device memory for torch.as_tensor (the CUDA array interface)."""

    def __init__(self, ptr: int, shape):
        self.__cuda_array_interface__ = {"shape": tuple(int(n) for n in shape), "typestr": "<f4",
                                         "data": (int(ptr), False), "version": 2, "strides": None}


class AdaptiveFilter:
    """The partitioned-block frequency-domain adaptive filter (crlot_fdaf_create /
    crlot_fdaf_hop): push(x, d) takes B samples per channel of the reference x and of the
    desired signal d and returns the error e = d - y, y the output of a K-tap filter
    per channel that adapts to make e small.  Blocks are (channels, B) float32 device
    tensors, (B, channels) when interleaved.  Creation touches no device; the state
    lives on the device that is current at prepare() or at the first call needing it."""

    def __init__(self, block: int, taps: int, channels: int, interleaved: bool = False):
        self._h = None
        h = C.c_void_p()
        _check(lib().crlot_fdaf_create(int(block), int(taps), int(channels), C.byref(h)), "crlot_fdaf_create")
        self._h = h
        self.block, self.taps_count, self.channels, self.interleaved = int(block), int(taps), int(channels), bool(interleaved)
        self.partitions = -(-int(taps) // int(block))
        self.bins = int(block) + 1
        self._device = None
        _check(lib().crlot_fdaf_set_layout(self._h, int(self.interleaved)))

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_fdaf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    @property
    def device(self) -> int:
        """The device of the state (the current device until the state exists)."""
        if self._device is None:
            return int(_torch().cuda.current_device())
        return self._device

    def prepare(self):
        """Make the internal plan and allocate and zero the state now, on the current device."""
        if self._device is None:
            dev = int(_torch().cuda.current_device())
            _check(lib().crlot_fdaf_prepare(self._h), "crlot_fdaf_prepare")
            self._device = dev

    @property
    def state_bytes(self) -> int:
        return _check(int(lib().crlot_fdaf_state_bytes(self._h)), "crlot_fdaf_state_bytes")

    @property
    def hops(self) -> int:
        n = C.c_int64()
        _check(lib().crlot_fdaf_info(self._h, None, None, None, None, C.byref(n)), "crlot_fdaf_info")
        return n.value

    def reset(self):
        """Zero the state (the weights too) and the hop counter."""
        _check(lib().crlot_fdaf_reset(self._h), "crlot_fdaf_reset")

    def set_step(self, mu: float = 0.5, lam: float = 0.9, delta: float = 1e-3):
        _check(lib().crlot_fdaf_set_step(self._h, float(mu), float(lam), float(delta)), "crlot_fdaf_set_step")

    def set_constraint(self, mode: int = 1):
        """0: none; 1: round-robin, partition k mod P after hop k; 2: every partition every hop."""
        _check(lib().crlot_fdaf_set_constraint(self._h, int(mode)), "crlot_fdaf_set_constraint")

    def set_adapt(self, on: bool = True):
        _check(lib().crlot_fdaf_set_adapt(self._h, int(bool(on))), "crlot_fdaf_set_adapt")

    def set_taps(self, h):
        """h: (K,) or (1, K) for every channel, or (channels, K), host float32."""
        h = np.ascontiguousarray(h, np.float32)
        h = h[None] if h.ndim == 1 else h
        if h.ndim != 2 or h.shape[1] != self.taps_count or h.shape[0] not in (1, self.channels):
            raise ValueError(f"taps must have shape ({self.taps_count},), (1, {self.taps_count}) or "
                             f"({self.channels}, {self.taps_count}), not {h.shape}")
        self.prepare()
        with _torch().cuda.device(self._device):
            _check(lib().crlot_fdaf_set_taps(self._h, _fptr(h), h.shape[0], h.shape[1]), "crlot_fdaf_set_taps")

    def taps(self) -> np.ndarray:
        """The filters in the time domain, (channels, K) float32, from the device."""
        self.prepare()
        out = np.zeros((self.channels, self.taps_count), np.float32)
        with _torch().cuda.device(self._device):
            _check(lib().crlot_fdaf_get_taps(self._h, _fptr(out), self.taps_count), "crlot_fdaf_get_taps")
        return out

    def state(self) -> dict:
        """The state on the device as float32 torch views (valid while this object lives, zeroed
        by reset): ring and W (channels, P, 2 (B+1)), E and G (channels, 2 (B+1)) as (re, im)
        pairs, pw (channels, B+1), prev (channels, B)."""
        torch = _torch()
        self.prepare()
        ptrs = [C.c_void_p() for _ in range(6)]
        _check(lib().crlot_fdaf_state(self._h, *[C.byref(p) for p in ptrs]), "crlot_fdaf_state")
        Cn, P, row, B = self.channels, self.partitions, 2 * self.bins, self.block
        shapes = {"ring": (Cn, P, row), "W": (Cn, P, row), "pw": (Cn, self.bins), "E": (Cn, row), "G": (Cn, row),
                  "prev": (Cn, B)}
        with torch.cuda.device(self._device):
            return {name: torch.as_tensor(_DeviceFloats(p.value, shape), device=f"cuda:{self._device}")
                    for (name, shape), p in zip(shapes.items(), ptrs)}

    def last_launch(self) -> dict:
        r = FdafLaunch()
        _check(lib().crlot_fdaf_last_launch(self._h, C.byref(r)), "crlot_fdaf_last_launch")
        d = {k: getattr(r, k) for k, _ in FdafLaunch._fields_ if k != "reserved"}
        d["kernels"] = [kid for kid in (r.hop_kernel, r.update_kernel, r.constrain_kernel) if kid]
        d["names"] = [kernel_name(kid) for kid in d["kernels"]]
        return d

    def _block(self, t, what):
        if not _torch().is_tensor(t):
            raise ValueError(f"{what} must be a float32 device tensor")
        _sconv_hop_layout(_tensor_layout(t), self.device, self.channels, self.block, self.interleaved, what)
        return t

    def push(self, x, d, e=None, y=None, stream: int | None = None):
        """x: the reference block, or None for a block of zeros; d: the desired block.  Returns
        e = d - y; y (optional) receives the filter's output."""
        torch = _torch()
        if x is not None:
            self._block(x, "x")
        self._block(d, "d")
        if e is None:
            e = torch.empty_like(d)
        else:
            self._block(e, "e")
        if y is not None:
            self._block(y, "y")
        ins = [t for t in (x, d) if t is not None]
        if any(_tensors_overlap(i, o) for i in ins for o in (e, y) if o is not None) or \
                (y is not None and _tensors_overlap(e, y)):
            raise ValueError("an output block overlaps another block")
        self.prepare()
        s = _stream_handle(d) if stream is None else stream
        _check(lib().crlot_fdaf_hop(self._h, None if x is None else x.data_ptr(), d.data_ptr(), e.data_ptr(),
                                    None if y is None else y.data_ptr(), s), "crlot_fdaf_hop")
        return e

    def constrain(self, p: int = -1, stream: int | None = None):
        """The gradient constraint alone on partition p of every channel (-1: every partition)."""
        self.prepare()
        if stream is None:
            stream = _torch().cuda.current_stream(self._device).cuda_stream
        _check(lib().crlot_fdaf_constrain(self._h, int(p), stream), "crlot_fdaf_constrain")


# ----------------------------------------------------------------- noise suppressor
DENOISE_DEFAULTS = dict(alpha_s=0.8, alpha_p=0.2, alpha_d=0.95, delta=5.0, window=64, alpha_dd=0.98, g_min=0.1)
DENOISE_PLANES = ("S", "Smin", "Stmp", "p", "lam", "A2")


def denoise_desc(**kw) -> DenoiseDesc:
    """A crlot_denoise_desc from DENOISE_DEFAULTS and the overrides given."""
    unknown = set(kw) - set(DENOISE_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown denoise parameters: {sorted(unknown)}")
    v = {**DENOISE_DEFAULTS, **kw}
    return DenoiseDesc(float(v["alpha_s"]), float(v["alpha_p"]), float(v["alpha_d"]), float(v["delta"]),
                       float(v["alpha_dd"]), float(v["g_min"]), int(v["window"]), 0)


class Denoiser:
    """The stationary-noise suppressor (crlot_denoiser_create; MCRA noise tracking and a
    decision-directed Wiener gain): gains(spec) gives the mask rows of a spectrogram,
    denoise(x) is stft -> gains -> masked istft_ola in one call, and Stream.denoise_hop
    runs it per hop with the state carried in this object.  Creation checks the
    parameters (ValueError) and touches no device."""

    def __init__(self, plan: "Plan", channels: int, **params):
        self._h = None
        self.plan, self.channels = plan, int(channels)
        self.bins = plan.frame_size // 2 + 1
        desc = denoise_desc(**params)
        h = C.c_void_p()
        _check(lib().crlot_denoiser_create(plan._h, C.byref(desc), int(channels), C.byref(h)), "crlot_denoiser_create")
        self._h = h
        self.params = {k: getattr(desc, k) for k in DENOISE_DEFAULTS}

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_denoiser_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _info(self):
        ch, bins, route, ok = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        frames = C.c_int64()
        _check(lib().crlot_denoiser_info(self._h, C.byref(ch), C.byref(bins), C.byref(frames), C.byref(route),
                                         C.byref(ok)), "crlot_denoiser_info")
        return {"channels": ch.value, "bins": bins.value, "frames": frames.value, "route": route.value,
                "fused_ok": bool(ok.value)}

    @property
    def frames(self) -> int:
        """Frames the carried state has seen since create / reset."""
        return self._info()["frames"]

    @property
    def fused_ok(self) -> bool:
        return self._info()["fused_ok"]

    def prepare(self):
        with _torch().cuda.device(self.plan._device_index()):
            _check(lib().crlot_denoiser_prepare(self._h), "crlot_denoiser_prepare")

    def reset(self):
        """Zero the state and the frame counter."""
        _check(lib().crlot_denoiser_reset(self._h), "crlot_denoiser_reset")

    def set_route(self, route: int = 0):
        """The per-hop route: 0 the library's choice, 1 fused (one launch), 2 staged (three)."""
        _check(lib().crlot_denoiser_set_route(self._h, int(route)), "crlot_denoiser_set_route")

    def state(self):
        """The carried state on the device, a (channels, 6, N/2+1) float32 torch view in
        DENOISE_PLANES order (valid while this object lives, zeroed by reset)."""
        torch = _torch()
        ptr = C.c_void_p()
        dev = self.plan._device_index()
        with torch.cuda.device(dev):
            _check(lib().crlot_denoiser_state(self._h, C.byref(ptr)), "crlot_denoiser_state")
            return torch.as_tensor(_DeviceFloats(ptr.value, (self.channels, 6, self.bins)), device=f"cuda:{dev}")

    def last_launch(self) -> dict:
        r = DenoiseLaunch()
        _check(lib().crlot_denoiser_last_launch(self._h, C.byref(r)), "crlot_denoiser_last_launch")
        kernels = [int(r.kernel[i]) for i in range(r.n_kernels)]
        return {"route": r.route, "kernels": kernels, "names": [kernel_name(k) for k in kernels],
                "grids": [int(r.grid[i]) for i in range(r.n_kernels)]}

    def gains(self, spec, mask=None, carry: bool = False, stream: int | None = None):
        """spec: (S, F, N/2+1) or (F, N/2+1) complex64 device tensor -> the gain rows, float32
        of the same shape (what Plan.set_spectral_mask takes).  carry=False: every stream
        starts at frame 0 and the object's state is left alone; carry=True: S must be the
        channel count, the run continues from the object's state and advances it."""
        torch = _torch()
        if len(spec.shape) == 2:
            return self.gains(spec[None], None if mask is None else mask[None], carry, stream)[0]
        dev = self.plan._device_index()
        ld_s, ldf_s = _stretch_spec_layout(*_tensor_layout(spec), dev, self.bins)
        S, F = int(spec.shape[0]), int(spec.shape[1])
        if carry and S != self.channels:
            raise ValueError(f"carry needs {self.channels} streams, not {S}")
        if mask is None:
            mask = torch.empty((S, F, self.bins), dtype=torch.float32, device=spec.device)
        _, _, ld_m, ldf_m = _gl_mag_layout(*_tensor_layout(mask), dev, self.bins, "mask", (S, F, self.bins))
        if _tensors_overlap(mask, spec):
            raise ValueError("mask overlaps spec")
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_denoise_gains(self._h, spec.data_ptr(), mask.data_ptr(), S, F, ld_s, ldf_s, ld_m, ldf_m,
                                         int(bool(carry)), s), "crlot_denoise_gains")
        return mask

    def denoise(self, x, y=None, stream: int | None = None):
        """x: (S, T) or (T,) float32 device tensor -> y: (S, F * H), istft_ola of stft(x) under
        gains(stft(x)), bit for bit, with the spectra and the gains in the plan's scratch.
        The plan must have no stored spectral mask."""
        if x.dim() == 1:
            return self.denoise(x[None], None if y is None else y[None], stream)[0]
        S, T = _spectrogram_x_layout(*_tensor_layout(x))
        if getattr(self.plan, "_mask", None) is not None:
            raise ValueError("denoise: the plan has a stored spectral mask; clear it first")
        L = self.plan.frame_count(T) * self.plan.hop_size
        if y is None:
            y = _torch().empty((S, L), dtype=x.dtype, device=x.device)
        ld_y = _gl_y_layout(*_tensor_layout(y), self.plan._device_index(), S, L)
        if _tensors_overlap(y, x):
            raise ValueError("y overlaps x")
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_denoise(self._h, x.data_ptr(), y.data_ptr(), S, T, _ld(x, 0, T), ld_y, s), "crlot_denoise")
        return y


# ----------------------------------------------------------------- cross-spectral estimation
XSPEC_PLANES = ("Saa", "Sbb", "Sr", "Si")
XSPEC_NONE, XSPEC_PHAT = 0, 1


def _xspec_rows_layout(shape, strides, dtype: str, device_index, plan_device: int, P: int, width: int, want: str,
                       what: str):
    """Validate one row per pair from its plain description (shape and strides in elements
    as tuples, dtype name, device index or None for a host tensor): (P, width) of dtype
    `want` on the plan's device, rows contiguous and at least `width` apart.  Returns the
    row stride in elements."""
    shape, strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
    if shape != (P, width) or len(strides) != 2:
        raise ValueError(f"{what} must be ({P}, {width}), not {shape}")
    if dtype != want:
        raise ValueError(f"{what} must be {want}, not {dtype}")
    if device_index is None or int(device_index) != int(plan_device):
        raise ValueError(f"{what} must live on the plan's device {plan_device}, not "
                         f"{'the host' if device_index is None else device_index}")
    if width > 1 and strides[1] != 1:
        raise ValueError(f"{what} must have contiguous rows")
    ld = strides[0] if P > 1 else width  # (a size-1 dim's stride is meaningless)
    if ld < width:
        raise ValueError(f"{what} rows overlap: the row stride is below {width}")
    return ld


class CrossSpectrum:
    """The cross-spectral estimator (crlot_xspec_create): averaged Saa, Sbb and Sab =
    conj(A) B of `pairs` pairs of spectra along the frame axis (alpha 0: Welch sums, alpha
    in (0, 1): exponential averaging), and what follows from them: coherence(), transfer()
    (H1 = Sab / Saa), weighted() and delay() (GCC-PHAT: the lag of b against a, positive
    when b is late).  accumulate takes spectra, estimate takes signals; carry=True
    continues from and advances this object's state.  Creation checks alpha (ValueError)
    and touches no device."""

    def __init__(self, plan: "Plan", pairs: int, alpha: float = 0.0):
        self._h = None
        self.plan, self.pairs, self.alpha = plan, int(pairs), float(alpha)
        self.bins = plan.frame_size // 2 + 1
        h = C.c_void_p()
        _check(lib().crlot_xspec_create(plan._h, int(pairs), float(alpha), C.byref(h)), "crlot_xspec_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_xspec_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _info(self):
        pairs, bins, frames = C.c_int32(), C.c_int32(), C.c_int64()
        lam, om = C.c_float(), C.c_float()
        _check(lib().crlot_xspec_info(self._h, C.byref(pairs), C.byref(bins), C.byref(frames), C.byref(lam),
                                      C.byref(om)), "crlot_xspec_info")
        return {"pairs": pairs.value, "bins": bins.value, "frames": frames.value, "lambda": lam.value,
                "omega": om.value}

    @property
    def frames(self) -> int:
        """Frames the carried state has seen since create / reset."""
        return self._info()["frames"]

    @property
    def factors(self) -> tuple:
        """(lambda, omega) as the kernels use them: (1, 1) for Welch sums."""
        i = self._info()
        return i["lambda"], i["omega"]

    def prepare(self):
        with _torch().cuda.device(self.plan._device_index()):
            _check(lib().crlot_xspec_prepare(self._h), "crlot_xspec_prepare")

    def reset(self):
        """Zero the state and the frame counter."""
        _check(lib().crlot_xspec_reset(self._h), "crlot_xspec_reset")

    def state(self):
        """The carried state on the device, a (pairs, 4, N/2+1) float32 torch view in
        XSPEC_PLANES order (valid while this object lives, zeroed by reset)."""
        torch = _torch()
        ptr = C.c_void_p()
        dev = self.plan._device_index()
        with torch.cuda.device(dev):
            _check(lib().crlot_xspec_state(self._h, C.byref(ptr)), "crlot_xspec_state")
            return torch.as_tensor(_DeviceFloats(ptr.value, (self.pairs, 4, self.bins)), device=f"cuda:{dev}")

    def last_launch(self) -> dict:
        r = XspecLaunch()
        _check(lib().crlot_xspec_last_launch(self._h, C.byref(r)), "crlot_xspec_last_launch")
        kernels = [int(r.kernel[i]) for i in range(r.n_kernels)]
        return {"kernels": kernels, "names": [kernel_name(k) for k in kernels],
                "grids": [int(r.grid[i]) for i in range(r.n_kernels)]}

    def _state_out(self, P: int, carry: bool, state_out, like, *inputs):
        """The state output of accumulate / estimate: checked, or allocated when a fresh run needs one."""
        torch = _torch()
        if carry and P != self.pairs:
            raise ValueError(f"carry needs {self.pairs} pairs, not {P}")
        if state_out is None:
            if carry:
                return None
            return torch.empty((P, 4, self.bins), dtype=torch.float32, device=like.device)
        shape, strides, dtype, dev = _tensor_layout(state_out)
        if shape != (P, 4, self.bins) or dtype != "float32" or not state_out.is_contiguous():
            raise ValueError(f"state_out must be a contiguous ({P}, 4, {self.bins}) float32 tensor")
        if dev is None or dev != self.plan._device_index():
            raise ValueError("state_out must live on the plan's device")
        if any(_tensors_overlap(state_out, t) for t in inputs):
            raise ValueError("state_out overlaps an input")
        return state_out

    def accumulate(self, a, b, carry: bool = False, state_out=None, stream: int | None = None):
        """a, b: (P, F, N/2+1) complex64 device tensors, Plan.stft's layout; a may be
        (F, N/2+1): one reference shared by every pair.  carry=False: fresh state, any P, the
        result in state_out (allocated when None), this object untouched.  carry=True: P must
        be the pair count; the run continues from this object's state and advances it.
        Returns the (P, 4, N/2+1) state the run ends with (the live view for carry=True
        without a state_out)."""
        if len(b.shape) == 2:
            b = b[None]
        dev = self.plan._device_index()
        P, F = int(b.shape[0]), int(b.shape[1])
        shared = len(a.shape) == 2
        a3 = a[None] if shared else a
        ld_b, ldf_b = _stretch_spec_layout(*_tensor_layout(b), dev, self.bins, "b")
        ld_a, ldf_a = _stretch_spec_layout(*_tensor_layout(a3), dev, self.bins, "a",
                                           expect=(1 if shared else P, F, self.bins))
        out = self._state_out(P, carry, state_out, b, a, b)
        s = _stream_handle(b) if stream is None else stream
        _check(lib().crlot_xspec_accumulate(self._h, a.data_ptr(), b.data_ptr(), P, F, 0 if shared else ld_a, ldf_a, ld_b,
                                            ldf_b, int(bool(carry)), None if out is None else out.data_ptr(), s),
               "crlot_xspec_accumulate")
        return self.state() if out is None else out

    def estimate(self, xa, xb, carry: bool = False, state_out=None, stream: int | None = None):
        """xa, xb: (P, T) float32 device tensors; xa may be (T,): one reference shared by every
        pair.  accumulate(stft(xa), stft(xb)) bit for bit, with the spectra in the plan's
        scratch.  Returns the state as accumulate does."""
        if xb.dim() == 1:
            xb = xb[None]
        P, T = _spectrogram_x_layout(*_tensor_layout(xb))
        shared = xa.dim() == 1
        Pa, Ta = _spectrogram_x_layout(*_tensor_layout(xa[None] if shared else xa))
        if Ta != T or (not shared and Pa != P):
            raise ValueError("xa must be (T,) or match xb's (P, T)")
        dev = self.plan._device_index()
        for t, what in ((xa, "xa"), (xb, "xb")):
            if (t.device.index if t.device.index is not None else 0) != dev:
                raise ValueError(f"{what} must live on the plan's device {dev}")
        ld_xb = _ld(xb, 0, T)
        ld_xa = 0 if shared else _ld(xa, 0, T)
        if ld_xb < T or (not shared and ld_xa < T):
            raise ValueError("rows overlap: the stream stride is below T")
        out = self._state_out(P, carry, state_out, xb, xa, xb)
        s = _stream_handle(xb) if stream is None else stream
        _check(lib().crlot_xspec_estimate(self._h, xa.data_ptr(), xb.data_ptr(), P, T, ld_xa, ld_xb, int(bool(carry)),
                                          None if out is None else out.data_ptr(), s), "crlot_xspec_estimate")
        return self.state() if out is None else out

    def _state_in(self, state):
        """(data pointer or None, P, a tensor on the device) of the state a derive / delay call reads."""
        if state is None:
            return None, self.pairs, self.state()
        shape, strides, dtype, dev = _tensor_layout(state)
        if len(shape) != 3 or shape[1:] != (4, self.bins) or dtype != "float32" or not state.is_contiguous():
            raise ValueError(f"state must be a contiguous (P, 4, {self.bins}) float32 tensor")
        if dev is None or dev != self.plan._device_index():
            raise ValueError("state must live on the plan's device")
        return state.data_ptr(), int(shape[0]), state

    def derive(self, state=None, weighting: int = XSPEC_NONE, want=("coherence", "transfer", "weighted"),
               coherence=None, transfer=None, weighted=None, stream: int | None = None) -> dict:
        """The rows derived from a state block (None: this object's) in one pass: any of
        "coherence" (P, N/2+1) float32, "transfer" (H1) and "weighted" (the cross-spectrum
        under `weighting`: XSPEC_NONE or XSPEC_PHAT), both (P, N/2+1) complex64.  `want`
        names the outputs; a tensor passed for one is written in place.  Returns a dict."""
        torch = _torch()
        names = ("coherence", "transfer", "weighted")
        given = dict(zip(names, (coherence, transfer, weighted)))
        want = set(want) | {k for k, v in given.items() if v is not None}
        if not want or not want <= set(names):
            raise ValueError(f"want must name at least one of {names}")
        if int(weighting) not in (XSPEC_NONE, XSPEC_PHAT):
            raise ValueError("weighting must be XSPEC_NONE or XSPEC_PHAT")
        ptr, P, st = self._state_in(state)
        dev = self.plan._device_index()
        outs, args = {}, []
        for k in names:
            if k not in want:
                args += [None, 0]
                continue
            cplx = k != "coherence"
            t = given[k]
            if t is None:
                t = torch.empty((P, self.bins), dtype=torch.complex64 if cplx else torch.float32, device=st.device)
            ld = _xspec_rows_layout(*_tensor_layout(t), dev, P, self.bins, "complex64" if cplx else "float32", k)
            if _tensors_overlap(t, st) or any(_tensors_overlap(t, o) for o in outs.values()):
                raise ValueError(f"{k} overlaps the state or another output")
            outs[k] = t
            args += [t.data_ptr(), 2 * ld if cplx else ld]
        s = _stream_handle(st) if stream is None else stream
        _check(lib().crlot_xspec_derive(self._h, ptr, P, int(weighting), *args, s), "crlot_xspec_derive")
        return outs

    def coherence(self, state=None, stream: int | None = None):
        """The magnitude-squared coherence |Sab|^2 / (Saa Sbb), (P, N/2+1) float32, not clamped."""
        return self.derive(state, want=("coherence",), stream=stream)["coherence"]

    def transfer(self, state=None, stream: int | None = None):
        """H1 = Sab / Saa, (P, N/2+1) complex64: Plan.irfft of it is the impulse response from a to b."""
        return self.derive(state, want=("transfer",), stream=stream)["transfer"]

    def weighted(self, state=None, weighting: int = XSPEC_PHAT, stream: int | None = None):
        """The cross-spectrum under `weighting`, (P, N/2+1) complex64."""
        return self.derive(state, weighting, want=("weighted",), stream=stream)["weighted"]

    def _lag(self, max_lag) -> int:
        n = self.plan.frame_size
        m = n // 2 - 1 if max_lag is None else int(max_lag)
        if not 1 <= m <= n // 2 - 1:
            raise ValueError(f"max_lag must lie in [1, {n // 2 - 1}] (a longer search takes a longer frame)")
        return m

    def _peak_out(self, P: int, out, like):
        if out is None:
            return _torch().empty((P, 3), dtype=_torch().float32, device=like.device), 3
        return out, _xspec_rows_layout(*_tensor_layout(out), self.plan._device_index(), P, 3, "float32", "out")

    def peak(self, cc, max_lag=None, out=None, stream: int | None = None):
        """cc: (P, N) float32 correlation rows -> (P, 3) float32 rows {lag, frac, value}: the
        first maximum over the lags -max_lag .. max_lag (None: N/2 - 1) and its parabolic
        refinement; lag + frac is the delay in samples."""
        m = self._lag(max_lag)
        if len(cc.shape) != 2:
            raise ValueError("cc must be (P, N)")
        P = int(cc.shape[0])
        ld_cc = _xspec_rows_layout(*_tensor_layout(cc), self.plan._device_index(), P, self.plan.frame_size, "float32",
                                   "cc")
        out, ld_out = self._peak_out(P, out, cc)
        if _tensors_overlap(out, cc):
            raise ValueError("out overlaps cc")
        s = _stream_handle(cc) if stream is None else stream
        _check(lib().crlot_xspec_peak(self._h, cc.data_ptr(), ld_cc, P, m, out.data_ptr(), ld_out, s), "crlot_xspec_peak")
        return out

    def delay(self, state=None, weighting: int = XSPEC_PHAT, max_lag=None, out=None, stream: int | None = None):
        """peak(Plan.irfft(weighted(state, weighting)), max_lag) bit for bit, the rows between
        in the plan's scratch: (P, 3) float32 rows {lag, frac, value} of b against a."""
        m = self._lag(max_lag)
        if int(weighting) not in (XSPEC_NONE, XSPEC_PHAT):
            raise ValueError("weighting must be XSPEC_NONE or XSPEC_PHAT")
        ptr, P, st = self._state_in(state)
        out, ld_out = self._peak_out(P, out, st)
        if _tensors_overlap(out, st):
            raise ValueError("out overlaps the state")
        s = _stream_handle(st) if stream is None else stream
        _check(lib().crlot_xspec_delay(self._h, ptr, P, int(weighting), m, out.data_ptr(), ld_out, s), "crlot_xspec_delay")
        return out


# ----------------------------------------------------------------- beamformer
BF_SOUDEN, BF_STEERED = 0, 1
BF_TARGET_BOTH, BF_TARGET_SPEECH, BF_TARGET_NOISE = 0, 1, 2
_BF_MODES = {"souden": BF_SOUDEN, "steered": BF_STEERED, BF_SOUDEN: BF_SOUDEN, BF_STEERED: BF_STEERED}


def steering_from_delays(delays, nfft: int):
    """The steering vectors exp(-2 pi i b tau / N) of microphones delayed by tau samples
    against the reference microphone (what CrossSpectrum.delay returns against it: lag +
    frac): delays (..., M) -> (..., M, N/2+1) complex64, computed in float64 and rounded
    once.  A host helper: no device, and no bit parity with anything else is claimed."""
    if int(nfft) < 2 or int(nfft) % 2:
        raise ValueError("nfft must be even and at least 2")
    tau = np.asarray(delays, np.float64)[..., None]
    if not np.all(np.isfinite(tau)):
        raise ValueError("delays must be finite")
    b = np.arange(int(nfft) // 2 + 1, dtype=np.float64)
    return np.exp(-2j * np.pi * b * tau / int(nfft)).astype(np.complex64)


def _bf_spec_layout(shape, strides, dtype: str, device_index, plan_device: int, M: int, bins: int, what: str = "spec"):
    """Validate the beamformer's spectra from their plain description (shape and strides in
    complex elements as tuples, dtype name, device index or None for a host tensor): (G, M,
    F, bins) complex64 on the plan's device, rows contiguous and at least `bins` apart,
    microphones not overlapping and the groups M microphone strides apart (stream g M + m).
    Returns (G, F, ld_spec, ldf_spec) in floats."""
    shape, strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
    if len(shape) != 4 or len(strides) != 4 or shape[1] != M or shape[3] != bins or min(shape) < 1:
        raise ValueError(f"{what} must be (G, {M}, F, {bins}) or ({M}, F, {bins}) complex64")
    if dtype != "complex64":
        raise ValueError(f"{what} must be complex64, not {dtype}")
    if device_index is None or int(device_index) != int(plan_device):
        raise ValueError(f"{what} must live on the plan's device {plan_device}, not "
                         f"{'the host' if device_index is None else device_index}")
    if strides[3] != 1:
        raise ValueError(f"{what} must have contiguous rows")
    G, F = shape[0], shape[2]
    ldf = strides[2] if F > 1 else bins
    ld = strides[1]
    if ldf < bins or ld < (F - 1) * ldf + bins:
        raise ValueError(f"{what} rows overlap")
    if G > 1 and strides[0] != M * ld:
        raise ValueError(f"{what}: the groups must be {M} microphone strides apart (stream g M + m)")
    return G, F, 2 * ld, 2 * ldf


def _bf_mask_layout(shape, strides, dtype: str, device_index, plan_device: int, G: int, F: int, bins: int):
    """The same for a mask: (G, F, bins) float32, or (F, bins): one set of rows for every
    group.  Returns (ld_mask, ldf_mask), ld_mask 0 for a shared mask."""
    shape, strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
    if shape not in ((G, F, bins), (F, bins)) or len(strides) != len(shape):
        raise ValueError(f"mask must be ({G}, {F}, {bins}) or ({F}, {bins}), not {shape}")
    if dtype != "float32":
        raise ValueError(f"mask must be float32, not {dtype}")
    if device_index is None or int(device_index) != int(plan_device):
        raise ValueError(f"mask must live on the plan's device {plan_device}, not "
                         f"{'the host' if device_index is None else device_index}")
    if strides[-1] != 1:
        raise ValueError("mask must have contiguous rows")
    ldf = strides[-2] if F > 1 else bins
    if ldf < bins:
        raise ValueError("mask rows overlap")
    if len(shape) == 2:
        return 0, ldf
    ld = strides[0] if G > 1 else F * ldf
    if G > 1 and ld == 0:
        return 0, ldf  # (an expanded mask: one set of rows)
    if ld < (F - 1) * ldf + bins:
        raise ValueError("mask rows overlap")
    return (ld if G > 1 else 0), ldf


class Beamformer:
    """The mask-driven MVDR beamformer (crlot_beamformer_create): `groups` independent
    arrays of `mics` microphones (2..8), one output per group.  accumulate averages the
    target and noise spatial covariance matrices per bin from spectra (Plan.stft's layout,
    (G, M, F, N/2+1)) under a mask ((G, F, N/2+1) or shared (F, N/2+1)), solve turns a state
    into weights (mode "souden": mask-based, against microphone `ref`; "steered": the
    classical MVDR towards steering()), apply forms y = w^H x per frame, beamform runs
    stft -> accumulate -> solve -> apply -> istft_ola on signals, hop is the per-hop chain.
    Creation checks the descriptor (ValueError) and touches no device."""

    def __init__(self, plan: "Plan", mics: int, groups: int = 1, ref: int = 0, mode="souden", alpha: float = 0.0,
                 loading: float = 1e-3, update_every: int = 1):
        self._h = None
        if isinstance(mode, str):
            mode = mode.lower()
        if mode not in _BF_MODES:
            raise ValueError('mode must be "souden" or "steered"')
        self.plan, self.mics, self.groups, self.ref = plan, int(mics), int(groups), int(ref)
        self.mode, self.alpha, self.loading, self.update_every = _BF_MODES[mode], float(alpha), float(loading), int(update_every)
        self.bins = plan.frame_size // 2 + 1
        d = BeamformDesc(self.mics, self.ref, self.mode, self.update_every, self.alpha, self.loading)
        h = C.c_void_p()
        _check(lib().crlot_beamformer_create(plan._h, C.byref(d), self.groups, C.byref(h)), "crlot_beamformer_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_beamformer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _info(self):
        g, m, b, fr = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        lam, om, ld = C.c_float(), C.c_float(), C.c_float()
        _check(lib().crlot_beamformer_info(self._h, C.byref(g), C.byref(m), C.byref(b), C.byref(fr), C.byref(lam),
                                           C.byref(om), C.byref(ld)), "crlot_beamformer_info")
        return {"groups": g.value, "mics": m.value, "bins": b.value, "frames": fr.value, "lambda": lam.value,
                "omega": om.value, "loading": ld.value}

    @property
    def frames(self) -> int:
        """Frames the carried state has seen since create / reset."""
        return self._info()["frames"]

    @property
    def factors(self) -> tuple:
        """(lambda, omega, loading) as the kernels use them."""
        i = self._info()
        return i["lambda"], i["omega"], i["loading"]

    def prepare(self):
        with _torch().cuda.device(self.plan._device_index()):
            _check(lib().crlot_beamformer_prepare(self._h), "crlot_beamformer_prepare")

    def reset(self):
        """Zero the state and the frame counter, restore the pass-through weights (the steering block stays)."""
        _check(lib().crlot_beamformer_reset(self._h), "crlot_beamformer_reset")

    def _view(self, fn, name, shape, cplx):
        torch = _torch()
        ptr = C.c_void_p()
        dev = self.plan._device_index()
        with torch.cuda.device(dev):
            _check(fn(self._h, C.byref(ptr)), name)
            t = torch.as_tensor(_DeviceFloats(ptr.value, shape + ((2,) if cplx else ())), device=f"cuda:{dev}")
        return torch.view_as_complex(t) if cplx else t

    def state(self):
        """The carried state on the device, a (groups, 2, M M, N/2+1) float32 torch view: the
        target matrix then the noise matrix, each the M diagonals, then Re, Im of every i < j."""
        return self._view(lib().crlot_beamformer_state, "crlot_beamformer_state",
                          (self.groups, 2, self.mics * self.mics, self.bins), False)

    def weights(self):
        """The object's weights, a (groups, M, N/2+1) complex64 torch view."""
        return self._view(lib().crlot_beamformer_weights, "crlot_beamformer_weights", (self.groups, self.mics, self.bins),
                          True)

    def steering(self):
        """The object's steering vectors (STEERED mode), a (groups, M, N/2+1) complex64 torch view."""
        return self._view(lib().crlot_beamformer_steering, "crlot_beamformer_steering",
                          (self.groups, self.mics, self.bins), True)

    def _set(self, view, value, what):
        torch = _torch()
        v = torch.as_tensor(np.ascontiguousarray(value, np.complex64)) if not torch.is_tensor(value) else value
        if v.dtype != torch.complex64:
            raise ValueError(f"{what} must be complex64")
        if tuple(v.shape) == (self.mics, self.bins):
            v = v[None].expand(self.groups, -1, -1)
        if tuple(v.shape) != (self.groups, self.mics, self.bins):
            raise ValueError(f"{what} must be ({self.groups}, {self.mics}, {self.bins}) or ({self.mics}, {self.bins})")
        view.copy_(v.to(view.device))

    def set_weights(self, w):
        """Replace the object's weights: (groups, M, N/2+1) or (M, N/2+1) complex64, host or device."""
        self._set(self.weights(), w, "weights")

    def set_steering(self, d):
        """Replace the object's steering vectors (see steering_from_delays)."""
        self._set(self.steering(), d, "steering")

    def last_launch(self) -> dict:
        r = BeamformLaunch()
        _check(lib().crlot_beamformer_last_launch(self._h, C.byref(r)), "crlot_beamformer_last_launch")
        kernels = [int(r.kernel[i]) for i in range(r.n_kernels)]
        return {"kernels": kernels, "names": [kernel_name(k) for k in kernels],
                "grids": [int(r.grid[i]) for i in range(r.n_kernels)]}

    def _spec(self, spec, what="spec"):
        if len(spec.shape) == 3:
            spec = spec[None]
        G, F, ld, ldf = _bf_spec_layout(*_tensor_layout(spec), self.plan._device_index(), self.mics, self.bins, what)
        return spec, G, F, ld, ldf

    def _block(self, t, G, cplx, what):
        """A caller's state / weights / steering block: (data pointer, tensor), checked."""
        shape = (G, self.mics, self.bins) if cplx else (G, 2, self.mics * self.mics, self.bins)
        want = "complex64" if cplx else "float32"
        tshape, _, dtype, dev = _tensor_layout(t)
        if tshape != shape or dtype != want or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {shape} {want} tensor")
        if dev is None or dev != self.plan._device_index():
            raise ValueError(f"{what} must live on the plan's device")
        return t.data_ptr()

    def accumulate(self, spec, mask=None, target: int = BF_TARGET_BOTH, carry: bool = False, state_out=None,
                   stream: int | None = None):
        """spec: (G, M, F, N/2+1) or (M, F, N/2+1) complex64 device tensor, Plan.stft's rows of
        stream g M + m.  mask: (G, F, N/2+1) float32, or (F, N/2+1) shared by every group;
        None (targets 1, 2): 1.  target BF_TARGET_BOTH: the target matrix with weight mask
        and the noise matrix with 1 - mask; BF_TARGET_SPEECH / BF_TARGET_NOISE: that matrix
        alone with weight mask.  carry=False: fresh state, any G, the result in state_out
        (allocated zeroed when None), this object untouched.  carry=True: G must be the group
        count; the run continues from this object's state and advances it.  Returns the
        (G, 2, M M, N/2+1) state the run ends with (the live view for carry=True without a
        state_out)."""
        torch = _torch()
        spec, G, F, ld, ldf = self._spec(spec)
        if int(target) not in (0, 1, 2):
            raise ValueError("target must be BF_TARGET_BOTH, BF_TARGET_SPEECH or BF_TARGET_NOISE")
        if int(target) == 0 and mask is None:
            raise ValueError("target BF_TARGET_BOTH needs a mask")
        if carry and G != self.groups:
            raise ValueError(f"carry needs {self.groups} groups, not {G}")
        mp, ldm, ldfm = None, 0, 0
        if mask is not None:
            ldm, ldfm = _bf_mask_layout(*_tensor_layout(mask), self.plan._device_index(), G, F, self.bins)
            mp = mask.data_ptr()
        out = state_out
        if out is None and not carry:
            out = torch.zeros((G, 2, self.mics * self.mics, self.bins), dtype=torch.float32, device=spec.device)
        op = None
        if out is not None:
            op = self._block(out, G, False, "state_out")
            if _tensors_overlap(out, spec) or (mask is not None and _tensors_overlap(out, mask)):
                raise ValueError("state_out overlaps an input")
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_beamform_accumulate(self._h, spec.data_ptr(), ld, ldf, mp, ldm, ldfm, G, F, int(target),
                                               int(bool(carry)), op, s), "crlot_beamform_accumulate")
        return self.state() if out is None else out

    def solve(self, state=None, steering=None, weights=None, stream: int | None = None):
        """The weights of a state block (None: this object's) in this object's mode; steering
        (STEERED mode; None: this object's) and weights (None: this object's, which is
        returned) are (G, M, N/2+1) complex64 device tensors."""
        G = self.groups if state is None else int(state.shape[0])
        sp = None if state is None else self._block(state, G, False, "state")
        dp = None if steering is None else self._block(steering, G, True, "steering")
        wp = None if weights is None else self._block(weights, G, True, "weights")
        if weights is not None and any(t is not None and _tensors_overlap(weights, t) for t in (state, steering)):
            raise ValueError("weights overlap the state or the steering block")
        if G != self.groups and (state is None or weights is None or (steering is None and self.mode == BF_STEERED)):
            raise ValueError(f"this object's blocks need {self.groups} groups, not {G}")
        like = next((t for t in (state, weights, steering) if t is not None), None)
        s = stream if stream is not None else (_stream_handle(like) if like is not None else _stream_handle(self.state()))
        with _torch().cuda.device(self.plan._device_index()):
            _check(lib().crlot_beamform_solve(self._h, sp, dp, G, wp, s), "crlot_beamform_solve")
        return self.weights() if weights is None else weights

    def apply(self, spec, weights=None, out=None, stream: int | None = None):
        """spec as accumulate's -> (G, F, N/2+1) complex64: sum over m of conj(w_m) x_m per frame
        and bin, with `weights` ((G, M, N/2+1) complex64; None: this object's)."""
        torch = _torch()
        squeeze = len(spec.shape) == 3
        spec, G, F, ld, ldf = self._spec(spec)
        wp = None if weights is None else self._block(weights, G, True, "weights")
        if weights is None and G != self.groups:
            raise ValueError(f"this object's weights need {self.groups} groups, not {G}")
        if out is None:
            out = torch.empty((G, F, self.bins), dtype=torch.complex64, device=spec.device)
        o3 = out[None] if len(out.shape) == 2 else out
        ld_o, ldf_o = _stretch_spec_layout(*_tensor_layout(o3), self.plan._device_index(), self.bins, "out",
                                           expect=(G, F, self.bins))
        if _tensors_overlap(o3, spec) or (weights is not None and _tensors_overlap(o3, weights)):
            raise ValueError("out overlaps an input")
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_beamform_apply(self._h, spec.data_ptr(), ld, ldf, wp, G, F, o3.data_ptr(), ld_o, ldf_o, s),
               "crlot_beamform_apply")
        return o3[0] if squeeze and len(out.shape) == 3 else out

    def beamform(self, x, mask=None, y=None, stream: int | None = None):
        """x: (G, M, T) or (M, T) float32 device tensor -> y: (G, F H): istft_ola of apply(stft(x))
        under solve(accumulate(stft(x), mask)), bit for bit, everything between in the plan's
        scratch; this object's state and weights are untouched.  mask as accumulate's; None
        is allowed in STEERED mode only (the noise matrix from every frame with weight 1: the
        minimum-power form).  The plan must have no stored spectral mask."""
        torch = _torch()
        squeeze = x.dim() == 2
        if squeeze:
            x = x[None]
        shape, strides, dtype, dev = _tensor_layout(x)
        if len(shape) != 3 or shape[1] != self.mics or dtype != "float32" or dev is None:
            raise ValueError(f"x must be a (G, {self.mics}, T) or ({self.mics}, T) float32 device tensor")
        if dev != self.plan._device_index():
            raise ValueError(f"x must live on the plan's device {self.plan._device_index()}")
        G, T = int(shape[0]), int(shape[2])
        if T > 1 and strides[2] != 1:
            raise ValueError("x must have contiguous rows")
        ld_x = int(strides[1])
        if ld_x < T or (G > 1 and int(strides[0]) != self.mics * ld_x):
            raise ValueError(f"x: rows overlap, or the groups are not {self.mics} microphone strides apart")
        if getattr(self.plan, "_mask", None) is not None:
            raise ValueError("beamform: the plan has a stored spectral mask; clear it first")
        if mask is None and self.mode != BF_STEERED:
            raise ValueError("SOUDEN mode needs a mask")
        if self.mode == BF_STEERED and G != self.groups:
            raise ValueError(f"STEERED mode reads this object's steering block: {self.groups} groups, not {G}")
        F = self.plan.frame_count(T)
        L = F * self.plan.hop_size
        mp, ldm, ldfm = None, 0, 0
        if mask is not None:
            ldm, ldfm = _bf_mask_layout(*_tensor_layout(mask), dev, G, F, self.bins)
            mp = mask.data_ptr()
        if y is None:
            y = torch.empty((G, L), dtype=x.dtype, device=x.device)
        y2 = y[None] if y.dim() == 1 else y
        ld_y = _gl_y_layout(*_tensor_layout(y2), dev, G, L)
        if _tensors_overlap(y2, x) or (mask is not None and _tensors_overlap(y2, mask)):
            raise ValueError("y overlaps an input")
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_beamform(self._h, x.data_ptr(), ld_x, mp, ldm, ldfm, y2.data_ptr(), ld_y, G, T, s),
               "crlot_beamform")
        return y2[0] if squeeze and y.dim() == 2 else y

    def hop(self, st_in: "Stream", st_out: "Stream", hop, mask, out=None, stream: int | None = None) -> tuple:
        """One hop of the per-hop chain (crlot_stream_beamform_hop): st_in a Stream of groups x
        mics channels (its analysis half), st_out one of groups channels (its synthesis
        half), both on this object's plan; hop as st_in.stft_hop's; mask the frame's row(s),
        (groups, N/2+1) or shared (N/2+1,) float32.  The state advances by one frame, the
        weights are solved again every update_every frames.  Returns (out, emitted): out as
        st_out's hops, written when emitted is H."""
        torch = _torch()
        if not isinstance(st_in, Stream) or not isinstance(st_out, Stream):
            raise ValueError("st_in and st_out must be Stream objects")
        if st_in.plan is not self.plan or st_out.plan is not self.plan:
            raise ValueError("the streams must be on the beamformer's plan")
        if st_in.channels != self.groups * self.mics or st_out.channels != self.groups:
            raise ValueError(f"st_in needs {self.groups * self.mics} channels and st_out {self.groups}")
        hop = st_in._hop_arg(hop)
        if mask is None:
            raise ValueError("hop needs a mask row")
        mp, ldm = st_out._mask_arg(mask, hop)
        H = self.plan.hop_size
        if out is None:
            out = torch.empty((H, self.groups) if st_out.interleaved else (self.groups, H), dtype=torch.float32,
                              device=hop.device)
        st_out._hop_arg(out, "out")
        em = C.c_int32()
        s = _stream_handle(hop) if stream is None else stream
        _check(lib().crlot_stream_beamform_hop(st_in._h, st_out._h, self._h, hop.data_ptr(), mp, ldm, out.data_ptr(),
                                               C.byref(em), s), "crlot_stream_beamform_hop")
        return out, em.value


# ----------------------------------------------------------------- dereverberation
class Dereverberator:
    """The WPE dereverberator (crlot_wpe_create): `groups` independent arrays of `mics`
    microphones (1..8), `taps` prediction taps (1..16, mics x taps <= 64) behind `delay`
    frames (1..8).  Spectra are (G, M, F, N/2+1) complex64 in Plan.stft's layout; every
    method that walks frames takes the run [f0, f1) of a tensor holding frames 0 .. f1-1.
    power gives the inverse power rows, accumulate the correlation statistics, solve the
    taps, filter the estimate, rls the recursive form on this object's inverse correlation
    matrix and taps, dereverb runs stft -> iterations x (power, accumulate, solve, filter) ->
    istft_ola on signals, hop is the per-hop chain.  Creation checks the descriptor
    (ValueError) and touches no device."""

    def __init__(self, plan: "Plan", mics: int, taps: int = 10, delay: int = 3, groups: int = 1, iterations: int = 3,
                 alpha: float = 0.9999, loading: float = 1e-3, floor: float = 1e-10):
        self._h = None
        self.plan, self.mics, self.taps_count, self.delay = plan, int(mics), int(taps), int(delay)
        self.groups, self.iterations = int(groups), int(iterations)
        self.alpha, self.loading, self.floor = float(alpha), float(loading), float(floor)
        self.bins = plan.frame_size // 2 + 1
        self.stack = self.mics * self.taps_count
        d = WpeDesc(self.mics, self.taps_count, self.delay, self.iterations, self.alpha, self.loading, self.floor)
        h = C.c_void_p()
        _check(lib().crlot_wpe_create(plan._h, C.byref(d), self.groups, C.byref(h)), "crlot_wpe_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_wpe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _info(self):
        i = [C.c_int32() for _ in range(6)]
        fr = C.c_int64()
        f = [C.c_float() for _ in range(3)]
        _check(lib().crlot_wpe_info(self._h, *[C.byref(v) for v in i], C.byref(fr), *[C.byref(v) for v in f]),
               "crlot_wpe_info")
        names = ("groups", "mics", "taps", "delay", "iterations", "bins")
        out = {n: v.value for n, v in zip(names, i)}
        out.update(frames=fr.value, alpha=f[0].value, loading=f[1].value, floor=f[2].value)
        return out

    @property
    def frames(self) -> int:
        """Frames the carried state (accumulate with carry, rls, hop) has seen since create / reset."""
        return self._info()["frames"]

    @property
    def state_planes(self) -> int:
        return self.stack * self.stack + 2 * self.stack * self.mics

    def prepare(self):
        with _torch().cuda.device(self.plan._device_index()):
            _check(lib().crlot_wpe_prepare(self._h), "crlot_wpe_prepare")

    def reset(self):
        """Zero the state, the ring, the taps and the frame counter; the inverse correlation matrix back to the identity."""
        _check(lib().crlot_wpe_reset(self._h), "crlot_wpe_reset")

    def _view(self, fn, name, shape, cplx):
        torch = _torch()
        ptr = C.c_void_p()
        dev = self.plan._device_index()
        with torch.cuda.device(dev):
            _check(fn(self._h, C.byref(ptr)), name)
            t = torch.as_tensor(_DeviceFloats(ptr.value, shape + ((2,) if cplx else ())), device=f"cuda:{dev}")
        return torch.view_as_complex(t) if cplx else t

    def state(self):
        """The carried statistics, a (groups, L L + 2 L M, N/2+1) float32 torch view: R as a
        Hermitian matrix (the L diagonals, then Re, Im of every i < j), then P as Re, Im, l-major."""
        return self._view(lib().crlot_wpe_state, "crlot_wpe_state", (self.groups, self.state_planes, self.bins), False)

    def inv_cov(self):
        """The RLS step's inverse correlation matrix, a (groups, L L, N/2+1) float32 torch view."""
        return self._view(lib().crlot_wpe_inv_cov, "crlot_wpe_inv_cov", (self.groups, self.stack * self.stack, self.bins),
                          False)

    def taps(self):
        """The object's taps, a (groups, L, M, N/2+1) complex64 torch view."""
        return self._view(lib().crlot_wpe_taps, "crlot_wpe_taps", (self.groups, self.stack, self.mics, self.bins), True)

    def set_taps(self, g):
        """Replace the object's taps: (groups, L, M, N/2+1) or (L, M, N/2+1) complex64, host or device."""
        torch = _torch()
        view = self.taps()
        v = torch.as_tensor(np.ascontiguousarray(g, np.complex64)) if not torch.is_tensor(g) else g
        if v.dtype != torch.complex64:
            raise ValueError("taps must be complex64")
        if tuple(v.shape) == tuple(view.shape[1:]):
            v = v[None].expand(self.groups, -1, -1, -1)
        if tuple(v.shape) != tuple(view.shape):
            raise ValueError(f"taps must be {tuple(view.shape)} or {tuple(view.shape[1:])}")
        view.copy_(v.to(view.device))

    def last_launch(self) -> dict:
        r = WpeLaunch()
        _check(lib().crlot_wpe_last_launch(self._h, C.byref(r)), "crlot_wpe_last_launch")
        kernels = [int(r.kernel[i]) for i in range(r.n_kernels)]
        return {"kernels": kernels, "names": [kernel_name(k) for k in kernels],
                "grids": [int(r.grid[i]) for i in range(r.n_kernels)]}

    def _spec(self, spec, what="spec"):
        if len(spec.shape) == 3:
            spec = spec[None]
        G, F, ld, ldf = _bf_spec_layout(*_tensor_layout(spec), self.plan._device_index(), self.mics, self.bins, what)
        return spec, G, F, ld, ldf

    def _run(self, F, f0, f1):
        f1 = F if f1 is None else int(f1)
        f0 = int(f0)
        if not 0 <= f0 <= f1 <= F:
            raise ValueError(f"the run [f0, f1) must lie within the {F} frames given")
        return f0, f1

    def _block(self, t, shape, dtype, what):
        tshape, _, tdtype, dev = _tensor_layout(t)
        if tshape != tuple(shape) or tdtype != dtype or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {tuple(shape)} {dtype} tensor")
        if dev is None or dev != self.plan._device_index():
            raise ValueError(f"{what} must live on the plan's device")
        return t.data_ptr()

    def _pow_layout(self, pw, G, F):
        shape, strides, dtype, dev = _tensor_layout(pw)
        if shape != (G, F, self.bins) or dtype != "float32" or dev is None or dev != self.plan._device_index():
            raise ValueError(f"power rows must be a ({G}, {F}, {self.bins}) float32 tensor on the plan's device")
        if strides[2] != 1:
            raise ValueError("power rows must be contiguous")
        ldf = strides[1] if F > 1 else self.bins
        ld = strides[0] if G > 1 else F * ldf
        if ldf < self.bins or ld < (F - 1) * ldf + self.bins:
            raise ValueError("power rows overlap")
        return int(ld), int(ldf)

    def power(self, z, f0: int = 0, f1=None, out=None, stream: int | None = None):
        """z: (G, M, F, N/2+1) -> the inverse power rows (G, F, N/2+1) float32 of the frames [f0, f1)
        (rows outside the run are left as they are; a fresh `out` is zeroed)."""
        torch = _torch()
        z, G, F, ld, ldf = self._spec(z, "z")
        f0, f1 = self._run(F, f0, f1)
        if out is None:
            out = torch.zeros((G, F, self.bins), dtype=torch.float32, device=z.device)
        ldp, ldfp = self._pow_layout(out, G, F)
        if _tensors_overlap(out, z):
            raise ValueError("out overlaps the spectra")
        s = _stream_handle(z) if stream is None else stream
        _check(lib().crlot_wpe_power(self._h, z.data_ptr(), ld, ldf, G, f0, f1, out.data_ptr(), ldp, ldfp, s),
               "crlot_wpe_power")
        return out

    def accumulate(self, spec, power, f0: int = 0, f1=None, carry: bool = False, state_out=None,
                   stream: int | None = None):
        """The statistics of the frames [f0, f1) of spec under the inverse power rows `power`
        ((G, F, N/2+1) float32).  carry=False: fresh state, any G, the result in state_out
        (allocated zeroed when None), this object untouched.  carry=True: G must be the group
        count; the run continues from this object's state and advances it.  Returns the
        (G, L L + 2 L M, N/2+1) state the run ends with."""
        torch = _torch()
        spec, G, F, ld, ldf = self._spec(spec)
        f0, f1 = self._run(F, f0, f1)
        ldp, ldfp = self._pow_layout(power, G, F)
        if carry and G != self.groups:
            raise ValueError(f"carry needs {self.groups} groups, not {G}")
        out = state_out
        if out is None and not carry:
            out = torch.zeros((G, self.state_planes, self.bins), dtype=torch.float32, device=spec.device)
        op = None
        if out is not None:
            op = self._block(out, (G, self.state_planes, self.bins), "float32", "state_out")
            if _tensors_overlap(out, spec) or _tensors_overlap(out, power):
                raise ValueError("state_out overlaps an input")
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_wpe_accumulate(self._h, spec.data_ptr(), ld, ldf, power.data_ptr(), ldp, ldfp, G, f0, f1,
                                          int(bool(carry)), op, s), "crlot_wpe_accumulate")
        return self.state() if out is None else out

    def solve(self, state=None, taps=None, stream: int | None = None):
        """The taps of a state block (None: this object's); taps (None: this object's, which is
        returned) is a (G, L, M, N/2+1) complex64 device tensor.  G may not exceed the group count."""
        G = self.groups if state is None else int(state.shape[0])
        if taps is not None and state is None:
            G = int(taps.shape[0])
        sp = None if state is None else self._block(state, (G, self.state_planes, self.bins), "float32", "state")
        tp = None if taps is None else self._block(taps, (G, self.stack, self.mics, self.bins), "complex64", "taps")
        if (state is None or taps is None) and G != self.groups:
            raise ValueError(f"this object's blocks need {self.groups} groups, not {G}")
        if G > self.groups:
            raise ValueError(f"solve runs in this object's workspace: at most {self.groups} groups, not {G}")
        if state is not None and taps is not None and _tensors_overlap(state, taps):
            raise ValueError("taps overlap the state")
        like = state if state is not None else taps
        s = stream if stream is not None else _stream_handle(like if like is not None else self.state())
        with _torch().cuda.device(self.plan._device_index()):
            _check(lib().crlot_wpe_solve(self._h, sp, G, tp, s), "crlot_wpe_solve")
        return self.taps() if taps is None else taps

    def _out(self, spec, G, F, out):
        torch = _torch()
        if out is None:
            out = torch.zeros((G, self.mics, F, self.bins), dtype=torch.complex64, device=spec.device)
        o4 = out[None] if len(out.shape) == 3 else out
        Go, Fo, ld_o, ldf_o = _bf_spec_layout(*_tensor_layout(o4), self.plan._device_index(), self.mics, self.bins, "out")
        if (Go, Fo) != (G, F):
            raise ValueError(f"out must hold {G} groups of {F} frames")
        if _tensors_overlap(o4, spec):
            raise ValueError("out overlaps the spectra")
        return out, o4, ld_o, ldf_o

    def filter(self, spec, taps=None, f0: int = 0, f1=None, out=None, stream: int | None = None):
        """spec -> the estimate (G, M, F, N/2+1) complex64 of the frames [f0, f1) with `taps` (None:
        this object's); frames outside the run are left as they are (a fresh `out` is zeroed)."""
        squeeze = len(spec.shape) == 3
        spec, G, F, ld, ldf = self._spec(spec)
        f0, f1 = self._run(F, f0, f1)
        tp = None if taps is None else self._block(taps, (G, self.stack, self.mics, self.bins), "complex64", "taps")
        if taps is None and G != self.groups:
            raise ValueError(f"this object's taps need {self.groups} groups, not {G}")
        out, o4, ld_o, ldf_o = self._out(spec, G, F, out)
        if taps is not None and _tensors_overlap(o4, taps):
            raise ValueError("out overlaps the taps")
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_wpe_filter(self._h, spec.data_ptr(), ld, ldf, tp, G, f0, f1, o4.data_ptr(), ld_o, ldf_o, s),
               "crlot_wpe_filter")
        return o4[0] if squeeze and len(out.shape) == 4 else out

    def rls(self, spec, f0: int = 0, f1=None, out=None, stream: int | None = None):
        """The recursive step over the frames [f0, f1) on this object's inverse correlation matrix
        and taps; spec must have the object's group count.  Returns the predictions (G, M, F,
        N/2+1) complex64 (frames outside the run as filter leaves them)."""
        squeeze = len(spec.shape) == 3
        spec, G, F, ld, ldf = self._spec(spec)
        if G != self.groups:
            raise ValueError(f"rls needs {self.groups} groups, not {G}")
        f0, f1 = self._run(F, f0, f1)
        out, o4, ld_o, ldf_o = self._out(spec, G, F, out)
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_wpe_rls(self._h, spec.data_ptr(), ld, ldf, f0, f1, o4.data_ptr(), ld_o, ldf_o, s),
               "crlot_wpe_rls")
        return o4[0] if squeeze and len(out.shape) == 4 else out

    def dereverb(self, x, y=None, stream: int | None = None):
        """x: (G, M, T) or (M, T) float32 device tensor -> y: (G, M, F H): istft_ola of `iterations`
        rounds of filter(solve(accumulate(power))) on stft(x), bit for bit, everything between
        in the plan's scratch; this object is untouched.  The plan must have no stored
        spectral mask."""
        torch = _torch()
        squeeze = x.dim() == 2
        if squeeze:
            x = x[None]
        shape, strides, dtype, dev = _tensor_layout(x)
        if len(shape) != 3 or shape[1] != self.mics or dtype != "float32" or dev is None:
            raise ValueError(f"x must be a (G, {self.mics}, T) or ({self.mics}, T) float32 device tensor")
        if dev != self.plan._device_index():
            raise ValueError(f"x must live on the plan's device {self.plan._device_index()}")
        G, T = int(shape[0]), int(shape[2])
        if T > 1 and strides[2] != 1:
            raise ValueError("x must have contiguous rows")
        ld_x = int(strides[1]) if self.mics > 1 else max(int(strides[1]), T)
        if ld_x < T or (G > 1 and int(strides[0]) != self.mics * ld_x):
            raise ValueError(f"x: rows overlap, or the groups are not {self.mics} microphone strides apart")
        if getattr(self.plan, "_mask", None) is not None:
            raise ValueError("dereverb: the plan has a stored spectral mask; clear it first")
        Ly = self.plan.frame_count(T) * self.plan.hop_size
        if y is None:
            y = torch.empty((G, self.mics, Ly), dtype=x.dtype, device=x.device)
        y3 = y[None] if y.dim() == 2 else y
        if tuple(y3.shape[:2]) != (G, self.mics) or not y3.is_contiguous():
            raise ValueError(f"y must be a contiguous ({G}, {self.mics}, >= {Ly}) float32 tensor")
        ld_y = _gl_y_layout(*_tensor_layout(y3.reshape(G * self.mics, -1)), dev, G * self.mics, Ly)
        if _tensors_overlap(y3, x):
            raise ValueError("y overlaps the input")
        s = _stream_handle(x) if stream is None else stream
        _check(lib().crlot_wpe(self._h, x.data_ptr(), ld_x, y3.data_ptr(), ld_y, G, T, s), "crlot_wpe")
        return y3[0] if squeeze and y.dim() == 3 else y

    def hop(self, st_in: "Stream", st_out: "Stream", hop, out=None, stream: int | None = None) -> tuple:
        """One hop of the per-hop chain (crlot_stream_wpe_hop): st_in (its analysis half) and
        st_out (its synthesis half) are Streams of groups x mics channels on this object's
        plan; hop as st_in.stft_hop's.  The inverse correlation matrix and the taps advance by
        one frame.  Returns (out, emitted): out as st_out's hops, written when emitted is H."""
        torch = _torch()
        if not isinstance(st_in, Stream) or not isinstance(st_out, Stream):
            raise ValueError("st_in and st_out must be Stream objects")
        if st_in.plan is not self.plan or st_out.plan is not self.plan:
            raise ValueError("the streams must be on the dereverberator's plan")
        C_ = self.groups * self.mics
        if st_in.channels != C_ or st_out.channels != C_:
            raise ValueError(f"st_in and st_out need {C_} channels each")
        hop = st_in._hop_arg(hop)
        H = self.plan.hop_size
        if out is None:
            out = torch.empty((H, C_) if st_out.interleaved else (C_, H), dtype=torch.float32, device=hop.device)
        st_out._hop_arg(out, "out")
        em = C.c_int32()
        s = _stream_handle(hop) if stream is None else stream
        _check(lib().crlot_stream_wpe_hop(st_in._h, st_out._h, self._h, hop.data_ptr(), out.data_ptr(), C.byref(em), s),
               "crlot_stream_wpe_hop")
        return out, em.value


class FftPlan:
    """dsp::fft::IFftPlan on the device (fft_api.h:26-48), both domains.

    Batched over the leading dim of torch CUDA tensors; `forward`/`inverse` for a
    Real plan, `forward_complex`/`inverse_complex` for a Complex plan (the other
    domain's calls raise RuntimeError with the reference's message)."""

    def __init__(self, nfft: int, domain: int = FFT_REAL, device: int = -1):
        self.nfft, self.domain = nfft, domain
        self._h = None
        h = C.c_void_p()
        _check(lib().crlot_fft_plan_create(C.byref(FftDesc(domain, nfft, device)), C.byref(h)),
               "crlot_fft_plan_create")
        self._h = h

    def close(self):
        if self._h:
            lib().crlot_fft_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        return self.nfft

    def forward(self, x):
        """(B, nfft) real -> (B, nfft/2+1) complex (sanitized input)."""
        torch = _torch()
        B, n = x.shape
        bins = n // 2 + 1
        out = torch.empty((B, bins), dtype=torch.complex64, device=x.device)
        _check(lib().crlot_fft_forward(self._h, x.data_ptr(), out.data_ptr(), B, _ld(x, 0, n),
                                       x.stride(1), 2 * bins, 1, _stream_handle(x)),
               "forward")
        return out

    def inverse(self, X):
        """(B, nfft/2+1) complex -> (B, nfft) real (*1/nfft, sanitize)."""
        torch = _torch()
        X = X.contiguous()
        B, bins = X.shape
        out = torch.empty((B, self.nfft), dtype=torch.float32, device=X.device)
        _check(lib().crlot_fft_inverse(self._h, X.data_ptr(), out.data_ptr(), B, 2 * bins, 1,
                                       self.nfft, 1, _stream_handle(X)),
               "inverse")
        return out

    def _cplx(self, fn, name, Z):
        torch = _torch()
        B, n = Z.shape
        out = torch.empty((B, n), dtype=torch.complex64, device=Z.device)
        ld = 2 * Z.stride(0) if B > 1 else 2 * n
        _check(fn(self._h, Z.data_ptr(), out.data_ptr(), B, ld, Z.stride(1), 2 * n, 1,
                  _stream_handle(Z)), name)
        return out

    def forward_complex(self, Z):
        """(B, nfft) complex64 -> (B, nfft) complex64, unnormalised."""
        return self._cplx(lib().crlot_fft_forward_complex, "forward_complex", Z)

    def inverse_complex(self, Z):
        """(B, nfft) complex64 -> (B, nfft) complex64, *1/nfft, sanitize."""
        return self._cplx(lib().crlot_fft_inverse_complex, "inverse_complex", Z)

    # -- host-pointer forms (numpy in/out; the reference's calling convention,
    #    served by the plan's resident call kernel)
    def forward_host(self, x, out=None, inc_in: int = 1, inc_out: int = 1):
        """x: (B, nfft*inc_in) float32 numpy -> (B, (nfft/2+1)*inc_out) complex64."""
        x = np.ascontiguousarray(x, np.float32)
        x2 = x.reshape(-1, x.shape[-1])
        B = x2.shape[0]
        bins = self.nfft // 2 + 1
        if out is None:
            out = np.zeros((B, bins * inc_out), np.complex64)
        _check(lib().crlot_fft_forward_host(self._h, x2.ctypes.data, out.ctypes.data, B, x2.shape[1], inc_in,
                                            2 * out.shape[1], inc_out), "forward_host")
        return out

    def inverse_host(self, X, out=None, inc_in: int = 1, inc_out: int = 1):
        """X: (B, (nfft/2+1)*inc_in) complex64 numpy -> (B, nfft*inc_out) float32."""
        X = np.ascontiguousarray(X, np.complex64)
        X2 = X.reshape(-1, X.shape[-1])
        B = X2.shape[0]
        if out is None:
            out = np.zeros((B, self.nfft * inc_out), np.float32)
        _check(lib().crlot_fft_inverse_host(self._h, X2.ctypes.data, out.ctypes.data, B, 2 * X2.shape[1], inc_in,
                                            out.shape[1], inc_out), "inverse_host")
        return out

    def _cplx_host(self, fn, name, Z):
        Z = np.ascontiguousarray(Z, np.complex64)
        Z2 = Z.reshape(-1, Z.shape[-1])
        out = np.zeros_like(Z2)
        _check(fn(self._h, Z2.ctypes.data, out.ctypes.data, Z2.shape[0], 2 * Z2.shape[1], 1, 2 * Z2.shape[1], 1),
               name)
        return out

    def forward_complex_host(self, Z):
        return self._cplx_host(lib().crlot_fft_forward_complex_host, "forward_complex_host", Z)

    def inverse_complex_host(self, Z):
        return self._cplx_host(lib().crlot_fft_inverse_complex_host, "inverse_complex_host", Z)


# ----------------------------------------------------------------- OLA kernels (free functions)
def axpy(dst, src, g: float, win=None, stream: int | None = None):
    """dsp::axpy / axpy_windowed on device tensors: dst (B, n) += (src (B, n) [* win (n)]) * g,
    per element fma(src, g, dst) / fma(fma(src, win, 0), g, dst) (kernels.cc:18-28)."""
    d2 = dst if dst.dim() == 2 else dst[None]
    s2 = src if src.dim() == 2 else src[None]
    B, n = d2.shape
    if d2.stride(1) != 1 or s2.stride(1) != 1 or s2.shape != d2.shape:
        raise ValueError("dst / src must be (B, n) with contiguous rows")
    s = _stream_handle(dst) if stream is None else stream
    if win is None:
        _check(lib().crlot_axpy(d2.data_ptr(), s2.data_ptr(), g, n, B, _ld(d2, 0, n), _ld(s2, 0, n), s), "axpy")
    else:
        _check(lib().crlot_axpy_windowed(d2.data_ptr(), s2.data_ptr(), win.data_ptr(), g, n, B, _ld(d2, 0, n),
                                         _ld(s2, 0, n), s), "axpy_windowed")
    return dst


def normalize_and_clear(out, acc, norm, eps: float, stream: int | None = None):
    """dsp::normalize_and_clear on device tensors: out (B, n) = acc / max(norm, eps), acc = 0."""
    o2 = out if out.dim() == 2 else out[None]
    a2 = acc if acc.dim() == 2 else acc[None]
    B, n = a2.shape
    s = _stream_handle(acc) if stream is None else stream
    _check(lib().crlot_normalize_and_clear(o2.data_ptr(), a2.data_ptr(), norm.data_ptr(), eps, n, B,
                                           _ld(o2, 0, n), _ld(a2, 0, n), s), "normalize_and_clear")
    return out


def axpy_host(dst: np.ndarray, src: np.ndarray, g: float, win: np.ndarray | None = None):
    """The reference's host-pointer dsp::axpy / axpy_windowed (in place on dst, numpy float32)."""
    assert dst.dtype == np.float32 and dst.flags.c_contiguous
    src = np.ascontiguousarray(src, np.float32)
    if win is None:
        _check(lib().crlot_call_axpy(dst.ctypes.data, src.ctypes.data, g, dst.size), "axpy")
    else:
        win = np.ascontiguousarray(win, np.float32)
        _check(lib().crlot_call_axpy_windowed(dst.ctypes.data, src.ctypes.data, win.ctypes.data, g, dst.size),
               "axpy_windowed")
    return dst


def normalize_and_clear_host(out: np.ndarray, acc: np.ndarray, norm: np.ndarray, eps: float):
    """The reference's host-pointer dsp::normalize_and_clear (numpy float32, acc zeroed)."""
    assert out.dtype == np.float32 and acc.dtype == np.float32 and acc.flags.c_contiguous
    norm = np.ascontiguousarray(norm, np.float32)
    _check(lib().crlot_call_normalize_and_clear(out.ctypes.data, acc.ctypes.data, norm.ctypes.data, eps, acc.size),
           "normalize_and_clear")
    return out


# ----------------------------------------------------------------- FrameQueue
def framequeue_count(T: int, frame_size: int, hop_size: int, center: bool = True) -> int:
    return _check(int(lib().crlot_framequeue_count(T, frame_size, hop_size, int(center))), "framequeue_count")


def framequeue_frames(x, frame_size: int, hop_size: int, center: bool = True, pad_mode: int = PAD_CONSTANT,
                      stream: int | None = None):
    """Batched device form: x (S, T) CUDA tensor -> frames (S, F, N) (crlot_framequeue_frames)."""
    torch = _torch()
    x2 = x if x.dim() == 2 else x[None]
    S, T = x2.shape
    F = framequeue_count(T, frame_size, hop_size, center)
    fr = torch.empty((S, F, frame_size), dtype=torch.float32, device=x.device)
    s = _stream_handle(x) if stream is None else stream
    _check(lib().crlot_framequeue_frames(x2.data_ptr() if T else None, S, T, _ld(x2, 0, T), frame_size, hop_size,
                                         int(center), pad_mode, fr.data_ptr(), s), "framequeue_frames")
    return fr if x.dim() == 2 else fr[0]


class FrameQueue:
    """dsp::FrameQueue (FrameQueue.h:35-59): frames built on the device at construction."""

    def __init__(self, x, frame_size: int, hop_size: int, center: bool = True, pad_mode: int = PAD_CONSTANT,
                 device: int = -1):
        self._h = None
        a = None if x is None else np.ascontiguousarray(x, np.float32).reshape(-1)
        n = 0 if a is None else a.size
        h = C.c_void_p()
        _check(lib().crlot_framequeue_create(None if a is None or n == 0 else a.ctypes.data, n, frame_size,
                                             hop_size, int(center), pad_mode, device, C.byref(h)), "FrameQueue")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_framequeue_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _info(self):
        f, n, h = C.c_int64(), C.c_int64(), C.c_int64()
        _check(lib().crlot_framequeue_info(self._h, C.byref(f), C.byref(n), C.byref(h)))
        return f.value, n.value, h.value

    def getNumFrames(self) -> int:
        return self._info()[0]

    def getFrameSize(self) -> int:
        return self._info()[1]

    def getHopSize(self) -> int:
        return self._info()[2]

    def getFrame(self, idx: int) -> np.ndarray:
        p = lib().crlot_framequeue_frame(self._h, idx)
        if not p:
            _check(ERANGE if idx < 0 or idx >= self.getNumFrames() else EINVAL, "getFrame")
        n = self.getFrameSize()
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (n,)).copy()

    def copyFrame(self, idx: int, out: np.ndarray):
        _check(lib().crlot_framequeue_copy_frame(self._h, idx, None if out is None else out.ctypes.data),
               "copyFrame")

    def getAllFrames(self) -> np.ndarray:
        f, n, _ = self._info()
        if f == 0:
            return np.zeros(0, np.float32)
        p = lib().crlot_framequeue_all_frames(self._h)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (f * n,)).copy()


class Stream:
    """Low-latency per-hop path (config 4): DROP-mode framing of `channels`
    channels fed one hop at a time; device state persists across calls."""

    def __init__(self, plan: Plan, channels: int, interleaved: bool = False):
        self.plan = plan
        self.channels = channels
        self.interleaved = interleaved
        h = C.c_void_p()
        _check(lib().crlot_stream_create(plan._h, channels, C.byref(h)), "crlot_stream_create")
        self._h = h
        _check(lib().crlot_stream_set_layout(self._h, int(interleaved)))

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def reset(self):
        _check(lib().crlot_stream_reset(self._h))

    def push_hop(self, hop, out=None, stream: int | None = None) -> tuple:
        """hop: (channels, H) float32 CUDA tensor ((H, channels) if interleaved).
        Returns (out, emitted) where emitted is 0 or H."""
        torch = _torch()
        if not hop.is_contiguous():
            raise ValueError("hop must be contiguous")
        if out is None:
            out = torch.empty_like(hop)
        em = C.c_int32()
        s = _stream_handle(hop) if stream is None else stream
        _check(lib().crlot_stream_push_hop(self._h, hop.data_ptr(), out.data_ptr(), C.byref(em), s),
               "crlot_stream_push_hop")
        return out, em.value

    # -- the hop with a time-varying spectral step (crlot_stream_stft_hop / _istft_hop / _push_hop_masked)
    def _hop_arg(self, hop, what="hop"):
        torch = _torch()
        H = self.plan.hop_size
        shape = (H, self.channels) if self.interleaved else (self.channels, H)
        if not torch.is_tensor(hop) or hop.dtype != torch.float32 or not hop.is_cuda:
            raise ValueError(f"{what} must be a float32 device tensor")
        if tuple(hop.shape) != shape or not hop.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {shape} tensor")
        return hop

    def _spec_arg(self, spec):
        """(channels, N/2+1) complex64 device rows -> ld_spec in floats."""
        torch = _torch()
        bins = self.plan.frame_size // 2 + 1
        if not torch.is_tensor(spec) or spec.dtype != torch.complex64 or not spec.is_cuda:
            raise ValueError("spec must be a complex64 device tensor")
        if tuple(spec.shape) != (self.channels, bins) or spec.stride(1) != 1:
            raise ValueError(f"spec must be ({self.channels}, {bins}) with contiguous rows")
        ld = _ld(spec, 0, bins)
        if ld < bins:
            raise ValueError("spec rows overlap")
        return 2 * ld

    def _mask_arg(self, mask, like):
        """A mask of (channels, N/2+1) rows or one shared (N/2+1,) row -> (pointer, ld_mask);
        checked here, because the C entry sees only a pointer."""
        torch = _torch()
        bins = self.plan.frame_size // 2 + 1
        if mask is None:
            return None, 0
        if not torch.is_tensor(mask) or mask.dtype != torch.float32:
            raise ValueError("mask must be a float32 tensor")
        if not mask.is_cuda or mask.device != like.device:
            raise ValueError("mask must be on the stream's device")
        if tuple(mask.shape) == (bins,):
            if mask.stride(0) != 1:
                raise ValueError("mask row must be contiguous")
            return mask.data_ptr(), 0
        if tuple(mask.shape) != (self.channels, bins) or mask.stride(1) != 1:
            raise ValueError(f"mask must be ({self.channels}, {bins}) or ({bins},) with contiguous rows")
        ld = _ld(mask, 0, bins)
        if ld < bins:
            raise ValueError("mask rows overlap")
        return mask.data_ptr(), ld

    def stft_hop(self, hop, spec=None, stream: int | None = None) -> tuple:
        """The analysis half of push_hop.  hop as push_hop's; returns (spec, emitted):
        spec a (channels, N/2+1) complex64 tensor holding, when emitted is 1, the
        spectrum of the frame this hop completes (Plan.stft's row), else untouched."""
        torch = _torch()
        hop = self._hop_arg(hop)
        if spec is None:
            spec = torch.empty((self.channels, self.plan.frame_size // 2 + 1), dtype=torch.complex64,
                               device=hop.device)
        ld = self._spec_arg(spec)
        em = C.c_int32()
        s = _stream_handle(hop) if stream is None else stream
        _check(lib().crlot_stream_stft_hop(self._h, hop.data_ptr(), spec.data_ptr(), ld, C.byref(em), s),
               "crlot_stream_stft_hop")
        return spec, em.value

    def features_hop(self, features, hop, out=None, spec=None, stream: int | None = None) -> tuple:
        """stft_hop with the features computed where the spectrum row would be stored
        (crlot_stream_features_hop).  features: a Features of this stream's plan; hop as
        push_hop's.  Returns (out, emitted): out a (channels, n_out) float32 tensor (rows
        may be padded) holding, when emitted is 1, the features of the frame this hop
        completes, else untouched.  spec (optional, (channels, N/2+1) complex64) also
        receives stft_hop's row from the same launch.  Shares stft_hop's hop counter."""
        torch = _torch()
        hop = self._hop_arg(hop)
        if not isinstance(features, Features):
            raise ValueError("features must be a Features object")
        if out is None:
            out = torch.empty((self.channels, features.n_out), dtype=torch.float32, device=hop.device)
        if not torch.is_tensor(out):
            raise ValueError("out must be a float32 device tensor")
        ld_feat = _features_hop_out_layout(*_tensor_layout(out), self.channels, features.n_out,
                                           features.plan is self.plan)
        sp, ld_spec = None, 0
        if spec is not None:
            ld_spec = self._spec_arg(spec)
            sp = spec.data_ptr()
        em = C.c_int32()
        s = _stream_handle(hop) if stream is None else stream
        _check(lib().crlot_stream_features_hop(self._h, features._h, hop.data_ptr(), out.data_ptr(), ld_feat, sp,
                                               ld_spec, C.byref(em), s), "crlot_stream_features_hop")
        return out, em.value

    def istft_hop(self, spec, mask=None, out=None, stream: int | None = None):
        """The synthesis half: spec (channels, N/2+1) complex64 -> the plan's gain, then
        `mask` ((channels, N/2+1) or (N/2+1,) float32, optional) -> inverse, overlap-add
        -> the next output block, laid out as a hop.  Returns the block."""
        torch = _torch()
        ld = self._spec_arg(spec)
        mp, ldm = self._mask_arg(mask, spec)
        H = self.plan.hop_size
        if out is None:
            out = torch.empty((H, self.channels) if self.interleaved else (self.channels, H), dtype=torch.float32,
                              device=spec.device)
        self._hop_arg(out, "out")
        s = _stream_handle(spec) if stream is None else stream
        _check(lib().crlot_stream_istft_hop(self._h, spec.data_ptr(), ld, mp, ldm, out.data_ptr(), s),
               "crlot_stream_istft_hop")
        return out

    def push_hop_masked(self, hop, mask, out=None, stream: int | None = None) -> tuple:
        """push_hop with a mask row ((channels, N/2+1) or (N/2+1,) float32; None: no
        mask) for the frame this hop completes.  Returns (out, emitted), emitted 0 or H."""
        torch = _torch()
        hop = self._hop_arg(hop)
        mp, ldm = self._mask_arg(mask, hop)
        if out is None:
            out = torch.empty_like(hop)
        self._hop_arg(out, "out")
        em = C.c_int32()
        s = _stream_handle(hop) if stream is None else stream
        _check(lib().crlot_stream_push_hop_masked(self._h, hop.data_ptr(), mp, ldm, out.data_ptr(), C.byref(em), s),
               "crlot_stream_push_hop_masked")
        return out, em.value


    def denoise_hop(self, denoiser, hop, out=None, stream: int | None = None) -> tuple:
        """push_hop with the noise suppressor's gain row of the frame this hop completes
        (crlot_stream_denoise_hop); denoiser: a Denoiser of this stream's plan and channel
        count, whose state the hop advances.  Returns (out, emitted), emitted 0 or H."""
        torch = _torch()
        hop = self._hop_arg(hop)
        if not isinstance(denoiser, Denoiser):
            raise ValueError("denoiser must be a Denoiser object")
        if denoiser.plan is not self.plan:
            raise ValueError("the denoiser was created on another plan")
        if denoiser.channels != self.channels:
            raise ValueError(f"the denoiser has {denoiser.channels} channels, the stream {self.channels}")
        if out is None:
            out = torch.empty_like(hop)
        self._hop_arg(out, "out")
        em = C.c_int32()
        s = _stream_handle(hop) if stream is None else stream
        _check(lib().crlot_stream_denoise_hop(self._h, denoiser._h, hop.data_ptr(), out.data_ptr(), C.byref(em), s),
               "crlot_stream_denoise_hop")
        return out, em.value


class StreamRT:
    """Resident low-latency per-hop path (config 4) for hops in host memory: the
    crlot_stream_rt_* entries.  Same contract and bits as Stream; hops are numpy
    float32 arrays (channels, H), or (H, channels) if interleaved."""

    def __init__(self, plan: Plan, channels: int, interleaved: bool = False, depth: int = 4):
        self.plan = plan
        self.channels = channels
        self.interleaved = interleaved
        self.depth = depth
        h = C.c_void_p()
        _check(lib().crlot_stream_rt_create(plan._h, channels, int(interleaved), depth, C.byref(h)),
               "crlot_stream_rt_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_stream_rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def reset(self):
        _check(lib().crlot_stream_rt_reset(self._h))

    def set_idle_timeout(self, idle_seconds: float, hop_timeout_seconds: float = 2.0):
        _check(lib().crlot_stream_rt_set_idle_timeout(self._h, idle_seconds, hop_timeout_seconds))

    def push_hop(self, hop, out=None) -> tuple:
        """Returns (out, emitted) where emitted is 0 or H (out untouched when 0)."""
        import numpy as np
        hop = np.ascontiguousarray(hop, dtype=np.float32)
        if out is None:
            out = np.zeros_like(hop)
        em = C.c_int32()
        _check(lib().crlot_stream_rt_push_hop(self._h, hop.ctypes.data, out.ctypes.data, C.byref(em)),
               "crlot_stream_rt_push_hop")
        return out, em.value

    def info(self) -> dict:
        hops, ns, run = C.c_int64(), C.c_double(), C.c_int32()
        _check(lib().crlot_stream_rt_info(self._h, C.byref(hops), C.byref(ns), C.byref(run)))
        return {"hops": hops.value, "last_device_ns": ns.value, "running": bool(run.value)}


# ----------------------------------------------------------------- Framer / OLAAccumulator
class Framer:
    """dsp::Framer (framer.h:26-127): host object, interleaved PCM in, frames out.
    set_params raises ValueError (std::invalid_argument) on zero sizes; push/pop
    return the reference's bools."""

    def __init__(self):
        h = C.c_void_p()
        _check(lib().crlot_framer_create(C.byref(h)), "crlot_framer_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_framer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def set_params(self, frame_size: int, hop_size: int, channels: int = 1,
                   boundary_mode: int = ZERO_PAD):
        _check(lib().crlot_framer_set_params(self._h, frame_size, hop_size, channels,
                                             boundary_mode), "set_params")

    def push(self, interleaved, frames: int | None = None) -> bool:
        if interleaved is None:
            return bool(_check(lib().crlot_framer_push(self._h, None, frames or 0)))
        a = np.ascontiguousarray(interleaved, np.float32).reshape(-1)
        ch = self.channels()
        frames = a.size // ch if frames is None else frames
        if frames * ch > a.size:
            raise ValueError("push: fewer samples than frames * channels")
        return bool(_check(lib().crlot_framer_push(self._h, a.ctypes.data if a.size else None,
                                                   frames)))

    def pop(self, out: np.ndarray | None = None):
        """Next frame (frame_size*channels floats) or None when none is available."""
        n, ch = self.frame_size(), self.channels()
        buf = np.empty(max(1, n * ch), np.float32) if out is None else out
        ok = _check(lib().crlot_framer_pop(self._h, buf.ctypes.data))
        return buf[:n * ch] if ok else None

    def available_frames(self) -> int:
        return _check(int(lib().crlot_framer_available(self._h)))

    def reset(self):
        _check(lib().crlot_framer_reset(self._h))

    def _info(self):
        n, h, c, b = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        m = C.c_int32()
        _check(lib().crlot_framer_info(self._h, C.byref(n), C.byref(h), C.byref(c), C.byref(m),
                                       C.byref(b)))
        return n.value, h.value, c.value, m.value, b.value

    def frame_size(self) -> int:
        return self._info()[0]

    def hop_size(self) -> int:
        return self._info()[1]

    def channels(self) -> int:
        return self._info()[2]

    def boundary_mode(self) -> int:
        return self._info()[3]

    def buffer_size(self) -> int:
        return self._info()[4]


@dataclass
class OLAConfig:
    """dsp::OLAConfig (OLAAccumulator.h:15-29)."""
    sample_rate: int = 48000
    frame_size: int = 1024
    hop_size: int = 256
    channels: int = 1
    eps: float = 1e-8
    apply_window_inside: bool = True
    shadow_ring: bool = False
    device: int = -1

    def isValid(self) -> bool:  # noqa: N802 (reference name)
        return (self.sample_rate > 0 and self.frame_size > 0 and self.hop_size > 0
                and self.channels > 0 and self.eps > 0.0)


class OLAAccumulator:
    """dsp::OLAAccumulator (OLAAccumulator.h:63-217) with its rings on the device.

    Host forms take numpy arrays (the reference's pointers); *_device forms take
    float32 CUDA tensors and run on the current torch stream."""

    def __init__(self, cfg: OLAConfig):
        self.cfg = cfg
        self._h = None
        c = OlaConfigC(cfg.sample_rate, cfg.frame_size, cfg.hop_size, cfg.channels, cfg.eps,
                       int(cfg.apply_window_inside), int(cfg.shadow_ring), cfg.device)
        h = C.c_void_p()
        _check(lib().crlot_ola_create(C.byref(c), C.byref(h)), "OLAAccumulator")
        self._h = h
        self._keep = None

    def close(self):
        if getattr(self, "_h", None):
            lib().crlot_ola_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def config(self) -> OLAConfig:
        return self.cfg

    def set_window(self, w, wlen: int | None = None):
        if w is None:
            _check(lib().crlot_ola_set_window(self._h, None, wlen or 0), "set_window")
            return
        a = np.ascontiguousarray(w, np.float32)
        _check(lib().crlot_ola_set_window(self._h, a.ctypes.data, a.size if wlen is None else wlen),
               "set_window")

    @staticmethod
    def _win(window):
        if window is None:
            return None, None
        a = np.ascontiguousarray(window, np.float32)
        return a, a.ctypes.data

    def add_frame_SoA(self, ch_frames, window, start_sample: int, start_off: int, size: int,  # noqa: N802
                      gain: float = 1.0):
        """ch_frames: sequence of per-channel arrays (None entries allowed, as null pointers)."""
        if ch_frames is None:
            _check(lib().crlot_ola_add_frame_soa(self._h, None, None, start_sample, start_off,
                                                 size, gain), "add_frame_SoA")
            return
        arrs = [None if f is None else np.ascontiguousarray(f, np.float32) for f in ch_frames]
        ptrs = (C.c_void_p * max(1, len(arrs)))(*[None if a is None else a.ctypes.data for a in arrs])
        wa, wp = self._win(window)
        _check(lib().crlot_ola_add_frame_soa(self._h, ptrs, wp, start_sample, start_off, size, gain),
               "add_frame_SoA")

    def push_frame_AoS(self, interleaved, window, start_sample: int, start_off: int, size: int,  # noqa: N802
                       gain: float = 1.0):
        a = None if interleaved is None else np.ascontiguousarray(interleaved, np.float32)
        wa, wp = self._win(window)
        _check(lib().crlot_ola_push_frame_aos(self._h, None if a is None else a.ctypes.data, wp,
                                              start_sample, start_off, size, gain),
               "push_frame_AoS")

    def produce(self, n: int, out=None):
        """Returns (count, [per-channel arrays of n floats]); out may be given
        as a list of float32 arrays (their tails beyond count stay untouched)."""
        ch = self.cfg.channels
        if out is None:
            out = [np.zeros(max(n, 1), np.float32) for _ in range(ch)]
        ptrs = (C.c_void_p * max(1, ch))(*[None if o is None else o.ctypes.data for o in out])
        got = C.c_int64()
        _check(lib().crlot_ola_produce(self._h, ptrs, n, C.byref(got)), "produce")
        return got.value, out

    # -- device forms (float32 CUDA tensors, current torch stream)
    def add_frame_SoA_device(self, frames, window, start_sample: int, start_off: int, size: int,  # noqa: N802
                             gain: float = 1.0):
        """frames: (channels, >= frame_size) tensor, rows contiguous."""
        ld = _ld(frames, 0, frames.shape[-1]) if frames.dim() == 2 else frames.shape[-1]
        _check(lib().crlot_ola_add_frame_soa_device(
            self._h, frames.data_ptr(), ld, None if window is None else window.data_ptr(),
            start_sample, start_off, size, gain, _stream_handle(frames)), "add_frame_SoA_device")

    def push_frame_AoS_device(self, interleaved, window, start_sample: int, start_off: int,  # noqa: N802
                              size: int, gain: float = 1.0):
        _check(lib().crlot_ola_push_frame_aos_device(
            self._h, interleaved.data_ptr(), None if window is None else window.data_ptr(),
            start_sample, start_off, size, gain, _stream_handle(interleaved)),
            "push_frame_AoS_device")

    def produce_device(self, out, n: int) -> int:
        """out: (channels, >= n) tensor; returns the samples provided."""
        got = C.c_int64()
        ld = _ld(out, 0, out.shape[-1]) if out.dim() == 2 else out.shape[-1]
        _check(lib().crlot_ola_produce_device(self._h, out.data_ptr(), ld, n, C.byref(got),
                                              _stream_handle(out)), "produce_device")
        return got.value

    def flush(self):
        _check(lib().crlot_ola_flush(self._h))

    def reset(self):
        _check(lib().crlot_ola_reset(self._h))

    def synchronize(self):
        _check(lib().crlot_ola_synchronize(self._h))

    def _info(self):
        p, r, rs = C.c_int64(), C.c_int64(), C.c_int64()
        hw = C.c_int32()
        _check(lib().crlot_ola_info(self._h, C.byref(p), C.byref(r), C.byref(rs), C.byref(hw)))
        return p.value, r.value, rs.value, bool(hw.value)

    def produced_samples(self) -> int:
        return self._info()[0]

    def read_pos(self) -> int:
        return self._info()[1]

    def ring_size(self) -> int:
        return self._info()[2]

    def has_window(self) -> bool:
        return self._info()[3]

    def meter_peak(self) -> float:
        v = C.c_float()
        _check(lib().crlot_ola_meter_peak(self._h, C.byref(v)))
        return v.value

    def norm(self) -> np.ndarray:
        out = np.zeros(self.ring_size(), np.float32)
        _check(lib().crlot_ola_norm_table(self._h, _fptr(out)))
        return out


# ----------------------------------------------------------------- WAV I/O
class WavReader:
    """io/wav.h WavReader (host): open() -> bool, read_all() -> interleaved float32."""

    def __init__(self):
        self._h = None
        self.last_error = ""

    def open(self, filename) -> bool:
        self.close()
        h = C.c_void_p()
        rc = lib().crlot_wav_reader_open(os.fsencode(filename), C.byref(h))
        if rc == ERUNTIME:
            self.last_error = lib().crlot_last_error().decode(errors="replace")
            return False
        _check(rc, "crlot_wav_reader_open")
        self._h = h
        ch, sr, bps = C.c_uint32(), C.c_uint32(), C.c_uint32()
        tf, fl = C.c_uint64(), C.c_int32()
        _check(lib().crlot_wav_reader_info(h, C.byref(ch), C.byref(sr), C.byref(tf), C.byref(bps),
                                           C.byref(fl)))
        self._info = (ch.value, sr.value, tf.value, bps.value, bool(fl.value))
        return True

    def close(self):
        if self._h:
            lib().crlot_wav_reader_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def is_open(self) -> bool:
        return bool(self._h)

    def get_channels(self) -> int:
        return self._info[0] if self._h else 0

    def get_sample_rate(self) -> int:
        return self._info[1] if self._h else 0

    def get_total_frames(self) -> int:
        return self._info[2] if self._h else 0

    def get_bits_per_sample(self) -> int:
        return self._info[3] if self._h else 0

    def read(self, frames: int) -> np.ndarray:
        """Next `frames` frames (fewer at the end), interleaved float32."""
        if not self._h:
            return np.zeros(0, np.float32)
        out = np.zeros(max(frames, 0) * self.get_channels(), np.float32)
        got = C.c_uint64()
        _check(lib().crlot_wav_reader_read(self._h, _fptr(out) if out.size else None, frames,
                                           C.byref(got)), "crlot_wav_reader_read")
        return out[:got.value * self.get_channels()]

    def read_all(self) -> np.ndarray:
        return self.read(self.get_total_frames())


class WavWriter:
    """io/wav.h WavWriter (host): open(path, channels, sample_rate, bits=16, float_format=False)."""

    def __init__(self):
        self._h = None
        self.last_error = ""

    def open(self, filename, channels: int, sample_rate: int, bits_per_sample: int = 16,
             float_format: bool = False) -> bool:
        self.close()
        h = C.c_void_p()
        rc = lib().crlot_wav_writer_open(os.fsencode(filename), channels, sample_rate,
                                         bits_per_sample, int(float_format), C.byref(h))
        if rc == ERUNTIME:
            self.last_error = lib().crlot_last_error().decode(errors="replace")
            return False
        _check(rc, "crlot_wav_writer_open")
        self._h = h
        self.channels = channels
        return True

    def write(self, data) -> int:
        """Interleaved float32 frames; returns the frames written."""
        if not self._h:
            return 0
        a = np.ascontiguousarray(data, np.float32).reshape(-1)
        frames = a.size // self.channels
        put = C.c_uint64()
        _check(lib().crlot_wav_writer_write(self._h, _fptr(a) if a.size else None, frames,
                                            C.byref(put)), "crlot_wav_writer_write")
        return put.value

    def close(self):
        if self._h:
            h, self._h = self._h, None
            _check(lib().crlot_wav_writer_close(h), "crlot_wav_writer_close")

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def is_open(self) -> bool:
        return bool(self._h)


def load_wav_mono(filename) -> tuple[np.ndarray, int]:
    """WavReader.read_all() mixed down to mono the way main/main.cc:155-160 does
    (sum the channels in float, divide by the channel count); returns (x, rate)."""
    r = WavReader()
    if not r.open(filename):
        raise RuntimeError(r.last_error)
    ch, sr = r.get_channels(), r.get_sample_rate()
    pcm = r.read_all().reshape(-1, ch)
    r.close()
    acc = np.zeros(pcm.shape[0], np.float32)
    for c in range(ch):
        acc = (acc + pcm[:, c]).astype(np.float32)
    return (acc / np.float32(ch)).astype(np.float32), sr
