"""ctypes binding of libnrsc5hip.so (include/nrsc5hip.h) -- the same stub a Python caller of the
reference would use next to support/nrsc5.py:676-690.  No fallbacks: if the HIP library is missing
or a call fails, this raises."""
from __future__ import annotations

import ctypes
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libnrsc5hip.so")
# A/B measurements only (tools/gpu_r5_ab.sh): another build of the library -- e.g. one made from an earlier commit -- in place of the tree's own.  The
# freshness check is then skipped WITH a notice on stderr; nothing measured this way may be recorded as this tree's result.
_AB_LIB = os.environ.get("NRSC5HIP_AB_LIB")
if _AB_LIB:
    import sys as _sys
    print(f"nrsc5_amd.engine: NRSC5HIP_AB_LIB={_AB_LIB}: running a library that is NOT built from this tree (A/B measurement)", file=_sys.stderr)
    DEFAULT_LIB = _AB_LIB

from . import abi
from .abi import *                                             # noqa: F401,F403  (every name of the ABI stays reachable as engine.<name>)
from .abi import _Config, _ChanConfig, _ScanConfig, _FmConfig, _RdsConfig, _FmSteerConfig, _SameConfig, _FmImpairConfig
from .consumers import (HdcConsumer, PsdConsumer, SisConsumer, feed_hdc, feed_hdc_batch, feed_psd_batch, feed_sis_batch,   # noqa: F401
                        sis_utf8, sis_text, _sis_device_info, sis_event_fields, rds_text, rds_callsign, rds_event_fields, same_fields, same_event_fields, same_line, AasConsumer, feed_aas_batch, aas_event_fields, aas_sig_table, aas_packets)


def l2_frame_to_dict(fr: L2Frame) -> dict:
    out = {k: int(getattr(fr, k)) for k in ("pci", "nbytes", "n_pdu", "status", "end_offset", "lost_sync")}
    out["pdus"] = []
    for i in range(min(fr.n_pdu, 16)):
        p = fr.pdu[i]
        d = {name: int(getattr(p, name)) for name, _ in p._fields_ if name != "loc"}
        d["loc"] = [int(x) for x in p.loc[:p.nop]]
        out["pdus"].append(d)
    return out


def load_library(path: str | None = None) -> ctypes.CDLL:
    path = path or DEFAULT_LIB
    if not os.path.exists(path):
        raise Nrsc5HipError(f"{path} not found: build it with `python -m nrsc5_amd.build` (hipcc, gfx950). "
                            "There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.nrsc5hip_engine_create.argtypes = [ctypes.POINTER(_Config), ctypes.POINTER(vp)]
    lib.nrsc5hip_engine_destroy.argtypes = [vp]
    lib.nrsc5hip_engine_destroy.restype = None
    lib.nrsc5hip_last_error.restype = ctypes.c_char_p
    lib.nrsc5hip_source_sha.restype = ctypes.c_char_p
    lib.nrsc5hip_engine_hip_stream.argtypes = [vp]
    lib.nrsc5hip_engine_hip_stream.restype = vp
    lib.nrsc5hip_push_cu8.argtypes = [vp, ci, vp, ctypes.c_uint32]
    lib.nrsc5hip_push_cs16.argtypes = [vp, ci, vp, ctypes.c_uint32]
    lib.nrsc5hip_stream_reset.argtypes = [vp, ci]
    lib.nrsc5hip_stream_fresh.argtypes = [vp, ci]
    lib.nrsc5hip_force_resync.argtypes = [vp, ci]
    lib.nrsc5hip_bytes_to_next_block.argtypes = [vp, ci, ci]
    lib.nrsc5hip_bytes_to_next_block.restype = ctypes.c_longlong
    lib.nrsc5hip_px_frame_bits.argtypes = [vp, ci, ci, ci, ci, vp]
    lib.nrsc5hip_batch_fetch_px.argtypes = [vp, ci, vp, vp]
    lib.nrsc5hip_stream_set_mode.argtypes = [vp, ci, ci]
    lib.nrsc5hip_am_frame_bits.argtypes = [vp, ci, ci, ci, ci, vp]
    lib.nrsc5hip_stage_viterbi_k9.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.nrsc5hip_batch_append_cu8.argtypes = [vp, ci, vp, vp, ctypes.c_longlong, vp]
    lib.nrsc5hip_batch_append_cs16.argtypes = [vp, ci, vp, vp, ctypes.c_longlong, vp]
    lib.nrsc5hip_batch_process.argtypes = [vp, ci, vp, ci, ctypes.POINTER(ci)]
    lib.nrsc5hip_batch_trim.argtypes = [vp, ci, vp, vp]
    lib.nrsc5hip_drain.argtypes = [vp, ci, vp, ci, ctypes.POINTER(ci)]
    lib.nrsc5hip_p1_frame_packed.argtypes = [vp, ci, ci, vp]
    lib.nrsc5hip_p1_frame_bits.argtypes = [vp, ci, ci, vp]
    lib.nrsc5hip_batch_fetch.argtypes = [vp, ci, vp, vp, ci, vp, vp]
    lib.nrsc5hip_unpack_bits.argtypes = [vp, ci, vp]
    lib.nrsc5hip_unpack_bits.restype = None
    lib.nrsc5hip_stage_halfband_fm_cu8.argtypes = [vp, vp, ctypes.c_uint32, vp]
    lib.nrsc5hip_stage_fft2048.argtypes = [vp, vp, vp, ci]
    lib.nrsc5hip_stage_viterbi_k7.argtypes = [vp, vp, ci, ci, vp]
    lib.nrsc5hip_debug_fetch.argtypes = [vp, ci, vp, vp]
    lib.nrsc5hip_debug_fetch_costas.argtypes = [vp, ci, vp, vp]
    lib.nrsc5hip_stage_selftest.argtypes = [vp, ctypes.POINTER(ci)]
    lib.nrsc5hip_stage_viterbi_k7_debug.argtypes = [vp, vp, ci, vp, vp]
    lib.nrsc5hip_stage_viterbi_bench.argtypes = [vp, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_float)]
    lib.nrsc5hip_debug_sync_phases.argtypes = [vp, vp]
    lib.nrsc5hip_debug_tune.argtypes = [vp, ci, ci]
    lib.nrsc5hip_debug_fwd_stats.argtypes = [vp, vp]
    lib.nrsc5hip_debug_flow_stats.argtypes = [vp, vp]
    lib.nrsc5hip_debug_host_capture_stats.argtypes = [vp, vp]
    lib.nrsc5hip_debug_k9_stats.argtypes = [vp, vp]
    lib.nrsc5hip_debug_tb_stats.argtypes = [vp, vp]
    lib.nrsc5hip_stage_first_header.argtypes = [vp, vp, ci, ci, ci, vp]
    lib.nrsc5hip_stage_math.argtypes = [vp, ci, vp, vp, ctypes.c_longlong, vp, vp]
    lib.nrsc5hip_stage_halfband_raw.argtypes = [vp, ci, vp, ctypes.c_size_t, ci, ctypes.c_longlong, ctypes.c_longlong, vp, vp]
    lib.nrsc5hip_stage_p1_deint.argtypes = [vp, vp, vp]
    lib.nrsc5hip_stage_p1_frame.argtypes = [vp, vp, ci, vp, vp]
    lib.nrsc5hip_stage_pids.argtypes = [vp, vp, ci, vp, vp, vp]
    lib.nrsc5hip_stage_px_interleave.argtypes = [vp, ci, ci, vp, vp, vp]
    lib.nrsc5hip_stage_am_deinterleave.argtypes = [vp, ci, ci, vp, vp, vp]
    lib.nrsc5hip_stage_am_epilogue.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp]
    lib.nrsc5hip_stage_acquire.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.nrsc5hip_stage_acquire_raw.argtypes = [vp, ci, vp, ctypes.c_longlong, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.nrsc5hip_stage_am_acquire.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp]
    lib.nrsc5hip_stage_nco_exact.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    abi.bind_am_block(lib)
    abi.bind_symbols(lib)
    lib.nrsc5hip_debug_poison_results.argtypes = [vp]
    lib.nrsc5hip_debug_seam_totals.argtypes = [vp, ci]
    lib.nrsc5hip_debug_seam_totals.restype = None
    lib.nrsc5hip_debug_seam_counts.argtypes = [vp, ci]
    lib.nrsc5hip_debug_seam_counts.restype = None
    lib.nrsc5hip_drain_ready.argtypes = [vp, ci, vp, ci, ctypes.POINTER(ci)]
    lib.nrsc5hip_stream_set_manual_step.argtypes = [vp, ci, ci]
    lib.nrsc5hip_stream_step.argtypes = [vp, ci]
    lib.nrsc5hip_stream_step_ahead.argtypes = [vp, ci, ctypes.POINTER(ci)]
    lib.nrsc5hip_batch_fetch_view.argtypes = [vp, ci, ctypes.POINTER(vp), vp, ctypes.POINTER(vp)]
    lib.nrsc5hip_reset_all.argtypes = [vp]
    lib.nrsc5hip_profile.argtypes = [vp, ci, vp, vp]
    lib.nrsc5hip_l2_index.argtypes = [vp, ci, vp, vp, vp, ctypes.c_longlong]
    lib.nrsc5hip_stage_l2_index.argtypes = [vp, vp, ci, ci, vp, vp, ctypes.c_longlong]
    lib.nrsc5hip_l2_frame_get.argtypes = [vp, ci, ci, vp]
    lib.nrsc5hip_batch_fetch_l2.argtypes = [vp, ci, vp, vp]
    lib.nrsc5hip_batch_fetch_l2_px.argtypes = [vp, ci, vp, vp]
    lib.nrsc5hip_batch_fetch_l2_am.argtypes = [vp, ci, vp, vp]
    lib.nrsc5hip_hdc_create.argtypes = [ci, ctypes.POINTER(vp)]
    lib.nrsc5hip_hdc_destroy.argtypes = [vp]
    lib.nrsc5hip_hdc_destroy.restype = None
    lib.nrsc5hip_hdc_reset.argtypes = [vp, ci]
    lib.nrsc5hip_hdc_push_frame.argtypes = [vp, ci, ci, vp, vp]
    lib.nrsc5hip_hdc_fixed_audio_end.argtypes = [vp, ci, ci, vp, ctypes.c_uint]
    lib.nrsc5hip_hdc_fixed_audio_end.restype = ctypes.c_uint
    lib.nrsc5hip_l2_apply_audio_end.argtypes = [vp, ctypes.c_uint]
    lib.nrsc5hip_hdc_frame_reset.argtypes = [vp, ci]
    lib.nrsc5hip_hdc_advance.argtypes = [vp, ci, ci, HDC_CB, vp]
    lib.nrsc5hip_hdc_adts.argtypes = [vp, ctypes.c_uint, vp]
    lib.nrsc5hip_hdc_adts.restype = ctypes.c_size_t
    lib.nrsc5hip_hdc_host_bytes.argtypes = [vp]
    lib.nrsc5hip_hdc_host_bytes.restype = ctypes.c_size_t
    lib.nrsc5hip_hdc_feed.argtypes = [vp, vp, ci, vp, vp, vp, vp, ci, HDC_CB, vp]
    lib.nrsc5hip_psd_create.argtypes = [vp, ci, ctypes.POINTER(vp)]
    lib.nrsc5hip_psd_destroy.argtypes = [vp]
    lib.nrsc5hip_psd_destroy.restype = None
    lib.nrsc5hip_psd_reset.argtypes = [vp, ci]
    lib.nrsc5hip_psd_feed.argtypes = [vp, vp, ci, vp, vp, vp, vp, ci, AAS_CB, vp]
    lib.nrsc5hip_psd_stats.argtypes = [vp, ci, vp]
    lib.nrsc5hip_stage_psd.argtypes = [vp, vp, ci, vp, ci, ci, ci, AAS_CB, vp]
    lib.nrsc5hip_stage_psd_streams.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, AAS_CB, vp]
    lib.nrsc5hip_sis_create.argtypes = [vp, ci, ctypes.POINTER(vp)]
    lib.nrsc5hip_sis_destroy.argtypes = [vp]
    lib.nrsc5hip_sis_destroy.restype = None
    lib.nrsc5hip_sis_reset.argtypes = [vp, ci]
    lib.nrsc5hip_sis_feed.argtypes = [vp, ci, vp, vp, vp, SIS_CB, vp]
    lib.nrsc5hip_sis_get.argtypes = [vp, ci, ctypes.POINTER(SisInfo)]
    lib.nrsc5hip_sis_stats.argtypes = [vp, ci, vp]
    lib.nrsc5hip_stage_sis.argtypes = [vp, ci, vp, vp, vp, vp, SIS_CB, vp]
    lib.nrsc5hip_sis_debug_arena.argtypes = [vp, ctypes.c_longlong]
    lib.nrsc5hip_aas_create.argtypes = [vp, ci, ci, ci, ctypes.POINTER(vp)]
    lib.nrsc5hip_aas_destroy.argtypes = [vp]
    lib.nrsc5hip_aas_destroy.restype = None
    lib.nrsc5hip_aas_reset.argtypes = [vp, ci]
    lib.nrsc5hip_aas_feed.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, ci, AAS_EVENT_CB, vp]
    lib.nrsc5hip_aas_stats.argtypes = [vp, ci, vp]
    lib.nrsc5hip_aas_sig.argtypes = [vp, ci, vp, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ci)]
    lib.nrsc5hip_stage_aas.argtypes = [vp, ci, vp, vp, vp, AAS_EVENT_CB, vp]
    lib.nrsc5hip_stage_aas_frames.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, AAS_EVENT_CB, vp]
    lib.nrsc5hip_aas_debug_arena.argtypes = [vp, ctypes.c_longlong]
    ll = ctypes.c_longlong
    lib.nrsc5hip_chan_create.argtypes = [ctypes.POINTER(_ChanConfig), ctypes.POINTER(vp)]
    lib.nrsc5hip_chan_destroy.argtypes = [vp]
    lib.nrsc5hip_chan_destroy.restype = None
    lib.nrsc5hip_chan_reset.argtypes = [vp]
    lib.nrsc5hip_chan_info.argtypes = [vp, vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.nrsc5hip_chan_taps.argtypes = [vp, vp]
    lib.nrsc5hip_chan_outputs_for.argtypes = [vp, ll]
    lib.nrsc5hip_chan_outputs_for.restype = ll
    lib.nrsc5hip_chan_process.argtypes = [vp, vp, ll, vp, ll, ll, ctypes.POINTER(ll)]
    lib.nrsc5hip_chan_clip_counts.argtypes = [vp, vp]
    lib.nrsc5hip_chan_feed.argtypes = [vp, vp, vp, vp, ll]
    lib.nrsc5hip_chan_feed_fm.argtypes = [vp, vp, vp, vp, vp, ll, vp, ll, ll, ctypes.POINTER(ll)]
    lib.nrsc5hip_fm_create.argtypes = [ctypes.POINTER(_FmConfig), ctypes.POINTER(vp)]
    lib.nrsc5hip_fm_destroy.argtypes = [vp]
    lib.nrsc5hip_fm_destroy.restype = None
    lib.nrsc5hip_fm_reset.argtypes = [vp]
    lib.nrsc5hip_fm_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ll)]
    lib.nrsc5hip_fm_taps.argtypes = [vp, vp, vp]
    lib.nrsc5hip_fm_outputs_for.argtypes = [vp, ll]
    lib.nrsc5hip_fm_outputs_for.restype = ll
    lib.nrsc5hip_fm_process.argtypes = [vp, vp, ll, ll, vp, ll, ll, ctypes.POINTER(ll)]
    lib.nrsc5hip_fm_clip_counts.argtypes = [vp, vp]
    lib.nrsc5hip_fm_pilot.argtypes = [vp, vp, vp]
    lib.nrsc5hip_stage_fm_mpx.argtypes = [vp, vp, ll, ll, vp, vp]
    abi.bind_rds(lib)
    abi.bind_carrier(lib)
    abi.bind_steer(lib)
    abi.bind_same(lib)
    abi.bind_impair(lib)
    lib.nrsc5hip_scan_create.argtypes = [ctypes.POINTER(_ScanConfig), ctypes.POINTER(vp)]
    lib.nrsc5hip_scan_destroy.argtypes = [vp]
    lib.nrsc5hip_scan_destroy.restype = None
    lib.nrsc5hip_scan_reset.argtypes = [vp]
    lib.nrsc5hip_scan_push.argtypes = [vp, vp, ll]
    lib.nrsc5hip_scan_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ll), ctypes.POINTER(ctypes.c_double)]
    lib.nrsc5hip_scan_spectrum.argtypes = [vp, vp]
    lib.nrsc5hip_scan_detect.argtypes = [vp, ctypes.POINTER(ScanParams), vp, ci, ctypes.POINTER(ci)]
    lib.nrsc5hip_scan_detect_psd.argtypes = [vp, ci, ctypes.c_double, ctypes.POINTER(ScanParams), vp, ci, ctypes.POINTER(ci)]
    return lib


EXPORTED_SYMBOLS = [
    "nrsc5hip_engine_create", "nrsc5hip_engine_destroy", "nrsc5hip_last_error", "nrsc5hip_source_sha", "nrsc5hip_engine_hip_stream",
    "nrsc5hip_push_cu8", "nrsc5hip_push_cs16", "nrsc5hip_stream_reset", "nrsc5hip_stream_fresh", "nrsc5hip_force_resync", "nrsc5hip_bytes_to_next_block",
    "nrsc5hip_batch_append_cu8", "nrsc5hip_batch_append_cs16", "nrsc5hip_batch_process", "nrsc5hip_batch_trim", "nrsc5hip_drain",
    "nrsc5hip_p1_frame_packed", "nrsc5hip_p1_frame_bits", "nrsc5hip_batch_fetch", "nrsc5hip_unpack_bits",
    "nrsc5hip_stage_halfband_fm_cu8", "nrsc5hip_stage_fft2048", "nrsc5hip_stage_viterbi_k7", "nrsc5hip_debug_fetch", "nrsc5hip_debug_fetch_costas",
    "nrsc5hip_debug_fetch_q15", "nrsc5hip_debug_alloc_copy", "nrsc5hip_debug_free", "nrsc5hip_reset_all", "nrsc5hip_profile", "nrsc5hip_stage_selftest", "nrsc5hip_stage_viterbi_k7_debug", "nrsc5hip_stage_viterbi_bench", "nrsc5hip_debug_sync_phases", "nrsc5hip_debug_tune", "nrsc5hip_debug_fwd_stats", "nrsc5hip_debug_flow_stats", "nrsc5hip_debug_host_capture_stats", "nrsc5hip_abi_version", "nrsc5hip_debug_tb_stats", "nrsc5hip_debug_k9_stats", "nrsc5hip_stage_first_header", "nrsc5hip_stage_math", "nrsc5hip_stage_halfband_raw", "nrsc5hip_stage_p1_deint", "nrsc5hip_stage_p1_frame", "nrsc5hip_stage_pids", "nrsc5hip_stage_px_interleave", "nrsc5hip_stage_am_deinterleave", "nrsc5hip_stage_am_epilogue", "nrsc5hip_stage_acquire", "nrsc5hip_stage_acquire_raw", "nrsc5hip_stage_am_acquire", "nrsc5hip_stage_am_block", "nrsc5hip_debug_fetch_am_sym", "nrsc5hip_stage_nco_exact", "nrsc5hip_stage_symbols", "nrsc5hip_debug_seam_totals", "nrsc5hip_debug_seam_counts", "nrsc5hip_drain_ready", "nrsc5hip_stream_set_manual_step", "nrsc5hip_stream_step", "nrsc5hip_stream_step_ahead", "nrsc5hip_debug_poison_results", "nrsc5hip_device_count", "nrsc5hip_device_upload", "nrsc5hip_device_free", "nrsc5hip_batch_fetch_view", "nrsc5hip_batch_fetch_l2_px", "nrsc5hip_batch_fetch_l2_am",
    "nrsc5hip_stream_set_mode", "nrsc5hip_am_frame_bits", "nrsc5hip_stage_viterbi_k9", "nrsc5hip_px_frame_bits",
    "nrsc5hip_batch_fetch_px", "nrsc5hip_debug_fetch_px", "nrsc5hip_stage_viterbi_k9_bench",
    "nrsc5hip_l2_index", "nrsc5hip_stage_l2_index", "nrsc5hip_l2_frame_get", "nrsc5hip_batch_fetch_l2",
    "nrsc5hip_hdc_create", "nrsc5hip_hdc_destroy", "nrsc5hip_hdc_reset", "nrsc5hip_hdc_push_frame", "nrsc5hip_hdc_advance",
    "nrsc5hip_hdc_adts", "nrsc5hip_hdc_host_bytes", "nrsc5hip_hdc_fixed_audio_end", "nrsc5hip_l2_apply_audio_end", "nrsc5hip_hdc_frame_reset",
    "nrsc5hip_hdc_feed",
    "nrsc5hip_psd_create", "nrsc5hip_psd_destroy", "nrsc5hip_psd_reset", "nrsc5hip_psd_feed", "nrsc5hip_psd_stats", "nrsc5hip_stage_psd", "nrsc5hip_stage_psd_streams",
    "nrsc5hip_sis_create", "nrsc5hip_sis_destroy", "nrsc5hip_sis_reset", "nrsc5hip_sis_feed", "nrsc5hip_sis_get", "nrsc5hip_sis_stats", "nrsc5hip_stage_sis",
    "nrsc5hip_sis_debug_arena",
    "nrsc5hip_aas_create", "nrsc5hip_aas_destroy", "nrsc5hip_aas_reset", "nrsc5hip_aas_feed", "nrsc5hip_aas_stats", "nrsc5hip_aas_sig", "nrsc5hip_stage_aas",
    "nrsc5hip_stage_aas_frames", "nrsc5hip_aas_debug_arena",
    "nrsc5hip_chan_create", "nrsc5hip_chan_destroy", "nrsc5hip_chan_reset", "nrsc5hip_chan_info", "nrsc5hip_chan_taps",
    "nrsc5hip_chan_outputs_for", "nrsc5hip_chan_process", "nrsc5hip_chan_clip_counts", "nrsc5hip_chan_feed",
    "nrsc5hip_scan_create", "nrsc5hip_scan_destroy", "nrsc5hip_scan_reset", "nrsc5hip_scan_push", "nrsc5hip_scan_info",
    "nrsc5hip_scan_spectrum", "nrsc5hip_scan_detect", "nrsc5hip_scan_detect_psd",
    "nrsc5hip_fm_create", "nrsc5hip_fm_destroy", "nrsc5hip_fm_reset", "nrsc5hip_fm_info", "nrsc5hip_fm_taps", "nrsc5hip_fm_outputs_for",
    "nrsc5hip_fm_process", "nrsc5hip_fm_clip_counts", "nrsc5hip_fm_pilot", "nrsc5hip_stage_fm_mpx", "nrsc5hip_chan_feed_fm",
    "nrsc5hip_fm_debug_launches", "nrsc5hip_fm_rds_enable", "nrsc5hip_fm_rds_read", "nrsc5hip_fm_rds_get", "nrsc5hip_fm_rds_stats", "nrsc5hip_fm_rds_info", "nrsc5hip_fm_rds_taps",
    "nrsc5hip_stage_rds_mf", "nrsc5hip_stage_rds_groups",
    "nrsc5hip_fm_carrier_enable", "nrsc5hip_fm_carrier", "nrsc5hip_stage_fm_carrier", "nrsc5hip_scan_detect_fm_psd", "nrsc5hip_scan_detect_fm",
    "nrsc5hip_fm_steer_enable", "nrsc5hip_fm_steer", "nrsc5hip_fm_steer_taps", "nrsc5hip_stage_fm_steer",
    "nrsc5hip_fm_same_enable", "nrsc5hip_fm_same_read", "nrsc5hip_fm_same_get", "nrsc5hip_fm_same_stats", "nrsc5hip_fm_same_info", "nrsc5hip_fm_same_table",
    "nrsc5hip_stage_same_tones", "nrsc5hip_stage_same_frames",
    "nrsc5hip_fm_impair_enable", "nrsc5hip_fm_impair", "nrsc5hip_fm_impair_taps", "nrsc5hip_stage_fm_impair"]


def library_sha(path: str | None = None) -> str:
    """Source fingerprint of the library FILE, read from its bytes -- not through dlopen: a library this process has already
    mapped keeps reporting the old build after the file was rebuilt (dlopen hands back the mapped handle)."""
    path = path or DEFAULT_LIB
    if not os.path.exists(path):
        raise Nrsc5HipError(f"{path} not found: build it with `python -m nrsc5_amd.build` (hipcc, gfx950). There is no CPU fallback.")
    data = open(path, "rb").read()
    marker = b"NRSC5HIP_SOURCE_SHA="
    k = data.find(marker)
    if k < 0:
        return "unmarked"
    return data[k + len(marker):k + len(marker) + 16].split(b"\0")[0].decode(errors="replace")


def check_fresh(path: str | None = None):
    """Raise unless the library was built from the device sources of THIS tree (a stale .so silently measures / tests old code).
    Looks at the file only, so that a caller can rebuild and check again in the same process."""
    from . import build
    if _AB_LIB and (path is None or path == _AB_LIB):
        return
    got = library_sha(path)
    want = build.source_sha()
    if got != want:
        raise Nrsc5HipError(f"{path or DEFAULT_LIB} was built from other sources (library {got}, tree {want}): run `python -m nrsc5_amd.build`")


def unpack_bits(words: np.ndarray, nbits: int) -> np.ndarray:
    w = np.ascontiguousarray(words, dtype="<u4")
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:nbits]


def _exact(a, dtype, size):
    """a stage hook's input: None stays None (the hook rejects it), anything else must hold exactly what the hook reads"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    if a.size != size:
        raise ValueError("expected %d elements, got %d" % (size, a.size))
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


class Engine:
    """One engine per GPU/process; `max_streams` independent IQ streams resident on the device."""

    def __init__(self, max_streams: int = 1, q15_capacity: int = 1 << 20, record_capacity: int = 256,
                 p1_slots: int = 4, p1_async: bool = False, device: int = 0, lib_path: str | None = None,
                 am_enable: bool = False, l2_feedback: bool = False, l2_index: bool = False, batch_zero_copy: bool = False):
        self.lib = load_library(lib_path)
        self.cfg = _Config(device, max_streams, q15_capacity, record_capacity, p1_slots, int(p1_async), int(l2_feedback), int(am_enable), int(batch_zero_copy), int(l2_index))
        self._h = ctypes.c_void_p()
        self._check(self.lib.nrsc5hip_engine_create(ctypes.byref(self.cfg), ctypes.byref(self._h)))
        self.max_streams, self.record_capacity, self.p1_slots = max_streams, record_capacity, p1_slots

    def _check(self, rc: int):
        if rc != 0:
            raise Nrsc5HipError(f"libnrsc5hip error {rc}: {self.lib.nrsc5hip_last_error().decode()}")

    def poison_results(self):
        """nrsc5hip_debug_poison_results: frame / record rings and their host mirrors get a pattern no decode produces"""
        self._check(self.lib.nrsc5hip_debug_poison_results(self._h))

    def tune(self, knob: int, value: int):
        """nrsc5hip_debug_tune: TUNE_DECODE_STREAMS / TUNE_AM_DECODE_STREAMS / TUNE_VERDICT_LAG (test hook) / TUNE_SYNC_PHASES"""
        self._check(self.lib.nrsc5hip_debug_tune(self._h, knob, value))

    def close(self):
        if self._h:
            self.lib.nrsc5hip_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def hip_stream(self) -> int:
        return self.lib.nrsc5hip_engine_hip_stream(self._h) or 0

    # ---- streaming seam ---------------------------------------------------------------------
    def push_cu8(self, stream: int, iq: np.ndarray):
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        self._check(self.lib.nrsc5hip_push_cu8(self._h, stream, iq.ctypes.data, iq.size))

    def push_cs16(self, stream: int, iq: np.ndarray):
        iq = np.ascontiguousarray(iq, dtype=np.int16)
        self._check(self.lib.nrsc5hip_push_cs16(self._h, stream, iq.ctypes.data, iq.size))

    def reset(self, stream: int):
        """input_reset of a session that may have been used: the FIR windows are rewound, not cleared (include/nrsc5hip.h)"""
        self._check(self.lib.nrsc5hip_stream_reset(self._h, stream))

    def fresh(self, stream: int):
        """a new session on this slot (nrsc5_close + nrsc5_open_pipe)"""
        self._check(self.lib.nrsc5hip_stream_fresh(self._h, stream))

    def set_mode(self, stream: int, mode: int):
        """nrsc5_set_mode for one stream (MODE_FM / MODE_AM); resets it."""
        self._check(self.lib.nrsc5hip_stream_set_mode(self._h, stream, mode))

    def reset_all(self):
        self._check(self.lib.nrsc5hip_reset_all(self._h))

    PROF_CLASSES = ("decimate", "acquire", "prepare", "mixfft", "sync", "p1_deint", "p1_viterbi", "pids", "am", "am_decode", "p1_traceback", "flow")

    def profile(self, enable: int = -1):
        """Per-kernel-class {name: (total_ms, launches)} from HIP events; enable 1/0 starts/stops, a class name starts timing
        that class only."""
        if isinstance(enable, str):
            enable = 0x100 | self.PROF_CLASSES.index(enable)
        ms = np.zeros(len(self.PROF_CLASSES), dtype=np.float64)
        n = np.zeros(len(self.PROF_CLASSES), dtype=np.int64)
        self._check(self.lib.nrsc5hip_profile(self._h, enable, ms.ctypes.data, n.ctypes.data))
        return {k: (float(a), int(b)) for k, a, b in zip(self.PROF_CLASSES, ms, n)}

    def bytes_to_next_block(self, stream: int, cu8: bool = True) -> int:
        return int(self.lib.nrsc5hip_bytes_to_next_block(self._h, stream, int(cu8)))

    def force_resync(self, stream: int):
        self._check(self.lib.nrsc5hip_force_resync(self._h, stream))

    # ---- batch path (device pointers as ints) ---------------------------------------------------
    def batch_append_cu8(self, dev_ptr: int, stride_bytes: int, nbytes, stream_ids=None):
        nb = np.ascontiguousarray(nbytes, dtype=np.uint32)
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        self._check(self.lib.nrsc5hip_batch_append_cu8(self._h, nb.size, None if ids is None else ids.ctypes.data,
                                                       dev_ptr, stride_bytes, nb.ctypes.data))

    def batch_append_cs16(self, dev_ptr: int, stride_elems: int, nelems, stream_ids=None):
        ne = np.ascontiguousarray(nelems, dtype=np.uint32)
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        self._check(self.lib.nrsc5hip_batch_append_cs16(self._h, ne.size, None if ids is None else ids.ctypes.data,
                                                        dev_ptr, stride_elems, ne.ctypes.data))

    def batch_process(self, nstreams: int, stream_ids=None, max_steps: int = 0) -> int:
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        done = ctypes.c_int()
        self._check(self.lib.nrsc5hip_batch_process(self._h, nstreams, None if ids is None else ids.ctypes.data,
                                                    max_steps, ctypes.byref(done)))
        return done.value

    def batch_trim(self, nstreams: int, stream_ids=None) -> np.ndarray:
        """nrsc5hip_batch_trim: give back the FIFO space in front of everything the listed streams (0..nstreams-1 without a list) may
        still read -- their read position and every replay checkpoint whose first-header verdict is still open.  -> the samples each
        stream retains (wr - base); at most TRIM_RETAIN_MAX once batch_process has run to the end.  Results are unchanged."""
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        kept = np.zeros(nstreams, dtype=np.int64)
        self._check(self.lib.nrsc5hip_batch_trim(self._h, nstreams, None if ids is None else ids.ctypes.data, kept.ctypes.data))
        return kept

    # ---- results ---------------------------------------------------------------------------------
    def drain(self, stream: int, max_records: int | None = None) -> np.ndarray:
        mx = max_records or self.record_capacity
        out = np.zeros(mx, dtype=RECORD_DTYPE)
        n = ctypes.c_int()
        self._check(self.lib.nrsc5hip_drain(self._h, stream, out.ctypes.data, mx, ctypes.byref(n)))
        return out[:n.value]

    def drain_ready(self, stream: int, max_records: int | None = None) -> np.ndarray:
        """nrsc5hip_drain_ready: the records reported so far; never waits for a block step that is still running"""
        mx = max_records or self.record_capacity
        out = np.zeros(mx, dtype=RECORD_DTYPE)
        n = ctypes.c_int()
        self._check(self.lib.nrsc5hip_drain_ready(self._h, stream, out.ctypes.data, mx, ctypes.byref(n)))
        return out[:n.value]

    def set_manual_step(self, stream: int, on: bool = True):
        self._check(self.lib.nrsc5hip_stream_set_manual_step(self._h, stream, int(on)))

    def stream_step(self, stream: int):
        self._check(self.lib.nrsc5hip_stream_step(self._h, stream))

    def stream_step_ahead(self, stream: int) -> bool:
        """nrsc5hip_stream_step_ahead: True if the next block's step was queued behind the one in flight"""
        done = ctypes.c_int()
        self._check(self.lib.nrsc5hip_stream_step_ahead(self._h, stream, ctypes.byref(done)))
        return bool(done.value)

    def seam_counts(self, reset: bool = False) -> dict:
        """deferred steps / mispredicted read positions / steps without P1 decode launches / late P1 decodes (calling thread)"""
        out = np.zeros(6, dtype=np.float64)
        self.lib.nrsc5hip_debug_seam_counts(out.ctypes.data, int(reset))
        return dict(zip(("deferred_steps", "mispredicted_rd", "steps_without_p1_launches", "late_p1_decodes", "steps_ahead", "host_capture_pushes"), (int(x) for x in out)))

    def p1_frame_bits(self, stream: int, slot: int) -> np.ndarray:
        bits = np.zeros(P1_BITS, dtype=np.uint8)
        self._check(self.lib.nrsc5hip_p1_frame_bits(self._h, stream, slot, bits.ctypes.data))
        return bits

    def px_frame_bits(self, stream: int, slot: int, channel: int, nbits: int) -> np.ndarray:
        """FM extended sidebands: channel 0 = P3, 1 = P4; nbits 2304 (MP2) or 4608 (MP3 / MP11)."""
        bits = np.zeros(nbits, dtype=np.uint8)
        self._check(self.lib.nrsc5hip_px_frame_bits(self._h, stream, slot, channel, nbits, bits.ctypes.data))
        return bits

    def batch_fetch_px(self, nstreams: int, stream_ids=None) -> np.ndarray:
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        out = np.zeros((nstreams, 8 * self.p1_slots, 2, PX_WORDS), dtype=np.uint32)
        self._check(self.lib.nrsc5hip_batch_fetch_px(self._h, nstreams, None if ids is None else ids.ctypes.data, out.ctypes.data))
        return out

    def am_frame_bits(self, stream: int, slot: int, which: int, nbits: int) -> np.ndarray:
        """AM: which = 0..7 -> P1 frame of that block (3750 bits), 8 -> the P3 frame (24000 / 30000 bits)."""
        bits = np.zeros(nbits, dtype=np.uint8)
        self._check(self.lib.nrsc5hip_am_frame_bits(self._h, stream, slot, which, nbits, bits.ctypes.data))
        return bits

    def p1_frame_packed(self, stream: int, slot: int) -> np.ndarray:
        w = np.zeros(P1_WORDS, dtype=np.uint32)
        self._check(self.lib.nrsc5hip_p1_frame_packed(self._h, stream, slot, w.ctypes.data))
        return w

    def batch_fetch(self, nstreams: int, stream_ids=None, with_frames: bool = True):
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        recs = np.zeros((nstreams, self.record_capacity), dtype=RECORD_DTYPE)
        counts = np.zeros(nstreams, dtype=np.int32)
        frames = np.zeros((nstreams, self.p1_slots, P1_WORDS), dtype=np.uint32) if with_frames else None
        self._check(self.lib.nrsc5hip_batch_fetch(self._h, nstreams, None if ids is None else ids.ctypes.data,
                                                  recs.ctypes.data, self.record_capacity, counts.ctypes.data,
                                                  None if frames is None else frames.ctypes.data))
        return recs, counts, frames

    def batch_fetch_view(self, nstreams: int, with_frames: bool = True):
        """Zero-copy views (numpy arrays over engine-owned pinned memory, valid until the next fetch/reset)."""
        rp, fp = ctypes.c_void_p(), ctypes.c_void_p()
        counts = np.zeros(nstreams, dtype=np.int32)
        self._check(self.lib.nrsc5hip_batch_fetch_view(self._h, nstreams, ctypes.byref(rp), counts.ctypes.data,
                                                       ctypes.byref(fp) if with_frames else None))
        rec_bytes = nstreams * self.record_capacity * RECORD_DTYPE.itemsize
        recs = np.frombuffer((ctypes.c_char * rec_bytes).from_address(rp.value), dtype=RECORD_DTYPE).reshape(nstreams, self.record_capacity)
        frames = None
        if with_frames:
            fr_bytes = nstreams * self.p1_slots * P1_WORDS * 4
            frames = np.frombuffer((ctypes.c_char * fr_bytes).from_address(fp.value), dtype=np.uint32).reshape(nstreams, self.p1_slots, P1_WORDS)
        return recs, counts, frames

    # ---- stage-level entry points (parity tests) ----------------------------------------------------
    def stage_halfband_fm_cu8(self, iq: np.ndarray) -> np.ndarray:
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        out = np.zeros((iq.size // 4, 2), dtype=np.int16)
        self._check(self.lib.nrsc5hip_stage_halfband_fm_cu8(self._h, iq.ctypes.data, iq.size, out.ctypes.data))
        return out

    def stage_fft2048(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1, 2048)
        out = np.zeros_like(x)
        self._check(self.lib.nrsc5hip_stage_fft2048(self._h, x.ctypes.data, out.ctypes.data, x.shape[0]))
        return out

    def stage_viterbi_k7(self, soft: np.ndarray, length: int) -> np.ndarray:
        soft = np.ascontiguousarray(soft, dtype=np.int8).reshape(-1, 3 * length)
        bits = np.zeros((soft.shape[0], length), dtype=np.uint8)
        self._check(self.lib.nrsc5hip_stage_viterbi_k7(self._h, soft.ctypes.data, length, soft.shape[0], bits.ctypes.data))
        return bits

    def stage_viterbi_k9(self, soft: np.ndarray, length: int, gens) -> np.ndarray:
        soft = np.ascontiguousarray(soft, dtype=np.int8).reshape(-1, 3 * length)
        bits = np.zeros((soft.shape[0], length), dtype=np.uint8)
        g = (ctypes.c_uint * 3)(*gens)
        self._check(self.lib.nrsc5hip_stage_viterbi_k9(self._h, soft.ctypes.data, length, soft.shape[0], g, bits.ctypes.data))
        return bits

    def l2_index(self, jobs, want_bytes: bool = True):
        """L2 audio transport index of decoded frames still on the device.  jobs: (stream, slot, kind, which, nbits)
        tuples; returns [(dict, PDU bytes or None)] in job order."""
        n = len(jobs)
        arr = (L2Job * n)(*[L2Job(*j) for j in jobs])
        out = (L2Frame * n)()
        stride = 18272
        by = np.zeros((n, stride), dtype=np.uint8) if want_bytes else None
        self._check(self.lib.nrsc5hip_l2_index(self._h, n, arr, out, by.ctypes.data if want_bytes else None, stride))
        return [(l2_frame_to_dict(out[k]), by[k, :out[k].nbytes].copy() if want_bytes else None) for k in range(n)]

    def l2_index_raw(self, jobs):
        """As l2_index, but returns the C structs themselves: (L2Frame ctypes array, PDU bytes [n, 18272]) -- what
        nrsc5hip_hdc_push_frame takes."""
        n = len(jobs)
        arr = (L2Job * n)(*[L2Job(*j) for j in jobs])
        out = (L2Frame * n)()
        by = np.zeros((n, 18272), dtype=np.uint8)
        self._check(self.lib.nrsc5hip_l2_index(self._h, n, arr, out, by.ctypes.data, 18272))
        return out, by

    def l2_frame(self, stream: int, slot: int) -> dict:
        """Engine option l2_index: the index computed in the pipeline for the P1 frame in `slot`."""
        fr = L2Frame()
        self._check(self.lib.nrsc5hip_l2_frame_get(self._h, stream, slot, ctypes.byref(fr)))
        return l2_frame_to_dict(fr)

    def batch_fetch_l2(self, nstreams: int):
        """[nstreams][p1_slots] L2Frame ctypes array for streams 0..nstreams-1."""
        out = ((L2Frame * self.p1_slots) * nstreams)()
        self._check(self.lib.nrsc5hip_batch_fetch_l2(self._h, nstreams, None, out))
        return out

    def batch_fetch_l2_px(self, nstreams: int):
        """[nstreams][8 * p1_slots][2] L2Frame array: pipeline index of the P3 ([slot][0]) / P4 ([slot][1]) frames."""
        out = (((L2Frame * 2) * (8 * self.p1_slots)) * nstreams)()
        self._check(self.lib.nrsc5hip_batch_fetch_l2_px(self._h, nstreams, None, out))
        return out

    def batch_fetch_l2_am(self, nstreams: int):
        """[nstreams][p1_slots][9] L2Frame array: pipeline index of the 8 P1 frames + the P3 frame of every AM L1 frame slot."""
        out = (((L2Frame * 9) * self.p1_slots) * nstreams)()
        self._check(self.lib.nrsc5hip_batch_fetch_l2_am(self._h, nstreams, None, out))
        return out

    def stage_l2_index(self, frames_bits: np.ndarray, want_bytes: bool = True):
        """Same kernel on logical frames given as frame_push takes them: frames_bits [nframes][nbits] of 0/1."""
        b = np.ascontiguousarray(frames_bits, dtype=np.uint8)
        if b.ndim == 1:
            b = b[None, :]
        n, nbits = b.shape
        out = (L2Frame * n)()
        stride = 18272
        by = np.zeros((n, stride), dtype=np.uint8) if want_bytes else None
        self._check(self.lib.nrsc5hip_stage_l2_index(self._h, b.ctypes.data, nbits, n, out, by.ctypes.data if want_bytes else None, stride))
        return [(l2_frame_to_dict(out[k]), by[k, :out[k].nbytes].copy() if want_bytes else None) for k in range(n)]

    def stage_l2_index_raw(self, frames_bits: np.ndarray):
        """As stage_l2_index, but returns the C structs themselves: (L2Frame ctypes array, PDU bytes [n, 18272])."""
        b = np.ascontiguousarray(frames_bits, dtype=np.uint8)
        if b.ndim == 1:
            b = b[None, :]
        n, nbits = b.shape
        out = (L2Frame * n)()
        by = np.zeros((n, 18272), dtype=np.uint8)
        self._check(self.lib.nrsc5hip_stage_l2_index(self._h, b.ctypes.data, nbits, n, out, by.ctypes.data, 18272))
        return out, by

    def stage_viterbi_k7_debug(self, soft: np.ndarray, length: int):
        soft = np.ascontiguousarray(soft, dtype=np.int8)
        bits = np.zeros(length, dtype=np.uint8)
        dec = np.zeros(length + 64, dtype=np.uint64)
        self._check(self.lib.nrsc5hip_stage_viterbi_k7_debug(self._h, soft.ctypes.data, length, bits.ctypes.data, dec.ctypes.data))
        return bits, dec

    def stage_viterbi_bench(self, length: int, nframes: int, phases: int = 3, reps: int = 3) -> float:
        ms = ctypes.c_float()
        self._check(self.lib.nrsc5hip_stage_viterbi_bench(self._h, length, nframes, phases, reps, ctypes.byref(ms)))
        return ms.value

    def stage_viterbi_k9_bench(self, length: int, nframes: int, phases: int = 3, reps: int = 3) -> float:
        ms = ctypes.c_float()
        self.lib.nrsc5hip_stage_viterbi_k9_bench.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        self._check(self.lib.nrsc5hip_stage_viterbi_k9_bench(self._h, length, nframes, phases, reps, ctypes.byref(ms)))
        return ms.value

    def fwd_stats(self):
        """(segment boundaries checked, segments repaired) of the segmented forward trellis pass since the engine was created"""
        st = (ctypes.c_int * 2)()
        self._check(self.lib.nrsc5hip_debug_fwd_stats(self._h, st))
        return int(st[0]), int(st[1])

    def flow_stats(self):
        """dataflow bursts (TUNE_FLOW_MIN): (bursts, block steps) issued as k_flow launches since the engine was created"""
        st = (ctypes.c_longlong * 2)()
        self._check(self.lib.nrsc5hip_debug_flow_stats(self._h, st))
        return int(st[0]), int(st[1])

    def host_capture_stats(self):
        """host-resident capture of the fast seam (TUNE_HOST_CAPTURE): dict(attaches, detaches, rebases, stream)"""
        st = (ctypes.c_longlong * 5)()
        self._check(self.lib.nrsc5hip_debug_host_capture_stats(self._h, st))
        return dict(zip(("attaches", "detaches", "rebases", "stream", "reports_folded"), (int(x) for x in st)))

    def tb_stats(self):
        """single-path traceback: (chunk boundaries checked, chunks re-walked) since the engine was created"""
        st = (ctypes.c_int * 2)()
        self._check(self.lib.nrsc5hip_debug_tb_stats(self._h, st))
        return int(st[0]), int(st[1])

    def stage_first_header(self, bits: np.ndarray, threads: int = 64) -> np.ndarray:
        """First-header verdicts (1 = the reference stays synchronised) of descrambled P1 frames, bits[nframes][146176 or 3750]."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        ok = np.zeros(bits.shape[0], dtype=np.int32)
        self._check(self.lib.nrsc5hip_stage_first_header(self._h, bits.ctypes.data, bits.shape[1], bits.shape[0], threads, ok.ctypes.data))
        return ok

    def k9_stats(self):
        """K=9 decode in segment waves: (forward boundaries checked, segments re-run, traceback boundaries checked, segments re-walked)"""
        st = (ctypes.c_int * 4)()
        self._check(self.lib.nrsc5hip_debug_k9_stats(self._h, st))
        return tuple(int(v) for v in st)

    def debug_sync_phases(self) -> np.ndarray:
        c = np.zeros(16, dtype=np.int64)                        # [0..7] k_sync, [8..15] k_mixfft (diagnostic build only)
        self._check(self.lib.nrsc5hip_debug_sync_phases(self._h, c.ctypes.data))
        return c

    def stage_math(self, fn: int, a: np.ndarray, b: np.ndarray | None = None):
        """nrsc5hip_stage_math: one function of csrc/fastmath.h (MATH_*) on every element of a (and b: the two arc tangents take y, x).
        float32 arrays, float64 for the two series.  -> one array, or (sin, cos) / (cos, sin) in the order the function itself returns them."""
        dt = np.float64 if fn in (MATH_SMALL_COS_SIN, MATH_SMALL_ATAN) else np.float32
        a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
        two_in, two_out = fn in (MATH_REF_ATAN2F, MATH_FAST_ATAN2), fn in (MATH_REF_SINCOSF, MATH_FAST_SINCOS, MATH_FAST_SINCOS_REDUCED, MATH_SMALL_COS_SIN)
        if two_in != (b is not None):
            raise ValueError("the arc tangents take two arrays, every other function one")
        if two_in:
            b = np.ascontiguousarray(b, dtype=dt).reshape(-1)
            if b.size != a.size:
                raise ValueError("a and b differ in length")
        out0 = np.empty_like(a)
        out1 = np.empty_like(a) if two_out else None
        self._check(self.lib.nrsc5hip_stage_math(self._h, fn, a.ctypes.data, b.ctypes.data if two_in else None, a.size,
                                                 out0.ctypes.data, out1.ctypes.data if two_out else None))
        return (out0, out1) if two_out else out0

    def stage_halfband_raw(self, form: int, iq: np.ndarray, a0: int, n: int, lead: int = 0, probe: bool = False):
        """nrsc5hip_stage_halfband_raw: the fused float32 half-band in one of its device forms (HB_*) on the cu8 capture iq, placed `lead`
        bytes into an aligned device buffer.  n symbols of 2160 samples from decimated sample a0 (n samples for HB_ACQ) -> int16 [.., 2], the
        reference's Q15 integers; with probe (symbol forms) also uint32 [n, work-items, 4]: the rounding and denormal probes before / behind."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1)
        per, lanes = (1, 0) if form == HB_ACQ else (HB_SYM_N, 256 if form == HB_SYM256 else 128)
        out = np.zeros((max(n, 0) * per, 2), dtype=np.int16)
        pr = np.zeros((max(n, 0), lanes, 4), dtype=np.uint32) if probe and lanes else None
        self._check(self.lib.nrsc5hip_stage_halfband_raw(self._h, form, iq.ctypes.data, iq.size, lead, a0, n, out.ctypes.data,
                                                         pr.ctypes.data if pr is not None else None))
        return (out, pr) if probe else out

    # the FEC stage's permutations, error counts and descramblers: the production device code on caller data (tests/fec_checks.py)
    def stage_p1_deint(self, pm: np.ndarray) -> np.ndarray:
        """nrsc5hip_stage_p1_deint: k_p1_deint on the soft-bit matrices pm int8 [16 * 23040] -> uint32 [146176], one dword per trellis step"""
        pm = _exact(pm, np.int8, 16 * 23040)
        out = np.zeros(146176, dtype=np.uint32)
        self._check(self.lib.nrsc5hip_stage_p1_deint(self._h, _ptr(pm), out.ctypes.data))
        return out

    def stage_p1_frame(self, soft: np.ndarray, walk: int = 1):
        """nrsc5hip_stage_p1_frame: forward pass, fix and the traceback of form `walk` on soft int8 [3 * 146176] -> (descrambled bits [146176], error count)"""
        soft = _exact(soft, np.int8, 3 * 146176)
        bits = np.zeros(146176, dtype=np.uint8)
        err = ctypes.c_int(-1)
        self._check(self.lib.nrsc5hip_stage_p1_frame(self._h, _ptr(soft), walk, bits.ctypes.data, ctypes.byref(err)))
        return bits, err.value

    def stage_pids(self, pm: np.ndarray, bc: int):
        """nrsc5hip_stage_pids: gather + depuncture of block bc, k_pids_decode -> (coded int8 [240], descrambled bits [80], CRC flag)"""
        pm = _exact(pm, np.int8, 16 * 23040)
        coded, bits, ok = np.zeros(240, dtype=np.int8), np.zeros(80, dtype=np.uint8), ctypes.c_int(-1)
        self._check(self.lib.nrsc5hip_stage_pids(self._h, _ptr(pm), bc, coded.ctypes.data, bits.ctypes.data, ctypes.byref(ok)))
        return coded, bits, ok.value

    def stage_px_interleave(self, length: int, pairs: np.ndarray, npairs: int | None = None):
        """nrsc5hip_stage_px_interleave: pairs int8 [npairs, 2, 2 * length] -> (int8 [npairs, 2, 3 * length], ready int32 [npairs])"""
        n = (pairs.size // max(4 * length, 1) if pairs is not None else 0) if npairs is None else npairs
        pairs = _exact(pairs, np.int8, max(n, 0) * 4 * length)
        out, ready = np.zeros((max(n, 0), 2, 3 * max(length, 0)), dtype=np.int8), np.full(max(n, 0), -1, dtype=np.int32)
        self._check(self.lib.nrsc5hip_stage_px_interleave(self._h, length, n, _ptr(pairs), out.ctypes.data, ready.ctypes.data))
        return out, ready

    def stage_am_deinterleave(self, psmi: int, sym: np.ndarray, nframes: int | None = None):
        """nrsc5hip_stage_am_deinterleave: sym uint8 [nframes, 4 (pl, pu, s, t), 6400] -> (v1 int8 [nframes, 90000], v3 int8 [nframes, 72000 | 90000])"""
        n = (sym.size // (4 * 6400) if sym is not None else 0) if nframes is None else nframes
        sym = _exact(sym, np.uint8, max(n, 0) * 4 * 6400)
        v1, v3 = np.zeros((max(n, 0), 90000), dtype=np.int8), np.zeros((max(n, 0), 90000 if psmi == 2 else 72000), dtype=np.int8)
        self._check(self.lib.nrsc5hip_stage_am_deinterleave(self._h, psmi, n, _ptr(sym), v1.ctypes.data, v3.ctypes.data))
        return v1, v3

    def stage_am_epilogue(self, soft: np.ndarray, bits: np.ndarray, length: int, code: int, threads: int = 64):
        """nrsc5hip_stage_am_epilogue: am_bit_errors + am_descramble -> (error count, descrambled bits [length], the packed words)"""
        soft, bits = _exact(soft, np.int8, 3 * max(length, 0)), _exact(bits, np.uint8, max(length, 0))
        out, words, err = np.zeros(max(length, 0), dtype=np.uint8), np.zeros((max(length, 0) + 31) // 32, dtype=np.uint32), ctypes.c_int(-1)
        self._check(self.lib.nrsc5hip_stage_am_epilogue(self._h, _ptr(soft), _ptr(bits), length, code, threads, ctypes.byref(err), out.ctypes.data, words.ctypes.data))
        return err.value, out, words

    # coarse acquisition: the production launches on caller windows (tests/acq_checks.py).  None for an array stays None: the hook rejects it
    def _acq_outputs(self, n, raw=False):
        n = max(n, 0)
        out = dict(filt=np.zeros((n, ACQ_WIN_FM, 2), dtype=np.int16), sums=np.zeros((n, ACQ_SYM_FM, 2), dtype=np.float32), samperr=np.zeros(n, dtype=np.int32),
                   peak=np.zeros((n, 2), dtype=np.float32), hist_out=np.zeros((n, 31, 2), dtype=np.int16))
        if raw:
            out["acq_win"] = np.zeros((n, ACQ_WIN_FM, 2), dtype=np.int16)
        return out

    def stage_acquire(self, win, hist, state, fill, n: int | None = None) -> dict:
        """nrsc5hip_stage_acquire: launch_acquire on streams 0 .. n-1.  win int16 [n, 71280, 2], hist int16 [n, 31, 2], state / fill int [n] ->
        dict(filt [n, 71280, 2], sums float32 [n, 2160, 2], samperr [n], peak float32 [n, 2], hist_out [n, 31, 2])"""
        n = len(state) if n is None else n
        m = max(n, 0)
        win, hist = _exact(win, np.int16, m * ACQ_WIN_FM * 2), _exact(hist, np.int16, m * 62)
        state, fill = _exact(state, np.int32, m), _exact(fill, np.int32, m)
        o = self._acq_outputs(n)
        self._check(self.lib.nrsc5hip_stage_acquire(self._h, n, _ptr(win), _ptr(hist), _ptr(state), _ptr(fill), o["filt"].ctypes.data, o["sums"].ctypes.data,
                                                    o["samperr"].ctypes.data, o["peak"].ctypes.data, o["hist_out"].ctypes.data))
        return o

    def stage_acquire_raw(self, iq, rd, hist, state, n: int | None = None) -> dict:
        """nrsc5hip_stage_acquire_raw (batch_zero_copy engine): iq uint8 [n, nbytes] attached as captures, rd int64 [n] -> as stage_acquire, plus
        acq_win [n, 71280, 2], the window k_acq_decimate made"""
        n = len(state) if n is None else n
        m = max(n, 0)
        nbytes = 0
        if iq is not None:
            iq = np.ascontiguousarray(iq, dtype=np.uint8)
            nbytes = iq.size // max(m, 1)
            iq = iq.reshape(-1)
        rd, hist, state = _exact(rd, np.int64, m), _exact(hist, np.int16, m * 62), _exact(state, np.int32, m)
        o = self._acq_outputs(n, raw=True)
        self._check(self.lib.nrsc5hip_stage_acquire_raw(self._h, n, _ptr(iq), nbytes, _ptr(rd), _ptr(hist), _ptr(state), o["acq_win"].ctypes.data, o["filt"].ctypes.data,
                                                        o["sums"].ctypes.data, o["samperr"].ctypes.data, o["peak"].ctypes.data, o["hist_out"].ctypes.data))
        return o

    def stage_am_acquire(self, win, hist, state: int, fill: int = ACQ_WIN_AM) -> dict:
        """nrsc5hip_stage_am_acquire: one launch_am_step on stream 0 (AM mode).  win int16 [8910, 2], hist int16 [31, 2] ->
        dict(samperr, peak float32 [2], hist_out [31, 2]) read from the stream state after the step"""
        win, hist = _exact(win, np.int16, ACQ_WIN_AM * 2), _exact(hist, np.int16, 62)
        se, peak, hist_out = ctypes.c_int(0), np.zeros(2, dtype=np.float32), np.zeros((31, 2), dtype=np.int16)
        self._check(self.lib.nrsc5hip_stage_am_acquire(self._h, _ptr(win), _ptr(hist), state, fill, ctypes.byref(se), peak.ctypes.data, hist_out.ctypes.data))
        return dict(samperr=np.array([se.value], dtype=np.int32), peak=peak[None], hist_out=hist_out[None])

    def stage_am_block(self, win, hist, state: dict, fill: int = ACQ_WIN_AM, dump: bool = False) -> dict:
        """nrsc5hip_stage_am_block: k_am_block alone on stream 0 (AM mode), <256> in order or <512> on a p1_async engine.  win int16 [8910, 2], hist int16 [31, 2],
        state: the words of abi.AM_BLOCK_STATE_IN (missing ones: as a fresh session has them -- psmi 1, the system bits -1, am_diversity_wait 4, the rest 0) ->
        dict(rec: one RECORD_DTYPE record, state: dict of every word of abi.AmBlockState afterwards, am_sym uint8 [4, 6400], pids_stage int8 [240]; with dump:
        spectra complex64 [32, 256], mult complex64 [4, 25]); whatever the kernel left alone still holds 0xA5 bytes"""
        win, hist = _exact(win, np.int16, ACQ_WIN_AM * 2), _exact(hist, np.int16, 62)
        words = dict(psmi=1, pli=-1, hppi=-1, aabi=-1, rdbi=-1, am_diversity_wait=4)
        words.update(state)
        unknown = set(words) - set(abi.AM_BLOCK_STATE_IN)
        if unknown:
            raise ValueError("not a state word of the AM block step: %s" % sorted(unknown))
        sin, sout = abi.AmBlockState(**words), abi.AmBlockState()
        rec = np.zeros(1, dtype=RECORD_DTYPE)
        am_sym, stage = np.zeros((4, abi.AM_SYMS), dtype=np.uint8), np.zeros(240, dtype=np.int8)
        spectra = np.zeros((abi.AM_NSYM, abi.AM_FFT), dtype=np.complex64) if dump else None
        mult = np.zeros((4, abi.AM_PW), dtype=np.complex64) if dump else None
        self._check(self.lib.nrsc5hip_stage_am_block(self._h, _ptr(win), _ptr(hist), ctypes.byref(sin), fill, 1 if dump else 0, rec.ctypes.data, ctypes.byref(sout),
                                                     am_sym.ctypes.data, stage.ctypes.data, _ptr(spectra), _ptr(mult)))
        out = dict(rec=rec[0], state={n: getattr(sout, n) for n, _ in abi.AmBlockState._fields_}, am_sym=am_sym, pids_stage=stage)
        if dump:
            out.update(spectra=spectra, mult=mult)
        return out

    def debug_fetch_am_sym(self, stream: int) -> np.ndarray:
        """the stream's hard-symbol matrices [4 (pl, pu, s, t), 6400]: block bc of the L1 frame being received at bc * 800"""
        out = np.zeros((4, abi.AM_SYMS), dtype=np.uint8)
        self._check(self.lib.nrsc5hip_debug_fetch_am_sym(self._h, stream, out.ctypes.data))
        return out

    def stage_nco_exact(self, start, inc, active, nco_mode, n: int | None = None):
        """nrsc5hip_stage_nco_exact: launch_nco_exact on streams 0 .. n-1.  start / inc float32 [n, 2], active / nco_mode int [n] ->
        (tab float32 [n, 32 * 2160, 2], rows the kernel left alone still filled with 0xA5 bytes; end float32 [n, 2])"""
        n = len(active) if n is None else n
        m = max(n, 0)
        start, inc = _exact(start, np.float32, 2 * m), _exact(inc, np.float32, 2 * m)
        active, nco_mode = _exact(active, np.int32, m), _exact(nco_mode, np.int32, m)
        tab, end = np.zeros((m, 32 * 2160, 2), dtype=np.float32), np.zeros((m, 2), dtype=np.float32)
        self._check(self.lib.nrsc5hip_stage_nco_exact(self._h, n, _ptr(start), _ptr(inc), _ptr(active), _ptr(nco_mode), tab.ctypes.data, end.ctypes.data))
        return tab, end

    def stage_symbols(self, form: int, streams, params_mode: int = 0, prepare: int = 0, ids=None, n: int | None = None):
        """nrsc5hip_stage_symbols: launch_mixfft in the form `form` (abi.SYM_FORMS), one block, on streams 0 .. n-1.  streams: per stream a dict with either
        raw (uint8 cu8 capture, read in place; lead 0 / 4 / 8 / 12) or q15 (int16 [., 2] FIFO window), optionally nco_tab (float32 [32, 2160, 2]), and the words
        of abi.SymStream for the mode: 0 -- a00, dtheta, theta, growth, active (default 1), nco_mode; 1 -- a FINE state samperr, cfo, angle, prev_angle, theta,
        rd, wr, run with launch_mixfft(local_prepare = 1) alone (prepare = 1) or launch_prepare first (prepare = 0).  ids: the launch's stream list, a
        permutation of 0 .. n-1, or None ->
        (bins complex64 [max_streams, 32, 534], rows the kernel left alone still filled with 0xA5 bytes; per stream a dict of abi.SymParams read back)"""
        n = len(streams) if n is None else n
        m = max(n, 0)
        arr, keep = (abi.SymStream * max(m, 1))(), []
        for s, d in enumerate(list(streams or ())[:m]):
            d = dict(d)
            c = arr[s]
            for key, dt in (("raw", np.uint8), ("q15", np.int16), ("nco_tab", np.float32)):
                a = d.pop(key, None)
                if a is None:
                    continue
                a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
                if key == "nco_tab" and a.size != 32 * 2160 * 2:
                    raise ValueError("nco_tab holds %d floats, not 32 * 2160 * 2" % a.size)
                keep.append(a)
                setattr(c, key, a.ctypes.data)
                if key == "raw":
                    c.raw_bytes = d.pop("raw_bytes", a.size)
                elif key == "q15":
                    c.q15_samples = d.pop("q15_samples", a.size // 2)
            c.active = 1
            for key, v in d.items():
                if key not in dict(abi.SymStream._fields_) or key in ("raw", "q15", "nco_tab", "pad0"):
                    raise ValueError("not a word of nrsc5hip_sym_stream: %s" % key)
                setattr(c, key, v)
        idl = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        bins = np.zeros((self.max_streams, abi.SYM_NSYM, abi.SYM_LIVE), dtype=np.complex64)
        out = (abi.SymParams * max(m, 1))()
        self._check(self.lib.nrsc5hip_stage_symbols(self._h, n, form, params_mode, prepare, ctypes.addressof(arr) if streams is not None else None, _ptr(idl),
                                                    bins.ctypes.data, ctypes.addressof(out)))
        return bins, [{k: getattr(out[s], k) for k, _ in abi.SymParams._fields_} for s in range(m)]

    def stage_selftest(self) -> int:
        n = ctypes.c_int(-1)
        self._check(self.lib.nrsc5hip_stage_selftest(self._h, ctypes.byref(n)))
        return n.value

    def debug_fetch_costas(self, stream: int):
        f = np.zeros(534, dtype=np.float32); p = np.zeros(534, dtype=np.float32)
        self._check(self.lib.nrsc5hip_debug_fetch_costas(self._h, stream, f.ctypes.data, p.ctypes.data))
        return f, p

    def debug_fetch_px(self, stream: int) -> np.ndarray:
        out = np.zeros((2, 2, 4608), dtype=np.int8)
        self.lib.nrsc5hip_debug_fetch_px.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        self._check(self.lib.nrsc5hip_debug_fetch_px(self._h, stream, out.ctypes.data))
        return out

    def debug_fetch(self, stream: int):
        pm = np.zeros(16 * 23040, dtype=np.int8)
        bins = np.zeros((32, 534), dtype=np.complex64)
        self._check(self.lib.nrsc5hip_debug_fetch(self._h, stream, pm.ctypes.data, bins.ctypes.data))
        return pm, bins


class Channelizer:
    """Wideband channelizer (nrsc5hip_chan_*): one capture at rate = rate_num / rate_den S/s in `fmt` (IQ_CU8 / IQ_CS16 / IQ_CF32)
    -> one reference-format cs16 stream at 744 187.5 S/s per entry of offsets_hz.  Input and output buffers are device pointers
    (ints) or torch tensors on the channelizer's device."""

    OUT_RATE = 744187.5

    def __init__(self, rate, fmt: int, offsets_hz, gains=None, device: int = 0, lib_path: str | None = None):
        from fractions import Fraction
        self.lib = load_library(lib_path)
        r = Fraction(rate).limit_denominator(1 << 20) if isinstance(rate, float) else Fraction(rate)
        self.rate_num, self.rate_den = r.numerator, r.denominator
        self.fmt, self.device = int(fmt), device
        self.offsets = np.ascontiguousarray(offsets_hz, dtype=np.float64).reshape(-1)
        self.gains = None if gains is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gains, dtype=np.float32), self.offsets.shape))
        self.nchan = int(self.offsets.size)
        self.cfg = _ChanConfig(device, self.fmt, self.nchan, self.rate_num, self.rate_den, self.offsets.ctypes.data,
                               None if self.gains is None else self.gains.ctypes.data)
        self._h = ctypes.c_void_p()
        self._check(self.lib.nrsc5hip_chan_create(ctypes.byref(self.cfg), ctypes.byref(self._h)))
        T, L = ctypes.c_int(), ctypes.c_int()
        self.realised = np.zeros(self.nchan, dtype=np.float64)
        self._check(self.lib.nrsc5hip_chan_info(self._h, self.realised.ctypes.data, ctypes.byref(T), ctypes.byref(L)))
        self.taps, self.phases = T.value, L.value

    def _check(self, rc: int):
        if rc != 0:
            err = Nrsc5HipError(f"libnrsc5hip error {rc}: {self.lib.nrsc5hip_last_error().decode()}")
            err.code = rc
            raise err

    def close(self):
        if self._h:
            self.lib.nrsc5hip_chan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._check(self.lib.nrsc5hip_chan_reset(self._h))

    def table(self) -> np.ndarray:
        """the prototype as stored: float32 [phases][taps]"""
        t = np.zeros((self.phases, self.taps), dtype=np.float32)
        self._check(self.lib.nrsc5hip_chan_taps(self._h, t.ctypes.data))
        return t

    def outputs_for(self, n_in: int) -> int:
        n = int(self.lib.nrsc5hip_chan_outputs_for(self._h, n_in))
        if n < 0:
            self._check(n)
        return n

    def clip_counts(self) -> np.ndarray:
        out = np.zeros(self.nchan, dtype=np.int64)
        self._check(self.lib.nrsc5hip_chan_clip_counts(self._h, out.ctypes.data))
        return out

    def process(self, dev_in: int, n_in: int, dev_out: int, stride_elems: int, capacity: int) -> int:
        """raw form: n_in samples at device pointer dev_in; channel k's outputs at dev_out + k * stride_elems (int16); -> outputs per channel"""
        n = ctypes.c_longlong()
        self._check(self.lib.nrsc5hip_chan_process(self._h, dev_in, n_in, dev_out, stride_elems, capacity, ctypes.byref(n)))
        return n.value

    def process_tensor(self, x):
        """torch device tensor of interleaved samples (uint8 / int16 / float32 by format) -> int16 tensor [nchan, n_out, 2]"""
        import torch
        n_in = x.numel() // 2
        n_out = self.outputs_for(n_in)
        out = torch.empty((self.nchan, max(n_out, 1), 2), dtype=torch.int16, device=x.device)
        x = x.contiguous()
        torch.cuda.current_stream(x.device).synchronize()          # the producer of x has finished: the channelizer runs on its own stream
        got = self.process(x.data_ptr(), n_in, out.data_ptr(), 2 * out.shape[1], out.shape[1])
        assert got == n_out
        return out[:, :n_out]

    def feed(self, engine: "Engine", stream_ids, dev_in: int, n_in: int):
        """channelize and append channel k's outputs to stream_ids[k] of `engine` (follow with engine.batch_process)"""
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32)
        assert ids.size == self.nchan
        self._check(self.lib.nrsc5hip_chan_feed(self._h, engine._h, ids.ctypes.data, dev_in, n_in))

    def feed_fm(self, engine: "Engine", stream_ids, fm: "FmDemod", dev_in: int, n_in: int, dev_audio: int, audio_stride_elems: int, audio_capacity: int) -> int:
        """feed(), and `fm` demodulates the same staged outputs on the device (nrsc5hip_chan_feed_fm); -> audio frames per channel"""
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32)
        assert ids.size == self.nchan
        n = ctypes.c_longlong()
        self._check(self.lib.nrsc5hip_chan_feed_fm(self._h, engine._h, ids.ctypes.data, fm._h, dev_in, n_in, dev_audio, audio_stride_elems,
                                                   audio_capacity, ctypes.byref(n)))
        return n.value


class FmDemod:
    """Analog FM audio (nrsc5hip_fm_*): nchan cs16 streams at 744 187.5 S/s -> 44.1 kS/s stereo int16 frames (L, R) per channel.
    deemphasis_us: 75, 50 or 0; pilot_min: least pilot level of a stereo block (0: the default, 0.03).  Buffers are device pointers
    (ints) or torch tensors on the demodulator's device."""

    AUDIO_RATE = FM_AUDIO_RATE

    def __init__(self, nchan: int, deemphasis_us: float = 75.0, pilot_min: float = 0.0, gains=None, device: int = 0, lib_path: str | None = None,
                 rds: bool = False, rds_raw_groups: bool = False, rds_correct_burst: int = 2, carrier: bool = False, steer=False,
                 same: bool = False, same_burst_events: bool = True, impair=False):
        self.lib = load_library(lib_path)
        self.nchan, self.device, self.deemphasis_us = int(nchan), device, float(deemphasis_us)
        self.gains = None if gains is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gains, dtype=np.float32), (self.nchan,)))
        self.cfg = _FmConfig(device, self.nchan, self.deemphasis_us, float(pilot_min), None if self.gains is None else self.gains.ctypes.data)
        self._h = ctypes.c_void_p()
        self._check(self.lib.nrsc5hip_fm_create(ctypes.byref(self.cfg), ctypes.byref(self._h)))
        ta, tb, ph, lat = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        self._check(self.lib.nrsc5hip_fm_info(self._h, ctypes.byref(ta), ctypes.byref(tb), ctypes.byref(ph), ctypes.byref(lat)))
        self.taps_channel, self.taps_audio, self.phases, self.latency_in = ta.value, tb.value, ph.value, lat.value
        self.rds = False
        self.carrier_enabled = False
        self.steer_config = None
        self.same = False
        self.impair_config = None
        if rds or carrier or steer or same or impair:
            try:
                if rds:
                    self.rds_enable(rds_raw_groups, rds_correct_burst)
                if carrier:
                    self.carrier_enable()
                if steer:
                    self.steer_enable(**({} if steer is True else dict(steer)))
                if same:
                    self.same_enable(same_burst_events)
                if impair:
                    self.impair_enable(**({} if impair is True else dict(impair)))
            except Nrsc5HipError:
                self.close()                                       # the demodulator that was created goes with the failed constructor
                raise

    _check = Channelizer._check

    # ---- RDS / RBDS of the analog host (nrsc5hip_fm_rds_*) ----------------------------------------------------------------------
    def rds_enable(self, raw_groups: bool = False, correct_burst: int = 2):
        """only before the first push; from then on every process() also decodes RDS on the same stream"""
        self._check(self.lib.nrsc5hip_fm_rds_enable(self._h, ctypes.byref(_RdsConfig(int(raw_groups), int(correct_burst)))))
        self.rds = True
        nt, ph, ppb, wb, lat = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        self._check(self.lib.nrsc5hip_fm_rds_info(self._h, ctypes.byref(nt), ctypes.byref(ph), ctypes.byref(ppb), ctypes.byref(wb), ctypes.byref(lat)))
        self.rds_taps, self.rds_phases, self.rds_points_per_bit, self.rds_window_bits, self.rds_latency_in = nt.value, ph.value, ppb.value, wb.value, lat.value

    def rds_read(self) -> list:
        """the events since the last read -> [{"channel", "kind", "group", "bit", "v", "data"}, ...], channel by channel, each channel's in order"""
        out = []

        def on_event(_opaque, channel, kind, group, bit, v, data, n):
            out.append({"channel": channel, "kind": RDS_KINDS[kind], "group": group, "bit": bit, "v": [int(v[k]) for k in range(8)], "data": ctypes.string_at(data, n)})

        self._check(min(self.lib.nrsc5hip_fm_rds_read(self._h, RDS_CB(on_event), None), 0))
        return out

    def rds_get(self, channel: int) -> dict:
        """the snapshot of one channel: PI (-1: none), PTY, flags, the last name and text reported (None: none yet), clock, synced"""
        info = RdsInfo()
        self._check(self.lib.nrsc5hip_fm_rds_get(self._h, channel, ctypes.byref(info)))
        return {"pi": info.pi, "pty": info.pty, "tp": info.tp, "ta": info.ta, "ms": info.ms, "di": info.di, "synced": info.synced,
                "ps": bytes(info.ps) if info.ps_len >= 0 else None, "rt": bytes(info.rt[:info.rt_len]) if info.rt_len >= 0 else None, "rt_ab": info.rt_ab,
                "clock": (info.mjd, info.hour, info.minute, info.offset_half_hours) if info.have_clock else None}

    def rds_stats(self, channel: int) -> dict:
        out = np.zeros(len(RDS_STATS), dtype=np.int64)
        self._check(self.lib.nrsc5hip_fm_rds_stats(self._h, channel, out.ctypes.data))
        return dict(zip(RDS_STATS, (int(x) for x in out)))

    def rds_tables(self) -> np.ndarray:
        """float32 [rds_phases][rds_taps]: the matched filter as stored"""
        tab = np.zeros((self.rds_phases, self.rds_taps), dtype=np.float32)
        self._check(self.lib.nrsc5hip_fm_rds_taps(self._h, tab.ctypes.data))
        return tab

    def stage_rds_mf(self, dev_in: int, in_stride_elems: int, n_in: int) -> dict:
        """nrsc5hip_stage_rds_mf -> {"y" complex64 [nchan][points], "energy" float32 [nchan][windows][8], "s" int32 [nchan][windows],
        "bits": per channel a list of uint8 arrays, one per window}"""
        m1 = (n_in + 1) // 2
        points = 0 if m1 < 628 else (304 * (m1 - 628) + 303) // 11907 + 1
        nw = points // (8 * self.rds_window_bits)
        y = np.zeros((self.nchan, points), dtype=np.complex64)
        energy, s = np.zeros((self.nchan, nw, 8), dtype=np.float32), np.zeros((self.nchan, nw), dtype=np.int32)
        bits, counts = np.zeros((self.nchan, nw, RDS_BITS_STRIDE), dtype=np.uint8), np.zeros((self.nchan, nw), dtype=np.int32)
        self._check(self.lib.nrsc5hip_stage_rds_mf(self._h, dev_in, in_stride_elems, n_in, y.ctypes.data, energy.ctypes.data, s.ctypes.data, bits.ctypes.data,
                                                   counts.ctypes.data))
        return {"y": y, "energy": energy, "s": s, "bits": [[bits[c, w, :counts[c, w]].copy() for w in range(nw)] for c in range(self.nchan)]}

    def stage_rds_groups(self, bits, channels=None, reset_at=None):
        """nrsc5hip_stage_rds_groups: bits[i] (uint8, one per bit) to the group decoder of channels[i] (default i); events come with rds_read()"""
        arrs = [np.ascontiguousarray(b, dtype=np.uint8) for b in bits]
        n = len(arrs)
        ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data if a.size else None for a in arrs])
        counts = np.array([a.size for a in arrs], dtype=np.int32)
        ch = None if channels is None else np.ascontiguousarray(channels, dtype=np.int32)
        rst = None if reset_at is None else np.ascontiguousarray(reset_at, dtype=np.int32)
        self._check(self.lib.nrsc5hip_stage_rds_groups(self._h, n, _ptr(ch), ptrs, counts.ctypes.data, _ptr(rst)))

    # ---- EAS alerts (SAME) of the analog host (nrsc5hip_fm_same_*) ------------------------------------------------------------------
    def same_enable(self, burst_events: bool = True):
        """only before the first push; from then on every process() also watches every channel's audio for SAME bursts on the same stream"""
        self._check(self.lib.nrsc5hip_fm_same_enable(self._h, ctypes.byref(_SameConfig(int(burst_events)))))
        self.same = True
        tb, ppb, wb, lat = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        self._check(self.lib.nrsc5hip_fm_same_info(self._h, ctypes.byref(tb), ctypes.byref(ppb), ctypes.byref(wb), ctypes.byref(lat)))
        self.same_table_size, self.same_points_per_bit, self.same_window_bits, self.same_latency_in = tb.value, ppb.value, wb.value, lat.value

    def same_read(self) -> list:
        """the events since the last read -> [{"channel", "kind", "first", "last", "v", "data"}, ...], channel by channel, each channel's in order"""
        out = []

        def on_event(_opaque, channel, kind, first, last, v, data, n):
            out.append({"channel": channel, "kind": SAME_KINDS[kind], "first": first, "last": last, "v": [int(v[k]) for k in range(8)], "data": ctypes.string_at(data, n)})

        self._check(min(self.lib.nrsc5hip_fm_same_read(self._h, SAME_CB(on_event), None), 0))
        return out

    def same_get(self, channel: int) -> dict:
        """the snapshot of one channel: the last message (None: none yet), its kind and bit indices, the bursts of the current group, in_message"""
        info = SameInfo()
        self._check(self.lib.nrsc5hip_fm_same_get(self._h, channel, ctypes.byref(info)))
        return {"text": bytes(info.text[:info.text_len]) if info.text_len >= 0 else None, "kind": SAME_BURST_KINDS[info.kind], "first": info.first_bit,
                "last": info.last_bit, "group_bursts": info.group_bursts, "group_kind": SAME_BURST_KINDS[info.group_kind], "in_message": int(info.in_message)}

    def same_stats(self, channel: int) -> dict:
        out = np.zeros(len(SAME_STATS), dtype=np.int64)
        self._check(self.lib.nrsc5hip_fm_same_stats(self._h, channel, out.ctypes.data))
        return dict(zip(SAME_STATS, (int(x) for x in out)))

    def same_table(self) -> np.ndarray:
        """float32 [35721][2]: (cos, sin) of 2 pi k / 35721 as stored"""
        tab = np.zeros((self.same_table_size, 2), dtype=np.float32)
        self._check(self.lib.nrsc5hip_fm_same_table(self._h, tab.ctypes.data))
        return tab

    def stage_same_tones(self, dev_in: int, in_stride_elems: int, n_in: int) -> dict:
        """nrsc5hip_stage_same_tones -> {"c" complex64 [nchan][segments][2] (mark, space), "q" float32 [nchan][windows * 512], "metric" float32
        [nchan][windows][8], "s" int32 [nchan][windows], "bits": per channel a list of uint8 arrays, one per window}"""
        segs = same_segments(n_in)
        nw = max(0, (segs - 7) // SAME_WIN_PTS)
        c = np.zeros((self.nchan, segs, 2), dtype=np.complex64)
        q, metric, s = np.zeros((self.nchan, nw * SAME_WIN_PTS), dtype=np.float32), np.zeros((self.nchan, nw, 8), dtype=np.float32), np.zeros((self.nchan, nw), dtype=np.int32)
        bits, counts = np.zeros((self.nchan, nw, SAME_BITS_STRIDE), dtype=np.uint8), np.zeros((self.nchan, nw), dtype=np.int32)
        self._check(self.lib.nrsc5hip_stage_same_tones(self._h, dev_in, in_stride_elems, n_in, c.ctypes.data, q.ctypes.data, metric.ctypes.data, s.ctypes.data,
                                                       bits.ctypes.data, counts.ctypes.data))
        return {"c": c, "q": q, "metric": metric, "s": s, "bits": [[bits[k, w, :counts[k, w]].copy() for w in range(nw)] for k in range(self.nchan)]}

    def stage_same_frames(self, bits, channels=None, reset_at=None):
        """nrsc5hip_stage_same_frames: bits[i] (uint8, one per bit) to the framer of channels[i] (default i); events come with same_read()"""
        arrs = [np.ascontiguousarray(b, dtype=np.uint8) for b in bits]
        n = len(arrs)
        ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data if a.size else None for a in arrs])
        counts = np.array([a.size for a in arrs], dtype=np.int32)
        ch = None if channels is None else np.ascontiguousarray(channels, dtype=np.int32)
        rst = None if reset_at is None else np.ascontiguousarray(reset_at, dtype=np.int32)
        self._check(self.lib.nrsc5hip_stage_same_frames(self._h, n, _ptr(ch), ptrs, counts.ctypes.data, _ptr(rst)))

    # ---- carrier quality of the analog host (nrsc5hip_fm_carrier*) -----------------------------------------------------------------
    def carrier_enable(self):
        """only before the first push; from then on every process() also measures every channel's carrier on the same stream"""
        self._check(self.lib.nrsc5hip_fm_carrier_enable(self._h))
        self.carrier_enabled = True

    def carrier(self) -> list:
        """one dict per channel: {"windowed": {...}, "running": {...}, "blocks", "audio_blocks"}; a report holds "level_db", "cnr_db", "offset_hz"
        and the sums behind them, "sum2", "sum4", "sum1", "count" (windowed: of the last audio block delivered; running: since create / reset)"""
        out = (FmCarrierInfo * self.nchan)()
        self._check(self.lib.nrsc5hip_fm_carrier(self._h, ctypes.addressof(out)))
        names = [n for n, _ in FmCarrierReport._fields_]
        return [{"windowed": {n: float(getattr(o.windowed, n)) for n in names}, "running": {n: float(getattr(o.running, n)) for n in names},
                 "blocks": int(o.blocks), "audio_blocks": int(o.audio_blocks)} for o in out]

    def stage_carrier(self, dev_in: int, in_stride_elems: int, n_in: int):
        """nrsc5hip_stage_fm_carrier -> (r float32 [nchan][(n_in + 1) // 2], block triples float64 [nchan][blocks][3]: s2, s4, s1)"""
        m1 = (n_in + 1) // 2
        r = np.zeros((self.nchan, m1), dtype=np.float32)
        t = np.zeros((self.nchan, m1 // 540, 3), dtype=np.float64)
        self._check(self.lib.nrsc5hip_stage_fm_carrier(self._h, dev_in, in_stride_elems, n_in, r.ctypes.data, t.ctypes.data))
        return r, t

    # ---- reception steering: blend, high-cut and mute by the carrier quality of the block (nrsc5hip_fm_steer*) ------------------------------
    def steer_enable(self, blend_db=None, highcut_db=None, mute_db=None, mute_floor_db=None, controls=None):
        """only before the first push, and once; enables the carrier measurement when it is off.  Thresholds are (lo_db, hi_db) in dB CNR as
        carrier() reports it; controls: FM_STEER_* or'ed, or names ("blend", "highcut", "mute").  No argument: the defaults (FM_STEER_DEFAULTS)"""
        cfg = dict(FM_STEER_DEFAULTS)
        for k, v in (("blend_db", blend_db), ("highcut_db", highcut_db), ("mute_db", mute_db), ("mute_floor_db", mute_floor_db), ("controls", controls)):
            if v is not None:
                cfg[k] = v
        if not isinstance(cfg["controls"], int):
            bits = 0
            for name in cfg["controls"]:
                bits |= FM_STEER_CONTROLS[name]
            cfg["controls"] = bits
        pair = lambda v: (ctypes.c_double * 2)(float(v[0]), float(v[1]))
        c = _FmSteerConfig(int(cfg["controls"]), pair(cfg["blend_db"]), pair(cfg["highcut_db"]), pair(cfg["mute_db"]), float(cfg["mute_floor_db"]))
        self._check(self.lib.nrsc5hip_fm_steer_enable(self._h, ctypes.byref(c)))
        self.steer_config = cfg
        self.carrier_enabled = True

    def steer(self) -> list:
        """one dict per channel: {"q", "blend", "highcut", "mute"} at the end of the last audio block delivered (all 0 before the first)"""
        out = np.zeros((self.nchan, 4), dtype=np.float32)
        self._check(self.lib.nrsc5hip_fm_steer(self._h, out.ctypes.data))
        return [{"q": float(v[0]), "blend": float(v[1]), "highcut": float(v[2]), "mute": float(v[3])} for v in out]

    def steer_taps(self) -> np.ndarray:
        """float32 [phases][taps_audio]: the narrow table as stored"""
        tab = np.zeros((self.phases, self.taps_audio), dtype=np.float32)
        self._check(self.lib.nrsc5hip_fm_steer_taps(self._h, tab.ctypes.data))
        return tab

    def stage_steer(self, dev_in: int, in_stride_elems: int, n_in: int) -> np.ndarray:
        """nrsc5hip_stage_fm_steer -> float32 [nchan][audio blocks][4]: (q, b, h, g) of every audio block of the input taken as a whole session"""
        out = np.zeros((self.nchan, max(0, ((n_in + 1) // 2) // 540 - 16), 4), dtype=np.float32)
        self._check(self.lib.nrsc5hip_stage_fm_steer(self._h, dev_in, in_stride_elems, n_in, out.ctypes.data))
        return out

    # ---- reception impairments: multipath and adjacent-channel detectors (nrsc5hip_fm_impair*) ---------------------------------------------
    def impair_enable(self, explained_min=None, depth_min=None, rho_min=None):
        """only before the first push, and once; enables the carrier measurement when it is off.  No argument: the defaults (FM_IMPAIR_DEFAULTS)"""
        cfg = dict(FM_IMPAIR_DEFAULTS)
        for k, v in (("explained_min", explained_min), ("depth_min", depth_min), ("rho_min", rho_min)):
            if v is not None:
                cfg[k] = float(v)
        c = _FmImpairConfig(cfg["explained_min"], cfg["depth_min"], cfg["rho_min"])
        self._check(self.lib.nrsc5hip_fm_impair_enable(self._h, ctypes.byref(c)))
        self.impair_config = cfg
        self.carrier_enabled = True

    def impair(self) -> list:
        """one dict per channel: {"windowed": {...}, "running": {...}, "blocks", "audio_blocks"}; a report holds the figures "explained", "depth",
        "slope", "curvature", "usn_db", "ripple_db", "rho", the verdict "multipath", "adjacent" (bool) and "side" (+1: the neighbour is above,
        -1: below, 0: none), and the sums behind them, FM_IMPAIR_SUMS and "count" (windowed: of the last audio block delivered; running: since
        create / reset)"""
        out = (FmImpairInfo * self.nchan)()
        self._check(self.lib.nrsc5hip_fm_impair(self._h, ctypes.addressof(out)))

        def report(r):
            v = {n: float(getattr(r, n)) for n in FM_IMPAIR_SUMS + ("count",) + FM_IMPAIR_FIGURES}
            v.update(multipath=bool(r.verdict & FM_IMPAIR_MULTIPATH), adjacent=bool(r.verdict & FM_IMPAIR_ADJACENT), side=int(r.side))
            return v

        return [{"windowed": report(o.windowed), "running": report(o.running), "blocks": int(o.blocks), "audio_blocks": int(o.audio_blocks)} for o in out]

    def impair_taps(self) -> np.ndarray:
        """float32 [63]: the 100 .. 170 kHz band-pass hU as stored"""
        hu = np.zeros(FM_IMPAIR_TAPS, dtype=np.float32)
        self._check(self.lib.nrsc5hip_fm_impair_taps(self._h, hu.ctypes.data))
        return hu

    def stage_impair(self, dev_in: int, in_stride_elems: int, n_in: int) -> dict:
        """nrsc5hip_stage_fm_impair -> {"e", "eu", "du" float32 [nchan][540 blocks], "sums" float64 [nchan][blocks][11] (FM_IMPAIR_SUMS)} of the
        input taken as a whole session"""
        nb = ((n_in + 1) // 2) // 540
        e, eu, du = (np.zeros((self.nchan, 540 * nb), dtype=np.float32) for _ in range(3))
        sums = np.zeros((self.nchan, nb, FM_IMPAIR_NSUMS), dtype=np.float64)
        self._check(self.lib.nrsc5hip_stage_fm_impair(self._h, dev_in, in_stride_elems, n_in, e.ctypes.data, eu.ctypes.data, du.ctypes.data, sums.ctypes.data))
        return {"e": e, "eu": eu, "du": du, "sums": sums}

    def close(self):
        if self._h:
            self.lib.nrsc5hip_fm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._check(self.lib.nrsc5hip_fm_reset(self._h))

    def tables(self):
        """-> (channel filter float32 [taps_channel], audio prototype float32 [phases][taps_audio]) as stored"""
        ha = np.zeros(self.taps_channel, dtype=np.float32)
        tab = np.zeros((self.phases, self.taps_audio), dtype=np.float32)
        self._check(self.lib.nrsc5hip_fm_taps(self._h, ha.ctypes.data, tab.ctypes.data))
        return ha, tab

    def outputs_for(self, n_in: int) -> int:
        n = int(self.lib.nrsc5hip_fm_outputs_for(self._h, n_in))
        if n < 0:
            self._check(n)
        return n

    def clip_counts(self) -> np.ndarray:
        """int64 [nchan][2]: clamped L and R samples since create / reset"""
        out = np.zeros((self.nchan, 2), dtype=np.int64)
        self._check(self.lib.nrsc5hip_fm_clip_counts(self._h, out.ctypes.data))
        return out

    def launches(self) -> int:
        """nrsc5hip_fm_debug_launches: kernel launches the pushes have issued since create / reset (test hook)"""
        n = ctypes.c_longlong()
        self._check(self.lib.nrsc5hip_fm_debug_launches(self._h, ctypes.byref(n)))
        return n.value

    def pilot(self):
        """-> (level float32 [nchan], stereo bool [nchan]) of the last audio block delivered"""
        level, flag = np.zeros(self.nchan, dtype=np.float32), np.zeros(self.nchan, dtype=np.int32)
        self._check(self.lib.nrsc5hip_fm_pilot(self._h, level.ctypes.data, flag.ctypes.data))
        return level, flag.astype(bool)

    def process(self, dev_in: int, in_stride_elems: int, n_in: int, dev_out: int, out_stride_elems: int, capacity: int) -> int:
        """raw form: channel k's n_in samples at dev_in + k * in_stride_elems, its frames to dev_out + k * out_stride_elems (int16
        elements); -> frames per channel"""
        n = ctypes.c_longlong()
        self._check(self.lib.nrsc5hip_fm_process(self._h, dev_in, in_stride_elems, n_in, dev_out, out_stride_elems, capacity, ctypes.byref(n)))
        return n.value

    def process_tensor(self, x):
        """torch int16 device tensor [nchan, n, 2] -> int16 tensor [nchan, frames, 2]"""
        import torch
        x = x.contiguous()
        n_in = x.shape[1]
        n_out = self.outputs_for(n_in)
        out = torch.empty((self.nchan, max(n_out, 1), 2), dtype=torch.int16, device=x.device)
        torch.cuda.current_stream(x.device).synchronize()          # the demodulator runs on its own stream
        got = self.process(x.data_ptr(), 2 * n_in, n_in, out.data_ptr(), 2 * out.shape[1], out.shape[1])
        assert got == n_out
        return out[:, :n_out]

    def stage_mpx(self, dev_in: int, in_stride_elems: int, n_in: int):
        """nrsc5hip_stage_fm_mpx -> (d float32 [nchan][(n_in + 1) // 2], block sums complex64 [nchan][blocks])"""
        m1 = (n_in + 1) // 2
        d = np.zeros((self.nchan, m1), dtype=np.float32)
        p = np.zeros((self.nchan, m1 // 540), dtype=np.complex64)
        self._check(self.lib.nrsc5hip_stage_fm_mpx(self._h, dev_in, in_stride_elems, n_in, d.ctypes.data, p.ctypes.data))
        return d, p


def _stations(out, n: int) -> list:
    return [{"offset_hz": float(s.offset_hz), "score_db": float(s.score_db), "lower_db": float(s.lower_db), "upper_db": float(s.upper_db),
             "floor_db": float(s.floor_db)} for s in out[:n]]


def detect_psd(psd, fs: float, threshold_db: float = 6.0, min_separation_hz: float = 100e3, max_stations: int = 512,
               lib: ctypes.CDLL | None = None, lib_path: str | None = None) -> list:
    """nrsc5hip_scan_detect_psd: the library's host detector on any spectrum (psd[i] at (i - nfft/2) * fs / nfft); no device, no scan
    object.  -> [{"offset_hz", "score_db", "lower_db", "upper_db", "floor_db"}, ...], highest score first"""
    lib = lib or load_library(lib_path)
    psd = np.ascontiguousarray(psd, dtype=np.float64)
    out = (ScanStation * max(max_stations, 1))()
    n = ctypes.c_int()
    rc = lib.nrsc5hip_scan_detect_psd(psd.ctypes.data, psd.size, float(fs), ctypes.byref(ScanParams(threshold_db, min_separation_hz)),
                                      ctypes.addressof(out), max_stations, ctypes.byref(n))
    if rc != 0:
        err = Nrsc5HipError(f"libnrsc5hip error {rc}: {lib.nrsc5hip_last_error().decode()}")
        err.code = rc
        raise err
    return _stations(out, min(n.value, max_stations))


def _fm_stations(out, n: int) -> list:
    return [{"offset_hz": float(s.offset_hz), "bin_hz": float(s.bin_hz), "score_db": float(s.score_db), "floor_db": float(s.floor_db)} for s in out[:n]]


def detect_fm_psd(psd, fs: float, threshold_db: float = 6.0, min_separation_hz: float = 150e3, max_stations: int = 512,
                  lib: ctypes.CDLL | None = None, lib_path: str | None = None) -> list:
    """nrsc5hip_scan_detect_fm_psd: the library's host detector of analog FM carriers on any spectrum; no device, no scan object.
    -> [{"offset_hz" (the centroid), "bin_hz" (the bin picked), "score_db", "floor_db"}, ...], highest score first"""
    lib = lib or load_library(lib_path)
    psd = np.ascontiguousarray(psd, dtype=np.float64)
    out = (ScanFmStation * max(max_stations, 1))()
    n = ctypes.c_int()
    rc = lib.nrsc5hip_scan_detect_fm_psd(psd.ctypes.data, psd.size, float(fs), ctypes.byref(ScanParams(threshold_db, min_separation_hz)),
                                         ctypes.addressof(out), max_stations, ctypes.byref(n))
    if rc != 0:
        err = Nrsc5HipError(f"libnrsc5hip error {rc}: {lib.nrsc5hip_last_error().decode()}")
        err.code = rc
        raise err
    return _fm_stations(out, min(n.value, max_stations))


class Scanner:
    """Band scan (nrsc5hip_scan_*): the averaged power spectrum of one capture at rate = rate_num / rate_den S/s in `fmt` (IQ_CU8 /
    IQ_CS16 / IQ_CF32) and the hybrid-FM stations in it.  nfft: a power of two in 512..8192, or 0 for the rate's default.  Input
    buffers are device pointers (ints) or torch tensors on the scanner's device."""

    def __init__(self, rate, fmt: int, nfft: int = 0, device: int = 0, lib_path: str | None = None):
        from fractions import Fraction
        self.lib = load_library(lib_path)
        r = Fraction(rate).limit_denominator(1 << 20) if isinstance(rate, float) else Fraction(rate)
        self.rate_num, self.rate_den = r.numerator, r.denominator
        self.rate = self.rate_num / self.rate_den
        self.fmt, self.device = int(fmt), device
        self._h = ctypes.c_void_p()
        cfg = _ScanConfig(device, self.fmt, self.rate_num, self.rate_den, int(nfft))
        self._check(self.lib.nrsc5hip_scan_create(ctypes.byref(cfg), ctypes.byref(self._h)))
        n, seg, bw = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_double()
        self._check(self.lib.nrsc5hip_scan_info(self._h, ctypes.byref(n), ctypes.byref(seg), ctypes.byref(bw)))
        self.nfft, self.bin_hz = n.value, bw.value

    def _check(self, rc: int):
        if rc != 0:
            err = Nrsc5HipError(f"libnrsc5hip error {rc}: {self.lib.nrsc5hip_last_error().decode()}")
            err.code = rc
            raise err

    def close(self):
        if self._h:
            self.lib.nrsc5hip_scan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._check(self.lib.nrsc5hip_scan_reset(self._h))

    @property
    def segments(self) -> int:
        seg = ctypes.c_longlong()
        self._check(self.lib.nrsc5hip_scan_info(self._h, None, ctypes.byref(seg), None))
        return seg.value

    def push(self, dev_in: int, n_in: int):
        """raw form: n_in samples at device pointer dev_in"""
        self._check(self.lib.nrsc5hip_scan_push(self._h, dev_in, n_in))

    def push_tensor(self, x):
        """torch device tensor of interleaved samples (uint8 / int16 / float32 by format)"""
        import torch
        x = x.contiguous()
        torch.cuda.current_stream(x.device).synchronize()          # the producer of x has finished: the scanner runs on its own stream
        self.push(x.data_ptr(), x.numel() // 2)

    def spectrum(self):
        """-> (freqs_hz [nfft], psd [nfft]), float64; bin i at (i - nfft/2) * bin_hz"""
        psd = np.zeros(self.nfft, dtype=np.float64)
        self._check(self.lib.nrsc5hip_scan_spectrum(self._h, psd.ctypes.data))
        return (np.arange(self.nfft) - self.nfft // 2) * self.bin_hz, psd

    def detect(self, threshold_db: float = 6.0, min_separation_hz: float = 100e3, max_stations: int = 512) -> list:
        """-> [{"offset_hz", "score_db", "lower_db", "upper_db", "floor_db"}, ...], highest score first"""
        out = (ScanStation * max(max_stations, 1))()
        n = ctypes.c_int()
        self._check(self.lib.nrsc5hip_scan_detect(self._h, ctypes.byref(ScanParams(threshold_db, min_separation_hz)), ctypes.addressof(out),
                                                  max_stations, ctypes.byref(n)))
        return _stations(out, min(n.value, max_stations))

    def detect_fm(self, threshold_db: float = 6.0, min_separation_hz: float = 150e3, max_stations: int = 512) -> list:
        """the analog FM carriers of the spectrum (nrsc5hip_scan_detect_fm) -> [{"offset_hz", "bin_hz", "score_db", "floor_db"}, ...]"""
        out = (ScanFmStation * max(max_stations, 1))()
        n = ctypes.c_int()
        self._check(self.lib.nrsc5hip_scan_detect_fm(self._h, ctypes.byref(ScanParams(threshold_db, min_separation_hz)), ctypes.addressof(out),
                                                     max_stations, ctypes.byref(n)))
        return _fm_stations(out, min(n.value, max_stations))


def l2_jobs_from_records(stream: int, recs: np.ndarray, mode: int = 0):
    """nrsc5hip_l2_job tuples for every logical frame the records announce, in the order frame_push would see them."""
    jobs = []
    for r in recs:
        fl = int(r["flags"])
        if mode == MODE_AM:
            if fl & REC_P1:
                jobs.append((stream, int(r["p1_slot"]), L2_AM, int(r["bc_decoded"]), AM_P1_BITS))
            if fl & REC_P3:
                jobs.append((stream, int(r["p1_slot"]), L2_AM, 8, 30000 if int(r["psmi"]) == 2 else 24000))
        else:
            if fl & REC_P1:
                jobs.append((stream, int(r["p1_slot"]), L2_FM_P1, 0, P1_BITS))
            for flag, ch in ((REC_P3, 0), (REC_P4, 1)):
                if fl & flag:
                    jobs.append((stream, int(r["sis"]), L2_FM_PX, ch, 2304 if int(r["psmi"]) == 2 else 4608))
    return jobs


_BLOCK_KEYS = ("state_before", "state_after", "samperr", "cfo", "keep", "bc", "psmi", "cfo_wait",
               "next_samperr", "prev_angle", "phase_re", "phase_im", "next_angle")


def am_records_to_log(engine: Engine, stream: int, recs: np.ndarray, frames: np.ndarray | None = None):
    """AM twin of records_to_log: the reference's order inside one acquire_process call is
    [state, sync], pids, P1 frame, [P3 frame, ber], block (sync.c:639-765, decode.c:507-554)."""
    out = []
    for r in recs:
        fl = int(r["flags"])
        if fl & REC_TO_COARSE:
            out.append(("state", {"old": int(r["state_before"]), "new": SYNC_COARSE}))
        if fl & REC_TO_FINE:
            sis = int(r["sis"])
            out.append(("state", {"old": SYNC_COARSE, "new": SYNC_FINE}))
            out.append(("sync", {"freq_offset": float(r["freq_offset"]), "psmi": int(r["psmi"]), "pli": sis & 1, "hppi": (sis >> 1) & 1,
                                 "aabi": (sis >> 2) & 1, "rdbi": (sis >> 3) & 1}))
        if fl & REC_PIDS:
            out.append(("pids", {"bits": unpack_bits(r["pids"], PIDS_BITS)}))
        slot, bc = int(r["p1_slot"]), int(r["bc_decoded"])
        if fl & REC_P1:
            if frames is not None:
                bits = unpack_bits(frames[slot][bc * AM_P1_WORDS:(bc + 1) * AM_P1_WORDS], AM_P1_BITS)
            else:
                bits = engine.am_frame_bits(stream, slot, bc, AM_P1_BITS)
            out.append(("frame", {"lc": 0, "bits": bits}))
            if fl & REC_LOST_SYNC:                              # frame_push(P1) -> frame_process -> input_set_sync_state(NONE)
                out.append(("state", {"old": SYNC_FINE, "new": SYNC_NONE}))
                out.append(("lost_sync", {}))
        if fl & REC_P3:
            n3 = 30000 if int(r["psmi"]) == 2 else 24000
            if frames is not None:
                bits = unpack_bits(frames[slot][AM_P3_WORD0:AM_P3_WORD0 + (n3 + 31) // 32], n3)
            else:
                bits = engine.am_frame_bits(stream, slot, 8, n3)
            out.append(("frame", {"lc": 1, "bits": bits}))
        if (fl & REC_P1) and bc == 7:
            out.append(("ber", {"cber": float(r["ber"])}))
        out.append(("block", {k: (float(r[k]) if RECORD_DTYPE[k].kind == "f" else int(r[k])) for k in _BLOCK_KEYS}))
    return out


def records_to_log(engine: Engine, stream: int, recs: np.ndarray, frames: np.ndarray | None = None, px_frames: np.ndarray | None = None):
    """Expand block records into the ordered event list used by the oracle/reference harness logs
    (oracle/ref.py: parse_log), i.e. the order in which the reference fires them inside one
    acquire_process call."""
    out = []
    for r in recs:
        fl = int(r["flags"])
        if fl & REC_TO_COARSE:
            out.append(("state", {"old": int(r["state_before"]), "new": SYNC_COARSE}))
        if fl & REC_TO_FINE:
            out.append(("state", {"old": SYNC_COARSE, "new": SYNC_FINE}))
            out.append(("sync", {"freq_offset": float(r["freq_offset"]), "psmi": int(r["psmi"]), "pli": -1, "hppi": -1, "aabi": -1, "rdbi": -1}))
        if fl & REC_MER:
            out.append(("mer", {"lower": float(r["mer_lb"]), "upper": float(r["mer_ub"])}))
        if fl & REC_PIDS:
            out.append(("pids", {"bits": unpack_bits(r["pids"], PIDS_BITS)}))
        if fl & REC_P1:
            out.append(("ber", {"cber": float(r["ber"])}))
            if frames is not None:
                bits = unpack_bits(frames[int(r["p1_slot"])], P1_BITS)
            else:
                bits = engine.p1_frame_bits(stream, int(r["p1_slot"]))
            out.append(("frame", {"lc": 0, "bits": bits}))
        for flag, ch in ((REC_P3, 0), (REC_P4, 1)):           # decode_push_px1 / px2 (decode.c:393-437)
            if fl & flag:
                nbits = 2304 if int(r["psmi"]) == 2 else 4608
                if px_frames is not None:
                    bits = unpack_bits(px_frames[int(r["sis"]), ch], nbits)
                else:
                    bits = engine.px_frame_bits(stream, int(r["sis"]), ch, nbits)
                out.append(("frame", {"lc": 1 + ch, "bits": bits}))
        if fl & REC_LOST_SYNC:
            out.append(("state", {"old": SYNC_FINE, "new": SYNC_NONE}))
            out.append(("lost_sync", {}))
        blk = {k: (float(r[k]) if RECORD_DTYPE[k].kind == "f" else int(r[k]))
               for k in ("state_before", "state_after", "samperr", "cfo", "keep", "bc", "psmi", "cfo_wait",
                         "next_samperr", "prev_angle", "phase_re", "phase_im", "next_angle")}
        out.append(("block", blk))
    return out
