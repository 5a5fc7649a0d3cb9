"""What include/nrsc5hip.h declares, as Python: constants, ctypes structures, callback types and the error every binding raises.  A leaf module:
engine.py and consumers.py both import it, and it imports neither."""
from __future__ import annotations

import ctypes
import numpy as np


SYNC_NONE, SYNC_COARSE, SYNC_FINE = 0, 1, 2
REC_PROCESSED, REC_TO_COARSE, REC_TO_FINE, REC_MER, REC_PIDS, REC_P1 = 1, 2, 4, 8, 16, 32
REC_P3, REC_P4 = 128, 256
REC_LOST_SYNC = 64
REC_PIDS_CRC = 512
REC_DISCARDED = 1024      # never delivered by drain / batch_fetch* (replay, k_replay.hip)
PX_WORDS = 144
MODE_FM, MODE_AM = 0, 1
AM_P1_BITS, AM_P1_WORDS, AM_P3_WORD0 = 3750, 118, 944
P1_BITS, P1_WORDS, PIDS_BITS = 146176, 4568, 80

RECORD_DTYPE = np.dtype([
    ("flags", "<u4"), ("state_before", "<i4"), ("state_after", "<i4"), ("samperr", "<i4"), ("cfo", "<i4"),
    ("keep", "<i4"), ("bc", "<i4"), ("psmi", "<i4"), ("cfo_wait", "<i4"), ("next_samperr", "<i4"),
    ("prev_angle", "<f4"), ("phase_re", "<f4"), ("phase_im", "<f4"), ("next_angle", "<f4"),
    ("freq_offset", "<f4"), ("mer_lb", "<f4"), ("mer_ub", "<f4"), ("ber", "<f4"),
    ("p1_slot", "<i4"), ("bc_decoded", "<i4"), ("pids", "<u4", (3,)), ("sis", "<u4")])
assert RECORD_DTYPE.itemsize == 96


class _Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("max_streams", ctypes.c_int), ("q15_capacity", ctypes.c_longlong),
                ("record_capacity", ctypes.c_int), ("p1_slots", ctypes.c_int), ("p1_async", ctypes.c_int),
                ("l2_feedback", ctypes.c_int), ("am_enable", ctypes.c_int), ("batch_zero_copy", ctypes.c_int), ("l2_index", ctypes.c_int)]


class L2Pdu(ctypes.Structure):
    """nrsc5hip_l2_pdu (include/nrsc5hip.h)"""
    _fields_ = ([("start", ctypes.c_uint32), ("psd_off", ctypes.c_uint32), ("psd_len", ctypes.c_int32), ("audio_off", ctypes.c_uint32),
                 ("crc_bad_lo", ctypes.c_uint32), ("crc_bad_hi", ctypes.c_uint32), ("pdu_marker", ctypes.c_uint32),
                 ("hef_pdu_len", ctypes.c_uint16), ("loc", ctypes.c_uint16 * 64)] +
                [(n, ctypes.c_uint8) for n in ("codec_mode", "stream_id", "pdu_seq", "blend_control", "per_stream_delay", "common_delay",
                                               "latency", "pfirst", "plast", "seq", "nop", "hef", "la_location", "rs_corrections",
                                               "class_ind", "prog_num", "access", "prog_type", "applied_services", "elastic_seq",
                                               "align_offset", "skipped")])


class L2Frame(ctypes.Structure):
    """nrsc5hip_l2_frame"""
    _fields_ = [("pci", ctypes.c_uint32), ("nbytes", ctypes.c_uint32), ("n_pdu", ctypes.c_uint32), ("status", ctypes.c_uint32),
                ("end_offset", ctypes.c_uint32), ("lost_sync", ctypes.c_uint32), ("pdu", L2Pdu * 16)]


class L2Job(ctypes.Structure):
    """nrsc5hip_l2_job"""
    _fields_ = [("stream", ctypes.c_int32), ("slot", ctypes.c_int32), ("kind", ctypes.c_int32), ("which", ctypes.c_int32),
                ("nbits", ctypes.c_int32)]


class _ChanConfig(ctypes.Structure):
    """nrsc5hip_chan_config"""
    _fields_ = [("device", ctypes.c_int), ("format", ctypes.c_int), ("nchan", ctypes.c_int), ("rate_num", ctypes.c_longlong),
                ("rate_den", ctypes.c_longlong), ("offset_hz", ctypes.c_void_p), ("gain", ctypes.c_void_p)]


class _FmConfig(ctypes.Structure):
    """nrsc5hip_fm_config"""
    _fields_ = [("device", ctypes.c_int), ("nchan", ctypes.c_int), ("deemphasis_us", ctypes.c_double), ("pilot_min", ctypes.c_double),
                ("gain", ctypes.c_void_p)]


class _ScanConfig(ctypes.Structure):
    """nrsc5hip_scan_config"""
    _fields_ = [("device", ctypes.c_int), ("format", ctypes.c_int), ("rate_num", ctypes.c_longlong), ("rate_den", ctypes.c_longlong),
                ("nfft", ctypes.c_int)]


class ScanParams(ctypes.Structure):
    """nrsc5hip_scan_params"""
    _fields_ = [("threshold_db", ctypes.c_double), ("min_separation_hz", ctypes.c_double)]


class ScanStation(ctypes.Structure):
    """nrsc5hip_scan_station"""
    _fields_ = [("offset_hz", ctypes.c_double), ("score_db", ctypes.c_float), ("lower_db", ctypes.c_float), ("upper_db", ctypes.c_float),
                ("floor_db", ctypes.c_float)]


IQ_CU8, IQ_CS16, IQ_CF32 = 0, 1, 2
IQ_FORMATS = {"cu8": IQ_CU8, "cs16": IQ_CS16, "cf32": IQ_CF32}
IQ_DTYPES = {IQ_CU8: np.uint8, IQ_CS16: np.int16, IQ_CF32: np.float32}
EINVAL, ENOMEM, EHIP, EOVERFLOW = -1, -2, -3, -4
TRIM_RETAIN_MAX = (8 * 16 + 1) * 71280      # NRSC5HIP_TRIM_RETAIN_MAX: what Engine.batch_trim can retain per FM stream (pipeline depth, include/nrsc5hip.h)
TRIM_RETAIN_MAX_AM = (8 * 8 + 1) * 8910     # NRSC5HIP_TRIM_RETAIN_MAX_AM: ... per AM stream

FM_AUDIO_RATE = 44100                       # what nrsc5hip_fm_* delivers: stereo int16 frames per second
L2_FM_P1, L2_FM_PX, L2_AM = 0, 1, 2
TUNE_DECODE_STREAMS, TUNE_AM_DECODE_STREAMS, TUNE_VERDICT_LAG, TUNE_SYNC_PHASES, TUNE_FWD_SEGMENTS, TUNE_FWD_WARM, TUNE_AM_SEGMENTS, TUNE_DECODE_CUS, TUNE_DECODE_PRIORITY, TUNE_AM_WARM, TUNE_MIXFFT_SYMS, TUNE_DEFER_WAIT, TUNE_TRACEBACK_WALK, TUNE_SYNC_LANES, TUNE_DIRECT_DECIMATE, TUNE_EARLY_FLUSH_KB, TUNE_SEAM_PREPARE, TUNE_NCO_EXACT, TUNE_FLOW_MIN, TUNE_LOOP_EXACT, TUNE_HOST_CAPTURE, TUNE_FOLD_REPORT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21
MATH_REF_SINCOSF, MATH_REF_ATAN2F, MATH_FAST_SINCOS, MATH_FAST_SINCOS_REDUCED, MATH_FAST_ATAN2, MATH_SMALL_COS_SIN, MATH_SMALL_ATAN = range(7)   # NRSC5HIP_MATH_*
HB_ACQ, HB_SYM128, HB_SYM256 = range(3)     # NRSC5HIP_HB_*: the forms of the fused half-band (csrc/halfband_raw.h)
CODE_E1, CODE_E2 = 1, 2                     # NRSC5HIP_CODE_*: the two K=9 codes of the AM path
HB_SYM_N = 2160                             # decimated samples of one symbol
ACQ_WIN_FM, ACQ_SYM_FM, ACQ_WIN_AM, ACQ_SYM_AM = 71280, 2160, 8910, 270   # acquisition window (33 symbols) and symbol, FM / AM
L2_STATUS = ("end", "no_audio", "fixed_data", "header_rs", "bad_locators", "too_many_pdus", "hef_overrun", "bad_stream", "bad_length", "audio_end")


HDC_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint, ctypes.c_uint)
AAS_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint)   # nrsc5hip_aas_cb
PSD_STATS = ("pdus", "span_bytes", "closed", "empty", "bad_fcs", "wrong_protocol", "truncated_escape", "overflows", "delivered", "d2h_bytes")   # nrsc5hip_psd_stats


SIS_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int,
                          ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint)                                     # nrsc5hip_sis_cb
SIS_KINDS = (None, "station_id", "station_name", "station_slogan", "station_message", "station_location", "audio_service", "data_service", "alert",
             "leap_second", "local_time", "exciter", "importer")                                         # NRSC5HIP_SIS_*
SIS_STATS = (("frames", "crc_good", "sis", "llds") + tuple("id%d" % k for k in range(16)) +
             ("unknown_id", "no_room", "never_complete_message", "never_complete_slogan", "never_complete_alert", "bad_checksum", "bad_crc7",
              "bad_cnt_len", "bad_cnt_crc", "events", "d2h_bytes"))                                       # nrsc5hip_sis_stats
SIS_EVENT_HEADER = 48                    # bytes of an event in the arena in front of its text (padded to 4); the arena header is 16


AAS_EVENT_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(ctypes.c_int32),
                                ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint)                               # nrsc5hip_aas_event_cb
AAS_KINDS = (None, "psd", "sig", "lot_header", "lot_fragment", "lot", "stream", "packet")               # NRSC5HIP_AAS_*
AAS_STATS = ("packets", "psd", "sig_packets", "sig_parsed", "sig_truncated", "sig_zero_length", "sig_empty", "unknown_port", "before_sig", "not_in_sig",
             "stream", "packet", "unknown_type", "lot_packets", "lot_dropped", "lot_short_header", "lot_headers", "lot_resets", "lot_fragments",
             "lot_duplicates", "lot_too_large", "lot_files", "lot_oversize", "lru_evictions", "pool_evictions", "events", "d2h_bytes")   # nrsc5hip_aas_stats
AAS_FRAGMENTS = 1                        # NRSC5HIP_AAS_FRAGMENTS
AAS_EVENT_HEADER = 48                    # bytes of an event in the arena in front of its data (padded to 4); the arena header is 16
AAS_SIG_MAX = 5632                       # NRSC5HIP_AAS_SIG_MAX
AAS_MAX_FILES = 64


class AasEvent(ctypes.Structure):        # an event of k_aas as it lies in the arena
    _fields_ = [("pos", ctypes.c_uint32), ("len", ctypes.c_uint32), ("kind", ctypes.c_uint16), ("port", ctypes.c_uint16), ("seq", ctypes.c_uint32),
                ("v", ctypes.c_int32 * 8)]


assert ctypes.sizeof(AasEvent) == AAS_EVENT_HEADER


class SisInfo(ctypes.Structure):         # nrsc5hip_sis_info
    _fields_ = [("country_code", ctypes.c_char * 4), ("fcc_facility_id", ctypes.c_int32),
                ("name_enc", ctypes.c_int32), ("name_len", ctypes.c_int32), ("name", ctypes.c_uint8 * 16),
                ("slogan_enc", ctypes.c_int32), ("slogan_len", ctypes.c_int32), ("slogan", ctypes.c_uint8 * 96),
                ("message_enc", ctypes.c_int32), ("message_len", ctypes.c_int32), ("message", ctypes.c_uint8 * 192),
                ("alert_enc", ctypes.c_int32), ("alert_len", ctypes.c_int32), ("alert_cnt_len", ctypes.c_int32), ("alert", ctypes.c_uint8 * 384),
                ("have_location", ctypes.c_int32), ("latitude", ctypes.c_int32), ("longitude", ctypes.c_int32), ("altitude", ctypes.c_int32),
                ("n_audio", ctypes.c_int32), ("audio", (ctypes.c_int32 * 4) * 8), ("n_data", ctypes.c_int32), ("data", (ctypes.c_int32 * 3) * 16)]


class AmBlockState(ctypes.Structure):
    """nrsc5hip_am_block_state: the words of StreamState / AmStream that k_am_block reads (nrsc5hip_stage_am_block); the last four are read back only"""
    _fields_ = [(n, ctypes.c_int32) for n in ("sync_state", "samperr", "cfo", "psmi", "bc", "cfo_wait")] + \
               [("prev_angle", ctypes.c_float), ("angle", ctypes.c_float), ("theta", ctypes.c_double),
                ("coarse_samperr", ctypes.c_int32), ("coarse_re", ctypes.c_float), ("coarse_im", ctypes.c_float), ("keep_extra", ctypes.c_int32),
                ("offset_history", ctypes.c_uint32)] + \
               [(n, ctypes.c_int32) for n in ("rdbi", "pli", "hppi", "aabi", "am_diversity_wait")] + [("am_errors", ctypes.c_uint32)] + \
               [(n, ctypes.c_int32) for n in ("fine_epoch", "active", "nblocks")] + [("rd", ctypes.c_longlong)]


assert ctypes.sizeof(AmBlockState) == 104
AM_BLOCK_STATE_IN = tuple(n for n, _ in AmBlockState._fields_[:21])       # what the hook writes into the stream before the launch
AM_SYMS, AM_FFT, AM_NSYM, AM_PW = 6400, 256, 32, 25                          # hard symbols per partition and L1 frame; FFT size; symbols per block; carriers per partition


def bind_am_block(lib) -> None:
    """argument types of the AM block-step stage hook and of the symbol fetch (include/nrsc5hip.h, ABI 18)"""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.nrsc5hip_stage_am_block.argtypes = [vp, vp, vp, ctypes.POINTER(AmBlockState), ci, ci, vp, ctypes.POINTER(AmBlockState), vp, vp, vp, vp]
    lib.nrsc5hip_debug_fetch_am_sym.argtypes = [vp, ci, vp]


class SymStream(ctypes.Structure):
    """nrsc5hip_sym_stream: one stream's samples and block parameters for nrsc5hip_stage_symbols"""
    _fields_ = [("raw", ctypes.c_void_p), ("raw_bytes", ctypes.c_size_t), ("lead", ctypes.c_int32), ("pad0", ctypes.c_int32),
                ("q15", ctypes.c_void_p), ("q15_samples", ctypes.c_longlong), ("nco_tab", ctypes.c_void_p),
                ("a00", ctypes.c_longlong), ("dtheta", ctypes.c_double), ("theta", ctypes.c_double), ("growth", ctypes.c_double),
                ("active", ctypes.c_int32), ("nco_mode", ctypes.c_int32),
                ("samperr", ctypes.c_int32), ("cfo", ctypes.c_int32), ("angle", ctypes.c_float), ("prev_angle", ctypes.c_float),
                ("rd", ctypes.c_longlong), ("wr", ctypes.c_longlong)]


class SymParams(ctypes.Structure):
    """nrsc5hip_sym_params: what the symbol kernel ran on, read back from the stream state"""
    _fields_ = [("a00", ctypes.c_longlong), ("dtheta", ctypes.c_double), ("theta", ctypes.c_double), ("growth", ctypes.c_double),
                ("active", ctypes.c_int32), ("nco_mode", ctypes.c_int32)]


assert ctypes.sizeof(SymStream) == 120 and ctypes.sizeof(SymParams) == 40
SYM_FORMS = (1, 2, 4, 8, 16, 32)         # the mixfft_syms values launch_mixfft knows: symbols per 128-lane workgroup, NPAR = 2, the 256-lane kernel
SYM_NSYM, SYM_LIVE = 32, 534             # symbols per block, live bins per symbol (478 .. 744, 1304 .. 1570 after the shift)


def bind_symbols(lib) -> None:
    """argument types of the symbol-transform stage hook (include/nrsc5hip.h, ABI 20)"""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.nrsc5hip_stage_symbols.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp]


class _RdsConfig(ctypes.Structure):
    """nrsc5hip_rds_config"""
    _fields_ = [("raw_groups", ctypes.c_int), ("correct_burst", ctypes.c_int)]


class RdsInfo(ctypes.Structure):
    """nrsc5hip_rds_info"""
    _fields_ = [(n, ctypes.c_int32) for n in ("pi", "pty", "tp", "ta", "ms", "di", "synced", "ps_len")] + [("ps", ctypes.c_uint8 * 8)] + \
               [("rt_len", ctypes.c_int32), ("rt_ab", ctypes.c_int32), ("rt", ctypes.c_uint8 * 64)] + \
               [(n, ctypes.c_int32) for n in ("have_clock", "mjd", "hour", "minute", "offset_half_hours")]


RDS_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int32),
                          ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint)                                     # nrsc5hip_rds_cb
RDS_KINDS = (None, "pi", "ps", "rt", "clock", "group")                                                  # NRSC5HIP_RDS_*
RDS_STATS = (("bits", "blocks_valid", "blocks_corrected", "blocks_invalid", "groups", "groups_dropped", "syncs_gained", "syncs_lost", "seam_drops",
              "seam_inserts") + tuple("g%d%s" % (t, v) for t in range(16) for v in "AB") + ("events",))      # nrsc5hip_fm_rds_stats
assert len(RDS_STATS) == 43
RDS_BITS_STRIDE = 160                    # bytes per window in what nrsc5hip_stage_rds_mf returns


def bind_rds(lib) -> None:
    """argument types of RDS on the analog FM object (include/nrsc5hip.h, ABI 19)"""
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.nrsc5hip_fm_debug_launches.argtypes = [vp, ctypes.POINTER(ll)]
    lib.nrsc5hip_fm_rds_enable.argtypes = [vp, ctypes.POINTER(_RdsConfig)]
    lib.nrsc5hip_fm_rds_read.argtypes = [vp, RDS_CB, vp]
    lib.nrsc5hip_fm_rds_get.argtypes = [vp, ci, ctypes.POINTER(RdsInfo)]
    lib.nrsc5hip_fm_rds_stats.argtypes = [vp, ci, vp]
    lib.nrsc5hip_fm_rds_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ll)]
    lib.nrsc5hip_fm_rds_taps.argtypes = [vp, vp]
    lib.nrsc5hip_stage_rds_mf.argtypes = [vp, vp, ll, ll, vp, vp, vp, vp, vp]
    lib.nrsc5hip_stage_rds_groups.argtypes = [vp, ci, vp, vp, vp, vp]


class ScanFmStation(ctypes.Structure):
    """nrsc5hip_scan_fm_station"""
    _fields_ = [("offset_hz", ctypes.c_double), ("bin_hz", ctypes.c_double), ("score_db", ctypes.c_float), ("floor_db", ctypes.c_float)]


class FmCarrierReport(ctypes.Structure):
    """nrsc5hip_fm_carrier_report"""
    _fields_ = [(n, ctypes.c_double) for n in ("sum2", "sum4", "sum1", "count", "level_db", "cnr_db", "offset_hz")]


class FmCarrierInfo(ctypes.Structure):
    """nrsc5hip_fm_carrier_info"""
    _fields_ = [("windowed", FmCarrierReport), ("running", FmCarrierReport), ("blocks", ctypes.c_longlong), ("audio_blocks", ctypes.c_longlong)]


assert ctypes.sizeof(FmCarrierInfo) == 128
FM_CARRIER_DB_MIN, FM_CARRIER_DB_MAX = -150.0, 150.0     # NRSC5HIP_FM_CARRIER_DB_MIN / _MAX


def bind_carrier(lib) -> None:
    """argument types of the carrier measurement and of the analog-carrier detector (include/nrsc5hip.h, ABI 21)"""
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.nrsc5hip_abi_version.restype = ci
    if lib.nrsc5hip_abi_version() < 21:                    # an older library loaded for an A/B comparison: it has everything but these
        return
    lib.nrsc5hip_fm_carrier_enable.argtypes = [vp]
    lib.nrsc5hip_fm_carrier.argtypes = [vp, vp]
    lib.nrsc5hip_stage_fm_carrier.argtypes = [vp, vp, ll, ll, vp, vp]
    lib.nrsc5hip_scan_detect_fm_psd.argtypes = [vp, ci, ctypes.c_double, ctypes.POINTER(ScanParams), vp, ci, ctypes.POINTER(ci)]
    lib.nrsc5hip_scan_detect_fm.argtypes = [vp, ctypes.POINTER(ScanParams), vp, ci, ctypes.POINTER(ci)]


FM_STEER_BLEND, FM_STEER_HIGHCUT, FM_STEER_MUTE, FM_STEER_ALL = 1, 2, 4, 7      # NRSC5HIP_FM_STEER_*
FM_STEER_CONTROLS = {"blend": FM_STEER_BLEND, "highcut": FM_STEER_HIGHCUT, "mute": FM_STEER_MUTE}
FM_STEER_DEFAULTS = dict(blend_db=(18.0, 30.0), highcut_db=(10.0, 20.0), mute_db=(2.0, 8.0), mute_floor_db=-20.0, controls=FM_STEER_ALL)


class _FmSteerConfig(ctypes.Structure):
    """nrsc5hip_fm_steer_config"""
    _fields_ = [("controls", ctypes.c_uint), ("blend_db", ctypes.c_double * 2), ("highcut_db", ctypes.c_double * 2), ("mute_db", ctypes.c_double * 2),
                ("mute_floor_db", ctypes.c_double)]


def bind_steer(lib) -> None:
    """argument types of reception steering on the analog FM object (include/nrsc5hip.h, ABI 22)"""
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    lib.nrsc5hip_abi_version.restype = ctypes.c_int
    if lib.nrsc5hip_abi_version() < 22:                    # an older library loaded for an A/B comparison: it has everything but these
        return
    lib.nrsc5hip_fm_steer_enable.argtypes = [vp, ctypes.POINTER(_FmSteerConfig)]
    lib.nrsc5hip_fm_steer.argtypes = [vp, vp]
    lib.nrsc5hip_fm_steer_taps.argtypes = [vp, vp]
    lib.nrsc5hip_stage_fm_steer.argtypes = [vp, vp, ll, ll, vp]


class _SameConfig(ctypes.Structure):
    """nrsc5hip_same_config"""
    _fields_ = [("burst_events", ctypes.c_int)]


class SameInfo(ctypes.Structure):
    """nrsc5hip_same_info"""
    _fields_ = [("text_len", ctypes.c_int32), ("kind", ctypes.c_int32), ("first_bit", ctypes.c_longlong), ("last_bit", ctypes.c_longlong),
                ("group_bursts", ctypes.c_int32), ("group_kind", ctypes.c_int32), ("in_message", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("text", ctypes.c_uint8 * 272)]


assert ctypes.sizeof(SameInfo) == 312
SAME_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int32),
                           ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint)                                    # nrsc5hip_same_cb
SAME_KINDS = (None, "burst", "message")                                                                 # NRSC5HIP_SAME_BURST / _MESSAGE
SAME_BURST_KINDS = (None, "header", "eom")                                                              # NRSC5HIP_SAME_HEADER / _EOM
SAME_STATS = ("bits", "preambles", "bursts", "bursts_aborted", "messages", "groups_no_message", "eom_messages", "seam_drops", "seam_inserts",
              "events")                                                                                  # nrsc5hip_fm_same_stats
SAME_TABLE, SAME_GRID, SAME_WIN_PTS, SAME_BITS_STRIDE, SAME_TEXT_MAX = 35721, 400, 512, 72, 268


def same_segments(n_in: int) -> int:
    """segments of the SAME grid that lie inside n_in input samples (nrsc5hip_stage_same_tones)"""
    return (SAME_GRID * ((n_in + 1) // 2 + 1) - 1) // SAME_TABLE


def bind_same(lib) -> None:
    """argument types of EAS alerts (SAME) on the analog FM object (include/nrsc5hip.h, ABI 23)"""
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.nrsc5hip_abi_version.restype = ci
    if lib.nrsc5hip_abi_version() < 23:                    # an older library loaded for an A/B comparison: it has everything but these
        return
    lib.nrsc5hip_fm_same_enable.argtypes = [vp, ctypes.POINTER(_SameConfig)]
    lib.nrsc5hip_fm_same_read.argtypes = [vp, SAME_CB, vp]
    lib.nrsc5hip_fm_same_get.argtypes = [vp, ci, ctypes.POINTER(SameInfo)]
    lib.nrsc5hip_fm_same_stats.argtypes = [vp, ci, vp]
    lib.nrsc5hip_fm_same_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ll)]
    lib.nrsc5hip_fm_same_table.argtypes = [vp, vp]
    lib.nrsc5hip_stage_same_tones.argtypes = [vp, vp, ll, ll, vp, vp, vp, vp, vp, vp]
    lib.nrsc5hip_stage_same_frames.argtypes = [vp, ci, vp, vp, vp, vp]


FM_IMPAIR_MULTIPATH, FM_IMPAIR_ADJACENT = 1, 2            # NRSC5HIP_FM_IMPAIR_*
FM_IMPAIR_TAPS, FM_IMPAIR_NSUMS = 63, 11
FM_IMPAIR_SUMS = ("sx", "sxx", "sxxx", "sxxxx", "sy", "sxy", "sxxy", "syy", "cee", "cdd", "ced")
FM_IMPAIR_FIGURES = ("explained", "depth", "slope", "curvature", "usn_db", "ripple_db", "rho")
FM_IMPAIR_DEFAULTS = dict(explained_min=0.5, depth_min=0.05, rho_min=0.5)


class _FmImpairConfig(ctypes.Structure):
    """nrsc5hip_fm_impair_config"""
    _fields_ = [("explained_min", ctypes.c_double), ("depth_min", ctypes.c_double), ("rho_min", ctypes.c_double)]


class FmImpairReport(ctypes.Structure):
    """nrsc5hip_fm_impair_report"""
    _fields_ = [(n, ctypes.c_double) for n in FM_IMPAIR_SUMS + ("count",) + FM_IMPAIR_FIGURES] + [("verdict", ctypes.c_int32), ("side", ctypes.c_int32)]


class FmImpairInfo(ctypes.Structure):
    """nrsc5hip_fm_impair_info"""
    _fields_ = [("windowed", FmImpairReport), ("running", FmImpairReport), ("blocks", ctypes.c_longlong), ("audio_blocks", ctypes.c_longlong)]


assert ctypes.sizeof(FmImpairInfo) == 336


def bind_impair(lib) -> None:
    """argument types of the reception impairments of the analog FM object (include/nrsc5hip.h, ABI 24)"""
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    lib.nrsc5hip_abi_version.restype = ctypes.c_int
    if lib.nrsc5hip_abi_version() < 24:                    # an older library loaded for an A/B comparison: it has everything but these
        return
    lib.nrsc5hip_fm_impair_enable.argtypes = [vp, ctypes.POINTER(_FmImpairConfig)]
    lib.nrsc5hip_fm_impair.argtypes = [vp, vp]
    lib.nrsc5hip_fm_impair_taps.argtypes = [vp, vp]
    lib.nrsc5hip_stage_fm_impair.argtypes = [vp, vp, ll, ll, vp, vp, vp, vp]


class Nrsc5HipError(RuntimeError):
    pass
