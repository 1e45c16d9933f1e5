"""ctypes binding of the C ABI (include/gnuais_hip.h -> gnuais_amd/libgnuais_hip.so).

There is no fallback: if the HIP library has not been built, or no HIP device
is usable, importing or calling raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgnuais_hip.so")

OK, E_ARG, E_HIP, E_OVERFLOW, E_STATE = 0, -1, -2, -3, -4

FRAME_DTYPE = np.dtype([("channel", "<u4"), ("end_bit", "<u4"), ("payload", "u1", (53,)),
                        ("flags", "u1"), ("nbits", "<u2")])
COUNTERS_DTYPE = np.dtype([("receivedframes", "<i4"), ("lostframes", "<i4"), ("lostframes2", "<i4")])
PLL_DTYPE = np.dtype([("pll", "<u4"), ("prev", "<i4"), ("lastbit", "<i4")])
FSM_DTYPE = np.dtype([("state", "<i4"), ("nstartsign", "<i4"), ("antallpreamble", "<i4"),
                      ("antallenner", "<i4"), ("bitstuff", "<i4"), ("last", "<i4"),
                      ("bufferpos", "<i4")])
assert FRAME_DTYPE.itemsize == 64
# struct gnuais_frame_signal: a frame's power (full scale 2^31), carrier error and blocks measured (0: no measurement)
SIGNAL_DTYPE = np.dtype([("power", "<u4"), ("ferr", "<i2"), ("blocks", "<u2")])
assert SIGNAL_DTYPE.itemsize == 8
# gnuais_hearer: one member of a cluster of gnuais_batch_drain_frames_heard()
HEARER_DTYPE = np.dtype([("channel", "<u4"), ("flags", "<u4"), ("t", "<i8"), ("signal", SIGNAL_DTYPE)])
assert HEARER_DTYPE.itemsize == 24
# struct gnuais_occupancy: a channel's epoch: the floor's code, busy and covered blocks, bursts
OCCUPANCY_DTYPE = np.dtype([("floor", "<u2"), ("busy", "<u2"), ("covered", "<u2"), ("bursts", "<u2")])
assert OCCUPANCY_DTYPE.itemsize == 8
OCCUPANCY_EPOCHS_HELD = 64    # final epochs the library keeps for gnuais_batch_drain_occupancy
# struct gnuais_long_frame: a message of three to five slots (gnuais_batch_long_frames)
LONG_FRAME_DTYPE = np.dtype([("channel", "<u4"), ("end_bit", "<u4"), ("t", "<i8"), ("nbits", "<u2"), ("flags", "u1"),
                             ("reserved", "u1"), ("payload", "u1", (132,))])
assert LONG_FRAME_DTYPE.itemsize == 152
LONG_MAX_BITS = 1008         # GNUAIS_LONG_MAX_BITS
FRAME_REPAIRED = 0x40        # GNUAIS_FRAME_REPAIRED: frame flags bit 6

# kinds of input for gnuais_batch_time_map (GNUAIS_INPUT_* in include/gnuais_hip.h)
INPUT_KINDS = {"audio": 0, "iq": 1, "wideband": 2}

# sample formats of wideband input (GNUAIS_FMT_* in include/gnuais_hip.h): value, and the dtype of an [len][M][2] array
FMT_CS16, FMT_CU8, FMT_CS8, FMT_CF32 = 0, 1, 2, 3
FORMATS = {"cs16": (FMT_CS16, np.dtype("<i2")), "cu8": (FMT_CU8, np.dtype("u1")), "cs8": (FMT_CS8, np.dtype("i1")),
           "cf32": (FMT_CF32, np.dtype("<f4"))}

# every symbol include/gnuais_hip.h declares: (restype, argtypes)
_P, _I, _U = C.c_void_p, C.c_int, C.c_uint
SYMBOLS = {
    "gnuais_batch_create": (_I, [C.POINTER(_P), _I, _I, _P, _I, _U, _I, _I]),
    "gnuais_batch_destroy": (None, [_P]),
    "gnuais_batch_reset": (_I, [_P]),
    "gnuais_batch_set_clock": (_I, [_P, C.c_longlong, _P]),
    "gnuais_batch_run": (_I, [_P, _P, _I, _P]),
    "gnuais_batch_run_host": (_I, [_P, _P, _I]),
    "gnuais_batch_run_host_async": (_I, [_P, _P, _I]),
    "gnuais_batch_run_iq": (_I, [_P, _P, _I, _P]),
    "gnuais_batch_run_iq_host": (_I, [_P, _P, _I]),
    "gnuais_batch_discriminate": (_I, [_P, _P, _I, _P, _P]),
    "gnuais_batch_afc": (_I, [_P, _I]),
    "gnuais_batch_afc_estimate": (_I, [_P, _P]),
    "gnuais_batch_afc_apply": (_I, [_P, _P, _I, _P, _P]),
    "gnuais_batch_channeliser": (_I, [_P, _I, _I, _P, _I, _P, _I]),
    "gnuais_batch_resampler": (_I, [_P, _I, _I, _I, _P, _I, _P, _I]),
    "gnuais_resampler_default_taps": (_I, [_I, _I, _P, _I, C.POINTER(_I)]),
    "gnuais_resampler_plan": (_I, [_I, _I, _P, _I, _P, _I, _P, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "gnuais_batch_run_wideband": (_I, [_P, _P, _I, _P]),
    "gnuais_batch_run_wideband_host": (_I, [_P, _P, _I]),
    "gnuais_batch_channelise": (_I, [_P, _P, _I, _P, _P]),
    "gnuais_batch_run_wideband_fmt": (_I, [_P, _I, _P, _I, _P]),
    "gnuais_batch_run_wideband_fmt_host": (_I, [_P, _I, _P, _I]),
    "gnuais_batch_channelise_fmt": (_I, [_P, _I, _P, _I, _P, _P]),
    "gnuais_sample_format_bytes": (_I, [_I]),
    "gnuais_convert_samples": (_I, [_I, _P, C.c_size_t, _P]),
    "gnuais_channeliser_default_taps": (_I, [_I, _P, _I, C.POINTER(_I)]),
    "gnuais_channeliser_mixer_table": (_I, [_I, _I, _P, _I, C.POINTER(_I)]),
    "gnuais_wav_open": (_I, [C.POINTER(_P), C.c_char_p, _I]),
    "gnuais_wav_channels": (_I, [_P]),
    "gnuais_wav_rate": (_I, [_P]),
    "gnuais_wav_read": (C.c_long, [_P, _P, C.c_long]),
    "gnuais_wav_close": (None, [_P]),
    "gnuais_batch_sync": (_I, [_P]),
    "gnuais_batch_filter": (_I, [_P, _P, _I, _P, _P]),
    "gnuais_batch_filter_host": (_I, [_P, _P, _I, _P]),
    "gnuais_batch_decode_bits": (_I, [_P, _P, _I, _P]),
    "gnuais_batch_last_bits": (_I, [_P, _P, _I, _P]),
    "gnuais_batch_last_signs": (_I, [_P, _P, _I]),
    "gnuais_batch_info": (_I, [_P, C.c_char_p, C.POINTER(C.c_double)]),
    "gnuais_batch_drain_frames": (_I, [_P, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_pending_frames": (_I, [_P, C.POINTER(_I)]),
    "gnuais_batch_frame_times": (_I, [_P, _I]),
    "gnuais_batch_drain_frames_timed": (_I, [_P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_frame_signal": (_I, [_P, _I]),
    "gnuais_batch_drain_frames_signal": (_I, [_P, _P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_signal_blocks": (_I, [_P, C.c_longlong, _I, _P]),
    "gnuais_frame_signal_span": (_I, [C.c_longlong, _I, _U, _I, _I, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(_I)]),
    "gnuais_batch_occupancy": (_I, [_P, _I, _I]),
    "gnuais_batch_drain_occupancy": (_I, [_P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_occupancy_lost": (_I, [_P, C.POINTER(C.c_longlong)]),
    "gnuais_batch_occupancy_blocks": (_I, [_P, C.c_longlong, _I, _P]),
    "gnuais_occupancy_code": (_I, [C.c_longlong, C.POINTER(_I)]),
    "gnuais_occupancy_power": (_I, [_I, C.POINTER(C.c_longlong)]),
    "gnuais_occupancy_cover_span": (_I, [C.c_longlong, _I, _U, _I, _I, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(_I)]),
    "gnuais_batch_time_map": (_I, [_P, _I, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "gnuais_batch_time_map_ratio": (_I, [_P, _I, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "gnuais_nmea_tagged_from_frames": (_I, [_P, _P, _I, _P, _I, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong,
                                            _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_I)]),
    "gnuais_batch_repair": (_I, [_P, _I]),
    "gnuais_batch_repaired": (_I, [_P, _P]),
    "gnuais_repair_candidate": (_I, [_P, _I, _P, C.POINTER(_I), C.POINTER(_I)]),
    "gnuais_batch_long_frames": (_I, [_P, _I]),
    "gnuais_batch_pending_long_frames": (_I, [_P, C.POINTER(_I)]),
    "gnuais_batch_drain_long_frames": (_I, [_P, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_long_counters": (_I, [_P, _P, _P]),
    "gnuais_batch_long_fsm_state": (_I, [_P, _P]),
    "gnuais_nmea_from_long_frames": (_I, [_P, _I, _P, _I, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_I)]),
    "gnuais_batch_long_repair": (_I, [_P, _I]),
    "gnuais_batch_long_repaired": (_I, [_P, _P]),
    "gnuais_long_repair_candidate": (_I, [_P, _I, _P, C.POINTER(_I), C.POINTER(_I)]),
    "gnuais_batch_unique": (_I, [_P, _I]),
    "gnuais_batch_drain_frames_unique": (_I, [_P, _P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_unique_late": (_I, [_P, C.POINTER(C.c_longlong)]),
    "gnuais_uniq_create": (_I, [C.POINTER(_P), C.c_longlong]),
    "gnuais_uniq_destroy": (None, [_P]),
    "gnuais_uniq_reset": (_I, [_P]),
    "gnuais_uniq_push": (_I, [_P, _P, _P, _I, C.c_longlong, _P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_uniq_late": (C.c_longlong, [_P]),
    "gnuais_batch_drain_frames_heard": (_I, [_P, _P, _P, _P, _I, C.POINTER(_I), _P, _P, C.POINTER(_I)]),
    "gnuais_uniq_push_heard": (_I, [_P, _P, _P, _P, _I, C.c_longlong, _P, _P, _P, _I, C.POINTER(_I), _P, _P, C.POINTER(_I)]),
    "gnuais_batch_long_unique": (_I, [_P, _I]),
    "gnuais_batch_drain_long_frames_unique": (_I, [_P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_drain_long_frames_heard": (_I, [_P, _P, _P, _I, C.POINTER(_I), _P, _P, C.POINTER(_I)]),
    "gnuais_batch_long_unique_late": (_I, [_P, C.POINTER(C.c_longlong)]),
    "gnuais_long_uniq_create": (_I, [C.POINTER(_P), C.c_longlong]),
    "gnuais_long_uniq_destroy": (None, [_P]),
    "gnuais_long_uniq_reset": (_I, [_P]),
    "gnuais_long_uniq_push": (_I, [_P, _P, _I, C.c_longlong, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_long_uniq_push_heard": (_I, [_P, _P, _I, C.c_longlong, _P, _P, _I, C.POINTER(_I), _P, _P, C.POINTER(_I)]),
    "gnuais_long_uniq_push_heard_signal": (_I, [_P, _P, _P, _I, C.c_longlong, _P, _P, _I, C.POINTER(_I), _P, _P, C.POINTER(_I)]),
    "gnuais_long_uniq_late": (C.c_longlong, [_P]),
    "gnuais_batch_long_frame_signal": (_I, [_P, _I]),
    "gnuais_batch_drain_long_frames_signal": (_I, [_P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_discard_frames": (_I, [_P, _P]),
    "gnuais_batch_counters": (_I, [_P, _P]),
    "gnuais_batch_total_received": (_I, [_P, C.POINTER(C.c_longlong)]),
    "gnuais_batch_maxval": (_I, [_P, _P]),
    "gnuais_batch_pll_state": (_I, [_P, _P]),
    "gnuais_batch_fsm_state": (_I, [_P, _P]),
    "gnuais_batch_protodec_reset": (_I, [_P]),
    "gnuais_batch_frame_bits": (_I, [_P, _I, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_history": (_I, [_P, _P]),
    "gnuais_batch_n_channels": (_I, [_P]),
    "gnuais_batch_n_taps": (_I, [_P]),
    "gnuais_default_taps": (_I, [_P]),
    "gnuais_crc16_batch": (_I, [_I, _P, _I, _P, _I, _P]),
    "gnuais_crc16_bits": (_I, [_I, _P, _I, _P, _P, _I]),
    "gnuais_nmea_from_frames": (_I, [_P, _I, _P, _I, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_I)]),
    "gnuais_messages_from_frames": (_I, [_P, _I, _P, _P, _I, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_I),
                                         _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_I)]),
    "gnuais_batch_drain_nmea": (_I, [_P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_I), C.POINTER(_I)]),
    "gnuais_batch_drain_messages": (_I, [_P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_I), _P, C.c_size_t,
                                         C.POINTER(C.c_size_t), C.POINTER(_I), C.POINTER(_I)]),
    "gnuais_batch_fold_vessels": (_I, [_P, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_vessel_table_enable": (_I, [_P, _I]),
    "gnuais_batch_vessel_table_update": (_I, [_P]),
    "gnuais_batch_vessel_table": (_I, [_P, _P, _I, C.POINTER(_I)]),
    "gnuais_batch_vessel_table_clear": (_I, [_P]),
    "gnuais_batch_stream_nmea": (_I, [_P, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(_I), C.POINTER(_I)]),
    "gnuais_batch_drain_frames_nmea": (_I, [_P, _P, _I, C.POINTER(_I), _P, _P, C.c_size_t, C.POINTER(C.c_size_t),
                                            C.POINTER(_I)]),
    "gnuais_range_from_frames": (_I, [_P, _I, _I, C.c_float, C.c_float, _P]),
    "gnuais_vessels_from_frames": (_I, [_P, _I, _P, _I, C.POINTER(_I)]),
    "gnuais_sql_plan_from_frames": (_I, [_P, _I, _P, _I, C.POINTER(_I)]),
    "gnuais_sql_calls_from_frames": (_I, [_P, _I, _I, _P, _I, C.POINTER(_I)]),
    "gnuais_tile_channels": (_I, [_P, _I, _I, _P, _I, _P]),
    "gnuais_batch_set_timing": (_I, [_P, _I]),
    "gnuais_batch_last_timing": (_I, [_P, _P]),
    "gnuais_batch_mean_timing": (_I, [_P, _P, C.POINTER(_I)]),
    "gnuais_batch_autotune": (_I, [_P, _P, _I, _P, C.POINTER(C.c_float)]),
    "gnuais_batch_autotune_delivery": (_I, [_P, _P, _I, _P, C.POINTER(C.c_float)]),
    "gnuais_batch_set_option": (_I, [_P, C.c_char_p, _I]),
    "gnuais_node_create": (_I, [C.POINTER(_P), _P, _I, _I, _P, _I, _U, _I, _I]),
    "gnuais_node_destroy": (None, [_P]),
    "gnuais_node_reset": (_I, [_P]),
    "gnuais_node_n_devices": (_I, [_P]),
    "gnuais_node_n_channels": (_I, [_P]),
    "gnuais_node_shard": (_I, [_P, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_P)]),
    "gnuais_node_run_host": (_I, [_P, _P, _I]),
    "gnuais_node_run": (_I, [_P, _P, _I, _P]),
    "gnuais_node_run_iq_host": (_I, [_P, _P, _I]),
    "gnuais_node_run_iq": (_I, [_P, _P, _I, _P]),
    "gnuais_node_channeliser": (_I, [_P, _I, _I, _P, _I, _P, _I]),
    "gnuais_node_resampler": (_I, [_P, _I, _I, _I, _P, _I, _P, _I]),
    "gnuais_node_run_wideband_host": (_I, [_P, _P, _I]),
    "gnuais_node_run_wideband_fmt_host": (_I, [_P, _I, _P, _I]),
    "gnuais_node_afc": (_I, [_P, _I]),
    "gnuais_node_sync": (_I, [_P]),
    "gnuais_node_pending_frames": (_I, [_P, C.POINTER(_I)]),
    "gnuais_node_drain_frames": (_I, [_P, _P, _I, C.POINTER(_I)]),
    "gnuais_node_frame_times": (_I, [_P, _I]),
    "gnuais_node_drain_frames_timed": (_I, [_P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_node_frame_signal": (_I, [_P, _I]),
    "gnuais_node_drain_frames_signal": (_I, [_P, _P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_node_occupancy": (_I, [_P, _I, _I]),
    "gnuais_node_drain_occupancy": (_I, [_P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_node_repair": (_I, [_P, _I]),
    "gnuais_node_repaired": (_I, [_P, _P]),
    "gnuais_node_long_frames": (_I, [_P, _I]),
    "gnuais_node_drain_long_frames": (_I, [_P, _P, _I, C.POINTER(_I)]),
    "gnuais_node_long_frame_signal": (_I, [_P, _I]),
    "gnuais_node_drain_long_frames_signal": (_I, [_P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_node_long_counters": (_I, [_P, _P, _P]),
    "gnuais_node_long_repair": (_I, [_P, _I]),
    "gnuais_node_long_repaired": (_I, [_P, _P]),
    "gnuais_node_unique": (_I, [_P, _I]),
    "gnuais_node_drain_frames_unique": (_I, [_P, _P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_node_unique_late": (_I, [_P, C.POINTER(C.c_longlong)]),
    "gnuais_node_drain_frames_heard": (_I, [_P, _P, _P, _P, _I, C.POINTER(_I), _P, _P, C.POINTER(_I)]),
    "gnuais_node_long_unique": (_I, [_P, _I]),
    "gnuais_node_drain_long_frames_unique": (_I, [_P, _P, _P, _I, C.POINTER(_I)]),
    "gnuais_node_drain_long_frames_heard": (_I, [_P, _P, _P, _I, C.POINTER(_I), _P, _P, C.POINTER(_I)]),
    "gnuais_node_long_unique_late": (_I, [_P, C.POINTER(C.c_longlong)]),
    "gnuais_node_stream_nmea": (_I, [_P, _P, _P, C.POINTER(_I), C.POINTER(_I)]),
    "gnuais_node_discard_frames": (_I, [_P]),
    "gnuais_node_counters": (_I, [_P, _P]),
    "gnuais_node_total_received": (_I, [_P, C.POINTER(C.c_longlong)]),
    "gnuais_node_maxval": (_I, [_P, _P]),
    "gnuais_node_pll_state": (_I, [_P, _P]),
    "gnuais_node_set_option": (_I, [_P, C.c_char_p, _I]),
    "gnuais_node_autotune": (_I, [_P, _P, _I, _P, C.POINTER(C.c_float)]),
    "gnuais_node_last_error": (C.c_char_p, []),
    "gnuais_node_warnings": (C.c_char_p, [_P]),
    "gnuais_node_mark": (_I, [_P]),
    "gnuais_node_shard_stats": (_I, [_P, _I, _P]),
    "gnuais_last_error": (C.c_char_p, []),
    "gnuais_version": (C.c_char_p, []),
}


class GnuaisError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"gnuais_hip error {code}: {msg}")
        self.code = code


_LIB = None


def load() -> C.CDLL:
    """dlopen the in-tree HIP library and bind every declared symbol."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C gnuais_amd/csrc` "
                "(or __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)          # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def check(rc: int, allow=()) -> int:
    if rc != OK and rc not in allow:
        raise GnuaisError(rc, load().gnuais_last_error().decode())
    return rc


def signal_dbfs(power) -> np.ndarray:
    """gnuais_frame_signal.power -> dB relative to full scale (2^31 = a pair of -32768s); -inf where it is 0"""
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(power, dtype=np.float64) / 2.0 ** 31)


def signal_hz(ferr, rate) -> np.ndarray:
    """gnuais_frame_signal.ferr -> Hz at `rate` chain rows per second"""
    return np.asarray(ferr, dtype=np.float64) * float(rate) / 65536.0


def frame_signal_span(t: int, nbits: int, pllinc: int, n_taps: int = 36, afc_window: int = 0, v0: int = 0):
    """gnuais_frame_signal_span(): (j_lo, nb), the whole blocks of 64 rows under a frame; (0, 0): no record"""
    j_lo, nb = C.c_longlong(0), C.c_int(0)
    check(load().gnuais_frame_signal_span(int(t), int(nbits), int(pllinc), int(n_taps), int(afc_window), int(v0),
                                          C.byref(j_lo), C.byref(nb)))
    return j_lo.value, nb.value


def occupancy_code(P: int) -> int:
    """gnuais_occupancy_code(): the code of a block's sum P (eight steps per octave), 0 <= P < 2^38"""
    code = C.c_int(0)
    check(load().gnuais_occupancy_code(int(P), C.byref(code)))
    return code.value


def occupancy_power(code: int) -> int:
    """gnuais_occupancy_power(): the lower edge of a code's bin, a block's sum"""
    P = C.c_longlong(0)
    check(load().gnuais_occupancy_power(int(code), C.byref(P)))
    return P.value


def occupancy_cover_span(t: int, nbits: int, pllinc: int, n_taps: int = 36, afc_window: int = 0, v0: int = 0):
    """gnuais_occupancy_cover_span(): (j_lo, nb), the blocks of 64 rows a frame's cover span intersects; (0, 0): none"""
    j_lo, nb = C.c_longlong(0), C.c_int(0)
    check(load().gnuais_occupancy_cover_span(int(t), int(nbits), int(pllinc), int(n_taps), int(afc_window), int(v0),
                                             C.byref(j_lo), C.byref(nb)))
    return j_lo.value, nb.value


def _bin_edge(code) -> np.ndarray:
    """power(code) of the definition on an array of codes, as float64"""
    c = np.asarray(code, dtype=np.int64)
    return np.where(c < 8, c, (8 + (c & 7)) * 2.0 ** (np.maximum(c, 8) // 8 - 1)).astype(np.float64)


def floor_dbfs(code) -> np.ndarray:
    """gnuais_occupancy.floor -> dB relative to full scale: 10 log10(power(code) / 64 / 2^31); -inf for code 0"""
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(_bin_edge(code) / 64.0 / 2.0 ** 31)


def snr_db(power, floor_code) -> np.ndarray:
    """a frame record's power (gnuais_frame_signal.power) against its epoch's floor (gnuais_occupancy.floor), in dB"""
    return signal_dbfs(power) - floor_dbfs(floor_code)


def default_taps() -> np.ndarray:
    t = np.zeros(36, dtype=np.float32)
    n = load().gnuais_default_taps(t.ctypes.data)
    assert n == 36
    return t
