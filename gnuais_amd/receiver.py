"""Host-side mirror of the reference receiver interface over the HIP batch.

The reference creates one `struct receiver` per audio channel with
init_receiver(name, num_ch, ch_ofs, ...) (src/receiver.c:52-74) and calls
receiver_run(rx, buf, len) once per channel on the same interleaved buffer
(src/ais.c:237-247).  `ReceiverBatch` is those N receivers at once: the same
buffer layout, the same carried state, the same counters, one launch.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import lib as _lib
from .lib import (COUNTERS_DTYPE, E_OVERFLOW, FRAME_DTYPE, FSM_DTYPE, LONG_FRAME_DTYPE, OK, PLL_DTYPE, GnuaisError,
                  check)


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class ReceiverBatch:
    """N independent AIS receivers on one MI355X.

    n_channels  -- num_ch of the interleaved input (receiver.c:102,107)
    taps/pllinc -- filter_init() table and rx->pllinc; None/0 = reference values
    max_len     -- largest len (frames per channel) of one run() call
    """

    def __init__(self, n_channels: int, taps=None, pllinc: int = 0, max_len: int = 48000,
                 device: int = 0, frame_capacity: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        t = None if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
        check(self._lib.gnuais_batch_create(C.byref(self._h), device, n_channels,
                                            None if t is None else t.ctypes.data,
                                            0 if t is None else int(t.size), pllinc, max_len,
                                            frame_capacity))
        self.n_channels = n_channels
        self.n_taps = self._lib.gnuais_batch_n_taps(self._h)
        self.on_overflow = "raise"        # stream_nmea(): "keep" returns an overflowed slot's text and counts it
        self.stream_overflows = 0
        self.max_len = max_len
        self.device = device

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.gnuais_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def reset(self):
        check(self._lib.gnuais_batch_reset(self._h))

    def set_clock(self, rows: int, bits=None):
        """gnuais_batch_set_clock(): the batch continues as if reset() had happened at chain row `rows` with bits[c] bits
        already fed to channel c's deframer (a scalar stands for every channel, None for 0).  Only before the first run
        or decode call since create / reset, and not with a wide stage or the AFC configured."""
        if bits is None:
            check(self._lib.gnuais_batch_set_clock(self._h, int(rows), None))
            return
        b = np.array(np.broadcast_to(np.asarray(bits, dtype=np.uint64), (self.n_channels,)), dtype=np.uint64)
        check(self._lib.gnuais_batch_set_clock(self._h, int(rows), b.ctypes.data))

    def set_option(self, name: str, value: int):
        check(self._lib.gnuais_batch_set_option(self._h, name.encode(), int(value)))

    # -- receiver_run() -------------------------------------------------------
    def run(self, samples, stream: Optional[int] = None, sync: bool = True):
        """samples: interleaved int16 [len][n_channels]; a CUDA/HIP torch tensor
        (used in place, asynchronous on `stream` or torch's current stream) or a
        numpy array (copied host->device, synchronous)."""
        self._run(samples, stream, sync, lambda x: x.ndim == 2 and x.shape[1] == self.n_channels,
                  self._lib.gnuais_batch_run, self._lib.gnuais_batch_run_host)

    def run_iq(self, samples, stream: Optional[int] = None, sync: bool = True):
        """Complex baseband in (gnuais_batch_run_iq): samples int16 [len][n_channels][2] = (I, Q) pairs; the
        discriminator defined in include/gnuais_hip.h turns them into the audio run() takes, on the device.  A CUDA/HIP
        torch tensor is used in place, asynchronously on `stream` or torch's current stream; a numpy array goes through
        gnuais_batch_run_iq_host (copy, run, sync)."""
        self._run(samples, stream, sync, lambda x: x.ndim == 3 and x.shape[1] == self.n_channels and x.shape[2] == 2,
                  self._lib.gnuais_batch_run_iq, self._lib.gnuais_batch_run_iq_host)

    def _run(self, samples, stream, sync, shape_ok, run, run_host):
        """run / run_iq / run_wideband: `run` on a CUDA/HIP torch tensor in place, else `run_host` on a host copy"""
        if _is_torch(samples):
            import torch
            assert samples.is_cuda and samples.dtype == torch.int16 and samples.is_contiguous()
            assert shape_ok(samples)
            if stream is None:
                stream = torch.cuda.current_stream(samples.device).cuda_stream
            check(run(self._h, samples.data_ptr(), int(samples.shape[0]), C.c_void_p(stream)))
            if sync:
                self.sync()
        else:
            x = np.ascontiguousarray(samples, dtype=np.int16)
            assert shape_ok(x)
            check(run_host(self._h, x.ctypes.data, int(x.shape[0])))

    def discriminate(self, samples):
        """The discriminator alone (gnuais_batch_discriminate): int16 [len][n_channels][2] -> torch int16
        [len][n_channels] on the device; advances the I/Q carry and nothing else."""
        return self._stage(samples, lambda x: x.ndim == 3 and x.shape[1] == self.n_channels and x.shape[2] == 2,
                           lambda n: (n, self.n_channels), self._lib.gnuais_batch_discriminate)

    def _stage(self, samples, shape_ok, out_shape, fn):
        """discriminate / channelise: `fn` alone on the device, into a new tensor of out_shape(len); synchronous"""
        import torch
        if not _is_torch(samples):
            samples = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int16)).to(f"cuda:{self.device}")
        assert samples.is_cuda and samples.dtype == torch.int16 and samples.is_contiguous()
        assert shape_ok(samples)
        out = torch.empty(out_shape(int(samples.shape[0])), dtype=torch.int16, device=samples.device)
        stream = torch.cuda.current_stream(samples.device)
        check(fn(self._h, samples.data_ptr(), int(samples.shape[0]), out.data_ptr(), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        return out

    def afc(self, window: int):
        """Carrier-error correction of I/Q input (gnuais_batch_afc, defined in include/gnuais_hip.h): window = 0 switches
        it off (the default), else the estimator's window in samples (a multiple of 128, 128 .. 16384; 2048 suits 48 kHz,
        8192 192 kHz).  From then on run_iq / run_wideband subtract each channel's estimated carrier error before the
        chain, which sees the audio W/2 samples late.  Clears the AFC state."""
        check(self._lib.gnuais_batch_afc(self._h, int(window)))

    def afc_estimate(self) -> np.ndarray:
        """int16 [n_channels]: each channel's carrier-error estimate at the last output row, in discriminator units
        (Hz = e * rate / 65536); zeros before there is an output row."""
        out = np.zeros(self.n_channels, dtype=np.int16)
        check(self._lib.gnuais_batch_afc_estimate(self._h, out.ctypes.data))
        return out

    def afc_apply(self, samples):
        """Discriminator and AFC alone (gnuais_batch_afc_apply): int16 [len][n_channels][2] -> torch int16
        [len][n_channels] on the device, the audio the chain would see; advances the I/Q carry and the AFC state."""
        return self._stage(samples, lambda x: x.ndim == 3 and x.shape[1] == self.n_channels and x.shape[2] == 2,
                           lambda n: (n, self.n_channels), self._lib.gnuais_batch_afc_apply)

    def _wide_configure(self, fn, ratio, in_rate_hz, offsets_hz, taps):
        """channeliser() / resampler(): the library entry `fn` with its ratio arguments, then the rate, offsets and taps"""
        off = np.ascontiguousarray(offsets_hz, dtype=np.int32)
        assert off.ndim == 1 and off.size >= 1
        t = None if taps is None else np.ascontiguousarray(taps, dtype=np.int16)
        check(fn(self._h, *ratio, int(in_rate_hz), off.ctypes.data, int(off.size),
                 None if t is None else t.ctypes.data, 0 if t is None else int(t.size)))
        self._chan = (ratio[-1], int(off.size))
        self._chan_up = ratio[0] if len(ratio) == 2 else 1

    def channeliser(self, decim: int, in_rate_hz: int, offsets_hz, taps=None):
        """Configure the wideband channeliser (gnuais_batch_channeliser, defined in include/gnuais_hip.h): the batch's
        n_channels receivers become n_channels / K wide streams x K offsets (receiver s*K + k = stream s at
        offsets_hz[k]), decimated by `decim` from `in_rate_hz`.  taps: int16 sequence, or None for the default design.
        Zeroes the channeliser's carry and sample count."""
        self._wide_configure(self._lib.gnuais_batch_channeliser, (int(decim),), in_rate_hz, offsets_hz, taps)

    def resampler(self, up: int, down: int, in_rate_hz: int, offsets_hz, taps=None):
        """Configure the wide stage at a rational ratio (gnuais_batch_resampler, defined in include/gnuais_hip.h): as
        channeliser(), with the chain's rate = in_rate_hz * up / down (up < down, no common factor).  Wideband calls then
        take len a multiple of `down` and give len * up / down rows.  taps: the int16 prototype at up * in_rate_hz, or
        None for the default design.  up = 1 with down <= 64 is channeliser(down, ...)."""
        self._wide_configure(self._lib.gnuais_batch_resampler, (int(up), int(down)), in_rate_hz, offsets_hz, taps)

    def channeliser_for_rate(self, in_rate_hz: int, offsets_hz, out_rate_hz: Optional[int] = None):
        """Configure the wide stage for a capture at `in_rate_hz`: the ratio out_rate_hz / in_rate_hz (out_rate_hz: the
        chain's rate, 48000 by default) reduced by its gcd, through channeliser() where it is 1 / D with D <= 64 and
        through resampler() otherwise.  Returns (up, down)."""
        import math
        out = 48000 if out_rate_hz is None else int(out_rate_hz)
        g = math.gcd(int(in_rate_hz), out)
        up, down = out // g, int(in_rate_hz) // g
        if up == 1 and down <= 64:
            self.channeliser(down, in_rate_hz, offsets_hz)
        else:
            self.resampler(up, down, in_rate_hz, offsets_hz)
        return up, down

    def _wide_shape_ok(self, x, n_rows):
        if not hasattr(self, "_chan"):                  # not configured: the library says so
            return x.ndim == 3 and x.shape[2] == 2
        d, k = self._chan
        return x.ndim == 3 and x.shape[1] * k == self.n_channels and x.shape[2] == 2 and n_rows % d == 0

    def _wide_native(self, samples, fmt):
        """The wide samples of sample format `fmt` ("cs16", "cu8", "cs8", "cf32": GNUAIS_FMT_* in include/gnuais_hip.h) as
        they go to the library, [len][M][2] in the format's own dtype -> (format value, array or tensor).  The dtype
        must already be the format's (int16, uint8, int8, float32; for cf32 also complex64 [len][M]): TypeError
        otherwise, nothing is cast."""
        if fmt not in _lib.FORMATS:
            raise ValueError(f"fmt must be one of {sorted(_lib.FORMATS)}, not {fmt!r}")
        value, dtype = _lib.FORMATS[fmt]
        if _is_torch(samples):
            import torch
            want = {"cs16": torch.int16, "cu8": torch.uint8, "cs8": torch.int8, "cf32": torch.float32}[fmt]
            if fmt == "cf32" and samples.dtype == torch.complex64:
                samples = torch.view_as_real(samples)
            if samples.dtype != want:
                raise TypeError(f"fmt={fmt!r} takes {want} samples, not {samples.dtype}")
            assert samples.is_cuda and samples.is_contiguous()
        else:
            if not isinstance(samples, np.ndarray):
                raise TypeError(f"fmt={fmt!r} takes a numpy array or a torch tensor of the format's dtype")
            if fmt == "cf32" and samples.dtype == np.complex64:
                samples = np.ascontiguousarray(samples).view(np.float32).reshape(samples.shape + (2,))
            if samples.dtype != dtype:
                raise TypeError(f"fmt={fmt!r} takes {dtype} samples, not {samples.dtype}")
            samples = np.ascontiguousarray(samples)
        assert self._wide_shape_ok(samples, int(samples.shape[0]))
        return value, samples

    def run_wideband(self, samples, stream: Optional[int] = None, sync: bool = True, fmt: Optional[str] = None):
        """Wideband in (gnuais_batch_run_wideband): samples int16 [len][n_channels / K][2] = (I, Q) of the wide streams,
        len a multiple of the decimation; channeliser, discriminator and chain on the device.  A CUDA/HIP torch tensor is
        used in place, asynchronously on `stream` or torch's current stream; a numpy array goes through
        gnuais_batch_run_wideband_host (copy, run, sync).
        fmt: the samples' format as an SDR wrote it, "cs16", "cu8", "cs8" or "cf32" (gnuais_batch_run_wideband_fmt; the
        dtypes are in _wide_native): converted on the device where the channeliser loads them, a numpy array crosses
        the bus in its native bytes.  Calls of different formats may follow each other."""
        if fmt is None:
            return self._run(samples, stream, sync, lambda x: self._wide_shape_ok(x, int(x.shape[0])),
                             self._lib.gnuais_batch_run_wideband, self._lib.gnuais_batch_run_wideband_host)
        value, x = self._wide_native(samples, fmt)
        if _is_torch(x):
            import torch
            if stream is None:
                stream = torch.cuda.current_stream(x.device).cuda_stream
            check(self._lib.gnuais_batch_run_wideband_fmt(self._h, value, x.data_ptr(), int(x.shape[0]), C.c_void_p(stream)))
            if sync:
                self.sync()
        else:
            check(self._lib.gnuais_batch_run_wideband_fmt_host(self._h, value, x.ctypes.data, int(x.shape[0])))

    def channelise(self, samples, fmt: Optional[str] = None):
        """The channeliser alone (gnuais_batch_channelise): int16 [len][n_channels / K][2] -> torch int16
        [len / D][n_channels][2] ([len * U / D] behind resampler()) on the device; advances the channeliser's state and nothing else.  fmt: as
        run_wideband (gnuais_batch_channelise_fmt)."""
        d, up = getattr(self, "_chan", (1, 1))[0], getattr(self, "_chan_up", 1)
        if fmt is None:
            return self._stage(samples, lambda x: self._wide_shape_ok(x, int(x.shape[0])),
                               lambda n: (n // d * up, self.n_channels, 2), self._lib.gnuais_batch_channelise)
        import torch
        value, x = self._wide_native(samples, fmt)
        if not _is_torch(x):
            x = torch.from_numpy(x).to(f"cuda:{self.device}")
        out = torch.empty((int(x.shape[0]) // d * up, self.n_channels, 2), dtype=torch.int16, device=x.device)
        stream = torch.cuda.current_stream(x.device)
        check(self._lib.gnuais_batch_channelise_fmt(self._h, value, x.data_ptr(), int(x.shape[0]), out.data_ptr(),
                                                    C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        return out

    def run_host_async(self, samples: np.ndarray):
        """Host input without waiting for the device: pinned double-buffered staging inside the
        library (gnuais_batch_run_host_async); results after sync()."""
        x = np.ascontiguousarray(samples, dtype=np.int16)
        assert x.ndim == 2 and x.shape[1] == self.n_channels
        check(self._lib.gnuais_batch_run_host_async(self._h, x.ctypes.data, int(x.shape[0])))

    def autotune(self, samples, stream: Optional[int] = None) -> float:
        """Measure the stage -> stream assignments on `samples` (CUDA/HIP int16 tensor) and keep the
        fastest; resets the batch.  Returns the best ms per call seen."""
        import torch
        assert samples.is_cuda and samples.dtype == torch.int16 and samples.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream(samples.device).cuda_stream
        ms = C.c_float(0)
        check(self._lib.gnuais_batch_autotune(self._h, samples.data_ptr(), int(samples.shape[0]),
                                              C.c_void_p(stream), C.byref(ms)))
        return ms.value

    def autotune_delivery(self, samples, stream: Optional[int] = None) -> float:
        """gnuais_batch_autotune_delivery(): place the copy stream of stream_nmea() by measurement; resets the
        batch and leaves it streaming.  Returns the best ms per run + stream_nmea seen."""
        import torch
        assert samples.is_cuda and samples.dtype == torch.int16 and samples.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream(samples.device).cuda_stream
        ms = C.c_float(0)
        check(self._lib.gnuais_batch_autotune_delivery(self._h, samples.data_ptr(), int(samples.shape[0]),
                                                       C.c_void_p(stream), C.byref(ms)))
        return ms.value

    def sync(self):
        check(self._lib.gnuais_batch_sync(self._h))

    # -- stage taps -----------------------------------------------------------
    def filter(self, samples):
        """filter_run_buf() for every channel -> float32 [len][n_channels] (torch, device)."""
        import torch
        if not _is_torch(samples):
            samples = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int16)).to(
                f"cuda:{self.device}")
        out = torch.empty(samples.shape, dtype=torch.float32, device=samples.device)
        stream = torch.cuda.current_stream(samples.device).cuda_stream
        check(self._lib.gnuais_batch_filter(self._h, samples.data_ptr(), int(samples.shape[0]),
                                            out.data_ptr(), C.c_void_p(stream)))
        self.sync()
        return out

    def decode_bits(self, bits_per_channel):
        """protodec_decode() for every channel; bits_per_channel: list of uint8 arrays."""
        assert len(bits_per_channel) == self.n_channels
        stride = max(1, max(len(b) for b in bits_per_channel))
        buf = np.zeros((self.n_channels, stride), dtype=np.uint8)
        cnt = np.zeros(self.n_channels, dtype=np.int32)
        for c, b in enumerate(bits_per_channel):
            buf[c, : len(b)] = b
            cnt[c] = len(b)
        check(self._lib.gnuais_batch_decode_bits(self._h, buf.ctypes.data, stride, cnt.ctypes.data))

    def last_bits(self):
        stride = self.max_len // 2 + 64
        buf = np.zeros((self.n_channels, stride), dtype=np.uint8)
        cnt = np.zeros(self.n_channels, dtype=np.int32)
        check(self._lib.gnuais_batch_last_bits(self._h, buf.ctypes.data, stride, cnt.ctypes.data))
        return [buf[c, : cnt[c]].copy() for c in range(self.n_channels)]

    def last_signs(self, length: int) -> np.ndarray:
        """The slicer's decisions of the last run call: uint8 [n_channels][length]."""
        out = np.zeros((self.n_channels, length), dtype=np.uint8)
        check(self._lib.gnuais_batch_last_signs(self._h, out.ctypes.data, length))
        return out

    def info(self, name: str) -> float:
        v = C.c_double()
        check(self._lib.gnuais_batch_info(self._h, name.encode(), C.byref(v)))
        return v.value

    # -- results --------------------------------------------------------------
    def pending_frames(self) -> int:
        n = C.c_int()
        check(self._lib.gnuais_batch_pending_frames(self._h, C.byref(n)))
        return n.value

    def discard_frames(self, stream: Optional[int] = None):
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device).cuda_stream
        check(self._lib.gnuais_batch_discard_frames(self._h, C.c_void_p(stream)))

    def drain_frames(self) -> np.ndarray:
        n = self.pending_frames()
        out = np.zeros(max(n, 1), dtype=FRAME_DTYPE)
        got = C.c_int()
        check(self._lib.gnuais_batch_drain_frames(self._h, out.ctypes.data, int(out.size),
                                                  C.byref(got)))
        return out[: got.value].copy()

    def frame_times(self, on: bool = True):
        """gnuais_batch_frame_times(): from now on every frame gets its receive time in chain rows (the definition is in
        include/gnuais_hip.h); one more small launch per call.  Synchronises.  Not on a streaming batch."""
        check(self._lib.gnuais_batch_frame_times(self._h, int(bool(on))))

    def repair(self, on: bool = True):
        """gnuais_batch_repair(): from now on a frame that fails the CRC by one symbol error (two adjacent bits) is
        repaired on the device and delivered with flags bit 6 set (the definition is in include/gnuais_hip.h); one more
        launch per call.  Synchronises.  Not on a streaming batch."""
        check(self._lib.gnuais_batch_repair(self._h, int(bool(on))))

    def repaired(self) -> np.ndarray:
        """gnuais_batch_repaired(): int32 [n_channels], the repairs per channel since create / reset"""
        out = np.zeros(self.n_channels, dtype=np.int32)
        check(self._lib.gnuais_batch_repaired(self._h, out.ctypes.data))
        return out

    def long_frames(self, on: bool = True):
        """gnuais_batch_long_frames(): from now on a second decoder per channel delivers the messages of three to five
        slots (427 .. 1008 bits), which the chain -- the reference bit for bit -- gives up at 449 stored bits, as records
        of their own (the definition is in include/gnuais_hip.h); one more launch per call.  Synchronises; switching
        resets that decoder, its ring and its counters.  Not on a streaming batch."""
        check(self._lib.gnuais_batch_long_frames(self._h, int(bool(on))))

    def pending_long_frames(self) -> int:
        n = C.c_int()
        check(self._lib.gnuais_batch_pending_long_frames(self._h, C.byref(n)))
        return n.value

    def drain_long_frames(self) -> np.ndarray:
        """gnuais_batch_drain_long_frames(): LONG_FRAME_DTYPE records in (channel, stamp) order, each with its receive
        time t in chain rows (-1: closed by decode_bits).  GnuaisError(E_OVERFLOW) carries what was delivered in
        `.frames`."""
        n = self.pending_long_frames()
        out = np.zeros(max(n, 1), dtype=LONG_FRAME_DTYPE)
        got = C.c_int()
        rc = self._lib.gnuais_batch_drain_long_frames(self._h, out.ctypes.data, int(out.size), C.byref(got))
        if rc == E_OVERFLOW:
            err = GnuaisError(rc, self._lib.gnuais_last_error().decode())
            err.frames = out[: got.value].copy()
            raise err
        check(rc)
        return out[: got.value].copy()

    def long_counters(self):
        """gnuais_batch_long_counters(): (delivered, failed), int32 [n_channels] each: the long frames the second decoder
        delivered and those (more than 426 bits) whose CRC failed"""
        d = np.zeros(self.n_channels, dtype=np.int32)
        f = np.zeros(self.n_channels, dtype=np.int32)
        check(self._lib.gnuais_batch_long_counters(self._h, d.ctypes.data, f.ctypes.data))
        return d, f

    def long_repair(self, on: bool = True):
        """gnuais_batch_long_repair(): from now on a long frame that fails the CRC by one symbol error (two adjacent
        bits) is repaired on the device and delivered with flags bit 6 set (the definition is in include/gnuais_hip.h).
        Needs long_frames() on; switching that off switches this off."""
        check(self._lib.gnuais_batch_long_repair(self._h, int(bool(on))))

    def long_repaired(self) -> np.ndarray:
        """gnuais_batch_long_repaired(): int32 [n_channels], the long frames repaired per channel"""
        out = np.zeros(self.n_channels, dtype=np.int32)
        check(self._lib.gnuais_batch_long_repaired(self._h, out.ctypes.data))
        return out

    def long_frame_signal(self, on: bool = True):
        """gnuais_batch_long_frame_signal(): from now on every long frame of I/Q and wideband input gets its signal power
        and carrier error, and covers its air time in occupancy() when that is switched on afterwards (the definition is
        in include/gnuais_hip.h); one more launch per call.  Needs long_frames() and frame_signal(), and occupancy() off
        at the switch.  Synchronises."""
        check(self._lib.gnuais_batch_long_frame_signal(self._h, int(bool(on))))

    def drain_long_frames_signal(self):
        """gnuais_batch_drain_long_frames_signal(): (records, signal): drain_long_frames() with signal[i] (lib.SIGNAL_DTYPE:
        power, ferr, blocks; blocks 0: no measurement) the record of records[i].  GnuaisError(E_OVERFLOW) carries what was
        delivered in `.frames`."""
        n = max(self.pending_long_frames(), 1)
        out = np.zeros(n, dtype=LONG_FRAME_DTYPE)
        sig = np.zeros(n, dtype=_lib.SIGNAL_DTYPE)
        got = C.c_int()
        rc = self._lib.gnuais_batch_drain_long_frames_signal(self._h, out.ctypes.data, sig.ctypes.data, n, C.byref(got))
        res = (out[: got.value].copy(), sig[: got.value].copy())
        if rc == E_OVERFLOW:
            err = GnuaisError(rc, self._lib.gnuais_last_error().decode())
            err.frames = res
            raise err
        check(rc)
        return res

    def long_fsm_state(self) -> np.ndarray:
        """gnuais_batch_long_fsm_state(): the second decoder's live fields, as fsm_state()"""
        return self._struct_array(self._lib.gnuais_batch_long_fsm_state, FSM_DTYPE)

    def drain_frames_timed(self):
        """gnuais_batch_drain_frames_timed(): (frames, int64 times), times[i] the receive time of frames[i] in chain rows
        since create / reset, -1 where there is none (decode_bits, or appended while the feature was off)."""
        n = self.pending_frames()
        out = np.zeros(max(n, 1), dtype=FRAME_DTYPE)
        times = np.zeros(max(n, 1), dtype=np.int64)
        got = C.c_int()
        check(self._lib.gnuais_batch_drain_frames_timed(self._h, out.ctypes.data, times.ctypes.data, int(out.size),
                                                        C.byref(got)))
        return out[: got.value].copy(), times[: got.value].copy()

    def frame_signal(self, on: bool = True):
        """gnuais_batch_frame_signal(): from now on every frame of I/Q and wideband input gets its signal power and
        carrier error (the definition is in include/gnuais_hip.h); one more launch per I/Q-type call and one per call.
        Needs frame_times().  Synchronises.  Not on a streaming batch."""
        check(self._lib.gnuais_batch_frame_signal(self._h, int(bool(on))))

    def drain_frames_signal(self):
        """gnuais_batch_drain_frames_signal(): (frames, int64 times, signal), signal a structured array (lib.SIGNAL_DTYPE)
        with power (full scale 2^31; signal_dbfs()), ferr (signal_hz()) and blocks (0: no measurement) of frames[i]"""
        n = max(self.pending_frames(), 1)
        out = np.zeros(n, dtype=FRAME_DTYPE)
        times = np.zeros(n, dtype=np.int64)
        sig = np.zeros(n, dtype=_lib.SIGNAL_DTYPE)
        got = C.c_int()
        check(self._lib.gnuais_batch_drain_frames_signal(self._h, out.ctypes.data, times.ctypes.data, sig.ctypes.data, n,
                                                         C.byref(got)))
        return out[: got.value].copy(), times[: got.value].copy(), sig[: got.value].copy()

    def signal_blocks(self, j0: int, count: int) -> np.ndarray:
        """gnuais_batch_signal_blocks(): int64 [count][n_channels][3], the sums (P, R, I) of the blocks [j0, j0 + count)
        of 64 rows (a parity tap)"""
        out = np.zeros((max(count, 0), self.n_channels, 3), dtype=np.int64)
        check(self._lib.gnuais_batch_signal_blocks(self._h, int(j0), int(count), out.ctypes.data))
        return out

    def occupancy(self, epoch_blocks: int = 1024, margin: int = 16):
        """gnuais_batch_occupancy(): from now on every channel gets, per epoch of epoch_blocks blocks of 64 rows of I/Q
        input, its noise floor, busy and covered blocks and bursts (the definition is in include/gnuais_hip.h); margin in
        code steps of 0.376 dB above the floor (16: 6.02 dB).  epoch_blocks = 0: off.  Needs frame_signal().
        Synchronises.  Not on a streaming batch."""
        check(self._lib.gnuais_batch_occupancy(self._h, int(epoch_blocks), int(margin)))

    def drain_occupancy(self):
        """gnuais_batch_drain_occupancy(): (int64 first_block[n], records[n][n_channels]) of the final epochs not
        delivered yet, oldest first; records a structured array (lib.OCCUPANCY_DTYPE)"""
        n = _lib.OCCUPANCY_EPOCHS_HELD
        rec = np.zeros((n, self.n_channels), dtype=_lib.OCCUPANCY_DTYPE)
        first = np.zeros(n, dtype=np.int64)
        got = C.c_int()
        check(self._lib.gnuais_batch_drain_occupancy(self._h, rec.ctypes.data, first.ctypes.data, n, C.byref(got)))
        return first[: got.value].copy(), rec[: got.value].copy()

    def occupancy_lost(self) -> int:
        """gnuais_batch_occupancy_lost(): final epochs overwritten before a drain took them"""
        lost = C.c_longlong()
        check(self._lib.gnuais_batch_occupancy_lost(self._h, C.byref(lost)))
        return lost.value

    def occupancy_blocks(self, j0: int, count: int) -> np.ndarray:
        """gnuais_batch_occupancy_blocks(): uint16 [count][n_channels], code | busy << 14 | cover << 15 of the blocks
        [j0, j0 + count) of final epochs (a tap, and the occupancy map)"""
        out = np.zeros((max(count, 0), self.n_channels), dtype=np.uint16)
        check(self._lib.gnuais_batch_occupancy_blocks(self._h, int(j0), int(count), out.ctypes.data))
        return out

    def unique(self, window: int):
        """gnuais_batch_unique(): window > 0 rows: drain_frames_unique() delivers each transmission once (equal frames
        whose receive times chain within the window; the definition is in include/gnuais_hip.h); 0: off.  Needs
        frame_times(); clears the carried state.  Synchronises.  Not on a streaming batch."""
        check(self._lib.gnuais_batch_unique(self._h, int(window)))

    def drain_frames_unique(self):
        """gnuais_batch_drain_frames_unique(): (frames, int64 times, int32 copies): one record per transmission -- the
        earliest intact copy and its own time -- and how many copies this drain merged into it"""
        n = max(self.pending_frames(), 1)
        out = np.zeros(n, dtype=FRAME_DTYPE)
        times = np.zeros(n, dtype=np.int64)
        copies = np.zeros(n, dtype=np.int32)
        got = C.c_int()
        check(self._lib.gnuais_batch_drain_frames_unique(self._h, out.ctypes.data, times.ctypes.data, copies.ctypes.data,
                                                         n, C.byref(got)))
        return out[: got.value].copy(), times[: got.value].copy(), copies[: got.value].copy()

    def drain_frames_heard(self):
        """gnuais_batch_drain_frames_heard(): (frames, int64 times, int32 copies, int32 first, members) -- what
        drain_frames_unique() delivers, and who heard each transmission: cluster i's members are
        members[first[i]:first[i + 1]] (lib.HEARER_DTYPE: channel, flags, t, signal) in the order (t, channel)"""
        n = max(self.pending_frames(), 1)
        out = np.zeros(n, dtype=FRAME_DTYPE)
        times = np.zeros(n, dtype=np.int64)
        copies = np.zeros(n, dtype=np.int32)
        first = np.zeros(n + 1, dtype=np.int32)
        members = np.zeros(n, dtype=_lib.HEARER_DTYPE)
        got, nm = C.c_int(), C.c_int()
        check(self._lib.gnuais_batch_drain_frames_heard(self._h, out.ctypes.data, times.ctypes.data, copies.ctypes.data,
                                                        n, C.byref(got), first.ctypes.data, members.ctypes.data,
                                                        C.byref(nm)))
        return (out[: got.value].copy(), times[: got.value].copy(), copies[: got.value].copy(),
                first[: got.value + 1].copy(), members[: nm.value].copy())

    def unique_late(self) -> int:
        """gnuais_batch_unique_late(): copies that arrived after a drain had delivered their transmission"""
        v = C.c_longlong()
        check(self._lib.gnuais_batch_unique_late(self._h, C.byref(v)))
        return v.value

    def long_unique(self, window: int):
        """gnuais_batch_long_unique(): window > 0 rows: drain_long_frames_unique() delivers each long transmission once
        (equal long frames whose own times t chain within the window; the definition is in include/gnuais_hip.h); 0:
        off.  Needs long_frames(); clears the carried state, which is this merge's own.  Synchronises."""
        check(self._lib.gnuais_batch_long_unique(self._h, int(window)))

    def _drain_long_merged(self, heard: bool):
        n = max(self.pending_long_frames(), 1)
        out = np.zeros(n, dtype=LONG_FRAME_DTYPE)
        copies = np.zeros(n, dtype=np.int32)
        got, nm = C.c_int(), C.c_int()
        if heard:
            first = np.zeros(n + 1, dtype=np.int32)
            members = np.zeros(n, dtype=_lib.HEARER_DTYPE)
            rc = self._lib.gnuais_batch_drain_long_frames_heard(self._h, out.ctypes.data, copies.ctypes.data, n,
                                                                C.byref(got), first.ctypes.data, members.ctypes.data,
                                                                C.byref(nm))
            res = (out[: got.value].copy(), copies[: got.value].copy(), first[: got.value + 1].copy(),
                   members[: nm.value].copy())
        else:
            rc = self._lib.gnuais_batch_drain_long_frames_unique(self._h, out.ctypes.data, copies.ctypes.data, n,
                                                                 C.byref(got))
            res = (out[: got.value].copy(), copies[: got.value].copy())
        if rc == E_OVERFLOW:
            err = GnuaisError(rc, self._lib.gnuais_last_error().decode())
            err.frames = res
            raise err
        check(rc)
        return res

    def drain_long_frames_unique(self):
        """gnuais_batch_drain_long_frames_unique(): (records, int32 copies): one LONG_FRAME_DTYPE record per long
        transmission -- the earliest intact copy, with its own t -- and how many copies this drain merged into it.
        GnuaisError(E_OVERFLOW) carries what was delivered in `.frames`."""
        return self._drain_long_merged(False)

    def drain_long_frames_heard(self):
        """gnuais_batch_drain_long_frames_heard(): (records, int32 copies, int32 first, members) -- what
        drain_long_frames_unique() delivers, and who heard each transmission: cluster i's members are
        members[first[i]:first[i + 1]] (lib.HEARER_DTYPE: channel, flags, t, and the copy's signal record while
        long_frame_signal() is on, else zeros) in the order (t, channel)"""
        return self._drain_long_merged(True)

    def long_unique_late(self) -> int:
        """gnuais_batch_long_unique_late(): long copies that arrived after a drain had delivered their transmission"""
        v = C.c_longlong()
        check(self._lib.gnuais_batch_long_unique_late(self._h, C.byref(v)))
        return v.value

    def time_map(self, kind: str = "audio"):
        """gnuais_batch_time_map(): (mul, off) with input sample index = t * mul + off for the batch's configuration as
        it is now; kind: "audio", "iq" or "wideband"."""
        mul, off = C.c_longlong(0), C.c_longlong(0)
        check(self._lib.gnuais_batch_time_map(self._h, _lib.INPUT_KINDS[kind], C.byref(mul), C.byref(off)))
        return mul.value, off.value

    def time_map_ratio(self, kind: str = "audio"):
        """gnuais_batch_time_map_ratio(): (num, den, off) with input sample index = (t * num + off) // den (floor) for
        the batch's configuration as it is now, whatever configured the wide stage; kind as time_map()."""
        num, den, off = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        check(self._lib.gnuais_batch_time_map_ratio(self._h, _lib.INPUT_KINDS[kind], C.byref(num), C.byref(den),
                                                    C.byref(off)))
        return num.value, den.value, off.value

    def drain_nmea(self, seqnr: np.ndarray):
        """The queued frames as !AIVDM sentences, formatted on the device (row f1); consumes them.
        seqnr: uint8[n_channels], updated in place.  Returns (text bytes, sentences, frames)."""
        assert seqnr.dtype == np.uint8 and seqnr.flags.c_contiguous and len(seqnr) == self.n_channels
        n = self.pending_frames()
        out = np.empty(164 * max(n, 1), dtype=np.uint8)
        ln, ns, nf = C.c_size_t(0), C.c_int(0), C.c_int(0)
        check(self._lib.gnuais_batch_drain_nmea(self._h, seqnr.ctypes.data, out.ctypes.data, out.size,
                                                C.byref(ln), C.byref(ns), C.byref(nf)))
        return out[: ln.value].tobytes(), ns.value, nf.value

    @property
    def stream_depth(self) -> int:
        return int(self.info("stream_depth"))

    def stream_nmea(self, copy: bool = True):
        """gnuais_batch_stream_nmea(): call after every run(); returns (text, sentences, frames) of the
        call self.stream_depth calls ago -- frames == -1 while the pipeline fills.  copy=False returns a
        uint8 view of the library's pinned buffer (valid until the next call) instead of bytes."""
        ptr, ln, ns, nf = C.c_void_p(), C.c_size_t(0), C.c_int(0), C.c_int(0)
        rc = self._lib.gnuais_batch_stream_nmea(self._h, C.cast(C.byref(ptr), C.POINTER(C.c_char_p)), C.byref(ln),
                                                C.byref(ns), C.byref(nf))
        # A slot's LATE error (its frame ring overflowed, a PLL-stage watchdog) comes with that slot's text: the text
        # that did fit is handed out and the pipeline goes on.  Build the result first, then raise with it attached
        # (GnuaisError.partial) -- or, for an overflow with on_overflow="keep", return it and count the event.
        if ln.value:
            view = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(ln.value,))
            res = ((view.tobytes() if copy else view), ns.value, nf.value)
        else:
            res = ((b"" if copy else np.zeros(0, dtype=np.uint8)), ns.value, nf.value)
        if rc != OK:
            if rc == E_OVERFLOW and self.on_overflow == "keep":
                self.stream_overflows += 1
                return res
            err = GnuaisError(rc, self._lib.gnuais_last_error().decode())
            err.partial = res
            raise err
        return res

    def fold_vessels(self) -> np.ndarray:
        """gnuais_batch_fold_vessels(): the vessel table of the queued frames (gnuais_vessel per MMSI, sorted),
        folded on the device; the frames stay queued."""
        out = np.zeros(max(self.pending_frames(), 1), dtype=VESSEL_DTYPE)
        n = C.c_int(0)
        check(self._lib.gnuais_batch_fold_vessels(self._h, out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    def vessel_table_enable(self, capacity: int) -> None:
        """gnuais_batch_vessel_table_enable(): an empty position cache for `capacity` vessels, carried on the device
        from batch to batch; stream_nmea() folds every span it takes off into it from now on."""
        check(self._lib.gnuais_batch_vessel_table_enable(self._h, capacity))
        self._vt_capacity = capacity

    def vessel_table_update(self) -> None:
        """gnuais_batch_vessel_table_update(): the queued frames into the carried table (drain-type use: call it
        before the drain that consumes them)."""
        check(self._lib.gnuais_batch_vessel_table_update(self._h))

    def vessel_table(self) -> np.ndarray:
        """gnuais_batch_vessel_table(): the carried table, sorted by MMSI."""
        out = np.zeros(max(getattr(self, "_vt_capacity", 1), 1), dtype=VESSEL_DTYPE)
        n = C.c_int(0)
        check(self._lib.gnuais_batch_vessel_table(self._h, out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    def vessel_table_clear(self) -> None:
        check(self._lib.gnuais_batch_vessel_table_clear(self._h))

    def drain_messages(self, seqnr: np.ndarray, chanid: Optional[bytes] = None):
        """gnuais_batch_drain_messages(): sentences and stdout lines of everything queued, both formatted
        on the device -> (nmea bytes, text bytes, sentences, lines, frames)."""
        assert seqnr.dtype == np.uint8 and seqnr.flags.c_contiguous and len(seqnr) == self.n_channels
        assert chanid is None or len(chanid) == self.n_channels
        n = max(self.pending_frames(), 1)
        nm = np.empty(164 * n, dtype=np.uint8)
        tx = np.empty(512 * n, dtype=np.uint8)
        nl, tl, ns, nlines, nf = C.c_size_t(0), C.c_size_t(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._lib.gnuais_batch_drain_messages(self._h, seqnr.ctypes.data, chanid, nm.ctypes.data, nm.size,
                                                    C.byref(nl), C.byref(ns), tx.ctypes.data, tx.size, C.byref(tl),
                                                    C.byref(nlines), C.byref(nf)))
        return nm[: nl.value].tobytes(), tx[: tl.value].tobytes(), ns.value, nlines.value, nf.value

    def drain_frames_nmea(self, seqnr: np.ndarray):
        """Records and device-formatted sentences of the same drained span: (frames, text, sentences)."""
        assert seqnr.dtype == np.uint8 and seqnr.flags.c_contiguous and len(seqnr) == self.n_channels
        n = self.pending_frames()
        fr = np.zeros(max(n, 1), dtype=FRAME_DTYPE)
        out = np.empty(164 * max(n, 1), dtype=np.uint8)
        ln, ns, nf = C.c_size_t(0), C.c_int(0), C.c_int(0)
        check(self._lib.gnuais_batch_drain_frames_nmea(self._h, fr.ctypes.data, int(fr.size), C.byref(nf),
                                                       seqnr.ctypes.data, out.ctypes.data, out.size,
                                                       C.byref(ln), C.byref(ns)))
        return fr[: nf.value].copy(), out[: ln.value].tobytes(), ns.value

    def _struct_array(self, fn, dtype):
        out = np.zeros(self.n_channels, dtype=dtype)
        check(fn(self._h, out.ctypes.data))
        return out

    def counters(self) -> np.ndarray:
        return self._struct_array(self._lib.gnuais_batch_counters, COUNTERS_DTYPE)

    def total_received(self) -> int:
        t = C.c_longlong()
        check(self._lib.gnuais_batch_total_received(self._h, C.byref(t)))
        return t.value

    def pll_state(self) -> np.ndarray:
        return self._struct_array(self._lib.gnuais_batch_pll_state, PLL_DTYPE)

    def fsm_state(self) -> np.ndarray:
        return self._struct_array(self._lib.gnuais_batch_fsm_state, FSM_DTYPE)

    def protodec_reset(self):
        """protodec_reset() (protodec.c:87-100) for every decoder: back to ST_SKURR, counters stay."""
        check(self._lib.gnuais_batch_protodec_reset(self._h))

    def frame_bits(self, channel: int):
        """d->buffer of one channel (protodec.h:52): the stored bits of the frame in progress or of the last frame that
        reached its stop bit, one per byte; None when neither is on record."""
        out = np.zeros(450, dtype=np.uint8)
        n = C.c_int(0)
        check(self._lib.gnuais_batch_frame_bits(self._h, int(channel), out.ctypes.data, out.size, C.byref(n)))
        return None if n.value < 0 else out[:min(n.value, out.size)].copy()

    def maxval(self) -> np.ndarray:
        out = np.zeros(self.n_channels, dtype=np.int16)
        check(self._lib.gnuais_batch_maxval(self._h, out.ctypes.data))
        return out

    def history(self) -> np.ndarray:
        out = np.zeros((self.n_channels, self.n_taps), dtype=np.int16)
        check(self._lib.gnuais_batch_history(self._h, out.ctypes.data))
        return out

    # -- timing ---------------------------------------------------------------
    KERNELS = ("fir_slice", "pll", "hdlc_deframe", "hdlc_crc")

    def set_timing(self, on: bool):
        check(self._lib.gnuais_batch_set_timing(self._h, int(on)))

    def mean_timing(self):
        ms = (C.c_float * 5)()
        n = C.c_int()
        check(self._lib.gnuais_batch_mean_timing(self._h, ms, C.byref(n)))
        d = dict(zip(self.KERNELS + ("total",), ms))
        d["calls"] = n.value
        return d

    def last_timing(self):
        ms = (C.c_float * 5)()
        check(self._lib.gnuais_batch_last_timing(self._h, ms))
        return dict(zip(self.KERNELS + ("total",), ms))


def crc16_batch(messages, device: int = 0) -> np.ndarray:
    """protodec_sdlc_crc() of each byte string, on the device."""
    lib = _lib.load()
    stride = max(1, max(len(m) for m in messages))
    data = np.zeros((len(messages), stride), dtype=np.uint8)
    lens = np.zeros(len(messages), dtype=np.int32)
    for i, m in enumerate(messages):
        data[i, : len(m)] = np.frombuffer(m, dtype=np.uint8)
        lens[i] = len(m)
    out = np.zeros(len(messages), dtype=np.uint16)
    check(lib.gnuais_crc16_batch(device, data.ctypes.data, stride, lens.ctypes.data,
                                 len(messages), out.ctypes.data))
    return out


def nmea_from_frames(frames: np.ndarray, seqnr: np.ndarray) -> bytes:
    """The "!AIVDM,...*hh\\r\\n" sentences the reference emits for these frame records
    (protodec_getdata / protodec_generate_nmea), concatenated.  `seqnr` (uint8 per channel)
    is the rolling sequence digit state, updated in place."""
    lib = _lib.load()
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    assert seqnr.dtype == np.uint8 and seqnr.flags.c_contiguous
    cap = 164 * max(1, len(frames))
    out = np.zeros(cap, dtype=np.uint8)
    need = C.c_size_t(0)
    n_sent = C.c_int(0)
    check(lib.gnuais_nmea_from_frames(frames.ctypes.data, len(frames), seqnr.ctypes.data, len(seqnr),
                                      out.ctypes.data, cap, C.byref(need), C.byref(n_sent)))
    return out[: need.value].tobytes()


def nmea_from_long_frames(frames: np.ndarray, seqnr: np.ndarray) -> bytes:
    """gnuais_nmea_from_long_frames(): the two or three "!AIVDM" sentences of each long frame record, concatenated;
    `seqnr` as in nmea_from_frames() (the same array may serve both)."""
    lib = _lib.load()
    frames = np.ascontiguousarray(frames, dtype=LONG_FRAME_DTYPE)
    assert seqnr.dtype == np.uint8 and seqnr.flags.c_contiguous
    cap = 3 * 82 * max(1, len(frames))
    out = np.zeros(cap, dtype=np.uint8)
    need = C.c_size_t(0)
    n_sent = C.c_int(0)
    check(lib.gnuais_nmea_from_long_frames(frames.ctypes.data, len(frames), seqnr.ctypes.data, len(seqnr),
                                           out.ctypes.data, cap, C.byref(need), C.byref(n_sent)))
    return out[: need.value].tobytes()


def nmea_tagged_from_frames(frames: np.ndarray, times: np.ndarray, seqnr: np.ndarray, mul: int = 1, off: int = 0,
                            rate_hz: int = 48000, epoch_s: int = 0) -> bytes:
    """nmea_from_frames() with a TAG block "\\c:<unix>*hh\\" in front of every sentence of a frame whose time is not -1:
    <unix> = epoch_s + floor((times[i] * mul + off) / rate_hz).  mul / off: ReceiverBatch.time_map(); rate_hz: the rate
    of the input samples; epoch_s: the UNIX second of input sample 0."""
    lib = _lib.load()
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    times = np.ascontiguousarray(times, dtype=np.int64)
    assert len(times) == len(frames)
    assert seqnr.dtype == np.uint8 and seqnr.flags.c_contiguous
    cap = (164 + 2 * 32) * max(1, len(frames))
    out = np.zeros(cap, dtype=np.uint8)
    need = C.c_size_t(0)
    n_sent = C.c_int(0)
    check(lib.gnuais_nmea_tagged_from_frames(frames.ctypes.data, times.ctypes.data, len(frames), seqnr.ctypes.data,
                                             len(seqnr), int(mul), int(off), int(rate_hz), int(epoch_s), out.ctypes.data,
                                             cap, C.byref(need), C.byref(n_sent)))
    return out[: need.value].tobytes()


def messages_from_frames(frames: np.ndarray, seqnr: np.ndarray, chanid: Optional[bytes] = None):
    """(NMEA sentences, stdout text) exactly as the reference's protodec_getdata() produces them
    for these frame records.  `seqnr` as in nmea_from_frames; `chanid` one byte per channel."""
    lib = _lib.load()
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    assert seqnr.dtype == np.uint8 and seqnr.flags.c_contiguous
    assert chanid is None or len(chanid) == len(seqnr)
    nm = np.zeros(164 * max(1, len(frames)), dtype=np.uint8)
    tx = np.zeros(1024 * max(1, len(frames)), dtype=np.uint8)
    nm_len, tx_len = C.c_size_t(0), C.c_size_t(0)
    check(lib.gnuais_messages_from_frames(frames.ctypes.data, len(frames), seqnr.ctypes.data, chanid,
                                          len(seqnr), nm.ctypes.data, nm.size, C.byref(nm_len), None,
                                          tx.ctypes.data, tx.size, C.byref(tx_len), None))
    return nm[: nm_len.value].tobytes(), tx[: tx_len.value].tobytes()


def range_from_frames(frames: np.ndarray, best_range_km: np.ndarray, my_lat_deg: float, my_lon_deg: float):
    """update_range() (range.c:32-45) over these frame records: best_range_km[channel] (float32,
    updated in place) keeps the farthest plausible position of a type 1-3 / 4 / 18 report."""
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    assert best_range_km.dtype == np.float32 and best_range_km.flags.c_contiguous
    check(_lib.load().gnuais_range_from_frames(frames.ctypes.data, len(frames), len(best_range_km),
                                               C.c_float(my_lat_deg), C.c_float(my_lon_deg),
                                               best_range_km.ctypes.data))
    return best_range_km


# struct gnuais_vessel (include/gnuais_hip.h) = the reference's struct cache_ent, strings inline
VESSEL_DTYPE = np.dtype([("mmsi", "<i4"), ("set", "<u4"), ("lat", "<f4"), ("lon", "<f4"), ("hdg", "<i4"),
                         ("course", "<f4"), ("sog", "<f4"), ("navstat", "<i4"), ("imo", "<i4"),
                         ("shiptype", "<i4"), ("A", "<i4"), ("B", "<i4"), ("C", "<i4"), ("D", "<i4"),
                         ("draught", "<f4"), ("persons_on_board", "<i4"), ("callsign", "S8"),
                         ("name", "S24"), ("destination", "S24")])
assert VESSEL_DTYPE.itemsize == 120


def vessels_from_frames(frames: np.ndarray, table: Optional[np.ndarray] = None) -> np.ndarray:
    """Fold frame records into the vessel table the reference's position cache would hold
    (cache.c:204-384), continuing from `table` (sorted by MMSI) or from an empty cache."""
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    n_old = 0 if table is None else len(table)
    out = np.zeros(n_old + len(frames), dtype=VESSEL_DTYPE)
    if n_old:
        out[:n_old] = table
    n = C.c_int(n_old)
    check(_lib.load().gnuais_vessels_from_frames(frames.ctypes.data, len(frames), out.ctypes.data, len(out),
                                                 C.byref(n)))
    return out[: n.value].copy()


def tile_channels(base, n_channels: int):
    """Device-side benchmark input builder: base torch int16 [K][L] ->
    interleaved [L][n_channels]."""
    import torch
    assert base.is_cuda and base.dtype == torch.int16 and base.is_contiguous()
    k, n = base.shape
    out = torch.empty((n, n_channels), dtype=torch.int16, device=base.device)
    stream = torch.cuda.current_stream(base.device).cuda_stream
    check(_lib.load().gnuais_tile_channels(base.data_ptr(), k, n, out.data_ptr(), n_channels,
                                           C.c_void_p(stream)))
    return out


class Uniq:
    """gnuais_uniq: the duplicate merge of gnuais_batch_unique() as a host object, no device (include/gnuais_hip.h).
    push() is one drain of the definition."""

    def __init__(self, window: int):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        rc = self._lib.gnuais_uniq_create(C.byref(self._h), int(window))
        if rc != _lib.OK:
            raise _lib.GnuaisError(rc, "gnuais_uniq_create: the window must be > 0")

    def close(self):
        if self._h:
            self._lib.gnuais_uniq_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def reset(self):
        self._lib.gnuais_uniq_reset(self._h)

    def late(self) -> int:
        return int(self._lib.gnuais_uniq_late(self._h))

    def push(self, frames: np.ndarray, times: np.ndarray, rows: int, cap: Optional[int] = None):
        """-> (frames, times, copies) of the clusters this drain delivers; cap: room offered (default: enough)"""
        frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
        times = np.ascontiguousarray(times, dtype=np.int64)
        assert frames.ndim == 1 and times.shape == frames.shape
        n = int(frames.size)
        cap = n if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=FRAME_DTYPE)
        out_t = np.zeros(max(cap, 1), dtype=np.int64)
        out_c = np.zeros(max(cap, 1), dtype=np.int32)
        got = C.c_int()
        rc = self._lib.gnuais_uniq_push(self._h, frames.ctypes.data, times.ctypes.data, n, int(rows), out.ctypes.data,
                                        out_t.ctypes.data, out_c.ctypes.data, cap, C.byref(got))
        if rc != _lib.OK:
            raise _lib.GnuaisError(rc, "gnuais_uniq_push: argument, or more records than cap")
        return out[: got.value].copy(), out_t[: got.value].copy(), out_c[: got.value].copy()

    def push_heard(self, frames: np.ndarray, times: np.ndarray, rows: int, signal: Optional[np.ndarray] = None,
                   cap: Optional[int] = None):
        """-> (frames, times, copies, first, members): push() with the clusters' member lists
        (gnuais_uniq_push_heard); signal: the frames' records (lib.SIGNAL_DTYPE), None for zeros"""
        frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
        times = np.ascontiguousarray(times, dtype=np.int64)
        assert frames.ndim == 1 and times.shape == frames.shape
        if signal is not None:
            signal = np.ascontiguousarray(signal, dtype=_lib.SIGNAL_DTYPE)
            assert signal.shape == frames.shape
        n = int(frames.size)
        cap = n if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=FRAME_DTYPE)
        out_t = np.zeros(max(cap, 1), dtype=np.int64)
        out_c = np.zeros(max(cap, 1), dtype=np.int32)
        first = np.zeros(cap + 1, dtype=np.int32)
        members = np.zeros(max(n, 1), dtype=_lib.HEARER_DTYPE)
        got, nm = C.c_int(), C.c_int()
        rc = self._lib.gnuais_uniq_push_heard(self._h, frames.ctypes.data, times.ctypes.data,
                                              signal.ctypes.data if signal is not None else None, n, int(rows),
                                              out.ctypes.data, out_t.ctypes.data, out_c.ctypes.data, cap, C.byref(got),
                                              first.ctypes.data, members.ctypes.data, C.byref(nm))
        if rc != _lib.OK:
            raise _lib.GnuaisError(rc, "gnuais_uniq_push_heard: argument, or more records than cap")
        return (out[: got.value].copy(), out_t[: got.value].copy(), out_c[: got.value].copy(),
                first[: got.value + 1].copy(), members[: nm.value].copy())


class LongUniq:
    """gnuais_long_uniq: the duplicate merge of gnuais_batch_long_unique() as a host object, no device
    (include/gnuais_hip.h).  push() is one drain of the definition; a record's time is its own t."""

    def __init__(self, window: int):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        rc = self._lib.gnuais_long_uniq_create(C.byref(self._h), int(window))
        if rc != _lib.OK:
            raise _lib.GnuaisError(rc, "gnuais_long_uniq_create: the window must be > 0")

    def close(self):
        if self._h:
            self._lib.gnuais_long_uniq_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def reset(self):
        self._lib.gnuais_long_uniq_reset(self._h)

    def late(self) -> int:
        return int(self._lib.gnuais_long_uniq_late(self._h))

    def push(self, frames: np.ndarray, rows: int, cap: Optional[int] = None):
        """-> (records, copies) of the clusters this drain delivers; cap: room offered (default: enough)"""
        frames = np.ascontiguousarray(frames, dtype=LONG_FRAME_DTYPE)
        assert frames.ndim == 1
        n = int(frames.size)
        cap = n if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=LONG_FRAME_DTYPE)
        out_c = np.zeros(max(cap, 1), dtype=np.int32)
        got = C.c_int()
        rc = self._lib.gnuais_long_uniq_push(self._h, frames.ctypes.data, n, int(rows), out.ctypes.data, out_c.ctypes.data,
                                             cap, C.byref(got))
        if rc != _lib.OK:
            raise _lib.GnuaisError(rc, "gnuais_long_uniq_push: argument, or more records than cap")
        return out[: got.value].copy(), out_c[: got.value].copy()

    def push_heard(self, frames: np.ndarray, rows: int, cap: Optional[int] = None, signal: Optional[np.ndarray] = None):
        """-> (records, copies, first, members): push() with the clusters' member lists (gnuais_long_uniq_push_heard);
        signal: the frames' records (lib.SIGNAL_DTYPE) for the members (gnuais_long_uniq_push_heard_signal), None: zeros"""
        frames = np.ascontiguousarray(frames, dtype=LONG_FRAME_DTYPE)
        assert frames.ndim == 1
        n = int(frames.size)
        if signal is not None:
            signal = np.ascontiguousarray(signal, dtype=_lib.SIGNAL_DTYPE)
            assert signal.shape == (n,)
        cap = n if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=LONG_FRAME_DTYPE)
        out_c = np.zeros(max(cap, 1), dtype=np.int32)
        first = np.zeros(cap + 1, dtype=np.int32)
        members = np.zeros(max(n, 1), dtype=_lib.HEARER_DTYPE)
        got, nm = C.c_int(), C.c_int()
        if signal is None:
            rc = self._lib.gnuais_long_uniq_push_heard(self._h, frames.ctypes.data, n, int(rows), out.ctypes.data,
                                                       out_c.ctypes.data, cap, C.byref(got), first.ctypes.data,
                                                       members.ctypes.data, C.byref(nm))
        else:
            rc = self._lib.gnuais_long_uniq_push_heard_signal(self._h, frames.ctypes.data, signal.ctypes.data, n, int(rows),
                                                              out.ctypes.data, out_c.ctypes.data, cap, C.byref(got),
                                                              first.ctypes.data, members.ctypes.data, C.byref(nm))
        if rc != _lib.OK:
            raise _lib.GnuaisError(rc, "gnuais_long_uniq_push_heard: argument, or more records than cap")
        return out[: got.value].copy(), out_c[: got.value].copy(), first[: got.value + 1].copy(), members[: nm.value].copy()
