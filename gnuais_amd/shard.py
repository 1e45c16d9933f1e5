"""Channel sharding over the GPUs of one node.

Channels are independent receivers (reference src/ais.c:141-147 creates one
struct receiver per channel, nothing is shared), so the path shards with NO
data-path collective: GPU g owns the contiguous block [g*N/G, (g+1)*N/G) of the
interleaved channel axis and runs its own batch.  torch.distributed is used only
for the benchmark's barrier and for reducing per-rank timings and counters.
"""
from __future__ import annotations


def shard_range(n_channels: int, world: int, rank: int):
    """[lo, hi) of rank's contiguous channel block; blocks tile [0, n_channels)."""
    assert 0 <= rank < world and n_channels >= 0
    return n_channels * rank // world, n_channels * (rank + 1) // world


def reduce_bench(dist, device, seconds: float, msgs: float, samples: float):
    """max over ranks of the elapsed time, sums of messages and samples."""
    import torch
    t = torch.tensor([seconds], dtype=torch.float64, device=device)
    s = torch.tensor([msgs, samples], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(s, op=dist.ReduceOp.SUM)
    return float(t.item()), float(s[0].item()), float(s[1].item())


class ReceiverNode:
    """ctypes face of the node object (include/gnuais_hip.h: gnuais_node_*; gnuais_amd/csrc/node.hip): N channels in
    contiguous blocks over `devices`, one batch and one host thread per device inside the library, results merged in
    the reference's order with global channel numbers.  The product path of BASELINE's C4."""

    def __init__(self, n_channels: int, devices=None, taps=None, pllinc: int = 0, max_len: int = 48000,
                 frame_capacity: int = 0):
        import ctypes as C
        import numpy as np
        from .lib import check, load
        self._C, self._np, self._check = C, np, check
        self._lib = load()
        self._h = C.c_void_p()
        dv = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        tp = None if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
        rc = self._lib.gnuais_node_create(C.byref(self._h), None if dv is None else dv.ctypes.data,
                                          0 if dv is None else len(dv), n_channels,
                                          None if tp is None else tp.ctypes.data, 0 if tp is None else len(tp),
                                          pllinc, max_len, frame_capacity)
        self._raise(rc)
        self.n_channels, self.max_len = n_channels, max_len
        self.shards = []
        for i in range(self._lib.gnuais_node_n_devices(self._h)):
            d, f, n = C.c_int(), C.c_int(), C.c_int()
            self._lib.gnuais_node_shard(self._h, i, C.byref(d), C.byref(f), C.byref(n), None)
            self.shards.append((d.value, f.value, n.value))

    def _raise(self, rc, allow=()):
        if rc != 0 and rc not in allow:
            from .lib import GnuaisError
            raise GnuaisError(rc, self._lib.gnuais_node_last_error().decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gnuais_node_destroy(self._h)
            self._h = None

    __del__ = close

    def run_host(self, samples):
        self._run_host(samples, lambda x: x.ndim == 2 and x.shape[1] == self.n_channels, self._lib.gnuais_node_run_host)

    def run_iq_host(self, samples):
        """Complex baseband in (gnuais_node_run_iq_host): one host array int16 [len][n_channels][2] of (I, Q) pairs."""
        self._run_host(samples, lambda x: x.ndim == 3 and x.shape[1] == self.n_channels and x.shape[2] == 2,
                       self._lib.gnuais_node_run_iq_host)

    def _wide_configure(self, fn, ratio, in_rate_hz, offsets_hz, taps):
        np = self._np
        off = np.ascontiguousarray(offsets_hz, dtype=np.int32)
        t = None if taps is None else np.ascontiguousarray(taps, dtype=np.int16)
        self._raise(fn(self._h, *ratio, int(in_rate_hz), off.ctypes.data, int(off.size),
                       None if t is None else t.ctypes.data, 0 if t is None else int(t.size)))
        self._chan_k = int(off.size)

    def channeliser(self, decim: int, in_rate_hz: int, offsets_hz, taps=None):
        """Wideband in (gnuais_node_channeliser): ReceiverBatch.channeliser on every shard; every shard's first channel
        and channel count must be multiples of len(offsets_hz)."""
        self._wide_configure(self._lib.gnuais_node_channeliser, (int(decim),), in_rate_hz, offsets_hz, taps)

    def resampler(self, up: int, down: int, in_rate_hz: int, offsets_hz, taps=None):
        """Wideband in at a rational ratio (gnuais_node_resampler): ReceiverBatch.resampler on every shard, under
        channeliser()'s rule for the shards."""
        self._wide_configure(self._lib.gnuais_node_resampler, (int(up), int(down)), in_rate_hz, offsets_hz, taps)

    def afc(self, window: int):
        """Carrier-error correction of I/Q input (gnuais_node_afc): ReceiverBatch.afc on every shard."""
        self._raise(self._lib.gnuais_node_afc(self._h, int(window)))

    def run_wideband_host(self, samples):
        """Wideband in (gnuais_node_run_wideband_host): one host array int16 [len][n_channels / K][2] of wide streams."""
        k = getattr(self, "_chan_k", 1)
        self._run_host(samples, lambda x: x.ndim == 3 and x.shape[1] * k == self.n_channels and x.shape[2] == 2,
                       self._lib.gnuais_node_run_wideband_host)

    def run_wideband_fmt_host(self, samples, fmt: str):
        """Wideband in from an SDR's own sample format (gnuais_node_run_wideband_fmt_host): one host array
        [len][n_channels / K][2] in the dtype of fmt ("cs16", "cu8", "cs8", "cf32"), split and copied in its native bytes."""
        from . import lib as _lib
        value, dtype = _lib.FORMATS[fmt]
        if not isinstance(samples, self._np.ndarray) or samples.dtype != dtype:
            raise TypeError(f"fmt={fmt!r} takes a numpy array of {dtype}")
        x = self._np.ascontiguousarray(samples)
        k = getattr(self, "_chan_k", 1)
        assert x.ndim == 3 and x.shape[1] * k == self.n_channels and x.shape[2] == 2
        self._raise(self._lib.gnuais_node_run_wideband_fmt_host(self._h, value, x.ctypes.data, int(x.shape[0])))

    def _run_host(self, samples, shape_ok, fn):
        """run_host / run_iq_host / run_wideband_host: `fn` on one host array"""
        x = self._np.ascontiguousarray(samples, dtype=self._np.int16)
        assert shape_ok(x)
        self._raise(fn(self._h, x.ctypes.data, int(x.shape[0])))

    def run_iq(self, slabs, streams=None):
        """slabs: one CUDA/HIP int16 tensor [len][n_i][2] of (I, Q) pairs per shard, each on its shard's device."""
        self._run_slabs(slabs, streams, (2,), self._lib.gnuais_node_run_iq)

    def run(self, slabs, streams=None):
        """slabs: one CUDA/HIP int16 tensor [len][n_i] per shard, each on its shard's device."""
        self._run_slabs(slabs, streams, (), self._lib.gnuais_node_run)

    def _run_slabs(self, slabs, streams, tail, fn):
        """run / run_iq: `fn` on one device slab [len][n_i] + tail per shard"""
        C = self._C
        assert len(slabs) == len(self.shards)
        ln = int(slabs[0].shape[0])
        for t, (d, f, n) in zip(slabs, self.shards):
            assert t.is_cuda and t.is_contiguous() and tuple(t.shape) == (ln, n) + tail and t.device.index == d
        ptrs = (C.c_void_p * len(slabs))(*[t.data_ptr() for t in slabs])
        st = None if streams is None else (C.c_void_p * len(slabs))(*streams)
        self._raise(fn(self._h, ptrs, ln, st))

    def autotune(self, slabs, streams=None) -> float:
        C = self._C
        ptrs = (C.c_void_p * len(slabs))(*[t.data_ptr() for t in slabs])
        st = None if streams is None else (C.c_void_p * len(slabs))(*streams)
        ms = C.c_float(0)
        self._raise(self._lib.gnuais_node_autotune(self._h, ptrs, int(slabs[0].shape[0]), st, C.byref(ms)))
        return ms.value

    def sync(self):
        self._raise(self._lib.gnuais_node_sync(self._h))

    def set_option(self, name: str, value: int):
        self._raise(self._lib.gnuais_node_set_option(self._h, name.encode(), int(value)))

    def reset(self):
        self._raise(self._lib.gnuais_node_reset(self._h))

    def pending_frames(self) -> int:
        n = self._C.c_int()
        self._raise(self._lib.gnuais_node_pending_frames(self._h, self._C.byref(n)))
        return n.value

    def stream_nmea(self):
        """gnuais_node_stream_nmea(): call after every run(); -> (sentences of every shard in shard order = the node's
        text for the call `stream_depth` calls ago, sentences, frames); frames == -1 while the pipelines fill.
        If a shard fails, the GnuaisError raised carries what the others delivered as `.partial` (bytes)."""
        C = self._C
        n = len(self.shards)
        texts, lens = (C.c_void_p * n)(), (C.c_size_t * n)()
        ns, nf = C.c_int(0), C.c_int(0)
        rc = self._lib.gnuais_node_stream_nmea(self._h, texts, lens, C.byref(ns), C.byref(nf))
        out = b"".join(C.string_at(texts[i], lens[i]) for i in range(n) if texts[i] and lens[i])
        try:
            self._raise(rc)
        except Exception as e:
            e.partial = out
            raise
        return out, ns.value, nf.value

    def mark(self):
        """start a per-shard measurement (gnuais_node_mark)"""
        self._raise(self._lib.gnuais_node_mark(self._h))

    def warnings(self):
        """what gnuais_node_create() could not do without failing (unpinned host threads), one text per shard"""
        return [l for l in self._lib.gnuais_node_warnings(self._h).decode().splitlines() if l]

    def shard_stats(self):
        """after sync(): per shard, where its host thread runs and how long it was busy since mark()"""
        C = self._C

        class Stat(C.Structure):
            _fields_ = [("device", C.c_int32), ("first_channel", C.c_int32), ("n_channels", C.c_int32),
                        ("numa_node", C.c_int32), ("pinned_cpus", C.c_int32), ("calls", C.c_longlong),
                        ("submit_ms", C.c_double), ("busy_ms", C.c_double), ("pci", C.c_char * 32)]
        out = []
        for i in range(len(self.shards)):
            st = Stat()
            self._raise(self._lib.gnuais_node_shard_stats(self._h, i, C.byref(st)))
            out.append(dict(device=st.device, first_channel=st.first_channel, n_channels=st.n_channels,
                            pci=st.pci.decode(), numa_node=st.numa_node, pinned_cpus=st.pinned_cpus, calls=st.calls,
                            submit_ms=st.submit_ms, busy_ms=st.busy_ms))
        return out

    def discard_frames(self):
        self._raise(self._lib.gnuais_node_discard_frames(self._h))

    def drain_frames(self):
        from .lib import FRAME_DTYPE
        out = self._np.zeros(max(self.pending_frames(), 1), dtype=FRAME_DTYPE)
        got = self._C.c_int()
        self._raise(self._lib.gnuais_node_drain_frames(self._h, out.ctypes.data, len(out), self._C.byref(got)))
        return out[: got.value].copy()

    def frame_times(self, on: bool = True):
        """gnuais_batch_frame_times() on every shard"""
        self._raise(self._lib.gnuais_node_frame_times(self._h, int(bool(on))))

    def repair(self, on: bool = True):
        """gnuais_batch_repair() on every shard"""
        self._raise(self._lib.gnuais_node_repair(self._h, int(bool(on))))

    def repaired(self):
        """gnuais_node_repaired(): int32 [n_channels], the repairs per global channel"""
        out = self._np.zeros(self.n_channels, dtype=self._np.int32)
        self._raise(self._lib.gnuais_node_repaired(self._h, out.ctypes.data))
        return out

    def long_frames(self, on: bool = True):
        """gnuais_batch_long_frames() on every shard"""
        self._raise(self._lib.gnuais_node_long_frames(self._h, int(bool(on))))

    def drain_long_frames(self):
        """gnuais_node_drain_long_frames(): the long frames of every shard, global channel numbers, (channel, stamp) order.
        The node has no count of them: the buffer doubles until the call takes it (a refused call consumes nothing)."""
        from .lib import E_ARG, E_OVERFLOW, LONG_FRAME_DTYPE
        n = 1024
        while True:
            out = self._np.zeros(n, dtype=LONG_FRAME_DTYPE)
            got = self._C.c_int()
            rc = self._lib.gnuais_node_drain_long_frames(self._h, out.ctypes.data, n, self._C.byref(got))
            if rc == E_ARG and n < 1 << 24:
                n *= 4
                continue
            self._raise(rc)
            return out[: got.value].copy()

    def long_frame_signal(self, on: bool = True):
        """gnuais_batch_long_frame_signal() on every shard"""
        self._raise(self._lib.gnuais_node_long_frame_signal(self._h, int(bool(on))))

    def drain_long_frames_signal(self):
        """gnuais_node_drain_long_frames_signal(): (records, signal): drain_long_frames() with every record's power,
        carrier error and blocks (lib.SIGNAL_DTYPE)"""
        from .lib import E_ARG, LONG_FRAME_DTYPE, SIGNAL_DTYPE
        n = 1024
        while True:
            out = self._np.zeros(n, dtype=LONG_FRAME_DTYPE)
            sig = self._np.zeros(n, dtype=SIGNAL_DTYPE)
            got = self._C.c_int()
            rc = self._lib.gnuais_node_drain_long_frames_signal(self._h, out.ctypes.data, sig.ctypes.data, n, self._C.byref(got))
            if rc == E_ARG and n < 1 << 24:
                n *= 4
                continue
            self._raise(rc)
            return out[: got.value].copy(), sig[: got.value].copy()

    def long_counters(self):
        """gnuais_node_long_counters(): (delivered, failed), int32 [n_channels] each, per global channel"""
        d = self._np.zeros(self.n_channels, dtype=self._np.int32)
        f = self._np.zeros(self.n_channels, dtype=self._np.int32)
        self._raise(self._lib.gnuais_node_long_counters(self._h, d.ctypes.data, f.ctypes.data))
        return d, f

    def long_repair(self, on: bool = True):
        """gnuais_batch_long_repair() on every shard"""
        self._raise(self._lib.gnuais_node_long_repair(self._h, int(bool(on))))

    def long_repaired(self):
        """gnuais_node_long_repaired(): int32 [n_channels], the long frames repaired per global channel"""
        out = self._np.zeros(self.n_channels, dtype=self._np.int32)
        self._raise(self._lib.gnuais_node_long_repaired(self._h, out.ctypes.data))
        return out

    def drain_frames_timed(self):
        """gnuais_node_drain_frames_timed(): (frames, int64 times), as drain_frames with every record's receive time"""
        from .lib import FRAME_DTYPE
        n = max(self.pending_frames(), 1)
        out, times = self._np.zeros(n, dtype=FRAME_DTYPE), self._np.zeros(n, dtype=self._np.int64)
        got = self._C.c_int()
        self._raise(self._lib.gnuais_node_drain_frames_timed(self._h, out.ctypes.data, times.ctypes.data, n,
                                                             self._C.byref(got)))
        return out[: got.value].copy(), times[: got.value].copy()

    def frame_signal(self, on: bool = True):
        """gnuais_batch_frame_signal() on every shard"""
        self._raise(self._lib.gnuais_node_frame_signal(self._h, int(bool(on))))

    def drain_frames_signal(self):
        """gnuais_node_drain_frames_signal(): (frames, int64 times, signal), as drain_frames_timed with every record's
        power, carrier error and blocks (lib.SIGNAL_DTYPE)"""
        from .lib import FRAME_DTYPE, SIGNAL_DTYPE
        np_ = self._np
        n = max(self.pending_frames(), 1)
        out, times, sig = np_.zeros(n, dtype=FRAME_DTYPE), np_.zeros(n, dtype=np_.int64), np_.zeros(n, dtype=SIGNAL_DTYPE)
        got = self._C.c_int()
        self._raise(self._lib.gnuais_node_drain_frames_signal(self._h, out.ctypes.data, times.ctypes.data, sig.ctypes.data,
                                                              n, self._C.byref(got)))
        return out[: got.value].copy(), times[: got.value].copy(), sig[: got.value].copy()

    def occupancy(self, epoch_blocks: int = 1024, margin: int = 16):
        """gnuais_batch_occupancy() on every shard"""
        self._raise(self._lib.gnuais_node_occupancy(self._h, int(epoch_blocks), int(margin)))

    def drain_occupancy(self):
        """gnuais_node_drain_occupancy(): (int64 first_block[n], records[n][n_channels]) of the final epochs, the shards'
        records side by side by global channel (lib.OCCUPANCY_DTYPE)"""
        from .lib import OCCUPANCY_DTYPE, OCCUPANCY_EPOCHS_HELD
        np_, n = self._np, OCCUPANCY_EPOCHS_HELD
        rec, first = np_.zeros((n, self.n_channels), dtype=OCCUPANCY_DTYPE), np_.zeros(n, dtype=np_.int64)
        got = self._C.c_int()
        self._raise(self._lib.gnuais_node_drain_occupancy(self._h, rec.ctypes.data, first.ctypes.data, n, self._C.byref(got)))
        return first[: got.value].copy(), rec[: got.value].copy()

    def unique(self, window: int):
        """gnuais_node_unique(): each transmission once over the whole node (merged on the host: the shards exchange
        nothing); window in rows, 0 = off.  Needs frame_times()."""
        self._raise(self._lib.gnuais_node_unique(self._h, int(window)))

    def drain_frames_unique(self):
        """gnuais_node_drain_frames_unique(): (frames, int64 times, int32 copies), one record per transmission"""
        from .lib import FRAME_DTYPE
        np_ = self._np
        n = max(self.pending_frames(), 1)
        out, times, copies = np_.zeros(n, dtype=FRAME_DTYPE), np_.zeros(n, dtype=np_.int64), np_.zeros(n, dtype=np_.int32)
        got = self._C.c_int()
        self._raise(self._lib.gnuais_node_drain_frames_unique(self._h, out.ctypes.data, times.ctypes.data,
                                                              copies.ctypes.data, n, self._C.byref(got)))
        return out[: got.value].copy(), times[: got.value].copy(), copies[: got.value].copy()

    def drain_frames_heard(self):
        """gnuais_node_drain_frames_heard(): (frames, int64 times, int32 copies, int32 first, members): the unique drain
        and, per transmission, the receivers that heard it (lib.HEARER_DTYPE, global channel numbers)"""
        from .lib import FRAME_DTYPE, HEARER_DTYPE
        np_ = self._np
        n = max(self.pending_frames(), 1)
        out, times, copies = np_.zeros(n, dtype=FRAME_DTYPE), np_.zeros(n, dtype=np_.int64), np_.zeros(n, dtype=np_.int32)
        first, members = np_.zeros(n + 1, dtype=np_.int32), np_.zeros(n, dtype=HEARER_DTYPE)
        got, nm = self._C.c_int(), self._C.c_int()
        self._raise(self._lib.gnuais_node_drain_frames_heard(self._h, out.ctypes.data, times.ctypes.data, copies.ctypes.data,
                                                             n, self._C.byref(got), first.ctypes.data, members.ctypes.data,
                                                             self._C.byref(nm)))
        return (out[: got.value].copy(), times[: got.value].copy(), copies[: got.value].copy(),
                first[: got.value + 1].copy(), members[: nm.value].copy())

    def unique_late(self) -> int:
        t = self._C.c_longlong()
        self._raise(self._lib.gnuais_node_unique_late(self._h, self._C.byref(t)))
        return t.value

    def long_unique(self, window: int):
        """gnuais_node_long_unique(): each long transmission once over the whole node (the shards' long drains merged on
        the host); window in rows, 0 = off.  Needs long_frames()."""
        self._raise(self._lib.gnuais_node_long_unique(self._h, int(window)))

    def _drain_long_merged(self, heard: bool):
        """the node has no count of its long frames: the buffers double until the call takes them (a refused call
        consumes nothing)"""
        from .lib import E_ARG, HEARER_DTYPE, LONG_FRAME_DTYPE
        np_, n = self._np, 1024
        while True:
            out, copies = np_.zeros(n, dtype=LONG_FRAME_DTYPE), np_.zeros(n, dtype=np_.int32)
            first, members = np_.zeros(n + 1, dtype=np_.int32), np_.zeros(n, dtype=HEARER_DTYPE)
            got, nm = self._C.c_int(), self._C.c_int()
            if heard:
                rc = self._lib.gnuais_node_drain_long_frames_heard(self._h, out.ctypes.data, copies.ctypes.data, n,
                                                                   self._C.byref(got), first.ctypes.data,
                                                                   members.ctypes.data, self._C.byref(nm))
            else:
                rc = self._lib.gnuais_node_drain_long_frames_unique(self._h, out.ctypes.data, copies.ctypes.data, n,
                                                                    self._C.byref(got))
            if rc == E_ARG and n < 1 << 24:
                n *= 4
                continue
            self._raise(rc)
            res = (out[: got.value].copy(), copies[: got.value].copy())
            return res + (first[: got.value + 1].copy(), members[: nm.value].copy()) if heard else res

    def drain_long_frames_unique(self):
        """gnuais_node_drain_long_frames_unique(): (records, int32 copies), one record per long transmission"""
        return self._drain_long_merged(False)

    def drain_long_frames_heard(self):
        """gnuais_node_drain_long_frames_heard(): (records, int32 copies, int32 first, members): the unique drain and, per
        transmission, the receivers that heard it (lib.HEARER_DTYPE, global channel numbers)"""
        return self._drain_long_merged(True)

    def long_unique_late(self) -> int:
        t = self._C.c_longlong()
        self._raise(self._lib.gnuais_node_long_unique_late(self._h, self._C.byref(t)))
        return t.value

    def time_map(self, kind: str = "audio"):
        """gnuais_batch_time_map() of the first shard: every shard has the node's configuration"""
        from .lib import INPUT_KINDS, check
        C = self._C
        dev, first, n, bh = C.c_int(), C.c_int(), C.c_int(), C.c_void_p()
        self._raise(self._lib.gnuais_node_shard(self._h, 0, C.byref(dev), C.byref(first), C.byref(n), C.byref(bh)))
        mul, off = C.c_longlong(0), C.c_longlong(0)
        check(self._lib.gnuais_batch_time_map(bh, INPUT_KINDS[kind], C.byref(mul), C.byref(off)))
        return mul.value, off.value

    def time_map_ratio(self, kind: str = "audio"):
        """gnuais_batch_time_map_ratio() of the first shard: (num, den, off), index = (t * num + off) // den"""
        from .lib import INPUT_KINDS, check
        C = self._C
        dev, first, n, bh = C.c_int(), C.c_int(), C.c_int(), C.c_void_p()
        self._raise(self._lib.gnuais_node_shard(self._h, 0, C.byref(dev), C.byref(first), C.byref(n), C.byref(bh)))
        num, den, off = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        check(self._lib.gnuais_batch_time_map_ratio(bh, INPUT_KINDS[kind], C.byref(num), C.byref(den), C.byref(off)))
        return num.value, den.value, off.value

    def counters(self):
        from .lib import COUNTERS_DTYPE
        out = self._np.zeros(self.n_channels, dtype=COUNTERS_DTYPE)
        self._raise(self._lib.gnuais_node_counters(self._h, out.ctypes.data))
        return out

    def total_received(self) -> int:
        t = self._C.c_longlong()
        self._raise(self._lib.gnuais_node_total_received(self._h, self._C.byref(t)))
        return t.value

    def maxval(self):
        out = self._np.zeros(self.n_channels, dtype=self._np.int16)
        self._raise(self._lib.gnuais_node_maxval(self._h, out.ctypes.data))
        return out

    def pll_state(self):
        from .lib import PLL_DTYPE
        out = self._np.zeros(self.n_channels, dtype=PLL_DTYPE)
        self._raise(self._lib.gnuais_node_pll_state(self._h, out.ctypes.data))
        return out
