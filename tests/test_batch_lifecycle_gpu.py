"""A batch gives back what it took: device memory after repeated create / use / destroy cycles.

One cycle creates a batch, takes it through every entry that allocates on first use or re-allocates on
re-configuration (the hand-off sets of nbuf = 8, the staging buffers of the host entries, the I/Q, AFC and channeliser
intermediates, the post-stage scratch of the drains, the carried vessel table, the rings, texts, events and the copy
stream of the streamed delivery) and destroys it.  A second kind of cycle is a create that the library refuses after it
has begun to allocate.  The library allocates with hipMalloc directly, so the device's free memory
(torch.cuda.mem_get_info) after a cycle shows what the cycle kept; torch's own tensors are made once, before the first
reading.

What the reading can see: free memory moves in steps of 2 MiB, and hipMalloc serves small requests out of blocks it
keeps.  A field of about a MB or more that is not released shows every cycle: with one slot's device text (2.0 MB,
sd_text[1]) taken out of its owner by hand, free memory fell by 2 MiB in each of the four steps and the test failed
with 8 MiB.  A field below that granularity need not show within five cycles: with d_word (16 bytes, the smallest
buffer a cycle allocates) taken out the same way, one run showed a single 2 MiB step, which is not something to rely on;
the same holds for the counters, sequence digits and tables of a few KB.
"""
import numpy as np
import pytest

from gnuais_amd import synth

pytestmark = pytest.mark.gpu

N_CH, ROWS, DECIM = 256, 6 * 1280, 4
# How far free memory after the last of the CYCLES measured cycles may lie below free memory after the first of them.
# Measured on the parent commit (a destroy that frees a hand-kept list, believed complete) on one MI355X: 0 bytes, so the
# slack is 0 (profiles/batch_lifecycle_vs_parent.txt).  The reading after the warm-up cycle is printed and not compared:
# in a fresh process the runtime takes another 80 MiB during the cycle after the warm-up, on the parent as well, and
# nothing from then on.
SLACK_BYTES = 0
CYCLES = 5


def _inputs():
    import torch
    base = np.stack([synth.make_stream(ROWS, seed=11, channel=c, occupancy=0.8)[0] for c in range(32)], axis=1)
    audio = np.ascontiguousarray(np.tile(base, (1, N_CH // 32)))
    rng = np.random.default_rng(5)
    iq = rng.integers(-20000, 20000, (1280, N_CH, 2), dtype=np.int16)
    wide = rng.integers(-20000, 20000, (1280 * DECIM, N_CH // 2, 2), dtype=np.int16)
    host = {"audio": audio, "iq": iq, "wide": wide}
    return host, {k: torch.from_numpy(v).cuda() for k, v in host.items()}


def _cycle(host, dev):
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import check
    b = ReceiverBatch(N_CH, max_len=ROWS)
    b.set_option("nbuf", 8)
    seq = np.zeros(N_CH, dtype=np.uint8)
    # audio: device entry, host entry, the pinned double-buffered host entry (two sizes: its buffers are re-made)
    b.run(dev["audio"])
    assert len(b.drain_frames()) > 0
    b.run(host["audio"])
    assert b.drain_nmea(seq)[2] > 0
    b.run_host_async(host["audio"][:1280])
    b.run_host_async(host["audio"])
    b.sync()
    assert len(b.fold_vessels()) >= 0
    b.vessel_table_enable(1000)
    b.vessel_table_update()
    assert b.drain_messages(seq)[4] > 0
    b.vessel_table()
    b.vessel_table_enable(5000)                         # another size: the table is re-made
    out = np.zeros((1280, N_CH), dtype=np.float32)
    check(b._lib.gnuais_batch_filter_host(b._h, host["audio"].ctypes.data, 1280, out.ctypes.data))
    # I/Q with the AFC on, wideband through the channeliser: device and host entries
    b.afc(1024)
    b.run_iq(dev["iq"])
    b.run_iq(host["iq"])
    b.channeliser(DECIM, 48000 * DECIM, [-25000, 25000])
    b.run_wideband(dev["wide"])
    b.run_wideband(host["wide"])
    b.drain_frames_nmea(seq)
    # streamed delivery: more calls than the ring is deep, then back
    b.on_overflow = "keep"
    for _ in range(b.stream_depth + 3):
        b.run(dev["audio"], sync=False)
        b.stream_nmea()
    b.set_option("streaming", 0)
    b.vessel_table()
    # re-configuration: another window, then off; other taps
    b.afc(2048)
    b.run_iq(dev["iq"])
    b.afc(0)
    b.channeliser(DECIM, 48000 * DECIM, [-25000, 25000], taps=np.array([100, 2000, 9000, 2000, 100], dtype=np.int16))
    b.run_wideband(dev["wide"])
    b.drain_frames()
    b.close()


def _refused_create():
    """refused after the FIR histories are allocated: the half-built batch has to release them"""
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import GnuaisError
    with pytest.raises(GnuaisError, match="pllinc too large"):
        ReceiverBatch(N_CH, pllinc=0x8000, max_len=ROWS)


def test_cycles_of_use_and_refused_creates_return_their_device_memory():
    import torch
    host, dev = _inputs()

    def free_after_cycle():
        _cycle(host, dev)
        _refused_create()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    first = free_after_cycle()                          # warm-up: the runtime's own one-time allocations are in here
    free = [free_after_cycle() for _ in range(CYCLES)]
    print(f"free device memory after the warm-up cycle {first}, after each of {CYCLES} more {free}; "
          f"from the first of them to the last it fell by {free[0] - free[-1]} bytes (slack {SLACK_BYTES})")
    assert free[0] - free[-1] <= SLACK_BYTES, (first, free)
