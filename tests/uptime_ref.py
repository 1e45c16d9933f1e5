"""The clocks of a long-running receiver, away from zero (TEST INFRASTRUCTURE shared by tests/test_uptime_cpu.py and
tests/test_uptime_gpu.py; the entry that moves them is gnuais_batch_set_clock in include/gnuais_hip.h).

No stage is modelled anew here.  The restatements take absolute positions already -- frame_time_ref.FrameTimeRef(rows,
bits), frame_signal_ref.FrameSignalRef(rows, bits) / BlockSums(base), occupancy_ref.OccupancyRef.run_iq(n0, ..),
unique_ref.UniqueRef.push(.., rows) -- and the CPU oracle always starts at zero.  What this file adds is the list of
origins every test uses, and the shift that turns the oracle's records into those of a receiver whose deframer had
bits[c] bits behind it:

  shift_frames(frames, bits)   the 37-bit stamp (bits[channel] + stamp) mod 2^37 into end_bit and flags bits 5:1;
                               everything else, and the ORDER, as the oracle gave them.  The order within a drain is
                               (channel, time), i.e. (channel, stamp) only while the stamp has not wrapped; taking it from
                               the oracle at origin zero instead of sorting the shifted stamps is what catches a device
                               sort on a broken key.

  ROWS     2^31 - 3840, 2^32 - 3840: with three calls of 7680 rows the carry falls inside call 1;
           2^32 - 7680: exactly on the seam of calls 1 and 2;  2^40 + 256: nowhere, every row needs 41 bits.
           All are multiples of 256, so blocks of 64 rows and epochs of 4 blocks stay aligned to the origin: a run at
           origin R gives what the run at 0 gives with every time + R and every block index + R / 64
           (tests/test_uptime_cpu.py shows it for the restatements on the CPU).
  bits     per channel and per test: sweep() puts the carry of channel c at bit p0 + step * c of the stream.
"""
import numpy as np

from frame_time_ref import M37, shift_frames, stamp  # noqa: F401  (shift_frames lives beside stamp(); this is its public name)

CALL = 7680
ROWS = (2 ** 31 - 3840, 2 ** 32 - 3840, 2 ** 32 - 7680, 2 ** 40 + 256)
CARRY32, CARRY37 = 1 << 32, 1 << 37


def origins():
    """the rows origins of every test"""
    return list(ROWS)


def sweep(n_ch: int, p0: int, carry: int = CARRY32, step: int = 1):
    """bits origins: channel c has fed carry - p0 - step * c bits, so its count reaches `carry` in front of bit
    p0 + step * c of what it is fed next; Python ints"""
    return [carry - p0 - step * c for c in range(n_ch)]


def after_carry(frames0: np.ndarray, bits, carry: int = CARRY32) -> np.ndarray:
    """per record of an origin-zero run: its closing bit has index >= carry at the bits origin (not reduced mod 2^37)"""
    b = np.asarray(bits, dtype=np.uint64).astype(np.int64)
    b = np.broadcast_to(b, (int(frames0["channel"].max()) + 1,)) if b.ndim == 0 else b
    return b[frames0["channel"].astype(np.int64)] + stamp(frames0) >= carry


def floors(frames0: np.ndarray, bits, n_ch: int, carry: int = CARRY32):
    """what keeps a test from passing empty, shown from the oracle alone: (frames per channel, frames per channel that
    close after the channel's carry)"""
    ch = frames0["channel"].astype(np.int64)
    return np.bincount(ch, minlength=n_ch), np.bincount(ch[after_carry(frames0, bits, carry)], minlength=n_ch)
