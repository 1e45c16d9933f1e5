"""The rational channeliser's configuration matrix, shared by the CPU tests (tests/test_resampler_cpu.py) and the device
tests (tests/test_resampler_gpu.py): the smallest shapes at which the wide stage's rational form can go wrong.  It reaches
every channeliser_kernel<K, 17, F, true> instance, the direct form and the carry copy of every format.

  ratios   2/3 (groups of 2 and 1: the lone-sample pair), 5/6, 3/64, 3/128 (groups of 43, 43, 42), 24/125, 1/65 (U = 1)
  streams  1, 3, 65 (a partial second wave), 130 (two stream groups and a partial third)
  offsets  K = 1..4 on the fast form, K = 5 on the direct form
  taps     the default design (T = 16 D + 1, ceil(T / D) = 17), and custom prototypes with T at both edges of the one
           fast bucket (T = 1: no carry at all; T = 17 D) and one past it (T = 17 D + 1: the direct form)
  calls    in periods of D wide samples: one period (U rows), three, a call shorter than the carry (1 period at 3/128:
           128 < H = 683), one of at least 257 rows (three segments of 128 rows and their halos), a reset in the middle
"""
import dataclasses

import numpy as np

import resample_ref

RATIOS = [(2, 3), (5, 6), (3, 64), (3, 128), (24, 125)]
# the ratios of the CPU tests of the host functions
HOST_RATIOS = [(2, 3), (5, 6), (3, 64), (3, 128), (24, 125), (12, 625)]
OFFS = {1: [25000], 2: [-25000, 25000], 3: [-25000, 25000, 12000], 4: [-25000, 25000, 12000, 0],
        5: [-25000, 25000, 12000, 0, -7000]}
FORMATS = ("cs16", "cu8", "cs8", "cf32")
FMT_VALUE = {"cs16": 0, "cu8": 1, "cs8": 2, "cf32": 3}


def bounded_taps(rng, up: int, T: int) -> np.ndarray:
    """a random asymmetric prototype of T taps whose per-phase sums |h| lie just under the bound, one phase exactly at
    65535 where it has at least two taps"""
    h = np.zeros(T, dtype=np.int64)
    for phi in range(min(up, T)):
        n = len(range(phi, T, up))
        v = rng.integers(-32767, 32768, n)
        s = max(int(np.abs(v).sum()), 1)
        if s > 65000:
            v = (v * (65000.0 / s)).astype(np.int64)
        h[phi::up] = v
    if T >= 2 * up:                                       # phase 0 exactly on the bound
        v = h[0::up]
        room = 65535 - int(np.abs(v).sum())
        i = int(np.argmin(np.abs(v)))
        v[i] += room if v[i] >= 0 else -room
        assert abs(v[i]) <= 32767
        h[0::up] = v
        assert int(np.abs(h[0::up]).sum()) == 65535
    return h.astype(np.int16)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    up: int
    down: int
    M: int
    K: int
    periods: tuple                   # the calls, in periods of `down` wide samples; 0 = a reset between two calls
    T: int = 0                       # 0: the default design; else a bounded_taps() prototype of T taps

    @property
    def rate(self):
        return 48000 * self.down // self.up if (48000 * self.down) % self.up == 0 else 1000 * self.down

    @property
    def offsets(self):
        return OFFS[self.K]

    @property
    def taps(self):
        if not self.T:
            return resample_ref.default_taps(self.up, self.down)
        return bounded_taps(np.random.default_rng(self.T * 131 + self.up), self.up, self.T)

    @property
    def n_taps(self):
        return self.T or 16 * self.down + 1

    @property
    def na(self):
        return resample_ref.fast_na(self.K, self.n_taps, self.down)

    @property
    def max_rows(self):
        return max(self.periods) * self.up


CASES = [
    Case("r2_3_m3_k2", 2, 3, 3, 2, (1, 3, 200, 0, 5, 1)),
    Case("r2_3_m65_k5_direct", 2, 3, 65, 5, (1, 3, 70)),
    Case("r5_6_m65_k1", 5, 6, 65, 1, (1, 3, 60, 0, 2)),
    Case("r3_64_m1_k3", 3, 64, 1, 3, (1, 3, 90)),
    Case("r3_128_m130_k2", 3, 128, 130, 2, (1, 3, 0, 2, 88)),
    Case("r3_128_m3_k5_direct", 3, 128, 3, 5, (1, 3, 6)),
    Case("r24_125_m3_k4", 24, 125, 3, 4, (1, 3, 11, 0, 1)),
    Case("r3_64_T1", 3, 64, 3, 2, (1, 3, 2), T=1),
    Case("r3_64_T1088_fast_edge", 3, 64, 3, 2, (1, 3, 44), T=17 * 64),
    Case("r3_64_T1089_direct", 3, 64, 3, 2, (1, 3, 5), T=17 * 64 + 1),
    # U = 1 past the integer entry's D <= 64: the edge between the two configurations (one group of 65; the carry is
    # 1040 rows, so a one-period call is shorter than it)
    Case("r1_65_m3_k2", 1, 65, 3, 2, (1, 3, 20, 0, 2)),
    Case("r1_65_m3_k5_direct", 1, 65, 3, 5, (1, 3, 6)),
]
CASE_IDS = [c.name for c in CASES]

# every format on 3/128 (K = 2) and on 2/3 at every K: all instances of the fast form, the direct form (K = 5) and the
# carry copy of each format
FORMAT_CASES = [(fmt, Case(f"{fmt}_r3_128_k2", 3, 128, 3, 2, (1, 3, 2))) for fmt in FORMATS] + \
               [(fmt, Case(f"{fmt}_r2_3_k{K}" + ("_direct" if K == 5 else ""), 2, 3, 3, K, (1, 3, 70)))
                for fmt in FORMATS for K in (1, 2, 3, 4, 5)]
FORMAT_IDS = [c.name for _, c in FORMAT_CASES]


def instances_reached():
    """the (K, NA, format value) instances of the fast form the matrix launches, and the formats of its direct calls"""
    fast, direct = set(), set()
    for c in CASES:
        (fast.add((c.K, c.na, 0)) if c.na else direct.add(0))
    for fmt, c in FORMAT_CASES:
        (fast.add((c.K, c.na, FMT_VALUE[fmt])) if c.na else direct.add(FMT_VALUE[fmt]))
    return fast, direct


for _c in CASES:
    resample_ref.check_config(_c.up, _c.down)
    assert (_c.na == 0) == ("direct" in _c.name), _c.name
