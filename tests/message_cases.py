"""Frame records that walk every number field of the message layer over its whole range (tests/test_message_cases_cpu.py
checks the builders, test_message_kernel_cpu.py and test_message_sweep_gpu.py feed them to nmea_device.hip).

Every builder is deterministic and returns FRAME_DTYPE records of whole bytes with flags = 1, spread over N_CH channels
in build order (channel = index mod N_CH, end_bit = index): in_print_order() gives the order the reference prints them in.
Bits no decoder reads come from a seeded generator.  The field offsets written here are the reference's decoders'
(src/protodec.c:357-776), restated; nothing of the library is used."""
import numpy as np

from oracle_lib import FRAME_DTYPE

N_CH = 8
MAX_BITS = 53 * 8
NAMES = ("positions", "positions_b", "edges", "type4", "weather", "lengths", "text", "longest")


class Payload:
    """424 bits, MSB first, as one integer"""

    def __init__(self, rng, msg_type, mmsi):
        self.v = rng if isinstance(rng, int) else int.from_bytes(rng.integers(0, 256, 53, dtype=np.uint8).tobytes(), "big")
        self.put(0, 6, msg_type)
        self.put(8, 30, mmsi)

    def put(self, pos, count, value):
        assert 0 <= pos and pos + count <= MAX_BITS
        sh = MAX_BITS - pos - count
        mask = ((1 << count) - 1) << sh
        self.v = (self.v & ~mask) | ((int(value) << sh) & mask)

    def text(self, pos, codes):
        for i, c in enumerate(codes):
            self.put(pos + 6 * i, 6, c)

    def record(self, nbytes):
        raw = np.frombuffer(self.v.to_bytes(53, "big"), dtype=np.uint8).copy()
        raw[nbytes:] = 0                            # the record keeps whole bytes only (protodec.c:133)
        return raw, 8 * nbytes


def _background(seed):
    """the bits no decoder reads: one seeded pattern for a whole group, so that the recorded text stays small"""
    return int.from_bytes(np.random.default_rng(seed).integers(0, 256, 53, dtype=np.uint8).tobytes(), "big")


def _records(rows):
    fr = np.zeros(len(rows), dtype=FRAME_DTYPE)
    for i, (raw, nbits) in enumerate(rows):
        fr[i]["channel"], fr[i]["end_bit"] = i % N_CH, i
        fr[i]["payload"], fr[i]["flags"], fr[i]["nbits"] = raw, 1, nbits
    return fr


def in_print_order(fr):
    """per channel, then time: what the reference prints and what the device's sort gives"""
    return fr[np.lexsort((fr["end_bit"], fr["channel"]))]


# ---- types 1-3 and 18 ---------------------------------------------------------------------------------------------
POS_A = dict(rot=40, sog=50, lon=61, lat=89, course=116, heading=128)      # protodec_pos
POS_B = dict(sog=46, lon=57, lat=85, course=112, heading=124)              # protodec_18


def _position(rng, msg_type, mmsi, lat, lon, course, sog, heading, rot=0):
    p = Payload(rng, msg_type, mmsi)
    o = POS_B if msg_type == 18 else POS_A
    if msg_type != 18:
        p.put(o["rot"], 8, rot)
    p.put(o["sog"], 10, sog)
    p.put(o["lon"], 28, lon & 0xfffffff)
    p.put(o["lat"], 27, lat & 0x7ffffff)
    p.put(o["course"], 12, course)
    p.put(o["heading"], 9, heading)
    return p.record(21)


def _sweep(k):
    return dict(lat=k - 2048, lon=(7 * k) % 4096 - 2048, course=k, sog=k % 1024, heading=k % 512, rot=k % 256)


def positions():
    """type 1 at every course 0..4095; speed, heading, turn rate and the coordinates -2048..2047 ride along"""
    rng = _background(1001)
    return _records([_position(rng, 1, 100000000 + k, **_sweep(k)) for k in range(4096)])


def positions_b():
    """types 2 and 3 on every 16th k of the same rule (the MMSIs of `positions`); type 18 at the 410 courses that end in
    5 -- the only exact ties of any %.0f / %.1f field -- and every 8th other course, its speed and heading by index"""
    rng = _background(1002)
    rows = []
    for t in (2, 3):
        rows += [_position(rng, t, 100000000 + k, **_sweep(k)) for k in range(t, 4096, 16)]
    ks = [k for k in range(4096) if k % 10 == 5 or k % 8 == 0]
    for j, k in enumerate(ks):
        s = _sweep(k)
        s.update(sog=j % 1024, heading=j % 512)
        rows.append(_position(rng, 18, 300000000 + j, **s))
    return _records(rows)


def edge_values(bits):
    """signed values of a `bits`-bit field: +-(2^k - 1), +-2^k, +-(2^k + 1) wherever they fit, both extremes, 91 and 181
    degrees, and values above 2^24 where int -> float rounds (ties to even among them)"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    vals = [0, lo, hi, 54600000, 108600000]
    for k in range(bits):
        for d in (-1, 0, 1):
            vals += [(1 << k) + d, -((1 << k) + d)]
    for v in ((1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6):
        vals += [v, -v]
    out = []
    for v in vals:
        if lo <= v <= hi and v not in out:
            out.append(v)
    return out


def _type4(rng, mmsi, lat, lon, year=2024, month=1, day=1, hour=0, minute=0, second=0):
    p = Payload(rng, 4, mmsi)
    for pos, cnt, v in ((40, 12, year), (52, 4, month), (56, 5, day), (61, 5, hour), (66, 6, minute), (72, 6, second)):
        p.put(pos, cnt, v)
    p.put(79, 28, lon & 0xfffffff)
    p.put(107, 27, lat & 0x7ffffff)
    return p.record(21)


def edges():
    """types 1, 18 and 4 with lat and lon at the edge values of their fields"""
    rng = _background(1003)
    la, lo = edge_values(27), edge_values(28)
    rows = []
    for i in range(len(lo)):
        lat, lon = la[i % len(la)], lo[(i * 5 + 3) % len(lo)]
        rows.append(_position(rng, 1, 400000000 + i, lat, lon, (i * 37) % 4096, i % 1024, i % 512, i % 256))
        rows.append(_position(rng, 18, 410000000 + i, lat, lon, (i * 41) % 4096, (i * 3) % 1024, i % 512))
        rows.append(_type4(rng, 420000000 + i, lat, lon, hour=i % 24, minute=i % 60, second=i % 60))
    return _records(rows)


def type4():
    """type 4: lat and lon over -600..600, the clock fields over their whole width, the year at its digit counts"""
    rng = _background(1004)
    rows = []
    for k in range(1201):
        rows.append(_type4(rng, 500000000 + k, k - 600, (7 * k) % 1201 - 600, year=(0, 9, 10, 4095)[k % 4],
                           month=k % 16, day=k % 32, hour=k % 32, minute=k % 64, second=(5 * k) % 64))
    return _records(rows)


# ---- the tide / weather report and persons on board (DAC 1, FI 11 / 40) inside types 6 and 8 -------------------------
def _binary(rng, msg_type, mmsi, fi, dst=0, seq=0, retx=0):
    p = Payload(rng, msg_type, mmsi)
    if msg_type == 6:
        p.put(38, 2, seq); p.put(40, 30, dst); p.put(70, 1, retx)
        p.put(72, 10, 1); p.put(82, 6, fi)
        return p, 88
    p.put(40, 10, 1); p.put(50, 6, fi)
    return p, 56


def unsigned_edges(bits):
    vals = list(range(601))
    for k in range(bits):
        for d in (-1, 0, 1):
            v = (1 << k) + d
            if 0 <= v < (1 << bits) and v not in vals:
                vals.append(v)
    vals.append((1 << bits) - 1)
    return vals


WEATHER_LAT, WEATHER_LON = unsigned_edges(24), unsigned_edges(25)
# lon's low nine bits are also wind and the top of gust: its all-ones value sits where the rule gives gust's low bits 31
_i = WEATHER_LON.index((1 << 25) - 1)
WEATHER_LON[_i], WEATHER_LON[31] = WEATHER_LON[31], WEATHER_LON[_i]


def weather_fields(k):
    """every field of the report from k.  The reference reads overlapping offsets (protodec_msg_11, :287-336): wind and
    the top two bits of gust are lon's low bits; wave is level's low four bits and wtemp's top four"""
    return dict(lat=WEATHER_LAT[k % len(WEATHER_LAT)], lon=WEATHER_LON[k % len(WEATHER_LON)], gust5=k % 32,
                wdir=k % 512, gdir=(3 * k) % 512, temp=k, hum=k % 128, dew=k % 1024, pres=(7 * k) % 512, tend=k % 4,
                vis=k % 256, level=k % 512, wtemp=(5 * k) % 1024)


def _weather(rng, msg_type, mmsi, f, nbytes=None, **kw):
    p, at = _binary(rng, msg_type, mmsi, 11, **kw)
    for off, cnt, name in ((0, 24, "lat"), (24, 25, "lon"), (49, 5, "gust5"), (54, 9, "wdir"), (63, 9, "gdir"),
                           (72, 11, "temp"), (83, 7, "hum"), (90, 10, "dew"), (100, 9, "pres"), (109, 2, "tend"),
                           (111, 8, "vis"), (119, 9, "level"), (128, 10, "wtemp")):
        p.put(at + off, cnt, f[name])
    return p.record(nbytes if nbytes else (at + 138 + 7) // 8)


def weather():
    rng = _background(1005)
    rows = [_weather(rng, 8, 600000000 + k, weather_fields(k)) for k in range(2048)]
    rows += [_weather(rng, 6, 610000000 + k, weather_fields(k), dst=620000000 + k, seq=k % 4, retx=k % 2)
             for k in (8 * j + j % 8 for j in range(256))]          # one k of every eight, every residue
    for t in (6, 8):
        for persons in (0, 1, 8190, 8191):
            p, at = _binary(rng, t, 630000000 + persons, 40, dst=5)
            p.put(at, 13, persons)
            rows.append(p.record((at + 13 + 7) // 8))
    return _records(rows)


# ---- field counts and text that depend on the frame's length -----------------------------------------------------------
LENGTH_TYPES = ((5, None), (7, None), (13, None), (19, None), (20, None), (24, 0), (24, 1))


def lengths():
    """every length 1..53 bytes: fields and text beyond the frame read 0"""
    rng = np.random.default_rng(1006)
    rows = []
    for n in range(1, 54):
        for t, part in LENGTH_TYPES:
            p = Payload(rng, t, 700000000 + 100 * n + t)
            if part is not None:
                p.put(38, 2, part)
            rows.append(p.record(n))
    return _records(rows)


def text_patterns(n):
    """six-bit codes of an n-character field"""
    pats = [[0] * n, [32] * n,
            [1] + [32] * (n - 1), [1] + [0] * (n - 1), [32] * (n - 1) + [26], [0] * (n - 1) + [26],
            [1, 2, 0, 32] + [32] * (n - 6) + [3, 4], [1, 32, 0, 0, 32, 2] + [0] * (n - 6),
            [1, 2, 3] + [(0, 32)[i % 2] for i in range(n - 3)], [24, 25] + [(32, 0, 0)[i % 3] for i in range(n - 2)]]
    for c in range(64):
        pats.append([c] + [32] * (n - 1))
        pats.append([0] * (n - 1) + [c])
    return pats


TEXT_TYPES = ((5, None), (19, None), (24, 0), (24, 1))


def text():
    rng = _background(1007)
    p20, p6 = text_patterns(20), text_patterns(6)     # (the call sign is read six characters long)
    rows = []
    for i in range(len(p20)):
        for t, part in TEXT_TYPES:
            p = Payload(rng, t, 800000000 + 10 * i + (t % 10) + (part or 0))
            if t == 5:
                p.text(70, p6[i]); p.text(112, p20[i]); p.text(302, p20[(i + 1) % len(p20)])
                p.put(294, 8, (i * 3) % 256)
                rows.append(p.record(53))
            elif t == 19:
                p.text(143, p20[i])
                rows.append(p.record(39))
            elif part == 0:
                p.put(38, 2, 0); p.text(40, p20[i])
                rows.append(p.record(20))
            else:
                p.put(38, 2, 1); p.text(90, p6[i])
                rows.append(p.record(21))
    # type 5 at every draught
    for d in range(256):
        p = Payload(rng, 5, 810000000 + d)
        p.put(294, 8, d)
        rows.append(p.record(53))
    return _records(rows)


def longest():
    """candidates for the longest line there is: type 6 with the weather report, every field at its widest -- the terms
    "- 60.0", "- 20.0" and "- 10.0" print widest at 0 ("-60.0"), but level 0 caps wave at 1.5, so both ways are tried --
    with nine- and ten-digit MMSIs, and at 45 bytes (one sentence of 60 characters in the brackets), 46 (two sentences)
    and 53"""
    rng = _background(1008)
    wide = dict(lat=(1 << 24) - 1, lon=(1 << 25) - 1, gust5=31, wdir=511, gdir=511, hum=127, pres=511, tend=3, vis=255)
    rows = []
    for temp, dew, level, wtemp in ((0, 0, 0, 0), (2047, 0, 511, 0), (0, 0, 511, 1023), (2047, 1023, 0, 1023),
                                    (0, 0, 15, 0)):
        f = dict(wide, temp=temp, dew=dew, level=level, wtemp=wtemp)
        for mmsi in (999999999, (1 << 30) - 1):
            for nbytes in (45, 46, 53):
                rows.append(_weather(rng, 6, mmsi, f, nbytes=nbytes, dst=mmsi, seq=3, retx=1))
    return _records(rows)


BUILDERS = dict(positions=positions, positions_b=positions_b, edges=edges, type4=type4, weather=weather,
                lengths=lengths, text=text, longest=longest)
_CACHE = {}


def group(name):
    if name not in _CACHE:
        _CACHE[name] = BUILDERS[name]()
        _CACHE[name].setflags(write=False)
    return _CACHE[name]


def everything():
    """all groups, each in print order, one after the other"""
    return np.concatenate([in_print_order(group(n)) for n in NAMES])
