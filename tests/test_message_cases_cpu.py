"""The builders of tests/message_cases.py checked by a plain bit reader (a restatement of the reference's offsets, not the
library): the frames really carry what the sweeps are for.  Where a condition here fails, the builder is wrong."""
import struct

import numpy as np
import pytest

import message_cases as mc


def get(f, pos, count):
    """`count` bits from `pos`, MSB first; 0 beyond the frame's whole bytes"""
    whole = int(f["nbits"]) // 8
    v = 0
    for i in range(pos, pos + count):
        k = i >> 3
        bit = (int(f["payload"][k]) >> (7 - (i & 7))) & 1 if k < whole and k < 53 else 0
        v = (v << 1) | bit
    return v


def sget(f, pos, count):
    v = get(f, pos, count)
    return v - (1 << count) if v >> (count - 1) else v


def msg_type(f):
    return get(f, 0, 6)


def shift_of(d):
    """the right shift LineOut::fixed takes for the double d: 1075 - biased exponent (1074 for 0 and denormals)"""
    ex = (struct.unpack("<Q", struct.pack("<d", d))[0] >> 52) & 0x7ff
    return 1074 if ex == 0 else 1075 - ex


def f32(x):
    return float(np.float32(x))


def test_groups_are_deterministic_whole_byte_records_of_bounded_size():
    for name in mc.NAMES:
        fr = mc.group(name)
        assert fr.dtype == mc.FRAME_DTYPE and 0 < len(fr) <= 4100, (name, len(fr))
        assert np.all(fr["flags"] == 1) and np.all(fr["nbits"] % 8 == 0) and np.all(fr["nbits"] >= 8), name
        assert np.all(fr["nbits"] <= 424) and np.all(fr["channel"] < mc.N_CH), name
        assert fr.tobytes() == mc.BUILDERS[name]().tobytes(), name
        for f in fr[:: max(1, len(fr) // 50)]:                       # nothing behind the whole bytes
            assert not f["payload"][int(f["nbits"]) // 8:].any(), name
        assert set(fr["channel"].tolist()) == set(range(mc.N_CH)), name
    assert len(mc.everything()) == sum(len(mc.group(n)) for n in mc.NAMES)


@pytest.fixture(scope="module")
def position_frames():
    return np.concatenate([mc.group(n) for n in ("positions", "positions_b", "edges", "type4")])


def test_every_shift_of_the_position_fields_occurs(position_frames):
    """every sh from 45 to 72 and the zero case, for the / 600000.0 fields and for the type 4 expression; 63, 64 and 65
    -- the last value of the first branch, the s2 == 0 case and the first ordinary value of the second -- for lat and
    for lon with both signs"""
    seen = {("deg", "lat"): set(), ("deg", "lon"): set(), ("t4", "lat"): set(), ("t4", "lon"): set()}
    for f in position_frames:
        t = msg_type(f)
        if t in (1, 2, 3):
            lat, lon = sget(f, 89, 27), sget(f, 61, 28)
        elif t == 18:
            lat, lon = sget(f, 85, 27), sget(f, 57, 28)
        elif t == 4:
            lat, lon = sget(f, 107, 27), sget(f, 79, 28)
        else:
            continue
        for which, v in (("lat", lat), ("lon", lon)):
            d = f32(f32(v) / 10000.0 / 60.0) if t == 4 else f32(v) / 600000.0
            seen[("t4" if t == 4 else "deg", which)].add((shift_of(d), v < 0))
    for key, s in seen.items():
        # |lat| <= 2^26 is below 128 degrees (sh 46 at the least), |lon| <= 2^27 below 256 (sh 45): nothing lies outside
        want = set(range(45 if key[1] == "lon" else 46, 73)) | {1074}
        shifts = {sh for sh, _ in s}
        assert shifts == want, (key, sorted(want ^ shifts))
        for sh in (63, 64, 65):
            assert (sh, False) in s and (sh, True) in s, (key, sh)


def test_courses_speeds_headings_and_draughts_are_complete(position_frames):
    course, speed, heading, ties18 = set(), set(), set(), set()
    per_type = {1: 0, 2: 0, 3: 0, 18: 0, 4: 0}
    for f in position_frames:
        t = msg_type(f)
        per_type[t] += 1
        if t in (1, 2, 3):
            c, s, h = get(f, 116, 12), get(f, 50, 10), get(f, 128, 9)
        elif t == 18:
            c, s, h = get(f, 112, 12), get(f, 46, 10), get(f, 124, 9)
            if c % 10 == 5:
                ties18.add(c)
        else:
            continue
        if t in (1, 18):
            course.add(c); speed.add(s); heading.add(h)
    assert course == set(range(4096)) and speed == set(range(1024)) and heading == set(range(512))
    assert len(ties18) == 410                       # every exact tie of "%.0f" also at type 18's offsets
    assert all(n > 200 for n in per_type.values()), per_type
    draughts = {get(f, 294, 8) for f in mc.group("text") if msg_type(f) == 5}
    assert draughts == set(range(256))


def test_type4_clock_fields_cover_their_width():
    fr = [f for f in mc.group("type4")]
    assert {sget(f, 107, 27) for f in fr} == set(range(-600, 601)) == {sget(f, 79, 28) for f in fr}
    assert any(sget(f, 107, 27) != sget(f, 79, 28) for f in fr)
    assert {get(f, 61, 5) for f in fr} == set(range(32))
    assert {get(f, 66, 6) for f in fr} == set(range(64)) == {get(f, 72, 6) for f in fr}
    assert {get(f, 40, 12) for f in fr} == {0, 9, 10, 4095}
    small = {(sget(f, 89, 27), sget(f, 61, 28)) for f in mc.group("positions")}
    assert {a for a, _ in small} == set(range(-2048, 2048)) == {b for _, b in small}
    assert sum(a != b for a, b in small) > 4000


WEATHER_FIELDS = (("lat", 0, 24), ("lon", 24, 25), ("wind", 40, 7), ("gust", 47, 7), ("wdir", 54, 9), ("gdir", 63, 9),
                  ("temp", 72, 11), ("hum", 83, 7), ("dew", 90, 10), ("pres", 100, 9), ("tend", 109, 2), ("vis", 111, 8),
                  ("level", 119, 9), ("wave", 124, 8), ("wtemp", 128, 10))


def test_weather_report_fields_cover_their_ranges():
    """read at the reference's own overlapping offsets: every value of the six %.1f fields, both ends of the others, in
    type 8 and (thinned) in type 6; persons on board at both ends in both types"""
    seen = {t: {n: set() for n, _, _ in WEATHER_FIELDS} for t in (6, 8)}
    persons = {6: set(), 8: set()}
    for f in mc.group("weather"):
        t = msg_type(f)
        at = 88 if t == 6 else 56
        dac, fi = get(f, at - 16, 10), get(f, at - 6, 6)
        assert dac == 1 and fi in (11, 40)
        if fi == 40:
            persons[t].add(get(f, at, 13))
            continue
        assert int(f["nbits"]) >= at + 138
        for n, off, cnt in WEATHER_FIELDS:
            seen[t][n].add(get(f, at + off, cnt))
    for n, _, cnt in WEATHER_FIELDS:
        if n in ("temp", "dew", "vis", "level", "wave", "wtemp"):
            assert seen[8][n] == set(range(1 << cnt)), n
        else:
            assert {0, (1 << cnt) - 1} <= seen[8][n], n
        assert len(seen[6][n]) >= min(1 << cnt, 4), n
    assert set(range(601)) <= seen[8]["lat"] and set(range(601)) <= seen[8]["lon"]
    assert {1 << k for k in range(24)} <= seen[8]["lat"] and {1 << k for k in range(25)} <= seen[8]["lon"]
    assert persons[6] == persons[8] == {0, 1, 8190, 8191}


def test_every_length_of_the_length_dependent_types_occurs():
    seen = {}
    for f in mc.group("lengths"):
        t = msg_type(f) if int(f["nbits"]) >= 8 else -1
        part = get(f, 38, 2) if t == 24 else None
        seen.setdefault((t, part), set()).add(int(f["nbits"]) // 8)
    for t in (5, 7, 13, 19, 20):
        assert seen[(t, None)] == set(range(1, 54)), t
    # type 24's part bits lie in byte 4: a shorter frame reads part A whatever was meant
    assert seen[(24, 0)] == set(range(1, 54)) and seen[(24, 1)] == set(range(5, 54))


def test_text_patterns_are_what_they_claim():
    names = {}
    for f in mc.group("text"):
        t = msg_type(f)
        if t == 5 and int(f["nbits"]) == 424:
            names.setdefault(5, []).append(tuple(get(f, 112 + 6 * i, 6) for i in range(20)))
            names.setdefault("dest", []).append(tuple(get(f, 302 + 6 * i, 6) for i in range(20)))
            names.setdefault("call5", []).append(tuple(get(f, 70 + 6 * i, 6) for i in range(6)))
        elif t == 19:
            names.setdefault(19, []).append(tuple(get(f, 143 + 6 * i, 6) for i in range(20)))
        elif t == 24 and get(f, 38, 2) == 0:
            names.setdefault("24A", []).append(tuple(get(f, 40 + 6 * i, 6) for i in range(20)))
        elif t == 24:
            names.setdefault("24B", []).append(tuple(get(f, 90 + 6 * i, 6) for i in range(6)))
    for key in (5, "dest", "call5", 19, "24A", "24B"):
        s = set(names[key])
        n = len(next(iter(s)))
        assert (0,) * n in s and (32,) * n in s, key
        assert {p[0] for p in s} == set(range(64)) == {p[-1] for p in s}, key
        assert any(p[0] not in (0, 32) and all(c in (0, 32) for c in p[1:]) for p in s), key       # one character first
        assert any(p[-1] not in (0, 32) and all(c in (0, 32) for c in p[:-1]) for p in s), key     # one character last
        assert any(0 in p[1:-1] and 32 in p[1:-1] and p[-1] not in (0, 32) and p[0] not in (0, 32) for p in s), key                                                                           # @ and blank inside
        assert any(p[0] not in (0, 32) and p[-1] in (0, 32) and 0 in p and 32 in p for p in s), key  # a trailing mix


def test_longest_candidates_are_type_6_weather_reports():
    fr = mc.group("longest")
    assert {int(n) for n in fr["nbits"]} == {360, 368, 424}
    for f in fr:
        assert msg_type(f) == 6 and get(f, 72, 10) == 1 and get(f, 82, 6) == 11
        assert get(f, 88, 24) == (1 << 24) - 1 and get(f, 88 + 24, 25) == (1 << 25) - 1
    assert {get(f, 8, 30) for f in fr} == {999999999, (1 << 30) - 1}
