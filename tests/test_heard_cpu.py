"""Who heard each transmission on the CPU: the host object's gnuais_uniq_push_heard (frame_unique.cpp) against the plain
restatement tests/heard_ref.py over the random record sets of test_unique_cpu.py -- whole and cut into drains, push and
push_heard alternating on one object -- with the invariants of the definition; its edges; the unit by itself under
ASan + UBSan; the kernels' own text behind tests/c/hip_cpu; and the new names of the ABI."""
import os
import subprocess

import numpy as np
import pytest

import heard_ref as hr
import hip_cpu_build
import unique_ref as ur
from oracle_lib import FRAME_DTYPE
from test_unique_cpu import cut_into_drains, random_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuais_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]


@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "gnuais_amd", "libgnuais_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-s", "-j8", "-C", CSRC])
    from gnuais_amd import lib
    return lib


@pytest.fixture(scope="module")
def Uniq(L):
    from gnuais_amd.receiver import Uniq
    return Uniq


def random_signal(rng, n, L):
    sg = np.zeros(n, dtype=L.SIGNAL_DTYPE)
    sg["power"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    sg["ferr"] = rng.integers(-32768, 32768, n).astype(np.int16)
    sg["blocks"] = rng.integers(0, 65536, n).astype(np.uint16)
    return sg


def same5(a, b):
    return (a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            and a[1].dtype == np.int64 and a[2].dtype == np.int32 and a[3].dtype == np.int32 and np.array_equal(a[3], b[3])
            and a[4].dtype == b[4].dtype and a[4].tobytes() == b[4].tobytes())


def same3(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_hearer_layout(L):
    d = L.HEARER_DTYPE
    assert d.itemsize == 24 and [d.fields[k][1] for k in ("channel", "flags", "t", "signal")] == [0, 4, 8, 16]
    assert d.fields["signal"][0] == L.SIGNAL_DTYPE


def test_the_new_names_are_declared_exported_and_bound(L):
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnuais_hip.h")).read(), flags=re.S)
    handle = L.load()
    for name in ("gnuais_batch_drain_frames_heard", "gnuais_uniq_push_heard", "gnuais_node_drain_frames_heard"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in L.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"typedef struct gnuais_hearer \{[^}]*\} gnuais_hearer;", text)


def test_push_heard_equals_the_restatement_whole_and_cut_into_drains(Uniq, L):
    rng = np.random.default_rng(2025)
    repaired_members = set()
    big = 0
    for s in range(1000):
        W = int(rng.choice([1, 5, 64, 128, 700]))
        fr, tm = random_set(rng, W)
        sg = random_signal(rng, len(fr), L)
        top = (int(tm.max()) + 1) if len(tm) else 1
        u, r, plain = Uniq(W), hr.HeardRef(W), Uniq(W)
        whole = u.push_heard(fr, tm, top + W + 1, signal=sg)
        assert same5(whole, r.push_heard(fr, tm, top + W + 1, signal=sg)), s
        assert same3(whole, plain.push(fr, tm, top + W + 1)), s     # the first three outputs are push()'s
        hr.check_invariants(*whole)
        assert u.late() == 0 and len(whole[4]) == len(fr)           # everything is listed: members + late = frames
        # every member is a frame of the input, with its own flags, time and record
        have = sorted(zip(fr["channel"].tolist(), np.where(tm < 0, -1, tm).tolist(), fr["flags"].tolist(), sg.tolist()))
        m = whole[4]
        assert sorted(zip(m["channel"].tolist(), m["t"].tolist(), m["flags"].tolist(), m["signal"].tolist())) == have, s
        repaired_members.update(bool(x & ur.REPAIRED) for x in m["flags"].tolist())
        big = max(big, int(whole[2].max()))
        # cut into drains, push and push_heard alternating on one object against one restatement
        u.reset()
        r.reset()
        plain.reset()
        listed = 0
        for d, (f, t, rows) in enumerate(cut_into_drains(rng, fr, tm)):
            g = random_signal(rng, len(f), L) if d % 3 else None
            if (d + s) % 2 == 0:
                got = u.push_heard(f, t, rows, signal=g)
                assert same5(got, r.push_heard(f, t, rows, signal=g)), (s, d)
                hr.check_invariants(*got)
                if g is None:
                    assert not got[4]["signal"].tobytes().strip(b"\0")      # signal = NULL gives zeros
                listed += len(got[4])
            else:
                got = u.push(f, t, rows)
                assert same3(got, r.push(f, t, rows)), (s, d)
                listed += int(got[2].sum())
            assert same3(got, plain.push(f, t, rows)), (s, d)
            assert u.late() == r.late == plain.late()
        assert listed + u.late() == len(fr), s
        for x in (u, plain):
            x.close()
    assert repaired_members == {False, True} and big >= 5


def test_members_of_the_intact_before_repaired_example(Uniq):
    fr = np.zeros(4, dtype=FRAME_DTYPE)
    fr["nbits"], fr["payload"][:, 0], fr["channel"] = 168, 9, [3, 2, 1, 0]
    fr["flags"] = [1 | ur.REPAIRED, 1, 1, 1 | ur.REPAIRED]
    tm = np.array([100, 110, 110 + 50, 110 + 50 + 51], dtype=np.int64)
    f, t, c, first, m = Uniq(50).push_heard(fr, tm, 10 ** 6)
    assert c.tolist() == [3, 1] and first.tolist() == [0, 3, 4] and t.tolist() == [110, 211]
    assert m["channel"].tolist() == [3, 2, 1, 0] and m["t"].tolist() == [100, 110, 160, 211]
    assert m["flags"].tolist() == [1 | ur.REPAIRED, 1, 1, 1 | ur.REPAIRED]
    assert not m["signal"].tobytes().strip(b"\0")


def test_empty_capacity_and_late_copies(Uniq, L):
    u = Uniq(100)
    got = u.push_heard(np.zeros(0, dtype=FRAME_DTYPE), np.zeros(0, dtype=np.int64), 0)
    assert [len(x) for x in got] == [0, 0, 0, 1, 0] and got[3].tolist() == [0]
    fr = np.zeros(3, dtype=FRAME_DTYPE)
    fr["nbits"], fr["payload"][:, 0], fr["flags"] = 168, [1, 2, 2], 1
    fr["channel"] = [0, 0, 1]
    tm = np.array([950, 960, 965], dtype=np.int64)
    with pytest.raises(L.GnuaisError) as e:
        u.push_heard(fr, tm, 1000, cap=1)       # two clusters do not fit one entry ...
    assert e.value.code == L.E_ARG
    f, t, c, first, m = u.push_heard(fr, tm, 1000, cap=2)   # ... and nothing was consumed
    assert c.tolist() == [1, 2] and first.tolist() == [0, 1, 3] and u.late() == 0
    assert m["channel"].tolist() == [0, 0, 1] and m["t"].tolist() == [950, 960, 965]
    fr2 = fr[1:2].copy()
    fr2["channel"] = 5
    got = u.push_heard(fr2, np.array([1010], dtype=np.int64), 1100)     # chains onto the open cluster: late, listed nowhere
    assert [len(x) for x in got] == [0, 0, 0, 1, 0] and u.late() == 1


def write_cases(path, cases, with_signal):
    with open(path, "wb") as f:
        for W, drains in cases:
            f.write(np.array([W, len(drains), int(with_signal)], dtype=np.int32).tobytes())
            for fr, tm, sg, rows in drains:
                f.write(np.int32(len(fr)).tobytes() + np.int64(rows).tobytes() + fr.tobytes() + tm.tobytes() + sg.tobytes())


def make_cases(seed, L, n_sets=120):
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n_sets):
        W = int(rng.choice([1, 64, 700]))
        fr, tm = random_set(rng, W)
        cases.append((W, [(f, t, random_signal(rng, len(f), L), rows) for f, t, rows in cut_into_drains(rng, fr, tm)]))
    cases.append((9, [(np.zeros(0, dtype=FRAME_DTYPE), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=L.SIGNAL_DTYPE), 0)]))
    return cases


def check_output(out, cases, with_signal, first_word):
    """the programs' common output against the restatement; first_word(value) is asserted on each drain's first int32"""
    pos = 0
    total = 0
    for W, drains in cases:
        ref = hr.HeardRef(W)
        for d, (fr, tm, sg, rows) in enumerate(drains):
            w0, got, nm = np.frombuffer(out, dtype=np.int32, count=3, offset=pos)
            late = int(np.frombuffer(out, dtype=np.int64, count=1, offset=pos + 12)[0])
            pos += 20
            total += first_word(int(w0))
            heard = d % 2 == 0
            want = ref.push_heard(fr, tm, rows, signal=sg if with_signal else None) if heard else ref.push(fr, tm, rows)
            assert got == len(want[0]) and late == ref.late
            assert out[pos:pos + 64 * got] == want[0].tobytes()
            assert out[pos + 64 * got:pos + 72 * got] == want[1].tobytes()
            assert out[pos + 72 * got:pos + 76 * got] == want[2].tobytes()
            pos += 76 * got
            if heard:
                assert nm == len(want[4])
                assert out[pos:pos + 4 * (got + 1)] == want[3].tobytes()
                pos += 4 * (got + 1)
                assert out[pos:pos + 24 * nm] == want[4].tobytes()
                pos += 24 * nm
            else:
                assert nm == -1
    assert pos == len(out)
    return total


@pytest.mark.parametrize("with_signal", [True, False])
def test_host_unit_standalone_under_asan_and_ubsan(tmp_path, L, with_signal):
    """frame_unique.cpp with tests/c/heard_main.cpp, built by g++ with -fsanitize=address,undefined and run as a program:
    push and push_heard alternating over random sets cut into drains; what it writes is the restatement's"""
    exe = str(tmp_path / "heard.bin")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "heard_main.cpp"), os.path.join(CSRC, "frame_unique.cpp"),
                           "-o", exe])
    cases = make_cases(79, L)
    src, dst = str(tmp_path / "sets.in"), str(tmp_path / "sets.out")
    write_cases(src, cases, with_signal)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])

    def rc_ok(rc):
        assert rc == 0
        return 0
    check_output(open(dst, "rb").read(), cases, with_signal, rc_ok)


@pytest.mark.parametrize("hash_bits", [64, 3, 1])
def test_the_kernels_own_text_on_the_cpu_equals_the_restatement(tmp_path, L, hash_bits):
    """frame_unique.hip compiled for the CPU behind tests/c/hip_cpu's serial mode under ASan + UBSan, driven by
    tests/c/heard_kernel_main.cpp as the heard drain drives it, every buffer at exactly the size the launch interface
    asks for: records, times, copies, offsets, members and the late count are the restatement's -- with the full hash
    without ever taking the exact path, with 3 and 1 bits through it -- and drains without lists in between leave the
    same state.  Run as a program; nothing is loaded into Python."""
    exe = hip_cpu_build.build("heard_kernel_main.cpp", tmp_path / "heard_kernel.bin", "-DHIP_CPU_SERIAL")
    cases = make_cases(80, L)
    src, dst = str(tmp_path / "sets.in"), str(tmp_path / "sets.out")
    with_signal = hash_bits != 3
    write_cases(src, cases, with_signal)
    r = subprocess.run([exe, src, dst, str(hash_bits)], capture_output=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    exact = check_output(open(dst, "rb").read(), cases, with_signal, lambda runs: runs)
    assert exact == 0 if hash_bits == 64 else exact > 80
