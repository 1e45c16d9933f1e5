"""tests/c/hip_cpu, the stand-in for the HIP headers behind which the kernel files' own text runs on the CPU, checked by
itself: every CPU kernel test rests on it.  One host program (tests/c/hip_cpu_main.cpp) under ASan + UBSan.  No GPU."""
import os
import subprocess

import pytest

import hip_cpu_build

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return hip_cpu_build.build("hip_cpu_main.cpp", tmp_path_factory.mktemp("hip_cpu") / "hip_cpu.bin")


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, env=ENV, timeout=120)


def ballot(first, lanes, keep):
    """the mask of a wave that holds the threads first .. first + lanes - 1"""
    return sum(1 << l for l in range(lanes) if keep(first + l))


def test_a_launch_runs_every_lane_of_every_block_with_its_own_indices_votes_and_shared_word(exe):
    r = run(exe, "grid")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    got = [[int(w, 16) if i == 2 else int(w) for i, w in enumerate(line.split())] for line in r.stdout.decode().splitlines()]
    third = lambda t: t % 3 == 0
    want = [[b, t, ballot(t & ~63, 64, third), 1000 + b, 3, 128] for b in range(3) for t in range(128)]
    # one block of 100 lanes: the second wave votes over the 36 lanes it has
    want += [[0, t, ballot(t & ~63, 64 if t < 64 else 36, third), 1000, 1, 100] for t in range(100)]
    assert got == want
    assert want[0][2] != want[64][2] and want[3 * 128 + 64][2] < 1 << 36


def test_dynamic_shared_memory_is_the_launchs_bytes_and_each_blocks_own(exe):
    """100 bytes: a kernel that stays inside them runs clean, through a handle at namespace scope and one inside the
    kernel, which name the same 16-byte aligned block; the second block finds none of the bytes the first one wrote"""
    r = run(exe, "lds", "100")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode().split() == ["0", "0", "0", str(0x5c)]


def test_the_first_byte_past_dynamic_shared_memory_stops_the_program(exe):
    r = run(exe, "lds", "101")
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr.decode()
    assert "lds_kernel" in r.stderr.decode()


def test_a_lane_that_returns_leaves_its_blocks_barrier_and_its_waves_vote(exe):
    r = run(exe, "early")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    even = ballot(0, 64, lambda t: t % 2 == 0)
    assert [int(w, 16) for w in r.stdout.decode().split()] == [1 if t & 1 else even for t in range(128)]


def test_the_serial_mode_has_no_barrier_vote_or_shared_memory(tmp_path):
    """-DHIP_CPU_SERIAL: the program, which uses all of them, does not compile"""
    with pytest.raises(subprocess.CalledProcessError):
        hip_cpu_build.build("hip_cpu_main.cpp", tmp_path / "serial.bin", "-DHIP_CPU_SERIAL", "-fmax-errors=3")
