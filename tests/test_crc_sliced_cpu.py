"""K3's CRC four bytes per step, CPU side: gnuais_amd/csrc/crc_sliced.h -- the text the kernel runs -- built by itself
(tests/c/crc_sliced_check.cpp) and held against the bitwise definition (protodec.c:106-118, restated here bit by bit):
every entry of the four tables, and the stepped register against the byte-wise one and the definition on random buffers
of every length from 0 to 64 bytes and on the project's known answers (tests/golden/crc16.npz).  No device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLY = 0x8408


def lfsr(reg, steps):
    """`steps` steps of the reflected register with nothing fed"""
    for _ in range(steps):
        reg = (reg >> 1) ^ (POLY if reg & 1 else 0)
    return reg


def crc_bitwise(data, reg=0xFFFF):
    """the register (no final complement) after the bytes, one bit at a time, LSB first"""
    for v in data:
        for b in range(8):
            fb = (reg ^ (v >> b)) & 1
            reg >>= 1
            if fb:
                reg ^= POLY
    return reg


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    so = str(tmp_path_factory.mktemp("crc_sliced") / "libcrc_sliced_check.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "c", "crc_sliced_check.cpp"), "-o", so])
    L = C.CDLL(so)
    L.crc_sliced_run.restype = L.crc_sliced_bytewise.restype = L.crc_sliced_entry.restype = C.c_uint
    L.crc_sliced_run.argtypes = L.crc_sliced_bytewise.argtypes = [C.c_void_p, C.c_int]
    L.crc_sliced_entry.argtypes = [C.c_int, C.c_uint]
    L.crc_sliced_tables.argtypes = [C.c_void_p]
    return L


def run(L, fn, data):
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8).copy()      # never a zero-sized buffer
    return getattr(L, fn)(buf.ctypes.data, len(data))


def test_every_table_entry_is_the_bitwise_definition(lib):
    n = lib.crc_sliced_slices()
    assert n == 4
    tabs = np.zeros((n, 256), dtype=np.uint16)
    lib.crc_sliced_tables(tabs.ctypes.data)
    for k in range(n):
        for b in range(256):
            want = lfsr(b, 8 * (k + 1))
            assert int(tabs[k, b]) == want, (k, b)
            assert lib.crc_sliced_entry(k, b) == want, (k, b)
    # table 0 is the byte table: the register after one byte fed into an empty register
    assert all(int(tabs[0, b]) == crc_bitwise([b], reg=0) for b in range(256))


def test_stepped_register_on_every_length_0_to_64(lib):
    rng = np.random.default_rng(1611)
    for n in range(65):
        for _ in range(24):
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            want = crc_bitwise(data)
            assert run(lib, "crc_sliced_bytewise", data) == want, (n, data.hex())
            assert run(lib, "crc_sliced_run", data) == want, (n, data.hex())
    for n in range(65):                      # the extremes of the look-ups' indices
        for fill in (0x00, 0xFF):
            data = bytes([fill]) * n
            assert run(lib, "crc_sliced_run", data) == crc_bitwise(data), (n, fill)


def test_known_answers(lib):
    g = np.load(os.path.join(ROOT, "tests", "golden", "crc16.npz"))
    data, lens, crc = g["data"].tobytes(), g["lens"], g["crc"]
    assert len(lens) >= 4
    pos = 0
    checked = 0
    for n, want in zip(lens.tolist(), crc.tolist()):
        msg = data[pos:pos + n]
        pos += n
        if n <= 128:                         # what the check library's word buffer holds
            assert (~run(lib, "crc_sliced_run", msg)) & 0xFFFF == want, (n, msg.hex())
            checked += 1
        assert (~run(lib, "crc_sliced_bytewise", msg)) & 0xFFFF == want, (n, msg.hex())
    assert pos == len(data) and checked >= 4
    assert (~run(lib, "crc_sliced_run", b"123456789")) & 0xFFFF == 0x906E       # CRC-16/X-25's check value
    # a frame with its FCS appended leaves the register K3 tests for (0xf0b8 = ~0x0f47, protodec.c:166)
    body = bytes(range(21))
    fcs = (~crc_bitwise(body)) & 0xFFFF
    assert run(lib, "crc_sliced_run", body + bytes([fcs & 0xFF, fcs >> 8])) == 0xF0B8
