"""nmea_device.hip's own text on the CPU: compiled by g++ behind tests/c/hip_cpu (a thread per lane, the blocks of a launch
one after the other, rocPRIM's sort and scans stood in for) under ASan + UBSan, as a stand-alone program
(tests/c/message_kernel_main.cpp).  The kernels' control flow, their bounds and the hand-written printf("%.Nf") of
LineOut::fixed cannot be checked on a device by the CPU suite; this is that check.  The chunk-table path and the carried
vessel table stay with their GPU tests."""
import os
import subprocess
import time

import numpy as np
import pytest

import hip_cpu_build
import message_cases as mc
from gnuais_amd.receiver import VESSEL_DTYPE

SEQ_IN = np.array([3, 9, 0, 7, 1, 8, 5, 2], dtype=np.uint8)
CHANID = b"ABXYZQRS"
SWEEP_STRIDE = 31
COMPARED = 38290985             # what the program counts at that stride


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return hip_cpu_build.build("message_kernel_main.cpp", tmp_path_factory.mktemp("message_kernel") / "message_kernel.bin",
                               "-Wno-unused-function", "-Wno-subobject-linkage", "-Wno-ignored-attributes")


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def run_frames(exe, tmp, groups=None):
    """every group of message_cases through the program, in build order (the channels interleaved: the sort has work to
    do) -> None, or what differs first"""
    from gnuais_amd import messages_from_frames, vessels_from_frames
    groups = groups or [(name, mc.group(name)) for name in mc.NAMES]
    src, dst = os.path.join(str(tmp), "groups.in"), os.path.join(str(tmp), "groups.out")
    with open(src, "wb") as f:
        f.write(np.int32(len(groups)).tobytes())
        for _, fr in groups:
            f.write(np.int32(len(fr)).tobytes() + SEQ_IN.tobytes() + CHANID + fr.tobytes())
    r = subprocess.run([exe, "frames", src, dst], capture_output=True, env=ENV, timeout=600)
    if r.returncode:
        return "exit %d: %s" % (r.returncode, r.stderr.decode()[-3000:])
    out = open(dst, "rb").read()
    pos = 0
    for name, fr in groups:
        fr = mc.in_print_order(fr)
        seq = SEQ_IN.copy()
        want_nm, want_tx = messages_from_frames(fr, seq, CHANID)
        totals = np.frombuffer(out, dtype=np.uint32, count=4, offset=pos)
        n_nm = int(totals[0]) + int(totals[1])
        nm = out[pos + 16:pos + 16 + n_nm]
        pos += 16 + n_nm
        seq_out = np.frombuffer(out, dtype=np.uint8, count=mc.N_CH, offset=pos)
        info2 = np.frombuffer(out, dtype=np.uint32, count=2, offset=pos + mc.N_CH)
        pos += mc.N_CH + 8
        tx = out[pos:pos + int(info2[0])]
        pos += int(info2[0])
        count = int(np.frombuffer(out, dtype=np.uint32, count=1, offset=pos)[0])
        table = np.frombuffer(out, dtype=VESSEL_DTYPE, count=count, offset=pos + 4)
        pos += 4 + count * VESSEL_DTYPE.itemsize
        if tx != want_tx:
            for a, b in zip(tx.split(b"\n"), want_tx.split(b"\n")):
                if a != b:
                    return "%s: line %r, want %r" % (name, a, b)
            return "%s: %d bytes of lines, want %d" % (name, len(tx), len(want_tx))
        if nm != want_nm:
            return "%s: sentences differ" % name
        if int(totals[2]) != want_nm.count(b"\r\n") or int(info2[1]) != want_tx.count(b"\n") or int(totals[3]):
            return "%s: counts %s %s" % (name, totals, info2)
        if not np.array_equal(seq_out, seq):
            return "%s: digits %s, want %s" % (name, seq_out, seq)
        want_table = vessels_from_frames(fr)
        if table.tobytes() != want_table.tobytes():
            return "%s: vessel table differs (%d entries, want %d)" % (name, len(table), len(want_table))
    assert pos == len(out)
    return None


def run_sweep(exe):
    r = subprocess.run([exe, "sweep", str(SWEEP_STRIDE)], capture_output=True, env=ENV, timeout=600)
    if r.returncode:
        return "exit %d: %s %s" % (r.returncode, r.stdout.decode(), r.stderr.decode()[-3000:])
    compared, wrong = (int(x) for x in r.stdout.decode().split()[0::2])
    assert wrong == 0 and compared == COMPARED, r.stdout
    return None


def test_launch_interface_over_every_group_equals_the_host_formatter(harness, tmp_path):
    """nmea_format_enqueue (sort path) + messages_format_enqueue + vessels_fold_enqueue over every group of
    message_cases, with a non-zero seq_in and a chanid string, every buffer allocated at exactly the size the interface
    asks for: sentences, lines, counts and sequence digits are messages_from_frames', the table is vessels_from_frames'
    byte for byte -- and test_message_sweep_cpu.py pins those to the reference."""
    assert run_frames(harness, tmp_path) is None


def test_fixed_and_dec_equal_printf_over_the_fields_whole_ranges(harness):
    """LineOut::fixed and ::dec called directly, against snprintf: v / 600000.0, the type 4 expression and v / 60000.0 at
    %.6f for every |v| <= 2^21 and every 31st value up to +-2^27; every %.1f expression of the file over its field's whole
    range; c / 10.0 at %.0f and %.1f for all 65 536 c; dec at widths 0, 2 and 9 around every power of ten and at the
    32-bit limits; and the length-dependent loops of types 7, 13 and 20 at every padded length.
    38 290 985 values; 19 s of the module's 32 s on eight cores (8 s are the build, 4 s the launches)."""
    t = time.time()
    assert run_sweep(harness) is None
    print("sweep: %.1f s" % (time.time() - t))
