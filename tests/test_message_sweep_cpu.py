"""The host formatter (nmea.cpp) pinned to the reference on the field sweeps of tests/message_cases.py: sentences, stdout
lines and sequence digits, byte for byte.  The reference's answer comes live from oracle/_ref where that is built, else
from tests/golden/message_sweep.npz (ref_pins.want_message_sweep).  The device formatter is compared with the host one
(test_message_kernel_cpu.py, test_message_sweep_gpu.py), so this is what ties it to the reference's own printf."""
import os

import numpy as np

import message_cases as mc
import ref_pins

LONGEST_LINE = 435          # bytes, '\n' included: what the reference printed for the `longest` group (MSG_LINE_MAX = 512)


def first_difference(got, want, sep):
    for i, (a, b) in enumerate(zip(got.split(sep), want.split(sep))):
        assert a == b, "line %d" % i
    assert len(got) == len(want)


def test_host_formatter_equals_the_reference_on_every_sweep():
    from gnuais_amd import messages_from_frames
    w = ref_pins.want_message_sweep()
    want_nm, want_tx = w["nmea"].tobytes(), w["text"].tobytes()
    fr = mc.everything()
    seq = np.zeros(mc.N_CH, dtype=np.uint8)
    nm, tx = messages_from_frames(fr, seq)
    if tx != want_tx:
        first_difference(tx, want_tx, b"\n")
    if nm != want_nm:
        first_difference(nm, want_nm, b"\r\n")
    assert nm == want_nm and tx == want_tx and np.array_equal(seq, w["seq"])
    # every frame is of an accepted type: a line each, in the order of the groups
    lines = want_tx.split(b"\n")
    assert lines.pop() == b"" and len(lines) == len(fr)
    start = len(fr) - len(mc.group("longest"))
    lens = np.array([len(l) + 1 for l in lines])
    assert lens.max() == lens[start:].max() == LONGEST_LINE < 512
    assert lens[:start].max() < LONGEST_LINE                      # and no other group comes near
    assert b"type 6 mmsi 1073741823: dst_mmsi 1073741823" in lines[start + int(np.argmax(lens[start:]))]


def test_the_stored_answer_fits_and_is_the_live_one():
    assert os.path.getsize(ref_pins.MESSAGE_SWEEP) <= 618165      # ref_pins.npz as committed with it
    with np.load(ref_pins.MESSAGE_SWEEP) as z:
        stored = {k: z[k] for k in z.files}
    assert sorted(stored) == ["nmea", "seq", "text"]
    live = ref_pins.want_message_sweep()                          # the stored copy itself where oracle/_ref is not built
    for k in stored:
        assert stored[k].tobytes() == live[k].tobytes(), k
