"""The device message layer (nmea_device.hip) over the field sweeps of tests/message_cases.py, on the GPU: every group goes
through the device deframer into the frame ring, and what gnuais_batch_drain_messages() and gnuais_batch_fold_vessels()
make of it equals the host formatter over the drained records of a twin batch -- which tests/test_message_sweep_cpu.py
pins to the reference's own printf on these very frames."""
import numpy as np
import pytest

import message_cases as mc

pytestmark = pytest.mark.gpu

CHANID = b"ABXYZQRS"


def channel_streams(frames):
    """the bits of every channel: its frames in build order, 24 training bits in front of each and a short gap behind"""
    from gnuais_amd import synth
    streams = [[np.zeros(8, dtype=np.uint8)] for _ in range(mc.N_CH)]
    for f in frames:
        c = int(f["channel"])
        streams[c].append(synth.hdlc_frame_bits(bytes(f["payload"][: int(f["nbits"]) // 8]), training_bits=24))
        streams[c].append(np.zeros(5, dtype=np.uint8))
    return [np.concatenate(s).astype(np.uint8) for s in streams]


@pytest.mark.parametrize("names", [("positions",), ("positions_b", "edges"), ("type4", "text"), ("weather",),
                                   ("lengths", "longest")], ids="+".join)
def test_device_lines_of_a_sweep_equal_the_host_formatter(names):
    """two spans, so that the sequence digits carry over (and a frame lies across the cut); text, sentences, n_lines,
    n_sent and digits are messages_from_frames' over the twin's drained records, and every frame sent arrives"""
    from gnuais_amd import ReceiverBatch, messages_from_frames
    sent = np.concatenate([mc.group(n) for n in names])
    streams = channel_streams(sent)
    a = ReceiverBatch(mc.N_CH, max_len=48000, frame_capacity=len(sent))
    b = ReceiverBatch(mc.N_CH, max_len=48000, frame_capacity=len(sent))
    seq_a = np.array([3, 9, 0, 7, 1, 8, 5, 2], dtype=np.uint8)
    seq_b = seq_a.copy()
    arrived, payloads = 0, []
    for piece in (0, 1):
        half = [st[: len(st) // 2] if piece == 0 else st[len(st) // 2:] for st in streams]
        a.decode_bits(half)
        b.decode_bits(half)
        pending = b.pending_frames()
        frames = a.drain_frames()
        assert pending == len(frames) > 0
        want_nm, want_tx = messages_from_frames(frames, seq_a, CHANID if piece else None)
        nm, tx, n_sent, n_lines, n_frames = b.drain_messages(seq_b, CHANID if piece else None)
        assert n_frames == len(frames) and b.pending_frames() == 0
        assert nm == want_nm and n_sent == want_nm.count(b"\r\n")
        if tx != want_tx:                             # show the first differing line
            for x, y in zip(tx.split(b"\n"), want_tx.split(b"\n")):
                assert x == y
        assert tx == want_tx and n_lines == want_tx.count(b"\n") == len(frames)
        assert np.array_equal(seq_a, seq_b)
        arrived += len(frames)
        payloads.append(frames)
    assert arrived == len(sent)
    got = np.concatenate(payloads)
    key = lambda fr: sorted((int(f["channel"]), int(f["nbits"]), f["payload"].tobytes()) for f in fr)
    assert key(got) == key(sent)                      # the records that arrived are the ones built


def test_device_vessel_table_of_the_position_sweeps_equals_the_host_fold():
    """gnuais_batch_fold_vessels() over every position-type sweep (types 1-4 and 18 at every course, speed and heading,
    the coordinates at their edges; types 2 and 3 write to the MMSIs of type 1): the table is vessels_from_frames' over
    the same records in print order, floats bit for bit"""
    from gnuais_amd import ReceiverBatch, vessels_from_frames
    sent = np.concatenate([mc.group(n) for n in ("positions", "positions_b", "edges", "type4")])
    sent = sent.copy()
    sent["channel"] = np.arange(len(sent)) % mc.N_CH
    b = ReceiverBatch(mc.N_CH, max_len=48000, frame_capacity=len(sent))
    b.decode_bits(channel_streams(sent))
    assert b.pending_frames() == len(sent)
    table = b.fold_vessels()
    assert b.pending_frames() == len(sent)            # the frames stay queued
    want = vessels_from_frames(b.drain_frames())
    assert len(table) == len(want) > 6000
    assert table.tobytes() == want.tobytes()
    assert np.array_equal(table["lat"].view(np.uint32), want["lat"].view(np.uint32))
