"""File -> device chain -> what gnuais would print / send, end to end.

  python scripts/decode_file.py capture.wav            # RIFF/WAVE, any channel count
  python scripts/decode_file.py capture.raw --raw 2    # bare int16 frames, as the reference reads them
  python scripts/decode_file.py iq.wav --iq           # complex baseband: 2N channels = N receivers' (I, Q) pairs
  python scripts/decode_file.py sdr.wav --wideband 6 --offsets -25000,25000
                                                      # wide I/Q (2M channels = M streams) at R = 6 x 48 kHz, each
                                                      # stream channelised on the device to one receiver per offset
  python scripts/decode_file.py rtl.cu8 --wideband 6 --rate 288000 [--format cu8|cs8|cs16|cf32] [--streams M]
                                                      # a bare SDR capture (rtl_sdr: .cu8, hackrf_transfer: .cs8, GNU Radio:
                                                      # .cf32 / .cfile, int16: .cs16): the format defaults to the one the
                                                      # extension names; the file goes to the device in its native format and
                                                      # is converted where the channeliser loads it
  python scripts/decode_file.py rtl.cu8 --wideband auto --rate 2048000
                                                      # any rate with 48000 / rate = U / D, U <= 64, D <= 1024 (250 k, 1.024 M,
                                                      # 2 M, 2.048 M, 2.5 M, ...): the ratio comes from the rate, the device
                                                      # resamples by U / D; the file's tail is trimmed to a multiple of D
  python scripts/decode_file.py iq.wav --iq --afc 2048
                                                      # --iq / --wideband: remove each receiver's carrier error on the device
                                                      # (an SDR's oscillator), estimated over a window of that many samples;
                                                      # the measured errors go to stderr
  ... --times [--start UNIX_SECONDS]
                                                      # every sentence behind an NMEA TAG block "\\c:<unix>*hh\\" with the
                                                      # second the frame was received in, counted in the file's own samples
                                                      # from --start (the UNIX second of the file's first sample; default 0)
  ... --repair
                                                      # frames that fail the CRC by one symbol error (two adjacent bits) are
                                                      # repaired on the device (gnuais_batch_repair) and printed like any
                                                      # frame; the summary on stderr counts them and names each one
  ... --unique ROWS [--verbose]
                                                      # several receivers of the file hear the same transmissions (overlapping
                                                      # stations, the two offsets of one stream): each transmission is printed
                                                      # once -- equal frames whose receive times chain within ROWS rows are
                                                      # merged on the device (gnuais_batch_unique) and the earliest intact copy
                                                      # is printed.  Implies --times.  --verbose: "copies N" per transmission on
                                                      # stderr; the summary counts copies and late copies
  ... --unique ROWS --heard
                                                      # who heard each transmission (gnuais_batch_drain_frames_heard): under
                                                      # the sentence(s) of every transmission one line "  heard:" on stdout
                                                      # with, per receiver that decoded a copy, its number, the copy's receive
                                                      # time in rows after the printed copy's (r = repaired), and -- for --iq /
                                                      # --wideband input, measured as for --signal -- its power in dBFS and its
                                                      # carrier error in Hz
  ... --signal
                                                      # --iq / --wideband: how strong every frame was and how far off frequency
                                                      # it arrived, measured on the device over the raw I/Q under the frame
                                                      # (gnuais_batch_frame_signal): one line per frame on stderr with its
                                                      # power in dBFS and its carrier error in Hz.  Implies --times.
  ... --occupancy [BLOCKS]
                                                      # --iq / --wideband: how loaded every channel is (gnuais_batch_occupancy):
                                                      # per receiver and epoch of BLOCKS blocks of 64 rows (default 1024, 1.4 s
                                                      # at 48 kHz) one line on stderr with the load (busy blocks / BLOCKS), the
                                                      # noise floor in dBFS and the share of the busy blocks that lie under a
                                                      # decoded frame.  The end of the file that no epoch covers is not reported.
  ... --long
                                                      # also the messages of three to five slots (427 .. 1008 bits: binary
                                                      # messages, safety text, DGNSS corrections), which the reference's
                                                      # decoder and so the chain give up on: a second decoder on the device
                                                      # (gnuais_batch_long_frames) delivers them, and their two or three
                                                      # sentences follow each call's other sentences -- behind TAG blocks of
                                                      # their own when --times is given; the summary counts them.  With
                                                      # --unique ROWS the copies of a long transmission are merged on the
                                                      # device as well (gnuais_batch_long_unique) and its sentences are
                                                      # printed once; with --heard a "  heard:" line follows them (receiver,
                                                      # rows behind the printed copy, r = repaired, and for --iq / --wideband
                                                      # input the copy's power and carrier error); the summary counts
                                                      # transmissions, copies and late copies.  With --signal every long frame
                                                      # gets its "  signal:" line on stderr like the others
                                                      # (gnuais_batch_long_frame_signal), and with --occupancy the long frames
                                                      # cover their air time
  ... --long-repair
                                                      # --long, and a long frame that fails its CRC by one wrong symbol is
                                                      # repaired on the device (gnuais_batch_long_repair); the summary counts
                                                      # the repairs
  ... --text   prints the reference's stdout lines instead of the bare NMEA sentences
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


CHAIN_RATE = 48000      # rows per second of the chain this script builds (the default table: ReceiverBatch without taps / pllinc)


def wideband_arg(v):
    return "auto" if v == "auto" else int(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--raw", type=int, default=0, metavar="CHANNELS")
    ap.add_argument("--text", action="store_true")
    ap.add_argument("--iq", action="store_true", help="the channels are (I, Q) pairs: 2N channels decode as N receivers "
                                                      "through the device's FM discriminator")
    ap.add_argument("--wideband", type=wideband_arg, default=0, metavar="D|auto",
                    help="the (I, Q) pairs are wide streams at D times the chain's rate: tune to every --offsets, "
                         "decimate by D on the device, one receiver per stream and offset (receiver s*K + k); auto: at "
                         "any rate, resampled by the ratio U / D = 48000 / rate (gnuais_batch_resampler)")
    ap.add_argument("--offsets", default="-25000,25000", help="--wideband: offsets in Hz from the tuned frequency")
    ap.add_argument("--rate", type=int, default=0, help="--wideband with --raw: the input rate in Hz")
    ap.add_argument("--format", choices=["cu8", "cs8", "cs16", "cf32"], default=None,
                    help="--wideband: the file is a bare capture of (I, Q) pairs in this sample format (default: the one its "
                         "extension names: .cu8 .cs8 .cs16 .cf32, .u8 .s8 .s16 .f32 .cfile); needs --rate")
    ap.add_argument("--streams", type=int, default=1, metavar="M", help="--format: wide streams interleaved in the file")
    ap.add_argument("--afc", type=int, default=0, metavar="W",
                    help="--iq / --wideband: carrier-error correction over a window of W samples (a multiple of 128; "
                         "2048 suits 48 kHz), 0 = off")
    ap.add_argument("--call", type=int, default=48000,
                    help="frames per device call (at the chain's rate; --wideband auto: rounded down to whole periods of U rows, "
                         "at least one)")
    ap.add_argument("--times", action="store_true",
                    help="a TAG block with the UNIX second of reception in front of every sentence (the frame's receive time "
                         "in input samples, gnuais_batch_frame_times)")
    ap.add_argument("--repair", action="store_true",
                    help="repair frames that fail the CRC by one symbol error (gnuais_batch_repair); the summary on stderr "
                         "counts them and names each by receiver and closing bit")
    ap.add_argument("--unique", type=int, default=0, metavar="ROWS",
                    help="print each transmission once: merge equal frames whose receive times chain within ROWS rows of the "
                         "chain's clock (gnuais_batch_unique; 128 suits receivers of one site); implies --times")
    ap.add_argument("--signal", action="store_true",
                    help="--iq / --wideband: every frame's power (dBFS) and carrier error (Hz) on stderr "
                         "(gnuais_batch_frame_signal); implies --times")
    ap.add_argument("--occupancy", type=int, nargs="?", const=1024, default=0, metavar="BLOCKS",
                    help="--iq / --wideband: per receiver and epoch of BLOCKS blocks of 64 rows (64..4096, default 1024) the "
                         "load, the noise floor in dBFS and the decoded share of the busy blocks, on stderr "
                         "(gnuais_batch_occupancy)")
    ap.add_argument("--heard", action="store_true",
                    help="--unique: under each transmission's sentences one line with the receivers that heard it: number, "
                         "rows after the printed copy, dBFS and Hz (--iq / --wideband)")
    ap.add_argument("--verbose", action="store_true", help="--unique: the copies of every printed transmission, on stderr")
    ap.add_argument("--long", action="store_true",
                    help="also decode the messages of three to five slots (427 .. 1008 bits: binary, safety text, DGNSS), "
                         "which the chain gives up on (gnuais_batch_long_frames); their sentences follow each call's others, "
                         "with TAG blocks when --times is given")
    ap.add_argument("--long-repair", action="store_true",
                    help="--long, and long frames that fail the CRC by one symbol error are repaired (gnuais_batch_long_repair)")
    ap.add_argument("--start", type=int, default=0, metavar="UNIX_SECONDS", help="--times: the second of the file's first sample")
    a = ap.parse_args()
    a.long = a.long or a.long_repair
    if a.unique < 0:
        sys.exit("--unique takes a window in rows, > 0")
    if a.signal and not (a.iq or a.wideband):
        sys.exit("--signal needs --iq or --wideband: it measures the I/Q under a frame, audio input has none")
    if a.occupancy and not (a.iq or a.wideband):
        sys.exit("--occupancy needs --iq or --wideband: it measures the I/Q of a channel, audio input has none")
    if a.heard and not a.unique:
        sys.exit("--heard lists the receivers of a merged transmission: it needs --unique ROWS")
    if a.signal and a.unique:
        sys.exit("--signal is not for --unique: --unique ROWS --heard lists every copy's power and carrier error")
    a.measure = a.signal or (a.heard and bool(a.iq or a.wideband))
    a.times = a.times or a.unique > 0 or a.signal
    if a.times and a.text:
        sys.exit("--times tags NMEA sentences: not with --text")
    import torch
    from gnuais_amd import ReceiverBatch, io, messages_from_frames
    fmt = a.format
    if a.wideband and not a.raw and fmt is None and os.path.splitext(a.path)[1].lower() in io.IQ_EXTENSIONS:
        fmt = io.format_of_path(a.path)
    if fmt and not a.wideband:
        sys.exit("--format needs --wideband: the sample formats are those of wide I/Q captures")
    if fmt:
        return decode_wideband(a, a.rate, io.read_iq_raw(a.path, fmt, a.streams), fmt)
    if a.raw:
        rate, x = a.rate, io.read_raw(a.path, a.raw)
    else:
        rate, x = io.read_wav(a.path)
    n_ch = x.shape[1]
    if a.afc and not (a.iq or a.wideband):
        sys.exit("--afc needs --iq or --wideband: audio input has no carrier")
    if a.wideband:
        return decode_wideband(a, rate, x)
    if a.iq:
        if n_ch % 2:
            sys.exit(f"{a.path}: --iq needs an even channel count (I, Q per receiver), the file has {n_ch}")
        n_ch //= 2
        x = x.reshape(x.shape[0], n_ch, 2)
    b = ReceiverBatch(n_ch, max_len=a.call)
    if a.afc:
        b.afc(a.afc)
        x = afc_flush(x, a.afc // 2)
    seq = np.zeros(n_ch, dtype=np.uint8)
    if a.times or a.occupancy:
        b.frame_times(True)
    if a.repair:
        b.repair(True)
    if a.measure or a.occupancy:
        b.frame_signal(True)
    if a.unique:
        b.unique(a.unique)
    if a.long:
        b.long_frames(True)
    if a.long_repair:
        b.long_repair(True)
    if a.long and a.unique:
        b.long_unique(a.unique)
    if a.long and a.measure:                                # before the occupancy switch: the long frames cover as well
        b.long_frame_signal(True)
    if a.occupancy:
        b.occupancy(a.occupancy)
    for part in io.chunks(x, a.call):
        d = torch.from_numpy(np.ascontiguousarray(part)).cuda()
        if a.iq:
            b.run_iq(d)
        else:
            b.run(d)
        write_sentences(a, b, seq, "iq" if a.iq else "audio", rate or 48000)
        write_long(a, b, seq, "iq" if a.iq else "audio", rate or 48000)
        occupancy_report(a, b)
    c = b.counters()
    sys.stderr.write(f"{int(c['receivedframes'].sum())} frames, {int(c['lostframes'].sum())} CRC errors, "
                     f"{n_ch} channels, {x.shape[0]} samples per channel\n")
    repair_report(a, b)
    afc_report(a, b, 48000)
    if a.long:
        sys.stderr.write(f"{getattr(a, 'long_frames', 0)} long frames (more than two slots)"
                         + (f", {getattr(a, 'long_repaired', 0)} of them repaired" if a.long_repair else "")
                         + (f", printed once from {getattr(a, 'long_copies', 0)} copies, {b.long_unique_late()} more copies "
                            "came after their transmission was printed" if a.unique else "") + "\n")


def write_sentences(a, b, seq, kind, rate):
    """what the batch has decoded since the last call, to stdout; rate: of the input samples (--times)"""
    from gnuais_amd import messages_from_frames, nmea_tagged_from_frames
    if a.unique and a.heard:
        return write_heard(a, b, seq, kind, rate)
    if a.unique:
        frames, times, copies = b.drain_frames_unique()
        a.unique_records = getattr(a, "unique_records", 0) + len(frames)
        a.unique_copies = getattr(a, "unique_copies", 0) + int(copies.sum())
        if a.verbose:
            for f, t, c in zip(frames, times, copies):
                sys.stderr.write(f"  copies {int(c)}: receiver {int(f['channel'])}, row {int(t)}, {int(f['nbits'])} bits\n")
    elif a.signal:
        from gnuais_amd.lib import signal_dbfs, signal_hz
        frames, times, sig = b.drain_frames_signal()
        for f, t, s in zip(frames, times, sig):
            if s["blocks"]:                                # ferr is counted in the chain's rows
                sys.stderr.write(f"  signal: receiver {int(f['channel'])}, row {int(t)}, {signal_dbfs(s['power']):.1f} dBFS, "
                                 f"{signal_hz(s['ferr'], CHAIN_RATE):+.0f} Hz\n")
            else:
                sys.stderr.write(f"  signal: receiver {int(f['channel'])}, row {int(t)}, not measured\n")
    elif a.times:
        frames, times = b.drain_frames_timed()
    if a.times:
        num, den, off = b.time_map_ratio(kind)         # index = (t * num + off) // den: floor(index / rate) in one division
        out = nmea_tagged_from_frames(frames, times, seq, num, off, rate * den, a.start)
    else:
        frames = b.drain_frames()
        nmea, text = messages_from_frames(frames, seq)
        out = text if a.text else nmea
    if a.repair:
        from gnuais_amd.lib import FRAME_REPAIRED
        a.repaired_frames = getattr(a, "repaired_frames", []) + [
            (int(f["channel"]), int(f["end_bit"]) | ((int(f["flags"]) >> 1 & 31) << 32), int(f["nbits"]))
            for f in frames[(frames["flags"] & FRAME_REPAIRED) != 0]]
    sys.stdout.write(out.decode("ascii", "replace"))


def write_long(a, b, seq, kind, rate):
    """--long: the sentences of the long frames closed since the last call, behind that call's other sentences; with
    --times each carries the TAG block of nmea_tagged_from_frames(): "\\c:<unix>*hh\\", from the record's own t"""
    if not a.long:
        return
    from gnuais_amd.receiver import nmea_from_long_frames
    first = members = None
    if a.unique and a.heard:                                # each long transmission once, and who heard it
        frames, copies, first, members = b.drain_long_frames_heard()
    elif a.unique:
        frames, copies = b.drain_long_frames_unique()
    elif a.signal:                                          # as write_sentences: one line per frame on stderr
        from gnuais_amd.lib import signal_dbfs, signal_hz
        frames, sig = b.drain_long_frames_signal()
        for f, s in zip(frames, sig):
            if s["blocks"]:
                sys.stderr.write(f"  signal: receiver {int(f['channel'])}, row {int(f['t'])}, {signal_dbfs(s['power']):.1f} dBFS, "
                                 f"{signal_hz(s['ferr'], CHAIN_RATE):+.0f} Hz\n")
            else:
                sys.stderr.write(f"  signal: receiver {int(f['channel'])}, row {int(f['t'])}, not measured\n")
    else:
        frames = b.drain_long_frames()
    if a.unique:
        a.long_copies = getattr(a, "long_copies", 0) + int(copies.sum())
        if a.verbose:
            for f, c in zip(frames, copies):
                sys.stderr.write(f"  copies {int(c)}: receiver {int(f['channel'])}, row {int(f['t'])}, {int(f['nbits'])} bits\n")
    a.long_frames = getattr(a, "long_frames", 0) + len(frames)
    a.long_repaired = getattr(a, "long_repaired", 0) + int(((frames["flags"] & 0x40) != 0).sum())
    num, den, off = b.time_map_ratio(kind) if a.times else (1, 1, 0)
    for i in range(len(frames)):
        text = nmea_from_long_frames(frames[i:i + 1], seq).decode("ascii", "replace")
        t = int(frames[i]["t"])
        if a.times and t >= 0:
            body = f"c:{a.start + (t * num + off) // (rate * den)}"
            chk = 0
            for ch in body.encode():
                chk ^= ch
            tag = f"\\{body}*{chk:02X}\\"
            text = "".join(tag + line + "\r\n" for line in text.split("\r\n")[:-1])
        sys.stdout.write(text)
        if members is not None:                             # as write_heard: receiver, rows behind the primary, r = repaired,
            from gnuais_amd.lib import signal_dbfs, signal_hz       # and the copy's level and carrier error where measured
            who = []
            for m in members[first[i]:first[i + 1]]:
                txt = f"{int(m['channel'])} {int(m['t']) - t:+d}" + ("r" if int(m["flags"]) & 0x40 else "")
                if m["signal"]["blocks"]:
                    txt += f" {signal_dbfs(m['signal']['power']):.1f}dBFS {signal_hz(m['signal']['ferr'], CHAIN_RATE):+.0f}Hz"
                who.append(txt)
            sys.stdout.write("  heard: " + ", ".join(who) + "\n")


def write_heard(a, b, seq, kind, rate):
    """--unique --heard: every transmission's sentences, and under them the receivers that heard it"""
    from gnuais_amd import nmea_tagged_from_frames
    from gnuais_amd.lib import FRAME_REPAIRED, signal_dbfs, signal_hz
    frames, times, copies, first, members = b.drain_frames_heard()
    a.unique_records = getattr(a, "unique_records", 0) + len(frames)
    a.unique_copies = getattr(a, "unique_copies", 0) + int(copies.sum())
    num, den, off = b.time_map_ratio(kind)
    for i in range(len(frames)):
        out = nmea_tagged_from_frames(frames[i:i + 1], times[i:i + 1], seq, num, off, rate * den, a.start)
        sys.stdout.write(out.decode("ascii", "replace"))
        who = []
        for m in members[first[i]:first[i + 1]]:
            txt = f"{int(m['channel'])} {int(m['t']) - int(times[i]):+d}" + ("r" if int(m["flags"]) & FRAME_REPAIRED else "")
            if m["signal"]["blocks"]:                       # ferr is counted in the chain's rows
                txt += f" {signal_dbfs(m['signal']['power']):.1f}dBFS {signal_hz(m['signal']['ferr'], CHAIN_RATE):+.0f}Hz"
            who.append(txt)
        sys.stdout.write("  heard: " + ", ".join(who) + "\n")
    if a.repair:
        a.repaired_frames = getattr(a, "repaired_frames", []) + [
            (int(f["channel"]), int(f["end_bit"]) | ((int(f["flags"]) >> 1 & 31) << 32), int(f["nbits"]))
            for f in frames[(frames["flags"] & FRAME_REPAIRED) != 0]]


def afc_flush(x, rows, fmt=None):
    """The AFC delays the audio by half its window: that many zero pairs push the end of the file through the chain.
    A format's zero is 0 for cs16, cs8 and cf32; no cu8 byte converts to 0 (zero lies at 127.5), so cu8 is flushed with
    128, which converts to +128: a constant, like zero, and 0.4 % of full scale."""
    return np.concatenate([x, np.full((rows,) + x.shape[1:], 128 if fmt == "cu8" else 0, dtype=x.dtype)])


def repair_report(a, b):
    """--unique: transmissions against copies; --repair: how many of the CRC errors came back, and which sentences"""
    if a.unique:
        sys.stderr.write(f"{getattr(a, 'unique_records', 0)} transmissions printed once from {getattr(a, 'unique_copies', 0)} "
                         f"copies, {b.unique_late()} more copies came after their transmission was printed\n")
    if a.repair:
        sys.stderr.write(f"{int(b.repaired().sum())} of the CRC errors repaired (one symbol error each; they are among the "
                         "sentences above)\n")
        for c, e, n in getattr(a, "repaired_frames", []):
            sys.stderr.write(f"  repaired: receiver {c}, closing bit {e}, {n} bits\n")


def occupancy_report(a, b):
    """--occupancy: the epochs that became final since the last call, one line per receiver and epoch"""
    if not a.occupancy:
        return
    from gnuais_amd.lib import floor_dbfs
    first, rec = b.drain_occupancy()
    for f, row in zip(first, rec):
        for c, r in enumerate(row):
            share = f"{100.0 * r['covered'] / r['busy']:.0f} %" if r["busy"] else "-"
            sys.stderr.write(f"  occupancy: receiver {c}, blocks {int(f)}..{int(f) + a.occupancy - 1}, load "
                             f"{100.0 * r['busy'] / a.occupancy:.1f} %, floor {floor_dbfs(r['floor']):.1f} dBFS, "
                             f"{int(r['bursts'])} bursts, decoded {share} of busy\n")


def afc_report(a, b, rate):
    if a.afc:
        hz = b.afc_estimate().astype(np.float64) * rate / 65536.0
        sys.stderr.write("carrier error at the end of the file, Hz per receiver: " + " ".join(f"{v:+.0f}" for v in hz) + "\n")


def decode_wideband(a, rate, x, fmt=None):
    """x: int16 [len][2M] from a WAV or int16 file, or (fmt given) [len][M][2] in the format's own dtype"""
    import torch
    from gnuais_amd import ReceiverBatch, io, messages_from_frames
    import math
    if a.wideband == "auto":
        if rate <= 0:
            sys.exit(f"{a.path}: --wideband auto needs the input rate (--rate for raw files)")
        U, D = 48000 // math.gcd(rate, 48000), rate // math.gcd(rate, 48000)
        if (U >= D and (U, D) != (1, 1)) or U > 64 or D > 1024:       # 48000 itself: the channeliser at D = 1
            sys.exit(f"{a.path}: input rate {rate} Hz is {D}/{U} of the chain's 48000 Hz: outside 1 <= U <= 64, U < D <= 1024")
    else:
        U, D = 1, a.wideband
    offsets = [int(v) for v in a.offsets.split(",") if v.strip()]
    if fmt is None and x.shape[1] % 2:
        sys.exit(f"{a.path}: --wideband needs an even channel count (I, Q per stream), the file has {x.shape[1]}")
    if rate <= 0 or rate * U != 48000 * D:              # auto: true by construction
        sys.exit(f"{a.path}: input rate {rate} Hz / {D} is not the chain's 48000 Hz (--rate for raw files)")
    M = x.shape[1] if fmt else x.shape[1] // 2
    n_ch = M * len(offsets)
    x = x[: x.shape[0] // D * D].reshape(-1, M, 2)
    b = ReceiverBatch(n_ch, max_len=max(a.call, U))
    if a.wideband == "auto":
        b.channeliser_for_rate(rate, offsets)
    else:
        b.channeliser(D, rate, offsets)
    if a.afc:
        b.afc(a.afc)
        x = afc_flush(x, -(-(a.afc // 2) // U) * D, fmt)
    seq = np.zeros(n_ch, dtype=np.uint8)
    if a.times or a.occupancy:
        b.frame_times(True)
    if a.repair:
        b.repair(True)
    if a.measure or a.occupancy:
        b.frame_signal(True)
    if a.unique:
        b.unique(a.unique)
    if a.long:
        b.long_frames(True)
    if a.long_repair:
        b.long_repair(True)
    if a.long and a.unique:
        b.long_unique(a.unique)
    if a.long and a.measure:                                # before the occupancy switch: the long frames cover as well
        b.long_frame_signal(True)
    if a.occupancy:
        b.occupancy(a.occupancy)
    # --call counts chain rows; a wide call is whole periods of D samples = U rows each, at least one
    for part in io.chunks(x, max(a.call // U, 1) * D):
        b.run_wideband(torch.from_numpy(np.ascontiguousarray(part)).cuda(), fmt=fmt)
        write_sentences(a, b, seq, "wideband", rate)
        write_long(a, b, seq, "wideband", rate)
        occupancy_report(a, b)
    c = b.counters()
    sys.stderr.write(f"{int(c['receivedframes'].sum())} frames, {int(c['lostframes'].sum())} CRC errors, "
                     f"{M} streams x {len(offsets)} offsets, {x.shape[0]} wide samples per stream\n")
    repair_report(a, b)
    afc_report(a, b, 48000)


if __name__ == "__main__":
    main()
