#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ from the REAL reference.

Runs only in the build container: it needs oracle/_ref/libgnuais_ref.so, i.e.
the unmodified gnuais translation units compiled in place from /root/reference
(recipe: oracle/Makefile).  The fixtures are data only -- int16 inputs and the
reference's outputs on them (fp32 bit patterns, recovered bits, frames,
counters, final PLL/FSM state).  Re-run with:  python tests/golden/make_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cases  # noqa: E402
from gnuais_amd import params  # noqa: E402
from oracle_lib import reference  # noqa: E402


def frames_raw(f):
    return np.frombuffer(f.tobytes(), dtype=np.uint8).reshape(-1, 64).copy()


def run_chain(x, taps=None, pllinc=0, chunk=1020):
    """Full chain through the reference; one receiver per interleaved channel."""
    ref = reference()
    n_ch = x.shape[1]
    ref.add_receivers(n_ch, taps=taps, pllinc=pllinc)
    t = ref.taps(0)
    out = {"x": x, "taps": t.view(np.uint32), "pllinc": np.uint32(pllinc or params.PLLINC_48K)}
    # floats: filter_run_buf on a private filter per channel
    filt = np.zeros(x.shape, dtype=np.uint32)
    maxv = np.zeros(n_ch, dtype=np.int16)
    for c in range(n_ch):
        f, mv = ref.filter_stream(t, x[:, c].copy(), 1, x.shape[0], x.shape[0])
        filt[:, c] = f.view(np.uint32)
        maxv[c] = mv[0]
    out["filtered_u32"] = filt
    out["maxval"] = maxv
    # bits: one pass per channel so each channel's bit stream is captured alone
    for c in range(n_ch):
        ref.reset()
        ref.add_receivers(n_ch, taps=taps, pllinc=pllinc)
        ref.run_stream(x, chunk, capture_bits_of=c)
        out[f"bits{c}"] = ref.bits()
    out["frames"] = frames_raw(ref.frames())
    out["counters"] = ref.counters()
    out["pll"] = np.array([ref.pll(c) for c in range(n_ch)], dtype=np.int64)
    out["fsm"] = np.array([list(ref.fsm(c).values()) for c in range(n_ch)], dtype=np.int32)
    return out


def make_nmea():
    """Row f1: frame records -> the sentences the reference's protodec_getdata() emits."""
    ref = reference()
    out = {}
    fr, n_ch = cases.nmea_frames()
    text, seq, printed = ref.nmea_of_frames(fr, n_ch, stdout=True)
    out["synthetic_frames"] = frames_raw(fr)
    out["synthetic_nch"] = np.array([n_ch])
    out["synthetic_text"] = np.frombuffer(text, dtype=np.uint8)
    out["synthetic_stdout"] = np.frombuffer(printed, dtype=np.uint8)
    out["synthetic_seqnr"] = seq
    for name in ("chain_48k", "chain_long"):       # frames the reference itself decoded
        g = np.load(os.path.join(HERE, name + ".npz"))
        fr = np.frombuffer(np.ascontiguousarray(g["frames"]).tobytes(), dtype=cases_frame_dtype())
        n_ch = int(fr["channel"].max()) + 1
        text, seq, printed = ref.nmea_of_frames(fr, n_ch, stdout=True)
        out[name + "_text"] = np.frombuffer(text, dtype=np.uint8)
        out[name + "_stdout"] = np.frombuffer(printed, dtype=np.uint8)
        out[name + "_seqnr"] = seq
    np.savez_compressed(os.path.join(HERE, "nmea.npz"), **out)
    print("nmea.npz", os.path.getsize(os.path.join(HERE, "nmea.npz")),
          {k: v.shape for k, v in out.items()})


def make_range():
    """Row f4: frame records -> best_range per channel for several station positions."""
    ref = reference()
    fr, n_ch = cases.range_frames()
    out = {"frames": frames_raw(fr), "nch": np.array([n_ch]),
           "stations": np.array(cases.RANGE_STATIONS, dtype=np.float32)}
    out["best_range"] = np.stack([ref.range_of_frames(fr, n_ch, la, lo) for la, lo in cases.RANGE_STATIONS])
    fr1, n1 = cases.range_frames(n_random=400, own_channel=True)       # one fix per channel: every distance
    out["single_frames"] = frames_raw(fr1)
    out["single_range"] = np.stack([ref.range_of_frames(fr1, n1, la, lo) for la, lo in cases.RANGE_STATIONS])
    np.savez_compressed(os.path.join(HERE, "range.npz"), **out)
    print("range.npz", os.path.getsize(os.path.join(HERE, "range.npz")), out["best_range"],
          "distinct single distances", len(np.unique(out["single_range"])))


def make_vessels():
    """Row f3: frame records -> the reference's position cache, flattened."""
    ref = reference()
    fr, n_ch = cases.vessel_frames()
    tab = ref.cache_of_frames(fr, n_ch)
    out = {"frames": frames_raw(fr), "nch": np.array([n_ch]),
           "vessels": np.frombuffer(tab.tobytes(), dtype=np.uint8)}
    np.savez_compressed(os.path.join(HERE, "vessels.npz"), **out)
    print("vessels.npz", os.path.getsize(os.path.join(HERE, "vessels.npz")), len(tab), "vessels; set bits",
          {int(b): int((tab["set"] == b).sum()) for b in np.unique(tab["set"])})


def make_fir_plan(harness):
    """fir_plan.npz: what the host derives from a tap table (the sign-exact slicer's bounds) and decides per call (kernel,
    segment length, thresholds), for tests/test_fir_plan_cpu.py.  FROZEN FROM THE COMMIT BEFORE gnuais_amd/csrc/fir_plan.cpp
    EXISTED, never from fir_plan.cpp itself: `harness` is a program that speaks the protocol of tests/fir_plan_cases.py and
    holds that commit's code verbatim -- gnuais_batch_create's bound block, fir_sign_mfma_taps, fill_fir, run_fir (launchers
    stubbed to record their FirLaunch) and gnuais_batch_info's sign_* lines behind a stub struct, built with
    g++ -O1 -std=c++17 -ffp-contract=off.  Re-running this needs such a harness again; the values do not change otherwise."""
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "scripts"))
    import fir_plan_cases as fc
    import fuzz_parity
    tables = [("48k", params.taps_48k()), ("192k", params.taps_192k())]
    for seed in fc.RANDOM_SEEDS:
        t, _, name = fuzz_parity.table(np.random.default_rng(seed))
        assert name.startswith("rand"), (seed, name)
        tables.append((f"s{seed}", t))
    with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
        f.write(fc.driver_input(tables, fc.PLAN_TABLES))
        f.flush()
        text = subprocess.run([harness, f.name], capture_output=True, text=True, check=True).stdout
    bounds, plans = fc.parse(text)
    out = {"names": np.array([n for n, _ in tables]),
           "taps": np.concatenate([np.asarray(t, dtype=np.float32).view(np.uint32) for _, t in tables]),
           "taps_len": np.array([len(t) for _, t in tables])}
    for k in bounds["48k"]:
        out["b_" + k] = np.stack([bounds[n][k] for n, _ in tables])
    out["plan_rows"] = np.array([len(plans[n]["kernel"]) for n in fc.PLAN_TABLES])
    for k in plans["48k"]:
        out["p_" + k] = np.concatenate([plans[n][k] for n in fc.PLAN_TABLES])
    path = os.path.join(HERE, "fir_plan.npz")
    np.savez_compressed(path, **out)
    census = {}
    for n, _ in tables[2:]:
        b = bounds[n]
        key = (f"NC {b['NC'][0]} forty {b['ok40'][0]} matrix pipe {b['mfma_ok'][0]} FL2 {int(b['fscale'][0] != 0)}"
               if b["ok"][0] else f"not admitted (forty {b['ok40'][0]})")
        census[key] = census.get(key, 0) + 1
    print("fir_plan.npz", os.path.getsize(path), len(tables), "tables,", int(out["plan_rows"].sum()), "plans;", census)


def make_message_sweep():
    """message_sweep.npz: what the reference sends and prints for every frame of tests/message_cases.py.  It may not
    outgrow ref_pins.npz as committed with it (618 165 bytes): thin the integer-only sweeps if it does, never the ones
    that feed a %.Nf field."""
    import ref_pins
    ref_pins.store_message_sweep()
    size = os.path.getsize(ref_pins.MESSAGE_SWEEP)
    print("message_sweep.npz", size)
    assert size <= 618165, size


def cases_frame_dtype():
    from oracle_lib import FRAME_DTYPE
    return FRAME_DTYPE


def main():
    if sys.argv[1:] == ["vessels"]:
        return make_vessels()
    if sys.argv[1:] == ["range"]:
        return make_range()
    if sys.argv[1:2] == ["fir_plan"]:       # + the path of the harness (see make_fir_plan)
        return make_fir_plan(sys.argv[2])
    if sys.argv[1:] == ["nmea"]:
        make_nmea()
        return
    if sys.argv[1:] == ["ref_pins"]:
        import ref_pins
        return ref_pins.store()
    if sys.argv[1:] == ["message_sweep"]:
        return make_message_sweep()
    ref = reference()
    # 1. full chain, 48 kHz, 2 channels (config C1 shape)
    np.savez_compressed(os.path.join(HERE, "chain_48k.npz"), **run_chain(cases.chain_48k()))
    # 2. full chain, 192 kHz parameters (config C5 shape), 1 channel
    np.savez_compressed(os.path.join(HERE, "chain_192k.npz"),
                        **run_chain(cases.chain_192k(), taps=params.taps_192k(),
                                    pllinc=params.PLLINC_192K, chunk=4096))
    # 3. long / odd-length messages
    np.savez_compressed(os.path.join(HERE, "chain_long.npz"), **run_chain(cases.long_messages()))
    # 4. FIR known answers
    ref = reference()
    ref.add_receivers(1)
    taps = ref.taps(0)
    kat = {"taps": taps.view(np.uint32)}
    for name, x in cases.fir_kats().items():
        f, mv = ref.filter_stream(taps, x, 1, x.size, 1020)
        kat["x_" + name] = x
        kat["y_" + name] = f.view(np.uint32)
        kat["m_" + name] = mv
    t192 = params.taps_192k()
    x = cases.fir_kats()["noise_full"]
    f, mv = ref.filter_stream(t192, x, 1, x.size, 1000)
    kat["taps192"] = t192.view(np.uint32)
    kat["y192_noise_full"] = f.view(np.uint32)
    np.savez_compressed(os.path.join(HERE, "fir_kat.npz"), **kat)
    # 5. CRC-16
    blobs = cases.crc_cases()
    crc = {"data": np.frombuffer(b"".join(blobs), dtype=np.uint8),
           "lens": np.array([len(b) for b in blobs], dtype=np.int32),
           "crc": np.array([ref.sdlc_crc(b) for b in blobs], dtype=np.uint16)}
    np.savez_compressed(os.path.join(HERE, "crc16.npz"), **crc)
    # 6. deframer on raw bit sequences (protodec_decode)
    fsm = {}
    for name, bits in cases.fsm_bit_cases().items():
        ref = reference()
        ref.add_receivers(1)
        ref.decode_bits(0, bits)
        fsm["bits_" + name] = np.packbits(bits)
        fsm["n_" + name] = np.int64(bits.size)
        fsm["frames_" + name] = frames_raw(ref.frames())
        fsm["counters_" + name] = ref.counters()[0]
        fsm["fsm_" + name] = np.array(list(ref.fsm(0).values()), dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "deframer_bits.npz"), **fsm)
    make_nmea()
    # 7. the reference's answers on the seeded inputs of the pin tests (tests/ref_pins.py)
    import ref_pins
    ref_pins.store()
    # 8. the sentences and stdout lines of the field sweeps (tests/message_cases.py)
    make_message_sweep()
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
