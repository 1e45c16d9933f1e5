"""The HIP chain (through the C ABI) beside the CPU restatement, call by call (TEST INFRASTRUCTURE shared by the GPU
parity tests): run_both() feeds both the same ragged calls and asserts bits, frames, counters, PLL carry and deframer
state equal."""
import numpy as np

from oracle_lib import Oracle

FSM_KEYS = ("state", "nstartsign", "antallpreamble", "antallenner", "bitstuff", "last", "bufferpos")


def batch(*a, **k):
    from gnuais_amd import ReceiverBatch
    return ReceiverBatch(*a, **k)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def fsm_rows(b):
    f = b.fsm_state()
    return [[int(r[k]) for k in FSM_KEYS] for r in f]


def oracle_fsm_rows(o, n, saturate=True):
    rows = []
    for c in range(n):
        h = o.hdlc(c)
        r = [h[k] for k in FSM_KEYS]
        if saturate:
            r[2] = min(r[2], 15)
        rows.append(r)
    return rows


def run_both(x, chunks, n_ch, taps=None, pllinc=0, fir_T=None, pll_variant=0, options=None, each_call=None):
    """each_call(b, o, i, seg, bits): called after call i (rows `seg`) with the batch, the oracle and last_bits()"""
    o = Oracle(n_ch, taps=taps, pllinc=pllinc)
    b = batch(n_ch, taps=taps, pllinc=pllinc, max_len=max(chunks))
    if fir_T:
        b.set_option("fir_T", fir_T)
    for k, v in (options or {}).items():
        b.set_option(k, v)
    b.set_option("pll_variant", pll_variant)      # 0: by channel count (the time-parallel form up to 1536 channels)
    pos = 0
    gbits = [[] for _ in range(n_ch)]
    obits = [[] for _ in range(n_ch)]
    for n in chunks:
        seg = x[pos:pos + n]
        pos += n
        r = o.run(seg, want_bits=True)
        b.run(dev(seg))
        lb = b.last_bits()
        if each_call:
            each_call(b, o, len(gbits[0]), seg, lb)
        for c in range(n_ch):
            gbits[c].append(lb[c])
            obits[c].append(r["bits"][c])
    assert pos == x.shape[0]
    for c in range(n_ch):
        assert np.array_equal(np.concatenate(gbits[c]), np.concatenate(obits[c])), c
    assert b.drain_frames().tobytes() == o.frames().tobytes()
    cnt = b.counters()
    assert np.array_equal(np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]],
                                   axis=1), o.counters())
    p = b.pll_state()
    assert [(int(a), int(bb), int(cc)) for a, bb, cc in zip(p["pll"], p["prev"], p["lastbit"])] == \
        [o.pll(c) for c in range(n_ch)]
    assert fsm_rows(b) == oracle_fsm_rows(o, n_ch)
    return o, b
