"""The long-table slicer kernels on the inputs built to break their certification (tests/slicer_cert_ref.py; what
makes those inputs adversarial is shown on the CPU by tests/test_slicer_cert_cpu.py): a lone opponent under an omitted
tap against a small central sum at every phase of the kernel's period, the omitted taps at their limit against a central
sum swept across the threshold, one sample in digital silence, and all of it again across call seams.  Sign words ==
(the oracle's filter > 0), sample for sample, under every chunking; peak, bits, PLL carry, frames and counters too."""
import numpy as np
import pytest

import slicer_cert_ref as sr
from chain_parity import batch, dev, run_both
from gnuais_amd import params
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

CASES = [("packed40", 70), ("packed48", 70), ("mfma", 64), ("mfma", 128)]


@pytest.mark.parametrize("name,n_ch", CASES)
def test_certified_signs_are_the_reference_signs(name, n_ch, tmp_path):
    taps = params.taps_192k()
    case = sr.make_case(taps, name, n_ch, tmp_path, sanitize=False)
    f, x, rows = case.form, case.x, case.x.shape[0]
    kw = dict(taps=taps, pllinc=params.PLLINC_192K)
    options = dict(f.options, fir_T=sr.FIR_T)
    print(f"{name} x {n_ch}: {rows} rows, {len(case.b.pats)} patterns, T {case.T}, head {case.head}; a lone opponent reaches taps "
          f"{ {cls: [q - f.j0 if q < f.j0 else q - f.j0 - f.nc + 1 for q in qs] for cls, qs in sr.reach(f).items()} }")
    # the kernel under test is the one the plan says: the matrix pipe for whole groups of 64 channels and calls past the head
    for ck in ("one call", "calls of 1920 + 1 rows"):
        assert {case.plan_of[n][0] for n in case.chunks[ck] if n > 640} == {"packed+mfma" if f.matrix else "packed"}
    assert case.T == sr.FIR_T and case.head == (640 if f.matrix else 0)
    xd = dev(x)
    for ck, chunks in case.chunks.items():
        b = batch(n_ch, max_len=max(chunks), **kw)
        for k, v in options.items():
            b.set_option(k, v)
        assert b.info("sign_exact") == 1 and b.info("sign_central_taps") == (40 if f.matrix else f.nc)
        assert b.info("sign_matrix_pipe") == (1 if f.matrix else 0)
        o = Oracle(n_ch, **kw)
        pos = 0
        for i, n in enumerate(chunks):
            r = o.run(x[pos:pos + n], want_filtered=True)
            want = (r["filtered"] > 0).T.astype(np.uint8)
            b.run(xd[pos:pos + n])
            got = b.last_signs(n)
            if not np.array_equal(got, want):
                bad = np.argwhere(got != want)
                pytest.fail(f"{name}, {ck}, call {i} (rows {pos} .. {pos + n - 1}): {len(bad)} signs differ; first: " +
                            "; ".join(f"{sr.describe(case.b, pos + int(t), int(c))} got {got[c, t]}" for c, t in bad[:8]))
            # the positive peak of the call (family C's lone samples, the -32768 rows that must not count)
            assert np.array_equal(b.maxval(), r["maxval"]), (ck, i)
            pos += n
        assert pos == rows
        b.close()
    # and the chain behind the slicer on the same input: bits, PLL carry, frames, counters
    run_both(x, [rows], n_ch, options=options, **kw)
