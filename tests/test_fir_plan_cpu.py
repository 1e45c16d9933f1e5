"""gnuais_amd/csrc/fir_plan.cpp on the CPU: the sign-exact slicer's error bounds and the choice of the FIR kernel.

Every decoded bit is the reference's because K1s trusts the sign of its central sum only where |y_c| > eps, and eps is
host arithmetic on the tap table.  The GPU parity tests show that eps was large enough for the inputs they tried; these
show that the numbers are what they were before the module existed (tests/golden/fir_plan.npz, frozen from the commit
before it: tests/golden/make_golden.py), that gnuais_batch_info() and the launch decision are one answer, and that the
bound holds against the oracle's exact filter where a CPU can check it.  The module runs behind tests/c/fir_plan_main.cpp,
built on demand with AddressSanitizer + UndefinedBehaviorSanitizer (`make -C tests/c fir_plan`)."""
import os

import numpy as np
import pytest

import fir_plan_cases as fc
from gnuais_amd import params
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_GENERIC, K_SCALAR32, K_SIGN, K_PACKED, K_PACKED_MFMA = range(5)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "fir_plan.npz"))
    names = [str(n) for n in g["names"]]
    off = np.concatenate([[0], np.cumsum(g["taps_len"])])
    tables = [(n, g["taps"][off[i]:off[i + 1]].view(np.float32)) for i, n in enumerate(names)]
    return g, names, tables


@pytest.fixture(scope="module")
def driver(golden, tmp_path_factory):
    """The driver's answer on the fixture's tables and the plan grid: (bounds, plans) of fir_plan_cases.parse"""
    _, _, tables = golden
    return fc.run_driver(fc.driver_input(tables, fc.PLAN_TABLES), tmp_path_factory.mktemp("fir_plan"))


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def test_the_fixture_holds_the_tables_and_the_outcomes_it_promises(golden):
    g, names, tables = golden
    assert names[:2] == ["48k", "192k"] and len(names) >= 42
    assert np.array_equal(tables[0][1].view(np.uint32), params.taps_48k().view(np.uint32))
    assert np.array_equal(tables[1][1].view(np.uint32), params.taps_192k().view(np.uint32))
    ok, nc, ok40, mfma = (g["b_" + k][2:, 0] for k in ("ok", "NC", "ok40", "mfma_ok"))
    fl2 = g["b_fscale"][2:, 0] != 0
    ne = np.array([len(fc.trim(t)[2]) for _, t in tables[2:]])
    for what, sel in (("not admitted", ok == 0), ("more than 128 effective taps", ne > 128), ("12 central taps", (ok == 1) & (nc == 12)),
                      ("48 with 40", (ok == 1) & (nc == 48) & (ok40 == 1)), ("48 without 40", (ok == 1) & (nc == 48) & (ok40 == 0)),
                      ("48 with the matrix pipe", (nc == 48) & (mfma == 1)), ("48 without the matrix pipe", (ok == 1) & (nc == 48) & (mfma == 0)),
                      ("12 with an FL2 scale", (nc == 12) & (ok == 1) & fl2), ("12 without an FL2 scale", (nc == 12) & (ok == 1) & ~fl2)):
        assert sel.sum() >= 2, what
    assert not g["b_ok"][2:][ne > 128].any()
    # the pins of the two tables the project ships, as hex floats
    want = {"48k": dict(NC=12, eps="0x1.be185ap-4", eps_pk="0x1.16ff88p-3", seen="0x1.ba18bcp-4", ahead="0x1.ffceb4p-11",
                        fscale="0x1p+4", ok40=0, mfma_ok=0),
            "192k": dict(NC=48, eps="0x1.f3cf66p-2", eps_pk="0x1.f3cf66p-2", seen="0x1.f16adap-2", ahead="0x1.324636p-9",
                         fscale="0x0p+0", ok40=1, eps_pk40="0x1.f34ebp-1", seen40="0x1.6fe8b8p-1", ahead40="0x1.06cbfp-2",
                         mfma_ok=1, mfma_seen_u="0x1.111a9ap-3")}
    for i, name in enumerate(("48k", "192k")):
        for k, v in want[name].items():
            got = g["b_" + k][i, 0]
            assert got == (fc.f32_bits(v)[0] if isinstance(v, str) else v), (name, k)
    # wherever a table is admitted, the share of the bound that scales with the samples seen is positive: the launchers'
    # `eps_seen <= 0` rejections never meet an admitted table
    assert (f32(g["b_seen"][:, 0])[g["b_ok"][:, 0] == 1] > 0).all() and (f32(g["b_seen40"][:, 0])[g["b_ok40"][:, 0] == 1] > 0).all()


def test_bounds_are_the_frozen_ones_bit_for_bit(golden, driver):
    g, names, _ = golden
    bounds, _ = driver
    for k in bounds["48k"]:
        got = np.stack([bounds[n][k] for n in names])
        differ = [names[i] for i in np.nonzero((got != g["b_" + k]).reshape(len(names), -1).any(axis=1))[0]]
        assert not differ, (k, differ)


def test_plans_are_the_frozen_ones(golden, driver):
    g, _, _ = golden
    _, plans = driver
    assert [len(plans[n]["kernel"]) for n in fc.PLAN_TABLES] == list(g["plan_rows"])
    for k in plans["48k"]:
        got = np.concatenate([plans[n][k] for n in fc.PLAN_TABLES])
        assert np.array_equal(got, g["p_" + k]), (k, int((got != g["p_" + k]).reshape(len(got), -1).any(axis=1).sum()))
    kernels = np.concatenate([plans[n]["kernel"][:, 0] for n in fc.PLAN_TABLES])
    assert set(kernels) == set(range(5))                    # the grid reaches every launch shape


def test_info_and_the_plan_are_one_answer(golden, driver):
    _, _, tables = golden
    _, plans = driver
    nt_of = {n: len(t) for n, t in tables}
    for name in fc.PLAN_TABLES:
        p, grid = plans[name], np.array(fc.plan_grid(nt_of[name]))
        kernel, dump = p["kernel"][:, 0], grid[:, 7] == 1
        k1s = kernel >= K_SIGN
        exact = f32(p["sign_exact"][:, 0]) == 1
        assert np.array_equal(k1s, exact & ~dump)
        assert np.array_equal(f32(p["sign_central_taps"][:, 0])[k1s], p["NC"][:, 0][k1s])
        assert np.array_equal(p["sign_eps_seen"][k1s], p["eps_seen"][k1s]) and np.array_equal(p["sign_eps_ahead"][k1s], p["eps_ahead"][k1s])
        direct = kernel == K_SIGN
        assert np.array_equal(p["sign_flag_scale"][direct], p["fscale"][direct])
        fs, eps = f32(p["sign_flag_scale"][:, 0]), f32(p["eps"][:, 0])
        want_eps = np.where(fs > 0, np.float32(2.0) / np.where(fs > 0, fs, 1).astype(np.float32), eps)
        assert np.array_equal(f32(p["sign_eps"][:, 0])[k1s], want_eps[k1s])
        # sign_matrix_pipe says ELIGIBLE: 1 exactly when some call length of the grid takes the matrix pipe
        pipe = f32(p["sign_matrix_pipe"][:, 0]) == 1
        groups = {}
        for row, takes, says in zip(grid, kernel == K_PACKED_MFMA, pipe):
            key = (row[0], *row[2:7])
            some, said = groups.get(key, (False, says))
            assert said == says
            groups[key] = (some or takes, said)
        for key, (some, said) in groups.items():
            assert some == said, (name, key)


# ---------------------------------------------------------------- the bound against the exact filter

def _inputs(taps, j0c, nc, eps, rng, n_rows):
    """int16 [n_rows][16]: full-scale noise, impulses in silence, +-full scale, a square wave, and the patterns of
    tests/test_hip_fullsize.py::test_sign_exact_slicer_on_its_threshold: |y_c| within 10 % of eps on both sides, each
    alone in silence, from three small integers under three central taps of decreasing size -- the first from the
    centre's edge (table index j0c) that reach m = min(eps / 4, the largest tap), m / 25, m / 250: for the reference table
    the test's own 0.0696, 0.0059, 0.00022"""
    nt = len(taps)
    x = np.zeros((n_rows, 16), dtype=np.int16)
    for c in range(0, 6):
        x[:, c] = rng.integers(-32768, 32768, n_rows)
    for c in range(6, 10):
        at = rng.integers(0, n_rows, n_rows // 100)
        x[at, c] = rng.integers(-32768, 32768, len(at))
    for c in range(10, 13):
        x[:, c] = rng.choice(np.array([-32768, 32767], dtype=np.int16), n_rows)
    x[:, 13] = np.where((np.arange(n_rows) // int(rng.integers(1, 9))) % 2, 32767, -32767)
    centre = np.abs(taps[j0c:j0c + nc // 2].astype(np.float64))
    top = min(eps / 4, centre.max())
    k3, k2, k1 = (j0c + int(np.argmax(centre >= top / q)) for q in (1, 25, 250))
    assert k3 > k2 > k1
    t3, t2, t1 = (float(taps[k]) for k in (k3, k2, k1))
    gap, placed, at = 2 * nt, 0, []                         # silence around a pattern: more than a window
    for a in (-3, -2, -1, 1, 2, 3):
        for frac in np.linspace(0.9, 1.1, 41):
            for sgn in (1.0, -1.0):
                rest = sgn * eps * frac - a * t3
                bq = int(np.round(rest / t2))
                cq = int(np.round((rest - bq * t2) / t1))
                c, n = 14 + placed % 2, gap * (placed // 2 + 1)             # the output whose window holds the pattern
                if abs(bq) > 30000 or abs(cq) > 30000 or n + gap >= n_rows:
                    continue
                x[n - nt + k3, c], x[n - nt + k2, c], x[n - nt + k1, c] = a, bq, cq
                at.append((n, c))
                placed += 1
    return x, at


def _central_sum(xp, te, k0, j0, nc, n_rows, paired):
    """y_c in float32, one rounding per product and per addition, in the kernel's documented order.  xp = NT rows of
    silence + the input; the sample under table tap k of output n is xp[n + k]."""
    def under(j):                      # samples under effective tap j, as float32 (exact)
        return xp[k0 + j:k0 + j + n_rows].astype(np.float32)
    y = None
    if paired:                         # 12: symmetric pre-add pairs, edge taps first
        for q in range(nc // 2):
            term = te[j0 + q] * (under(j0 + q) + under(j0 + nc - 1 - q))
            y = term if y is None else y + term
    else:                              # 48 and 40: tap order
        for j in range(j0, j0 + nc):
            term = te[j] * under(j)
            y = term if y is None else y + term
    assert y.dtype == np.float32
    return y


@pytest.mark.parametrize("table,nc", [("48k", 12), ("192k", 48), ("192k", 40)])
def test_the_bound_holds_against_the_exact_filter(golden, driver, table, nc):
    """|y_c - y_ref| <= eps for >= 10^6 outputs per table -- no margin: eps is a proved bound, its 1.1 is inside it -- with
    the global eps of the kernel's order of operations and with eps = seen * M / 32768 + ahead, M = the largest |x| under
    the taps up to the centre's last (the rows a kernel has seen cover at least those).  Plus the input that drives the
    omitted taps to their limit, and a bracket of eps from the table alone."""
    _, _, tables = golden
    bounds, _ = driver
    taps = dict(tables)[table]
    b = bounds[table]
    assert b["ok"][0] == 1 and b["NC"][0] == (12 if nc == 12 else 48) and (nc != 40 or b["ok40"][0] == 1)
    nt, d, te = fc.trim(taps)
    ne, k0 = len(te), nt - d
    j0 = (ne - nc) // 2
    if nc == 40:
        eps, seen, ahead = (float(f32(b[k])[0]) for k in ("eps_pk40", "seen40", "ahead40"))
    else:       # 12: the direct form's bound; 48: the transposed sum's, which is the same number
        eps, seen, ahead = (float(f32(b[k])[0]) for k in ("eps" if nc == 12 else "eps_pk", "seen", "ahead"))
    assert nc != 48 or b["eps"][0] == b["eps_pk"][0]

    # the bracket, from the table alone: the omitted taps are a term of the derivation; the textbook gamma_n bound for both
    # sums is what it refines
    t64 = np.abs(te.astype(np.float64))
    outer = t64[:j0].sum() + t64[j0 + nc:].sum()
    gamma = (1.0 + 2.0 ** -24) ** ne - 1.0
    lo, hi = 1.1 * 32768 * outer, 1.1 * 32768 * (outer + 2 * gamma * t64.sum())
    print(f"{table} {nc}: {lo:.4f} <= eps {eps:.4f} <= {hi:.4f}; seen {seen:.4f} ahead {ahead:.6f}")
    assert lo <= eps <= hi

    n_rows = 70000                                          # x 16 channels: 1.12 million outputs
    x, patterns = _inputs(taps, k0 + j0, nc, eps, np.random.default_rng(20260 + nc), n_rows)
    assert len(patterns) > 100
    # the omitted taps at their limit, alone in silence at the end of the first impulse channel
    n_lim = n_rows - 2 * nt
    x[n_lim - 3 * nt:, 6] = 0
    sign = np.sign(te).astype(np.int32)
    sign[j0:j0 + nc] = 0
    x[n_lim - nt + k0:n_lim - nt + k0 + ne, 6] = np.clip(-32768 * sign, -32768, 32767)
    y_ref = Oracle(16, taps=taps).run(x, want_filtered=True)["filtered"]
    xp = np.concatenate([np.zeros((nt, 16), dtype=np.int16), x])
    y_c = _central_sum(xp, te, k0, j0, nc, n_rows, paired=nc == 12)
    err = np.abs(y_c.astype(np.float64) - y_ref.astype(np.float64))
    near = np.array([abs(float(y_c[n, c])) / eps for n, c in patterns])      # the patterns do what they say: |y_c| around eps
    assert near.min() > 0.85 and near.max() < 1.15 and (near < 1).sum() > 50 and (near > 1).sum() > 50
    m = np.zeros((n_rows, 16), dtype=np.int32)
    for j in range(j0 + nc):
        np.maximum(m, np.abs(xp[k0 + j:k0 + j + n_rows].astype(np.int32)), out=m)
    eps_m = seen * m / 32768.0 + ahead
    print(f"  {err.size} outputs: largest |y_c - y_ref| {err.max():.6f}, largest against seen/ahead {np.max(err / eps_m):.4f} of the bound; "
          f"omitted taps at their limit {err[n_lim, 6]:.6f} (32768 x sum |outer| = {32768 * outer:.6f})")
    assert err.size >= 10 ** 6
    assert abs(err[n_lim, 6] - 32768 * outer) <= 1e-3 * 32768 * outer + 1e-6    # the construction does what it says
    assert err[n_lim, 6] <= eps
    assert err.max() <= eps
    assert (err <= eps_m).all()
