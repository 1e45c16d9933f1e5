"""The adversarial inputs of tests/test_slicer_cert_gpu.py have teeth -- shown without a GPU.

tests/slicer_cert_ref.py restates the certification rule of the three long-table slicer kernels (fir_sign_pk.hip at 40
and 48 central taps, fir_sign_mfma.hip) with the rule as a parameter.  Here: on the inputs the GPU test feeds, the rule
as the kernels' comments state it never certifies a sign the oracle's filter contradicts; each way of getting the rule
subtly wrong does (or cannot, by arithmetic that the test checks and prints); every phase of every kernel's period holds
a pattern that would notice.  Expected values are always the oracle's `filtered > 0`."""
import numpy as np
import pytest

import slicer_cert_ref as sr
from gnuais_amd import params
from oracle_lib import Oracle

FORMS = [("packed40", 70), ("packed48", 70), ("mfma", 64)]
MUTANT_CHUNKINGS = ("one call", "family D cuts")


class Run:
    pass


_RUNS = {}


@pytest.fixture(scope="module", params=FORMS, ids=[f[0] for f in FORMS])
def run(request, tmp_path_factory):
    name, n_ch = request.param
    if name not in _RUNS:
        r = Run()
        taps = params.taps_192k()
        r.case = sr.make_case(taps, name, n_ch, tmp_path_factory.mktemp("cert_" + name))
        r.sums = sr.central_sums(r.case.form, r.case.x)
        r.ref = Oracle(n_ch, taps=taps).run(r.case.x, want_filtered=True)["filtered"]
        r.pos = r.ref > 0
        r.sound = {k: sr.model(r.case.form, r.case.x, c, r.case.plan_of, sums=r.sums) for k, c in r.case.chunks.items()}
        _RUNS[name] = r
    return _RUNS[name]


def by_family(b, mask):
    out = {}
    for o in b.owner[mask]:
        k = b.pats[o]["family"] if o >= 0 else "no pattern"
        out[k] = out.get(k, 0) + 1
    return out


def test_the_sound_rule_never_certifies_a_wrong_sign(run):
    """0 wrong certifications under every chunking; and the bound test of tests/test_fir_plan_cpu.py extended to the
    M-scaled thresholds under adversarial input: |y_c - y_ref| <= the threshold the kernel applies, at every output."""
    c, f = run.case, run.case.form
    print(f"{f.name}: {c.x.shape[0]} rows x {c.n_ch} channels, {len(c.b.pats)} patterns, T {c.T}, head {c.head}")
    for name, res in run.sound.items():
        w = sr.wrong(res, run.pos)
        kernels = sorted({c.plan_of[n][0] for n in c.chunks[name]})
        print(f"  {name} ({len(c.chunks[name])} calls, {'/'.join(kernels)}): {int(res['cert'].sum())} certified, {int(res['zero'].sum())} taken "
              f"for silence, {int((~res['cert'] & ~res['zero']).sum())} left to the exact sum, WRONG {int(w.sum())}")
        assert w.sum() == 0, [sr.describe(c.b, n, ch) for n, ch in np.argwhere(w)[:5]]
        unit = np.where(res["cls"] < 0, 256.0 / f.S if f.matrix else 1.0, 1.0)        # the matrix pipe counts in units of 256 / S
        err = np.abs(res["yc"] * unit - run.ref.astype(np.float64))
        live = ~res["zero"]
        worst = float(np.max(err[live] / (res["thr"] * unit)[live]))
        print(f"    largest |y_c - y_ref| against the applied threshold: {worst:.4f}")
        assert worst <= 1.0
    if f.matrix:
        assert {c.plan_of[n][0] for n in c.chunks["one call"]} == {"packed+mfma"}


def _exempt(f, name, rule):
    """Why a mutant cannot bite, where arithmetic forbids it (None: it has to)"""
    rc = sr.reach(f)
    reachable = {q for qs in rc.values() for q in qs}
    if name == "class one later":
        # a later class prices more taps at full scale: its threshold is at least the sound one for every M in [0, 32768]
        # (at M = 32768 both are 1.1 x the whole bound, split differently: equal up to the two float32 roundings)
        ok = all(f.ahead_k[q + 1] >= f.ahead_k[q] and
                 np.float64(f.seen_k[q + 1]) + f.ahead_k[q + 1] >= (np.float64(f.seen_k[q]) + f.ahead_k[q]) * (1 - 2.0 ** -22) for q in range(3))
        return "its threshold is never below the sound one (checked at M = 0 and 32768; it is linear in M)" if ok else None
    if name == "one history turn fewer":
        U = sr.unroll(f.nc)
        lost = [j for j in range(f.j0) if f.nc - 1 + f.j0 - j > U * (rule.nhist - 1)]
        if not set(lost) & reachable:
            return (f"{rule.nhist - 1} turn(s) of {U} rows still cover all but taps {lost} behind a turn's first output, and no lone "
                    f"opponent under those outweighs a certifiable central sum")
    if name == "threshold x 0.8" and f.matrix:
        # what an input can do: the omitted taps and the quantisation at their limit, M everywhere, + 1 for the floor; the
        # rest of the threshold is the reference's worst-case rounding, which no input is known to reach
        outer = np.abs(f.te.astype(np.float64))
        outer = outer[:f.j0].sum() + outer[f.j0 + f.nc:].sum()
        bq = np.abs(np.asarray(f.tq) / f.S - f.te[f.j0:f.j0 + f.nc].astype(np.float64)).sum()
        share = max((M * (outer + bq) * f.S / 256.0 + 1.0) / np.ceil(0.8 * np.float32(f.seen_u * M + f.abs_u)) for M in (1, 2, 300, 12000, 32768))
        if share < 1.0:
            return f"omitted taps, quantisation and floor at their limit reach {share:.3f} of the scaled threshold at most"
    return None


def test_each_mutant_certifies_a_wrong_sign(run):
    """Every listed way of getting M, the class or the threshold wrong flips at least one sign on these inputs -- or is
    exempt BY NAME with the arithmetic that says why no input can catch it."""
    c, f = run.case, run.case.form
    print(f"{f.name}: wrong outputs per mutant over {MUTANT_CHUNKINGS}")
    for name, rule in sr.mutants(f).items():
        n_wrong, fam = 0, {}
        for ck in MUTANT_CHUNKINGS:
            w = sr.wrong(sr.model(f, c.x, c.chunks[ck], c.plan_of, rule=rule, sums=run.sums), run.pos)
            n_wrong += int(w.sum())
            for k, v in by_family(c.b, w).items():
                fam[k] = fam.get(k, 0) + v
        why = _exempt(f, name, rule)
        print(f"  {name}: {n_wrong} {fam}" + (f"   EXEMPT: {why}" if why else ""))
        if why is None:
            assert n_wrong > 0, name
        else:
            assert n_wrong == 0, (name, "exempt but it bites: drop the exemption")
    exempt = sorted(n for n, r in sr.mutants(f).items() if _exempt(f, n, r))
    assert exempt == {"packed40": ["class one later", "one history turn fewer"], "packed48": ["class one later"],
                      "mfma": ["threshold x 0.8"]}[f.name]


def test_teeth_census(run):
    """Every phase of the kernel's period holds a family-A pattern on each side of the centre that a kernel whose M missed
    the opponent's row would get wrong, and a family-C pattern; where a (class, side) can hold none, the census says so."""
    c, f = run.case, run.case.form
    res = run.sound["one call"]
    rc = sr.reach(f)
    rel = lambda q: q - f.j0 if q < f.j0 else q - f.j0 - f.nc + 1
    print(f"{f.name}: omitted taps a lone opponent reaches, by class (-k: k-th behind the centre, +k: k-th ahead): "
          f"{ {cls: [rel(q) for q in qs] for cls, qs in rc.items()} }")
    teeth = {}
    counts = {}
    for p in c.b.pats:
        key = (p["family"], p["phase"])
        counts[key] = counts.get(key, 0) + 1
        if p["family"] not in ("A", "D") or p.get("tap") is None:
            continue
        n, ch = p["n"], p["c"]
        # the spacing: nothing but the pattern's own samples is under the sound maximum of its designated output
        if p["family"] == "A" and res["cls"][n, ch] == (-1 if f.matrix else p["cls"]):
            assert res["M"][n, ch] == max(abs(p["V"]), abs(p["a"])), sr.describe(c.b, n, ch)
        if f.matrix and res["cls"][n, ch] >= 0:
            continue                                    # an output of the head: the packed kernel's, not this form's
        y = res["yc"][n, ch] * (256.0 / f.S if f.matrix else 1.0)
        fooled = abs(y) >= sr.thr_at(f, abs(p["a"]), p["cls"]) and (y > 0) != run.pos[n, ch]
        assert fooled, sr.describe(c.b, n, ch)
        assert not res["cert"][n, ch]
        if p["family"] == "A":
            teeth[(p["phase"], p["side"])] = teeth.get((p["phase"], p["side"]), 0) + 1
    missing, exempt = [], set()
    for ph in range(f.period):
        cls = sr.class_of(f, ph)
        for side in ("behind", "ahead"):
            if not [q for q in rc[cls] if sr.side_of(f, q) == side]:
                exempt.add((cls, side))
            elif not teeth.get((ph, side)):
                missing.append((ph, side))
        if not counts.get(("C", ph)):
            missing.append((ph, "C"))
    print(f"  patterns per family: { {k: sum(v for (fm, _), v in counts.items() if fm == k) for k in 'ABCD'} }")
    print("  per phase A behind / A ahead / C: " + " ".join(f"{ph}:{teeth.get((ph, 'behind'), 0)}/{teeth.get((ph, 'ahead'), 0)}/{counts.get(('C', ph), 0)}"
                                                          for ph in range(f.period)))
    for cls, side in sorted(exempt):
        print(f"  class {cls}, {side}: no tooth -- ahead_k[{cls}] = {f.ahead_k[cls]:.3e} prices every tap from the "
              f"{7 - 2 * cls}th ahead at full scale and exceeds 32768 x the largest omitted tap "
              f"({32768 * float(f.te[f.j0 - 1]):.3e}), which bounds what any lone opponent adds")
    assert not missing, missing
    # class 3 alone is without family-A teeth, on both sides, and for the reason printed
    assert exempt == (set() if f.matrix else {(3, "behind"), (3, "ahead")})
    if not f.matrix:
        assert f.ahead_k[3] > 32768 * float(f.te[f.j0 - 1])


def test_the_patterns_do_what_they_say(run):
    c, f = run.case, run.case.form
    res = run.sound["one call"]
    te = f.te.astype(np.float64)
    a_pats = [p for p in c.b.pats if p["family"] in ("A", "D") and p.get("tap") is not None]
    for p in a_pats[::7]:
        want = p["a"] * te[p["j"]] + p["V"] * te[p["tap"]]
        got = float(run.ref[p["n"], p["c"]])
        assert abs(got - want) <= 1e-6 * (abs(p["a"] * te[p["j"]]) + abs(p["V"] * te[p["tap"]])), sr.describe(c.b, p["n"], p["c"])
        assert (got > 0) == (p["V"] * te[p["tap"]] > 0)                      # the reference's sign is the opponent's
    # B: the central sum sweeps the applied threshold on both sides, the omitted taps stand at their limit
    fr = {}
    for p in (p for p in c.b.pats if p["family"] == "B"):
        n, ch = p["n"], p["c"]
        if f.matrix and res["cls"][n, ch] >= 0:
            continue
        assert res["M"][n, ch] == p["M"], sr.describe(c.b, n, ch)
        got = res["yc"][n, ch] / res["thr"][n, ch]
        fr.setdefault((p["cls"], p["M"]), []).append(abs(got))
        exact = sum(v * te[j] for j, v in p["samples"].items())
        assert abs(float(run.ref[n, ch]) - exact) <= 1e-3 * max(abs(exact), 1e-3)
        unit = 256.0 / f.S if f.matrix else 1.0
        omitted = sum(v * te[j] for j, v in p["samples"].items() if j < f.j0 or j >= f.j0 + f.nc)
        assert abs(res["yc"][n, ch] * unit + omitted - exact) <= res["thr"][n, ch] * unit
    for key, v in sorted(fr.items()):
        print(f"  B class {key[0]} M {key[1]}: |y_c| / threshold from {min(v):.3f} to {max(v):.3f}, {sum(x < 1 for x in v)} below, {sum(x >= 1 for x in v)} at or above")
        assert min(v) < 0.7 and max(v) > 1.15 and sum(x < 1 for x in v) >= 8 and sum(x >= 1 for x in v) >= 8, key
    # C: every output whose window holds the lone positive sample is positive, across all effective taps
    for p in (p for p in c.b.pats if p["family"] in ("C", "D") and p.get("tap") is None):
        col = run.ref[p["n"]:p["n"] + f.ne, p["c"]]
        assert len(col) == min(f.ne, c.x.shape[0] - p["n"]) and (col > 0).all(), sr.describe(c.b, p["n"], p["c"])
