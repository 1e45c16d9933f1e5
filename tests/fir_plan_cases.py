"""The tables, the call grid and the text protocol of tests/c/fir_plan_main.cpp (gnuais_amd/csrc/fir_plan.*), shared by
tests/test_fir_plan_cpu.py, tests/slicer_cert_ref.py (the thresholds and plans its model of the slicer kernels works with)
and the fixture's recipe in tests/golden/make_golden.py.

The driver reads
    table NAME NT d NE <NE taps as hex words>       the trimmed table
    plan N len fir_variant fir_T fir_pk_taps fir_flag2 fir_mfma dump
and answers one line each, `bounds k=v ...` / `plan k=v ...`, floats as C hex floats."""
import itertools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "c", "fir_plan.bin")

N_GRID = (1, 64, 66, 16384)
HEAD_192K = 640                 # the packed kernel's share of a call beside the matrix pipe, 192 kHz table
T_GRID = (64, 512, 4096)
# seeds of scripts/fuzz_parity.py's table(), kinds 6-9 (sign changes, asymmetric, zero-padded ends, plain): every outcome
# of sign_bounds() at least twice -- see make_golden.py, which prints the census
RANDOM_SEEDS = (2, 3, 8, 13, 17, 18,               # not admitted: asymmetric
                4, 10, 82, 93,                      #   more than 128 effective taps
                12, 15, 32, 41, 45,                 #   an odd number of taps around the centre, or fewer than 12
                5, 7, 28, 29, 33,                   #   bound >= 2
                26, 775, 826,                       #   ... at 48 central taps where 40 alone would pass
                136, 152, 156, 192, 263, 287,       # 12 central taps, FL2
                20646, 26945, 28155,                #   no FL2 scale
                72, 694, 875, 886,                  # 48 central taps, matrix pipe, 40 not admitted
                7265, 27097, 39636,                 #   neither the matrix pipe nor 40
                39, 70, 378, 385, 412, 435)         #   40 admitted, matrix pipe
# the tables whose plans are pinned as well: one of each kind
PLAN_TABLES = ("48k", "192k", "s2", "s4", "s26", "s136", "s20646", "s72", "s7265", "s39")


def trim(taps):
    """What gnuais_batch_create does with a table: (NT, d, te), te = the taps without the exactly-zero ends"""
    t = np.asarray(taps, dtype=np.float32)
    nt = len(t)
    k0, k1 = 0, nt - 1
    while k0 < nt - 1 and t[k0] == 0:
        k0 += 1
    while k1 > k0 and t[k1] == 0:
        k1 -= 1
    return nt, nt - k0, t[k0:k1 + 1].copy()


def len_grid(nt):
    return tuple(dict.fromkeys((1, 33, HEAD_192K, HEAD_192K + 1, nt - 1, 4096, 48000, 192000)))


def plan_grid(nt):
    """(N, len, fir_variant, fir_T, fir_pk_taps, fir_flag2, fir_mfma, dump): every option at both of its values, crossed"""
    return [c for c in itertools.product(N_GRID, len_grid(nt), (3, 0), T_GRID, (0, 48), (1, 0), (1, 0), (0, 1)) if c[1] > 0]


def table_line(name, taps):
    nt, d, te = trim(taps)
    return f"table {name} {nt} {d} {len(te)} " + " ".join(f"{w:08x}" for w in te.view(np.uint32))


def driver_input(tables, with_plans):
    """tables: [(name, taps)]; with_plans: names whose plan grid follows the table"""
    lines = []
    for name, taps in tables:
        lines.append(table_line(name, taps))
        if name in with_plans:
            lines += ["plan " + " ".join(str(v) for v in c) for c in plan_grid(len(taps))]
    return "\n".join(lines) + "\n"


def f32_bits(text):
    """C hex float(s), comma separated -> the float32 bit patterns"""
    return np.array([float.fromhex(v) for v in text.split(",")], dtype=np.float64).astype(np.float32).view(np.uint32)


BOUND_FLOATS = ("eps", "eps_pk", "seen", "ahead", "fscale", "seen_k", "ahead_k", "eps_pk40", "seen40", "ahead40", "seen_k40",
                "ahead_k40", "mfma_seen_u", "mfma_abs_u")
BOUND_INTS = ("ok", "NC", "ok40", "mfma_ok", "k0", "tq")
PLAN_FLOATS = ("eps", "eps_pk", "eps_seen", "eps_ahead", "fscale", "seen_k", "ahead_k", "mfma_seen_u", "mfma_abs_u",
               "sign_exact", "sign_central_taps", "sign_eps", "sign_flag_scale", "sign_eps_seen", "sign_eps_ahead", "sign_matrix_pipe")
PLAN_INTS = ("NC", "T", "head")
KERNELS = ("generic", "scalar32", "sign", "packed", "packed+mfma")


def parse(text):
    """The driver's answer -> (bounds, plans): per table name a dict of arrays (floats as bit patterns), and per table
    name the plan rows in grid order as a dict of stacked arrays"""
    bounds, plans, cur = {}, {}, None
    for line in text.splitlines():
        kind, *kv = line.split()
        d = dict(item.split("=", 1) for item in kv)
        if kind == "bounds":
            cur = d.pop("name")
            b = {k: f32_bits(d[k]) for k in BOUND_FLOATS}
            b.update({k: np.array([int(v) for v in d[k].split(",")], dtype=np.int64) for k in BOUND_INTS})
            b["S"] = np.array([float.fromhex(d["S"])], dtype=np.float64).view(np.uint64)
            bounds[cur] = b
            plans[cur] = []
        else:
            assert kind == "plan", line
            row = {k: f32_bits(d[k]) for k in PLAN_FLOATS}
            row.update({k: np.array([int(d[k])], dtype=np.int64) for k in PLAN_INTS})
            row["kernel"] = np.array([KERNELS.index(d["kernel"])], dtype=np.int64)
            plans[cur].append(row)
    plans = {name: {k: np.stack([r[k] for r in rows]) for k in rows[0]} for name, rows in plans.items() if rows}
    return bounds, plans


def run_driver(text, workdir, sanitize=True):
    """Builds the driver if it is stale -- tests/c/fir_plan.bin with AddressSanitizer + UndefinedBehaviorSanitizer, or
    (sanitize=False, for tests that run beside a GPU) tests/c/fir_plan_plain.bin without --, runs it on `text` (the protocol
    above; the file goes into `workdir`) and returns parse() of its answer"""
    if sanitize:
        exe = EXE
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), "fir_plan"])
    else:
        exe = os.path.join(ROOT, "tests", "c", "fir_plan_plain.bin")
        src = [os.path.join(ROOT, "tests", "c", "fir_plan_main.cpp"), os.path.join(ROOT, "gnuais_amd", "csrc", "fir_plan.cpp")]
        deps = src + [os.path.join(ROOT, "gnuais_amd", "csrc", "fir_plan.h")]
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", *src, "-o", exe, "-lm"])
    path = os.path.join(str(workdir), "in.txt")
    with open(path, "w") as f:
        f.write(text)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    return parse(p.stdout)
