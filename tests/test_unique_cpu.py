"""One record per transmission on the CPU: the host object gnuais_uniq (frame_unique.cpp) against the plain restatement
tests/unique_ref.py over random record sets, whole and cut into drains, with the two invariants of the definition; its
edges; the unit by itself under ASan + UBSan; and, on the oracle, the property the tail rule rests on and that the GPU
test's input really merges."""
import collections
import os
import subprocess

import numpy as np
import pytest

import frame_time_ref as ftr
import hip_cpu_build
import unique_ref as ur
from oracle_lib import FRAME_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuais_amd", "csrc")


@pytest.fixture(scope="module")
def Uniq():
    so = os.path.join(ROOT, "gnuais_amd", "libgnuais_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-s", "-j8", "-C", CSRC])
    from gnuais_amd.receiver import Uniq
    return Uniq


def random_set(rng, W):
    """frames, times: keys from a pool of 1..50 (nbits 168 or 424), transmissions whose copies lie on different channels
    -- equal t among them, gaps of exactly W and W + 1 -- both values of flags bit 6, some t = -1; shuffled"""
    pool = []
    for _ in range(int(rng.integers(1, 51))):
        nbits = int(rng.choice([168, 424]))
        p = np.zeros(53, dtype=np.uint8)
        p[: nbits // 8] = rng.integers(0, 256, nbits // 8, dtype=np.uint8)
        pool.append((nbits, p))
    n_ch = int(rng.integers(1, 40))
    rec, seen = [], set()
    for _ in range(int(rng.integers(1, 30))):
        k = int(rng.integers(0, len(pool)))
        t = int(rng.integers(0, 6000))
        for _ in range(int(rng.integers(1, 9))):        # a chain: the next copy 0, a few, exactly W, or W + 1 rows on
            step = int(rng.choice([0, 0, int(rng.integers(1, W + 1)), W, W + 1]))
            t += step
            ch = int(rng.integers(0, n_ch))
            untimed = rng.random() < 0.08
            if not untimed and (ch, t) in seen:         # one channel never closes two frames on one row
                continue
            seen.add((ch, t))
            rec.append((k, ch, -1 if untimed else t, int(rng.integers(0, 2))))
    order = rng.permutation(len(rec))
    fr = np.zeros(len(rec), dtype=FRAME_DTYPE)
    tm = np.zeros(len(rec), dtype=np.int64)
    for j, i in enumerate(order):
        k, ch, t, rep = rec[i]
        fr[j]["channel"], fr[j]["end_bit"] = ch, 1000 + 7 * int(i)          # the stamp: unique, unrelated to t
        fr[j]["payload"], fr[j]["nbits"] = pool[k][1], pool[k][0]
        fr[j]["flags"] = 1 | (ur.REPAIRED if rep else 0) | (int(rng.integers(0, 32)) << 1)
        tm[j] = t
    return fr, tm


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) \
        and a[2].dtype == np.int32 and a[1].dtype == np.int64


def cut_into_drains(rng, fr, tm):
    """[(frames, times, rows)]: 1..5 drains at random rows; drain d holds the frames with rows[d-1] <= t < rows[d], the
    untimed ones anywhere"""
    top = int(tm.max()) + 1 if len(tm) else 1
    n = int(rng.integers(1, 6))
    rows = sorted(int(r) for r in rng.integers(0, top + 1, n - 1)) + [top + int(rng.integers(0, 3000))]
    which = np.searchsorted(np.array(rows), tm, side="right")
    which[tm < 0] = rng.integers(0, n, int(np.count_nonzero(tm < 0)))
    return [(fr[which == d], tm[which == d], rows[d]) for d in range(n)]


def test_push_equals_the_restatement_whole_and_cut_into_drains(Uniq):
    rng = np.random.default_rng(2024)
    flag_pairs = set()
    n_sets = 2000
    for s in range(n_sets):
        W = int(rng.choice([1, 5, 64, 128, 700]))
        fr, tm = random_set(rng, W)
        top = (int(tm.max()) + 1) if len(tm) else 1
        u, r = Uniq(W), ur.UniqueRef(W)
        whole = u.push(fr, tm, top + W + 1)
        assert same(whole, r.push(fr, tm, top + W + 1)), s
        assert u.late() == r.late == 0 and not r.tail
        assert int(whole[2].sum()) == len(fr)
        for c, f in zip(whole[2], whole[0]):
            if c > 1:
                flag_pairs.add(bool(f["flags"] & ur.REPAIRED))
        # the same records cut into drains: the C object equals the restatement drain by drain, and for any cuts
        # sum(copies) + late = the frames, and the clusters are those of the single drain
        u.reset()
        r.reset()
        copies, keys = 0, collections.Counter()
        for f, t, rows in cut_into_drains(rng, fr, tm):
            got = u.push(f, t, rows)
            assert same(got, r.push(f, t, rows)), s
            copies += int(got[2].sum())
            keys.update(ur.key_of(x) for x in got[0])
        assert u.late() == r.late
        assert copies + u.late() == len(fr), s
        assert keys == collections.Counter(ur.key_of(x) for x in whole[0]), s
        u.close()
    assert flag_pairs == {False, True}          # clusters led by an intact and by a repaired copy both occurred


def test_primary_is_the_earliest_intact_copy_and_the_window_is_inclusive(Uniq):
    fr = np.zeros(4, dtype=FRAME_DTYPE)
    fr["nbits"], fr["payload"][:, 0], fr["channel"] = 168, 9, [3, 2, 1, 0]
    fr["flags"] = [1 | ur.REPAIRED, 1, 1, 1 | ur.REPAIRED]
    tm = np.array([100, 110, 110 + 50, 110 + 50 + 51], dtype=np.int64)
    f, t, c = Uniq(50).push(fr, tm, 10 ** 6)
    assert c.tolist() == [3, 1] and t.tolist() == [110, 211] and f["channel"].tolist() == [2, 0]
    assert f["flags"].tolist() == [1, 1 | ur.REPAIRED]
    fr["flags"] = 1 | ur.REPAIRED               # every copy repaired: the earliest one
    f, t, c = Uniq(50).push(fr, tm, 10 ** 6)
    assert t.tolist() == [100, 211] and f["channel"].tolist() == [3, 0]


def test_empty_capacity_and_reset(Uniq):
    u = Uniq(100)
    f, t, c = u.push(np.zeros(0, dtype=FRAME_DTYPE), np.zeros(0, dtype=np.int64), 0)
    assert len(f) == len(t) == len(c) == 0
    fr = np.zeros(3, dtype=FRAME_DTYPE)
    fr["nbits"], fr["payload"][:, 0], fr["flags"] = 168, [1, 2, 2], 1
    fr["channel"] = [0, 0, 1]
    tm = np.array([950, 960, 965], dtype=np.int64)
    from gnuais_amd.lib import E_ARG, GnuaisError
    with pytest.raises(GnuaisError) as e:
        u.push(fr, tm, 1000, cap=1)             # two clusters do not fit one entry ...
    assert e.value.code == E_ARG
    f, t, c = u.push(fr, tm, 1000, cap=2)       # ... and nothing was consumed: the same push still delivers both
    assert c.tolist() == [1, 2] and u.late() == 0
    fr2 = fr[1:2].copy()
    fr2["channel"] = 5
    f, t, c = u.push(fr2, np.array([1010], dtype=np.int64), 1100)   # chains onto the open cluster: late
    assert len(f) == 0 and u.late() == 1
    u.reset()                                   # the tail and the count are gone: the same frame is a transmission again
    assert u.late() == 0
    f, t, c = u.push(fr2, np.array([1010], dtype=np.int64), 1100)
    assert c.tolist() == [1] and u.late() == 0
    with pytest.raises(GnuaisError):
        Uniq(0)


SAN_MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gnuais_hip.h"
/* in: int32 W, int32 drains, then per drain int32 n, int64 rows, n records, n times.  out: per drain int32 rc, int32
 * n_out, int64 late, the records, times and copies -- every buffer allocated at its exact size */
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t head[2];
    while (fread(head, sizeof head, 1, f) == 1) {
        gnuais_uniq *u = NULL;
        if (gnuais_uniq_create(&u, head[0]) != GNUAIS_OK) return 4;
        for (int d = 0; d < head[1]; ++d) {
            int32_t n;
            int64_t rows;
            if (fread(&n, sizeof n, 1, f) != 1 || fread(&rows, sizeof rows, 1, f) != 1) return 5;
            gnuais_frame *fr = malloc(sizeof *fr * (size_t) (n ? n : 1)), *out = malloc(sizeof *out * (size_t) (n ? n : 1));
            int64_t *tm = malloc(8 * (size_t) (n ? n : 1)), *ot = malloc(8 * (size_t) (n ? n : 1));
            int32_t *oc = malloc(4 * (size_t) (n ? n : 1));
            if (n && (fread(fr, sizeof *fr, (size_t) n, f) != (size_t) n || fread(tm, 8, (size_t) n, f) != (size_t) n)) return 6;
            int got = -1;
            const int32_t rc = gnuais_uniq_push(u, fr, tm, n, rows, out, ot, oc, n, &got);
            const int32_t r2[2] = {rc, got};
            const int64_t late = gnuais_uniq_late(u);
            fwrite(r2, sizeof r2, 1, g);
            fwrite(&late, sizeof late, 1, g);
            fwrite(out, sizeof *out, (size_t) got, g);
            fwrite(ot, 8, (size_t) got, g);
            fwrite(oc, 4, (size_t) got, g);
            free(fr); free(out); free(tm); free(ot); free(oc);
        }
        if (gnuais_uniq_reset(u) != GNUAIS_OK || gnuais_uniq_late(u) != 0) return 8;
        gnuais_uniq_destroy(u);
    }
    int got = 0;
    if (gnuais_uniq_push(NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, 0, &got) != GNUAIS_E_ARG) return 9;
    gnuais_uniq_destroy(NULL);
    fclose(f);
    fclose(g);
    return 0;
}
'''


def test_host_unit_standalone_under_asan_and_ubsan(tmp_path):
    """frame_unique.cpp has no HIP dependency: g++ builds it by itself with -fsanitize=address,undefined; a small C main
    drives it over random sets cut into drains, and what it writes is the restatement's"""
    exe = str(tmp_path / "uniq.bin")
    (tmp_path / "main.c").write_text(SAN_MAIN)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"), "-c",
                           str(tmp_path / "main.c"), "-o", str(tmp_path / "main.o")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *san, "-c", os.path.join(CSRC, "frame_unique.cpp"),
                           "-o", str(tmp_path / "frame_unique.o")])
    subprocess.check_call(["g++", *san, str(tmp_path / "main.o"), str(tmp_path / "frame_unique.o"), "-o", exe])
    rng = np.random.default_rng(77)
    cases = []
    for _ in range(150):
        W = int(rng.choice([1, 64, 700]))
        fr, tm = random_set(rng, W)
        cases.append((W, cut_into_drains(rng, fr, tm)))
    cases.append((9, [(np.zeros(0, dtype=FRAME_DTYPE), np.zeros(0, dtype=np.int64), 0)]))
    src, dst = str(tmp_path / "sets.in"), str(tmp_path / "sets.out")
    write_cases(src, cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    out = open(dst, "rb").read()
    pos = 0
    for W, drains in cases:
        ref = ur.UniqueRef(W)
        for fr, tm, rows in drains:
            rc, got = np.frombuffer(out, dtype=np.int32, count=2, offset=pos)
            late = int(np.frombuffer(out, dtype=np.int64, count=1, offset=pos + 8)[0])
            pos += 16
            wf, wt, wc = ref.push(fr, tm, rows)
            assert rc == 0 and got == len(wf) and late == ref.late
            assert out[pos:pos + 64 * got] == wf.tobytes()
            assert out[pos + 64 * got:pos + 72 * got] == wt.tobytes()
            assert out[pos + 72 * got:pos + 76 * got] == wc.tobytes()
            pos += 76 * got
    assert pos == len(out)


def write_cases(path, cases):
    with open(path, "wb") as f:
        for W, drains in cases:
            f.write(np.array([W, len(drains)], dtype=np.int32).tobytes())
            for fr, tm, rows in drains:
                f.write(np.int32(len(fr)).tobytes() + np.int64(rows).tobytes() + fr.tobytes() + tm.tobytes())


@pytest.mark.parametrize("hash_bits", [64, 3, 1])
def test_the_kernels_own_text_on_the_cpu_equals_the_restatement(tmp_path, hash_bits):
    """frame_unique.hip compiled for the CPU behind tests/c/hip_cpu's serial mode (its kernels have no barrier: a launch is
    a loop over lanes; rocPRIM's sort and scan are stood in for by stable CPU ones) under ASan + UBSan, driven as the
    drain drives it with buffers of exactly the sizes the interface asks for: over random sets cut into drains the
    records, times, copies and the late count are the restatement's -- with the full hash without ever taking the exact
    path, with 3 and 1 bits through it.  The kernels' control flow and bounds cannot be checked on a device by the CPU
    suite; this is that check."""
    exe = hip_cpu_build.build("unique_kernel_main.cpp", tmp_path / "unique_kernel.bin", "-DHIP_CPU_SERIAL")
    rng = np.random.default_rng(78)
    cases = []
    for _ in range(150):
        W = int(rng.choice([1, 64, 700]))
        fr, tm = random_set(rng, W)
        cases.append((W, cut_into_drains(rng, fr, tm)))
    cases.append((9, [(np.zeros(0, dtype=FRAME_DTYPE), np.zeros(0, dtype=np.int64), 0)]))
    src, dst = str(tmp_path / "sets.in"), str(tmp_path / "sets.out")
    write_cases(src, cases)
    r = subprocess.run([exe, src, dst, str(hash_bits)], capture_output=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    out = open(dst, "rb").read()
    pos = exact = 0
    for W, drains in cases:
        ref = ur.UniqueRef(W)
        for fr, tm, rows in drains:
            runs, got = np.frombuffer(out, dtype=np.int32, count=2, offset=pos)
            late = int(np.frombuffer(out, dtype=np.int64, count=1, offset=pos + 8)[0])
            pos += 16
            exact += int(runs)
            wf, wt, wc = ref.push(fr, tm, rows)
            assert got == len(wf) and late == ref.late
            assert out[pos:pos + 64 * got] == wf.tobytes()
            assert out[pos + 64 * got:pos + 72 * got] == wt.tobytes()
            assert out[pos + 72 * got:pos + 76 * got] == wc.tobytes()
            pos += 76 * got
    assert pos == len(out)
    assert exact == 0 if hash_bits == 64 else exact > 100


@pytest.fixture(scope="module")
def six_receivers():
    """the GPU test's six receivers on the oracle, call by call: [(frames, times, rows before, rows after)]"""
    x = ur.receivers(1, ur.DELAYS6)
    ref = ftr.FrameTimeRef(x.shape[1])
    cuts = ur.ragged_cuts()
    drains = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        ref.run(x[a:e])
        fr, t = ref.drain()
        drains.append((fr, t, int(a), int(e)))
    return drains


def test_every_time_of_a_drain_lies_inside_the_rows_of_its_call(six_receivers):
    """THE PROPERTY RELIED ON (include/gnuais_hip.h): a frame's time is a row of the call that closed it, so every frame
    of a later drain has t >= the rows at this one"""
    n = 0
    for fr, t, a, e in six_receivers:
        assert np.all((t >= a) & (t < e)), (a, e, t)
        n += len(fr)
    assert n == 8 * 6


def test_the_receivers_input_merges_into_clusters_of_six(six_receivers):
    """the input is good: with W = 128 the restatement finds exactly 8 clusters of 6 copies, every copy within +-4 rows
    of the first copy + its delay -- so the GPU tests cannot pass on an input where nothing merges"""
    fr = np.concatenate([d[0] for d in six_receivers])
    t = np.concatenate([d[1] for d in six_receivers])
    f, tt, c = ur.UniqueRef(128).push(fr, t, ur.TOTAL)
    assert c.tolist() == [6] * 8
    for rec, t0 in zip(f, tt):
        mine = [(int(x["channel"]), int(y)) for x, y in zip(fr, t) if ur.key_of(x) == ur.key_of(rec)]
        assert sorted(ch for ch, _ in mine) == list(range(6))
        first = dict(mine)[0]
        assert all(abs(y - first - ur.DELAYS6[ch]) <= 4 for ch, y in mine), mine
    # drained call by call: the same 8 transmissions, the copies behind a cut counted late
    r = ur.UniqueRef(128)
    got = [r.push(d[0], d[1], d[3]) for d in six_receivers]
    assert sum(len(g[0]) for g in got) == 8 and sum(int(g[2].sum()) for g in got) + r.late == 48
