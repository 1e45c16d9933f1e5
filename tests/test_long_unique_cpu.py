"""Each long transmission once, on the CPU: the host object gnuais_long_uniq (frame_unique.cpp over LongRec) against the
restatement tests/long_unique_ref.py over random record sets cut into drains, with the lists and the invariants of the
definition; the unit by itself under ASan + UBSan; the device stage's own text (frame_unique.hip over LongDev) behind
tests/c/hip_cpu under ASan + UBSan with the full and with a truncated hash; on the oracle, the property the tail rule
rests on and that the GPU tests' input really merges; and the header, the exports and the build's resource check."""
import collections
import os
import subprocess

import numpy as np
import pytest

import hip_cpu_build
import long_unique_ref as lur
import unique_ref as ur
from gnuais_amd.lib import HEARER_DTYPE, LONG_FRAME_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuais_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]


@pytest.fixture(scope="module")
def LongUniq():
    so = os.path.join(ROOT, "gnuais_amd", "libgnuais_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-s", "-j8", "-C", CSRC])
    from gnuais_amd.receiver import LongUniq
    return LongUniq


def test_push_equals_the_restatement_with_and_without_the_lists(LongUniq):
    """150 random sets, W from {1, 64, 700}, each cut into random drains that alternate between push and push_heard on
    one state: records, copies, lists and late are the restatement's byte for byte; sum(copies) + late = the records; the
    clusters are those of one push over everything; every member's signal record is zero"""
    flag_pairs, near = set(), collections.Counter()
    for s, (W, drains) in enumerate(lur.random_cases(2025)):
        fr = np.concatenate([d[0] for d in drains])
        top = max(int(fr["t"].max()) + 1 if len(fr) else 1, 1)
        u, r = LongUniq(W), lur.LongUniqueRef(W)
        whole = u.push(fr, top + W + 1)
        want = r.push(fr, top + W + 1)
        assert whole[0].tobytes() == want[0].tobytes() and np.array_equal(whole[1], want[1]) and whole[1].dtype == np.int32, s
        assert u.late() == r.late == 0 and not r.tail and int(whole[1].sum()) == len(fr)
        for c, f in zip(whole[1], whole[0]):
            if c > 1:
                flag_pairs.add(bool(f["flags"] & lur.REPAIRED))
        keys_whole = collections.Counter(ur.key_of(x) for x in whole[0])
        by_payload = collections.Counter(k[1] for k in keys_whole)
        near["nbits"] += sum(1 for v in by_payload.values() if v > 1 and len(fr))
        u.reset()
        r.reset()
        copies, keys = 0, collections.Counter()
        for d, (f, rows) in enumerate(drains):
            if d & 1:
                got, ref = u.push(f, rows), r.push(f, rows)
            else:
                got, ref = u.push_heard(f, rows), r.push_heard(f, rows)
                assert np.array_equal(got[2], ref[2]) and got[2].dtype == np.int32, s
                assert got[3].tobytes() == ref[3].tobytes() and got[3].dtype == HEARER_DTYPE, s
                assert not got[3]["signal"]["power"].any() and not got[3]["signal"]["blocks"].any()
                assert np.array_equal(np.diff(got[2]), got[1])
            assert got[0].tobytes() == ref[0].tobytes() and np.array_equal(got[1], ref[1]), s
            assert u.late() == r.late
            copies += int(got[1].sum())
            keys.update(ur.key_of(x) for x in got[0])
        assert copies + u.late() == len(fr), s
        assert keys == keys_whole, s
        u.close()
    assert flag_pairs == {False, True}          # clusters led by an intact and by a repaired copy both occurred
    assert near["nbits"] > 5                    # keys that differ in nbits alone were told apart


def test_keys_that_differ_in_one_place_only_do_not_merge(LongUniq):
    """nbits alone, the last used payload byte alone, word 37 alone: four transmissions; flags, reserved, channel, end_bit
    and the stamp do not split one"""
    fr = np.zeros(8, dtype=LONG_FRAME_DTYPE)
    fr["nbits"], fr["flags"], fr["t"] = 432, 1, 100
    fr["payload"][:, :54] = np.arange(54, dtype=np.uint8) + 3
    fr["channel"] = np.arange(8)
    fr["nbits"][1] = 440
    fr["payload"][2, 53] ^= 0x80
    fr["payload"][3, 131] = 1
    fr["flags"][5], fr["reserved"][6], fr["end_bit"][7] = 1 | lur.REPAIRED | (9 << 1), 0xEE, 77
    f, c = LongUniq(10).push(fr, 10 ** 6)
    assert c.tolist() == [5, 1, 1, 1] and f["channel"].tolist() == [0, 1, 2, 3]


def test_primary_window_untimed_capacity_and_reset(LongUniq):
    from gnuais_amd.lib import E_ARG, GnuaisError
    fr = np.zeros(4, dtype=LONG_FRAME_DTYPE)
    fr["nbits"], fr["payload"][:, 0], fr["channel"] = 800, 9, [3, 2, 1, 0]
    fr["flags"] = [1 | lur.REPAIRED, 1, 1, 1 | lur.REPAIRED]
    fr["t"] = [100, 110, 110 + 50, 110 + 50 + 51]
    f, c = LongUniq(50).push(fr, 10 ** 6)       # the window is inclusive; the earliest intact copy leads
    assert c.tolist() == [3, 1] and f["t"].tolist() == [110, 211] and f["channel"].tolist() == [2, 0]
    fr["flags"] = 1 | lur.REPAIRED              # every copy repaired: the earliest one
    f, c = LongUniq(50).push(fr, 10 ** 6)
    assert f["t"].tolist() == [100, 211] and f["channel"].tolist() == [3, 0]
    fr["t"][:2] = -1                            # untimed: each by itself, first, by (channel, stamp)
    f, c, first, mem = LongUniq(50).push_heard(fr, 10 ** 6)
    assert c.tolist() == [1, 1, 1, 1] and f["channel"].tolist() == [2, 3, 1, 0] and mem["t"].tolist() == [-1, -1, 160, 211]
    u = LongUniq(100)
    f, c = u.push(np.zeros(0, dtype=LONG_FRAME_DTYPE), 0)
    assert len(f) == len(c) == 0
    fr = np.zeros(3, dtype=LONG_FRAME_DTYPE)
    fr["nbits"], fr["payload"][:, 0], fr["flags"], fr["channel"], fr["t"] = 480, [1, 2, 2], 1, [0, 0, 1], [950, 960, 965]
    with pytest.raises(GnuaisError) as e:
        u.push(fr, 1000, cap=1)                 # two clusters do not fit one entry ...
    assert e.value.code == E_ARG
    f, c = u.push(fr, 1000, cap=2)              # ... and nothing was consumed
    assert c.tolist() == [1, 2] and u.late() == 0
    fr2 = fr[1:2].copy()
    fr2["channel"], fr2["t"] = 5, 1010
    assert len(u.push(fr2, 1100)[0]) == 0 and u.late() == 1     # chains onto the open cluster: late
    fr2["t"] = 1111                             # 1111 - 1010 > 100: it no longer chains onto the tail, a transmission again
    f, c = u.push(fr2, 1200)
    assert c.tolist() == [1] and u.late() == 1
    u.reset()
    assert u.late() == 0
    with pytest.raises(GnuaisError):
        LongUniq(0)


SAN_MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gnuais_hip.h"
/* in: int32 W, int32 drains, then per drain int32 n, int64 rows, n records.  out: per drain int32 rc, int32 n_out, int32
 * members (-1: no lists), int64 late, the records, the copies, with lists n_out + 1 offsets and the members -- every buffer
 * allocated at its exact size */
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t head[2];
    while (fread(head, sizeof head, 1, f) == 1) {
        gnuais_long_uniq *u = NULL;
        if (gnuais_long_uniq_create(&u, head[0]) != GNUAIS_OK) return 4;
        for (int d = 0; d < head[1]; ++d) {
            int32_t n;
            int64_t rows;
            if (fread(&n, sizeof n, 1, f) != 1 || fread(&rows, sizeof rows, 1, f) != 1) return 5;
            const size_t N = (size_t) (n ? n : 1);
            gnuais_long_frame *fr = malloc(sizeof *fr * N), *out = malloc(sizeof *out * N);
            int32_t *oc = malloc(4 * N), *first = malloc(4 * ((size_t) n + 1));
            gnuais_hearer *mem = malloc(sizeof *mem * N);
            if (n && fread(fr, sizeof *fr, (size_t) n, f) != (size_t) n) return 6;
            int got = -1, nm = -1;
            const int32_t rc = (d & 1) ? gnuais_long_uniq_push(u, fr, n, rows, out, oc, n, &got)
                                       : gnuais_long_uniq_push_heard(u, fr, n, rows, out, oc, n, &got, first, mem, &nm);
            const int32_t r3[3] = {rc, got, nm};
            const int64_t late = gnuais_long_uniq_late(u);
            fwrite(r3, sizeof r3, 1, g);
            fwrite(&late, sizeof late, 1, g);
            fwrite(out, sizeof *out, (size_t) got, g);
            fwrite(oc, 4, (size_t) got, g);
            if (nm >= 0) {
                fwrite(first, 4, (size_t) got + 1, g);
                fwrite(mem, sizeof *mem, (size_t) nm, g);
            }
            free(fr); free(out); free(oc); free(first); free(mem);
        }
        if (gnuais_long_uniq_reset(u) != GNUAIS_OK || gnuais_long_uniq_late(u) != 0) return 8;
        gnuais_long_uniq_destroy(u);
    }
    int got = 0;
    if (gnuais_long_uniq_push(NULL, NULL, 0, 0, NULL, NULL, 0, &got) != GNUAIS_E_ARG) return 9;
    gnuais_long_uniq_destroy(NULL);
    fclose(f);
    fclose(g);
    return 0;
}
'''


def check_output(out, cases, first_word_is_rc):
    """the stand-alone programs' output against the restatement; -> the sum of the first word where it counts exact runs"""
    pos = total = 0
    for W, drains in cases:
        ref = lur.LongUniqueRef(W)
        for d, (fr, rows) in enumerate(drains):
            w0, got, nm = (int(v) for v in np.frombuffer(out, dtype=np.int32, count=3, offset=pos))
            late = int(np.frombuffer(out, dtype=np.int64, count=1, offset=pos + 12)[0])
            pos += 20
            if first_word_is_rc:
                assert w0 == 0
            else:
                total += w0
            heard = (d & 1) == 0
            want = ref.push_heard(fr, rows) if heard else ref.push(fr, rows)
            assert got == len(want[0]) and late == ref.late
            assert out[pos:pos + 152 * got] == want[0].tobytes()
            assert out[pos + 152 * got:pos + 156 * got] == want[1].tobytes()
            pos += 156 * got
            if heard:
                assert nm == len(want[3])
                assert out[pos:pos + 4 * (got + 1)] == want[2].tobytes()
                assert out[pos + 4 * (got + 1):pos + 4 * (got + 1) + 24 * nm] == want[3].tobytes()
                pos += 4 * (got + 1) + 24 * nm
            else:
                assert nm == -1
    assert pos == len(out)
    return total


def test_host_unit_standalone_under_asan_and_ubsan(tmp_path):
    """frame_unique.cpp has no HIP dependency: g++ builds it by itself with -fsanitize=address,undefined; a small C main
    drives the long object over random sets cut into drains, and what it writes is the restatement's"""
    exe = str(tmp_path / "long_uniq.bin")
    (tmp_path / "main.c").write_text(SAN_MAIN)
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", *SAN, "-I", os.path.join(ROOT, "include"), "-c",
                           str(tmp_path / "main.c"), "-o", str(tmp_path / "main.o")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-c", os.path.join(CSRC, "frame_unique.cpp"),
                           "-o", str(tmp_path / "frame_unique.o")])
    subprocess.check_call(["g++", *SAN, str(tmp_path / "main.o"), str(tmp_path / "frame_unique.o"), "-o", exe])
    cases = lur.random_cases(77)
    src, dst = str(tmp_path / "sets.in"), str(tmp_path / "sets.out")
    lur.write_cases(src, cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    check_output(open(dst, "rb").read(), cases, True)


@pytest.fixture(scope="module")
def kernel_exe(tmp_path_factory):
    return hip_cpu_build.build("long_unique_kernel_main.cpp", tmp_path_factory.mktemp("luq") / "long_unique_kernel.bin",
                               "-DHIP_CPU_SERIAL")


@pytest.mark.parametrize("hash_bits", [64, 3, 1])
def test_the_kernels_own_text_on_the_cpu_equals_the_restatement(tmp_path, kernel_exe, hash_bits):
    """frame_unique.hip compiled for the CPU behind tests/c/hip_cpu's serial mode under ASan + UBSan, driven as the drain
    drives it with buffers of exactly the sizes the interface asks for, drains with and without the lists alternating: the
    records, copies, lists and the late count are the restatement's -- with the full hash without ever taking the exact
    path, with 3 and 1 bits through it in more than 100 drains"""
    cases = lur.random_cases(78)
    src, dst = str(tmp_path / "sets.in"), str(tmp_path / "sets.out")
    lur.write_cases(src, cases)
    r = subprocess.run([kernel_exe, src, dst, str(hash_bits)], capture_output=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    exact = check_output(open(dst, "rb").read(), cases, False)
    assert exact == 0 if hash_bits == 64 else exact > 100


@pytest.fixture(scope="module")
def seven():
    """the GPU tests' seven receivers on the oracle, call by call over the ragged cuts: [(records, rows before, after)]"""
    x = lur.seven_receivers()
    ref = lur.SampleRef(7)
    cuts = lur.ragged_cuts7()
    calls = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        ref.run(x[a:e])
        calls.append((ref.drain(), int(a), int(e)))
    return calls


def test_every_t_of_a_call_lies_inside_the_rows_of_that_call(seven):
    """THE PROPERTY RELIED ON (include/gnuais_hip.h): D' computes t at its closing bit, a row of the call that closed the
    frame, so every record of a later drain has t >= the rows at this one"""
    n = 0
    for fr, a, e in seven:
        assert np.all((fr["t"] >= a) & (fr["t"] < e)), (a, e, fr["t"])
        n += len(fr)
    assert n == sum(lur.COUNTS7)


def test_the_seven_receivers_merge_into_five_clusters(seven):
    """the input is good: 5, 5, 4, 5, 5, 5, 5 long frames (receiver 2 loses the 432-bit one, at sigma = 1000 too); with
    W = 128 the restatement finds 5 clusters of 6, 7, 7, 7, 7 copies -- the GPU tests cannot pass on an input where nothing
    merges"""
    fr = np.concatenate([c[0] for c in seven])
    assert np.bincount(fr["channel"], minlength=7).tolist() == lur.COUNTS7
    assert 432 not in fr["nbits"][fr["channel"] == 2]
    f, c = lur.LongUniqueRef(128).push(fr, lur.TOTAL7)
    assert sorted(c.tolist()) == [6, 7, 7, 7, 7] and int(f["nbits"][np.argmin(c)]) == 432
    r = lur.LongUniqueRef(128)                  # call by call: the same five, the copies behind a cut counted late
    got = [r.push(c[0], c[2]) for c in seven]
    assert sum(len(g[0]) for g in got) == 5 and sum(int(g[1].sum()) for g in got) + r.late == 34


def test_receiver_two_loses_its_frame_at_the_larger_sigma_too():
    x = lur.seven_receivers(sigma=1000.0)[:, 2:3]
    ref = lur.SampleRef(1)
    ref.run(np.ascontiguousarray(x))
    assert 432 not in ref.drain()["nbits"]


def test_symbols_declared_exported_bound_and_the_kernels_are_in_the_builds_resource_check():
    from gnuais_amd import lib
    header = open(os.path.join(ROOT, "include", "gnuais_hip.h")).read()
    names = ["gnuais_batch_long_unique", "gnuais_batch_drain_long_frames_unique", "gnuais_batch_drain_long_frames_heard",
             "gnuais_batch_long_unique_late", "gnuais_long_uniq_create", "gnuais_long_uniq_destroy", "gnuais_long_uniq_reset",
             "gnuais_long_uniq_push", "gnuais_long_uniq_push_heard", "gnuais_long_uniq_late", "gnuais_node_long_unique",
             "gnuais_node_drain_long_frames_unique", "gnuais_node_drain_long_frames_heard", "gnuais_node_long_unique_late"]
    for name in names:
        assert name in lib.SYMBOLS and name + "(" in header and hasattr(lib.load(), name), name
    assert "no duplicate merge" not in header and '"long_unique"' in header and '"long_unique_late"' in header
    mk = open(os.path.join(CSRC, "Makefile")).read()
    # every kernel of the long stage: an instance of frame_unique.hip's templates, counted with the short kind's (=2); the
    # tail kernel is the long kind's alone, slot2q is no template (=1)
    kernels = {"uniq_keys_kernel": 2, "uniq_digit_kernel": 2, "uniq_boundary_kernel": 2, "uniq_members_kernel": 2,
               "uniq_clusters_kernel": 2, "uniq_tail_kernel": 1, "uniq_gather_kernel": 2, "uniq_slot2q_kernel": 1,
               "uniq_heard_kernel": 2}
    assert "$(CHECK_RES) $(BUILD)/frame_unique.s " + " ".join(f"{k}={n}" for k, n in kernels.items()) + "\n" in mk
    assert "$(BUILD)/frame_unique.o" in mk
    text = open(os.path.join(CSRC, "frame_unique.hip")).read()
    for k in kernels:
        assert f"void {k}(" in text
    assert "cluster_enqueue<LongDev>" in text and "deliver_enqueue<LongDev>" in text
    assert "__shared__" not in text and "asm" not in text
    dev = open(os.path.join(CSRC, "frame_unique_dev.h")).read()
    assert "__shared__" not in dev and "asm" not in dev
    from gnuais_amd import receiver
    for m in ("long_unique", "drain_long_frames_unique", "drain_long_frames_heard", "long_unique_late"):
        assert hasattr(receiver.ReceiverBatch, m)
    assert hasattr(receiver, "LongUniq")
