"""A CPU model of the certification rule of the three long-table slicer kernels, and the adversarial inputs built with it
(TEST INFRASTRUCTURE shared by tests/test_slicer_cert_cpu.py and tests/test_slicer_cert_gpu.py).

K1s keeps the sign of its central sum y_c where |y_c| reaches a threshold and re-evaluates the reference's ordered sum
elsewhere.  What can go wrong silently is the threshold's data-dependent part: which rows the running maximum M covers,
which class an output falls in, how |x| is read.  The model restates those rules from the kernels' own comments
(gnuais_amd/csrc/fir_sign_pk.hip, fir_sign_mfma.hip) with the rule as a PARAMETER, so that a test can ask "would this
input notice if the kernel's M missed that row?" without a GPU.  The thresholds are the driver's (tests/c/fir_plan_main.cpp
behind fir_plan_cases.run_driver).  The model never decides an expected value: that is always the oracle's filter > 0.

Geometry (192 kHz table: NT 144, d 135, NE 126): y[n] = sum_j te[j] x[n - d + j]; the NC central taps are j = J0 .. J0+NC-1,
J0 = (NE - NC) / 2; "behind" are the omitted taps j < J0 (older rows), "ahead" the omitted taps j >= J0 + NC."""
from dataclasses import dataclass, replace

import numpy as np

import fir_plan_cases as fc

SLOT = 512                      # rows between two patterns of a channel: more than any running maximum reaches (checked by the CPU test)
D_CUTS = (1, 16, 39, 48, 87, 143)
FIR_T = 3840                    # whole quanta of all three kernels (640, 384, 128): segment seams of the tests' inputs


# ---------------------------------------------------------------------------------------------- the forms

@dataclass(frozen=True)
class Form:
    name: str                   # packed40, packed48, mfma
    nc: int                     # central taps of the kernel that certifies (mfma: 48)
    head_nc: int                # mfma: central taps of the packed kernel that keeps a call's head
    nt: int
    d: int
    te: np.ndarray              # float32[NE]
    seen_k: tuple = ()          # packed: float32 x 4
    ahead_k: tuple = ()
    tq: tuple = ()              # mfma: the 48 integer taps
    S: float = 0.0
    seen_u: float = 0.0
    abs_u: float = 0.0
    options: tuple = ()         # batch options that select the form

    @property
    def ne(self): return len(self.te)
    @property
    def j0(self): return (self.ne - self.nc) // 2
    @property
    def dc(self): return self.d - self.j0
    @property
    def period(self): return 128 if self.name == "mfma" else unroll(self.nc)
    @property
    def matrix(self): return self.name == "mfma"


def unroll(nc):
    """fir_sign_pk.hip: whole turns of the accumulator ring and whole 16-row groups"""
    return 48 if 48 % nc == 0 else nc * 16 // np.gcd(nc, 16)


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def load_forms(taps, workdir, name="t", sanitize=True):
    """The three forms for one table, thresholds from the driver"""
    bounds, _ = fc.run_driver(fc.table_line(name, taps) + "\n", workdir, sanitize)
    b = bounds[name]
    assert b["ok"][0] == 1 and b["NC"][0] == 48 and b["ok40"][0] == 1 and b["mfma_ok"][0] == 1
    nt, d, te = fc.trim(taps)
    S = float(b["S"].view(np.float64)[0])
    common = dict(nt=nt, d=d, te=te)
    return {
        "packed40": Form("packed40", 40, 40, seen_k=tuple(f32(b["seen_k40"])), ahead_k=tuple(f32(b["ahead_k40"])), **common),
        "packed48": Form("packed48", 48, 48, seen_k=tuple(f32(b["seen_k"])), ahead_k=tuple(f32(b["ahead_k"])),
                         options=(("fir_pk_taps", 48),), **common),
        "mfma": Form("mfma", 48, 40, seen_k=tuple(f32(b["seen_k40"])), ahead_k=tuple(f32(b["ahead_k40"])),
                     tq=tuple(int(v) for v in b["tq"]), S=S, seen_u=float(f32(b["mfma_seen_u"])[0]),
                     abs_u=float(f32(b["mfma_abs_u"])[0]), **common),
    }


def plans(taps, workdir, n_ch, lengths, fir_T, pk_taps=0, name="t", sanitize=True):
    """{len: (kernel name, T, head)} from plan_fir() for the call lengths of a chunking"""
    lengths = sorted(set(int(v) for v in lengths))
    text = fc.table_line(name, taps) + "\n" + "".join(f"plan {n_ch} {n} 3 {fir_T} {pk_taps} 1 1 0\n" for n in lengths)
    _, p = fc.run_driver(text, workdir, sanitize)
    p = p[name]
    return {n: (fc.KERNELS[int(p["kernel"][i, 0])], int(p["T"][i, 0]), int(p["head"][i, 0])) for i, n in enumerate(lengths)}


# ---------------------------------------------------------------------------------------------- the rules

@dataclass(frozen=True)
class PackedRule:
    """fir_sign_pk.hip, INLOOP: eps = seen_k[class] * M / 32768 + ahead_k[class]"""
    nhist: int = 3              # "three maxima: this loop turn's groups so far, the turn before, the turn before that"
    group_rows: int = 16        # "the rows behind AND the rest of the output's own 16-row group": rows of the group under M
    warm_from_j0: bool = True   # the warm-up maximum spans m0 - J0 .. m0 + NC - 2
    warm_history: bool = True   # ... through the history rows (rows before the call)
    primed: bool = True         # hmax[] starts from the warm-up maximum (else 0 in each segment)
    class_shift: int = 0        # classes by pair step: >= 6, 4, 2, 0 rows of the group still to come (steps 0-4, 5, 6, 7)
    thr_scale: float = 1.0
    abs_min: int = 32768        # |-32768|
    silence_behind: int = 0     # rows the silence shortcut looks at less than J0 + NC - 1 behind / J0 past a word
    silence_ahead: int = 0


@dataclass(frozen=True)
class MatrixRule:
    """fir_sign_mfma.hip: |y'| against ceil(seen_u * M + abs_u), M over blocks k .. k+5 of the step"""
    row_lo: int = -64           # first row under M relative to the step's first WINDOW row (block k = 64 rows before it)
    row_hi: int = 127           # last row under M (block k + 5 ends 128 rows after it)
    primed: bool = True         # blocks 0 .. 4 of a segment are primed in the prologue (else M starts at 0 in each segment)
    thr_scale: float = 1.0
    abs_min: int = 32768        # the packed unsigned 16-bit |x|: -32768 -> 0x8000


def mutants(form):
    """name -> rule: the ways the rule could be wrong without a crash"""
    if form.matrix:
        s = MatrixRule()
        # a step of 32 outputs needs rows -39 (= dc - d) .. +117 (= 31 + NE - 1 - d + dc) relative to its first window row
        lo, hi = form.dc - form.d, 31 + form.ne - 1 - form.d + form.dc
        return {"newest row ahead missed": replace(s, row_hi=hi - 1), "newest 2 rows ahead missed": replace(s, row_hi=hi - 2),
                "oldest rows behind missed": replace(s, row_lo=lo + 1),
                "one block fewer, oldest": replace(s, row_lo=s.row_lo + 32), "one block fewer, newest": replace(s, row_hi=s.row_hi - 32),
                "threshold x 0.8": replace(s, thr_scale=0.8), "|-32768| read as 0": replace(s, abs_min=0),
                "segment not primed": replace(s, primed=False)}
    s = PackedRule()
    return {"newest row ahead missed": replace(s, group_rows=15), "newest 2 rows ahead missed": replace(s, group_rows=14),
            "oldest rows behind missed": replace(s, warm_from_j0=False),
            "one history turn fewer": replace(s, nhist=2),
            "class one earlier": replace(s, class_shift=-1), "class one later": replace(s, class_shift=1),
            "threshold x 0.8": replace(s, thr_scale=0.8), "|-32768| read as 0": replace(s, abs_min=0),
            "warm-up skips the history": replace(s, warm_history=False), "segment not primed": replace(s, primed=False),
            "silence shortcut one row short behind": replace(s, silence_behind=1),
            "silence shortcut one row short ahead": replace(s, silence_ahead=1)}


# ---------------------------------------------------------------------------------------------- central sums

def central_sums(form, x):
    """Per output of the whole input (history: silence): the packed kernels' fp32 central sum in tap order, one fused
    rounding per term, for form.nc and form.head_nc; and the matrix pipe's exact integer floor(sum tq x / 256)"""
    n, _ = x.shape
    xp = np.concatenate([np.zeros((form.nt, x.shape[1]), dtype=np.int16), x])
    k0 = form.nt - form.d
    out = {}
    for nc in {form.nc, form.head_nc} if not form.matrix else {form.head_nc}:
        j0 = (form.ne - nc) // 2
        y = np.zeros(x.shape, dtype=np.float32)
        for j in range(j0, j0 + nc):            # float64 holds tap x sample exactly: one rounding per fused term
            y = (y.astype(np.float64) + np.float64(form.te[j]) * xp[k0 + j:k0 + j + n].astype(np.float64)).astype(np.float32)
        out[nc] = y
    if form.matrix:
        Y = np.zeros(x.shape, dtype=np.int64)
        for q, t in enumerate(form.tq):
            Y += np.int64(t) * xp[k0 + form.j0 + q:k0 + form.j0 + q + n].astype(np.int64)
        out["int"] = Y >> 8                     # arithmetic shift = floor
    return out


# ---------------------------------------------------------------------------------------------- the model

def _packed_call(form, nc, rule, xx, L, T, n_seg, yc, res, lo, upto=None):
    """One packed launch over a call: xx = int32 [NT + L][C] (history rows first), outputs 0 .. (upto or L) - 1 of the call
    are global rows lo + ..; fills res[...][lo + n]"""
    NT, ne = form.nt, form.ne
    j0 = (ne - nc) // 2
    dc = form.d - j0
    U = unroll(nc)
    NG = U // 16
    seen, ahead = (form.seen_k, form.ahead_k)
    ax = np.abs(xx)
    ax[xx == -32768] = rule.abs_min
    C = xx.shape[1]
    row = lambda m: np.clip(m, -NT, L - 1) + NT
    for by in range(n_seg):
        t0 = by * T
        if t0 >= L:
            break
        t1 = min(t0 + T, L)
        m0 = t0 - dc
        ng = (t1 - t0 + 31) // 32 * 2
        rows = m0 + nc - 1 + np.arange(ng * 16)
        G = ax[np.minimum(rows, L - 1) + NT].reshape(ng, 16, C)         # rows past the call are clamped, rows before it are history
        gm = G[:, :rule.group_rows].max(axis=1)
        gfull = G.max(axis=1)
        plo, phi = m0 - (j0 if rule.warm_from_j0 else 0), m0 + nc - 2
        w = np.maximum(np.arange(plo, phi + 1), -NT)
        wa = ax[w + NT]
        if not rule.warm_history:
            wa = np.where((w < 0)[:, None], 0, wa)
        Pm = wa.max(axis=0) if rule.primed else np.zeros(C, dtype=ax.dtype)
        h = [Pm.copy() for _ in range(rule.nhist)]
        M = np.empty((ng, C), dtype=np.int64)
        for gi in range(ng):
            if gi % NG == 0:
                h = [gm[gi]] + h[:-1]
            else:
                h[0] = np.maximum(h[0], gm[gi])
            M[gi] = np.maximum.reduce(h)
        p = np.arange(ng * 16) % 16
        cls = np.clip(np.where(p // 2 <= 4, 0, p // 2 - 4) + rule.class_shift, 0, 3)
        Mo = np.repeat(M, 16, axis=0)                                   # per output
        Mn = (Mo.astype(np.float32) * np.float32(1.0 / 32768.0)).astype(np.float64)
        thr = (np.asarray(seen, dtype=np.float64)[cls][:, None] * Mn + np.asarray(ahead, dtype=np.float64)[cls][:, None]).astype(np.float32)
        thr = (thr.astype(np.float64) * rule.thr_scale).astype(np.float32)
        nv = min(t1, upto if upto is not None else L) - t0              # outputs of this segment that this launch keeps
        if nv <= 0:
            continue
        g = slice(lo + t0, lo + t0 + nv)
        y = yc[g]
        cert = np.abs(y) >= thr[:nv]
        zero = np.zeros_like(cert)
        for wd in range((nv + 31) // 32):                               # the silence shortcut, per finished sign word
            a, b = wd * 32, min(wd * 32 + 32, nv)
            opn = ~cert[a:b]
            mb = m0 + nc - 1 + a
            before = j0 + nc - 1
            cand = (opn.sum(axis=0) >= 8) & (gfull[2 * wd] == 0) & (gfull[2 * wd + 1] == 0)
            if not cand.any():
                continue
            zb = (xx[row(np.arange(mb - before + rule.silence_behind, mb))] == 0).all(axis=0)
            za = (xx[row(np.arange(mb + 32, mb + 32 + j0 - rule.silence_ahead))] == 0).all(axis=0)
            zero[a:b] = opn & (cand & zb & za)[None, :]
        res["yc"][g], res["M"][g], res["cls"][g], res["thr"][g] = y, Mo[:nv], cls[:nv, None], thr[:nv]
        res["cert"][g], res["zero"][g] = cert, zero


def _matrix_call(form, rule, xx, L, T, head, yi, res, lo):
    NT, dc = form.nt, form.dc
    C = xx.shape[1]
    ax = np.abs(xx[NT:])
    ax[xx[NT:] == -32768] = rule.abs_min
    ax = np.concatenate([ax, np.zeros((T + 512, C), dtype=ax.dtype)])   # rows past the call's end read as zero
    for t0 in range(head, L, T):
        t1 = min(t0 + T, L)
        for k in range((t1 - t0 + 31) // 32):
            s0 = t0 + 32 * k
            w0 = s0 - dc                                                # the step's first window row
            a, b = w0 + rule.row_lo, w0 + rule.row_hi + 1
            if not rule.primed:
                a = max(a, t0)                                          # blocks 0 .. 4 are the rows before the segment's first output
            M = ax[a:b].max(axis=0) if b > a else np.zeros(C, dtype=ax.dtype)
            eps = (np.float64(np.float32(form.seen_u)) * M.astype(np.float64) + np.float64(form.abs_u)).astype(np.float32)
            E = np.ceil((eps.astype(np.float64) * rule.thr_scale).astype(np.float32)).astype(np.int64)
            nv = min(t1, s0 + 32) - s0
            g = slice(lo + s0, lo + s0 + nv)
            y = yi[g]
            res["yc"][g], res["M"][g], res["cls"][g], res["thr"][g] = y, M[None, :], -1, E[None, :]
            res["cert"][g] = (np.abs(y) >= E[None, :]) & (M != 0)[None, :]
            res["zero"][g] = np.broadcast_to((M == 0)[None, :], y.shape)   # "a channel whose M is 0 has y = +0 exactly"


def model(form, x, chunks, plan_of, rule=None, sums=None):
    """The certification decisions of `form` for input x (int16 [rows][C]) fed as calls of `chunks` rows.
    plan_of: {len: (kernel, T, head)} (plans()).  Returns arrays [rows][C]: yc (float64: the fp32 sum, or the integer y'),
    M, cls (-1: matrix pipe), thr, cert, zero (taken for +0 without a look: the silence shortcuts), pos (the certified
    sign is 'positive')."""
    rule = rule if rule is not None else (MatrixRule() if form.matrix else PackedRule())
    sums = sums if sums is not None else central_sums(form, x)
    n, C = x.shape
    res = {"yc": np.zeros((n, C)), "M": np.zeros((n, C), dtype=np.int64), "cls": np.zeros((n, C), dtype=np.int8),
           "thr": np.zeros((n, C)), "cert": np.zeros((n, C), dtype=bool), "zero": np.zeros((n, C), dtype=bool)}
    hist = np.zeros((form.nt, C), dtype=np.int32)
    lo = 0
    prule = rule if not form.matrix else PackedRule()
    for L in chunks:
        xx = np.concatenate([hist, x[lo:lo + L].astype(np.int32)])
        kernel, T, head = plan_of[L]
        if kernel == "packed+mfma":
            assert form.matrix
            _packed_call(form, form.head_nc, prule, xx, L, head, 1, sums[form.head_nc], res, lo, upto=head)
            _matrix_call(form, rule, xx, L, T, head, sums["int"], res, lo)
        else:
            assert kernel == "packed", kernel
            nc = form.head_nc if form.matrix else form.nc
            _packed_call(form, nc, prule, xx, L, T, (L + T - 1) // T, sums[nc], res, lo)
        hist = xx[-form.nt:]
        lo += L
    assert lo == n
    res["pos"] = res["cert"] & (res["yc"] > 0)
    return res


def wrong(res, ref_pos):
    """Outputs whose sign the model settles without the exact sum, and differently from the reference"""
    return (res["cert"] & (res["pos"] != ref_pos)) | (res["zero"] & ~res["cert"] & ref_pos)


# ---------------------------------------------------------------------------------------------- thresholds for the builder

def thr_at(form, M, cls):
    """The sound threshold at maximum M, in units of y (matrix pipe: E x 256 / S)"""
    if form.matrix:
        eps = np.float32(np.float64(np.float32(form.seen_u)) * M + form.abs_u)
        return float(np.ceil(eps)) * 256.0 / form.S
    return float(np.float32(np.float64(form.seen_k[cls]) * float(np.float32(M) * np.float32(1.0 / 32768.0)) + np.float64(form.ahead_k[cls])))


def central_unit(form):
    """What one unit of x under central tap q adds to the certified sum, in units of y"""
    if form.matrix:
        return np.asarray(form.tq, dtype=np.float64) / form.S
    return form.te[form.j0:form.j0 + form.nc].astype(np.float64)


def class_of(form, n):
    if form.matrix:
        return 0
    p = n % 16
    return 0 if p // 2 <= 4 else p // 2 - 4


def lone_opponent(form, cls, q, V):
    """Family A: (j, a) -- a small integer a under central tap j whose product a kernel that misses the opponent's row
    would certify (above the threshold at M = |a|, with 5 % to spare and one unit of the floor), while the opponent V
    under omitted tap q outweighs it by 5 %: the reference's sign is the opponent's.  None where no such pair exists."""
    tc = central_unit(form)
    opp = float(V) * float(form.te[q])
    best = None
    for a in (1, 2, 3):
        need = 1.05 * thr_at(form, a, cls) + (2 * 256.0 / form.S if form.matrix else 0.0)
        ok = np.nonzero(a * np.abs(tc) >= need)[0]
        if not len(ok):
            continue
        jq = ok[np.argmin(np.abs(tc[ok]))]
        v = a * abs(tc[jq])
        if best is None or v < best[0]:
            best = (v, int(jq), a)
    if best is None or abs(opp) < 1.05 * best[0] + (2 * 256.0 / form.S if form.matrix else 0.0):
        return None
    v, jq, a = best
    return form.j0 + jq, int(-np.sign(opp) * np.sign(tc[jq]) * a)


def reach(form, values=(32767, -32768)):
    """{class: [omitted taps a lone opponent can be put under]}: the teeth family A has"""
    out = {}
    for cls in (range(4) if not form.matrix else (0,)):
        out[cls] = [q for q in list(range(form.j0)) + list(range(form.j0 + form.nc, form.ne))
                    if any(lone_opponent(form, cls, q, V) for V in values)]
    return out


# ---------------------------------------------------------------------------------------------- the inputs

class Builder:
    """One pattern per (channel, time slot); explicit rows first, the rest fills the free slots in order"""

    def __init__(self, form, n_ch, rows):
        self.form, self.n_ch, self.rows = form, n_ch, rows
        self.x = np.zeros((rows, n_ch), dtype=np.int16)
        self.owner = np.full((rows, n_ch), -1, dtype=np.int32)
        self.busy = np.zeros((rows // SLOT + 2, n_ch), dtype=bool)
        self.pats = []
        self.cursor = 0
        self.rot = 0

    def _take_explicit(self, n):
        a, b = max(0, -(-(n - 708) // SLOT)), (n + 187) // SLOT
        for i in range(self.n_ch):
            c = (self.rot + i) % self.n_ch
            if not self.busy[a:b + 1, c].any():
                self.busy[a:b + 1, c] = True
                self.rot = (c + 1) % self.n_ch
                return c
        raise RuntimeError(f"no free channel for a pattern at output {n}")

    def _take_phase(self, phase):
        while True:
            k, c = 1 + self.cursor // self.n_ch, self.cursor % self.n_ch
            self.cursor += 1
            if (k + 1) * SLOT > self.rows - 700:
                raise RuntimeError("the input is too short for its patterns")
            if not self.busy[k, c]:
                self.busy[k, c] = True
                base = k * SLOT + 256
                return base + (phase - base) % self.form.period, c

    def put(self, family, samples, n=None, phase=None, out_lo=None, out_hi=None, **what):
        """samples: {effective tap j: value} under the window of output n (row n - d + j); n or the phase of n is given.
        owner[] names the pattern for every output whose window can hold one of its samples (out_lo .. out_hi around n)."""
        out_lo = -(self.form.ne - 1) if out_lo is None else out_lo
        out_hi = self.form.ne - 1 if out_hi is None else out_hi
        if n is None:
            n, c = self._take_phase(phase)
        else:
            c = self._take_explicit(n)
        f = self.form
        for j, v in samples.items():
            r = n - f.d + j
            assert 0 <= r < self.rows and self.x[r, c] == 0, (family, n, j)
            self.x[r, c] = v
        self.owner[max(0, n + out_lo):n + out_hi + 1, c] = len(self.pats)
        self.pats.append(dict(family=family, n=n, c=c, phase=n % f.period, cls=class_of(f, n), samples=dict(samples), **what))
        return n, c


def side_of(form, q):
    return "behind" if q < form.j0 else "ahead"


def greedy_central(form, target, M):
    """Integers of magnitude <= M under the central taps whose certified sum comes as close to `target` as the taps allow"""
    tc = central_unit(form)
    vals, rest = {}, target
    for jq in np.argsort(-np.abs(tc), kind="stable"):
        if tc[jq] == 0:
            continue
        v = int(np.clip(np.round(rest / tc[jq]), -min(M, 32767), min(M, 32767)))
        if v:
            vals[form.j0 + int(jq)] = v
            rest -= v * tc[jq]
    return vals


B_LEVELS = (2, 300, 12000, 32767, 32768)
B_FRACTIONS = tuple(np.round(np.arange(0.5, 1.3001, 0.05), 2))


def special_rows(form, T, head, rows):
    """Outputs at the places where the kernels change course, in the whole-input call: the first and the last step of a
    segment, either side of the head the packed kernel keeps beside the matrix pipe, the last 32 and the last output"""
    first = head if form.matrix else 0
    seams = [first + k * T for k in (1, 2)]
    out = []
    for s in seams:
        out += [(s + o, "segment seam") for o in (0, 15, 31, -1, -17, -32)]
    out += [(640 + o, "head") for o in (-32, -1, 0, 1, 32)]
    out += [(rows + o, "call end") for o in (-1, -17, -32)]
    return out


def d_rows(rows):
    """Designated outputs of family D, well inside the input and far from each other and from every seam: one per
    (cut, length of the previous call)"""
    base = 9 * SLOT + 200
    return [(base + 2 * SLOT * i, cut, short) for i, (cut, short) in enumerate((c, s) for s in (False, True) for c in D_CUTS)]


def d_chunks(rows):
    """The calls of the family-D chunking: each designated output lies `cut` rows into a call whose predecessor is long
    (whatever lies before) or short (100 rows: less than a window)"""
    cuts = []
    for n, cut, short in d_rows(rows):
        if short:
            cuts.append(n - cut - 100)
        cuts.append(n - cut)
    cuts = sorted(set(cuts))
    edges = [0] + cuts + [rows]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


def build(form, n_ch, T, head, rows=None):
    """The input of one form: families A (lone opponent), B (omitted taps at their limit), C (one sample in silence) and
    the copies of A and C whose opponent lies in the previous call of the family-D chunking.  -> (x, Builder)"""
    f = form
    ne, j0, nc, P = f.ne, f.j0, f.nc, f.period
    values = (32767, -32768, 12000, -12000)
    rc = reach(f)
    near = {cls: [q for q in qs if q >= j0 - 2 and q < j0 + nc + 2] for cls, qs in rc.items()}
    n_a = sum(len(rc[class_of(f, ph)]) for ph in range(P)) * len(values)
    n_b = len(B_LEVELS) * len(B_FRACTIONS) * 2 * (1 if f.matrix else 4)
    n_c = 2 * P * 3
    if rows is None:
        rows = SLOT * (4 + -(-int(1.15 * (n_a + n_b + n_c) + 40 * 30) // n_ch))
        rows = max(rows, 9 * SLOT + 200 + 2 * SLOT * 12 + 4 * SLOT, head + 2 * T + 4 * SLOT)
    b = Builder(f, n_ch, rows)

    def family_a(n=None, phase=None, taps=None, vals=values, family="A", **what):
        cls = class_of(f, n if n is not None else phase)
        for q in (taps if taps is not None else rc[cls]):
            for V in vals:
                ja = lone_opponent(f, cls, q, V)
                if ja is not None:
                    b.put(family, {q: V, ja[0]: ja[1]}, n=n, phase=phase, tap=q, side=side_of(f, q), V=V, j=ja[0], a=ja[1], **what)

    def family_c(r=None, phase=None, vals=(32767, 1), family="C", **what):
        # the lone sample (row r, or any row of that phase) sits under effective tap NE - 1 of output r + d - NE + 1: every
        # output up to r + d holds it
        for v in vals:
            n, _ = b.put(family, {ne - 1: v}, n=None if r is None else r + f.d - ne + 1,
                         phase=None if phase is None else (phase + f.d - ne + 1) % P, out_lo=0, out_hi=ne - 1, tap=None, V=v, **what)
            b.pats[-1]["row"] = n - f.d + ne - 1
            b.pats[-1]["phase"] = b.pats[-1]["row"] % P

    # explicit places first: the opponent under the nearest omitted taps, a lone sample under the window's two ends
    for n, where in special_rows(f, T, head, rows):
        family_a(n=n, taps=near[class_of(f, n)], vals=(32767, -32768), where=where)
        family_c(r=n - f.d + ne - 1, vals=(32767,), where=where)
        family_c(r=n - f.d, vals=(1,), where=where)
    for n, cut, short in d_rows(rows):
        family_a(n=n, taps=near[class_of(f, n)], vals=(32767, -32768), family="D", cut=cut, short=short)
        for back in (1, 60):                            # a lone sample `back` rows before the call's first row
            if cut + back <= f.d:
                family_c(r=n - cut - back, family="D", cut=cut, short=short)
    # every phase of the period
    for ph in range(P):
        family_a(phase=ph)
    for ph in range(P):
        family_c(phase=ph)
    # B: the omitted taps at their limit, the central sum swept across the threshold
    sign = np.sign(f.te.astype(np.float64))
    for cls in (range(4) if not f.matrix else (0,)):
        phase = (9, 11, 13, 15)[cls] if not f.matrix else 37
        priced = 6 - 2 * cls if not f.matrix else ne              # rows ahead that the class leaves to M
        for M in B_LEVELS:
            for frac in B_FRACTIONS:
                for sgn in (1.0, -1.0):
                    s = {}
                    for j in list(range(j0)) + list(range(j0 + nc, ne)):
                        lim = M if j < j0 + nc + priced else 32768
                        s[j] = int(np.clip(-lim * sign[j], -32768, 32767))
                    s.update(greedy_central(f, sgn * frac * thr_at(f, M, cls), M))
                    b.put("B", s, phase=phase, tap=None, M=M, frac=float(frac), sgn=sgn)
    return b.x, b


def chunkings(rows, T):
    """name -> call lengths: what the GPU test feeds and the CPU test models"""
    around = [640, 641, 639, T, T + 1, T - 1, 1, 33]
    return {"one call": [rows],
            "on and around the head and the segment length": around + [rows - sum(around)],
            "family D cuts": d_chunks(rows),
            "calls of 1920 + 1 rows": [1921] * (rows // 1921) + ([rows % 1921] if rows % 1921 else [])}


def describe(b, n, c):
    """The pattern an output belongs to, for a failure message"""
    o = int(b.owner[n, c])
    if o < 0:
        return f"output {n} channel {c}: no pattern"
    p = b.pats[o]
    return (f"output {n} channel {c}: family {p['family']} phase {p['phase']} class {p['cls']} tap {p.get('tap')} "
            f"value {p.get('V', p.get('M'))} designated output {p['n']}" + (f" cut {p['cut']}" if "cut" in p else ""))


@dataclass
class Case:
    form: Form
    n_ch: int
    T: int
    head: int
    x: np.ndarray
    b: Builder
    chunks: dict                # chunkings()
    plan_of: dict               # {len: (kernel, T, head)} for every call length of every chunking


def make_case(taps, name, n_ch, workdir, sanitize=True):
    """The input of one form with its chunkings and their plans (fir_T = FIR_T)"""
    form = load_forms(taps, workdir, sanitize=sanitize)[name]
    pk = dict(form.options).get("fir_pk_taps", 0)
    _, T, head = plans(taps, workdir, n_ch, [10 ** 6], FIR_T, pk, sanitize=sanitize)[10 ** 6]
    x, b = build(form, n_ch, T, head)
    ch = chunkings(x.shape[0], T)
    plan_of = plans(taps, workdir, n_ch, [n for c in ch.values() for n in c], FIR_T, pk, sanitize=sanitize)
    return Case(form, n_ch, T, head, x, b, ch, plan_of)
