"""csrc/rsik_math.hpp at the places where its algorithms can go wrong, against mpmath at 50 digits.

test_device_math_accuracy (test_gpu_parity.py) draws its inputs at random and compares with the host libm.  The seams of these
algorithms have measure zero — the rounding points of the unit-atan table index, the octant diagonal, c = +-0, the rint ties of
the sincos reduction, the & 63 wrap of its table row, the end of its documented domain — so every input here is constructed, none
is drawn, and the reference is evaluated on the very doubles that are uploaded.  Each test prints its largest error in radians
(or as a value) and in ulp of the true result before it asserts.

Part A (ops 0-5 and 7 of rsik_debug_math) runs width 1 of every function, op 7 also against an exact-arithmetic emulation
that takes the documented table row (an error bound cannot see a seam that sits slightly off); Part B (ops 9-19) runs the same inputs through every
lock-step width the kernels instantiate, every input visiting every slot.  test_inputs_hit_the_seams needs no GPU: it checks
that the inputs are where the GPU tests need them to be."""
import functools
import math
import os
import re
import struct
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from gpu_support import torch_mod  # noqa: F401

MP = mpmath.mp.clone()
MP.dps = 50

PI, TWO_PI = math.pi, 2 * math.pi
STEPS, HALF = 24, 18          # rsik_poly_gen.hpp: kUnitAtanSteps, kUnitAtanHalf
UNIT_ATAN_BOUND = 1.2e-15     # rad: test_device_math_accuracy's bound for op 7 (dropped x^9 term of the asin + roundings)
SINCOS_BOUND = 2e-16          # rsik_math.hpp: "fast_sincos ... abs error < 2e-16"
# rsik_math.hpp claimed "fast_atan2 ... abs error < 3e-16 rad".  That holds for |result| <= pi/2 (asserted below); where x < 0 the
# last step pi - r adds fl(pi)'s own 1.22e-16 and a rounding of up to 2.22e-16 (half an ulp of a result in [2, 4)), and the
# MI355X gives 3.8652e-16 at (y, x) = (0x1.81cd6c8b43954p+13, -0x1.81cd6c8b43958p+13), true angle 2.356194490192345223523... (docs/experiments.md,
# part M).  The bound is that measured maximum plus 10 %: the reference is exact and the kernel deterministic, the margin only
# covers a later re-ordering of independent operations.
ATAN2_BOUND = 4.2518e-16
ATAN2_BOUND_RIGHT_HALF = 3e-16
SQRT_EXACT_FROM = 2.0 ** -970   # sqrt_cr / sqrt_rsqrt are correctly rounded from here up (rsik_math.hpp; reasoning in root_set)
WIDTH_OPS = {"unit_atan2": {2: 9, 3: 10, 4: 11, 7: 12}, "fast_atan2": {2: 13, 3: 14, 4: 15, 7: 16}, "fast_sincos": {2: 17, 3: 18, 4: 19}}


# ------------------------------------------------------------------------------------------------ doubles, exactly
def step(x, k):
    """x moved by k ulp on its magnitude (k > 0: away from zero); x finite and not 0."""
    m = np.array([abs(x)], dtype=np.float64)
    out = float((m.view(np.int64) + k).view(np.float64)[0])
    return math.copysign(out, x)


def ibits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def split(vals):
    """mpf values as double-double (hi, lo): (g - hi) - lo is then g's error to ~1e-32 relative, in float64 arithmetic."""
    hi = np.array([float(v) for v in vals], dtype=np.float64)
    lo = np.array([float(v - MP.mpf(h)) for v, h in zip(vals, hi.tolist())], dtype=np.float64)
    return hi, lo


def error(got, ref):
    hi, lo = ref
    return np.abs((got - hi) - lo)


def ulp_of(hi):
    """ulp of the true result (0 where it is 0)."""
    _, e = np.frexp(hi)
    return np.where(hi == 0, 0.0, np.ldexp(1.0, e - 53))


def report(name, err, ref, *inputs, say=True):
    k = int(np.argmax(err))
    u = ulp_of(ref[0])
    in_ulp = np.where(u > 0, err / np.where(u > 0, u, 1.0), 0.0)
    ku = int(np.argmax(in_ulp))
    if say:
        print(f"{name}: n = {len(err)}, max |error| = {err[k]:.4e} at {tuple(float(a[k]).hex() for a in inputs)} (true {ref[0][k]!r}); "
              f"max = {in_ulp[ku]:.3f} ulp of the true result at {tuple(float(a[ku]).hex() for a in inputs)}")
    return float(err[k])


def pythagoras_defect(s, c):
    """|s^2 + c^2 - 1| for |s|, |c| <= 1 to ~1e-32, in float64: Dekker's exact squares, an exact sum, then 1 comes off exactly."""
    def square(a):
        t = 134217729.0 * a
        ah = t - (t - a)
        al = a - ah
        p = a * a
        return p, ((ah * ah - p) + 2.0 * ah * al) + al * al

    (ps, es), (pc, ec) = square(s), square(c)
    t = ps + pc
    v = t - ps
    e = (ps - (t - v)) + (pc - v)
    return np.abs((t - 1.0) + (e + es + ec))


def scaled(v, num):
    """fl(v * (1 + num * 2^-53)), rounded once."""
    return float(Fraction(v) * (1 + Fraction(num, 2 ** 53)))


def unit_atan_index(mn):
    """idx = (int)fma(mn, 24, 0.5) as the device computes it: one rounding, then truncation."""
    return int(float(Fraction(mn) * STEPS + Fraction(1, 2)))


def fma(a, b, c):
    """a * b + c rounded once, like v_fma_f64."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@functools.lru_cache(maxsize=None)
def unit_atan_tables():
    """c_unit_atan_tab and the three asin coefficients (highest first) as the generated header holds them."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reachy2_symbolic_ik_amd", "csrc")
    with open(os.path.join(csrc, "rsik_poly_gen.hpp")) as fh:
        src = fh.read()
    rows = re.findall(r"\{([^{}]+)\}", src[src.index("c_unit_atan_tab"):])[:3]
    tab = [[float(v) for v in r.split(",")] for r in rows]
    assert [len(r) for r in tab] == [4 * HALF] * 3
    words = re.findall(r"s_mov_b32 s9[45], 0x([0-9a-f]{8})", src[src.index("void horner_asin_p<1>"):])[:6]   # low word, high word
    coeffs = [struct.unpack("<d", struct.pack("<II", int(lo, 16), int(hi, 16)))[0] for lo, hi in zip(words[0::2], words[1::2])]
    return tab, coeffs


def emulate_unit_atan2(s, c):
    """unit_atan2_n's own sequence of operations (rsik_math.hpp) in exact arithmetic, each step rounded once, with the table row the
    header documents: idx = (int)(mn * 24 + 0.5), the half from c's sign bit, the octant from |s| > |c|."""
    tab, (c2, c1, c0) = unit_atan_tables()
    ac, as_ = abs(c), abs(s)
    mx, mn = max(ac, as_), min(ac, as_)
    row = 2 * (unit_atan_index(mn) + HALF * int(math.copysign(1.0, c) < 0)) + int(as_ > ac)
    ci, si, phi = tab[0][row], tab[1][row], tab[2][row]
    x = fma(mn, ci, -(mx * si))
    x2 = x * x
    p = fma(fma(c2, x2, c1), x2, c0)
    return math.copysign(phi + fma(x * x2, p, x), s)


# ------------------------------------------------------------------------------------------------ input sets (built once)
class Points:
    def __init__(self):
        self.cols, self.ladders, self.tags = [], [], []

    def add(self, rows, tag, ladder=False):
        first = len(self.cols)
        self.cols.extend(rows)
        self.tags.extend([tag] * len(rows))
        idx = list(range(first, len(self.cols)))
        if ladder:
            self.ladders.append(idx)
        return idx


def _unit_vectors():
    """(s, c) of op 7, unscaled: seams, diagonal, axes, smallest angles, table nodes; ladders are runs of ulp neighbours."""
    P = Points()
    comp = lambda v: float(MP.sqrt(1 - MP.mpf(v) ** 2))  # noqa: E731  the larger component, rounded once
    signs = [(a, b) for a in (1.0, -1.0) for b in (1.0, -1.0)]

    def both_octants(mns, tag):
        for swap in (False, True):
            for ss, sc in signs:
                rows = [(ss * comp(mn), sc * mn) if swap else (ss * mn, sc * comp(mn)) for mn in mns]
                P.add(rows, tag, ladder=len(rows) > 1)

    for i in range(HALF - 1):  # the 17 rounding seams of idx = (int)(mn * 24 + 0.5)
        both_octants([step((i + 0.5) / STEPS, d) for d in range(-8, 9)], f"seam{i}")
    h = float(MP.sqrt(MP.mpf(1) / 2))
    for ss, sc in signs:  # the diagonal |s| = |c| and +-1 ... 4 ulp in each component: rows and columns of a 9 x 9 grid
        grid = [P.add([(ss * step(h, ds), sc * step(h, dc)) for dc in range(-4, 5)], "diagonal", ladder=True) for ds in range(-4, 5)]
        P.ladders.extend([[grid[r][c] for r in range(9)] for c in range(9)])
    axes = [(0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (1.0, -0.0), (-1.0, 0.0), (-1.0, -0.0)]
    P.add(axes, "axis")
    # smallest angles s = +-2^-k beside c = +-1: c is sqrt(1 - s^2) rounded, which IS +-1 from k = 27 on (below that (s, +-1) is no
    # unit vector: its norm is off by 2^(-2k-1)); and the same beside the other axis
    both_octants([2.0 ** -k for k in range(10, 61)], "small")
    for i in range(1, HALF - 1):  # exact table nodes mn = i / 24 (i = 0 is the axes), with their ulp neighbours
        both_octants([step(i / STEPS, d) if d else i / STEPS for d in (-1, 0, 1)], f"node{i}")
    return P


@functools.lru_cache(maxsize=None)
def unit_atan_set():
    """Every unit vector of _unit_vectors() as built and with both components scaled by 1 +- j 2^-53, j = 1 ... 4 (what
    rsqrt_fast's normalisation supplies); the mpmath angle of each uploaded pair; ladder neighbours as index pairs."""
    P = _unit_vectors()
    n0 = len(P.cols)
    s, c, tags, pairs = [], [], [], []
    for num in [0] + [sg * j for j in range(1, 5) for sg in (1, -1)]:
        off = len(s)
        s.extend(scaled(a, num) for a, _ in P.cols)
        c.extend(scaled(b, num) for _, b in P.cols)
        tags.extend(P.tags)
        for lad in P.ladders:
            pairs.extend((off + p, off + q) for p, q in zip(lad[:-1], lad[1:]))
    ref = []
    for a, b in zip(s, c):
        t = MP.atan2(MP.mpf(abs(a)), MP.mpf(b))  # (mpf has no -0: the sign of s, zero included, is put back)
        ref.append(-t if math.copysign(1.0, a) < 0 else t)
    pairs = np.array(pairs)
    return dict(s=np.array(s), c=np.array(c), tags=tags, n_unscaled=n0, ref=split(ref), p=pairs[:, 0], q=pairs[:, 1],
                axes=[i for i, t in enumerate(P.tags) if t == "axis"])


def _sincos_ks():
    """(k, inside the documented domain |x| < 1e5) of the reduction seams x = (k + 1/2) pi/32."""
    ks = list(range(-64, 65))
    for c in (2 ** 10, 2 ** 15):
        ks += [sg * (c + d) for sg in (1, -1) for d in range(-2, 3)]
    kmax = int(MP.floor(MP.mpf(10) ** 5 * 32 / MP.pi - MP.mpf(1) / 2))
    while not step(float((2 * kmax + 1) * MP.pi / 64), 8) < 1e5:
        kmax -= 1
    ks += [kmax]   # the largest k with |x| < 1e5, ladder included (sincos_set adds every x's mirror image)
    inside = [(k, True) for k in ks]
    # k up to 2^20 is what the header states for the exactness of the head product; these x (|x| ~ 1.03e5) lie past its "|x| < 1e5"
    edge = [(sg * (2 ** 20 - 64 + d), False) for sg in (1, -1) for d in range(-2, 3)]
    return inside + edge


@functools.lru_cache(maxsize=None)
def sincos_set():
    xs, tags = [], []

    def add(vals, tag):
        xs.extend(vals)
        tags.extend([tag] * len(vals))

    for k, inside in _sincos_ks():
        tag = "seam" if inside else "seam_2^20"
        add([step(float((2 * k + 1) * MP.pi / 64), d) for d in range(-8, 9)], tag)   # rint can fall either way
        if k:
            add([float(k * MP.pi / 32)], "node" if inside else "node_2^20")           # r ~ 0
    for m in range(-8, 9):
        if m:
            add([step(float(m * MP.pi / 2), d) for d in range(-4, 5)], "quadrant")    # one of sin / cos tiny, the other +-1
    add([0.0], "zero")
    add([2.0 ** -k for k in range(1, 61)], "small")
    add([float(np.nextafter(1e5, 0.0))], "top")
    x = np.array(xs + [-v for v in xs])   # every x with its mirror image: [0, n) and [n, 2n)
    tags = tags + tags
    sn, cs = zip(*[(MP.sin(MP.mpf(v)), MP.cos(MP.mpf(v))) for v in x.tolist()])
    return dict(x=x, tags=tags, half=len(xs), sin=split(sn), cos=split(cs))


@functools.lru_cache(maxsize=None)
def atan2_set():
    P = Points()
    signs = [(a, b) for a in (1.0, -1.0) for b in (1.0, -1.0)]
    for m in (1.0, 0.3, 1.0 / 3.0, 7.0, 1e-3, 12345.678, 1e-150, 1e150):   # |y| = |x|: ay > ax flips, a crosses 1
        for sy, sx in signs:
            P.add([(sy * step(m, d), sx * m) for d in range(-4, 5)], "diagonal", ladder=True)
            P.add([(sy * m, sx * step(m, d)) for d in range(-4, 5)], "diagonal", ladder=True)
    for sy, sx in signs:   # ratios 2^-k both ways; every operand and every true result is a normal number
        P.add([(sy * 2.0 ** -k, sx * 1.0) for k in range(1, 1001)], "ratio")
        P.add([(sy * 1.0, sx * 2.0 ** -k) for k in range(1, 1001)], "ratio")
    for ratio in (1.0, 0.75, 0.1, 1e-3):   # the same ratio from 1e-150 to 1e150
        for sy, sx in signs:
            P.add([(sy * ratio * 10.0 ** e, sx * 10.0 ** e) for e in range(-150, 151, 10)], "magnitude")
            P.add([(sy * 10.0 ** e, sx * ratio * 10.0 ** e) for e in range(-150, 151, 10)], "magnitude")
    zeros = [(y, x) for y in (0.0, -0.0) for x in (0.0, -0.0, 1.0, -1.0)] + [(y, x) for y in (1.0, -1.0) for x in (0.0, -0.0)]
    P.add(zeros, "zero")
    # test_device_math_accuracy's edge list
    P.add(list(zip([0.0, 0.0, -0.0, 1.0, -1.0, 0.0, 1e-300, 3.0], [0.0, -0.0, -0.0, 0.0, 0.0, -2.0, 1.0, 3.0])), "edge")
    y = np.array([r[0] for r in P.cols])
    x = np.array([r[1] for r in P.cols])
    ref = []
    for a, b in P.cols:
        if a == 0 and b == 0:
            t = MP.pi if math.copysign(1.0, b) < 0 else MP.mpf(0)   # C's atan2(+-0, -0) = +-pi, atan2(+-0, +0) = +-0
        elif b == 0:
            t = MP.pi / 2
        else:
            t = MP.atan2(MP.mpf(abs(a)), MP.mpf(b))
        ref.append(-t if math.copysign(1.0, a) < 0 else t)
    pairs = np.array([(p, q) for lad in P.ladders for p, q in zip(lad[:-1], lad[1:])])
    return dict(y=y, x=x, tags=P.tags, ref=split(ref), p=pairs[:, 0], q=pairs[:, 1], zeros=[i for i, t in enumerate(P.tags) if t == "zero"])


@functools.lru_cache(maxsize=None)
def root_set():
    """Normal x > 0 whose 1/x, sqrt(x) and 1/sqrt(x) are normal too.  The roots are correctly rounded from x = 2^-970 up and not
    below: their last two steps need the residual x - g^2 exactly, g^2 is a multiple of ulp(g)^2 = 2^(2 (floor(e/2) - 52)) for x in
    [2^e, 2^(e+1)), and that is below the smallest denormal, 2^-1074, for e < -970.  (The kernels take roots of squared lengths.)"""
    xs = []
    for k in range(-1021, 1022):   # powers of two (below and above each power of four the v_rsq seed changes exponent parity)
        xs += [step(2.0 ** k, -1), 2.0 ** k, step(2.0 ** k, 1)]
    squares = list(range(1, 130)) + [2 ** 26 - 1, 2 ** 26, 2 ** 26 + 1, 94906265, 3 ** 16, 10 ** 7]   # n^2 <= 2^53: exact
    for n in squares:
        xs += [step(float(n * n), -1), float(n * n), step(float(n * n), 1)]
    for k in range(1, 53):   # mantissas 1 + 2^-k at both exponent parities, and far out
        xs += [e * (1.0 + 2.0 ** -k) for e in (1.0, 2.0, 2.0 ** -40, 2.0 ** 41)]
    x = np.array(xs)
    assert np.all(x > 0) and np.all(np.isfinite(x))
    m = [MP.mpf(v) for v in xs]
    cr = lambda vals: np.array([float(v) for v in vals])  # noqa: E731  correctly rounded: 50 digits, then one rounding
    return dict(x=x, rcp=cr(1 / v for v in m), sqrt=cr(MP.sqrt(v) for v in m), rsqrt=cr(1 / MP.sqrt(v) for v in m))


@functools.lru_cache(maxsize=None)
def pymod_set():
    """(a, b) of op 5.  pymod_2pi's comment gives its domain as "the small quotients on this path": the largest here is 1000 turns."""
    a, b = [], []

    def add(av, bv=0.0):
        a.append(av)
        b.append(bv)

    add(0.0), add(-0.0)
    for k in range(1, 101):
        add(-(2.0 ** -k)), add(2.0 ** -k)      # -2^-k: Python gives fl(2 pi - 2^-k), which is fl(2 pi) itself from k = 51 on
    for k in range(-1000, 1001):
        t = k * TWO_PI
        for d in (-2, -1, 0, 1, 2):
            add(step(t, d) if (d and k) else t)
    for v in (PI, -PI, 3 * PI, -3 * PI):
        for d in range(-4, 5):
            add(step(v, d))
    for bv in (0.5, 1.0, 2.0, PI / 2, -1.25, 3.0, 1e-3):   # (a - b) + pi within 4 ulp of 0 and of fl(2 pi)
        for d in range(-4, 5):
            add(step(bv - PI, d), bv)
            add(step(bv + PI, d), bv)
            add(bv, step(bv + PI, d))
            add(bv, step(bv - PI, d))
    a, b = np.array(a), np.array(b)
    mod = np.array([v % TWO_PI for v in a.tolist()])
    diff = np.array([((u - v + PI) % TWO_PI) - PI for u, v in zip(a.tolist(), b.tolist())])
    return dict(a=a, b=b, mod=mod, diff=diff)


# ------------------------------------------------------------------------------------------------ the inputs themselves (no GPU)
def test_inputs_hit_the_seams():
    """The GPU tests cannot pass vacuously: every unit-atan seam has inputs whose table index differs on its two sides (in both
    octants and all four sign combinations, at every scaling), every unit vector is within 8 ulp(1) = 8 x 2^-52 of norm 1, every
    residue k mod 64 of either sign occurs among the sincos inputs, and every sincos input is inside |x| < 1e5 — except the ones
    the k ~ 2^20 - 64 seams need, which lie past 1e5 (|x| ~ 1.03e5) but inside |k| < 2^20, the limit the header gives for the exact
    head product."""
    U = unit_atan_set()
    s, c = U["s"], U["c"]
    norm_err = max(abs(float(MP.sqrt(MP.mpf(a) ** 2 + MP.mpf(b) ** 2) - 1)) for a, b in zip(s[::7].tolist(), c[::7].tolist()))
    nerr2 = np.abs(s * s + c * c - 1.0).max()   # (all of them, in float64: |s^2 + c^2 - 1| ~ 2 |norm - 1|)
    assert norm_err <= 8 * 2.0 ** -52 and nerr2 <= 2 * 8 * 2.0 ** -52 + 2.0 ** -52, (norm_err, nerr2)
    idx = np.array([unit_atan_index(min(abs(a), abs(b))) for a, b in zip(s.tolist(), c.tolist())])
    tags = np.array(U["tags"])
    n0 = U["n_unscaled"]
    for block in range(len(s) // n0):
        sl = slice(block * n0, (block + 1) * n0)
        for i in range(HALF - 1):
            m = tags[sl] == f"seam{i}"
            for swap in (False, True):
                for neg_s in (False, True):
                    for neg_c in (False, True):
                        sel = m & ((np.abs(s[sl]) > np.abs(c[sl])) == swap) & (np.signbit(s[sl]) == neg_s) & (np.signbit(c[sl]) == neg_c)
                        assert set(idx[sl][sel]) == {i, i + 1}, (block, i, swap, neg_s, neg_c, set(idx[sl][sel]))
    assert idx.max() == HALF - 1 and idx.min() == 0   # the diagonal reaches the last row of each half

    S = sincos_set()
    x, stags = S["x"], np.array(S["tags"])
    k = np.array([int(MP.nint(MP.mpf(v) * 32 / MP.pi)) for v in x.tolist()])
    inside = ~np.isin(stags, ["seam_2^20", "node_2^20"])
    assert np.all(np.abs(x[inside]) < 1e5) and np.abs(x[inside]).max() == np.nextafter(1e5, 0.0)
    assert np.all(np.abs(k) < 2 ** 20) and np.abs(k[~inside]).min() >= 2 ** 20 - 67
    assert {int(v) % 64 for v in k[k > 0]} == set(range(64)) and {int(v) % 64 for v in k[k < 0]} == set(range(64))
    # each seam ladder straddles its tie: the device's own k = rint(fl(x * fl(32/pi))) takes two values on it
    kd = np.rint(x * 10.185916357881302)
    lad = kd[: S["half"]][stags[: S["half"]] == "seam"].reshape(-1, 17)
    assert np.all(lad.max(axis=1) - lad.min(axis=1) == 1)
    assert np.array_equal(x[: S["half"]], -x[S["half"]:])

    A = atan2_set()
    assert np.all((np.abs(A["y"]) >= 2.0 ** -1022) | (A["y"] == 0)) and np.all((np.abs(A["x"]) >= 2.0 ** -1022) | (A["x"] == 0))
    R = root_set()
    tiny = 2.0 ** -1022
    assert min(R["x"].min(), R["rcp"].min(), R["sqrt"].min(), R["rsqrt"].min()) >= tiny and len(set(R["x"].tolist())) > 6000
    M = pymod_set()
    assert np.any(M["mod"] == TWO_PI) and np.any(M["diff"] == PI) and np.any(M["diff"] == -PI) and np.abs(M["a"]).max() < 6284


# ------------------------------------------------------------------------------------------------ Part A: width 1
def _solver():
    from reachy2_symbolic_ik_amd import HipSolver

    return HipSolver(0)


def _run(torch_mod, hs, op, a, b=None):
    t = lambda v: torch_mod.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).cuda()  # noqa: E731
    o0, o1 = hs.debug_math(op, t(a), None if b is None else t(b))
    return o0.cpu().numpy(), o1.cpu().numpy()


def _rotated(torch_mod, hs, op, rot, a, b=None):
    """Element i goes through slot (i + rot) mod N of the width-N ops; the results come back in the inputs' order."""
    o0, o1 = _run(torch_mod, hs, op, np.roll(a, rot), None if b is None else np.roll(b, rot))
    return np.roll(o0, -rot), np.roll(o1, -rot)


def check_unit_atan2(got, name, say=True):
    U = unit_atan_set()
    s, ref = U["s"], U["ref"]
    err = error(got, ref)
    worst = report(name, err, ref, s, U["c"], say=say)
    assert np.array_equal(np.signbit(got), np.signbit(s)), "the result's sign is the sign of s"
    assert np.all(np.abs(got) <= PI)
    ax = U["axes"]
    want = np.array([math.atan2(a, b) for a, b in zip(s[ax].tolist(), U["c"][ax].tolist())])
    assert np.array_equal(ibits(got[ax]), ibits(want)), (got[ax], want)   # +-0, +-pi, +-pi/2 with C's signs
    assert worst < UNIT_ATAN_BOUND
    # ulp neighbours, across every seam and the diagonal: a wrong row is a jump, and the result follows the true angle's order
    p, q = U["p"], U["q"]
    e = (got - ref[0]) - ref[1]
    jump = np.abs(e[q] - e[p])
    if say:
        print(f"{name}: largest jump between ulp neighbours = {jump.max():.4e} rad over {len(p)} pairs")
    assert jump.max() <= 2 * UNIT_ATAN_BOUND
    rising = ((ref[0][q] - ref[0][p]) + (ref[1][q] - ref[1][p])) >= 0
    assert np.all((got[q] - got[p])[rising] >= -2 * UNIT_ATAN_BOUND) and np.all((got[p] - got[q])[~rising] >= -2 * UNIT_ATAN_BOUND)
    return worst


def check_sincos(sn, cs, name, say=True):
    S = sincos_set()
    x, h = S["x"], S["half"]
    es = report(name + " sin", error(sn, S["sin"]), S["sin"], x, say=say)
    ec = report(name + " cos", error(cs, S["cos"]), S["cos"], x, say=say)
    zero = x == 0
    assert np.all(sn[zero] == 0) and np.all(cs[zero] == 1.0)
    one = pythagoras_defect(sn, cs)
    if say:
        print(f"{name}: max |sin^2 + cos^2 - 1| = {one.max() / 2.0 ** -52:.3f} ulp(1)")
    assert one.max() <= 4 * 2.0 ** -52
    # odd / even, bit for bit: k = rint(x * fl(32/pi)) is odd in x, ties included (to even on both sides), and so is all that follows
    assert np.array_equal(sn[:h], -sn[h:]) and np.array_equal(cs[:h], cs[h:])
    assert es < SINCOS_BOUND and ec < SINCOS_BOUND, (es, ec)
    return max(es, ec)


def check_atan2(got, name, say=True):
    A = atan2_set()
    y, x, ref = A["y"], A["x"], A["ref"]
    worst = report(name, error(got, ref), ref, y, x, say=say)
    z = A["zeros"]
    want = np.array([math.atan2(a, b) for a, b in zip(y[z].tolist(), x[z].tolist())])
    assert np.array_equal(ibits(got[z]), ibits(want)), (got[z], want)
    assert np.array_equal(np.signbit(got), np.signbit(y)) and np.all(np.abs(got) <= PI)
    e = (got - ref[0]) - ref[1]
    assert np.abs(e[A["q"]] - e[A["p"]]).max() <= 2 * ATAN2_BOUND
    right = np.abs(ref[0]) <= PI / 2
    if say:
        print(f"{name}: max |error| = {np.abs(e[right]).max():.4e} where |result| <= pi/2")
    assert worst < ATAN2_BOUND and np.abs(e[right]).max() < ATAN2_BOUND_RIGHT_HALF
    return worst


@pytest.mark.gpu
def test_unit_atan2_at_its_table_seams(torch_mod):
    """op 7, unit_atan2_n<1>: both sides of all 17 index seams in both octants and four sign combinations, the diagonal, the
    axes (C's signed results exactly), angles down to 2^-60, the table nodes — as built (the larger component is
    sqrt(1 - mn^2) rounded) and scaled by 1 +- j 2^-53.  Against mpmath.atan2 of the uploaded doubles: 1.2e-15 rad, the
    sign of s, |result| <= fl(pi), and no jump or inversion between ulp neighbours beyond twice the bound."""
    U = unit_atan_set()
    got, _ = _run(torch_mod, _solver(), 7, U["s"], U["c"])
    check_unit_atan2(got, "unit_atan2_n<1>")


@pytest.mark.gpu
def test_unit_atan2_takes_the_documented_table_row(torch_mod):
    """op 7 on the unscaled seam, diagonal, axis, small-angle and node inputs against emulate_unit_atan2, bit for bit.  The error
    bound cannot see a seam that sits a little off (i + 0.5)/24: either neighbouring row stays within 1.2e-15 there (the dropped
    asin term only grows with the 9th power of the overshoot).  The bits can: the two rows round differently."""
    U = unit_atan_set()
    n = U["n_unscaled"]
    s, c = U["s"][:n], U["c"][:n]
    got, _ = _run(torch_mod, _solver(), 7, s, c)
    want = np.array([emulate_unit_atan2(a, b) for a, b in zip(s.tolist(), c.tolist())])
    bad = np.flatnonzero(ibits(got) != ibits(want))
    print(f"unit_atan2_n<1>: {len(bad)} of {n} results differ from the emulation with the documented row" + "".join(
        f"\n    (s, c) = ({float(s[i]).hex()}, {float(c[i]).hex()}) [{U['tags'][i]}]: device {float(got[i]).hex()}, emulation {float(want[i]).hex()}"
        for i in bad[:8]))
    assert len(bad) == 0


@pytest.mark.gpu
def test_sincos_at_its_reduction_seams(torch_mod):
    """op 4, fast_sincos_n<1>: x = fl((k + 1/2) pi/32) +- 0 ... 8 ulp (|r| reaches pi/64 and rint falls either way) and fl(k pi/32) for
    every residue of k mod 64 of either sign, k near 2^10, 2^15, the largest k inside |x| < 1e5 and k near 2^20 - 64 (the header's
    limit for the exact head product; these |x| ~ 1.03e5 are past the "|x| < 1e5" of the same header and held to the same bound);
    multiples of pi/2 +- 0 ... 4 ulp, +-0, +-2^-k, +-nextafter(1e5, 0).  Against mpmath on the uploaded doubles: the header's 2e-16
    for sin and cos, sin(+-0) = 0 and cos(0) = 1 exactly, sin^2 + cos^2 within 4 ulp of 1, and odd / even symmetry bit for bit
    (rint's ties go to even on both sides of 0, so they do not break it)."""
    sn, cs = _run(torch_mod, _solver(), 4, sincos_set()["x"])
    check_sincos(sn, cs, "fast_sincos_n<1>")


@pytest.mark.gpu
def test_atan2_at_the_diagonal_and_extreme_ratios(torch_mod):
    """op 3, fast_atan2_n<1>: |y| = |x| +- 0 ... 4 ulp in the four quadrants, ratios 2^-k (k = 1 ... 1000) both ways, magnitudes
    1e-150 ... 1e150 at fixed ratios, the signed zeros (math.atan2 exactly) and test_device_math_accuracy's edge list.  Against
    mpmath: 3e-16 rad where |result| <= pi/2, ATAN2_BOUND (see there: the header's 3e-16 was optimistic for x < 0) everywhere."""
    A = atan2_set()
    got, _ = _run(torch_mod, _solver(), 3, A["y"], A["x"])
    check_atan2(got, "fast_atan2_n<1>")


@pytest.mark.gpu
def test_rcp_sqrt_rsqrt_over_the_exponent_range(torch_mod):
    """ops 0-2: 2^k and 2^k (1 +- ulp) for every k whose results are normal (the v_rsq seed changes exponent parity at each power
    of four), perfect squares and their ulp neighbours, mantissas 1 + 2^-k.  sqrt_rsqrt's and sqrt_cr's roots are the correctly
    rounded mpmath.sqrt bit for bit; fast_rcp and rsqrt_fast are within 1 ulp of the correctly rounded value, counted on the
    integer representation.  Roots of x < 2^-970, outside the header's (corrected) domain, are only reported."""
    R = root_set()
    hs = _solver()
    x = R["x"]
    r, _ = _run(torch_mod, hs, 0, x)
    s1, s2 = _run(torch_mod, hs, 1, x)
    rs, _ = _run(torch_mod, hs, 2, x)
    dom = x >= SQRT_EXACT_FROM
    for name, got in (("sqrt_rsqrt", s1), ("sqrt_cr", s2)):
        off = np.abs(ibits(got) - ibits(R["sqrt"]))
        bad = np.flatnonzero(off)
        print(f"{name}: {len(bad)} of {len(x)} roots are not correctly rounded" + (
            f": x from {float(x[bad].min()).hex()} to {float(x[bad].max()).hex()}, {off.max()} ulp at most" if len(bad) else "")
            + f"; {int(np.count_nonzero(off[dom]))} of them at x >= 2^-970")
    d_rcp = np.abs(ibits(r) - ibits(R["rcp"]))
    d_rs = np.abs(ibits(rs) - ibits(R["rsqrt"]))
    print(f"fast_rcp: max {d_rcp.max()} ulp from the correctly rounded value at x = {float(x[np.argmax(d_rcp)]).hex()}; "
          f"rsqrt_fast: max {d_rs.max()} ulp at x = {float(x[np.argmax(d_rs)]).hex()}")
    assert np.array_equal(ibits(s1[dom]), ibits(R["sqrt"][dom])) and np.array_equal(ibits(s2[dom]), ibits(R["sqrt"][dom]))
    assert d_rcp.max() <= 1 and d_rs.max() <= 1


@pytest.mark.gpu
def test_python_modulo_and_angle_diff_at_the_turns(torch_mod):
    """op 5, pymod_2pi and angle_diff against Python's own % on the same doubles, bit for bit: +-0, +-2^-k (-2^-k % 2 pi rounds to
    fl(2 pi) itself from k = 51 on), k fl(2 pi) and its ulp neighbours for |k| <= 1000, +-pi, +-3 pi and neighbours, and (a - b) + pi
    within 4 ulp of 0 and of fl(2 pi)."""
    M = pymod_set()
    m, ad = _run(torch_mod, _solver(), 5, M["a"], M["b"])
    bad_m = np.flatnonzero(ibits(m) != ibits(M["mod"]))
    bad_d = np.flatnonzero(ibits(ad) != ibits(M["diff"]))
    for name, bad, got, want in (("pymod_2pi", bad_m, m, M["mod"]), ("angle_diff", bad_d, ad, M["diff"])):
        print(f"{name}: {len(bad)} of {len(got)} differ from Python" + "".join(
            f"\n    a = {M['a'][i]!r}, b = {M['b'][i]!r}: device {got[i]!r}, Python {want[i]!r}" for i in bad[:8]))
    assert len(bad_m) == 0 and len(bad_d) == 0


# ------------------------------------------------------------------------------------------------ Part B: every lock-step width
@pytest.mark.gpu
def test_every_lockstep_width_in_every_slot(torch_mod):
    """ops 9-19: unit_atan2_n<N> and fast_atan2_n<N> for N = 2, 3, 4, 7 and fast_sincos_n<N> for N = 2, 3, 4 (its callers' NC is
    2 or 4) — the widths the kernels instantiate, each with generated Horner blocks and operand numbering of its own.  The
    whole Part A input set of each function goes through each width N times, rotated by 0 ... N - 1 places, so that every seam
    value visits every slot; Part A's assertions hold in every slot, and every slot returns the bits of width 1: per element
    the widths run the same sequence of operations."""
    hs = _solver()
    U, S, A = unit_atan_set(), sincos_set(), atan2_set()
    one_u, _ = _run(torch_mod, hs, 7, U["s"], U["c"])
    one_a, _ = _run(torch_mod, hs, 3, A["y"], A["x"])
    one_s, one_c = _run(torch_mod, hs, 4, S["x"])
    differ, worst = {}, {}
    for N, op in WIDTH_OPS["unit_atan2"].items():
        for rot in range(N):
            got, _ = _rotated(torch_mod, hs, op, rot, U["s"], U["c"])
            worst[f"unit_atan2_n<{N}>"] = max(worst.get(f"unit_atan2_n<{N}>", 0.0), check_unit_atan2(got, f"unit_atan2_n<{N}> rotated by {rot}", say=False))
            differ[f"unit_atan2_n<{N}>+{rot}"] = int(np.abs(ibits(got) - ibits(one_u)).max())
    for N, op in WIDTH_OPS["fast_atan2"].items():
        for rot in range(N):
            got, _ = _rotated(torch_mod, hs, op, rot, A["y"], A["x"])
            worst[f"fast_atan2_n<{N}>"] = max(worst.get(f"fast_atan2_n<{N}>", 0.0), check_atan2(got, f"fast_atan2_n<{N}> rotated by {rot}", say=False))
            differ[f"fast_atan2_n<{N}>+{rot}"] = int(np.abs(ibits(got) - ibits(one_a)).max())
    for N, op in WIDTH_OPS["fast_sincos"].items():
        for rot in range(N):
            sn, cs = _rotated(torch_mod, hs, op, rot, S["x"])
            worst[f"fast_sincos_n<{N}>"] = max(worst.get(f"fast_sincos_n<{N}>", 0.0), check_sincos(sn, cs, f"fast_sincos_n<{N}> rotated by {rot}", say=False))
            differ[f"fast_sincos_n<{N}>+{rot}"] = max(int(np.abs(ibits(sn) - ibits(one_s)).max()), int(np.abs(ibits(cs) - ibits(one_c)).max()))
    print("max |error| over all slots:", {k: f"{v:.4e}" for k, v in worst.items()})
    print("ulp between a width's slots and width 1:", {k: v for k, v in differ.items() if v} or "none anywhere")
    assert not any(differ.values()), differ
    # a ragged last group: its padded slots are evaluated and not stored (the outputs' tails would show a write past n)
    for fn, args in (("unit_atan2", (U["s"][:5], U["c"][:5])), ("fast_atan2", (A["y"][:5], A["x"][:5])), ("fast_sincos", (S["x"][:5],))):
        for N, op in WIDTH_OPS[fn].items():
            for n in range(1, 6):
                o0, _ = _run(torch_mod, hs, op, *(v[:n] for v in args))
                full = {"unit_atan2": one_u, "fast_atan2": one_a, "fast_sincos": one_s}[fn]
                assert np.array_equal(ibits(o0), ibits(full[:n])), (fn, N, n)
