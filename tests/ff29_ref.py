"""Big-integer reference and operand sets for the 9 x 29-bit field forms (csrc/ff29.h and the
generated csrc/ff29_asm.h).  A helper module shared by tests/test_native_ff29.py (host build of
the C++ forms) and tests/test_gpu_primitives.py (zkmi_ff29_op: the asm and C++ forms on the GPU).

A Montgomery product is ONE integer, and the normalised limb form of an integer is unique, so the
reference scans no columns:  T = sum a*b over the limb VALUES as signed integers,
m = -T p^-1 mod 2^261,  v = (T + m p) / 2^261 (exact);  limbs 0..7 = (v >> 29 i) & MASK, limb 8 =
v >> 232 (signed).  For the image ops (pack_canonical) the reference is the value mod p as 8 x u32.

Every case is checked against the CONTRACT of its form before it is handed out (conditions on the
inputs, never on what the code under test returns):
  column bound  sum over the product terms of 9 max|a limb| max|b limb|, + 9 2^58 + 2^35 < 2^63
                (sqr: the doubled cross terms count, nine products per column as for mul), and
                |limb| < 2^29 for sqr / mul_add2, < 2^30 for mul;
  value bound   |sum a*b| < 64 p^2; the reference result then lies in (-p/2, 3p/2);
  wred          |value| < 2^7 p, |limb| < 2^31; with the float32 quotient |result| < 0.6 p;
  pack          normalised, value in (-p, 2p).
"""
import functools
import random

import numpy as np

MASK = (1 << 29) - 1
FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FQ = 21888242871839275222246405745257275088696311157297823662689037894645226208583
MOD = (FR, FQ)                       # field 0 = fr, 1 = fq (zkmi_ff29_op's numbering)
FIELDS = ("fr", "fq")
RBITS = 261
WAVE = 64

# op numbers of zkmi_ff29_op (include/zkmi.h)
OPS = ("mul_asm", "sqr_asm", "mul_add2_asm", "mul_asm_s", "mul", "sqr", "mul_add2", "mul_ilp",
       "wred_pack", "pack")
ARITY = (2, 1, 4, 2, 2, 1, 4, 2, 1, 1)
MUL_ASM_S, WRED_PACK, PACK = 3, 8, 9
# the C++ form with the same result (what the host program runs for an asm form)
KIND = ("mul", "sqr", "mul_add2", "mul_s", "mul", "sqr", "mul_add2", "mul", "wred_pack", "pack")


def limbs(v):
    """the normalised form of an integer"""
    return tuple((v >> (29 * i)) & MASK for i in range(8)) + (v >> 232,)


def value(a):
    return sum(int(x) << (29 * i) for i, x in enumerate(a))


def add_l(a, b):
    return tuple(x + y for x, y in zip(a, b))


def sub_l(a, b):
    return tuple(x - y for x, y in zip(a, b))


def neg_l(a):
    return tuple(-x for x in a)


def maxabs(a):
    return max(abs(int(x)) for x in a)


def mont(p, terms):
    """(sum a*b) / 2^261 as ff29.h's mul / sqr / mul_add2 define it; terms: [(a limbs, b limbs)]"""
    t = sum(value(a) * value(b) for a, b in terms)
    m = (-t * pow(p, -1, 1 << RBITS)) % (1 << RBITS)
    v, rem = divmod(t + m * p, 1 << RBITS)
    assert rem == 0
    assert -p < 2 * v < 3 * p, "reference result outside (-p/2, 3p/2)"
    if t % p == 0:
        assert v in (0, p)       # what is_zero_mulout relies on
    return limbs(v)


def _words(v):
    return tuple((v >> (32 * i)) & 0xffffffff for i in range(8)) + (0,)


def _terms(kind, c):
    if kind == "sqr":
        return [(c[0], c[0])]
    if kind == "mul_add2":
        return [(c[0], c[1]), (c[2], c[3])]
    return [(c[0], c[1])]


def check_contract(field, op, c):
    """Asserts that case c (a tuple of ARITY[op] limb tuples, for mul_asm_s with the b operand the
    form really uses) is inside the contract of the form."""
    p, kind = MOD[field], KIND[op]
    for a in c:
        assert len(a) == 9
    if kind == "wred_pack":
        a = c[0]
        assert maxabs(a) < 1 << 31 and abs(value(a)) < p << 7
        # the quotient as wred() estimates it: float32 division of the normalised top limb
        top = value(a) >> 232
        q = int(np.rint(np.float32(top) / (np.float32(p >> 232) + np.float32(0.5))))
        assert 10 * abs(value(a) - q * p) < 6 * p, "wred result outside 0.6 p"
        return
    if kind == "pack":
        a = c[0]
        assert all(0 <= x <= MASK for x in a[:8]) and -p < value(a) < 2 * p
        return
    terms = _terms(kind, c)
    col = sum(9 * maxabs(a) * maxabs(b) for a, b in terms) + 9 * (1 << 58) + (1 << 35)
    assert col < 1 << 63, "column bound"
    lim = 1 << 30 if kind in ("mul", "mul_s") else 1 << 29
    assert all(maxabs(a) < lim for a in c), "limb bound"
    assert abs(sum(value(a) * value(b) for a, b in terms)) < 64 * p * p, "value bound"


def reference(field, op, c):
    p, kind = MOD[field], KIND[op]
    check_contract(field, op, c)
    if kind in ("wred_pack", "pack"):
        return _words(value(c[0]) % p)
    return mont(p, _terms(kind, c))


# ---- operand pools ---------------------------------------------------------------------------------
def _norm_in(rnd, lo, hi):
    return limbs(rnd.randrange(lo, hi))


def _edges(p):
    """canonical images at their edges (and p itself)"""
    r = 1 << RBITS
    vals = [0, 1, 2, p - 2, p - 1, p, (1 << 252) - 1, 1 << 252, (1 << 252) + 1, r % p,
            (1 << 256) % p, (1 << 266) % p, MASK, 1 << 29, (1 << 232) - 1, 1 << 232]
    return [limbs(v) for v in vals]


def _canon(p, rnd, n):
    return ([_norm_in(rnd, 1 << 252, p) for _ in range(n // 2)] +
            [_norm_in(rnd, 0, p) for _ in range(n - n // 2)])


def _mulout(p, rnd):
    """a normalised value in the range of a product, (-p/2, 3p/2)"""
    return _norm_in(rnd, -(p // 2) + 1, 3 * p // 2)


def _diffs(p, rnd, n):
    """differences of two normalised values, |limb| < 2^29, value out to +-6.5 p (madd29's p, r)"""
    out = []
    for i in range(n):
        d = sub_l(_mulout(p, rnd), _norm_in(rnd, -5 * p + 1, 5 * p))
        out.append(d if i % 2 else neg_l(d))
    return out


def _lazy(p, rnd, n):
    """sums with |limb| < 2^30: the butterfly's x[i1] after one stage, msqr of Fq2"""
    out = []
    for i in range(n):
        if i % 3 == 0:
            out.append(add_l(_mulout(p, rnd), _mulout(p, rnd)))
        elif i % 3 == 1:
            a = _norm_in(rnd, 0, p)
            out.append(add_l(a, a))
        else:
            out.append(add_l(sub_l(_mulout(p, rnd), _norm_in(rnd, -9 * p // 2, 9 * p // 2)),
                             _mulout(p, rnd)))
    return out


def _negs(p, rnd, n):
    """all limbs non-positive: neg(y) of a normalised y >= 0"""
    return ([neg_l(limbs(v)) for v in (1, p - 1, p, (1 << 232) - 1, 2 * p - 1)] +
            [neg_l(_norm_in(rnd, 0, 2 * p)) for _ in range(n - 5)])


def _extremes(p, width, tenths):
    """limbs 0..7 all +m, all -m or alternating (m = 2^width - 1); top limb at both ends of
    |value| < tenths/10 p, and at 0, +-p8"""
    m = (1 << width) - 1
    bound = tenths * p // 10
    out = []
    for low in ((m,) * 8, (-m,) * 8, (m, -m) * 4, (-m, m) * 4):
        lv = value(low + (0,))
        t_max = (bound - 1 - lv) >> 232
        t_min = -((bound - 1 + lv) >> 232)
        for t in (t_max, t_min, 0, p >> 232, -(p >> 232)):
            a = low + (t,)
            assert abs(value(a)) < bound
            out.append(a)
    return out


def _zeros(p, rnd, n):
    """operands whose value is 0 mod p, |limb| < 2^29"""
    out = [(0,) * 9, limbs(p), sub_l(limbs(p), limbs(p)), neg_l(limbs(p)), limbs(2 * p),
           limbs(-p), limbs(-2 * p)]
    while len(out) < n:
        x = _norm_in(rnd, 0, p)
        out.append(sub_l(x, x))
        out.append(sub_l(limbs(value(x) + p), x))          # p as a difference with borrows
        out.append(sub_l(x, limbs(value(x) + 3 * p)))      # -3p
    return out[:n]


def _lazy_zeros(p, rnd, n):
    """value 0 with limbs in {0, 1, -2^29, 1 - 2^29}: (x + y) - x - y, a lazy operand of mul"""
    out = []
    while len(out) < n:
        x, y = _norm_in(rnd, 0, p), _norm_in(rnd, 0, p)
        out.append(sub_l(sub_l(limbs(value(x) + value(y)), x), y))
        assert value(out[-1]) == 0
    return out


def _fits(p, terms):
    return abs(sum(value(a) * value(b) for a, b in terms)) < 64 * p * p


def _pairs(p, A, B, n, step=7):
    """n pairs (A[i], a B that keeps the value bound), walking B with a fixed stride"""
    out, j = [], 0
    for i in range(n):
        a = A[i % len(A)]
        for _ in range(len(B)):
            b = B[j % len(B)]
            j += step
            if _fits(p, [(a, b)]):
                out.append((a, b))
                break
        else:
            raise AssertionError("no partner inside the value bound")
    return out


def _negative_results(p, rnd, n, make):
    """cases whose reference result has a negative top limb"""
    out = []
    for _ in range(40 * n):
        c = make()
        if mont(p, _terms("mul_add2" if len(c) == 4 else "mul", c))[8] < 0:
            out.append(c)
            if len(out) == n:
                return out
    raise AssertionError("too few negative results")


def _mul_classes(field):
    p, rnd = MOD[field], random.Random(2900 + field)
    edges, canon, diffs = _edges(p), _canon(p, rnd, 60), _diffs(p, rnd, 120)
    lazy, negs = _lazy(p, rnd, 60), _negs(p, rnd, 40)
    e29, e30 = _extremes(p, 29, 80), _extremes(p, 30, 80)
    zeros, lz = _zeros(p, rnd, 25), _lazy_zeros(p, rnd, 10)
    small = edges + canon + negs
    cls = []
    cls.append(("canonical", [(a, b) for a in edges for b in edges] +
                _pairs(p, canon, canon[::-1], 37)))
    cls.append(("difference", _pairs(p, diffs, diffs[::-1], 100) + _pairs(p, diffs, canon, 25) +
                _pairs(p, canon, diffs, 25)))
    cls.append(("lazy", _pairs(p, lazy, canon, 40) + _pairs(p, canon, lazy, 40) +
                _pairs(p, lazy, diffs, 40) + _pairs(p, diffs, lazy, 40)))
    cls.append(("non-positive", _pairs(p, negs, canon, 33) + _pairs(p, canon, negs, 33) +
                _pairs(p, negs, negs[::-1], 33)))
    cls.append(("limb-extremes", [(a, b) for a in e29 for b in e29] +
                [(a, b) for a in e30[::2] for b in e29[::2]] +
                [(b, a) for a in e30[1::2] for b in e29[1::2]] +
                _pairs(p, e30, diffs, 45)))
    cls.append(("zero-products", _pairs(p, zeros, small + diffs + e29, 75) +
                _pairs(p, small + diffs + e29, zeros, 75) +
                _pairs(p, lz, small + diffs, 20) + _pairs(p, small + diffs, lz, 20)))

    def neg_case():
        a = _norm_in(rnd, 6 * p, 8 * p)
        b = sub_l(_mulout(p, rnd), _norm_in(rnd, 6 * p, 13 * p // 2))
        c = (a, b) if rnd.random() < 0.5 else (neg_l(b), neg_l(a))
        return c if _fits(p, [c]) else (limbs(1), neg_l(limbs(1)))
    cls.append(("negative-result", _negative_results(p, rnd, 70, neg_case)))
    cls.append(("single", [(limbs(p - 1), limbs(p - 1))]))
    return cls


def _mul_s_classes(field):
    """mul_asm_s: element i uses the b operand of element 64 * (i // 64).  Every class of the mul
    set, regrouped: each wave gets one b of the class as its leader's operand, the other lanes
    carry a b of their own that the form must NOT use."""
    p, rnd = MOD[field], random.Random(2950 + field)
    cls = []
    for name, pairs in _mul_classes(field):
        if len(pairs) == 1:
            cls.append((name, pairs))
            continue
        seen, bs = set(), []
        for _, b in pairs:
            if b not in seen:
                seen.add(b)
                bs.append(b)
        bs = bs[::max(1, len(bs) // 10)][:10]
        out = []
        for g, b in enumerate(bs):
            size = WAVE if g + 1 < len(bs) else 37       # a ragged last wave
            ok = [a for a, _ in pairs if _fits(p, [(a, b)]) and
                  9 * maxabs(a) * maxabs(b) + 9 * (1 << 58) + (1 << 35) < 1 << 63]
            assert ok
            rnd.shuffle(ok)
            for j in range(size):
                decoy = pairs[(g * WAVE + j) % len(pairs)][1]
                out.append((ok[j % len(ok)], b if j == 0 else decoy))
        cls.append((name, out))
    return cls


def _sqr_classes(field):
    p, rnd = MOD[field], random.Random(2960 + field)
    return [("canonical", _edges(p) + _canon(p, rnd, 53)),
            ("difference", _diffs(p, rnd, 130)),
            ("non-positive", _negs(p, rnd, 65)),
            ("limb-extremes", _extremes(p, 29, 80)),
            ("zero-products", _zeros(p, rnd, 67)),
            ("single", [limbs(p - 1)])]


def _mul_add2_classes(field):
    p, rnd = MOD[field], random.Random(2970 + field)
    edges, canon = _edges(p), _canon(p, rnd, 40)
    e56, e80 = _extremes(p, 29, 56), _extremes(p, 29, 80)
    cls = []
    # ec29.h madd29: y3 = r (q - x3) - y1 ppp
    y3 = []
    for _ in range(130):
        r = sub_l(_mulout(p, rnd), _norm_in(rnd, -2 * p + 1, 2 * p))
        qx3 = sub_l(_mulout(p, rnd), _norm_in(rnd, -5 * p + 1, 3 * p))
        y3.append((r, qx3, neg_l(_norm_in(rnd, -2 * p + 1, 2 * p)), _mulout(p, rnd)))
    cls.append(("madd-y3", y3))

    # the Fq2 product: (a0 b0 - a1 b1, a0 b1 + a1 b0) on canonical table entries, weakly reduced
    # accumulator components (|c| < 0.6 p) and differences of the two
    def comp(i):
        if i % 3 == 0:
            return _norm_in(rnd, 0, p)
        if i % 3 == 1:
            return _norm_in(rnd, -6 * p // 10, 6 * p // 10)
        return sub_l(_norm_in(rnd, 0, p), _norm_in(rnd, -6 * p // 10, 6 * p // 10))
    fq2 = []
    for i in range(65):
        a0, a1, b0, b1 = comp(i), comp(i + 1), comp(i + 2), comp(2 * i)
        fq2 += [(a0, b0, neg_l(a1), b1), (a0, b1, a1, b0)]
    cls.append(("fq2-product", fq2))
    cls.append(("canonical", [(a, b, edges[(i + 3 * j) % 16], edges[(5 * i + j + 1) % 16])
                              for i, a in enumerate(edges) for j, b in enumerate(edges)] +
                [tuple(canon[(4 * i + k) % 40] for k in range(4)) for i in range(3)]))
    ext = [(e56[i % 20], e56[(i // 20 + i) % 20], e56[(7 * i + 3) % 20], e56[(11 * i + 5) % 20])
           for i in range(200)]
    ext += [(e80[i % 20], canon[i % 40], canon[(i + 1) % 40], e80[(3 * i + 1) % 20])
            for i in range(61)]
    cls.append(("limb-extremes", ext))
    cls.append(("non-positive", [tuple(neg_l(_norm_in(rnd, 0, 2 * p)) for _ in range(4))
                                 for _ in range(65)]))
    zero = [((0,) * 9, canon[0], (0,) * 9, canon[1]), (limbs(p), canon[2], canon[3], (0,) * 9)]
    for i in range(33):
        x, y = _diffs(p, rnd, 1)[0], _mulout(p, rnd)
        zero.append((x, y, neg_l(x), y))                              # T = 0
        x = _norm_in(rnd, -2 * p, 2 * p)
        zero.append((x, y, x, sub_l(limbs(p), y)))                    # T = x p
    cls.append(("zero-products", zero))

    def neg_case():
        a, c = _norm_in(rnd, 5 * p, 56 * p // 10), _norm_in(rnd, 5 * p, 56 * p // 10)
        b, d = neg_l(_norm_in(rnd, 5 * p, 56 * p // 10)), neg_l(_norm_in(rnd, 5 * p, 56 * p // 10))
        return (a, b, d, c)
    cls.append(("negative-result", _negative_results(p, rnd, 70, neg_case)))
    cls.append(("single", [(limbs(p - 1), limbs(p - 1), limbs(p - 1), limbs(p - 1))]))
    return cls


def _with_top(low, v8):
    """raw limbs `low` (0..7) with the top limb that makes the NORMALISED top limb v8"""
    return low + (v8 - (value(low + (0,)) >> 232),)


def _wred_classes(field):
    p, rnd = MOD[field], random.Random(2980 + field)
    m31, p8 = (1 << 31) - 1, p >> 232
    wide = []
    for _ in range(200):
        low = tuple(rnd.randint(-m31, m31) for _ in range(8))
        wide.append(_with_top(low, rnd.randint(-126 * p8, 126 * p8)))
    # what the kernels feed it: sums and differences of up to four normalised values
    sums = []
    for _ in range(100):
        a = _mulout(p, rnd)
        for k in range(rnd.randint(1, 3)):
            b = _mulout(p, rnd)
            a = add_l(a, b) if rnd.random() < 0.5 else sub_l(a, b)
        sums.append(a)
    ext = []
    for low in ((m31,) * 8, (-m31,) * 8, (m31, -m31) * 4, (-m31, m31) * 4):
        for v8 in (126 * p8, -126 * p8, 0, 1, -1):
            ext.append(_with_top(low, v8))
    # the float quotient rounds at v8 = (k + 1/2)(p8 + 1/2): normalised and wide low limbs
    bnd = []
    for k in range(-127, 127):
        mid = ((2 * k + 1) * (2 * p8 + 1)) // 4
        for d in (-2, -1, 0, 1, 2):
            low = (tuple(rnd.randrange(1 << 29) for _ in range(8)) if (k + d) % 2 else
                   tuple(rnd.randint(-m31, m31) for _ in range(8)))
            bnd.append(_with_top(low, mid + d))
    return [("random-wide", wide), ("kernel-sums", sums), ("limb-extremes", ext),
            ("rounding-boundaries", bnd), ("single", [limbs(p - 1)])]


def _pack_classes(field):
    p, rnd = MOD[field], random.Random(2990 + field)
    ends = [limbs(v) for v in (-p + 1, -p // 2, -2, -1, p + 1, 3 * p // 2, 2 * p - 2, 2 * p - 1,
                               -(1 << 232), -(1 << 232) - 1, p - (1 << 232))]
    return [("canonical", _edges(p) + _canon(p, rnd, 53)),
            ("product-range", ends + [_mulout(p, rnd) for _ in range(90)]),
            ("full-range", [_norm_in(rnd, -p + 1, 2 * p) for _ in range(130)]),
            ("single", [limbs(-1)])]


@functools.lru_cache(maxsize=None)
def vectors(field, op):
    """[(class name, operands int32 [n][arity][9], expected int32 [n][9])] of one field x op.
    Built once per process (fixed seeds) and shared; callers must not write to the arrays."""
    kind = KIND[op]
    classes = {"mul": _mul_classes, "mul_s": _mul_s_classes, "sqr": _sqr_classes,
               "mul_add2": _mul_add2_classes, "wred_pack": _wred_classes,
               "pack": _pack_classes}[kind](field)
    out = []
    for name, cases in classes:
        if ARITY[op] == 1:
            cases = [c if isinstance(c[0], tuple) else (c,) for c in cases]
        want = []
        for i, c in enumerate(cases):
            used = (c[0], cases[i - i % WAVE][1]) if kind == "mul_s" else c
            want.append(reference(field, op, used))
        ops = np.array(cases, dtype=np.int64)
        assert ops.shape == (len(cases), ARITY[op], 9) and np.abs(ops).max() < 1 << 31
        exp = np.array(want, dtype=np.int64)
        ops, exp = ops.astype(np.int32), exp.astype(np.uint32).view(np.int32)
        ops.setflags(write=False)
        exp.setflags(write=False)
        out.append((name, ops, exp))
    return out


def write_operand_file(path):
    """Every field x op x class as one record of int32: field, op, arity, n, then the operands --
    what tests/native/ff29_ops.cpp reads.  Returns the records in file order."""
    recs = []
    with open(path, "wb") as f:
        for field in (0, 1):
            for op in range(len(OPS)):
                for name, ops, exp in vectors(field, op):
                    np.array([field, op, ARITY[op], len(ops)], dtype=np.int32).tofile(f)
                    ops.tofile(f)
                    recs.append((field, op, name, exp))
    return recs
