"""What the tests of the gnark-shaped R1CS solve share (a plain module, no test in it): the dump that
tests/native/r1cs_plan_check.cpp reads and the OUT it writes, the program's two builds, and the
systems with their Python-integer references that the host tests and the GPU tests both solve."""
import types

import numpy as np
import pytest

from gnark_crypto_primitives_amd.frontend.api import OP_BAND, OP_BXOR
from gnark_crypto_primitives_amd.frontend.compile import Public, Secret, to_mont_array
from gnark_crypto_primitives_amd.std import emulated as em
from tests import helpers as H
from tests import native_build

(RK_ASSERT, RK_SOLVE_O, RK_SOLVE_L, RK_SOLVE_R, RK_INVZERO, RK_NBITS, RK_LIMBS, RK_BYTEOP,
 RK_COUNT_BEGIN, RK_COUNT_Q, RK_COUNT_END, RK_COMMIT, RK_EMUL_STEP, RK_EMUL_END) = range(14)
K_LIMBS, K_COUNT, K_COMMIT, K_BYTEOP, K_EMUL = 3, 4, 5, 6, 7
BASIC, STD, EMULATED = 0, 1, 3
POW2 = (1, 2, 4, 8, 16, 32, 64)
LANES_MSG = "r1cs solver: lanes_per_proof must be 0 (auto) or a power of two, 1 .. 64"


# ---- the check program: its builds, its dump, its answer ------------------------------------------

@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """(directory for the dumps, [plain, sanitized]): built once, whichever modules ask"""
    return native_build.build_once("r1cs_plan_check.cpp", tmp_path_factory)


def hint_list(cc):
    """[[kind, [expression = [(coefficient index, wire)]], [output wires]]] of a compiled circuit"""
    kinds, in_ptr, lc_ptr, hcol, hcid, out_ptr, outs = cc.hint_arrays
    res = []
    for h, kind in enumerate(kinds.tolist()):
        exprs = [[(int(hcid[t]), int(hcol[t])) for t in range(lc_ptr[e], lc_ptr[e + 1])]
                 for e in range(in_ptr[h], in_ptr[h + 1])]
        res.append([kind, exprs, outs[out_ptr[h]:out_ptr[h + 1]].tolist()])
    return res


def description(cc, inputs, hint_set=STD, hints=None, commit_values=()):
    """the arrays of the dump, by name, as the test may edit them"""
    hints = hint_list(cc) if hints is None else hints
    d = {"header": np.array([cc.n_wires, cc.n_public, cc.n_secret, cc.n_constraints, len(hints), hint_set]),
         "coeffs": to_mont_array(cc.consts).view(np.uint32).reshape(-1)}
    for name, (ptr, col, cid) in (("l", cc.L), ("r", cc.Rm), ("o", cc.O)):
        d[name + "_ptr"] = ptr.copy()
        d[name + "_terms"] = np.stack([cid, col], axis=1).reshape(-1)
    in_ptr, lc_ptr, terms, out_ptr, outs = [0], [0], [], [0], []
    for kind, exprs, ows in hints:
        for e in exprs:
            terms += [x for t in e for x in t]
            lc_ptr.append(len(terms) // 2)
        in_ptr.append(len(lc_ptr) - 1)
        outs += ows
        out_ptr.append(len(outs))
    d.update(instr=cc.instr.reshape(-1).copy(), hint_kind=np.array([h[0] for h in hints]),
             hint_in_ptr=np.array(in_ptr), hint_lc_ptr=np.array(lc_ptr), hint_terms=np.array(terms),
             hint_out_ptr=np.array(out_ptr), hint_out=np.array(outs),
             inputs=np.ascontiguousarray(inputs).view(np.uint32).reshape(-1),
             commit_values=np.ascontiguousarray(commit_values, dtype=np.uint64).view(np.uint32).reshape(-1))
    return d


def coefficient(d, value):
    """index of a coefficient with this value, appended to the description's table"""
    d["coeffs"] = np.concatenate([d["coeffs"], to_mont_array([value % H.R]).view(np.uint32).reshape(-1)])
    return d["coeffs"].size // 8 - 1


ORDER = ("header", "coeffs", "l_ptr", "l_terms", "r_ptr", "r_terms", "o_ptr", "o_terms", "instr",
         "hint_kind", "hint_in_ptr", "hint_lc_ptr", "hint_terms", "hint_out_ptr", "hint_out", "inputs",
         "commit_values")


def write_sections(path, dump, order):
    with open(path, "wb") as f:
        for name in order:
            a = np.ascontiguousarray(dump[name], dtype=np.uint32)
            f.write(np.uint32(a.size).tobytes())
            f.write(a.tobytes())


def lines_by_s(text, s_first, s_last):
    """the program's stdout, one line per S, without the "S=<s> " in front"""
    lines = {}
    for line in text.splitlines():
        head, rest = line.split(" ", 1)
        lines[int(head[2:])] = rest
    assert sorted(lines) == list(range(s_first, s_last + 1))
    return lines


def run(builds, desc, s_first, s_last, tag="case"):
    """(stdout lines by S, bytes of OUT) -- the same from both builds"""
    d, exes = builds
    src, dst = str(d / (tag + ".in")), str(d / (tag + ".out"))
    write_sections(src, desc, ORDER)
    _, text, blob = native_build.run_both(exes, [src, dst, str(s_first), str(s_last)], out_file=dst)
    return lines_by_s(text, s_first, s_last), blob


def parse(blob, n_wires, n_constraints):
    """[(S, ext, records [n + 1, 8], terms [m, 2], outs, commits [(instruction, record, wire, hashed,
    private)], n_coeffs, [(status, wires, a, b, c)])]"""
    w = np.frombuffer(blob, dtype=np.uint32)
    plans, o = [], 0

    def take(n):
        nonlocal o
        r = w[o:o + n]
        o += n
        return r
    while o < w.size:
        S, ext = (int(x) for x in take(2))
        recs = take(8 * int(take(1)[0])).reshape(-1, 8)
        terms = take(2 * int(take(1)[0])).reshape(-1, 2)
        outs = take(int(take(1)[0]))
        commits = []
        for _ in range(int(take(1)[0])):
            instr, rec, wire = (int(x) for x in take(3))
            hashed = take(int(take(1)[0])).tolist()
            commits.append((instr, rec, wire, hashed, take(int(take(1)[0])).tolist()))
        n_coeffs, batch = (int(x) for x in take(2))
        sol = []
        for _ in range(batch):
            st = int(take(1)[0].astype(np.int32))
            arrs = [take(8 * n).view(np.uint64).reshape(n, 4)
                    for n in (n_wires, n_constraints, n_constraints, n_constraints)]
            sol.append((st, *arrs))
        plans.append((S, ext, recs, terms, outs, commits, n_coeffs, sol))
    return plans


# ---- HintsPlain: the hints of ZKMI_HINTS_STD without a commitment ---------------------------------

class HintsPlain:
    """two limb hints, one lookup-multiplicity hint over 53 queries of one or two terms (l0 + 40 is
    never below 32: counted nowhere), two byte operations over two-term expressions, no commitment"""
    X = Public()
    Y = Secret()
    Z = Secret()

    def define(self, api):
        l = api.NewHintLimbs(self.Y, 5, 51)
        api.AssertIsEqual(api.Sum([api.Mul(v, 1 << (5 * i)) for i, v in enumerate(l)]), self.Y)
        m = api.NewHintLimbs(self.Z, 16, 16)
        q = list(l) + [api.Add(l[0], 40), api.Add(api.Mul(l[1], 3), l[2])]
        c = api.NewHintCount(q, 32)
        x = api.NewHintByteOp(OP_BXOR, api.Add(m[0], api.Mul(m[5], 1 << 16)),
                              api.Add(l[3], api.Mul(l[4], 256)))
        a = api.NewHintByteOp(OP_BAND, m[1], m[2])
        acc = api.Sum([api.Mul(v, i + 1) for i, v in enumerate(c)])
        api.AssertIsEqual(api.Add(acc, api.Mul(x, 1 << 20), api.Mul(a, 1 << 60), m[3]), self.X)


def limbs_of(v, width, count):
    return [(v >> (width * j)) & ((1 << width) - 1) if width * j < 256 else 0 for j in range(count)]


def hints_plain_x(y, z):
    """the X that satisfies HintsPlain for (Y, Z), with Python integers"""
    l, m = limbs_of(y, 5, 51), limbs_of(z, 16, 16)
    q = l + [l[0] + 40, 3 * l[1] + l[2]]
    c = [sum(1 for v in q if v == j) for j in range(32)]
    x = ((m[0] + (m[5] << 16)) & 0xffffffff) ^ ((l[3] + l[4] * 256) & 0xffffffff)
    a = m[1] & m[2]
    return (sum(v * (i + 1) for i, v in enumerate(c)) + (x << 20) + (a << 60) + m[3]) % H.R


def hints_plain_assignments(n, rng):
    """n assignments: lane 0 has Z = r - 1, lane 7 (if there) a wrong X"""
    asg = []
    for i in range(n):
        y, z = rng.randrange(1 << 253), H.R - 1 if i == 0 else rng.randrange(H.R)
        asg.append({"X": hints_plain_x(y, z), "Y": y, "Z": z})
    if n > 7:
        asg[7]["X"] = (asg[7]["X"] + 1) % H.R
    return asg


# ---- EmulDirect: the emulated product (kind 7) called directly ------------------------------------

M64 = (1 << 64) - 1
# (na, nb, nk) -> widths of the limbs of a and of b: a < 2^(64 (na - 1) + wa + 1) < 2^384, b alike, and
# a b / 2^224 < 2^(64 nk) for the smallest modulus
SHAPES = {(1, 1, 1): (100, 100), (4, 3, 4): (90, 66), (2, 4, 5): (100, 100), (4, 4, 8): (100, 100)}
MODULI = (em.Secp256k1Fp.modulus, em.BN254Fr.modulus, em.BN254Fp.modulus,
          1 << 224,           # three empty limb expressions, top 32-bit word 1
          (1 << 256) - 1)     # top word all ones: the division normalises by a shift of 0
CALLS = [(shape, p) for p in MODULI for shape in SHAPES]
IN_MAX = (1 << 63) - 1        # the inputs U, V stay below 2^63


def _limb_values(u, v, first, n, width):
    """limb i = U (2^(width - 64) - 1) + 3 V for even i (a two-term lazy sum), U (2^(width - 64) - 1)
    for odd i: below 2^width for U, V < 2^63"""
    k = (1 << (width - 64)) - 1
    return [u[first + i] * k + (3 * v[first + i] if i % 2 == 0 else 0) for i in range(n)]


def emul_outputs(al, bl, p, nk):
    """what the hint writes for these limb values, with Python integers: nk limbs of the quotient,
    four of the remainder, the carries as field elements; and (quotient, remainder)"""
    na, nb = len(al), len(bl)
    a = sum(x << (64 * i) for i, x in enumerate(al))
    b = sum(x << (64 * i) for i, x in enumerate(bl))
    assert a < 1 << 384 and b < 1 << 384
    k, r = divmod(a * b, p)
    assert k < 1 << (64 * nk)
    kl = [(k >> (64 * i)) & M64 for i in range(nk)]
    rl = [(r >> (64 * i)) & M64 for i in range(4)]
    pl = [(p >> (64 * i)) & M64 for i in range(4)]
    ncols = max(na + nb - 1, nk + 3)
    inv64 = pow(1 << 64, -1, H.R)
    carries, prev = [], 0
    for j in range(ncols - 1):
        t = prev + sum(al[i] * bl[j - i] for i in range(na) if 0 <= j - i < nb)
        t -= rl[j] if j < 4 else 0
        t -= sum(kl[i] * pl[j - i] for i in range(nk) if 0 <= j - i < 4)
        prev = t * inv64 % H.R
        carries.append(prev)
    return kl + rl + carries, (k, r)


class EmulDirect:
    """one NewHintEmulMul per (shape, modulus) of CALLS on limbs formed from the inputs U, V; every
    output of every hint is folded into the public X by a weighted sum.  No commitment, no range
    check: the test's inputs keep the operands inside the hint's contract."""
    X = Public()
    U = Secret(8)
    V = Secret(8)

    def define(self, api):
        outs = []
        for (na, nb, nk), p in CALLS:
            wa, wb = SHAPES[(na, nb, nk)]

            def limbs(first, n, width):
                k = (1 << (width - 64)) - 1
                return [api.Add(api.Mul(self.U[first + i], k), api.Mul(self.V[first + i], 3)) if i % 2 == 0
                        else api.Mul(self.U[first + i], k) for i in range(n)]
            k, r, c = api.NewHintEmulMul(limbs(0, na, wa), limbs(4, nb, wb), p, nk)
            outs += list(k) + list(r) + list(c)
        api.AssertIsEqual(api.Sum([api.Mul(v, n * n + 3 * n + 1) for n, v in enumerate(outs)]), self.X)


def emul_direct_model(u, v):
    """(X, [(quotient, remainder, a, b, p)] per call) for the inputs U, V"""
    outs, qr = [], []
    for (na, nb, nk), p in CALLS:
        wa, wb = SHAPES[(na, nb, nk)]
        al, bl = _limb_values(u, v, 0, na, wa), _limb_values(u, v, 4, nb, wb)
        o, (k, r) = emul_outputs(al, bl, p, nk)
        outs += o
        qr.append((k, r))
    return sum(x * (n * n + 3 * n + 1) for n, x in enumerate(outs)) % H.R, qr


def emul_direct_assignments(n, rng, bad=()):
    """n assignments: 1 all zero, 2 every input at its maximum, 4 U at its maximum and V zero, 5 small
    values, the others random; the lanes in `bad` get a wrong X"""
    asg = []
    for i in range(n):
        if i == 1:
            u, v = [0] * 8, [0] * 8
        elif i == 2:
            u, v = [IN_MAX] * 8, [IN_MAX] * 8
        elif i == 4:
            u, v = [IN_MAX] * 8, [0] * 8
        elif i == 5:
            u, v = [rng.randrange(1 << 10) for _ in range(8)], [rng.randrange(4) for _ in range(8)]
        else:
            u, v = [rng.randrange(IN_MAX + 1) for _ in range(8)], [rng.randrange(IN_MAX + 1) for _ in range(8)]
        x = emul_direct_model(u, v)[0]
        asg.append({"X": (x + 1) % H.R if i in bad else x, "U": u, "V": v})
    return asg


NO_KEYS = types.SimpleNamespace(commitment_keys=[])     # the oracle's solver without a commitment key
