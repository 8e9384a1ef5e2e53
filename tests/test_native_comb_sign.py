"""Sign-pattern comb tables read the signs of every window straight from the scalar image
(csrc/comb_sign.h).  tests/native/comb_sign_check.cpp prints, through the same function the digit
kernel calls, the signs C_0 .. C_253 and the parity e of edge and random scalars; built plain and with
-fsanitize=address,undefined, the two builds must print the same.  Checked here in Python integers:
sum_j (2 C_j - 1) 2^j = t | 1, e = 1 - (t & 1), and the constants that carry a scalar from one
Montgomery image to the other."""
import random

from tests import helpers as H
from tests import native_build

R = H.R


def _values():
    rng = random.Random(253)
    edge = [0, 1, 2, R - 1, R - 2, 1 << 253, (1 << 253) - 1, (1 << 32) - 1, 1 << 32,
            (1 << 64) - 1, 1 << 64, (1 << 224) + 1, (1 << 252) | (1 << 31)]
    return edge + [rng.randrange(R) for _ in range(40)]


@native_build.needs_gxx
def test_comb_sign_native(tmp_path):
    vals = _values()
    _, out, _ = native_build.run_both(native_build.build("comb_sign_check.cpp", tmp_path),
                                      ["%064x" % v for v in vals])
    lines = out.splitlines()
    assert lines[0] == "ok map"
    assert len(lines) == 1 + len(vals) + 2
    for t, line in zip(vals, lines[1:]):
        assert len(line) == 255 and set(line) <= {"0", "1"}, line
        c, e = [int(ch) for ch in line[:254]], int(line[254])
        assert sum((2 * cj - 1) << j for j, cj in enumerate(c)) == t | 1, hex(t)
        assert e == 1 - (t & 1), hex(t)
        assert t + e == t | 1
    for line, want in zip(lines[-2:], (("c256", pow(2, 256, R)), ("c266", pow(2, 266, R)))):
        name, *limbs = line.split()
        assert name == want[0]
        assert sum(int(v) << (29 * i) for i, v in enumerate(limbs)) == want[1]
        assert all(0 <= int(v) < 1 << 29 for v in limbs)


def test_scaled_bases_identity_in_integers():
    """sum_i s_i P_i = 2 H - W_254 - S over the bases P'' = P / (2 R'), with t the image s R' mod r
    read as an integer: the identity the native tables rest on, the bases taken as scalars."""
    rng = random.Random(254)
    for rprime in (1 << 256, 1 << 261):
        scale = pow(2 * rprime, R - 2, R)
        n = 7
        P = [rng.randrange(1, R) for _ in range(n)]
        s = [0, 1, 2, R - 1, R - 2] + [rng.randrange(R) for _ in range(n - 5)]
        Pq = [p * scale % R for p in P]
        t = [si * rprime % R for si in s]
        C = [((ti & ~1) + (1 << 254)) >> 1 for ti in t]
        e = [1 - (ti & 1) for ti in t]
        for ti, ci in zip(t, C):
            assert ci >> 253 == 1 and ci & ((1 << 253) - 1) == ti >> 1   # a shift, no carry
        Hsum = sum((1 << j) * sum((2 * ((C[i] >> j) & 1) - 1) * Pq[i] for i in range(n))
                   for j in range(254))
        W254 = sum((2 * e[i] - 1) * Pq[i] for i in range(n))
        assert (2 * Hsum - W254 - sum(Pq)) % R == sum(si * p for si, p in zip(s, P)) % R
