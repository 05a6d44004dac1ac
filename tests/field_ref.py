"""Reference for the BLS12-381 field units of hbbft_amd/csrc/pairing.hip, in
plain Python integers, and the operand classes that tests/test_field_cpu.py
(properties, no GPU) and tests/test_field_probe.py (byte-exact on the GPU,
through tests/hip/libfieldprobe.so) share.

Taken from the code under test: the Montgomery radices (2^406 for Fp, 2^256 for
Fr) and the moduli p and r, nothing else.  Operands are *raw* Montgomery-form
values: the probe converts nothing, so `fp_mul(a, b)` here is a b 2^-406 mod p
on the values as given.  Tower operations take the operands out of Montgomery
form, go through oracle/bls_oracle.py and put the result back.

The second half is a model of the 29-bit product scanning (fp_to29, fp_mul,
fp2_sqr_in with fp2_redc, fp_from29) on unbounded integers.  It returns what
the kernel cannot show: each output's value before the final reduction and the
largest column the accumulators hold.  The CPU tests use it to prove that a
crafted operand takes the branch it was built for.
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import bls_oracle as B  # noqa: E402

P = B.P
RORD = B.R                      # r: the modulus of Fr
RBITS = 406
RM = 1 << RBITS                 # Fp Montgomery radix
RM_INV = pow(RM, -1, P)
FR_RM = 1 << 256
FR_RM_INV = pow(FR_RM, -1, RORD)
NL, NR = 12, 8
M29 = (1 << 29) - 1
M32 = (1 << 32) - 1


def mont(v):
    return v * RM % P


def unmont(v):
    return v * RM_INV % P


def words(v, n):
    """n little-endian 32-bit words of v."""
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & M32 for i in range(n)]


def from_words(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


# ---------------------------------------------------------------- Fp, raw values
def fp_add(a, b):
    return (a + b) % P


def fp_sub(a, b):
    return (a - b) % P


def fp_neg(a, _b=None):
    return -a % P


def fp_dbl(a, _b=None):
    return 2 * a % P


def fp_mul(a, b):
    return a * b * RM_INV % P


def fp_sqr(a, _b=None):
    return a * a * RM_INV % P


def fp_inv(a):
    """mont(1 / unmont(a)); 0 for 0 (Fermat)."""
    return mont(pow(unmont(a), P - 2, P))


def fp_sqrt(a):
    """(mont(unmont(a)^((p-3)/4)), 1 iff unmont(a) is a square)."""
    v = unmont(a)
    t = pow(v, (P - 3) // 4, P)
    y = t * v % P
    return mont(t), int(y * y % P == v)


# ---------------------------------------------------------------- the tower, raw values
def _un2(a):
    return (unmont(a[0]), unmont(a[1]))


def _mo2(a):
    return (mont(a[0]), mont(a[1]))


def fp2_mul(a, b):
    return _mo2(B.f2mul(_un2(a), _un2(b)))


def fp2_sqr(a):
    return fp2_mul(a, a)


def fp2_inv(a):
    return _mo2(B.f2inv(_un2(a)))


def fp2_mul_xi(a):
    return _mo2(B.f2mul(_un2(a), B.XI))


def fp2_sqrt(a):
    """pairing.hip's norm method restated on plain values: (y, flag).  When the
    flag is 0 the y is still what the unit computes (it is deterministic)."""
    a0, a1 = _un2(a)
    e = (P - 3) // 4
    half = pow(2, -1, P)
    n = (a0 * a0 + a1 * a1) % P
    d = pow(n, e, P) * n % P
    delta = (a0 + d) * half % P
    if delta == 0:
        delta = a0
    t = pow(delta, e, P)
    x0 = t * delta % P
    x1 = a1 * t * half % P
    y = (x0, x1) if x0 * x0 % P == delta else (-x1 % P, x0)
    return _mo2(y), int(B.f2eq(B.f2mul(y, y), (a0, a1)))


def _un_t(t):
    """tower coefficients (a flat list of Fp2 pairs) out of Montgomery form"""
    return [_un2(c) for c in t]


def _mo_t(t):
    return [_mo2(c) for c in t]


def fp12_mul(a, b):
    """a, b: six Fp2 pairs each, in the tower order c0.c0 c0.c1 c0.c2 c1.c0 c1.c1 c1.c2"""
    return _mo_t(B.to_tower(B.f12mul(B.from_tower(_un_t(a)), B.from_tower(_un_t(b)))))


def fp12_sqr(a):
    return fp12_mul(a, a)


def fp6_mul(a, b):
    """Fp6 is the w^0 half of the tower: (a + 0 w)(b + 0 w) = a b"""
    z = [(0, 0)] * 3
    r = fp12_mul(list(a) + z, list(b) + z)
    assert r[3:] == z
    return r[:3]


def fp12_mul_by_014(f, c0, c1, c4):
    """f (c0 + c1 v + c4 v w)"""
    z = (0, 0)
    return fp12_mul(f, [c0, c1, z, z, c4, z])


def fp12_frob(a, k):
    return _mo_t(B.to_tower(B.f12frob(B.from_tower(_un_t(a)), k)))


def fp12_inv(a):
    return _mo_t(B.to_tower(B.f12inv(B.from_tower(_un_t(a)))))


def _f2dbl(a):
    return B.f2add(a, a)


def _fp4_sqr(a, b):
    t0, t1 = B.f2mul(a, a), B.f2mul(b, b)
    s = B.f2add(a, b)
    return B.f2add(B.f2mul(t1, B.XI), t0), B.f2sub(B.f2sub(B.f2mul(s, s), t0), t1)


def fp12_cyclo_sqr(f):
    """Granger-Scott's formula restated: an identity of the coefficients, so it
    is defined (and compared) on every input, not only on the subgroup."""
    z0, z4, z3, z2, z1, z5 = _un_t(f)
    t0, t1 = _fp4_sqr(z0, z1)
    z0 = B.f2add(_f2dbl(B.f2sub(t0, z0)), t0)
    z1 = B.f2add(_f2dbl(B.f2add(t1, z1)), t1)
    t0, t1 = _fp4_sqr(z2, z3)
    t2, t3 = _fp4_sqr(z4, z5)
    z4 = B.f2add(_f2dbl(B.f2sub(t0, z4)), t0)
    z5 = B.f2add(_f2dbl(B.f2add(t1, z5)), t1)
    t0 = B.f2mul(t3, B.XI)
    z2 = B.f2add(_f2dbl(B.f2add(t0, z2)), t0)
    z3 = B.f2add(_f2dbl(B.f2sub(t2, z3)), t2)
    return _mo_t([z0, z4, z3, z2, z1, z5])


def cyclotomic(f):
    """f^((p^6 - 1)(p^2 + 1)) of a raw tower value: in the cyclotomic subgroup"""
    a = B.from_tower(_un_t(f))
    e = B.f12mul(B.f12conj(a), B.f12inv(a))
    e = B.f12mul(B.f12frob(e, 2), e)
    return _mo_t(B.to_tower(e))


# ---------------------------------------------------------------- Fr, raw values
def fr_add(a, b):
    return (a + b) % RORD


def fr_sub(a, b):
    return (a - b) % RORD


def fr_mul(a, b):
    return a * b * FR_RM_INV % RORD


def fr_inv(a):
    return pow(a * FR_RM_INV % RORD, RORD - 2, RORD) * FR_RM % RORD


# ---------------------------------------------------------------- pre-reduction values, closed form
def pre_value(v):
    """(v + m p) / 2^406 for the m in [0, 2^406) that makes it whole: the value a
    Montgomery reduction of the (signed) column sum v holds before its final
    subtraction or addition of p"""
    m = -v * pow(P, -1, RM) % RM
    q, rem = divmod(v + m * P, RM)
    assert rem == 0
    return q


def pre_fp_mul(a, b):
    return pre_value(a * b)


def pre_fp2_sqr(a0, a1):
    return pre_value((a0 + a1) * (a0 - a1)), pre_value(2 * a0 * a1)


# ---------------------------------------------------------------- the 29-bit model
P29 = [(P >> (29 * i)) & M29 for i in range(14)]
PINV29 = -pow(P, -1, 1 << 29) % (1 << 29)


class Cols:
    """the extremes of every value an accumulator holds"""

    def __init__(self):
        self.lo = self.hi = 0

    def see(self, v):
        if v < self.lo:
            self.lo = v
        if v > self.hi:
            self.hi = v
        return v

    @property
    def mag(self):
        return max(self.hi, -self.lo)


def to29(v):
    """fp_to29 through the 12 limbs: digit i = bits 29 i .. 29 i + 28, read from
    limb q and the one above (alignbit), limb 12 read as zero"""
    w = words(v, NL)
    o = []
    for i in range(14):
        q, s = (29 * i) >> 5, (29 * i) & 31
        lo, hi = w[q], (w[q + 1] if q + 1 < NL else 0)
        o.append((((hi << 32 | lo) >> s) & M32 if s else lo) & M29)
    return o


def from29(o, neg):
    """fp_from29: 14 digits (the top one a 32-bit two's complement word) to 12
    limbs, p added (mod 2^384) when `neg`, then one conditional subtraction"""
    t = []
    for j in range(NL):
        i, s = (32 * j) // 29, (32 * j) % 29
        v = o[i] >> s
        if i + 1 < 14:
            v |= o[i + 1] << (29 - s)
        if s > 26 and i + 2 < 14:
            v |= o[i + 2] << (58 - s)
        t.append(v & M32)
    x = from_words(t)
    if neg:
        x = (x + P) % (1 << 384)
    return x - P if x >= P else x


def model_fp_mul(a, b):
    """fp_mul digit by digit: (result, value before the final subtraction, Cols)"""
    x, y, m, o, c = to29(a), to29(b), [0] * 14, [0] * 14, Cols()
    acc = 0
    for k in range(27):
        lo, hi = max(0, k - 13), min(k, 13)
        e = [acc, 0]
        q = 0
        for i in range(lo, hi + 1):
            e[q % 2] = c.see(e[q % 2] + x[i] * y[k - i])
            q += 1
        for i in range(lo, hi + 1 if k >= 14 else k):
            e[q % 2] = c.see(e[q % 2] + m[i] * P29[k - i])
            q += 1
        acc = c.see(e[0] + e[1])
        if k < 14:
            m[k] = ((acc & M32) * PINV29) & M29
            acc = c.see(acc + m[k] * P29[0])
            assert acc & M29 == 0
        else:
            o[k - 14] = acc & M29
        acc >>= 29
    o[13] = acc & M32
    assert acc < 32
    pre = sum(d << (29 * i) for i, d in enumerate(o))
    return from29(o, False), pre, c


def model_fp2_sqr(a0, a1):
    """fp2_sqr_in with fp2_redc: ((c0, c1), (pre0, pre1), Cols of the signed
    lane, Cols of the unsigned lane)"""
    x0, x1 = to29(a0), to29(a1)
    s = [u + v for u, v in zip(x0, x1)]
    d = [u - v for u, v in zip(x0, x1)]
    t2 = [v << 1 for v in x1]
    m0, m1, o0, o1 = [0] * 14, [0] * 14, [0] * 14, [0] * 14
    c0, c1 = Cols(), Cols()
    A0 = A1 = 0
    for k in range(27):
        lo, hi = max(0, k - 13), min(k, 13)
        q0 = q1 = 0
        for i in range(lo, hi + 1):
            q0 = c0.see(q0 + s[i] * d[k - i])
            q1 = c1.see(q1 + x0[i] * t2[k - i])
        e0, e1 = c0.see(A0 + q0), c1.see(A1 + q1)
        for i in range(lo, min(k, 14)):
            e0 = c0.see(e0 + m0[i] * P29[k - i])
            e1 = c1.see(e1 + m1[i] * P29[k - i])
        if k < 14:
            m0[k] = ((e0 & M32) * PINV29) & M29
            m1[k] = ((e1 & M32) * PINV29) & M29
            e0 = c0.see(e0 + m0[k] * P29[0])
            e1 = c1.see(e1 + m1[k] * P29[0])
            assert e0 & M29 == 0 and e1 & M29 == 0
        else:
            o0[k - 14], o1[k - 14] = e0 & M29, e1 & M29
        A0, A1 = e0 >> 29, e1 >> 29     # Python's >> on a negative int is arithmetic
    assert -(1 << 31) <= A0 < 1 << 31 and 0 <= A1 < 32
    pre0 = sum(v << (29 * i) for i, v in enumerate(o0[:13])) + (A0 << (29 * 13))
    pre1 = sum(v << (29 * i) for i, v in enumerate(o1[:13])) + (A1 << (29 * 13))
    o0[13], o1[13] = A0 & M32, A1 & M32
    neg = o0[13] >> 31 == 1
    return (from29(o0, neg), from29(o1, False)), (pre0, pre1), c0, c1


# ---------------------------------------------------------------- operand classes
def _digits(ds):
    return sum(d << (29 * i) for i, d in enumerate(ds))


def fp_values():
    """class (a): the value list (raw representations), a few dozen, sorted"""
    top = (P >> (29 * 13)) - 1          # the largest top digit with 13 full digits below p
    full = _digits([M29] * 13 + [top])
    alt0 = _digits([M29 if i % 2 == 0 else 0 for i in range(13)] + [top])
    alt1 = _digits([M29 if i % 2 == 1 else 0 for i in range(13)] + [top])
    assert full < P and _digits([M29] * 13 + [top + 1]) >= P
    v = {0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, RM % P, RM * RM % P, full, alt0, alt1}
    for k in range(0, 381):
        if k % 29 == 0 or k % 32 == 0:
            v |= {1 << k, (1 << k) - 1}
    for i in range(14):                 # one full 29-bit digit
        v.add((P >> 377) << 377 if i == 13 else M29 << (29 * i))
    for j in range(NL):                 # one full 32-bit limb
        v.add(M32 << (32 * j) if j < NL - 1 else (P >> 352) << 352)
    v = sorted(x for x in v if 0 <= x < P)
    return v


def _solve(t, a, parity=None):
    """b in [0, p) with a b + m p = t 2^406 for an m in [0, 2^406), or None.
    t < 0 asks for a b - m p = |t| 2^406, the negative pre-reduction value of
    the signed lane (a b is then the magnitude of the negative column sum)."""
    m0 = t * RM * pow(P, -1, a) % a         # m = m0 + j a, j >= 0
    if t >= 0:
        b0, rem = divmod(t * RM - m0 * P, a)    # b = b0 - j p
        j = b0 // P
    else:
        b0, rem = divmod(-t * RM + m0 * P, a)   # a b = |t| R + m p: b = b0 + j p
        j = 0
    assert rem == 0
    b, m = b0 - j * P if t >= 0 else b0, m0 + j * a
    if not (0 <= b < P and j >= 0 and m < RM):
        return None
    if parity is not None and b % 2 != parity:
        return None
    return b


# d = 0 (a pre-reduction value of exactly p) exists only for fp2_sqr's c0: the
# value is congruent to the column sum times 2^-406, so it is p only when p
# divides the sum; a b and 2 a0 a1 with factors in [1, p) never are, and a zero
# factor gives 0, not p.  (a0 + a1)(a0 - a1) is, with a0 + a1 = p.
FINAL_SUB_D = [1, 2, 1 << 32, (1 << 64) - 1]


def _ds(rng, n):
    out = list(FINAL_SUB_D)
    while len(out) < n:
        out.append(rng.randrange(1 << rng.randrange(65, 300)))
    return out


def final_sub_fp_mul(n=24, seed=0xB1):
    """class (b) for fp_mul: (a, b, t) with pre-reduction value t = p + d"""
    rng = random.Random(seed)
    out = []
    for d in _ds(rng, n):
        for _ in range(1000):    # a case that cannot be built fails, never spins
            a = P - 1 - rng.randrange(1 << 64)
            b = _solve(P + d, a)
            if b is not None:
                out.append((a, b, P + d))
                break
        else:
            raise AssertionError("no operands for d = %d" % d)
    return out


def final_sub_fp2_c1(n=24, seed=0xB2):
    """class (b) for fp2_sqr's c1 = 2 a0 a1: (a0, a1, t)"""
    rng = random.Random(seed)
    out = []
    for d in _ds(rng, n):
        for _ in range(1000):    # a case that cannot be built fails, never spins
            a0 = P - 1 - rng.randrange(1 << 64)
            a1 = _solve(P + d, 2 * a0)
            if a1 is not None:
                out.append((a0, a1, P + d))
                break
        else:
            raise AssertionError("no operands for d = %d" % d)
    return out


def _split(s, dd):
    """a0 + a1 = s, a0 - a1 = dd"""
    return (s + dd) // 2, (s - dd) // 2


def _signed_lane(t, rng):
    """(a0, a1) in [0, p) with c0's pre-reduction value exactly t (t != 0)"""
    for _ in range(1000):
        s = P - 1 - rng.randrange(1 << 64)
        dd = _solve(t, s, parity=s % 2)
        if dd is None or dd > s or s + dd >= 2 * P:
            continue
        hi, lo = _split(s, dd)
        return (hi, lo) if t > 0 else (lo, hi)
    raise AssertionError("no operands for t = %d" % t)


def final_sub_fp2_c0(n=24, seed=0xB3):
    """class (b) for fp2_sqr's c0 = (a0 + a1)(a0 - a1): (a0, a1, t)"""
    rng = random.Random(seed)
    out = [_split(P, dd) + (P,) for dd in (1, 3, P - 2)]     # a0 + a1 = p: exactly p
    return out + [_signed_lane(P + d, rng) + (P + d,) for d in _ds(rng, n - len(out))]


def signed_lane_cases(n=24, seed=0xC1):
    """class (c): (a0, a1, t) with a0 <= a1 and c0's pre-reduction value t in
    (-p, 0]: exactly -1, -2, ..., random, the deepest the lane reaches, and 0"""
    rng = random.Random(seed)
    out = []
    es = [1, 2, 3, 1 << 29, 1 << 32, (1 << 64) - 1, 1 << 300]
    while len(es) < n - 6:
        es.append(rng.randrange(1, 1 << rng.randrange(2, 350)))
    for e in es:
        out.append(_signed_lane(-e, rng) + (-e,))
    for a in (0, 1, P - 1, fp_values()[len(fp_values()) // 2]):     # a0 == a1: exactly 0
        out.append((a, a, 0))
    for a0, a1 in ((0, P - 1), (1, P - 1)):                         # the most negative sums
        out.append((a0, a1, pre_fp2_sqr(a0, a1)[0]))
    return out


def column_extremes(seed=0xC2, randoms=64):
    """class (c), the columns: model-found operand pairs with the most negative
    and the most positive column of the signed lane and the largest of the
    unsigned one, searched over digit patterns of 0 and 2^29 - 1 and a few
    random pairs.  Returns [(a0, a1)] (three pairs, maybe equal)."""
    rng = random.Random(seed)
    top = (P >> (29 * 13)) - 1
    pats = [[M29] * 13, [0] * 13,
            [M29 if i % 2 == 0 else 0 for i in range(13)],
            [M29 if i % 2 == 1 else 0 for i in range(13)],
            [M29] * 7 + [0] * 6, [0] * 6 + [M29] * 7]
    cand = [_digits(pt + [tp]) for pt in pats for tp in (0, top)]
    pairs = [(u, v) for u in cand for v in cand]
    pairs += [(rng.randrange(P), rng.randrange(P)) for _ in range(randoms)]
    best = {}
    for a0, a1 in pairs:
        _, _, c0, c1 = model_fp2_sqr(a0, a1)
        for key, val in (("neg", -c0.lo), ("pos", c0.hi), ("uns", c1.hi)):
            if key not in best or val > best[key][0]:
                best[key] = (val, (a0, a1))
    return [best[k][1] for k in ("neg", "pos", "uns")]


def fr_values():
    """class (e): the Fr value list"""
    v = {0, 1, RORD - 1, RORD - 2, FR_RM % RORD,
         (RORD >> 224) << 224,                       # the top limb at its maximum, zeros below
         ((RORD >> 224) << 224) | M32,
         (1 << 224) - 1,                             # all-ones low limbs
         (((RORD >> 224) - 1) << 224) | ((1 << 224) - 1),
         (1 << 32) - 1, (1 << 255) % RORD, 1 << 254}
    return sorted(x for x in v if 0 <= x < RORD)


def rand_fp(rng, n):
    return [rng.randrange(P) for _ in range(n)]


def rand_fr(rng, n):
    return [rng.randrange(RORD) for _ in range(n)]
