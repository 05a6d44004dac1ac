"""The operand classes of tests/field_ref.py hit the branches they were built
for, proved on the CPU through the model of the 29-bit product scanning, and
the model equals the big-integer reference on every class.  No GPU: the same
lists run byte-exact through the kernels in tests/test_field_probe.py."""
import math
import random

import field_ref as F

P = F.P


def _check_mul(a, b):
    r, pre, c = F.model_fp_mul(a, b)
    assert r == F.fp_mul(a, b) and pre == F.pre_fp_mul(a, b), (a, b)
    assert 0 <= pre < 2 * P and c.lo == 0 and c.hi < 1 << 64
    return pre, c


def _check_sqr(a0, a1):
    r, pre, c0, c1 = F.model_fp2_sqr(a0, a1)
    assert r == F.fp2_sqr((a0, a1)) and pre == F.pre_fp2_sqr(a0, a1), (a0, a1)
    assert -P < pre[0] < 2 * P and 0 <= pre[1] < 2 * P
    assert c1.lo == 0 and c1.hi < 1 << 64       # the unsigned lane
    return pre, c0, c1


def test_value_list():
    v = F.fp_values()
    top = (P >> 377) - 1
    want = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, F.RM % P, F.RM ** 2 % P,
            sum(F.M29 << (29 * i) for i in range(13)) + (top << 377)]
    want += [1 << k for k in range(381) if k % 29 == 0 or k % 32 == 0]
    want += [(1 << k) - 1 for k in range(381) if k % 29 == 0 or k % 32 == 0]
    want += [F.M29 << (29 * i) for i in range(13)] + [F.M32 << (32 * j) for j in range(11)]
    assert set(want) <= set(v) and all(0 <= x < P for x in v) and v == sorted(set(v))
    assert 36 <= len(v) <= 96, len(v)           # a few dozen: all pairs stay a small launch
    # both packing paths see set bits: a digit that spans three limbs' worth of
    # shift (s > 26) and the aligned one (s == 0), through the limbs and back
    for x in v:
        d = F.to29(x)
        assert sum(t << (29 * i) for i, t in enumerate(d)) == x
        assert F.from29(d, False) == x
    r = F.fr_values()
    assert {0, 1, F.RORD - 1, F.RORD - 2, F.FR_RM % F.RORD} <= set(r) and all(x < F.RORD for x in r)


def test_model_equals_reference_on_value_pairs():
    v = F.fp_values()
    hi = 0
    for a in v:
        for b in v:
            hi = max(hi, _check_mul(a, b)[1].hi)
            _check_sqr(a, b)
    assert hi < 1 << 63, "fp_mul column 2^%.3f" % math.log2(hi)


def test_final_subtraction_class_takes_it():
    """class (b): every case has a pre-reduction value of at least p"""
    mul, c1, c0 = F.final_sub_fp_mul(), F.final_sub_fp2_c1(), F.final_sub_fp2_c0()
    assert min(len(mul), len(c1), len(c0)) >= 16
    for a, b, t in mul:
        assert 0 <= a < P and 0 <= b < P
        assert _check_mul(a, b)[0] == t >= P
    for a0, a1, t in c1:
        assert 0 <= a0 < P and 0 <= a1 < P
        assert _check_sqr(a0, a1)[0][1] == t >= P
    for a0, a1, t in c0:
        assert 0 <= a0 < P and 0 <= a1 < P
        assert _check_sqr(a0, a1)[0][0] == t >= P
    ds = lambda cs: {t - P for _, _, t in cs}
    assert set(F.FINAL_SUB_D) <= ds(mul) & ds(c1) & ds(c0) and 0 in ds(c0)


def test_exactly_p_needs_a_sum_divisible_by_p():
    """why d = 0 is in the c0 list only: t = p means p divides the column sum"""
    for v in (0, P - 1, (P - 1) ** 2, 2 * (P - 1) * (P - 2)):
        assert F.pre_value(v) != P
    assert F.pre_value(P * 5) == P and F.pre_value(0) == 0


def test_random_operands_never_take_the_rare_branches():
    """the reason the crafted classes exist: 20,000 random pairs, none with a
    pre-reduction value >= p, none with a negative c0"""
    rng = random.Random(0xF1E1D)
    for i in range(20000):
        a, b = rng.randrange(P), rng.randrange(P)
        assert F.pre_fp_mul(a, b) < P
        p0, p1 = F.pre_fp2_sqr(a, b)
        assert 0 <= p0 < P and p1 < P
        if i % 100 == 0:
            _check_mul(a, b)
            _check_sqr(a, b)


def test_signed_lane_class():
    """class (c): a0 <= a1, c0 before the reduction in (-p, 0], with -1 and 0;
    every column of the signed lane below 2^63 in magnitude (fp2_redc's claim)"""
    cases = F.signed_lane_cases()
    mag = 0
    for a0, a1, t in cases[:-2]:
        assert 0 <= a0 <= a1 < P and -P < t <= 0
        pre, c0, _ = _check_sqr(a0, a1)
        assert pre[0] == t
        mag = max(mag, c0.mag)
    ts = [t for _, _, t in cases]
    assert -1 in ts and any(t == 0 and a0 == a1 for a0, a1, t in cases)
    assert sum(t < 0 for t in ts) >= 16 and min(ts) < -(1 << 320)
    uns = 0
    for a0, a1 in [c[:2] for c in cases[-2:]] + F.column_extremes():
        _, c0, c1 = _check_sqr(a0, a1)
        mag, uns = max(mag, c0.mag), max(uns, c1.hi)
    msg = "largest column: signed lane 2^%.3f, unsigned lane 2^%.3f" % (math.log2(mag), math.log2(uns))
    assert mag < 1 << 63 and uns < 1 << 63, msg
    # the figures DESIGN.md 6e records
    assert "signed lane 2^62.105, unsigned lane 2^62.889" in msg, msg


def test_fr_reference():
    r = F.RORD
    for a in F.fr_values():
        for b in F.fr_values():
            assert F.fr_mul(a, b) * F.FR_RM % r == a * b % r
        if a:
            assert F.fr_mul(F.fr_inv(a), a) == F.FR_RM % r
