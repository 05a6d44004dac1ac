"""Writes bls_consts.hpp: BLS12-381 base-field constants for pairing.hip, as
little-endian 32-bit limbs, field elements in Montgomery form (R = 2^406: the
product in pairing.hip runs 14 reduction rounds of 29-bit limbs, kP29 / kPinv29).

Run: python gen_bls_consts.py > bls_consts.hpp  (the output is committed; the
build does not run this).  The values follow from p, x and xi = u + 1 alone:
the Frobenius coefficients are xi^((p^k - 1)/3), xi^(2(p^k - 1)/3) (Fp6) and
xi^((p^k - 1)/6) (Fp12) for k = 1, 2, 3 -- the constants the `pairing` crate
tabulates as FROBENIUS_COEFF_FQ6_C1/C2 and FROBENIUS_COEFF_FQ12_C1.

Subgroup checks (pairing.hip g1_in_subgroup / g2_in_subgroup, the endomorphism
tests of Scott, ePrint 2021/1130 section 6 / 2022/352): beta is the cube root
of unity with phi(P) = (beta x, y) = -[x^2] P on G1, and psi(x, y) =
(conj(x) xi^-((p-1)/3), conj(y) xi^-((p-1)/2)) the untwist-Frobenius-twist
with psi(Q) = [x] Q on G2; oracle/bls_oracle.py checks both against the
crate's [r] P == O test.

Scalar field Fr (the decryption-share combine's Lagrange coefficients): the
group order r in 8 limbs, Montgomery form with R = 2^256 (a plain 32-bit-limb
product: Fr products are not a hot loop).

Threshold signatures (the G2 share check and combine): G1::one(), whose
negative is the constant G1 point of every check e(pk, H) == e(G1::one(), sig),
and gamma = N(xi^-((p-1)/3)) in Fp with psi^2(x, y) = (gamma x, -y) = [x^2] Q on
G2 (no sign flip, unlike phi on G1); main() asserts gamma against psi o psi.

Compressed encodings (decompress_g1 / decompress_g2): p = 3 mod 4, so for a
square a the power t = a^((p-3)/4) is 1/sqrt(a) and t a the root; kSqrtExp is
that exponent as plain limbs (fp_pow_sqrt walks it in 4-bit windows, top
window first, which main() asserts to be non-zero) and kHalf = 1/2, for the
(a0 + |a|)/2 of the square root in Fp2 by norms.

Key generation (g1_base_mul_check_kernel): the three operands of the GLV loop
for the fixed base G1::one() -- the generator, Q = [x^2] G1::one() and their
sum -- as affine constants.
"""
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
X_ABS = 0xd201000000010000
RM = 1 << 406   # 14 rounds of 29 bits (pairing.hip fp_mul)
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
RM_FR = 1 << 256   # 8 rounds of 32 bits (pairing.hip fr_mul)
# G1::one(), the standard generator (affine x, y)
G1_X = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
G1_Y = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1


# the cofactor of E'(Fp2) in the BLS parameter x = -X_ABS (hash_g2.hip)
H2, _H2_REM = divmod(X_ABS ** 8 + 4 * X_ABS ** 7 + 5 * X_ABS ** 6 - 4 * X_ABS ** 4
                     - 6 * X_ABS ** 3 - 4 * X_ABS ** 2 + 4 * X_ABS + 13, 9)
assert _H2_REM == 0 and H2 % 2 == 1

SQRT_EXP = (P - 3) // 4
SQRT_WINDOWS = (SQRT_EXP.bit_length() + 3) // 4


def limbs(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)]


def mont(v):
    return v * RM % P


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2pow(a, e):
    out = (1, 0)
    while e:
        if e & 1:
            out = f2mul(out, a)
        a = f2mul(a, a)
        e >>= 1
    return out


def f2inv(a):
    t = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (a[0] * t % P, (-a[1]) * t % P)


def beta_g1():
    """The cube root of unity beta with (beta x, y) = -[x^2] (x, y) on G1:
    g^((p-1)/3) for the least g giving a nontrivial root (the other root,
    beta^2, fails on the generator; tests/test_bls_oracle.py checks this)."""
    g = 2
    while pow(g, (P - 1) // 3, P) == 1:
        g += 1
    return pow(g, (P - 1) // 3, P)


def psi_coeffs():
    xi = (1, 1)
    return f2inv(f2pow(xi, (P - 1) // 3)), f2inv(f2pow(xi, (P - 1) // 2))


def psi_map(x, y):
    """psi as a map of coordinates: (conj(x) cx, conj(y) cy)."""
    cx, cy = psi_coeffs()
    return f2mul((x[0], (-x[1]) % P), cx), f2mul((y[0], (-y[1]) % P), cy)


def gamma_g2():
    """gamma in Fp with psi(psi(x, y)) = (gamma x, -y): the norm of psi's x
    coefficient (the y coefficient's norm is -1); asserted on coordinate pairs,
    since psi acts on each coordinate by a semilinear map."""
    cx, cy = psi_coeffs()
    gamma = (cx[0] * cx[0] + cx[1] * cx[1]) % P
    assert (cy[0] * cy[0] + cy[1] * cy[1]) % P == P - 1
    assert gamma != 1 and pow(gamma, 3, P) == 1
    for x, y in (((1, 0), (0, 1)), ((3, 5), (7, 11)), ((P - 2, 12345), (G1_X, G1_Y))):
        px, py = psi_map(*psi_map(x, y))
        assert px == (gamma * x[0] % P, gamma * x[1] % P), "gamma"
        assert py == ((-y[0]) % P, (-y[1]) % P), "psi^2 negates y"
    return gamma


def g1_add(a, b):
    """Affine addition on y^2 = x^3 + 4 (None = infinity)."""
    if a is None or b is None:
        return b if a is None else a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], P - 2, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], P - 2, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def g1_gen_glv():
    """Q = [x^2] G1::one() = (beta x, -y) and G1::one() + Q, the operands of
    the fixed-base GLV loop (g1_base_mul_check_kernel); Q is asserted against
    plain double-and-add."""
    g, acc, pt, k = (G1_X, G1_Y), None, (G1_X, G1_Y), X_ABS * X_ABS
    while k:
        if k & 1:
            acc = g1_add(acc, pt)
        pt = g1_add(pt, pt)
        k >>= 1
    q = (beta_g1() * G1_X % P, P - G1_Y)
    assert acc == q, "Q = [x^2] G"
    return q, g1_add(g, q)


def arr(name, v):
    return "constexpr uint32_t %s[12] = {%s};" % (name, ", ".join("0x%08xu" % x for x in limbs(v)))


def arr8(name, v):
    return "constexpr uint32_t %s[8] = {%s};" % (
        name, ", ".join("0x%08xu" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(8)))


def fp2_arr(name, vals):
    rows = []
    for a in vals:
        rows.append("{{%s}, {%s}}" % (", ".join("0x%08xu" % x for x in limbs(mont(a[0]))),
                                      ", ".join("0x%08xu" % x for x in limbs(mont(a[1])))))
    return "constexpr uint32_t %s[%d][2][12] = {\n    %s};" % (name, len(vals), ",\n    ".join(rows))


def main():
    xi = (1, 1)
    assert (G1_Y * G1_Y - G1_X ** 3 - 4) % P == 0
    assert P % 4 == 3 and SQRT_EXP >> (4 * (SQRT_WINDOWS - 1)) != 0
    assert pow(9, SQRT_EXP, P) * 3 % P in (1, P - 1)   # 1/sqrt(9) = +-1/3
    inv29 = (-pow(P, -1, 1 << 29)) % (1 << 29)
    gen_q, gen_t = g1_gen_glv()
    out = [
        "// Generated by gen_bls_consts.py -- BLS12-381 constants for pairing.hip.",
        "// Limbs little-endian (32-bit); field elements in Montgomery form, R = 2^406.",
        "#pragma once",
        "#include <stdint.h>",
        "namespace hbrbc { namespace bls {",
        arr("kP", P),
        arr("kPminus2", P - 2),
        "constexpr uint32_t kP29[14] = {%s};  // p in 29-bit limbs"
        % ", ".join("0x%08xu" % ((P >> (29 * i)) & ((1 << 29) - 1)) for i in range(14)),
        "constexpr uint32_t kPinv29 = 0x%08xu;  // -p^-1 mod 2^29" % inv29,
        arr("kR2", RM * RM % P) + "  // R^2 mod p (to Montgomery form)",
        arr("kOne", mont(1)) + "  // R mod p",
        arr("kB1", mont(4)) + "  // curve constant b = 4",
        "constexpr uint64_t kXAbs = 0x%016xull;  // |x|, x < 0" % X_ABS,
        fp2_arr("kFrob6C1", [f2pow(xi, (P ** k - 1) // 3) for k in range(4)]),
        fp2_arr("kFrob6C2", [f2pow(xi, 2 * (P ** k - 1) // 3) for k in range(4)]),
        fp2_arr("kFrob12C1", [f2pow(xi, (P ** k - 1) // 6) for k in range(4)]),
        arr("kBeta", mont(beta_g1())) + "  // G1 endomorphism: phi(x, y) = (beta x, y)",
        "constexpr uint64_t kXSqHi = 0x%016xull, kXSqLo = 0x%016xull;  // x^2 (128 bits)"
        % ((X_ABS * X_ABS) >> 64, (X_ABS * X_ABS) & ((1 << 64) - 1)),
        fp2_arr("kPsi", [f2inv(f2pow(xi, (P - 1) // 3)), f2inv(f2pow(xi, (P - 1) // 2))])
        + "  // G2 psi: x, y coefficients",
        arr8("kFrR", R_ORDER) + "  // r: the order of G1, the modulus of Fr",
        arr8("kFrMinus2", R_ORDER - 2),
        "constexpr uint32_t kFrInv32 = 0x%08xu;  // -r^-1 mod 2^32"
        % ((-pow(R_ORDER, -1, 1 << 32)) % (1 << 32)),
        arr8("kFrR2", RM_FR * RM_FR % R_ORDER) + "  // 2^512 mod r (to Montgomery form)",
        arr8("kFrOne", RM_FR % R_ORDER) + "  // 2^256 mod r",
        arr("kG1GenX", mont(G1_X)) + "  // G1::one(), affine x",
        arr("kG1GenNegY", mont(P - G1_Y)) + "  // -G1::one(): p - y",
        arr("kGammaG2", mont(gamma_g2())) + "  // G2: psi^2(x, y) = (gamma x, -y) = [x^2] Q",
        arr("kSqrtExp", SQRT_EXP) + "  // (p - 3) / 4, plain: a^this = 1/sqrt(a)",
        "constexpr int kSqrtExpWindows = %d;  // 4-bit windows of kSqrtExp" % SQRT_WINDOWS,
        arr("kHalf", mont((P + 1) // 2)) + "  // 1/2",
        arr("kG1GenY", mont(G1_Y)) + "  // G1::one(), affine y",
        arr("kG1GenQX", mont(gen_q[0])) + "  // Q = [x^2] G1::one() = (beta x, -y): x (y is kG1GenNegY)",
        arr("kG1GenTX", mont(gen_t[0])) + "  // G1::one() + Q, affine x",
        arr("kG1GenTY", mont(gen_t[1])) + "  // G1::one() + Q, affine y",
        arr("kRand384", pow(2, 406 + 22, P))
        + "  // 2^428 mod p: fp_mul(v, this) = v 2^22, the Montgomery form of v 2^-384 (hash_g2.hip)",
        "constexpr uint32_t kH2[16] = {%s};  // the cofactor of E'(Fp2), %d bits"
        % (", ".join("0x%08xu" % ((H2 >> (32 * i)) & 0xFFFFFFFF) for i in range(16)),
           H2.bit_length()),
        "constexpr int kH2Top = %d;  // the cofactor's leading bit" % (H2.bit_length() - 1),
        "}}  // namespace hbrbc::bls",
    ]
    print("\n".join(out))


if __name__ == "__main__":
    main()
