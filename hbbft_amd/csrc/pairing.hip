// pairing.hip -- batched BLS12-381 pairing checks for threshold-decrypt share
// verification.
//
// Reference: /root/reference/src/threshold_decrypt.rs:142 (`ct.verify()`) and
// :220-228 (`pk.verify_decryption_share(share, ct)`), both in `threshold_crypto`
// (git rev 624eeee, Cargo.toml:36), which evaluate
//
//     Ciphertext::verify                   e(G1::one(), W) == e(U, H)
//     PublicKeyShare::verify_decryption_share  e(share, H) == e(pk_i, W)
//
// with H = hash_g1_g2(U, V) and `PEngine::pairing` = the `pairing` crate's
// BLS12-381 optimal ate pairing.  A check here is e(a, b) == e(c, d),
// evaluated as one final exponentiation of f_a,b * f_-c,d (the two GT values
// are equal iff that product exponentiates to 1; GT has prime order r).
//
// MI355X layout.  One lane owns one Miller loop (kernel 1) or one final
// exponentiation (kernel 2): the arithmetic is serial 381-bit Montgomery
// products (12 x 32-bit limbs at rest, 14 x 29-bit limbs inside fp_mul), so a lane-per-pairing
// mapping keeps every limb in VGPRs with no cross-lane traffic.  The Miller
// values travel between the kernels in a limb-major workspace
// ([144 words][pairings]), so every store and load is one coalesced dword per
// lane.  Points arrive in the crate's uncompressed encodings (G1 96 bytes
// x || y, G2 192 bytes x.c1 || x.c0 || y.c1 || y.c0, big-endian, flag bits
// in byte 0) and are checked for canonical coordinates, curve membership and
// membership of the order-r subgroup, as the crate's deserialisation does.
//
// Tower: Fp2 = Fp[u]/(u^2+1), Fp6 = Fp2[v]/(v^3 - (u+1)), Fp12 = Fp6[w]/(w^2 - v),
// the crate's.  Miller loop over |x| = 0xd201000000010000 with homogeneous
// projective doubling/addition on the M-type twist y^2 = x^3 + 4(u+1); each
// line is scaled into the sparse form (c0, c1, c4) and applied with
// mul_by_014; f is conjugated at the end (x < 0).  Final exponentiation: easy
// part, then the crate's hard-part chain (= f^(3 (p^4 - p^2 + 1)/r)).
#include <cstdlib>

#include "bls_consts.hpp"
#include "device_common.hpp"
#include "pairing_tables.hpp"

namespace hbrbc {

namespace {

using namespace bls;

constexpr int NL = 12;  // 32-bit limbs per Fp element

struct Fp { uint32_t l[NL]; };
struct Fp2 { Fp c0, c1; };
struct Fp6 { Fp2 c0, c1, c2; };
struct Fp12 { Fp6 c0, c1; };

#define DEV __device__ __forceinline__
// Call boundaries: out-of-line units keep compile time bounded; everything
// below an NOINL unit is inlined into it.
#define NOINL __device__ __noinline__

// ---------------------------------------------------------------- Fp
DEV void fp_set(Fp &r, const uint32_t (&v)[NL]) {
#pragma unroll
    for (int i = 0; i < NL; ++i) r.l[i] = v[i];
}

DEV void fp_zero(Fp &r) {
#pragma unroll
    for (int i = 0; i < NL; ++i) r.l[i] = 0;
}

DEV bool fp_is_zero(const Fp &a) {
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) t |= a.l[i];
    return t == 0;
}

DEV bool fp_eq(const Fp &a, const Fp &b) {
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) t |= a.l[i] ^ b.l[i];
    return t == 0;
}

// 32-bit add / subtract with carry (v_add_co_ci_u32 / v_sub_co_ci_u32 chains)
DEV uint32_t addc(uint32_t a, uint32_t b, uint32_t cin, uint32_t *cout) {
    return __builtin_addc(a, b, cin, cout);
}
DEV uint32_t subb(uint32_t a, uint32_t b, uint32_t bin, uint32_t *bout) {
    return __builtin_subc(a, b, bin, bout);
}

// r = t - p if t >= p else t  (t < 2p)
DEV void fp_reduce_once(Fp &r, const uint32_t (&t)[NL]) {
    uint32_t s[NL];
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) s[i] = subb(t[i], kP[i], br, &br);
#pragma unroll
    for (int i = 0; i < NL; ++i) r.l[i] = br ? t[i] : s[i];
}

DEV void fp_add(Fp &r, const Fp &a, const Fp &b) {
    uint32_t t[NL];
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) t[i] = addc(a.l[i], b.l[i], c, &c);
    fp_reduce_once(r, t);  // a + b < 2p < 2^382: no carry out of limb 11
}

DEV void fp_sub(Fp &r, const Fp &a, const Fp &b) {
    uint32_t t[NL];
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) t[i] = subb(a.l[i], b.l[i], br, &br);
    const uint32_t mask = 0u - br;  // add p back on borrow
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) r.l[i] = addc(t[i], kP[i] & mask, c, &c);
}

DEV void fp_dbl(Fp &r, const Fp &a) { fp_add(r, a, a); }

DEV void fp_neg(Fp &r, const Fp &a) {
    Fp z;
    fp_zero(z);
    fp_sub(r, z, a);
}

// Montgomery product a*b*2^-406 mod p (R = 2^406, bls_consts.hpp), product
// scanning over 14 limbs of 29 bits: column k of a*b + M*p is a sum of at
// most 28 products < 2^58 plus the carry, so it accumulates in a 64-bit value
// fed straight by v_mad_u64_u32 (the accumulator is the 64-bit addend: no
// zero-extending moves, no carry chains, no carry-flag hazards); each of the
// first 14 columns fixes one 29-bit Montgomery digit m_k.  Two accumulators per
// column (even / odd i) halve the dependent chains.  561 VALU per product
// against 1078 for 32-bit-limb CIOS (288 mads + 248 moves + 264 add-with-carry
// + 205 hazard nops), DESIGN.md §6e.  Inputs < p in 12 x 32-bit limbs; the
// result < 2p is reduced once.
constexpr uint32_t kM29 = (1u << 29) - 1;

DEV void fp_to29(uint32_t (&o)[14], const uint32_t (&w)[NL]) {
#pragma unroll
    for (int i = 0; i < 14; ++i) {
        const int bit = 29 * i, q = bit >> 5, s = bit & 31;
        const uint32_t lo = w[q], hi = (q + 1 < NL) ? w[q + 1] : 0u;
        o[i] = (s ? __builtin_amdgcn_alignbit(hi, lo, s) : lo) & kM29;
    }
}

// 14 digits (13 of 29 bits and a top one, two's complement when `neg`) to
// 12 x 32-bit limbs of the value mod p: value in (-p, 0) gets p added, value
// in [0, 2p) is reduced once.
DEV void fp_from29(Fp &r, const uint32_t (&o)[14], bool neg) {
    uint32_t t[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int bit = 32 * j, i = bit / 29, s = bit % 29;
        uint32_t v = o[i] >> s;
        if (i + 1 < 14) v |= o[i + 1] << (29 - s);
        if (s > 26 && i + 2 < 14) v |= o[i + 2] << (58 - s);
        t[j] = v;
    }
    const uint32_t mask = neg ? 0xFFFFFFFFu : 0u;   // value + p (mod 2^384) when negative
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < NL; ++j) t[j] = addc(t[j], kP[j] & mask, c, &c);
    fp_reduce_once(r, t);
}

// NC independent 64-bit accumulators per column (the products of a column are
// split round-robin over them; each v_mad_u64_u32 depends on the previous one
// of its chain).  2 (round 3) won the A/B against 4.
DEV void fp_mul(Fp &r, const Fp &a, const Fp &b) {
    constexpr int NC = 2;
    uint32_t x[14], y[14], m[14], o[14];
    fp_to29(x, a.l);
    fp_to29(y, b.l);
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 14; ++k) {
        uint64_t e[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) e[c] = c ? 0 : acc;
        int q = 0;
#pragma unroll
        for (int i = 0; i <= k; ++i, ++q) e[q % NC] += (uint64_t)x[i] * y[k - i];
#pragma unroll
        for (int i = 0; i < k; ++i, ++q) e[q % NC] += (uint64_t)m[i] * kP29[k - i];
        acc = e[0];
#pragma unroll
        for (int c = 1; c < NC; ++c) acc += e[c];
        m[k] = ((uint32_t)acc * kPinv29) & kM29;
        acc += (uint64_t)m[k] * kP29[0];   // low 29 bits become 0
        acc >>= 29;
    }
#pragma unroll
    for (int k = 14; k < 27; ++k) {
        uint64_t e[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) e[c] = c ? 0 : acc;
        int q = 0;
#pragma unroll
        for (int i = k - 13; i < 14; ++i, ++q) e[q % NC] += (uint64_t)x[i] * y[k - i];
#pragma unroll
        for (int i = k - 13; i < 14; ++i, ++q) e[q % NC] += (uint64_t)m[i] * kP29[k - i];
        acc = e[0];
#pragma unroll
        for (int c = 1; c < NC; ++c) acc += e[c];
        o[k - 14] = (uint32_t)acc & kM29;
        acc >>= 29;
    }
    o[13] = (uint32_t)acc;   // < 2^5: the result is below 2p < 2^382
    fp_from29(r, o, false);
}

DEV void fp_sqr(Fp &r, const Fp &a) { fp_mul(r, a, a); }

// a^(p-2) (Fermat); once per final exponentiation.
__device__ __noinline__ void fp_inv(Fp &r, const Fp &a) {
    Fp acc, base = a;
    fp_set(acc, kOne);
    for (int w = 0; w < NL; ++w) {
        uint32_t e = kPminus2[w];
        for (int b = 0; b < 32; ++b) {
            if (e & 1u) fp_mul(acc, acc, base);
            fp_sqr(base, base);
            e >>= 1;
        }
    }
    r = acc;
}

// ---------------------------------------------------------------- Fp2
DEV void fp2_add(Fp2 &r, const Fp2 &a, const Fp2 &b) { fp_add(r.c0, a.c0, b.c0); fp_add(r.c1, a.c1, b.c1); }
DEV void fp2_sub(Fp2 &r, const Fp2 &a, const Fp2 &b) { fp_sub(r.c0, a.c0, b.c0); fp_sub(r.c1, a.c1, b.c1); }
DEV void fp2_dbl(Fp2 &r, const Fp2 &a) { fp_dbl(r.c0, a.c0); fp_dbl(r.c1, a.c1); }
DEV void fp2_neg(Fp2 &r, const Fp2 &a) { fp_neg(r.c0, a.c0); fp_neg(r.c1, a.c1); }
DEV void fp2_conj(Fp2 &r, const Fp2 &a) { r.c0 = a.c0; fp_neg(r.c1, a.c1); }
DEV void fp2_zero(Fp2 &r) { fp_zero(r.c0); fp_zero(r.c1); }
DEV bool fp2_is_zero(const Fp2 &a) { return fp_is_zero(a.c0) && fp_is_zero(a.c1); }
DEV bool fp2_eq(const Fp2 &a, const Fp2 &b) { return fp_eq(a.c0, b.c0) && fp_eq(a.c1, b.c1); }

// Fp2 products with lazy reduction: both output coefficients of an Fp2
// product or square are column sums of 29-bit-limb products, accumulated in
// 64-bit values (c0's two's complement: a0 b0 - a1 b1) and Montgomery-reduced
// once each -- Karatsuba's three products share one pass over the columns and
// need two reductions, not three (980 instead of 1176 mads per Fp2 product),
// and the limb conversions and 12-word additions around the products go away.
// Every column stays below 2^63 in magnitude.
template <class Cols>
DEV void fp2_redc(Fp2 &r, Cols cols) {
    uint32_t m0[14], m1[14], o0[14], o1[14];
    uint64_t A0 = 0, A1 = 0;   // A0: two's complement (c0 may be negative)
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        uint64_t e0 = A0, e1 = A1;
        cols(k, e0, e1);
        const int lo = k > 13 ? k - 13 : 0, hi = k < 14 ? k : 14;
#pragma unroll
        for (int i = lo; i < hi; ++i) {
            e0 += (uint64_t)m0[i] * kP29[k - i];
            e1 += (uint64_t)m1[i] * kP29[k - i];
        }
        if (k < 14) {
            m0[k] = ((uint32_t)e0 * kPinv29) & kM29;
            m1[k] = ((uint32_t)e1 * kPinv29) & kM29;
            e0 += (uint64_t)m0[k] * kP29[0];
            e1 += (uint64_t)m1[k] * kP29[0];
        } else {
            o0[k - 14] = (uint32_t)e0 & kM29;
            o1[k - 14] = (uint32_t)e1 & kM29;
        }
        A0 = (uint64_t)((int64_t)e0 >> 29);
        A1 = e1 >> 29;
    }
    o0[13] = (uint32_t)A0;   // c0 in (-p, 2p): a negative top digit
    o1[13] = (uint32_t)A1;   // c1 in [0, 2p)
    fp_from29(r.c0, o0, (int32_t)o0[13] < 0);
    fp_from29(r.c1, o1, false);
}

// The square is the lazily reduced form; the product is three Fp products
// (the lazy product lost its A/B), with a scheduling barrier
// between them so the scheduler cannot interleave them (fewer live digits,
// less ILP; round 6: Miller 71.1 -> 66.8, final exp 68.8 -> 66.8 ms, r6u).
DEV void fp2_mul_in(Fp2 &r, const Fp2 &a, const Fp2 &b) {
    Fp t0, t1, s0, s1;
    fp_mul(t0, a.c0, b.c0);
    __builtin_amdgcn_sched_barrier(0);
    fp_mul(t1, a.c1, b.c1);
    __builtin_amdgcn_sched_barrier(0);
    fp_add(s0, a.c0, a.c1);
    fp_add(s1, b.c0, b.c1);
    fp_mul(s0, s0, s1);
    __builtin_amdgcn_sched_barrier(0);
    fp_sub(r.c0, t0, t1);
    fp_sub(s0, s0, t0);
    fp_sub(r.c1, s0, t1);
}

DEV void fp2_sqr_in(Fp2 &r, const Fp2 &a) {
    uint32_t x0[14], x1[14], s[14], t2[14];
    int32_t d[14];
    fp_to29(x0, a.c0.l);
    fp_to29(x1, a.c1.l);
#pragma unroll
    for (int i = 0; i < 14; ++i) {
        s[i] = x0[i] + x1[i];
        d[i] = (int32_t)x0[i] - (int32_t)x1[i];
        t2[i] = x1[i] << 1;
    }
    fp2_redc(r, [&](int k, uint64_t &e0, uint64_t &e1) {
        const int lo = k > 13 ? k - 13 : 0, hi = k < 13 ? k : 13;
        int64_t q0 = 0;
        uint64_t q1 = 0;
#pragma unroll
        for (int i = lo; i <= hi; ++i) {
            q0 += (int64_t)(int32_t)s[i] * d[k - i];   // (a0 + a1)(a0 - a1)
            q1 += (uint64_t)x0[i] * t2[k - i];         // 2 a0 a1
        }
        e0 += (uint64_t)q0;
        e1 += q1;
    });
}

// Out-of-line forms for cold code (inversions, Frobenius, input checks); the
// hot units (Fp6 products, the sparse line product, the cyclotomic square, the
// Miller steps) inline fp2_mul_in / fp2_sqr_in into their own bodies.
NOINL void fp2_mul(Fp2 &r, const Fp2 &a, const Fp2 &b) { fp2_mul_in(r, a, b); }
NOINL void fp2_sqr(Fp2 &r, const Fp2 &a) { fp2_sqr_in(r, a); }

DEV void fp2_mul_fp(Fp2 &r, const Fp2 &a, const Fp &s) { fp_mul(r.c0, a.c0, s); fp_mul(r.c1, a.c1, s); }

// * xi = u + 1
DEV void fp2_mul_xi(Fp2 &r, const Fp2 &a) {
    Fp t0, t1;
    fp_sub(t0, a.c0, a.c1);
    fp_add(t1, a.c0, a.c1);
    r.c0 = t0;
    r.c1 = t1;
}

DEV void fp2_inv(Fp2 &r, const Fp2 &a) {
    Fp n0, n1;
    fp_sqr(n0, a.c0);
    fp_sqr(n1, a.c1);
    fp_add(n0, n0, n1);
    fp_inv(n0, n0);
    fp_mul(r.c0, a.c0, n0);
    fp_mul(n1, a.c1, n0);
    fp_neg(r.c1, n1);
}

DEV void fp2_frob(Fp2 &r, const Fp2 &a, int k) {
    if (k & 1) fp2_conj(r, a);
    else r = a;
}

DEV void fp2_const(Fp2 &r, const uint32_t (&v)[2][NL]) { fp_set(r.c0, v[0]); fp_set(r.c1, v[1]); }

// ---------------------------------------------------------------- Fp6
DEV void fp6_add(Fp6 &r, const Fp6 &a, const Fp6 &b) { fp2_add(r.c0, a.c0, b.c0); fp2_add(r.c1, a.c1, b.c1); fp2_add(r.c2, a.c2, b.c2); }
DEV void fp6_sub(Fp6 &r, const Fp6 &a, const Fp6 &b) { fp2_sub(r.c0, a.c0, b.c0); fp2_sub(r.c1, a.c1, b.c1); fp2_sub(r.c2, a.c2, b.c2); }
DEV void fp6_neg(Fp6 &r, const Fp6 &a) { fp2_neg(r.c0, a.c0); fp2_neg(r.c1, a.c1); fp2_neg(r.c2, a.c2); }
DEV void fp6_dbl(Fp6 &r, const Fp6 &a) { fp2_dbl(r.c0, a.c0); fp2_dbl(r.c1, a.c1); fp2_dbl(r.c2, a.c2); }

// * v: (a0, a1, a2) -> (xi a2, a0, a1)
DEV void fp6_mul_v(Fp6 &r, const Fp6 &a) {
    Fp2 t;
    fp2_mul_xi(t, a.c2);
    r.c2 = a.c1;
    r.c1 = a.c0;
    r.c0 = t;
}

DEV void fp6_mul_in(Fp6 &r, const Fp6 &a, const Fp6 &b) {
    Fp2 aa, bb, cc, s, t, t1, t2, t3;
    fp2_mul_in(aa, a.c0, b.c0);
    fp2_mul_in(bb, a.c1, b.c1);
    fp2_mul_in(cc, a.c2, b.c2);
    fp2_add(s, a.c1, a.c2);
    fp2_add(t, b.c1, b.c2);
    fp2_mul_in(t1, s, t);
    fp2_sub(t1, t1, bb);
    fp2_sub(t1, t1, cc);
    fp2_mul_xi(t1, t1);
    fp2_add(t1, t1, aa);
    fp2_add(s, a.c0, a.c2);
    fp2_add(t, b.c0, b.c2);
    fp2_mul_in(t3, s, t);
    fp2_sub(t3, t3, aa);
    fp2_add(t3, t3, bb);
    fp2_sub(t3, t3, cc);
    fp2_add(s, a.c0, a.c1);
    fp2_add(t, b.c0, b.c1);
    fp2_mul_in(t2, s, t);
    fp2_sub(t2, t2, aa);
    fp2_sub(t2, t2, bb);
    fp2_mul_xi(cc, cc);
    fp2_add(t2, t2, cc);
    r.c0 = t1;
    r.c1 = t2;
    r.c2 = t3;
}
NOINL void fp6_mul(Fp6 &r, const Fp6 &a, const Fp6 &b) { fp6_mul_in(r, a, b); }

// (a0 + a1 v + a2 v^2)(c0 + c1 v)
DEV void fp6_mul_by_01(Fp6 &r, const Fp6 &a, const Fp2 &c0, const Fp2 &c1) {
    Fp2 aa, bb, s, t1, t2, t3;
    fp2_mul_in(aa, a.c0, c0);
    fp2_mul_in(bb, a.c1, c1);
    fp2_add(s, a.c1, a.c2);
    fp2_mul_in(t1, s, c1);
    fp2_sub(t1, t1, bb);
    fp2_mul_xi(t1, t1);
    fp2_add(t1, t1, aa);
    fp2_add(s, a.c0, a.c2);
    fp2_mul_in(t3, s, c0);
    fp2_sub(t3, t3, aa);
    fp2_add(t3, t3, bb);
    Fp2 cs;
    fp2_add(cs, c0, c1);
    fp2_add(s, a.c0, a.c1);
    fp2_mul_in(t2, s, cs);
    fp2_sub(t2, t2, aa);
    fp2_sub(t2, t2, bb);
    r.c0 = t1;
    r.c1 = t2;
    r.c2 = t3;
}

// (a0 + a1 v + a2 v^2) c1 v
DEV void fp6_mul_by_1(Fp6 &r, const Fp6 &a, const Fp2 &c1) {
    Fp2 t0, t1, t2;
    fp2_mul_in(t2, a.c1, c1);
    fp2_mul_in(t1, a.c0, c1);
    fp2_mul_in(t0, a.c2, c1);
    fp2_mul_xi(r.c0, t0);
    r.c1 = t1;
    r.c2 = t2;
}

DEV void fp6_inv(Fp6 &r, const Fp6 &a) {
    Fp2 c0, c1, c2, t, u;
    fp2_sqr(c0, a.c0);
    fp2_mul(t, a.c1, a.c2);
    fp2_mul_xi(t, t);
    fp2_sub(c0, c0, t);           // a0^2 - xi a1 a2
    fp2_sqr(c1, a.c2);
    fp2_mul_xi(c1, c1);
    fp2_mul(t, a.c0, a.c1);
    fp2_sub(c1, c1, t);           // xi a2^2 - a0 a1
    fp2_sqr(c2, a.c1);
    fp2_mul(t, a.c0, a.c2);
    fp2_sub(c2, c2, t);           // a1^2 - a0 a2
    fp2_mul(t, a.c2, c1);
    fp2_mul(u, a.c1, c2);
    fp2_add(t, t, u);
    fp2_mul_xi(t, t);
    fp2_mul(u, a.c0, c0);
    fp2_add(t, t, u);             // norm
    fp2_inv(t, t);
    fp2_mul(r.c0, c0, t);
    fp2_mul(r.c1, c1, t);
    fp2_mul(r.c2, c2, t);
}

DEV void fp6_frob(Fp6 &r, const Fp6 &a, int k) {
    Fp2 g, t;
    fp2_frob(r.c0, a.c0, k);
    fp2_frob(t, a.c1, k);
    fp2_const(g, kFrob6C1[k]);
    fp2_mul(r.c1, t, g);
    fp2_frob(t, a.c2, k);
    fp2_const(g, kFrob6C2[k]);
    fp2_mul(r.c2, t, g);
}

// ---------------------------------------------------------------- Fp12
DEV void fp12_one(Fp12 &r) {
    Fp2 z;
    fp2_zero(z);
    r.c0.c0 = z; r.c0.c1 = z; r.c0.c2 = z;
    r.c1 = r.c0;
    fp_set(r.c0.c0.c0, kOne);
}

DEV bool fp12_is_one(const Fp12 &a) {
    Fp one;
    fp_set(one, kOne);
    return fp_eq(a.c0.c0.c0, one) && fp_is_zero(a.c0.c0.c1) && fp2_is_zero(a.c0.c1) &&
           fp2_is_zero(a.c0.c2) && fp2_is_zero(a.c1.c0) && fp2_is_zero(a.c1.c1) &&
           fp2_is_zero(a.c1.c2);
}

DEV void fp12_conj(Fp12 &r, const Fp12 &a) { r.c0 = a.c0; fp6_neg(r.c1, a.c1); }

// INL: the Fp6 products inlined into the product (fp12_exp_by_x); the
// out-of-line fp12_mul keeps them as calls (the inlined form lost its A/B)
template <bool INL>
DEV void fp12_mul_t(Fp12 &r, const Fp12 &a, const Fp12 &b) {
    Fp6 aa, bb, s, t;
    if (INL) fp6_mul_in(aa, a.c0, b.c0); else fp6_mul(aa, a.c0, b.c0);
    if (INL) fp6_mul_in(bb, a.c1, b.c1); else fp6_mul(bb, a.c1, b.c1);
    fp6_add(s, a.c0, a.c1);
    fp6_add(t, b.c0, b.c1);
    if (INL) fp6_mul_in(s, s, t); else fp6_mul(s, s, t);
    fp6_sub(s, s, aa);
    fp6_sub(r.c1, s, bb);
    fp6_mul_v(bb, bb);
    fp6_add(r.c0, aa, bb);
}
NOINL void fp12_mul(Fp12 &r, const Fp12 &a, const Fp12 &b) { fp12_mul_t<false>(r, a, b); }

// INL: the Fp6 products inlined (no call boundary inside the unit, so no
// stack traffic for their operands; tools/fp_microbench.hip: the same 26.8 k
// lane-ops per squaring run 1.47x faster in this form)
template <bool INL>
DEV void fp12_sqr_t(Fp12 &r, const Fp12 &a) {
    Fp6 ab, s, t;
    if (INL) fp6_mul_in(ab, a.c0, a.c1); else fp6_mul(ab, a.c0, a.c1);
    fp6_add(s, a.c0, a.c1);
    fp6_mul_v(t, a.c1);
    fp6_add(t, t, a.c0);
    if (INL) fp6_mul_in(s, s, t); else fp6_mul(s, s, t);
    fp6_sub(s, s, ab);
    fp6_mul_v(t, ab);
    fp6_sub(r.c0, s, t);
    fp6_dbl(r.c1, ab);
}
NOINL void fp12_sqr(Fp12 &r, const Fp12 &a) { fp12_sqr_t<false>(r, a); }

// f * (c0 + c1 v + c4 v w): the sparse line value
DEV void fp12_mul_by_014_in(Fp12 &f, const Fp2 &c0, const Fp2 &c1, const Fp2 &c4) {
    Fp6 aa, bb, s;
    Fp2 o;
    fp6_mul_by_01(aa, f.c0, c0, c1);
    fp6_mul_by_1(bb, f.c1, c4);
    fp2_add(o, c1, c4);
    fp6_add(s, f.c1, f.c0);
    fp6_mul_by_01(s, s, c0, o);
    fp6_sub(s, s, aa);
    fp6_sub(f.c1, s, bb);
    fp6_mul_v(bb, bb);
    fp6_add(f.c0, bb, aa);
}
NOINL void fp12_mul_by_014(Fp12 &f, const Fp2 &c0, const Fp2 &c1, const Fp2 &c4) {
    fp12_mul_by_014_in(f, c0, c1, c4);
}

DEV void fp12_inv(Fp12 &r, const Fp12 &a) {
    Fp6 t0, t1;
    fp6_mul(t0, a.c0, a.c0);
    fp6_mul(t1, a.c1, a.c1);
    fp6_mul_v(t1, t1);
    fp6_sub(t0, t0, t1);          // a0^2 - v a1^2
    fp6_inv(t0, t0);
    fp6_mul(r.c0, a.c0, t0);
    fp6_mul(t1, a.c1, t0);
    fp6_neg(r.c1, t1);
}

NOINL void fp12_frob(Fp12 &r, const Fp12 &a, int k) {
    Fp6 c1;
    Fp2 g;
    fp6_frob(r.c0, a.c0, k);
    fp6_frob(c1, a.c1, k);
    fp2_const(g, kFrob12C1[k]);
    fp2_mul(r.c1.c0, c1.c0, g);
    fp2_mul(r.c1.c1, c1.c1, g);
    fp2_mul(r.c1.c2, c1.c2, g);
}

// (a + b s)^2 in Fp4 = Fp2[s]/(s^2 - xi): (a^2 + xi b^2, 2ab)
DEV void fp4_sqr(Fp2 &c0, Fp2 &c1, const Fp2 &a, const Fp2 &b) {
    Fp2 t0, t1, t2;
    fp2_sqr_in(t0, a);
    fp2_sqr_in(t1, b);
    fp2_mul_xi(t2, t1);
    fp2_add(c0, t2, t0);
    fp2_add(t2, a, b);
    fp2_sqr_in(t2, t2);
    fp2_sub(t2, t2, t0);
    fp2_sub(c1, t2, t1);
}

// Granger-Scott squaring, valid on the cyclotomic subgroup (every value of
// the hard part): 9 Fp2 squarings instead of the 2 Fp6 products of fp12_sqr.
// Inlined into fp12_exp_by_x's loop, so the running value stays in registers
// instead of passing through the stack 62 times per call (round 5: 262144
// grouped checks 159.1 -> 157.3 ms; with 1 wave/SIMD as well 168.1,
// profiles/r5n_f4_cyclo_inline_ab.txt)
DEV void fp12_cyclo_sqr(Fp12 &f) {
    Fp2 z0 = f.c0.c0, z4 = f.c0.c1, z3 = f.c0.c2, z2 = f.c1.c0, z1 = f.c1.c1, z5 = f.c1.c2;
    Fp2 t0, t1, t2, t3;
    fp4_sqr(t0, t1, z0, z1);
    fp2_sub(z0, t0, z0);
    fp2_dbl(z0, z0);
    fp2_add(z0, z0, t0);          // 3 t0 - 2 z0
    fp2_add(z1, t1, z1);
    fp2_dbl(z1, z1);
    fp2_add(z1, z1, t1);          // 3 t1 + 2 z1
    fp4_sqr(t0, t1, z2, z3);
    fp4_sqr(t2, t3, z4, z5);
    fp2_sub(z4, t0, z4);
    fp2_dbl(z4, z4);
    fp2_add(z4, z4, t0);
    fp2_add(z5, t1, z5);
    fp2_dbl(z5, z5);
    fp2_add(z5, z5, t1);
    fp2_mul_xi(t0, t3);
    fp2_add(z2, t0, z2);
    fp2_dbl(z2, z2);
    fp2_add(z2, z2, t0);
    fp2_sub(z3, t2, z3);
    fp2_dbl(z3, z3);
    fp2_add(z3, z3, t2);
    f.c0.c0 = z0; f.c0.c1 = z4; f.c0.c2 = z3;
    f.c1.c0 = z2; f.c1.c1 = z1; f.c1.c2 = z5;
}

// f^x for the BLS parameter x < 0 (the crate's exp_by_x: pow by |x|, then
// conjugate -- the inverse on the cyclotomic subgroup).  `shift` gives |x|>>1.
// The five products by `a` are inlined too (Fp6 products inlined), so the
// whole f^|x| is one unit with no call inside its loop (round 6, on the
// serialised Fp2 base: final exp 66.9 -> 59.1 ms, r6z)
NOINL void fp12_exp_by_x(Fp12 &r, const Fp12 &a, int shift) {
    const uint64_t e = kXAbs >> shift;
    Fp12 acc = a;
    for (int b = 62 - shift; b >= 0; --b) {
        fp12_cyclo_sqr(acc);
        if ((e >> b) & 1u) {
            fp12_mul_t<true>(acc, acc, a);
        }
    }
    fp12_conj(r, acc);
}

// ---------------------------------------------------------------- Miller loop
struct G2Proj { Fp2 x, y, z; };

// T <- 2T and the tangent line at T before it is evaluated at P, scaled by
// 2YZ^2: L0 + (L1 xp) v + (L4 yp) v w with L0 = 3X^3 - 2Y^2 Z, L1 = -3X^2 Z,
// L4 = 2 Y Z^2.
// The G2 line units use the serialised Fp2 product too (G2 preparation: one
// lane per point, latency-bound at 1/16 of the wave slots, where the
// serialisation only lengthens the chain -- and still it won its A/B).
NOINL void g2_dbl_line(G2Proj &T, Fp2 &l0, Fp2 &l1, Fp2 &l4) {
    Fp2 xx, w, s, ss, sss, rr, RR, B, h, t;
    fp2_sqr_in(xx, T.x);
    fp2_dbl(w, xx);
    fp2_add(w, w, xx);            // w = 3 X^2
    fp2_mul_in(s, T.y, T.z);
    fp2_dbl(s, s);                // s = 2 Y Z
    fp2_sqr_in(ss, s);
    fp2_mul_in(sss, s, ss);
    fp2_mul_in(rr, T.y, s);       // R = Y s = 2 Y^2 Z
    fp2_sqr_in(RR, rr);
    fp2_add(B, T.x, rr);
    fp2_sqr_in(B, B);
    fp2_sub(B, B, xx);
    fp2_sub(B, B, RR);            // B = (X + R)^2 - X^2 - R^2
    fp2_mul_in(l0, T.x, w);
    fp2_sub(l0, l0, rr);          // 3X^3 - 2Y^2 Z
    fp2_mul_in(l1, w, T.z);
    fp2_neg(l1, l1);              // -3X^2 Z
    fp2_mul_in(l4, s, T.z);       // 2 Y Z^2
    fp2_sqr_in(h, w);
    fp2_sub(h, h, B);
    fp2_sub(h, h, B);             // h = w^2 - 2B
    fp2_mul_in(T.x, h, s);
    fp2_sub(t, B, h);
    fp2_mul_in(t, w, t);
    fp2_dbl(RR, RR);
    fp2_sub(T.y, t, RR);          // w (B - h) - 2 R^2
    T.z = sss;
}

// T <- T + Q (Q affine) and the line through T and Q before evaluation at P,
// scaled by (xq Z - X): L0 = u xq - v yq, L1 = -u, L4 = v with u = yq Z - Y,
// v = xq Z - X.
NOINL void g2_add_line(G2Proj &T, const Fp2 &xq, const Fp2 &yq, Fp2 &l0, Fp2 &l1, Fp2 &l4) {
    Fp2 u, v, uu, vv, vvv, R, A, t;
    fp2_mul_in(u, yq, T.z);
    fp2_sub(u, u, T.y);
    fp2_mul_in(v, xq, T.z);
    fp2_sub(v, v, T.x);
    fp2_mul_in(l0, u, xq);
    fp2_mul_in(t, v, yq);
    fp2_sub(l0, l0, t);
    fp2_neg(l1, u);
    l4 = v;
    fp2_sqr_in(uu, u);
    fp2_sqr_in(vv, v);
    fp2_mul_in(vvv, v, vv);
    fp2_mul_in(R, vv, T.x);
    fp2_mul_in(A, uu, T.z);
    fp2_sub(A, A, vvv);
    fp2_sub(A, A, R);
    fp2_sub(A, A, R);             // A = uu Z - vvv - 2R
    fp2_mul_in(T.x, v, A);
    fp2_sub(t, R, A);
    fp2_mul_in(t, u, t);
    fp2_mul_in(vvv, vvv, T.y);
    fp2_sub(T.y, t, vvv);
    fp2_mul_in(T.z, T.z, vv);
    fp2_mul_in(T.z, T.z, v);      // Z vvv
}

// f <- f * line(P): the line evaluated at P = (xp, yp) (sparse (c0, c1, c4))
DEV void apply_line(Fp12 &f, const Fp2 &l0, const Fp2 &l1, const Fp2 &l4, const Fp &xp,
                    const Fp &yp) {
    Fp2 a, b;
    fp2_mul_fp(a, l1, xp);
    fp2_mul_fp(b, l4, yp);
    fp12_mul_by_014(f, l0, a, b);
}

NOINL void miller_dbl(G2Proj &T, Fp12 &f, const Fp &xp, const Fp &yp) {
    Fp2 l0, l1, l4;
    g2_dbl_line(T, l0, l1, l4);
    apply_line(f, l0, l1, l4, xp, yp);
}

NOINL void miller_add(G2Proj &T, Fp12 &f, const Fp2 &xq, const Fp2 &yq, const Fp &xp,
                      const Fp &yp) {
    Fp2 l0, l1, l4;
    g2_add_line(T, xq, yq, l0, l1, l4);
    apply_line(f, l0, l1, l4, xp, yp);
}

// ---------------------------------------------------------------- encodings
// 48 big-endian bytes -> limbs (little-endian words); returns false if the
// value is not below p.  `top_mask` clears flag bits of the first byte.
DEV bool load_be48(Fp &r, const uint8_t *src, uint32_t top_mask) {
#pragma unroll
    for (int w = 0; w < NL; ++w) {
        const uint8_t *q = src + 44 - 4 * w;
        uint32_t v = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
        r.l[w] = v;
    }
    r.l[NL - 1] &= top_mask;
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const uint64_t d = (uint64_t)r.l[i] - kP[i] - br;
        br = (d >> 32) & 1u;
    }
    return br != 0;  // r < p
}

DEV void to_mont(Fp &r, const Fp &a) {
    Fp r2;
    fp_set(r2, kR2);
    fp_mul(r, a, r2);
}

DEV void from_mont(Fp &r, const Fp &a) {
    Fp one;
    fp_zero(one);
    one.l[0] = 1;
    fp_mul(r, a, one);
}

DEV bool all_zero(const uint8_t *p, int n, uint8_t first_mask) {
    uint32_t t = p[0] & first_mask;
    for (int i = 1; i < n; ++i) t |= p[i];
    return t == 0;
}

// Status of a decoded point: 0 ok, 1 infinity, 2 invalid.
enum { PT_OK = 0, PT_INF = 1, PT_BAD = 2 };

// ------------------------------------------------------- subgroup checks
// The crate's deserialisation (`into_affine`: on-curve, then
// is_in_correct_subgroup_assuming_on_curve = [r] P == O) rejects points of
// E(Fp) / E'(Fp2) outside the order-r subgroup before any pairing.  Here the
// equivalent endomorphism tests (Scott, ePrint 2021/1130 sec. 6, proof in
// 2022/352): P in G1 iff phi(P) = (beta x, y) = -[x^2] P, and Q in G2 iff
// psi(Q) = [x] Q, i.e. a 128-bit and a 64-bit scalar multiplication instead
// of a 255-bit one.  oracle/bls_oracle.py restates the crate's [r] P test and
// tests/test_pairing.py feeds on-curve points outside the subgroup (status 2).
// Complete projective formulas for y^2 = x^3 + b (Renes-Costello-Batina 2016,
// algorithms 7 and 9 with a = 0), so no exceptional case arises mid-chain.
template <class F> struct PtProj { F x, y, z; };

DEV void fe_mul(Fp &r, const Fp &a, const Fp &b) { fp_mul(r, a, b); }
DEV void fe_mul(Fp2 &r, const Fp2 &a, const Fp2 &b) { fp2_mul_in(r, a, b); }
DEV void fe_add(Fp &r, const Fp &a, const Fp &b) { fp_add(r, a, b); }
DEV void fe_add(Fp2 &r, const Fp2 &a, const Fp2 &b) { fp2_add(r, a, b); }
DEV void fe_sub(Fp &r, const Fp &a, const Fp &b) { fp_sub(r, a, b); }
DEV void fe_sub(Fp2 &r, const Fp2 &a, const Fp2 &b) { fp2_sub(r, a, b); }
DEV void fe_zero(Fp &r) { fp_zero(r); }
DEV void fe_zero(Fp2 &r) { fp2_zero(r); }
DEV void fe_one(Fp &r) { fp_set(r, kOne); }
DEV void fe_one(Fp2 &r) { fp_set(r.c0, kOne); fp_zero(r.c1); }
// 3b: 12 on E, 12 (u + 1) on the twist
DEV void fe_mul_b3(Fp &r, const Fp &a) {
    Fp t;
    fp_add(t, a, a);
    fp_add(t, t, a);
    fp_add(t, t, t);
    fp_add(r, t, t);
}
DEV void fe_mul_b3(Fp2 &r, const Fp2 &a) {
    Fp2 x;
    fp2_mul_xi(x, a);
    fe_mul_b3(r.c0, x.c0);
    fe_mul_b3(r.c1, x.c1);
}

template <class F>
NOINL void pt_dbl(PtProj<F> &p) {
    F t0, t1, t2, x3, y3, z3;
    fe_mul(t0, p.y, p.y);
    fe_add(z3, t0, t0);
    fe_add(z3, z3, z3);
    fe_add(z3, z3, z3);
    fe_mul(t1, p.y, p.z);
    fe_mul(t2, p.z, p.z);
    fe_mul_b3(t2, t2);
    fe_mul(x3, t2, z3);
    fe_add(y3, t0, t2);
    fe_mul(z3, t1, z3);
    fe_add(t1, t2, t2);
    fe_add(t2, t1, t2);
    fe_sub(t0, t0, t2);
    fe_mul(y3, t0, y3);
    fe_add(y3, x3, y3);
    fe_mul(t1, p.x, p.y);
    fe_mul(x3, t0, t1);
    fe_add(p.x, x3, x3);
    p.y = y3;
    p.z = z3;
}

// p <- p + (qx, qy, 1)
template <class F>
NOINL void pt_add_affine(PtProj<F> &p, const F &qx, const F &qy) {
    F t0, t1, t2, t3, t4, x3, y3, z3;
    fe_mul(t0, p.x, qx);
    fe_mul(t1, p.y, qy);
    t2 = p.z;
    fe_add(t3, p.x, p.y);
    fe_add(t4, qx, qy);
    fe_mul(t3, t3, t4);
    fe_add(t4, t0, t1);
    fe_sub(t3, t3, t4);
    fe_mul(t4, qy, p.z);
    fe_add(t4, t4, p.y);            // Y1 + Y2 Z1
    fe_mul(y3, qx, p.z);
    fe_add(y3, y3, p.x);            // X1 + X2 Z1
    fe_add(x3, t0, t0);
    fe_add(t0, x3, t0);
    fe_mul_b3(t2, t2);
    fe_add(z3, t1, t2);
    fe_sub(t1, t1, t2);
    fe_mul_b3(y3, y3);
    fe_mul(x3, t4, y3);
    fe_mul(t2, t3, t1);
    fe_sub(x3, t2, x3);
    fe_mul(y3, y3, t0);
    fe_mul(t1, t1, z3);
    fe_add(y3, t1, y3);
    fe_mul(t0, t0, t3);
    fe_mul(z3, z3, t4);
    fe_add(p.z, z3, t0);
    p.x = x3;
    p.y = y3;
}

// [k] (x, y) for the bits of k below its leading one (k's top bit at `top`)
template <class F>
DEV void pt_mul_bits(PtProj<F> &acc, const F &x, const F &y, uint64_t hi, uint64_t lo, int top) {
    acc.x = x;
    acc.y = y;
    fe_one(acc.z);
    for (int b = top - 1; b >= 0; --b) {
        pt_dbl(acc);
        const uint64_t w = b >= 64 ? hi : lo;
        if ((w >> (b & 63)) & 1u) pt_add_affine(acc, x, y);
    }
}

// p <- p + q, both projective (Renes-Costello-Batina algorithm 7 with a = 0
// and 3b = 12 on E, 12 (u + 1) on the twist).  Complete on E(Fp), which has
// odd order.  E'(Fp2) has even order, so the formulas are not complete on all
// of it; they are on the order-r subgroup (odd order: no point of order 2, the
// only exception), and every G2 operand is a checked G2 point or a sum of
// such.  One template: cross-compiled, every kernel kept its VGPRs, spills,
// scratch and instruction count against the former Fp and Fp2 overloads.
template <class F>
NOINL void pt_add_proj(PtProj<F> &p, const PtProj<F> &q) {
    F t0, t1, t2, t3, t4, x3, y3, z3;
    fe_mul(t0, p.x, q.x);
    fe_mul(t1, p.y, q.y);
    fe_mul(t2, p.z, q.z);
    fe_add(t3, p.x, p.y);
    fe_add(t4, q.x, q.y);
    fe_mul(t3, t3, t4);
    fe_add(t4, t0, t1);
    fe_sub(t3, t3, t4);             // X1 Y2 + X2 Y1
    fe_add(t4, p.y, p.z);
    fe_add(x3, q.y, q.z);
    fe_mul(t4, t4, x3);
    fe_add(x3, t1, t2);
    fe_sub(t4, t4, x3);             // Y1 Z2 + Y2 Z1
    fe_add(x3, p.x, p.z);
    fe_add(y3, q.x, q.z);
    fe_mul(x3, x3, y3);
    fe_add(y3, t0, t2);
    fe_sub(y3, x3, y3);             // X1 Z2 + X2 Z1
    fe_add(x3, t0, t0);
    fe_add(t0, x3, t0);
    fe_mul_b3(t2, t2);
    fe_add(z3, t1, t2);
    fe_sub(t1, t1, t2);
    fe_mul_b3(y3, y3);
    fe_mul(x3, t4, y3);
    fe_mul(t2, t3, t1);
    fe_sub(x3, t2, x3);
    fe_mul(y3, y3, t0);
    fe_mul(t1, t1, z3);
    fe_add(y3, t1, y3);
    fe_mul(t0, t0, t3);
    fe_mul(z3, z3, t4);
    fe_add(p.z, z3, t0);
    p.x = x3;
    p.y = y3;
}

template <class F>
DEV void pt_identity(PtProj<F> &p) {
    fe_zero(p.x);
    fe_one(p.y);
    fe_zero(p.z);
}

// Projective points between the kernels: limb-major like store_f12, word w of
// share j at ws[w * n + j] (X, Y, Z: 36 words over Fp, 72 over Fp2).
template <class F>
DEV void store_pt(uint32_t *ws, size_t n, size_t j, const PtProj<F> &p) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&p);
#pragma unroll 4
    for (int w = 0; w < (int)(sizeof(PtProj<F>) / 4); ++w) ws[(size_t)w * n + j] = src[w];
}

template <class F>
DEV void load_pt(PtProj<F> &p, const uint32_t *ws, size_t n, size_t j) {
    uint32_t *dst = reinterpret_cast<uint32_t *>(&p);
#pragma unroll 4
    for (int w = 0; w < (int)(sizeof(PtProj<F>) / 4); ++w) dst[w] = ws[(size_t)w * n + j];
}

// Affine table entries (Montgomery form): the words of x, then of y, moved as
// uint4 -- x || y for G1 (kG1KeyWords), x.c0, x.c1, y.c0, y.c1 for G2
// (kG2PtWords).
constexpr int kG1KeyWords = 2 * NL;
constexpr int kG2PtWords = 4 * NL;

DEV void store_fe(uint32_t *dst, const Fp &a) {
#pragma unroll
    for (int w = 0; w < NL; w += 4)
        *reinterpret_cast<uint4 *>(dst + w) = make_uint4(a.l[w], a.l[w + 1], a.l[w + 2], a.l[w + 3]);
}
DEV void store_fe(uint32_t *dst, const Fp2 &a) { store_fe(dst, a.c0); store_fe(dst + NL, a.c1); }
DEV void load_fe(Fp &a, const uint32_t *src) {
#pragma unroll
    for (int w = 0; w < NL; w += 4) {
        const uint4 q = *reinterpret_cast<const uint4 *>(src + w);
        a.l[w] = q.x; a.l[w + 1] = q.y; a.l[w + 2] = q.z; a.l[w + 3] = q.w;
    }
}
DEV void load_fe(Fp2 &a, const uint32_t *src) { load_fe(a.c0, src); load_fe(a.c1, src + NL); }

template <class F>
DEV void store_affine(uint32_t *dst, const F &x, const F &y) {
    store_fe(dst, x);
    store_fe(dst + sizeof(F) / 4, y);
}
template <class F>
DEV void load_affine(const uint32_t *src, F &x, F &y) {
    load_fe(x, src);
    load_fe(y, src + sizeof(F) / 4);
}

// (x, y) affine (Montgomery form), already on E: phi(P) == -[x^2] P, i.e.
// [x^2] P == (beta x, -y) in projective coordinates (Z != 0)
NOINL bool g1_in_subgroup(const Fp &x, const Fp &y) {
    PtProj<Fp> a;
    pt_mul_bits(a, x, y, kXSqHi, kXSqLo, 127);
    Fp bx, ny, l, r;
    fp_set(bx, kBeta);
    fp_mul(bx, bx, x);
    fp_neg(ny, y);
    fp_mul(l, bx, a.z);
    fp_mul(r, ny, a.z);
    return !fp_is_zero(a.z) && fp_eq(l, a.x) && fp_eq(r, a.y);
}

// (x, y) on E': psi(Q) == [x] Q = -[|x|] Q, i.e. [|x|] Q == (psi_x, -psi_y)
NOINL bool g2_in_subgroup(const Fp2 &x, const Fp2 &y) {
    PtProj<Fp2> a;
    pt_mul_bits(a, x, y, 0, kXAbs, 63);
    Fp2 cx, cy, px, py, l, r;
    fp2_const(cx, kPsi[0]);
    fp2_const(cy, kPsi[1]);
    fp2_conj(px, x);
    fp2_mul(px, px, cx);
    fp2_conj(py, y);
    fp2_mul(py, py, cy);
    fp2_neg(py, py);
    fp2_mul(l, px, a.z);
    fp2_mul(r, py, a.z);
    return !fp2_is_zero(a.z) && fp2_eq(l, a.x) && fp2_eq(r, a.y);
}

DEV int decode_g1(const uint8_t *src, Fp &x, Fp &y) {
    const uint8_t f = src[0];
    if (f & 0xA0) return PT_BAD;                       // compressed / sort flags
    if (f & 0x40) return all_zero(src, 96, 0x1F) ? PT_INF : PT_BAD;
    Fp xr, yr;
    if (!load_be48(xr, src, 0x1FFFFFFFu) || !load_be48(yr, src + 48, 0xFFFFFFFFu)) return PT_BAD;
    to_mont(x, xr);
    to_mont(y, yr);
    Fp l, r, b;
    fp_sqr(l, y);
    fp_sqr(r, x);
    fp_mul(r, r, x);
    fp_set(b, kB1);
    fp_add(r, r, b);
    if (!fp_eq(l, r)) return PT_BAD;                   // y^2 = x^3 + 4
    return g1_in_subgroup(x, y) ? PT_OK : PT_BAD;      // order r (the crate's into_affine)
}

// the encoding and the curve equation only (no order-r check)
DEV int decode_g2_curve(const uint8_t *src, Fp2 &x, Fp2 &y) {
    const uint8_t f = src[0];
    if (f & 0xA0) return PT_BAD;
    if (f & 0x40) return all_zero(src, 192, 0x1F) ? PT_INF : PT_BAD;
    Fp a, b, c, d;
    if (!load_be48(a, src, 0x1FFFFFFFu) || !load_be48(b, src + 48, 0xFFFFFFFFu) ||
        !load_be48(c, src + 96, 0xFFFFFFFFu) || !load_be48(d, src + 144, 0xFFFFFFFFu))
        return PT_BAD;
    to_mont(x.c1, a);
    to_mont(x.c0, b);
    to_mont(y.c1, c);
    to_mont(y.c0, d);
    Fp2 l, r, bb;
    fp2_sqr(l, y);
    fp2_sqr(r, x);
    fp2_mul(r, r, x);
    fp_set(bb.c0, kB1);
    bb.c1 = bb.c0;                                     // 4 (u + 1)
    fp2_add(r, r, bb);
    return fp2_eq(l, r) ? PT_OK : PT_BAD;
}

DEV int decode_g2(const uint8_t *src, Fp2 &x, Fp2 &y) {
    const int st = decode_g2_curve(src, x, y);
    if (st != PT_OK) return st;
    return g2_in_subgroup(x, y) ? PT_OK : PT_BAD;
}

// Limb-major workspace: word w of pairing i at ws[w * n + i].
DEV void store_f12(uint32_t *ws, size_t n, size_t i, const Fp12 &f) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&f);
#pragma unroll 4
    for (int w = 0; w < 12 * NL; ++w) ws[(size_t)w * n + i] = src[w];
}

DEV void load_f12(Fp12 &f, const uint32_t *ws, size_t n, size_t i) {
    uint32_t *dst = reinterpret_cast<uint32_t *>(&f);
#pragma unroll 4
    for (int w = 0; w < 12 * NL; ++w) dst[w] = ws[(size_t)w * n + i];
}

constexpr int kPairBlock = 64;
// waves per SIMD of every pairing kernel (512 / kPairWpe VGPRs per lane).
// The 29-bit-limb product holds x, y, m and the output digits (56 VGPRs) on
// top of the tower operands: at 4 waves (128 VGPRs) the kernels spilled
// (1.02 M checks/s), at 2 waves (256 VGPRs) 1.57 M, at 1 wave 1.53 M (r3,
// tools/gpu_f4_wpe.sh)
constexpr int kPairWpe = 2;

// Kernel 1: one Miller loop per lane.  Pairing i takes G1 point g1[i] and G2
// point g2[i]; with `negate_odd`, odd pairings negate their G1 point (the
// c of a check a,b == c,d sits at pairing 2i+1).  status[i] gets the point
// status (max of the two); an infinity or invalid input leaves f = 1.
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void miller_kernel(
    const uint8_t *__restrict__ g1, size_t g1_stride, const uint8_t *__restrict__ g2,
    size_t g2_stride, size_t n, int pair_inputs, uint32_t *__restrict__ ws,
    uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n) return;
    // pair_inputs: pairing 2c reads (a_c, b_c) from the first halves of the
    // arrays, 2c+1 reads (c_c, d_c) from the second halves (see launcher)
    const uint8_t *p1 = g1 + i * g1_stride;
    const uint8_t *p2 = g2 + i * g2_stride;
    Fp xp, yp;
    Fp2 xq, yq;
    const int s1 = decode_g1(p1, xp, yp);
    const int s2 = decode_g2(p2, xq, yq);
    Fp12 f;
    fp12_one(f);
    const int st = s1 > s2 ? s1 : s2;
    if (st == PT_OK && s1 == PT_OK && s2 == PT_OK) {
        if (pair_inputs && (i & 1)) fp_neg(yp, yp);
        G2Proj T;
        T.x = xq;
        T.y = yq;
        fp_set(T.z.c0, kOne);
        fp_zero(T.z.c1);
        for (int b = 62; b >= 0; --b) {
            fp12_sqr(f, f);
            miller_dbl(T, f, xp, yp);
            if ((kXAbs >> b) & 1u) miller_add(T, f, xq, yq, xp, yp);
        }
        fp12_conj(f, f);
    }
    status[i] = (uint8_t)((s1 == PT_BAD || s2 == PT_BAD) ? PT_BAD : PT_OK);
    store_f12(ws, n, i, f);
}

// Kernel 1b: one lane per check e(a, b) == e(c, d) (g1 holds a, c and g2 b, d
// at rows 2i, 2i+1): the two Miller loops of f_a,b * f_-c,d share one
// squaring of f per step (a multi-Miller loop; the product is what the final
// exponentiation needs).  An infinity drops its pairing's lines (factor 1).
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void miller2_kernel(
    const uint8_t *__restrict__ g1, const uint8_t *__restrict__ g2, size_t count,
    uint32_t *__restrict__ ws, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= count) return;
    Fp xa, ya, xc, yc;
    Fp2 xb, yb, xd, yd;
    const int sa = decode_g1(g1 + (2 * i) * 96, xa, ya);
    const int sc = decode_g1(g1 + (2 * i + 1) * 96, xc, yc);
    const int sb = decode_g2(g2 + (2 * i) * 192, xb, yb);
    const int sd = decode_g2(g2 + (2 * i + 1) * 192, xd, yd);
    const bool bad = sa == PT_BAD || sb == PT_BAD || sc == PT_BAD || sd == PT_BAD;
    const bool on1 = !bad && sa == PT_OK && sb == PT_OK;
    const bool on2 = !bad && sc == PT_OK && sd == PT_OK;
    Fp12 f;
    fp12_one(f);
    if (on1 || on2) {
        fp_neg(yc, yc);   // e(-c, d) = e(c, d)^-1
        G2Proj T1, T2;
        T1.x = xb;
        T1.y = yb;
        fp_set(T1.z.c0, kOne);
        fp_zero(T1.z.c1);
        T2.x = xd;
        T2.y = yd;
        T2.z = T1.z;
        for (int b = 62; b >= 0; --b) {
            fp12_sqr(f, f);
            if (on1) miller_dbl(T1, f, xa, ya);
            if (on2) miller_dbl(T2, f, xc, yc);
            if ((kXAbs >> b) & 1u) {
                if (on1) miller_add(T1, f, xb, yb, xa, ya);
                if (on2) miller_add(T2, f, xd, yd, xc, yc);
            }
        }
        fp12_conj(f, f);
    }
    status[i] = bad ? PT_BAD : PT_OK;
    store_f12(ws, count, i, f);
}

// ---------------------------------------------------------------- prepared G2
// G2 points prepared once (the crate's G2Prepared): the 68 lines of the Miller
// loop over |x| (63 doublings, 5 additions) before evaluation at P, so every
// check against the same G2 point (hbbft: all N shares of a ciphertext share
// H and W) skips the twist arithmetic.  Table: point q, line s at
// prep + (q * kLines + s) * kLineWords words: L0, L1, L4 (Fp2, Montgomery).
constexpr int kLines = 68;
constexpr int kLineWords = 6 * NL;

DEV void store_line(uint32_t *dst, const Fp2 &l0, const Fp2 &l1, const Fp2 &l4) {
    const Fp *v[6] = {&l0.c0, &l0.c1, &l1.c0, &l1.c1, &l4.c0, &l4.c1};
#pragma unroll
    for (int e = 0; e < 6; ++e)
#pragma unroll
        for (int w = 0; w < NL; w += 4)
            *reinterpret_cast<uint4 *>(dst + e * NL + w) =
                make_uint4(v[e]->l[w], v[e]->l[w + 1], v[e]->l[w + 2], v[e]->l[w + 3]);
}

DEV void load_line(const uint32_t *src, Fp2 &l0, Fp2 &l1, Fp2 &l4) {
    Fp *v[6] = {&l0.c0, &l0.c1, &l1.c0, &l1.c1, &l4.c0, &l4.c1};
#pragma unroll
    for (int e = 0; e < 6; ++e)
#pragma unroll
        for (int w = 0; w < NL; w += 4) {
            const uint4 q = *reinterpret_cast<const uint4 *>(src + e * NL + w);
            v[e]->l[w] = q.x;
            v[e]->l[w + 1] = q.y;
            v[e]->l[w + 2] = q.z;
            v[e]->l[w + 3] = q.w;
        }
}

// The point's order-r check and its 68 lines are independent chains (the
// lines of a point that fails the check are never read: its status says
// invalid), so they run in two waves side by side -- block 2j checks points
// 64j.., block 2j + 1 computes their lines (the preparation's latency is the
// longer chain, not the sum; one ciphertext batch has only 8192 points, an
// eighth of a wave per SIMD).
//
// One lane per G2 point and role: its 68 lines, or its status (0 ok,
// 1 infinity, 2 invalid) at pst[q].
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void g2_prepare_kernel(
    const uint8_t *__restrict__ g2, size_t count, uint32_t *__restrict__ prep,
    uint8_t *__restrict__ pst) {
    const size_t q = (size_t)(blockIdx.x >> 1) * kPairBlock + threadIdx.x;
    if (q >= count) return;
    Fp2 xq, yq;
    if (!(blockIdx.x & 1)) {   // the status (wave-uniform role)
        pst[q] = (uint8_t)decode_g2(g2 + q * 192, xq, yq);
        return;
    }
    if (decode_g2_curve(g2 + q * 192, xq, yq) != PT_OK) return;
    G2Proj T;
    T.x = xq;
    T.y = yq;
    fp_set(T.z.c0, kOne);
    fp_zero(T.z.c1);
    uint32_t *dst = prep + q * (size_t)kLines * kLineWords;
    Fp2 l0, l1, l4;
    for (int b = 62; b >= 0; --b) {
        g2_dbl_line(T, l0, l1, l4);
        store_line(dst, l0, l1, l4);
        dst += kLineWords;
        if ((kXAbs >> b) & 1u) {
            g2_add_line(T, xq, yq, l0, l1, l4);
            store_line(dst, l0, l1, l4);
            dst += kLineWords;
        }
    }
}

// The prepared Miller loop's per-bit work as units of their own: the
// squaring with its Fp6 products inlined, and the line application with the
// sparse product inlined (their Fp6 operands do not pass through the stack;
// round 6: Miller 85.97 -> 80.0-80.5 ms per 262,144 checks, r6e).
NOINL void miller_sqr(Fp12 &f) { fp12_sqr_t<true>(f, f); }
NOINL void apply_prepared_in(Fp12 &f, const uint32_t *line, const Fp &xp, const Fp &yp) {
    Fp2 l0, l1, l4, a, b;
    load_line(line, l0, l1, l4);
    fp2_mul_fp(a, l1, xp);
    fp2_mul_fp(b, l4, yp);
    fp12_mul_by_014_in(f, l0, a, b);
}

// Prepared G1 keys: hbbft checks every decryption share against the public
// key share pk_i of its sender (threshold_decrypt.rs:220-228), and the
// validator set's N key shares are the same for every ciphertext of an epoch
// -- the crate holds them as curve points, so it decodes and checks them once,
// not per share.  One lane per key: decoded and checked like any G1 input
// (canonical coordinates, on the curve, order r), stored as Montgomery affine
// x || y (store_affine), status at kst[q] (0 ok, 1 infinity, 2 invalid).
//
// The body of the four table kernels (G1 keys and G2 points, from either wire
// form): one lane per point, `decode` (src + q * stride, x, y) giving the
// Montgomery affine coordinates and the status; zeros unless valid and finite.
template <class F, class Decode>
DEV void prepare_table(const uint8_t *src, size_t stride, size_t count, uint32_t *tab,
                       uint8_t *tst, Decode decode) {
    const size_t q = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (q >= count) return;
    F x, y;
    const int st = decode(src + q * stride, x, y);
    if (st != PT_OK) {
        fe_zero(x);
        fe_zero(y);
    }
    store_affine(tab + q * (2 * sizeof(F) / 4), x, y);
    tst[q] = (uint8_t)st;
}

// kG1PrepWpe: waves per SIMD of the G1 preparation (affine Fp points and
// their order-r checks need far fewer registers than the tower arithmetic)
constexpr int kG1PrepWpe = kPairWpe;
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kG1PrepWpe, kG1PrepWpe))) void g1_prepare_kernel(
    const uint8_t *__restrict__ g1, size_t count, uint32_t *__restrict__ keys,
    uint8_t *__restrict__ kst) {
    prepare_table<Fp>(g1, 96, count, keys, kst,
                      [](const uint8_t *p, Fp &x, Fp &y) { return decode_g1(p, x, y); });
}

// ------------------------------------------------- decryption-share combine
// ThresholdDecrypt's output step (threshold_decrypt.rs:232-252, try_output):
// `public_key_set().decrypt(shares, &ct)` is, in threshold_crypto, the
// Lagrange interpolation at 0 of the shares in G1,
//
//     g = sum_i lambda_i share_i,   x_i = node index + 1,
//     lambda_i = prod_{j != i} x_j / (x_j - x_i)   in Fr,
//
// followed by xor_with_hash(g, V) (the caller's).  Three kernels: the
// coefficients (one lane per share, Fr arithmetic), [lambda_i] share_i (one
// lane per share, the shares read decoded and checked from a g1_prepare
// table), and the sum of each group with its two encodings (one lane per
// group).  Groups are ragged: offsets[g] .. offsets[g + 1] of the flat share
// arrays.  Every read through `offsets` is clamped to the share count, so a
// malformed prefix sum gives wrong answers, never an out-of-bounds access.

// Fr: the 255-bit scalar field, 8 x 32-bit limbs, Montgomery form R = 2^256.
constexpr int NR = 8;
struct Fr { uint32_t l[NR]; };

DEV void fr_set(Fr &r, const uint32_t (&v)[NR]) {
#pragma unroll
    for (int i = 0; i < NR; ++i) r.l[i] = v[i];
}

DEV bool fr_is_zero(const Fr &a) {
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) t |= a.l[i];
    return t == 0;
}

// a < r (canonical)
DEV bool fr_is_canonical(const Fr &a) {
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) (void)subb(a.l[i], kFrR[i], br, &br);
    return br != 0;
}

DEV void fr_sub(Fr &r, const Fr &a, const Fr &b) {
    uint32_t t[NR];
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) t[i] = subb(a.l[i], b.l[i], br, &br);
    const uint32_t mask = 0u - br;  // add r back on borrow
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) r.l[i] = addc(t[i], kFrR[i] & mask, c, &c);
}

// Montgomery product a*b*2^-256 mod r (CIOS over 32-bit limbs; inputs < r,
// the sum stays below 2r < 2^256 and is reduced once)
DEV void fr_mul(Fr &r, const Fr &a, const Fr &b) {
    uint32_t t[NR + 1];
#pragma unroll
    for (int i = 0; i <= NR; ++i) t[i] = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            c += (uint64_t)a.l[j] * b.l[i] + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t[NR];
        t[NR] = (uint32_t)c;
        const uint32_t t9 = (uint32_t)(c >> 32);
        const uint32_t m = t[0] * kFrInv32;
        c = (uint64_t)m * kFrR[0] + t[0];   // low word becomes 0
        c >>= 32;
#pragma unroll
        for (int j = 1; j < NR; ++j) {
            c += (uint64_t)m * kFrR[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t[NR];
        t[NR - 1] = (uint32_t)c;
        t[NR] = t9 + (uint32_t)(c >> 32);
    }
    uint32_t s[NR];
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) s[i] = subb(t[i], kFrR[i], br, &br);
    const bool keep = br && !t[NR];   // t < r
#pragma unroll
    for (int i = 0; i < NR; ++i) r.l[i] = keep ? t[i] : s[i];
}

// canonical 64-bit value -> Montgomery form
DEV void fr_from_u64(Fr &r, uint64_t v) {
    Fr a, r2;
#pragma unroll
    for (int i = 0; i < NR; ++i) a.l[i] = 0;
    a.l[0] = (uint32_t)v;
    a.l[1] = (uint32_t)(v >> 32);
    fr_set(r2, kFrR2);
    fr_mul(r, a, r2);
}

// a^(r-2) (Fermat); once per coefficient
NOINL void fr_inv(Fr &r, const Fr &a) {
    Fr acc, base = a;
    fr_set(acc, kFrOne);
    for (int w = 0; w < NR; ++w) {
        uint32_t e = kFrMinus2[w];
        for (int b = 0; b < 32; ++b) {
            if (e & 1u) fr_mul(acc, acc, base);
            fr_mul(base, base, base);
            e >>= 1;
        }
    }
    r = acc;
}

// 32 big-endian bytes <-> limbs (little-endian words), canonical form
DEV void fr_load_be32(Fr &r, const uint8_t *src) {
#pragma unroll
    for (int w = 0; w < NR; ++w) {
        const uint8_t *q = src + 28 - 4 * w;
        r.l[w] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    }
}

DEV void fr_store_be32(uint8_t *dst, const Fr &a) {
#pragma unroll
    for (int w = 0; w < NR; ++w) {
        const uint32_t v = a.l[NR - 1 - w];
        dst[4 * w + 0] = (uint8_t)(v >> 24);
        dst[4 * w + 1] = (uint8_t)(v >> 16);
        dst[4 * w + 2] = (uint8_t)(v >> 8);
        dst[4 * w + 3] = (uint8_t)v;
    }
}

// Group statuses of the combine: CB_INF = ok and the sum is the point at
// infinity; CB_DUP = two equal node indices (the crate's DuplicateEntry)
enum { CB_OK = 0, CB_INF = 1, CB_BAD = 2, CB_DUP = 3 };

// the shares [b, e) of group g, clamped to the share count
DEV void group_range(const uint32_t *offsets, size_t g, size_t total, size_t &b, size_t &e) {
    const size_t hi = offsets[g + 1], lo = offsets[g];
    e = hi < total ? hi : total;
    b = lo < e ? lo : e;
}

// Kernel: one lane per (group, share).  Share j of group g (found by binary
// search in the prefix sum) forms x = idx + 1 in 64 bits (idx = 0xFFFFFFFF is
// x = 2^32, not 0) and writes lambda_j as 32 canonical big-endian bytes.  A
// zero denominator is a repeated index: status 3 for the group (the caller
// clears `status` before the launch; only failing lanes write), zero bytes
// for the coefficient.
__global__ __launch_bounds__(kPairBlock) void lagrange_kernel(
    const uint32_t *__restrict__ idx, const uint32_t *__restrict__ offsets, size_t groups,
    size_t total, uint8_t *__restrict__ coeffs, uint8_t *__restrict__ status) {
    const size_t j = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (j >= total) return;
    uint8_t *dst = coeffs + 32 * j;
    size_t lo = 0, hi = groups;   // the first group starting past j
    while (lo < hi) {
        const size_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= j) lo = mid + 1; else hi = mid;
    }
    size_t b = 0, e = 0;
    if (lo > 0) group_range(offsets, lo - 1, total, b, e);
    Fr lam;
#pragma unroll
    for (int i = 0; i < NR; ++i) lam.l[i] = 0;
    if (j >= b && j < e) {   // else: malformed offsets, share in no group
        Fr xi, num, den;
        fr_from_u64(xi, (uint64_t)idx[j] + 1);
        fr_set(num, kFrOne);
        fr_set(den, kFrOne);
        for (size_t k = b; k < e; ++k) {
            if (k == j) continue;
            Fr xk, d;
            fr_from_u64(xk, (uint64_t)idx[k] + 1);
            fr_sub(d, xk, xi);
            fr_mul(num, num, xk);
            fr_mul(den, den, d);
        }
        if (fr_is_zero(den)) {
            status[lo - 1] = CB_DUP;
        } else {
            Fr one;
            fr_inv(den, den);
            fr_mul(lam, num, den);
#pragma unroll
            for (int i = 0; i < NR; ++i) one.l[i] = 0;
            one.l[0] = 1;
            fr_mul(lam, lam, one);   // out of Montgomery form
        }
    }
    fr_store_be32(dst, lam);
}

// k <<= 1
DEV void fr_shl1(Fr &k) {
#pragma unroll
    for (int i = NR - 1; i > 0; --i) k.l[i] = (k.l[i] << 1) | (k.l[i - 1] >> 31);
    k.l[0] <<= 1;
}

// k = k1 + k2 x^2, k < r: bit-serial long division by the 128-bit x^2 (a few
// thousand integer operations against a million in the curve arithmetic)
DEV void glv_split(Fr k, uint64_t &k1hi, uint64_t &k1lo, uint64_t &k2hi, uint64_t &k2lo) {
    uint64_t rhi = 0, rlo = 0, qhi = 0, qlo = 0;
    fr_shl1(k);   // bit 254 to the top
    for (int b = 254; b >= 0; --b) {
        const uint64_t bit = k.l[NR - 1] >> 31;
        fr_shl1(k);
        const uint64_t carry = rhi >> 63;   // the remainder doubled may reach 2^128
        rhi = (rhi << 1) | (rlo >> 63);
        rlo = (rlo << 1) | bit;
        const bool ge = carry || rhi > kXSqHi || (rhi == kXSqHi && rlo >= kXSqLo);
        if (ge) {
            const uint64_t borrow = rlo < kXSqLo;
            rlo -= kXSqLo;
            rhi -= kXSqHi + borrow;
        }
        qhi = (qhi << 1) | (qlo >> 63);
        qlo = (qlo << 1) | (ge ? 1u : 0u);
    }
    k1hi = rhi;
    k1lo = rlo;
    k2hi = qhi;
    k2lo = qlo;
}

// the next digit of the joint chain, most significant first: bit 0 from k1,
// bit 1 from k2 (0 none, 1 P, 2 Q, 3 P + Q); the halves shift left
DEV unsigned glv_digit(uint64_t &k1hi, uint64_t &k1lo, uint64_t &k2hi, uint64_t &k2lo) {
    const unsigned sel = (unsigned)(k1hi >> 63) | ((unsigned)(k2hi >> 63) << 1);
    k1hi = (k1hi << 1) | (k1lo >> 63);
    k1lo <<= 1;
    k2hi = (k2hi << 1) | (k2lo >> 63);
    k2lo <<= 1;
    return sel;
}

// [x^2] (x, y) by the endomorphism: (beta x, -y) on G1; on G2 psi(Q) = [x] Q
// (g2_in_subgroup above), so psi^2(Q) = (gamma x, -y) = [x^2] Q with gamma in
// Fp (bls_consts.hpp) -- no sign flip, unlike phi on G1, and the same shape
// of operand.
DEV void glv_endo(Fp &qx, Fp &qy, const Fp &x, const Fp &y) {
    fp_set(qx, kBeta);
    fp_mul(qx, qx, x);
    fp_neg(qy, y);
}
DEV void glv_endo(Fp2 &qx, Fp2 &qy, const Fp2 &x, const Fp2 &y) {
    Fp gamma;
    fp_set(gamma, kGammaG2);
    fp2_mul_fp(qx, x, gamma);
    fp2_neg(qy, y);
}

// The scalar multiplication of both groups goes through the endomorphism (it
// won its A/Bs against plain double-and-add over 255 bits).
// phi(P) = (beta x, y) = -[x^2] P on G1 (g1_in_subgroup above), so with
// k = k1 + k2 x^2 (k1 < x^2 by plain long division; k2 < 2^128 because
// k < r = x^4 - x^2 + 1)
//     [k] P = [k1] P + [k2] Q,   Q = [x^2] P = (beta x, -y),
// two 128-bit halves on one doubling chain.  Per bit the lane adds P, Q or
// P + Q, chosen by the two bits, through one call of the projective addition
// with a selected operand: lanes with different bits do not serialise three
// additions, and a wave pays 128 doublings and 128 additions where the plain
// loop with per-lane scalars pays 255 and nearly 255.
//
// acc = [k] (x, y), k < r.  The complete formulas take the identity as a start
// value and any intermediate sum, so there is no leading-bit search and no
// special case; k = 0 gives the identity.
template <class F>
DEV void pt_mul_glv(PtProj<F> &acc, const F &x, const F &y, const Fr &k) {
    pt_identity(acc);
    uint64_t k1hi, k1lo, k2hi, k2lo;
    glv_split(k, k1hi, k1lo, k2hi, k2lo);
    PtProj<F> pp, qq, tt;   // P, Q = [x^2] P, P + Q
    pp.x = x;
    pp.y = y;
    fe_one(pp.z);
    glv_endo(qq.x, qq.y, x, y);
    qq.z = pp.z;
    tt = pp;
    pt_add_proj(tt, qq);
    const uint32_t *wp = reinterpret_cast<const uint32_t *>(&pp);
    const uint32_t *wq = reinterpret_cast<const uint32_t *>(&qq);
    const uint32_t *wt = reinterpret_cast<const uint32_t *>(&tt);
    for (int b = 127; b >= 0; --b) {
        pt_dbl(acc);
        const unsigned sel = glv_digit(k1hi, k1lo, k2hi, k2lo);
        if (sel) {
            PtProj<F> op;
            uint32_t *wo = reinterpret_cast<uint32_t *>(&op);
#pragma unroll
            for (int w = 0; w < (int)(sizeof(PtProj<F>) / 4); ++w)
                wo[w] = sel == 1 ? wp[w] : (sel == 2 ? wq[w] : wt[w]);
            pt_add_proj(acc, op);
        }
    }
}

// Kernel: one lane per share, [k_j] P_j (pt_mul_glv).
// P_j = row rows[j] of a g1_prepare table of `nprep` points, k_j = 32
// big-endian bytes.  k = 0 and a table entry at infinity give the identity;
// k >= r, an invalid table entry and a row outside the table give pst = 2.
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kG1PrepWpe, kG1PrepWpe))) void g1_scalar_mul_kernel(
    const uint32_t *__restrict__ tab, const uint8_t *__restrict__ tst, size_t nprep,
    const int32_t *__restrict__ rows, const uint8_t *__restrict__ scalars, size_t total,
    uint32_t *__restrict__ ws, uint8_t *__restrict__ pst) {
    const size_t j = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (j >= total) return;
    const int32_t row = rows[j];
    // a row past the table is an invalid input, never an out-of-bounds read
    int st = (row >= 0 && (size_t)row < nprep) ? tst[row] : PT_BAD;
    Fr k;
    fr_load_be32(k, scalars + 32 * j);
    if (!fr_is_canonical(k)) st = PT_BAD;
    PtProj<Fp> acc;
    if (st == PT_OK) {
        Fp x, y;
        load_affine(tab + (size_t)row * kG1KeyWords, x, y);
        pt_mul_glv(acc, x, y, k);
    } else {
        pt_identity(acc);
    }
    pst[j] = (uint8_t)(st == PT_BAD ? PT_BAD : PT_OK);
    store_pt(ws, total, j, acc);
}

// 48 big-endian bytes of a canonical (non-Montgomery) value, `flags` or-ed
// into byte 0
DEV void store_be48_raw(uint8_t *dst, const Fp &c, uint8_t flags) {
#pragma unroll
    for (int w = 0; w < NL; ++w) {
        const uint32_t v = c.l[NL - 1 - w];
        dst[4 * w + 0] = (uint8_t)(v >> 24);
        dst[4 * w + 1] = (uint8_t)(v >> 16);
        dst[4 * w + 2] = (uint8_t)(v >> 8);
        dst[4 * w + 3] = (uint8_t)v;
    }
    dst[0] |= flags;
}

// sign of y - (-y) as integers for a canonical (non-Montgomery) y, -0 = 0: the
// comparison behind the 0x20 flag of the compressed encodings
DEV int fp_cmp_neg(const Fp &yc) {
    Fp nc;
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) nc.l[i] = subb(kP[i], yc.l[i], br, &br);
    if (fp_is_zero(yc)) nc = yc;
    int cmp = 0;
#pragma unroll
    for (int i = NL - 1; i >= 0; --i)
        if (cmp == 0 && yc.l[i] != nc.l[i]) cmp = yc.l[i] > nc.l[i] ? 1 : -1;
    return cmp;
}

// A projective result to affine with one inversion: (xm, ym) Montgomery
// (zero for infinity) and, where the pointers are non-null, the two encodings
// described below into buffers the caller has zeroed.  Returns CB_OK or CB_INF.
DEV int g1_affine_encode(const PtProj<Fp> &acc, Fp &xm, Fp &ym, uint8_t *o96, uint8_t *o48) {
    if (fp_is_zero(acc.z)) {
        fp_zero(xm);
        fp_zero(ym);
        if (o96) o96[0] = 0x40;
        if (o48) o48[0] = 0xC0;
        return CB_INF;
    }
    Fp zi, x, y;
    fp_inv(zi, acc.z);
    fp_mul(xm, acc.x, zi);
    fp_mul(ym, acc.y, zi);
    if (!o96 && !o48) return CB_OK;
    from_mont(x, xm);
    from_mont(y, ym);
    if (o96) {
        store_be48_raw(o96, x, 0);
        store_be48_raw(o96 + 48, y, 0);
    }
    if (o48) store_be48_raw(o48, x, (uint8_t)(0x80 | (fp_cmp_neg(y) > 0 ? 0x20 : 0)));
    return CB_OK;
}

// canonical affine (x, y) on the twist as x.c1 || x.c0 || y.c1 || y.c0
DEV void g2_store_be192(uint8_t *o192, const Fp2 &x, const Fp2 &y) {
    store_be48_raw(o192, x.c1, 0);
    store_be48_raw(o192 + 48, x.c0, 0);
    store_be48_raw(o192 + 96, y.c1, 0);
    store_be48_raw(o192 + 144, y.c0, 0);
}
DEV void fp2_from_mont(Fp2 &r, const Fp2 &a) { from_mont(r.c0, a.c0); from_mont(r.c1, a.c1); }

// The G2 flavour, always with both encodings (into zeroed buffers) and the
// parity byte: the XOR of all bits of the uncompressed encoding.  y against
// -y by c1 first, by c0 only when the c1 are equal.
DEV int g2_affine_encode(const PtProj<Fp2> &acc, uint8_t *o192, uint8_t *o96, uint8_t &par) {
    if (fp2_is_zero(acc.z)) {
        o192[0] = 0x40;
        o96[0] = 0xC0;
        par = 1;
        return CB_INF;
    }
    Fp2 zi, x, y;
    fp2_inv(zi, acc.z);
    fp2_mul(x, acc.x, zi);
    fp2_mul(y, acc.y, zi);
    fp2_from_mont(x, x);
    fp2_from_mont(y, y);
    int cmp = fp_cmp_neg(y.c1);
    if (cmp == 0) cmp = fp_cmp_neg(y.c0);
    g2_store_be192(o192, x, y);
    store_be48_raw(o96, x.c1, (uint8_t)(0x80 | (cmp > 0 ? 0x20 : 0)));
    store_be48_raw(o96 + 48, x.c0, 0);
    uint32_t acc32 = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) acc32 ^= x.c0.l[i] ^ x.c1.l[i] ^ y.c0.l[i] ^ y.c1.l[i];
    par = (uint8_t)(__popc(acc32) & 1);
    return CB_OK;
}

// The front of the two reduce kernels, one lane per group g: the status from
// the Lagrange kernel (`lst`, may be null) and the group's shares, and for an
// ok group the sum of its projective points in acc.
template <class F>
DEV int reduce_group(PtProj<F> &acc, const uint32_t *ws, const uint8_t *pst,
                     const uint32_t *offsets, size_t g, size_t total, const uint8_t *lst) {
    size_t b, e;
    group_range(offsets, g, total, b, e);
    int st = (lst && lst[g] == CB_DUP) ? CB_DUP : CB_OK;
    if (st == CB_OK)
        for (size_t k = b; k < e; ++k)
            if (pst[k] == PT_BAD) st = CB_BAD;
    if (st != CB_OK) return st;
    PtProj<F> q;
    pt_identity(acc);
    for (size_t k = b; k < e; ++k) {
        load_pt(q, ws, total, k);
        pt_add_proj(acc, q);
    }
    return CB_OK;
}

// Kernel: one lane per group.  Sums the group's projective points, converts
// to affine with one inversion and writes the uncompressed encoding (96
// bytes, x || y) and the compressed one (48 bytes: x with 0x80 set, 0x20 set
// iff y > p - y as integers; infinity = 0xC0 and zeros) -- zkcrypto's
// G1Uncompressed / G1Compressed.  status: 0 ok, 1 ok and the sum is the
// point at infinity, 2 an invalid share / scalar / row in the group, 3 a
// repeated index (`lst`, from lagrange_kernel; may be null); for 2 and 3
// both outputs are zero bytes.  An empty group is the empty sum: status 1.
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kG1PrepWpe, kG1PrepWpe))) void g1_reduce_encode_kernel(
    const uint32_t *__restrict__ ws, const uint8_t *__restrict__ pst,
    const uint32_t *__restrict__ offsets, size_t groups, size_t total,
    const uint8_t *__restrict__ lst, uint8_t *__restrict__ out96, uint8_t *__restrict__ out48,
    uint8_t *__restrict__ status) {
    const size_t g = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (g >= groups) return;
    uint8_t *o96 = out96 + 96 * g, *o48 = out48 + 48 * g;
    for (int i = 0; i < 96; ++i) o96[i] = 0;
    for (int i = 0; i < 48; ++i) o48[i] = 0;
    PtProj<Fp> acc;
    Fp xm, ym;
    int st = reduce_group(acc, ws, pst, offsets, g, total, lst);
    if (st == CB_OK) st = g1_affine_encode(acc, xm, ym, o96, o48);
    status[g] = (uint8_t)st;
}

// ------------------------------------------------------------ key generation
// SyncKeyGen (sync_key_gen.rs) evaluates G1 commitments at node indices:
// `commit.row(our_idx + 1)` per Part (:557), `commit.evaluate(our_idx + 1,
// sender_idx + 1)` per Ack (:603), `commit.row(0)` summed in `generate`
// (:516-534), and `PublicKeySet::public_key_share(i)` = `commit.evaluate(i +
// 1)` for the key shares every share check reads.  The evaluation points are
// integers of a few bits, so Horner's rule needs bits(x) doublings per
// coefficient where a linear combination with scalars x^k mod r pays a
// 128-step GLV multiplication per term.
//
// Kernel: one lane per evaluation e of polynomial poly[e] at x[e] (the raw
// point: the crate's IntoFr of an integer, not index + 1).  Polynomial p has
// the coefficients T[rows[offsets[p] .. offsets[p + 1])] of a g1_prepare
// table, constant term first; degrees are ragged and the row count is
// offsets[polys], to which every range is clamped.  From acc = identity, for
// k from the top coefficient down: acc = [x] acc (left-to-right double-and-
// add over the 32 - clz(x) significant bits on a copy of acc, which stands
// for the leading one: complete formulas, no special cases -- no bits give
// the identity, so x = 0 yields C_0, and x = 1 the plain sum), then acc +=
// C_k by the mixed addition (a coefficient at infinity is skipped).  Loop bounds are per lane: lanes of a wave may differ in degree
// and bit length.  An invalid coefficient, a row outside the table or a poly
// outside [0, polys) gives status 2.
// The result goes out in g1_prepare table form (Montgomery affine x || y,
// zero unless the status is 0; status byte 0 ok, 1 infinity, 2 invalid), so
// it serves as the table of a second evaluation or of the check below, and,
// where out96 / out48 are non-null, in the encodings of the combine.
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kG1PrepWpe, kG1PrepWpe))) void g1_horner_kernel(
    const uint32_t *__restrict__ tab, const uint8_t *__restrict__ tst, size_t nprep,
    const int32_t *__restrict__ rows, const uint32_t *__restrict__ offsets, size_t polys,
    const int32_t *__restrict__ poly, const uint32_t *__restrict__ xs, size_t evals,
    uint32_t *__restrict__ otab, uint8_t *__restrict__ ost, uint8_t *__restrict__ out96,
    uint8_t *__restrict__ out48, uint8_t *__restrict__ status) {
    const size_t e = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (e >= evals) return;
    const int32_t p = poly[e];
    const uint32_t xv = xs[e];
    const int nbits = xv ? 32 - __builtin_clz(xv) : 0;
    int st = PT_OK;
    size_t b = 0, en = 0;
    if (p >= 0 && (size_t)p < polys)
        group_range(offsets, (size_t)p, offsets[polys], b, en);
    else
        st = PT_BAD;
    PtProj<Fp> acc;
    pt_identity(acc);
    for (size_t k = en; k > b && st == PT_OK; --k) {
        if (k != en) {   // [x] acc; the top coefficient starts from the identity
            PtProj<Fp> t = acc;   // the leading one of x
            if (nbits == 0) pt_identity(t);
            for (int bit = nbits - 2; bit >= 0; --bit) {
                pt_dbl(t);
                if ((xv >> bit) & 1u) pt_add_proj(t, acc);
            }
            acc = t;
        }
        const int32_t row = rows[k - 1];
        const int cst = (row >= 0 && (size_t)row < nprep) ? tst[row] : PT_BAD;
        if (cst == PT_OK) {
            Fp cx, cy;
            load_affine(tab + (size_t)row * kG1KeyWords, cx, cy);
            pt_add_affine(acc, cx, cy);
        } else if (cst != PT_INF) {
            st = PT_BAD;
        }
    }
    uint8_t *o96 = out96 ? out96 + 96 * e : nullptr, *o48 = out48 ? out48 + 48 * e : nullptr;
    if (o96)
        for (int i = 0; i < 96; ++i) o96[i] = 0;
    if (o48)
        for (int i = 0; i < 48; ++i) o48[i] = 0;
    Fp xm, ym;
    if (st == PT_OK) {
        st = g1_affine_encode(acc, xm, ym, o96, o48);   // CB_OK / CB_INF = PT_OK / PT_INF
    } else {
        fp_zero(xm);
        fp_zero(ym);
    }
    store_affine(otab + e * kG1KeyWords, xm, ym);
    ost[e] = (uint8_t)st;
    status[e] = (uint8_t)st;
}

// Kernel: one lane per check [s_i] G1::one() == T[rows[i]] -- the
// `row.commitment() != commit_row` of a Part (sync_key_gen.rs:569, one check
// per coefficient) and the `G1Affine::one().mul(val)` of an Ack (:603).  s is
// 32 big-endian bytes; the multiplication is the GLV loop of
// g1_scalar_mul_kernel with P = G1::one(), Q = [x^2] P and P + Q as affine
// constants (the mixed addition with a selected operand), the comparison
// projective against affine: X == x Z, Y == y Z, Z != 0; a table entry at
// infinity equals a result at infinity.  ok: 1 equal, 0 not, 2 for an invalid
// table entry, a row outside the table or s >= r.
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kG1PrepWpe, kG1PrepWpe))) void g1_base_mul_check_kernel(
    const uint32_t *__restrict__ tab, const uint8_t *__restrict__ tst, size_t nprep,
    const int32_t *__restrict__ rows, const uint8_t *__restrict__ scalars, size_t count,
    uint8_t *__restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= count) return;
    const int32_t row = rows[i];
    int st = (row >= 0 && (size_t)row < nprep) ? tst[row] : PT_BAD;
    Fr k;
    fr_load_be32(k, scalars + 32 * i);
    if (!fr_is_canonical(k)) st = PT_BAD;
    if (st == PT_BAD) {
        ok[i] = 2;
        return;
    }
    uint64_t k1hi, k1lo, k2hi, k2lo;
    glv_split(k, k1hi, k1lo, k2hi, k2lo);
    PtProj<Fp> acc;
    pt_identity(acc);
    for (int b = 127; b >= 0; --b) {
        pt_dbl(acc);
        const unsigned sel = glv_digit(k1hi, k1lo, k2hi, k2lo);
        if (sel) {
            Fp ox, oy;
#pragma unroll
            for (int w = 0; w < NL; ++w) {
                ox.l[w] = sel == 1 ? kG1GenX[w] : (sel == 2 ? kG1GenQX[w] : kG1GenTX[w]);
                oy.l[w] = sel == 1 ? kG1GenY[w] : (sel == 2 ? kG1GenNegY[w] : kG1GenTY[w]);
            }
            pt_add_affine(acc, ox, oy);
        }
    }
    bool eq;
    if (st == PT_INF) {
        eq = fp_is_zero(acc.z);
    } else {
        Fp x, y, l, r;
        load_affine(tab + (size_t)row * kG1KeyWords, x, y);
        fp_mul(l, x, acc.z);
        fp_mul(r, y, acc.z);
        eq = !fp_is_zero(acc.z) && fp_eq(l, acc.x) && fp_eq(r, acc.y);
    }
    ok[i] = eq ? 1 : 0;
}

// One lane per check e(a, b) == e(c, d) with b, d prepared (points ib[i],
// id[i] of the table): g1 holds a, c at rows 2i, 2i+1.  Lanes of a wave
// checking against the same points read the same lines (one cache line
// serves the wave).
// KEYS: c comes from a table of prepared G1 keys (g1_prepare_kernel) by
// index ic[i] and g1 holds only a_0, a_1, ...; otherwise g1 holds a_0, c_0,
// a_1, c_1, ... and both points of a check are decoded here.
// PTS (with KEYS): a also comes decoded, from a g1_prepare table of the
// `count` shares (entry i, statuses `ast`), so the share decoding -- an
// order-r check each -- runs as its own launch beside the G2 preparation.
template <bool KEYS, bool PTS = false>
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void miller_prepared_kernel(
    const uint8_t *__restrict__ g1, const uint32_t *__restrict__ keys,
    const uint8_t *__restrict__ kst, const uint32_t *__restrict__ ic, size_t nkeys,
    const uint32_t *__restrict__ prep,
    const uint8_t *__restrict__ pst, const uint32_t *__restrict__ ib,
    const uint32_t *__restrict__ id, size_t points, size_t count, uint32_t *__restrict__ ws,
    uint8_t *__restrict__ status, const uint32_t *__restrict__ atab = nullptr,
    const uint8_t *__restrict__ ast = nullptr) {
    const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= count) return;
    Fp xa, ya, xc, yc;
    int sa, sc;
    if constexpr (KEYS) {
        if constexpr (PTS) {
            sa = ast[i];
            load_affine(atab + i * kG1KeyWords, xa, ya);   // zeros unless the point is valid
        } else {
            sa = decode_g1(g1 + i * 96, xa, ya);
        }
        const uint32_t qc = ic[i];
        // an index past the key table is an invalid input, never an out-of-bounds read
        sc = qc < nkeys ? kst[qc] : PT_BAD;
        if (sc == PT_OK) {
            load_affine(keys + (size_t)qc * kG1KeyWords, xc, yc);
        } else {
            fp_zero(xc);
            fp_zero(yc);
        }
    } else {
        sa = decode_g1(g1 + (2 * i) * 96, xa, ya);
        sc = decode_g1(g1 + (2 * i + 1) * 96, xc, yc);
    }
    uint32_t qb = ib[i], qd = id[i];
    // an index past the table is an invalid input, never an out-of-bounds read
    const bool range_ok = qb < points && qd < points;
    if (!range_ok) qb = qd = 0;
    const int sb = range_ok ? pst[qb] : PT_BAD, sd = range_ok ? pst[qd] : PT_BAD;
    const bool bad = sa == PT_BAD || sb == PT_BAD || sc == PT_BAD || sd == PT_BAD;
    const bool on1 = !bad && sa == PT_OK && sb == PT_OK;
    const bool on2 = !bad && sc == PT_OK && sd == PT_OK;
    Fp12 f;
    fp12_one(f);
    if (on1 || on2) {
        fp_neg(yc, yc);   // e(-c, d) = e(c, d)^-1
        const uint32_t *p1 = prep + (size_t)qb * kLines * kLineWords;
        const uint32_t *p2 = prep + (size_t)qd * kLines * kLineWords;
        for (int b = 62; b >= 0; --b) {
            miller_sqr(f);
            if (on1) apply_prepared_in(f, p1, xa, ya);
            if (on2) apply_prepared_in(f, p2, xc, yc);
            p1 += kLineWords;
            p2 += kLineWords;
            if ((kXAbs >> b) & 1u) {
                if (on1) apply_prepared_in(f, p1, xa, ya);
                if (on2) apply_prepared_in(f, p2, xc, yc);
                p1 += kLineWords;
                p2 += kLineWords;
            }
        }
        fp12_conj(f, f);
    }
    status[i] = bad ? PT_BAD : PT_OK;
    store_f12(ws, count, i, f);
}

// ------------------------------------------------- threshold signatures
// ThresholdSign, the common coin of BinaryAgreement (threshold_sign.rs): every
// received share is checked with `pk_i.verify_g2(share, H)` (:216-225),
//
//     e(pk_i, H) == e(G1::one(), share_i),     H = hash_g2(doc),
//
// and more than num_faulty valid shares are combined by the Lagrange
// interpolation at 0 in G2 (`combine_signatures`, :249-270), the result being
// checked once more against the master public key.  The G2 point on the right
// differs per share, so it cannot come from the prepared-lines table: the
// shares are decoded and order-checked once into a table of affine points
// (g2_points_kernel, the G2 twin of g1_prepare_kernel), from which the check
// walks its twist chain and the combine takes its operands.
// One lane per G2 point: decoded and checked (canonical coordinates, on the
// twist, order r), stored as Montgomery affine coordinates (zeros unless the
// point is valid and finite), status at gst[q] (0 ok, 1 infinity, 2 invalid).
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void g2_points_kernel(
    const uint8_t *__restrict__ g2, size_t count, uint32_t *__restrict__ tab,
    uint8_t *__restrict__ gst) {
    prepare_table<Fp2>(g2, 192, count, tab, gst,
                       [](const uint8_t *p, Fp2 &x, Fp2 &y) { return decode_g2(p, x, y); });
}

// One lane per check e(K[ic[i]], P[ih[i]]) == e(G1::one(), S[i]), evaluated as
// f_{K,P} * f_{-G1::one(),S}.  Leg 1 is the c leg of miller_prepared_kernel:
// the key from a g1_prepare table, the lines of P from a g2_prepare table
// (lanes of a wave checking one document read the same lines).  Leg 2 walks
// T from S[i], entry i of a g2_points table of `nsig` points, and applies its
// lines at the constant -G1::one().  Both legs share one squaring of f per
// bit.  An invalid point, an index past its table or i >= nsig gives status 2;
// an infinity drops its leg.
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void miller_sig_kernel(
    const uint32_t *__restrict__ stab, const uint8_t *__restrict__ sst, size_t nsig,
    const uint32_t *__restrict__ keys, const uint8_t *__restrict__ kst,
    const uint32_t *__restrict__ ic, size_t nkeys, const uint32_t *__restrict__ prep,
    const uint8_t *__restrict__ pst, const uint32_t *__restrict__ ih, size_t points, size_t count,
    uint32_t *__restrict__ ws, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= count) return;
    // an index past its table is an invalid input, never an out-of-bounds read
    const uint32_t qk = ic[i];
    uint32_t qh = ih[i];
    const int sk = qk < nkeys ? kst[qk] : PT_BAD;
    const int sh = qh < points ? pst[qh] : PT_BAD;
    const int ss = i < nsig ? sst[i] : PT_BAD;
    if (qh >= points) qh = 0;
    Fp xk, yk;
    if (sk == PT_OK) {
        load_affine(keys + (size_t)qk * kG1KeyWords, xk, yk);
    } else {
        fp_zero(xk);
        fp_zero(yk);
    }
    const bool bad = sk == PT_BAD || sh == PT_BAD || ss == PT_BAD;
    const bool on1 = !bad && sk == PT_OK && sh == PT_OK;
    const bool on2 = !bad && ss == PT_OK;
    Fp12 f;
    fp12_one(f);
    if (on1 || on2) {
        Fp gx, gy;
        fp_set(gx, kG1GenX);
        fp_set(gy, kG1GenNegY);   // e(-G1::one(), S) = e(G1::one(), S)^-1
        Fp2 xs, ys;
        G2Proj T;
        if (on2) {
            load_affine(stab + i * kG2PtWords, xs, ys);
        } else {
            fp2_zero(xs);
            fp2_zero(ys);
        }
        T.x = xs;
        T.y = ys;
        fp_set(T.z.c0, kOne);
        fp_zero(T.z.c1);
        const uint32_t *p1 = prep + (size_t)qh * kLines * kLineWords;
        for (int b = 62; b >= 0; --b) {
            miller_sqr(f);
            if (on1) apply_prepared_in(f, p1, xk, yk);
            if (on2) miller_dbl(T, f, gx, gy);
            p1 += kLineWords;
            if ((kXAbs >> b) & 1u) {
                if (on1) apply_prepared_in(f, p1, xk, yk);
                if (on2) miller_add(T, f, xs, ys, gx, gy);
                p1 += kLineWords;
            }
        }
        fp12_conj(f, f);
    }
    status[i] = bad ? PT_BAD : PT_OK;
    store_f12(ws, count, i, f);
}

// Kernel: one lane per share, [k_j] Q_j (pt_mul_glv).  Q_j = row rows[j] of a g2_points
// table of `nprep` points, k_j = 32 big-endian bytes.  k = 0 and a table entry
// at infinity give the identity; k >= r, an invalid table entry and a row
// outside the table give pst = 2.
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void g2_scalar_mul_kernel(
    const uint32_t *__restrict__ tab, const uint8_t *__restrict__ tst, size_t nprep,
    const int32_t *__restrict__ rows, const uint8_t *__restrict__ scalars, size_t total,
    uint32_t *__restrict__ ws, uint8_t *__restrict__ pst) {
    const size_t j = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (j >= total) return;
    const int32_t row = rows[j];
    // a row past the table is an invalid input, never an out-of-bounds read
    int st = (row >= 0 && (size_t)row < nprep) ? tst[row] : PT_BAD;
    Fr k;
    fr_load_be32(k, scalars + 32 * j);
    if (!fr_is_canonical(k)) st = PT_BAD;
    PtProj<Fp2> acc;
    if (st == PT_OK) {
        Fp2 x, y;
        load_affine(tab + (size_t)row * kG2PtWords, x, y);
        pt_mul_glv(acc, x, y, k);
    } else {
        pt_identity(acc);
    }
    pst[j] = (uint8_t)(st == PT_BAD ? PT_BAD : PT_OK);
    store_pt(ws, total, j, acc);
}

// Kernel: one lane per group.  Sums the group's projective points, converts
// to affine with one Fp2 inversion and writes the uncompressed encoding (192
// bytes, x.c1 || x.c0 || y.c1 || y.c0), the compressed one (96 bytes: x.c1 ||
// x.c0 with 0x80 set, 0x20 set iff y is the larger of y and -y, c1 compared
// first and c0 only when the c1 are equal; infinity = 0xC0 and zeros) --
// zkcrypto's G2Uncompressed / G2Compressed -- and the parity byte: the XOR of
// all bits of the uncompressed encoding (threshold_crypto's
// Signature::parity(), the coin).  status as g1_reduce_encode_kernel; for 2
// and 3 all three outputs are zero bytes.  An empty group is status 1.
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void g2_reduce_encode_kernel(
    const uint32_t *__restrict__ ws, const uint8_t *__restrict__ pst,
    const uint32_t *__restrict__ offsets, size_t groups, size_t total,
    const uint8_t *__restrict__ lst, uint8_t *__restrict__ out192, uint8_t *__restrict__ out96,
    uint8_t *__restrict__ parity, uint8_t *__restrict__ status) {
    const size_t g = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (g >= groups) return;
    uint8_t *o192 = out192 + 192 * g, *o96 = out96 + 96 * g;
    for (int i = 0; i < 192; ++i) o192[i] = 0;
    for (int i = 0; i < 96; ++i) o96[i] = 0;
    uint8_t par = 0;
    PtProj<Fp2> acc;
    int st = reduce_group(acc, ws, pst, offsets, g, total, lst);
    if (st == CB_OK) st = g2_affine_encode(acc, o192, o96, par);
    parity[g] = par;
    status[g] = (uint8_t)st;
}

// ------------------------------------------------------------ share creation
// What a node does to send: `decrypt_share_no_verify` ([sk_i] U,
// threshold_decrypt.rs:161), `sign_g2` ([sk_i] H, threshold_sign.rs:167), the
// dealer's `BivarPoly::commitment()` and `SecretKeyShare::public_key_share`
// ([s] G1::one()), and SyncKeyGen's Fr side: `our_part.row(i + 1)`
// (sync_key_gen.rs:413-417), `row.evaluate(idx + 1)` (:459) and the
// interpolation of `generate` (:523-524).  The multiplications are the GLV
// loops above with the result kept on the device: one inversion per lane, the
// affine point written as an entry of a g1_prepare / g2_points table (bit for
// bit what the decoders give for the result's bytes: every field operation
// returns the canonical representative, and a product of a checked point stays
// in the order-r subgroup, so no second check is due) and, where asked, in the
// wire encodings.  The loops branch on scalar bits: not constant-time, meant
// for simulations and test networks that hold every node's secrets anyway.

// The G2 twin of g1_affine_encode: Montgomery affine (xm, ym), zero for
// infinity, and the encodings into zeroed buffers where the pointers are
// non-null (no parity byte: a share is not a signature).
DEV int g2_affine_encode_pt(const PtProj<Fp2> &acc, Fp2 &xm, Fp2 &ym, uint8_t *o192,
                            uint8_t *o96) {
    if (fp2_is_zero(acc.z)) {
        fp2_zero(xm);
        fp2_zero(ym);
        if (o192) o192[0] = 0x40;
        if (o96) o96[0] = 0xC0;
        return CB_INF;
    }
    Fp2 zi, x, y;
    fp2_inv(zi, acc.z);
    fp2_mul(xm, acc.x, zi);
    fp2_mul(ym, acc.y, zi);
    if (!o192 && !o96) return CB_OK;
    fp2_from_mont(x, xm);
    fp2_from_mont(y, ym);
    if (o192) g2_store_be192(o192, x, y);
    if (o96) {
        int cmp = fp_cmp_neg(y.c1);
        if (cmp == 0) cmp = fp_cmp_neg(y.c0);
        store_be48_raw(o96, x.c1, (uint8_t)(0x80 | (cmp > 0 ? 0x20 : 0)));
        store_be48_raw(o96 + 48, x.c0, 0);
    }
    return CB_OK;
}

DEV int pt_affine_encode(const PtProj<Fp> &acc, Fp &xm, Fp &ym, uint8_t *ou, uint8_t *oc) {
    return g1_affine_encode(acc, xm, ym, ou, oc);
}
DEV int pt_affine_encode(const PtProj<Fp2> &acc, Fp2 &xm, Fp2 &ym, uint8_t *ou, uint8_t *oc) {
    return g2_affine_encode_pt(acc, xm, ym, ou, oc);
}

// The tail of the three multiplication kernels: result j (acc, unless st is
// PT_BAD) as entry j of the output table with its status byte, and in the
// uncompressed (2 sizeof(F) bytes) and compressed (sizeof(F) bytes) encodings
// where the pointers are non-null; zero bytes for PT_BAD.
template <class F>
DEV void store_result(const PtProj<F> &acc, int st, size_t j, uint32_t *otab, uint8_t *ost,
                      uint8_t *out_u, uint8_t *out_c, uint8_t *status) {
    constexpr int kU = 2 * (int)sizeof(F), kC = (int)sizeof(F);
    uint8_t *ou = out_u ? out_u + (size_t)kU * j : nullptr;
    uint8_t *oc = out_c ? out_c + (size_t)kC * j : nullptr;
    if (ou)
        for (int i = 0; i < kU; ++i) ou[i] = 0;
    if (oc)
        for (int i = 0; i < kC; ++i) oc[i] = 0;
    F xm, ym;
    if (st != PT_BAD) {
        st = pt_affine_encode(acc, xm, ym, ou, oc);   // CB_OK / CB_INF = PT_OK / PT_INF
    } else {
        fe_zero(xm);
        fe_zero(ym);
    }
    store_affine(otab + j * (2 * sizeof(F) / 4), xm, ym);
    ost[j] = (uint8_t)st;
    status[j] = (uint8_t)st;
}

// The body of the two variable-base kernels, one lane per result j:
// [scalars[sidx[j]]] T[rows[j]] (sidx null: scalar j) over a g1_prepare /
// g2_points table of `nprep` points.  A zero scalar and an entry at infinity
// give infinity (status 1); an invalid entry, a row outside the table, an
// sidx outside [0, nscalars) and a scalar >= r give status 2 -- an index out
// of range is never a read out of range.  Lanes of a wave that share a scalar
// share their GLV digits, so the branch on the digit and the operand select
// of pt_mul_glv are uniform for the wave.
template <class F>
DEV void mul_table(const uint32_t *tab, const uint8_t *tst, size_t nprep, const int32_t *rows,
                   const uint8_t *scalars, size_t nscalars, const int32_t *sidx, size_t count,
                   uint32_t *otab, uint8_t *ost, uint8_t *out_u, uint8_t *out_c,
                   uint8_t *status) {
    const size_t j = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (j >= count) return;
    const int32_t row = rows[j];
    int st = (row >= 0 && (size_t)row < nprep) ? tst[row] : PT_BAD;
    const int64_t si = sidx ? (int64_t)sidx[j] : (int64_t)j;
    Fr k;
    if (si >= 0 && (uint64_t)si < nscalars) {
        fr_load_be32(k, scalars + 32 * (size_t)si);
        if (!fr_is_canonical(k)) st = PT_BAD;
    } else {
        st = PT_BAD;
    }
    PtProj<F> acc;
    if (st == PT_OK) {
        F x, y;
        load_affine(tab + (size_t)row * (2 * sizeof(F) / 4), x, y);
        pt_mul_glv(acc, x, y, k);
    } else {
        pt_identity(acc);
    }
    store_result(acc, st, j, otab, ost, out_u, out_c, status);
}

__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kG1PrepWpe, kG1PrepWpe))) void g1_mul_table_kernel(
    const uint32_t *__restrict__ tab, const uint8_t *__restrict__ tst, size_t nprep,
    const int32_t *__restrict__ rows, const uint8_t *__restrict__ scalars, size_t nscalars,
    const int32_t *__restrict__ sidx, size_t count, uint32_t *__restrict__ otab,
    uint8_t *__restrict__ ost, uint8_t *__restrict__ out96, uint8_t *__restrict__ out48,
    uint8_t *__restrict__ status) {
    mul_table<Fp>(tab, tst, nprep, rows, scalars, nscalars, sidx, count, otab, ost, out96, out48,
                  status);
}

__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void g2_mul_table_kernel(
    const uint32_t *__restrict__ tab, const uint8_t *__restrict__ tst, size_t nprep,
    const int32_t *__restrict__ rows, const uint8_t *__restrict__ scalars, size_t nscalars,
    const int32_t *__restrict__ sidx, size_t count, uint32_t *__restrict__ otab,
    uint8_t *__restrict__ ost, uint8_t *__restrict__ out192, uint8_t *__restrict__ out96,
    uint8_t *__restrict__ status) {
    mul_table<Fp2>(tab, tst, nprep, rows, scalars, nscalars, sidx, count, otab, ost, out192,
                   out96, status);
}

// Kernel: one lane per result [s_i] G1::one(), the GLV loop of
// g1_base_mul_check_kernel (the generator, [x^2] G and their sum as affine
// constants through the mixed addition) with the result written as
// g1_horner_kernel writes its own.  s = 0 gives infinity (status 1), s >= r
// status 2.
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kG1PrepWpe, kG1PrepWpe))) void g1_base_mul_kernel(
    const uint8_t *__restrict__ scalars, size_t count, uint32_t *__restrict__ otab,
    uint8_t *__restrict__ ost, uint8_t *__restrict__ out96, uint8_t *__restrict__ out48,
    uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= count) return;
    Fr k;
    fr_load_be32(k, scalars + 32 * i);
    const int st = fr_is_canonical(k) ? PT_OK : PT_BAD;
    PtProj<Fp> acc;
    pt_identity(acc);
    if (st == PT_OK) {
        uint64_t k1hi, k1lo, k2hi, k2lo;
        glv_split(k, k1hi, k1lo, k2hi, k2lo);
        for (int b = 127; b >= 0; --b) {
            pt_dbl(acc);
            const unsigned sel = glv_digit(k1hi, k1lo, k2hi, k2lo);
            if (sel) {
                Fp ox, oy;
#pragma unroll
                for (int w = 0; w < NL; ++w) {
                    ox.l[w] = sel == 1 ? kG1GenX[w] : (sel == 2 ? kG1GenQX[w] : kG1GenTX[w]);
                    oy.l[w] = sel == 1 ? kG1GenY[w] : (sel == 2 ? kG1GenNegY[w] : kG1GenTY[w]);
                }
                pt_add_affine(acc, ox, oy);
            }
        }
    }
    store_result(acc, st, i, otab, ost, out96, out48, status);
}

DEV void fr_zero(Fr &r) {
#pragma unroll
    for (int i = 0; i < NR; ++i) r.l[i] = 0;
}

// a + b mod r for a, b < r (the sum stays below 2^256)
DEV void fr_add(Fr &r, const Fr &a, const Fr &b) {
    uint32_t t[NR], s[NR];
    uint32_t c = 0, br = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) t[i] = addc(a.l[i], b.l[i], c, &c);
#pragma unroll
    for (int i = 0; i < NR; ++i) s[i] = subb(t[i], kFrR[i], br, &br);
#pragma unroll
    for (int i = 0; i < NR; ++i) r.l[i] = br ? t[i] : s[i];
}

// Kernel: the Fr twin of g1_horner_kernel, one lane per evaluation e of
// polynomial poly[e] at the raw 32-bit x[e].  Polynomial p has the
// coefficients scalars[rows[offsets[p] .. offsets[p + 1])] (32 big-endian
// bytes each, constant term first), ranges clamped to offsets[polys].
// Horner's rule on canonical values: acc <- acc x + c with x in Montgomery
// form, so the Montgomery product returns the canonical acc x.  x = 0 gives
// the constant term, the empty polynomial 0.  A coefficient >= r, a row
// outside [0, nscalars) or a poly outside [0, polys): status 2, zero bytes.
__global__ __launch_bounds__(kPairBlock) void fr_horner_kernel(
    const uint8_t *__restrict__ scalars, size_t nscalars, const int32_t *__restrict__ rows,
    const uint32_t *__restrict__ offsets, size_t polys, const int32_t *__restrict__ poly,
    const uint32_t *__restrict__ xs, size_t evals, uint8_t *__restrict__ out,
    uint8_t *__restrict__ status) {
    const size_t e = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (e >= evals) return;
    const int32_t p = poly[e];
    int st = PT_OK;
    size_t b = 0, en = 0;
    if (p >= 0 && (size_t)p < polys)
        group_range(offsets, (size_t)p, offsets[polys], b, en);
    else
        st = PT_BAD;
    Fr xm, acc;
    fr_from_u64(xm, xs[e]);
    fr_zero(acc);
    for (size_t k = en; k > b && st == PT_OK; --k) {
        const int32_t row = rows[k - 1];
        Fr c;
        if (row < 0 || (size_t)row >= nscalars) {
            st = PT_BAD;   // a row past the scalars is an invalid input, never a read
            break;
        }
        fr_load_be32(c, scalars + 32 * (size_t)row);
        if (!fr_is_canonical(c)) st = PT_BAD;
        fr_mul(acc, acc, xm);
        fr_add(acc, acc, c);
    }
    if (st != PT_OK) fr_zero(acc);
    fr_store_be32(out + 32 * e, acc);
    status[e] = (uint8_t)st;
}

// Kernel: one lane per group g, sum_j a_j b_j mod r over j in [offsets[g],
// offsets[g + 1]) clamped to `total` (32 big-endian bytes per operand).  The
// Montgomery products carry a factor 2^-256 each, their sum one product with
// 2^512 takes out.  An operand >= r: status 2, zero bytes; an empty group is 0.
// With the coefficients of lagrange_kernel this is the
// `Poly::interpolate(..).evaluate(0)` of `generate`.
__global__ __launch_bounds__(kPairBlock) void fr_dot_kernel(
    const uint8_t *__restrict__ a, const uint8_t *__restrict__ bb,
    const uint32_t *__restrict__ offsets, size_t groups, size_t total,
    uint8_t *__restrict__ out, uint8_t *__restrict__ status) {
    const size_t g = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (g >= groups) return;
    size_t b, e;
    group_range(offsets, g, total, b, e);
    int st = PT_OK;
    Fr acc;
    fr_zero(acc);
    for (size_t j = b; j < e; ++j) {
        Fr x, y;
        fr_load_be32(x, a + 32 * j);
        fr_load_be32(y, bb + 32 * j);
        if (!fr_is_canonical(x) || !fr_is_canonical(y)) {
            st = PT_BAD;
            break;
        }
        fr_mul(x, x, y);
        fr_add(acc, acc, x);
    }
    if (st == PT_OK) {
        Fr r2;
        fr_set(r2, kFrR2);
        fr_mul(acc, acc, r2);
    } else {
        fr_zero(acc);
    }
    fr_store_be32(out + 32 * g, acc);
    status[g] = (uint8_t)st;
}

// ------------------------------------------------- compressed encodings
// hbbft's messages carry every point in the crate's compressed form: 48 bytes
// for G1 (DecryptionShare, PublicKeyShare, a ciphertext's U), 96 for G2
// (SignatureShare, a ciphertext's W) -- x big-endian (G2: x.c1 || x.c0) with
// three flag bits in byte 0: 0x80 compressed (must be set), 0x40 infinity
// (then every other bit must be zero), 0x20 "y is the larger of y and -y".
// decompress_g1 / decompress_g2 restate the `pairing` crate's
// G1Compressed::into_affine / G2Compressed::into_affine: flags, x < p,
// y = sqrt(x^3 + b) (no root: invalid), the choice between y and -y by the
// comparison the two encode kernels above apply, then the order-r check.
//
// p = 3 mod 4: for a square a, t = a^((p-3)/4) is 1/sqrt(a) and t a the root.
// The exponent is a constant (kSqrtExp, 379 bits), walked in 4-bit windows:
// 14 products for a^1 .. a^15, then 4 squarings and at most one product per
// window -- 376 squarings and 89 products, a third of the products of
// g1_in_subgroup's 127 doublings and 64 additions.  The digit is
// wave-uniform, so the table is indexed by a scalar and the skipped product of
// a zero digit is a uniform branch; the table itself (15 x 12 words) lives in
// scratch beside the stack of the NOINL units, read once per window.
NOINL void fp_pow_sqrt(Fp &r, const Fp &a) {
    Fp tab[15];
    tab[0] = a;
    for (int i = 1; i < 15; ++i) fp_mul(tab[i], tab[i - 1], a);
    constexpr int top = kSqrtExpWindows - 1;
    constexpr uint32_t topd = (kSqrtExp[top >> 3] >> (4 * (top & 7))) & 15u;
    static_assert(topd != 0, "the top window holds the exponent's leading bits");
    Fp acc = tab[topd - 1];
    for (int w = top - 1; w >= 0; --w) {
#pragma unroll 1
        for (int k = 0; k < 4; ++k) fp_sqr(acc, acc);
        const uint32_t d = (kSqrtExp[w >> 3] >> (4 * (w & 7))) & 15u;
        if (d) fp_mul(acc, acc, tab[d - 1]);
    }
    r = acc;
}

DEV int decompress_g1(const uint8_t *src, Fp &x, Fp &y) {
    const uint8_t f = src[0];
    if (!(f & 0x80)) return PT_BAD;                    // not a compressed encoding
    if (f & 0x40) return all_zero(src, 48, 0x3F) ? PT_INF : PT_BAD;
    Fp xr;
    if (!load_be48(xr, src, 0x1FFFFFFFu)) return PT_BAD;
    to_mont(x, xr);
    Fp a, b, t, c;
    fp_sqr(a, x);
    fp_mul(a, a, x);
    fp_set(b, kB1);
    fp_add(a, a, b);                                   // x^3 + 4
    fp_pow_sqrt(t, a);
    fp_mul(y, t, a);
    fp_sqr(c, y);
    if (!fp_eq(c, a)) return PT_BAD;                   // y^2 = x^3 + 4, or no root
    from_mont(c, y);
    if ((fp_cmp_neg(c) > 0) != ((f & 0x20) != 0)) fp_neg(y, y);
    return g1_in_subgroup(x, y) ? PT_OK : PT_BAD;
}

// Square root in Fp2 by norms: two exponentiations in Fp and no retry.  With
// d = sqrt(a0^2 + a1^2) (a square in Fp iff a is one in Fp2) and
// delta = (a0 + d)/2, t = delta^((p-3)/4) and x0 = t delta: either x0^2 =
// delta, then t = 1/x0 and the root is x0 + a1/(2 x0) u; or x0^2 = -delta
// (delta is no square, so (a0 - d)/2 = a1^2 / (4 x0^2) is one), then -t =
// 1/x0 and the root is a1/(2 x0) + x0 u.  delta = 0 only for a1 = 0 and d =
// -a0, where (a0 - d)/2 = a0 takes its place.  Returns whether y^2 == a,
// checked on the result itself: a non-square norm gives some d, t and a y
// that fails here.
NOINL bool fp2_sqrt(Fp2 &y, const Fp2 &a) {
    Fp n, t, d, h, delta, x0, x1, c;
    fp_sqr(n, a.c0);
    fp_sqr(t, a.c1);
    fp_add(n, n, t);
    fp_pow_sqrt(t, n);
    fp_mul(d, t, n);
    fp_set(h, kHalf);
    fp_add(delta, a.c0, d);
    fp_mul(delta, delta, h);
    if (fp_is_zero(delta)) delta = a.c0;
    fp_pow_sqrt(t, delta);
    fp_mul(x0, t, delta);
    fp_sqr(c, x0);
    const bool res = fp_eq(c, delta);
    fp_mul(x1, a.c1, t);
    fp_mul(x1, x1, h);                                 // +- a1 / (2 x0)
    if (res) {
        y.c0 = x0;
        y.c1 = x1;
    } else {
        fp_neg(y.c0, x1);
        y.c1 = x0;
    }
    Fp2 s;
    fp2_sqr(s, y);
    return fp2_eq(s, a);
}

DEV int decompress_g2(const uint8_t *src, Fp2 &x, Fp2 &y) {
    const uint8_t f = src[0];
    if (!(f & 0x80)) return PT_BAD;
    if (f & 0x40) return all_zero(src, 96, 0x3F) ? PT_INF : PT_BAD;
    Fp a, b;
    if (!load_be48(a, src, 0x1FFFFFFFu) || !load_be48(b, src + 48, 0xFFFFFFFFu)) return PT_BAD;
    to_mont(x.c1, a);
    to_mont(x.c0, b);
    Fp2 r, bb;
    fp2_sqr(r, x);
    fp2_mul(r, r, x);
    fp_set(bb.c0, kB1);
    bb.c1 = bb.c0;                                     // 4 (u + 1)
    fp2_add(r, r, bb);
    if (!fp2_sqrt(y, r)) return PT_BAD;
    from_mont(a, y.c1);
    from_mont(b, y.c0);
    int cmp = fp_cmp_neg(a);                           // c1 first, c0 when the c1 are equal
    if (cmp == 0) cmp = fp_cmp_neg(b);
    if ((cmp > 0) != ((f & 0x20) != 0)) fp2_neg(y, y);
    return g2_in_subgroup(x, y) ? PT_OK : PT_BAD;
}

// g1_prepare_kernel for compressed input (48 bytes per point): the same table.
// Waves per SIMD: 2 like g1_prepare_kernel.  hipcc -S: 248 VGPRs, no spills,
// 944 bytes of scratch -- the 272 of g1_prepare_kernel (the stack of the NOINL
// units: pt_dbl and pt_add_affine take their operands by reference, so no
// occupancy frees that kernel of scratch either) and the window table, which
// is indexed by the digit and so could stay in registers only fully unrolled.
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kG1PrepWpe, kG1PrepWpe))) void g1_prepare_compressed_kernel(
    const uint8_t *__restrict__ g1c, size_t count, uint32_t *__restrict__ keys,
    uint8_t *__restrict__ kst) {
    prepare_table<Fp>(g1c, 48, count, keys, kst,
                      [](const uint8_t *p, Fp &x, Fp &y) { return decompress_g1(p, x, y); });
}

// g2_points_kernel for compressed input (96 bytes per point): the same table.
// Waves per SIMD: 2 like g2_points_kernel: the Fp2 chain of g2_in_subgroup
// sets the register need, the Fp roots add none (hipcc -S: 256 VGPRs, 2
// spilled, 1572 bytes of scratch against 4 and 1684 of g2_points_kernel).
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void g2_points_compressed_kernel(
    const uint8_t *__restrict__ g2c, size_t count, uint32_t *__restrict__ tab,
    uint8_t *__restrict__ gst) {
    prepare_table<Fp2>(g2c, 96, count, tab, gst,
                       [](const uint8_t *p, Fp2 &x, Fp2 &y) { return decompress_g2(p, x, y); });
}

// a Montgomery affine point as canonical big-endian x || y (G2: x.c1 || x.c0 ||
// y.c1 || y.c0)
DEV void store_be_affine(uint8_t *o, Fp x, Fp y) {
    from_mont(x, x);
    from_mont(y, y);
    store_be48_raw(o, x, 0);
    store_be48_raw(o + 48, y, 0);
}
DEV void store_be_affine(uint8_t *o, Fp2 x, Fp2 y) {
    fp2_from_mont(x, x);
    fp2_from_mont(y, y);
    g2_store_be192(o, x, y);
}

// Compressed to uncompressed, one lane per point: out + 2 * stride * q gets the
// uncompressed encoding of the `stride` bytes at src + stride * q (zero bytes
// for an invalid point, 0x40 and zeros for infinity), status[q] 0 ok,
// 1 infinity, 2 invalid.  For points that go on to an entry taking the
// uncompressed form (a ciphertext's U and W).
template <class F, class Decompress>
DEV void decompress_points(const uint8_t *src, size_t stride, size_t count, uint8_t *out,
                           uint8_t *status, Decompress decompress) {
    const size_t q = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (q >= count) return;
    F x, y;
    const int st = decompress(src + q * stride, x, y);
    uint8_t *o = out + q * (2 * stride);
    if (st == PT_OK) {
        store_be_affine(o, x, y);
    } else {
        for (size_t i = 0; i < 2 * stride; ++i) o[i] = 0;
        if (st == PT_INF) o[0] = 0x40;
    }
    status[q] = (uint8_t)st;
}

__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kG1PrepWpe, kG1PrepWpe))) void g1_decompress_kernel(
    const uint8_t *__restrict__ g1c, size_t count, uint8_t *__restrict__ out96,
    uint8_t *__restrict__ status) {
    decompress_points<Fp>(g1c, 48, count, out96, status,
                          [](const uint8_t *p, Fp &x, Fp &y) { return decompress_g1(p, x, y); });
}

__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void g2_decompress_kernel(
    const uint8_t *__restrict__ g2c, size_t count, uint8_t *__restrict__ out192,
    uint8_t *__restrict__ status) {
    decompress_points<Fp2>(g2c, 96, count, out192, status,
                           [](const uint8_t *p, Fp2 &x, Fp2 &y) { return decompress_g2(p, x, y); });
}

// The crate's final exponentiation (Bls12::final_exponentiation): easy part
// f^((p^6 - 1)(p^2 + 1)), then the hard-part chain.
DEV void final_exp(Fp12 &out, const Fp12 &f) {
    Fp12 r, t, y0, y1, y2, y3;
    fp12_inv(t, f);
    fp12_conj(r, f);
    fp12_mul(r, r, t);            // f^(p^6 - 1)
    fp12_frob(t, r, 2);
    fp12_mul(r, t, r);            // ^(p^2 + 1)
    fp12_sqr(y0, r);
    fp12_exp_by_x(y1, y0, 0);
    fp12_exp_by_x(y2, y1, 1);
    fp12_conj(y3, r);
    fp12_mul(y1, y1, y3);
    fp12_conj(y1, y1);
    fp12_mul(y1, y1, y2);
    fp12_exp_by_x(y2, y1, 0);
    fp12_exp_by_x(y3, y2, 0);
    fp12_conj(y1, y1);
    fp12_mul(y3, y3, y1);
    fp12_conj(y1, y1);
    fp12_frob(y1, y1, 3);
    fp12_frob(y2, y2, 2);
    fp12_mul(y1, y1, y2);
    fp12_exp_by_x(y2, y3, 0);
    fp12_mul(y2, y2, y0);
    fp12_mul(y2, y2, r);
    fp12_mul(y1, y1, y2);
    fp12_frob(y2, y3, 1);
    fp12_mul(out, y1, y2);
}

DEV void store_be48(uint8_t *dst, const Fp &a) {
    Fp c;
    from_mont(c, a);
#pragma unroll
    for (int w = 0; w < NL; ++w) {
        const uint32_t v = c.l[NL - 1 - w];
        dst[4 * w + 0] = (uint8_t)(v >> 24);
        dst[4 * w + 1] = (uint8_t)(v >> 16);
        dst[4 * w + 2] = (uint8_t)(v >> 8);
        dst[4 * w + 3] = (uint8_t)v;
    }
}

// Kernel 2: one final exponentiation per lane.  `per_out` Miller values
// (1: a pairing, 2: a check) are multiplied first.  gt_out (if set) gets the
// 576-byte GT value; ok_out (if set) gets 1 if the value is 1 (the check
// holds), 0 if not, 2 if an input point was invalid.
constexpr int kFinalExpWpe = kPairWpe;   // the final exponentiation's own occupancy
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kFinalExpWpe, kFinalExpWpe))) void final_exp_kernel(
    const uint32_t *__restrict__ ws, size_t n_miller, size_t n_out, int per_out,
    const uint8_t *__restrict__ status, uint8_t *__restrict__ gt_out,
    uint8_t *__restrict__ ok_out) {
    const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_out) return;
    Fp12 f;
    load_f12(f, ws, n_miller, i * per_out);
    int bad = status[i * per_out] == PT_BAD;
    for (int j = 1; j < per_out; ++j) {
        Fp12 g;
        load_f12(g, ws, n_miller, i * per_out + j);
        fp12_mul(f, f, g);
        bad |= status[i * per_out + j] == PT_BAD;
    }
    Fp12 e;
    final_exp(e, f);
    if (gt_out) {
        uint8_t *dst = gt_out + i * 576;
        const Fp2 *c = &e.c0.c0;
        const Fp2 *cs[6] = {&e.c0.c0, &e.c0.c1, &e.c0.c2, &e.c1.c0, &e.c1.c1, &e.c1.c2};
        (void)c;
        for (int k = 0; k < 6; ++k) {
            store_be48(dst + 96 * k, cs[k]->c0);
            store_be48(dst + 96 * k + 48, cs[k]->c1);
        }
    }
    if (ok_out) ok_out[i] = bad ? 2 : (fp12_is_one(e) ? 1 : 0);
}

}  // namespace

// The kernels run at 4 waves/SIMD (128 VGPRs, the rest of the tower state in
// scratch); 1 and 2 waves measured within 5 %.
hipError_t launch_pairing_miller(const uint8_t *g1, size_t g1_stride, const uint8_t *g2,
                                 size_t g2_stride, size_t n, int pair_inputs, PairWs ws,
                                 hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(miller_kernel, dim3(blocks), dim3(kPairBlock), 0, s, g1, g1_stride, g2, g2_stride, n,
                       pair_inputs, ws.gt, ws.status);
    return hipGetLastError();
}

hipError_t launch_pairing_miller2(const uint8_t *g1, const uint8_t *g2, size_t count, PairWs ws,
                                  hipStream_t s) {
    if (count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(miller2_kernel, dim3(blocks), dim3(kPairBlock), 0, s, g1, g2, count, ws.gt,
                       ws.status);
    return hipGetLastError();
}

size_t pairing_prepared_words(size_t points) { return points * (size_t)kLines * kLineWords; }

hipError_t launch_g2_prepare(const uint8_t *g2, TableOut<G2Lines> prep, hipStream_t s) {
    if (prep.count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((prep.count + kPairBlock - 1) / kPairBlock) * 2;
    hipLaunchKernelGGL(g2_prepare_kernel, dim3(blocks), dim3(kPairBlock), 0, s, g2, prep.count,
                       prep.words, prep.status);
    return hipGetLastError();
}

hipError_t launch_pairing_miller_prepared(const uint8_t *g1, Table<G2Lines> prep,
                                          const uint32_t *ib, const uint32_t *id, size_t count,
                                          PairWs ws, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (prep.count == 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(miller_prepared_kernel<false>, dim3(blocks), dim3(kPairBlock), 0, s, g1,
                       nullptr, nullptr, nullptr, (size_t)0, prep.words, prep.status, ib, id,
                       prep.count, count, ws.gt, ws.status);
    return hipGetLastError();
}

size_t g1_key_words(size_t points) { return points * (size_t)kG1KeyWords; }

hipError_t launch_pairing_miller_prepared_pts(Table<G1Keys> a, Table<G1Keys> keys,
                                              const uint32_t *ic, Table<G2Lines> prep,
                                              const uint32_t *ib, const uint32_t *id, size_t count,
                                              PairWs ws, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (prep.count == 0 || keys.count == 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL((miller_prepared_kernel<true, true>), dim3(blocks), dim3(kPairBlock), 0, s,
                       nullptr, keys.words, keys.status, ic, keys.count, prep.words, prep.status,
                       ib, id, prep.count, count, ws.gt, ws.status, a.words, a.status);
    return hipGetLastError();
}

hipError_t launch_g1_prepare(const uint8_t *g1, TableOut<G1Keys> keys, hipStream_t s) {
    if (keys.count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((keys.count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g1_prepare_kernel, dim3(blocks), dim3(kPairBlock), 0, s, g1, keys.count,
                       keys.words, keys.status);
    return hipGetLastError();
}

size_t g1_point_words(size_t shares) { return shares * (sizeof(PtProj<Fp>) / 4); }

hipError_t launch_lagrange(const uint32_t *idx, const uint32_t *offsets, size_t groups,
                           size_t total, uint8_t *coeffs, uint8_t *status, hipStream_t s) {
    if (total == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((total + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(lagrange_kernel, dim3(blocks), dim3(kPairBlock), 0, s, idx, offsets, groups,
                       total, coeffs, status);
    return hipGetLastError();
}

hipError_t launch_g1_scalar_mul(Table<G1Keys> tab, const int32_t *rows, const uint8_t *scalars,
                                size_t total, uint32_t *ws, uint8_t *pst, hipStream_t s) {
    if (total == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((total + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g1_scalar_mul_kernel, dim3(blocks), dim3(kPairBlock), 0, s, tab.words,
                       tab.status, tab.count, rows, scalars, total, ws, pst);
    return hipGetLastError();
}

hipError_t launch_g1_reduce_encode(const uint32_t *ws, const uint8_t *pst, const uint32_t *offsets,
                                   size_t groups, size_t total, const uint8_t *lst, uint8_t *out96,
                                   uint8_t *out48, uint8_t *status, hipStream_t s) {
    if (groups == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((groups + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g1_reduce_encode_kernel, dim3(blocks), dim3(kPairBlock), 0, s, ws, pst,
                       offsets, groups, total, lst, out96, out48, status);
    return hipGetLastError();
}

hipError_t launch_g1_horner(Table<G1Keys> tab, const int32_t *rows, const uint32_t *offsets,
                            size_t polys, const int32_t *poly, const uint32_t *x,
                            TableOut<G1Keys> out, uint8_t *out96, uint8_t *out48, uint8_t *status,
                            hipStream_t s) {
    if (out.count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((out.count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g1_horner_kernel, dim3(blocks), dim3(kPairBlock), 0, s, tab.words,
                       tab.status, tab.count, rows, offsets, polys, poly, x, out.count, out.words,
                       out.status, out96, out48, status);
    return hipGetLastError();
}

hipError_t launch_g1_base_mul_check(Table<G1Keys> tab, const int32_t *rows, const uint8_t *scalars,
                                    size_t count, uint8_t *ok, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g1_base_mul_check_kernel, dim3(blocks), dim3(kPairBlock), 0, s, tab.words,
                       tab.status, tab.count, rows, scalars, count, ok);
    return hipGetLastError();
}

size_t g2_point_table_words(size_t points) { return points * (size_t)kG2PtWords; }
size_t g2_point_words(size_t shares) { return shares * (sizeof(PtProj<Fp2>) / 4); }

hipError_t launch_g2_points(const uint8_t *g2, TableOut<G2Points> tab, hipStream_t s) {
    if (tab.count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((tab.count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g2_points_kernel, dim3(blocks), dim3(kPairBlock), 0, s, g2, tab.count,
                       tab.words, tab.status);
    return hipGetLastError();
}

hipError_t launch_pairing_miller_sig(Table<G2Points> sig, Table<G1Keys> keys, const uint32_t *ic,
                                     Table<G2Lines> prep, const uint32_t *ih, size_t count,
                                     PairWs ws, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (prep.count == 0 || keys.count == 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(miller_sig_kernel, dim3(blocks), dim3(kPairBlock), 0, s, sig.words,
                       sig.status, sig.count, keys.words, keys.status, ic, keys.count, prep.words,
                       prep.status, ih, prep.count, count, ws.gt, ws.status);
    return hipGetLastError();
}

hipError_t launch_g2_scalar_mul(Table<G2Points> tab, const int32_t *rows, const uint8_t *scalars,
                                size_t total, uint32_t *ws, uint8_t *pst, hipStream_t s) {
    if (total == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((total + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g2_scalar_mul_kernel, dim3(blocks), dim3(kPairBlock), 0, s, tab.words,
                       tab.status, tab.count, rows, scalars, total, ws, pst);
    return hipGetLastError();
}

hipError_t launch_g2_reduce_encode(const uint32_t *ws, const uint8_t *pst, const uint32_t *offsets,
                                   size_t groups, size_t total, const uint8_t *lst,
                                   uint8_t *out192, uint8_t *out96, uint8_t *parity,
                                   uint8_t *status, hipStream_t s) {
    if (groups == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((groups + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g2_reduce_encode_kernel, dim3(blocks), dim3(kPairBlock), 0, s, ws, pst,
                       offsets, groups, total, lst, out192, out96, parity, status);
    return hipGetLastError();
}

hipError_t launch_g1_mul_table(Table<G1Keys> tab, const int32_t *rows, const uint8_t *scalars,
                               size_t nscalars, const int32_t *sidx, TableOut<G1Keys> out,
                               uint8_t *out96, uint8_t *out48, uint8_t *status, hipStream_t s) {
    if (out.count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((out.count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g1_mul_table_kernel, dim3(blocks), dim3(kPairBlock), 0, s, tab.words,
                       tab.status, tab.count, rows, scalars, nscalars, sidx, out.count, out.words,
                       out.status, out96, out48, status);
    return hipGetLastError();
}

hipError_t launch_g2_mul_table(Table<G2Points> tab, const int32_t *rows, const uint8_t *scalars,
                               size_t nscalars, const int32_t *sidx, TableOut<G2Points> out,
                               uint8_t *out192, uint8_t *out96, uint8_t *status, hipStream_t s) {
    if (out.count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((out.count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g2_mul_table_kernel, dim3(blocks), dim3(kPairBlock), 0, s, tab.words,
                       tab.status, tab.count, rows, scalars, nscalars, sidx, out.count, out.words,
                       out.status, out192, out96, status);
    return hipGetLastError();
}

hipError_t launch_g1_base_mul(const uint8_t *scalars, TableOut<G1Keys> out, uint8_t *out96,
                              uint8_t *out48, uint8_t *status, hipStream_t s) {
    if (out.count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((out.count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g1_base_mul_kernel, dim3(blocks), dim3(kPairBlock), 0, s, scalars,
                       out.count, out.words, out.status, out96, out48, status);
    return hipGetLastError();
}

hipError_t launch_fr_horner(const uint8_t *scalars, size_t nscalars, const int32_t *rows,
                            const uint32_t *offsets, size_t polys, const int32_t *poly,
                            const uint32_t *x, size_t evals, uint8_t *out, uint8_t *status,
                            hipStream_t s) {
    if (evals == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((evals + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(fr_horner_kernel, dim3(blocks), dim3(kPairBlock), 0, s, scalars, nscalars,
                       rows, offsets, polys, poly, x, evals, out, status);
    return hipGetLastError();
}

hipError_t launch_fr_dot(const uint8_t *a, const uint8_t *b, const uint32_t *offsets,
                         size_t groups, size_t total, uint8_t *out, uint8_t *status,
                         hipStream_t s) {
    if (groups == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((groups + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(fr_dot_kernel, dim3(blocks), dim3(kPairBlock), 0, s, a, b, offsets, groups,
                       total, out, status);
    return hipGetLastError();
}

hipError_t launch_g1_prepare_compressed(const uint8_t *g1c, TableOut<G1Keys> keys, hipStream_t s) {
    if (keys.count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((keys.count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g1_prepare_compressed_kernel, dim3(blocks), dim3(kPairBlock), 0, s, g1c,
                       keys.count, keys.words, keys.status);
    return hipGetLastError();
}

hipError_t launch_g2_points_compressed(const uint8_t *g2c, TableOut<G2Points> tab, hipStream_t s) {
    if (tab.count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((tab.count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g2_points_compressed_kernel, dim3(blocks), dim3(kPairBlock), 0, s, g2c,
                       tab.count, tab.words, tab.status);
    return hipGetLastError();
}

hipError_t launch_g1_decompress(const uint8_t *g1c, size_t count, uint8_t *out96, uint8_t *status,
                                hipStream_t s) {
    if (count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g1_decompress_kernel, dim3(blocks), dim3(kPairBlock), 0, s, g1c, count,
                       out96, status);
    return hipGetLastError();
}

hipError_t launch_g2_decompress(const uint8_t *g2c, size_t count, uint8_t *out192,
                                uint8_t *status, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(g2_decompress_kernel, dim3(blocks), dim3(kPairBlock), 0, s, g2c, count,
                       out192, status);
    return hipGetLastError();
}

hipError_t launch_pairing_miller_prepared_keys(const uint8_t *g1_a, Table<G1Keys> keys,
                                               const uint32_t *ic, Table<G2Lines> prep,
                                               const uint32_t *ib, const uint32_t *id, size_t count,
                                               PairWs ws, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (prep.count == 0 || keys.count == 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((count + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(miller_prepared_kernel<true>, dim3(blocks), dim3(kPairBlock), 0, s, g1_a,
                       keys.words, keys.status, ic, keys.count, prep.words, prep.status, ib, id,
                       prep.count, count, ws.gt, ws.status);
    return hipGetLastError();
}

hipError_t launch_pairing_final(PairWs ws, size_t n_miller, size_t n_out, int per_out,
                                uint8_t *gt_out, uint8_t *ok_out, hipStream_t s) {
    if (n_out == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n_out + kPairBlock - 1) / kPairBlock);
    hipLaunchKernelGGL(final_exp_kernel, dim3(blocks), dim3(kPairBlock), 0, s, ws.gt, n_miller, n_out, per_out,
                       ws.status, gt_out, ok_out);
    return hipGetLastError();
}

// hash_g2, hash_g1_g2 and xor_with_hash: kernels and launchers over the units
// above (this file's anonymous namespace), kept in a file of their own
#include "hash_g2.hip"

}  // namespace hbrbc
