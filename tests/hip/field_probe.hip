// field_probe.hip -- test infrastructure, not product: one C entry that runs
// the BLS12-381 field units of hbbft_amd/csrc/pairing.hip on raw operands, so
// tests/test_field_probe.py can feed them chosen internal representations and
// compare the result words with Python integers (tests/field_ref.py).
//
// The units live in pairing.hip's anonymous namespace; like
// tools/fp_microbench.hip this file #includes pairing.hip to reach them, so
// every op below runs the product's own function, compiled with the product's
// flags.  It links into tests/hip/libfieldprobe.so, never into libhbrbc.so.
//
//   int hbprobe_run(uint32_t op, const uint32_t *in, uint32_t *out,
//                   size_t count, void *stream);
//
// `in` / `out`: device pointers, item-major (item i at in + i * in_words, out
// + i * out_words), one lane per item.  Operands are raw Montgomery-form limbs
// (12 little-endian 32-bit words per Fp, R = 2^406; 8 per Fr, R = 2^256): no
// conversion here, the caller chooses the representation.  Every Fp / Fr
// operand must be below its modulus (the units' own precondition).  Returns 0,
// or a hipError_t: hipErrorInvalidValue for count == 0 or an unknown op.
//
//   op  name             unit                       in words   out words
//    0  fp_add           fp_add(a, b)               24         12
//    1  fp_sub           fp_sub(a, b)               24         12
//    2  fp_neg           fp_neg(a)       (b unused) 24         12
//    3  fp_dbl           fp_dbl(a)       (b unused) 24         12
//    4  fp_mul           fp_mul(a, b)               24         12
//    5  fp_sqr           fp_sqr(a)       (b unused) 24         12
//    6  fp_inv           fp_inv(a)                  12         12
//    7  fp2_mul          fp2_mul_in(a, b)           48         24
//    8  fp2_sqr          fp2_sqr_in(a)              24         24
//    9  fp2_inv          fp2_inv(a)                 24         24
//   10  fp2_mul_xi       fp2_mul_xi(a)              24         24
//   11  fp6_mul          fp6_mul_in(a, b)           144        72
//   12  fp12_mul_inl     fp12_mul_t<true>(a, b)     288        144
//   13  fp12_mul         fp12_mul_t<false>(a, b)    288        144
//   14  fp12_sqr_inl     fp12_sqr_t<true>(a)        144        144
//   15  fp12_sqr         fp12_sqr_t<false>(a)       144        144
//   16  fp12_mul_by_014  fp12_mul_by_014(f,c0,c1,c4) 216       144
//   17  fp12_cyclo_sqr   fp12_cyclo_sqr(f)          144        144
//   18  fp12_frob1       fp12_frob(a, 1)            144        144
//   19  fp12_frob2       fp12_frob(a, 2)            144        144
//   20  fp12_frob3       fp12_frob(a, 3)            144        144
//   21  fp12_inv         fp12_inv(a)                144        144
//   22  fp_sqrt          t = fp_pow_sqrt(a); flag = ((t a)^2 == a)   12   13
//   23  fp2_sqrt         flag = fp2_sqrt(y, a)      24         25 (y, flag)
//   24  fr_add           fr_add(a, b)               16         8
//   25  fr_sub           fr_sub(a, b)               16         8
//   26  fr_mul           fr_mul(a, b)               16         8
//   27  fr_inv           fr_inv(a)                  8          8
//
// Block size and occupancy are the product's: kPairBlock lanes, and
// amdgpu_waves_per_eu(kPairWpe) for the Fp tower as in the pairing and point
// kernels; the Fr kernels carry the launch bound alone, as lagrange_kernel,
// fr_horner_kernel and fr_dot_kernel do.
#include "pairing.hip"

namespace hbrbc {
namespace {

enum : uint32_t {
    OP_FP_ADD, OP_FP_SUB, OP_FP_NEG, OP_FP_DBL, OP_FP_MUL, OP_FP_SQR, OP_FP_INV,
    OP_FP2_MUL, OP_FP2_SQR, OP_FP2_INV, OP_FP2_MUL_XI, OP_FP6_MUL,
    OP_FP12_MUL_INL, OP_FP12_MUL, OP_FP12_SQR_INL, OP_FP12_SQR, OP_FP12_MUL_BY_014,
    OP_FP12_CYCLO_SQR, OP_FP12_FROB1, OP_FP12_FROB2, OP_FP12_FROB3, OP_FP12_INV,
    OP_FP_SQRT, OP_FP2_SQRT, OP_FR_ADD, OP_FR_SUB, OP_FR_MUL, OP_FR_INV, OP_COUNT
};

#define PROBE_FP __global__ __launch_bounds__(kPairBlock) \
    __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe)))
#define PROBE_FR __global__ __launch_bounds__(kPairBlock)

// T is a struct of 32-bit limbs only (Fp ... Fp12, Fr): plain word copies
template <class T>
DEV void ld(T &r, const uint32_t *src) {
    uint32_t *w = reinterpret_cast<uint32_t *>(&r);
    for (size_t j = 0; j < sizeof(T) / 4; ++j) w[j] = src[j];
}
template <class T>
DEV void st(uint32_t *dst, const T &a) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(&a);
    for (size_t j = 0; j < sizeof(T) / 4; ++j) dst[j] = w[j];
}

// lane -> item, or false past the end
DEV bool item(size_t &i, size_t count) {
    i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    return i < count;
}

template <uint32_t OP>
PROBE_FP void probe_fp_lin(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp a, b, r;
    ld(a, in + i * 24);
    ld(b, in + i * 24 + 12);
    if (OP == OP_FP_ADD) fp_add(r, a, b);
    else if (OP == OP_FP_SUB) fp_sub(r, a, b);
    else if (OP == OP_FP_NEG) fp_neg(r, a);
    else fp_dbl(r, a);
    st(out + i * 12, r);
}

template <uint32_t OP>
PROBE_FP void probe_fp_mul(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp a, b, r;
    ld(a, in + i * 24);
    ld(b, in + i * 24 + 12);
    if (OP == OP_FP_MUL) fp_mul(r, a, b);
    else fp_sqr(r, a);
    st(out + i * 12, r);
}

PROBE_FP void probe_fp_inv(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp a, r;
    ld(a, in + i * 12);
    fp_inv(r, a);
    st(out + i * 12, r);
}

PROBE_FP void probe_fp2_mul(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp2 a, b, r;
    ld(a, in + i * 48);
    ld(b, in + i * 48 + 24);
    fp2_mul_in(r, a, b);
    st(out + i * 24, r);
}

template <uint32_t OP>
PROBE_FP void probe_fp2_unary(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp2 a, r;
    ld(a, in + i * 24);
    if (OP == OP_FP2_SQR) fp2_sqr_in(r, a);
    else if (OP == OP_FP2_INV) fp2_inv(r, a);
    else fp2_mul_xi(r, a);
    st(out + i * 24, r);
}

PROBE_FP void probe_fp6_mul(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp6 a, b, r;
    ld(a, in + i * 144);
    ld(b, in + i * 144 + 72);
    fp6_mul_in(r, a, b);
    st(out + i * 72, r);
}

template <bool INL>
PROBE_FP void probe_fp12_mul(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp12 a, b, r;
    ld(a, in + i * 288);
    ld(b, in + i * 288 + 144);
    fp12_mul_t<INL>(r, a, b);
    st(out + i * 144, r);
}

template <bool INL>
PROBE_FP void probe_fp12_sqr(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp12 a, r;
    ld(a, in + i * 144);
    fp12_sqr_t<INL>(r, a);
    st(out + i * 144, r);
}

PROBE_FP void probe_fp12_mul_by_014(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp12 f;
    Fp2 c0, c1, c4;
    ld(f, in + i * 216);
    ld(c0, in + i * 216 + 144);
    ld(c1, in + i * 216 + 168);
    ld(c4, in + i * 216 + 192);
    fp12_mul_by_014(f, c0, c1, c4);
    st(out + i * 144, f);
}

PROBE_FP void probe_fp12_cyclo_sqr(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp12 f;
    ld(f, in + i * 144);
    fp12_cyclo_sqr(f);
    st(out + i * 144, f);
}

PROBE_FP void probe_fp12_frob(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count, int k) {
    size_t i;
    if (!item(i, count)) return;
    Fp12 a, r;
    ld(a, in + i * 144);
    fp12_frob(r, a, k);
    st(out + i * 144, r);
}

PROBE_FP void probe_fp12_inv(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp12 a, r;
    ld(a, in + i * 144);
    fp12_inv(r, a);
    st(out + i * 144, r);
}

PROBE_FP void probe_fp_sqrt(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp a, t, y, c;
    ld(a, in + i * 12);
    fp_pow_sqrt(t, a);
    fp_mul(y, t, a);
    fp_sqr(c, y);
    st(out + i * 13, t);
    out[i * 13 + 12] = fp_eq(c, a) ? 1u : 0u;
}

PROBE_FP void probe_fp2_sqrt(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fp2 a, y;
    ld(a, in + i * 24);
    const bool ok = fp2_sqrt(y, a);
    st(out + i * 25, y);
    out[i * 25 + 24] = ok ? 1u : 0u;
}

template <uint32_t OP>
PROBE_FR void probe_fr_bin(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fr a, b, r;
    ld(a, in + i * 16);
    ld(b, in + i * 16 + 8);
    if (OP == OP_FR_ADD) fr_add(r, a, b);
    else if (OP == OP_FR_SUB) fr_sub(r, a, b);
    else fr_mul(r, a, b);
    st(out + i * 8, r);
}

PROBE_FR void probe_fr_inv(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count) {
    size_t i;
    if (!item(i, count)) return;
    Fr a, r;
    ld(a, in + i * 8);
    fr_inv(r, a);
    st(out + i * 8, r);
}

}  // namespace
}  // namespace hbrbc

extern "C" __attribute__((visibility("default")))
int hbprobe_run(uint32_t op, const uint32_t *in, uint32_t *out, size_t count, void *stream) {
    using namespace hbrbc;
    if (count == 0 || op >= OP_COUNT || !in || !out) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((count + kPairBlock - 1) / kPairBlock)), block(kPairBlock);
    hipStream_t s = (hipStream_t)stream;
#define GO(kernel, ...) hipLaunchKernelGGL(kernel, grid, block, 0, s, in, out, count, ##__VA_ARGS__); break
    switch (op) {
    case OP_FP_ADD: GO(probe_fp_lin<OP_FP_ADD>);
    case OP_FP_SUB: GO(probe_fp_lin<OP_FP_SUB>);
    case OP_FP_NEG: GO(probe_fp_lin<OP_FP_NEG>);
    case OP_FP_DBL: GO(probe_fp_lin<OP_FP_DBL>);
    case OP_FP_MUL: GO(probe_fp_mul<OP_FP_MUL>);
    case OP_FP_SQR: GO(probe_fp_mul<OP_FP_SQR>);
    case OP_FP_INV: GO(probe_fp_inv);
    case OP_FP2_MUL: GO(probe_fp2_mul);
    case OP_FP2_SQR: GO(probe_fp2_unary<OP_FP2_SQR>);
    case OP_FP2_INV: GO(probe_fp2_unary<OP_FP2_INV>);
    case OP_FP2_MUL_XI: GO(probe_fp2_unary<OP_FP2_MUL_XI>);
    case OP_FP6_MUL: GO(probe_fp6_mul);
    case OP_FP12_MUL_INL: GO(probe_fp12_mul<true>);
    case OP_FP12_MUL: GO(probe_fp12_mul<false>);
    case OP_FP12_SQR_INL: GO(probe_fp12_sqr<true>);
    case OP_FP12_SQR: GO(probe_fp12_sqr<false>);
    case OP_FP12_MUL_BY_014: GO(probe_fp12_mul_by_014);
    case OP_FP12_CYCLO_SQR: GO(probe_fp12_cyclo_sqr);
    case OP_FP12_FROB1: GO(probe_fp12_frob, 1);
    case OP_FP12_FROB2: GO(probe_fp12_frob, 2);
    case OP_FP12_FROB3: GO(probe_fp12_frob, 3);
    case OP_FP12_INV: GO(probe_fp12_inv);
    case OP_FP_SQRT: GO(probe_fp_sqrt);
    case OP_FP2_SQRT: GO(probe_fp2_sqrt);
    case OP_FR_ADD: GO(probe_fr_bin<OP_FR_ADD>);
    case OP_FR_SUB: GO(probe_fr_bin<OP_FR_SUB>);
    case OP_FR_MUL: GO(probe_fr_bin<OP_FR_MUL>);
    case OP_FR_INV: GO(probe_fr_inv);
    default: return (int)hipErrorInvalidValue;
    }
#undef GO
    return (int)hipGetLastError();
}
