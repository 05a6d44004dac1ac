// hash_g2.hip -- bytes to group elements and back: `threshold_crypto`'s
// hash_g2, hash_g1_g2 and xor_with_hash (DESIGN.md §6e "Hashes and the pad").
//
// Not a translation unit of its own: pairing.hip includes this file at its
// end, inside namespace hbrbc, because the field, curve and table units it is
// built from live in pairing.hip's anonymous namespace (fp2_sqrt, pt_dbl,
// pt_add_affine, store_result, ...).  The Makefile lists it among pairing.o's
// prerequisites; srchash.py hashes it like every *.hip of this directory.
//
// The definition (tests/hash_ref.py restates it in Python; the crate itself is
// not available to this project, so parity with it is NOT pinned):
//
//   stream(seed32)   ChaCha20 keystream (20 rounds) as little-endian 32-bit
//                    words: key = seed, 64-bit block counter from 0 in state
//                    words 12, 13, words 14, 15 zero.  u32() is the next word,
//                    u64() two words, low first.
//   Fq draw          six u64() as limbs 0..5, the top three bits of limb 5
//                    cleared, redrawn until the 384-bit value v is < p; the
//                    element is v 2^-384 mod p (the crate keeps v as its
//                    Montgomery representation, R = 2^384).  This file's
//                    Montgomery radix is 2^406, so the limb vector is NOT taken
//                    as is: one product with 2^428 mod p gives v 2^22, the
//                    2^406-form of v 2^-384.
//   one attempt      c0 = Fq draw, c1 = Fq draw, greatest = u32() & 1 (drawn
//                    whether or not a root exists); x = c0 + c1 u, y a root of
//                    x^3 + 4 (u + 1), none: next attempt on the same stream;
//                    y or -y by `greatest` in the order of the compressed
//                    encodings (c1 first, then c0).
//   cofactor         the point times the full cofactor of E'(Fp2) (kH2, 507
//                    bits; not reduced mod r: the point is not in G2 yet).
//   hash_g2(m)       the above with seed = sha3_256(m)
//   hash_g1_g2(U, m) hash_g2(m' || compressed48(U)), m' = m when len(m) <= 64,
//                    sha3_256(m) otherwise
//   xor_with_hash(g, data)[i] = data[i] ^ (w_i & 0xff) over
//                    stream(sha3_256(compressed48(g))): a byte per word.
//
// The one stated deviation: the crate draws again when the product with the
// cofactor is the point at infinity (probability about 2^-255); here that is
// status 3 and nothing is redrawn.
//
// Two launches per hash.  The sample kernel (seed, attempt loop) diverges: the
// lanes of a wave accept after different numbers of attempts (about one in
// three is accepted).  The cofactor kernel takes the same branches on every
// lane -- the bits of kH2 are constants -- so its 506 doublings and 255
// additions never run under a partial mask.  (x, y) travels between the two as
// the item's entry of the output table, which the cofactor kernel overwrites.
//
// E'(Fp2) has odd order (kH2 and r are odd), so it has no point of order 2 and
// the complete formulas of pt_dbl / pt_add_affine hold on all of it, not only
// on G2.

namespace {

// ---------------------------------------------------------------- SHA3-256
// of `total` bytes given by get(i), i < total: any alignment, any source (the
// sponges of device_common.hpp want 8-byte-aligned rows with a readable tail
// word).  A byte per load: these messages are tens of bytes.
template <class Get>
DEV void sha3_256_bytes(Get get, uint32_t total, uint32_t (&out)[8]) {
    uint32_t L[25], H[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) L[i] = H[i] = 0u;
    for (uint32_t pos = 0;; pos += 136) {
        const bool last = total - pos < 136u;   // the block that takes the padding
#pragma unroll
        for (int w = 0; w < 17; ++w) {
            uint32_t v[2] = {0u, 0u};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t i = pos + 8 * w + k;
                const uint32_t b = i < total ? get(i) : (i == total ? 0x06u : 0u);
                v[k >> 2] |= b << (8 * (k & 3));
            }
            L[w] ^= v[0];
            H[w] ^= v[1];
        }
        if (last) H[16] ^= 0x80000000u;
        keccak_f1600(L, H);
        if (last) break;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        out[2 * w] = L[w];
        out[2 * w + 1] = H[w];
    }
}

// SHA3-256(head32 || tail48), 80 bytes (hash_g1_g2 with a message above 64
// bytes), or without HEAD SHA3-256(tail48): one block either way.
template <bool HEAD>
DEV void sha3_256_digest_point(const uint32_t *head, const uint8_t *tail48, uint32_t (&out)[8]) {
    constexpr int w0 = HEAD ? 4 : 0;
    uint32_t L[25], H[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) L[i] = H[i] = 0u;
    if (HEAD) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            L[w] = head[2 * w];
            H[w] = head[2 * w + 1];
        }
    }
#pragma unroll
    for (int w = 0; w < 6; ++w) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            L[w0 + w] |= (uint32_t)tail48[8 * w + k] << (8 * k);
            H[w0 + w] |= (uint32_t)tail48[8 * w + 4 + k] << (8 * k);
        }
    }
    L[w0 + 6] = 0x06u;
    H[16] = 0x80000000u;
    keccak_f1600(L, H);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        out[2 * w] = L[w];
        out[2 * w + 1] = H[w];
    }
}

// ---------------------------------------------------------------- ChaCha20
DEV uint32_t rotl32(uint32_t v, int n) { return __builtin_amdgcn_alignbit(v, v, 32 - n); }

#define HB_CHACHA_QR(a, b, c, d)                                                                 \
    s[a] += s[b]; s[d] = rotl32(s[d] ^ s[a], 16);                                                \
    s[c] += s[d]; s[b] = rotl32(s[b] ^ s[c], 12);                                                \
    s[a] += s[b]; s[d] = rotl32(s[d] ^ s[a], 8);                                                 \
    s[c] += s[d]; s[b] = rotl32(s[b] ^ s[c], 7)

// Block `counter` of stream(key): 16 words.
DEV void chacha_block(uint32_t (&out)[16], const uint32_t (&key)[8], uint32_t counter) {
    uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u,
                       key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                       counter, 0u, 0u, 0u};
    uint32_t s[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = in[i];
#pragma unroll 2
    for (int r = 0; r < 10; ++r) {
        HB_CHACHA_QR(0, 4, 8, 12);
        HB_CHACHA_QR(1, 5, 9, 13);
        HB_CHACHA_QR(2, 6, 10, 14);
        HB_CHACHA_QR(3, 7, 11, 15);
        HB_CHACHA_QR(0, 5, 10, 15);
        HB_CHACHA_QR(1, 6, 11, 12);
        HB_CHACHA_QR(2, 7, 8, 13);
        HB_CHACHA_QR(3, 4, 9, 14);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = s[i] + in[i];
}
#undef HB_CHACHA_QR

// The word stream of one lane: `pos` words consumed, the block that holds word
// `pos - 1` in buf.  Lanes of a wave stand at different words, so buf is
// indexed per lane (scratch).
struct ChaStream {
    uint32_t key[8];
    uint32_t buf[16];
    uint32_t pos;
};

NOINL uint32_t cha_u32(ChaStream &s) {
    const uint32_t i = s.pos & 15u;
    if (i == 0) chacha_block(s.buf, s.key, s.pos >> 4);
    ++s.pos;
    return s.buf[i];
}

// A sampler that has drawn this many words gives up (status 2).  An attempt
// takes 25 words and more only after a rejection, and one in three is
// accepted: 2^16 words are some 2,600 attempts, a probability below 2^-1500.
// The bound only keeps a lane from spinning on a stream that never accepts.
constexpr uint32_t kMaxWords = 1u << 16;

DEV bool fp_below_p(const Fp &a) {
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) (void)subb(a.l[i], kP[i], br, &br);
    return br != 0;
}

// Fq draw: twelve words (six u64, low word first, are twelve 32-bit limbs in
// order), 381 bits kept, redrawn until below p.  false: the word bound.
DEV bool fq_draw(ChaStream &cs, Fp &r) {
    Fp v;
    do {
        if (cs.pos >= kMaxWords) return false;
        for (int w = 0; w < NL; ++w) v.l[w] = cha_u32(cs);
        v.l[NL - 1] &= 0x1FFFFFFFu;
    } while (!fp_below_p(v));
    Fp k;
    fp_set(k, kRand384);
    fp_mul(r, v, k);
    return true;
}

// The attempt loop on stream(seed): (x, y) on E'(Fp2) in Montgomery form.
DEV bool sample_curve_point(const uint32_t (&seed)[8], Fp2 &x, Fp2 &y, uint32_t &words) {
    ChaStream cs;
#pragma unroll
    for (int i = 0; i < 8; ++i) cs.key[i] = seed[i];
    cs.pos = 0;
    bool found = false;
    uint32_t greatest = 0;
    while (!found) {
        if (!fq_draw(cs, x.c0) || !fq_draw(cs, x.c1)) break;
        greatest = cha_u32(cs) & 1u;
        Fp2 a, bb;
        fp2_sqr(a, x);
        fp2_mul(a, a, x);
        fp_set(bb.c0, kB1);
        bb.c1 = bb.c0;                                 // 4 (u + 1)
        fp2_add(a, a, bb);
        found = fp2_sqrt(y, a);
    }
    words = cs.pos;
    if (!found) return false;
    Fp c1, c0;
    from_mont(c1, y.c1);
    from_mont(c0, y.c0);
    int cmp = fp_cmp_neg(c1);                          // c1 first, c0 when the c1 are equal
    if (cmp == 0) cmp = fp_cmp_neg(c0);
    if ((cmp > 0) != (greatest != 0)) fp2_neg(y, y);
    return true;
}

// Sample kernel, one lane per item.  Item i hashes msgs[offsets[i] ..
// offsets[i + 1]) -- WITH_U: that message, or its SHA3-256 when it is longer
// than 64 bytes, followed by the 48 bytes at u48 + 48 i -- and writes (x, y)
// as entry i of `tab`, tst[i] = 0, or zeros and tst[i] = 2 for a range that is
// reversed or ends past `total` (nothing of it is read) or a sampler that hit
// kMaxWords.  words_out (nullable): the stream words drawn.
template <bool WITH_U>
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void hash_g2_sample_kernel(
    const uint8_t *__restrict__ u48, const uint8_t *__restrict__ msgs,
    const uint32_t *__restrict__ offsets, size_t count, size_t total, uint32_t *__restrict__ tab,
    uint8_t *__restrict__ tst, uint32_t *__restrict__ words_out) {
    const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= count) return;
    const size_t b = offsets[i], e = offsets[i + 1];
    int st = (b <= e && e <= total) ? PT_OK : PT_BAD;
    Fp2 x, y;
    uint32_t words = 0;
    if (st == PT_OK) {
        const uint8_t *m = msgs + b;
        const uint32_t len = (uint32_t)(e - b);
        uint32_t seed[8];
        if (!WITH_U) {
            sha3_256_bytes([&](uint32_t k) { return (uint32_t)m[k]; }, len, seed);
        } else {
            const uint8_t *u = u48 + 48 * i;
            if (len <= 64) {
                sha3_256_bytes([&](uint32_t k) { return (uint32_t)(k < len ? m[k] : u[k - len]); },
                               len + 48, seed);
            } else {
                uint32_t d[8];
                sha3_256_bytes([&](uint32_t k) { return (uint32_t)m[k]; }, len, d);
                sha3_256_digest_point<true>(d, u, seed);
            }
        }
        if (!sample_curve_point(seed, x, y, words)) st = PT_BAD;
    }
    if (st != PT_OK) {
        fp2_zero(x);
        fp2_zero(y);
    }
    store_affine(tab + i * kG2PtWords, x, y);
    tst[i] = (uint8_t)st;
    if (words_out) words_out[i] = words;
}

// Cofactor kernel, one lane per item: entry j of `tab` times kH2, written back
// as entry j in the form of g2_points_kernel (store_result, as
// g2_mul_table_kernel writes its own) and, where the pointers are non-null, in
// the two encodings.  status[j]: 0, 2 (from the sample kernel; zero bytes), or
// 3 for a product at infinity (the table entry then says infinity, 1).
__global__ __launch_bounds__(kPairBlock) __attribute__((amdgpu_waves_per_eu(kPairWpe, kPairWpe))) void hash_g2_cofactor_kernel(
    size_t count, uint32_t *__restrict__ tab, uint8_t *__restrict__ tst,
    uint8_t *__restrict__ out192, uint8_t *__restrict__ out96, uint8_t *__restrict__ status) {
    const size_t j = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (j >= count) return;
    const int st = tst[j];
    PtProj<Fp2> acc;
    if (st == PT_OK) {
        Fp2 x, y;
        load_affine(tab + j * kG2PtWords, x, y);
        acc.x = x;
        acc.y = y;
        fe_one(acc.z);
        for (int b = kH2Top - 1; b >= 0; --b) {
            pt_dbl(acc);
            if ((kH2[b >> 5] >> (b & 31)) & 1u) pt_add_affine(acc, x, y);
        }
    } else {
        pt_identity(acc);
    }
    const bool inf = st == PT_OK && fp2_is_zero(acc.z);
    store_result(acc, st == PT_OK ? PT_OK : PT_BAD, j, tab, tst, out192, out96, status);
    if (inf) status[j] = 3;
}

// ---------------------------------------------------------------- the pad
constexpr int kPadBlock = 256;

// One lane per row: seeds[8 i ..] = SHA3-256 of the 48 bytes at g48 + 48 i.
__global__ __launch_bounds__(kPadBlock) void pad_seed_kernel(const uint8_t *__restrict__ g48,
                                                            size_t count,
                                                            uint32_t *__restrict__ seeds) {
    const size_t i = (size_t)blockIdx.x * kPadBlock + threadIdx.x;
    if (i >= count) return;
    uint32_t d[8];
    sha3_256_digest_point<false>(nullptr, g48 + 48 * i, d);
#pragma unroll
    for (int w = 0; w < 8; ++w) seeds[8 * i + w] = d[w];
}

// One lane per (row, 16-byte chunk): ChaCha is seekable, chunk c of a row is
// block c of the row's stream, a byte per word.  No prefix table: row r owns
// the lanes from base(r) = offsets[r] / 16 + r on, one per chunk; base(r + 1)
// - base(r) >= ceil(len(r) / 16), so rows never share a lane, at most one lane
// per row idles, and total / 16 + count + 1 lanes cover every description.  A
// lane finds its row by bisection over base (offsets clamped to `total`).
// Row r: data[offsets[r] .. offsets[r + 1]) to the same range of `out` (out
// may be data); a range that is reversed or ends past `total` is status 2 and
// neither read nor written.  The offsets are expected to ascend; where they do
// not, rows may be left unwritten, but every access stays inside a valid
// row's own range.
__global__ __launch_bounds__(kPadBlock) void pad_xor_kernel(
    const uint32_t *__restrict__ seeds, const uint8_t *data, const uint32_t *__restrict__ offsets,
    size_t count, size_t total, size_t lanes, uint8_t *out, uint8_t *__restrict__ status) {
    const size_t lane = (size_t)blockIdx.x * kPadBlock + threadIdx.x;
    if (lane >= lanes) return;
    if (lane < count) {
        const size_t b = offsets[lane], e = offsets[lane + 1];
        status[lane] = (uint8_t)((b <= e && e <= total) ? PT_OK : PT_BAD);
    }
    auto base = [&](size_t r) {
        const size_t o = offsets[r];
        return (o < total ? o : total) / 16 + r;
    };
    size_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (base(mid) <= lane) lo = mid; else hi = mid;
    }
    const size_t r = lo, b = offsets[r], e = offsets[r + 1];
    if (!(b <= e && e <= total)) return;
    const size_t first = base(r);
    if (lane < first) return;
    const size_t c = lane - first, len = e - b;
    if (c * 16 >= len) return;
    const uint32_t n = (uint32_t)(len - c * 16 < 16 ? len - c * 16 : 16);
    uint32_t key[8], w[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) key[k] = seeds[8 * r + k];
    chacha_block(w, key, (uint32_t)c);
    const uint8_t *src = data + b + c * 16;
    uint8_t *dst = out + b + c * 16;
    if (n == 16 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3u) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t pad = (w[4 * q] & 0xFFu) | ((w[4 * q + 1] & 0xFFu) << 8) |
                                 ((w[4 * q + 2] & 0xFFu) << 16) | (w[4 * q + 3] << 24);
            reinterpret_cast<uint32_t *>(dst)[q] = reinterpret_cast<const uint32_t *>(src)[q] ^ pad;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if ((uint32_t)k < n) dst[k] = (uint8_t)(src[k] ^ (uint8_t)w[k]);
    }
}

}  // namespace

hipError_t launch_hash_g2(const uint8_t *u48, const uint8_t *msgs, const uint32_t *offsets,
                          size_t total, TableOut<G2Points> out, uint8_t *out192, uint8_t *out96,
                          uint8_t *status, uint32_t *words, hipStream_t s) {
    if (out.count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((out.count + kPairBlock - 1) / kPairBlock);
    // HBRBC_HASH_G2_PHASE=1 / 2: the sample / the cofactor launch alone, for
    // timing them apart (tools/hash_bench.py).  The cofactor kernel alone
    // multiplies whatever the table holds: its branches are constants, so its
    // time over the points of an earlier call is its time over fresh samples.
    const char *ph = getenv("HBRBC_HASH_G2_PHASE");
    const int phase = ph ? atoi(ph) : 0;
    if (phase == 2) {
        hipLaunchKernelGGL(hash_g2_cofactor_kernel, dim3(blocks), dim3(kPairBlock), 0, s,
                           out.count, out.words, out.status, out192, out96, status);
        return hipGetLastError();
    }
    if (u48)
        hipLaunchKernelGGL(hash_g2_sample_kernel<true>, dim3(blocks), dim3(kPairBlock), 0, s, u48,
                           msgs, offsets, out.count, total, out.words, out.status, words);
    else
        hipLaunchKernelGGL(hash_g2_sample_kernel<false>, dim3(blocks), dim3(kPairBlock), 0, s, u48,
                           msgs, offsets, out.count, total, out.words, out.status, words);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || phase == 1) return e;
    hipLaunchKernelGGL(hash_g2_cofactor_kernel, dim3(blocks), dim3(kPairBlock), 0, s, out.count,
                       out.words, out.status, out192, out96, status);
    return hipGetLastError();
}

hipError_t launch_xor_with_hash(const uint8_t *g48, const uint8_t *data, const uint32_t *offsets,
                                size_t count, size_t total, uint8_t *out, uint8_t *status,
                                uint32_t *seeds, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(pad_seed_kernel, dim3((unsigned)((count + kPadBlock - 1) / kPadBlock)),
                       dim3(kPadBlock), 0, s, g48, count, seeds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t lanes = total / 16 + count + 1;
    hipLaunchKernelGGL(pad_xor_kernel, dim3((unsigned)((lanes + kPadBlock - 1) / kPadBlock)),
                       dim3(kPadBlock), 0, s, seeds, data, offsets, count, total, lanes, out,
                       status);
    return hipGetLastError();
}
