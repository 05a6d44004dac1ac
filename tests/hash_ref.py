"""Python definition of `threshold_crypto`'s byte <-> group functions as this
project implements them: hash_g2, hash_g1_g2, xor_with_hash, and the encrypt /
decrypt built on them.  The crate is not available here, so this file IS the
definition (DESIGN.md §6e "Hashes and the pad"): restated from `pairing` 0.14
`G2::rand` driven by `rand_chacha` 0.1 `ChaChaRng::from_seed`, anchored by
hashlib (SHA3), `openssl enc -chacha20` (the block function) and the cofactor
polynomial; the order of the draws is recalled, not pinned.

tests/golden/gen_hash_g2.py builds its vectors with it and the GPU tests read
their expectations from those vectors.
"""
import hashlib

from oracle import bls_oracle as B
from tests import compressed_ref as C

P = B.P
MASK32 = 0xFFFFFFFF
# the full cofactor of E'(Fp2), 507 bits (not reduced mod r)
H2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5
R384_INV = pow(1 << 384, -1, P)


def cofactor_from_x():
    """h2 from the BLS parameter: (x^8 - 4x^7 + 5x^6 - 4x^4 + 6x^3 - 4x^2 - 4x + 13) / 9."""
    x = -B.X_ABS
    n = x**8 - 4 * x**7 + 5 * x**6 - 4 * x**4 + 6 * x**3 - 4 * x**2 - 4 * x + 13
    assert n % 9 == 0
    return n // 9


def sha3(b):
    return hashlib.sha3_256(bytes(b)).digest()


def _rotl(v, n):
    return ((v << n) | (v >> (32 - n))) & MASK32


def chacha_block(key32, counter):
    """The 16 little-endian words of ChaCha20 block `counter` (64-bit counter in
    state words 12, 13; words 14, 15 zero)."""
    k = [int.from_bytes(key32[4 * i:4 * i + 4], "little") for i in range(8)]
    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + k + \
           [counter & MASK32, (counter >> 32) & MASK32, 0, 0]
    s = list(init)

    def qr(a, b, c, d):
        s[a] = (s[a] + s[b]) & MASK32; s[d] = _rotl(s[d] ^ s[a], 16)
        s[c] = (s[c] + s[d]) & MASK32; s[b] = _rotl(s[b] ^ s[c], 12)
        s[a] = (s[a] + s[b]) & MASK32; s[d] = _rotl(s[d] ^ s[a], 8)
        s[c] = (s[c] + s[d]) & MASK32; s[b] = _rotl(s[b] ^ s[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return [(a + b) & MASK32 for a, b in zip(s, init)]


class Stream:
    """stream(seed32): the keystream as 32-bit words; `words` counts the draws."""

    def __init__(self, seed32):
        assert len(seed32) == 32
        self.key, self.words, self._block, self._buf = bytes(seed32), 0, -1, None

    def u32(self):
        b, i = divmod(self.words, 16)
        if b != self._block:
            self._block, self._buf = b, chacha_block(self.key, b)
        self.words += 1
        return self._buf[i]

    def u64(self):
        lo = self.u32()
        return lo | (self.u32() << 32)


def fq_draw(st):
    """-> (field element, rejections)."""
    rej = 0
    while True:
        v = 0
        for i in range(6):
            limb = st.u64()
            if i == 5:
                limb &= (1 << 61) - 1
            v |= limb << (64 * i)
        if v < P:
            return v * R384_INV % P, rej
        rej += 1


def sample(seed32):
    """The attempt loop: -> ((x, y) on E'(Fp2) before the cofactor, words, trace)."""
    st = Stream(seed32)
    trace = {"rej_c0": 0, "rej_c1": 0, "nonsquare": 0}
    while True:
        c0, r0 = fq_draw(st)
        c1, r1 = fq_draw(st)
        greatest = st.u32() & 1
        trace["rej_c0"] += r0
        trace["rej_c1"] += r1
        x = (c0, c1)
        y = B._f2sqrt(B.f2add(B.f2mul(B.f2mul(x, x), x), B.B2))
        if y is None:
            trace["nonsquare"] += 1
            continue
        ny = B.f2neg(y)
        trace["greatest"] = greatest
        # of the root as B._f2sqrt returns it (the device's own root may be the
        # other one): with `greatest` it says whether the choice negated it
        trace["y_lt_neg"] = not C._larger_fp2(y)
        lo, hi = (ny, y) if C._larger_fp2(y) else (y, ny)
        return (x, hi if greatest else lo), st.words, trace


def cofactor_mul(pt):
    return B._smul(B.g2_add, pt, H2)


def hash_g2_seeded(seed32):
    pt, words, trace = sample(seed32)
    return cofactor_mul(pt), pt, words, trace


def hash_g2(msg):
    """-> (point or None, point before the cofactor, words, trace)."""
    return hash_g2_seeded(sha3(msg))


def hash_g1_g2_input(u48, msg):
    assert len(u48) == 48
    m = bytes(msg) if len(msg) <= 64 else sha3(msg)
    return m + bytes(u48)


def hash_g1_g2(u48, msg):
    return hash_g2(hash_g1_g2_input(u48, msg))


def pad_bytes(seed32, n):
    st = Stream(seed32)
    return bytes(st.u32() & 0xFF for _ in range(n))


def xor_with_hash(g48, data):
    pad = pad_bytes(sha3(g48), len(data))
    return bytes(a ^ b for a, b in zip(data, pad))


def encrypt(pk, msg, r):
    """pk an affine G1 point, r a scalar in [1, r) -> (U48, V, W96)."""
    u = C.compress_g1(B.g1_mul(B.G1_GEN, r))
    v = xor_with_hash(C.compress_g1(B.g1_mul(pk, r)), msg)
    h = hash_g1_g2(u, v)[0]
    return u, v, C.compress_g2(B.g2_mul(h, r))
