"""Python restatement of the `pairing` crate's compressed point encodings
(`G1Compressed` / `G2Compressed`, `into_affine`), on the curve arithmetic of
oracle/bls_oracle.py.  tests/golden/gen_compressed.py builds its vectors with
it and the tests of the compressed entries read their expectations from it.

Decoding, in order: bit 0x80 of byte 0 must be set; bit 0x40 means infinity,
valid only with every other bit zero; otherwise bit 0x20 says that y is the
larger of y and -y, the rest is x big-endian (G2: x.c1 || x.c0), every
coordinate < p; y = sqrt(x^3 + b), no root being invalid; y or -y by the flag
(integers in Fp; in Fp2 c1 compared first, c0 when the c1 are equal); the
point must have order r.

Status values are the device's: 0 ok, 1 infinity, 2 invalid.
"""
from oracle import bls_oracle as B

P = B.P
OK, INF, BAD = 0, 1, 2
ZERO96, ZERO192 = b"\0" * 96, b"\0" * 192


def _larger_fp(y):
    return y > (-y) % P


def _larger_fp2(y):
    n = ((-y[0]) % P, (-y[1]) % P)
    return (y[1], y[0]) > (n[1], n[0])


def compress_g1(pt):
    """Affine point (or None) -> 48 bytes.  No subgroup check: a point outside
    G1 compresses like any other."""
    if pt is None:
        return b"\xc0" + b"\0" * 47
    b = bytearray(B.fp_bytes(pt[0]))
    b[0] |= 0x80 | (0x20 if _larger_fp(pt[1]) else 0)
    return bytes(b)


def compress_g2(pt):
    if pt is None:
        return b"\xc0" + b"\0" * 95
    (x0, x1), y = pt
    b = bytearray(B.fp_bytes(x1) + B.fp_bytes(x0))
    b[0] |= 0x80 | (0x20 if _larger_fp2(y) else 0)
    return bytes(b)


def parse_g1(raw):
    """Uncompressed 96 bytes of a point on the curve -> affine point or None."""
    if raw[0] & 0x40:
        return None
    return (int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big"))


def parse_g2(raw):
    if raw[0] & 0x40:
        return None
    v = [int.from_bytes(raw[48 * i:48 * i + 48], "big") for i in range(4)]
    return ((v[1], v[0]), (v[3], v[2]))


def decompress_g1(raw):
    """48 bytes -> (status, uncompressed 96 bytes; zero bytes when invalid)."""
    assert len(raw) == 48
    f = raw[0]
    if not f & 0x80:
        return BAD, ZERO96
    if f & 0x40:
        if f & 0x3F or any(raw[1:]):
            return BAD, ZERO96
        return INF, B.g1_bytes(None)
    x = int.from_bytes(bytes([f & 0x1F]) + raw[1:], "big")
    if x >= P:
        return BAD, ZERO96
    a = (x * x * x + B.B1) % P
    y = pow(a, (P + 1) // 4, P)
    if y * y % P != a:
        return BAD, ZERO96
    if _larger_fp(y) != bool(f & 0x20):
        y = (-y) % P
    if not B.g1_in_subgroup((x, y)):
        return BAD, ZERO96
    return OK, B.g1_bytes((x, y))


def decompress_g2(raw):
    """96 bytes -> (status, uncompressed 192 bytes; zero bytes when invalid)."""
    assert len(raw) == 96
    f = raw[0]
    if not f & 0x80:
        return BAD, ZERO192
    if f & 0x40:
        if f & 0x3F or any(raw[1:]):
            return BAD, ZERO192
        return INF, B.g2_bytes(None)
    x1 = int.from_bytes(bytes([f & 0x1F]) + raw[1:48], "big")
    x0 = int.from_bytes(raw[48:], "big")
    if x1 >= P or x0 >= P:
        return BAD, ZERO192
    x = (x0, x1)
    y = B._f2sqrt(B.f2add(B.f2mul(B.f2mul(x, x), x), B.B2))
    if y is None:
        return BAD, ZERO192
    if _larger_fp2(y) != bool(f & 0x20):
        y = B.f2neg(y)
    if not B.g2_in_subgroup((x, y)):
        return BAD, ZERO192
    return OK, B.g2_bytes((x, y))
