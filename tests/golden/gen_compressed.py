"""Writes tests/golden/compressed_vectors.json: compressed G1 / G2 encodings
(zkcrypto `G1Compressed` / `G2Compressed`, the form hbbft's messages carry)
with the status and the uncompressed encoding that `into_affine` gives each.

Run from the repo root: python tests/golden/gen_compressed.py (under a minute).
Points come from oracle/bls_oracle.py; the decoding rules are restated in
tests/compressed_ref.py, and every case is built here from the point itself
(or from the rule it breaks) and then run through that restatement, which must
agree.  Seeds are fixed, so the file is reproducible.

Cases per group: valid points k G, some with their negatives (same x, the other
sign flag); infinity; infinity with the sign flag or a trailing byte set; a
valid encoding without the compression flag; x = p (and for G2 x.c0 = p under
a valid x.c1); an x with no y on the curve; a point of the curve outside the
order-r subgroup; a valid x under the other sign flag, which is -P and not P.
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import bls_oracle as B  # noqa: E402
import compressed_ref as C  # noqa: E402

P, R = B.P, B.R


def group(tag, gen, mul, neg, to_bytes, compress, decompress, width, no_root, off_point, extra):
    """The cases of one group: [{name, c, status, u}]."""
    rng = random.Random(0x434F4D50 + width)
    zero = b"\0" * (2 * width)
    cases = []

    def add(name, c, status, u):
        assert len(c) == width and len(u) == 2 * width, name
        assert decompress(c) == (status, u), name
        cases.append({"name": name, "c": c.hex(), "status": status, "u": u.hex()})

    pts = [mul(gen, k) for k in [1, 2, R - 1] + [rng.randrange(1, R) for _ in range(5)]]
    for i, pt in enumerate(pts):
        add("%s_valid_%d" % (tag, i), compress(pt), C.OK, to_bytes(pt))
        if i in (3, 4, 5):
            add("%s_valid_%d_neg" % (tag, i), compress(neg(pt)), C.OK, to_bytes(neg(pt)))
    flags = {int(c["c"][:2], 16) & 0x20 for c in cases}
    assert flags == {0, 0x20}, flags
    inf = b"\xc0" + b"\0" * (width - 1)
    add(tag + "_infinity", inf, C.INF, to_bytes(None))
    add(tag + "_infinity_with_sign_flag", b"\xe0" + inf[1:], C.BAD, zero)
    add(tag + "_infinity_with_trailing_byte", inf[:-1] + b"\x01", C.BAD, zero)
    ok = compress(pts[3])
    add(tag + "_compression_flag_clear", bytes([ok[0] & 0x7F]) + ok[1:], C.BAD, zero)
    # p's top byte is 0x1a: it survives the mask of the three flag bits
    xp = bytearray(P.to_bytes(48, "big") + ok[48:])
    xp[0] |= 0x80
    add(tag + "_x_is_p", bytes(xp), C.BAD, zero)
    for name, c in extra(ok):
        add(tag + name, c, C.BAD, zero)
    add(tag + "_x_without_root", no_root, C.BAD, zero)
    off = compress(off_point)
    add(tag + "_outside_subgroup", off, C.BAD, zero)
    add(tag + "_outside_subgroup_neg", bytes([off[0] ^ 0x20]) + off[1:], C.BAD, zero)
    # the other sign flag on a valid x: -P, not P
    for i in (0, 6):
        c = compress(pts[i])
        add("%s_other_flag_%d" % (tag, i), bytes([c[0] ^ 0x20]) + c[1:], C.OK,
            to_bytes(neg(pts[i])))
        assert to_bytes(neg(pts[i])) != to_bytes(pts[i])
    print(tag, len(cases), "cases", flush=True)
    return cases


def main():
    # x = 1 on E: 1 + 4 = 5 is no square in Fp
    assert pow(5, (P - 1) // 2, P) == P - 1
    g1_no_root = bytearray((1).to_bytes(48, "big"))
    g1_no_root[0] |= 0x80
    # x = 6 + u on the twist: x^3 + 4 (u + 1) has no root in Fp2
    x = (6, 1)
    assert B._f2sqrt(B.f2add(B.f2mul(B.f2mul(x, x), x), B.B2)) is None
    g2_no_root = bytearray(B.fp_bytes(1) + B.fp_bytes(6))
    g2_no_root[0] |= 0x80
    off1, off2 = B.g1_curve_point(0x5EED), B.g2_curve_point(0x5EED)
    assert B.g1_on_curve(off1) and not B.g1_in_subgroup(off1)
    assert B.g2_on_curve(off2) and not B.g2_in_subgroup(off2)

    def g2_neg(pt):
        return None if pt is None else (pt[0], B.f2neg(pt[1]))

    def g2_extra(ok):
        # x.c0 = p under a valid x.c1
        return [("_x_c0_is_p", ok[:48] + P.to_bytes(48, "big"))]

    out = {"source": "oracle/bls_oracle.py points, tests/compressed_ref.py decoding rules",
           "g1": group("g1", B.G1_GEN, B.g1_mul, B.g1_neg, B.g1_bytes, C.compress_g1,
                       C.decompress_g1, 48, bytes(g1_no_root), off1, lambda ok: []),
           "g2": group("g2", B.G2_GEN, B.g2_mul, g2_neg, B.g2_bytes, C.compress_g2,
                       C.decompress_g2, 96, bytes(g2_no_root), off2, g2_extra)}
    path = os.path.join(ROOT, "tests", "golden", "compressed_vectors.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
