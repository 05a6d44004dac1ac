"""Writes tests/golden/sign_vectors.json: threshold-signature vectors
(`ThresholdSign`, threshold_sign.rs:216-270: share checks, `combine_signatures`
and the check of the combined signature) from the CPU restatement
oracle/bls_oracle.py.

Run from the repo root: python tests/golden/gen_sign.py (a minute or two: every
scalar multiplication is Python integers).  Every group comes from a seeded
random polynomial f of degree t over Fr and a point H = h G2 (standing for
hash_g2(doc)); node idx holds the share S = f(idx + 1) H, and the expected
signature is f(0) H.  The generator itself asserts sum lambda_i S_i == f(0) H
with Python-integer lambda_i = prod_{j != i} x_j / (x_j - x_i), and that the
compressed encodings cover both values of the sign flag 0x20.  Every result
carries its parity (the XOR of all bits of the uncompressed encoding).  Seeds
are fixed, so the file is reproducible.
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import bls_oracle as B  # noqa: E402

R, P = B.R, B.P


def g2_compressed(pt):
    """zkcrypto `G2Compressed`: x.c1 || x.c0 big-endian with 0x80 set in byte
    0, 0x20 set iff y is the larger of y and -y (c1 compared first, c0 only
    when the c1 are equal); infinity = 0xC0 and 95 zero bytes."""
    if pt is None:
        return b"\xc0" + b"\0" * 95
    (x0, x1), (y0, y1) = pt
    b = bytearray(B.fp_bytes(x1) + B.fp_bytes(x0))
    b[0] |= 0x80
    ny0, ny1 = (-y0) % P, (-y1) % P
    if (y1, y0) > (ny1, ny0):
        b[0] |= 0x20
    return bytes(b)


def parity(enc):
    """The XOR of all bits of an encoding."""
    acc = 0
    for byte in enc:
        acc ^= byte
    return bin(acc).count("1") & 1


def result(pt):
    enc = B.g2_bytes(pt)
    return {"status": 0 if pt is not None else 1, "sig192": enc.hex(),
            "sig96": g2_compressed(pt).hex(), "parity": parity(enc)}


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def lagrange(idx):
    xs = [i + 1 for i in idx]
    out = []
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if j != i:
                num = num * xj % R
                den = den * (xj - xi) % R
        out.append(num * pow(den, R - 2, R) % R)
    return out


def group(name, coeffs, h, idx):
    """One fixture group: shares of the polynomial `coeffs` (constant first) on
    H = h G2 at the node indices `idx`."""
    H = B.g2_mul(B.G2_GEN, h)
    vals = [poly_eval(coeffs, i + 1) for i in idx]
    shares = [B.g2_mul(H, v) if v else None for v in vals]
    lam = lagrange(idx)
    want = B.g2_mul(H, coeffs[0]) if coeffs[0] else None
    acc = None
    for l, s in zip(lam, shares):
        acc = B.g2_add(acc, B.g2_mul(s, l) if s is not None else None)
    assert acc == want, name
    assert sum(lam) % R == 1 and sum(l * v for l, v in zip(lam, vals)) % R == coeffs[0], name
    print("group", name, "t =", len(coeffs) - 1, "shares", len(idx), flush=True)
    out = {"name": name, "t": len(coeffs) - 1, "poly": ["%064x" % c for c in coeffs],
           "h": "%064x" % h, "idx": list(idx), "shares": [B.g2_bytes(s).hex() for s in shares],
           "lambdas": ["%064x" % l for l in lam]}
    out.update(result(want))
    return out


def main():
    rng = random.Random(0x5349474E)

    def poly(t):
        return [rng.randrange(1, R) for _ in range(t + 1)]

    def scalar():
        return rng.randrange(1, R)

    groups = [group("t0", poly(0), scalar(), [0]),
              group("t1", poly(1), scalar(), [0, 1]),
              group("t2_of_7", poly(2), scalar(), [1, 4, 6])]
    # t = 21 of N = 64: two 22-subsets of one polynomial give the same signature
    f21, h21 = poly(21), scalar()
    sub_a = list(range(22))
    sub_b = sorted(rng.sample(range(64), 22))
    assert sub_a != sub_b
    groups += [group("cfg3_a", f21, h21, sub_a), group("cfg3_b", f21, h21, sub_b)]
    assert groups[-1]["sig192"] == groups[-2]["sig192"]
    groups.append(group("x_2_32", poly(2), scalar(), [0, 5, 0xFFFFFFFF]))
    groups.append(group("f0_zero", [0] + poly(1), scalar(), [2, 3, 5]))
    assert groups[-1]["status"] == 1 and groups[-1]["parity"] == 1
    # a share at infinity: f = (X - 4) (a X + b) has a root at node index 3
    a, b = scalar(), scalar()
    root = [(-4 * b) % R, (b - 4 * a) % R, a]
    assert poly_eval(root, 4) == 0
    groups.append(group("share_at_infinity", root, scalar(), [0, 3, 6]))
    assert "40" + "00" * 191 in groups[-1]["shares"]
    flags = {int(g["sig96"][:2], 16) & 0x20 for g in groups if g["status"] == 0}
    assert flags == {0, 0x20}, flags

    # scalar cases of the linear combination on one point: the edges of the
    # split k = k1 + k2 x^2 (k2 = 0 against 1; r - 1 = (x^2 - 1) x^2, k1 = 0)
    x2 = B.X_ABS * B.X_ABS
    assert R - 1 == (x2 - 1) * x2
    pt = B.g2_mul(B.G2_GEN, 0xC0FFEE)
    cases = []
    for k in (0, 1, 2, x2 - 1, x2, x2 + 1, R - 1, 1 << 254):
        assert k < R
        c = {"k": "%064x" % k}
        c.update(result(B.g2_mul(pt, k)))
        cases.append(c)
    cases.append({"k": "%064x" % R, "status": 2, "sig192": "00" * 192, "sig96": "00" * 96,
                  "parity": 0})
    print("scalar cases", flush=True)

    # a small epoch: N = 7, t = 2, two documents; pk_i = f(i + 1) G1, public
    # key f(0) G1, H = h G2 (standing for hash_g2(doc)), share_i = f(i + 1) H
    fe = poly(2)
    sks = [poly_eval(fe, i + 1) for i in range(7)]
    pks = [B.g1_mul(B.G1_GEN, s) for s in sks]
    stranger = B.g1_mul(B.G1_GEN, 0x5712A96E12)        # a key of no validator
    off_g1 = B.g1_curve_point(0x5EED)                 # on the curve, outside G1
    assert not B.g1_in_subgroup(off_g1)
    off_g2 = B.g2_curve_point(0x5EED)                 # on the twist, outside G2
    assert B.g2_on_curve(off_g2) and not B.g2_in_subgroup(off_g2)
    docs = []
    for d in range(2):
        H = B.g2_mul(B.G2_GEN, scalar())
        order = list(range(7))
        rng.shuffle(order)
        sh = []
        for node in order:
            share, pk, expect = B.g2_mul(H, sks[node]), pks[node], True
            if d == 0 and node == 1:       # tampered share
                share, expect = B.g2_add(share, B.G2_GEN), False
            if d == 0 and node == 4:       # share outside the subgroup: invalid
                share, expect = off_g2, False
            if d == 0 and node == 6:       # key outside the group: invalid
                pk, expect = off_g1, False
            if d == 1 and node == 0:       # a key of no validator
                pk, expect = stranger, False
            if d == 1 and node == 3:       # a valid point, but e(pk, H) != 1
                share, expect = None, False
            sh.append({"node": node, "share": B.g2_bytes(share).hex(), "pk": B.g1_bytes(pk).hex(),
                       "expect": expect})
        doc = {"hash": B.g2_bytes(H).hex(), "shares": sh, "verified": True}
        doc.update(result(B.g2_mul(H, fe[0])))
        docs.append(doc)
        print("epoch document", d, flush=True)
    out = {"source": "oracle/bls_oracle.py (Lagrange interpolation at 0 in G2, Python integers)",
           "groups": groups,
           "scalar_cases": {"point": B.g2_bytes(pt).hex(), "cases": cases},
           "epoch": {"n": 7, "t": 2, "poly": ["%064x" % c for c in fe],
                     "public_key": B.g1_bytes(B.g1_mul(B.G1_GEN, fe[0])).hex(),
                     "stranger_key": B.g1_bytes(stranger).hex(), "documents": docs}}
    path = os.path.join(ROOT, "tests", "golden", "sign_vectors.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path, len(groups), "groups", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
