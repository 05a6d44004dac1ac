"""Writes tests/golden/combine_vectors.json: decryption-share combine vectors
(`PublicKeySet::decrypt` up to g, threshold_decrypt.rs:232-252) from the CPU
restatement oracle/bls_oracle.py.

Run from the repo root: python tests/golden/gen_combine.py (a minute or two:
every scalar multiplication is Python integers).  Every group comes from a
seeded random polynomial f of degree t over Fr and a point U = u G1; node idx
holds the share S = f(idx + 1) U, and the expected result is g = f(0) U.  The
generator itself asserts sum lambda_i S_i == f(0) U with Python-integer
lambda_i = prod_{j != i} x_j / (x_j - x_i), and that the compressed encodings
cover both values of the sign flag 0x20.  Seeds are fixed, so the file is
reproducible.
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import bls_oracle as B  # noqa: E402

R, P = B.R, B.P


def g1_compressed(pt):
    """zkcrypto `G1Compressed`: x big-endian with 0x80 set in byte 0, 0x20 set
    iff y > p - y; infinity = 0xC0 and 47 zero bytes."""
    if pt is None:
        return b"\xc0" + b"\0" * 47
    b = bytearray(B.fp_bytes(pt[0]))
    b[0] |= 0x80
    if pt[1] > P - pt[1]:
        b[0] |= 0x20
    return bytes(b)


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


def group(name, coeffs, u, idx):
    """One fixture group: shares of the polynomial `coeffs` (constant first) on
    U = u G1 at the node indices `idx`."""
    U = B.g1_mul(B.G1_GEN, u)
    vals = [poly_eval(coeffs, i + 1) for i in idx]
    shares = [B.g1_mul(U, v) if v else None for v in vals]
    lam = lagrange(idx)
    want = B.g1_mul(U, coeffs[0]) if coeffs[0] else None
    acc = None
    for l, s in zip(lam, shares):
        acc = B.g1_add(acc, B.g1_mul(s, l) if s is not None else None)
    assert acc == want, name
    assert sum(lam) % R == 1 and sum(l * v for l, v in zip(lam, vals)) % R == coeffs[0], name
    print("group", name, "t =", len(coeffs) - 1, "shares", len(idx), flush=True)
    return {"name": name, "t": len(coeffs) - 1, "poly": ["%064x" % c for c in coeffs],
            "u": "%064x" % u, "idx": list(idx), "shares": [B.g1_bytes(s).hex() for s in shares],
            "lambdas": ["%064x" % l for l in lam], "status": 0 if want is not None else 1,
            "g96": B.g1_bytes(want).hex(), "g48": g1_compressed(want).hex()}


def main():
    rng = random.Random(0x434F4D42)

    def poly(t):
        return [rng.randrange(1, R) for _ in range(t + 1)]

    def scalar():
        return rng.randrange(1, R)

    groups = [group("t0", poly(0), scalar(), [0]),
              group("t1", poly(1), scalar(), [0, 1]),
              group("t2_of_7", poly(2), scalar(), [1, 4, 6])]
    # t = 21 of N = 64: two 22-subsets of one polynomial give the same g
    f21, u21 = poly(21), scalar()
    sub_a = list(range(22))
    sub_b = sorted(rng.sample(range(64), 22))
    assert sub_a != sub_b
    groups += [group("cfg3_a", f21, u21, sub_a), group("cfg3_b", f21, u21, sub_b)]
    assert groups[-1]["g96"] == groups[-2]["g96"]
    groups.append(group("x_2_32", poly(2), scalar(), [0, 5, 0xFFFFFFFF]))
    groups.append(group("f0_zero", [0] + poly(1), scalar(), [2, 3, 5]))
    # a share at infinity: f = (X - 4) (a X + b) has a root at node index 3
    a, b = scalar(), scalar()
    root = [(-4 * b) % R, (b - 4 * a) % R, a]
    assert poly_eval(root, 4) == 0
    groups.append(group("share_at_infinity", root, scalar(), [0, 3, 6]))
    assert "40" + "00" * 95 in groups[-1]["shares"]
    flags = {int(g["g48"][:2], 16) & 0x20 for g in groups if g["status"] == 0}
    assert flags == {0, 0x20}, flags

    # scalar cases of the linear combination on one point
    pt = B.g1_mul(B.G1_GEN, 0xC0FFEE)
    cases = []
    for k in (0, 1, 2, R - 1, 1 << 254):
        want = B.g1_mul(pt, k)
        assert k < R
        cases.append({"k": "%064x" % k, "status": 0 if want is not None else 1,
                      "g96": B.g1_bytes(want).hex(), "g48": g1_compressed(want).hex()})
    cases.append({"k": "%064x" % R, "status": 2, "g96": "00" * 96, "g48": "00" * 48})

    # a small epoch: N = 7, t = 2, two ciphertexts; pk_i = f(i + 1) G1,
    # H = h G2 (standing for hash_g1_g2), U = r G1, W = r H, share_i = f(i + 1) U
    fe = poly(2)
    sks = [poly_eval(fe, i + 1) for i in range(7)]
    pks = [B.g1_mul(B.G1_GEN, s) for s in sks]
    stranger = B.g1_mul(B.G1_GEN, 0x5712A96E12)        # a key of no validator
    off_group = B.g1_curve_point(0x5EED)              # on the curve, outside G1
    assert not B.g1_in_subgroup(off_group)
    cts = []
    for c in range(2):
        h, r_enc = scalar(), scalar()
        H = B.g2_mul(B.G2_GEN, h)
        U = B.g1_mul(B.G1_GEN, r_enc)
        W = B.g2_mul(H, r_enc)
        order = list(range(7))
        rng.shuffle(order)
        sh = []
        for node in order:
            share, pk, expect = B.g1_mul(U, sks[node]), pks[node], True
            if c == 0 and node == 1:       # tampered share
                share, expect = B.g1_add(share, B.G1_GEN), False
            if c == 0 and node == 6:       # key outside the group: invalid
                pk, expect = off_group, False
            if c == 1 and node == 0:       # a key of no validator
                pk, expect = stranger, False
            sh.append({"node": node, "share": B.g1_bytes(share).hex(), "pk": B.g1_bytes(pk).hex(),
                       "expect": expect})
        g = B.g1_mul(U, fe[0])
        cts.append({"hash": B.g2_bytes(H).hex(), "w": B.g2_bytes(W).hex(), "shares": sh,
                    "g96": B.g1_bytes(g).hex(), "g48": g1_compressed(g).hex()})
        print("epoch ciphertext", c, flush=True)
    out = {"source": "oracle/bls_oracle.py (Lagrange interpolation at 0 in G1, Python integers)",
           "groups": groups,
           "scalar_cases": {"point": B.g1_bytes(pt).hex(), "cases": cases},
           "epoch": {"n": 7, "t": 2, "poly": ["%064x" % c for c in fe], "ciphertexts": cts}}
    path = os.path.join(ROOT, "tests", "golden", "combine_vectors.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path, len(groups), "groups", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
