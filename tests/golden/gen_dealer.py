"""Writes tests/golden/dealer_vectors.json: the scalar-field side of share
creation and of SyncKeyGen's dealer (hbrbc_fr_poly_eval, hbrbc_fr_dot and
`generate`'s secret key share, sync_key_gen.rs:523-524), from Python integers
only.

Run from the repo root: python tests/golden/gen_dealer.py (a second).  The
seed is fixed, so the file is reproducible.  Scalars are 32 big-endian bytes in
hex.  The secret key shares are those of the two transcripts of
keygen_vectors.json, whose polynomials and ack senders this generator reads.

The generator asserts its own invariants: every interpolation at 0 of t + 1
values of a part is the part's f(0, node + 1), and every node's secret key
share is the master polynomial -- the sum of the complete parts' f(0, y) -- at
node + 1, so [sk_i] G1::one() is the fixture's key share i.
"""
import json
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# the order of BLS12-381's G1, G2 and GT: the modulus of Fr
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def fr(v):
    return "%064x" % v


def pos(i, j):
    lo, hi = min(i, j), max(i, j)
    return lo + hi * (hi + 1) // 2


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def interpolate_at_0(pairs):
    """`Poly::interpolate(pairs).evaluate(0)` for pairs (x, value)."""
    acc = 0
    for xi, vi in pairs:
        num = den = 1
        for xj, _ in pairs:
            if xj != xi:
                num = num * xj % R
                den = den * (xj - xi) % R
        acc = (acc + vi * num * pow(den, R - 2, R)) % R
    return acc


def poly_cases(rng):
    """A scalar table and polynomials over it (lists of table rows, constant
    term first): `evals` name (polynomial, x) with the expected value."""
    table = [rng.randrange(1, R) for _ in range(22)] + [0, R - 1, R]
    zero, top, bad = 22, 23, 24
    polys = [("degree0", [3]), ("degree1", [5, 9]), ("degree21", list(range(22))),
             ("empty", []), ("zero_and_r_minus_1", [zero, top, top]),
             ("coefficient_is_r", [1, bad, 2]), ("row_negative", [4, -1]),
             ("row_past_the_end", [len(table), 6])]
    xs = [0, 1, 2, 64, 0xFFFFFFFF]
    evals = []
    for p, (name, rows) in enumerate(polys):
        for x in xs:
            ok = all(0 <= r < len(table) and table[r] < R for r in rows)
            # x = 0 reads the constant term alone in exact arithmetic, but the
            # entry walks every coefficient: an invalid one is status 2 at any x
            v = poly_eval([table[r] for r in rows], x) if ok else 0
            evals.append({"name": "%s_at_%d" % (name, x), "poly": p, "x": x,
                          "status": 0 if ok else 2, "value": fr(v)})
    for p in (-1, len(polys)):
        evals.append({"name": "poly_%d" % p, "poly": p, "x": 3, "status": 2, "value": fr(0)})
    deg21 = [table[r] for r in range(22)]
    assert poly_eval(deg21, 0) == table[0] and poly_eval(deg21, 1) == sum(deg21) % R
    assert poly_eval([], 7) == 0
    return {"table": [fr(v) for v in table], "polys": [{"name": n, "rows": r} for n, r in polys],
            "evals": evals}


def dot_cases(rng):
    groups = []
    for name, n in (("empty", 0), ("one", 1), ("terms22", 22), ("terms65", 65),
                    ("operand_is_r", 22), ("edge_values", 4)):
        a = [rng.randrange(R) for _ in range(n)]
        b = [rng.randrange(R) for _ in range(n)]
        if name == "operand_is_r":
            b[13] = R
        if name == "edge_values":
            a, b = [0, R - 1, R - 1, 1], [R - 1, R - 1, 1, 0]
        ok = all(v < R for v in a + b)
        v = sum(x * y for x, y in zip(a, b)) % R if ok else 0
        groups.append({"name": name, "a": [fr(x) for x in a], "b": [fr(x) for x in b],
                       "status": 0 if ok else 2, "value": fr(v)})
    return groups


def secret_shares(tr):
    """Per node the secret key share of `generate`, and per (node, complete
    part) the pairs it interpolates: the first t + 1 distinct ack senders in
    ascending order, x = sender + 1, value = values[p][sender][node]."""
    n, t = tr["n"], tr["t"]
    polys = [[int(c, 16) for c in f] for f in tr["polys"]]
    complete = [p for p in range(n) if len(set(tr["ack_senders"][p])) > 2 * t]
    assert complete == tr["complete"]
    master = [sum(polys[p][pos(0, j)] for p in complete) % R for j in range(t + 1)]
    out = []
    for node in range(n):
        sk = 0
        for p in complete:
            senders = sorted(set(tr["ack_senders"][p]))[:t + 1]
            pairs = [(s + 1, int(tr["values"][p][s][node], 16)) for s in senders]
            part = interpolate_at_0(pairs)
            # f_p(0, node + 1): the row of x = 0 evaluated at the node
            assert part == poly_eval([polys[p][pos(0, j)] for j in range(t + 1)], node + 1)
            sk = (sk + part) % R
        assert sk == poly_eval(master, node + 1), ("sk_i == master(i + 1)", node)
        out.append(fr(sk))
    return {"n": n, "t": t, "complete": complete, "master": [fr(c) for c in master],
            "secret_key_shares": out}


def main():
    rng = random.Random(0x4445414C)
    keygen = json.load(open(os.path.join(ROOT, "tests", "golden", "keygen_vectors.json")))
    big = keygen["transcripts"][1]
    assert big["n"] == 7 and big["complete"] == [0, 1, 2, 3, 4, 5]   # part 6: 2t Acks only
    assert len(big["ack_senders"][5]) != len(set(big["ack_senders"][5]))   # a repeated sender
    out = {"source": "Python integers (tests/golden/gen_dealer.py)",
           "poly_eval": poly_cases(rng), "dot": dot_cases(rng),
           "transcripts": [secret_shares(tr) for tr in keygen["transcripts"]]}
    path = os.path.join(ROOT, "tests", "golden", "dealer_vectors.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
