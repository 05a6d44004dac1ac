"""Writes tests/golden/keygen_vectors.json: SyncKeyGen vectors (sync_key_gen.rs
:516-608: commitment rows, Part and Ack checks, the generated key set and its
key shares) from the CPU restatement oracle/bls_oracle.py.

Run from the repo root: python tests/golden/gen_keygen.py (a few minutes:
every scalar multiplication is Python integers).  Seeds are fixed, so the file
is reproducible.  Scalars are 32 big-endian bytes, points the compressed
encoding (48 bytes) unless named g96; a bivariate polynomial or commitment is
the list of its (t + 1)(t + 2) / 2 entries (i, j) = (j, i) at position
min(i, j) + max(i, j) (max(i, j) + 1) / 2 (hbbft_amd.keygen.coeff_pos).

The generator asserts its own invariants: every polynomial and commitment is
symmetric; every commitment row at x, formed by point arithmetic, is the
commitment of the polynomial's row at x; every ack value v = f(x, y) satisfies
commit.evaluate(x, y) == [v] G1.
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import bls_oracle as B  # noqa: E402

R, P = B.R, B.P
INF48 = b"\xc0" + b"\0" * 47


def pos(i, j):
    lo, hi = min(i, j), max(i, j)
    return lo + hi * (hi + 1) // 2


def g1_compressed(pt):
    """zkcrypto `G1Compressed`: x big-endian with 0x80 set in byte 0, 0x20 set
    iff y > p - y; infinity = 0xC0 and 47 zero bytes."""
    if pt is None:
        return INF48
    b = bytearray(B.fp_bytes(pt[0]))
    b[0] |= 0x80
    if pt[1] > P - pt[1]:
        b[0] |= 0x20
    return bytes(b)


def fr(v):
    return "%064x" % v


_BASE = {}


def base_mul(k):
    """[k] G1::one() (memoised: the transcripts repeat scalars)."""
    k %= R
    if k not in _BASE:
        _BASE[k] = B.g1_mul(B.G1_GEN, k)
    return _BASE[k]


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def point_eval(points, x):
    """Horner in G1 over affine points (None = infinity)."""
    acc = None
    for c in reversed(points):
        acc = B.g1_add(B.g1_mul(acc, x) if acc is not None and x else None, c)
    return acc


def bivar_row(f, t, x):
    """Coefficients in y of f(x, y)."""
    return [sum(f[pos(i, j)] * pow(x, i, R) for i in range(t + 1)) % R for j in range(t + 1)]


def commit_row(c, t, x):
    return [point_eval([c[pos(i, j)] for i in range(t + 1)], x) for j in range(t + 1)]


def transcript(rng, n, t, ack_senders):
    """All of one key generation: proposer p's polynomial and commitment, node
    m's row of it, and the value sender s puts into its Ack of p for node m."""
    m = (t + 1) * (t + 2) // 2
    polys = [[rng.randrange(1, R) for _ in range(m)] for _ in range(n)]
    commits = [[base_mul(c) for c in f] for f in polys]
    for f in polys:
        assert all(f[pos(i, j)] == f[pos(j, i)] for i in range(t + 1) for j in range(t + 1))
    rows = [[bivar_row(f, t, node + 1) for node in range(n)] for f in polys]
    values = [[[poly_eval(rows[p][s], node + 1) for node in range(n)] for s in range(n)]
              for p in range(n)]
    for p in range(n):
        for node in range(n):
            crow = commit_row(commits[p], t, node + 1)
            assert crow == [base_mul(c) for c in rows[p][node]], ("row", p, node)
            for s in range(n):
                # symmetric: f(node + 1, s + 1) from either row
                assert values[p][s][node] == poly_eval(rows[p][node], s + 1)
                assert point_eval(crow, s + 1) == base_mul(values[p][s][node]), ("ack", p, s, node)
        print("transcript n =", n, "proposer", p, flush=True)
    complete = [p for p in range(n) if len(set(ack_senders[p])) > 2 * t]
    key_set = [None] * (t + 1)
    for p in complete:
        key_set = [B.g1_add(a, commits[p][pos(0, j)]) for j, a in enumerate(key_set)]
    master = [sum(polys[p][pos(0, j)] for p in complete) % R for j in range(t + 1)]
    assert key_set == [base_mul(c) for c in master]
    shares = [point_eval(key_set, i + 1) for i in range(n)]
    assert shares == [base_mul(poly_eval(master, i + 1)) for i in range(n)]
    return {"n": n, "t": t,
            "polys": [[fr(c) for c in f] for f in polys],
            "commitments": [[g1_compressed(c).hex() for c in cm] for cm in commits],
            "rows": [[[fr(c) for c in rows[p][node]] for node in range(n)] for p in range(n)],
            "values": [[[fr(v) for v in values[p][s]] for s in range(n)] for p in range(n)],
            "ack_senders": ack_senders, "complete": complete,
            "key_set": [{"g96": B.g1_bytes(c).hex(), "g48": g1_compressed(c).hex()}
                        for c in key_set],
            "key_shares": [{"g96": B.g1_bytes(s).hex(), "g48": g1_compressed(s).hex()}
                           for s in shares]}


def univariate(rng):
    """A table of points and polynomials over it (lists of table rows, constant
    term first) with the expected evaluation at x."""
    off_group = B.g1_curve_point(0x5EED)
    assert not B.g1_in_subgroup(off_group)
    scal = [rng.randrange(1, R) for _ in range(22)]
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    root = [(-4 * b) % R, (b - 4 * a) % R, a]            # (X - 4)(a X + b)
    assert poly_eval(root, 4) == 0
    table = [base_mul(s) for s in scal] + [None, off_group] + [base_mul(c) for c in root]
    tsc = scal + [0, None] + root
    inf, bad, r0 = 22, 23, 24
    polys = [("degree0", [3]), ("degree1", [5, 9]), ("degree2", [7, 0, 21]),
             ("degree21", list(range(22))), ("infinity_in_the_middle", [1, inf, 2]),
             ("infinity_leading", [4, 6, inf]), ("root_at_4", [r0, r0 + 1, r0 + 2]),
             ("invalid_coefficient", [8, bad, 10]), ("invalid_leading", [8, bad]),
             ("empty", [])]
    xs = {"degree0": [0, 5], "degree1": [1, 100], "degree2": [2, 77],
          "degree21": [0, 1, 2, 64, 65, 0xFFFFFFFF], "infinity_in_the_middle": [3, 0xFFFFFFFF],
          "infinity_leading": [3, 64], "root_at_4": [4, 5], "invalid_coefficient": [0, 2],
          "invalid_leading": [1], "empty": [9]}
    cases = []
    for name, rows in polys:
        for x in xs[name]:
            if any(tsc[r] is None for r in rows):
                st, want = 2, None
            else:
                v = poly_eval([tsc[r] for r in rows], x)
                want = base_mul(v) if v else None
                assert want == point_eval([table[r] for r in rows], x), (name, x)
                st = 0 if want is not None else 1
            cases.append({"name": "%s_at_%d" % (name, x), "rows": rows, "x": x, "status": st,
                          "g96": ("00" * 96) if st == 2 else B.g1_bytes(want).hex(),
                          "g48": ("00" * 48) if st == 2 else g1_compressed(want).hex()})
        print("univariate", name, flush=True)
    assert [c["status"] for c in cases if c["name"].startswith("root_at_4")] == [1, 0]
    return {"table": [g1_compressed(p).hex() for p in table], "cases": cases}


def main():
    rng = random.Random(0x4B455947)
    small = transcript(rng, 4, 1, [[0, 1, 2, 3]] * 4)
    # proposer 6 collects 2t Acks only: not complete, left out of the key set;
    # proposer 5 has a repeated sender, which counts once
    big = transcript(rng, 7, 2, [list(range(7))] * 5 + [[0, 1, 2, 3, 3, 4], [0, 1, 2, 3]])
    assert big["complete"] == [0, 1, 2, 3, 4, 5]

    off_group = g1_compressed(B.g1_curve_point(0x5EED)).hex()
    t0 = small
    wrong_row = fr((int(t0["rows"][2][1][1], 16) + 1) % R)
    wrong_val = fr((int(t0["values"][1][3][1], 16) + 1) % R)
    # each case replaces one item of transcript 0 as node `our_idx` sees it
    tamper = [
        {"name": "row_coefficient_changed", "transcript": 0, "our_idx": 1, "field": "row",
         "part": 2, "index": 1, "bytes": wrong_row, "expect": False},
        {"name": "ack_value_changed", "transcript": 0, "our_idx": 1, "field": "value",
         "part": 1, "index": 3, "bytes": wrong_val, "expect": False},
        {"name": "commitment_point_outside_g1", "transcript": 0, "our_idx": 2, "field": "commit",
         "part": 3, "index": 1, "bytes": off_group, "expect": None},
        {"name": "ack_value_is_r", "transcript": 0, "our_idx": 0, "field": "value",
         "part": 0, "index": 2, "bytes": fr(R), "expect": None},
        {"name": "row_coefficient_is_r", "transcript": 0, "our_idx": 3, "field": "row",
         "part": 1, "index": 0, "bytes": fr(R), "expect": None},
    ]

    comb = json.load(open(os.path.join(ROOT, "tests", "golden", "combine_vectors.json")))
    fe = [int(c, 16) for c in comb["epoch"]["poly"]]
    epoch = [g1_compressed(base_mul(c)).hex() for c in fe]
    pks = {}
    for ct in comb["epoch"]["ciphertexts"]:
        for s in ct["shares"]:
            if s["expect"]:
                pks[s["node"]] = s["pk"]
    for node, pk in pks.items():
        assert pk == B.g1_bytes(base_mul(poly_eval(fe, node + 1))).hex()
    assert sorted(pks) == list(range(comb["epoch"]["n"]))

    out = {"source": "oracle/bls_oracle.py (SyncKeyGen's commitment arithmetic, Python integers)",
           "transcripts": [small, big], "tamper": tamper, "univariate": univariate(rng),
           "epoch_commitment": epoch}
    path = os.path.join(ROOT, "tests", "golden", "keygen_vectors.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
