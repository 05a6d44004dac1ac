"""GPU parity of the decryption-share combine (`PublicKeySet::decrypt` up to g,
threshold_decrypt.rs:232-252) against tests/golden/combine_vectors.json
(oracle/bls_oracle.py, Python integers): both encodings and the status of
every group bit-exact, alone, in ragged batches and across block boundaries;
failed groups isolated; Lagrange coefficients against Python-integer values;
the scalar cases of the linear combination; the host-bytes entries; and the
verify-then-combine helper on a small epoch."""
import json
import os

import numpy as np
import pytest

from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "combine_vectors.json")))
GROUPS = {g["name"]: g for g in GOLD["groups"]}
INF96, INF48 = "40" + "00" * 95, "c0" + "00" * 47
ZERO96, ZERO48 = "00" * 96, "00" * 48

pytestmark = pytest.mark.gpu


def _i32(values):
    """Unsigned 32-bit values as the int32 device tensor the wrappers take."""
    import torch
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")


def _bytes_t(rows, width):
    import torch
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)
    return torch.from_numpy(a.copy()).to("cuda:0")


def _prepare(points):
    """g1_prepare table of host-byte points; returns (table, count)."""
    from hbbft_amd import threshold as T
    return T.g1_prepare(_bytes_t(points, 96)), len(points)


@pytest.fixture(scope="module")
def table():
    """Every share of every fixture group in one prepared table: (table,
    count, {group name: first row})."""
    points, first = [], {}
    for g in GOLD["groups"]:
        first[g["name"]] = len(points)
        points += [bytes.fromhex(s) for s in g["shares"]]
    tab, count = _prepare(points)
    return tab, count, first


def _run(tab, count, groups):
    """groups = [(rows, idx)] -> [(g96 hex, g48 hex, status)] through
    decrypt_combine_prepared."""
    from hbbft_amd import threshold as T
    rows = [r for rs, _ in groups for r in rs]
    idx = [i for _, ix in groups for i in ix]
    offs = np.cumsum([0] + [len(rs) for rs, _ in groups])
    o96, o48, st = T.decrypt_combine_prepared(tab, count, _i32(rows), _i32(idx), _i32(offs))
    o96, o48, st = o96.cpu().numpy(), o48.cpu().numpy(), st.cpu().tolist()
    return [(bytes(o96[g]).hex(), bytes(o48[g]).hex(), st[g]) for g in range(len(groups))]


def _fixture_group(first, name):
    g = GROUPS[name]
    return (list(range(first[name], first[name] + len(g["idx"]))), g["idx"])


def _want(name):
    g = GROUPS[name]
    return (g["g96"], g["g48"], g["status"])


def test_fixture_groups_alone_and_in_one_batch(table):
    tab, count, first = table
    names = [g["name"] for g in GOLD["groups"]]
    for name in names:
        assert _run(tab, count, [_fixture_group(first, name)]) == [_want(name)], name
    assert _want("f0_zero") == (INF96, INF48, 1)
    # one ragged batch, with an empty group (the empty sum: infinity) inside
    batch = [_fixture_group(first, n) for n in names]
    batch.insert(3, ([], []))
    want = [_want(n) for n in names]
    want.insert(3, (INF96, INF48, 1))
    assert _run(tab, count, batch) == want


def test_batch_across_block_boundaries(table):
    """67 groups of 3 and 7 groups of 22: 355 shares and 74 groups, neither a
    multiple of the 64-lane block, groups straddling blocks in the per-share
    kernels and the batch spanning two blocks of the per-group kernel."""
    tab, count, first = table
    batch = [_fixture_group(first, "t2_of_7")] * 67 + [_fixture_group(first, "cfg3_a")] * 7
    got = _run(tab, count, batch)
    assert got == [_want("t2_of_7")] * 67 + [_want("cfg3_a")] * 7


def test_failed_groups_are_isolated():
    from hbbft_amd import threshold as T
    t2, t1 = GROUPS["t2_of_7"], GROUPS["t1"]
    off_curve = bytearray(bytes.fromhex(t2["shares"][1]))
    off_curve[-1] ^= 1
    off_group = B.g1_bytes(B.g1_curve_point(0x5EED))   # on the curve, outside G1
    points = [bytes.fromhex(s) for s in t2["shares"] + t1["shares"]] + [bytes(off_curve), off_group]
    tab, count = _prepare(points)
    assert count == 7
    good2, good1 = ([0, 1, 2], t2["idx"]), ([3, 4], t1["idx"])
    batch = [good2,
             ([0, 1, 2], [1, 4, 1]),        # repeated index
             ([0, 5, 2], t2["idx"]),        # a share off the curve
             good1,
             ([0, 6, 2], t2["idx"]),        # a share outside the subgroup
             ([0, 1, 7], t2["idx"]),        # a row past the table
             ([0, -1 & 0xFFFFFFFF, 2], t2["idx"]),   # a negative row
             good2]
    zero = lambda st: (ZERO96, ZERO48, st)  # noqa: E731
    want2, want1 = (t2["g96"], t2["g48"], 0), (t1["g96"], t1["g48"], 0)
    assert _run(tab, count, batch) == [want2, zero(3), zero(2), want1, zero(2), zero(2), zero(2),
                                       want2]
    # the table's size must be that of the count it was prepared with (sizes
    # are rounded to 256 bytes: 15 points need more than 7)
    with pytest.raises(AssertionError):
        T.decrypt_combine_prepared(tab, count + 8, _i32([0]), _i32([0]), _i32([0, 1]))


def _lagrange(idx):
    xs = [i + 1 for i in idx]
    out = []
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if j != i:
                num = num * xj % B.R
                den = den * (xj - xi) % B.R
        out.append(num * pow(den, B.R - 2, B.R) % B.R)
    return out


def test_lagrange_coeffs_match_python_integers():
    from hbbft_amd import threshold as T
    big = list(range(0, 250, 3))                    # 84 of N = 250
    assert len(big) == 84
    sets = [g["idx"] for g in GOLD["groups"]] + [big, [], [7, 2, 7, 9], [0xFFFFFFFF, 0xFFFFFFFE]]
    offs = np.cumsum([0] + [len(s) for s in sets])
    coeffs, st = T.lagrange_coeffs(_i32([i for s in sets for i in s]), _i32(offs))
    coeffs, st = coeffs.cpu().numpy(), st.cpu().tolist()
    assert st == [0] * (len(sets) - 2) + [3, 0]
    for k, s in enumerate(sets):
        got = [bytes(coeffs[j]).hex() for j in range(offs[k], offs[k + 1])]
        if st[k] == 3:     # the lanes of the repeated index write zero bytes
            assert got[0] == got[2] == "00" * 32
            continue
        assert got == ["%064x" % l for l in _lagrange(s)], k
    for k, g in enumerate(GOLD["groups"]):
        assert [bytes(coeffs[j]).hex() for j in range(offs[k], offs[k + 1])] == g["lambdas"]


def test_g1_lincomb_scalar_cases(table):
    from hbbft_amd import threshold as T
    sc = GOLD["scalar_cases"]
    tab, count = _prepare([bytes.fromhex(sc["point"])])
    cases = sc["cases"]
    assert [int(c["k"], 16) for c in cases] == [0, 1, 2, B.R - 1, 1 << 254, B.R]
    n = len(cases)
    o96, o48, st = T.g1_lincomb_prepared(
        tab, count, _i32([0] * n), _bytes_t([bytes.fromhex(c["k"]) for c in cases], 32),
        _i32(range(n + 1)))
    got = [(bytes(o96[i].cpu().numpy()).hex(), bytes(o48[i].cpu().numpy()).hex(), int(st[i]))
           for i in range(n)]
    assert got == [(c["g96"], c["g48"], c["status"]) for c in cases]
    assert got[0] == (INF96, INF48, 1) and got[1][0] == sc["point"] and got[5] == (ZERO96, ZERO48, 2)
    # several terms with explicit scalars: the fixture's lambdas give its g
    tab, count, first = table
    g = GROUPS["t2_of_7"]
    rows = list(range(first["t2_of_7"], first["t2_of_7"] + 3))
    o96, o48, st = T.g1_lincomb_prepared(
        tab, count, _i32(rows), _bytes_t([bytes.fromhex(l) for l in g["lambdas"]], 32), _i32([0, 3]))
    assert (bytes(o96[0].cpu().numpy()).hex(), bytes(o48[0].cpu().numpy()).hex(), int(st[0])) == \
        _want("t2_of_7")


def _host_group(name):
    g = GROUPS[name]
    return [(i, bytes.fromhex(s)) for i, s in zip(g["idx"], g["shares"])]


def test_host_bytes_entries():
    from hbbft_amd import RseError
    from hbbft_amd import threshold as T
    t1, t2 = _host_group("t1"), _host_group("t2_of_7")
    dup = [(t2[0][0], t2[0][1]), (t2[1][0], t2[1][1]), (t2[0][0], t2[2][1])]
    want1 = (bytes.fromhex(GROUPS["t1"]["g96"]), bytes.fromhex(GROUPS["t1"]["g48"]))
    want2 = (bytes.fromhex(GROUPS["t2_of_7"]["g96"]), bytes.fromhex(GROUPS["t2_of_7"]["g48"]))
    assert T.combine_decryption_shares([t1, t2, dup]) == [want1, want2, None]
    assert T.decrypt_combine(t1) == want1
    assert T.decrypt_combine(t2) == want2
    with pytest.raises(RseError) as e:
        T.decrypt_combine(dup)
    assert e.value.code == 100    # HBRBC_E_INVALID_ARG


def test_decrypt_shares_grouped_epoch():
    from hbbft_amd import threshold as T
    ep = GOLD["epoch"]
    t = ep["t"]
    cts = [(bytes.fromhex(c["hash"]), bytes.fromhex(c["w"])) for c in ep["ciphertexts"]]
    shares, items, expect = [], [], []
    for ci, c in enumerate(ep["ciphertexts"]):
        for s in c["shares"]:
            share, pk = bytes.fromhex(s["share"]), bytes.fromhex(s["pk"])
            shares.append((ci, s["node"], share, pk))
            items.append((share, pk, cts[ci][0], cts[ci][1]))
            expect.append(s["expect"])
    assert expect.count(False) == 3
    # interleave the two ciphertexts' shares: input order is not table order
    perm = sorted(range(len(shares)), key=lambda i: (i % 7, i // 7))
    shares, items, expect = ([x[i] for i in perm] for x in (shares, items, expect))
    flags, outs = T.decrypt_shares_grouped(cts, shares, t)
    assert flags == expect == T.verify_decryption_shares(items)
    assert outs == [(bytes.fromhex(c["g96"]), bytes.fromhex(c["g48"])) for c in ep["ciphertexts"]]
    # the combine takes the first t + 1 valid shares by node index: the result
    # is that of exactly those (ciphertext 0: nodes 0, 2, 3 -- 1 is tampered)
    c0 = ep["ciphertexts"][0]
    by_node = {s["node"]: bytes.fromhex(s["share"]) for s in c0["shares"]}
    assert [s["node"] for s in c0["shares"] if not s["expect"]] != []
    assert T.combine_decryption_shares([[(n, by_node[n]) for n in (0, 2, 3)]]) == [outs[0]]
    assert T.combine_decryption_shares([[(n, by_node[n]) for n in (0, 1, 2)]]) != [outs[0]]
    # ciphertext 1 left with t valid shares (and its share under a stranger's key): no output
    keep = [s for s in shares if s[0] == 0]
    valid1 = [s for s, ok in zip(shares, expect) if s[0] == 1 and ok][:t]
    bad1 = [s for s, ok in zip(shares, expect) if s[0] == 1 and not ok]
    flags, outs2 = T.decrypt_shares_grouped(cts, keep + valid1 + bad1, t)
    assert flags == [e for s, e in zip(shares, expect) if s[0] == 0] + [True] * t + [False] * len(bad1)
    assert outs2 == [outs[0], None]
