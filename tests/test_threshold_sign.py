"""GPU parity of the threshold-signature path (`ThresholdSign`,
threshold_sign.rs:216-270) against tests/golden/sign_vectors.json
(oracle/bls_oracle.py, Python integers): the G2 combine's two encodings, parity
and status of every group bit-exact, alone, in ragged batches and across block
boundaries; failed groups isolated; the scalar cases of the linear combination
(the edges of the endomorphism split); the share check against the existing
pairing_check_batch and the fixture's expectations; the host-bytes entries;
and the whole of ThresholdSign on a small epoch."""
import json
import os

import numpy as np
import pytest

from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "sign_vectors.json")))
GROUPS = {g["name"]: g for g in GOLD["groups"]}
EPOCH = GOLD["epoch"]
INF192, INF96 = "40" + "00" * 191, "c0" + "00" * 95
ZERO192, ZERO96 = "00" * 192, "00" * 96
OFF_G1 = B.g1_bytes(B.g1_curve_point(0x5EED))   # on the curve, outside G1
OFF_G2 = B.g2_bytes(B.g2_curve_point(0x5EED))   # on the twist, outside G2

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
    """g2_points_prepare table of host-byte points; returns (table, count)."""
    from hbbft_amd import threshold as T
    return T.g2_points_prepare(_bytes_t(points, 192)), len(points)


@pytest.fixture(scope="module")
def table():
    """Every share of every fixture group in one point table: (table, count,
    {group name: first row})."""
    points, first = [], {}
    for g in GOLD["groups"]:
        first[g["name"]] = len(points)
        points += [bytes.fromhex(s) for s in g["shares"]]
    tab, count = _prepare(points)
    return tab, count, first


def _rows(out):
    o192, o96, par, st = (t.cpu().numpy() for t in out)
    return [(bytes(o192[g]).hex(), bytes(o96[g]).hex(), int(par[g]), int(st[g]))
            for g in range(len(st))]


def _run(tab, count, groups):
    """groups = [(rows, idx)] -> [(sig192 hex, sig96 hex, parity, status)]
    through sig_combine_prepared."""
    from hbbft_amd import threshold as T
    rows = [r for rs, _ in groups for r in rs]
    idx = [i for _, ix in groups for i in ix]
    offs = np.cumsum([0] + [len(rs) for rs, _ in groups])
    return _rows(T.sig_combine_prepared(tab, count, _i32(rows), _i32(idx), _i32(offs)))


def _fixture_group(first, name):
    g = GROUPS[name]
    return (list(range(first[name], first[name] + len(g["idx"]))), g["idx"])


def _want(g):
    if isinstance(g, str):
        g = GROUPS[g]
    return (g["sig192"], g["sig96"], g["parity"], g["status"])


def test_fixture_groups_alone_and_in_one_batch(table):
    tab, count, first = table
    names = [g["name"] for g in GOLD["groups"]]
    for name in names:
        assert _run(tab, count, [_fixture_group(first, name)]) == [_want(name)], name
    assert _want("f0_zero") == (INF192, INF96, 1, 1)
    assert _want("cfg3_a") == _want("cfg3_b")
    # one ragged batch, with an empty group (the empty sum: infinity) inside
    batch = [_fixture_group(first, n) for n in names]
    batch.insert(3, ([], []))
    want = [_want(n) for n in names]
    want.insert(3, (INF192, INF96, 1, 1))
    assert _run(tab, count, batch) == want


def test_batch_across_block_boundaries():
    """67 groups of 3 and 7 groups of 22, each on table rows of its own: 355
    shares and 74 groups, neither a multiple of the 64-lane block, groups
    straddling blocks in the per-share kernels and the batch spanning two
    blocks of the per-group kernel."""
    t2, c3 = GROUPS["t2_of_7"], GROUPS["cfg3_a"]
    reps = [t2] * 67 + [c3] * 7
    points, batch = [], []
    for g in reps:
        batch.append((list(range(len(points), len(points) + len(g["idx"]))), g["idx"]))
        points += [bytes.fromhex(s) for s in g["shares"]]
    assert len(points) == 355
    tab, count = _prepare(points)
    assert _run(tab, count, batch) == [_want(g) for g in reps]


def test_failed_groups_are_isolated():
    from hbbft_amd import threshold as T
    t2, t1 = GROUPS["t2_of_7"], GROUPS["t1"]
    big_x = bytearray(bytes.fromhex(t2["shares"][1]))
    big_x[48:96] = B.P.to_bytes(48, "big")               # x.c0 = p: not canonical
    off_curve = bytearray(bytes.fromhex(t2["shares"][1]))
    off_curve[-1] ^= 1
    points = [bytes.fromhex(s) for s in t2["shares"] + t1["shares"]] + [
        bytes(big_x), bytes(off_curve), OFF_G2]
    tab, count = _prepare(points)
    assert count == 8
    good2, good1 = ([0, 1, 2], t2["idx"]), ([3, 4], t1["idx"])
    batch = [good2,
             ([0, 1, 2], [1, 4, 1]),        # repeated index
             good1,
             ([0, 5, 2], t2["idx"]),        # a coordinate >= p
             good2,
             ([0, 6, 2], t2["idx"]),        # a share off the twist
             good1,
             ([0, 7, 2], t2["idx"]),        # on the twist, outside the subgroup
             good2,
             ([0, 1, 8], t2["idx"]),        # a row past the table
             good1,
             ([0, -1 & 0xFFFFFFFF, 2], t2["idx"]),   # a negative row
             good2]
    zero = lambda st: (ZERO192, ZERO96, 0, st)  # noqa: E731
    w2, w1 = _want(t2), _want(t1)
    assert _run(tab, count, batch) == [w2, zero(3), w1, zero(2), w2, zero(2), w1, zero(2), w2,
                                       zero(2), w1, zero(2), w2]
    # the table's size must be that of the count it was prepared with (sizes
    # are rounded to 256 bytes: 16 points need more than 8)
    with pytest.raises(AssertionError):
        T.sig_combine_prepared(tab, count + 8, _i32([0]), _i32([0]), _i32([0, 1]))


def test_g2_lincomb_scalar_cases(table):
    from hbbft_amd import threshold as T
    sc = GOLD["scalar_cases"]
    tab, count = _prepare([bytes.fromhex(sc["point"])])
    cases = sc["cases"]
    x2 = B.X_ABS ** 2
    assert [int(c["k"], 16) for c in cases] == [0, 1, 2, x2 - 1, x2, x2 + 1, B.R - 1, 1 << 254, B.R]
    n = len(cases)
    got = _rows(T.g2_lincomb_prepared(
        tab, count, _i32([0] * n), _bytes_t([bytes.fromhex(c["k"]) for c in cases], 32),
        _i32(range(n + 1))))
    assert got == [_want(c) for c in cases]
    assert got[0] == (INF192, INF96, 1, 1) and got[1][0] == sc["point"]
    assert got[8] == (ZERO192, ZERO96, 0, 2)
    # several terms with explicit scalars: the fixture's lambdas give its signature
    tab, count, first = table
    g = GROUPS["t2_of_7"]
    rows = list(range(first["t2_of_7"], first["t2_of_7"] + 3))
    got = _rows(T.g2_lincomb_prepared(
        tab, count, _i32(rows), _bytes_t([bytes.fromhex(l) for l in g["lambdas"]], 32),
        _i32([0, 3])))
    assert got == [_want("t2_of_7")]


def _epoch_shares():
    """[(document, node, share, pk, expected outcome 1 / 0 / 2)] of the epoch."""
    out = []
    for d, doc in enumerate(EPOCH["documents"]):
        for s in doc["shares"]:
            share, pk = bytes.fromhex(s["share"]), bytes.fromhex(s["pk"])
            invalid = share == OFF_G2 or pk == OFF_G1
            assert not (invalid and s["expect"])
            out.append((d, s["node"], share, pk, 2 if invalid else int(s["expect"])))
    return out


@pytest.fixture(scope="module")
def epoch_tables():
    """The epoch's hashes as prepared lines and its distinct keys as a key
    table: (prep, hashes, ktab, keys)."""
    from hbbft_amd import threshold as T
    hashes = [bytes.fromhex(d["hash"]) for d in EPOCH["documents"]]
    keys = []
    for _, _, _, pk, _ in _epoch_shares():
        if pk not in keys:
            keys.append(pk)
    return (T.g2_prepare(_bytes_t(hashes, 192)), hashes, T.g1_prepare(_bytes_t(keys, 96)), keys)


def test_share_check_agrees_with_pairing_check_batch(epoch_tables):
    """67 + 7 checks e(pk, H) == e(G1::one(), share) through the new kernel and
    through the existing two-Miller-loop entry, with the tampered, invalid and
    infinity inputs of the epoch mixed in."""
    from hbbft_amd import threshold as T
    prep, hashes, ktab, keys = epoch_tables
    ep = _epoch_shares()
    assert sorted(e[4] for e in ep) == [0] * 3 + [1] * 9 + [2] * 2
    assert ("40" + "00" * 191) in [e[2].hex() for e in ep]
    checks = [ep[i % len(ep)] for i in range(70)]
    # a share checked against the other document's hash, and against another
    # node's key: both fail
    a = next(e for e in ep if e[0] == 0 and e[4] == 1)
    b = next(e for e in ep if e[0] == 1 and e[4] == 1 and e[3] != a[3])
    checks += [(1, a[1], a[2], a[3], 0), (0, a[1], a[2], b[3], 0)]
    ik = [keys.index(c[3]) for c in checks]
    ih = [c[0] for c in checks]
    want = [c[4] for c in checks]
    # two checks with an index past its table: invalid, whatever the points
    checks += [a, a]
    ik += [len(keys), ik[checks.index(a)]]
    ih += [0, len(hashes)]
    want += [2, 2]
    assert len(checks) == 74
    stab, count = _prepare([c[2] for c in checks])
    got = T.sig_check_prepared(stab, count, ktab, len(keys), _i32(ik), prep, len(hashes),
                               _i32(ih)).cpu().tolist()
    assert got == want
    # the existing entry: a = pk, b = H, c = G1::one(), d = share; it has no
    # indices, so the two out-of-range checks carry an invalid key instead
    g1 = [x for c in checks[:72] for x in (c[3], T.G1_ONE)] + [OFF_G1, T.G1_ONE] * 2
    g2 = [x for c in checks for x in (hashes[c[0]], c[2])]
    ref = T.pairing_check_batch(_bytes_t(g1, 96), _bytes_t(g2, 192)).cpu().tolist()
    assert ref == got


def test_keys_and_documents_shared_across_lanes(epoch_tables):
    """80 checks sorted by document, 40 each: document 1's shares straddle the
    64-lane block, and every key serves shares of both documents."""
    from hbbft_amd import threshold as T
    prep, hashes, ktab, keys = epoch_tables
    ep = _epoch_shares()
    by_doc = [[e for e in ep if e[0] == d] for d in range(2)]
    checks = [by_doc[d][i % 7] for d in range(2) for i in range(40)]
    used = [{keys.index(c[3]) for c in checks if c[0] == d} for d in range(2)]
    assert len(used[0] & used[1]) >= 5
    stab, count = _prepare([c[2] for c in checks])
    got = T.sig_check_prepared(stab, count, ktab, len(keys),
                               _i32([keys.index(c[3]) for c in checks]), prep, len(hashes),
                               _i32([c[0] for c in checks])).cpu().tolist()
    assert got == [c[4] for c in checks]


def _doc_want(doc, verified=True):
    return (bytes.fromhex(doc["sig192"]), bytes.fromhex(doc["sig96"]), doc["parity"], verified)


def test_threshold_sign_grouped_epoch():
    from hbbft_amd import threshold as T
    t = EPOCH["t"]
    pk = bytes.fromhex(EPOCH["public_key"])
    docs = [bytes.fromhex(d["hash"]) for d in EPOCH["documents"]]
    ep = _epoch_shares()
    shares = [(d, node, share, key) for d, node, share, key, _ in ep]
    expect = [st == 1 for *_, st in ep]
    assert expect.count(False) == 5
    # interleave the two documents' shares: input order is not table order
    perm = sorted(range(len(shares)), key=lambda i: (i % 7, i // 7))
    shares, expect = ([x[i] for i in perm] for x in (shares, expect))
    flags, outs = T.threshold_sign_grouped(docs, shares, t, pk)
    assert flags == expect
    assert all(d["verified"] for d in EPOCH["documents"])
    assert outs == [_doc_want(d) for d in EPOCH["documents"]]
    assert flags == T.verify_signature_shares(
        [(s, key, docs[d]) for d, _, s, key in shares])
    # the combine takes the first t + 1 valid shares by node index: the result
    # is that of exactly those (document 0: nodes 0, 2, 3 -- 1 is tampered)
    by_node = {n: s for d, n, s, _ in shares if d == 0}
    assert T.combine_signature_shares([[(n, by_node[n]) for n in (0, 2, 3)]]) == [outs[0][:3]]
    assert T.combine_signature_shares([[(n, by_node[n]) for n in (0, 1, 2)]]) != [outs[0][:3]]
    # a node's valid share delivered twice counts once (counted twice, nodes
    # 0, 2, 2 would be a repeated index)
    dup = next(s for s, ok in zip(shares, expect) if s[0] == 0 and s[1] == 2 and ok)
    flags2, outs2 = T.threshold_sign_grouped(docs, shares + [dup], t, pk)
    assert flags2 == expect + [True] and outs2 == outs
    # document 1 left with t valid shares (and its failing ones): no output
    keep = [s for s in shares if s[0] == 0]
    valid1 = [s for s, ok in zip(shares, expect) if s[0] == 1 and ok][:t]
    bad1 = [s for s, ok in zip(shares, expect) if s[0] == 1 and not ok]
    flags3, outs3 = T.threshold_sign_grouped(docs, keep + valid1 + bad1, t, pk)
    assert flags3 == [e for s, e in zip(shares, expect) if s[0] == 0] + [True] * t + \
        [False] * len(bad1)
    assert outs3 == [outs[0], None]
    # a wrong public key: the same signatures, not verified
    flags4, outs4 = T.threshold_sign_grouped(docs, shares, t, bytes.fromhex(EPOCH["stranger_key"]))
    assert flags4 == expect
    assert outs4 == [_doc_want(d, False) for d in EPOCH["documents"]]


def _host_group(name):
    g = GROUPS[name]
    return [(i, bytes.fromhex(s)) for i, s in zip(g["idx"], g["shares"])]


def _host_want(name):
    g = GROUPS[name]
    return (bytes.fromhex(g["sig192"]), bytes.fromhex(g["sig96"]), g["parity"])


def test_host_bytes_entries():
    from hbbft_amd import RseError
    from hbbft_amd import threshold as T
    t1, t2 = _host_group("t1"), _host_group("t2_of_7")
    dup = [(t2[0][0], t2[0][1]), (t2[1][0], t2[1][1]), (t2[0][0], t2[2][1])]
    bad = [t2[0], (t2[1][0], OFF_G2), t2[2]]
    want1, want2 = _host_want("t1"), _host_want("t2_of_7")
    assert T.combine_signature_shares([t1, t2, dup, bad]) == [want1, want2, None, None]
    assert T.sig_combine(t1) == want1
    assert T.sig_combine(t2) == want2
    assert T.sig_combine(_host_group("f0_zero")) == _host_want("f0_zero")
    for grp in (dup, bad):
        with pytest.raises(RseError) as e:
            T.sig_combine(grp)
        assert e.value.code == 100    # HBRBC_E_INVALID_ARG
    ep = _epoch_shares()
    docs = [bytes.fromhex(d["hash"]) for d in EPOCH["documents"]]
    assert T.verify_signature_shares([(s, key, docs[d]) for d, _, s, key, _ in ep]) == \
        [st == 1 for *_, st in ep]
    assert T.verify_signature_shares([]) == []
