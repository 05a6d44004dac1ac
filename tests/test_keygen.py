"""GPU parity of the key generation path (SyncKeyGen, sync_key_gen.rs:516-608)
against tests/golden/keygen_vectors.json (oracle/bls_oracle.py, Python
integers): every univariate evaluation with table bytes, status and both
encodings exact, alone and in launches that mix degrees and bit lengths inside
a wave and across block boundaries; invalid lanes isolated; the Horner kernel
against the independent linear combination with scalars x^k mod r; the
fixed-base check at the edge scalars; the key shares of the combine fixture's
epoch, bit for bit the table g1_prepare gives, and usable by the share checks;
both transcripts through the Part and Ack checks, the key set and the grouped
call, for every node; the tampered messages rejected with the right value."""
import json
import os
import random

import numpy as np
import pytest

from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


GOLD = _gold("keygen_vectors.json")
UNI = GOLD["univariate"]
R = B.R

pytestmark = pytest.mark.gpu


def _i32(values):
    """32-bit values, signed or unsigned, as the int32 device tensor the
    wrappers take."""
    import torch
    a = np.asarray(values, dtype=np.int64).reshape(-1).astype(np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to("cuda:0")


def _bytes_t(rows, width):
    import torch
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)
    return torch.from_numpy(a.copy()).to("cuda:0")


def _offsets(lengths):
    return _i32(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))


@pytest.fixture(scope="module")
def uni_table():
    from hbbft_amd import threshold as T
    pts = [bytes.fromhex(p) for p in UNI["table"]]
    return T.g1_prepare_compressed(_bytes_t(pts, 48)), len(pts)


def _eval(tab, count, polys, evals):
    """polys = [rows], evals = [(poly, x)] -> (the 96 table bytes of each
    evaluation, [(g96 hex, g48 hex, status)])."""
    from hbbft_amd import keygen as K
    rows = [r for p in polys for r in p]
    out, o96, o48, st = K.poly_eval_prepared(
        tab, count, _i32(rows), _offsets([len(p) for p in polys]), _i32([p for p, _ in evals]),
        _i32([x for _, x in evals]))
    n = len(evals)
    raw = out.cpu().numpy()
    stat_at = (n * 96 + 255) // 256 * 256
    a, b, s = o96.cpu().numpy(), o48.cpu().numpy(), st.cpu().tolist()
    assert raw[stat_at:stat_at + n].tolist() == s   # the table carries the statuses
    return ([bytes(raw[96 * e:96 * e + 96]) for e in range(n)],
            [(bytes(a[e]).hex(), bytes(b[e]).hex(), s[e]) for e in range(n)])


def _expected_entries(cases):
    """Table entries g1_prepare gives for the expected points (the existing,
    independent decoder): Montgomery x || y, zero for infinity and invalid."""
    from hbbft_amd import threshold as T
    tab = T.g1_prepare(_bytes_t([bytes.fromhex(c["g96"]) for c in cases], 96)).cpu().numpy()
    return [bytes(tab[96 * e:96 * e + 96]) for e in range(len(cases))]


def _same_table(tab, ref, n):
    """Two g1_prepare tables of n points agree bit for bit: the coordinates
    and the status bytes (the padding between and behind them is never
    written)."""
    assert tab.shape == ref.shape
    a, b = tab.cpu().numpy(), ref.cpu().numpy()
    stat_at = (n * 96 + 255) // 256 * 256
    assert np.array_equal(a[:n * 96], b[:n * 96])
    assert np.array_equal(a[stat_at:stat_at + n], b[stat_at:stat_at + n])


@pytest.fixture(scope="module")
def uni_entries():
    return _expected_entries(UNI["cases"])


def test_every_univariate_case_alone(uni_table, uni_entries):
    tab, count = uni_table
    for c, want in zip(UNI["cases"], uni_entries):
        entries, res = _eval(tab, count, [c["rows"]], [(0, c["x"])])
        assert res == [(c["g96"], c["g48"], c["status"])], c["name"]
        assert entries == [want], c["name"]


@pytest.mark.parametrize("evals", [1, 63, 64, 65, 130])
def test_mixed_launches(uni_table, uni_entries, evals):
    """Degrees 0, 1, 2 and 21, x of 0, 1, 7 and 32 bits and invalid lanes side
    by side in one launch; 65 and 130 cross block boundaries."""
    tab, count = uni_table
    cases = UNI["cases"]
    polys, slot = [], {}
    for c in cases:
        if tuple(c["rows"]) not in slot:
            slot[tuple(c["rows"])] = len(polys)
            polys.append(c["rows"])
    # a stride coprime to the case count walks all cases in a scrambled order
    assert len(cases) % 7 and len(cases) < 63
    order = [(5 + 7 * e) % len(cases) for e in range(evals)]
    entries, res = _eval(tab, count, polys,
                         [(slot[tuple(cases[k]["rows"])], cases[k]["x"]) for k in order])
    for e, k in enumerate(order):
        c = cases[k]
        assert res[e] == (c["g96"], c["g48"], c["status"]), (e, c["name"])
        assert entries[e] == uni_entries[k], (e, c["name"])
    if evals >= 63:
        names = {cases[k]["name"] for k in order}
        assert {"degree0_at_0", "degree1_at_1", "degree2_at_77", "degree21_at_4294967295",
                "degree21_at_65", "invalid_coefficient_at_2"} <= names


def test_out_of_range_rows_and_polys(uni_table, uni_entries):
    tab, count = uni_table
    by = {c["name"]: k for k, c in enumerate(UNI["cases"])}
    good = UNI["cases"][by["degree2_at_77"]]
    polys = [good["rows"], [3, count, 5], [3, -1], good["rows"], [0x7FFFFFFF]]
    evals = [(0, 77), (1, 77), (3, 77), (2, 1), (5, 77), (0, 77), (-1, 77), (3, 77), (4, 0),
             (0x7FFFFFFF, 2), (0, 77)]
    entries, res = _eval(tab, count, polys, evals)
    ok = (good["g96"], good["g48"], 0)
    bad = ("00" * 96, "00" * 48, 2)
    assert res == [ok, bad, ok, bad, bad, ok, bad, ok, bad, bad, ok]
    for e, r in enumerate(res):
        assert entries[e] == (uni_entries[by["degree2_at_77"]] if r == ok else b"\0" * 96)


def test_horner_against_the_linear_combination(uni_table):
    """Seeded random polynomials of degree 0..5 over the table: the same values
    through g1_lincomb_prepared with scalars x^k mod r."""
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    tab, count = uni_table
    rng = random.Random(0x484F524E)
    valid = [r for r in range(count) if r != 23]   # row 23 is outside G1
    polys, evals = [], []
    for p in range(24):
        polys.append([rng.choice(valid) for _ in range(p % 6 + 1)])
        for x in (rng.choice([0, 1, 2, 3]), rng.randrange(4, 200), rng.randrange(1 << 31, 1 << 32)):
            evals.append((p, x))
    rows = [r for p in polys for r in p]
    _, o96, o48, st = K.poly_eval_prepared(tab, count, _i32(rows),
                                           _offsets([len(p) for p in polys]),
                                           _i32([p for p, _ in evals]),
                                           _i32([x for _, x in evals]))
    lrows = [r for p, _ in evals for r in polys[p]]
    scal = [(pow(x, k, R)).to_bytes(32, "big") for p, x in evals for k in range(len(polys[p]))]
    w96, w48, wst = T.g1_lincomb_prepared(tab, count, _i32(lrows), _bytes_t(scal, 32),
                                          _offsets([len(polys[p]) for p, _ in evals]))
    assert st.cpu().tolist() == wst.cpu().tolist()
    assert set(wst.cpu().tolist()) <= {0, 1}
    assert np.array_equal(o96.cpu().numpy(), w96.cpu().numpy())
    assert np.array_equal(o48.cpu().numpy(), w48.cpu().numpy())


def test_base_mul_check_edge_scalars():
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    ks = [0, 1, 2, R - 1, 1 << 254]
    # [k] G1: 0 is infinity, R - 1 the negative of the generator; 2 and 2^254 by the oracle
    pts = [None, B.G1_GEN, B.g1_mul(B.G1_GEN, 2), B.g1_neg(B.G1_GEN), B.g1_mul(B.G1_GEN, 1 << 254)]
    off = B.g1_curve_point(0x5EED)
    tab = T.g1_prepare(_bytes_t([B.g1_bytes(p) for p in pts + [off]], 96))
    rows, scal, want = [], [], []
    for i, k in enumerate(ks):
        for j in range(len(pts)):   # the matching point and every other
            rows.append(j)
            scal.append(k.to_bytes(32, "big"))
            want.append(1 if i == j else 0)
    for k, row, exp in ((R, 1, 2), (R + 1, 1, 2), ((1 << 256) - 1, 0, 2), (1, 5, 2), (1, 6, 2),
                        (1, -1, 2), (1, 1, 1)):
        rows.append(row)
        scal.append(k.to_bytes(32, "big"))
        want.append(exp)
    ok = K.base_mul_check(tab, len(pts) + 1, _i32(rows), _bytes_t(scal, 32))
    assert ok.cpu().tolist() == want


def test_base_mul_check_random_scalars_across_blocks():
    """150 checks over three blocks: seeded scalars against points the
    existing linear combination made from the generator."""
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    rng = random.Random(0x42415345)
    n = 75
    ks = [rng.randrange(1, R) for _ in range(n)]
    gen = T.g1_prepare(_bytes_t([B.g1_bytes(B.G1_GEN)], 96))
    o96, _, st = T.g1_lincomb_prepared(gen, 1, _i32([0] * n),
                                       _bytes_t([k.to_bytes(32, "big") for k in ks], 32),
                                       _offsets([1] * n))
    assert st.cpu().tolist() == [0] * n
    tab = T.g1_prepare(o96)
    scal = [k.to_bytes(32, "big") for k in ks] + [((k + 1) % R).to_bytes(32, "big") for k in ks]
    ok = K.base_mul_check(tab, n, _i32(list(range(n)) * 2), _bytes_t(scal, 32))
    assert ok.cpu().tolist() == [1] * n + [0] * n


def test_public_key_shares_of_the_combine_epoch():
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    epoch = _gold("combine_vectors.json")["epoch"]
    n = epoch["n"]
    pks = {}
    for ct in epoch["ciphertexts"]:
        for s in ct["shares"]:
            if s["expect"]:
                pks[s["node"]] = bytes.fromhex(s["pk"])
    want = [pks[i] for i in range(n)]
    tab, o96, o48, st, pk = K.public_key_shares(
        [bytes.fromhex(c) for c in GOLD["epoch_commitment"]], n)
    ref = T.g1_prepare(_bytes_t(want, 96))
    _same_table(tab, ref, n)
    assert st.cpu().tolist() == [0] * n
    assert [bytes(r) for r in o96.cpu().numpy()] == want
    f0 = B.g1_mul(B.G1_GEN, int(epoch["poly"][0], 16))
    assert pk[0] == B.g1_bytes(f0)
    assert bytes.fromhex(GOLD["epoch_commitment"][0]) == pk[1]
    assert T.g1_decompress(o48)[0].cpu().numpy().tolist() == o96.cpu().numpy().tolist()
    # the derived table in the share checks: the epoch's flags, with the keys
    # the fixture marks as foreign or invalid failing as before
    ct = epoch["ciphertexts"]
    prep = T.g2_prepare(_bytes_t([bytes.fromhex(c[k]) for c in ct for k in ("hash", "w")], 192))
    shares, ic, ib, expect = [], [], [], []
    for c, item in enumerate(ct):
        for s in item["shares"]:
            shares.append(bytes.fromhex(s["share"]))
            ic.append(s["node"])
            ib.append(2 * c)
            # a share checked against the validator's true key: only tampering fails
            expect.append(bytes.fromhex(s["pk"]) != want[s["node"]] or s["expect"])
    ok = T.pairing_check_prepared_keys(_bytes_t(shares, 96), tab, n, _i32(ic), prep, 2 * len(ct),
                                       _i32(ib), _i32([b + 1 for b in ib]))
    got = [v == T.CHECK_OK for v in ok.cpu().tolist()]
    assert got == expect and not all(got)
    # the epoch's flags as stored: the derived keys for the validators, and the
    # two keys of no validator the fixture names spliced in behind them
    import torch
    foreign = sorted({bytes.fromhex(s["pk"]) for item in ct for s in item["shares"]} - set(want))
    assert len(foreign) == 2
    ftab = T.g1_prepare(_bytes_t(foreign, 96))
    total = n + len(foreign)

    def stat_at(count):
        return (count * 96 + 255) // 256 * 256

    ktab = torch.zeros_like(T.g1_prepare(_bytes_t(want + foreign, 96)))
    ktab[:n * 96] = tab[:n * 96]
    ktab[n * 96:total * 96] = ftab[:len(foreign) * 96]
    ktab[stat_at(total):stat_at(total) + n] = tab[stat_at(n):stat_at(n) + n]
    ktab[stat_at(total) + n:stat_at(total) + total] = ftab[stat_at(2):stat_at(2) + 2]
    pos = [s["node"] if bytes.fromhex(s["pk"]) == want[s["node"]]
           else n + foreign.index(bytes.fromhex(s["pk"])) for item in ct for s in item["shares"]]
    ok = T.pairing_check_prepared_keys(_bytes_t(shares, 96), ktab, total, _i32(pos), prep,
                                       2 * len(ct), _i32(ib), _i32([b + 1 for b in ib]))
    stored = [s["expect"] for item in ct for s in item["shares"]]
    assert [v == T.CHECK_OK for v in ok.cpu().tolist()] == stored


def _parts(tr, node):
    return [([bytes.fromhex(c) for c in tr["commitments"][p]],
             [bytes.fromhex(c) for c in tr["rows"][p][node]]) for p in range(tr["n"])]


def _acks(tr, node):
    return [(p, s, bytes.fromhex(tr["values"][p][s][node]))
            for p in range(tr["n"]) for s in tr["ack_senders"][p]]


def _pairs(items):
    return [(bytes.fromhex(c["g96"]), bytes.fromhex(c["g48"])) for c in items]


@pytest.mark.parametrize("k", [0, 1])
def test_transcripts_for_every_node(k):
    from hbbft_amd import keygen as K
    tr = GOLD["transcripts"][k]
    n, t = tr["n"], tr["t"]
    key_set, shares = _pairs(tr["key_set"]), _pairs(tr["key_shares"])
    complete = [tr["commitments"][p] for p in tr["complete"]]
    assert K.generate_public(t, [[bytes.fromhex(c) for c in cm] for cm in complete]) == key_set
    for node in range(n):
        parts, acks = _parts(tr, node), _acks(tr, node)
        part_ok, row_tables = K.check_parts(t, node, parts)
        assert part_ok == [True] * n, node
        assert K.check_acks(t, row_tables, acks) == [True] * len(acks), node
        g_parts, g_acks, g_complete, g_set, g_shares = K.sync_key_gen_grouped(t, node, parts, acks)
        assert g_parts == part_ok and g_acks == [True] * len(acks)
        assert g_complete == tr["complete"] and g_set == key_set
        stab, s96, s48, sst, pk = g_shares
        assert pk == key_set[0] and sst.cpu().tolist() == [0] * n
        got = zip(s96.cpu().numpy(), s48.cpu().numpy())
        assert [(bytes(a), bytes(b)) for a, b in got] == shares
    # a row and values meant for another node do not pass as ours
    part_ok, row_tables = K.check_parts(t, 0, _parts(tr, 1))
    assert part_ok == [False] * n
    assert K.check_acks(t, row_tables, _acks(tr, 1)[:n]) == [False] * n


def test_key_share_table_of_a_transcript_matches_g1_prepare():
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    tr = GOLD["transcripts"][1]
    shares = K.public_key_shares([bytes.fromhex(c["g48"]) for c in tr["key_set"]], tr["n"])
    ref = T.g1_prepare(_bytes_t([bytes.fromhex(c["g96"]) for c in tr["key_shares"]], 96))
    _same_table(shares[0], ref, tr["n"])
    assert shares[4] == _pairs(tr["key_set"])[0]


@pytest.mark.parametrize("case", GOLD["tamper"], ids=lambda c: c["name"])
def test_tampered_messages(case):
    from hbbft_amd import keygen as K
    tr = GOLD["transcripts"][case["transcript"]]
    n, t, node, p = tr["n"], tr["t"], case["our_idx"], case["part"]
    parts, acks = _parts(tr, node), _acks(tr, node)
    raw = bytes.fromhex(case["bytes"])
    want_parts, want_acks = [True] * n, [True] * len(acks)
    if case["field"] == "row":
        parts[p][1][case["index"]] = raw
        want_parts[p] = case["expect"]
    elif case["field"] == "commit":
        parts[p][0][case["index"]] = raw
        want_parts[p] = case["expect"]
        # no value can be checked against a commitment that does not decode
        want_acks = [case["expect"] if a[0] == p else True for a in acks]
    else:
        hit = [i for i, a in enumerate(acks) if a[0] == p and a[1] == case["index"]]
        assert len(hit) == 1
        acks[hit[0]] = (p, case["index"], raw)
        want_acks[hit[0]] = case["expect"]
    part_ok, row_tables = K.check_parts(t, node, parts)
    assert part_ok == want_parts
    assert K.check_acks(t, row_tables, acks) == want_acks
    g = K.sync_key_gen_grouped(t, node, parts, acks)
    assert g[0] == want_parts and g[1] == want_acks and g[2] == tr["complete"]
    key_set = _pairs(tr["key_set"])
    if case["field"] == "commit":
        # entry (0, 1) of the part is gone: coefficient 1 of the key set with it
        assert case["index"] == K.coeff_pos(0, 1)
        assert g[3] == [key_set[0], None]
    else:
        assert g[3] == key_set
