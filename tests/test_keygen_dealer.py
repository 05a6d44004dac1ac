"""GPU parity of SyncKeyGen's sending side: hbrbc_fr_poly_eval and hbrbc_fr_dot
against tests/golden/dealer_vectors.json (Python integers), the rows, values
and commitments of keygen_vectors.json's transcripts produced from their
polynomials, every node's secret key share (the N = 7 transcript leaves out the
part with only 2t Acks and counts its repeated sender once), the whole network
run against the fixture, and the pipeline end to end at N = 4: key generation,
share creation, the share checks, the combines."""
import json
import os

import numpy as np
import pytest

from hbbft_amd import keygen as K
from hbbft_amd import threshold as T
from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


KEYGEN, DEALER = _gold("keygen_vectors.json"), _gold("dealer_vectors.json")
COMPRESSED = _gold("compressed_vectors.json")
R = B.R

pytestmark = pytest.mark.gpu


def _i32(values):
    import torch
    a = np.asarray(values, dtype=np.int64).reshape(-1).astype(np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to("cuda:0")


def _bytes_t(rows, width):
    import torch
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)
    return torch.from_numpy(a.copy()).to("cuda:0")


def _fr(v):
    return int(v).to_bytes(32, "big")


def _offsets(lengths):
    return _i32(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))


def _hex_rows(t):
    return [bytes(v).hex() for v in t.cpu().numpy()]


def test_fr_poly_eval_fixture_cases_in_one_launch():
    """Degrees 0, 1 and 21 at 0, 1, 2, 64 and 2^32 - 1, the empty polynomial, a
    coefficient equal to r, rows and poly indices out of range: 42 lanes that
    mix degrees and failures inside one wave."""
    pe = DEALER["poly_eval"]
    table = _bytes_t([bytes.fromhex(v) for v in pe["table"]], 32)
    rows = [r for p in pe["polys"] for r in p["rows"]]
    offs = _offsets([len(p["rows"]) for p in pe["polys"]])
    ev = pe["evals"]
    assert {e["x"] for e in ev} >= {0, 1, 2, 64, 0xFFFFFFFF} and {e["status"] for e in ev} == {0, 2}
    out, st = K.fr_poly_eval(table, _i32(rows), offs, _i32([e["poly"] for e in ev]),
                             _i32([e["x"] for e in ev]))
    assert st.cpu().tolist() == [e["status"] for e in ev]
    assert _hex_rows(out) == [e["value"] for e in ev]


@pytest.mark.parametrize("lanes", [1, 63, 64, 65, 130])
def test_fr_poly_eval_lane_counts(lanes):
    pe = DEALER["poly_eval"]
    table = _bytes_t([bytes.fromhex(v) for v in pe["table"]], 32)
    rows = [r for p in pe["polys"] for r in p["rows"]]
    offs = _offsets([len(p["rows"]) for p in pe["polys"]])
    ev = [pe["evals"][(5 * j + 2) % len(pe["evals"])] for j in range(lanes)]
    out, st = K.fr_poly_eval(table, _i32(rows), offs, _i32([e["poly"] for e in ev]),
                             _i32([e["x"] for e in ev]))
    assert st.cpu().tolist() == [e["status"] for e in ev]
    assert _hex_rows(out) == [e["value"] for e in ev]


def test_fr_dot_fixture_groups():
    """Groups of 0, 1, 22 and 65 terms, one with an operand equal to r, the
    edge values 0 and r - 1; and the same groups behind a second block."""
    groups = DEALER["dot"]
    assert [len(g["a"]) for g in groups][:4] == [0, 1, 22, 65]
    for reps in (1, 12):   # 6 and 72 groups: one lane per group
        gs = groups * reps
        a = [bytes.fromhex(v) for g in gs for v in g["a"]]
        b = [bytes.fromhex(v) for g in gs for v in g["b"]]
        out, st = K.fr_dot(_bytes_t(a, 32), _bytes_t(b, 32), _offsets([len(g["a"]) for g in gs]))
        assert st.cpu().tolist() == [g["status"] for g in gs]
        assert _hex_rows(out) == [g["value"] for g in gs]


@pytest.mark.parametrize("k", [0, 1])
def test_generate_part_and_ack_values_give_the_transcript(k):
    tr = KEYGEN["transcripts"][k]
    n, t = tr["n"], tr["t"]
    for p in (0, n - 1):
        commit, rows = K.generate_part(t, [bytes.fromhex(c) for c in tr["polys"][p]], n)
        assert [c.hex() for c in commit] == tr["commitments"][p]
        assert [[c.hex() for c in row] for row in rows] == tr["rows"][p]
        for s in (0, n - 1):   # sender s's Ack of part p: values[p][s][node]
            vals = K.ack_values(rows[s], n)
            assert [v.hex() for v in vals] == tr["values"][p][s]


@pytest.mark.parametrize("k", [0, 1])
def test_secret_key_shares_of_the_transcripts(k):
    """The pairs arrive unsorted and with the repeated sender; part 6 of the
    N = 7 transcript (2t Acks) is not among the complete parts."""
    tr, want = KEYGEN["transcripts"][k], DEALER["transcripts"][k]
    n = tr["n"]
    assert want["complete"] == tr["complete"]
    if k == 1:
        assert 6 not in tr["complete"] and tr["ack_senders"][5].count(3) == 2
    for node in range(n):
        parts = [[(s, bytes.fromhex(tr["values"][p][s][node]))
                  for s in reversed(tr["ack_senders"][p])] for p in tr["complete"]]
        assert K.secret_key_share(tr["t"], parts).hex() == want["secret_key_shares"][node]
    # with fewer than t + 1 pairs the crate interpolates what there is: one
    # pair gives the value itself; no part gives zero
    v = bytes.fromhex(tr["values"][0][2][1])
    assert K.secret_key_share(tr["t"], [[(2, v)]]) == v
    assert K.secret_key_share(tr["t"], []) == b"\0" * 32


@pytest.fixture(scope="module")
def networks():
    out = []
    for tr in KEYGEN["transcripts"]:
        polys = [[bytes.fromhex(c) for c in f] for f in tr["polys"]]
        out.append(K.sync_key_gen_network(tr["t"], polys, ack_senders=tr["ack_senders"]))
    return out


@pytest.mark.parametrize("k", [0, 1])
def test_network_run_equals_the_transcript(networks, k):
    tr, want, net = KEYGEN["transcripts"][k], DEALER["transcripts"][k], networks[k]
    n = tr["n"]
    assert [[c.hex() for c in cm] for cm in net["commitments"]] == tr["commitments"]
    assert [[[c.hex() for c in row] for row in part] for part in net["rows"]] == tr["rows"]
    assert [[[v.hex() for v in vs] for vs in part] for part in net["values"]] == tr["values"]
    assert net["part_ok"] == [[True] * n] * n
    acks = sum(len(a) for a in tr["ack_senders"])
    assert net["ack_ok"] == [[True] * acks] * n
    assert net["complete"] == tr["complete"]
    assert [(a.hex(), b.hex()) for a, b in net["key_set"]] == \
        [(c["g96"], c["g48"]) for c in tr["key_set"]]
    stab, s96, s48, sst, pk = net["key_shares"]
    assert sst.cpu().tolist() == [0] * n
    assert _hex_rows(s96) == [c["g96"] for c in tr["key_shares"]]
    assert _hex_rows(s48) == [c["g48"] for c in tr["key_shares"]]
    assert pk[0].hex() == tr["key_set"][0]["g96"]
    assert [s.hex() for s in net["secret_key_shares"]] == want["secret_key_shares"]
    # [sk_i] G1::one() is pk_i, by the existing check on the pk_i table
    ok = K.base_mul_check(stab, n, _i32(list(range(n))), _bytes_t(net["secret_key_shares"], 32))
    assert ok.cpu().tolist() == [1] * n


def test_default_network_run_has_every_part_complete(networks):
    tr = KEYGEN["transcripts"][0]
    polys = [[bytes.fromhex(c) for c in f] for f in tr["polys"]]
    net = K.sync_key_gen_network(tr["t"], polys)
    assert net["complete"] == [0, 1, 2, 3]
    assert net["secret_key_shares"] == networks[0]["secret_key_shares"]


def test_end_to_end_keygen_shares_checks_combines(networks):
    """N = 4, t = 1, two ciphertexts and two documents: every created share
    passes the prepared checks, a share made with another node's scalar fails
    alone, and any t + 1 shares combine to [f(0) u] G1::one() and to a
    signature the master public key verifies."""
    import torch
    tr, net = KEYGEN["transcripts"][0], networks[0]
    n, t, C = 4, 1, 2
    sks = net["secret_key_shares"]
    pk_tab = net["key_shares"][0]
    master = sum(int(tr["polys"][p][0], 16) for p in tr["complete"]) % R
    us = [0x1234567 + (1 << 200), R - 77]     # a ciphertext's r: U = [u] G1::one()
    hs = [0xABCDEF + (1 << 131), 5]           # H = [h] G2::one() stands for the hashes
    gen = next(x for x in COMPRESSED["g2"] if x["name"] == "g2_valid_0")
    gtab = T.g2_points_prepare(_bytes_t([bytes.fromhex(gen["u"])], 192))
    htab, h192, _, hst = T.g2_mul_prepared(gtab, 1, _i32([0, 0]), _bytes_t([_fr(h) for h in hs], 32))
    _, w192, _, wst = T.g2_mul_prepared(htab, 2, _i32([0, 1]), _bytes_t([_fr(u) for u in us], 32))
    _, _, u48, ust = K.base_mul(_bytes_t([_fr(u) for u in us], 32))
    assert hst.cpu().tolist() == wst.cpu().tolist() == ust.cpu().tolist() == [0, 0]
    hashes = [bytes(v) for v in h192.cpu().numpy()]
    us48 = [bytes(v) for v in u48.cpu().numpy()]
    nodes = [i for i in range(n) for _ in range(C)]
    items = [c for _ in range(n) for c in range(C)]
    assert [T.share_row(i, c, C) for i, c in zip(nodes, items)] == list(range(n * C))

    # decryption shares: e(share, H) == e(pk_i, W), prepared points H_0, W_0, H_1, W_1
    dtab, count, d96, d48, dst = T.create_decryption_shares(sks, us48)
    assert count == n * C and dst.cpu().tolist() == [0] * count
    prep = T.g2_prepare(torch.stack([h192, w192], dim=1).reshape(2 * C, 192).contiguous())
    ib = _i32([2 * c for c in items])
    id_ = _i32([2 * c + 1 for c in items])
    ok = T.pairing_check_prepared_pts(dtab, count, pk_tab, n, _i32(nodes), prep, 2 * C, ib, id_)
    assert ok.cpu().tolist() == [1] * count
    utab = T.g1_prepare_compressed(u48)
    sidx = list(nodes)
    sidx[T.share_row(1, 0, C)] = 2            # node 1 signs ciphertext 0 with sk_2
    bad_tab, _, _, bst = T.g1_mul_prepared(utab, C, _i32(items), _bytes_t(sks, 32), _i32(sidx))
    assert bst.cpu().tolist() == [0] * count
    ok = T.pairing_check_prepared_pts(bad_tab, count, pk_tab, n, _i32(nodes), prep, 2 * C, ib, id_)
    assert ok.cpu().tolist() == [int(j != T.share_row(1, 0, C)) for j in range(count)]
    for pair in ((0, 1), (1, 3), (2, 3)):     # any t + 1 = 2 nodes, per ciphertext
        rows = [T.share_row(i, c, C) for c in range(C) for i in pair]
        g96, _, gst = T.decrypt_combine_prepared(dtab, count, _i32(rows), _i32(list(pair) * C),
                                                 _offsets([t + 1] * C))
        assert gst.cpu().tolist() == [0] * C
        eq = K.base_mul_check(T.g1_prepare(g96), C, _i32(list(range(C))),
                              _bytes_t([_fr(master * u % R) for u in us], 32))
        assert eq.cpu().tolist() == [1] * C, pair

    # signature shares: e(pk_i, H_d) == e(G1::one(), share)
    stab, count, s192, s96, sst = T.create_signature_shares(sks, hashes)
    assert count == n * C and sst.cpu().tolist() == [0] * count
    hprep = T.g2_prepare(h192)
    ok = T.sig_check_prepared(stab, count, pk_tab, n, _i32(nodes), hprep, C, _i32(items))
    assert ok.cpu().tolist() == [1] * count
    bad_tab, _, _, _ = T.g2_mul_prepared(htab, C, _i32(items), _bytes_t(sks, 32), _i32(sidx))
    ok = T.sig_check_prepared(bad_tab, count, pk_tab, n, _i32(nodes), hprep, C, _i32(items))
    assert ok.cpu().tolist() == [int(j != T.share_row(1, 0, C)) for j in range(count)]
    master_tab = T.g1_prepare(_bytes_t([net["key_set"][0][0]], 96))
    sigs = set()
    for pair in ((0, 1), (1, 3), (2, 3)):
        rows = [T.share_row(i, c, C) for c in range(C) for i in pair]
        g192, _, _, gst = T.sig_combine_prepared(stab, count, _i32(rows), _i32(list(pair) * C),
                                                 _offsets([t + 1] * C))
        assert gst.cpu().tolist() == [0] * C
        ver = T.sig_check_prepared(T.g2_points_prepare(g192), C, master_tab, 1, _i32([0] * C),
                                   hprep, C, _i32(list(range(C))))
        assert ver.cpu().tolist() == [1] * C, pair
        sigs.add(g192.cpu().numpy().tobytes())
    assert len(sigs) == 1                     # the signature does not depend on the signers
