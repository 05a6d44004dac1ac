"""GPU parity of the compressed wire encodings against tests/golden/
compressed_vectors.json and the restatement in tests/compressed_ref.py:
g1_decompress / g2_decompress bit-exact on every case, at block boundaries with
valid and invalid lanes mixed in a wave; the tables of g1_prepare_compressed /
g2_points_prepare_compressed identical to those of the uncompressed entries;
the compressed outputs of the two combines decompressed back to their
uncompressed ones; and the two golden epochs in wire form."""
import json
import os

import numpy as np
import pytest

import compressed_ref as C
from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


GOLD = _gold("compressed_vectors.json")
COMBINE = _gold("combine_vectors.json")
SIGN = _gold("sign_vectors.json")

pytestmark = pytest.mark.gpu


def _bytes_t(rows, width):
    import torch
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)
    return torch.from_numpy(a.copy()).to("cuda:0")


def _i32(values):
    import torch
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")


def _cases(key):
    """(compressed rows, uncompressed rows, statuses) of one group."""
    cs = GOLD[key]
    return ([bytes.fromhex(c["c"]) for c in cs], [bytes.fromhex(c["u"]) for c in cs],
            [c["status"] for c in cs])


def _decompress(key, rows):
    from hbbft_amd import threshold as T
    fn, width = (T.g1_decompress, 48) if key == "g1" else (T.g2_decompress, 96)
    out, st = fn(_bytes_t(rows, width))
    out = out.cpu().numpy()
    return [bytes(out[i]) for i in range(len(rows))], st.cpu().tolist()


@pytest.mark.parametrize("key", ["g1", "g2"])
def test_decompress_matches_the_fixture(key):
    c, u, st = _cases(key)
    got_u, got_st = _decompress(key, c)
    assert got_st == st
    for name, g, w in zip((x["name"] for x in GOLD[key]), got_u, u):
        assert g == w, name


@pytest.mark.parametrize("key", ["g1", "g2"])
def test_decompress_across_block_boundaries(key):
    """1, 63, 64, 65 and 130 points: the fixture rows tiled from a different
    start each, so that valid, infinite and invalid lanes share waves and the
    last block is partly empty."""
    c, u, st = _cases(key)
    n = len(c)
    for k, count in enumerate((1, 63, 64, 65, 130)):
        pick = [(3 * k + i) % n for i in range(count)]
        got_u, got_st = _decompress(key, [c[i] for i in pick])
        assert got_st == [st[i] for i in pick], count
        assert got_u == [u[i] for i in pick], count
    assert len({st[(3 + i) % n] for i in range(63)}) == 3


def _twin_rows(key):
    """The fixture's compressed rows and, per row, an uncompressed encoding
    the uncompressed entry treats alike: the point itself, infinity, or --
    for an invalid row -- its stored zero bytes, except that the points
    outside the subgroup go in as themselves (on the curve, rejected by the
    order-r check on both sides)."""
    c, u, st = _cases(key)
    off = (B.g1_bytes(B.g1_curve_point(0x5EED)) if key == "g1"
           else B.g2_bytes(B.g2_curve_point(0x5EED)))
    names = [x["name"] for x in GOLD[key]]
    u = list(u)
    u[names.index(key + "_outside_subgroup")] = off
    return c, u, st


def _same_table(a, b, point_bytes, count, statuses):
    """Two tables of `count` points hold the same bytes: the coordinates
    (point_bytes per point) and, behind them at the next multiple of 256, the
    status bytes.  The padding after each part is written by neither entry."""
    import torch
    assert a.shape == b.shape
    off = (point_bytes * count + 255) // 256 * 256
    assert a.numel() == off + (count + 255) // 256 * 256
    assert torch.equal(a[:point_bytes * count], b[:point_bytes * count])
    assert torch.equal(a[off:off + count], b[off:off + count])
    assert a[off:off + count].cpu().tolist() == statuses
    # rows that are not valid and finite hold zeros
    rows = a[:point_bytes * count].reshape(count, point_bytes).cpu().numpy()
    for r, st in zip(rows, statuses):
        assert bool(r.any()) == (st == 0)


@pytest.mark.parametrize("count", [22, 65, 130])
def test_g1_table_is_that_of_the_uncompressed_entry(count):
    from hbbft_amd import threshold as T
    c, u, st = _twin_rows("g1")
    pick = [i % len(c) for i in range(count)]
    a = T.g1_prepare_compressed(_bytes_t([c[i] for i in pick], 48))
    b = T.g1_prepare(_bytes_t([u[i] for i in pick], 96))
    _same_table(a, b, 96, count, [st[i] for i in pick])


@pytest.mark.parametrize("count", [22, 65, 130])
def test_g2_table_is_that_of_the_uncompressed_entry(count):
    from hbbft_amd import threshold as T
    c, u, st = _twin_rows("g2")
    pick = [i % len(c) for i in range(count)]
    a = T.g2_points_prepare_compressed(_bytes_t([c[i] for i in pick], 96))
    b = T.g2_points_prepare(_bytes_t([u[i] for i in pick], 192))
    _same_table(a, b, 192, count, [st[i] for i in pick])


def test_round_trip_through_the_g1_encoder():
    """decrypt_combine_prepared writes both encodings of its results; the
    compressed ones decompress to the uncompressed ones (statuses 0 and 1)."""
    from hbbft_amd import threshold as T
    groups = [g for g in COMBINE["groups"] if g["status"] in (0, 1)]
    points = [bytes.fromhex(s) for g in groups for s in g["shares"]]
    offs = np.cumsum([0] + [len(g["shares"]) for g in groups])
    tab = T.g1_prepare(_bytes_t(points, 96))
    o96, o48, st = T.decrypt_combine_prepared(
        tab, len(points), _i32(range(len(points))), _i32([i for g in groups for i in g["idx"]]),
        _i32(offs))
    assert st.cpu().tolist() == [g["status"] for g in groups]
    assert {0, 1} == set(st.cpu().tolist())
    back, bst = T.g1_decompress(o48)
    import torch
    assert torch.equal(back, o96) and torch.equal(bst, st)
    assert [bytes(r).hex() for r in o48.cpu().numpy()] == [g["g48"] for g in groups]


def test_round_trip_through_the_g2_encoder():
    import torch
    from hbbft_amd import threshold as T
    groups = [g for g in SIGN["groups"] if g["status"] in (0, 1)]
    points = [bytes.fromhex(s) for g in groups for s in g["shares"]]
    offs = np.cumsum([0] + [len(g["shares"]) for g in groups])
    tab = T.g2_points_prepare(_bytes_t(points, 192))
    o192, o96, _, st = T.sig_combine_prepared(
        tab, len(points), _i32(range(len(points))), _i32([i for g in groups for i in g["idx"]]),
        _i32(offs))
    assert st.cpu().tolist() == [g["status"] for g in groups]
    assert {0, 1} == set(st.cpu().tolist())
    back, bst = T.g2_decompress(o96)
    assert torch.equal(back, o192) and torch.equal(bst, st)
    assert [bytes(r).hex() for r in o96.cpu().numpy()] == [g["sig96"] for g in groups]


def _c1(h):
    return C.compress_g1(C.parse_g1(bytes.fromhex(h)))


def _c2(h):
    return C.compress_g2(C.parse_g2(bytes.fromhex(h)))


def test_threshold_sign_epoch_in_wire_form():
    """threshold_sign_grouped_wire on the epoch of sign_vectors.json, every
    received point compressed (the share and the key outside their subgroups
    included): the flags and outputs of threshold_sign_grouped."""
    from hbbft_amd import threshold as T
    ep = SIGN["epoch"]
    docs = [bytes.fromhex(d["hash"]) for d in ep["documents"]]
    plain, wire, expect = [], [], []
    for d, doc in enumerate(ep["documents"]):
        for s in doc["shares"]:
            plain.append((d, s["node"], bytes.fromhex(s["share"]), bytes.fromhex(s["pk"])))
            wire.append((d, s["node"], _c2(s["share"]), _c1(s["pk"])))
            expect.append(s["expect"])
    off1, off2 = B.g1_bytes(B.g1_curve_point(0x5EED)), B.g2_bytes(B.g2_curve_point(0x5EED))
    assert off1 in [p[3] for p in plain] and off2 in [p[2] for p in plain]
    assert all(len(w[2]) == 96 and len(w[3]) == 48 for w in wire)
    perm = sorted(range(len(plain)), key=lambda i: (i % 7, i // 7))
    plain, wire, expect = ([x[i] for i in perm] for x in (plain, wire, expect))
    want = T.threshold_sign_grouped(docs, plain, ep["t"], bytes.fromhex(ep["public_key"]))
    got = T.threshold_sign_grouped_wire(docs, wire, ep["t"], _c1(ep["public_key"]))
    assert got == want
    assert got[0] == expect and expect.count(False) == 5
    assert got[1] == [(bytes.fromhex(d["sig192"]), bytes.fromhex(d["sig96"]), d["parity"], True)
                      for d in ep["documents"]]
    # a wrong public key: the same signatures, not verified
    got = T.threshold_sign_grouped_wire(docs, wire, ep["t"], _c1(ep["stranger_key"]))
    assert got == T.threshold_sign_grouped(docs, plain, ep["t"], bytes.fromhex(ep["stranger_key"]))
    assert [o[3] for o in got[1]] == [False, False]
    # the uncompressed public key is the caller's error, as a compressed one is to the twin
    with pytest.raises(ValueError):
        T.threshold_sign_grouped_wire(docs, wire, ep["t"], bytes.fromhex(ep["public_key"]))
    with pytest.raises(ValueError):
        T.threshold_sign_grouped(docs, plain, ep["t"], _c1(ep["public_key"]))


def test_decrypt_epoch_in_wire_form():
    """decrypt_shares_grouped_wire on the epoch of combine_vectors.json: W,
    the shares and the key shares compressed, H a point."""
    from hbbft_amd import threshold as T
    ep = COMBINE["epoch"]
    cts = [(bytes.fromhex(c["hash"]), bytes.fromhex(c["w"])) for c in ep["ciphertexts"]]
    cts_w = [(bytes.fromhex(c["hash"]), _c2(c["w"])) for c in ep["ciphertexts"]]
    plain, wire, expect = [], [], []
    for ci, c in enumerate(ep["ciphertexts"]):
        for s in c["shares"]:
            plain.append((ci, s["node"], bytes.fromhex(s["share"]), bytes.fromhex(s["pk"])))
            wire.append((ci, s["node"], _c1(s["share"]), _c1(s["pk"])))
            expect.append(s["expect"])
    perm = sorted(range(len(plain)), key=lambda i: (i % 7, i // 7))
    plain, wire, expect = ([x[i] for i in perm] for x in (plain, wire, expect))
    want = T.decrypt_shares_grouped(cts, plain, ep["t"])
    got = T.decrypt_shares_grouped_wire(cts_w, wire, ep["t"])
    assert got == want
    assert got[0] == expect and expect.count(False) == 3
    assert got[1] == [(bytes.fromhex(c["g96"]), bytes.fromhex(c["g48"]))
                      for c in ep["ciphertexts"]]
    # a W that does not decode (its compression flag cleared) fails every
    # share of its ciphertext and leaves the other alone
    bad_w = bytes([cts_w[1][1][0] & 0x7F]) + cts_w[1][1][1:]
    flags, outs = T.decrypt_shares_grouped_wire([cts_w[0], (cts_w[1][0], bad_w)], wire, ep["t"])
    assert flags == [e and s[0] == 0 for s, e in zip(wire, expect)]
    assert outs == [want[1][0], None]
    with pytest.raises(ValueError):
        T.decrypt_shares_grouped_wire(cts, wire, ep["t"])
