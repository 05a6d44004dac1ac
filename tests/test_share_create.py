"""GPU parity of share creation (`decrypt_share_no_verify`, `sign_g2`, the
fixed-base multiplication with a result) against the existing fixtures: the
edge scalars of combine_vectors.json / sign_vectors.json with encodings, status
and table bytes exact (the table must be what g1_prepare / g2_points_prepare
make of the expected bytes); the same cases with a table entry at infinity, an
invalid entry, rows and scalar indices out of range, in launches of 1, 63, 64,
65 and 130 lanes with one scalar per launch, scalars mixed inside a wave and
no index array; every fixture group created from its polynomial and combined
from the created table; base_mul against the commitments of
keygen_vectors.json, the edge scalars and its own check.  Expectations come
from fixture bytes and the library's independent decoders, never from the
kernels under test; the Python oracle multiplies once (2^254 G1::one())."""
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


COMB, SIGN, KEYGEN = (_gold(n) for n in ("combine_vectors.json", "sign_vectors.json",
                                          "keygen_vectors.json"))
COMPRESSED = _gold("compressed_vectors.json")
R = B.R
LANES = (1, 63, 64, 65, 130)

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


class Group:
    """The two groups behind one set of names: the fixture's scalar cases as
    (k, status, uncompressed, compressed) and a three-entry table -- the case
    point, infinity, an on-curve point outside the order-r subgroup."""

    def __init__(self, g2):
        self.g2 = g2
        self.width = 192 if g2 else 96
        sc = (SIGN if g2 else COMB)["scalar_cases"]
        u, c = ("sig192", "sig96") if g2 else ("g96", "g48")
        self.cases = [(bytes.fromhex(x["k"]), x["status"], bytes.fromhex(x[u]),
                       bytes.fromhex(x[c])) for x in sc["cases"]]
        self.point = bytes.fromhex(sc["point"])
        one = next(x for x in self.cases if int.from_bytes(x[0], "big") == 1)
        assert one[2] == self.point
        self.inf_u = b"\x40" + b"\0" * (self.width - 1)
        self.inf_c = b"\xc0" + b"\0" * (self.width // 2 - 1)
        if g2:
            off = next(x["c"] for x in COMPRESSED["g2"] if x["name"] == "g2_outside_subgroup")
        else:
            off = KEYGEN["univariate"]["table"][23]
        self.wire = [one[3], self.inf_c, bytes.fromhex(off)]

    def table(self):
        pts = _bytes_t(self.wire, self.width // 2)
        return (T.g2_points_prepare_compressed if self.g2 else T.g1_prepare_compressed)(pts), 3

    def prepare(self, encodings):
        pts = _bytes_t(encodings, self.width)
        return (T.g2_points_prepare if self.g2 else T.g1_prepare)(pts)

    def mul(self, tab, count, rows, scalars, sidx):
        f = T.g2_mul_prepared if self.g2 else T.g1_mul_prepared
        return f(tab, count, _i32(rows), _bytes_t(scalars, 32),
                 None if sidx is None else _i32(sidx))

    def split(self, tab, count):
        """(coordinate bytes, status bytes) of a table of `count` points."""
        h = tab.cpu().numpy()
        at = (count * self.width + 255) // 256 * 256
        return h[:count * self.width].tobytes(), h[at:at + count].tobytes()


G1, G2 = Group(False), Group(True)
GROUPS = pytest.mark.parametrize("G", [G1, G2], ids=["g1", "g2"])


def _agrees(G, out, want):
    """out = (table, uncompressed, compressed, status) of a launch, want =
    [(status, uncompressed, compressed)] per lane: encodings and status exact,
    the table bit for bit the decoder's table of the expected bytes."""
    tab, ou, oc, st = out
    n = len(want)
    assert st.cpu().tolist() == [w[0] for w in want]
    assert ou.cpu().numpy().tobytes() == b"".join(w[1] for w in want)
    assert oc.cpu().numpy().tobytes() == b"".join(w[2] for w in want)
    coords, status = G.split(tab, n)
    ref_coords, ref_status = G.split(G.prepare([w[1] for w in want]), n)
    assert status == ref_status == bytes(w[0] for w in want)
    assert coords == ref_coords


@GROUPS
def test_edge_scalars_exact_with_table_bytes(G):
    ks = [int.from_bytes(c[0], "big") for c in G.cases]
    assert {0, 1, 2, R - 1, 1 << 254, R} <= set(ks)
    tab, count = G.table()
    out = G.mul(tab, count, [0] * len(G.cases), [c[0] for c in G.cases], None)
    _agrees(G, out, [(c[1], c[2], c[3]) for c in G.cases])
    # without the encodings the table is the same
    f = T.g2_mul_prepared if G.g2 else T.g1_mul_prepared
    bare, ou, oc, st = f(tab, count, _i32([0] * len(G.cases)),
                         _bytes_t([c[0] for c in G.cases], 32), encode=False)
    assert ou is None and oc is None and st.cpu().tolist() == [c[1] for c in G.cases]
    assert G.split(bare, len(G.cases)) == G.split(out[0], len(G.cases))


def _expect(G, row, si, nscalars, scalars):
    bad = (2, b"\0" * G.width, b"\0" * (G.width // 2))
    if not 0 <= si < nscalars or not 0 <= row < 3 or row == 2:
        return bad
    k = int.from_bytes(scalars[si], "big")
    if k >= R:
        return bad
    if row == 1:
        return (1, G.inf_u, G.inf_c)
    c = next(c for c in G.cases if c[0] == scalars[si])
    return (c[1], c[2], c[3])


@GROUPS
@pytest.mark.parametrize("form", ["one_scalar", "mixed", "no_sidx"])
@pytest.mark.parametrize("lanes", LANES)
def test_lane_counts_and_divergence(G, form, lanes):
    """Invalid lanes (invalid entry, rows -1 and past the end, scalar indices
    -1 and past the end, k = r) sit between valid ones, inside a wave and
    across the block boundary; the neighbours are unaffected."""
    tab, count = G.table()
    scalars = [c[0] for c in G.cases]
    ns = len(scalars)
    row_cycle = [0, 1, 0, 2, 0, -1, 0, 3, 0]
    if form == "one_scalar":     # every lane on 2^254 through sidx; rows vary
        big = next(i for i, s in enumerate(scalars) if int.from_bytes(s, "big") == 1 << 254)
        rows = [row_cycle[j % len(row_cycle)] for j in range(lanes)]
        sidx = [big] * lanes
    elif form == "mixed":        # scalars (and bad indices) change from lane to lane
        sidx_cycle = list(range(ns)) + [-1, 1, ns, 2]
        rows = [row_cycle[(j // 3) % len(row_cycle)] for j in range(lanes)]
        sidx = [sidx_cycle[j % len(sidx_cycle)] for j in range(lanes)]
    else:                        # sidx null: one scalar per lane
        rows = [row_cycle[(j // 2) % len(row_cycle)] for j in range(lanes)]
        scalars = [scalars[(5 * j + 1) % ns] for j in range(lanes)]
        ns, sidx = lanes, None
    if lanes > 1:
        assert {0, 2} <= set(rows)
    out = G.mul(tab, count, rows, scalars, sidx)
    want = [_expect(G, rows[j], j if sidx is None else sidx[j], ns, scalars)
            for j in range(lanes)]
    if lanes >= 63:
        assert {0, 1, 2} == {w[0] for w in want}
    _agrees(G, out, want)


def _poly_at(poly, idx):
    acc = 0
    for c in reversed([int(c, 16) for c in poly]):
        acc = (acc * (idx + 1) + c) % R
    return acc


def test_decryption_shares_of_every_fixture_group_and_their_combine():
    """U = base_mul(u), shares = [f(idx + 1)] U equal the fixture's; the
    created table goes unchanged through decrypt_combine_prepared."""
    for g in COMB["groups"]:
        utab, _, _, ust = K.base_mul(_bytes_t([bytes.fromhex(g["u"])], 32))
        assert ust.cpu().tolist() == [0]
        n = len(g["idx"])
        sk = [_fr(_poly_at(g["poly"], i)) for i in g["idx"]]
        tab, o96, _, st = T.g1_mul_prepared(utab, 1, _i32([0] * n), _bytes_t(sk, 32))
        assert [bytes(s).hex() for s in o96.cpu().numpy()] == g["shares"], g["name"]
        assert all(s in (0, 1) for s in st.cpu().tolist())
        c96, c48, cst = T.decrypt_combine_prepared(tab, n, _i32(list(range(n))), _i32(g["idx"]),
                                                   _offsets([n]))
        assert cst.cpu().tolist() == [g["status"]], g["name"]
        assert bytes(c96[0].cpu().numpy()).hex() == g["g96"], g["name"]
        assert bytes(c48[0].cpu().numpy()).hex() == g["g48"], g["name"]


def test_signature_shares_of_every_fixture_group_and_their_combine():
    """H = [h] of the G2 generator's table entry, shares = [f(idx + 1)] H equal
    the fixture's; the created table goes unchanged through
    sig_combine_prepared to the signature and its parity."""
    gen = next(x for x in COMPRESSED["g2"] if x["name"] == "g2_valid_0")
    assert bytes.fromhex(gen["u"]) == B.g2_bytes(B.G2_GEN)
    gtab = T.g2_points_prepare(_bytes_t([bytes.fromhex(gen["u"])], 192))
    for g in SIGN["groups"]:
        htab, _, _, hst = T.g2_mul_prepared(gtab, 1, _i32([0]),
                                            _bytes_t([bytes.fromhex(g["h"])], 32))
        assert hst.cpu().tolist() == [0]
        n = len(g["idx"])
        sk = [_fr(_poly_at(g["poly"], i)) for i in g["idx"]]
        tab, o192, _, st = T.g2_mul_prepared(htab, 1, _i32([0] * n), _bytes_t(sk, 32))
        assert [bytes(s).hex() for s in o192.cpu().numpy()] == g["shares"], g["name"]
        s192, s96, par, cst = T.sig_combine_prepared(tab, n, _i32(list(range(n))),
                                                     _i32(g["idx"]), _offsets([n]))
        assert cst.cpu().tolist() == [g["status"]], g["name"]
        assert bytes(s192[0].cpu().numpy()).hex() == g["sig192"], g["name"]
        assert bytes(s96[0].cpu().numpy()).hex() == g["sig96"], g["name"]
        assert par.cpu().tolist() == [g["parity"]], g["name"]


def test_create_shares_lay_node_i_item_c_at_row_i_c_plus_c():
    """create_decryption_shares / create_signature_shares over N = 3 secret
    shares and C = 2 points: one launch, row share_row(i, c, C), the bytes of
    the per-lane entry."""
    ks = [c[0] for c in G1.cases if c[1] == 0][:3]
    one48 = next(c for c in G1.cases if int.from_bytes(c[0], "big") == 1)[3]
    two48 = next(c for c in G1.cases if int.from_bytes(c[0], "big") == 2)[3]
    tab, count, o96, o48, st = T.create_decryption_shares(ks, [one48, two48])
    assert count == 6 and st.cpu().tolist() == [0] * 6
    ptab = T.g1_prepare_compressed(_bytes_t([one48, two48], 48))
    for i in range(3):
        for c in range(2):
            _, w96, w48, _ = T.g1_mul_prepared(ptab, 2, _i32([c]), _bytes_t([ks[i]], 32))
            r = T.share_row(i, c, 2)
            assert r == 2 * i + c
            assert bytes(o96[r].cpu().numpy()) == bytes(w96[0].cpu().numpy())
            assert bytes(o48[r].cpu().numpy()) == bytes(w48[0].cpu().numpy())
    assert G1.split(tab, 6) == G1.split(G1.prepare([bytes(v) for v in o96.cpu().numpy()]), 6)
    one192 = G2.point
    two192 = next(c for c in G2.cases if int.from_bytes(c[0], "big") == 2)[2]
    tab, count, o192, o96, st = T.create_signature_shares(ks, [one192, two192])
    assert count == 6 and st.cpu().tolist() == [0] * 6
    want = {int.from_bytes(c[0], "big"): c[2] for c in G2.cases}
    for i in range(3):   # [k] P at item 0
        assert bytes(o192[2 * i].cpu().numpy()) == want[int.from_bytes(ks[i], "big")]
    assert G2.split(tab, 6) == G2.split(G2.prepare([bytes(v) for v in o192.cpu().numpy()]), 6)


def test_base_mul_gives_the_transcripts_commitments():
    for tr in KEYGEN["transcripts"]:
        flat = [bytes.fromhex(c) for f in tr["polys"] for c in f]
        _, _, o48, st = K.base_mul(_bytes_t(flat, 32))
        assert st.cpu().tolist() == [0] * len(flat)
        assert [bytes(v).hex() for v in o48.cpu().numpy()] == \
            [c for cm in tr["commitments"] for c in cm]


@pytest.fixture(scope="module")
def base_cases():
    """(scalar, status, g96) for the edge scalars and the transcripts'
    coefficients: 1 is G1::one(), 2 its double, r - 1 its negative, 2^254 the
    oracle's one multiplication; a coefficient's point is its commitment."""
    one = B.G1_GEN
    neg = (one[0], B.P - one[1])
    inf96 = b"\x40" + b"\0" * 95
    cases = [(0, 1, inf96), (1, 0, T.G1_ONE), (2, 0, B.g1_bytes(B.g1_add(one, one))),
             (R - 1, 0, B.g1_bytes(neg)), (1 << 254, 0, B.g1_bytes(B.g1_mul(one, 1 << 254))),
             (R, 2, b"\0" * 96), ((1 << 256) - 1, 2, b"\0" * 96)]
    tr = KEYGEN["transcripts"][1]
    pts = T.g1_decompress(_bytes_t([bytes.fromhex(c) for cm in tr["commitments"] for c in cm],
                                   48))[0].cpu().numpy()
    coeffs = [int(c, 16) for f in tr["polys"] for c in f]
    return cases + [(k, 0, bytes(p)) for k, p in zip(coeffs, pts)]


@pytest.mark.parametrize("lanes", LANES)
def test_base_mul_edge_scalars_lane_counts_and_its_own_check(base_cases, lanes):
    pick = [base_cases[(3 * j) % len(base_cases)] for j in range(lanes)]
    if lanes == 1:
        pick = [base_cases[4]]
    scalars = _bytes_t([_fr(k) for k, _, _ in pick], 32)
    tab, o96, o48, st = K.base_mul(scalars)
    assert st.cpu().tolist() == [s for _, s, _ in pick]
    assert o96.cpu().numpy().tobytes() == b"".join(g for _, _, g in pick)
    assert G1.split(tab, lanes) == G1.split(G1.prepare([g for _, _, g in pick]), lanes)
    ref48 = T.g1_prepare_compressed(o48)   # the compressed form decodes to the same table
    assert G1.split(ref48, lanes) == G1.split(tab, lanes)
    # the existing check against the table base_mul wrote: [s] G1::one() == T[i]
    ok = K.base_mul_check(tab, lanes, _i32(list(range(lanes))), scalars).cpu().tolist()
    assert ok == [2 if s == 2 else 1 for _, s, _ in pick]
    if lanes > 1:   # and it tells a neighbour's point from its own
        shifted = K.base_mul_check(tab, lanes, _i32([(j + 1) % lanes for j in range(lanes)]),
                                   scalars).cpu().tolist()
        for j, (k, s, _) in enumerate(pick):
            nk, ns, _ = pick[(j + 1) % lanes]
            assert shifted[j] == (2 if s == 2 or ns == 2 else int(k % R == nk % R)), j
