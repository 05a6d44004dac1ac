"""GPU check of the prepared tables' status offset (csrc/pairing_tables.hpp):
for each table kind, counts whose coordinates end exactly on a 256-byte
boundary and their neighbours (G1 keys 96 bytes a point: 8 against 7 and 9; G2
points 192 bytes: 4 against 3 and 5; Miller-loop lines 19,584 bytes: 2 against
1 and 3).  Each count is prepared twice, every row valid and the last row
invalid, and the first and the last row are read back through a consumer of
that kind: an invalid row must come back as 2, a valid one as the outcome the
oracle recorded in tests/golden/bls_vectors.json (its GT values, and the
scalars of its points for the fixed-base check).  The output-table view is
covered by multiplying into tables of the same counts and reading them back."""
import json
import os

import numpy as np
import pytest

from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


PAIRINGS = _gold("bls_vectors.json")["pairings"]
COMPRESSED = _gold("compressed_vectors.json")
# the oracle's GT value of e([a] G1::one(), [b] G2::one()), and those points
GT = {(p["g1_scalar"], p["g2_scalar"]): p["gt"] for p in PAIRINGS}
G1 = {p["g1_scalar"]: bytes.fromhex(p["g1"]) for p in PAIRINGS}
G2 = {p["g2_scalar"]: bytes.fromhex(p["g2"]) for p in PAIRINGS}
assert GT[(2, 1)] == GT[(1, 2)] != GT[(1, 1)]
C48 = {e["name"]: bytes.fromhex(e["c"]) for e in COMPRESSED["g1"]}
C96 = {e["name"]: bytes.fromhex(e["c"]) for e in COMPRESSED["g2"]}
U = {e["name"]: bytes.fromhex(e["u"]) for e in COMPRESSED["g1"] + COMPRESSED["g2"]}
assert U["g1_valid_0"] == G1[1] and U["g1_valid_1"] == G1[2]
assert U["g2_valid_0"] == G2[1] and U["g2_valid_1"] == G2[2]

pytestmark = pytest.mark.gpu


def _i32(values):
    import torch
    return torch.tensor(values, dtype=torch.int32, device="cuda:0")


def _bytes_t(rows, width):
    import torch
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)
    return torch.from_numpy(a.copy()).to("cuda:0")


def _fr(v):
    return (v % B.R).to_bytes(32, "big")


def _off_curve(point):
    """A golden point with its last coordinate bit flipped: on no curve."""
    return point[:-1] + bytes([point[-1] ^ 1])


def _scalars(count, last_valid):
    """Row scalars of a table: 2 in the first row, 1 between, 2 (or None: an
    invalid point) in the last; a table of one row is its last row."""
    return ([2] + [1] * (count - 2) if count > 1 else []) + [2 if last_valid else None]


def _gt_outcome(left, right):
    """A check's outcome from the oracle's GT values: left and right are
    (G1 scalar, G2 scalar), a None scalar is an invalid point."""
    if None in left + right:
        return 2
    return int(GT[left] == GT[right])


@pytest.mark.parametrize("count", [7, 8, 9])
@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("last_valid", [True, False])
def test_g1_table_status_offset(count, compressed, last_valid):
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    m = _scalars(count, last_valid)
    assert all(B.g1_bytes(B.g1_mul(B.G1_GEN, s)) == G1[s] for s in (1, 2))
    if compressed:
        rows = [C48["g1_valid_%d" % (s - 1)] if s else C48["g1_outside_subgroup"] for s in m]
        tab = T.g1_prepare_compressed(_bytes_t(rows, 48))
    else:
        tab = T.g1_prepare(_bytes_t([G1[s] if s else _off_curve(G1[1]) for s in m], 96))
    assert tab.numel() == T.lib().hbrbc_g1_prepared_size(count)
    # [s] G1::one() == T[row]: the first row against its scalar and another, the last row
    read = [(0, 2), (0, 1), (count - 1, 2), (count - 1, 1)]
    ok = K.base_mul_check(tab, count, _i32([r for r, _ in read]),
                          _bytes_t([_fr(s) for _, s in read], 32))
    assert ok.cpu().tolist() == [2 if m[r] is None else int(m[r] == s) for r, s in read]
    # the same rows as the a_i of e(a_i, P[0]) == e(K[0], P[1]), read by position i
    keys = T.g1_prepare(_bytes_t([G1[1]], 96))
    prep = T.g2_prepare(_bytes_t([G2[1], G2[2]], 192))
    zero, one = _i32([0] * count), _i32([1] * count)
    ok = T.pairing_check_prepared_pts(tab, count, keys, 1, zero, prep, 2, zero, one)
    got = ok.cpu().tolist()
    assert [got[0], got[-1]] == [_gt_outcome((m[i], 1), (1, 2)) for i in (0, count - 1)]


@pytest.mark.parametrize("count", [1, 2, 3])
@pytest.mark.parametrize("last_valid", [True, False])
def test_lines_table_status_offset(count, last_valid):
    from hbbft_amd import threshold as T
    # rows [2] G2::one() first, G2::one() after it; the last one invalid or not
    m = ([2] + [1] * (count - 2) if count > 1 else []) + [1 if last_valid else None]
    prep = T.g2_prepare(_bytes_t([G2[s] if s else _off_curve(G2[1]) for s in m], 192))
    assert prep.numel() == T.lib().hbrbc_g2_prepared_size(count)
    # e([a] G1::one(), P[b]) == e([c] G1::one(), P[d]) as (a, b, c, d)
    last = count - 1
    checks = [(1, 0, 1, 0), (1, 0, 2, last), (1, 0, 1, last), (1, last, 1, last),
              (2, last, 1, last)]
    g1 = _bytes_t([G1[s] for a, _, c, _ in checks for s in (a, c)], 96)
    ok = T.pairing_check_prepared(g1, prep, count, _i32([b for _, b, _, _ in checks]),
                                  _i32([d for _, _, _, d in checks]))
    want = [_gt_outcome((a, m[b]), (c, m[d])) for a, b, c, d in checks]
    assert ok.cpu().tolist() == want and (not last_valid or {0, 1} <= set(want))


@pytest.mark.parametrize("count", [3, 4, 5])
@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("last_valid", [True, False])
def test_g2_points_table_status_offset(count, compressed, last_valid):
    from hbbft_amd import threshold as T
    m = _scalars(count, last_valid)
    if compressed:
        rows = [C96["g2_valid_%d" % (s - 1)] if s else C96["g2_outside_subgroup"] for s in m]
        stab = T.g2_points_prepare_compressed(_bytes_t(rows, 96))
    else:
        stab = T.g2_points_prepare(_bytes_t([G2[s] if s else _off_curve(G2[1]) for s in m], 192))
    assert stab.numel() == T.lib().hbrbc_g2_points_size(count)
    keys = T.g1_prepare(_bytes_t([G1[1], G1[2]], 96))
    prep = T.g2_prepare(_bytes_t([G2[1]], 192))
    zero = _i32([0] * count)
    # check i is e(K[k], P[0]) == e(G1::one(), S[i]) for K = G1::one() (k = 0) and [2] G1::one()
    for k in (0, 1):
        ok = T.sig_check_prepared(stab, count, keys, 2, _i32([k] * count), prep, 1, zero)
        assert ok.cpu().tolist() == [_gt_outcome((k + 1, 1), (1, s)) for s in m]


@pytest.mark.parametrize("count", [7, 8, 9])
def test_g1_output_table_status_offset(count):
    """g1_mul_prepared into a table of `count` results whose last one is
    invalid, read back through base_mul_check."""
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    tab = T.g1_prepare(_bytes_t([G1[2], _off_curve(G1[1])], 96))
    s = 0x1234567 + (1 << 130)
    out, o96, _, st = T.g1_mul_prepared(tab, 2, _i32([0] * (count - 1) + [1]),
                                        _bytes_t([_fr(s)] * count, 32))
    assert out.numel() == T.lib().hbrbc_g1_prepared_size(count)
    assert st.cpu().tolist() == [0] * (count - 1) + [2]
    assert bytes(o96[0].cpu().numpy()) == B.g1_bytes(B.g1_mul(B.G1_GEN, 2 * s % B.R))
    read = [(0, 2 * s), (0, s), (count - 2, 2 * s), (count - 1, 2 * s)]
    ok = K.base_mul_check(out, count, _i32([r for r, _ in read]),
                          _bytes_t([_fr(v) for _, v in read], 32))
    assert ok.cpu().tolist() == [1, 0, 1, 2]
