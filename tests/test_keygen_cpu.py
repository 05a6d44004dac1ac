"""CPU-side checks of the key generation path: tests/golden/keygen_vectors.json
agrees with a recomputation through oracle/bls_oracle.py (all scalars, and the
points of the small transcripts by sampling: Python-integer multiplications
take a fifth of a second each); the C ABI, the built library, the Python module
and the Rust declarations carry the two entries; without a GPU every call
fails loudly; the commitment layout is a bijection on unordered pairs."""
import ctypes
import json
import os
import re

import pytest

import __graft_entry__
import compressed_ref as C
from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "keygen_vectors.json")))
R, P = B.R, B.P
SYMBOLS = ["hbrbc_g1_poly_eval_prepared", "hbrbc_g1_base_mul_check"]
PY_NAMES = ["coeff_pos", "poly_eval_prepared", "base_mul_check", "commitment_rows",
            "public_key_shares", "check_parts", "check_acks", "generate_public",
            "sync_key_gen_grouped"]


@pytest.fixture(scope="module")
def built():
    __graft_entry__.build()


def _point(hex48):
    """A compressed point of the fixture as an affine pair (no order-r check:
    the generator made it by multiplying the generator)."""
    raw = bytes.fromhex(hex48)
    if raw[0] & 0x40:
        return None
    x = int.from_bytes(bytes([raw[0] & 0x1F]) + raw[1:], "big")
    y = pow((x * x * x + B.B1) % P, (P + 1) // 4, P)
    if (y > P - y) != bool(raw[0] & 0x20):
        y = P - y
    assert B.g1_on_curve((x, y))
    return (x, y)


def _eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def _point_eval(points, x):
    acc = None
    for c in reversed(points):
        acc = B.g1_add(B.g1_mul(acc, x) if acc is not None and x else None, c)
    return acc


def test_coeff_pos_is_symmetric_and_covers_the_triangle():
    from hbbft_amd import keygen as K
    for t in (0, 1, 2, 5, 21):
        seen = {}
        for i in range(t + 1):
            for j in range(t + 1):
                assert K.coeff_pos(i, j) == K.coeff_pos(j, i)
                seen.setdefault(K.coeff_pos(i, j), set()).add(frozenset((i, j)))
        assert sorted(seen) == list(range((t + 1) * (t + 2) // 2))
        assert all(len(pairs) == 1 for pairs in seen.values())
        assert K.commitment_len(t) == len(seen)


def test_transcript_scalars_follow_from_the_polynomials():
    from hbbft_amd.keygen import coeff_pos as pos
    for tr in GOLD["transcripts"]:
        n, t = tr["n"], tr["t"]
        polys = [[int(c, 16) for c in f] for f in tr["polys"]]
        assert all(len(f) == (t + 1) * (t + 2) // 2 and all(0 < c < R for c in f) for f in polys)
        for p, f in enumerate(polys):
            for node in range(n):
                row = [sum(f[pos(i, j)] * pow(node + 1, i, R) for i in range(t + 1)) % R
                       for j in range(t + 1)]
                assert [int(c, 16) for c in tr["rows"][p][node]] == row
                for s in range(n):
                    assert int(tr["values"][p][s][node], 16) == _eval(row, s + 1)
        complete = [p for p in range(n) if len(set(tr["ack_senders"][p])) > 2 * t]
        assert complete == tr["complete"] and len(complete) > t
    assert GOLD["transcripts"][0]["complete"] == [0, 1, 2, 3]
    assert GOLD["transcripts"][1]["complete"] == [0, 1, 2, 3, 4, 5]   # 2t Acks are not enough


def test_transcript_points_agree_with_the_oracle():
    from hbbft_amd.keygen import coeff_pos as pos
    for k, tr in enumerate(GOLD["transcripts"]):
        n, t = tr["n"], tr["t"]
        commits = [[_point(c) for c in cm] for cm in tr["commitments"]]
        # the key set: sums of stored points; its constant term against the scalars
        key_set = [None] * (t + 1)
        for p in tr["complete"]:
            key_set = [B.g1_add(a, commits[p][pos(0, j)]) for j, a in enumerate(key_set)]
        for j, want in enumerate(key_set):
            assert tr["key_set"][j]["g96"] == B.g1_bytes(want).hex()
            assert tr["key_set"][j]["g48"] == C.compress_g1(want).hex()
        for i in range(n):   # node indices of a few bits: cheap in Python too
            share = _point_eval(key_set, i + 1)
            assert tr["key_shares"][i]["g96"] == B.g1_bytes(share).hex()
            assert tr["key_shares"][i]["g48"] == C.compress_g1(share).hex()
        if k:
            continue
        master = sum(int(tr["polys"][p][0], 16) for p in tr["complete"]) % R
        assert key_set[0] == B.g1_mul(B.G1_GEN, master)
        # one commitment point, one row coefficient and one ack value by multiplication
        p, node, s = 2, 1, 3
        assert commits[p][pos(1, 0)] == B.g1_mul(B.G1_GEN, int(tr["polys"][p][pos(1, 0)], 16))
        crow = [_point_eval([commits[p][pos(i, j)] for i in range(t + 1)], node + 1)
                for j in range(t + 1)]
        assert crow[1] == B.g1_mul(B.G1_GEN, int(tr["rows"][p][node][1], 16))
        assert _point_eval(crow, s + 1) == B.g1_mul(B.G1_GEN, int(tr["values"][p][s][node], 16))


def test_tamper_and_univariate_cases_cover_the_rules():
    t0 = GOLD["transcripts"][0]
    by = {c["name"]: c for c in GOLD["tamper"]}
    assert {c["field"] for c in GOLD["tamper"]} == {"row", "value", "commit"}
    c = by["row_coefficient_changed"]
    assert c["bytes"] != t0["rows"][c["part"]][c["our_idx"]][c["index"]] and c["expect"] is False
    c = by["ack_value_changed"]
    assert c["bytes"] != t0["values"][c["part"]][c["index"]][c["our_idx"]] and c["expect"] is False
    assert int(by["ack_value_is_r"]["bytes"], 16) == R and by["ack_value_is_r"]["expect"] is None
    off = B.g1_curve_point(0x5EED)   # on the curve: only the order-r check rejects it
    assert by["commitment_point_outside_g1"]["bytes"] == C.compress_g1(off).hex()
    uni = GOLD["univariate"]
    assert uni["table"][23] == C.compress_g1(off).hex() and uni["table"][22] == "c0" + "00" * 47
    names = {c["name"] for c in uni["cases"]}
    for x in (0, 1, 2, 64, 65, 0xFFFFFFFF):
        assert "degree21_at_%d" % x in names
    assert {"degree0_at_0", "infinity_in_the_middle_at_3", "infinity_leading_at_3",
            "root_at_4_at_4"} <= names
    assert {c["status"] for c in uni["cases"]} == {0, 1, 2}
    for c in uni["cases"]:
        assert all(0 <= r < len(uni["table"]) for r in c["rows"])
        if c["status"] == 2:
            assert c["g96"] == "00" * 96 and c["g48"] == "00" * 48
        if c["status"] == 1:
            assert c["g96"] == "40" + "00" * 95 and c["g48"] == "c0" + "00" * 47
        if c["x"] == 0 and c["status"] == 0:   # x = 0: the constant term itself
            assert c["g48"] == uni["table"][c["rows"][0]]
    case = next(c for c in uni["cases"] if c["name"] == "degree1_at_100")
    pts = [_point(uni["table"][r]) for r in case["rows"]]
    assert B.g1_bytes(_point_eval(pts, 100)).hex() == case["g96"]
    # the epoch of combine_vectors.json: its key shares follow from this commitment
    comb = json.load(open(os.path.join(ROOT, "tests", "golden", "combine_vectors.json")))["epoch"]
    epoch = [_point(c) for c in GOLD["epoch_commitment"]]
    assert len(epoch) == comb["t"] + 1
    share = next(s for s in comb["ciphertexts"][0]["shares"] if s["expect"])
    assert B.g1_bytes(_point_eval(epoch, share["node"] + 1)).hex() == share["pk"]


def test_header_declares_and_library_exports_the_entries(built):
    import hbbft_amd as hb
    from hbbft_amd import keygen as K
    src = open(os.path.join(ROOT, "include", "hbrbc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(hbrbc_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(hb.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert hasattr(hb.lib(), s), s
    for name in PY_NAMES:
        assert callable(getattr(K, name)), name
    rs = open(os.path.join(ROOT, "hbbft-hip", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert "pub fn %s(" % s in rs, s


def test_entries_check_their_arguments(built):
    import hbbft_amd as hb
    L = hb.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    # zero counts are ok whatever the pointers; a null pointer is 100
    assert L.hbrbc_g1_poly_eval_prepared(None, 0, None, None, 0, None, None, 0, None, None, None,
                                         None, None) == 0
    assert L.hbrbc_g1_base_mul_check(None, 0, None, None, 0, None, None) == 0
    full = [p, 1, p, p, 1, p, p, 1, p, p, p, p, None]
    for k in (0, 2, 3, 5, 6, 8, 11):
        args = list(full)
        args[k] = None
        assert L.hbrbc_g1_poly_eval_prepared(*args) == 100, k
    full = [p, 1, p, p, 1, p, None]
    for k in (0, 2, 3, 5):
        args = list(full)
        args[k] = None
        assert L.hbrbc_g1_base_mul_check(*args) == 100, k


def test_no_cpu_fallback_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import hbbft_amd as hb
    from hbbft_amd import keygen as K
    L = hb.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert L.hbrbc_g1_poly_eval_prepared(p, 1, p, p, 1, p, p, 1, p, None, None, p, None) == 102
    assert L.hbrbc_g1_base_mul_check(p, 1, p, p, 1, p, None) == 102   # HBRBC_E_NO_DEVICE
    tr = GOLD["transcripts"][0]
    t = tr["t"]
    parts = [([bytes.fromhex(c) for c in tr["commitments"][q]],
              [bytes.fromhex(c) for c in tr["rows"][q][0]]) for q in range(tr["n"])]
    acks = [(0, 1, bytes.fromhex(tr["values"][0][1][0]))]
    tab = torch.zeros(hb.lib().hbrbc_g1_prepared_size(1), dtype=torch.uint8)
    i32 = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(hb.HbrbcUnavailable):
        K.poly_eval_prepared(tab, 1, i32, torch.tensor([0, 1], dtype=torch.int32), i32, i32)
    with pytest.raises(hb.HbrbcUnavailable):
        K.base_mul_check(tab, 1, i32, torch.zeros((1, 32), dtype=torch.uint8))
    with pytest.raises(hb.HbrbcUnavailable):
        K.check_parts(t, 0, parts)
    with pytest.raises(hb.HbrbcUnavailable):
        K.check_acks(t, (tab, 1), acks)
    with pytest.raises(hb.HbrbcUnavailable):
        K.generate_public(t, [parts[0][0]])
    with pytest.raises(hb.HbrbcUnavailable):
        K.public_key_shares([bytes.fromhex(c) for c in GOLD["epoch_commitment"]], 7)
    with pytest.raises(hb.HbrbcUnavailable):
        K.sync_key_gen_grouped(t, 0, parts, acks)
    # a node index whose x = idx + 1 does not fit 32 bits, and a wrong length,
    # are the caller's errors before any device is looked for
    with pytest.raises(ValueError):
        K.check_parts(t, 0xFFFFFFFF, parts)
    with pytest.raises(ValueError):
        K.check_acks(t, (tab, 1), [(0, 0xFFFFFFFF, acks[0][2])])
    with pytest.raises(ValueError):
        K.sync_key_gen_grouped(t, 1 << 32, parts, acks)
    with pytest.raises(ValueError):
        K.public_key_shares([b"\0" * 96], 4)
