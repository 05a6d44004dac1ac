"""CPU-side checks of the threshold-signature path (`ThresholdSign`): the
fixture tests/golden/sign_vectors.json is consistent with its own polynomials
in integers and, for one group, on the twist through oracle/bls_oracle.py; the
parity bytes and compressed flags follow from the stored encodings; the C ABI,
the built library, the Python module and the Rust declarations carry the new
entries; without a GPU every call fails loudly."""
import ctypes
import json
import os
import re

import pytest

import __graft_entry__
from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "sign_vectors.json")))
SYMBOLS = ["hbrbc_g2_points_size", "hbrbc_g2_points_prepare", "hbrbc_sig_check_prepared",
           "hbrbc_g2_combine_workspace_size", "hbrbc_g2_lincomb_prepared",
           "hbrbc_sig_combine_prepared", "hbrbc_sig_combine"]
PY_NAMES = ["g2_points_prepare", "sig_check_prepared", "g2_lincomb_prepared",
            "sig_combine_prepared", "combine_g2_workspace", "verify_signature_shares",
            "combine_signature_shares", "sig_combine", "threshold_sign_grouped"]


@pytest.fixture(scope="module")
def built():
    __graft_entry__.build()


def _poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % B.R
    return acc


def _decode(h):
    """192 bytes x.c1 || x.c0 || y.c1 || y.c0 -> ((x0, x1), (y0, y1))."""
    raw = bytes.fromhex(h)
    v = [int.from_bytes(raw[48 * i:48 * i + 48], "big") for i in range(4)]
    return ((v[1], v[0]), (v[3], v[2]))


def _results():
    """Every stored result: groups, scalar cases and documents."""
    return GOLD["groups"] + GOLD["scalar_cases"]["cases"] + GOLD["epoch"]["documents"]


def test_fixture_is_consistent_in_integers():
    """sum lambda_i = 1 and sum lambda_i f(x_i) = f(0) mod r for every group,
    with x_i = idx_i + 1."""
    assert [g["name"] for g in GOLD["groups"]] == [
        "t0", "t1", "t2_of_7", "cfg3_a", "cfg3_b", "x_2_32", "f0_zero", "share_at_infinity"]
    for g in GOLD["groups"]:
        f = [int(c, 16) for c in g["poly"]]
        lam = [int(c, 16) for c in g["lambdas"]]
        assert len(f) == g["t"] + 1 == len(g["idx"]) == len(lam) == len(g["shares"]), g["name"]
        assert sum(lam) % B.R == 1, g["name"]
        vals = [_poly_eval(f, i + 1) for i in g["idx"]]
        assert sum(l * v for l, v in zip(lam, vals)) % B.R == f[0], g["name"]
        assert (g["status"] == 1) == (f[0] == 0)
    by = {g["name"]: g for g in GOLD["groups"]}
    assert by["t0"]["sig192"] == by["t0"]["shares"][0]
    assert by["cfg3_a"]["sig192"] == by["cfg3_b"]["sig192"]
    assert by["cfg3_a"]["idx"] != by["cfg3_b"]["idx"]
    assert 0xFFFFFFFF in by["x_2_32"]["idx"]
    assert by["f0_zero"]["sig192"] == "40" + "00" * 191
    assert by["f0_zero"]["sig96"] == "c0" + "00" * 95
    assert "40" + "00" * 191 in by["share_at_infinity"]["shares"]
    x2 = B.X_ABS ** 2
    assert [int(c["k"], 16) for c in GOLD["scalar_cases"]["cases"]] == [
        0, 1, 2, x2 - 1, x2, x2 + 1, B.R - 1, 1 << 254, B.R]
    ep = GOLD["epoch"]
    assert ep["n"] == 7 and ep["t"] == 2 and len(ep["documents"]) == 2
    assert all(len(d["shares"]) == 7 and d["verified"] for d in ep["documents"])
    assert sum(not s["expect"] for d in ep["documents"] for s in d["shares"]) == 5


def test_group_t1_on_the_twist():
    """Group t1 through the oracle's curve arithmetic (two scalar
    multiplications in G2)."""
    g = GOLD["groups"][1]
    s0, s1 = (_decode(s) for s in g["shares"])
    lam = [int(c, 16) for c in g["lambdas"]]
    got = B.g2_add(B.g2_mul(s0, lam[0]), B.g2_mul(s1, lam[1]))
    assert B.g2_bytes(got).hex() == g["sig192"]


def test_parity_is_the_xor_of_the_stored_bits():
    seen = set()
    for r in _results():
        bits = sum(bin(b).count("1") for b in bytes.fromhex(r["sig192"]))
        assert r["parity"] == bits & 1
        seen.add(r["parity"])
    assert seen == {0, 1}


def test_compressed_flags_follow_from_y():
    """x.c1 || x.c0 with 0x80 set; 0x20 set iff y is the larger of y and -y,
    c1 compared first and c0 only when the c1 are equal."""
    flags = set()
    for r in _results():
        if r["status"] != 0:
            continue
        (x0, x1), (y0, y1) = _decode(r["sig192"])
        n0, n1 = (-y0) % B.P, (-y1) % B.P
        larger = y1 > n1 if y1 != n1 else y0 > n0
        want = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
        want[0] |= 0x80 | (0x20 if larger else 0)
        assert bytes(want).hex() == r["sig96"]
        flags.add(want[0] & 0x20)
    assert flags == {0, 0x20}


def test_header_declares_and_library_exports_the_entries(built):
    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    src = open(os.path.join(ROOT, "include", "hbrbc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(hbrbc_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(hb.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert hasattr(hb.lib(), s), s
    for name in PY_NAMES:
        assert callable(getattr(T, name)), name
    pts = hb.lib().hbrbc_g2_points_size
    assert pts(0) == 0
    # 48 words per affine point and a status byte
    assert pts(7) >= 7 * (48 * 4 + 1) and pts(64) > pts(7)
    size = hb.lib().hbrbc_g2_combine_workspace_size
    assert size(0, 0) == 0
    # 72 words per projective point, a status byte and a coefficient per share
    assert size(22, 1) >= 22 * (72 * 4 + 1 + 32) + 1
    assert size(44, 2) > size(22, 1)


def test_ffi_rs_lists_the_entries():
    rs = open(os.path.join(ROOT, "hbbft-hip", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert "pub fn %s(" % s in rs, s
    lib_rs = open(os.path.join(ROOT, "hbbft-hip", "src", "lib.rs")).read()
    assert "pub fn sig_combine(" in lib_rs and "ffi::hbrbc_sig_combine(" in lib_rs


def test_no_cpu_fallback_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    g = GOLD["groups"][1]
    grp = [(i, bytes.fromhex(s)) for i, s in zip(g["idx"], g["shares"])]
    ep = GOLD["epoch"]
    doc = ep["documents"][0]
    h, s0 = bytes.fromhex(doc["hash"]), doc["shares"][0]
    share, pk = bytes.fromhex(s0["share"]), bytes.fromhex(s0["pk"])
    with pytest.raises(hb.HbrbcUnavailable):
        T.combine_signature_shares([grp])
    with pytest.raises(hb.HbrbcUnavailable):
        T.verify_signature_shares([(share, pk, h)])
    with pytest.raises(hb.HbrbcUnavailable):
        T.threshold_sign_grouped([h], [(0, s0["node"], share, pk)], ep["t"],
                                 bytes.fromhex(ep["public_key"]))
    with pytest.raises(hb.HbrbcUnavailable):   # HBRBC_E_NO_DEVICE (102) from the C entry
        T.sig_combine(grp)
    o192, o96 = ctypes.create_string_buffer(192), ctypes.create_string_buffer(96)
    par = ctypes.create_string_buffer(1)
    idx = (ctypes.c_uint32 * 2)(*g["idx"])
    assert hb.lib().hbrbc_sig_combine(b"".join(s for _, s in grp), ctypes.addressof(idx), 2,
                                      o192, o96, par) == 102
    assert hb.lib().hbrbc_g2_points_prepare(None, 1, None, None) == 100   # null argument
