"""CPU-side checks of the decryption-share combine (`PublicKeySet::decrypt` up
to g): the fixture tests/golden/combine_vectors.json is consistent with its
own polynomials in integers and, for one group, on the curve through
oracle/bls_oracle.py; the C ABI, the built library and the Rust declarations
carry the five entries; without a GPU the call fails loudly."""
import ctypes
import json
import os
import re

import pytest

import __graft_entry__
from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "combine_vectors.json")))
SYMBOLS = ["hbrbc_g1_combine_workspace_size", "hbrbc_lagrange_coeffs", "hbrbc_g1_lincomb_prepared",
           "hbrbc_decrypt_combine_prepared", "hbrbc_decrypt_combine"]


@pytest.fixture(scope="module")
def built():
    __graft_entry__.build()


def _poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % B.R
    return acc


def test_fixture_is_consistent_in_integers():
    """sum lambda_i = 1 and sum lambda_i f(x_i) = f(0) mod r for every group,
    with x_i = idx_i + 1."""
    assert [g["name"] for g in GOLD["groups"]] == [
        "t0", "t1", "t2_of_7", "cfg3_a", "cfg3_b", "x_2_32", "f0_zero", "share_at_infinity"]
    for g in GOLD["groups"]:
        f = [int(c, 16) for c in g["poly"]]
        lam = [int(c, 16) for c in g["lambdas"]]
        assert len(f) == g["t"] + 1 == len(g["idx"]) == len(lam) == len(g["shares"]), g["name"]
        assert all(0 <= l < B.R for l in lam)
        assert sum(lam) % B.R == 1, g["name"]
        vals = [_poly_eval(f, i + 1) for i in g["idx"]]
        assert sum(l * v for l, v in zip(lam, vals)) % B.R == f[0], g["name"]
        assert (g["status"] == 1) == (f[0] == 0)
    by = {g["name"]: g for g in GOLD["groups"]}
    assert by["t1"]["lambdas"] == ["%064x" % 2, "%064x" % (B.R - 1)]
    assert by["t0"]["g96"] == by["t0"]["shares"][0]
    assert by["cfg3_a"]["g96"] == by["cfg3_b"]["g96"] and by["cfg3_a"]["idx"] != by["cfg3_b"]["idx"]
    assert 0xFFFFFFFF in by["x_2_32"]["idx"]
    assert by["f0_zero"]["g96"] == "40" + "00" * 95 and by["f0_zero"]["g48"] == "c0" + "00" * 47
    assert "40" + "00" * 95 in by["share_at_infinity"]["shares"]
    flags = {int(g["g48"][:2], 16) & 0x20 for g in GOLD["groups"] if g["status"] == 0}
    assert flags == {0, 0x20}


def _decode(h):
    raw = bytes.fromhex(h)
    return (int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big"))


def test_group_t1_on_the_curve_and_compressed_rule():
    """Group t1 through the oracle's curve arithmetic (two scalar
    multiplications), and the compressed encoding of its g: x with 0x80 set,
    0x20 set iff y > p - y."""
    g = GOLD["groups"][1]
    s0, s1 = (_decode(s) for s in g["shares"])
    lam = [int(c, 16) for c in g["lambdas"]]
    got = B.g1_add(B.g1_mul(s0, lam[0]), B.g1_mul(s1, lam[1]))
    assert B.g1_bytes(got).hex() == g["g96"]
    x, y = _decode(g["g96"])
    want = bytearray(x.to_bytes(48, "big"))
    want[0] |= 0x80 | (0x20 if y > B.P - y else 0)
    assert bytes(want).hex() == g["g48"]


def test_header_declares_and_library_exports_the_entries(built):
    import hbbft_amd as hb
    src = open(os.path.join(ROOT, "include", "hbrbc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(hbrbc_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(hb.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
    size = hb.lib().hbrbc_g1_combine_workspace_size
    assert size(0, 0) == 0
    # 36 words per projective point, a status byte and a coefficient per share
    assert size(22, 1) >= 22 * (36 * 4 + 1 + 32) + 1
    assert size(44, 2) > size(22, 1)


def test_ffi_rs_lists_the_entries():
    rs = open(os.path.join(ROOT, "hbbft-hip", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert "pub fn %s(" % s in rs, s
    assert "ffi::hbrbc_decrypt_combine(" in open(os.path.join(ROOT, "hbbft-hip", "src", "lib.rs")).read()


def test_no_cpu_fallback_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    g = GOLD["groups"][1]
    grp = [(i, bytes.fromhex(s)) for i, s in zip(g["idx"], g["shares"])]
    with pytest.raises(hb.HbrbcUnavailable):
        T.combine_decryption_shares([grp])
    with pytest.raises(hb.HbrbcUnavailable):   # HBRBC_E_NO_DEVICE (102) from the C entry
        T.decrypt_combine(grp)
    o96, o48 = ctypes.create_string_buffer(96), ctypes.create_string_buffer(48)
    idx = (ctypes.c_uint32 * 2)(*g["idx"])
    assert hb.lib().hbrbc_decrypt_combine(b"".join(s for _, s in grp), ctypes.addressof(idx), 2,
                                          o96, o48) == 102
