"""CPU-side checks of the compressed wire encodings: the Python restatement of
`G1Compressed::into_affine` / `G2Compressed::into_affine` (tests/
compressed_ref.py) maps every case of tests/golden/compressed_vectors.json to
its stored result and every compressed result of the two combine fixtures back
to its uncompressed one; the C ABI, the built library, the Python module and
the Rust declarations carry the four entries; without a GPU every call fails
loudly."""
import ctypes
import json
import os
import re

import pytest

import __graft_entry__
import compressed_ref as C
from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


GOLD = _gold("compressed_vectors.json")
SYMBOLS = ["hbrbc_g1_prepare_compressed", "hbrbc_g2_points_prepare_compressed",
           "hbrbc_g1_decompress", "hbrbc_g2_decompress"]
PY_NAMES = ["g1_prepare_compressed", "g2_points_prepare_compressed", "g1_decompress",
            "g2_decompress", "decrypt_shares_grouped_wire", "threshold_sign_grouped_wire"]


@pytest.fixture(scope="module")
def built():
    __graft_entry__.build()


def test_restatement_maps_every_fixture_case():
    for key, dec, width in (("g1", C.decompress_g1, 48), ("g2", C.decompress_g2, 96)):
        cases = GOLD[key]
        assert len(cases) >= 20
        for c in cases:
            raw = bytes.fromhex(c["c"])
            assert len(raw) == width
            assert dec(raw) == (c["status"], bytes.fromhex(c["u"])), c["name"]
        assert {c["status"] for c in cases} == {C.OK, C.INF, C.BAD}
        # both sign flags among the valid points, and pairs that differ in the
        # flag alone and decode to a point and its negative
        ok = [c for c in cases if c["status"] == C.OK]
        assert {int(c["c"][:2], 16) & 0x20 for c in ok} == {0, 0x20}
        by_x = {}
        for c in ok:
            raw = bytearray(bytes.fromhex(c["c"]))
            raw[0] &= 0xDF
            by_x.setdefault(bytes(raw), []).append(c)
        pairs = [v for v in by_x.values() if len(v) == 2]
        assert len(pairs) >= 4
        for a, b in pairs:
            half = width
            assert a["u"][:2 * half] == b["u"][:2 * half] and a["u"] != b["u"]
        # invalid cases decode to zero bytes, infinity to 0x40 and zeros
        for c in cases:
            if c["status"] == C.BAD:
                assert c["u"] == "00" * (2 * width), c["name"]
            if c["status"] == C.INF:
                assert c["u"] == "40" + "00" * (2 * width - 1)


def test_fixture_covers_the_rules():
    """Each rule of the decoding has a case that only it rejects."""
    for key, width in (("g1", 48), ("g2", 96)):
        by = {c["name"][3:]: c for c in GOLD[key]}
        assert by["infinity"]["c"] == "c0" + "00" * (width - 1)
        assert by["infinity_with_sign_flag"]["c"] == "e0" + "00" * (width - 1)
        assert by["infinity_with_trailing_byte"]["c"] == "c0" + "00" * (width - 2) + "01"
        clear = bytearray(bytes.fromhex(by["compression_flag_clear"]["c"]))
        assert not clear[0] & 0x80
        clear[0] |= 0x80
        assert bytes(clear).hex() in [c["c"] for c in GOLD[key] if c["status"] == C.OK]
        xp = bytearray(bytes.fromhex(by["x_is_p"]["c"])[:48])
        assert xp[0] & 0xE0 == 0x80
        xp[0] &= 0x1F
        assert int.from_bytes(xp, "big") == B.P
        for name in ("outside_subgroup", "outside_subgroup_neg", "x_without_root"):
            assert by[name]["status"] == C.BAD
    # the points outside the subgroups are on their curves: only rule 6 rejects
    off1, off2 = B.g1_curve_point(0x5EED), B.g2_curve_point(0x5EED)
    assert C.compress_g1(off1).hex() in (GOLD["g1"][i]["c"] for i in range(len(GOLD["g1"])))
    assert C.compress_g2(off2).hex() in (GOLD["g2"][i]["c"] for i in range(len(GOLD["g2"])))
    c0 = next(c for c in GOLD["g2"] if c["name"] == "g2_x_c0_is_p")
    raw = bytes.fromhex(c0["c"])
    assert int.from_bytes(raw[48:], "big") == B.P
    assert int.from_bytes(bytes([raw[0] & 0x1F]) + raw[1:48], "big") < B.P


def test_restatement_inverts_the_combine_fixtures():
    """Every g48 of combine_vectors.json and every sig96 of sign_vectors.json
    decodes to the g96 / sig192 stored beside it."""
    comb, sign = _gold("combine_vectors.json"), _gold("sign_vectors.json")
    g1 = comb["groups"] + comb["scalar_cases"]["cases"] + comb["epoch"]["ciphertexts"]
    g2 = sign["groups"] + sign["scalar_cases"]["cases"] + sign["epoch"]["documents"]
    assert len(g1) >= 16 and len(g2) >= 16
    seen = 0
    for r in g1:
        st = r.get("status", 0)   # the epoch's ciphertexts store finite results only
        if st in (0, 1):
            assert C.decompress_g1(bytes.fromhex(r["g48"])) == (st, bytes.fromhex(r["g96"]))
            seen += 1
    for r in g2:
        if r["status"] in (0, 1):
            assert C.decompress_g2(bytes.fromhex(r["sig96"])) == (r["status"],
                                                                  bytes.fromhex(r["sig192"]))
            seen += 1
    assert seen >= 30


def test_compress_inverts_parse():
    """The helper's compress is the inverse of its decompress on the epochs'
    points, the ones outside the subgroups aside (those do not decode)."""
    sign = _gold("sign_vectors.json")
    for doc in sign["epoch"]["documents"]:
        for s in doc["shares"]:
            u2, u1 = bytes.fromhex(s["share"]), bytes.fromhex(s["pk"])
            st2, d2 = C.decompress_g2(C.compress_g2(C.parse_g2(u2)))
            st1, d1 = C.decompress_g1(C.compress_g1(C.parse_g1(u1)))
            assert (st2 == C.BAD) == (not B.g2_in_subgroup(C.parse_g2(u2)))
            assert (st1 == C.BAD) == (not B.g1_in_subgroup(C.parse_g1(u1)))
            assert st2 == C.BAD or d2 == u2
            assert st1 == C.BAD or d1 == u1


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
    rs = open(os.path.join(ROOT, "hbbft-hip", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert "pub fn %s(" % s in rs, s


def test_entries_check_their_arguments(built):
    import hbbft_amd as hb
    L = hb.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    # count == 0 is ok whatever the pointers; a null pointer is 100
    assert L.hbrbc_g1_prepare_compressed(None, 0, None, None) == 0
    assert L.hbrbc_g2_points_prepare_compressed(None, 0, None, None) == 0
    assert L.hbrbc_g1_decompress(None, 0, None, None, None) == 0
    assert L.hbrbc_g2_decompress(None, 0, None, None, None) == 0
    assert L.hbrbc_g1_prepare_compressed(None, 1, p, None) == 100
    assert L.hbrbc_g1_prepare_compressed(p, 1, None, None) == 100
    assert L.hbrbc_g2_points_prepare_compressed(None, 1, p, None) == 100
    assert L.hbrbc_g2_points_prepare_compressed(p, 1, None, None) == 100
    for fn in (L.hbrbc_g1_decompress, L.hbrbc_g2_decompress):
        assert fn(None, 1, p, p, None) == 100
        assert fn(p, 1, None, p, None) == 100
        assert fn(p, 1, p, None, None) == 100


def test_no_cpu_fallback_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    L = hb.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert L.hbrbc_g1_prepare_compressed(p, 1, p, None) == 102   # HBRBC_E_NO_DEVICE
    assert L.hbrbc_g2_points_prepare_compressed(p, 1, p, None) == 102
    assert L.hbrbc_g1_decompress(p, 1, p, p, None) == 102
    assert L.hbrbc_g2_decompress(p, 1, p, p, None) == 102
    sign = _gold("sign_vectors.json")["epoch"]
    doc = sign["documents"][0]
    s0 = doc["shares"][0]
    share = C.compress_g2(C.parse_g2(bytes.fromhex(s0["share"])))
    pk = C.compress_g1(C.parse_g1(bytes.fromhex(s0["pk"])))
    pub = C.compress_g1(C.parse_g1(bytes.fromhex(sign["public_key"])))
    with pytest.raises(hb.HbrbcUnavailable):
        T.threshold_sign_grouped_wire([bytes.fromhex(doc["hash"])],
                                      [(0, s0["node"], share, pk)], sign["t"], pub)
    comb = _gold("combine_vectors.json")["epoch"]
    ct = comb["ciphertexts"][0]
    c0 = ct["shares"][0]
    with pytest.raises(hb.HbrbcUnavailable):
        T.decrypt_shares_grouped_wire(
            [(bytes.fromhex(ct["hash"]), C.compress_g2(C.parse_g2(bytes.fromhex(ct["w"]))))],
            [(0, c0["node"], C.compress_g1(C.parse_g1(bytes.fromhex(c0["share"]))),
              C.compress_g1(C.parse_g1(bytes.fromhex(c0["pk"]))))], comb["t"])
    # a wrong length is the caller's error before any device is looked for
    with pytest.raises(ValueError):
        T.threshold_sign_grouped_wire([bytes.fromhex(doc["hash"])],
                                      [(0, s0["node"], share, pk)], sign["t"],
                                      bytes.fromhex(sign["public_key"]))
