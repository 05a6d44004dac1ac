"""CPU-side checks of share creation and the dealer's side of key generation:
tests/golden/dealer_vectors.json agrees with a recomputation in Python
integers (and, for one secret key share, with the fixture's public key share
through oracle/bls_oracle.py); the C ABI, the built library, the Python
modules and the Rust declarations carry the five entries; the entries check
their arguments; without a GPU every call fails loudly; the wrappers reject
malformed tensors before they look for a device."""
import ctypes
import json
import os
import re

import pytest

import __graft_entry__
from oracle import bls_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


DEALER, KEYGEN = _gold("dealer_vectors.json"), _gold("keygen_vectors.json")
R = B.R
SYMBOLS = ["hbrbc_g1_base_mul", "hbrbc_g1_mul_prepared", "hbrbc_g2_mul_prepared",
           "hbrbc_fr_poly_eval", "hbrbc_fr_dot"]
KEYGEN_NAMES = ["base_mul", "fr_poly_eval", "fr_dot", "generate_part", "ack_values",
                "secret_key_share", "sync_key_gen_network"]
THRESHOLD_NAMES = ["g1_mul_prepared", "g2_mul_prepared", "create_decryption_shares",
                   "create_signature_shares", "share_row"]


@pytest.fixture(scope="module")
def built():
    __graft_entry__.build()


def _eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def test_poly_eval_cases_follow_from_the_table():
    pe = DEALER["poly_eval"]
    table = [int(v, 16) for v in pe["table"]]
    assert table[-1] == R and table[-2] == R - 1 and table[-3] == 0
    names = {e["name"] for e in pe["evals"]}
    for deg in ("degree0", "degree1", "degree21"):
        for x in (0, 1, 2, 64, 0xFFFFFFFF):
            assert "%s_at_%d" % (deg, x) in names
    assert {"empty_at_0", "coefficient_is_r_at_2", "row_negative_at_1", "row_past_the_end_at_64",
            "poly_-1", "poly_%d" % len(pe["polys"])} <= names
    assert [len(p["rows"]) for p in pe["polys"]][:4] == [1, 2, 22, 0]
    for e in pe["evals"]:
        p = e["poly"]
        if not 0 <= p < len(pe["polys"]):
            assert e["status"] == 2 and int(e["value"], 16) == 0
            continue
        rows = pe["polys"][p]["rows"]
        ok = all(0 <= r < len(table) and table[r] < R for r in rows)
        assert e["status"] == (0 if ok else 2), e["name"]
        want = _eval([table[r] for r in rows], e["x"]) if ok else 0
        assert int(e["value"], 16) == want, e["name"]
        if ok and e["x"] == 0:
            assert want == (table[rows[0]] if rows else 0)


def test_dot_cases_follow_from_their_operands():
    groups = DEALER["dot"]
    assert [len(g["a"]) for g in groups][:4] == [0, 1, 22, 65]
    assert sum(g["status"] == 2 for g in groups) == 1
    for g in groups:
        a, b = [int(v, 16) for v in g["a"]], [int(v, 16) for v in g["b"]]
        ok = all(v < R for v in a + b)
        assert g["status"] == (0 if ok else 2), g["name"]
        assert int(g["value"], 16) == (sum(x * y for x, y in zip(a, b)) % R if ok else 0)
        if not ok:
            assert R in a + b


def test_secret_key_shares_are_the_master_polynomial_at_the_nodes():
    from hbbft_amd.keygen import coeff_pos as pos
    for k, (tr, d) in enumerate(zip(KEYGEN["transcripts"], DEALER["transcripts"])):
        n, t = tr["n"], tr["t"]
        assert (d["n"], d["t"], d["complete"]) == (n, t, tr["complete"])
        polys = [[int(c, 16) for c in f] for f in tr["polys"]]
        master = [sum(polys[p][pos(0, j)] for p in tr["complete"]) % R for j in range(t + 1)]
        assert [int(c, 16) for c in d["master"]] == master
        for i in range(n):
            assert int(d["secret_key_shares"][i], 16) == _eval(master, i + 1)
        # an incomplete part changes every share: leaving it out is visible
        if len(tr["complete"]) < n:
            full = [sum(f[pos(0, j)] for f in polys) % R for j in range(t + 1)]
            assert all(_eval(full, i + 1) != _eval(master, i + 1) for i in range(n))
    assert DEALER["transcripts"][1]["complete"] == [0, 1, 2, 3, 4, 5]
    # one share against the fixture's public key share, by the oracle
    tr, d = KEYGEN["transcripts"][0], DEALER["transcripts"][0]
    pk = B.g1_mul(B.G1_GEN, int(d["secret_key_shares"][2], 16))
    assert B.g1_bytes(pk).hex() == tr["key_shares"][2]["g96"]


def test_header_declares_and_library_exports_the_entries(built):
    import hbbft_amd as hb
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    src = open(os.path.join(ROOT, "include", "hbrbc.h")).read()
    assert "constant-time" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(hbrbc_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(hb.LIB_PATH)
    rs = open(os.path.join(ROOT, "hbbft-hip", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert hasattr(hb.lib(), s), s
        assert "pub fn %s(" % s in rs, s
    for name in KEYGEN_NAMES:
        assert callable(getattr(K, name)), name
    for name in THRESHOLD_NAMES:
        assert callable(getattr(T, name)), name
    assert [T.share_row(i, c, 3) for i in range(2) for c in range(3)] == list(range(6))


def _null_each(fn, full, required):
    for k in required:
        args = list(full)
        args[k] = None
        assert fn(*args) == 100, (fn.__name__, k)


def test_entries_check_their_arguments(built):
    import hbbft_amd as hb
    L = hb.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    # zero counts are ok whatever the pointers
    assert L.hbrbc_g1_base_mul(None, 0, None, None, None, None, None) == 0
    assert L.hbrbc_g1_mul_prepared(None, 0, None, None, 0, None, 0, None, None, None, None,
                                   None) == 0
    assert L.hbrbc_g2_mul_prepared(None, 0, None, None, 0, None, 0, None, None, None, None,
                                   None) == 0
    assert L.hbrbc_fr_poly_eval(None, 0, None, None, 0, None, None, 0, None, None, None) == 0
    assert L.hbrbc_fr_dot(None, None, None, 0, 0, None, None, None) == 0
    # a null required pointer is 100; the encodings and sidx may be null
    _null_each(L.hbrbc_g1_base_mul, [p, 1, p, None, None, p, None], (0, 2, 5))
    for fn in (L.hbrbc_g1_mul_prepared, L.hbrbc_g2_mul_prepared):
        _null_each(fn, [p, 1, p, p, 1, None, 1, p, None, None, p, None], (0, 2, 3, 7, 10))
        # without sidx every result needs a scalar of its own
        assert fn(p, 1, p, p, 1, None, 2, p, None, None, p, None) == 100
    _null_each(L.hbrbc_fr_poly_eval, [p, 1, p, p, 1, p, p, 1, p, p, None], (0, 2, 3, 5, 6, 8, 9))
    _null_each(L.hbrbc_fr_dot, [p, p, p, 1, 1, p, p, None], (0, 1, 2, 5, 6))
    assert b"null" in L.hbrbc_last_error()


def test_no_cpu_fallback_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import hbbft_amd as hb
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    L = hb.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert L.hbrbc_g1_base_mul(p, 1, p, None, None, p, None) == 102   # HBRBC_E_NO_DEVICE
    assert L.hbrbc_g1_mul_prepared(p, 1, p, p, 1, None, 1, p, None, None, p, None) == 102
    assert L.hbrbc_g2_mul_prepared(p, 1, p, p, 1, p, 1, p, p, p, p, None) == 102
    assert L.hbrbc_fr_poly_eval(p, 1, p, p, 1, p, p, 1, p, p, None) == 102
    assert L.hbrbc_fr_dot(p, p, p, 1, 1, p, p, None) == 102
    tr = KEYGEN["transcripts"][0]
    polys = [[bytes.fromhex(c) for c in f] for f in tr["polys"]]
    sc = torch.zeros((1, 32), dtype=torch.uint8)
    i32 = torch.zeros(1, dtype=torch.int32)
    offs = torch.tensor([0, 1], dtype=torch.int32)
    g1 = torch.zeros(L.hbrbc_g1_prepared_size(1), dtype=torch.uint8)
    g2 = torch.zeros(L.hbrbc_g2_points_size(1), dtype=torch.uint8)
    calls = [lambda: K.base_mul(sc),
             lambda: K.fr_poly_eval(sc, i32, offs, i32, i32),
             lambda: K.fr_dot(sc, sc, offs),
             lambda: T.g1_mul_prepared(g1, 1, i32, sc),
             lambda: T.g2_mul_prepared(g2, 1, i32, sc, i32),
             lambda: K.generate_part(tr["t"], polys[0], tr["n"]),
             lambda: K.ack_values([bytes.fromhex(c) for c in tr["rows"][0][0]], tr["n"]),
             lambda: K.secret_key_share(tr["t"], [[(0, bytes.fromhex(tr["values"][0][0][0]))]]),
             lambda: K.sync_key_gen_network(tr["t"], polys),
             lambda: T.create_decryption_shares([b"\0" * 32], [b"\xc0" + b"\0" * 47]),
             lambda: T.create_signature_shares([b"\0" * 32], [b"\x40" + b"\0" * 191])]
    for k, call in enumerate(calls):
        with pytest.raises(hb.HbrbcUnavailable):
            call()
            pytest.fail("call %d returned" % k)


def test_wrappers_reject_malformed_input_before_any_device(built):
    import torch
    import hbbft_amd as hb
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    L = hb.lib()
    sc = torch.zeros((2, 32), dtype=torch.uint8)
    i32 = torch.zeros(2, dtype=torch.int32)
    offs = torch.tensor([0, 2], dtype=torch.int32)
    g1 = torch.zeros(L.hbrbc_g1_prepared_size(1), dtype=torch.uint8)
    g2 = torch.zeros(L.hbrbc_g2_points_size(1), dtype=torch.uint8)
    bad = [lambda: K.base_mul(torch.zeros((2, 31), dtype=torch.uint8)),
           lambda: K.base_mul(sc.to(torch.int32)),
           lambda: K.fr_poly_eval(sc, i32.long(), offs, i32, i32),
           lambda: K.fr_poly_eval(sc, i32, torch.tensor([0, 3], dtype=torch.int32), i32, i32),
           lambda: K.fr_poly_eval(sc, i32, offs, i32, i32[:1]),
           lambda: K.fr_dot(sc, sc[:1], offs),
           lambda: K.fr_dot(sc, sc, torch.tensor([0, 1], dtype=torch.int32)),
           lambda: T.g1_mul_prepared(g1[:-1], 1, i32, sc),
           lambda: T.g1_mul_prepared(g1, 1, i32, sc[:1]),          # no sidx: a scalar per lane
           lambda: T.g1_mul_prepared(g1, 1, i32, sc, i32[:1]),
           lambda: T.g2_mul_prepared(g2, 2, i32, sc),              # the table's own count
           lambda: T.g2_mul_prepared(g2, 1, i32, sc, i32.long())]
    for k, call in enumerate(bad):
        with pytest.raises(AssertionError):
            call()
            pytest.fail("call %d returned" % k)
    tr = KEYGEN["transcripts"][0]
    polys = [[bytes.fromhex(c) for c in f] for f in tr["polys"]]
    with pytest.raises(ValueError):
        K.generate_part(tr["t"], polys[0][:-1], 4)
    with pytest.raises(ValueError):
        K.generate_part(tr["t"], polys[0], 0)
    with pytest.raises(ValueError):
        K.ack_values([], 4)
    with pytest.raises(ValueError):
        K.sync_key_gen_network(tr["t"], [f[:-1] for f in polys])
    with pytest.raises(ValueError):
        K.sync_key_gen_network(tr["t"], polys, ack_senders=[[0, 4]] * 4)
    with pytest.raises(ValueError):
        T.create_decryption_shares([b"\0" * 31], [b"\xc0" + b"\0" * 47])
    with pytest.raises(ValueError):
        T.create_decryption_shares([b"\0" * 32], [b"\x40" + b"\0" * 95])   # U arrives compressed
    with pytest.raises(ValueError):
        T.create_signature_shares([b"\0" * 32], [b"\xc0" + b"\0" * 95])    # H arrives uncompressed
    with pytest.raises(ValueError):
        T.create_signature_shares([], [])
