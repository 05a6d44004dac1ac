"""CPU-side checks of hash_g2, hash_g1_g2 and xor_with_hash: the definition in
tests/hash_ref.py is anchored where it can be (the ChaCha20 block function
against the words `openssl enc -chacha20` gave, the cofactor against the BLS
parameter), tests/golden/hash_g2_vectors.json still holds every crafted class
and agrees with a recomputation, its points lie in G2, the pad is an
involution, and the C ABI, the library, the Python module and the Rust
declarations carry the entries, which check their arguments and fail loudly
without a GPU."""
import ctypes
import json
import os
import re

import pytest

import __graft_entry__
from oracle import bls_oracle as B
from tests import compressed_ref as C
from tests import hash_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "hash_g2_vectors.json")))
SYMBOLS = ["hbrbc_hash_g2_batch", "hbrbc_hash_g1_g2_batch", "hbrbc_xor_with_hash_batch",
           "hbrbc_xor_with_hash_workspace_size"]
NAMES = ["hash_g2", "hash_g1_g2", "xor_with_hash", "hash_g2_batch", "xor_with_hash_batch",
         "encrypt_batch", "decrypt_ciphertexts_grouped"]
CLASSES = ["first_attempt", "rej_c0_only", "rej_c1_only", "nonsquare_3", "words_gt_64",
           "greatest_0_ylt_0", "greatest_0_ylt_1", "greatest_1_ylt_0", "greatest_1_ylt_1"]


@pytest.fixture(scope="module")
def built():
    __graft_entry__.build()


def test_chacha_block_equals_the_openssl_words():
    assert len(GOLD["chacha"]) == 2
    for row in GOLD["chacha"]:
        key = bytes.fromhex(row["key"])
        assert len(row["words"]) == 48
        assert [w for b in range(3) for w in H.chacha_block(key, b)] == row["words"]
        st = H.Stream(key)
        assert [st.u32() for _ in range(48)] == row["words"]
        # a u64 across the block boundary: words 15 and 16, low word first
        st = H.Stream(key)
        for _ in range(15):
            st.u32()
        assert st.u64() == row["words"][15] | (row["words"][16] << 32) and st.words == 17


def test_cofactor_is_the_curve_parameter_polynomial():
    assert H.cofactor_from_x() == H.H2 == int(GOLD["h2"], 16)
    assert H.H2.bit_length() == 507 and H.H2 % 2 == 1 and H.H2 % B.R != H.H2
    consts = open(os.path.join(ROOT, "hbbft_amd", "csrc", "bls_consts.hpp")).read()
    words = re.search(r"kH2\[16\] = \{(.*?)\}", consts).group(1).split(",")
    assert sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(words)) == H.H2
    k = re.search(r"kRand384\[12\] = \{(.*?)\}", consts).group(1).split(",")
    assert sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(k)) == \
        pow(2, 428, B.P)


def test_fq_draw_is_v_times_2_to_minus_384():
    st = H.Stream(bytes(32))
    words = [w for b in range(4) for w in H.chacha_block(bytes(32), b)]
    pos, rej = 0, 0
    while True:
        v = sum(w << (32 * i) for i, w in enumerate(words[pos:pos + 12])) & ((1 << 381) - 1)
        pos += 12
        if v < B.P:
            break
        rej += 1
    got, r = H.fq_draw(st)
    assert (got * (1 << 384) - v) % B.P == 0 and r == rej and st.words == pos


def test_every_crafted_class_is_in_the_fixture():
    items = GOLD["hash_g2"]
    assert 90 <= len(items) <= 110
    for c in CLASSES:
        assert any(c in it["classes"] for it in items), c
    by_len = {len(it["msg"]) // 2 for it in items}
    assert {0, 1, 135, 136, 137, 300} <= by_len
    assert [len(it["msg"]) // 2 for it in GOLD["hash_g1_g2"]] == [0, 64, 65, 200]
    # the classes are what the traces say
    for it in items:
        tr, w = it["trace"], it["words"]
        assert ("first_attempt" in it["classes"]) == (w == 25)
        assert ("nonsquare_3" in it["classes"]) == (tr["nonsquare"] >= 3)
        assert ("words_gt_64" in it["classes"]) == (w > 64)
        assert ("rej_c0_only" in it["classes"]) == (tr["rej_c0"] > 0 and tr["rej_c1"] == 0)
        assert ("rej_c1_only" in it["classes"]) == (tr["rej_c1"] > 0 and tr["rej_c0"] == 0)
        assert w == 25 * (tr["nonsquare"] + 1) + 12 * (tr["rej_c0"] + tr["rej_c1"])
    # after three non-squares without a rejection the fourth attempt starts at
    # word 75, an odd word: its u64 draws then straddle block boundaries
    assert any(it["trace"]["nonsquare"] >= 3 for it in items)


def test_sampler_recomputed_for_every_fixture_item():
    """The attempt loop alone is cheap: x, y, the word count and the trace of
    every item, hash_g1_g2 rows included, recomputed from the message."""
    for it in GOLD["hash_g2"] + GOLD["hash_g1_g2"]:
        msg = bytes.fromhex(it["msg"])
        if "u48" in it:
            msg = H.hash_g1_g2_input(bytes.fromhex(it["u48"]), msg)
        (x, y), words, tr = H.sample(H.sha3(msg))
        assert ["%096x" % v for v in x] == it["x"] and ["%096x" % v for v in y] == it["y"]
        assert words == it["words"] and tr == it["trace"]
        assert B.g2_on_curve((x, y))
        assert C._larger_fp2(y) == bool(tr["greatest"])
    long = GOLD["hash_g1_g2"][2]
    assert H.hash_g1_g2_input(bytes(48), bytes.fromhex(long["msg"]))[:32] == \
        H.sha3(bytes.fromhex(long["msg"]))


def test_eight_fixture_points_recomputed_and_in_g2():
    items = GOLD["hash_g2"]
    for it in items[:6] + items[-1:] + GOLD["hash_g1_g2"][2:3]:
        x = tuple(int(v, 16) for v in it["x"])
        y = tuple(int(v, 16) for v in it["y"])
        q = H.cofactor_mul((x, y))
        assert q is not None and B.g2_on_curve(q)
        assert B.g2_bytes(q).hex() == it["g192"] and C.compress_g2(q).hex() == it["g96"]
        assert B._smul(B.g2_add, q, B.R) is None
        # reducing the cofactor mod r first gives another point: (x, y) is not in G2
        assert B.g2_mul((x, y), H.H2) != q


def test_pad_vectors_and_involution():
    for row in GOLD["pad"]:
        g, data = bytes.fromhex(row["g48"]), bytes.fromhex(row["data"])
        out = H.xor_with_hash(g, data)
        assert out.hex() == row["out"]
        assert H.xor_with_hash(g, out) == data
        seed = H.sha3(g)
        assert out[:16] == bytes(d ^ (w & 0xFF) for d, w in zip(data, H.chacha_block(seed, 0)))
    assert [len(r["data"]) // 2 for r in GOLD["pad"]] == [0, 1, 15, 16, 17, 63, 64, 65, 4099]


def test_encrypt_vectors_verify_as_ciphertexts():
    """One row per key set recomputed; its W satisfies Ciphertext::verify's
    equation in the exponent: W = [r] H."""
    assert [(e["n"], e["t"]) for e in GOLD["encrypt"]] == [(4, 1), (7, 2)]
    for e in GOLD["encrypt"]:
        row = e["rows"][1]
        pk = C.parse_g1(C.decompress_g1(bytes.fromhex(e["pk48"]))[1])
        u, v, w = H.encrypt(pk, bytes.fromhex(row["msg"]), int(row["r"], 16))
        assert (u.hex(), v.hex(), w.hex()) == (row["u48"], row["v"], row["w96"])
        assert len(v) == len(row["msg"]) // 2


def test_names_symbols_and_ffi(built):
    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    L = ctypes.CDLL(hb.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "hbrbc.h")).read()
    rs = open(os.path.join(ROOT, "hbbft-hip", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and re.search(r"\b%s\s*\(" % s, hdr) and "pub fn %s(" % s in rs, s
    for n in NAMES:
        assert callable(getattr(T, n)), n
    assert "hash_g2.hip" in open(os.path.join(ROOT, "hbbft_amd", "csrc", "Makefile")).read()
    from hbbft_amd.srchash import source_files
    assert "hbbft_amd/csrc/hash_g2.hip" in source_files()
    assert hb.lib().hbrbc_xor_with_hash_workspace_size(9) >= 9 * 32


def test_entries_check_their_arguments(built):
    import hbbft_amd as hb
    L = hb.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    # count = 0 returns without a launch, whatever the pointers
    assert L.hbrbc_hash_g2_batch(None, None, 0, 0, None, None, None, None, None, None) == 0
    assert L.hbrbc_hash_g1_g2_batch(None, None, None, 0, 0, None, None, None, None, None,
                                    None) == 0
    assert L.hbrbc_xor_with_hash_batch(None, None, None, 0, 0, None, None, None, None) == 0
    # a null required pointer is 100; the encodings and words_out may be null,
    # and so may the messages when there are no bytes
    full = [p, p, 1, 8, p, None, None, p, None, None]
    for k in (0, 1, 4, 7):
        args = list(full)
        args[k] = None
        assert L.hbrbc_hash_g2_batch(*args) == 100, k
    full = [p, p, p, 1, 8, p, None, None, p, None, None]
    for k in (0, 1, 2, 5, 8):
        args = list(full)
        args[k] = None
        assert L.hbrbc_hash_g1_g2_batch(*args) == 100, k
    full = [p, p, p, 1, 8, p, p, p, None]
    for k in (0, 1, 2, 5, 6, 7):
        args = list(full)
        args[k] = None
        assert L.hbrbc_xor_with_hash_batch(*args) == 100, k
    assert b"null" in L.hbrbc_last_error()
    assert L.hbrbc_hash_g2_batch(p, p, 1, 1 << 32, p, None, None, p, None, None) == 100


def test_no_cpu_fallback_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        return   # the GPU tests cover the entries there
    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    L = hb.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert L.hbrbc_hash_g2_batch(p, p, 1, 8, p, None, None, p, None, None) == 102
    assert L.hbrbc_hash_g1_g2_batch(p, p, p, 1, 8, p, None, None, p, None, None) == 102
    assert L.hbrbc_xor_with_hash_batch(p, p, p, 1, 8, p, p, p, None) == 102
    for call in (lambda: T.hash_g2([b"doc"]), lambda: T.hash_g1_g2([bytes(48)], [b"v"]),
                 lambda: T.xor_with_hash([bytes(48)], [b"data"]),
                 lambda: T.encrypt_batch(bytes(48), [b"m"], [bytes(31) + b"\x01"]),
                 lambda: T.decrypt_ciphertexts_grouped([(bytes(48), b"v", bytes(96))], [], 1)):
        with pytest.raises(hb.HbrbcUnavailable):
            call()
    # malformed input is rejected before any device is looked for
    with pytest.raises(ValueError):
        T.hash_g1_g2([bytes(47)], [b"v"])
    with pytest.raises(ValueError):
        T.encrypt_batch(bytes(48), [b"m"], [bytes(31)])
    with pytest.raises(ValueError):
        T.xor_with_hash([bytes(48)], [])
    assert T.hash_g2([]) == [] and T.xor_with_hash([], []) == []
