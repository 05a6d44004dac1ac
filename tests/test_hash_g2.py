"""GPU parity of hash_g2, hash_g1_g2 and xor_with_hash against
tests/golden/hash_g2_vectors.json (computed by tests/hash_ref.py, the
definition): encodings, status and the stream words drawn -- which prove the
device took the same rejections as the reference -- for every fixture item in
one launch, through the point table, and in launches of 1, 63, 64, 65 and 4,097
items cycled from the fixture; the pad at every lane-edge length, ragged, one
row per launch, twice, and into a poisoned buffer; encrypt and decrypt end to
end at N = 4 and N = 7 with keys from sync_key_gen_network.  Expectations are
fixture bytes, indexed, never recomputed here."""
import json
import os

import numpy as np
import pytest

from hbbft_amd import keygen as K
from hbbft_amd import threshold as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


GOLD, KEYGEN = _gold("hash_g2_vectors.json"), _gold("keygen_vectors.json")
ITEMS = GOLD["hash_g2"]
MSGS = [bytes.fromhex(it["msg"]) for it in ITEMS]
PAD_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 4099]

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def _rows(hexes):
    return np.stack([np.frombuffer(bytes.fromhex(h), np.uint8) for h in hexes])


@pytest.fixture(scope="module")
def expected():
    """Fixture bytes as arrays, built once and shared (read-only)."""
    e = {"g192": _rows([it["g192"] for it in ITEMS]), "g96": _rows([it["g96"] for it in ITEMS]),
         "words": np.asarray([it["words"] for it in ITEMS], np.int32)}
    for v in e.values():
        v.setflags(write=False)
    return e


def _hash(msgs, us48=None, **kw):
    flat, offs = T._ragged_bytes(msgs, "cuda:0")
    u = _dev(_rows([x.hex() for x in us48])) if us48 is not None else None
    tab, o192, o96, st, wd = T.hash_g2_batch(flat, offs, us48=u, words=True, **kw)
    return (tab,) + tuple(None if t is None else t.cpu().numpy() for t in (o192, o96, st, wd))


def test_whole_fixture_in_one_launch(expected):
    _, o192, o96, st, wd = _hash(MSGS)
    assert st.tolist() == [0] * len(MSGS)
    assert wd.tolist() == expected["words"].tolist()
    assert np.array_equal(o192, expected["g192"]) and np.array_equal(o96, expected["g96"])


def test_point_table_is_what_the_decoder_makes_of_the_bytes(expected):
    """The table entries bit for bit those of g2_points_prepare over the
    expected bytes, and g2_mul_prepared with scalar 1 reads them back."""
    import torch
    n = len(MSGS)
    tab, _, _, _, _ = _hash(MSGS, encode=False)
    want = T.g2_points_prepare(_dev(expected["g192"]))
    # the coordinates, then the status bytes after the padding to 256 (the
    # padding itself is nobody's)
    at = (n * 192 + 255) // 256 * 256
    assert tab.numel() == want.numel() >= at + n
    assert torch.equal(tab[:n * 192], want[:n * 192])
    assert torch.equal(tab[at:at + n], want[at:at + n]) and not want[at:at + n].any()
    one = _dev(np.tile(np.frombuffer((1).to_bytes(32, "big"), np.uint8), (n, 1)))
    _, m192, m96, mst = T.g2_mul_prepared(tab, n, torch.arange(n, dtype=torch.int32,
                                                               device="cuda:0"), one)
    assert mst.cpu().tolist() == [0] * n
    assert np.array_equal(m192.cpu().numpy(), expected["g192"])
    assert np.array_equal(m96.cpu().numpy(), expected["g96"])


@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097])
def test_batches_cycled_from_the_fixture(expected, count):
    idx = np.arange(count) % len(MSGS)
    if count == 1:
        idx = np.asarray([len(MSGS) - 1])
    _, o192, o96, st, wd = _hash([MSGS[i] for i in idx])
    assert not st.any()
    assert np.array_equal(wd, expected["words"][idx])
    assert np.array_equal(o192, expected["g192"][idx]) and np.array_equal(o96, expected["g96"][idx])


def test_hash_g1_g2_rows():
    rows = GOLD["hash_g1_g2"]
    assert [len(r["msg"]) // 2 for r in rows] == [0, 64, 65, 200]
    us = [bytes.fromhex(r["u48"]) for r in rows]
    vs = [bytes.fromhex(r["msg"]) for r in rows]
    _, o192, o96, st, wd = _hash(vs, us48=us)
    assert st.tolist() == [0] * 4 and wd.tolist() == [r["words"] for r in rows]
    assert np.array_equal(o192, _rows([r["g192"] for r in rows]))
    assert np.array_equal(o96, _rows([r["g96"] for r in rows]))
    assert T.hash_g1_g2(us, vs) == [(bytes.fromhex(r["g192"]), bytes.fromhex(r["g96"]))
                                    for r in rows]
    # U is part of the input: another U, another point
    assert T.hash_g1_g2([us[0][:-1] + b"\x01"], vs[:1]) != T.hash_g1_g2(us[:1], vs[:1])
    assert T.hash_g2(MSGS[:2]) == [(bytes.fromhex(it["g192"]), bytes.fromhex(it["g96"]))
                                   for it in ITEMS[:2]]


def test_ranges_are_clamped_and_empty_descriptions_return():
    """A reversed range and one past the buffer are status 2 with zero bytes
    and no words; their neighbours are computed; an empty message is a message;
    count = 0 returns before any launch."""
    import torch
    flat = _dev(np.frombuffer(MSGS[6] + MSGS[7], np.uint8))
    a, total = len(MSGS[6]), len(MSGS[6]) + len(MSGS[7])
    cases = [([0, a, total], [0, 0]), ([a, 0, a], [2, 0]), ([0, a, total + 1], [0, 2]),
             ([0, 0, a], [0, 0])]
    by_msg = {m: i for i, m in enumerate(MSGS)}
    for offs, want in cases:
        tab, o192, o96, st, wd = T.hash_g2_batch(flat, _dev(np.asarray(offs, np.int32)),
                                                 words=True)
        assert st.cpu().tolist() == want, offs
        for i, s in enumerate(want):
            got = bytes(o192[i].cpu().numpy())
            if s == 2:
                assert got == bytes(192) and not o96[i].any() and wd[i].item() == 0
            else:
                m = bytes(flat[offs[i]:offs[i + 1]].cpu().numpy())
                assert got.hex() == ITEMS[by_msg[m]]["g192"] and \
                    wd[i].item() == ITEMS[by_msg[m]]["words"]
    assert b"" in by_msg
    empty = torch.zeros((0,), dtype=torch.uint8, device="cuda:0")
    _, o192, _, st, _ = T.hash_g2_batch(empty, _dev(np.zeros(2, np.int32)))
    assert st.cpu().tolist() == [0] and bytes(o192[0].cpu().numpy()).hex() == \
        ITEMS[by_msg[b""]]["g192"]
    _, o192, _, st, _ = T.hash_g2_batch(empty, _dev(np.zeros(1, np.int32)))
    assert o192.shape == (0, 192) and st.numel() == 0
    assert T.hash_g2([]) == [] and T.xor_with_hash([], []) == []


# ---- the pad ----
def _pad_case():
    rows = GOLD["pad"]
    assert [len(r["data"]) // 2 for r in rows] == PAD_LENGTHS
    return ([bytes.fromhex(r["g48"]) for r in rows], [bytes.fromhex(r["data"]) for r in rows],
            [bytes.fromhex(r["out"]) for r in rows])


def test_pad_ragged_launch_and_twice():
    gs, datas, outs = _pad_case()
    assert T.xor_with_hash(gs, datas) == outs
    assert T.xor_with_hash(gs, outs) == datas
    # in place, on the device tensors
    flat, offs = T._ragged_bytes(datas, "cuda:0")
    g = _dev(_rows([x.hex() for x in gs]))
    out, st = T.xor_with_hash_batch(g, flat, offs, out=flat)
    assert out.data_ptr() == flat.data_ptr() and st.cpu().tolist() == [0] * len(datas)
    assert bytes(flat.cpu().numpy()) == b"".join(outs)


def test_pad_one_row_per_launch_leaves_every_other_byte():
    """Each row alone over a poisoned buffer with bytes before the first row
    and after the last: only the row's own bytes change."""
    import torch
    gs, datas, outs = _pad_case()
    lead, trail = 5, 37
    blob = bytes(lead) + b"".join(datas) + bytes(trail)
    data = _dev(np.frombuffer(blob, np.uint8))
    pos = lead
    for g, d, o in zip(gs, datas, outs):
        out = torch.full_like(data, 0xEE)
        offs = _dev(np.asarray([pos, pos + len(d)], np.int32))
        _, st = T.xor_with_hash_batch(_dev(_rows([g.hex()])), data, offs, out=out)
        got = bytes(out.cpu().numpy())
        assert st.cpu().tolist() == [0]
        assert got == b"\xee" * pos + o + b"\xee" * (len(blob) - pos - len(d)), len(d)
        pos += len(d)
    # all rows in one launch over the same buffer: lead and trail untouched
    out = torch.full_like(data, 0xEE)
    offs = _dev(np.concatenate([[lead], lead + np.cumsum([len(d) for d in datas])]).astype(np.int32))
    _, st = T.xor_with_hash_batch(_dev(_rows([g.hex() for g in gs])), data, offs, out=out)
    assert bytes(out.cpu().numpy()) == b"\xee" * lead + b"".join(outs) + b"\xee" * trail
    # a reversed range and one past the end: status 2, nothing written
    out = torch.full_like(data, 0xEE)
    offs = _dev(np.asarray([16, 0, len(blob) + 1], np.int32))
    _, st = T.xor_with_hash_batch(_dev(_rows([gs[0].hex()] * 2)), data, offs, out=out)
    assert st.cpu().tolist() == [2, 2] and bytes(out.cpu().numpy()) == b"\xee" * len(blob)


# ---- encrypt and decrypt end to end ----
@pytest.mark.parametrize("which", [0, 1])
def test_encrypt_decrypt_end_to_end(which):
    enc = GOLD["encrypt"][which]
    n, t = enc["n"], enc["t"]
    assert (n, t) == ((4, 1), (7, 2))[which]
    tr = [x for x in KEYGEN["transcripts"] if len(x["polys"]) == n][0]
    keys = K.sync_key_gen_network(t, [[bytes.fromhex(c) for c in f] for f in tr["polys"]])
    pk48 = keys["key_set"][0][1]
    assert pk48.hex() == enc["pk48"]
    msgs = [bytes.fromhex(r["msg"]) for r in enc["rows"]]
    cts = T.encrypt_batch(pk48, msgs, [bytes.fromhex(r["r"]) for r in enc["rows"]])
    assert [(u.hex(), v.hex(), w.hex()) for u, v, w in cts] == \
        [(r["u48"], r["v"], r["w96"]) for r in enc["rows"]]

    # Ciphertext::verify with the device's own H
    def verify(cts):
        hs = T.hash_g1_g2([u for u, _, _ in cts], [v for _, v, _ in cts])
        u96, _ = T.g1_decompress(_dev(_rows([u.hex() for u, _, _ in cts])))
        w192, _ = T.g2_decompress(_dev(_rows([w.hex() for _, _, w in cts])))
        return T.verify_ciphertexts([(bytes(a), bytes(b), h[0]) for a, b, h in
                                     zip(u96.cpu().numpy(), w192.cpu().numpy(), hs)])
    assert verify(cts) == [True] * len(cts)

    C = len(cts)
    _, count, _, d48, dst = T.create_decryption_shares(keys["secret_key_shares"],
                                                       [u for u, _, _ in cts])
    assert count == n * C and not dst.cpu().numpy().any()
    d48 = d48.cpu().numpy()
    pks = keys["key_shares"][2].cpu().numpy()

    def shares(nodes):
        return [(c, i, bytes(d48[T.share_row(i, c, C)]), bytes(pks[i]))
                for c in range(C) for i in nodes]
    for nodes in (range(0, t + 1), range(t, 2 * t + 1)):
        flags, plain = T.decrypt_ciphertexts_grouped(cts, shares(nodes), t)
        assert flags == [True] * (C * (t + 1)) and plain == msgs
    # too few shares: the failure, not a plaintext
    flags, plain = T.decrypt_ciphertexts_grouped(cts, shares(range(t)), t)
    assert flags == [True] * (C * t) and plain == [T.FAIL_SHARES] * C

    # one byte of V flipped: H changes, so the ciphertext and its shares fail
    u, v, w = cts[1]
    bad = list(cts)
    bad[1] = (u, bytes([v[0] ^ 1]) + v[1:], w)
    assert verify(bad) == [c != 1 for c in range(C)]
    flags, plain = T.decrypt_ciphertexts_grouped(bad, shares(range(t + 1)), t)
    assert plain == [T.FAIL_CIPHERTEXT if c == 1 else msgs[c] for c in range(C)]
    assert flags == [c != 1 for c in range(C) for _ in range(t + 1)]
