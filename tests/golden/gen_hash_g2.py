"""Writes tests/golden/hash_g2_vectors.json: the vectors of hash_g2,
hash_g1_g2, xor_with_hash and encrypt, computed by tests/hash_ref.py (the
definition), with the ChaCha20 anchor taken from `openssl enc -chacha20`.

    python tests/golden/gen_hash_g2.py          (from the repository root)

The cofactor multiplication costs about 0.3 s per point in Python, so the file
holds about 100 hashes.  Data only.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import bls_oracle as B          # noqa: E402
from tests import compressed_ref as C       # noqa: E402
from tests import hash_ref as H             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "hash_g2_vectors.json")
KEYS = [bytes(range(32)), H.sha3(b"hash_g2 chacha anchor")]
TOTAL_HASHES = 96


def openssl_words(key, blocks):
    """Keystream words of blocks 0 .. blocks-1: openssl's 16-byte IV is the
    32-bit counter (little-endian) and a 96-bit nonce, all zero here, which is
    the 64-bit counter from 0 with zero words 14, 15 for these few blocks."""
    out = subprocess.run(["openssl", "enc", "-chacha20", "-K", key.hex(), "-iv", "00" * 16],
                         input=bytes(64 * blocks), capture_output=True, check=True).stdout
    assert len(out) == 64 * blocks
    return [int.from_bytes(out[4 * i:4 * i + 4], "little") for i in range(16 * blocks)]


def classes(msg, words, tr):
    """The crafted classes an item belongs to, from its trace."""
    c = []
    if words == 25:
        c.append("first_attempt")
    if tr["rej_c0"] and not tr["rej_c1"]:
        c.append("rej_c0_only")
    if tr["rej_c1"] and not tr["rej_c0"]:
        c.append("rej_c1_only")
    if tr["nonsquare"] >= 3:
        c.append("nonsquare_3")
    if words > 64:
        c.append("words_gt_64")
    c.append("greatest_%d_ylt_%d" % (tr["greatest"], int(tr["y_lt_neg"])))
    return c


WANTED = ["first_attempt", "rej_c0_only", "rej_c1_only", "nonsquare_3", "words_gt_64",
          "greatest_0_ylt_0", "greatest_0_ylt_1", "greatest_1_ylt_0", "greatest_1_ylt_1"]
LENGTHS = [0, 1, 135, 136, 137, 300]


def fq2_hex(a):
    return ["%096x" % a[0], "%096x" % a[1]]


def hash_item(msg, u48=None):
    data = msg if u48 is None else H.hash_g1_g2_input(u48, msg)
    q, pt, words, tr = H.hash_g2(data)
    assert q is not None
    item = {"msg": msg.hex(), "x": fq2_hex(pt[0]), "y": fq2_hex(pt[1]),
            "g192": B.g2_bytes(q).hex(), "g96": C.compress_g2(q).hex(), "words": words,
            "trace": tr, "classes": classes(msg, words, tr)}
    if u48 is not None:
        item["u48"] = u48.hex()
    return item


def main():
    assert H.cofactor_from_x() == H.H2
    chacha = []
    for key in KEYS:
        words = openssl_words(key, 3)
        assert words == [w for b in range(3) for w in H.chacha_block(key, b)]
        chacha.append({"key": key.hex(), "words": words})

    # messages of the stated lengths, then a search for every crafted class
    # (the sampler alone is cheap), then filler up to TOTAL_HASHES
    msgs = [bytes((7 * i + n) & 0xFF for i in range(n)) for n in LENGTHS]
    have = set()
    for m in msgs:
        _, w, tr = H.sample(H.sha3(m))
        have.update(classes(m, w, tr))
    i = 0
    per_class = {c: 0 for c in WANTED}
    while len(msgs) < TOTAL_HASHES:
        m = b"hash_g2 vector %d" % i
        i += 1
        _, w, tr = H.sample(H.sha3(m))
        cs = classes(m, w, tr)
        rare = [c for c in cs if c in per_class and per_class[c] < 2 and c != "first_attempt"]
        missing = [c for c in WANTED if per_class[c] == 0]
        if rare or not missing or i > 4000:
            msgs.append(m)
            for c in cs:
                if c in per_class:
                    per_class[c] += 1
    assert all(per_class[c] for c in WANTED), per_class
    hashes = [hash_item(m) for m in msgs]

    u = C.compress_g1(B.g1_mul(B.G1_GEN, 0x1234567 + (1 << 200)))
    g1g2 = [hash_item(bytes((3 * i + n) & 0xFF for i in range(n)), u) for n in (0, 64, 65, 200)]

    g = C.compress_g1(B.g1_mul(B.G1_GEN, 77))
    pad = []
    for k, n in enumerate([0, 1, 15, 16, 17, 63, 64, 65, 4099]):
        data = bytes((11 * i + k) & 0xFF for i in range(n))
        pad.append({"g48": g.hex(), "data": data.hex(), "out": H.xor_with_hash(g, data).hex()})

    # encrypt under the master key of the default SyncKeyGen run over the
    # polynomials of keygen_vectors.json (every part complete: the master
    # secret is the sum of the constant terms)
    keygen = json.load(open(os.path.join(ROOT, "tests", "golden", "keygen_vectors.json")))
    enc = []
    for tr in keygen["transcripts"]:
        n, t = len(tr["polys"]), tr["t"]
        master = sum(int(f[0], 16) for f in tr["polys"]) % B.R
        pk = B.g1_mul(B.G1_GEN, master)
        rows = []
        for k, ln in enumerate([0, 5, 33, 100]):
            msg = bytes((13 * i + k + n) & 0xFF for i in range(ln))
            r = int.from_bytes(H.sha3(b"encrypt r %d %d" % (n, k)), "big") % (B.R - 1) + 1
            u48, v, w96 = H.encrypt(pk, msg, r)
            rows.append({"msg": msg.hex(), "r": "%064x" % r, "u48": u48.hex(), "v": v.hex(),
                         "w96": w96.hex()})
        enc.append({"n": n, "t": t, "pk48": C.compress_g1(pk).hex(), "rows": rows})

    doc = {"source": "tests/golden/gen_hash_g2.py over tests/hash_ref.py; parity with "
                     "threshold_crypto is not pinned (DESIGN.md §2)",
           "h2": "%x" % H.H2, "chacha": chacha, "hash_g2": hashes, "hash_g1_g2": g1g2,
           "pad": pad, "encrypt": enc}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d hashes, %d bytes" % (OUT, len(hashes), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
