#!/usr/bin/env python3
"""Times the decoding of compressed wire points on the GPU beside the
uncompressed entries it joins.

hbbft's messages carry G1 points in 48 bytes and G2 points in 96; the
uncompressed entries (g1_prepare, g2_points_prepare) take 96 / 192.  The
compressed ones add a square root in Fp (G1) or Fp2 (G2) and a sign choice per
point in front of the same curve and order-r checks.  All in one process,
device events after a warm-up, the median of --steps runs, every table compared
with its twin's before anything is timed:

  (a) g1_prepare_compressed against g1_prepare, --points points;
  (b) g2_points_prepare_compressed against g2_points_prepare;
  (c) g1_decompress and g2_decompress (the square roots, checks and the
      uncompressed bytes);
  (d) threshold_sign_grouped_wire against threshold_sign_grouped on the epoch
      of tests/golden/sign_vectors.json, --epoch-copies copies of its two
      documents in one call (host work included: both functions build their
      index arrays in Python).

The points are valid and finite (an invalid one leaves its lane early): the 22
shares of group `cfg3_a` of combine_vectors.json and the valid shares of the
sign epoch, tiled.  Writes profiles/wire_ingest.json and prints it as one JSON
line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from combine_bench import event_ms, kernel_resources  # noqa: E402

KERNELS = {"g1_prepare": "g1_prepare_kernel", "g1_prepare_compressed": "g1_prepare_compressed_kernel",
           "g2_points": "g2_points_kernel", "g2_points_compressed": "g2_points_compressed_kernel",
           "g1_decompress": "g1_decompress_kernel", "g2_decompress": "g2_decompress_kernel"}


def tiled(torch, np, rows, width, count):
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)
    reps = (count + len(rows) - 1) // len(rows)
    return torch.from_numpy(np.tile(a, (reps, 1))[:count].copy()).cuda()


def same_table(torch, a, b, point_bytes, count):
    """The written parts of two tables agree: the coordinates and, behind them
    at the next multiple of 256, the status bytes (the padding is nobody's)."""
    off = (point_bytes * count + 255) // 256 * 256
    return (a.shape == b.shape and torch.equal(a[:point_bytes * count], b[:point_bytes * count])
            and torch.equal(a[off:off + count], b[off:off + count]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--epoch-copies", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire_ingest.json"),
                    help="result file ('' writes none)")
    a = ap.parse_args()
    import numpy as np
    import torch

    import compressed_ref as C
    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    from oracle import bls_oracle as O
    assert torch.cuda.is_available(), "ingest_bench needs a GPU"
    n = a.points
    res = {"what": "compressed wire points: %d per launch" % n, "points": n, "steps": a.steps,
           "library": hb.lib().hbrbc_version().decode(),
           "kernel_resources": kernel_resources(hb.LIB_PATH, KERNELS)}
    comb = json.load(open(os.path.join(ROOT, "tests", "golden", "combine_vectors.json")))
    sign = json.load(open(os.path.join(ROOT, "tests", "golden", "sign_vectors.json")))
    u1 = [bytes.fromhex(s) for g in comb["groups"] if g["name"] == "cfg3_a" for s in g["shares"]]
    skip = {O.g2_bytes(O.g2_curve_point(0x5EED)), O.g2_bytes(None)}
    u2 = [bytes.fromhex(s["share"]) for d in sign["epoch"]["documents"] for s in d["shares"]]
    u2 = [s for s in u2 if s not in skip]
    c1 = [C.compress_g1(C.parse_g1(u)) for u in u1]
    c2 = [C.compress_g2(C.parse_g2(u)) for u in u2]
    assert {c[0] & 0x20 for c in c1} == {0, 0x20} and {c[0] & 0x20 for c in c2} == {0, 0x20}
    du1, dc1 = tiled(torch, np, u1, 96, n), tiled(torch, np, c1, 48, n)
    du2, dc2 = tiled(torch, np, u2, 192, n), tiled(torch, np, c2, 96, n)

    legs = {"g1_prepare": lambda: T.g1_prepare(du1),
            "g1_prepare_compressed": lambda: T.g1_prepare_compressed(dc1),
            "g2_points_prepare": lambda: T.g2_points_prepare(du2),
            "g2_points_prepare_compressed": lambda: T.g2_points_prepare_compressed(dc2),
            "g1_decompress": lambda: T.g1_decompress(dc1),
            "g2_decompress": lambda: T.g2_decompress(dc2)}
    assert same_table(torch, legs["g1_prepare"](), legs["g1_prepare_compressed"](), 96, n), \
        "G1 tables differ"
    assert same_table(torch, legs["g2_points_prepare"](), legs["g2_points_prepare_compressed"](),
                      192, n), "G2 tables differ"
    o1, s1 = legs["g1_decompress"]()
    o2, s2 = legs["g2_decompress"]()
    assert torch.equal(o1, du1) and torch.equal(o2, du2) and not s1.any() and not s2.any(), \
        "decompressed bytes differ"
    del o1, o2, s1, s2
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {}
    for name, fn in legs.items():
        med, lo, hi = event_ms(torch, fn, a.steps)
        ms[name] = med
        res[name] = {"ms": med, "ms_min": lo, "ms_max": hi, "points_per_s": n / med * 1e3}
    res["ratios"] = {
        "g1_compressed_over_uncompressed": ms["g1_prepare_compressed"] / ms["g1_prepare"],
        "g2_compressed_over_uncompressed": ms["g2_points_prepare_compressed"] / ms["g2_points_prepare"],
        "outputs_exact": True}
    del du1, dc1, du2, dc2

    # ---- (d) the epoch through both grouped functions
    ep = sign["epoch"]
    docs, plain, wire = [], [], []
    for k in range(a.epoch_copies):
        for d, doc in enumerate(ep["documents"]):
            docs.append(bytes.fromhex(doc["hash"]))
            for s in doc["shares"]:
                share, pk = bytes.fromhex(s["share"]), bytes.fromhex(s["pk"])
                plain.append((2 * k + d, s["node"], share, pk))
                wire.append((2 * k + d, s["node"], C.compress_g2(C.parse_g2(share)),
                             C.compress_g1(C.parse_g1(pk))))
    pub = bytes.fromhex(ep["public_key"])
    pub_c = C.compress_g1(C.parse_g1(pub))

    def grouped():
        return T.threshold_sign_grouped(docs, plain, ep["t"], pub)

    def grouped_wire():
        return T.threshold_sign_grouped_wire(docs, wire, ep["t"], pub_c)

    assert grouped() == grouped_wire(), "the wire epoch differs"
    for _ in range(a.warmup):
        grouped()
        grouped_wire()
    steps = max(3, a.steps // 3)
    gms, glo, ghi = event_ms(torch, grouped, steps)
    wms, wlo, whi = event_ms(torch, grouped_wire, steps)
    res["epoch"] = {"documents": len(docs), "shares": len(plain),
                    "threshold_sign_grouped_ms": gms, "threshold_sign_grouped_ms_min": glo,
                    "threshold_sign_grouped_ms_max": ghi,
                    "threshold_sign_grouped_wire_ms": wms, "threshold_sign_grouped_wire_ms_min": wlo,
                    "threshold_sign_grouped_wire_ms_max": whi, "wire_over_uncompressed": wms / gms,
                    "outputs_equal": True}
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
