#!/usr/bin/env python3
"""Times the threshold-signature path (`ThresholdSign`, the coin) on the GPU:
the share check e(pk_i, H) == e(G1::one(), share_i) and the G2 combine, each
against what the library offered before.

Shape (cfg3): --docs documents of 64 shares each (262,144 checks at 4096) and
--docs groups of 22 shares.  All in one process, device events after a
warm-up, the median of --steps runs, results checked against the fixtures
before anything is timed:

  (a) sig_check_prepared, tables prepared outside the timing, and the time to
      prepare them (hashes, keys, shares);
  (b) pairing_check_batch on the same inputs: the existing way to run this
      check (both G2 points decoded and walked per lane);
  (c) pairing_check_prepared_pts on the decryption-share shape, for context;
  (d) sig_combine_prepared against decrypt_combine_prepared at the same shape.

The checks are the valid-point shares of the epoch of
tests/golden/sign_vectors.json (true ones, a tampered one, a stranger's key),
64 per document; the groups are its 22-share group `cfg3_a` replicated, each
on table rows of its own.  --combine-only runs (d) alone (for an A/B of two
libraries: HBRBC_LIB picks the library).  Per-kernel times come from a kernel trace taken
in a run of its own, as for tools/combine_bench.py (--kernel-stats).  Register
and scratch sizes are read from the code object inside libhbrbc.so.  Writes
profiles/threshold_sign.json and prints it as one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from combine_bench import event_ms, kernel_resources  # noqa: E402

KERNELS = {"g2_points": "g2_points_kernel", "miller_sig": "miller_sig_kernel",
           "g2_scalar_mul": "g2_scalar_mul_kernel", "g2_reduce_encode": "g2_reduce_encode_kernel"}
TRACED = dict(KERNELS, lagrange="lagrange_kernel", final_exp="final_exp_kernel",
              miller2="miller2_kernel", g2_prepare="g2_prepare_kernel",
              g1_scalar_mul="g1_scalar_mul_kernel")
# the operation-count model: an Fp2 product is three Fp
# products and a square two, so the G2 combine costs about 3x the G1 combine
MODEL_G2_OVER_G1 = 3.0


def kernel_stats(path):
    """Average ms per launch of the traced kernels from a rocprofv3
    kernel-stats CSV."""
    import csv
    out = {}
    for row in csv.DictReader(open(path)):
        for key, name in TRACED.items():
            if name in row["Name"]:
                out[key] = {"avg_ms": float(row["AverageNs"]) / 1e6, "calls": int(row["Calls"])}
    return out


def rows_t(torch, np, items, width):
    a = np.frombuffer(b"".join(items), np.uint8).reshape(len(items), width)
    return torch.from_numpy(a.copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096, help="documents and groups (B)")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--combine-only", action="store_true", help="only (d), the combine")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel-stats CSV of a run of this script")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "threshold_sign.json"),
                    help="result file ('' writes none)")
    a = ap.parse_args()
    import numpy as np
    import torch

    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    assert torch.cuda.is_available(), "sign_bench needs a GPU"
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "sign_vectors.json")))
    B = a.docs
    res = {"what": "ThresholdSign: %d documents x 64 share checks, %d groups of 22 shares" % (B, B),
           "docs": B, "steps": a.steps, "library": hb.lib().hbrbc_version().decode(),
           "kernel_resources": kernel_resources(hb.LIB_PATH, KERNELS)}

    # ---- (d) the combine, G2 against G1 at the same shape
    grp = next(g for g in gold["groups"] if g["name"] == "cfg3_a")
    n = len(grp["idx"])
    total = n * B
    sh2 = np.frombuffer(b"".join(bytes.fromhex(s) for s in grp["shares"]), np.uint8)
    stab = T.g2_points_prepare(torch.from_numpy(np.tile(sh2.reshape(n, 192), (B, 1))).cuda())
    rows = torch.arange(total, dtype=torch.int32, device="cuda")
    idx = torch.tensor(grp["idx"] * B, dtype=torch.int32, device="cuda")
    offs = torch.arange(B + 1, dtype=torch.int32, device="cuda") * n
    ws2 = T.combine_g2_workspace(total, B)

    def combine_g2():
        return T.sig_combine_prepared(stab, total, rows, idx, offs, ws2)

    o192, o96, par, st = combine_g2()
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * B and par.cpu().tolist() == [grp["parity"]] * B
    assert (o192.cpu().numpy() == np.frombuffer(bytes.fromhex(grp["sig192"]), np.uint8)).all()
    assert (o96.cpu().numpy() == np.frombuffer(bytes.fromhex(grp["sig96"]), np.uint8)).all(), \
        "combine differs from the fixture"
    cg = json.load(open(os.path.join(ROOT, "tests", "golden", "combine_vectors.json")))
    grp1 = next(g for g in cg["groups"] if g["name"] == "cfg3_a")
    assert len(grp1["idx"]) == n
    sh1 = np.frombuffer(b"".join(bytes.fromhex(s) for s in grp1["shares"]), np.uint8)
    tab1 = T.g1_prepare(torch.from_numpy(np.tile(sh1.reshape(n, 96), (B, 1))).cuda())
    idx1 = torch.tensor(grp1["idx"] * B, dtype=torch.int32, device="cuda")
    ws1 = T.combine_workspace(total, B)

    def combine_g1():
        return T.decrypt_combine_prepared(tab1, total, rows, idx1, offs, ws1)

    g96 = combine_g1()[0]
    torch.cuda.synchronize()
    assert (g96.cpu().numpy() == np.frombuffer(bytes.fromhex(grp1["g96"]), np.uint8)).all()
    for _ in range(a.warmup):
        combine_g2()
        combine_g1()
    torch.cuda.synchronize()
    ms2, lo2, hi2 = event_ms(torch, combine_g2, a.steps)
    ms1, lo1, hi1 = event_ms(torch, combine_g1, a.steps)
    res["combine"] = {
        "groups": B, "shares_per_group": n,
        "sig_combine_ms": ms2, "sig_combine_ms_min": lo2, "sig_combine_ms_max": hi2,
        "sig_combines_per_s": B / ms2 * 1e3, "g2_scalar_muls_per_s": total / ms2 * 1e3,
        "decrypt_combine_ms": ms1, "decrypt_combine_ms_min": lo1, "decrypt_combine_ms_max": hi1,
        "g2_over_g1": ms2 / ms1, "model_g2_over_g1": MODEL_G2_OVER_G1, "outputs_exact": True}
    del stab, tab1, ws1, ws2

    if not a.combine_only:
        # ---- (a) the share check from prepared tables
        ep = gold["epoch"]
        from oracle import bls_oracle as O
        docs_h = [bytes.fromhex(d["hash"]) for d in ep["documents"]]
        every = [(bytes.fromhex(s["share"]), bytes.fromhex(s["pk"]), docs_h[d], s["expect"])
                 for d, doc in enumerate(ep["documents"]) for s in doc["shares"]]
        assert T.verify_signature_shares([e[:3] for e in every]) == [e[3] for e in every], \
            "check outcomes differ from the fixture"
        # timed: the entries whose points are all valid and finite (an invalid
        # point or an infinity idles its lane for one or both legs)
        skip = {O.g1_bytes(O.g1_curve_point(0x5EED)), O.g2_bytes(O.g2_curve_point(0x5EED)),
                O.g2_bytes(None)}
        per_doc = [[(s, pk, e) for s, pk, h, e in every if h == docs_h[d] and s not in skip
                    and pk not in skip] for d in range(2)]
        assert [len(e) for e in per_doc] == [5, 6]
        keys = []
        for ents in per_doc:
            for _, pk, _ in ents:
                if pk not in keys:
                    keys.append(pk)
        checks = 64 * B
        shares, ik, expect = [], [], []
        for q in range(B):
            ents = per_doc[q % 2]
            for s in range(64):
                share, pk, e = ents[s % len(ents)]
                shares.append(share)
                ik.append(keys.index(pk))
                expect.append(1 if e else 0)
        assert set(expect) == {0, 1}
        d_hash = rows_t(torch, np, [docs_h[q % 2] for q in range(B)], 192)
        d_keys = rows_t(torch, np, keys, 96)
        d_sh = rows_t(torch, np, shares, 192)
        ik_t = torch.tensor(ik, dtype=torch.int32, device="cuda")
        ih_t = torch.arange(checks, dtype=torch.int32, device="cuda") // 64
        tabs = {}

        def prepare():
            tabs["prep"] = T.g2_prepare(d_hash)
            tabs["keys"] = T.g1_prepare(d_keys)
            tabs["sig"] = T.g2_points_prepare(d_sh)

        prepare()
        vws = T.workspace(checks)

        def check():
            return T.sig_check_prepared(tabs["sig"], checks, tabs["keys"], len(keys), ik_t,
                                        tabs["prep"], B, ih_t, vws)

        ok = check()
        torch.cuda.synchronize()
        assert ok.cpu().tolist() == expect, "check outcomes differ from the fixture"
        for _ in range(a.warmup):
            check()
        torch.cuda.synchronize()
        steps = max(3, a.steps // 3)
        cms, clo, chi = event_ms(torch, check, steps)
        pms = event_ms(torch, prepare, steps)[0]
        pms_sig = event_ms(torch, lambda: T.g2_points_prepare(d_sh), steps)[0]
        res["share_check"] = {
            "checks": checks, "sig_check_prepared_ms": cms, "sig_check_prepared_ms_min": clo,
            "sig_check_prepared_ms_max": chi, "checks_per_s": checks / cms * 1e3,
            "prepare_ms": pms, "prepare_shares_ms": pms_sig,
            "checks_per_s_with_prepare": checks / (cms + pms) * 1e3, "outcomes_exact": True}
        del vws

        # ---- (b) the same checks through the existing entry: a = pk, b = H,
        # c = G1::one(), d = share
        one = np.frombuffer(T.G1_ONE, np.uint8)
        g1 = np.empty((2 * checks, 96), np.uint8)
        g1[0::2] = d_keys.cpu().numpy()[np.asarray(ik)]
        g1[1::2] = one
        g2 = np.empty((2 * checks, 192), np.uint8)
        g2[0::2] = np.repeat(d_hash.cpu().numpy(), 64, axis=0)
        g2[1::2] = d_sh.cpu().numpy()
        dg1, dg2 = torch.from_numpy(g1).cuda(), torch.from_numpy(g2).cuda()
        bws = T.workspace(2 * checks)

        def batch():
            return T.pairing_check_batch(dg1, dg2, bws)

        okb = batch()
        torch.cuda.synchronize()
        assert okb.cpu().tolist() == expect, "pairing_check_batch differs from the fixture"
        bms, blo, bhi = event_ms(torch, batch, 3)
        res["share_check"].update({
            "pairing_check_batch_ms": bms, "pairing_check_batch_ms_min": blo,
            "pairing_check_batch_ms_max": bhi,
            "batch_over_prepared": bms / cms, "batch_over_prepared_with_prepare": bms / (cms + pms)})
        del dg1, dg2, bws, tabs, d_sh

        # ---- (c) the decryption-share check at the same count, for context
        vg = json.load(open(os.path.join(ROOT, "tests", "golden", "bls_vectors.json")))["bench_groups"]
        g2c = np.empty((2 * B, 192), np.uint8)
        sh = np.empty((checks, 96), np.uint8)
        expect_d = []
        for q in range(B):
            c = vg[q % len(vg)]
            g2c[2 * q] = np.frombuffer(bytes.fromhex(c["hash"]), np.uint8)
            g2c[2 * q + 1] = np.frombuffer(bytes.fromhex(c["w"]), np.uint8)
            for s, item in enumerate(c["shares"]):
                sh[q * 64 + s] = np.frombuffer(bytes.fromhex(item["share"]), np.uint8)
                expect_d.append(1 if item["expect"] else 0)
        keys_h = np.stack([np.frombuffer(bytes.fromhex(item["pk"]), np.uint8)
                           for c in vg for item in c["shares"]])
        ic = torch.from_numpy(np.array([(q % len(vg)) * 64 + s for q in range(B)
                                        for s in range(64)], np.int32)).cuda()
        ib = torch.arange(checks, dtype=torch.int32, device="cuda") // 64 * 2
        idd = ib + 1
        prep = T.g2_prepare(torch.from_numpy(g2c).cuda())
        dkeys = T.g1_prepare(torch.from_numpy(keys_h).cuda())
        sprep = T.g1_prepare(torch.from_numpy(sh).cuda())
        dws = T.workspace(checks)

        def verify():
            return T.pairing_check_prepared_pts(sprep, checks, dkeys, keys_h.shape[0], ic, prep,
                                                2 * B, ib, idd, dws)

        okd = verify()
        torch.cuda.synchronize()
        assert okd.cpu().tolist() == expect_d, "decryption-share outcomes differ from the fixtures"
        verify()
        torch.cuda.synchronize()
        vms = event_ms(torch, verify, steps)[0]
        res["decrypt_share_check"] = {"checks": checks, "pairing_check_prepared_pts_ms": vms,
                                      "checks_per_s": checks / vms * 1e3,
                                      "sig_over_decrypt": cms / vms}
    if a.kernel_stats:
        res["kernel_ms"] = kernel_stats(a.kernel_stats)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
