#!/usr/bin/env python3
"""Times SyncKeyGen's G1 work on the GPU at N = 64, t = 21 and sets it against
the only way the library had to form the same values before: the linear
combination with full-width scalars.

One node's load is N^2 = 4,096 Ack checks (sync_key_gen.rs:603): the value
commitment of each -- the part's row commitment, degree t, evaluated at
sender_idx + 1 by `hbrbc_g1_poly_eval_prepared` -- and the comparison with
[val] G1::one() by `hbrbc_g1_base_mul_check`.  Timed with device events after a
warm-up, entries called directly on preallocated buffers (device work only):

    check_acks            the two entries in sequence, 4,096 checks
    check_acks_all_nodes  the same load replicated 64 times (262,144 checks),
                          each replica over its own copy of the row tables
                          (its two halves also alone, and the evaluations with
                          the lanes part-major -- all 64 points in every wave --
                          where check_acks orders them by sender)
    commitment_rows       the N row commitments a node forms once per Part
                          (N (t + 1) evaluations of degree t; check_parts' share)
    public_key_shares     N = 64 evaluations of the key set's commitment (one wave)
    baseline_lincomb      the same 4,096 value commitments through
                          `g1_lincomb_prepared`: (t + 1)^2 = 484 terms each over
                          the bivariate commitment, scalars x^i y^j mod r

The N bivariate commitments (16,192 points) are made on the device from
seeded Python-integer polynomials; before anything is timed every check must
hold, one tampered value must fail, and the baseline's encodings must equal
the Horner path's.  Writes profiles/keygen.json and prints it as one JSON
line."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = {"horner": "g1_horner_kernel", "base_mul_check": "g1_base_mul_check_kernel",
           "scalar_mul": "g1_scalar_mul_kernel"}
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keygen.json"),
                    help="result file ('' writes none)")
    a = ap.parse_args()
    import ctypes

    import numpy as np
    import torch

    import hbbft_amd as hb
    from combine_bench import event_ms, kernel_resources
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    assert torch.cuda.is_available(), "keygen_bench needs a GPU"
    L = hb.lib()
    dev = "cuda:0"
    n, t, our = 64, 21, 5
    m, x_our = K.commitment_len(t), our + 1
    rng = random.Random(0x4B47424E)

    def dev_i32(v):
        a = np.asarray(v, dtype=np.int64).astype(np.uint32).view(np.int32)
        return torch.from_numpy(a).to(dev)

    def dev_scalars(vals):
        return torch.from_numpy(np.frombuffer(b"".join(v.to_bytes(32, "big") for v in vals),
                                              np.uint8).reshape(len(vals), 32).copy()).to(dev)

    # N symmetric bivariate polynomials and their commitments [f_ij] G1 (on the device)
    polys = [[rng.randrange(1, R) for _ in range(m)] for _ in range(n)]
    one = np.frombuffer(T.G1_ONE, np.uint8).reshape(1, 96).copy()
    gen = T.g1_prepare(torch.from_numpy(one).to(dev))
    c96, _, cst = T.g1_lincomb_prepared(
        gen, 1, torch.zeros(n * m, dtype=torch.int32, device=dev),
        dev_scalars([c for f in polys for c in f]),
        torch.arange(n * m + 1, dtype=torch.int32, device=dev))
    assert int(cst.max()) == 0
    ctab = T.g1_prepare(c96)
    # our rows f_p(x_our, .) and the values f_p(x_our, s + 1) of every Ack
    rows = [[sum(f[K.coeff_pos(i, j)] * pow(x_our, i, R) for i in range(t + 1)) % R
             for j in range(t + 1)] for f in polys]

    def horner(c, x):
        acc = 0
        for v in reversed(c):
            acc = (acc * x + v) % R
        return acc

    # lanes in the order of the senders, as check_acks runs them: a wave shares
    # its evaluation point; part-major (a wave holds all 64 points) for comparison
    acks = [(p, s) for s in range(n) for p in range(n)]
    part_major = [(p, s) for p in range(n) for s in range(n)]
    value_of = {(p, s): horner(rows[p], s + 1) for p, s in acks}
    checks = len(acks)

    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def table(count):
        return torch.empty(L.hbrbc_g1_prepared_size(count), dtype=torch.uint8, device=dev)

    # commitment_rows: row(x_our) of every part, N (t + 1) evaluations
    r_rows = dev_i32([p * m + K.coeff_pos(i, j) for p in range(n) for j in range(t + 1)
                      for i in range(t + 1)])
    r_offs = dev_i32([(t + 1) * k for k in range(n * (t + 1) + 1)])
    r_poly = dev_i32(list(range(n * (t + 1))))
    r_x = dev_i32([x_our] * (n * (t + 1)))
    rtab, r_st = table(n * (t + 1)), torch.empty(n * (t + 1), dtype=torch.uint8, device=dev)

    def commitment_rows():
        hb._check(L.hbrbc_g1_poly_eval_prepared(
            ctab.data_ptr(), n * m, r_rows.data_ptr(), r_offs.data_ptr(), n * (t + 1),
            r_poly.data_ptr(), r_x.data_ptr(), n * (t + 1), rtab.data_ptr(), None, None,
            r_st.data_ptr(), stream))

    commitment_rows()
    assert int(r_st.max()) == 0
    part_ok = K.base_mul_check(rtab, n * (t + 1), r_poly, dev_scalars([c for r in rows for c in r]))
    assert part_ok.cpu().tolist() == [1] * (n * (t + 1)), "a row does not match its commitment"

    def ack_load(replicas, acks=acks):
        """Buffers and the closure of `replicas` copies of the node's Ack checks."""
        vals = [value_of[a] for a in acks]
        cnt, pts = checks * replicas, n * (t + 1)
        big = table(pts * replicas)
        big[:pts * replicas * 96] = rtab[:pts * 96].repeat(replicas)
        stat_at = (pts * replicas * 96 + 255) // 256 * 256
        big[stat_at:stat_at + pts * replicas] = 0
        a_rows = torch.arange(pts * replicas, dtype=torch.int32, device=dev)
        a_offs = torch.arange(n * replicas + 1, dtype=torch.int32, device=dev) * (t + 1)
        a_poly = dev_i32([k * n + p for k in range(replicas) for p, _ in acks])
        a_x = dev_i32([s + 1 for _, s in acks] * replicas)
        a_val = dev_scalars(vals).repeat(replicas, 1)
        a_idx = torch.arange(cnt, dtype=torch.int32, device=dev)
        vtab = table(cnt)
        o48 = torch.empty((cnt, 48), dtype=torch.uint8, device=dev)
        v_st = torch.empty(cnt, dtype=torch.uint8, device=dev)
        ok = torch.empty(cnt, dtype=torch.uint8, device=dev)

        def values(encode=False):
            hb._check(L.hbrbc_g1_poly_eval_prepared(
                big.data_ptr(), pts * replicas, a_rows.data_ptr(), a_offs.data_ptr(), n * replicas,
                a_poly.data_ptr(), a_x.data_ptr(), cnt, vtab.data_ptr(), None,
                o48.data_ptr() if encode else None, v_st.data_ptr(), stream))

        def compare():
            hb._check(L.hbrbc_g1_base_mul_check(vtab.data_ptr(), cnt, a_idx.data_ptr(),
                                                a_val.data_ptr(), cnt, ok.data_ptr(), stream))

        return values, compare, ok, o48, a_val

    values, compare, ok, o48, a_val = ack_load(1)
    values(encode=True)
    compare()
    assert ok.cpu().tolist() == [1] * checks, "an Ack value does not match its commitment"
    keep = a_val[77].clone()
    a_val[77, 31] ^= 1
    compare()
    assert ok.cpu().tolist() == [0 if k == 77 else 1 for k in range(checks)]
    a_val[77] = keep

    # the baseline: the same value commitments as linear combinations of the
    # bivariate commitment's (t + 1)^2 entries with scalars x^i y^j mod r
    terms = (t + 1) ** 2
    sc = np.empty((n, terms, 32), np.uint8)
    for s in range(n):
        sc[s] = np.frombuffer(b"".join(
            (pow(x_our, i, R) * pow(s + 1, j, R) % R).to_bytes(32, "big")
            for i in range(t + 1) for j in range(t + 1)), np.uint8).reshape(terms, 32)
    b_scal = torch.from_numpy(sc[[s for _, s in acks]].reshape(checks * terms, 32)).to(dev)
    posn = np.asarray([K.coeff_pos(i, j) for i in range(t + 1) for j in range(t + 1)], np.int32)
    b_rows = np.concatenate([p * m + posn for p, _ in acks]).astype(np.int32)
    b_rows = torch.from_numpy(b_rows).to(dev)
    b_offs = torch.arange(checks + 1, dtype=torch.int32, device=dev) * terms
    b_ws = T.combine_workspace(checks * terms, checks)
    b96 = torch.empty((checks, 96), dtype=torch.uint8, device=dev)
    b48 = torch.empty((checks, 48), dtype=torch.uint8, device=dev)
    b_st = torch.empty(checks, dtype=torch.uint8, device=dev)

    def baseline():
        hb._check(L.hbrbc_g1_lincomb_prepared(
            ctab.data_ptr(), n * m, b_rows.data_ptr(), b_scal.data_ptr(), b_offs.data_ptr(), checks,
            b96.data_ptr(), b48.data_ptr(), b_st.data_ptr(), b_ws.data_ptr(), stream))

    baseline()
    torch.cuda.synchronize()
    assert int(b_st.max()) == 0
    assert torch.equal(b48, o48), "the linear combination and the Horner path differ"

    # public_key_shares: the key set of all N parts, evaluated at 1 .. N
    gtab, _, _, gst = K._generate(t, ctab, n, list(range(n)), dev)
    assert int(gst.max()) == 0
    master = [sum(f[K.coeff_pos(0, j)] for f in polys) % R for j in range(t + 1)]
    k_rows, k_offs = dev_i32(list(range(t + 1))), dev_i32([0, t + 1])
    k_poly, k_x = dev_i32([0] * n), dev_i32([i + 1 for i in range(n)])
    ktab, k96 = table(n), torch.empty((n, 96), dtype=torch.uint8, device=dev)
    k48 = torch.empty((n, 48), dtype=torch.uint8, device=dev)
    k_st = torch.empty(n, dtype=torch.uint8, device=dev)

    def key_shares():
        hb._check(L.hbrbc_g1_poly_eval_prepared(
            gtab.data_ptr(), t + 1, k_rows.data_ptr(), k_offs.data_ptr(), 1, k_poly.data_ptr(),
            k_x.data_ptr(), n, ktab.data_ptr(), k96.data_ptr(), k48.data_ptr(), k_st.data_ptr(),
            stream))

    key_shares()
    share_ok = K.base_mul_check(ktab, n, torch.arange(n, dtype=torch.int32, device=dev),
                                dev_scalars([horner(master, i + 1) for i in range(n)]))
    assert share_ok.cpu().tolist() == [1] * n, "a key share is not [f(i + 1)] G1"

    def both(v, c):
        def run():
            v()
            c()
        return run

    values_all, compare_all, ok_all, _, _ = ack_load(n)
    both(values_all, compare_all)()
    values_pm, compare_pm, ok_pm, _, _ = ack_load(n, part_major)
    both(values_pm, compare_pm)()
    torch.cuda.synchronize()
    assert int(ok_all.min()) == 1 and int(ok_all.max()) == 1
    assert int(ok_pm.min()) == 1 and int(ok_pm.max()) == 1

    runs = {"check_acks": both(values, compare), "horner_values": values,
            "base_mul_check": compare, "commitment_rows": commitment_rows,
            "public_key_shares": key_shares, "baseline_lincomb": baseline,
            "check_acks_all_nodes": both(values_all, compare_all),
            "horner_values_all_nodes": values_all, "base_mul_check_all_nodes": compare_all,
            "horner_values_all_nodes_part_major": values_pm}
    ms = {}
    for name, fn in runs.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        med, lo, hi = event_ms(torch, fn, a.steps)
        ms[name] = {"ms": med, "min": lo, "max": hi}
    res = {"what": "SyncKeyGen at N = %d, t = %d: device work per entry (events, median of %d)"
                   % (n, t, a.steps),
           "n": n, "t": t, "checks": checks, "checks_all_nodes": checks * n, "steps": a.steps,
           "timings": ms,
           "check_acks_per_s": checks / ms["check_acks"]["ms"] * 1e3,
           "check_acks_all_nodes_per_s": checks * n / ms["check_acks_all_nodes"]["ms"] * 1e3,
           # forming the 4,096 value commitments: the parent's path over the new one
           # (the new one also forms the N rows once per node: included)
           "values_speedup": ms["baseline_lincomb"]["ms"]
                             / (ms["horner_values"]["ms"] + ms["commitment_rows"]["ms"]),
           # the whole check, both with the same comparison step
           "check_speedup": (ms["baseline_lincomb"]["ms"] + ms["base_mul_check"]["ms"])
                            / (ms["check_acks"]["ms"] + ms["commitment_rows"]["ms"]),
           "baseline_terms": checks * terms,
           "outputs_exact": True, "library": L.hbrbc_version().decode(),
           "kernel_resources": kernel_resources(hb.LIB_PATH, KERNELS)}
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
