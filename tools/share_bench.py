#!/usr/bin/env python3
"""Times share creation on the GPU at N = 64, t = 21, C = 4,096 -- the N C =
262,144 decryption shares [sk_i] U_c and signature shares [sk_i] H_c a
simulator makes per batch -- and sets it against the only way the parent
commit had to make them on the device.

    g1_shares / g2_shares     `hbrbc_g1_mul_prepared` / `hbrbc_g2_mul_prepared`,
                              one launch, lanes scalar-major (a wave's 64 lanes
                              share sk_i) and ciphertext-major (a wave holds all
                              64 sk_i), results as a table plus both encodings
    base_mul_253 / _64x253    `hbrbc_g1_base_mul`: one BivarPoly commitment at
                              t = 21, and those of 64 dealers
    generate_part, ack_values one node's calls of the Python functions, host
                              work and read-backs included (wall clock)
    baseline_g1 / baseline_g2 the same shares through `g1_lincomb_prepared` /
                              `g2_lincomb_prepared` with one-term groups and
                              `g1_prepare` / `g2_points_prepare` of the returned
                              bytes (the table the next step reads)

Device events after a warm-up, median of --steps, entries called directly on
preallocated buffers.  Before anything is timed the new path's encodings must
equal the baseline's byte for byte in both lane orders, and its tables the
baseline's prepared tables.  The baseline runs in a child process that binds
only entries the parent commit has, so --parent-lib can name a libhbrbc.so
built from the parent commit's tree; the rounds alternate baseline and new path.
Without --parent-lib the baseline runs on this library (the same kernels).
Writes profiles/share_create.json and prints it as one JSON line."""
import argparse
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = {"g1_mul_table": "g1_mul_table_kernel", "g2_mul_table": "g2_mul_table_kernel",
           "g1_base_mul": "g1_base_mul_kernel", "fr_horner": "fr_horner_kernel",
           "fr_dot": "fr_dot_kernel", "g1_scalar_mul": "g1_scalar_mul_kernel",
           "g2_scalar_mul": "g2_scalar_mul_kernel", "g1_base_mul_check": "g1_base_mul_check_kernel"}
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N, T_DEG, C = 64, 21, 4096


def timed(torch, fn, steps):
    from combine_bench import event_ms
    med, lo, hi = event_ms(torch, fn, steps)
    return {"ms": med, "min": lo, "max": hi}


def table_digest(tab, count, width):
    """sha256 of a point table's coordinates and status bytes (not its padding)."""
    h = tab.cpu().numpy()
    at = (count * width + 255) // 256 * 256
    return hashlib.sha256(h[:count * width].tobytes() + h[at:at + count].tobytes()).hexdigest()


def baseline(a):
    """Child process: the parent commit's path on the library at a.lib."""
    import numpy as np
    import torch
    P, S = ctypes.c_void_p, ctypes.c_size_t
    L = ctypes.CDLL(a.lib)
    sig = {"hbrbc_g1_prepared_size": (S, [S]), "hbrbc_g2_points_size": (S, [S]),
           "hbrbc_g1_combine_workspace_size": (S, [S, S]),
           "hbrbc_g2_combine_workspace_size": (S, [S, S]),
           "hbrbc_g1_prepare": (ctypes.c_int, [P, S, P, P]),
           "hbrbc_g2_points_prepare": (ctypes.c_int, [P, S, P, P]),
           "hbrbc_g1_lincomb_prepared": (ctypes.c_int, [P, S, P, P, P, S, P, P, P, P, P]),
           "hbrbc_g2_lincomb_prepared": (ctypes.c_int, [P, S, P, P, P, S, P, P, P, P, P, P]),
           "hbrbc_version": (ctypes.c_char_p, [])}
    for name, (res, args) in sig.items():
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    dev = "cuda:0"
    inp = np.load(a.inputs)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    total = N * C
    sk = torch.from_numpy(inp["sk"]).to(dev)
    scal = sk.repeat_interleave(C, dim=0).contiguous()        # lane i C + c: sk_i
    rows = torch.arange(C, dtype=torch.int32, device=dev).repeat(N).contiguous()
    offs = torch.arange(total + 1, dtype=torch.int32, device=dev)
    out = {"library": L.hbrbc_version().decode()}

    def ok(rc):
        assert rc == 0, rc

    for g2, key, width in ((False, "u96", 96), (True, "h192", 192)):
        size = L.hbrbc_g2_points_size if g2 else L.hbrbc_g1_prepared_size
        prepare = L.hbrbc_g2_points_prepare if g2 else L.hbrbc_g1_prepare
        ws_size = L.hbrbc_g2_combine_workspace_size if g2 else L.hbrbc_g1_combine_workspace_size
        pts = torch.from_numpy(inp[key]).to(dev)
        tab = torch.empty(size(C), dtype=torch.uint8, device=dev)
        ok(prepare(pts.data_ptr(), C, tab.data_ptr(), stream))
        ws = torch.empty(ws_size(total, total), dtype=torch.uint8, device=dev)
        ou = torch.empty((total, width), dtype=torch.uint8, device=dev)
        oc = torch.empty((total, width // 2), dtype=torch.uint8, device=dev)
        par = torch.empty(total, dtype=torch.uint8, device=dev)
        st = torch.empty(total, dtype=torch.uint8, device=dev)
        otab = torch.empty(size(total), dtype=torch.uint8, device=dev)

        def run():
            if g2:
                ok(L.hbrbc_g2_lincomb_prepared(tab.data_ptr(), C, rows.data_ptr(), scal.data_ptr(),
                                               offs.data_ptr(), total, ou.data_ptr(), oc.data_ptr(),
                                               par.data_ptr(), st.data_ptr(), ws.data_ptr(), stream))
            else:
                ok(L.hbrbc_g1_lincomb_prepared(tab.data_ptr(), C, rows.data_ptr(), scal.data_ptr(),
                                               offs.data_ptr(), total, ou.data_ptr(), oc.data_ptr(),
                                               st.data_ptr(), ws.data_ptr(), stream))
            ok(prepare(ou.data_ptr(), total, otab.data_ptr(), stream))

        run()
        torch.cuda.synchronize()
        assert int(st.max()) == 0
        name = "baseline_g2" if g2 else "baseline_g1"
        out[name + "_digest"] = [hashlib.sha256(ou.cpu().numpy().tobytes()).hexdigest(),
                                 hashlib.sha256(oc.cpu().numpy().tobytes()).hexdigest(),
                                 table_digest(otab, total, width)]
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        out[name] = timed(torch, run, a.steps)
        del ws, ou, oc, par, st, otab
    print("BASELINE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of baseline and new path")
    ap.add_argument("--parent-lib", default="", help="libhbrbc.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "share_create.json"),
                    help="result file ('' writes none)")
    ap.add_argument("--role", default="main", choices=["main", "baseline"])
    ap.add_argument("--lib", default="")
    ap.add_argument("--inputs", default="")
    a = ap.parse_args()
    if a.role == "baseline":
        return baseline(a)

    import numpy as np
    import torch

    import hbbft_amd as hb
    from combine_bench import kernel_resources
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    assert torch.cuda.is_available(), "share_bench needs a GPU"
    L = hb.lib()
    dev = "cuda:0"
    rng = random.Random(0x53484152)
    total = N * C
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def dev_scalars(vals):
        return torch.from_numpy(np.frombuffer(b"".join(v.to_bytes(32, "big") for v in vals),
                                              np.uint8).reshape(len(vals), 32).copy()).to(dev)

    def horner(c, x):
        acc = 0
        for v in reversed(c):
            acc = (acc * x + v) % R
        return acc

    # the epoch's secret key shares, the ciphertexts' U = [u] G1::one() and the
    # documents' H = [h] G2::one() (standing for hash_g2), made on the device
    f = [rng.randrange(1, R) for _ in range(T_DEG + 1)]
    sk = dev_scalars([horner(f, i + 1) for i in range(N)])
    _, u96, u48, ust = K.base_mul(dev_scalars([rng.randrange(1, R) for _ in range(C)]))
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "compressed_vectors.json")))
    g2_one = bytes.fromhex(next(x["u"] for x in gold["g2"] if x["name"] == "g2_valid_0"))
    gtab = T.g2_points_prepare(torch.from_numpy(
        np.frombuffer(g2_one, np.uint8).reshape(1, 192).copy()).to(dev))
    _, h192, _, hst = T.g2_mul_prepared(gtab, 1, torch.zeros(C, dtype=torch.int32, device=dev),
                                        dev_scalars([rng.randrange(1, R) for _ in range(C)]))
    assert int(ust.max()) == 0 and int(hst.max()) == 0
    utab, htab = T.g1_prepare(u96), T.g2_points_prepare(h192)

    lanes = torch.arange(total, dtype=torch.int32, device=dev)
    orders = {   # lane -> (table row c, scalar index i)
        "scalar_major": ((lanes % C).contiguous(), (lanes // C).to(torch.int32).contiguous()),
        "ciphertext_major": ((lanes // N).to(torch.int32).contiguous(), (lanes % N).contiguous())}
    # position of (i, c) in the ciphertext-major launch, listed scalar-major
    to_scalar_major = ((lanes % C) * N + lanes // C).long()

    runs, outs = {}, {}
    for g2, tab, width, name in ((False, utab, 96, "g1_shares"), (True, htab, 192, "g2_shares")):
        entry = L.hbrbc_g2_mul_prepared if g2 else L.hbrbc_g1_mul_prepared
        size = L.hbrbc_g2_points_size if g2 else L.hbrbc_g1_prepared_size
        otab = torch.empty(size(total), dtype=torch.uint8, device=dev)
        ou = torch.empty((total, width), dtype=torch.uint8, device=dev)
        oc = torch.empty((total, width // 2), dtype=torch.uint8, device=dev)
        st = torch.empty(total, dtype=torch.uint8, device=dev)
        outs[name] = (otab, ou, oc, st, width)
        for order, (rows, sidx) in orders.items():
            def run(entry=entry, tab=tab, rows=rows, sidx=sidx, otab=otab, ou=ou, oc=oc, st=st):
                hb._check(entry(tab.data_ptr(), C, rows.data_ptr(), sk.data_ptr(), N,
                                sidx.data_ptr(), total, otab.data_ptr(), ou.data_ptr(),
                                oc.data_ptr(), st.data_ptr(), stream))
            runs["%s_%s" % (name, order)] = run

    # base_mul: one dealer's commitment at t = 21 (253 scalars) and 64 dealers'
    m = K.commitment_len(T_DEG)
    poly = [rng.randrange(1, R) for _ in range(m)]
    for count, name in ((m, "base_mul_%d" % m), (N * m, "base_mul_%dx%d" % (N, m))):
        sc = dev_scalars([poly[k % m] for k in range(count)])
        btab = torch.empty(L.hbrbc_g1_prepared_size(count), dtype=torch.uint8, device=dev)
        b48 = torch.empty((count, 48), dtype=torch.uint8, device=dev)
        bst = torch.empty(count, dtype=torch.uint8, device=dev)

        def run(sc=sc, count=count, btab=btab, b48=b48, bst=bst):
            hb._check(L.hbrbc_g1_base_mul(sc.data_ptr(), count, btab.data_ptr(), None,
                                          b48.data_ptr(), bst.data_ptr(), stream))
        run()
        ok = K.base_mul_check(btab, count, torch.arange(count, dtype=torch.int32, device=dev), sc)
        assert int(bst.max()) == 0 and int(ok.min()) == 1 and int(ok.max()) == 1
        runs[name] = run

    # the baseline's digests come from its first run; the new path must match
    tmp = tempfile.mkdtemp(prefix="share_bench_")
    inputs = os.path.join(tmp, "inputs.npz")
    np.savez(inputs, sk=sk.cpu().numpy(), u96=u96.cpu().numpy(), h192=h192.cpu().numpy())
    base_lib = a.parent_lib or hb.LIB_PATH

    def run_baseline():
        cmd = [sys.executable, os.path.abspath(__file__), "--role", "baseline", "--lib", base_lib,
               "--inputs", inputs, "--steps", str(a.steps), "--warmup", str(a.warmup)]
        res = subprocess.run(cmd, capture_output=True, text=True, stdin=subprocess.DEVNULL)
        if res.returncode != 0:
            raise RuntimeError("baseline failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
        line = next(ln for ln in res.stdout.splitlines() if ln.startswith("BASELINE "))
        return json.loads(line[len("BASELINE "):])

    def time_new():
        ms = {}
        for name, fn in runs.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            ms[name] = timed(torch, fn, a.steps)
        return ms

    rounds = []
    for r in range(a.rounds):
        base = run_baseline()
        if r == 0:   # every output checked before the new path is timed
            for name, key in (("g1_shares", "baseline_g1_digest"), ("g2_shares", "baseline_g2_digest")):
                otab, ou, oc, st, width = outs[name]
                runs[name + "_scalar_major"]()
                torch.cuda.synchronize()
                assert int(st.max()) == 0
                got = [hashlib.sha256(ou.cpu().numpy().tobytes()).hexdigest(),
                       hashlib.sha256(oc.cpu().numpy().tobytes()).hexdigest(),
                       table_digest(otab, total, width)]
                assert got == base[key], "%s differs from the baseline" % name
                sm = ou.clone()
                runs[name + "_ciphertext_major"]()
                torch.cuda.synchronize()
                assert int(st.max()) == 0 and torch.equal(ou[to_scalar_major], sm), \
                    "%s: the lane orders disagree" % name
        rounds.append({"baseline": base, "new": time_new()})
    try:
        os.remove(inputs)
        os.rmdir(tmp)
    except OSError:
        pass

    # one node's dealer calls, host work and read-backs included
    wall = {}
    polyb = [v.to_bytes(32, "big") for v in poly]
    row = K.generate_part(T_DEG, polyb, N)[1][5]
    for name, fn in (("generate_part", lambda: K.generate_part(T_DEG, polyb, N)),
                     ("ack_values", lambda: K.ack_values(row, N))):
        fn()
        ts = []
        for _ in range(a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        wall[name] = {"ms": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}

    def med(vals):
        vals = sorted(vals)
        return vals[len(vals) // 2]

    summary = {}
    for g, width in (("g1", 96), ("g2", 192)):
        b = [r["baseline"]["baseline_" + g]["ms"] for r in rounds]
        sm = [r["new"][g + "_shares_scalar_major"]["ms"] for r in rounds]
        cm = [r["new"][g + "_shares_ciphertext_major"]["ms"] for r in rounds]
        spread = (max(b) - min(b)) / med(b)
        summary[g] = {"baseline_ms": med(b), "baseline_rounds_ms": b,
                      "baseline_spread": spread,
                      "scalar_major_ms": med(sm), "scalar_major_rounds_ms": sm,
                      "ciphertext_major_ms": med(cm), "ciphertext_major_rounds_ms": cm,
                      "shares_per_s_scalar_major": total / med(sm) * 1e3,
                      "shares_per_s_ciphertext_major": total / med(cm) * 1e3,
                      "shares_per_s_baseline": total / med(b) * 1e3,
                      "speedup_over_baseline": med(b) / med(sm),
                      # required: not slower than the baseline beyond its own spread
                      "bound_ms": med(b) * (1 + spread),
                      "not_slower_than_baseline": med(sm) <= med(b) * (1 + spread)}
    res = {"what": "share creation at N = %d, t = %d, C = %d: %d shares per launch (events, "
                   "median of %d, %d alternating rounds)" % (N, T_DEG, C, total, a.steps, a.rounds),
           "n": N, "t": T_DEG, "ciphertexts": C, "shares": total, "steps": a.steps,
           "summary": summary, "rounds": rounds, "wall_clock": wall,
           "baseline_library": rounds[0]["baseline"]["library"],
           "baseline_is_parent_build": bool(a.parent_lib),
           "outputs_exact": True, "library": L.hbrbc_version().decode(),
           "kernel_resources": kernel_resources(hb.LIB_PATH, KERNELS)}
    for v in (res["kernel_resources"] or {}).values():
        v["waves_per_simd"] = min(8, 512 // ((v["vgprs"] + 7) // 8 * 8))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
