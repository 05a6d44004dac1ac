#!/usr/bin/env python3
"""Times the decryption-share combine (`PublicKeySet::decrypt` up to g) on the
GPU and sets it against the share verification of the same ciphertexts.

The 22-share group `cfg3_a` of tests/golden/combine_vectors.json (t = 21 of
N = 64) is replicated over --groups ciphertexts, each with its own 22 rows of
one g1_prepare table; `decrypt_combine_prepared` is timed with device events
after a warm-up, and so are its two halves through `lagrange_coeffs` and
`g1_lincomb_prepared`.  In the same process `pairing_check_prepared_pts` runs
the N = 64 share checks per ciphertext of as many ciphertexts (the grouped
fixture of tests/golden/bls_vectors.json tiled, tables prepared outside the
timing).  Results are checked against the fixtures before anything is timed.

Per-kernel times come from a kernel trace taken in a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- \\
        python tools/combine_bench.py --steps 3 --no-verify --out ""
    python tools/combine_bench.py --kernel-stats DIR/.../trace_kernel_stats.csv

The scratch sizes are read from the code object inside libhbrbc.so (its
metadata notes, through llvm-readelf).  Writes profiles/decrypt_combine.json
and prints it as one JSON line."""
import argparse
import csv
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"lagrange": "lagrange_kernel", "scalar_mul": "g1_scalar_mul_kernel",
           "reduce_encode": "g1_reduce_encode_kernel"}
# the operation-count model: a combine is 22 scalar
# multiplications of 255 doublings and 128-255 additions, 3-5 k Fp products
# each; a share check is about 12.5 M lane-operations, 64 per ciphertext
MODEL_RATIO = (0.05, 0.06)


def kernel_resources(lib_path, kernels=None):
    """{kernel: {scratch_bytes, vgprs, vgpr_spills}} of the combine kernels (or
    of `kernels`, {key: kernel name}), from the gfx950 code objects bundled in
    the library; None without llvm-readelf."""
    kernels = kernels or KERNELS
    readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        return None
    data = open(lib_path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out = {}
    pos = data.find(magic)
    while pos >= 0:
        (count,) = struct.unpack_from("<Q", data, pos + len(magic))
        p = pos + len(magic) + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" not in triple or size == 0:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co") as fh:
                fh.write(data[pos + off:pos + off + size])
                fh.flush()
                notes = subprocess.run([readelf, "--notes", fh.name], capture_output=True,
                                       text=True).stdout
            cur = {}
            for line in notes.splitlines() + ["  - end"]:
                line = line.strip()
                if line.startswith("- "):       # next kernel's record
                    for key, name in kernels.items():
                        if name in cur.get(".name", ""):
                            out[key] = {"scratch_bytes": int(cur[".private_segment_fixed_size"]),
                                        "vgprs": int(cur[".vgpr_count"]),
                                        "vgpr_spills": int(cur[".vgpr_spill_count"])}
                    cur = {}
                    line = line[2:]
                if ":" in line:
                    k, v = line.split(":", 1)
                    cur[k.strip()] = v.strip()
        pos = data.find(magic, pos + 1)
    return out or None


def kernel_stats(path):
    """Average ms per launch of the combine kernels from a rocprofv3
    kernel-stats CSV."""
    out = {}
    for row in csv.DictReader(open(path)):
        for key, name in KERNELS.items():
            if name in row["Name"]:
                out[key] = float(row["AverageNs"]) / 1e6
    return out


def event_ms(torch, fn, steps):
    """Median device-event time of fn() over `steps` runs (ms)."""
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4096, help="ciphertexts (B)")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-verify", action="store_true", help="skip the share-verification leg")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel-stats CSV of a run of this script")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decrypt_combine.json"),
                    help="result file ('' writes none)")
    a = ap.parse_args()
    import numpy as np
    import torch

    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    assert torch.cuda.is_available(), "combine_bench needs a GPU"
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "combine_vectors.json")))
    grp = next(g for g in gold["groups"] if g["name"] == "cfg3_a")
    n, B = len(grp["idx"]), a.groups
    total = n * B
    shares = np.frombuffer(b"".join(bytes.fromhex(s) for s in grp["shares"]), np.uint8)
    g1 = torch.from_numpy(np.tile(shares.reshape(n, 96), (B, 1))).cuda()
    tab = T.g1_prepare(g1)
    rows = torch.arange(total, dtype=torch.int32, device="cuda")
    idx = torch.tensor(grp["idx"] * B, dtype=torch.int32, device="cuda")
    offs = torch.arange(B + 1, dtype=torch.int32, device="cuda") * n
    ws = T.combine_workspace(total, B)

    def combine():
        return T.decrypt_combine_prepared(tab, total, rows, idx, offs, ws)

    o96, o48, st = combine()
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * B
    want96 = np.frombuffer(bytes.fromhex(grp["g96"]), np.uint8)
    want48 = np.frombuffer(bytes.fromhex(grp["g48"]), np.uint8)
    assert (o96.cpu().numpy() == want96).all() and (o48.cpu().numpy() == want48).all(), \
        "combine differs from the fixture"
    coeffs, _ = T.lagrange_coeffs(idx, offs)
    for _ in range(a.warmup):
        combine()
        T.lagrange_coeffs(idx, offs)
        T.g1_lincomb_prepared(tab, total, rows, coeffs, offs, ws)
    torch.cuda.synchronize()
    ms, lo, hi = event_ms(torch, combine, a.steps)
    lag_ms = event_ms(torch, lambda: T.lagrange_coeffs(idx, offs), a.steps)[0]
    lin_ms = event_ms(torch, lambda: T.g1_lincomb_prepared(tab, total, rows, coeffs, offs, ws),
                      a.steps)[0]
    res = {"what": "decrypt_combine_prepared: %d groups of %d shares (t = %d of N = 64)" % (B, n, n - 1),
           "groups": B, "shares_per_group": n, "steps": a.steps,
           "combine_ms": ms, "combine_ms_min": lo, "combine_ms_max": hi,
           "combines_per_s": B / ms * 1e3, "scalar_muls_per_s": total / ms * 1e3,
           "entry_ms": {"lagrange_coeffs": lag_ms, "g1_lincomb_prepared": lin_ms},
           "outputs_exact": True, "library": hb.lib().hbrbc_version().decode(),
           "kernel_resources": kernel_resources(hb.LIB_PATH)}
    if a.kernel_stats:
        res["kernel_ms"] = kernel_stats(a.kernel_stats)
    if not a.no_verify:
        vg = json.load(open(os.path.join(ROOT, "tests", "golden", "bls_vectors.json")))["bench_groups"]
        checks = 64 * B
        g2 = np.empty((2 * B, 192), np.uint8)
        sh = np.empty((checks, 96), np.uint8)
        expect = []
        for q in range(B):
            c = vg[q % len(vg)]
            g2[2 * q] = np.frombuffer(bytes.fromhex(c["hash"]), np.uint8)
            g2[2 * q + 1] = np.frombuffer(bytes.fromhex(c["w"]), np.uint8)
            for s, item in enumerate(c["shares"]):
                sh[q * 64 + s] = np.frombuffer(bytes.fromhex(item["share"]), np.uint8)
                expect.append(1 if item["expect"] else 0)
        keys_h = np.stack([np.frombuffer(bytes.fromhex(item["pk"]), np.uint8)
                           for c in vg for item in c["shares"]])
        ic = torch.from_numpy(np.array([(q % len(vg)) * 64 + s for q in range(B)
                                        for s in range(64)], np.int32)).cuda()
        ib = torch.arange(checks, dtype=torch.int32, device="cuda") // 64 * 2
        idd = ib + 1
        prep = T.g2_prepare(torch.from_numpy(g2).cuda())
        keys = T.g1_prepare(torch.from_numpy(keys_h).cuda())
        sprep = T.g1_prepare(torch.from_numpy(sh).cuda())
        vws = T.workspace(checks)

        def verify():
            return T.pairing_check_prepared_pts(sprep, checks, keys, keys_h.shape[0], ic, prep,
                                                2 * B, ib, idd, vws)

        ok = verify()
        torch.cuda.synchronize()
        assert ok.cpu().tolist() == expect, "check outcomes differ from the fixtures"
        for _ in range(a.warmup):
            verify()
        torch.cuda.synchronize()
        vms = event_ms(torch, verify, max(3, a.steps // 3))[0]
        res.update({"verify_checks": checks, "verify_ms": vms, "verify_checks_per_s": checks / vms * 1e3,
                    "combine_over_verify": ms / vms, "model_combine_over_verify": list(MODEL_RATIO)})
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
