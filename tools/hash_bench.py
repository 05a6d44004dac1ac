#!/usr/bin/env python3
"""Times hash_g2, xor_with_hash and the encrypt pipeline on the GPU.

    hash_g2_4096 / _262144   `hbrbc_hash_g2_batch` over 32-byte documents, both
                             launches, table and both encodings
    sample_* / cofactor_*    the two launches apart (HBRBC_HASH_G2_PHASE = 1 /
                             2 in a child process each: the library reads it
                             per call, the children keep this process's
                             environment clean)
    g2_mul_*                 the yardstick, in the same process as hash_g2_*:
                             `hbrbc_g2_mul_prepared` over the same count, one
                             255-bit scalar per lane, on the hashes themselves.
                             The cofactor is one fixed 507-bit multiplication,
                             so sample + about twice this is the expectation.
    pad_4096x256KiB          `hbrbc_xor_with_hash_batch`, 1 GiB in place
    encrypt_262144           the five launches of encrypt_batch for N = 64
                             nodes x 4,096 messages of 32 bytes (device work;
                             the list handling of the Python function is not in)

Device events after a warm-up, median of --steps.  No threshold: nothing
comparable existed before.  Writes profiles/hash_g2.json and prints it as one
JSON line."""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
COUNTS = (4096, 262144)


def timed(torch, fn, steps, warmup):
    from combine_bench import event_ms
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    med, lo, hi = event_ms(torch, fn, steps)
    return {"ms": med, "min": lo, "max": hi}


def documents(torch, count):
    import numpy as np
    rng = np.random.default_rng(0x48415348 + count)
    flat = torch.from_numpy(rng.integers(0, 256, 32 * count, dtype=np.uint8)).to("cuda:0")
    offs = torch.arange(0, 32 * count + 1, 32, dtype=torch.int32, device="cuda:0")
    return flat, offs


def scalars(torch, count, seed):
    import numpy as np
    rng = random.Random(seed)
    raw = b"".join(rng.randrange(1 << 254, R).to_bytes(32, "big") for _ in range(count))
    return torch.from_numpy(np.frombuffer(raw, np.uint8).reshape(count, 32).copy()).to("cuda:0")


def phase_child(a):
    """Child process: hash_g2 per count with only launch a.phase taken.  The
    full call first allocates and fills the table the cofactor launch reads;
    the knob is set only around the timed calls (the library reads it per
    call)."""
    import ctypes

    import torch

    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    L = hb.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream("cuda:0").cuda_stream)
    res = {}
    for count in COUNTS:
        flat, offs = documents(torch, count)
        os.environ.pop("HBRBC_HASH_G2_PHASE", None)
        tab, o192, o96, st, _ = T.hash_g2_batch(flat, offs)

        def run():
            hb._check(L.hbrbc_hash_g2_batch(flat.data_ptr(), offs.data_ptr(), count,
                                            flat.numel(), tab.data_ptr(), o192.data_ptr(),
                                            o96.data_ptr(), st.data_ptr(), None, stream))
        os.environ["HBRBC_HASH_G2_PHASE"] = a.phase
        res[str(count)] = timed(torch, run, a.steps, a.warmup)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--phase", help="child: print the hash timings of this phase")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_g2.json"))
    a = ap.parse_args()
    if a.phase:
        phase_child(a)
        return

    import torch
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    assert torch.cuda.is_available(), "hash_bench needs a GPU"
    os.environ.pop("HBRBC_HASH_G2_PHASE", None)
    timings = {}
    for count in COUNTS:
        flat, offs = documents(torch, count)
        tab, _, _, st, wd = T.hash_g2_batch(flat, offs, words=True)
        assert int(st.max()) == 0
        t = timed(torch, lambda: T.hash_g2_batch(flat, offs), a.steps, a.warmup)
        t["hashes_per_s"] = count / t["ms"] * 1e3
        t["mean_words"] = float(wd.float().mean())
        timings["hash_g2_%d" % count] = t
        k = scalars(torch, count, count)
        rows = torch.arange(count, dtype=torch.int32, device="cuda:0")
        y = timed(torch, lambda: T.g2_mul_prepared(tab, count, rows, k), a.steps, a.warmup)
        y["per_s"] = count / y["ms"] * 1e3
        timings["g2_mul_%d" % count] = y
    for phase, name in (("1", "sample"), ("2", "cofactor")):
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--phase", phase,
                                "--steps", str(a.steps), "--warmup", str(a.warmup)],
                               check=True, capture_output=True, text=True, timeout=600,
                               stdin=subprocess.DEVNULL)
        for count, t in json.loads(child.stdout.strip().splitlines()[-1]).items():
            timings["%s_%s" % (name, count)] = t

    # the pad: 4,096 rows of 256 KiB, in place
    rows_n, row_len = 4096, 256 << 10
    data = torch.zeros(rows_n * row_len, dtype=torch.uint8, device="cuda:0")
    offs = torch.arange(0, rows_n * row_len + 1, row_len, dtype=torch.int64,
                        device="cuda:0").to(torch.int32)
    _, _, g48, gst = K.base_mul(scalars(torch, rows_n, 7))
    assert int(gst.max()) == 0
    t = timed(torch, lambda: T.xor_with_hash_batch(g48, data, offs, out=data), a.steps, a.warmup)
    t["GB_per_s"] = rows_n * row_len / t["ms"] / 1e6
    timings["pad_4096x256KiB"] = t
    del data

    # encrypt: N = 64 x 4,096 messages of 32 bytes under one public key
    n = 64 * 4096
    r = scalars(torch, n, 11)
    msgs, moffs = documents(torch, n)
    _, pk96, _, _ = K.base_mul(scalars(torch, 1, 13))
    pktab = T.g1_prepare(pk96)
    zeros = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    lanes = torch.arange(n, dtype=torch.int32, device="cuda:0")

    def encrypt():
        _, _, u48, _ = K.base_mul(r)
        _, _, g48, _ = T.g1_mul_prepared(pktab, 1, zeros, r)
        v, _ = T.xor_with_hash_batch(g48, msgs, moffs)
        htab, _, _, _, _ = T.hash_g2_batch(v, moffs, us48=u48, encode=False)
        return T.g2_mul_prepared(htab, n, lanes, r)
    t = timed(torch, encrypt, a.steps, a.warmup)
    t["ciphertexts_per_s"] = n / t["ms"] * 1e3
    timings["encrypt_%d" % n] = t

    import hbbft_amd as hb
    res = {"what": "hash_g2, xor_with_hash and the encrypt pipeline (device events, median of "
                   "%d after %d warm-up runs)" % (a.steps, a.warmup),
           "library": hb.lib().hbrbc_version().decode(), "device": torch.cuda.get_device_name(0),
           "steps": a.steps, "timings": timings}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
