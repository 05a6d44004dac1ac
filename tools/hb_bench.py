#!/usr/bin/env python3
"""HoneyBadger epochs on one GPU (hbbft_amd/hb_sim.py: the Subset's two phases,
then hb_sim.hip): honest runs of the payload-free scenarios of
tools/subset_bench.py at N=16 x 1024 instances and N=64 x 32 instances, plain
and encrypted (forced decryption tables).  Per run: total ms (all rounds,
launches and read-backs included), rounds, phase 3's ms from device events
around its launch in every round of one further run, and the Subset-only run
of the same scenario in the same process as the reference point.  Then
`decrypt_plane` over real keys (a seeded SyncKeyGen run) with its four steps
timed separately, at instance counts that keep the pairing work to seconds.
Writes profiles/hb_sim.json.

usage: python tools/hb_bench.py [--reps 5] [--no-plane]
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import subset_bench as sb  # noqa: E402

PLANE_SHAPES = ((16, 64), (64, 2))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001   # the group order


def bench_hb(n, count, encrypted, reps):
    import torch
    from hbbft_amd import hb_sim, subset_sim
    sscn = sb.scenario(n, count)
    scn = hb_sim.Scenario(n, [hb_sim.Instance(i, 0, encrypted) for i in sscn.instances], sb.COINS)
    dev = torch.device("cuda", 0)
    ok, dec = sb.forced_plane(n, count * n, dev)
    kw = dict(max_out=8, bc_max_faults=4, ba_max_faults=4)
    rank = hb_sim.HbRank(scn, 0, ok, dec, hb_max_faults=4, **kw)
    rounds, ts = sb.timed(lambda: hb_sim.run_rounds(rank), reps)
    assert int((rank.batch_round == hb_sim.NO_BATCH).sum()) == 0, "an honest node has no batch"
    assert int(rank.fault_count.max()) == 0
    ds = rank.dstate.cpu().numpy()
    assert (ds == (hb_sim.DS_ACCEPTED | hb_sim.DS_COMPLETE)).all()
    events = []
    assert hb_sim.run_rounds(rank, events) == rounds
    torch.cuda.synchronize()
    events = [(e0, e1) for name, e0, e1 in events if name == "phase3"]
    p3 = sum(e0.elapsed_time(e1) for e0, e1 in events)
    sub = subset_sim.SubsetRank(sscn, 0, ok, dec, **kw)
    sub_rounds, sts = sb.timed(lambda: subset_sim.run_rounds(sub), reps)
    return {"what": "HoneyBadger epoch, %s" % ("encrypted" if encrypted else "plain"), "n": n,
            "instances": count, "nodes": count * n, "threads_phase3": count * n * n,
            "rounds": rounds, "hb_records": rank.hb_records,
            "batch_rounds": sorted({int(v) for v in rank.batch_round.cpu().numpy().reshape(-1)}),
            "ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1], "reps": reps,
            "phase3_ms": p3, "phase3_launches": len(events),
            "phase_note": "device time of phase 3's launches of one further run, all rounds, "
                          "the empty ones after quiescence included",
            "subset_only_rounds": sub_rounds, "subset_only_ms_median": sts[len(sts) // 2],
            "subset_only_ms_min": sts[0], "subset_only_ms_max": sts[-1]}


def bench_plane(n, count, reps):
    import numpy as np
    import torch
    from hbbft_amd import hb_sim
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    f = (n - 1) // 3
    rng = random.Random("hb_bench/keys/%d" % n)
    polys = [[rng.randrange(1, R).to_bytes(32, "big") for _ in range(K.commitment_len(f))]
             for _ in range(n)]
    keys = K.sync_key_gen_network(f, polys)
    sscn = sb.scenario(n, count)
    scn = hb_sim.Scenario(n, [hb_sim.Instance(i, 0, True) for i in sscn.instances], sb.COINS)
    C = count * n

    def scalars(values):
        raw = b"".join(v.to_bytes(32, "big") for v in values)
        return torch.from_numpy(np.frombuffer(raw, np.uint8).reshape(len(values), 32).copy()).to(
            "cuda:0")

    # stand-in ciphertexts: H = [h] G2::one(), U = [r] G1::one(), W = [r] H
    # (a valid G2 point from the wire-encoding vectors serves as the base)
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "compressed_vectors.json")))
    gen = next(x for x in vec["g2"] if x["name"] == "g2_valid_0")
    one = torch.from_numpy(np.frombuffer(bytes.fromhex(gen["u"]), np.uint8).copy()).view(
        1, 192).to("cuda:0")
    hs = scalars([rng.randrange(1, R) for _ in range(C)])
    rs = scalars([rng.randrange(1, R) for _ in range(C)])
    htab, h192, _, _ = T.g2_mul_prepared(T.g2_points_prepare(one), 1,
                                         torch.zeros(C, dtype=torch.int32, device="cuda:0"), hs)
    _, _, w96, _ = T.g2_mul_prepared(htab, C, torch.arange(C, dtype=torch.int32, device="cuda:0"),
                                     rs)
    _, _, u48, _ = K.base_mul(rs)
    u, w, h = u48.cpu().numpy(), w96.cpu().numpy(), h192.cpu().numpy()
    cts = [(bytes(u[c]), bytes(w[c]), bytes(h[c])) for c in range(C)]
    steps = []
    for _ in range(reps + 1):   # (the first is the warm-up)
        tm = {}
        ct_state, share_ok, _, _ = hb_sim.decrypt_plane(scn, cts, keys, timings=tm)
        steps.append(tm)
    assert int(ct_state.max()) == 0 and bool((share_ok[:, 0, 0] == 1).all())
    assert bool((share_ok[:, 0, 1] == 0).all())
    med = {k: sorted(t[k] for t in steps[1:])[reps // 2] for k in steps[0]}
    return {"what": "decrypt_plane", "n": n, "instances": count, "ciphertexts": C,
            "shares": C * n, "share_checks": 2 * C * n, "reps": reps,
            "ms_median": med, "note": "host packing and read-backs of each step included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-plane", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hb_sim.json"))
    a = ap.parse_args()
    import torch
    rows = []
    for n, count in sb.SHAPES:
        for encrypted in (False, True):
            rows.append(bench_hb(n, count, encrypted, a.reps))
            print(json.dumps(rows[-1]), flush=True)
    if not a.no_plane:
        for n, count in PLANE_SHAPES:
            rows.append(bench_plane(n, count, a.reps))
            print(json.dumps(rows[-1]), flush=True)
    doc = {"tool": "tools/hb_bench.py", "device": torch.cuda.get_device_name(0),
           "note": "one process, one session; ms per run = every round of the batch until "
                   "quiescence, launches and read-backs included, median of reps",
           "rows": rows}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
