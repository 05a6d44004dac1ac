#!/usr/bin/env python3
"""BinaryAgreement rounds alone (hbbft_amd/ba_sim.py over ba_sim.hip): honest
runs of 2048 instances at N=64 and N=128 on one GPU, seeded random inputs (so
the runs span several epochs and flip coins) and forced coin tables.  Per N
and launch form: ms per run (all rounds, read-backs included), rounds, the
highest decision epoch, records, node-rounds per second.  Beside it, as the
reader's yardstick, the Broadcast state machine (tools/sm_bench.py's loop) at
the same N and instance count in the same process, and the host restatement
(hbbft_amd/binary_agreement.py in tests/ba_net.py's rounds) on a small slice
of the same scenarios on the CPU -- reported as measured, not extrapolated.
Writes profiles/ba_sim.json.

usage: python tools/ba_bench.py [--reps 7] [--instances 2048] [--host-slice 4]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COINS = 8


def scenario(n, count, seed=0):
    from hbbft_amd.ba_sim import Instance, Scenario
    rng = random.Random("ba_bench/%d/%d" % (n, seed))
    return Scenario(n, [Instance(n, [rng.randrange(2) for _ in range(n)],
                                 coin_bits=[rng.randrange(2) for _ in range(COINS)])
                        for _ in range(count)], COINS)


def timed(fn, reps):
    import torch
    fn()                                    # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return out, ts


def bench_ba(n, count, reps, form_name, form):
    from hbbft_amd import ba_sim
    scn = scenario(n, count)
    rank = ba_sim.BaRank.from_scenario(scn, 0, max_out=8, max_faults=4, form=form)
    rounds, ts = timed(lambda: ba_sim.run_rounds(rank), reps)
    dec, ep = rank.decisions()
    assert (dec != ba_sim.NONE).all() and (dec.min(axis=1) == dec.max(axis=1)).all(), \
        "an honest run did not reach agreement"
    assert int(rank.fault_count.max()) == 0
    med = ts[len(ts) // 2]
    return {"what": "BinaryAgreement", "form": form_name, "n": n, "instances": count,
            "nodes": count * n, "rounds": rounds, "max_epoch": int(ep.max()),
            "records": rank.records, "ms_median": med, "ms_min": ts[0], "ms_max": ts[-1],
            "reps": reps, "node_rounds_per_s": count * n * rounds / (med * 1e-3)}, scn, dec, ep


def bench_broadcast(n, count, reps):
    """tools/sm_bench.py's measurement at this N and instance count."""
    import torch
    from hbbft_amd.rbc_sim import StateMachineRank, honest_tensors, run_rounds
    dev = torch.device("cuda", 0)
    ok = torch.zeros((count, 1, 2, n), dtype=torch.uint8, device=dev)
    ok[:, 0, 0, :] = 1
    dec = torch.ones((count, 1), dtype=torch.uint8, device=dev)
    sm = StateMachineRank(n, count, 1, honest_tensors(n, [i % n for i in range(count)], dev), 0, 1,
                          device=0, max_out=4, max_faults=4, ok=ok, dec=dec)
    rounds, ts = timed(lambda: run_rounds([sm]), reps)
    assert bool((sm.output_root == 0).all()), "an honest node did not decide"
    med = ts[len(ts) // 2]
    return {"what": "Broadcast (sm_bench)", "n": n, "instances": count, "nodes": count * n,
            "rounds": rounds, "records": sm.records, "ms_median": med, "ms_min": ts[0],
            "ms_max": ts[-1], "reps": reps, "node_rounds_per_s": count * n * rounds / (med * 1e-3)}


def bench_host(scn, k, dec, ep):
    """The host restatement on the first k instances of `scn`, one CPU thread."""
    import ba_net
    t0 = time.perf_counter()
    res = [ba_net.run_rounds(scn.n, i.inputs, scn.host_table(r), i.role, i.flip, i.ahead)
           for r, i in enumerate(scn.instances[:k])]
    ms = (time.perf_counter() - t0) * 1e3
    for r, h in enumerate(res):   # the slice agrees with the GPU run
        assert [h.decisions[j] for j in range(scn.n)] == dec[r].tolist()
        assert [h.decision_epochs[j] for j in range(scn.n)] == ep[r].tolist()
    return {"what": "host restatement (CPU, one thread), the first instances of the same scenario",
            "n": scn.n, "instances": k, "nodes": k * scn.n, "rounds": max(h.rounds for h in res),
            "ms_total": ms, "ms_per_instance": ms / k,
            "node_rounds_per_s": sum(scn.n * h.rounds for h in res) / (ms * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--instances", type=int, default=2048)
    ap.add_argument("--host-slice", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_sim.json"))
    a = ap.parse_args()
    import torch
    from hbbft_amd import ba_sim
    rows = []
    for n in (64, 128):
        first = None
        for name, form in [("auto", ba_sim.FORM_AUTO)] + sorted(ba_sim.FORMS.items()):
            row, scn, dec, ep = bench_ba(n, a.instances, a.reps, name, form)
            if first is None:
                first = (dec.copy(), ep.copy())
            assert (dec == first[0]).all() and (ep == first[1]).all(), "the forms disagree"
            rows.append(row)
            print(json.dumps(row), flush=True)
        rows.append(bench_broadcast(n, a.instances, a.reps))
        print(json.dumps(rows[-1]), flush=True)
        rows.append(bench_host(scn, a.host_slice, *first))
        print(json.dumps(rows[-1]), flush=True)
    doc = {"tool": "tools/ba_bench.py", "device": torch.cuda.get_device_name(0),
           "note": "one process, one session; ms per run = every round of the batch until "
                   "quiescence, launches and read-backs included, median of reps",
           "rows": rows}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
