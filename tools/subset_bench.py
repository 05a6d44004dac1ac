#!/usr/bin/env python3
"""Subset rounds on one GPU (hbbft_amd/subset_sim.py over sim.hip with
HBRBC_SM_SUBSET and subset_sim.hip): honest runs of random payload-free
scenarios -- every proof valid, every decode Ok, seeded coin bits -- at N=16 x
1024 instances and N=64 x 32 instances.  Per run: total ms (all rounds,
launches and read-backs included), rounds, and the ms of each phase from
device events around every launch of one further run.  Beside them, from the
same process, the standalone Broadcast (tools/sm_bench.py's loop) and
BinaryAgreement (tools/ba_bench.py's) runs over the same count x n instance
counts.  Writes profiles/subset_sim.json; `--sm-rows FILE` copies the
tools/sm_bench.py lines collected in FILE (one JSON object per line, each with
a "build" key) into it.

usage: python tools/subset_bench.py [--reps 5] [--sm-rows FILE]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COINS = 8
SHAPES = ((16, 1024), (64, 32))


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


def scenario(n, count):
    from hbbft_amd import rbc_sim, subset_sim
    rng = random.Random("subset_bench/%d" % n)
    # (payload-free: the values only name the codewords, the outcomes are forced)
    bcs = [rbc_sim.Instance(n, p, [b""]) for p in range(n)]
    return subset_sim.Scenario(n, [subset_sim.Instance(
        n, bcs, coin_bits=[[rng.randrange(2) for _ in range(COINS)] for _ in range(n)])
        for _ in range(count)], COINS)


def forced_plane(n, instances, dev):
    import torch
    ok = torch.zeros((instances, 1, 2, n), dtype=torch.uint8, device=dev)
    ok[:, 0, 0, :] = 1
    return ok, torch.ones((instances, 1), dtype=torch.uint8, device=dev)


def phase_ms(rank):
    """One more run with a device event around every launch (the round
    loop's timing hook): (phase 1 ms, phase 2 ms) summed over the rounds."""
    import torch
    from hbbft_amd import subset_sim
    ev = []
    rounds = subset_sim.run_rounds(rank, ev)
    torch.cuda.synchronize()
    tot = {"phase1": 0.0, "phase2": 0.0}
    for name, e0, e1 in ev:
        tot[name] += e0.elapsed_time(e1)
    return rounds, [tot["phase1"], tot["phase2"]]


def bench_subset(n, count, reps):
    import torch
    from hbbft_amd import subset_sim
    scn = scenario(n, count)
    dev = torch.device("cuda", 0)
    ok, dec = forced_plane(n, count * n, dev)
    rank = subset_sim.SubsetRank(scn, 0, ok, dec, max_out=8, bc_max_faults=4, ba_max_faults=4)
    rounds, ts = timed(lambda: subset_sim.run_rounds(rank), reps)
    ln = rank.out_len.cpu().numpy()
    seq = rank.out_seq.cpu().numpy()
    assert (ln == n + 1).all() and (seq[:, :, n] == subset_sim.SEQ_DONE).all(), \
        "an honest node did not output every contribution and Done"
    assert int(rank.fault_count.max()) == 0 and int(rank.bc.fault_count.max()) == 0
    r2, (p1, p2) = phase_ms(rank)
    assert r2 == rounds
    med = ts[len(ts) // 2]
    return {"what": "Subset", "n": n, "instances": count, "nodes": count * n,
            "sub_instances": count * n, "rounds": rounds, "bc_records": rank.bc_records,
            "ba_records": rank.ba_records, "ms_median": med, "ms_min": ts[0], "ms_max": ts[-1],
            "reps": reps, "phase1_ms": p1, "phase2_ms": p2,
            "phase_note": "device time of the launches of one further run, all rounds"}


def bench_broadcast(n, instances, reps):
    import torch
    from hbbft_amd.rbc_sim import StateMachineRank, honest_tensors, run_rounds
    dev = torch.device("cuda", 0)
    ok, dec = forced_plane(n, instances, dev)
    sm = StateMachineRank(n, instances, 1, honest_tensors(n, [i % n for i in range(instances)], dev),
                          0, 1, device=0, max_out=8, max_faults=4, ok=ok, dec=dec)
    rounds, ts = timed(lambda: run_rounds([sm]), reps)
    assert bool((sm.output_root == 0).all()), "an honest node did not decide"
    return {"what": "Broadcast alone (rbc_sim)", "n": n, "instances": instances,
            "nodes": instances * n, "rounds": rounds, "records": sm.records,
            "ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1], "reps": reps}


def bench_ba(n, instances, reps):
    from hbbft_amd import ba_sim
    rng = random.Random("subset_bench/ba/%d" % n)
    scn = ba_sim.Scenario(n, [ba_sim.Instance(n, [1] * n,
                                              coin_bits=[rng.randrange(2) for _ in range(COINS)])
                              for _ in range(instances)], COINS)
    rank = ba_sim.BaRank.from_scenario(scn, 0, max_out=8, max_faults=4)
    rounds, ts = timed(lambda: ba_sim.run_rounds(rank), reps)
    dec, _ = rank.decisions()
    assert (dec == 1).all(), "a unanimous run did not decide true"
    return {"what": "BinaryAgreement alone (ba_sim, every input true, form auto)", "n": n,
            "instances": instances, "nodes": instances * n, "rounds": rounds,
            "records": rank.records, "ms_median": ts[len(ts) // 2], "ms_min": ts[0],
            "ms_max": ts[-1], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sm-rows", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_sim.json"))
    a = ap.parse_args()
    import torch
    rows = []
    for n, count in SHAPES:
        for row in (bench_subset(n, count, a.reps), bench_broadcast(n, count * n, a.reps),
                    bench_ba(n, count * n, a.reps)):
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = {"tool": "tools/subset_bench.py", "device": torch.cuda.get_device_name(0),
           "note": "one process, one session; ms per run = every round of the batch until "
                   "quiescence, launches and read-backs included, median of reps",
           "rows": rows}
    if a.sm_rows:
        doc["sm_bench_unflagged"] = {
            "note": "tools/sm_bench.py (hbrbc_sm_round without HBRBC_SM_SUBSET): the parent "
                    "commit's library twice, this change's once, one session",
            "rows": [json.loads(l) for l in open(a.sm_rows) if l.strip().startswith("{")]}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
