"""Subset on the GPU (hbbft_amd/subset_sim.py, hbbft_amd/csrc/subset_sim.hip,
HBRBC_SM_SUBSET in sim.hip) against the host restatement.

Every scenario runs twice: through the two round kernels, and through
hbbft_amd/subset.py nodes driven in the same schedule by tests/subset_net.py.
Every node's output sequence (proposers and payload bytes, then Done), every
per-proposer decision and decision epoch, both fault logs (blamed node and
FaultKind, in order), the round count and the per-round record totals of both
protocols must be EQUAL.

Shapes (subset_net.GPU_SHAPES): N = 1, 2 (f = 0); honest N = 4, 7; N = 4, 7,
10 with 1..f dead nodes (the crossing, propose(false), rejections that write
DROPPED, agreements that outlive the broadcasts); N = 7, 10 with a seeded
mixture of the existing adversary roles; N = 33 with a dead node in each mask
word.  Further: the crossing with a higher proposer's records still waiting,
the real coin's tables, the flag of the broadcast kernel by itself, repeated
runs and the driver's rejections.
"""
import json
import os

import numpy as np
import pytest
import torch

import subset_net as sn
import virtual_net as vn
from hbbft_amd import ba_sim, rbc_sim, subset_sim
from hbbft_amd.binary_agreement import CoinSlotError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def assert_equal_to_host(scn, run, host):
    n = scn.n
    for i, h in enumerate(host):
        for j in range(n):
            where = (n, i, j)
            assert run.outputs[(i, j)] == h.outputs[j], where
            assert run.accepted[(i, j)] == h.accepted[j], where
            for p in range(n):
                assert run.decisions[(i, j, p)] == h.decisions[(j, p)], where + (p,)
                assert run.decision_epochs[(i, j, p)] == h.decision_epochs[(j, p)], where + (p,)
                assert run.bc_faults[(i, j, p)] == h.bc_faults[(j, p)], where + (p,)
                assert run.ba_faults[(i, j, p)] == h.ba_faults[(j, p)], where + (p,)
    rounds = max(h.rounds for h in host)
    assert run.rounds == rounds
    assert run.bc_emitted == [sum(h.bc_emitted[r] for h in host if r < h.rounds)
                              for r in range(rounds)]
    assert run.ba_emitted == [sum(h.ba_emitted[r] for h in host if r < h.rounds)
                              for r in range(rounds)]


@pytest.mark.parametrize("n,kind,count", sn.GPU_SHAPES)
def test_matches_host(n, kind, count):
    scn, host = sn.scenario(n, kind, count)
    run = subset_sim.run(scn)
    assert_equal_to_host(scn, run, host)
    if kind != "faulty":   # nobody misbehaves visibly
        assert not any(run.bc_faults.values()) and not any(run.ba_faults.values())


def test_scenarios_reach_what_they_are_for():
    """The dead-node shapes cross, vote false, reject and let the agreements
    outlive the broadcasts; the faulty ones log faults of both protocols and
    queue messages of a future epoch (else the equalities above say little)."""
    bc_kinds, ba_kinds, queued = set(), set(), 0
    for n, kind, count in sn.GPU_SHAPES:
        _, host = sn.scenario(n, kind, count)
        for h in host:
            bc_kinds |= {k for fl in h.bc_faults.values() for _, k in fl}
            ba_kinds |= {k for fl in h.ba_faults.values() for _, k in fl}
            queued = max(queued, h.max_queued_ahead)
            if kind.startswith("dead"):
                assert h.crossings and h.false_votes and h.rejected
                assert max(r for r, c in enumerate(h.ba_emitted) if c) >= \
                    max(r for r, c in enumerate(h.bc_emitted) if c) + 2
    assert "InvalidProof" in bc_kinds and {"DuplicateBVal", "DuplicateAux"} <= ba_kinds
    assert queued >= 1


def test_crossing_before_a_higher_proposers_records():
    """In one round of one node the accepted count reaches N - f on a proposer
    p* while a higher proposer still has unhandled agreement records and no
    estimate: propose(false) must precede those records (asserted of the host
    run first; subset_net.scenario_late_crossing says why the case takes one
    fault more than f)."""
    scn, host = sn.scenario_late_crossing(7, sn.LATE_CROSSING_START)
    late = [c for c in host[0].crossings if c[3]]
    assert late and all(q > p for _, _, p, waiting in late for q in waiting)
    assert_equal_to_host(scn, subset_sim.run(scn), host)


def test_runs_repeat_and_simulate_returns_the_results():
    """A second run of the same rank object equals the first (reset restores
    the dead nodes' presets); simulate() returns run()'s results."""
    scn, host = sn.scenario(7, "dead", 6)
    ok, dec, payloads, _ = rbc_sim.data_plane(scn.rbc_scenario(), 0)
    rank = subset_sim.SubsetRank(scn, 0, ok, dec)
    first = subset_sim.SubsetRun(rank, subset_sim.run_rounds(rank), payloads)
    assert_equal_to_host(scn, first, host)
    again = subset_sim.SubsetRun(rank, subset_sim.run_rounds(rank), payloads)
    for attr in ("outputs", "accepted", "decisions", "decision_epochs", "bc_faults", "ba_faults",
                 "rounds", "bc_emitted", "ba_emitted", "bc_records", "ba_records"):
        assert getattr(again, attr) == getattr(first, attr), attr
    res = subset_sim.simulate(scn)
    assert res == (first.outputs, first.accepted, first.bc_faults, first.ba_faults,
                   first.decisions, first.decision_epochs, first.rounds, first.bc_emitted,
                   first.ba_emitted)


def test_limits_raise():
    scn, host = sn.scenario(7, "faulty", 12)
    with pytest.raises(RuntimeError, match="more than 1 (broadcast|agreement) messages"):
        subset_sim.run(scn, max_out=1)
    assert max(len(fl) for h in host for fl in h.ba_faults.values()) > 1
    with pytest.raises(RuntimeError, match="agreement fault log overflow"):
        subset_sim.run(scn, ba_max_faults=1)


# ---- the real coin --------------------------------------------------------------
def _gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


def _stand_in_hashes(count):
    """H = [h] G2::one() for seeded scalars h, stand-ins for hash_g2(coin id)
    as in tests/test_ba_sim.py."""
    from hbbft_amd import threshold as T
    gen = next(x for x in _gold("compressed_vectors.json")["g2"] if x["name"] == "g2_valid_0")
    one = torch.from_numpy(np.frombuffer(bytes.fromhex(gen["u"]), np.uint8).copy()).view(1, 192)
    gtab = T.g2_points_prepare(one.to("cuda:0"))
    hs = [(0x5B5 + 613 * c + (1 << (131 + c))).to_bytes(32, "big") for c in range(count)]
    sc = torch.from_numpy(np.frombuffer(b"".join(hs), np.uint8).reshape(count, 32).copy())
    rows = torch.zeros(count, dtype=torch.int32, device="cuda:0")
    _, h192, _, st = T.g2_mul_prepared(gtab, 1, rows, sc.to("cuda:0"))
    assert st.cpu().tolist() == [0] * count
    return [bytes(v) for v in h192.cpu().numpy()]


def test_coin_plane_tables():
    """N = 4, one instance, two coin slots: the tables ba_sim.coin_plane
    computes over the count x n agreement instances drive the GPU run and the
    host run alike."""
    import random
    from hbbft_amd import keygen as K
    tr = _gold("keygen_vectors.json")["transcripts"][0]
    n, f = len(tr["polys"]), tr["t"]
    assert (n, f) == (4, 1)
    keys = K.sync_key_gen_network(f, [[bytes.fromhex(c) for c in p] for p in tr["polys"]])
    rng = random.Random("subset/coin_plane")
    inst = sn.make_instance(n, "faulty", rng)
    bad = next(j for j in range(n) if j in inst.faulty)
    inst.ba_role[bad] = ba_sim.BAD_COIN
    scn = subset_sim.Scenario(n, [inst], coins=2)
    share_ok, coin, info = ba_sim.coin_plane(scn.ba_scenario(), _stand_in_hashes(n * 2), keys)
    so = share_ok.cpu().numpy()
    assert so.shape == (n, 2, 2, n) and coin.shape == (n, 2)
    assert (so[:, :, 0, :] == 1).all() and (so[:, :, 1, :] == 0).all()
    assert bool((info["verified"] == 1).all())
    scn.set_tables(share_ok, coin)
    try:
        host = [sn.run_rounds(inst, sn._oracle(), scn.host_tables(0))]
    except CoinSlotError:   # the run needs a third coin: then the driver rejects it too
        with pytest.raises(RuntimeError, match="coin slot"):
            subset_sim.run(scn)
        return
    assert_equal_to_host(scn, subset_sim.run(scn), host)


# ---- HBRBC_SM_SUBSET by itself ----------------------------------------------
def _drive(sm, preset=None):
    """The broadcast rounds one by one, read back after each: (rounds, the
    out_count of every round)."""
    sm.reset()
    if preset is not None:
        preset(sm)
    counts = []
    for r in range(sm.max_rounds):
        sm.round(r)
        counts.append(sm.out_count.reshape(sm.count, sm.R).cpu().numpy().copy())
        emitted, flags = (int(v) for v in sm.hist[r].cpu().numpy())
        assert not flags
        sm.swap_local()
        if emitted == 0:
            return r + 1, counts
    raise AssertionError("no quiescence")


def _flag_instances(n=7):
    f = (n - 1) // 3
    corrupt = [rbc_sim.CORRUPT_ECHO if j < f else rbc_sim.HONEST for j in range(n)]
    two = [1 if j % 3 == 0 else 0 for j in range(n)]
    two[0] = 0
    return [rbc_sim.Instance(n, 2, [b"flag-honest"]),
            rbc_sim.Instance(n, 3, [b"flag-corrupt-echo"], role=corrupt),
            rbc_sim.Instance(n, 0, [b"flag-two-A", b"flag-two-B"], value_root=two),
            rbc_sim.Instance(n, n - 1, [b"flag-last-proposer"])]


def _rank(scn, flags=0):
    ok, dec, payloads, _ = rbc_sim.data_plane(scn, 0)
    sm = rbc_sim.StateMachineRank.from_scenario(scn, 0, 1, 0, 24, 64, ok, dec)
    sm.flags |= flags
    return sm, payloads


def _snapshot(sm):
    return [t.cpu().numpy().copy() for t in (sm.output_root, sm.fault_count, sm.faults, sm.hist)]


def test_flag_dropped_node_emits_nothing():
    """A node preset to DROPPED emits nothing in any round, logs nothing and
    keeps its mark -- as the proposer too (round 0); the others deliver."""
    n, d = 7, 6
    scn = rbc_sim.Scenario(n, _flag_instances(n))
    sm, _ = _rank(scn, subset_sim.SM_SUBSET)

    def preset(sm):
        sm.output_root[:, d] = subset_sim.DROPPED

    rounds, counts = _drive(sm, preset)
    assert rounds > 3
    assert all((c[:, d] == 0).all() for c in counts)
    root = sm.output_root.cpu().numpy()
    assert (root[:, d] == subset_sim.DROPPED).all()
    assert (sm.fault_count.cpu().numpy()[:, d] == 0).all()
    live = [j for j in range(n) if j != d]
    assert (root[:3][:, live] == 0).all()          # the others deliver root 0
    assert all((c[3] == 0).all() for c in counts)  # a dropped proposer: a silent instance
    assert (root[3][live] == rbc_sim.NONE).all()


def test_flag_decided_node_ignores_later_records():
    """Without the flag a decided node still handles what arrives: the
    CORRUPT_ECHO nodes' remaining Echoes (sent at 2f + 1 Readys, after the
    receivers decided) are logged as faults, and a duplicate Ready for another
    root injected after the run is logged by every node.  With the flag
    neither is: the ProposalState has dropped the Broadcast."""
    n = 7
    scn = rbc_sim.Scenario(n, _flag_instances(n))
    plain, _ = _rank(scn)
    flagged, _ = _rank(scn, subset_sim.SM_SUBSET)
    rp, _ = _drive(plain)
    rf, _ = _drive(flagged)
    assert (plain.output_root.cpu().numpy() == flagged.output_root.cpu().numpy()).all()
    lp, lf = plain.fault_logs(), flagged.fault_logs()
    # the corrupt-echo instance: nodes 0 and 1 corrupt, their honest right-hand
    # nodes 5 and 6 get the remaining Echoes a round after they decided
    late = [k for k in lp if k[0] == 1 and len(lp[k]) > len(lf[k])]
    assert sorted(late) == [(1, 5), (1, 6)]
    assert all(lp[k][:len(lf[k])] == lf[k] and
               set(lp[k][len(lf[k]):]) <= {(0, "InvalidProof"), (1, "InvalidProof")} for k in late)
    # one more round whose inbox holds one record: sender 1's Ready for root 1
    # of the two-root instance, to everybody
    for sm, r in ((plain, rp), (flagged, rf)):
        sm.inbox.zero_()
        sm.inbox_count.zero_()
        sm.inbox[0, 2, 1, 0, 0] = 2 | (1 << 8)
        sm.inbox[0, 2, 1, 0, 1:] = -1
        sm.inbox_count[0, 2, 1] = 1
        before = sm.fault_count.cpu().numpy().copy()
        sm.round(r)
        sm.extra = sm.fault_count.cpu().numpy() - before
        assert int(sm.hist[r, 0]) == 0
    decided = plain.output_root.cpu().numpy()[2] != rbc_sim.NONE
    assert decided.all()
    others = np.arange(n) != 1
    assert (plain.extra[2][others] == 1).all()                # MultipleReadys, logged
    assert plain.fault_logs()[(2, 0)][-1] == (1, "MultipleReadys")
    assert (flagged.extra == 0).all()


def test_without_the_flag_nothing_changes():
    """The same scenarios without the flag: the rank driven round by round is
    byte-identical to rbc_sim's own driver, whose results are the host's."""
    n = 7
    scn = rbc_sim.Scenario(n, _flag_instances(n))
    mine, payloads = _rank(scn)
    assert not mine.flags & subset_sim.SM_SUBSET
    rounds, _ = _drive(mine)
    theirs, _ = _rank(scn)
    assert rbc_sim.run_rounds([theirs]) == rounds
    for a, b in zip(_snapshot(mine), _snapshot(theirs)):
        assert a.tobytes() == b.tobytes()
    outputs, faults, sim_rounds = rbc_sim.simulate(scn, max_faults=64)
    assert sim_rounds == rounds and faults == mine.fault_logs()
    for i, inst in enumerate(scn.instances):
        outs, hfaults, hrounds = vn.run_rounds(inst, sn._oracle())
        for j in range(n):
            assert outputs[(i, j)] == (outs[j][0] if outs[j] else None)
            assert faults[(i, j)] == hfaults[j]
    assert rounds == max(vn.run_rounds(inst, sn._oracle())[2] for inst in scn.instances)
