"""hbbft_amd/subset.py (the host restatement of the reference's src/subset/)
without a GPU, the broadcasts on the CPU oracle backend.

The reference's tests/subset.rs properties under an asynchronous network
(tests/subset_net.py run_random); ProposalState's transitions one by one; the
round model of the GPU state machine (subset_net.run_rounds) on its own; and
the seeded scenario generators of tests/test_subset_sim.py, which must find
their full counts inside the ring of queue_epochs = 4.
"""
import random

import pytest

import oracle_backend
import subset_net as sn
from hbbft_amd import subset as sub
from hbbft_amd.binary_agreement import CoinTable
from hbbft_amd.broadcast import Step, ValidatorSet


def _tables(n, rng, coins=8):
    return [CoinTable.forced(n, [rng.randrange(2) for _ in range(coins)]) for _ in range(n)]


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("n", [1, 2, 4, 5, 7])
def test_random_network_properties(n, seed):
    rng = random.Random("subset_cpu/%d/%d" % (n, seed))
    f = (n - 1) // 3
    dead = set(rng.sample(range(n), rng.randint(0, f)))
    proposals = [b"contribution-%d-%d-" % (n, j) + bytes(rng.randrange(256) for _ in range(j))
                 for j in range(n)]
    outputs = sn.run_random(n, proposals, _tables(n, rng), dead, rng, oracle_backend)
    assert set(outputs) == set(range(n)) - dead
    sn.check_properties(n, outputs, proposals)


def _state(n=4, our=0, proposer=1):
    return sub.ProposalState(our, ValidatorSet(range(n)), proposer,
                             CoinTable.forced(n, [1] * 8), backend=oracle_backend)


def _decides(value):
    def f(ba):
        ba.decision, ba.decision_epoch = value, ba.epoch
        s = Step()
        s.output.append(value)
        return s
    return f


def _delivers(value):
    def f(bc):
        s = Step()
        s.output.append(value)
        return s
    return f


def test_accepted_then_value_completes_with_the_output():
    st = _state()
    step = st.handle_agreement(_decides(True))
    assert st.state == sub.ACCEPTED and st.accepted() and not st.received() and not st.complete()
    assert not step.output and st.agreement is None and st.broadcast is not None
    step = st.handle_broadcast(_delivers(b"value"))
    assert st.state == sub.COMPLETE and st.result is True and step.output == [b"value"]
    assert st.accepted() and st.received() and st.complete()


def test_value_then_true_completes_with_the_output():
    st = _state()
    step = st.handle_broadcast(_delivers(b"value"))
    # propose(true) ran inline: the BVal is in the same step
    assert st.state == sub.HAS_VALUE and st.agreement.estimated is True and not step.output
    assert [tm.message.protocol for tm in step.messages] == [sub.Protocol.Agreement]
    step = st.handle_agreement(_decides(True))
    assert st.state == sub.COMPLETE and st.result is True and step.output == [b"value"]


def test_false_drops_the_broadcast_and_later_records_are_no_ops():
    st = _state()
    called = []
    step = st.handle_agreement(_decides(False))
    assert st.state == sub.COMPLETE and st.result is False and not step.output
    assert st.broadcast is None and st.agreement is None and not st.accepted()
    for content in (sub.Content(sub.Protocol.Broadcast, object()),
                    sub.Content(sub.Protocol.Agreement, object())):
        step = st.handle_message(2, content)
        assert not (step.output or step.messages or step.fault_log)
    step = st.handle_broadcast(lambda bc: called.append(bc))
    assert not called and not (step.output or step.messages or step.fault_log)
    assert not st.vote_false().messages
    # HasValue then false: the value is dropped too
    st = _state()
    st.handle_broadcast(_delivers(b"value"))
    step = st.handle_agreement(_decides(False))
    assert st.state == sub.COMPLETE and st.result is False and not step.output


def test_vote_false_only_without_an_estimate_in_epoch_0():
    st = _state()
    step = st.vote_false()
    assert st.agreement.estimated is False
    assert [(tm.message.msg.kind, tm.message.msg.value) for tm in step.messages] == [(0, 0)]
    again = st.vote_false()   # after an estimate
    assert not (again.messages or again.output or again.fault_log)
    st = _state()
    st.handle_broadcast(_delivers(b"value"))   # voted true
    step = st.vote_false()
    assert st.agreement.estimated is True and not step.messages
    st = _state()
    st.agreement.epoch = 1   # epoch > 0
    step = st.vote_false()
    assert st.agreement.estimated is None and not step.messages


def test_faults_are_wrapped_by_protocol():
    from hbbft_amd.binary_agreement import FaultKind as BaFault
    from hbbft_amd.broadcast import FaultKind as BcFault
    st = _state()
    step = st.handle_broadcast(lambda bc: Step.from_fault(3, BcFault.InvalidProof))
    assert [(f.node_id, f.kind.name) for f in step.fault_log] == \
        [(3, "BroadcastFault(InvalidProof)")]
    step = st.handle_agreement(lambda ba: Step.from_fault(2, BaFault.DuplicateAux))
    assert [(f.node_id, f.kind) for f in step.fault_log] == \
        [(2, sub.SubsetFault(sub.Protocol.Agreement, BaFault.DuplicateAux))]


@pytest.mark.parametrize("n,kind,count", [s for s in sn.GPU_SHAPES if s[0] <= 10])
def test_round_model_and_generators(n, kind, count):
    """The seeded generators find their full count (scenario() asserts it), and
    the round model by itself gives what Subset promises: the live nodes that
    are not faulty output the same set, of at least N - f contributions, each
    one its proposer's first value unless the proposer sent two, then Done."""
    scn, host = sn.scenario(n, kind, count)
    assert scn.count == count and len(host) == count
    f = (n - 1) // 3
    for inst, res in zip(scn.instances, host):
        good = [j for j in range(n) if j not in inst.faulty]
        sets = []
        for j in good:
            outs = res.outputs[j]
            assert outs and outs[-1] == sn.DONE and outs.count(sn.DONE) == 1, (n, kind, j, outs)
            sets.append(dict(outs[:-1]))
            assert set(sets[-1]) == res.accepted[j]
        assert all(s == sets[0] for s in sets) and len(sets[0]) >= n - f
        for p, v in sets[0].items():
            assert v in inst.broadcasts[p].values and (p in inst.faulty or
                                                       v == inst.broadcasts[p].values[0])
        for j in inst.dead:
            assert res.outputs[j] == [] and not res.accepted[j]
        assert res.max_queued_ahead <= scn.queue_epochs
        assert res.rounds == len(res.bc_emitted) == len(res.ba_emitted)
        assert res.bc_emitted[-1] + res.ba_emitted[-1] == 0


def test_dead_nodes_reach_the_coupling_rules():
    """The dead-node scenarios are there for the crossing, propose(false),
    rejections and agreements that outlive the broadcasts: they have them."""
    for n, kind, count in [s for s in sn.GPU_SHAPES if s[1] == "dead"]:
        _, host = sn.scenario(n, kind, count)
        for res in host:
            assert res.crossings and res.false_votes and res.rejected
            last_bc = max(r for r, c in enumerate(res.bc_emitted) if c)
            last_ba = max(r for r, c in enumerate(res.ba_emitted) if c)
            assert last_ba >= last_bc + 2, (res.bc_emitted, res.ba_emitted)


def test_late_crossing_scenario_has_its_property():
    scn, host = sn.scenario_late_crossing(7, sn.LATE_CROSSING_START)
    late = [c for c in host[0].crossings if c[3]]
    assert late and all(q > p for _, _, p, waiting in late for q in waiting)
    # and with no more than f faults the search finds none (the reason the
    # case needs f + 1: see scenario_late_crossing)
    for n, kind, count in sn.GPU_SHAPES:
        if n <= 10:
            assert not any(sn.has_late_crossing(r) for r in sn.scenario(n, kind, count)[1])
