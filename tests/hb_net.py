"""In-process test networks for hbbft_amd.honey_badger.HoneyBadger.

TEST INFRASTRUCTURE: two small drivers of the host restatement.

`run_rounds` is the schedule of the GPU state machine (hbbft_amd/hb_sim.py):
the synchronous rounds of tests/subset_net.py -- a node first handles every
broadcast record addressed to it, then every agreement record, each in
(proposer, sender, emission) order -- and then every DecryptionShare record of
the round in the same order (not its own).  Every record goes through
`HoneyBadger.handle_message`, so a node whose batch is out drops what is left
of the round as late.  What leaves a node passes the role transforms of
subset_net for the Subset's messages and the hb_role of the node for its
shares: SILENT sends none, BAD_SHARE its variant-1 share, TWICE every share
twice, STRAY a variant-1 share for every proposer at the start of round 1 and
of the round after it saw Done.  A dead node is absent.

`run_random` delivers one seeded random pending message per crank over several
epochs: the asynchronous network of the reference's tests/honey_badger.rs,
whose properties `check_properties` asserts.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ba_net  # noqa: E402
import subset_net as sn  # noqa: E402
import virtual_net as vn  # noqa: E402
from hbbft_amd import broadcast as bcm  # noqa: E402
from hbbft_amd import honey_badger as hbm  # noqa: E402
from hbbft_amd import subset as sub  # noqa: E402
from hbbft_amd.binary_agreement import CoinTable  # noqa: E402

# hbbft_amd.hb_sim's constants (that module needs torch; this one does not)
HONEST, SILENT, BAD_SHARE, TWICE, STRAY = range(5)
NONE = 0xFF
DONE = "Done"


class Result(sn.Result):
    """subset_net.Result (without crossings), and: batch {node: {proposer:
    bytes} or None}; batch_round {node: round or None}; hb_faults {(node,
    proposer): [(blamed, kind name)]}; hb_emitted: the share records that left
    the nodes, per round; what the run reached: postponed (shares purged by
    remove_invalid_shares), removed_at_done (faults logged for removed states),
    immediate_unverified, immediate_unexpected, and late_batches [(round, node,
    p*, [non-accepted proposers above p* with share records for the node in
    that round])]."""

    def __init__(self):
        super().__init__()
        self.batch, self.batch_round, self.hb_faults, self.hb_emitted = {}, {}, {}, []
        self.postponed = self.removed_at_done = 0
        self.immediate_unverified = self.immediate_unexpected = 0
        self.late_batches = []


def run_rounds(inst, backend, coin_tables=None, tables=None, max_rounds=256):
    """One hbbft_amd.hb_sim.Instance in synchronous rounds: a Result.
    coin_tables[p]: the CoinTable of proposer p's agreement (default: forced
    from the coin bits); tables[p][r]: the DecryptTables (default: forced,
    inst.host_tables())."""
    si = inst.subset
    n, epoch = inst.n, inst.epoch
    ids = list(range(n))
    if coin_tables is None:
        coin_tables = [CoinTable.forced(n, si.coin_bits[p]) for p in ids]
    if tables is None:
        tables = inst.host_tables()
    live = [j for j in ids if j not in si.dead]
    params = hbm.Params(0, inst.strategy, hbm.EncryptionSchedule.always() if inst.encrypted
                        else hbm.EncryptionSchedule.never())
    nodes = {j: hbm.HoneyBadger(j, ids, lambda e: tables, lambda e: coin_tables, params, epoch,
                                backend=backend) for j in live}
    res = Result()
    for j in ids:
        res.outputs[j], res.batch[j], res.batch_round[j] = [], None, None
        for p in ids:
            res.bc_faults[(j, p)], res.ba_faults[(j, p)], res.hb_faults[(j, p)] = [], [], []
    trees = {p: [vn.codeword_tree(backend, n, v) for v in si.broadcasts[p].values] for p in live}
    flip = set(si.flip)
    states, seen, done_round = {}, {j: 0 for j in ids}, {}
    rounds = 0

    def record(j, step, rec_p, bc_out, ba_out, hb_out, first_round=False):
        """Log the step's batch and faults; file its messages, transformed by
        the node's roles, under their proposer."""
        es = states[j]
        for o in es.subset_outputs[seen[j]:]:
            res.outputs[j].append(DONE if o is sub.DONE else (o.proposer_id, o.value))
            if o is sub.DONE:
                done_round[j] = rounds
        seen[j] = len(es.subset_outputs)
        for b in step.output:
            assert res.batch[j] is None and b.epoch == epoch
            res.batch[j], res.batch_round[j] = dict(b.contributions), rounds
        for fl in step.fault_log:
            k = fl.kind
            if k.kind is hbm.HbFaultKind.SubsetFault:
                log = res.bc_faults if k.inner.protocol is sub.Protocol.Broadcast else \
                    res.ba_faults
                log[(j, rec_p)].append((fl.node_id, k.inner.kind.name))
            else:
                res.hb_faults[(j, k.proposer)].append((fl.node_id, k.name))
        for tm in step.messages:
            assert tm.message.epoch == epoch
            c = tm.message.content
            if c.subset is None:   # our share of proposer c.proposer_id's ciphertext
                role = inst.hb_role[j]
                if role == BAD_SHARE:
                    hb_out[j][c.proposer_id].append(1)
                elif role != SILENT:
                    hb_out[j][c.proposer_id] += [c.share] * (2 if role == TWICE else 1)
                continue
            p, c = c.subset.proposer_id, c.subset.content
            if c.protocol is sub.Protocol.Agreement:
                ba_out[j][p] += ba_net.leaving(n, j, si.ba_role[j], flip, si.ahead,
                                               [tm.target.message(c.msg)])
                continue
            role = si.broadcasts[p].role[j]
            msg = c.msg
            if role == sn.BC_SILENT and not first_round:
                continue
            if msg.kind == bcm.Message.ECHO:
                if role == sn.BC_WITHHOLD_ECHO:
                    continue
                if role == sn.BC_CORRUPT_ECHO:
                    msg = bcm.Message.echo(sn._tampered(msg.payload))
            bc_out[j][p].append(tm.target.message(msg))

    def fresh():
        return tuple({j: {p: [] for p in ids} for j in ids} for _ in range(3))

    def totals(bc_out, ba_out, hb_out, first_round=False):
        bc = 0
        for j in ids:
            for p in ids:
                msgs = bc_out[j][p]
                if first_round and j == p and j in nodes:
                    bc += 1 + sum(1 for tm in msgs if tm.message.kind != bcm.Message.VALUE)
                else:
                    bc += len(msgs)
        res.bc_emitted.append(bc)
        res.ba_emitted.append(sum(len(ba_out[j][p]) for j in ids for p in ids))
        res.hb_emitted.append(sum(len(hb_out[j][p]) for j in ids for p in ids))
        return bc + res.ba_emitted[-1] + res.hb_emitted[-1]

    def hb_msg(p, protocol, msg):
        return hbm.Message(epoch, hbm.Content(subset=sub.Message(p, sub.Content(protocol, msg))))

    # round 0: HoneyBadger::propose with the scenario's Values
    bc_out, ba_out, hb_out = fresh()
    for j in live:
        bi = si.broadcasts[j]

        def proof(c, i, t, j=j):
            pr = trees[j][c].proof(i)
            return sn._tampered(pr) if t else pr

        def broadcast(bc, bi=bi, j=j, proof=proof):
            bc.value_sent = True
            step = bcm.Step()
            for i in ids:
                if i != j and bi.value_root[i] != NONE:
                    step.messages.append(bcm.Target.node(i).message(
                        bcm.Message.value(proof(bi.value_root[i], i, bi.value_tamper[i]))))
            return step.join(bc._handle_value(j, proof(bi.value_root[j], j, bi.value_tamper[j])))

        states[j] = nodes[j]._epoch_state_mut(epoch)
        record(j, nodes[j].propose_with(broadcast), j, bc_out, ba_out, hb_out, first_round=True)
    rounds = 1
    emitted = totals(bc_out, ba_out, hb_out, first_round=True)
    while emitted:
        if rounds >= max_rounds:
            raise sn.NoQuiescence("no quiescence in %d rounds" % max_rounds)
        nbc, nba, nhb = fresh()
        for r in live:
            if inst.hb_role[r] == STRAY and (rounds == 1 or done_round.get(r) == rounds - 1):
                for p in ids:
                    nhb[r][p].append(1)
        for r in live:
            node, es = nodes[r], states[r]
            for p in ids:   # phase 1: the broadcast records
                for s in ids:
                    if s == r:
                        continue
                    for tm in bc_out[s][p]:
                        if tm.target.contains(r):
                            record(r, node.handle_message(
                                s, hb_msg(p, sub.Protocol.Broadcast, tm.message)), p,
                                nbc, nba, nhb)
            for p in ids:   # phase 2: the agreement records
                for s in ids:
                    if s == r:
                        continue
                    for m, to in ba_out[s][p]:
                        if r in to:
                            record(r, node.handle_message(
                                s, hb_msg(p, sub.Protocol.Agreement, m)), p, nbc, nba, nhb)
            for p in ids:   # phase 3: the share records
                for s in ids:
                    if s == r:
                        continue
                    for share in hb_out[s][p]:
                        had_batch = res.batch[r] is not None
                        st = es.decryption.get(p)
                        with_ct = isinstance(st, hbm.ThresholdDecrypt) and \
                            st.ciphertext is not None
                        step = node.handle_message(s, hbm.Message(epoch, hbm.Content(
                            proposer_id=p, share=share)))
                        for fl in step.fault_log:
                            if fl.kind.kind is hbm.HbFaultKind.UnexpectedDecryptionShare:
                                res.immediate_unexpected += 1
                            elif with_ct and fl.kind.inner is \
                                    hbm.TdFaultKind.UnverifiedDecryptionShareSender:
                                res.immediate_unverified += 1
                        record(r, step, p, nbc, nba, nhb)
                        if not had_batch and res.batch[r] is not None:
                            above = sorted(q for q in ids if q > p and q not in es.accepted_ids
                                           and any(hb_out[t][q] for t in ids if t != r))
                            res.late_batches.append((rounds, r, p, above))
        bc_out, ba_out, hb_out = nbc, nba, nhb
        emitted = totals(bc_out, ba_out, hb_out)
        rounds += 1
    res.rounds = rounds
    for j in ids:
        res.accepted[j] = set()
        es = states.get(j)
        for p in ids:
            st = es.subset.proposal_states[p] if es is not None else None
            res.decisions[(j, p)] = None if st is None or st.decision is None else int(st.decision)
            res.decision_epochs[(j, p)] = None if st is None else st.decision_epoch
            if st is not None:
                res.max_queued_ahead = max(res.max_queued_ahead, st.max_queued_ahead)
                if st.accepted():
                    res.accepted[j].add(p)
    # what the run reached, from the logs: a purge is an Unverified fault that
    # no share record of that moment explains; a removal an Unexpected one
    unv = sum(1 for fl in res.hb_faults.values() for _, k in fl
              if k == "DecryptionFault(UnverifiedDecryptionShareSender)")
    unx = sum(1 for fl in res.hb_faults.values() for _, k in fl
              if k == "UnexpectedDecryptionShare")
    res.postponed = unv - res.immediate_unverified
    res.removed_at_done = unx - res.immediate_unexpected
    res.done_round = dict(done_round)
    res.nodes = nodes
    return res


def run_random(n, epochs, proposals, tables, coin_tables, params, dead, rng, backend,
               max_cranks=4000000):
    """Honest nodes over an asynchronous network, `epochs` epochs: every crank
    delivers one pending message picked by `rng`; a node proposes
    proposals[e][j] for epoch e as soon as it reaches it.  tables(e) /
    coin_tables(e): the epoch's DecryptTables and CoinTables.  Returns {node:
    [Batch]} of the live nodes."""
    ids = list(range(n))
    live = [j for j in ids if j not in dead]
    nodes = {j: hbm.HoneyBadger(j, ids, tables, coin_tables, params, backend=backend)
             for j in live}
    batches = {j: [] for j in live}
    pending = []

    def process(j, step):
        assert not step.fault_log, (j, step.fault_log)   # nobody misbehaves
        batches[j].extend(step.output)
        for tm in step.messages:
            pending.extend((j, r, tm.message) for r in live if r != j and tm.target.contains(r))
        nd = nodes[j]
        if step.output and nd.epoch < epochs and not nd.has_input:
            process(j, nd.propose(proposals[nd.epoch][j]))

    for j in live:
        process(j, nodes[j].propose(proposals[0][j]))
    cranks = 0
    while pending and not all(len(b) >= epochs for b in batches.values()):
        cranks += 1
        assert cranks <= max_cranks, "no termination in %d cranks" % max_cranks
        k = rng.randrange(len(pending))
        pending[k], pending[-1] = pending[-1], pending[k]
        s, r, m = pending.pop()
        process(r, nodes[r].handle_message(s, m))
    return batches


def check_properties(n, epochs, batches, plain):
    """tests/honey_badger.rs: every live node outputs the same batches, in
    epoch order; each has at least N - f contributions, each what its proposer
    proposed (plain[e][p])."""
    f = (n - 1) // 3
    first = next(iter(batches.values()))
    for j, bs in batches.items():
        assert [b.epoch for b in bs[:epochs]] == list(range(epochs)), (j, bs)
        assert bs[:epochs] == first[:epochs], (j, bs, first)
    for b in first[:epochs]:
        assert len(b.contributions) >= n - f, b
        for p, v in b.contributions.items():
            assert v == bytes(plain[b.epoch][p]), (b.epoch, p)


# ---- seeded scenarios (shared by the CPU and the GPU tests) -----------------
HB_ROLES = (SILENT, BAD_SHARE, TWICE, STRAY)
_cache = {}


def make_instance(n, kind, rng, tag=0, force=None):
    """One hbbft_amd.hb_sim.Instance over subset_net.make_instance(n, kind):
    encryption and strategy drawn per instance (force: (encrypted, strategy));
    in a "faulty" one the Subset's faulty nodes also get a seeded hb_role, and
    a faulty proposer may send a ciphertext that does not deserialise or does
    not verify, or a contribution that does not deserialise."""
    from hbbft_amd import hb_sim
    si = sn.make_instance(n, kind, rng, tag)
    encrypted, strategy = force if force is not None else (rng.random() < 0.7, rng.randrange(2))
    hb_role = [HONEST] * n
    ct_state = [[0] * len(b.values) for b in si.broadcasts]
    undes = [[0] * len(b.values) for b in si.broadcasts]
    plain = [[b"P-%d-%d-%d-%d" % (n, tag, p, r) for r in range(len(b.values))]
             for p, b in enumerate(si.broadcasts)]
    max_faulty = None
    if kind == "faulty":
        for j in sorted(si.faulty):
            hb_role[j] = rng.choice(HB_ROLES + (HONEST,))
            how = rng.randrange(6)
            for r in range(len(ct_state[j])):
                if how in (1, 2):
                    ct_state[j][r] = how
                elif how == 3:
                    undes[j][r] = 1
    elif kind == "dead" and len(si.faulty) < (n - 1) // 3:
        # a live STRAY node beside the dead ones, while that stays within f:
        # its shares for a dead proposer wait in states that Done removes
        hb_role[rng.choice([j for j in range(n) if j not in si.dead])] = STRAY
    elif kind == "late_crossing":   # (f + 1 faults, as subset_net's: see scenario_late_batch)
        max_faulty = (n - 1) // 3 + 1
        bad = sorted(si.faulty - si.dead)
        if bad:
            hb_role[rng.choice(bad)] = STRAY
    return hb_sim.Instance(si, tag, encrypted, strategy, hb_role, ct_state, undes, plain,
                           max_faulty=max_faulty)


def scenario(n, kind, count, seed=0, queue_epochs=4, want=None, start=0, tries=None):
    """(Scenario, [Result]) of `count` seeded instances of `kind`, each one's
    host run included, as subset_net.scenario: only instances whose host run
    stays inside the queue ring and the coin slots (and for which `want(res)`
    holds) are taken.  Every scenario's first instances are forced to
    (encrypted, Incremental), (plain, AllAtEnd) and (encrypted, AllAtEnd), so
    each mixes both; the fourth instance of a faulty scenario is the first
    try, encrypted, that reaches what _NEEDS names."""
    import random
    from hbbft_amd import hb_sim
    from hbbft_amd.binary_agreement import CoinSlotError
    key = (n, kind, count, seed, queue_epochs, want, start)
    if key not in _cache:
        insts, results = [], []
        for t in range(start, start + (40 * count if tries is None else tries)):
            # (subset_net.scenario's generator: the Subset instance of try t is
            # the one tests/test_subset_sim.py runs; the draws for this layer
            # follow it)
            rng = random.Random("subset/%d/%s/%d/%d" % (n, kind, seed, t))
            force = {0: (True, hbm.INCREMENTAL), 1: (False, hbm.ALL_AT_END),
                     2: (True, hbm.ALL_AT_END)}.get(len(insts))
            need = _NEEDS.get((n, kind, len(insts)))
            if count == 1 or need:
                force = (True, hbm.INCREMENTAL)
            inst = make_instance(n, kind, rng, t, force)
            try:
                res = run_rounds(inst, sn._oracle())
            except (CoinSlotError, sn.NoQuiescence):
                continue
            if need and not getattr(res, need):
                continue
            if res.max_queued_ahead <= queue_epochs and (want is None or want(res)):
                insts.append(inst)
                results.append(res)
                if len(insts) == count:
                    break
        assert len(insts) == count, "too few %s instances at n=%d: %d of %d" % (
            kind, n, len(insts), count)
        _cache[key] = (hb_sim.Scenario(n, insts, sn.COINS, queue_epochs), results)
    return _cache[key]


# (n, kind, position) -> the Result counter that instance must have raised: a
# share for a proposer that Done has rejected (it takes a STRAY node, a rejected
# proposer and a batch that waits), and a tampered share that arrives after the
# ciphertext and before f + 1 valid ones (a BAD_SHARE node of a low index)
_NEEDS = {(10, "faulty", 3): "immediate_unexpected", (7, "faulty", 3): "immediate_unverified"}


def has_late_batch(res):
    """A node's batch left in step (b) at a proposer p* below a non-accepted
    proposer that still had share records for the node in that round."""
    return any(above for _, _, _, above in res.late_batches)


def scenario_late_batch():
    """One instance in which a node's batch leaves in step (b) at a proposer
    p* below a non-accepted proposer that has share records for the node in
    that round.  Such records come from a STRAY node only, sent in the round
    after it saw Done, so they arrive two rounds after its Done -- and with at
    most f dead or faulty nodes every live node sees Done in the same round t
    (subset_net.scenario_late_crossing says why all cross together; the rest
    of the Subset is as symmetric) and has every share by round t + 1, a round
    too early.  The case therefore takes the Subset instance of
    subset_net.LATE_CROSSING_START (N = 7, the last node dead, f more faulty
    nodes), in which node 3 sees Done a round after the others, AllAtEnd and
    encryption, so that node 3's shares leave a round late; node 0 is STRAY,
    nodes 1, 2 and 4 SILENT, and so node 5 holds f shares per proposer until
    node 3's arrive together with node 0's stray ones: its batch leaves at p*
    = 5, and the record for the dead proposer 6 is dropped with the epoch.
    Nothing but the equality of the GPU and the host run is asserted about
    such a run."""
    import random
    from hbbft_amd import hb_sim
    key = "late_batch"
    if key not in _cache:
        n, t = 7, sn.LATE_CROSSING_START
        rng = random.Random("subset/%d/%s/%d/%d" % (n, "late_crossing", 0, t))
        si = sn.make_instance(n, "late_crossing", rng, t)
        role = [STRAY, SILENT, SILENT, HONEST, SILENT, HONEST, HONEST]
        inst = hb_sim.Instance(si, t, True, hbm.ALL_AT_END, role, max_faulty=n)
        res = run_rounds(inst, sn._oracle())
        assert res.max_queued_ahead <= 4
        _cache[key] = (hb_sim.Scenario(n, [inst], sn.COINS, 4), [res])
    return _cache[key]


# the seeded scenarios of tests/test_hb_sim.py: (n, kind, count)
GPU_SHAPES = [(1, "honest", 2), (2, "honest", 2), (4, "honest", 8), (7, "honest", 8),
              (4, "dead", 4), (7, "dead", 6), (10, "dead", 6), (7, "faulty", 12),
              (10, "faulty", 8), (33, "dead_two_words", 1)]
