"""In-process test networks for hbbft_amd.subset.Subset.

TEST INFRASTRUCTURE: two small drivers of the host restatement.

`run_rounds` is the schedule of the GPU state machine (hbbft_amd/subset_sim.py):
synchronous rounds -- what a node emits in round t is delivered in round
t + 1 -- in which a node first handles every broadcast record addressed to it,
in (proposer, sender, emission) order, then every agreement record in the same
order.  Round 0 is `Subset::propose` of every live node.  What leaves a node
passes the role transforms of the two existing nets (tests/virtual_net.py
run_rounds for the broadcasts, tests/ba_net.py `leaving` for the agreements).
A dead node is absent: it never proposes, handles or sends.

`run_random` delivers one seeded random pending message per crank: the
asynchronous network of the reference's tests/subset.rs, whose properties
`check_properties` asserts.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ba_net  # noqa: E402
import virtual_net as vn  # noqa: E402
from hbbft_amd import broadcast as bcm  # noqa: E402
from hbbft_amd import subset as sub  # noqa: E402
from hbbft_amd.binary_agreement import CoinTable  # noqa: E402

# hbbft_amd.rbc_sim's constants (that module needs torch; this one does not)
NONE = 0xFF
BC_HONEST, BC_SILENT, BC_CORRUPT_ECHO, BC_WITHHOLD_ECHO = range(4)
DONE = "Done"


class NoQuiescence(AssertionError):
    pass


class Result:
    """outputs {node: [(proposer, value), ..., DONE]} in emission order;
    accepted {node: set of proposers}; decisions / decision_epochs
    {(node, proposer): value or None}; bc_faults / ba_faults {(node, proposer):
    [(blamed, FaultKind name)]}; rounds; bc_emitted / ba_emitted: the records
    that left the nodes, per round; crossings: [(round, node, p*, [higher
    proposers that still had unhandled agreement records of that round and no
    estimate])], one per node whose accepted count reached N - f while it
    handled an agreement record of p*."""

    def __init__(self):
        self.outputs, self.accepted = {}, {}
        self.decisions, self.decision_epochs = {}, {}
        self.bc_faults, self.ba_faults = {}, {}
        self.rounds, self.bc_emitted, self.ba_emitted = 0, [], []
        self.crossings = []
        self.max_queued_ahead = 0
        self.false_votes = 0      # propose(false) calls that took effect
        self.rejected = 0         # (node, proposer) pairs completed with `false`


def _tampered(p):
    v = p.value()
    return type(p)(bytes([v[0] ^ 1]) + v[1:], p.index(), p.digests(), p.root_hash())


def run_rounds(inst, backend, tables=None, max_rounds=256):
    """One hbbft_amd.subset_sim.Instance in synchronous rounds: a Result.
    tables[p]: the CoinTable of proposer p's agreement (default: forced tables
    from inst.coin_bits)."""
    n = inst.n
    ids = list(range(n))
    if tables is None:
        tables = [CoinTable.forced(n, inst.coin_bits[p]) for p in ids]
    live = [j for j in ids if j not in inst.dead]
    nodes = {j: sub.Subset(j, ids, tables, backend=backend) for j in live}
    res = Result()
    for j in ids:
        res.outputs[j] = []
        for p in ids:
            res.bc_faults[(j, p)], res.ba_faults[(j, p)] = [], []
    trees = {p: [vn.codeword_tree(backend, n, v) for v in inst.broadcasts[p].values] for p in live}
    flip = set(inst.flip)

    def record(j, step, rec_p, rec_proto, bc_out, ba_out, first_round=False):
        """Log the step's outputs and faults; file its messages, transformed
        by the node's roles, under their proposer."""
        for o in step.output:
            res.outputs[j].append(DONE if o is sub.DONE else (o.proposer_id, o.value))
        for fl in step.fault_log:
            # (a fault comes from the handler of the record itself: propose()
            # of an agreement, the only cross-protocol call, logs none)
            assert fl.kind.protocol is rec_proto
            log = res.bc_faults if rec_proto is sub.Protocol.Broadcast else res.ba_faults
            log[(j, rec_p)].append((fl.node_id, fl.kind.kind.name))
        for tm in step.messages:
            p, c = tm.message.proposer_id, tm.message.content
            if c.protocol is sub.Protocol.Agreement:
                ba_out[j][p] += ba_net.leaving(n, j, inst.ba_role[j], flip, inst.ahead,
                                               [tm.target.message(c.msg)])
                continue
            role = inst.broadcasts[p].role[j]
            msg = c.msg
            if role == BC_SILENT and not first_round:
                continue
            if msg.kind == bcm.Message.ECHO:
                if role == BC_WITHHOLD_ECHO:
                    continue
                if role == BC_CORRUPT_ECHO:
                    msg = bcm.Message.echo(_tampered(msg.payload))
            bc_out[j][p].append(tm.target.message(msg))

    def fresh():
        return ({j: {p: [] for p in ids} for j in ids}, {j: {p: [] for p in ids} for j in ids})

    def totals(bc_out, ba_out, first_round=False):
        bc = 0
        for j in ids:
            for p in ids:
                msgs = bc_out[j][p]
                if first_round and j == p and j in nodes:
                    # the proposer's Values are one record with a recipient mask
                    bc += 1 + sum(1 for tm in msgs if tm.message.kind != bcm.Message.VALUE)
                else:
                    bc += len(msgs)
        res.bc_emitted.append(bc)
        res.ba_emitted.append(sum(len(ba_out[j][p]) for j in ids for p in ids))
        return bc + res.ba_emitted[-1]

    # round 0: Subset::propose with the scenario's Values (virtual_net.run_rounds)
    bc_out, ba_out = fresh()
    for j in live:
        bi = inst.broadcasts[j]

        def proof(c, i, t, j=j):
            pr = trees[j][c].proof(i)
            return _tampered(pr) if t else pr

        def broadcast(bc, bi=bi, j=j, proof=proof):
            bc.value_sent = True
            step = bcm.Step()
            for i in ids:
                if i != j and bi.value_root[i] != NONE:
                    step.messages.append(bcm.Target.node(i).message(
                        bcm.Message.value(proof(bi.value_root[i], i, bi.value_tamper[i]))))
            return step.join(bc._handle_value(j, proof(bi.value_root[j], j, bi.value_tamper[j])))

        record(j, nodes[j].propose_with(broadcast), j, sub.Protocol.Broadcast, bc_out, ba_out,
               first_round=True)
    rounds = 1
    emitted = totals(bc_out, ba_out, first_round=True)
    while emitted:
        if rounds >= max_rounds:
            raise NoQuiescence("no quiescence in %d rounds" % max_rounds)
        nbc, nba = fresh()
        for r in live:
            node = nodes[r]
            for p in ids:   # phase 1: the broadcast records
                for s in ids:
                    if s == r:
                        continue
                    for tm in bc_out[s][p]:
                        if tm.target.contains(r):
                            m = sub.Message(p, sub.Content(sub.Protocol.Broadcast, tm.message))
                            record(r, node.handle_message(s, m), p, sub.Protocol.Broadcast,
                                   nbc, nba)
            # phase 2: the agreement records
            todo = [(p, s, m) for p in ids for s in ids if s != r
                    for m, to in ba_out[s][p] if r in to]
            for k, (p, s, m) in enumerate(todo):
                before = node.count_accepted()
                waiting, could = [], set()
                if before == n - (n - 1) // 3 - 1:
                    could = {q for q, st in node.proposal_states.items()
                             if st.state in (sub.ONGOING, sub.HAS_VALUE)
                             and st.agreement.can_propose()}
                    later = {q for q, _, _ in todo[k + 1:] if q > p}
                    waiting = sorted(could & later)
                step = node.handle_message(
                    s, sub.Message(p, sub.Content(sub.Protocol.Agreement, m)))
                record(r, step, p, sub.Protocol.Agreement, nbc, nba)
                if before < n - (n - 1) // 3 <= node.count_accepted():
                    res.crossings.append((rounds, r, p, waiting))
                    res.false_votes += len(could - {p})
        bc_out, ba_out = nbc, nba
        emitted = totals(bc_out, ba_out)
        rounds += 1
    res.rounds = rounds
    for j in ids:
        res.accepted[j] = set()
        for p in ids:
            st = nodes[j].proposal_states[p] if j in nodes else None
            res.decisions[(j, p)] = None if st is None or st.decision is None else int(st.decision)
            res.decision_epochs[(j, p)] = None if st is None else st.decision_epoch
            if st is not None:
                res.max_queued_ahead = max(res.max_queued_ahead, st.max_queued_ahead)
                if st.accepted():
                    res.accepted[j].add(p)
                if st.complete() and not st.result:
                    res.rejected += 1
    res.nodes = nodes
    return res


def run_random(n, proposals, tables, dead, rng, backend, max_cranks=2000000):
    """Honest nodes over an asynchronous network: every crank delivers one
    pending message picked by `rng`; the nodes in `dead` are absent.
    proposals[j]: node j's contribution.  Returns {node: [outputs]} of the
    live nodes, Contributions as (proposer, value) and DONE."""
    ids = list(range(n))
    live = [j for j in ids if j not in dead]
    nodes = {j: sub.Subset(j, ids, tables, backend=backend) for j in live}
    outputs = {j: [] for j in live}
    pending = []

    def process(j, step):
        assert not step.fault_log, (j, step.fault_log)   # nobody misbehaves
        for o in step.output:
            outputs[j].append(DONE if o is sub.DONE else (o.proposer_id, o.value))
        for tm in step.messages:
            pending.extend((j, r, tm.message) for r in live if r != j and tm.target.contains(r))

    for j in live:
        process(j, nodes[j].propose(proposals[j]))
    cranks = 0
    while pending and not all(nd.terminated() for nd in nodes.values()):
        cranks += 1
        assert cranks <= max_cranks, "no termination in %d cranks" % max_cranks
        k = rng.randrange(len(pending))
        pending[k], pending[-1] = pending[-1], pending[k]
        s, r, m = pending.pop()
        process(r, nodes[r].handle_message(s, m))
    return outputs


def check_properties(n, outputs, proposals):
    """tests/subset.rs: every live honest node outputs Done exactly once and
    last, all output the same set, of at least N - f contributions, each what
    its proposer proposed."""
    f = (n - 1) // 3
    sets = []
    for j, outs in outputs.items():
        assert outs and outs[-1] == DONE and outs.count(DONE) == 1, (j, outs)
        got = outs[:-1]
        assert len({p for p, _ in got}) == len(got), (j, got)
        sets.append(dict(got))
    assert all(s == sets[0] for s in sets), sets
    assert len(sets[0]) >= n - f, sets[0]
    for p, v in sets[0].items():
        assert v == bytes(proposals[p]), (p, v)


# ---- seeded scenarios (shared by the CPU and the GPU tests) -----------------
COINS = 8
BA_ROLES = (ba_net.SILENT, ba_net.TWO_FACED, ba_net.BAD_COIN, ba_net.REPLAY, ba_net.AHEAD)
_cache = {}


def _oracle():
    import oracle_backend
    return oracle_backend


def make_instance(n, kind, rng, tag=0):
    """One hbbft_amd.subset_sim.Instance.  kind: "honest"; "dead" (1..f dead
    nodes); "dead_two_words" (n > 32: two dead nodes, one in each word of the
    sender masks); "faulty" (up to f nodes, each with a seeded mixture of the
    existing roles: SILENT / CORRUPT_ECHO / WITHHOLD_ECHO in the broadcasts, a
    proposer that sends two codewords or withholds Values, SILENT / TWO_FACED
    / BAD_COIN / REPLAY / AHEAD 1 in the agreements); "late_crossing" (the
    last node dead and f more faulty nodes -- ONE MORE than the protocol
    tolerates, see scenario_late_crossing)."""
    from hbbft_amd import rbc_sim
    from hbbft_amd.subset_sim import Instance
    f = (n - 1) // 3
    dead, bad = set(), []
    if kind == "dead":
        dead = set(rng.sample(range(n), rng.randint(1, f)))
    elif kind == "faulty":
        bad = rng.sample(range(n), rng.randint(1, f))
    elif kind == "dead_two_words":   # (n > 32: one dead node in each mask word)
        dead = {rng.randrange(32), rng.randrange(32, n)}
    elif kind == "late_crossing":
        dead = {n - 1}
        bad = rng.sample(range(n - 1), f)
    ba_role = [ba_net.HONEST] * n
    for j in bad:
        ba_role[j] = rng.choice(BA_ROLES if kind == "faulty" else
                                (ba_net.TWO_FACED, ba_net.SILENT, ba_net.HONEST))
    flip = rng.sample(range(n), n // 2) if bad else ()
    broadcasts = []
    for p in range(n):
        vals = [b"S-%d-%d-%d-" % (n, tag, p) + bytes(rng.randrange(256)
                                                   for _ in range(rng.randrange(0, 40)))]
        role = [rbc_sim.HONEST] * n
        vr, vt = [0] * n, [0] * n
        for j in bad:
            role[j] = rng.choice([rbc_sim.HONEST, rbc_sim.SILENT, rbc_sim.CORRUPT_ECHO,
                                  rbc_sim.WITHHOLD_ECHO])
        if p in bad:
            how = rng.choice(["two", "withhold", "plain"])
            if how == "two":
                vals.append(b"T-%d-%d-%d" % (n, tag, p))
                for j in range(n):
                    vr[j] = rng.randrange(2)
                vr[p] = 0
            elif how == "withhold":
                for j in rng.sample(range(n), min(n - 1, f + 1)):
                    if j != p:
                        vr[j] = NONE
        broadcasts.append(rbc_sim.Instance(n, p, vals, vr, vt, role))
    return Instance(n, broadcasts, ba_role, flip, 1 if bad else 0,
                    [[rng.randrange(2) for _ in range(COINS)] for _ in range(n)], dead,
                    max_faulty=f + 1 if kind == "late_crossing" else None)


def scenario(n, kind, count, seed=0, queue_epochs=4, want=None, start=0, tries=None):
    """(Scenario, [Result]) of `count` seeded instances of `kind` with forced
    coin tables, each one's host run included.  Only instances whose host run
    stays inside the ring of `queue_epochs` and the COINS coin slots -- and for
    which `want(result)` holds, if given -- are taken; the full count must be
    found.  Try t draws from a generator of its own, so a search can start
    at a known `start`.  Cached: the host runs are computed once."""
    import random
    from hbbft_amd.binary_agreement import CoinSlotError
    from hbbft_amd.subset_sim import Scenario
    key = (n, kind, count, seed, queue_epochs, want, start)
    if key not in _cache:
        insts, results = [], []
        for t in range(start, start + (40 * count if tries is None else tries)):
            rng = random.Random("subset/%d/%s/%d/%d" % (n, kind, seed, t))
            inst = make_instance(n, kind, rng, t)
            try:
                res = run_rounds(inst, _oracle())
            except (CoinSlotError, NoQuiescence):
                continue
            if res.max_queued_ahead <= queue_epochs and (want is None or want(res)):
                insts.append(inst)
                results.append(res)
                if len(insts) == count:
                    break
        assert len(insts) == count, "too few %s instances at n=%d: %d of %d" % (
            kind, n, len(insts), count)
        _cache[key] = (Scenario(n, insts, COINS, queue_epochs), results)
    return _cache[key]


def has_late_crossing(res):
    """A node's accepted count reached N - f on a proposer p* while a higher
    proposer still had unhandled agreement records of that round and no
    estimate: its propose(false) precedes those records."""
    return any(waiting for _, _, _, waiting in res.crossings)


def scenario_late_crossing(n=7, start=0, tries=1):
    """One instance in which some node's crossing falls on a proposer p* while
    a higher proposer still has unhandled agreement records of that round and
    no estimate.  With at most f dead or faulty nodes the live honest nodes
    alone meet every threshold of every broadcast and of every agreement that
    starts unanimous, in the same round everywhere, so all of them cross in
    the same round and a proposal that has agreement records in that round has
    been delivered -- and so has an estimate -- at every one of them.  The
    case therefore takes ONE fault more than f (a dead node, f others): the
    nodes a TWO_FACED one lies to then cross a round after the others, whose
    propose(false) records are waiting.  Nothing but the equality of the GPU
    and the host run is asserted about such a run."""
    return scenario(n, "late_crossing", 1, want=has_late_crossing, start=start, tries=tries)


# the seeded scenarios of tests/test_subset_sim.py: (n, kind, count)
GPU_SHAPES = [(1, "honest", 2), (2, "honest", 2), (4, "honest", 8), (7, "honest", 8),
              (4, "dead", 4), (7, "dead", 6), (10, "dead", 6), (7, "faulty", 12),
              (10, "faulty", 8), (33, "dead_two_words", 1)]
LATE_CROSSING_START = 76   # the first try of scenario_late_crossing(7) that has the property
