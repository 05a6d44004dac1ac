"""In-process test networks for hbbft_amd.binary_agreement.BinaryAgreement.

TEST INFRASTRUCTURE (tests/virtual_net.py is Broadcast-specific): two small
drivers of the host restatement.

`RoundNet` / `run_rounds` is the schedule of the GPU state machine (hbbft_amd/ba_sim.py):
synchronous rounds -- what a node emits in round t is delivered in round
t + 1, each node handling its inbox in (sender index, emission order) -- with
the role transforms applied to what leaves a node.

`run_random` delivers one seeded random pending message per crank, to up to f
silent nodes among honest ones: the asynchronous network of the reference's
tests/binary_agreement.rs, whose properties (agreement, termination,
validity) `check_properties` asserts.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hbbft_amd.binary_agreement import BinaryAgreement, CoinTable, Message  # noqa: E402

# hbbft_amd.ba_sim's constants (that module needs torch; this one does not)
NONE = 0xFF
HONEST, SILENT, TWO_FACED, BAD_COIN, REPLAY, AHEAD, REPLAY_AHEAD = range(7)


class NoQuiescence(AssertionError):
    pass


def complement(m):
    """What a TWO_FACED node tells the recipients it lies to: b -> !b for a
    bool, {false} <-> {true} for a singleton Conf; both and Coin unchanged."""
    if m.kind == Message.COIN:
        return m
    if m.kind == Message.CONF:
        return Message(m.epoch, m.kind, m.value ^ 3 if m.value in (1, 2) else m.value, m.tampered)
    return Message(m.epoch, m.kind, m.value ^ 1, m.tampered)


def leaving(n, node, role, flip, ahead, tmsgs):
    """The records [(Message, [recipients])] that leave `node` for the
    messages of one step (all of them Target::all())."""
    others = [r for r in range(n) if r != node]
    out = []
    if role == SILENT:
        return out
    for tm in tmsgs:
        m = tm.message
        assert tm.target.all_except and not tm.target.ids
        m = Message(m.epoch + (ahead if role in (AHEAD, REPLAY_AHEAD) else 0), m.kind, m.value,
                    1 if role == BAD_COIN and m.kind == Message.COIN else m.tampered)
        if role == TWO_FACED:
            out.append((m, [r for r in others if r not in flip]))
            out.append((complement(m), [r for r in others if r in flip]))
        elif role in (REPLAY, REPLAY_AHEAD):
            out += [(m, others), (m, others)]
        else:
            out.append((m, others))
    return out


class RoundResult:
    def __init__(self):
        self.decisions, self.decision_epochs, self.faults = {}, {}, {}
        self.rounds, self.emitted = 0, []
        self.max_queued_ahead = 0   # the ring a GPU run of this instance needs


def run_rounds(n, inputs, table, role=None, flip=(), ahead=0, max_rounds=256):
    """One instance in synchronous rounds.  inputs[j]: 0 / 1 / NONE / None.
    Returns a RoundResult: decisions / decision_epochs {node: value or None},
    faults {node: [(blamed, FaultKind name)]}, rounds, emitted (records that
    left the nodes, per round)."""
    role = list(role) if role is not None else [HONEST] * n
    flip = set(flip)
    nodes = [BinaryAgreement(j, n, table) for j in range(n)]
    res = RoundResult()
    res.faults = {j: [] for j in range(n)}

    def record(j, st):
        res.faults[j].extend((fl.node_id, fl.kind.name) for fl in st.fault_log)
        return leaving(n, j, role[j], flip, ahead, st.messages)

    outbox = {j: [] for j in range(n)}
    for j in range(n):   # round 0: propose
        if inputs[j] is not None and inputs[j] != NONE:
            outbox[j] = record(j, nodes[j].propose(bool(inputs[j])))
    res.emitted.append(sum(len(v) for v in outbox.values()))
    rounds = 1
    while any(outbox.values()):
        if rounds >= max_rounds:
            raise NoQuiescence("no quiescence in %d rounds" % max_rounds)
        nxt = {j: [] for j in range(n)}
        for r in range(n):
            for s in range(n):
                if s == r:
                    continue
                for m, to in outbox[s]:
                    if r in to:
                        nxt[r].extend(record(r, nodes[r].handle_message(s, m)))
        outbox = nxt
        res.emitted.append(sum(len(v) for v in outbox.values()))
        rounds += 1
    res.rounds = rounds
    for j, nd in enumerate(nodes):
        res.decisions[j] = None if nd.decision is None else int(nd.decision)
        res.decision_epochs[j] = nd.decision_epoch
    res.max_queued_ahead = max(nd.max_queued_ahead for nd in nodes)
    return res


def run_scenario(scn, max_rounds=256):
    """hbbft_amd.ba_sim.Scenario through run_rounds: per instance a
    RoundResult, on the scenario's own coin tables."""
    return [run_rounds(scn.n, i.inputs, scn.host_table(r), i.role, i.flip, i.ahead, max_rounds)
            for r, i in enumerate(scn.instances)]


def run_random(n, inputs, table, silent, rng, max_cranks=200000):
    """One instance over an asynchronous network: every crank delivers one
    pending message picked by `rng`; the nodes in `silent` send nothing.
    Returns the nodes."""
    nodes = [BinaryAgreement(j, n, table) for j in range(n)]
    pending = []

    def process(j, st):
        assert not st.fault_log, (j, st.fault_log)   # nobody misbehaves visibly
        if j in silent:
            return
        for tm in st.messages:
            pending.extend((j, r, tm.message) for r in range(n) if r != j)

    for j in range(n):
        if inputs[j] is not None and inputs[j] != NONE:
            process(j, nodes[j].propose(bool(inputs[j])))
    cranks = 0
    while pending and not all(nodes[j].terminated() for j in range(n) if j not in silent):
        cranks += 1
        assert cranks <= max_cranks, "no termination in %d cranks" % max_cranks
        k = rng.randrange(len(pending))
        pending[k], pending[-1] = pending[-1], pending[k]
        s, r, m = pending.pop()
        process(r, nodes[r].handle_message(s, m))
    return nodes


def check_properties(decisions, inputs, honest):
    """Agreement, termination and validity among `honest` (tests/
    binary_agreement.rs): every honest node decided, all on one value, and
    that value was some honest node's input."""
    got = [decisions[j] for j in honest]
    assert all(d is not None for d in got), "termination: %r" % (got,)
    assert len(set(got)) == 1, "agreement: %r" % (got,)
    proposed = {int(bool(inputs[j])) for j in honest
                if inputs[j] is not None and inputs[j] != NONE}
    assert got[0] in proposed, "validity: %r not in %r" % (got[0], proposed)


class RoundNet:
    """The round model of hbbft_amd/ba_sim.py over host BinaryAgreement nodes
    (run_rounds), for a whole Scenario."""

    def __init__(self, scn, max_rounds=256):
        self.scn, self.max_rounds = scn, max_rounds

    def run(self):
        return run_scenario(self.scn, self.max_rounds)


# ---- seeded scenarios (shared by the CPU and the GPU tests) -----------------
KINDS = ["true", "false", "split", "random", "no_input", "silent", "two_faced", "bad_coin",
         "replay", "replay_ahead1", "replay_ahead2", "ahead1", "ahead2", "ahead1001", "mixture"]
COINS = 8
_cache = {}


def _instance(n, kind, rng):
    from hbbft_amd.ba_sim import Instance
    f = (n - 1) // 3
    inputs = [rng.randrange(2) for _ in range(n)]
    if kind == "true":
        inputs = [1] * n
    elif kind == "false":
        inputs = [0] * n
    elif kind == "split":
        inputs = [j % 2 for j in range(n)]
    role = [HONEST] * n
    flip, ahead = (), 0
    bad = rng.sample(range(n), rng.randint(1, f)) if f else []
    if kind == "no_input":
        for j in bad:
            inputs[j] = NONE
    elif kind == "mixture":
        for j in bad:
            role[j] = rng.choice([SILENT, TWO_FACED, BAD_COIN, REPLAY, AHEAD, REPLAY_AHEAD])
        ahead = rng.choice([1, 2])
        flip = rng.sample(range(n), n // 2)
    elif kind in ("silent", "two_faced", "bad_coin", "replay"):
        r = {"silent": SILENT, "two_faced": TWO_FACED, "bad_coin": BAD_COIN, "replay": REPLAY}[kind]
        for j in bad:
            role[j] = r
        flip = rng.sample(range(n), n // 2)
    elif "ahead" in kind:   # (replay_ahead: the duplicates land in the receivers' queues)
        for j in bad:
            role[j] = REPLAY_AHEAD if kind.startswith("replay") else AHEAD
        ahead = int(kind[kind.index("ahead") + 5:])
    return Instance(n, inputs, role, flip, ahead, [rng.randrange(2) for _ in range(COINS)])


def scenario(n, kind, count, seed=0, queue_epochs=4):
    """(Scenario, [RoundResult]) of `count` seeded instances of `kind` with
    forced coin tables, each one's host run included.  Only instances whose
    host run queues no message further ahead than the ring of `queue_epochs`
    are taken (the GPU state machine rejects the others; the rejection has a
    test of its own).  Cached: the host runs are computed once."""
    import random
    from hbbft_amd.ba_sim import Scenario
    key = (n, kind, count, seed, queue_epochs)
    if key not in _cache:
        rng = random.Random("%d/%s/%d" % (n, kind, seed))
        insts, results = [], []
        for _ in range(200):
            inst = _instance(n, kind, rng)
            one = Scenario(n, [inst], COINS, queue_epochs)
            res = run_rounds(n, inst.inputs, one.host_table(0), inst.role, inst.flip, inst.ahead)
            if res.max_queued_ahead <= queue_epochs:
                insts.append(inst)
                results.append(res)
                if len(insts) == count:
                    break
        assert len(insts) == count, "too few %s instances inside the ring at n=%d" % (kind, n)
        _cache[key] = (Scenario(n, insts, COINS, queue_epochs), results)
    return _cache[key]


__all__ = ["BinaryAgreement", "CoinTable", "Message", "run_rounds", "run_scenario", "run_random",
           "check_properties", "leaving", "complement", "NoQuiescence"]
