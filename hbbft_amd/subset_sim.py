"""Subset on the GPU: per node N broadcasts and N agreements, in rounds.

Control plane.  A round has two phases.  Phase 1 is `hbrbc_sm_round`
(hbbft_amd/csrc/sim.hip) over count x n broadcast instances -- instance (i, p)
at index i n + p, proposer p -- with HBRBC_SM_SUBSET: a node whose proposal
state has dropped the Broadcast (it output, or the agreement said `false`:
output_root != NONE) handles nothing, and a node that decides stops taking
records in that round.  Phase 2 is `hbrbc_subset_round` (hbbft_amd/csrc/
subset_sim.hip): one thread per (instance, node) runs the reference's
subset/subset.rs and subset/proposal_state.rs over the BinaryAgreement
handlers of ba_node.hpp -- a broadcast that phase 1 delivered votes `true`,
the (N - f)-th accepted proposal votes `false` on every other agreement at
once, a `false` decision writes HBRBC_SM_DROPPED for phase 1, all complete
gives Done.  What a node emits in round t is delivered in round t + 1; round
0 is `Subset::propose` of every live node; a run ends with the first round in
which neither protocol emits a record.  The host restatement
hbbft_amd/subset.py, driven by tests/subset_net.py in the same schedule, is
the checker (tests/test_subset_sim.py).

Data plane.  `rbc_sim.data_plane` over the count x n codewords; the coin
tables are forced (coin_bits per proposer) or `ba_sim.coin_plane` over the
count x n agreement instances (Scenario.ba_scenario, set_tables).

Scenarios: per proposer an `rbc_sim.Instance` (a proposer that sends two
codewords, tampered proofs or no Value to some nodes; SILENT / CORRUPT_ECHO /
WITHHOLD_ECHO nodes; no injected broadcasts), per node an agreement role
(ba_sim), and dead nodes: a dead node never proposes and emits nothing in any
sub-protocol; all its proposal states start dropped.
"""
import numpy as np
import torch

from . import ba_sim, rbc_sim, rounds as shared
from .rounds import I32, U32, USIZE

NONE = 0xFF
DROPPED = 0xFE            # HBRBC_SM_DROPPED
DONE = "Done"
SEQ_DONE = 0xFF           # HBRBC_SUBSET_DONE in the output sequence
SM_SUBSET = 2             # HBRBC_SM_SUBSET
# the proposal-state byte (enum hbrbc_subset_proposal)
PS_ONGOING, PS_HAS_VALUE, PS_ACCEPTED, PS_COMPLETE_FALSE, PS_COMPLETE_TRUE = range(5)

SubsetArgs = shared.args_struct(
    "SubsetArgs", "hbrbc_subset_args",
    [("count", USIZE), ("n", U32), ("max_out", U32), ("max_faults", U32), ("queue_epochs", U32),
     ("coins", U32), ("round", I32)],
    ("role", "flip", "ahead", "share_ok", "coin", "in_", "in_count", "out", "out_count", "state",
     "decision", "decision_epoch", "faults", "fault_count", "output_root", "proposal",
     "node_state", "out_seq", "out_len", "emitted", "active"))
SUBSET_ROUND = shared.Entry("hbrbc_subset_round", SubsetArgs)

# the flags of both sides of a round (hbrbc_sm_args.emitted[1], then
# hbrbc_subset_args.emitted[1]), in the order the read-back looks at them
BC_ROUND_FLAGS = (
    (2, "subset: a Value / Fake record reached a broadcast round run without those handlers"),
    (shared.ANY, "subset: a node emitted more than {0.max_out} broadcast messages in a round"))
BA_ROUND_FLAGS = (
    (ba_sim.BAD_QUEUE, "subset: an agreement message for an epoch beyond the future-epoch ring "
                       "of {0.queue_epochs} slots (raise queue_epochs)"),
    (ba_sim.BAD_COINS, "subset: a node reached a coin slot past the {0.coins} of the tables"),
    (ba_sim.BAD_OUT, "subset: a node emitted more than {0.max_out} agreement messages in a "
                     "round"),
    (shared.ANY, "subset: internal limit hit (flags {1:#x})"))


# ------------------------------------------------------------------ scenario --
class Instance:
    """One Subset instance of n nodes.  broadcasts[p]: the rbc_sim.Instance of
    proposer p's broadcast (proposer == p, no fake_from); ba_role[j] what leaves
    node j in every agreement, `flip` the recipients a TWO_FACED node lies to,
    `ahead` the epochs an AHEAD node adds; coin_bits[p] the forced coins of
    proposer p's agreement; `dead` the nodes that are absent."""

    def __init__(self, n, broadcasts, ba_role=None, flip=(), ahead=0, coin_bits=None, dead=(),
                 max_faulty=None):
        self.n = n
        self.broadcasts = list(broadcasts)
        self.ba_role = list(ba_role) if ba_role is not None else [ba_sim.HONEST] * n
        self.flip = sorted(set(flip))
        self.ahead = int(ahead)
        self.coin_bits = [[int(bool(b)) for b in bits] for bits in
                          (coin_bits if coin_bits is not None else [()] * n)]
        self.dead = frozenset(dead)
        assert len(self.broadcasts) == n and len(self.ba_role) == n and len(self.coin_bits) == n
        faulty = set(self.dead)
        for p, b in enumerate(self.broadcasts):
            assert b.n == n and b.proposer == p and b.fake_from is None, \
                "broadcast %d: proposer p, no injected broadcasts" % p
            faulty |= {j for j in range(n) if b.role[j] != rbc_sim.HONEST}
            if any(r != 0 for r in b.value_root) or any(b.value_tamper):
                faulty.add(p)
        faulty |= {j for j in range(n) if self.ba_role[j] != ba_sim.HONEST}
        assert all(0 <= j < n for j in self.dead | set(self.flip))
        # (max_faulty: a schedule test may ask for more than the protocol
        # tolerates; nothing is promised about such a run but that the GPU and
        # the host restatement agree on it)
        assert len(faulty) <= ((n - 1) // 3 if max_faulty is None else max_faulty), \
            "more than f dead or faulty nodes"
        self.faulty = frozenset(faulty)

    def live(self):
        return [j for j in range(self.n) if j not in self.dead]


class Scenario:
    """`count` Subset instances of one validator count n, `coins` coin slots
    per agreement."""

    def __init__(self, n, instances, coins=None, queue_epochs=4):
        self.n = n
        self.instances = list(instances)
        assert self.instances and all(i.n == n for i in self.instances) and 1 <= n <= 255
        self.coins = max(1, max(len(b) for i in self.instances for b in i.coin_bits)) \
            if coins is None else coins
        self.queue_epochs = queue_epochs
        self._ba = ba_sim.Scenario(
            n, [ba_sim.Instance(n, [NONE] * n, i.ba_role, i.flip, i.ahead, i.coin_bits[p])
                for i in self.instances for p in range(n)], self.coins, queue_epochs)
        self._rbc = rbc_sim.Scenario(n, [b for i in self.instances for b in i.broadcasts])

    @property
    def count(self):
        return len(self.instances)

    def ba_scenario(self):
        """The count x n agreement instances (instance (i, p) at i n + p) as a
        ba_sim.Scenario: what ba_sim.coin_plane takes."""
        return self._ba

    def rbc_scenario(self):
        """The count x n broadcast instances as an rbc_sim.Scenario: what
        rbc_sim.data_plane takes."""
        return self._rbc

    def set_tables(self, share_ok, coin):
        """share_ok [count n][coins][2][n], coin [count n][coins]."""
        self._ba.set_tables(share_ok, coin)

    def host_tables(self, inst):
        """The CoinTables the host restatement of instance `inst` reads."""
        return [self._ba.host_table(inst * self.n + p) for p in range(self.n)]

    def dead_mask(self):
        """[count n][n] bool: node j of instance i is dead (every proposer)."""
        m = np.zeros((self.count, self.n, self.n), bool)
        for r, i in enumerate(self.instances):
            for j in i.dead:
                m[r, :, j] = True
        return torch.from_numpy(m.reshape(self.count * self.n, self.n))


# ------------------------------------------------------------- one rank -----
class SubsetRank(shared.HasAgreement):
    """Every node of `count` Subset instances on one GPU (world = 1).  ok /
    dec: the data plane's proof_ok and decode_ok over the count x n broadcast
    instances."""

    def __init__(self, scn, device=0, ok=None, dec=None, max_out=24, bc_max_faults=None,
                 ba_max_faults=None, queue_epochs=None, max_rounds=256):
        n, cnt = scn.n, scn.count
        self.n, self.count, self.coins = n, cnt, scn.coins
        self.max_out = max_out
        self.max_faults = max(64, 8 * n) if ba_max_faults is None else ba_max_faults
        self.queue_epochs = queue_epochs or scn.queue_epochs
        self.max_rounds = max_rounds
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.device = dev
        B = cnt * n
        self.bc = rbc_sim.StateMachineRank(
            n, B, scn.rbc_scenario().roots, scn.rbc_scenario().tensors(dev), 0, 1, device,
            max_out, max(32, 4 * n) if bc_max_faults is None else bc_max_faults, ok, dec,
            max_rounds)
        self.bc.flags |= SM_SUBSET
        self.dead = scn.dead_mask().to(dev)
        self.sc = scn.ba_scenario().tensors(dev)
        del self.sc["input"]   # hbrbc_subset_args has none: the Subset proposes
        SUBSET_ROUND.bind()
        i32 = dict(dtype=torch.int32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        self.ag = shared.AgreementState(B, n, ba_sim.state_bytes(n, self.queue_epochs), max_out,
                                        self.max_faults, dev)
        self.proposal = torch.zeros((B, n), **u8)
        self.node_state = torch.zeros((cnt, n), **i32)
        self.out_seq = torch.zeros((cnt, n, n + 1), **u8)
        self.out_len = torch.zeros((cnt, n), **i32)
        # per round: agreement records emitted, flags (hbrbc_subset_args.emitted)
        self.hist = torch.zeros((max_rounds, 2), **i32)
        # act[r]: the records of both protocols in round r - 1 (phase 2's `active`)
        self.act = torch.zeros(max_rounds + 1, **i32)
        self.bc_records = self.ba_records = 0

    def reset(self):
        """Fresh nodes (before round 0 of another run); the dead nodes' proposal
        states start dropped."""
        self.bc.reset()
        self.bc.output_root.masked_fill_(self.dead, DROPPED)
        self.ag.reset()
        for t in (self.proposal, self.node_state, self.out_seq, self.out_len, self.hist, self.act):
            t.zero_()
        self.bc_records = self.ba_records = 0

    def phase2(self, r, active=None, stream=None):
        """hbrbc_subset_round of round r (after phase 1 of the same round)."""
        if r >= self.max_rounds:
            raise RuntimeError("subset: round %d past max_rounds %d" % (r, self.max_rounds))
        a = SubsetArgs(count=self.count, n=self.n, max_out=self.max_out,
                       max_faults=self.max_faults, queue_epochs=self.queue_epochs,
                       coins=self.coins, round=r)
        self.ag.write(a)
        a.output_root = self.bc.output_root.data_ptr()
        a.proposal, a.node_state = self.proposal.data_ptr(), self.node_state.data_ptr()
        a.out_seq, a.out_len = self.out_seq.data_ptr(), self.out_len.data_ptr()
        shared.fill(a, self.sc, self.hist, r, active)
        SUBSET_ROUND.launch(a, self.device, stream)

    def round(self, r, phase=shared.call):
        """Both phases of round r, then the swap of both sides' buffers.  The
        broadcasts quiesce rounds before the agreements do, and a round kernel
        that returns on `active == 0` leaves its out_count untouched: the
        broadcast side's counts are cleared before every round, so the swap
        after a round it skipped delivers nothing.  phase: the loop's hook around
        every launch (rounds.Rounds)."""
        bc = self.bc
        bc.out_count.zero_()
        phase("phase1", bc.round, r, None if r == 0 else bc.emitted(r - 1))
        phase("phase2", self.phase2, r, None if r == 0 else self.act[r])
        torch.add(bc.hist[r, 0], self.hist[r, 0], out=self.act[r + 1])
        bc.swap_local()
        self.ag.swap()


ROUND_BATCH = 8   # rounds enqueued per read-back


def protocols(rank):
    """The read-back's part of both sides of a SubsetRank, broadcasts first."""
    return [shared.Protocol(BC_ROUND_FLAGS, rank, rank, "bc_records"),
            shared.Protocol(BA_ROUND_FLAGS, rank, rank, "ba_records")]


def run_rounds(rank, events=None):
    """Drive both state machines until neither emits a record (rounds.Rounds):
    batches of ROUND_BATCH rounds are enqueued and the per-round counts and
    flags of both sides read back once per batch.  Returns the number of
    rounds (the index of the first round without records + 1).  Every run
    starts from fresh nodes.  events: a list that receives (phase name, start,
    end) device events of every launch, "phase1" and "phase2" per round."""
    return shared.Rounds(protocols(rank), rank.max_rounds, ROUND_BATCH, "subset", events=events,
                         reset=rank.reset, enqueue=rank.round,
                         read=shared.hist_rows([rank.bc, rank])).launch().wait()


class SubsetRun:
    """The results of one run.  Per (inst, node): outputs -- the sequence
    [(proposer, payload bytes), ..., DONE] in emission order -- and accepted,
    the set of accepted proposers.  Per (inst, node, proposer): bc_faults and
    ba_faults [(blamed, FaultKind name)], decisions and decision_epochs (None:
    undecided).  rounds; bc_emitted / ba_emitted: the records of every round."""

    def __init__(self, rank, rounds, payloads):
        n, cnt = rank.n, rank.count
        seq, ln = rank.out_seq.cpu().numpy(), rank.out_len.cpu().numpy()
        root = rank.bc.output_root.cpu().numpy().reshape(cnt, n, n)
        prop = rank.proposal.cpu().numpy().reshape(cnt, n, n)
        dec = rank.decision.cpu().numpy().reshape(cnt, n, n)
        ep = rank.decision_epoch.cpu().numpy().view(np.uint16).reshape(cnt, n, n)
        bcf = shared.fault_logs(rank.bc.fault_count[:, :n], rank.bc.faults, rank.bc.max_faults,
                                rbc_sim.FAULT_KINDS, "broadcast ")
        baf = shared.fault_logs(rank.fault_count, rank.faults, rank.max_faults,
                                ba_sim.FAULT_KINDS, "agreement ")
        self.outputs, self.accepted = {}, {}
        self.decisions, self.decision_epochs, self.bc_faults, self.ba_faults = {}, {}, {}, {}
        for i in range(cnt):
            for j in range(n):
                outs = []
                if int(ln[i, j]) > n + 1:
                    raise RuntimeError("output sequence overflow at (%d, %d)" % (i, j))
                for v in seq[i, j, :int(ln[i, j])]:
                    p = int(v)
                    outs.append(DONE if p == SEQ_DONE
                                else (p, payloads[(i * n + p, int(root[i, p, j]))]))
                self.outputs[(i, j)] = outs
                self.accepted[(i, j)] = {p for p in range(n) if int(prop[i, p, j])
                                         in (PS_ACCEPTED, PS_COMPLETE_TRUE)}
                for p in range(n):
                    d = int(dec[i, p, j])
                    self.decisions[(i, j, p)] = None if d == NONE else d
                    self.decision_epochs[(i, j, p)] = None if d == NONE else int(ep[i, p, j])
                    self.bc_faults[(i, j, p)] = bcf[(i * n + p, j)]
                    self.ba_faults[(i, j, p)] = baf[(i * n + p, j)]
        self.rounds = rounds
        self.bc_emitted = [int(v) for v in rank.bc.hist[:rounds, 0].cpu().numpy()]
        self.ba_emitted = [int(v) for v in rank.hist[:rounds, 0].cpu().numpy()]
        self.bc_records, self.ba_records = rank.bc_records, rank.ba_records


def run(scn, device=0, **kw):
    """Every node of every instance of `scn` on one GPU: a SubsetRun.  Raises
    on a message beyond the queue ring, a coin slot past scn.coins, or more
    than max_out records of a node in a round of either protocol."""
    ok, dec, payloads, _ = rbc_sim.data_plane(scn.rbc_scenario(), device)
    rank = SubsetRank(scn, device, ok, dec, **kw)
    return SubsetRun(rank, run_rounds(rank), payloads)


def simulate(scn, device=0, **kw):
    """(outputs, accepted, bc_faults, ba_faults, decisions, decision_epochs,
    rounds, bc_emitted, ba_emitted) of `run`."""
    r = run(scn, device, **kw)
    return (r.outputs, r.accepted, r.bc_faults, r.ba_faults, r.decisions, r.decision_epochs,
            r.rounds, r.bc_emitted, r.ba_emitted)
