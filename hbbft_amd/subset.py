"""Host restatement of `subset::Subset`.

The reference's src/subset/subset.rs and src/subset/proposal_state.rs restated
handler by handler: per proposer a `ProposalState` holding one
`hbbft_amd.broadcast.Broadcast` and one `hbbft_amd.binary_agreement.
BinaryAgreement`, and the three rules that couple them -- a delivered
broadcast votes `true` in its agreement, the (N - f)-th accepted proposal
votes `false` in every other one, all complete gives `Done`.  It is the
checker of the GPU path (hbbft_amd/csrc/subset_sim.hip, hbbft_amd/
subset_sim.py) and a usable class.

Node ids are the indices 0..n-1 (BinaryAgreement's convention).  The coin of
proposer p's agreement travels by reference: `tables[p]` is its CoinTable
(hbbft_amd/binary_agreement.py).
"""
import enum

from .binary_agreement import BinaryAgreement
from .broadcast import Broadcast, Fault, Step, ValidatorSet

__all__ = ["ONGOING", "HAS_VALUE", "ACCEPTED", "COMPLETE", "Protocol", "SubsetFault", "Content",
           "Message", "Contribution", "DONE", "ProposalState", "Subset", "SubsetError"]

# ProposalState (proposal_state.rs:17-28); Complete carries its bool in `.result`
ONGOING, HAS_VALUE, ACCEPTED, COMPLETE = range(4)


class Protocol(enum.Enum):
    """The two arms of `MessageContent` (subset/message.rs) and of the
    subset `FaultKind` (BroadcastFault / BaFault)."""
    Broadcast = 0
    Agreement = 1


class SubsetFault:
    """`subset::FaultKind::{BroadcastFault, BaFault}(kind)`."""
    __slots__ = ("protocol", "kind")

    def __init__(self, protocol, kind):
        self.protocol, self.kind = protocol, kind

    @property
    def name(self):
        return "%sFault(%s)" % ("Broadcast" if self.protocol is Protocol.Broadcast else "Ba",
                                self.kind.name)

    def __eq__(self, other):
        return isinstance(other, SubsetFault) and (self.protocol, self.kind) == \
            (other.protocol, other.kind)

    def __hash__(self):
        return hash((self.protocol, self.kind))

    def __repr__(self):
        return self.name


class Content:
    """`MessageContent::{Broadcast, Agreement}(msg)`."""
    __slots__ = ("protocol", "msg")

    def __init__(self, protocol, msg):
        self.protocol, self.msg = protocol, msg

    def with_proposer(self, proposer_id):
        return Message(proposer_id, self)


class Message:
    """`subset::Message { proposer_id, content }`."""
    __slots__ = ("proposer_id", "content")

    def __init__(self, proposer_id, content):
        self.proposer_id, self.content = proposer_id, content

    def __repr__(self):
        return "%s[%r](%r)" % (self.content.protocol.name, self.proposer_id, self.content.msg)


class Contribution:
    """`SubsetOutput::Contribution(proposer, value)` (subset.rs:19-29)."""
    __slots__ = ("proposer_id", "value")

    def __init__(self, proposer_id, value):
        self.proposer_id, self.value = proposer_id, bytes(value)

    def __eq__(self, other):
        return isinstance(other, Contribution) and (self.proposer_id, self.value) == \
            (other.proposer_id, other.value)

    def __hash__(self):
        return hash((self.proposer_id, self.value))

    def __repr__(self):
        return "Contribution(%r, %s)" % (self.proposer_id, self.value.hex()[:10])


class _Done:
    def __repr__(self):
        return "Done"


DONE = _Done()   # `SubsetOutput::Done`


class SubsetError(Exception):
    """`subset::Error::UnknownProposer`."""


def _wrap(step, protocol):
    """`Step::extend_with` as convert_bc / convert_ba use it
    (proposal_state.rs:139-161): faults and messages wrapped, the last output
    popped.  Returns (output or None, Step)."""
    out = Step()
    out.fault_log.extend(Fault(fl.node_id, SubsetFault(protocol, fl.kind))
                         for fl in step.fault_log)
    for tm in step.messages:
        out.messages.append(tm.target.message(Content(protocol, tm.message)))
    value = step.output[-1] if step.output else None
    return value, out


class ProposalState:
    """`ProposalState<N, S>` (proposal_state.rs:17-173).  `state` is ONGOING
    (broadcast and agreement), HAS_VALUE (value and agreement), ACCEPTED
    (broadcast) or COMPLETE (`result`: accepted and output, or dropped).  A
    dropped instance is forgotten (`broadcast` / `agreement` None) as the
    reference's enum forgets it; the agreement's decision and decision epoch
    are kept for the record."""

    def __init__(self, our_id, val_set, proposer_id, table, backend=None):   # 32-38
        self.proposer_id = proposer_id
        self.state = ONGOING
        self.agreement = BinaryAgreement(our_id, val_set.num(), table)
        self.broadcast = Broadcast(our_id, val_set, proposer_id, backend=backend)
        self.value = None
        self.result = None
        self.decision = None
        self.decision_epoch = None
        self.max_queued_ahead = 0   # (BinaryAgreement's bookkeeping for the GPU ring)

    def received(self):   # 41-47
        return self.state == HAS_VALUE or (self.state == COMPLETE and self.result)

    def accepted(self):   # 50-56
        return self.state == ACCEPTED or (self.state == COMPLETE and self.result)

    def complete(self):   # 59-66
        return self.state == COMPLETE

    def propose(self, value):   # 69-71
        return self.handle_broadcast(lambda bc: bc.broadcast(value))

    def handle_message(self, sender_id, content):   # 74-83
        if content.protocol is Protocol.Agreement:
            return self.handle_agreement(lambda ba: ba.handle_message(sender_id, content.msg))
        return self.handle_broadcast(lambda bc: bc.handle_message(sender_id, content.msg))

    def vote_false(self):   # 86-88
        return self.handle_agreement(lambda ba: ba.propose(False))

    def handle_broadcast(self, f):
        """proposal_state.rs:91-113.  `f` takes the Broadcast and returns its
        step."""
        if self.state == ONGOING:
            value, step = _wrap(f(self.broadcast), Protocol.Broadcast)
            if value is None:
                return step
            self.state, self.value, self.broadcast = HAS_VALUE, value, None
            return step.join(self.handle_agreement(lambda ba: ba.propose(True)))
        if self.state == ACCEPTED:
            value, step = _wrap(f(self.broadcast), Protocol.Broadcast)
            if value is None:
                return step
            self._complete(True)
            step.output.append(value)
            return step
        return Step()   # HasValue, Complete: the broadcast is gone

    def handle_agreement(self, f):
        """proposal_state.rs:117-137.  `f` takes the BinaryAgreement and
        returns its step."""
        if self.state not in (ONGOING, HAS_VALUE):
            return Step()   # Accepted, Complete: the agreement is gone
        ba = self.agreement
        decision, step = _wrap(f(ba), Protocol.Agreement)
        self.max_queued_ahead = ba.max_queued_ahead
        if decision is None:
            return step
        self.decision, self.decision_epoch = bool(decision), ba.decision_epoch
        self.agreement = None
        if self.state == ONGOING:
            if decision:
                self.state = ACCEPTED
            else:
                self._complete(False)
        else:
            value = self.value
            self._complete(bool(decision))
            if decision:
                step.output.append(value)
        return step

    def _complete(self, result):
        self.state, self.result = COMPLETE, result
        self.broadcast = self.agreement = self.value = None


class Subset:
    """`Subset<N, S>` (subset.rs:31-170) of node `our_id` among `ids`;
    tables[i]: the CoinTable of the agreement about the i-th proposer."""

    def __init__(self, our_id, ids, tables, backend=None):   # 79-98
        self.our_id = our_id
        self.val_set = ids if isinstance(ids, ValidatorSet) else ValidatorSet(ids)
        self.proposal_states = {
            pid: ProposalState(our_id, self.val_set, pid, tables[idx], backend)
            for idx, pid in enumerate(self.val_set.all_ids())}
        self.decided = False

    def handle_input(self, value):
        return self.propose(value)

    def terminated(self):
        return self.decided

    def propose(self, value):   # 103-115
        return self.propose_with(lambda bc: bc.broadcast(value))

    def propose_with(self, f):
        """`propose` with the broadcast call handed in (a test network's
        proposer sends Values of its own making)."""
        if not self.val_set.contains(self.our_id):
            return Step()
        state = self.proposal_states.get(self.our_id)
        if state is None:
            raise SubsetError("UnknownProposer")
        step = self._convert_step(self.our_id, state.handle_broadcast(f))
        return step.join(self._try_output())

    def handle_message(self, sender_id, msg):   # 120-128
        state = self.proposal_states.get(msg.proposer_id)
        if state is None:
            raise SubsetError("UnknownProposer")
        step = self._convert_step(msg.proposer_id, state.handle_message(sender_id, msg.content))
        return step.join(self._try_output())

    def received_proposals(self):   # 131-134
        return sum(1 for s in self.proposal_states.values() if s.received())

    @staticmethod
    def _convert_step(proposer_id, prop_step):   # 136-144
        step = Step()
        step.fault_log.extend(prop_step.fault_log)
        step.messages.extend(tm.target.message(tm.message.with_proposer(proposer_id))
                             for tm in prop_step.messages)
        if prop_step.output:
            step.output.append(Contribution(proposer_id, prop_step.output[-1]))
        return step

    def count_accepted(self):   # 147-150
        return sum(1 for s in self.proposal_states.values() if s.accepted())

    def _try_output(self):
        """subset.rs:154-169: while exactly N - f proposals are accepted every
        call votes `false` on all of them (a no-op wherever the agreement has an
        estimate, has left epoch 0 or is gone)."""
        if self.decided or self.count_accepted() < self.val_set.num_correct():
            return Step()
        step = Step()
        if self.count_accepted() == self.val_set.num_correct():
            for pid in self.val_set.all_ids():
                step.extend(self._convert_step(pid, self.proposal_states[pid].vote_false()))
        if all(s.complete() for s in self.proposal_states.values()):
            self.decided = True
            step.output.append(DONE)
        return step
