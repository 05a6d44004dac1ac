"""Host restatement of `honey_badger::HoneyBadger`.

The reference's src/threshold_decrypt.rs (as a message handler),
src/honey_badger/epoch_state.rs and src/honey_badger/honey_badger.rs restated
handler by handler over `hbbft_amd.subset.Subset`.  It is the checker of the
GPU path (hbbft_amd/csrc/hb_sim.hip, hbbft_amd/hb_sim.py) and a usable class;
`HoneyBadger` is multi-epoch here (the GPU path runs one epoch).

Node ids are the indices 0..n-1.  Ciphertexts and decryption shares travel by
reference, as the coin does in `binary_agreement.CoinTable`: what the Subset
delivers for a proposer is looked up, by its bytes, among that proposer's
`DecryptTable`s (one per root slot of its broadcast), and a share is the
`variant` of its sender's share of that ciphertext (0 the honest share, 1 a
tampered one).  The lookup of the plaintext is exact: `PublicKeySet::decrypt`
interpolates g = sum lambda_i share_i at zero, every valid share is
[x_i] U for the point x_i of one polynomial of degree f, so g = [x(0)] U
whichever more-than-f valid shares a node combines -- and only valid shares
are combined (threshold_decrypt.rs:192, 204-217).  bincode and
the encryption of a proposal (threshold.encrypt_batch) stay with the
caller: `propose` takes the bytes that go into the Subset, and whether bytes
deserialise (a ciphertext, a contribution) is a flag of the table.
"""
import enum

from .broadcast import Fault, Step, Target, ValidatorSet
from .subset import DONE, Subset

__all__ = ["TdFaultKind", "TdError", "DecryptTable", "ThresholdDecrypt", "HbFaultKind", "HbFault",
           "Content", "Message", "Batch", "INCREMENTAL", "ALL_AT_END", "EpochState",
           "EncryptionSchedule", "Params", "HoneyBadger", "CT_VALID", "CT_UNDESERIALISABLE",
           "CT_INVALID"]

CT_VALID, CT_UNDESERIALISABLE, CT_INVALID = range(3)   # DecryptTable.ct_state
INCREMENTAL, ALL_AT_END = range(2)                      # SubsetHandlingStrategy


# --------------------------------------------------------------------------
# threshold_decrypt.rs:26-253, ciphertext and shares by reference
# --------------------------------------------------------------------------
class TdFaultKind(enum.Enum):
    """`threshold_decrypt::FaultKind` (50-58)."""
    MultipleDecryptionShares = 0
    UnverifiedDecryptionShareSender = 1


class TdError(Exception):
    """`threshold_decrypt::Error` (27-44): kind is MultipleInputs,
    InvalidCiphertext or CiphertextIsNone."""

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


class DecryptTable:
    """The data plane's outcomes for one (proposer, root slot): `payload`, the
    bytes the Subset delivers; ct_state -- 0 valid, 1 does not deserialise as a
    Ciphertext, 2 fails `Ciphertext::verify`; share_ok[variant][sender] --
    `pk_sender.verify_decryption_share(share, ct)` of the sender's honest
    (0) or tampered (1) share; `plaintext`, what the ciphertext decrypts to;
    `deserialises`: the contribution (the plaintext, or the payload of an epoch
    without encryption) deserialises."""

    def __init__(self, payload, ct_state, share_ok, plaintext, deserialises=True):
        self.payload, self.ct_state = bytes(payload), int(ct_state)
        self._ok = share_ok
        self.plaintext = bytes(plaintext)
        self.deserialises = bool(deserialises)

    @classmethod
    def forced(cls, n, payload, plaintext=None, ct_state=CT_VALID, deserialises=True):
        """Tables set by construction: every honest share valid, every
        tampered one invalid."""
        return cls(payload, ct_state, [[1] * n, [0] * n],
                   payload if plaintext is None else plaintext, deserialises)

    def share_ok(self, variant, sender):
        return bool(self._ok[variant][sender])


class ThresholdDecrypt:
    """`ThresholdDecrypt<N>` (70-253).  The ciphertext is a DecryptTable, a
    share its variant; `shares`: sender -> variant of the stored share."""

    def __init__(self, our_id, n):   # 117-125
        self.our_id, self.n, self.f = our_id, n, (n - 1) // 3
        self.ciphertext = None
        self.shares = {}
        self.had_input = False
        self.terminated = False

    def set_ciphertext(self, ct):   # 138-147
        if self.ciphertext is not None:
            raise TdError("MultipleInputs")
        if ct.ct_state != CT_VALID:   # !ct.verify()
            raise TdError("InvalidCiphertext")
        self.ciphertext = ct

    def start_decryption(self):   # 151-170
        if self.had_input:
            return Step()
        if self.ciphertext is None:
            raise TdError("CiphertextIsNone")
        step = Step()
        step.fault_log.extend(self._remove_invalid_shares())
        self.had_input = True
        step.messages.append(Target.all().message(0))   # our honest share
        self.shares[self.our_id] = 0
        step.extend(self._try_output())
        return step

    def sender_ids(self):   # 173-175
        return sorted(self.shares)

    def handle_message(self, sender_id, share):   # 182-201
        if self.terminated:
            return Step()
        if not 0 <= sender_id < self.n:
            raise TdError("UnknownSender")
        if not self._is_share_valid(sender_id, share):
            return Step.from_fault(sender_id, TdFaultKind.UnverifiedDecryptionShareSender)
        had = sender_id in self.shares
        self.shares[sender_id] = share   # (insert replaces the stored share)
        if had:
            return Step.from_fault(sender_id, TdFaultKind.MultipleDecryptionShares)
        return self._try_output()

    def _remove_invalid_shares(self):   # 204-217
        bad = [s for s in sorted(self.shares) if not self._is_share_valid(s, self.shares[s])]
        for s in bad:
            del self.shares[s]
        return [Fault(s, TdFaultKind.UnverifiedDecryptionShareSender) for s in bad]

    def _is_share_valid(self, sender_id, share):   # 220-229
        if self.ciphertext is None:
            return True   # verification postponed
        return self.ciphertext.share_ok(share, sender_id)

    def _try_output(self):   # 232-252
        if self.terminated or len(self.shares) <= self.f or self.ciphertext is None:
            return Step()
        self.terminated = True
        step = self.start_decryption()   # (had_input: a no-op)
        step.output.append(self.ciphertext.plaintext)
        return step


# --------------------------------------------------------------------------
# honey_badger/error.rs, message.rs, batch.rs
# --------------------------------------------------------------------------
class HbFaultKind(enum.Enum):
    """`honey_badger::FaultKind` (error.rs:36-62)."""
    UnexpectedDecryptionShare = 0
    DeserializeCiphertext = 1
    InvalidCiphertext = 2
    UnexpectedHbMessageEpoch = 3
    BatchDeserializationFailed = 4
    SubsetFault = 5
    DecryptionFault = 6


class HbFault:
    """A `honey_badger::FaultKind`; SubsetFault and DecryptionFault carry the
    sub-protocol's kind in `inner`.  `proposer`: whose proposal, ciphertext or
    decryption the fault arose in (bookkeeping for per-proposer logs: not part
    of the value)."""
    __slots__ = ("kind", "inner", "proposer")

    def __init__(self, kind, inner=None, proposer=None):
        self.kind, self.inner, self.proposer = kind, inner, proposer

    @property
    def name(self):
        return self.kind.name if self.inner is None else "%s(%s)" % (self.kind.name,
                                                                       self.inner.name)

    def __eq__(self, other):
        return isinstance(other, HbFault) and (self.kind, self.inner) == (other.kind, other.inner)

    def __hash__(self):
        return hash((self.kind, self.inner))

    def __repr__(self):
        return self.name


class Content:
    """`MessageContent::{Subset(msg), DecryptionShare { proposer_id, share }}`
    (message.rs): `subset` is the subset.Message or None."""
    __slots__ = ("subset", "proposer_id", "share")

    def __init__(self, subset=None, proposer_id=None, share=None):
        self.subset, self.proposer_id, self.share = subset, proposer_id, share

    def with_epoch(self, epoch):
        return Message(epoch, self)


class Message:
    """`honey_badger::Message { epoch, content }`."""
    __slots__ = ("epoch", "content")

    def __init__(self, epoch, content):
        self.epoch, self.content = epoch, content

    def __repr__(self):
        c = self.content
        return "Hb[%d](%r)" % (self.epoch, c.subset if c.subset is not None
                               else ("DecryptionShare", c.proposer_id, c.share))


class Batch:
    """`Batch { epoch, contributions }` (batch.rs): {proposer: bytes}."""
    __slots__ = ("epoch", "contributions")

    def __init__(self, epoch, contributions):
        self.epoch, self.contributions = epoch, dict(contributions)

    def __eq__(self, other):
        return isinstance(other, Batch) and (self.epoch, self.contributions) == \
            (other.epoch, other.contributions)

    def __repr__(self):
        return "Batch(%d, %r)" % (self.epoch, sorted(self.contributions))


# --------------------------------------------------------------------------
# honey_badger/epoch_state.rs
# --------------------------------------------------------------------------
class _Complete:
    """`DecryptionState::Complete(plaintext)` (epoch_state.rs:25-30); Ongoing
    is the ThresholdDecrypt itself."""
    __slots__ = ("plaintext", "table")

    def __init__(self, plaintext, table):
        self.plaintext, self.table = plaintext, table


class EpochState:
    """`EpochState<C, N>` (epoch_state.rs:177-395).  tables[p]: the
    DecryptTables of proposer p, one per root slot of its broadcast;
    coin_tables[p]: the CoinTable of its agreement.  Kept for the record:
    `subset` stays after completion (the reference keeps the accepted set
    only) and `subset_outputs` lists what it output."""

    def __init__(self, our_id, ids, epoch, tables, coin_tables, strategy=INCREMENTAL,
                 require_decryption=True, backend=None):   # 201-220
        self.our_id, self.epoch = our_id, epoch
        self.val_set = ids if isinstance(ids, ValidatorSet) else ValidatorSet(ids)
        self.n = self.val_set.num()
        self.tables = tables
        self.subset = Subset(our_id, self.val_set, coin_tables, backend=backend)
        self.accepted_ids = None          # SubsetState::Complete(ids)
        self.decryption = {}
        self.accepted_proposers = set()
        self.strategy = strategy
        self._held = []                   # SubsetHandler::AllAtEnd
        self.require_decryption = bool(require_decryption)
        self.subset_outputs = []

    def _table(self, proposer_id, value):
        for t in self.tables[proposer_id]:
            if t.payload == value:
                return t
        raise KeyError("no DecryptTable of proposer %r for the delivered bytes" % (proposer_id,))

    def propose(self, payload):   # 223-236 (serialisation and encryption: the caller's)
        return self.propose_with(lambda bc: bc.broadcast(payload))

    def propose_with(self, f):
        if self.accepted_ids is not None:   # SubsetState::handle_input, 69-75
            return Step()
        return self._process_subset(self.subset.propose_with(f))

    def received_proposals(self):   # 240-242, 88-93
        return len(self.accepted_ids) if self.accepted_ids is not None \
            else self.subset.received_proposals()

    def handle_message_content(self, sender_id, content):   # 245-273
        if content.subset is not None:
            if self.accepted_ids is not None:   # SubsetState::handle_message, 78-84
                return Step()
            return self._process_subset(self.subset.handle_message(sender_id, content.subset))
        p = content.proposer_id
        if self.accepted_ids is not None and p not in self.accepted_ids:
            return Step.from_fault(sender_id,
                                   HbFault(HbFaultKind.UnexpectedDecryptionShare, None, p))
        st = self.decryption.get(p)
        if st is None:
            st = self.decryption[p] = ThresholdDecrypt(self.our_id, self.n)
        td_step = Step() if isinstance(st, _Complete) else st.handle_message(sender_id,
                                                                             content.share)
        return self._process_decryption(p, td_step)

    def try_output_batch(self):   # 277-303
        if self.accepted_ids is None:
            return None
        plaintexts = []
        for p in sorted(self.accepted_ids):
            st = self.decryption.get(p)
            if not isinstance(st, _Complete):
                return None
            plaintexts.append((p, st))
        faults, contributions = [], {}
        for p, st in plaintexts:
            if st.table.deserialises:
                contributions[p] = st.plaintext
            else:
                faults.append(Fault(p, HbFault(HbFaultKind.BatchDeserializationFailed, None, p)))
        return Batch(self.epoch, contributions), faults

    def _process_subset(self, cs_step):   # 306-354
        step = Step()
        for fl in cs_step.fault_log:
            step.fault_log.append(Fault(fl.node_id, HbFault(HbFaultKind.SubsetFault, fl.kind)))
        for tm in cs_step.messages:
            step.messages.append(tm.target.message(Content(subset=tm.message)
                                                   .with_epoch(self.epoch)))
        for o in cs_step.output:
            self.subset_outputs.append(o)
            if o is DONE:   # SubsetHandler::handle, 132-162
                contributions, self._held, is_done = self._held, [], True
            elif self.strategy == ALL_AT_END:
                self._held.append((o.proposer_id, o.value))
                contributions, is_done = [], False
            else:
                contributions, is_done = [(o.proposer_id, o.value)], False
            for p, v in contributions:
                if self.require_decryption:
                    step.extend(self._send_decryption_share(p, v))
                else:
                    self.decryption[p] = _Complete(v, self._table(p, v))
                self.accepted_proposers.add(p)
            if is_done:
                self.accepted_ids = frozenset(self.accepted_proposers)
                for p in sorted(q for q in self.decryption if q not in self.accepted_proposers):
                    st = self.decryption.pop(p)
                    if not isinstance(st, _Complete):
                        for s in st.sender_ids():
                            step.fault_log.append(Fault(s, HbFault(
                                HbFaultKind.UnexpectedDecryptionShare, None, p)))
        return step

    def _process_decryption(self, proposer_id, td_step):   # 357-371
        step = Step()
        for fl in td_step.fault_log:
            step.fault_log.append(Fault(fl.node_id, HbFault(HbFaultKind.DecryptionFault, fl.kind,
                                                            proposer_id)))
        for tm in td_step.messages:
            step.messages.append(tm.target.message(
                Content(proposer_id=proposer_id, share=tm.message).with_epoch(self.epoch)))
        if td_step.output:
            self.decryption[proposer_id] = _Complete(td_step.output[0],
                                                     self.decryption[proposer_id].ciphertext)
        return step

    def _send_decryption_share(self, proposer_id, v):   # 375-394
        ct = self._table(proposer_id, v)
        if ct.ct_state == CT_UNDESERIALISABLE:
            return Step.from_fault(proposer_id, HbFault(HbFaultKind.DeserializeCiphertext, None,
                                                        proposer_id))
        st = self.decryption.get(proposer_id)
        if st is None:
            st = self.decryption[proposer_id] = ThresholdDecrypt(self.our_id, self.n)
        if isinstance(st, _Complete):   # DecryptionState::set_ciphertext, 47-55
            return Step()
        try:
            st.set_ciphertext(ct)
        except TdError as e:
            if e.kind == "InvalidCiphertext":
                return Step.from_fault(proposer_id, HbFault(HbFaultKind.InvalidCiphertext, None,
                                                            proposer_id))
            raise
        return self._process_decryption(proposer_id, st.start_decryption())


# --------------------------------------------------------------------------
# honey_badger/honey_badger.rs, params.rs
# --------------------------------------------------------------------------
class EncryptionSchedule:
    """`EncryptionSchedule` (honey_badger.rs:215-237): ("Always",), ("Never",),
    ("EveryNthEpoch", n) or ("TickTock", on, off)."""

    def __init__(self, kind, *args):
        assert (kind, len(args)) in (("Always", 0), ("Never", 0), ("EveryNthEpoch", 1),
                                     ("TickTock", 2))
        self.kind, self.args = kind, tuple(int(a) for a in args)

    @classmethod
    def always(cls):
        return cls("Always")

    @classmethod
    def never(cls):
        return cls("Never")

    @classmethod
    def every_nth_epoch(cls, n):
        return cls("EveryNthEpoch", n)

    @classmethod
    def tick_tock(cls, on, off):
        return cls("TickTock", on, off)

    def use_on_epoch(self, epoch):   # 229-236, as the reference computes it
        if self.kind == "Always":
            return True
        if self.kind == "Never":
            return False
        if self.kind == "EveryNthEpoch":
            return epoch % self.args[0] == 0
        on, off = self.args
        return epoch % (on + off) <= on   # (`<=`: on + 1 encrypted epochs of on + off)


class Params:
    """`Params` (params.rs:7-24)."""

    def __init__(self, max_future_epochs=3, subset_handling_strategy=INCREMENTAL,
                 encryption_schedule=None):
        self.max_future_epochs = max_future_epochs
        self.subset_handling_strategy = subset_handling_strategy
        self.encryption_schedule = encryption_schedule or EncryptionSchedule.always()


class HoneyBadger:
    """`HoneyBadger<C, N>` (honey_badger.rs:17-211).  tables(epoch)[p]: the
    DecryptTables of proposer p in that epoch; coin_tables(epoch)[p]: the
    CoinTable of its agreement."""

    def __init__(self, our_id, ids, tables, coin_tables, params=None, epoch=0, backend=None):
        self.our_id = our_id
        self.val_set = ids if isinstance(ids, ValidatorSet) else ValidatorSet(ids)
        self._tables, self._coin_tables, self._be = tables, coin_tables, backend
        self.params = params or Params()
        self.epoch = epoch
        self.has_input = False
        self.epochs = {}

    def propose(self, payload):   # 88-95
        return self.propose_with(lambda bc: bc.broadcast(payload))

    def propose_with(self, f):
        if not self.val_set.contains(self.our_id):
            return Step()
        self.has_input = True
        step = self._epoch_state_mut(self.epoch).propose_with(f)
        return step.join(self._try_output_batches())

    def handle_message(self, sender_id, message):   # 100-116
        if not self.val_set.contains(sender_id):
            raise ValueError("UnknownSender")
        if message.epoch > self.epoch + self.params.max_future_epochs:
            return Step.from_fault(sender_id, HbFault(HbFaultKind.UnexpectedHbMessageEpoch))
        if message.epoch < self.epoch:
            return Step()   # the message is late; discard it
        step = self._epoch_state_mut(message.epoch).handle_message_content(sender_id,
                                                                           message.content)
        return step.join(self._try_output_batches())

    def next_epoch(self):   # 130-132
        return self.epoch

    def skip_to_epoch(self, epoch):   # 143-147
        while self.epoch < epoch:
            self._update_epoch()

    def received_proposals(self):   # 157-161
        es = self.epochs.get(self.epoch)
        return 0 if es is None else es.received_proposals()

    def _update_epoch(self):   # 164-169
        self.epochs.pop(self.epoch, None)
        self.epoch += 1
        self.has_input = False

    def _try_output_batches(self):   # 172-185
        step = Step()
        while True:
            es = self.epochs.get(self.epoch)
            got = None if es is None else es.try_output_batch()
            if got is None:
                return step
            step.output.append(got[0])
            step.fault_log.extend(got[1])
            self._update_epoch()

    def _epoch_state_mut(self, epoch):   # 189-200
        es = self.epochs.get(epoch)
        if es is None:
            es = self.epochs[epoch] = EpochState(
                self.our_id, self.val_set, epoch, self._tables(epoch), self._coin_tables(epoch),
                self.params.subset_handling_strategy,
                self.params.encryption_schedule.use_on_epoch(epoch), self._be)
        return es
