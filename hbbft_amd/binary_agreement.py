"""Host restatement of `binary_agreement::BinaryAgreement`.

The state machine of the reference's src/binary_agreement/binary_agreement.rs
(handle_message, the Conf round, the `false, true, coin` schedule, Term and
the future-epoch queue), of sbv_broadcast.rs (BVal / Aux) and bool_set.rs, and
of the `ThresholdSign` it drives (threshold_sign.rs:127-270), restated handler
by handler in Python with the Step / Fault / Target plumbing of
hbbft_amd/broadcast.py.  It is the checker of the GPU state machine
(hbbft_amd/csrc/ba_sim.hip, hbbft_amd/ba_sim.py) and a usable class.

The coin travels by reference.  A `Coin` message names its sender's signature
share of the epoch's document (or a tampered copy) and carries no bytes:
`is_share_valid` is `table.share_ok(slot, tampered, sender)` and the parity of
`combine_and_verify_sig` is `table.coin(slot)`, coin slot q being epoch
3q + 2.  A BLS threshold signature is unique -- any f + 1 valid shares
interpolate to the same [sk] H -- so the parity does not depend on which
shares a node happened to hold; hbbft_amd/ba_sim.py coin_plane computes both
tables with the G2 kernels of hbbft_amd/threshold.py.

All nodes are validators (observers are out of scope).
"""
import enum

from .broadcast import Fault, Step, Target

__all__ = ["NONE", "FALSE", "TRUE", "BOTH", "FaultKind", "Message", "CoinTable", "CoinSlotError",
           "ThresholdSign", "SbvBroadcast", "BinaryAgreement", "MAX_FUTURE_EPOCHS"]

# ---- bool_set.rs:6-16: a set of bools as two bits --------------------------
NONE, FALSE, TRUE, BOTH = 0, 1, 2, 3
MAX_FUTURE_EPOCHS = 1000   # binary_agreement.rs:214


def bs_from(b):
    """`BoolSet::from(bool)` (bool_set.rs:58-66)."""
    return TRUE if b else FALSE


def bs_iter(s):
    """`BoolSetIter` (bool_set.rs:72-86): `true` first."""
    return [b for b in (True, False) if s & bs_from(b)]


def bs_definite(s):
    """`BoolSet::definite` (bool_set.rs:49-55)."""
    return {FALSE: False, TRUE: True}.get(s)


def bs_subset(s, other):
    """`BoolSet::is_subset` (bool_set.rs:44-46)."""
    return s & other == s


class FaultKind(enum.Enum):
    """`binary_agreement::FaultKind` (mod.rs:110-129), in declaration order.
    CoinFault wraps threshold_sign::FaultKind; the only one a by-reference
    coin can raise is UnverifiedSignatureShareSender."""
    DuplicateBVal = 0
    DuplicateAux = 1
    MultipleConf = 2
    MultipleTerm = 3
    AgreementEpoch = 4
    CoinFault = 5


class Message:
    """`binary_agreement::Message { epoch, content }` (mod.rs:133-171).  kind:
    BVAL / AUX (value: bool), CONF (value: a BoolSet), TERM (value: bool),
    COIN (a share by reference: `tampered`)."""
    BVAL, AUX, CONF, TERM, COIN = range(5)
    _NAMES = ("BVal", "Aux", "Conf", "Term", "Coin")
    __slots__ = ("epoch", "kind", "value", "tampered")

    def __init__(self, epoch, kind, value=0, tampered=0):
        self.epoch, self.kind, self.value, self.tampered = epoch, kind, int(value), int(tampered)

    def can_expire(self):   # mod.rs:156-161
        return self.kind != Message.TERM

    def key(self):
        return (self.epoch, self.kind, self.value, self.tampered)

    def __eq__(self, other):
        return isinstance(other, Message) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return "%s(%d%s)@%d" % (self._NAMES[self.kind], self.value,
                                ", tampered" if self.tampered else "", self.epoch)


class CoinSlotError(Exception):
    """A node reached a coin epoch past the table."""


class CoinTable:
    """The data plane's outcomes for one instance: share_ok[q][t][j] --
    `pk_j.verify_g2(share, hash)` of node j's share of slot q's document
    (t = 1: the tampered copy) -- and coin[q], the parity of the slot's
    combined signature."""

    def __init__(self, share_ok, coin):
        self._ok = share_ok
        self._coin = [int(c) for c in coin]

    @classmethod
    def forced(cls, n, bits):
        """Tables set by construction: every genuine share valid, every
        tampered one invalid, coin[q] = bits[q]."""
        return cls([[[1] * n, [0] * n] for _ in bits], bits)

    def __len__(self):
        return len(self._coin)

    def _slot(self, q):
        if not 0 <= q < len(self._coin):
            raise CoinSlotError("coin slot %d past the table of %d" % (q, len(self._coin)))
        return q

    def share_ok(self, q, tampered, sender):
        return bool(self._ok[self._slot(q)][tampered][sender])

    def coin(self, q):
        return bool(self._coin[self._slot(q)])


# --------------------------------------------------------------------------
# threshold_sign.rs:127-270, shares by reference
# --------------------------------------------------------------------------
class ThresholdSign:
    """`ThresholdSign<N>` with its document set (binary_agreement.rs:444-447
    set_document): the coin of slot q."""

    def __init__(self, our_id, num_faulty, table, slot):
        self.our_id, self.f, self.table, self.slot = our_id, num_faulty, table, slot
        table._slot(slot)
        self.received_shares = {}   # sender -> tampered flag of the stored share
        self.had_input = False
        self.terminated = False

    def sign(self):
        """threshold_sign.rs:157-174."""
        if self.had_input:
            return Step()
        self.had_input = True
        step = Step()
        step.fault_log.extend(self._remove_invalid_shares())
        msg = 0   # our own genuine share
        step.messages.append(Target.all().message(msg))
        step.extend(self.handle_message(self.our_id, msg))
        return step

    def handle_message(self, sender_id, tampered):
        """threshold_sign.rs:181-197."""
        if self.terminated:
            return Step()
        if not self._is_share_valid(sender_id, tampered):
            return Step.from_fault(sender_id, FaultKind.CoinFault)
        self.received_shares[sender_id] = tampered
        return self._try_output()

    def _remove_invalid_shares(self):
        """threshold_sign.rs:200-213 (the document is set from the start, so
        every stored share was checked: nothing to remove)."""
        bad = [s for s, t in sorted(self.received_shares.items())
               if not self._is_share_valid(s, t)]
        for s in bad:
            del self.received_shares[s]
        return [Fault(s, FaultKind.CoinFault) for s in bad]

    def _is_share_valid(self, sender_id, tampered):   # 216-225
        return self.table.share_ok(self.slot, tampered, sender_id)

    def _try_output(self):
        """threshold_sign.rs:227-247: sign() runs AFTER `terminated` is set, so
        a node that collects f + 1 shares before its own Conf round finishes
        sends its share now and does not handle it."""
        if not self.terminated and len(self.received_shares) > self.f:
            sig = self.table.coin(self.slot)   # combine_and_verify_sig (249-270), parity
            self.terminated = True
            step = self.sign()
            step.output.append(sig)
            return step
        return Step()


# --------------------------------------------------------------------------
# sbv_broadcast.rs:51-187
# --------------------------------------------------------------------------
class SbvBroadcast:
    """Messages of its steps are (Message.BVAL | Message.AUX, bool) pairs;
    its output a BoolSet."""

    def __init__(self, our_id, n, f):
        self.our_id, self.n, self.f = our_id, n, f
        self.bin_values = NONE
        self.received_bval = {False: set(), True: set()}
        self.sent_bval = NONE
        self.received_aux = {False: set(), True: set()}
        self.terminated = False

    def clear(self, init):
        """sbv_broadcast.rs:81-87: the Term senders count as BVal and Aux."""
        self.bin_values = NONE
        self.received_bval = {b: set(init[b]) for b in (False, True)}
        self.sent_bval = NONE
        self.received_aux = {b: set(init[b]) for b in (False, True)}
        self.terminated = False

    def handle_message(self, sender_id, kind, b):   # 89-94
        return self.handle_bval(sender_id, b) if kind == Message.BVAL \
            else self.handle_aux(sender_id, b)

    def send_bval(self, b):   # 102-108
        if self.sent_bval & bs_from(b):
            return Step()
        self.sent_bval |= bs_from(b)
        return self._send(Message.BVAL, b)

    def handle_bval(self, sender_id, b):
        """sbv_broadcast.rs:114-137: `== 2f + 1` is tested before `== f + 1`;
        at f = 0 both fire on the first BVal, in that order."""
        if sender_id in self.received_bval[b]:
            return Step.from_fault(sender_id, FaultKind.DuplicateBVal)
        self.received_bval[b].add(sender_id)
        count_bval = len(self.received_bval[b])
        step = Step()
        if count_bval == 2 * self.f + 1:
            self.bin_values |= bs_from(b)
            if self.bin_values != BOTH:
                step.extend(self._send(Message.AUX, b))   # first entry: send Aux(b)
            else:
                step.extend(self._try_output())
        if count_bval == self.f + 1:
            step.extend(self.send_bval(b))
        return step

    def _send(self, kind, b):   # 140-147
        step = Step.from_message(Target.all().message((kind, b)))
        return step.join(self.handle_message(self.our_id, kind, b))

    def handle_aux(self, sender_id, b):   # 150-155
        if sender_id in self.received_aux[b]:
            return Step.from_fault(sender_id, FaultKind.DuplicateAux)
        self.received_aux[b].add(sender_id)
        return self._try_output()

    def _try_output(self):   # 158-168
        if self.terminated or self.bin_values == NONE:
            return Step()
        count, vals = self._count_aux()
        if count < self.n - self.f:
            return Step()
        self.terminated = True
        step = Step()
        step.output.append(vals)
        return step

    def _count_aux(self):   # 176-186
        values, count = NONE, 0
        for b in bs_iter(self.bin_values):
            if self.received_aux[b]:
                values |= bs_from(b)
                count += len(self.received_aux[b])
        return count, values


# --------------------------------------------------------------------------
# binary_agreement.rs
# --------------------------------------------------------------------------
class _Received:
    """`ReceivedMessages` (binary_agreement.rs:46-138): one sender's messages
    of one future epoch."""
    __slots__ = ("bval", "aux", "conf", "term", "coin")

    def __init__(self):
        self.bval, self.aux, self.conf, self.term, self.coin = NONE, NONE, None, None, None

    def insert(self, m):   # 72-109
        if m.kind == Message.BVAL:
            if self.bval & bs_from(m.value):
                return FaultKind.DuplicateBVal
            self.bval |= bs_from(m.value)
        elif m.kind == Message.AUX:
            if self.aux & bs_from(m.value):
                return FaultKind.DuplicateAux
            self.aux |= bs_from(m.value)
        elif m.kind == Message.CONF:
            if self.conf is not None:
                return FaultKind.MultipleConf
            self.conf = m.value
        elif m.kind == Message.TERM:
            if self.term is not None:
                return FaultKind.MultipleTerm
            self.term = m.value
        else:
            if self.coin is not None:
                return FaultKind.AgreementEpoch
            self.coin = m.tampered
        return None

    def messages(self):
        """binary_agreement.rs:112-137 as (kind, value, tampered): BVal(true),
        BVal(false), Aux(true), Aux(false), Conf, Term, Coin."""
        out = [(Message.BVAL, b, 0) for b in bs_iter(self.bval)]
        out += [(Message.AUX, b, 0) for b in bs_iter(self.aux)]
        if self.conf is not None:
            out.append((Message.CONF, self.conf, 0))
        if self.term is not None:
            out.append((Message.TERM, self.term, 0))
        if self.coin is not None:
            out.append((Message.COIN, 0, self.coin))
        return out


class BinaryAgreement:
    """`BinaryAgreement<N, S>` (binary_agreement.rs:142-521) of node `our_id`
    among nodes 0..n-1; `table` is the instance's CoinTable."""

    def __init__(self, our_id, n, table):
        self.our_id, self.n, self.f = our_id, n, (n - 1) // 3
        self.table = table
        self.epoch = 0
        self.sbv = SbvBroadcast(our_id, n, self.f)
        self.received_conf = {}
        self.received_term = {False: set(), True: set()}
        self.estimated = None
        self.decision = None
        self.decision_epoch = None
        self.incoming_queue = {}     # epoch -> {sender -> _Received}
        self.conf_values = None
        self.coin_state = True       # a bool: Decided(b); a ThresholdSign: InProgress
        # (not in the reference) how far ahead the furthest queued message was:
        # the GPU state machine keeps a bounded ring (ba_sim.py queue_epochs)
        self.max_queued_ahead = 0

    def terminated(self):
        return self.decision is not None

    def handle_input(self, value):
        return self.propose(value)

    def can_propose(self):   # 273-275
        return self.epoch == 0 and self.estimated is None

    def propose(self, value):   # 232-240
        if not self.can_propose():
            return Step()
        self.estimated = bool(value)
        return self._handle_sbvb_step(self.sbv.send_bval(bool(value)))

    def handle_message(self, sender_id, msg):
        """binary_agreement.rs:245-269."""
        if self.decision is not None or (msg.epoch < self.epoch and msg.can_expire()):
            return Step()
        if msg.epoch > self.epoch + MAX_FUTURE_EPOCHS:
            return Step.from_fault(sender_id, FaultKind.AgreementEpoch)
        if msg.epoch > self.epoch:
            self.max_queued_ahead = max(self.max_queued_ahead, msg.epoch - self.epoch)
            received = self.incoming_queue.setdefault(msg.epoch, {}).setdefault(
                sender_id, _Received())
            fault = received.insert(msg)
            return Step() if fault is None else Step.from_fault(sender_id, fault)
        return self._handle_content(sender_id, msg.kind, msg.value, msg.tampered)

    def _handle_content(self, sender_id, kind, value, tampered):   # 278-289
        if kind in (Message.BVAL, Message.AUX):
            return self._handle_sbvb_step(self.sbv.handle_message(sender_id, kind, bool(value)))
        if kind == Message.CONF:
            return self._handle_conf(sender_id, value)
        if kind == Message.TERM:
            return self._handle_term(sender_id, bool(value))
        return self._handle_coin(sender_id, tampered)

    def _msg(self, kind, value=0, tampered=0, epoch=None):
        return Target.all().message(Message(self.epoch if epoch is None else epoch, kind, value,
                                            tampered))

    def _handle_sbvb_step(self, sbvb_step):
        """binary_agreement.rs:303-327."""
        step = Step()
        step.fault_log.extend(sbvb_step.fault_log)
        step.messages.extend(self._msg(k, b) for k, b in
                             (tm.message for tm in sbvb_step.messages))
        if self.conf_values is not None:
            return step   # the Conf round has already started
        if sbvb_step.output:
            aux_vals = sbvb_step.output[0]
            if isinstance(self.coin_state, bool):
                self.conf_values = aux_vals
                step.extend(self._try_update_epoch())
            else:
                step.extend(self._send_conf(aux_vals))
        return step

    def _handle_conf(self, sender_id, v):   # 331-334 (a second Conf overwrites)
        self.received_conf[sender_id] = v
        return self._try_finish_conf_round()

    def _handle_term(self, sender_id, b):
        """binary_agreement.rs:339-353: insert, decide when more than f agree,
        else the Term counts as the sender's BVal, Aux and Conf."""
        self.received_term[b].add(sender_id)
        if self.decision is not None:
            return Step()
        if len(self.received_term[b]) > self.f:
            return self._decide(b)
        sbvb_step = self.sbv.handle_bval(sender_id, b)
        sbvb_step.extend(self.sbv.handle_aux(sender_id, b))
        step = self._handle_sbvb_step(sbvb_step)
        return step.join(self._handle_conf(sender_id, bs_from(b)))

    def _handle_coin(self, sender_id, tampered):   # 357-365
        if isinstance(self.coin_state, bool):
            return Step()
        return self._on_coin_step(self.coin_state.handle_message(sender_id, tampered))

    def _send_conf(self, values):   # 368-382
        if self.conf_values is not None:
            return Step()
        self.conf_values = values
        return self._send(Message.CONF, values)

    def _send(self, kind, value):   # 385-394
        step = Step.from_message(self._msg(kind, value))
        return step.join(self._handle_content(self.our_id, kind, value, 0))

    def _on_coin_step(self, ts_step):   # 397-408
        step = Step()
        step.fault_log.extend(ts_step.fault_log)   # (already CoinFault)
        step.messages.extend(self._msg(Message.COIN, 0, tm.message) for tm in ts_step.messages)
        if ts_step.output:
            self.coin_state = bool(ts_step.output[0])
            step.extend(self._try_update_epoch())
        return step

    def _try_update_epoch(self):   # 416-435
        if self.decision is not None:
            return Step()
        if not isinstance(self.coin_state, bool):
            return Step()
        coin = self.coin_state
        if self.conf_values is None:
            return Step()
        def_bin_value = bs_definite(self.conf_values)
        if def_bin_value is not None and def_bin_value == coin:
            return self._decide(coin)
        return self._update_epoch(coin if def_bin_value is None else def_bin_value)

    def _new_coin_state(self):   # 439-450
        if self.epoch % 3 == 0:
            return True
        if self.epoch % 3 == 1:
            return False
        return ThresholdSign(self.our_id, self.f, self.table, (self.epoch - 2) // 3)

    def _decide(self, b):
        """binary_agreement.rs:453-468: Term(b) goes out with epoch + 1 and is
        not handled by the decider itself."""
        if self.decision is not None:
            return Step()
        step = Step()
        step.output.append(b)
        self.decision = b
        self.decision_epoch = self.epoch
        step.messages.append(self._msg(Message.TERM, b, epoch=self.epoch + 1))
        return step

    def _try_finish_conf_round(self):   # 471-482
        if self.conf_values is None or self._count_conf() < self.n - self.f:
            return Step()
        if isinstance(self.coin_state, bool):
            return Step()
        ts_step = self.coin_state.sign()
        return self._on_coin_step(ts_step).join(self._try_update_epoch())

    def _count_conf(self):   # 485-488
        return sum(1 for c in self.received_conf.values() if bs_subset(c, self.sbv.bin_values))

    def _update_epoch(self, b):
        """binary_agreement.rs:491-520."""
        self.sbv.clear(self.received_term)
        self.received_conf = {}
        for v in (False, True):   # BoolMultimap iterates `false` first
            for s in sorted(self.received_term[v]):
                self.received_conf[s] = bs_from(v)
        self.conf_values = None
        self.epoch += 1
        self.coin_state = self._new_coin_state()
        self.estimated = b
        step = self._handle_sbvb_step(self.sbv.send_bval(b))
        epoch = self.epoch
        epoch_state = self.incoming_queue.pop(epoch, {})
        for sender_id in sorted(epoch_state):
            for kind, value, tampered in epoch_state[sender_id].messages():
                step.extend(self._handle_content(sender_id, kind, value, tampered))
                if self.decision is not None or self.epoch > epoch:
                    return step
        return step
