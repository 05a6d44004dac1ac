"""The host restatement of BinaryAgreement (hbbft_amd/binary_agreement.py), no
GPU: the properties of the reference's tests/binary_agreement.rs under an
asynchronous random-order network and under the synchronous rounds of the GPU
state machine (tests/ba_net.py); the facts that follow from the `true, false,
coin` schedule; one hand-built message sequence per fault kind and per subtle
point of the reference's handlers; and the ABI of the GPU entry
(hbrbc_ba_state_bytes; the hbrbc_ba_args layouts are in tests/test_crate.py)."""
import ctypes
import random

import pytest

import ba_net
from ba_net import NONE, SILENT, check_properties, run_random, run_rounds
from hbbft_amd import binary_agreement as ba
from hbbft_amd.binary_agreement import BinaryAgreement, CoinTable, FaultKind, Message

BVAL, AUX, CONF, TERM, COIN = range(5)


def _table(n, seed=0, slots=16):
    rng = random.Random(seed)
    return CoinTable.forced(n, [rng.randrange(2) for _ in range(slots)])


def _inputs(n, how, rng):
    return {"true": [1] * n, "false": [0] * n}.get(how) or [rng.randrange(2) for _ in range(n)]


def _faults(step):
    return [(f.node_id, f.kind) for f in step.fault_log]


def _msgs(step):
    return [tm.message for tm in step.messages]


# ---- properties (tests/binary_agreement.rs) ---------------------------------
@pytest.mark.parametrize("n", range(1, 11))
@pytest.mark.parametrize("how", ["true", "false", "random"])
def test_properties_random_order(n, how):
    f = (n - 1) // 3
    for seed in range(3):
        for nsilent in range(f + 1):
            rng = random.Random("%d/%s/%d/%d" % (n, how, seed, nsilent))
            inputs = _inputs(n, how, rng)
            silent = set(rng.sample(range(n), nsilent))
            nodes = run_random(n, inputs, _table(n, seed), silent, rng)
            honest = [j for j in range(n) if j not in silent]
            check_properties({j: nd.decision for j, nd in enumerate(nodes)}, inputs, honest)


@pytest.mark.parametrize("n", range(1, 11))
@pytest.mark.parametrize("how", ["true", "false", "random"])
def test_properties_round_net(n, how):
    f = (n - 1) // 3
    for seed in range(3):
        for nsilent in range(f + 1):
            rng = random.Random("%d/%s/%d/%d" % (n, how, seed, nsilent))
            inputs = _inputs(n, how, rng)
            silent = set(rng.sample(range(n), nsilent))
            role = [SILENT if j in silent else 0 for j in range(n)]
            res = run_rounds(n, inputs, _table(n, seed), role)
            check_properties(res.decisions, inputs, [j for j in range(n) if j not in silent])
            assert not any(res.faults.values())


@pytest.mark.parametrize("kind", ba_net.KINDS)
@pytest.mark.parametrize("n", [4, 7, 10])
def test_properties_of_the_seeded_scenarios(n, kind):
    """The scenarios the GPU tests run (roles included): the honest nodes
    agree, terminate and decide an honest node's input, and a fault never
    blames an honest node."""
    scn, host = ba_net.scenario(n, kind, 12)
    for inst, res in zip(scn.instances, host):
        check_properties(res.decisions, inst.inputs, inst.honest())
        for j in inst.honest():
            assert all(inst.role[b] != 0 for b, _ in res.faults[j]), (kind, res.faults[j])


# ---- the coin schedule --------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 7, 10])
def test_unanimous_inputs_decide_by_schedule(n):
    """Epoch 0's coin is `true`, epoch 1's `false`: all-honest unanimous true
    decides in epoch 0, unanimous false in epoch 1."""
    for b, epoch in ((1, 0), (0, 1)):
        res = run_rounds(n, [b] * n, _table(n))
        assert set(res.decisions.values()) == {b}
        assert set(res.decision_epochs.values()) == {epoch}


def test_single_node_decides_in_round_zero():
    for b, epoch in ((True, 0), (False, 1)):
        node = BinaryAgreement(0, 1, _table(1))
        step = node.propose(b)
        assert step.output == [b] and node.decision is b and node.decision_epoch == epoch
        assert _msgs(step)[-1] == Message(epoch + 1, TERM, b)
    res = run_rounds(1, [1], _table(1))
    assert res.rounds == 2 and res.emitted == [3, 0]   # BVal, Aux, Term; nothing after


# ---- handle_message (binary_agreement.rs:245-269) ----------------------------
def _node(n=4, me=0, epoch=0, slots=4, coin=(1, 0, 1, 0)):
    node = BinaryAgreement(me, n, CoinTable.forced(n, list(coin)[:slots]))
    for _ in range(epoch):   # bare epoch moves: no estimate, nothing queued
        node.conf_values = None
        node.epoch += 1
        node.coin_state = node._new_coin_state()
    return node


def test_decided_node_ignores_everything():
    node = _node()
    node._decide(True)
    for m in (Message(0, BVAL, 1), Message(5, TERM, 0), Message(2000, AUX, 1)):
        st = node.handle_message(1, m)
        assert not st.messages and not st.fault_log and not st.output
    assert not node.incoming_queue and node.received_term == {False: set(), True: set()}


def test_past_epochs_are_dropped_unless_term():
    node = _node(epoch=1)
    for kind in (BVAL, AUX, CONF, COIN):
        st = node.handle_message(1, Message(0, kind, 1))
        assert not st.messages and not st.fault_log
    assert not node.sbv.received_bval[True] and not node.received_conf
    node.handle_message(1, Message(0, TERM, 1))
    assert node.received_term[True] == {1} and node.sbv.received_bval[True] == {1}


def test_agreement_epoch_at_1001_and_queue_at_1000():
    node = _node()
    st = node.handle_message(2, Message(1001, BVAL, 1))
    assert _faults(st) == [(2, FaultKind.AgreementEpoch)] and not node.incoming_queue
    st = node.handle_message(2, Message(1000, BVAL, 1))
    assert not st.fault_log and list(node.incoming_queue) == [1000]
    node = _node(epoch=1)
    assert _faults(node.handle_message(2, Message(1002, TERM, 1))) == [(2, FaultKind.AgreementEpoch)]
    assert not node.handle_message(2, Message(1001, TERM, 1)).fault_log


def test_future_messages_are_queued_term_included():
    node = _node()
    for m in (Message(1, BVAL, 0), Message(1, TERM, 1), Message(3, COIN, 0, 1)):
        st = node.handle_message(3, m)
        assert not st.messages and not st.fault_log
    assert sorted(node.incoming_queue) == [1, 3]
    got = node.incoming_queue[1][3]
    assert (got.bval, got.term) == (ba.FALSE, 1) and node.incoming_queue[3][3].coin == 1
    assert node.received_term == {False: set(), True: set()}   # not handled yet
    assert node.max_queued_ahead == 3


def test_queue_insertion_faults():
    node = _node()
    seq = [(Message(1, BVAL, 1), None), (Message(1, BVAL, 0), None),
           (Message(1, BVAL, 1), FaultKind.DuplicateBVal),
           (Message(1, AUX, 0), None), (Message(1, AUX, 0), FaultKind.DuplicateAux),
           (Message(1, CONF, ba.TRUE), None), (Message(1, CONF, ba.BOTH), FaultKind.MultipleConf),
           (Message(1, TERM, 1), None), (Message(1, TERM, 1), FaultKind.MultipleTerm),
           (Message(1, TERM, 0), FaultKind.MultipleTerm),
           (Message(2, COIN, 0), None), (Message(2, COIN, 0, 1), FaultKind.AgreementEpoch)]
    for m, want in seq:
        st = node.handle_message(2, m)
        assert _faults(st) == ([] if want is None else [(2, want)]), m
    # another sender's entries are its own
    assert not node.handle_message(3, Message(1, BVAL, 1)).fault_log
    assert node.incoming_queue[1][2].conf == ba.TRUE and node.incoming_queue[2][2].coin == 0


def test_current_epoch_conf_and_coin_overwrite_without_fault():
    node = _node(epoch=2)
    assert not node.handle_message(1, Message(2, CONF, ba.TRUE)).fault_log
    assert not node.handle_message(1, Message(2, CONF, ba.BOTH)).fault_log
    assert node.received_conf == {1: ba.BOTH}
    assert not node.handle_message(1, Message(2, COIN, 0)).fault_log
    assert not node.handle_message(1, Message(2, COIN, 0)).fault_log
    assert node.coin_state.received_shares == {1: 0}
    # a tampered copy is a fault and leaves the stored share alone
    assert _faults(node.handle_message(1, Message(2, COIN, 0, 1))) == [(1, FaultKind.CoinFault)]
    assert node.coin_state.received_shares == {1: 0}


# ---- the queue replay (binary_agreement.rs:510-518) --------------------------
def _spy(node):
    seen = []
    inner = node._handle_content

    def handle(sender, kind, value, tampered):
        seen.append((sender, kind, int(value), tampered))
        return inner(sender, kind, value, tampered)
    node._handle_content = handle
    return seen


def test_replay_order_senders_ascending_true_first():
    node = _node(n=7)
    for s in (5, 2):   # inserted in descending order, every kind, `false` before `true`
        for m in (Message(1, COIN, 0), Message(1, CONF, ba.BOTH), Message(1, AUX, 0),
                  Message(1, BVAL, 0), Message(1, AUX, 1), Message(1, BVAL, 1)):
            assert not node.handle_message(s, m).fault_log
    seen = _spy(node)
    node._update_epoch(True)
    # (our own BVal of the new epoch goes through the sbv instance's send)
    per = lambda s: [(s, BVAL, 1, 0), (s, BVAL, 0, 0), (s, AUX, 1, 0), (s, AUX, 0, 0),
                     (s, CONF, ba.BOTH, 0), (s, COIN, 0, 0)]
    assert seen == per(2) + per(5)
    assert node.epoch == 1 and 1 not in node.incoming_queue


def test_replay_term_sits_between_conf_and_coin():
    node = _node(n=7)
    for m in (Message(1, COIN, 0), Message(1, TERM, 0), Message(1, CONF, ba.FALSE)):
        node.handle_message(3, m)
    seen = _spy(node)
    node._update_epoch(True)
    assert seen == [(3, CONF, ba.FALSE, 0), (3, TERM, 0, 0), (3, COIN, 0, 0)]


def test_replay_stops_at_a_decision_and_drops_the_rest():
    node = _node(n=4)   # f = 1: two Terms decide
    node.handle_message(1, Message(1, TERM, 1))
    node.handle_message(2, Message(1, BVAL, 0))
    node.handle_message(2, Message(1, TERM, 1))
    node.handle_message(2, Message(1, COIN, 0))
    node.handle_message(3, Message(1, BVAL, 0))
    seen = _spy(node)
    step = node._update_epoch(False)
    assert node.decision is True and step.output == [True]
    assert seen[-1] == (2, TERM, 1, 0) and all(s != 3 for s, *_ in seen)
    assert 1 not in node.incoming_queue          # the whole epoch left the queue
    assert not node.sbv.received_bval[False] - {0, 2}


def test_replay_stops_when_the_epoch_moves_again():
    """n = 1 .. 3 have f = 0; at n = 2 the peer's queued BVal, Aux of epoch 1
    complete epoch 1 during the replay, and its Conf is never handled."""
    node = _node(n=2)
    for m in (Message(1, BVAL, 1), Message(1, AUX, 1), Message(1, CONF, ba.TRUE)):
        node.handle_message(1, m)
    node.handle_message(1, Message(2, BVAL, 1))
    seen = _spy(node)
    node._update_epoch(True)       # epoch 1: coin false, both vote true -> epoch 2
    assert node.epoch == 2 and not node.incoming_queue
    assert (1, CONF, ba.TRUE, 0) not in seen
    assert seen[-1] == (1, BVAL, 1, 0) and node.sbv.received_bval[True] == {0, 1}


# ---- sbv_broadcast.rs ---------------------------------------------------------
def test_f0_double_threshold_fires_2f1_before_f1():
    node = _node(n=2)              # f = 0: 2f + 1 = f + 1 = 1
    step = node.handle_message(1, Message(0, BVAL, 1))
    assert _msgs(step) == [Message(0, AUX, 1), Message(0, BVAL, 1)]
    assert node.sbv.bin_values == ba.TRUE and node.sbv.sent_bval == ba.TRUE
    assert node.sbv.received_bval[True] == {0, 1} and node.sbv.received_aux[True] == {0}


def test_f1_thresholds_are_equalities():
    node = _node(n=4)
    assert not _msgs(node.handle_message(1, Message(0, BVAL, 0)))
    # f + 1: our BVal goes out; handling it makes 2f + 1: the Aux follows
    assert _msgs(node.handle_message(2, Message(0, BVAL, 0))) == [Message(0, BVAL, 0),
                                                                  Message(0, AUX, 0)]
    assert node.sbv.bin_values == ba.FALSE
    node = _node(n=7)
    for s in (1, 2):
        assert not _msgs(node.handle_message(s, Message(0, BVAL, 0)))
    assert _msgs(node.handle_message(3, Message(0, BVAL, 0))) == [Message(0, BVAL, 0)]
    assert node.sbv.bin_values == ba.NONE
    assert _msgs(node.handle_message(4, Message(0, BVAL, 0))) == [Message(0, AUX, 0)]
    assert not _msgs(node.handle_message(5, Message(0, BVAL, 0)))   # 2f + 2: nothing
    assert _faults(node.handle_message(5, Message(0, BVAL, 0))) == [(5, FaultKind.DuplicateBVal)]
    assert not node.handle_message(5, Message(0, AUX, 0)).fault_log
    assert _faults(node.handle_message(5, Message(0, AUX, 0))) == [(5, FaultKind.DuplicateAux)]


# ---- Term --------------------------------------------------------------------
def test_term_counts_as_bval_aux_and_conf_and_logs_duplicates():
    node = _node(n=7)              # f = 2: three Terms decide
    node.handle_message(1, Message(0, BVAL, 1))
    node.handle_message(1, Message(0, AUX, 1))
    st = node.handle_message(1, Message(1, TERM, 1))     # queued: epoch + 1
    assert not st.fault_log and node.received_term[True] == set()
    st = node.handle_message(1, Message(0, TERM, 1))
    assert _faults(st) == [(1, FaultKind.DuplicateBVal), (1, FaultKind.DuplicateAux)]
    assert node.received_term[True] == {1} and node.received_conf == {1: ba.TRUE}
    st = node.handle_message(2, Message(0, TERM, 1))
    assert not st.fault_log and node.decision is None
    assert node.sbv.received_bval[True] == {1, 2} and node.sbv.received_aux[True] == {1, 2}
    assert node.received_conf == {1: ba.TRUE, 2: ba.TRUE}
    st = node.handle_message(3, Message(0, TERM, 1))     # more than f agree
    assert st.output == [True] and node.decision is True
    assert 3 not in node.sbv.received_bval[True]         # decided before the BVal / Aux / Conf
    assert _msgs(st) == [Message(1, TERM, 1)]


def test_new_epoch_starts_from_the_term_senders():
    node = _node(n=7)
    node.handle_message(4, Message(0, TERM, 0))
    node.handle_message(5, Message(0, TERM, 1))
    node.handle_message(5, Message(0, TERM, 0))          # (a faulty sender in both sets)
    node.handle_message(6, Message(0, CONF, ba.BOTH))
    node._update_epoch(True)
    assert node.sbv.received_bval == {False: {4, 5}, True: {0, 5}}
    assert node.sbv.received_aux == {False: {4, 5}, True: {5}}
    assert node.received_conf == {4: ba.FALSE, 5: ba.TRUE}   # `true` is inserted last; 6 is gone
    assert node.sbv.bin_values == ba.NONE and node.sbv.sent_bval == ba.TRUE
    assert node.conf_values is None and node.coin_state is False and node.estimated is True


def test_decide_sends_term_for_the_next_epoch_and_does_not_handle_it():
    node = _node(n=4, epoch=1)
    step = node._decide(False)
    assert _msgs(step) == [Message(2, TERM, 0)] and step.output == [False]
    assert node.received_term == {False: set(), True: set()}
    assert node.decision_epoch == 1 and not node._decide(True).messages and node.decision is False


# ---- the coin -----------------------------------------------------------------
def test_share_is_sent_at_early_coin_termination_and_not_handled():
    """threshold_sign.rs:227-247: f + 1 shares arrive before the node's own
    Conf round finishes; try_output sets `terminated`, then sign() sends the
    node's share, whose own handle_message returns at once."""
    node = _node(n=4, epoch=2, coin=(1,))
    ts = node.coin_state
    assert isinstance(ts, ba.ThresholdSign) and ts.slot == 0
    assert not _msgs(node.handle_message(1, Message(2, COIN, 0)))
    step = node.handle_message(2, Message(2, COIN, 0))
    assert _msgs(step) == [Message(2, COIN, 0)]
    assert ts.terminated and ts.had_input and ts.received_shares == {1: 0, 2: 0}
    assert node.coin_state is True and node.epoch == 2 and node.conf_values is None
    # the coin is known; the epoch ends when the sbv round outputs
    for s in (1, 2, 3):
        node.handle_message(s, Message(2, BVAL, 0))
    for s in (1, 2):
        node.handle_message(s, Message(2, AUX, 0))
    assert node.epoch == 3 and node.estimated is False   # {false} against coin true


def test_bad_share_is_a_coin_fault_and_does_not_count():
    node = _node(n=4, epoch=2, coin=(0,))
    st = node.handle_message(1, Message(2, COIN, 0, 1))
    assert _faults(st) == [(1, FaultKind.CoinFault)] and not node.coin_state.received_shares
    node.handle_message(2, Message(2, COIN, 0))
    assert isinstance(node.coin_state, ba.ThresholdSign)   # one valid share: no coin yet
    node.handle_message(3, Message(2, COIN, 0))
    assert node.coin_state is False


def test_conf_round_signs_then_tries_the_epoch_twice():
    """try_finish_conf_round (471-482): sign(), on_coin_step and a second
    try_update_epoch joined after it."""
    node = _node(n=4, epoch=2, coin=(1,))
    for s in (1, 2, 3):
        node.handle_message(s, Message(2, BVAL, 1))
    node.handle_message(1, Message(2, COIN, 0))
    calls = []
    inner = node._try_update_epoch
    node._try_update_epoch = lambda: (calls.append(node.epoch), inner())[1]
    step = node.handle_message(1, Message(2, AUX, 1))
    assert not calls and node.conf_values is None
    step = node.handle_message(2, Message(2, AUX, 1))   # N - f Aux with ours: Conf goes out
    assert _msgs(step) == [Message(2, CONF, ba.TRUE)] and node.conf_values == ba.TRUE
    node.handle_message(1, Message(2, CONF, ba.TRUE))
    step = node.handle_message(2, Message(2, CONF, ba.TRUE))   # N - f Confs: the coin
    assert _msgs(step)[0] == Message(2, COIN, 0)         # our share; with node 1's: f + 1
    assert calls == [2, 2] and node.decision is True and node.decision_epoch == 2
    assert _msgs(step)[1:] == [Message(3, TERM, 1)]


def test_coin_slot_past_the_table_is_an_error():
    node = _node(n=4, epoch=1, slots=1)
    node.coin_state = False
    node.conf_values = ba.TRUE     # epoch 1's coin is false: the epoch moves on to 2
    node._try_update_epoch()
    assert node.epoch == 2
    node = _node(n=4, epoch=4, slots=1)
    node.conf_values = ba.BOTH
    with pytest.raises(ba.CoinSlotError):
        node._try_update_epoch()   # epoch 5 is coin slot 1


# ---- the ABI of the GPU entry -------------------------------------------------
def test_state_block_size():
    """hbrbc_ba_state_bytes (include/hbrbc.h): per node epoch, flags and nine
    sender masks, then two bytes per sender and ring slot, rounded to 16;
    ba_sim.ba_state_bytes_host mirrors it."""
    import __graft_entry__
    __graft_entry__.build()
    import hbbft_amd as hb
    from hbbft_amd.ba_sim import ba_state_bytes_host
    L = hb.lib()
    L.hbrbc_ba_state_bytes.restype = ctypes.c_size_t
    L.hbrbc_ba_state_bytes.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    for n in (1, 4, 7, 31, 32, 33, 64, 128, 255):
        w = (n + 31) // 32
        for q in (1, 4, 16):
            want = (4 * (2 + 9 * w) + 2 * n * q + 15) & ~15
            got = L.hbrbc_ba_state_bytes(n, q)
            assert got == want and got % 16 == 0, (n, q, got, want)
            assert ba_state_bytes_host(n, q) == got
    assert 590 <= ba_state_bytes_host(64, 4) <= 600
