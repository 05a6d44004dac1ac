"""The BinaryAgreement state machine on the GPU (hbbft_amd/ba_sim.py,
hbbft_amd/csrc/ba_sim.hip, ba_node.hpp) against the host restatement.

Every scenario runs twice: through the GPU state machine (every node of every
instance in synchronous rounds) and through hbbft_amd/binary_agreement.py
nodes driven round by round by tests/ba_net.py on the same coin tables.  Every
node's decision, decision epoch and fault log (blamed node and FaultKind, in
order), the round count and the records emitted in every round must be EQUAL.

Sizes: N = 1 (f = 0, the thresholds coincide), 4, 7, 10, 33 (a second, partly
filled mask word), 64 (two full words, a full wave per instance).  Kinds
(tests/ba_net.py KINDS): honest runs with unanimous, split and random inputs,
nodes without input, SILENT / TWO_FACED / BAD_COIN / REPLAY / AHEAD (1, 2,
1001) / REPLAY_AHEAD (the queue's duplicate faults) nodes and a mixture, each instance with forced coin tables of its own
seed.  Further: every launch form, the driver's rejections, and the real coin
(coin_plane over the G2 kernels) at N = 4 and 7.
"""
import json
import os

import numpy as np
import pytest
import torch

import ba_net
from hbbft_amd import ba_sim
from hbbft_amd.ba_sim import AHEAD, BAD_COIN, HONEST, Instance, Scenario
from hbbft_amd.binary_agreement import CoinSlotError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SIZES = [1, 4, 7, 10, 33, 64]


def _count(n):
    return 12 if n < 33 else 4


def assert_equal_to_host(scn, run, host):
    for i, h in enumerate(host):
        for j in range(scn.n):
            where = (scn.n, i, j)
            assert run.decisions[(i, j)] == h.decisions[j], where
            assert run.decision_epochs[(i, j)] == h.decision_epochs[j], where
            assert run.faults[(i, j)] == h.faults[j], where
    rounds = max(h.rounds for h in host)
    assert run.rounds == rounds
    assert run.emitted == [sum(h.emitted[r] for h in host if r < h.rounds) for r in range(rounds)]


def assert_honest_properties(scn, run):
    """Agreement, validity and termination among the honest nodes, on the
    GPU's results by themselves."""
    for i, inst in enumerate(scn.instances):
        ba_net.check_properties({j: run.decisions[(i, j)] for j in range(scn.n)}, inst.inputs,
                                inst.honest())
        for j in inst.honest():   # no honest node is ever blamed
            assert all(inst.role[b] != HONEST for b, _ in run.faults[(i, j)])


@pytest.mark.parametrize("kind", ba_net.KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_matches_host(n, kind):
    scn, host = ba_net.scenario(n, kind, _count(n))
    run = ba_sim.run(scn)
    assert_equal_to_host(scn, run, host)
    assert_honest_properties(scn, run)


def test_scenarios_reach_what_they_are_for():
    """The seeded scenarios span several epochs, both coin outcomes, the
    queue and every fault kind (else the equalities above say little)."""
    epochs, kinds, queued = set(), set(), 0
    for n in (4, 7, 10):
        for kind in ba_net.KINDS:
            scn, host = ba_net.scenario(n, kind, _count(n))
            for h in host:
                epochs |= {e for e in h.decision_epochs.values() if e is not None}
                kinds |= {k for fl in h.faults.values() for _, k in fl}
                queued = max(queued, h.max_queued_ahead)
    assert {0, 1, 2, 3} <= epochs and max(epochs) >= 5, epochs
    assert kinds == set(ba_sim.FAULT_KINDS), kinds
    assert queued >= 2


@pytest.mark.parametrize("n", SIZES)
def test_launch_forms_agree_and_runs_repeat(n):
    """Every launch form that ships, forced through hbrbc_ba_args.form, on one
    mixed scenario per N: identical to the host and so to each other; a second
    run of the same rank object is identical to the first."""
    scn, host = ba_net.scenario(n, "mixture", _count(n))
    assert sorted(ba_sim.FORMS.values()) == [1, 2, 3]   # enum hbrbc_ba_form, all but AUTO
    for name, form in sorted(ba_sim.FORMS.items()) + [("auto", ba_sim.FORM_AUTO)]:
        rank = ba_sim.BaRank.from_scenario(scn, 0, max_faults=max(64, 8 * n), form=form)
        first = ba_sim.BaRun(rank, ba_sim.run_rounds(rank))
        assert_equal_to_host(scn, first, host)
        again = ba_sim.BaRun(rank, ba_sim.run_rounds(rank))
        for attr in ("decisions", "decision_epochs", "faults", "rounds", "emitted", "records"):
            assert getattr(again, attr) == getattr(first, attr), (name, attr)


def test_simulate_returns_the_four_results():
    scn, host = ba_net.scenario(7, "random", 12)
    dec, ep, faults, rounds = ba_sim.simulate(scn)
    assert rounds == max(h.rounds for h in host)
    assert all(dec[(i, j)] == h.decisions[j] and ep[(i, j)] == h.decision_epochs[j] and
               faults[(i, j)] == h.faults[j] for i, h in enumerate(host) for j in range(7))


# ---- arbitrary inboxes ----------------------------------------------------------
def _header(m):
    return m.kind | (m.value << 8) | (m.tampered << 12) | (m.epoch << 16)


@pytest.mark.parametrize("n", [4, 7, 33])
def test_random_inboxes_match_host(n):
    """Rounds whose inboxes are written by the test, not by the nodes: seeded
    random records of every kind, value and sender, for past, current and
    future epochs (inside the ring, and past epoch + 1000), to random
    recipients.  Synchronous runs keep the honest nodes level, so the queue,
    its replay, nested epoch changes and Terms replayed from the queue are
    rare there; here they are the common case.  After every round each node's
    emitted records (in order), fault log, decision and decision epoch equal
    those of a host node fed the same messages in the same order."""
    import random
    from hbbft_amd.binary_agreement import BinaryAgreement, CoinTable, Message
    rng = random.Random(1000 + n)
    count, Q, max_out, rounds, coins = 6, 4, 48, 24, 40
    W = (n + 31) // 32
    insts = [Instance(n, [rng.choice([0, 1, ba_sim.NONE]) for _ in range(n)],
                      coin_bits=[rng.randrange(2) for _ in range(coins)]) for _ in range(count)]
    scn = Scenario(n, insts, coins, Q)
    rank = ba_sim.BaRank.from_scenario(scn, 0, max_out=max_out, max_faults=4096)
    rank.reset()
    host = [[BinaryAgreement(j, n, scn.host_table(i)) for j in range(n)] for i in range(count)]
    faults = [[[] for _ in range(n)] for _ in range(count)]
    seen = {"nested": 0, "term_moved": 0, "replayed": 0, "depth": 0}

    def watch(nd):   # which of the rare paths the host nodes took
        upd, term, content = nd._update_epoch, nd._handle_term, nd._handle_content

        def update(b):
            seen["nested"] += seen["depth"] > 0
            seen["depth"] += 1
            try:
                return upd(b)
            finally:
                seen["depth"] -= 1

        def handle_term(s, b):
            e0 = nd.epoch
            st = term(s, b)
            seen["term_moved"] += nd.epoch != e0   # handle_conf ran on the next epoch's state
            return st

        def handle_content(*a):
            seen["replayed"] += seen["depth"] > 0
            return content(*a)
        nd._update_epoch, nd._handle_term, nd._handle_content = update, handle_term, handle_content
    for row in host:
        for nd in row:
            watch(nd)
    all_bits = [sum(1 << b for b in range(32) if 32 * w + b < n) for w in range(W)]

    def check(r, steps):
        out = rank.out.cpu().numpy().view(np.uint32)
        oc = rank.out_count.cpu().numpy()
        assert int(rank.hist[r, 1]) == 0, (r, int(rank.hist[r, 1]))
        dec, ep = rank.decisions()
        logs = rank.fault_logs()
        for i in range(count):
            for j in range(n):
                want = []
                for tm in steps[i][j].messages:
                    mask = list(all_bits)
                    mask[j // 32] &= ~(1 << (j % 32))
                    want.append([_header(tm.message)] + mask)
                assert out[i, j, :oc[i, j]].tolist() == want, (r, i, j)
                faults[i][j] += [(f.node_id, f.kind.name) for f in steps[i][j].fault_log]
                assert logs[(i, j)] == faults[i][j], (r, i, j)
                nd = host[i][j]
                assert (None if dec[i, j] == ba_sim.NONE else bool(dec[i, j])) == nd.decision
                assert nd.decision is None or int(ep[i, j]) == nd.decision_epoch

    from hbbft_amd.broadcast import Step
    rank.round(0)
    check(0, [[host[i][j].propose(bool(v)) if v != ba_sim.NONE else Step()
               for j, v in enumerate(insts[i].inputs)] for i in range(count)])
    for r in range(1, rounds):
        inbox = np.zeros((count, n, max_out, 1 + W), np.uint32)
        cnt = np.zeros((count, n), np.int32)
        steps = [[Step() for _ in range(n)] for _ in range(count)]
        msgs = [[[] for _ in range(n)] for _ in range(count)]
        for i in range(count):
            live = [nd.epoch for nd in host[i] if nd.decision is None] or [0]
            lo, hi = min(live), max(live)
            for s in range(n):
                for e in range(rng.randrange(4)):
                    kind = rng.choice([0] * 6 + [1] * 6 + [2] * 3 + [4] * 3 + [3])   # (Terms end a run)
                    value = rng.choice([1, 2, 3]) if kind == 2 else rng.randrange(2)
                    epoch = rng.choice([lo, lo, hi, hi, hi + 1, lo + 1, lo + 2, lo + Q,
                                        max(0, lo - 1), hi + 1040, hi + 1100])   # (the far ones stay
                    # past epoch + 1000 while the receiver moves on during the round)
                    m = Message(epoch, kind, 0 if kind == 4 else value,
                                rng.randrange(2) if kind == 4 else 0)
                    # random recipients; a future message only to nodes whose ring holds it
                    to = [j for j in range(n) if j != s and rng.random() < 0.7 and
                          not Q < epoch - host[i][j].epoch <= 1000]
                    rec = [_header(m)] + [sum(1 << (j % 32) for j in to if j // 32 == w)
                                          for w in range(W)]
                    inbox[i, s, cnt[i, s]] = rec
                    cnt[i, s] += 1
                    msgs[i][s].append((m, to))
        rank.inbox.copy_(torch.from_numpy(inbox.view(np.int32)))
        rank.inbox_count.copy_(torch.from_numpy(cnt))
        for i in range(count):   # the host, per node: (sender, emission) order
            for j in range(n):
                for s in range(n):
                    for m, to in msgs[i][s]:
                        if j in to:
                            steps[i][j].extend(host[i][j].handle_message(s, m))
        rank.round(r)
        check(r, steps)
    epochs = [nd.epoch for row in host for nd in row]
    assert max(epochs) >= 3 and any(nd.decision is not None for row in host for nd in row)
    assert seen["replayed"] and seen["nested"] and seen["term_moved"], seen


# ---- rejections ---------------------------------------------------------------
def _ahead_instance(n, ahead):
    role = [HONEST] * n
    role[1] = AHEAD
    return Instance(n, [j % 2 for j in range(n)], role, ahead=ahead, coin_bits=[1, 0, 1, 0, 1, 0])


def test_message_beyond_the_queue_ring_is_rejected():
    """An AHEAD node 6 epochs ahead with a ring of 4: the driver raises; with
    the ring raised to 8 the same scenario runs and matches the host."""
    scn = Scenario(7, [_ahead_instance(7, 6)] * 3, queue_epochs=4)
    host = ba_net.run_scenario(scn)
    assert 4 < max(h.max_queued_ahead for h in host) <= 8
    with pytest.raises(RuntimeError, match="ring"):
        ba_sim.run(scn)
    run = ba_sim.run(scn, queue_epochs=8)
    assert_equal_to_host(scn, run, host)
    assert_honest_properties(scn, run)


def test_max_out_too_small_is_rejected():
    scn, host = ba_net.scenario(7, "split", 12)
    with pytest.raises(RuntimeError, match="more than 1 messages"):
        ba_sim.run(scn, max_out=1)
    assert_equal_to_host(scn, ba_sim.run(scn, max_out=8), host)


def test_coin_slot_past_the_tables_is_rejected():
    """A run that needs coin slot 1 with tables of one slot: the host
    restatement raises CoinSlotError, the driver RuntimeError."""
    n = 4
    scn, host = ba_net.scenario(n, "two_faced", 12)
    long = [inst for inst, h in zip(scn.instances, host)
            if max(e for e in h.decision_epochs.values() if e is not None) >= 5]
    assert long
    short = Scenario(n, long[:1], coins=1)
    with pytest.raises(CoinSlotError):
        ba_net.run_scenario(short)
    with pytest.raises(RuntimeError, match="coin slot"):
        ba_sim.run(short)


# ---- the real coin --------------------------------------------------------------
def _gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


def _stand_in_hashes(count):
    """H = [h] G2::one() for seeded scalars h: STAND-INS for hash_g2(coin id)
    (the crate's hash_g2 is a ChaCha-seeded sample this project does not
    restate); any G2 point serves the share checks and the combine."""
    from hbbft_amd import threshold as T
    gen = next(x for x in _gold("compressed_vectors.json")["g2"] if x["name"] == "g2_valid_0")
    one = torch.from_numpy(np.frombuffer(bytes.fromhex(gen["u"]), np.uint8).copy()).view(1, 192)
    gtab = T.g2_points_prepare(one.to("cuda:0"))
    hs = [(0xC01 + 977 * c + (1 << (130 + c))).to_bytes(32, "big") for c in range(count)]
    sc = torch.from_numpy(np.frombuffer(b"".join(hs), np.uint8).reshape(count, 32).copy())
    rows = torch.zeros(count, dtype=torch.int32, device="cuda:0")
    _, h192, _, st = T.g2_mul_prepared(gtab, 1, rows, sc.to("cuda:0"))
    assert st.cpu().tolist() == [0] * count
    return [bytes(v) for v in h192.cpu().numpy()]


@pytest.mark.parametrize("which", [0, 1])
def test_real_coin(which):
    """coin_plane at N = 4 and N = 7, two instances, two coin slots: every
    genuine share passes and every tampered one fails; every combined
    signature verifies against the master key; another f + 1 subset of the
    same shares gives the same parity (the uniqueness the by-reference coin
    rests on); a scenario with a BAD_COIN node on those tables matches the
    host on the same tables."""
    from hbbft_amd import keygen as K
    tr = _gold("keygen_vectors.json")["transcripts"][which]
    n, f = len(tr["polys"]), tr["t"]
    assert (n, f) == ((4, 1), (7, 2))[which] and f == (n - 1) // 3
    keys = K.sync_key_gen_network(f, [[bytes.fromhex(c) for c in p] for p in tr["polys"]])
    role = [HONEST] * n
    role[0] = BAD_COIN   # the lowest sender: its share is handled before f + 1 good ones
    scn = Scenario(n, [Instance(n, [j % 2 for j in range(n)], role),
                       Instance(n, [(j // 2) % 2 for j in range(n)], role)], coins=2)
    share_ok, coin, info = ba_sim.coin_plane(scn, _stand_in_hashes(4), keys)
    so = share_ok.cpu().numpy()
    assert so.shape == (2, 2, 2, n) and coin.shape == (2, 2)
    assert (so[:, :, 0, :] == 1).all() and (so[:, :, 1, :] == 0).all()
    assert bool((info["verified"] == 1).all())
    par, ver = ba_sim.coin_parity(info, list(range(n - f - 1, n)), "cuda:0")   # another subset
    assert bool((ver == 1).all())
    assert par.cpu().tolist() == coin.view(-1).cpu().tolist()
    scn.set_tables(share_ok, coin)
    try:
        host = ba_net.run_scenario(scn)
    except CoinSlotError:   # the run needs a third coin: then the driver rejects it too
        with pytest.raises(RuntimeError, match="coin slot"):
            ba_sim.run(scn)
        return
    run = ba_sim.run(scn)
    assert_equal_to_host(scn, run, host)
    assert_honest_properties(scn, run)
    assert max(e for e in run.decision_epochs.values() if e is not None) >= 2   # a coin was flipped
    assert any(k == "CoinFault" for fl in run.faults.values() for _, k in fl)
