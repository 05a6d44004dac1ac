"""HoneyBadger epochs on the GPU (hbbft_amd/hb_sim.py, hbbft_amd/csrc/
hb_sim.hip) against the host restatement.

Every scenario runs twice: through the three round kernels, and through
hbbft_amd/honey_badger.py nodes driven in the same schedule by tests/hb_net.py.
Every node's batch (proposers and bytes) and batch round, all three fault logs
(blamed node and FaultKind, in order), the Subset results tests/
test_subset_sim.py compares, the round count and the per-round record totals
of all three protocols must be EQUAL.

Shapes (hb_net.GPU_SHAPES, the Subset instances of subset_net.GPU_SHAPES):
N = 1 (the batch leaves in round 0), 2 (f = 0); honest N = 4, 7; N = 4, 7, 10
with 1..f dead nodes and, where f allows it, a STRAY node; N = 7, 10 with a
seeded mixture of the hb_roles, the Subset adversaries, ciphertexts that do
not deserialise or verify and contributions that do not deserialise; N = 33
with a dead node in each mask word.  Each scenario mixes encrypted and plain
instances and both strategies.  Further: the batch point below a stray
record, the real decryption tables, repeated runs and the driver's limits.
"""
import json
import os
import random

import numpy as np
import pytest
import torch

import hb_net as hn
import subset_net as sn
from hbbft_amd import hb_sim, rbc_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def assert_equal_to_host(scn, run, host):
    n = scn.n
    for i, h in enumerate(host):
        for j in range(n):
            where = (n, i, j)
            assert run.batch[(i, j)] == h.batch[j], where
            assert run.batch_round[(i, j)] == h.batch_round[j], where
            assert run.outputs[(i, j)] == h.outputs[j], where
            assert run.accepted[(i, j)] == h.accepted[j], where
            for p in range(n):
                assert run.hb_faults[(i, j, p)] == h.hb_faults[(j, p)], where + (p,)
                assert run.decisions[(i, j, p)] == h.decisions[(j, p)], where + (p,)
                assert run.decision_epochs[(i, j, p)] == h.decision_epochs[(j, p)], where + (p,)
                assert run.bc_faults[(i, j, p)] == h.bc_faults[(j, p)], where + (p,)
                assert run.ba_faults[(i, j, p)] == h.ba_faults[(j, p)], where + (p,)
    rounds = max(h.rounds for h in host)
    assert run.rounds == rounds
    for mine, theirs in ((run.bc_emitted, "bc_emitted"), (run.ba_emitted, "ba_emitted"),
                         (run.hb_emitted, "hb_emitted")):
        assert mine == [sum(getattr(h, theirs)[r] for h in host if r < h.rounds)
                        for r in range(rounds)], theirs


@pytest.mark.parametrize("n,kind,count", hn.GPU_SHAPES)
def test_matches_host(n, kind, count):
    scn, host = hn.scenario(n, kind, count)
    if count > 1:   # encrypted and plain, Incremental and AllAtEnd in one launch
        assert {(i.encrypted, i.strategy) for i in scn.instances} >= {(True, 0), (False, 1)}
    run = hb_sim.run(scn)
    assert_equal_to_host(scn, run, host)
    if n == 1:
        assert all(r == 0 for r in run.batch_round.values())
    if kind == "honest":   # nobody misbehaves: full batches everywhere, no faults
        assert not any(run.hb_faults.values())
        for i, inst in enumerate(scn.instances):
            want = {p: (inst.plaintexts[p][0] if inst.encrypted
                        else inst.subset.broadcasts[p].values[0]) for p in range(n)}
            assert all(run.batch[(i, j)] == want for j in range(n))


def test_scenarios_reach_what_they_are_for():
    """The shapes log every fault kind of an epoch (UnexpectedHbMessageEpoch
    needs a second epoch: tests/test_honey_badger_cpu.py), both share faults
    at both timings -- UnverifiedDecryptionShareSender at once and postponed to
    set_ciphertext, UnexpectedDecryptionShare at once and at the removal at
    Done --, and batches that leave in step (b); the late-batch scenario has a
    batch that leaves at a p* below a non-accepted proposer with share records
    in that round (else the equalities above say little)."""
    kinds, tot = set(), dict(postponed=0, removed_at_done=0, immediate_unverified=0,
                             immediate_unexpected=0)
    step_b = no_batch = 0
    for n, kind, count in hn.GPU_SHAPES:
        _, host = hn.scenario(n, kind, count)
        for h in host:
            kinds |= {k for fl in h.hb_faults.values() for _, k in fl}
            for k in tot:
                tot[k] += getattr(h, k)
            step_b += len(h.late_batches)
            no_batch += sum(1 for j, b in h.batch.items() if b is None and h.outputs[j])
            if kind == "dead":   # the live nodes output the same batch without the dead ones
                live = [j for j in h.batch if h.outputs[j]]
                assert live and all(h.batch[j] == h.batch[live[0]] is not None for j in live)
    assert kinds == set(hb_sim.FAULT_KINDS)
    assert all(tot.values()), tot
    assert step_b and no_batch
    _, (late,) = hn.scenario_late_batch()
    assert hn.has_late_batch(late)
    assert all(q > p for _, _, p, above in late.late_batches for q in above)


def test_batch_leaves_below_a_stray_record():
    """The batch-point reduction: in one round of node 5 the batch leaves at
    p* = 5 while the dead proposer 6 has a STRAY node's record waiting; the
    thread of proposer 6 must log nothing (hn.scenario_late_batch says why the
    case takes more than f faults)."""
    scn, host = hn.scenario_late_batch()
    assert_equal_to_host(scn, hb_sim.run(scn), host)


def test_runs_repeat_and_simulate_returns_the_results():
    scn, host = hn.scenario(7, "dead", 6)
    ok, dec, payloads, _ = rbc_sim.data_plane(scn.subset.rbc_scenario(), 0)
    rank = hb_sim.HbRank(scn, 0, ok, dec)
    first = hb_sim.HbRun(rank, hb_sim.run_rounds(rank), payloads, scn)
    assert_equal_to_host(scn, first, host)
    again = hb_sim.HbRun(rank, hb_sim.run_rounds(rank), payloads, scn)
    attrs = ("batch", "batch_round", "hb_faults", "outputs", "accepted", "bc_faults", "ba_faults",
             "rounds", "bc_emitted", "ba_emitted", "hb_emitted")
    for attr in attrs + ("decisions", "decision_epochs", "dstate", "hb_records"):
        assert getattr(again, attr) == getattr(first, attr), attr
    assert hb_sim.simulate(scn) == tuple(getattr(first, a) for a in attrs)


def test_limits_raise():
    scn, host = hn.scenario(10, "faulty", 8)
    assert max(len(fl) for h in host for fl in h.hb_faults.values()) > 1
    with pytest.raises(RuntimeError, match="honey badger fault log overflow"):
        hb_sim.run(scn, hb_max_faults=1)
    with pytest.raises(RuntimeError, match="did not quiesce in 4 rounds"):
        hb_sim.run(scn, max_rounds=4)


# ---- the real decryption tables ------------------------------------------------
def _gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


def _g2_gen_table():
    from hbbft_amd import threshold as T
    gen = next(x for x in _gold("compressed_vectors.json")["g2"] if x["name"] == "g2_valid_0")
    one = torch.from_numpy(np.frombuffer(bytes.fromhex(gen["u"]), np.uint8).copy()).view(1, 192)
    return T.g2_points_prepare(one.to("cuda:0"))


def _scalars(values):
    raw = b"".join(v.to_bytes(32, "big") for v in values)
    return torch.from_numpy(np.frombuffer(raw, np.uint8).reshape(len(values), 32).copy()).to(
        "cuda:0")


def _ciphertexts(count, tampered):
    """Per ciphertext c: a stand-in H = [h_c] G2::one() (as tests/
    test_subset_sim.py makes its hashes), U = [r_c] G1::one(), W = [r_c] H --
    so e(G1, W) == e(U, H) -- for seeded r_c; the tampered one carries the W
    of its neighbour.  Returns ([(U48, W96, H192)], [r_c])."""
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    hs = [0x5B5 + 613 * c + (1 << (131 + c)) for c in range(count)]
    rs = [0xC1F + 977 * c + (1 << (97 + c)) for c in range(count)]
    rows = torch.zeros(count, dtype=torch.int32, device="cuda:0")
    htab, h192, _, st = T.g2_mul_prepared(_g2_gen_table(), 1, rows, _scalars(hs))
    assert st.cpu().tolist() == [0] * count
    _, _, w96, st = T.g2_mul_prepared(htab, count, torch.arange(count, dtype=torch.int32,
                                                                device="cuda:0"), _scalars(rs))
    assert st.cpu().tolist() == [0] * count
    _, _, u48, st = K.base_mul(_scalars(rs))
    assert st.cpu().tolist() == [0] * count
    u, w, h = u48.cpu().numpy(), w96.cpu().numpy(), h192.cpu().numpy()
    w[tampered] = w[(tampered + 1) % count]
    return [(bytes(u[c]), bytes(w[c]), bytes(h[c])) for c in range(count)], rs


@pytest.mark.parametrize("which", [0, 1])
def test_decrypt_plane_tables(which):
    """N = 4 and N = 7, four instances, real keys: the run on decrypt_plane's
    tables equals the host run on the same tables; ct_state is 2 exactly for
    the tampered ciphertext; share_ok variant 0 is all ones and variant 1 all
    zeros -- over the valid ciphertexts: a share is checked against W, e(share,
    H) == e(pk_i, W), so against the tampered W the honest shares fail as
    well (that row is all zeros; set_ciphertext rejects the ciphertext and no
    node ever consults it); the combine over nodes 0..f equals the combine over nodes f..2f byte for
    byte -- the uniqueness the by-reference plaintext rests on -- and both are
    [r] times the master key."""
    from hbbft_amd import keygen as K
    from hbbft_amd import threshold as T
    tr = [t for t in _gold("keygen_vectors.json")["transcripts"]
          if len(t["polys"]) == (4, 7)[which]]
    assert tr, "no key-generation transcript of that size"
    tr = tr[0]
    n, f = len(tr["polys"]), tr["t"]
    assert f == (n - 1) // 3
    keys = K.sync_key_gen_network(f, [[bytes.fromhex(c) for c in p] for p in tr["polys"]])
    count = 4
    insts = []
    for i in range(count):
        rng = random.Random("hb/decrypt_plane/%d/%d" % (n, i))
        si = sn.make_instance(n, "honest", rng, i)
        role = [hn.HONEST] * n
        role[rng.randrange(n)] = (hn.BAD_SHARE, hn.STRAY, hn.TWICE, hn.SILENT)[i]
        insts.append(hb_sim.Instance(si, i, True, i % 2, role,
                                     plaintexts=[[b"plain-%d-%d" % (i, p)] for p in range(n)]))
    scn = hb_sim.Scenario(n, insts, sn.COINS)
    tampered = n + 1   # instance 1, proposer 1
    cts, rs = _ciphertexts(count * n, tampered)
    ct_state, share_ok, g48, info = hb_sim.decrypt_plane(scn, cts, keys)
    cs = ct_state.cpu().numpy().reshape(-1)
    assert [int(v) for v in cs] == [2 if c == tampered else 0 for c in range(count * n)]
    so = share_ok.cpu().numpy()
    assert so.shape == (count * n, 1, 2, n)
    valid = cs == 0
    assert (so[valid, 0, 0, :] == 1).all() and (so[:, 0, 1, :] == 0).all()
    assert (so[tampered, 0, 0, :] == 0).all()
    other = hb_sim.decrypt_combine(info, list(range(f, 2 * f + 1)), "cuda:0")
    assert torch.equal(g48, other)
    master = T.g1_prepare(T._g1_rows([keys["key_set"][0][0]], "cuda:0"))
    _, _, want48, st = T.g1_mul_prepared(master, 1, torch.zeros(count * n, dtype=torch.int32,
                                                                 device="cuda:0"), _scalars(rs))
    assert st.cpu().tolist() == [0] * (count * n)
    assert torch.equal(g48, want48)
    scn.set_tables(ct_state, share_ok)
    assert scn.instances[1].ct_state[1] == [2]
    host = [hn.run_rounds(inst, sn._oracle(), tables=scn.host_tables(i))
            for i, inst in enumerate(scn.instances)]
    run = hb_sim.run(scn)
    assert_equal_to_host(scn, run, host)
    assert any("InvalidCiphertext" in [k for _, k in fl] for fl in run.hb_faults.values())
