"""The BinaryAgreement state machine of many instances and nodes on the GPU.

Control plane.  `hbrbc_ba_round` (hbbft_amd/csrc/ba_sim.hip, ba_node.hpp) runs
the reference's binary_agreement.rs, sbv_broadcast.rs and the ThresholdSign
state machine (threshold_sign.rs:127-270) for every (instance, node) in the
synchronous rounds of hbbft_amd/rbc_sim.py: what a node emits in round t is
delivered in round t + 1, handled in (sender index, emission order), own
records and records whose recipient mask excludes the node skipped; a node
handles its own messages at the moment it sends them, as the reference's
`send` does.  Round 0 is propose(input) of every node that has an input; a run
ends with the first round in which nobody emits.  One rank hosts all nodes.

Data plane.  The coin travels by reference: a Coin record names its sender's
signature share of the epoch's document (coin slot q is epoch 3q + 2) or a
tampered copy, and the state machine looks `is_share_valid` up in
share_ok[inst][q][tampered][sender] and the parity of the combined signature
in coin[inst][q].  That is exact: a BLS threshold signature is unique, any
f + 1 valid shares interpolate to the same [sk] H.  `coin_plane` computes both
tables with the G2 entries of hbbft_amd/threshold.py; a Scenario may carry
forced tables instead (seeded coin bits, every genuine share valid and every
tampered one invalid by construction).

Scenarios: per (instance, node) a role that transforms what LEAVES the node
(the node itself runs the honest state machine on what it receives and on its
own untransformed messages): SILENT, TWO_FACED, BAD_COIN, REPLAY, AHEAD and
REPLAY_AHEAD (include/hbrbc.h enum hbrbc_ba_role; the last one, both at once,
is what puts duplicates into a receiver's future-epoch queue: in synchronous
rounds the honest nodes run level, so a REPLAY node's doubles arrive in the
current epoch).  tests/test_ba_sim.py checks every
node's decision, decision epoch, fault log, the round count and the per-round
record totals against the host restatement (hbbft_amd/binary_agreement.py
driven by tests/ba_net.py RoundNet) on the same scenarios.
"""
import numpy as np
import torch

from . import rounds as shared
from .binary_agreement import CoinTable
from .rounds import I32, U32, USIZE

NONE = 0xFF
HONEST, SILENT, TWO_FACED, BAD_COIN, REPLAY, AHEAD, REPLAY_AHEAD = range(7)
# FaultKind (binary_agreement/mod.rs:110-129), in declaration order
FAULT_KINDS = ["DuplicateBVal", "DuplicateAux", "MultipleConf", "MultipleTerm", "AgreementEpoch",
               "CoinFault"]
MSG_KINDS = ["BVal", "Aux", "Conf", "Term", "Coin"]
FORM_AUTO, FORM_GLOBAL, FORM_STAGED, FORM_STAGED_W3 = range(4)
# every launch form that ships (enum hbrbc_ba_form)
FORMS = {"global": FORM_GLOBAL, "staged": FORM_STAGED, "staged_w3": FORM_STAGED_W3}
# hbrbc_ba_args.emitted[1]
BAD_OUT, BAD_QUEUE, BAD_COINS, BAD_EPOCH, BAD_STACK = 1, 2, 4, 8, 16

# hbrbc_ba_args.emitted[1] of a round, in the order the read-back looks at them
ROUND_FLAGS = (
    (BAD_QUEUE, "agreement: a message for an epoch beyond the future-epoch ring of "
                "{0.queue_epochs} slots (raise queue_epochs)"),
    (BAD_COINS, "agreement: a node reached a coin slot past the {0.coins} of the tables"),
    (BAD_OUT, "agreement: a node emitted more than {0.max_out} messages in a round"),
    (shared.ANY, "agreement: internal limit hit (flags {1:#x})"))

BaArgs = shared.args_struct(
    "BaArgs", "hbrbc_ba_args",
    [("count", USIZE), ("n", U32), ("max_out", U32), ("max_faults", U32), ("queue_epochs", U32),
     ("coins", U32), ("round", I32), ("form", U32)],
    ("input", "role", "flip", "ahead", "share_ok", "coin", "in_", "in_count", "out", "out_count",
     "state", "decision", "decision_epoch", "faults", "fault_count", "emitted", "active"))
BA_ROUND = shared.Entry("hbrbc_ba_round", BaArgs, sizes=("hbrbc_ba_state_bytes",))


def ba_state_bytes_host(n, queue_epochs):
    """hbrbc_ba_state_bytes without the library (hbbft_amd/csrc/launchers.hpp
    ba_state_bytes): per node the core -- epoch, flags and nine sender masks
    of W = ceil(n / 32) words -- and the future-epoch ring, two bytes per
    sender and slot; rounded to 16 bytes."""
    w = (n + 31) // 32
    return (4 * (2 + 9 * w) + 2 * n * queue_epochs + 15) & ~15


def state_bytes(n, queue_epochs):
    """hbrbc_ba_state_bytes of the library."""
    return BA_ROUND.bind().hbrbc_ba_state_bytes(n, queue_epochs)


# ------------------------------------------------------------------ scenario --
class Instance:
    """One agreement instance: inputs[j] 0, 1 or NONE (node j never proposes);
    role[j] what leaves node j; `flip` the recipients a TWO_FACED node lies
    to; `ahead` the epochs an AHEAD node adds; coin_bits[q] the forced coin of
    slot q (ignored when the Scenario carries computed tables)."""

    def __init__(self, n, inputs, role=None, flip=(), ahead=0, coin_bits=()):
        self.n = n
        self.inputs = [NONE if v is None or v == NONE else int(bool(v)) for v in inputs]
        self.role = list(role) if role is not None else [HONEST] * n
        self.flip = sorted(set(flip))
        self.ahead = int(ahead)
        self.coin_bits = [int(bool(b)) for b in coin_bits]
        assert len(self.inputs) == n and len(self.role) == n
        assert all(0 <= j < n for j in self.flip) and 0 <= self.ahead < 60000
        assert sum(r != HONEST for r in self.role) <= (n - 1) // 3, "more than f faulty nodes"

    def honest(self):
        return [j for j in range(self.n) if self.role[j] == HONEST]


class Scenario:
    """`count` instances of one validator count n with `coins` coin slots each
    (a run that reaches coin epoch 3 coins + 2 is an error raised to the
    caller).  Forced tables come from the instances' coin_bits; `set_tables`
    installs the ones coin_plane computed."""

    def __init__(self, n, instances, coins=None, queue_epochs=4):
        self.n = n
        self.instances = list(instances)
        assert self.instances and all(i.n == n for i in self.instances) and 1 <= n <= 255
        self.coins = max(1, max(len(i.coin_bits) for i in self.instances)) if coins is None \
            else coins
        self.queue_epochs = queue_epochs
        self._tables = None

    @property
    def count(self):
        return len(self.instances)

    def set_tables(self, share_ok, coin):
        """share_ok [count][coins][2][n], coin [count][coins] (arrays or tensors)."""
        so = np.asarray(torch.as_tensor(share_ok).cpu(), dtype=np.uint8)
        co = np.asarray(torch.as_tensor(coin).cpu(), dtype=np.uint8)
        assert so.shape == (self.count, self.coins, 2, self.n) and co.shape == so.shape[:2]
        self._tables = (so, co)

    def tables(self):
        if self._tables is not None:
            return self._tables
        cnt, n, C = self.count, self.n, self.coins
        so = np.zeros((cnt, C, 2, n), np.uint8)
        so[:, :, 0, :] = 1   # genuine shares valid, tampered ones invalid: by construction
        co = np.zeros((cnt, C), np.uint8)
        for r, i in enumerate(self.instances):
            bits = i.coin_bits[:C]
            co[r, :len(bits)] = bits
        return so, co

    def host_table(self, inst):
        """The CoinTable the host restatement of instance `inst` reads."""
        so, co = self.tables()
        return CoinTable(so[inst].tolist(), co[inst].tolist())

    def tensors(self, device):
        n, cnt = self.n, self.count
        W = (n + 31) // 32
        flip = np.zeros((cnt, W), np.uint32)
        for r, i in enumerate(self.instances):
            for j in i.flip:
                flip[r, j // 32] |= np.uint32(1 << (j % 32))
        so, co = self.tables()
        t = dict(input=torch.tensor([i.inputs for i in self.instances], dtype=torch.uint8),
                 role=torch.tensor([i.role for i in self.instances], dtype=torch.uint8),
                 flip=torch.from_numpy(flip.view(np.int32)),   # bit patterns (uint32 words)
                 ahead=torch.from_numpy(np.asarray([i.ahead for i in self.instances],
                                                   np.uint16).view(np.int16)),
                 share_ok=torch.from_numpy(so), coin=torch.from_numpy(co))
        return {k: v.contiguous().to(device) for k, v in t.items()}


# ------------------------------------------------------------- one rank -----
class BaRank(shared.HasAgreement):
    """Every node of `count` instances.  `sc`: the scenario tensors
    (Scenario.tensors).  form: FORM_AUTO or one of FORMS (the launch form is
    an argument of every round, hbrbc_ba_args.form)."""

    def __init__(self, n, count, coins, sc, device=0, max_out=24, max_faults=64, queue_epochs=4,
                 max_rounds=256, form=FORM_AUTO):
        self.n, self.count, self.coins = n, count, coins
        self.max_out, self.max_faults, self.queue_epochs = max_out, max_faults, queue_epochs
        self.max_rounds, self.form = max_rounds, form
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.device = dev
        self.sc = sc
        self.ag = shared.AgreementState(count, n, state_bytes(n, queue_epochs), max_out,
                                        max_faults, dev)
        # per round: records emitted, flags (hbrbc_ba_args.emitted of round r)
        self.hist = torch.zeros((max_rounds, 2), dtype=torch.int32, device=dev)
        self.records = 0   # records emitted over the last run (all rounds)

    @classmethod
    def from_scenario(cls, scn, device=0, **kw):
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        kw.setdefault("queue_epochs", scn.queue_epochs)
        return cls(scn.n, scn.count, scn.coins, scn.tensors(dev), device, **kw)

    def reset(self):
        """Fresh nodes (before round 0 of another run)."""
        self.ag.reset()
        self.hist.zero_()
        self.records = 0

    def round(self, r, active=None, stream=None):
        """Handle round r's inbox (round 0: propose).  active: None, or a
        device int32 scalar tensor -- the records emitted in round r - 1; the
        kernel returns at once when it is 0."""
        if r >= self.max_rounds:
            raise RuntimeError("agreement: round %d past max_rounds %d" % (r, self.max_rounds))
        a = BaArgs(count=self.count, n=self.n, max_out=self.max_out, max_faults=self.max_faults,
                   queue_epochs=self.queue_epochs, coins=self.coins, round=r, form=self.form)
        self.ag.write(a)
        shared.fill(a, self.sc, self.hist, r, active)
        BA_ROUND.launch(a, self.device, stream)

    def emitted(self, r):
        """Device int32 scalar: records emitted in round r."""
        return self.hist[r, 0]

    # -- results -------------------------------------------------------------
    def decisions(self):
        """([count][n] 0 / 1 / NONE, [count][n] the epoch of the decision)."""
        return self.decision.cpu().numpy(), self.decision_epoch.cpu().numpy().view(np.uint16)

    def fault_logs(self):
        """{(inst, node): [(blamed node, FaultKind name)]}."""
        return shared.fault_logs(self.fault_count, self.faults, self.max_faults, FAULT_KINDS)


ROUND_BATCH = 8   # rounds enqueued per read-back


def run_rounds(rank, stream=None, events=None):
    """Drive the state machine until no node emits a message (rounds.Rounds):
    batches of ROUND_BATCH rounds are enqueued, round r with the device count
    of round r - 1 as `active` (a quiescent network costs empty launches), and
    the per-round counts and flags are read back once per batch.  Returns the
    number of rounds, in rbc_sim's convention: the index of the first round
    without records + 1.  Every run starts from fresh nodes.  events: a list
    that receives ("agreement", start, end) device events of every launch."""
    def enqueue(r, phase):
        phase("agreement", rank.round, r, None if r == 0 else rank.emitted(r - 1))
        rank.ag.swap()
    return shared.Rounds([shared.Protocol(ROUND_FLAGS, rank, rank, "records")], rank.max_rounds,
                         ROUND_BATCH, "agreement", stream, events, reset=rank.reset,
                         enqueue=enqueue, read=shared.hist_rows([rank])).launch().wait()


class BaRun:
    """The results of one run: decisions / decision_epochs {(inst, node): 0,
    1 or None}, faults {(inst, node): [(blamed, kind)]}, rounds, emitted (the
    records of every round, all nodes)."""

    def __init__(self, rank, rounds):
        dec, ep = rank.decisions()
        self.decisions, self.decision_epochs = {}, {}
        for i in range(rank.count):
            for j in range(rank.n):
                d = int(dec[i, j])
                self.decisions[(i, j)] = None if d == NONE else d
                self.decision_epochs[(i, j)] = None if d == NONE else int(ep[i, j])
        self.faults = rank.fault_logs()
        self.rounds = rounds
        self.emitted = [int(v) for v in rank.hist[:rounds, 0].cpu().numpy()]
        self.records = rank.records


def run(scn, device=0, max_out=24, max_faults=None, queue_epochs=None, form=FORM_AUTO,
        max_rounds=256):
    """Every node of every instance of `scn` on one GPU: a BaRun.  Raises on a
    message beyond the queue ring, a coin slot past scn.coins, or more than
    max_out records of a node in a round."""
    if max_faults is None:   # REPLAY and TWO_FACED nodes cost a few faults per epoch
        max_faults = max(64, 8 * scn.n)
    rank = BaRank.from_scenario(scn, device, max_out=max_out, max_faults=max_faults,
                                queue_epochs=queue_epochs or scn.queue_epochs, form=form,
                                max_rounds=max_rounds)
    return BaRun(rank, run_rounds(rank))


def simulate(scn, device=0, **kw):
    """(decisions, decision_epochs, faults, rounds) of `run`."""
    r = run(scn, device, **kw)
    return r.decisions, r.decision_epochs, r.faults, r.rounds


# ------------------------------------------------------------- data plane ---
def coin_plane(scn, hashes192, keys, device=0):
    """The data plane of the coin, on the existing G2 entries (hbbft_amd/
    threshold.py): hashes192[inst * coins + q] is the document point H of
    (instance, coin slot) as an uncompressed G2 point -- the caller's hash_g2;
    keys is the dict keygen.sync_key_gen_network returns (secret_key_shares,
    key_shares, key_set).  All N shares of every document come from
    create_signature_shares; node j's tampered share of a document is its
    share of the instance's NEXT slot's document (a valid subgroup point that
    fails the check); sig_check_prepared runs over both; sig_combine_prepared
    combines the shares of nodes 0..f and the result is checked against the
    master key.  Returns (share_ok [count][coins][2][n], coin [count][coins]
    -- uint8 on the device --, info) with info: verified [count][coins] (the
    combined signature passes the master key), sig_tab / sig_count / docs (the
    share table, node-major: threshold.share_row) for further combines."""
    from . import threshold as T
    u32 = T._u32_tensor
    n, cnt = scn.n, scn.count
    C = len(hashes192)
    coins = C // cnt
    if coins * cnt != C or coins != scn.coins or C < 2:
        raise ValueError("coin_plane: %d documents for %d instances x %d coin slots (two at "
                         "least)" % (C, cnt, scn.coins))
    f = (n - 1) // 3
    sks = keys["secret_key_shares"]
    if len(sks) != n:
        raise ValueError("coin_plane: %d key shares for %d nodes" % (len(sks), n))
    dev = "cuda:%d" % device if isinstance(device, int) else str(device)
    pk_tab = keys["key_shares"][0]
    stab, total, s192, _, sst = T.create_signature_shares(sks, hashes192, device=torch.device(dev).index)
    if sst.cpu().numpy().any():
        raise ValueError("coin_plane: a document or key share did not decode")
    nodes = [i for i in range(n) for _ in range(C)]
    docs = [c for _ in range(n) for c in range(C)]
    # the document whose share stands in for the tampered share of document c
    other = [(c // coins) * coins + (c % coins + 1) % coins if coins > 1 else (c + 1) % C
             for c in range(C)]
    hprep = T.g2_prepare(T._g2_rows(hashes192, dev))
    ok0 = T.sig_check_prepared(stab, total, pk_tab, n, u32(nodes, dev), hprep, C, u32(docs, dev))
    swapped = s192[u32([T.share_row(i, other[c], C) for i, c in zip(nodes, docs)], dev).long()]
    ok1 = T.sig_check_prepared(T.g2_points_prepare(swapped.contiguous()), total, pk_tab, n,
                               u32(nodes, dev), hprep, C, u32(docs, dev))
    # [node][doc] -> [inst][slot][node]
    share_ok = torch.stack([(o == T.CHECK_OK).to(torch.uint8).view(n, cnt, coins).permute(1, 2, 0)
                            for o in (ok0, ok1)], dim=2).contiguous()
    par, ver = coin_parity(dict(sig_tab=stab, sig_count=total, docs=C, hprep=hprep, keys=keys),
                           list(range(f + 1)), dev)
    info = dict(sig_tab=stab, sig_count=total, docs=C, hprep=hprep, keys=keys,
                verified=ver.view(cnt, coins))
    return share_ok, par.view(cnt, coins).contiguous(), info


def coin_parity(info, nodes, dev):
    """Combine the shares of `nodes` (f + 1 distinct node indices) for every
    document of a coin_plane: (parity uint8 [docs], verified uint8 [docs]: the
    signature passes the master public key)."""
    from . import threshold as T
    u32 = T._u32_tensor
    C, k = info["docs"], len(nodes)
    rows = [T.share_row(i, c, C) for c in range(C) for i in nodes]
    offs = u32(np.arange(C + 1) * k, dev)
    g192, _, par, st = T.sig_combine_prepared(info["sig_tab"], info["sig_count"], u32(rows, dev),
                                              u32(list(nodes) * C, dev), offs)
    if st.cpu().numpy().any():
        raise ValueError("coin_plane: a combine failed")
    master = T.g1_prepare(T._g1_rows([info["keys"]["key_set"][0][0]], dev))
    ver = T.sig_check_prepared(T.g2_points_prepare(g192), C, master, 1,
                               u32([0] * C, dev), info["hprep"], C, u32(list(range(C)), dev))
    return par.to(torch.uint8), (ver == T.CHECK_OK).to(torch.uint8)
