"""HoneyBadger epochs on the GPU: Subset, then N threshold decryptions a node.

Control plane.  One epoch of `HoneyBadger` for every node of `count`
independent networks, in the synchronous rounds of `subset_sim`.  A round is
three launches: phase 1 `hbrbc_sm_round` and phase 2 `hbrbc_subset_round`
exactly as `subset_sim.SubsetRank` issues them, then phase 3 `hbrbc_hb_round`
(hbbft_amd/csrc/hb_sim.hip), one thread per (instance, node, proposer): the
new entries of phase 2's output sequence -- a contribution is Complete in a
plain instance and sets the ciphertext, purges the waiting shares, sends the
node's own share and tries to output in an encrypted one; Done removes the
decryption states of the proposers that were not accepted -- then the round's
DecryptionShare records, then the batch once every accepted proposer is
Complete (include/hbrbc.h states the batch point).  What a node emits in round
t is delivered in round t + 1; a run ends with the first round in which none
of the three protocols emits a record.  The host restatement
hbbft_amd/honey_badger.py, driven by tests/hb_net.py in the same schedule, is
the checker (tests/test_hb_sim.py).

Data plane.  `subset_sim`'s for the broadcasts and the coins; the decryption
tables -- ct_state, share_ok of both variants of every node's share, the
plaintext -- are forced (Instance) or `decrypt_plane` over real keys.
The plane takes a stand-in H per ciphertext and the plaintext and the
deserialisation outcomes by reference: `hash_g1_g2` and `xor_with_hash` are in
threshold.py (parity with the threshold_crypto crate unpinned), feeding the
plane real hashes is a follow-up, and the bincode of a `Ciphertext` stays
with the caller.

One epoch only: several live `EpochState`s per node (`max_future_epochs`) are
the host class's; the device runs them one after the other.
"""
import numpy as np
import torch

from . import rbc_sim, rounds as shared, subset_sim
from .honey_badger import ALL_AT_END, CT_INVALID, CT_VALID, INCREMENTAL, DecryptTable
from .rounds import I32, U32, USIZE
from .subset_sim import ROUND_BATCH

HONEST, SILENT, BAD_SHARE, TWICE, STRAY, ABSENT = range(6)   # enum hbrbc_hb_role
ENCRYPTED_FLAG, ALL_AT_END_FLAG = 1, 2                       # inst_flags
NO_BATCH = -1
DS_ABSENT, DS_NO_CIPHERTEXT, DS_ONGOING, DS_COMPLETE, DS_REMOVED = range(5)
DS_ACCEPTED = 8
# enum hbrbc_hb_fault, by the names of honey_badger.HbFault
FAULT_KINDS = ("UnexpectedDecryptionShare", "DeserializeCiphertext", "InvalidCiphertext",
               "BatchDeserializationFailed", "DecryptionFault(MultipleDecryptionShares)",
               "DecryptionFault(UnverifiedDecryptionShareSender)")
BAD_INDEX, BAD_SEQ = 1, 2

# hbrbc_hb_args.emitted[1] of a round, in the order the read-back looks at them
ROUND_FLAGS = (
    (BAD_INDEX, "honey badger: a root slot, ct_state or role out of range"),
    (shared.ANY, "honey badger: an output sequence out of range (flags {1:#x})"))

HbArgs = shared.args_struct(
    "HbArgs", "hbrbc_hb_args",
    [("count", USIZE), ("n", U32), ("roots", U32), ("max_faults", U32), ("round", I32)],
    ("inst_flags", "role", "ct_state", "undeserialisable", "share_ok", "output_root", "out_seq",
     "out_len", "in_", "out", "node_state", "done_round", "batch_round", "dstate", "mask",
     "faults", "fault_count", "emitted", "active"))
HB_ROUND = shared.Entry("hbrbc_hb_round", HbArgs)


# ------------------------------------------------------------------ scenario --
class Instance:
    """One HoneyBadger epoch of n nodes over `subset` (a subset_sim.Instance,
    whose dead nodes are absent here too).  `encrypted`: the caller's
    EncryptionSchedule.use_on_epoch(epoch); strategy: INCREMENTAL or
    ALL_AT_END; hb_role[j]: what node j's decryption layer sends.  Per
    proposer p and root slot r of its broadcast (a value of
    subset.broadcasts[p].values): ct_state[p][r] -- 0 valid, 1 does not
    deserialise, 2 fails verify --, undeserialisable[p][r] -- the contribution
    does not deserialise -- and plaintexts[p][r], the bytes the ciphertext
    decrypts to (None or absent: the value itself).  The share tables are
    forced (honest shares valid, tampered ones not) unless Scenario.set_tables
    gives decrypt_plane's."""

    def __init__(self, subset, epoch=0, encrypted=True, strategy=INCREMENTAL, hb_role=None,
                 ct_state=None, undeserialisable=None, plaintexts=None, max_faulty=None):
        n = subset.n
        self.n, self.subset, self.epoch = n, subset, int(epoch)
        self.encrypted, self.strategy = bool(encrypted), strategy
        assert strategy in (INCREMENTAL, ALL_AT_END)
        self.hb_role = list(hb_role) if hb_role is not None else [HONEST] * n
        slots = [len(b.values) for b in subset.broadcasts]
        self.ct_state = [list(ct_state[p]) if ct_state is not None else [CT_VALID] * slots[p]
                         for p in range(n)]
        self.undeserialisable = [[int(bool(v)) for v in undeserialisable[p]]
                                 if undeserialisable is not None else [0] * slots[p]
                                 for p in range(n)]
        self.plaintexts = [[(plaintexts[p][r] if plaintexts is not None and
                             plaintexts[p][r] is not None else subset.broadcasts[p].values[r])
                            for r in range(slots[p])] for p in range(n)]
        assert len(self.hb_role) == n and all(HONEST <= r <= STRAY for r in self.hb_role)
        for p in range(n):
            assert len(self.ct_state[p]) == len(self.undeserialisable[p]) == slots[p]
            assert all(0 <= c <= CT_INVALID for c in self.ct_state[p])
        faulty = set(subset.faulty) | {j for j in range(n) if self.hb_role[j] != HONEST}
        faulty |= {p for p in range(n) if any(self.ct_state[p]) or any(self.undeserialisable[p])}
        assert len(faulty) <= ((n - 1) // 3 if max_faulty is None else max_faulty), \
            "more than f dead or faulty nodes"
        self.faulty = frozenset(faulty)

    def host_tables(self, share_ok=None):
        """tables[p][r]: the honey_badger.DecryptTable of (proposer, root
        slot); share_ok[p][r][variant][sender], forced when None."""
        n = self.n
        return [[DecryptTable(v, self.ct_state[p][r],
                              [[1] * n, [0] * n] if share_ok is None else share_ok[p][r],
                              self.plaintexts[p][r] if self.encrypted else v,
                              not self.undeserialisable[p][r])
                 for r, v in enumerate(self.subset.broadcasts[p].values)] for p in range(n)]


class Scenario:
    """`count` epochs of one validator count n; one scenario may mix plain and
    encrypted instances and both strategies."""

    def __init__(self, n, instances, coins=None, queue_epochs=4):
        self.n = n
        self.instances = list(instances)
        assert self.instances and all(i.n == n for i in self.instances)
        self.subset = subset_sim.Scenario(n, [i.subset for i in self.instances], coins,
                                          queue_epochs)
        self.roots = self.subset.rbc_scenario().roots
        self._share_ok = None

    @property
    def count(self):
        return len(self.instances)

    def set_tables(self, ct_state, share_ok):
        """decrypt_plane's: ct_state [count n][roots] replaces the instances'
        for the valid / invalid outcome (a ct_state of 1 stays: the caller's),
        share_ok [count n][roots][2][n]."""
        cs = ct_state.cpu().numpy().reshape(self.count, self.n, self.roots)
        for i, inst in enumerate(self.instances):
            for p in range(self.n):
                for r in range(len(inst.ct_state[p])):
                    if inst.ct_state[p][r] != 1:
                        inst.ct_state[p][r] = int(cs[i, p, r])
        self._share_ok = share_ok.to(torch.uint8).contiguous()
        assert tuple(self._share_ok.shape) == (self.count * self.n, self.roots, 2, self.n)

    def host_tables(self, inst):
        """The DecryptTables the host restatement of instance `inst` reads."""
        so = None
        if self._share_ok is not None:
            so = self._share_ok.cpu().numpy().reshape(self.count, self.n, self.roots, 2, self.n)[
                inst].tolist()
        return self.instances[inst].host_tables(so)

    def tensors(self, device):
        n, cnt, R = self.n, self.count, self.roots
        flags = np.zeros(cnt, np.uint8)
        role = np.zeros((cnt, n), np.uint8)
        cs = np.zeros((cnt, n, R), np.uint8)
        und = np.zeros((cnt, n, R), np.uint8)
        for i, inst in enumerate(self.instances):
            flags[i] = (ENCRYPTED_FLAG if inst.encrypted else 0) | \
                (ALL_AT_END_FLAG if inst.strategy == ALL_AT_END else 0)
            role[i] = inst.hb_role
            for j in inst.subset.dead:
                role[i, j] = ABSENT
            for p in range(n):
                k = len(inst.ct_state[p])
                cs[i, p, :k] = inst.ct_state[p]
                und[i, p, :k] = inst.undeserialisable[p]
        if self._share_ok is None:
            so = np.zeros((cnt * n, R, 2, n), np.uint8)
            so[:, :, 0, :] = 1
            share_ok = torch.from_numpy(so).to(device)
        else:
            share_ok = self._share_ok.to(device)
        t = lambda a: torch.from_numpy(a).to(device)   # noqa: E731
        return dict(inst_flags=t(flags), role=t(role), ct_state=t(cs.reshape(cnt * n, R)),
                    undeserialisable=t(und.reshape(cnt * n, R)), share_ok=share_ok)


# ------------------------------------------------------------- one rank -----
class HbRank:
    """Every node of `count` epochs on one GPU: a subset_sim.SubsetRank and
    phase 3's state."""

    def __init__(self, scn, device=0, ok=None, dec=None, hb_max_faults=None, max_rounds=256, **kw):
        self.sub = subset_sim.SubsetRank(scn.subset, device, ok, dec, max_rounds=max_rounds, **kw)
        n, cnt = scn.n, scn.count
        self.n, self.count, self.roots = n, cnt, scn.roots
        self.W = (n + 31) // 32
        self.max_rounds = max_rounds
        self.max_faults = max(16, 4 * n) if hb_max_faults is None else hb_max_faults
        dev = self.device = self.sub.device
        self.sc = scn.tensors(dev)
        HB_ROUND.bind()
        B = cnt * n
        i32 = dict(dtype=torch.int32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        self.out = torch.zeros((B, n), **u8)
        self.inbox = torch.zeros((B, n), **u8)
        self.node_state = torch.zeros((cnt, n), **i32)
        self.done_round = torch.zeros((cnt, n), **i32)
        self.batch_round = torch.full((cnt, n), NO_BATCH, **i32)
        self.dstate = torch.zeros((B, n), **u8)
        self.mask = torch.zeros((B, 2 * self.W, n), **i32)
        self.faults = torch.zeros((B, n, max(1, self.max_faults)), dtype=torch.int16, device=dev)
        self.fault_count = torch.zeros((B, n), **i32)
        # per round: share records emitted, flags (hbrbc_hb_args.emitted)
        self.hist = torch.zeros((max_rounds, 2), **i32)
        # act[r]: the records of all three protocols in round r - 1
        self.act = torch.zeros(max_rounds + 1, **i32)
        self.hb_records = 0

    def reset(self):
        self.sub.reset()
        for t in (self.out, self.inbox, self.node_state, self.done_round, self.dstate, self.mask,
                  self.fault_count, self.hist, self.act):
            t.zero_()
        self.batch_round.fill_(NO_BATCH)
        self.hb_records = 0

    def phase3(self, r, active=None, stream=None):
        """hbrbc_hb_round of round r (after phases 1 and 2 of the same round)."""
        if r >= self.max_rounds:
            raise RuntimeError("honey badger: round %d past max_rounds %d" % (r, self.max_rounds))
        a = HbArgs(count=self.count, n=self.n, roots=self.roots, max_faults=self.max_faults,
                   round=r)
        a.output_root = self.sub.bc.output_root.data_ptr()
        a.out_seq, a.out_len = self.sub.out_seq.data_ptr(), self.sub.out_len.data_ptr()
        a.in_, a.out = self.inbox.data_ptr(), self.out.data_ptr()
        a.node_state, a.done_round = self.node_state.data_ptr(), self.done_round.data_ptr()
        a.batch_round, a.dstate = self.batch_round.data_ptr(), self.dstate.data_ptr()
        a.mask, a.faults = self.mask.data_ptr(), self.faults.data_ptr()
        a.fault_count = self.fault_count.data_ptr()
        shared.fill(a, self.sc, self.hist, r, active)
        HB_ROUND.launch(a, self.device, stream)

    def round(self, r, phase=shared.call):
        """The three phases of round r, then the swap of the share records.
        Phases 1 and 2 are subset_sim.SubsetRank.round as it is (phase 3 reads
        out_seq, out_len and output_root, which the Subset's own swap leaves
        alone); once the Subset is quiescent it stays so -- nothing of phase 3
        feeds back into it -- while share records may go on for a round or
        two, so phase 3's `active` counts the records of all three protocols.
        phase: the loop's hook around every launch (rounds.Rounds)."""
        sub = self.sub
        sub.round(r, phase)
        self.out.zero_()
        phase("phase3", self.phase3, r, None if r == 0 else self.act[r])
        torch.add(sub.act[r + 1], self.hist[r, 0], out=self.act[r + 1])
        self.inbox, self.out = self.out, self.inbox


def run_rounds(rank, events=None):
    """Drive the three state machines until none emits a record, ROUND_BATCH
    rounds per read-back (rounds.Rounds).  Returns the number of rounds.
    Every run starts from fresh nodes.  events: a list that receives (phase
    name, start, end) device events of every launch: "phase1", "phase2" and
    "phase3" per round."""
    sub = rank.sub
    return shared.Rounds(subset_sim.protocols(sub) +
                         [shared.Protocol(ROUND_FLAGS, rank, rank, "hb_records")],
                         rank.max_rounds, ROUND_BATCH, "honey badger", events=events,
                         reset=rank.reset, enqueue=rank.round,
                         read=shared.hist_rows([sub.bc, sub, rank])).launch().wait()


class HbRun(subset_sim.SubsetRun):
    """The results of one run: everything SubsetRun has, and per (inst, node)
    batch -- {proposer: contribution bytes}, or None -- and batch_round; per
    (inst, node, proposer) hb_faults [(blamed, kind name)], dstate (DS_*) and
    accepted_hb; rounds; hb_emitted: the share records of every round."""

    def __init__(self, rank, rounds, payloads, scn):
        super().__init__(rank.sub, rounds, payloads)
        n, cnt = rank.n, rank.count
        br = rank.batch_round.cpu().numpy()
        ds = rank.dstate.cpu().numpy().reshape(cnt, n, n)
        root = rank.sub.bc.output_root.cpu().numpy().reshape(cnt, n, n)
        logs = shared.fault_logs(rank.fault_count, rank.faults, rank.max_faults, FAULT_KINDS,
                                 "honey badger ")
        self.batch, self.batch_round, self.hb_faults, self.dstate = {}, {}, {}, {}
        for i, inst in enumerate(scn.instances):
            for j in range(n):
                b = int(br[i, j])
                self.batch_round[(i, j)] = None if b == NO_BATCH else b
                self.batch[(i, j)] = None
                if b != NO_BATCH:
                    batch = {}
                    for p in range(n):
                        r = int(root[i, p, j])
                        if int(ds[i, p, j]) & DS_ACCEPTED and not inst.undeserialisable[p][r]:
                            batch[p] = bytes(inst.plaintexts[p][r]) if inst.encrypted else \
                                bytes(inst.subset.broadcasts[p].values[r])
                    self.batch[(i, j)] = batch
                for p in range(n):
                    self.hb_faults[(i, j, p)] = logs[(i * n + p, j)]
                    self.dstate[(i, j, p)] = int(ds[i, p, j]) & 7
        self.hb_emitted = [int(v) for v in rank.hist[:rounds, 0].cpu().numpy()]
        self.hb_records = rank.hb_records


def run(scn, device=0, **kw):
    """Every node of every instance of `scn` on one GPU: an HbRun.  Raises as
    subset_sim.run does, and on a fault-log overflow."""
    ok, dec, payloads, _ = rbc_sim.data_plane(scn.subset.rbc_scenario(), device)
    rank = HbRank(scn, device, ok, dec, **kw)
    return HbRun(rank, run_rounds(rank), payloads, scn)


def simulate(scn, device=0, **kw):
    """(batch, batch_round, hb_faults, outputs, accepted, bc_faults, ba_faults,
    rounds, bc_emitted, ba_emitted, hb_emitted) of `run`."""
    r = run(scn, device, **kw)
    return (r.batch, r.batch_round, r.hb_faults, r.outputs, r.accepted, r.bc_faults, r.ba_faults,
            r.rounds, r.bc_emitted, r.ba_emitted, r.hb_emitted)


# ------------------------------------------------------------- data plane ---
def decrypt_plane(scn, ciphertexts, keys, device=0, timings=None):
    """The data plane of the decryptions, on the existing entries
    (hbbft_amd/threshold.py): ciphertexts[inst * n + p] = (U compressed G1, 48
    bytes; W compressed G2, 96 bytes; H = the caller's hash_g1_g2(U, V) as an
    uncompressed G2 point) of proposer p's contribution (root slot 0; the
    scenario has one root slot per broadcast); keys is the dict
    keygen.sync_key_gen_network returns.  verify_ciphertexts gives ct_state 0
    or 2; create_decryption_shares makes the shares of all N nodes; node j's
    tampered share of a ciphertext is its share of the instance's NEXT
    ciphertext (a valid subgroup point that fails the check);
    pairing_check_prepared_keys runs over both variants; decrypt_combine_
    prepared over nodes 0..f gives g.  Returns (ct_state [count n][1], share_ok
    [count n][1][2][n] -- uint8 on the device --, g48 [count n][48], info) with
    info: share_tab / share_count / items for further combines.  timings: a
    dict that receives the milliseconds of the four steps."""
    from . import threshold as T
    u32 = T._u32_tensor
    n, cnt = scn.n, scn.count
    C = len(ciphertexts)
    if C != cnt * n or scn.roots != 1 or n < 2:
        raise ValueError("decrypt_plane: %d ciphertexts for %d instances x %d proposers with one "
                         "root slot each (two proposers at least)" % (C, cnt, n))
    f = (n - 1) // 3
    sks = keys["secret_key_shares"]
    if len(sks) != n:
        raise ValueError("decrypt_plane: %d key shares for %d nodes" % (len(sks), n))
    dev = "cuda:%d" % device if isinstance(device, int) else str(device)
    index = torch.device(dev).index
    pk_tab = keys["key_shares"][0]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record()
    u96, ust = T.g1_decompress(T._g1_rows([u for u, _, _ in ciphertexts], dev,
                                          T.G1_COMPRESSED_BYTES))
    w192, wst = T.g2_decompress(T._g2_rows([w for _, w, _ in ciphertexts], dev,
                                           T.G2_COMPRESSED_BYTES))
    uh, wh = u96.cpu().numpy(), w192.cpu().numpy()
    valid = T.verify_ciphertexts([(bytes(uh[c]), bytes(wh[c]), ciphertexts[c][2])
                                  for c in range(C)], index)
    bad_point = (ust.cpu().numpy() != 0) | (wst.cpu().numpy() != 0)
    ct_state = torch.from_numpy(np.where(np.asarray(valid) & ~bad_point, 0, 2).astype(np.uint8))
    ev[1].record()
    stab, total, s96, _, sst = T.create_decryption_shares(sks, [u for u, _, _ in ciphertexts],
                                                          index)
    if sst.cpu().numpy().any():
        raise ValueError("decrypt_plane: a U or key share did not decode")
    ev[2].record()
    nodes = [i for i in range(n) for _ in range(C)]
    items = [c for _ in range(n) for c in range(C)]
    other = [(c // n) * n + (c % n + 1) % n for c in range(C)]
    hw = torch.stack([T._g2_rows([h for _, _, h in ciphertexts], dev), w192], dim=1)
    prep = T.g2_prepare(hw.reshape(2 * C, T.G2_BYTES).contiguous())
    idx_b, idx_d = u32([2 * c for c in items], dev), u32([2 * c + 1 for c in items], dev)
    ok0 = T.pairing_check_prepared_keys(s96.contiguous(), pk_tab, n, u32(nodes, dev), prep, 2 * C,
                                        idx_b, idx_d)
    swapped = s96[u32([T.share_row(i, other[c], C) for i, c in zip(nodes, items)], dev).long()]
    ok1 = T.pairing_check_prepared_keys(swapped.contiguous(), pk_tab, n, u32(nodes, dev), prep,
                                        2 * C, idx_b, idx_d)
    # [node][item] -> [item][slot 0][variant][node]
    share_ok = torch.stack([(o == T.CHECK_OK).to(torch.uint8).view(n, C).t() for o in (ok0, ok1)],
                           dim=1).view(C, 1, 2, n).contiguous()
    ev[3].record()
    info = dict(share_tab=stab, share_count=total, items=C)
    g48 = decrypt_combine(info, list(range(f + 1)), dev)
    ev[4].record()
    if timings is not None:
        torch.cuda.synchronize()
        for k, name in enumerate(("verify_ciphertexts", "create_shares", "check_shares",
                                  "combine")):
            timings[name] = ev[k].elapsed_time(ev[k + 1])
    return ct_state.view(C, 1).to(dev), share_ok, g48, info


def decrypt_combine(info, nodes, dev):
    """Combine the shares of `nodes` (f + 1 distinct node indices) for every
    ciphertext of a decrypt_plane: g compressed, uint8 [items][48]."""
    from . import threshold as T
    u32 = T._u32_tensor
    C, k = info["items"], len(nodes)
    rows = [T.share_row(i, c, C) for c in range(C) for i in nodes]
    offs = u32(np.arange(C + 1) * k, dev)
    _, g48, st = T.decrypt_combine_prepared(info["share_tab"], info["share_count"],
                                            u32(rows, dev), u32(list(nodes) * C, dev), offs)
    if st.cpu().numpy().any():
        raise ValueError("decrypt_plane: a combine failed")
    return g48
