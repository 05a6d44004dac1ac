"""The host driver the four round simulations share (hbbft_amd/rounds.py), on
CPU tensors with fake protocols in the style of test_rbc_sim._FakeLocalSm: a
round ADDS its records into hist[r] and returns at once when `active` is 0.
The loop's batching, its one read per batch, flags before counts, the tallies,
the return at the first silent round, the max_rounds error, repeated runs and
the timing hook; then the fault-log decoder and the agreement buffers."""
import numpy as np
import pytest
import torch

from hbbft_amd import rounds

TABLE = ((2, "fake: the second flag, limit {0.limit}"), (rounds.ANY, "fake: flags {1:#x}"))
BATCH = 4


class _Fake:
    """One protocol: round r emits emits[r] records (0 past the list).  The
    flags of `flags` ({round: bits}) are set whether or not the round runs,
    so a test can put one after the silent round."""
    limit = 7

    def __init__(self, emits, flags=None, max_rounds=32):
        self.emits, self.flags = list(emits), dict(flags or {})
        self.hist = torch.zeros((max_rounds, 2), dtype=torch.int32)
        self.reset()

    def reset(self):
        self.hist.zero_()
        self.records, self.ran = 0, []

    def round(self, r, active=None):
        self.hist[r, 1] |= self.flags.get(r, 0)
        if active is not None and int(active) == 0:
            return
        self.ran.append((r, None if active is None else int(active)))
        self.hist[r, 0] += self.emits[r] if r < len(self.emits) else 0   # accumulated


class _Net:
    """Fake protocols side by side, as the phases of one round: each gets the
    records of all of them in round r - 1 as `active` (act[r])."""

    def __init__(self, protos, max_rounds=32, **kw):
        self.protos, self.reads, self.enqueued = protos, 0, []
        self.act = torch.zeros(max_rounds + 1, dtype=torch.int32)
        read = rounds.hist_rows(protos)

        def counted(r, hi):
            self.reads += 1
            return read(r, hi)
        self.loop = rounds.Rounds([rounds.Protocol(TABLE, p, p, "records") for p in protos],
                                  max_rounds, BATCH, "fake", reset=self.reset,
                                  enqueue=self.round, read=counted, **kw)

    def reset(self):
        for p in self.protos:
            p.reset()
        self.act.zero_()
        self.reads, self.enqueued = 0, []

    def round(self, r, phase):
        self.enqueued.append(r)
        for k, p in enumerate(self.protos):
            phase("phase%d" % (k + 1), p.round, r, None if r == 0 else self.act[r])
        self.act[r + 1] = sum(int(p.hist[r, 0]) for p in self.protos)

    def run(self):
        return self.loop.launch().wait()


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("last", [BATCH - 2, BATCH - 1])
def test_quiescence_at_a_batch_edge(k, last):
    """k protocols side by side, the longest emitting through round `last`:
    the silent round is the last of the first batch (one read, nothing more
    enqueued) or the first of the second (two reads; the rest of that batch
    was enqueued and returned at once).  A second run of the same objects
    gives the same rounds and totals."""
    protos = [_Fake([3 + j] * (last + 1 - j)) for j in range(k)]
    net = _Net(protos)
    for _ in range(2):
        assert net.run() == last + 2
        in_first = last + 1 < BATCH
        assert net.reads == (1 if in_first else 2)
        assert net.enqueued == list(range(BATCH if in_first else 2 * BATCH))
        for j, p in enumerate(protos):
            assert p.records == (3 + j) * (last + 1 - j)
            assert [r for r, _ in p.ran] == list(range(last + 2))   # the silent round ran
            assert int(p.hist[:, 0].sum()) == p.records             # not added to the first run's


def test_one_protocol_still_emits():
    """The Subset after its broadcasts went quiet: the first protocol emits
    nothing from round 2 on, the second through round 5.  The run goes on,
    and the silent protocol's rounds run with `active` = the sum."""
    bc, ba = _Fake([4, 4]), _Fake([1, 2, 3, 5, 6, 7])
    assert _Net([bc, ba]).run() == 7
    assert (bc.records, ba.records) == (8, 24)
    assert bc.ran == [(0, None), (1, 5), (2, 6), (3, 3), (4, 5), (5, 6), (6, 7)]
    assert ba.ran == bc.ran


def test_flag_after_the_silent_round_is_not_looked_at():
    p, q = _Fake([2]), _Fake([1], flags={2: 1})
    assert _Net([p, q]).run() == 2   # round 1 is silent; round 2 is in the same batch
    assert int(q.hist[2, 1]) == 1 and (p.records, q.records) == (2, 1)


@pytest.mark.parametrize("count", [0, 5])
def test_flag_wins_over_the_count_of_its_round(count):
    """Round 1 has a flag of the second protocol and `count` records: the
    flag's error is raised -- not the return of a silent round --, and before
    any tally of that round."""
    p, q = _Fake([2, count]), _Fake([1, 0], flags={1: 4})
    with pytest.raises(RuntimeError, match="^fake: flags 0x4$"):
        _Net([p, q]).run()
    assert (p.records, q.records) == (2, 1)
    with pytest.raises(RuntimeError, match="^fake: the second flag, limit 7$"):
        _Net([_Fake([2, count], flags={1: 3})]).run()   # the table's order, not the bits'


def test_max_rounds_between_batches():
    p = _Fake([1] * 40)
    net = _Net([p], max_rounds=BATCH + 2)
    with pytest.raises(RuntimeError, match="^fake did not quiesce in 6 rounds$"):
        net.run()
    assert net.enqueued == list(range(BATCH + 2)) and net.reads == 2 and p.records == 6


class _Event:
    clock = 0

    def record(self):
        _Event.clock += 1
        self.at = _Event.clock


def test_timing_hook_gets_every_phase_launch_in_order():
    events = []
    net = _Net([_Fake([2, 2]), _Fake([1]), _Fake([])], events=events, new_event=_Event)
    assert net.run() == 3
    # one triple per launch of the enqueued batch, the empty ones included
    assert [name for name, _, _ in events] == ["phase1", "phase2", "phase3"] * BATCH
    at = [t for _, e0, e1 in events for t in (e0.at, e1.at)]
    assert at == sorted(at) and len(set(at)) == len(at)
    _Event.clock = 0
    assert _Net([_Fake([2, 2])]).run() == 3 and _Event.clock == 0   # no list: no hook


def test_fault_logs_window_and_overflow_texts():
    kinds = ["A", "B", "C"]
    counts = torch.tensor([[1, 2, 0], [0, 3, 9]], dtype=torch.int32)
    logs = torch.zeros((2, 3, 3), dtype=torch.int16)
    logs[0, 0, 0] = (5 << 8) | 1
    logs[0, 1, :2] = torch.tensor([(200 << 8) | 2 - 65536, 2 << 8], dtype=torch.int16)
    logs[1, 1, :] = 1 << 8
    # a sharded rank's window: rows are nodes 4, 5 and a padding row past n = 6
    got = rounds.fault_logs(counts, logs, 3, kinds, node_lo=4, n=6)
    assert got == {(0, 4): [(5, "B")], (0, 5): [(200, "C"), (2, "A")], (1, 4): [],
                   (1, 5): [(1, "A")] * 3}
    with pytest.raises(RuntimeError, match=r"^fault log overflow at \(1, 2\): 9 records$"):
        rounds.fault_logs(counts, logs, 3, kinds)
    for what in ("agreement ", "honey badger "):
        with pytest.raises(RuntimeError, match="^%sfault log overflow at" % what):
            rounds.fault_logs(counts, logs, 2, kinds, what)


def test_agreement_state_swap_reset_and_pointers():
    from hbbft_amd.ba_sim import BaArgs
    from hbbft_amd.subset_sim import SubsetArgs
    ag = rounds.AgreementState(3, 5, 16, 2, 0, torch.device("cpu"))
    assert ag.out.shape == (3, 5, 2, 2) and ag.faults.shape == (3, 5, 1)
    out, inbox = ag.out, ag.inbox
    ag.out_count.fill_(2)
    ag.decision.zero_()
    ag.swap()
    assert ag.inbox is out and ag.out is inbox and int(ag.inbox_count.sum()) == 30
    for args in (BaArgs(), SubsetArgs()):
        ag.write(args)
        for field, name in [("in_", "inbox"), ("in_count", "inbox_count")] + [
                (f, f) for f in rounds.AgreementState.NAMES if not f.startswith("inbox")]:
            assert getattr(args, field) == getattr(ag, name).data_ptr(), field
    ag.reset()
    assert int(ag.inbox_count.sum()) == 0 and bool((ag.decision == rounds.NONE).all())
    assert np.asarray(ag.state).sum() == 0
