"""What the round simulations share on the host (rbc_sim, ba_sim, subset_sim,
hb_sim): the round loop, the agreement-side buffers, the fault-log decoder,
the flag-to-error translation and the ctypes plumbing of a round entry point.

The loop (`Rounds`).  A run is rounds 0, 1, ... until the first round in which
no protocol emits a record.  Rounds are enqueued in batches: round r gets the
device count of round r - 1 as its kernels' `active` operand and those return
at once when it is 0, so the rounds past quiescence cost empty launches and
the host reads the per-round [records, flags] rows back once per batch, not
once per round.  Per round of a batch the flags are looked at first (a set
flag raises, by the protocol's table), then the records are tallied, and the
first round without records ends the run; the rounds after it are not looked
at.  What differs between the simulations is handed in: what resets the nodes,
what enqueues one round, how the rows reach the host, and the flag tables.
"""
import collections
import contextlib
import ctypes

import numpy as np
import torch

from . import _check, lib

NONE = 0xFF
P = ctypes.c_void_p
USIZE, U32, I32 = ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int32


# ------------------------------------------------------- round entry points --
def args_struct(name, c_name, scalars, pointers, tail=()):
    """The ctypes Structure `name` of struct `c_name` (include/hbrbc.h): the
    (field, type) scalars, then the pointer fields, then the scalars of `tail`."""
    return type(name, (ctypes.Structure,), {
        "__doc__": "struct %s (include/hbrbc.h)." % c_name,
        "_fields_": list(scalars) + [(p, P) for p in pointers] + list(tail)})


class Entry:
    """A round entry point `int name(args *, stream)` of the library --
    `handle`: `int name(context, args *, stream)` -- and the `size_t
    f(size_t, size_t)` functions in `sizes`, bound once per library object."""

    def __init__(self, name, args, handle=False, sizes=()):
        self.name, self.args, self.handle, self.sizes = name, args, handle, sizes
        self.lib = self.fn = None

    def bind(self):
        L = lib()
        if L is not self.lib:
            for f in self.sizes:
                getattr(L, f).restype = ctypes.c_size_t
                getattr(L, f).argtypes = [ctypes.c_size_t, ctypes.c_size_t]
            fn = getattr(L, self.name)
            fn.restype = ctypes.c_int
            fn.argtypes = ([P] if self.handle else []) + [ctypes.POINTER(self.args), P]
            self.lib, self.fn = L, fn
        return L

    def launch(self, a, device, stream=None, handle=None):
        """Enqueue the entry with args `a` on `stream` (default: the current
        stream of `device`); a status other than 0 raises."""
        st = stream if stream is not None else torch.cuda.current_stream(device)
        if lib() is not self.lib:
            self.bind()
        if self.handle:   # the context carries the device
            _check(self.fn(handle, ctypes.byref(a), P(st.cuda_stream)))
        else:
            with torch.cuda.device(device):
                _check(self.fn(ctypes.byref(a), P(st.cuda_stream)))


def fill(a, tensors, hist, r, active):
    """The operands of round r that are not node state: a.<name> = the address
    of tensors[name] for every name (the scenario's tables), `emitted` row r
    of hist (int32 [max_rounds][2]; its address without a tensor op, this runs
    every round), `active` a device int32 scalar tensor or None."""
    for name, t in tensors.items():
        setattr(a, name, t.data_ptr())
    a.emitted = hist.data_ptr() + 8 * r
    a.active = None if active is None else active.data_ptr()


# -------------------------------------------------------- agreement buffers --
class AgreementState:
    """The BinaryAgreement tensors of B instances of n nodes: per-node state
    blocks, this round's records and the previous round's (`out` / `inbox`
    with their counts), decisions and fault logs.  ba_sim.BaRank holds one
    with B = count, subset_sim.SubsetRank one with B = count n."""
    NAMES = ("state", "out", "out_count", "inbox", "inbox_count", "decision", "decision_epoch",
             "faults", "fault_count")

    def __init__(self, B, n, state_bytes, max_out, max_faults, dev):
        i32 = dict(dtype=torch.int32, device=dev)
        rec = 1 + (n + 31) // 32
        self.state = torch.zeros((B, n, state_bytes), dtype=torch.uint8, device=dev)
        self.out = torch.zeros((B, n, max_out, rec), **i32)
        self.out_count = torch.zeros((B, n), **i32)
        self.inbox = torch.zeros((B, n, max_out, rec), **i32)
        self.inbox_count = torch.zeros((B, n), **i32)
        self.decision = torch.full((B, n), NONE, dtype=torch.uint8, device=dev)
        self.decision_epoch = torch.zeros((B, n), dtype=torch.int16, device=dev)
        self.faults = torch.zeros((B, n, max(1, max_faults)), dtype=torch.int16, device=dev)
        self.fault_count = torch.zeros((B, n), **i32)

    def reset(self):
        """Fresh nodes (before round 0 of another run)."""
        for t in (self.state, self.out_count, self.inbox_count, self.decision_epoch,
                  self.fault_count):
            t.zero_()
        self.decision.fill_(NONE)

    def swap(self):
        """This round's records become the next round's inbox."""
        self.inbox, self.out = self.out, self.inbox
        self.inbox_count, self.out_count = self.out_count, self.inbox_count

    def write(self, a):
        """The pointers into an args struct with the agreement field names
        (hbrbc_ba_args, hbrbc_subset_args)."""
        a.in_, a.in_count = self.inbox.data_ptr(), self.inbox_count.data_ptr()
        a.out, a.out_count = self.out.data_ptr(), self.out_count.data_ptr()
        a.state = self.state.data_ptr()
        a.decision, a.decision_epoch = self.decision.data_ptr(), self.decision_epoch.data_ptr()
        a.faults, a.fault_count = self.faults.data_ptr(), self.fault_count.data_ptr()


class HasAgreement:
    """A rank whose `ag` is an AgreementState: the tensors stay readable on
    the rank itself, under the names the tests and tools use."""

    def __getattr__(self, name):
        if name in AgreementState.NAMES:
            return getattr(self.ag, name)
        raise AttributeError(name)


# --------------------------------------------------------------- read-back ---
def fault_logs(counts, logs, limit, kinds, what="", node_lo=0, n=None):
    """{(instance, node): [(blamed node, FaultKind name)]} of the fault logs
    logs [B][R][limit] (int16: blamed << 8 | kind) with counts [B][R]; a count
    above `limit` raises "<what>fault log overflow".  node_lo, n: row r is
    node node_lo + r, and the rows at or past node n are padding (a sharded
    Broadcast rank's hosted window)."""
    fc = counts.cpu().numpy()
    fl = logs.cpu().numpy().view(np.uint16)
    out = {}
    for b in range(fc.shape[0]):
        for r in range(fc.shape[1]):
            node = node_lo + r
            if n is not None and node >= n:
                continue
            c = int(fc[b, r])
            if c > limit:
                raise RuntimeError("%sfault log overflow at (%d, %d): %d records"
                                   % (what, b, node, c))
            out[(b, node)] = [(int(v) >> 8, kinds[int(v) & 0xFF]) for v in fl[b, r, :c]]
    return out


ANY = -1   # a flag table's last mask: whatever is set


def check_flags(table, flags, limits):
    """Raise the message of the first (mask, message) of `table` that `flags`
    meets; the message may name the attributes of `limits` as {0.name} and
    the flags as {1}."""
    for mask, message in table:
        if flags & mask:
            raise RuntimeError(message.format(limits, flags))


# One protocol's (or rank's) part in the read-back: its flag table, the object
# whose limits the messages name, and the object and attribute that tally its
# records.
Protocol = collections.namedtuple("Protocol", "flags limits owner attr")


def check_batch(protocols, rows, total, r0):
    """One batch's read-back, rounds r0..: rows [protocol][round][records,
    flags] and total [round] (None: the sum of the rows' records) on the host.
    Per round the flags first, then the tallies; returns the number of rounds
    run at the first round without records anywhere (the rounds after it are
    not looked at), else None.  (Plain ints from here on: this runs inside
    every timed run.)"""
    rows = rows.tolist()
    total = total if total is None else total.tolist()
    for i in range(len(rows[0])):
        for p, row in zip(protocols, rows):
            if row[i][1]:
                check_flags(p.flags, row[i][1], p.limits)
        t = 0
        for p, row in zip(protocols, rows):
            t += row[i][0]
            setattr(p.owner, p.attr, getattr(p.owner, p.attr) + row[i][0])
        if (t if total is None else total[i]) == 0:
            return r0 + i + 1
    return None


def hist_rows(owners):
    """read(r, hi) of a Rounds over the `hist` tensors [max_rounds][2] of
    `owners`, one per protocol: the rows [protocol][round][records, flags] of
    rounds r..hi in one host read; their sum decides quiescence (total None)."""
    def read(r, hi):
        if len(owners) == 1:
            return owners[0].hist[r:hi].cpu().numpy()[None], None
        return torch.stack([o.hist[r:hi] for o in owners]).cpu().numpy(), None
    return read


# ---------------------------------------------------------------- the loop ---
def call(name, fn, *args):
    """A phase launch without the timing hook."""
    fn(*args)


class Rounds:
    """A run of synchronous rounds, split into enqueue and read-back so a
    caller can overlap them with other work: `launch()` resets the nodes and
    enqueues the first `batch` rounds on `stream` (default: the current
    stream) and returns at once; `wait()` reads the rows of the enqueued
    rounds back (one host read, synchronising that stream only), enqueues and
    reads further batches until a round without records, and returns the
    number of rounds: the index of that round + 1.

    reset(): fresh nodes -- every run starts from them: the kernels accumulate
    into the per-round rows, and the inboxes of the rounds after the last
    quiescent one still hold records, so a run never continues another.
    enqueue(r, phase): round r; every kernel launch goes through
    phase(name, fn, *args).  read(r, hi): (rows [protocol][round][2] --
    records to tally, flags --, total [round]: the records that decide
    quiescence, None for the rows' sum) of rounds r..hi, on the host.  The three are given as
    callables, or are the methods of a subclass (which then holds no reference
    to itself: its nodes' memory goes with the last reference to it).
    protocols: a Protocol per row of `rows`.  what: the name in the "did not
    quiesce" error.  events: a list that receives (phase name, start event,
    end event) of every phase launch."""

    def __init__(self, protocols, max_rounds, batch, what, stream=None, events=None,
                 new_event=None, reset=None, enqueue=None, read=None):
        if reset is not None:
            self.reset, self.enqueue, self.read = reset, enqueue, read
        self.protocols, self.max_rounds, self.batch, self.what = protocols, max_rounds, batch, what
        self.stream, self.events, self.new_event = stream, events, new_event
        self.next = 0

    def _timed(self, name, fn, *args):
        new = self.new_event or (lambda: torch.cuda.Event(enable_timing=True))
        e0, e1 = new(), new()
        e0.record()
        fn(*args)
        e1.record()
        self.events.append((name, e0, e1))

    def _ctx(self):
        return torch.cuda.stream(self.stream) if self.stream is not None \
            else contextlib.nullcontext()

    def _enqueue(self, r):
        hi = min(self.max_rounds, r + self.batch)
        phase = call if self.events is None else self._timed
        for rr in range(r, hi):
            self.enqueue(rr, phase)
        self.next = hi

    def launch(self):
        with self._ctx():
            self.reset()
            self._enqueue(0)
        return self

    def wait(self):
        r = 0   # first round whose rows have not been read
        with self._ctx():
            while True:
                hi = self.next
                done = check_batch(self.protocols, *self.read(r, hi), r)   # one read
                if done is not None:
                    return done
                if hi >= self.max_rounds:
                    raise RuntimeError("%s did not quiesce in %d rounds"
                                       % (self.what, self.max_rounds))
                self._enqueue(hi)
                r = hi
