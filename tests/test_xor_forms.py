"""The matrix-specialised XOR-network kernels (csrc/jit.hip, dispatched from
api.hip) at every form the generator emits and at the shard lengths where a
lane's two 16-byte pieces meet the end of a row.

Forms.  gen_xor_source writes different code for the streaming and the LDS
form, for one and for several passes, for one and for several LDS stages, and
a matrix may be split over programs of different forms.  ENCODERS and DECODERS
list one shape per form; the unmarked tests prove from the code-object names
alone (no compile) that each shape still reaches the form it is listed for, so
a changed default fails here instead of silently thinning the GPU sweep.

Lengths.  A lane owns 16 bytes at `off` and 16 at `off + 1024` of a 2 KB
chunk.  LENGTHS takes round_up(S, 16) % 2048 across 0, 16, 1024, 1040 and 2032
(the `active`, `full`, clamp and `edge` conditions), S % 16 and S % 4 through
0, 1 and 15 / 3, and S below 4 (the length prefix spread over several rows).
Payload lengths P = k*S - 4 - d take P % 4 through every residue (the
frame_fixup kernel adds the last P & 3 bytes and their parity), include the
shortest payload of each S, and put the partial last dword across a row
boundary where S <= k.

Every comparison is bit-exact against oracle/pyoracle.py: slabs are poisoned
with 0x5A, payload buffers hold 0xC3 past P, erased rows 0xA5."""
import os
import re

import numpy as np
import pytest

import hbbft_amd as hb
from oracle import pyoracle as orc

gpu = pytest.mark.gpu


def default_f(n):
    return (n - 1) // 3


# ------------------------------------------------------------- the forms ---
# Encoders, as RbcBatch(n, f): k = n - 2f data rows, m = 2f parity rows.
# programs: (LDS form, first parity row, end parity row, row tile, passes) of
# every code object.  shipped: built by __graft_entry__.build().
ENCODERS = [
    dict(n=4, f=1, shipped=True, programs=[(False, 0, 2, 2, 1)],
         form="streaming, one pass"),
    dict(n=16, f=5, shipped=True, programs=[(False, 0, 10, 10, 1)],
         form="streaming, one pass of 10 rows"),
    dict(n=64, f=21, shipped=True, programs=[(True, 0, 42, 7, 6)],
         form="LDS, one stage (22 inputs), six passes"),
    dict(n=128, f=42, shipped=True, programs=[(True, 0, 48, 6, 8), (True, 48, 84, 6, 6)],
         form="LDS, two stages (24 + 20), two programs"),
    dict(n=250, f=83, shipped=True,
         programs=[(True, 0, 48, 6, 8), (True, 48, 96, 6, 8), (True, 96, 144, 6, 8),
                   (True, 144, 166, 6, 4)],
         form="LDS, four stages (24 + 24 + 24 + 12), four programs"),
    dict(n=31, f=10, shipped=False, programs=[(False, 0, 20, 10, 2)],
         form="streaming, two passes of 10 (the switch over waves w, w + nw), pairwise "
              "network, data-row stores spread over the passes"),
    dict(n=30, f=7, shipped=False, programs=[(True, 0, 14, 7, 2)],
         form="LDS at its lower edge (16 inputs, 14 outputs), two passes, one stage"),
    dict(n=39, f=7, shipped=False, programs=[(True, 0, 14, 7, 2)],
         form="LDS, stages of 24 + 1 inputs: wave 1 loads nothing in the second stage "
              "but meets its barriers"),
    dict(n=74, f=29, shipped=False, programs=[(True, 0, 48, 6, 8), (False, 48, 58, 6, 2)],
         form="two programs of different forms: rows 0-48 LDS in eight passes of 6, rows "
              "48-58 streaming in two passes"),
]


def _missing(n, rows):
    p = np.ones(n, np.uint8)
    p[list(rows)] = 0
    return p


# Decoders: the erasure pattern as the set of missing rows; programs as above
# with output-row ranges (indices into the missing rows).
DECODERS = [
    dict(n=31, f=10, shipped=False, missing=range(0, 20), programs=[(False, 0, 20, 10, 2)],
         form="streaming, two passes; every data row gone, row 0 (the length) rebuilt"),
    dict(n=64, f=21, shipped=False, missing=range(1, 14), programs=[(False, 0, 13, 14, 1)],
         form="streaming, one pass: 13 outputs, one below the LDS threshold"),
    dict(n=64, f=21, shipped=False, missing=range(1, 15), programs=[(True, 0, 14, 7, 2)],
         form="LDS, two passes: 14 outputs, the threshold"),
    dict(n=76, f=25, shipped=False, missing=range(0, 50),
         programs=[(True, 0, 50, 7, 8)],
         form="LDS, stages of 24 + 2 inputs, eight waves of which six load nothing in the "
              "second stage"),
    dict(n=250, f=83, shipped=True,
         missing=[i for i in range(250) if not 84 <= i < 168],
         programs=[(True, 0, 48, 6, 8), (True, 48, 96, 6, 8), (True, 96, 144, 6, 8),
                   (True, 144, 166, 6, 4)],
         form="the shipped worst case: only parity rows k..2k-1 present, four programs"),
]
for _e in DECODERS:
    _e["present"] = _missing(_e["n"], _e["missing"])


def _km(e):
    return e["n"] - 2 * e["f"], 2 * e["f"]


def _eid(e):
    return "n%d_f%d" % (e["n"], e["f"]) + ("_miss%d" % len(e["missing"]) if "missing" in e else "")


def parse_name(name):
    """(LDS form, r_lo, r_hi, rt, passes, waves-per-SIMD target or 0, fused unframe)."""
    assert name.endswith(".co"), name
    rt = int(re.search(r"_rt(\d+)_", name).group(1))
    lo, hi = map(int, re.search(r"_r(\d+)_(\d+)", name).groups())
    lds = re.search(r"_L\d*_", name) is not None
    wpe = re.search(r"_w([1-9])_", name)
    return (lds, lo, hi, rt, -(-(hi - lo) // rt), int(wpe.group(1)) if wpe else 0,
            re.search(r"_uf_v\d+\.co$", name) is not None)


def encoder_names(e):
    k, m = _km(e)
    return [hb.jit_file_name(k, m, g) for g in range(hb.jit_encode_groups(k, m))]


def decoder_names(e, uf):
    k, m = _km(e)
    return [hb.jit_decode_file_name(k, m, e["present"], g, fused_unframe=uf)
            for g in range(hb.jit_decode_groups(k, m, e["present"]))]


def check_programs(names, want, uf=False):
    got = [parse_name(s) for s in names]
    assert [g[:5] for g in got] == want, names
    for (lds, lo, hi, rt, npass, wpe, is_uf), s in zip(got, names):
        assert is_uf == uf, s
        # the LDS form runs one wave per pass, 2..8 of them, and its short
        # passes target four waves per SIMD
        assert not lds or 2 <= npass <= 8, s
        assert wpe == ((4 if rt <= 8 else 3) if lds else 0), s


@pytest.mark.parametrize("e", ENCODERS, ids=_eid)
def test_encoder_reaches_its_form(e):
    k, m = _km(e)
    assert e["f"] == default_f(e["n"]) or not e["shipped"]
    names = encoder_names(e)
    check_programs(names, e["programs"])
    assert names[0].startswith("hbrbc_enc_k%d_m%d_" % (k, m))
    assert e["programs"][0][1] == 0 and e["programs"][-1][2] == m
    assert all(a[2] == b[1] for a, b in zip(e["programs"], e["programs"][1:]))


@pytest.mark.parametrize("uf", [False, True], ids=["plain", "uf"])
@pytest.mark.parametrize("e", DECODERS, ids=_eid)
def test_decoder_reaches_its_form(e, uf):
    k, m = _km(e)
    names = decoder_names(e, uf)
    check_programs(names, e["programs"], uf)
    assert names[0].startswith("hbrbc_dec_n%d_" % e["n"])
    assert e["programs"][-1][2] == len(e["missing"]) <= m
    assert e["present"].sum() >= k


def test_form_table_covers_every_generated_form():
    """What the shapes are in the table for, restated from the parsed names:
    both forms, one and several passes in each, one / two / four LDS stages, a
    last LDS stage shorter than the wave count, the LDS threshold pair and a
    matrix split over programs of both forms."""
    enc = {(e["n"], e["f"]): ([parse_name(s) for s in encoder_names(e)], _km(e)[0])
           for e in ENCODERS}
    dec = [([parse_name(s) for s in decoder_names(e, False)], _km(e)[0], len(e["missing"]))
           for e in DECODERS]
    progs = [(p, k) for ps, k in enc.values() for p in ps] + \
            [(p, k) for ps, k, _ in dec for p in ps]
    stream = [(p, k) for p, k in progs if not p[0]]
    lds = [(p, k) for p, k in progs if p[0]]
    assert any(p[4] == 1 for p, _ in stream) and any(p[4] >= 2 for p, _ in stream)
    assert {-(-k // 24) for _, k in lds} >= {1, 2, 4}                 # LDS stages of 24 inputs
    assert any(0 < k % 24 < p[4] for p, k in lds)                     # idle loader waves
    assert any(k == 16 and p[2] - p[1] == 14 for p, k in lds)         # the threshold itself
    # the threshold pair: same inputs, 13 outputs streaming, 14 outputs LDS
    pair = {n_out: ps[0][0] for ps, k, n_out in dec if k == 22}
    assert pair == {13: False, 14: True}
    assert any({p[0] for p in ps} == {True, False} for ps, _ in enc.values())
    # streaming with several passes takes the pairwise network only above 8 rows a pass
    assert any(not p[0] and p[4] >= 2 and p[3] > 8 for p, _ in progs)


# ----------------------------------------------------------- the lengths ---
LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33,
           1007, 1008, 1009, 1023, 1024, 1025, 1039, 1040, 1041,
           2031, 2032, 2033, 2047, 2048, 2049, 2064,
           3071, 3072, 3073, 3088, 3089, 4095, 4096, 4097]
BANDS = {"tiny": (1, 64), "1k": (1000, 1100), "2k": (2000, 2100), "3-4k": (3000, 4100)}


def band(name):
    lo, hi = BANDS[name]
    return [S for S in LENGTHS if lo <= S < hi]


def deltas(S, k):
    """d of the payload lengths P = k*S - 4 - d of one shard length: every
    residue of P % 4, the shortest payload of that S, and (S <= k) a partial
    last dword that lies across a row boundary."""
    return sorted({d for d in (0, 1, 2, 3, k - 1, S - 2, S - 1, S) if 0 <= d <= k - 1})


def cases(k, lengths=LENGTHS, ds=None):
    """(S, d, P) of a sweep; the cases left out are returned too."""
    run, skipped = [], []
    for S in lengths:
        for d in deltas(S, k):
            if ds is not None and d not in ds:
                continue
            P = k * S - 4 - d
            (run if P >= 0 else skipped).append((S, d, P))
    return run, skipped


def straddles(S, P):
    """The last partial payload dword (frame_fixup's bytes) lies in two rows."""
    return P % 4 != 0 and ((P & ~3) + 4) // S != (P + 3) // S


def test_bands_partition_the_lengths():
    assert sorted(S for b in BANDS for S in band(b)) == LENGTHS
    for r in (0, 16, 1024, 1040, 2032):
        assert any((S + 15) // 16 * 16 % 2048 == r for S in LENGTHS), r
        # and one byte to either side of the boundary
        assert any((S - 1 + 15) // 16 * 16 % 2048 == r and (S + 15) // 16 * 16 % 2048 != r
                   for S in LENGTHS), r
    assert {S % 16 for S in LENGTHS} >= {0, 1, 15} and {S % 4 for S in LENGTHS} == {0, 1, 2, 3}


@pytest.mark.parametrize("e", ENCODERS, ids=_eid)
def test_sweep_conditions(e):
    """What the sweep claims to cover, asserted: the library agrees on S for
    every case, nothing is left out at S >= 4, only a negative payload length
    is left out below, every residue of P % 4 occurs, and shapes with k >= 6
    have payloads whose last partial dword straddles two rows."""
    k, _ = _km(e)
    run, skipped = cases(k)
    assert all(hb.shard_len(P, k) == S == orc.shard_len(P, k) for S, _, P in run)
    assert all(S < 4 and P < 0 for S, _, P in skipped)
    assert {S for S, _, _ in run} >= {S for S in LENGTHS if S >= 4}
    assert {P % 4 for _, _, P in run} == {0, 1, 2, 3}
    for S in LENGTHS:
        if S >= 4 and k >= 4:       # d = 0..3 all exist: every residue at every length
            assert {P % 4 for s, _, P in run if s == S} == {0, 1, 2, 3}, S
    if k >= 6:
        assert any(straddles(S, P) for S, _, P in run)
    # the decode legs run d in {0, 3}: shard lengths of every residue mod 4
    sub, _ = cases(k, ds=(0, 3))
    assert {S % 4 for S, _, _ in sub} == {0, 1, 2, 3}


# ------------------------------------------------------------- GPU sweep ---
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def forms_dir(tmp_path_factory):
    """Every shape that build() does not ship, compiled once (hiprtc) into one
    code-object directory: the encoders, and each decoder with its
    fused-unframe variant.  The sweep below compiles nothing further."""
    d = str(tmp_path_factory.mktemp("xor_forms_jit"))
    for e in ENCODERS:
        if not e["shipped"]:
            hb.jit_build_encode(*_km(e), d)
    for e in DECODERS:
        if not e["shipped"]:
            k, m = _km(e)
            for uf in (False, True):
                for g in range(hb.jit_decode_groups(k, m, e["present"])):
                    hb.jit_build_decode(k, m, e["present"], g, directory=d, fused_unframe=uf)
    return d


def shipped_dir():
    return os.path.join(os.path.dirname(hb.LIB_PATH), "jit")


def jit_dir_of(e, monkeypatch, forms_dir):
    """Point the library at the directory that holds this shape's code objects."""
    if e["shipped"]:
        monkeypatch.delenv("HBRBC_JIT_DIR", raising=False)
        return shipped_dir()
    monkeypatch.setenv("HBRBC_JIT_DIR", forms_dir)
    return forms_dir


def instances(e):
    return 2 if e["n"] >= 128 else 3


_REF = {}


def reference(n, f, S, d, i):
    """(payload, the oracle's shards [n, S], root) of instance i of a case.
    Computed once for the d the encode and decode legs share."""
    key = (n, f, S, d, i)
    if key in _REF:
        return _REF[key]
    k = n - 2 * f
    P = k * S - 4 - d
    pay = orc.gen_payload(0x58464D53 + 131 * S + d, i, P)
    sh, nodes = orc.send_shards(n, f, pay.tobytes())
    assert sh.shape == (n, S)
    for a in (pay, sh):
        a.setflags(write=False)
    r = (pay, sh, nodes[-1].tobytes())
    if d in (0, 3):
        _REF[key] = r
    return r


def expected_slab(refs, stride):
    n, S = refs[0][1].shape
    out = np.zeros((len(refs), n, stride), np.uint8)
    for i, r in enumerate(refs):
        out[i, :, :S] = r[1]
    return out


def guarded(torch, count, n, stride):
    """A [count, n, stride] slab poisoned with 0x5A inside a larger poisoned
    allocation: at least one row stride of guard bytes on either side."""
    g = max(stride, 256)
    body = count * n * stride
    buf = torch.full((g + body + g,), 0x5A, dtype=torch.uint8, device="cuda")
    return buf, buf[g:g + body].view(count, n, stride), g


def check_slab(buf, g, want, ctx):
    h = buf.cpu().numpy()
    assert (h[:g] == 0x5A).all() and (h[h.size - g:] == 0x5A).all(), ("guard band written", ctx)
    got = h[g:h.size - g].reshape(want.shape)
    if not np.array_equal(got, want):
        S = ctx[1]
        bad = sorted({(int(i), int(j)) for i, j, _ in np.argwhere(got != want)})
        pad = bool((got[:, :, S:] != want[:, :, S:]).any())
        raise AssertionError("(n, S, P) = %r: rows (instance, row) %r differ from the oracle%s"
                             % (ctx, bad[:12], "; padding not zero" if pad else ""))


def upload_payloads(torch, refs, P):
    pstride = max(16, (P + 15) // 16 * 16)
    t = torch.full((len(refs), pstride), 0xC3, dtype=torch.uint8, device="cuda")   # junk past P
    if P:
        t[:, :P] = torch.from_numpy(np.stack([r[0] for r in refs])).cuda()
    return t


@gpu
@pytest.mark.parametrize("b", list(BANDS))
@pytest.mark.parametrize("e", ENCODERS, ids=_eid)
def test_frame_encode_lengths(torch_cuda, monkeypatch, forms_dir, e, b):
    """Fused frame+encode: every row equals the oracle's shard, every padding
    byte is zero and nothing outside the slab is written.  With several
    programs and P % 4 != 0 the first program's twin, frame_fixup and the
    other programs must run in that order over completed data rows."""
    torch = torch_cuda
    n, f = e["n"], e["f"]
    jit_dir_of(e, monkeypatch, forms_dir)
    rb = hb.RbcBatch(n, f, device=0)
    assert rb.coding.encode_kernel() == "specialised"
    run, _ = cases(rb.k, band(b))
    assert run
    count = instances(e)
    for S, d, P in run:
        refs = [reference(n, f, S, d, i) for i in range(count)]
        stride = rb.stride_for(S)
        buf, slab, g = guarded(torch, count, n, stride)
        rb.frame_encode(upload_payloads(torch, refs, P), P, slab)
        torch.cuda.synchronize()
        check_slab(buf, g, expected_slab(refs, stride), (n, S, P))


def one_delta(k, S):
    """One payload length of a shard length: d = 3 where that payload exists."""
    run, _ = cases(k, [S])
    return ([c for c in run if c[1] == 3] or run or [None])[0]


@gpu
@pytest.mark.parametrize("b", list(BANDS))
@pytest.mark.parametrize("e", ENCODERS, ids=_eid)
def test_encode_lengths(torch_cuda, monkeypatch, forms_dir, e, b):
    """Plain encode from the oracle's framed data rows: parity rows and their
    padding equal the oracle's, the data rows are left alone."""
    torch = torch_cuda
    n, f = e["n"], e["f"]
    jit_dir_of(e, monkeypatch, forms_dir)
    rb = hb.RbcBatch(n, f, device=0)
    assert rb.coding.encode_kernel() == "specialised"
    count = instances(e)
    ran = 0
    for S in band(b):
        c = one_delta(rb.k, S)
        if c is None:
            assert S < 4
            continue
        _, d, P = c
        refs = [reference(n, f, S, d, i) for i in range(count)]
        stride = rb.stride_for(S)
        want = expected_slab(refs, stride)
        buf, slab, g = guarded(torch, count, n, stride)
        slab[:, :rb.k] = torch.from_numpy(want[:, :rb.k]).cuda()
        rb.encode(slab, S)
        torch.cuda.synchronize()
        check_slab(buf, g, want, (n, S, P))
        ran += 1
    assert ran >= len([S for S in band(b) if S >= 4])


def erasures(e, count, S):
    """Two instances of the specialised pattern and one of another f-erasure
    pattern, which the generic kernel serves in the same call."""
    n, f = e["n"], e["f"]
    present = np.tile(e["present"], (count, 1))
    rng = np.random.default_rng(n * 7919 + S)
    while True:
        other = _missing(n, rng.permutation(n)[:f])
        if not np.array_equal(other, e["present"]):
            break
    present[count - 1] = other
    return present


def received(torch, want, present):
    """The oracle's slab with every erased row slot, padding included, 0xA5."""
    count, n, stride = want.shape
    buf, slab, g = guarded(torch, count, n, stride)
    slab.copy_(torch.from_numpy(want).cuda())
    slab[torch.from_numpy(present).cuda() == 0] = 0xA5
    return buf, slab, g


@gpu
@pytest.mark.parametrize("b", list(BANDS))
@pytest.mark.parametrize("e", DECODERS, ids=_eid)
def test_reconstruct_lengths(torch_cuda, monkeypatch, forms_dir, e, b):
    """Specialised reconstruct from the oracle's shards: the whole slab,
    padding included, equals the oracle's and every status is 0."""
    torch = torch_cuda
    n, f = e["n"], e["f"]
    jit_dir_of(e, monkeypatch, forms_dir)
    rb = hb.RbcBatch(n, f, device=0)
    rb.specialise_decoder(e["present"])
    run, _ = cases(rb.k, band(b), ds=(0, 3))
    assert {S for S, _, _ in run} >= {S for S in band(b) if S >= 4}
    count = 3
    for S, d, P in run:
        refs = [reference(n, f, S, d, i) for i in range(count)]
        want = expected_slab(refs, rb.stride_for(S))
        present = erasures(e, count, S)
        buf, slab, g = received(torch, want, present)
        status = torch.full((count,), -1, dtype=torch.int32, device="cuda")
        rb.reconstruct(slab, S, torch.from_numpy(present).cuda(), status)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * count, (n, S, P)
        check_slab(buf, g, want, (n, S, P))


# the shipped N = 250 decoder runs the tiny and the 2 KB band
UF_CASES = [pytest.param(e, b, id="%s-%s" % (_eid(e), b)) for e in DECODERS for b in BANDS
            if not e["shipped"] or b in ("tiny", "2k")]


@gpu
@pytest.mark.parametrize("e,b", UF_CASES)
def test_decode_fused_unframe_lengths(torch_cuda, monkeypatch, forms_dir, e, b):
    """decode_from_shards through the `_uf` programs (HBRBC_UNFRAME_FUSED=1)
    and through the separate unframe (=0): payload slot, length and status of
    both equal the oracle's, the slot is zero past the payload, at shard
    lengths of every residue mod 4."""
    torch = torch_cuda
    n, f = e["n"], e["f"]
    where = jit_dir_of(e, monkeypatch, forms_dir)
    rb = hb.RbcBatch(n, f, device=0)
    k = rb.k
    rb.specialise_decoder(e["present"])
    run, _ = cases(k, band(b), ds=(0, 3))
    assert {S for S, _, _ in run} >= {S for S in band(b) if S >= 4}
    count = 3
    fused_any = False
    for S, d, P in run:
        refs = [reference(n, f, S, d, i) for i in range(count)]
        want = expected_slab(refs, rb.stride_for(S))
        present = erasures(e, count, S)
        pres_d = torch.from_numpy(present).cuda()
        roots = torch.from_numpy(np.stack([np.frombuffer(r[2], np.uint8) for r in refs])).cuda()
        slot = (k * S - 4 + 15) // 16 * 16          # unframe defines the chunks covering k*S - 4
        ostride = max(16, (k * S + 15) // 16 * 16)
        got = {}
        for env in ("1", "0"):
            monkeypatch.setenv("HBRBC_UNFRAME_FUSED", env)
            buf, slab, g = received(torch, want, present)
            out = torch.full((count, ostride), 0x5A, dtype=torch.uint8, device="cuda")
            plo = torch.full((count,), -1, dtype=torch.int32, device="cuda")
            st = torch.full((count,), -1, dtype=torch.int32, device="cuda")
            rb.decode(slab, S, pres_d, roots, rb.alloc_nodes(count), out, plo, st)
            torch.cuda.synchronize()
            if env == "1" and k * S > 4:
                # the _uf variant loaded: a missing one falls back silently
                assert rb.unframe_fused(S, ostride), (n, S)
                fused_any = True
            check_slab(buf, g, want, (n, S, P))
            got[env] = (out.cpu().numpy()[:, :slot], plo.cpu().numpy(), st.cpu().numpy())
        for x, y in zip(got["1"], got["0"]):
            assert np.array_equal(x, y), (n, S, P)
        out, plo, st = got["1"]
        for i in range(count):
            sh = want[i, :, :S].copy()
            sh[present[i] == 0] = 0xA5
            ref, code, _ = orc.decode_from_shards(n, f, sh, present[i], refs[i][2])
            assert ref == refs[i][0].tobytes() and code == 0
            assert st[i] == 0 and plo[i] == len(ref) == P, (n, S, P, i)
            assert out[i, :P].tobytes() == ref, (n, S, P, i)
            assert not out[i, P:].any(), ("slot not zero past the payload", n, S, P, i)
    assert fused_any
    for s in decoder_names(e, True):
        assert os.path.exists(os.path.join(where, s)), s


@gpu
def test_frame_encode_blocked_lengths(torch_cuda, monkeypatch):
    """The blocked row layout (rows_per_block = 8 at N = 64, whose code
    objects ship) at lane-edge lengths: the plain layout's oracle bytes."""
    torch = torch_cuda
    monkeypatch.delenv("HBRBC_JIT_DIR", raising=False)
    n, f, R, count, d = 64, 21, 8, 3, 3
    rb = hb.RbcBatch(n, f, device=0)
    k = rb.k
    assert os.path.exists(os.path.join(shipped_dir(), hb.jit_file_name(k, 2 * f, 0, R)))
    for S in (1009, 1040, 2049):
        P = k * S - 4 - d
        refs = [reference(n, f, S, d, i) for i in range(count)]
        st = rb.stride_for(S)
        G = -(-n // R)
        # [G][count][R][stride]: block q of every instance, then the next block
        buf = torch.full((G + 2, count, R, st), 0x5A, dtype=torch.uint8, device="cuda")
        rb.frame_encode_rows(upload_payloads(torch, refs, P), P, buf[1:G + 1], count, st, R,
                             count * R * st, R * st)
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert (h[0] == 0x5A).all() and (h[G + 1] == 0x5A).all(), "guard band written"
        want = expected_slab(refs, st)
        for i in range(count):
            got = h[1:G + 1, i].reshape(G * R, st)[:n]
            assert np.array_equal(got, want[i]), (S, P, i)
