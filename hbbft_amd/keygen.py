"""SyncKeyGen's G1 work on the MI355X: commitment evaluation, Part and Ack
checks, the generated key set and its key shares.

hbbft's `SyncKeyGen` (src/sync_key_gen.rs of the reference; DynamicHoneyBadger
runs it at every validator change) has every proposer commit to a symmetric
bivariate polynomial f of degree t: the `BivarCommitment` C[i][j] = [f_ij] G1.
From `threshold_crypto` (rev 624eeee), for integer points x, y:

    BivarCommitment::row(x)          the Commitment with coefficient j = sum_i [x^i] C[i][j]
    BivarCommitment::evaluate(x, y)  sum_ij [x^i y^j] C[i][j] = row(x).evaluate(y)
    Commitment::evaluate(y)          sum_j [y^j] c_j
    PublicKeySet::public_key_share(i)  commit.evaluate(i + 1); public_key() = coefficient 0

What a node computes with them:

    handle_part_or_fault (:542-573)  commit.row(our_idx + 1) (:557) and
                                     row.commitment() != commit_row (:569):
                                     [row_j] G1::one() == row(our_idx + 1)_j for every j
    handle_ack_or_fault (:576-608)   commit.evaluate(our_idx + 1, sender_idx + 1)
                                     != G1Affine::one().mul(val) (:603)
    generate (:516-534)              pk_commit += part.commit.row(0) over the complete
                                     parts (is_complete, :342-344: more than 2t Acks)

All of it is polynomial evaluation in G1 at node indices of a few bits plus
fixed-base comparisons: `hbrbc_g1_poly_eval_prepared` (Horner's rule, one lane
per evaluation, results in g1_prepare table form so they feed the next step on
the device) and `hbrbc_g1_base_mul_check` (hbbft_amd/csrc/pairing.hip).

The sending side is here too, for a simulator or test network that hosts
every node: `base_mul` ([s] G1::one() with a result: `BivarPoly::commitment`,
`public_key_share`), `fr_poly_eval` (`BivarPoly::row`, `Poly::evaluate`) and
`fr_dot` (with the Lagrange coefficients: the `Poly::interpolate(..)
.evaluate(0)` of `generate`, :523-524) carry `generate_part` (:413-417),
`ack_values` (:459), `secret_key_share` and `sync_key_gen_network`, an honest
N-node run whose secret key shares feed threshold.create_decryption_shares /
create_signature_shares.  These kernels branch on scalar bits: they are not
constant-time.

Encrypting and decrypting rows and values stays with the caller
(`sec_key.decrypt`, :564-567, :596-599; threshold.py has xor_with_hash and
hash_g1_g2 to build it from); the functions here take and return Fr scalars as
32 big-endian bytes.
So does `BivarPoly::random`.
Commitment points arrive compressed (48 bytes), as the messages carry them.
Functions that take node indices form x = idx + 1 and raise ValueError for
idx >= 0xFFFFFFFF.  There is no CPU fallback: without the library or a GPU
the calls raise `HbrbcUnavailable`.
"""
from . import HbrbcUnavailable, _check, lib  # noqa: F401
from .threshold import (CHECK_FAIL, CHECK_INVALID, CHECK_OK, FR_BYTES,  # noqa: F401
                        G1_BYTES, G1_COMPRESSED_BYTES, _g1_rows, _need_gpu, _ragged, _stream,
                        _torch, _u32_tensor, g1_prepare_compressed)

EVAL_OK, EVAL_INFINITY, EVAL_INVALID = 0, 1, 2


def coeff_pos(i, j):
    """Position of the entry (i, j) = (j, i) of a `BivarCommitment` of degree t
    among its (t + 1)(t + 2) / 2 points: min(i, j) + max(i, j) (max(i, j) + 1)
    / 2 -- the lower triangle row by row.  The crate's source is not at hand,
    so this layout is the project's own definition of the point order, kept in
    this one helper; a caller with another order permutes once."""
    lo, hi = (i, j) if i <= j else (j, i)
    return lo + hi * (hi + 1) // 2


def commitment_len(t):
    """Points of a `BivarCommitment` of degree t."""
    return (t + 1) * (t + 2) // 2


def _x_of(idx):
    if not 0 <= idx < 0xFFFFFFFF:
        raise ValueError("node index %r: x = idx + 1 must fit 32 bits" % (idx,))
    return idx + 1


def _i32(values, dev):
    import numpy as np
    return _torch().from_numpy(np.asarray(values, dtype=np.int32).reshape(-1)).to(dev)


def _offsets(lengths, dev):
    import numpy as np
    offs = np.zeros(len(lengths) + 1, np.int32)
    offs[1:] = np.cumsum(lengths)
    return _torch().from_numpy(offs).to(dev)


def poly_eval_prepared(tab, prepared_count, rows, offsets, poly, x, encode=True, stream=None):
    """Evaluates ragged G1 polynomials over T = tab, a g1_prepare table of
    exactly `prepared_count` points: polynomial p has the coefficients
    T[rows[offsets[p] .. offsets[p + 1])], constant term first (rows int32
    [total], offsets int32 [polys + 1]); evaluation e is polynomial poly[e] at
    x[e] (poly int32 [evals]; x int32 [evals], the bits of an unsigned 32-bit
    value: the raw point, not index + 1).  Returns (table uint8 -- the results
    as a g1_prepare table of `evals` points --, out96 uint8 [evals, 96], out48
    uint8 [evals, 48] (both None without `encode`), status uint8 [evals]: 0 ok,
    1 infinity, 2 invalid table entry, row or poly index)."""
    _need_gpu()
    torch = _torch()
    assert tab.numel() == lib().hbrbc_g1_prepared_size(prepared_count)
    assert rows.dtype == torch.int32 and rows.dim() == 1
    polys, total = _ragged(offsets, rows)
    assert poly.dtype == torch.int32 and poly.dim() == 1 and poly.is_contiguous()
    assert x.dtype == torch.int32 and x.shape == poly.shape and x.is_contiguous()
    assert tab.device == rows.device == poly.device == x.device
    evals = poly.shape[0]
    dev = rows.device
    out = torch.empty(max(1, lib().hbrbc_g1_prepared_size(evals)), dtype=torch.uint8, device=dev)
    o96 = o48 = None
    if encode:
        o96 = torch.empty((evals, G1_BYTES), dtype=torch.uint8, device=dev)
        o48 = torch.empty((evals, G1_COMPRESSED_BYTES), dtype=torch.uint8, device=dev)
    st = torch.empty((evals,), dtype=torch.uint8, device=dev)
    if total == 0:   # only empty polynomials: the entry still wants a rows pointer
        rows = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(lib().hbrbc_g1_poly_eval_prepared(
        tab.data_ptr(), prepared_count, rows.data_ptr(), offsets.data_ptr(), polys,
        poly.data_ptr(), x.data_ptr(), evals, out.data_ptr(),
        o96.data_ptr() if encode else None, o48.data_ptr() if encode else None, st.data_ptr(),
        _stream(dev, stream)))
    return out, o96, o48, st


def base_mul_check(tab, prepared_count, rows, scalars, stream=None):
    """count checks [s_i] G1::one() == T[rows[i]] over T = tab, a g1_prepare
    table of exactly `prepared_count` points: rows int32 [count], scalars uint8
    [count, 32] (big-endian).  Returns uint8 [count]: 1 equal, 0 not, 2 invalid
    table entry, row or scalar (>= r)."""
    _need_gpu()
    torch = _torch()
    assert tab.numel() == lib().hbrbc_g1_prepared_size(prepared_count)
    assert rows.dtype == torch.int32 and rows.dim() == 1 and rows.is_contiguous()
    count = rows.shape[0]
    assert scalars.dtype == torch.uint8 and scalars.shape == (count, FR_BYTES)
    assert scalars.is_contiguous() and tab.device == rows.device == scalars.device
    ok = torch.empty((count,), dtype=torch.uint8, device=rows.device)
    _check(lib().hbrbc_g1_base_mul_check(tab.data_ptr(), prepared_count, rows.data_ptr(),
                                         scalars.data_ptr(), count, ok.data_ptr(),
                                         _stream(rows.device, stream)))
    return ok


def base_mul(scalars, encode=True, stream=None):
    """[s_i] G1::one() for scalars uint8 [count, 32] (big-endian, < r):
    `Poly::commitment`, `BivarPoly::commitment`, `public_key_share`.  Returns
    (table uint8 -- the results as a g1_prepare table of `count` points --,
    out96 uint8 [count, 96], out48 uint8 [count, 48] (both None without
    `encode`), status uint8 [count]: 0 ok, 1 infinity (s = 0), 2 s >= r).  Not
    constant-time."""
    torch = _torch()
    assert scalars.dtype == torch.uint8 and scalars.dim() == 2 and scalars.shape[1] == FR_BYTES
    assert scalars.is_contiguous()
    _need_gpu()
    count, dev = scalars.shape[0], scalars.device
    out = torch.empty(max(1, lib().hbrbc_g1_prepared_size(count)), dtype=torch.uint8, device=dev)
    o96 = o48 = None
    if encode:
        o96 = torch.empty((count, G1_BYTES), dtype=torch.uint8, device=dev)
        o48 = torch.empty((count, G1_COMPRESSED_BYTES), dtype=torch.uint8, device=dev)
    st = torch.empty((count,), dtype=torch.uint8, device=dev)
    _check(lib().hbrbc_g1_base_mul(scalars.data_ptr(), count, out.data_ptr(),
                                   o96.data_ptr() if encode else None,
                                   o48.data_ptr() if encode else None, st.data_ptr(),
                                   _stream(dev, stream)))
    return out, o96, o48, st


def fr_poly_eval(scalars, rows, offsets, poly, x, stream=None):
    """poly_eval_prepared in the scalar field: polynomial p has the
    coefficients scalars[rows[offsets[p] .. offsets[p + 1])], constant term
    first (scalars uint8 [nscalars, 32], rows int32 [total], offsets int32
    [polys + 1]); evaluation e is polynomial poly[e] at x[e] (int32 [evals],
    x the bits of an unsigned 32-bit value).  Returns (out uint8 [evals, 32],
    status uint8 [evals]: 0 ok, 2 a coefficient >= r, a row or poly index out
    of range -- zero bytes)."""
    torch = _torch()
    assert scalars.dtype == torch.uint8 and scalars.dim() == 2 and scalars.shape[1] == FR_BYTES
    assert scalars.is_contiguous()
    assert rows.dtype == torch.int32 and rows.dim() == 1
    polys, total = _ragged(offsets, rows)
    assert poly.dtype == torch.int32 and poly.dim() == 1 and poly.is_contiguous()
    assert x.dtype == torch.int32 and x.shape == poly.shape and x.is_contiguous()
    assert scalars.device == rows.device == poly.device == x.device
    _need_gpu()
    evals, dev = poly.shape[0], rows.device
    out = torch.empty((evals, FR_BYTES), dtype=torch.uint8, device=dev)
    st = torch.empty((evals,), dtype=torch.uint8, device=dev)
    if total == 0:   # only empty polynomials: the entry still wants a rows pointer
        rows = torch.zeros(1, dtype=torch.int32, device=dev)
    if scalars.shape[0] == 0:
        scalars = torch.zeros((1, FR_BYTES), dtype=torch.uint8, device=dev)
        nscalars = 0
    else:
        nscalars = scalars.shape[0]
    _check(lib().hbrbc_fr_poly_eval(scalars.data_ptr(), nscalars, rows.data_ptr(),
                                    offsets.data_ptr(), polys, poly.data_ptr(), x.data_ptr(),
                                    evals, out.data_ptr(), st.data_ptr(), _stream(dev, stream)))
    return out, st


def fr_dot(a, b, offsets, stream=None):
    """Per group sum_j a_j b_j mod r over ragged groups: a, b uint8 [total, 32],
    offsets int32 [groups + 1].  Returns (out uint8 [groups, 32], status uint8
    [groups]: 0 ok, 2 an operand >= r -- zero bytes).  With the coefficients of
    threshold.lagrange_coeffs this interpolates at 0."""
    torch = _torch()
    for s in (a, b):
        assert s.dtype == torch.uint8 and s.dim() == 2 and s.shape[1] == FR_BYTES
    groups, total = _ragged(offsets, a, b)
    _need_gpu()
    dev = a.device
    out = torch.empty((groups, FR_BYTES), dtype=torch.uint8, device=dev)
    st = torch.empty((groups,), dtype=torch.uint8, device=dev)
    _check(lib().hbrbc_fr_dot(a.data_ptr(), b.data_ptr(), offsets.data_ptr(), groups, total,
                              out.data_ptr(), st.data_ptr(), _stream(dev, stream)))
    return out, st


def commitment_rows(commit_tab, commits, t, requests, stream=None):
    """`BivarCommitment::row(x)` for requests = [(commitment, x)] over
    commit_tab, the g1_prepare table of `commits` commitments of degree t laid
    end to end (commitment_len(t) points each, in coeff_pos order).  Coefficient
    j of a row is one polynomial over the entries (0..t, j), evaluated at x.
    Returns (the g1_prepare table of len(requests) * (t + 1) points, request-
    major; status uint8 [len(requests) * (t + 1)])."""
    m = commitment_len(t)
    dev = commit_tab.device
    used = sorted({c for c, _ in requests})
    slot = {c: k for k, c in enumerate(used)}
    rows = [c * m + coeff_pos(i, j) for c in used for j in range(t + 1) for i in range(t + 1)]
    poly = [slot[c] * (t + 1) + j for c, _ in requests for j in range(t + 1)]
    xs = [x for _, x in requests for _ in range(t + 1)]
    tab, _, _, st = poly_eval_prepared(
        commit_tab, commits * m, _i32(rows, dev), _offsets([t + 1] * (len(used) * (t + 1)), dev),
        _i32(poly, dev), _u32_tensor(xs, dev), encode=False, stream=stream)
    return tab, st


def _points48(points, what):
    for p in points:
        if len(p) != G1_COMPRESSED_BYTES:
            raise ValueError("%s of %d bytes, expected %d" % (what, len(p), G1_COMPRESSED_BYTES))


def _scalars(values, dev, what):
    import numpy as np
    for v in values:
        if len(v) != FR_BYTES:
            raise ValueError("%s of %d bytes, expected %d" % (what, len(v), FR_BYTES))
    a = np.empty((len(values), FR_BYTES), np.uint8)
    for r, v in enumerate(values):
        a[r] = np.frombuffer(v, np.uint8)
    return _torch().from_numpy(a).to(dev)


def _encodings(o96, o48, st):
    a, b, s = o96.cpu().numpy(), o48.cpu().numpy(), st.cpu().tolist()
    return [(bytes(a[k]), bytes(b[k])) if v != EVAL_INVALID else None for k, v in enumerate(s)]


def _key_shares(tab, count, n, dev):
    """public_key() and public_key_share(0..n) of the commitment in `tab`."""
    rows, offs = _i32(list(range(count)), dev), _offsets([count], dev)
    shares = poly_eval_prepared(tab, count, rows, offs, _i32([0] * n, dev),
                                _u32_tensor([i + 1 for i in range(n)], dev))
    _, p96, p48, pst = poly_eval_prepared(tab, count, rows, offs, _i32([0], dev),
                                          _u32_tensor([0], dev))
    return shares, _encodings(p96, p48, pst)[0]


def public_key_shares(commitment48, n, device=0):
    """The keys of a `PublicKeySet`: commitment48 = its Commitment, t + 1
    compressed G1 points, constant term first.  `public_key()` is coefficient
    0, `public_key_share(i)` = commit.evaluate(i + 1) for i < n.  Returns
    (table, out96 uint8 [n, 96], out48 uint8 [n, 48], status uint8 [n],
    public_key): `table` is the g1_prepare table of the n key shares -- what
    pairing_check_prepared_keys and sig_check_prepared take as keys, bit for bit
    the table g1_prepare gives for the same points --, public_key the pair
    (96 bytes, 48 bytes), or None when the commitment does not decode."""
    _points48(commitment48, "commitment point")
    if not 0 < n <= 0xFFFFFFFF:
        raise ValueError("n = %r key shares" % (n,))
    _need_gpu()
    dev = "cuda:%d" % device
    count = len(commitment48)
    tab = g1_prepare_compressed(_g1_rows(commitment48, dev, G1_COMPRESSED_BYTES))
    (stab, o96, o48, st), pk = _key_shares(tab, count, n, dev)
    return stab, o96, o48, st, pk


def _outcomes(ok, per):
    """Per group of `per` check outcomes: None with an invalid one, else all equal."""
    out = []
    for g in range(len(ok) // per):
        part = ok[g * per:(g + 1) * per]
        out.append(None if CHECK_INVALID in part else all(v == CHECK_OK for v in part))
    return out


def _prepare_parts(t, parts, dev):
    """The g1_prepare table of every part's commitment, end to end."""
    m = commitment_len(t)
    flat = []
    for commit, _ in parts:
        if len(commit) != m:
            raise ValueError("commitment of %d points, expected %d" % (len(commit), m))
        flat += commit
    _points48(flat, "commitment point")
    return g1_prepare_compressed(_g1_rows(flat, dev, G1_COMPRESSED_BYTES))


def _check_parts(t, x, parts, ctab, dev):
    n = len(parts)
    coeffs = []
    for _, row in parts:
        if len(row) != t + 1:
            raise ValueError("row of %d coefficients, expected %d" % (len(row), t + 1))
        coeffs += row
    rtab, _ = commitment_rows(ctab, n, t, [(p, x) for p in range(n)])
    ok = base_mul_check(rtab, n * (t + 1), _i32(list(range(n * (t + 1))), dev),
                        _scalars(coeffs, dev, "row coefficient"))
    return _outcomes(ok.cpu().tolist(), t + 1), (rtab, n)


def check_parts(t, our_idx, parts, device=0):
    """`handle_part_or_fault`'s check (sync_key_gen.rs:557, :569) for parts =
    [(BivarCommitment: commitment_len(t) compressed points in coeff_pos order,
    our decrypted row: t + 1 coefficients of 32 bytes, constant term first)].
    Per part: commit.row(our_idx + 1), then [row_j] G1::one() against its
    coefficient j for every j.  Returns (outcomes, row_tables): per part True,
    False (PartFault::RowCommitment) or None (a commitment point that does not
    decode, or a coefficient >= r: the message does not deserialise);
    row_tables, the rows' commitments on the device, is what check_acks takes."""
    x = _x_of(our_idx)
    if not parts:
        return [], (None, 0)
    _need_gpu()
    dev = "cuda:%d" % device
    return _check_parts(t, x, parts, _prepare_parts(t, parts, dev), dev)


def _ack_checks(t, row_tables, acks, dev, stream=None):
    """Device work of check_acks: the outcome tensor of the acks.  The lanes
    run in the order of the senders, so a wave shares its evaluation point (or
    a few neighbours) and pays the doublings and additions of that point's
    bits only; the outcomes come back in the order of `acks`."""
    rtab, n = row_tables
    count = len(acks)
    order = sorted(range(count), key=lambda k: acks[k][1])
    back = [0] * count
    for r, k in enumerate(order):
        back[k] = r
    vtab, _, _, _ = poly_eval_prepared(
        rtab, n * (t + 1), _i32(list(range(n * (t + 1))), dev), _offsets([t + 1] * n, dev),
        _i32([acks[k][0] for k in order], dev),
        _u32_tensor([_x_of(acks[k][1]) for k in order], dev), encode=False, stream=stream)
    ok = base_mul_check(vtab, count, _i32(list(range(count)), dev),
                        _scalars([acks[k][2] for k in order], dev, "ack value"), stream=stream)
    return ok[_i32(back, dev).long()]


def check_acks(t, row_tables, acks, device=0):
    """`handle_ack_or_fault`'s check (sync_key_gen.rs:603) for acks = [(part,
    sender_idx, our decrypted value: 32 bytes)] against the row_tables of
    check_parts: commit.evaluate(our_idx + 1, sender_idx + 1) is the part's row
    commitment evaluated at sender_idx + 1, compared with [val] G1::one().
    Returns per ack True, False (AckFault::ValueCommitment) or None (val >= r,
    a part outside the tables or one whose commitment did not decode)."""
    for _, s, _ in acks:
        _x_of(s)
    if not acks:
        return []
    _need_gpu()
    if row_tables[0] is None:
        return [None] * len(acks)
    ok = _ack_checks(t, row_tables, acks, "cuda:%d" % device).cpu().tolist()
    return [None if v == CHECK_INVALID else v == CHECK_OK for v in ok]


def _generate(t, ctab, commits, complete, dev):
    """The key set commitment as a device table of t + 1 points."""
    m = commitment_len(t)
    rows = [c * m + coeff_pos(0, j) for j in range(t + 1) for c in complete]
    return poly_eval_prepared(ctab, commits * m, _i32(rows, dev),
                              _offsets([len(complete)] * (t + 1), dev),
                              _i32(list(range(t + 1)), dev), _u32_tensor([1] * (t + 1), dev))


def generate_public(t, complete_commitments, device=0):
    """The `PublicKeySet` of `generate` (sync_key_gen.rs:516-534): coefficient
    j of its commitment is the sum of the entries (0, j) -- `commit.row(0)` --
    over the complete parts' commitments (each commitment_len(t) compressed
    points), one evaluation at x = 1 over that list.  Returns t + 1 pairs (96
    bytes, 48 bytes), constant term (the public key) first; None in place of a
    coefficient that meets a point that does not decode."""
    _need_gpu()
    if not complete_commitments:   # Poly::zero().commitment()
        return [(b"\x40" + b"\0" * 95, b"\xc0" + b"\0" * 47)] * (t + 1)
    dev = "cuda:%d" % device
    n = len(complete_commitments)
    ctab = _prepare_parts(t, [(c, None) for c in complete_commitments], dev)
    _, o96, o48, st = _generate(t, ctab, n, list(range(n)), dev)
    return _encodings(o96, o48, st)


def sync_key_gen_grouped(t, our_idx, parts, acks, n=None, device=0):
    """One node's whole `SyncKeyGen` in one call: parts as for check_parts (part
    p comes from proposer p), acks as for check_acks, `n` validators (default:
    one per part).  The commitments are decoded once; rows, values, the key set
    and the key shares are computed from tables that stay on the device.
    Returns (part outcomes, ack outcomes, complete, key_set, key_shares):
    `complete` the parts with Acks from more than 2t distinct senders, valid or
    not (`is_complete`, :342-344; the crate counts an Ack before it checks it,
    :588); key_set the t + 1 pairs of generate_public over those parts;
    key_shares what public_key_shares returns for that key set and n."""
    x = _x_of(our_idx)
    for _, s, _ in acks:
        _x_of(s)
    n = len(parts) if n is None else n
    if not parts or n <= 0:
        raise ValueError("no parts")
    _need_gpu()
    dev = "cuda:%d" % device
    ctab = _prepare_parts(t, parts, dev)
    part_ok, row_tables = _check_parts(t, x, parts, ctab, dev)
    ack_ok = []
    if acks:
        okh = _ack_checks(t, row_tables, acks, dev).cpu().tolist()
        ack_ok = [None if v == CHECK_INVALID else v == CHECK_OK for v in okh]
    senders = [set() for _ in parts]
    for p, s, _ in acks:
        if 0 <= p < len(parts):
            senders[p].add(s)
    complete = [p for p, s in enumerate(senders) if len(s) > 2 * t]
    ktab, o96, o48, st = _generate(t, ctab, len(parts), complete, dev)
    (stab, s96, s48, sst), pk = _key_shares(ktab, t + 1, n, dev)
    return part_ok, ack_ok, complete, _encodings(o96, o48, st), (stab, s96, s48, sst, pk)


# ---- the sending side: the dealer's Part, the Acks, the secret key share ----
def _bivar_rows(t, dpolys, nparts, n, dev):
    """`BivarPoly::row(node + 1)` of `nparts` polynomials (dpolys uint8 [nparts
    * commitment_len(t), 32]) for node < n: coefficient j of a row is the
    polynomial over the entries (0..t, j), as commitment_rows builds it in G1.
    Returns (uint8 [nparts * n * (t + 1), 32], part-major then node; status)."""
    m = commitment_len(t)
    rows = [p * m + coeff_pos(i, j) for p in range(nparts) for j in range(t + 1)
            for i in range(t + 1)]
    poly = [p * (t + 1) + j for p in range(nparts) for _ in range(n) for j in range(t + 1)]
    xs = [node + 1 for _ in range(nparts) for node in range(n) for _ in range(t + 1)]
    return fr_poly_eval(dpolys, _i32(rows, dev), _offsets([t + 1] * (nparts * (t + 1)), dev),
                        _i32(poly, dev), _u32_tensor(xs, dev))


def _row_values(t, drows, nrows, n, dev):
    """`row.evaluate(idx + 1)` for idx < n of `nrows` rows of t + 1 scalars laid
    end to end.  Returns (uint8 [nrows * n, 32], row-major; status)."""
    poly = [r for r in range(nrows) for _ in range(n)]
    xs = [idx + 1 for _ in range(nrows) for idx in range(n)]
    return fr_poly_eval(drows, _i32(list(range(nrows * (t + 1))), dev),
                        _offsets([t + 1] * nrows, dev), _i32(poly, dev), _u32_tensor(xs, dev))


def _scalar_list(dev_scalars):
    return [bytes(v) for v in dev_scalars.cpu().numpy()]


def _all_ok(st, what):
    if int(st.max()) != EVAL_OK:
        raise ValueError("%s: a scalar is not below r" % what)


def generate_part(t, poly, n, device=0):
    """The dealer's half of a `Part` (sync_key_gen.rs:413-417): poly = the
    commitment_len(t) coefficients of a symmetric `BivarPoly` of degree t in
    coeff_pos order, 32 bytes each (`BivarPoly::random` stays with the caller,
    like the encryption of the rows).  Returns (`our_part.commitment()` as
    commitment_len(t) compressed points, `our_part.row(i + 1)` for i < n as n
    lists of t + 1 scalars).  A coefficient >= r raises ValueError."""
    if len(poly) != commitment_len(t):
        raise ValueError("polynomial of %d coefficients, expected %d"
                         % (len(poly), commitment_len(t)))
    if not 0 < n < 0xFFFFFFFF:
        raise ValueError("n = %r nodes" % (n,))
    dev = "cuda:%d" % device
    _need_gpu()
    dpoly = _scalars(poly, dev, "coefficient")
    _, _, c48, cst = base_mul(dpoly)
    rows, rst = _bivar_rows(t, dpoly, 1, n, dev)
    _all_ok(rst, "generate_part")
    flat = _scalar_list(rows)
    return ([bytes(v) for v in c48.cpu().numpy()],
            [flat[i * (t + 1):(i + 1) * (t + 1)] for i in range(n)])


def ack_values(row, n, device=0):
    """The values of an `Ack` (sync_key_gen.rs:459): `row.evaluate(idx + 1)` for
    idx < n of our decrypted row (scalars of 32 bytes, constant term first), to
    be encrypted to node idx by the caller.  Returns n scalars."""
    if not row:
        raise ValueError("empty row")
    if not 0 < n < 0xFFFFFFFF:
        raise ValueError("n = %r nodes" % (n,))
    dev = "cuda:%d" % device
    _need_gpu()
    vals, st = _row_values(len(row) - 1, _scalars(row, dev, "row coefficient"), 1, n, dev)
    _all_ok(st, "ack_values")
    return _scalar_list(vals)


def _take(t, pairs):
    """The first t + 1 (sender_idx, value) of a part in ascending sender, a
    sender counting once: `part.values.iter().take(threshold + 1)` (:523) over
    the BTreeMap that :606 fills (a repeated Ack returns at :588-590)."""
    seen = {}
    for s, v in pairs:
        _x_of(s)
        seen.setdefault(s, v)
    return sorted(seen.items())[:t + 1]


def _secret_key_shares(t, nodes, dev):
    """sum over a node's parts of the interpolation at 0 of the part's pairs,
    for every node of `nodes` = [values_by_part]: one Lagrange group per (node,
    part), one dot product per node over all of its terms."""
    from .threshold import lagrange_coeffs
    idx, vals, lag, dot = [], [], [], []
    for parts in nodes:
        for pairs in parts:
            pick = _take(t, pairs)
            idx += [s for s, _ in pick]
            vals += [v for _, v in pick]
            lag.append(len(pick))
        dot.append(len(idx) - sum(dot))
    coeffs, _ = lagrange_coeffs(_u32_tensor(idx, dev), _offsets(lag, dev))
    out, st = fr_dot(coeffs, _scalars(vals, dev, "value"), _offsets(dot, dev))
    _all_ok(st, "secret_key_share")
    return _scalar_list(out)


def secret_key_share(t, values_by_part, device=0):
    """The secret half of `generate` (sync_key_gen.rs:516-534): values_by_part
    holds, per complete part, the (sender_idx, value) pairs that passed
    handle_ack.  Per part the pairs are sorted by sender and the first t + 1
    interpolated at 0 (x = sender_idx + 1; with fewer pairs what there is, as
    the crate does), and the results summed: sk_i, 32 bytes.  No part gives
    zero (`Fr::zero()`)."""
    _need_gpu()
    return _secret_key_shares(t, [values_by_part], "cuda:%d" % device)[0]


def sync_key_gen_network(t, polys, device=0, ack_senders=None):
    """An honest run of `SyncKeyGen` among N = len(polys) nodes hosted in one
    process, from given polynomials (polys[p]: node p's `BivarPoly`, as for
    generate_part): every commitment, row and Ack value is produced on the
    device, every node checks every Part and every Ack through the checks of
    check_parts / check_acks, and `generate` runs for every node.
    ack_senders[p] lists the nodes whose Acks of part p are handled (default:
    all N); a part is complete with more than 2t distinct ones.  Returns a
    dict: commitments [p][k] 48 bytes, rows [p][node][j] and values
    [p][sender][node] 32 bytes, part_ok [node][p] and ack_ok [node] (one
    outcome per (p, sender) of ack_senders, in that order), complete, key_set
    (generate_public's pairs), key_shares (public_key_shares' tuple: the pk_i
    table first), secret_key_shares [node] 32 bytes."""
    n = len(polys)
    m = commitment_len(t)
    if n == 0:
        raise ValueError("no nodes")
    for f in polys:
        if len(f) != m:
            raise ValueError("polynomial of %d coefficients, expected %d" % (len(f), m))
    if ack_senders is None:
        ack_senders = [list(range(n))] * n
    if len(ack_senders) != n or any(not 0 <= s < n for a in ack_senders for s in a):
        raise ValueError("ack_senders: one list of node indices per part")
    _need_gpu()
    dev = "cuda:%d" % device
    dpolys = _scalars([c for f in polys for c in f], dev, "coefficient")
    ctab, _, c48, cst = base_mul(dpolys)
    _all_ok(cst, "commitment")
    drows, rst = _bivar_rows(t, dpolys, n, n, dev)
    _all_ok(rst, "rows")
    dvals, vst = _row_values(t, drows, n * n, n, dev)
    _all_ok(vst, "values")
    c48h, rowh, valh = [bytes(v) for v in c48.cpu().numpy()], _scalar_list(drows), _scalar_list(dvals)
    commitments = [c48h[p * m:(p + 1) * m] for p in range(n)]
    rows = [[rowh[(p * n + i) * (t + 1):(p * n + i + 1) * (t + 1)] for i in range(n)]
            for p in range(n)]
    values = [[valh[(p * n + s) * n:(p * n + s + 1) * n] for s in range(n)] for p in range(n)]
    part_ok, ack_ok = [], []
    for i in range(n):
        ok, row_tables = _check_parts(t, i + 1, [(None, rows[p][i]) for p in range(n)], ctab, dev)
        part_ok.append(ok)
        acks = [(p, s, values[p][s][i]) for p in range(n) for s in ack_senders[p]]
        okh = _ack_checks(t, row_tables, acks, dev).cpu().tolist() if acks else []
        ack_ok.append([None if v == CHECK_INVALID else v == CHECK_OK for v in okh])
    complete = [p for p in range(n) if len(set(ack_senders[p])) > 2 * t]
    ktab, o96, o48, st = _generate(t, ctab, n, complete, dev)
    (stab, s96, s48, sst), pk = _key_shares(ktab, t + 1, n, dev)
    sks = _secret_key_shares(
        t, [[[(s, values[p][s][i]) for s in ack_senders[p]] for p in complete] for i in range(n)],
        dev)
    return {"commitments": commitments, "rows": rows, "values": values, "part_ok": part_ok,
            "ack_ok": ack_ok, "complete": complete, "key_set": _encodings(o96, o48, st),
            "key_shares": (stab, s96, s48, sst, pk), "secret_key_shares": sks}
