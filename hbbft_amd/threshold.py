"""Threshold-decrypt share verification on the MI355X.

hbbft's `ThresholdDecrypt` (/root/reference/src/threshold_decrypt.rs) checks
every ciphertext once (`ct.verify()`, line 142) and every received decryption
share (`pk.verify_decryption_share(share, ct)`, lines 220-228), both from
`threshold_crypto` (rev 624eeee):

    Ciphertext::verify                      e(G1::one(), W) == e(U, H)
    PublicKeyShare::verify_decryption_share e(share, H)     == e(pk_i, W)

with H = hash_g1_g2(U, V), a G2 point computed once per ciphertext (SHA3-256
and a ChaCha-seeded G2 sample: `hash_g1_g2` below runs it on the device; the
check functions take H as a point from whoever computed it).  In an epoch every node verifies N shares of each of N
ciphertexts, so the pairing checks come in batches of N^2 per node; this
module runs them through `hbrbc_pairing_check_batch` (hbbft_amd/csrc/
pairing.hip): one Miller loop per lane, one final exponentiation per check.

Once more than `num_faulty` valid shares are in, `try_output` (lines 232-252)
calls `public_key_set().decrypt(shares, &ct)`: the Lagrange interpolation at 0
of the shares in G1, g = sum lambda_i share_i, followed by xor_with_hash(g, V).
`decrypt_combine_prepared` computes g for batches of ciphertexts from the same
prepared table the checks read, so the verified shares never leave the device;
`decrypt_shares_grouped` is the two steps in one call.  `xor_with_hash` turns
g into the plaintext; it hashes the compressed encoding of g, which comes back
beside the uncompressed one.  `decrypt_ciphertexts_grouped` is the whole of it
from wire ciphertexts (U, V, W) to plaintexts, and `encrypt_batch` is
`PublicKey::encrypt` with given scalars.

`ThresholdSign` (threshold_sign.rs), the common coin of `BinaryAgreement`, is
the third consumer: every received signature share goes through
`pk_i.verify_g2(share, hash)` (lines 216-225),

    PublicKeyShare::verify_g2               e(pk_i, H) == e(G1::one(), share_i)

and `combine_and_verify_sig` (lines 249-270) interpolates t + 1 valid shares
at 0 in G2 and checks the result against the master public key; the coin is
the signature's parity.  `sig_check_prepared` and `sig_combine_prepared` are
the two steps on device tables, `threshold_sign_grouped` the whole for many
coins.  H arrives as a G2 point; `hash_g2` below computes hash_g2(doc) on the
device.

The three byte <-> group functions (`hash_g2`, `hash_g1_g2`, `xor_with_hash`;
hbbft_amd/csrc/hash_g2.hip) follow the definition written out in that file and
in tests/hash_ref.py.  `threshold_crypto` itself is not available to this
project, so their byte parity with the crate is not pinned, and
one deviation is stated: a hash whose product with the cofactor is the point at
infinity (probability about 2^-255) raises here, where the crate draws again.

Points are the crate's uncompressed encodings (G1: 96 bytes, G2: 192 bytes,
big-endian; see include/hbrbc.h) or, as hbbft's messages carry them, the
compressed ones (48 / 96 bytes): `g1_prepare_compressed` and
`g2_points_prepare_compressed` build the same tables from those,
`g1_decompress` / `g2_decompress` turn them into the uncompressed form, and
`decrypt_shares_grouped_wire` / `threshold_sign_grouped_wire` are the grouped
functions with every received point in wire form.

The sending side is here too, for a simulator or test network that hosts all
N nodes: `create_decryption_shares` (`decrypt_share_no_verify`, line 161:
[sk_i] U) and `create_signature_shares` (`sign_g2`, threshold_sign.rs:167:
[sk_i] H) make the N C shares of C ciphertexts or documents in one launch of
`g1_mul_prepared` / `g2_mul_prepared`, straight into the tables the checks and
the combines read; the secret key shares come from hbbft_amd/keygen.py.  These
multiplications branch on scalar bits and are not constant-time.

There is no CPU fallback: without the library or a GPU the calls raise
`HbrbcUnavailable`.
"""
import ctypes

from . import HbrbcUnavailable, RseError, _check, lib  # noqa: F401

G1_BYTES = 96
G2_BYTES = 192
GT_BYTES = 576

# G1::one() (the standard generator), uncompressed: the `a` of Ciphertext::verify.
G1_ONE = bytes.fromhex(
    "17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
    "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1")

CHECK_OK, CHECK_FAIL, CHECK_INVALID = 1, 0, 2

G1_COMPRESSED_BYTES = 48
G2_COMPRESSED_BYTES = 96
FR_BYTES = 32
# per-group status of the combine entries
COMBINE_OK, COMBINE_INFINITY, COMBINE_INVALID, COMBINE_DUPLICATE = 0, 1, 2, 3


def _torch():
    import torch
    return torch


def workspace(pairings, device=0):
    """Device workspace for `pairings` Miller loops (reusable across calls)."""
    torch = _torch()
    n = lib().hbrbc_pairing_workspace_size(pairings)
    return torch.empty(max(n, 1), dtype=torch.uint8, device="cuda:%d" % device)


def _stream(dev, stream):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    return ctypes.c_void_p(s.cuda_stream)


def pairing_batch(g1, g2, ws=None, stream=None):
    """`PEngine::pairing(g1[i], g2[i])` for every row: g1 uint8 [n, 96], g2 uint8
    [n, 192] on one device.  Returns (gt uint8 [n, 576], status uint8 [n];
    0 ok, 2 invalid point)."""
    torch = _torch()
    n = g1.shape[0]
    assert g1.shape == (n, G1_BYTES) and g2.shape == (n, G2_BYTES), (g1.shape, g2.shape)
    assert g1.is_contiguous() and g2.is_contiguous() and g1.device == g2.device
    gt = torch.empty((n, GT_BYTES), dtype=torch.uint8, device=g1.device)
    st = torch.empty((n,), dtype=torch.uint8, device=g1.device)
    if ws is None:
        ws = workspace(n, g1.device.index)
    assert ws.numel() >= lib().hbrbc_pairing_workspace_size(n)
    _check(lib().hbrbc_pairing_batch(g1.data_ptr(), g2.data_ptr(), n, gt.data_ptr(),
                                     st.data_ptr(), ws.data_ptr(), _stream(g1.device, stream)))
    return gt, st


def pairing_check_batch(g1, g2, ws=None, stream=None):
    """count checks e(a_i, b_i) == e(c_i, d_i): g1 uint8 [2 count, 96] = a_0,
    c_0, a_1, c_1, ...; g2 uint8 [2 count, 192] = b_0, d_0, ....  Returns
    uint8 [count]: 1 equal, 0 not, 2 invalid point."""
    torch = _torch()
    n2 = g1.shape[0]
    assert n2 % 2 == 0 and g1.shape == (n2, G1_BYTES) and g2.shape == (n2, G2_BYTES)
    assert g1.is_contiguous() and g2.is_contiguous() and g1.device == g2.device
    ok = torch.empty((n2 // 2,), dtype=torch.uint8, device=g1.device)
    if ws is None:
        ws = workspace(n2, g1.device.index)
    assert ws.numel() >= lib().hbrbc_pairing_workspace_size(n2)
    _check(lib().hbrbc_pairing_check_batch(g1.data_ptr(), g2.data_ptr(), n2 // 2, ok.data_ptr(),
                                           ws.data_ptr(), _stream(g1.device, stream)))
    return ok


def _table_sized(tab, size):
    """A prepared table must hold exactly `size` bytes: the entries find its
    status bytes at an offset that depends on the count it was prepared with.
    (The preparations allocate one byte for a table of no points.)"""
    return tab.numel() == size or (size == 0 and tab.numel() == 1)


def g2_prepare(g2, stream=None):
    """Prepare G2 points (uint8 [n, 192]) once: the Miller-loop lines every
    check against them reuses (the crate's G2Prepared).  Returns the device
    table (uint8) for pairing_check_prepared."""
    torch = _torch()
    n = g2.shape[0]
    assert g2.shape == (n, G2_BYTES) and g2.is_contiguous()
    prep = torch.empty(max(1, lib().hbrbc_g2_prepared_size(n)), dtype=torch.uint8,
                       device=g2.device)
    _check(lib().hbrbc_g2_prepare(g2.data_ptr(), n, prep.data_ptr(), _stream(g2.device, stream)))
    return prep


def pairing_check_prepared(g1, prep, points, idx_b, idx_d, ws=None, stream=None):
    """count checks e(a_i, P[idx_b[i]]) == e(c_i, P[idx_d[i]]) against `points`
    prepared G2 points: g1 uint8 [2 count, 96] = a_0, c_0, ...; idx_* int32
    [count].  Returns uint8 [count]: 1 equal, 0 not, 2 invalid point."""
    torch = _torch()
    n2 = g1.shape[0]
    count = n2 // 2
    assert n2 % 2 == 0 and g1.shape == (n2, G1_BYTES) and g1.is_contiguous()
    assert idx_b.shape == (count,) and idx_d.shape == (count,)
    assert idx_b.dtype == torch.int32 and idx_d.dtype == torch.int32
    assert idx_b.is_contiguous() and idx_d.is_contiguous()
    assert _table_sized(prep, lib().hbrbc_g2_prepared_size(points))
    # an index outside [0, points) makes that check's outcome 2 (invalid) on the device
    ok = torch.empty((count,), dtype=torch.uint8, device=g1.device)
    if ws is None:
        ws = workspace(count, g1.device.index)
    assert ws.numel() >= lib().hbrbc_pairing_workspace_size(count)
    _check(lib().hbrbc_pairing_check_prepared(g1.data_ptr(), prep.data_ptr(), points,
                                              idx_b.data_ptr(), idx_d.data_ptr(), count,
                                              ok.data_ptr(), ws.data_ptr(),
                                              _stream(g1.device, stream)))
    return ok


def g1_prepare(g1, stream=None):
    """Decode and check G1 points (uint8 [n, 96]) once -- hbbft's public key
    shares pk_i, which the crate holds as curve points and does not decode per
    share.  Returns the device table (uint8) for pairing_check_prepared_keys."""
    torch = _torch()
    n = g1.shape[0]
    assert g1.shape == (n, G1_BYTES) and g1.is_contiguous()
    keys = torch.empty(max(1, lib().hbrbc_g1_prepared_size(n)), dtype=torch.uint8,
                       device=g1.device)
    _check(lib().hbrbc_g1_prepare(g1.data_ptr(), n, keys.data_ptr(), _stream(g1.device, stream)))
    return keys


def g1_prepare_compressed(g1c, stream=None):
    """g1_prepare for compressed points (uint8 [n, 48], the wire form of a
    DecryptionShare or a PublicKeyShare): the same table, bit for bit."""
    torch = _torch()
    n = g1c.shape[0]
    assert g1c.shape == (n, G1_COMPRESSED_BYTES) and g1c.is_contiguous()
    keys = torch.empty(max(1, lib().hbrbc_g1_prepared_size(n)), dtype=torch.uint8,
                       device=g1c.device)
    _check(lib().hbrbc_g1_prepare_compressed(g1c.data_ptr(), n, keys.data_ptr(),
                                             _stream(g1c.device, stream)))
    return keys


def g1_decompress(g1c, stream=None):
    """Compressed G1 points (uint8 [n, 48]) to the uncompressed encoding.
    Returns (uint8 [n, 96], status uint8 [n]: 0 ok, 1 infinity, 2 invalid); an
    invalid point gives zero bytes, which every entry rejects."""
    torch = _torch()
    n = g1c.shape[0]
    assert g1c.shape == (n, G1_COMPRESSED_BYTES) and g1c.is_contiguous()
    out = torch.empty((n, G1_BYTES), dtype=torch.uint8, device=g1c.device)
    st = torch.empty((n,), dtype=torch.uint8, device=g1c.device)
    _check(lib().hbrbc_g1_decompress(g1c.data_ptr(), n, out.data_ptr(), st.data_ptr(),
                                     _stream(g1c.device, stream)))
    return out, st


def g2_decompress(g2c, stream=None):
    """Compressed G2 points (uint8 [n, 96]) to the uncompressed encoding.
    Returns (uint8 [n, 192], status uint8 [n]) as g1_decompress."""
    torch = _torch()
    n = g2c.shape[0]
    assert g2c.shape == (n, G2_COMPRESSED_BYTES) and g2c.is_contiguous()
    out = torch.empty((n, G2_BYTES), dtype=torch.uint8, device=g2c.device)
    st = torch.empty((n,), dtype=torch.uint8, device=g2c.device)
    _check(lib().hbrbc_g2_decompress(g2c.data_ptr(), n, out.data_ptr(), st.data_ptr(),
                                     _stream(g2c.device, stream)))
    return out, st


def pairing_check_prepared_keys(shares, keys, key_points, idx_c, prep, points, idx_b, idx_d,
                                ws=None, stream=None):
    """count checks e(a_i, P[idx_b[i]]) == e(K[idx_c[i]], P[idx_d[i]]): shares
    uint8 [count, 96] = a_0, a_1, ...; K = `key_points` prepared G1 keys
    (g1_prepare), P = `points` prepared G2 points (g2_prepare); idx_* int32
    [count].  Returns uint8 [count]: 1 equal, 0 not, 2 invalid point or index."""
    torch = _torch()
    count = shares.shape[0]
    assert shares.shape == (count, G1_BYTES) and shares.is_contiguous()
    for t in (idx_b, idx_c, idx_d):
        assert t.shape == (count,) and t.dtype == torch.int32 and t.is_contiguous()
    assert _table_sized(keys, lib().hbrbc_g1_prepared_size(key_points))
    assert _table_sized(prep, lib().hbrbc_g2_prepared_size(points))
    ok = torch.empty((count,), dtype=torch.uint8, device=shares.device)
    if ws is None:
        ws = workspace(count, shares.device.index)
    assert ws.numel() >= lib().hbrbc_pairing_workspace_size(count)
    _check(lib().hbrbc_pairing_check_prepared_keys(
        shares.data_ptr(), keys.data_ptr(), key_points, idx_c.data_ptr(), prep.data_ptr(), points,
        idx_b.data_ptr(), idx_d.data_ptr(), count, ok.data_ptr(), ws.data_ptr(),
        _stream(shares.device, stream)))
    return ok


def pairing_check_prepared_pts(a_prep, count, keys, key_points, idx_c, prep, points, idx_b, idx_d,
                               ws=None, stream=None):
    """pairing_check_prepared_keys with the shares decoded beforehand:
    a_prep = g1_prepare(shares) over the `count` shares (a_i = entry i), so
    their decoding can run as its own launch (e.g. beside g2_prepare on
    another stream).  Returns uint8 [count] as pairing_check_prepared_keys."""
    torch = _torch()
    for t in (idx_b, idx_c, idx_d):
        assert t.shape == (count,) and t.dtype == torch.int32 and t.is_contiguous()
    assert _table_sized(a_prep, lib().hbrbc_g1_prepared_size(count))
    assert _table_sized(keys, lib().hbrbc_g1_prepared_size(key_points))
    assert _table_sized(prep, lib().hbrbc_g2_prepared_size(points))
    ok = torch.empty((count,), dtype=torch.uint8, device=a_prep.device)
    if ws is None:
        ws = workspace(count, a_prep.device.index)
    assert ws.numel() >= lib().hbrbc_pairing_workspace_size(count)
    _check(lib().hbrbc_pairing_check_prepared_pts(
        a_prep.data_ptr(), keys.data_ptr(), key_points, idx_c.data_ptr(), prep.data_ptr(), points,
        idx_b.data_ptr(), idx_d.data_ptr(), count, ok.data_ptr(), ws.data_ptr(),
        _stream(a_prep.device, stream)))
    return ok


def verify_decryption_shares_grouped(ciphertexts, shares, device=0):
    """`verify_decryption_share` for many shares of a few ciphertexts, as
    ThresholdDecrypt receives them: ciphertexts = [(hash G2, W G2)], shares =
    [(ciphertext index, share G1, pk_share G1)].  Each ciphertext's H and W
    are prepared once, each distinct key share pk_i is decoded and checked
    once (the crate holds the validator set's key shares as points), the
    received shares are decoded in a launch of their own; shares are grouped
    by ciphertext so a wave shares its lines.  Returns bools in the order of
    `shares`."""
    if not shares:
        return []
    okh, order, _ = _verify_grouped(ciphertexts, shares, device)
    out = [False] * len(shares)
    for r, i in enumerate(order):
        out[i] = okh[r] == CHECK_OK
    return out


def _verify_grouped(ciphertexts, shares, device, wire=False, h_rows=None):
    """The work of verify_decryption_shares_grouped: returns (outcomes by
    table row, the input position of each row, the g1_prepare table of the
    shares -- row r holds share order[r]).  `wire`: W, the shares and the key
    shares arrive compressed (H stays a point).  `h_rows` (wire only): the H of
    every ciphertext as a device tensor uint8 [C, 192] in place of the host
    bytes (hash_g1_g2_batch leaves them there)."""
    import numpy as np
    torch = _torch()
    dev = "cuda:%d" % device
    g1_width = G1_COMPRESSED_BYTES if wire else G1_BYTES
    g1_table = g1_prepare_compressed if wire else g1_prepare
    if wire:
        # W decompressed on the device (an invalid one becomes zero bytes,
        # which g2_prepare rejects), then interleaved with H: H_0, W_0, ...
        dw, _ = g2_decompress(_g2_rows([w for _, w in ciphertexts], dev, G2_COMPRESSED_BYTES))
        dh = h_rows if h_rows is not None else _g2_rows([h for h, _ in ciphertexts], dev)
        d2 = torch.stack([dh, dw], dim=1)
        d2 = d2.reshape(2 * len(ciphertexts), G2_BYTES)
    else:
        g2 = np.empty((2 * len(ciphertexts), G2_BYTES), np.uint8)
        for j, (h, w) in enumerate(ciphertexts):
            g2[2 * j] = np.frombuffer(h, np.uint8)
            g2[2 * j + 1] = np.frombuffer(w, np.uint8)
        d2 = torch.from_numpy(g2).to(dev)
    key_ids = {}
    for _, _, pk in shares:
        key_ids.setdefault(bytes(pk), len(key_ids))
    kt = np.stack([np.frombuffer(k, np.uint8) for k in key_ids])
    order = sorted(range(len(shares)), key=lambda i: shares[i][0])
    g1 = np.empty((len(shares), g1_width), np.uint8)
    ib = np.empty(len(shares), np.int32)
    ic = np.empty(len(shares), np.int32)
    for r, i in enumerate(order):
        ct, share, pk = shares[i]
        g1[r] = np.frombuffer(share, np.uint8)
        ib[r] = 2 * ct
        ic[r] = key_ids[bytes(pk)]
    dk, d1 = (torch.from_numpy(x).to(dev) for x in (kt, g1))
    # the three preparations are independent: the G2 points and the key
    # shares are latency-bound chains on few waves, the received shares fill
    # the chip -- each on a stream of its own, the checks wait for all three
    cur = torch.cuda.current_stream(dev)
    sides = [torch.cuda.Stream(dev) for _ in range(3)]
    for s_ in sides:
        s_.wait_stream(cur)
    with torch.cuda.stream(sides[0]):
        prep = g2_prepare(d2)
    with torch.cuda.stream(sides[1]):
        ktab = g1_table(dk)
    with torch.cuda.stream(sides[2]):
        sprep = g1_table(d1)
    for s_ in sides:
        cur.wait_stream(s_)
    for t_, s_ in ((d2, sides[0]), (dk, sides[1]), (d1, sides[2])):
        t_.record_stream(s_)
    for t_ in (prep, ktab, sprep):
        t_.record_stream(cur)
    ok = pairing_check_prepared_pts(sprep, len(shares), ktab, len(key_ids),
                                    torch.from_numpy(ic).to(dev), prep, 2 * len(ciphertexts),
                                    torch.from_numpy(ib).to(dev), torch.from_numpy(ib + 1).to(dev))
    return ok.cpu().tolist(), order, sprep


def _combine_workspace(g2, total_shares, groups, device):
    torch = _torch()
    size = lib().hbrbc_g2_combine_workspace_size if g2 else lib().hbrbc_g1_combine_workspace_size
    return torch.empty(max(size(total_shares, groups), 1), dtype=torch.uint8,
                       device="cuda:%d" % device)


def combine_workspace(total_shares, groups, device=0):
    """Device workspace for combining `total_shares` shares in `groups` groups."""
    return _combine_workspace(False, total_shares, groups, device)


def _ragged(offsets, *per_share):
    """Checks a ragged batch: offsets int32 [groups + 1], a prefix sum ending at
    the length of every per-share tensor (read back once: the C entries size
    their launches by it).  Returns (groups, total)."""
    torch = _torch()
    assert offsets.dtype == torch.int32 and offsets.dim() == 1 and offsets.numel() >= 1
    assert offsets.is_contiguous()
    total = per_share[0].shape[0]
    for t in per_share:
        assert t.shape[0] == total and t.is_contiguous() and t.device == offsets.device
    assert int(offsets[-1]) == total, (int(offsets[-1]), total)
    return offsets.numel() - 1, total


def lagrange_coeffs(idx, offsets, stream=None):
    """Lagrange coefficients at 0 of ragged groups of node indices: idx int32
    [total] (the bits of an unsigned 32-bit index; x = idx + 1), offsets int32
    [groups + 1].  Returns (coeffs uint8 [total, 32], big-endian and canonical;
    status uint8 [groups]: 0 ok, 3 a repeated index)."""
    torch = _torch()
    assert idx.dtype == torch.int32 and idx.dim() == 1
    groups, total = _ragged(offsets, idx)
    coeffs = torch.empty((total, FR_BYTES), dtype=torch.uint8, device=idx.device)
    st = torch.empty((groups,), dtype=torch.uint8, device=idx.device)
    _check(lib().hbrbc_lagrange_coeffs(idx.data_ptr(), offsets.data_ptr(), groups,
                                       coeffs.data_ptr(), st.data_ptr(),
                                       _stream(idx.device, stream)))
    return coeffs, st


def _combine_prepared(g2, lagrange, tab, count, rows, coef, offsets, ws, stream):
    """The body of the four prepared combines, over the G1 table (g1_prepare)
    or, with g2, the G2 table (g2_points_prepare) `tab` of exactly `count`
    points; `coef` is per share: the caller's scalars or, with lagrange, the
    node indices.  Returns (uncompressed, compressed, [parity,] status)."""
    torch = _torch()
    L = lib()
    if g2:
        entry = L.hbrbc_sig_combine_prepared if lagrange else L.hbrbc_g2_lincomb_prepared
    else:
        entry = L.hbrbc_decrypt_combine_prepared if lagrange else L.hbrbc_g1_lincomb_prepared
    table_size, ws_size, width = ((L.hbrbc_g2_points_size, L.hbrbc_g2_combine_workspace_size,
                                   G2_BYTES) if g2 else
                                  (L.hbrbc_g1_prepared_size, L.hbrbc_g1_combine_workspace_size,
                                   G1_BYTES))
    assert tab.numel() == table_size(count)
    assert rows.dtype == torch.int32 and rows.dim() == 1
    if lagrange:
        assert coef.dtype == torch.int32 and coef.dim() == 1
    else:
        assert coef.dtype == torch.uint8 and coef.shape == (rows.shape[0], FR_BYTES)
    groups, total = _ragged(offsets, rows, coef)
    dev = rows.device
    assert tab.device == dev
    # the encodings, G2's parity byte, the status
    outs = [torch.empty(shape, dtype=torch.uint8, device=dev)
            for shape in [(groups, width), (groups, width // 2)] + [(groups,)] * (2 if g2 else 1)]
    if ws is None:
        ws = _combine_workspace(g2, total, groups, dev.index)
    assert ws.numel() >= ws_size(total, groups)
    _check(entry(
        tab.data_ptr(), count, rows.data_ptr(), coef.data_ptr(), offsets.data_ptr(), groups,
        *[o.data_ptr() for o in outs], ws.data_ptr(), _stream(dev, stream)))
    return tuple(outs)


def g1_lincomb_prepared(a_prep, prepared_count, rows, scalars, offsets, ws=None, stream=None):
    """Per group sum_j scalars[j] * T[rows[j]] over T = a_prep, a g1_prepare
    table of exactly `prepared_count` points: rows int32 [total], scalars uint8
    [total, 32] (big-endian, < r), offsets int32 [groups + 1].  Returns (out96
    uint8 [groups, 96], out48 uint8 [groups, 48] compressed, status uint8
    [groups]: 0 ok, 1 infinity, 2 invalid input; failed groups are zero bytes)."""
    return _combine_prepared(False, False, a_prep, prepared_count, rows, scalars, offsets, ws,
                             stream)


def decrypt_combine_prepared(a_prep, prepared_count, rows, idx, offsets, ws=None, stream=None):
    """`PublicKeySet::decrypt` up to g for ragged groups of shares: share j is
    row rows[j] of a_prep (a g1_prepare table of exactly `prepared_count`
    points) and comes from node idx[j]; rows, idx int32 [total], offsets int32
    [groups + 1].  Returns (out96, out48, status) as g1_lincomb_prepared, with
    status 3 for a group that repeats an index."""
    return _combine_prepared(False, True, a_prep, prepared_count, rows, idx, offsets, ws, stream)


def _u32_tensor(values, dev):
    """Unsigned 32-bit values as the int32 tensor the wrappers take."""
    import numpy as np
    return _torch().from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32)).to(dev)


def _combine_results(out96, out48, st):
    o96, o48, sth = out96.cpu().numpy(), out48.cpu().numpy(), st.cpu().tolist()
    return [(bytes(o96[g]), bytes(o48[g])) if s in (COMBINE_OK, COMBINE_INFINITY) else None
            for g, s in enumerate(sth)]


def combine_decryption_shares(groups, device=0):
    """`PublicKeySet::decrypt` up to g for host bytes: groups = [[(node index,
    share G1)]].  Returns per group (g uncompressed 96 bytes, g compressed 48
    bytes), or None for a group with an invalid share or a repeated index."""
    import numpy as np
    torch = _torch()
    lib()
    if not groups:
        return []
    flat = [item for grp in groups for item in grp]
    for _, share in flat:
        if len(share) != G1_BYTES:
            raise ValueError("share of %d bytes, expected %d" % (len(share), G1_BYTES))
    total = len(flat)
    if not torch.cuda.is_available():
        raise HbrbcUnavailable("no HIP device visible")
    dev = "cuda:%d" % device
    g1 = np.empty((total, G1_BYTES), np.uint8)
    for r, (_, share) in enumerate(flat):
        g1[r] = np.frombuffer(share, np.uint8)
    offs = np.zeros(len(groups) + 1, np.int32)
    offs[1:] = np.cumsum([len(grp) for grp in groups])
    tab = g1_prepare(torch.from_numpy(g1).to(dev))
    out = decrypt_combine_prepared(tab, total, torch.arange(total, dtype=torch.int32, device=dev),
                                   _u32_tensor([i for i, _ in flat], dev),
                                   torch.from_numpy(offs).to(dev))
    return _combine_results(*out)


def decrypt_combine(shares):
    """Per-call shim: one group [(node index, share G1)] of host bytes through
    hbrbc_decrypt_combine (one device round trip).  Returns (g96, g48); raises
    RseError(InvalidArgument) on an invalid share or a repeated index."""
    import numpy as np
    for _, share in shares:
        if len(share) != G1_BYTES:
            raise ValueError("share of %d bytes, expected %d" % (len(share), G1_BYTES))
    idx = np.asarray([i for i, _ in shares], dtype=np.uint32)
    o96 = ctypes.create_string_buffer(G1_BYTES)
    o48 = ctypes.create_string_buffer(G1_COMPRESSED_BYTES)
    _check(lib().hbrbc_decrypt_combine(b"".join(bytes(s) for _, s in shares), idx.ctypes.data,
                                       len(shares), o96, o48))
    return o96.raw, o48.raw


def decrypt_shares_grouped(ciphertexts, shares, threshold, device=0):
    """ThresholdDecrypt's share handling for many ciphertexts: ciphertexts =
    [(hash G2, W G2)], shares = [(ciphertext index, node index, share G1,
    pk_share G1)].  The shares are prepared and verified as in
    verify_decryption_shares_grouped; then each ciphertext combines its first
    `threshold + 1` valid shares in ascending node index (the order of
    ThresholdDecrypt's share map; a node counts once) straight from the
    prepared table.  Returns (bools in the order of `shares`, per ciphertext
    (g96, g48) or None with fewer than threshold + 1 valid shares)."""
    return _decrypt_shares(ciphertexts, shares, threshold, device, False)


def decrypt_shares_grouped_wire(ciphertexts, shares, threshold, device=0):
    """decrypt_shares_grouped on messages as they arrive: ciphertexts = [(hash
    G2 uncompressed -- the host computes it as a point --, W G2 compressed, 96
    bytes)], shares = [(ciphertext index, node index, share G1 compressed, 48
    bytes, pk_share G1 compressed, 48 bytes)].  The points are decompressed on
    the device (the square roots, sign choices and order-r checks of
    `into_affine`); a point that does not decode fails its checks.  Returns
    what decrypt_shares_grouped returns."""
    for _, w in ciphertexts:
        if len(w) != G2_COMPRESSED_BYTES:
            raise ValueError("W of %d bytes, expected %d" % (len(w), G2_COMPRESSED_BYTES))
    for _, _, share, pk in shares:
        for x in (share, pk):
            if len(x) != G1_COMPRESSED_BYTES:
                raise ValueError("G1 encoding of %d bytes, expected %d"
                                 % (len(x), G1_COMPRESSED_BYTES))
    _need_gpu()
    return _decrypt_shares(ciphertexts, shares, threshold, device, True)


def _decrypt_shares(ciphertexts, shares, threshold, device, wire, h_rows=None):
    """The body of decrypt_shares_grouped and its wire twin."""
    import numpy as np
    torch = _torch()
    outs = [None] * len(ciphertexts)
    if not shares:
        return [], outs
    okh, order, sprep = _verify_grouped(ciphertexts, [(c, s, pk) for c, _, s, pk in shares],
                                        device, wire, h_rows)
    flags = [False] * len(shares)
    valid = [[] for _ in ciphertexts]   # per ciphertext: (node index, table row)
    for r, i in enumerate(order):
        flags[i] = okh[r] == CHECK_OK
        if flags[i]:
            valid[shares[i][0]].append((shares[i][1], r))
    rows, idx, offs, cts = [], [], [0], []
    for c, cand in enumerate(valid):
        seen, pick = set(), []
        for node, r in sorted(cand):
            if node not in seen:
                seen.add(node)
                pick.append((node, r))
        if len(pick) < threshold + 1:
            continue
        pick = pick[:threshold + 1]
        rows += [r for _, r in pick]
        idx += [node for node, _ in pick]
        offs.append(len(rows))
        cts.append(c)
    if cts:
        dev = "cuda:%d" % device
        out = decrypt_combine_prepared(
            sprep, len(shares), torch.from_numpy(np.asarray(rows, np.int32)).to(dev),
            _u32_tensor(idx, dev), torch.from_numpy(np.asarray(offs, np.int32)).to(dev))
        for c, res in zip(cts, _combine_results(*out)):
            outs[c] = res
    return flags, outs


# ---- threshold signatures: ThresholdSign, the coin of BinaryAgreement ----
def g2_points_prepare(g2, stream=None):
    """Decode and check G2 points (uint8 [n, 192]) once -- the received
    signature shares, which differ per check and so cannot be prepared lines.
    Returns the device table (uint8) for sig_check_prepared and the G2
    combine."""
    torch = _torch()
    n = g2.shape[0]
    assert g2.shape == (n, G2_BYTES) and g2.is_contiguous()
    tab = torch.empty(lib().hbrbc_g2_points_size(n), dtype=torch.uint8, device=g2.device)
    _check(lib().hbrbc_g2_points_prepare(g2.data_ptr(), n, tab.data_ptr(),
                                         _stream(g2.device, stream)))
    return tab


def g2_points_prepare_compressed(g2c, stream=None):
    """g2_points_prepare for compressed points (uint8 [n, 96], the wire form
    of a SignatureShare): the same table, bit for bit."""
    torch = _torch()
    n = g2c.shape[0]
    assert g2c.shape == (n, G2_COMPRESSED_BYTES) and g2c.is_contiguous()
    tab = torch.empty(lib().hbrbc_g2_points_size(n), dtype=torch.uint8, device=g2c.device)
    _check(lib().hbrbc_g2_points_prepare_compressed(g2c.data_ptr(), n, tab.data_ptr(),
                                                    _stream(g2c.device, stream)))
    return tab


def sig_check_prepared(sig_tab, sig_count, keys, key_points, idx_key, prep, points, idx_h,
                       ws=None, stream=None):
    """`PublicKeyShare::verify_g2` for sig_count shares: check i is
    e(K[idx_key[i]], P[idx_h[i]]) == e(G1::one(), S[i]) with S = sig_tab
    (g2_points_prepare over exactly `sig_count` shares), K = `key_points` keys
    (g1_prepare), P = `points` prepared G2 points (g2_prepare: the hashes);
    idx_* int32 [sig_count].  Returns uint8 [sig_count]: 1 equal, 0 not, 2
    invalid point or index."""
    torch = _torch()
    count = sig_count
    for t in (idx_key, idx_h):
        assert t.shape == (count,) and t.dtype == torch.int32 and t.is_contiguous()
    assert sig_tab.numel() == lib().hbrbc_g2_points_size(sig_count)
    assert keys.numel() == lib().hbrbc_g1_prepared_size(key_points)
    assert prep.numel() == lib().hbrbc_g2_prepared_size(points)
    ok = torch.empty((count,), dtype=torch.uint8, device=sig_tab.device)
    if ws is None:
        ws = workspace(count, sig_tab.device.index)
    assert ws.numel() >= lib().hbrbc_pairing_workspace_size(count)
    _check(lib().hbrbc_sig_check_prepared(
        sig_tab.data_ptr(), sig_count, keys.data_ptr(), key_points, idx_key.data_ptr(),
        prep.data_ptr(), points, idx_h.data_ptr(), count, ok.data_ptr(), ws.data_ptr(),
        _stream(sig_tab.device, stream)))
    return ok


def combine_g2_workspace(total_shares, groups, device=0):
    """Device workspace for combining `total_shares` G2 shares in `groups` groups."""
    return _combine_workspace(True, total_shares, groups, device)


def g2_lincomb_prepared(sig_tab, sig_count, rows, scalars, offsets, ws=None, stream=None):
    """Per group sum_j scalars[j] * S[rows[j]] over S = sig_tab, a
    g2_points_prepare table of exactly `sig_count` points: rows int32 [total],
    scalars uint8 [total, 32] (big-endian, < r), offsets int32 [groups + 1].
    Returns (out192 uint8 [groups, 192], out96 uint8 [groups, 96] compressed,
    parity uint8 [groups], status uint8 [groups]: 0 ok, 1 infinity, 2 invalid
    input; failed groups are zero bytes)."""
    return _combine_prepared(True, False, sig_tab, sig_count, rows, scalars, offsets, ws, stream)


def sig_combine_prepared(sig_tab, sig_count, rows, idx, offsets, ws=None, stream=None):
    """`combine_signatures` for ragged groups of shares: share j is row rows[j]
    of sig_tab (a g2_points_prepare table of exactly `sig_count` points) and
    comes from node idx[j]; rows, idx int32 [total], offsets int32 [groups +
    1].  Returns (out192, out96, parity, status) as g2_lincomb_prepared, with
    status 3 for a group that repeats an index."""
    return _combine_prepared(True, True, sig_tab, sig_count, rows, idx, offsets, ws, stream)


def _sig_results(out192, out96, par, st):
    o192, o96 = out192.cpu().numpy(), out96.cpu().numpy()
    parh, sth = par.cpu().tolist(), st.cpu().tolist()
    return [(bytes(o192[g]), bytes(o96[g]), parh[g]) if s in (COMBINE_OK, COMBINE_INFINITY)
            else None for g, s in enumerate(sth)]


def _need_gpu():
    lib()
    if not _torch().cuda.is_available():
        raise HbrbcUnavailable("no HIP device visible")


def _g2_rows(points, dev, width=G2_BYTES):
    import numpy as np
    for p in points:
        if len(p) != width:
            raise ValueError("G2 encoding of %d bytes, expected %d" % (len(p), width))
    a = np.empty((len(points), width), np.uint8)
    for r, p in enumerate(points):
        a[r] = np.frombuffer(p, np.uint8)
    return _torch().from_numpy(a).to(dev)


def _g1_rows(points, dev, width=G1_BYTES):
    import numpy as np
    for p in points:
        if len(p) != width:
            raise ValueError("G1 encoding of %d bytes, expected %d" % (len(p), width))
    a = np.empty((len(points), width), np.uint8)
    for r, p in enumerate(points):
        a[r] = np.frombuffer(p, np.uint8)
    return _torch().from_numpy(a).to(dev)


def _dedup(values):
    """(distinct values in first-seen order, the position of each input)."""
    ids = {}
    pos = [ids.setdefault(bytes(v), len(ids)) for v in values]
    return list(ids), pos


def verify_signature_shares(items, device=0):
    """Batched `PublicKeyShare::verify_g2` (threshold_sign.rs:216-225): items =
    [(share G2, pk_share G1, hash G2)] host bytes.  Each distinct hash and key
    is prepared once.  Returns a list of bools (an invalid point is False)."""
    import numpy as np
    torch = _torch()
    if not items:
        return []
    _need_gpu()
    dev = "cuda:%d" % device
    keys, ik = _dedup([pk for _, pk, _ in items])
    hashes, ih = _dedup([h for _, _, h in items])
    stab = g2_points_prepare(_g2_rows([s for s, _, _ in items], dev))
    ktab = g1_prepare(_g1_rows(keys, dev))
    prep = g2_prepare(_g2_rows(hashes, dev))
    ok = sig_check_prepared(stab, len(items), ktab, len(keys),
                            torch.from_numpy(np.asarray(ik, np.int32)).to(dev), prep, len(hashes),
                            torch.from_numpy(np.asarray(ih, np.int32)).to(dev))
    return [v == CHECK_OK for v in ok.cpu().tolist()]


def combine_signature_shares(groups, device=0):
    """`combine_signatures` for host bytes: groups = [[(node index, share
    G2)]].  Returns per group (signature uncompressed 192 bytes, compressed 96
    bytes, parity 0 / 1), or None for a group with an invalid share or a
    repeated index."""
    import numpy as np
    torch = _torch()
    if not groups:
        return []
    _need_gpu()
    dev = "cuda:%d" % device
    flat = [item for grp in groups for item in grp]
    total = len(flat)
    offs = np.zeros(len(groups) + 1, np.int32)
    offs[1:] = np.cumsum([len(grp) for grp in groups])
    tab = g2_points_prepare(_g2_rows([s for _, s in flat], dev))
    out = sig_combine_prepared(tab, total, torch.arange(total, dtype=torch.int32, device=dev),
                               _u32_tensor([i for i, _ in flat], dev),
                               torch.from_numpy(offs).to(dev))
    return _sig_results(*out)


def sig_combine(shares):
    """Per-call shim: one group [(node index, share G2)] of host bytes through
    hbrbc_sig_combine (one device round trip).  Returns (sig192, sig96,
    parity); raises RseError(InvalidArgument) on an invalid share or a repeated
    index."""
    import numpy as np
    for _, share in shares:
        if len(share) != G2_BYTES:
            raise ValueError("share of %d bytes, expected %d" % (len(share), G2_BYTES))
    idx = np.asarray([i for i, _ in shares], dtype=np.uint32)
    o192 = ctypes.create_string_buffer(G2_BYTES)
    o96 = ctypes.create_string_buffer(G2_COMPRESSED_BYTES)
    par = ctypes.create_string_buffer(1)
    _check(lib().hbrbc_sig_combine(b"".join(bytes(s) for _, s in shares), idx.ctypes.data,
                                   len(shares), o192, o96, par))
    return o192.raw, o96.raw, par.raw[0]


def threshold_sign_grouped(documents, shares, threshold, public_key, device=0):
    """The whole of `ThresholdSign` for many coins: documents = [hash G2],
    shares = [(document index, node index, share G2, pk_share G1)].  Each hash
    and each distinct pk_i is prepared once and the shares are decoded once (on
    side streams); all shares are checked; each document then combines its
    first `threshold + 1` valid shares in ascending node index (the order of
    the BTreeMap in combine_and_verify_sig; a node counts once) straight from
    the share table, and every combined signature is checked against
    `public_key` through the same check kernel.  Returns (bools in the order of
    `shares`, per document (sig192, sig96, parity, verified) or None with fewer
    than threshold + 1 valid shares)."""
    return _threshold_sign(documents, shares, threshold, public_key, device, False)


def threshold_sign_grouped_wire(documents, shares, threshold, public_key, device=0):
    """threshold_sign_grouped on messages as they arrive: documents = [hash G2
    uncompressed -- the host computes it as a point], shares = [(document
    index, node index, share G2 compressed, 96 bytes, pk_share G1 compressed,
    48 bytes)], public_key G1 compressed, 48 bytes.  The points are
    decompressed on the device; a point that does not decode fails its checks.
    Returns what threshold_sign_grouped returns."""
    return _threshold_sign(documents, shares, threshold, public_key, device, True)


def _threshold_sign(documents, shares, threshold, public_key, device, wire):
    """The body of threshold_sign_grouped and its wire twin."""
    import numpy as np
    torch = _torch()
    g1_width = G1_COMPRESSED_BYTES if wire else G1_BYTES
    g2_width = G2_COMPRESSED_BYTES if wire else G2_BYTES
    g1_table = g1_prepare_compressed if wire else g1_prepare
    g2_table = g2_points_prepare_compressed if wire else g2_points_prepare
    if len(public_key) != g1_width:
        raise ValueError("public key of %d bytes, expected %d" % (len(public_key), g1_width))
    _need_gpu()
    outs = [None] * len(documents)
    if not shares:
        return [], outs
    dev = "cuda:%d" % device
    # the public key is key 0 of the table, the validators' keys follow
    keys, ik = _dedup([public_key] + [pk for _, _, _, pk in shares])
    order = sorted(range(len(shares)), key=lambda i: shares[i][0])
    d2 = _g2_rows(documents, dev)
    dk = _g1_rows(keys, dev, g1_width)
    ds = _g2_rows([shares[i][2] for i in order], dev, g2_width)
    ih = np.asarray([shares[i][0] for i in order], np.int32)
    ic = np.asarray([ik[1 + i] for i in order], np.int32)
    # three independent preparations, each on a stream of its own (see
    # _verify_grouped); the checks wait for all three
    cur = torch.cuda.current_stream(dev)
    sides = [torch.cuda.Stream(dev) for _ in range(3)]
    for s_ in sides:
        s_.wait_stream(cur)
    with torch.cuda.stream(sides[0]):
        prep = g2_prepare(d2)
    with torch.cuda.stream(sides[1]):
        ktab = g1_table(dk)
    with torch.cuda.stream(sides[2]):
        stab = g2_table(ds)
    for s_ in sides:
        cur.wait_stream(s_)
    for t_, s_ in ((d2, sides[0]), (dk, sides[1]), (ds, sides[2])):
        t_.record_stream(s_)
    for t_ in (prep, ktab, stab):
        t_.record_stream(cur)
    okh = sig_check_prepared(stab, len(shares), ktab, len(keys), torch.from_numpy(ic).to(dev),
                             prep, len(documents), torch.from_numpy(ih).to(dev)).cpu().tolist()
    flags = [False] * len(shares)
    valid = [[] for _ in documents]   # per document: (node index, table row)
    for r, i in enumerate(order):
        flags[i] = okh[r] == CHECK_OK
        if flags[i]:
            valid[shares[i][0]].append((shares[i][1], r))
    rows, idx, offs, docs = [], [], [0], []
    for d, cand in enumerate(valid):
        seen, pick = set(), []
        for node, r in sorted(cand):
            if node not in seen:
                seen.add(node)
                pick.append((node, r))
        if len(pick) < threshold + 1:
            continue
        pick = pick[:threshold + 1]
        rows += [r for _, r in pick]
        idx += [node for node, _ in pick]
        offs.append(len(rows))
        docs.append(d)
    if docs:
        o192, o96, par, st = sig_combine_prepared(
            stab, len(shares), torch.from_numpy(np.asarray(rows, np.int32)).to(dev),
            _u32_tensor(idx, dev), torch.from_numpy(np.asarray(offs, np.int32)).to(dev))
        # the combined signatures, still on the device, become a share table of
        # their own: e(public_key, H_d) == e(G1::one(), sig_d)
        ctab = g2_points_prepare(o192)
        ver = sig_check_prepared(ctab, len(docs), ktab, len(keys),
                                 torch.zeros(len(docs), dtype=torch.int32, device=dev), prep,
                                 len(documents),
                                 torch.from_numpy(np.asarray(docs, np.int32)).to(dev))
        verh = ver.cpu().tolist()
        for j, (d, res) in enumerate(zip(docs, _sig_results(o192, o96, par, st))):
            if res is not None:
                outs[d] = res + (verh[j] == CHECK_OK,)
    return flags, outs


# ---- share creation: what a node sends ----
def _mul_prepared(g2, tab, table_count, rows, scalars, sidx, encode, stream):
    """The body of g1_mul_prepared and g2_mul_prepared."""
    torch = _torch()
    L = lib()
    entry, table_size, width = ((L.hbrbc_g2_mul_prepared, L.hbrbc_g2_points_size, G2_BYTES) if g2
                                else (L.hbrbc_g1_mul_prepared, L.hbrbc_g1_prepared_size, G1_BYTES))
    assert tab.numel() == table_size(table_count)
    assert rows.dtype == torch.int32 and rows.dim() == 1 and rows.is_contiguous()
    count = rows.shape[0]
    assert scalars.dtype == torch.uint8 and scalars.dim() == 2 and scalars.shape[1] == FR_BYTES
    assert scalars.is_contiguous() and tab.device == rows.device == scalars.device
    nscalars = scalars.shape[0]
    if sidx is None:
        assert nscalars >= count, (nscalars, count)
    else:
        assert sidx.dtype == torch.int32 and sidx.shape == (count,) and sidx.is_contiguous()
        assert sidx.device == rows.device
    _need_gpu()
    dev = rows.device
    out = torch.empty(max(1, table_size(count)), dtype=torch.uint8, device=dev)
    ou = oc = None
    if encode:
        ou = torch.empty((count, width), dtype=torch.uint8, device=dev)
        oc = torch.empty((count, width // 2), dtype=torch.uint8, device=dev)
    st = torch.empty((count,), dtype=torch.uint8, device=dev)
    _check(entry(tab.data_ptr(), table_count, rows.data_ptr(), scalars.data_ptr(), nscalars,
                 sidx.data_ptr() if sidx is not None else None, count, out.data_ptr(),
                 ou.data_ptr() if encode else None, oc.data_ptr() if encode else None,
                 st.data_ptr(), _stream(dev, stream)))
    return out, ou, oc, st


def g1_mul_prepared(a_prep, prepared_count, rows, scalars, sidx=None, encode=True, stream=None):
    """Result j is [scalars[sidx[j]]] T[rows[j]] over T = a_prep, a g1_prepare
    table of exactly `prepared_count` points: rows int32 [count], scalars uint8
    [nscalars, 32] (big-endian, < r), sidx int32 [count] or None (scalar j;
    nscalars >= count).  Returns (table uint8 -- the results as a g1_prepare
    table of `count` points --, out96 uint8 [count, 96], out48 uint8 [count,
    48] (both None without `encode`), status uint8 [count]: 0 ok, 1 infinity, 2
    invalid table entry, row, sidx or scalar).  Not constant-time."""
    return _mul_prepared(False, a_prep, prepared_count, rows, scalars, sidx, encode, stream)


def g2_mul_prepared(tab, table_count, rows, scalars, sidx=None, encode=True, stream=None):
    """g1_mul_prepared in G2: T = tab is a g2_points_prepare table of exactly
    `table_count` points, the results a g2_points_prepare table of `count`
    points with out192 uint8 [count, 192] and out96 uint8 [count, 96]."""
    return _mul_prepared(True, tab, table_count, rows, scalars, sidx, encode, stream)


def share_row(node, item, items):
    """Row of (node i, item c) in the tables of create_decryption_shares and
    create_signature_shares over `items` ciphertexts / documents: i * items +
    c, node-major -- the lanes of a wave share one secret key share."""
    return node * items + item


def _create_shares(g2, secret_shares, points, device):
    import numpy as np
    torch = _torch()
    for s in secret_shares:
        if len(s) != FR_BYTES:
            raise ValueError("secret key share of %d bytes, expected %d" % (len(s), FR_BYTES))
    width = G2_BYTES if g2 else G1_COMPRESSED_BYTES
    for p in points:
        if len(p) != width:
            raise ValueError("point of %d bytes, expected %d" % (len(p), width))
    if not secret_shares or not points:
        raise ValueError("no shares to create")
    _need_gpu()
    dev = "cuda:%d" % device
    n, c = len(secret_shares), len(points)
    if g2:
        tab = g2_points_prepare(_g2_rows(points, dev))
    else:
        tab = g1_prepare_compressed(_g1_rows(points, dev, G1_COMPRESSED_BYTES))
    sk = np.frombuffer(b"".join(bytes(s) for s in secret_shares), np.uint8).reshape(n, FR_BYTES)
    lanes = torch.arange(n * c, dtype=torch.int32, device=dev)
    rows = (lanes % max(c, 1)).contiguous()
    sidx = torch.div(lanes, max(c, 1), rounding_mode="floor").to(torch.int32).contiguous()
    out, ou, oc, st = _mul_prepared(g2, tab, c, rows, torch.from_numpy(sk.copy()).to(dev), sidx,
                                    True, None)
    return out, n * c, ou, oc, st


def create_decryption_shares(secret_shares, us48, device=0):
    """`decrypt_share_no_verify` (threshold_decrypt.rs:161) of every node for
    every ciphertext: secret_shares = the N sk_i (32 bytes each), us48 = the U
    of C ciphertexts (compressed G1, 48 bytes, decoded and checked once).  All
    N C shares [sk_i] U_c come from one launch.  Returns (table, count, out96
    uint8 [N C, 96], out48 uint8 [N C, 48] -- the wire form of a
    DecryptionShare --, status uint8 [N C]): `table` is the g1_prepare table of
    the count = N C shares, the share of (node i, ciphertext c) at row
    share_row(i, c, C) = i C + c, which pairing_check_prepared_pts (a_prep,
    with idx_c = the row's node) and decrypt_combine_prepared read as it is.
    Status 1: a U at infinity or sk_i = 0; 2: a U that does not decode or
    sk_i >= r.  Not constant-time: for simulations and test networks."""
    return _create_shares(False, secret_shares, us48, device)


def create_signature_shares(secret_shares, hashes192, device=0):
    """`sign_g2` (threshold_sign.rs:167) of every node for every document:
    hashes192 = H = hash_g2(doc) of C documents (uncompressed G2, 192 bytes;
    the caller's, decoded and checked once).  Returns (table, count, out192
    uint8 [N C, 192], out96 uint8 [N C, 96] -- the wire form of a
    SignatureShare --, status) as create_decryption_shares: `table` is the
    g2_points_prepare table that sig_check_prepared and sig_combine_prepared
    read, (node i, document c) at row share_row(i, c, C)."""
    return _create_shares(True, secret_shares, hashes192, device)


def pairing_check(a, b, c, d):
    """Per-call shim: e(a, b) == e(c, d) for host byte strings (one device
    round trip).  Raises RseError(InvalidArgument) on an invalid point."""
    for x, n in ((a, G1_BYTES), (b, G2_BYTES), (c, G1_BYTES), (d, G2_BYTES)):
        if len(x) != n:
            raise ValueError("point encoding of %d bytes, expected %d" % (len(x), n))
    res = ctypes.c_int(0)
    _check(lib().hbrbc_pairing_check(bytes(a), bytes(b), bytes(c), bytes(d), ctypes.byref(res)))
    return bool(res.value)


def _pack(items, device):
    """[(a, b, c, d)] host bytes -> (g1 [2n, 96], g2 [2n, 192]) on `device`."""
    import numpy as np
    torch = _torch()
    n = len(items)
    g1 = np.empty((2 * n, G1_BYTES), dtype=np.uint8)
    g2 = np.empty((2 * n, G2_BYTES), dtype=np.uint8)
    for i, (a, b, c, d) in enumerate(items):
        g1[2 * i] = np.frombuffer(a, np.uint8)
        g1[2 * i + 1] = np.frombuffer(c, np.uint8)
        g2[2 * i] = np.frombuffer(b, np.uint8)
        g2[2 * i + 1] = np.frombuffer(d, np.uint8)
    dev = "cuda:%d" % device
    return torch.from_numpy(g1).to(dev), torch.from_numpy(g2).to(dev)


def verify_decryption_shares(items, device=0):
    """Batched `PublicKeyShare::verify_decryption_share` (threshold_decrypt.rs:
    220-228): items = [(share G1, pk_share G1, hash G2, W G2)] host bytes.
    Returns a list of bools (an invalid point is False, as a share that does
    not deserialise never reaches the check)."""
    if not items:
        return []
    g1, g2 = _pack([(s, h, pk, w) for s, pk, h, w in items], device)
    ok = pairing_check_batch(g1, g2).cpu().tolist()
    return [v == CHECK_OK for v in ok]


def verify_ciphertexts(items, device=0):
    """Batched `Ciphertext::verify` (threshold_decrypt.rs:142): items =
    [(U G1, W G2, hash G2)]; e(G1::one(), W) == e(U, hash)."""
    if not items:
        return []
    g1, g2 = _pack([(G1_ONE, w, u, h) for u, w, h in items], device)
    ok = pairing_check_batch(g1, g2).cpu().tolist()
    return [v == CHECK_OK for v in ok]


# ---- hashes and the pad: hash_g2, hash_g1_g2, xor_with_hash ----
HASH_OK, HASH_INVALID, HASH_INFINITY = 0, 2, 3
FAIL_CIPHERTEXT = "invalid ciphertext"
FAIL_SHARES = "too few valid shares"


def _ragged_bytes(items, dev):
    """Host byte strings as (flat uint8 tensor, offsets int32 [n + 1]) on dev."""
    import numpy as np
    torch = _torch()
    offs = np.zeros(len(items) + 1, np.int64)
    offs[1:] = np.cumsum([len(x) for x in items])
    if offs[-1] >= 1 << 31:
        raise ValueError("more than 2^31 - 1 bytes in one batch")
    flat = np.frombuffer(b"".join(bytes(x) for x in items), np.uint8)
    return (torch.from_numpy(flat.copy()).to(dev),
            torch.from_numpy(offs.astype(np.int32)).to(dev))


def _ragged_args(flat, offsets):
    torch = _torch()
    assert flat.dtype == torch.uint8 and flat.dim() == 1 and flat.is_contiguous()
    assert offsets.dtype == torch.int32 and offsets.dim() == 1 and offsets.numel() >= 1
    assert offsets.is_contiguous() and offsets.device == flat.device
    return offsets.numel() - 1, flat.numel()


def hash_g2_batch(msgs, offsets, us48=None, encode=True, words=False, stream=None):
    """hash_g2 of the ragged messages msgs[offsets[i] .. offsets[i + 1]) (msgs
    uint8 [total], offsets int32 [count + 1], one device) or, with us48 uint8
    [count, 48], hash_g1_g2(U_i, message i).  Returns (table -- the hashes as a
    g2_points_prepare table of `count` points, which g2_mul_prepared and
    sig_check_prepared read --, out192 uint8 [count, 192], out96 uint8 [count,
    96] (both None without `encode`), status uint8 [count]: 0 ok, 2 a range
    that is reversed or ends past the messages, 3 the point at infinity after
    the cofactor, words int32 [count] -- the stream words the sampler drew --
    or None without `words`).  A range is never read outside msgs."""
    torch = _torch()
    count, total = _ragged_args(msgs, offsets)
    dev = msgs.device
    if us48 is not None:
        assert us48.dtype == torch.uint8 and us48.shape == (count, G1_COMPRESSED_BYTES)
        assert us48.is_contiguous() and us48.device == dev
    _need_gpu()
    L = lib()
    tab = torch.empty(max(1, L.hbrbc_g2_points_size(count)), dtype=torch.uint8, device=dev)
    o192 = o96 = wd = None
    if encode:
        o192 = torch.empty((count, G2_BYTES), dtype=torch.uint8, device=dev)
        o96 = torch.empty((count, G2_COMPRESSED_BYTES), dtype=torch.uint8, device=dev)
    if words:
        wd = torch.empty((count,), dtype=torch.int32, device=dev)
    st = torch.empty((count,), dtype=torch.uint8, device=dev)
    tail = (offsets.data_ptr(), count, total, tab.data_ptr(),
            o192.data_ptr() if encode else None, o96.data_ptr() if encode else None,
            st.data_ptr(), wd.data_ptr() if words else None, _stream(dev, stream))
    if us48 is None:
        _check(L.hbrbc_hash_g2_batch(msgs.data_ptr(), *tail))
    else:
        _check(L.hbrbc_hash_g1_g2_batch(us48.data_ptr(), msgs.data_ptr(), *tail))
    return tab, o192, o96, st, wd


def _hash_results(o192, o96, st):
    sth = st.cpu().tolist()
    if any(s != HASH_OK for s in sth):
        # status 3 is the stated deviation: the crate would draw again
        raise ValueError("hash statuses %r (3: the point at infinity after the cofactor)"
                         % sorted(set(sth)))
    a, b = o192.cpu().numpy(), o96.cpu().numpy()
    return [(bytes(a[i]), bytes(b[i])) for i in range(len(sth))]


def hash_g2(docs, device=0):
    """`hash_g2(doc)` for a list of byte strings: [(H uncompressed 192 bytes, H
    compressed 96 bytes)].  For device tensors see hash_g2_batch."""
    if not docs:
        return []
    _need_gpu()
    _, o192, o96, st, _ = hash_g2_batch(*_ragged_bytes(docs, "cuda:%d" % device))
    return _hash_results(o192, o96, st)


def hash_g1_g2(us48, vs, device=0):
    """`hash_g1_g2(U, V)` for lists of compressed U (48 bytes, hashed as they
    are: no point is decoded) and byte strings V: [(H192, H96)]."""
    if len(us48) != len(vs):
        raise ValueError("%d U for %d V" % (len(us48), len(vs)))
    for u in us48:
        if len(u) != G1_COMPRESSED_BYTES:
            raise ValueError("U of %d bytes, expected %d" % (len(u), G1_COMPRESSED_BYTES))
    if not vs:
        return []
    _need_gpu()
    dev = "cuda:%d" % device
    u = _g1_rows(us48, dev, G1_COMPRESSED_BYTES)
    _, o192, o96, st, _ = hash_g2_batch(*_ragged_bytes(vs, dev), us48=u)
    return _hash_results(o192, o96, st)


def xor_with_hash_batch(gs48, data, offsets, out=None, stream=None):
    """`xor_with_hash(g_i, row i)` for ragged rows data[offsets[i] .. offsets[i
    + 1]) (data uint8 [total], offsets int32 [count + 1], ascending) and gs48
    uint8 [count, 48], the compressed encoding of each g.  Returns (out uint8
    [total] -- `out` if given, which may be `data` --, status uint8 [count]: 0
    ok, 2 a range that is reversed or ends past the data, left untouched).
    Its own inverse; one lane per 16 bytes of a row."""
    torch = _torch()
    count, total = _ragged_args(data, offsets)
    dev = data.device
    assert gs48.dtype == torch.uint8 and gs48.shape == (count, G1_COMPRESSED_BYTES)
    assert gs48.is_contiguous() and gs48.device == dev
    if out is None:
        out = torch.empty_like(data)
    assert out.dtype == torch.uint8 and out.shape == data.shape and out.is_contiguous()
    assert out.device == dev
    _need_gpu()
    L = lib()
    ws = torch.empty(max(1, L.hbrbc_xor_with_hash_workspace_size(count)), dtype=torch.uint8,
                     device=dev)
    st = torch.empty((count,), dtype=torch.uint8, device=dev)
    _check(L.hbrbc_xor_with_hash_batch(gs48.data_ptr(), data.data_ptr(), offsets.data_ptr(),
                                       count, total, out.data_ptr(), st.data_ptr(),
                                       ws.data_ptr(), _stream(dev, stream)))
    return out, st


def _split(flat, items):
    raw, out, pos = bytes(flat.cpu().numpy()), [], 0
    for x in items:
        out.append(raw[pos:pos + len(x)])
        pos += len(x)
    return out


def xor_with_hash(gs48, datas, device=0):
    """`xor_with_hash(g, data)` for lists of compressed g (48 bytes) and byte
    strings: the list of padded byte strings."""
    if len(gs48) != len(datas):
        raise ValueError("%d g for %d rows" % (len(gs48), len(datas)))
    if not datas:
        return []
    _need_gpu()
    dev = "cuda:%d" % device
    flat, offs = _ragged_bytes(datas, dev)
    out, _ = xor_with_hash_batch(_g1_rows(gs48, dev, G1_COMPRESSED_BYTES), flat, offs)
    return _split(out, datas)


def _scalar_rows(scalars, dev):
    import numpy as np
    a = np.frombuffer(b"".join(bytes(s) for s in scalars), np.uint8).reshape(-1, FR_BYTES)
    return _torch().from_numpy(a.copy()).to(dev)


def encrypt_batch(pk, messages, r_scalars, device=0):
    """`PublicKey::encrypt(msg)` with the scalar r given (the crate draws it):
    pk = the public key, compressed G1 (48 bytes); r_scalars = one 32-byte
    big-endian scalar in [1, r) per message.  U = [r] G1::one(), V =
    xor_with_hash([r] pk, msg), W = [r] hash_g1_g2(U, V): five launches for the
    batch, and neither [r] pk nor H leaves the device.  Returns [(U compressed
    48 bytes, V, W compressed 96 bytes)] -- a Ciphertext's fields in wire form.
    Raises ValueError on a pk that does not decode or a scalar that is zero or
    >= r.  Not constant-time: for simulations and test networks."""
    torch = _torch()
    if len(pk) != G1_COMPRESSED_BYTES:
        raise ValueError("public key of %d bytes, expected %d" % (len(pk), G1_COMPRESSED_BYTES))
    if len(messages) != len(r_scalars):
        raise ValueError("%d scalars for %d messages" % (len(r_scalars), len(messages)))
    for x in r_scalars:
        if len(x) != FR_BYTES:
            raise ValueError("scalar of %d bytes, expected %d" % (len(x), FR_BYTES))
    if not messages:
        return []
    _need_gpu()
    dev = "cuda:%d" % device
    n = len(messages)
    r = _scalar_rows(r_scalars, dev)
    L = lib()
    # U = [r] G1::one()
    utab = torch.empty(max(1, L.hbrbc_g1_prepared_size(n)), dtype=torch.uint8, device=dev)
    u48 = torch.empty((n, G1_COMPRESSED_BYTES), dtype=torch.uint8, device=dev)
    ust = torch.empty((n,), dtype=torch.uint8, device=dev)
    _check(L.hbrbc_g1_base_mul(r.data_ptr(), n, utab.data_ptr(), None, u48.data_ptr(),
                               ust.data_ptr(), _stream(torch.device(dev), None)))
    # g = [r] pk, compressed: the pad's key
    pktab = g1_prepare_compressed(_g1_rows([pk], dev, G1_COMPRESSED_BYTES))
    zeros = torch.zeros((n,), dtype=torch.int32, device=dev)
    _, _, g48, gst = g1_mul_prepared(pktab, 1, zeros, r)
    flat, offs = _ragged_bytes(messages, dev)
    v, _ = xor_with_hash_batch(g48, flat, offs)
    # W = [r] hash_g1_g2(U, V), H read from its table
    htab, _, _, hst, _ = hash_g2_batch(v, offs, us48=u48, encode=False)
    _, _, w96, wst = g2_mul_prepared(htab, n, torch.arange(n, dtype=torch.int32, device=dev), r)
    for what, st in (("U", ust), ("[r] pk", gst), ("H", hst), ("W", wst)):
        bad = sorted(set(st.cpu().tolist()) - {0})
        if bad:
            raise ValueError("encrypt: %s has statuses %r" % (what, bad))
    uh, wh = u48.cpu().numpy(), w96.cpu().numpy()
    return [(bytes(uh[i]), vi, bytes(wh[i])) for i, vi in enumerate(_split(v, messages))]


def decrypt_ciphertexts_grouped(ciphertexts, shares, threshold, device=0):
    """ThresholdDecrypt from wire ciphertexts to plaintexts: ciphertexts = [(U
    compressed 48 bytes, V, W compressed 96 bytes)], shares = [(ciphertext
    index, node index, share G1 compressed, pk_share G1 compressed)].  H =
    hash_g1_g2(U, V) is computed on the device and stays there;
    `Ciphertext::verify` is checked with it; the shares are verified and
    combined as in decrypt_shares_grouped_wire; xor_with_hash(g, V) gives the
    plaintext.  Returns (bools in the order of `shares`, per ciphertext the
    plaintext bytes, or FAIL_CIPHERTEXT for one that fails its own check, or
    FAIL_SHARES with fewer than threshold + 1 valid shares)."""
    torch = _torch()
    for u, _, w in ciphertexts:
        if len(u) != G1_COMPRESSED_BYTES or len(w) != G2_COMPRESSED_BYTES:
            raise ValueError("ciphertext with U of %d and W of %d bytes" % (len(u), len(w)))
    if not ciphertexts:
        return [False] * len(shares), []
    _need_gpu()
    dev = "cuda:%d" % device
    u48 = _g1_rows([u for u, _, _ in ciphertexts], dev, G1_COMPRESSED_BYTES)
    vs = [v for _, v, _ in ciphertexts]
    flat, offs = _ragged_bytes(vs, dev)
    _, h192, _, hst, _ = hash_g2_batch(flat, offs, us48=u48)
    if any(s != HASH_OK for s in hst.cpu().tolist()):
        raise ValueError("hash_g1_g2 at infinity after the cofactor")
    # Ciphertext::verify: e(G1::one(), W) == e(U, H), points decompressed here
    n = len(ciphertexts)
    u96, _ = g1_decompress(u48)
    w192, _ = g2_decompress(_g2_rows([w for _, _, w in ciphertexts], dev, G2_COMPRESSED_BYTES))
    one = torch.frombuffer(bytearray(G1_ONE), dtype=torch.uint8).to(dev).expand(n, G1_BYTES)
    g1 = torch.stack([one, u96], dim=1).reshape(2 * n, G1_BYTES).contiguous()
    g2 = torch.stack([w192, h192], dim=1).reshape(2 * n, G2_BYTES).contiguous()
    ct_ok = [c == CHECK_OK for c in pairing_check_batch(g1, g2).cpu().tolist()]
    for _, _, share, pk in shares:
        for x in (share, pk):
            if len(x) != G1_COMPRESSED_BYTES:
                raise ValueError("G1 encoding of %d bytes, expected %d"
                                 % (len(x), G1_COMPRESSED_BYTES))
    flags, gs = _decrypt_shares([(None, w) for _, _, w in ciphertexts], shares, threshold, device,
                                True, h_rows=h192)
    outs = [FAIL_SHARES if ok else FAIL_CIPHERTEXT for ok in ct_ok]
    todo = [c for c in range(n) if ct_ok[c] and gs[c] is not None]
    if todo:
        plain = xor_with_hash([gs[c][1] for c in todo], [vs[c] for c in todo], device)
        for c, m in zip(todo, plain):
            outs[c] = m
    return flags, outs
