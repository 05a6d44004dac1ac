"""CPU-side checks of the prepared-table layout (csrc/pairing_tables.hpp): the
byte sizes of the three table kinds and of the pairing and combine workspaces
are pinned to the values of the library before the layout moved into one
header, and the threshold.py wrappers whose entries place a table's status
bytes by the count passed with it reject a table tensor of any other size
before they look for a device."""
import pytest

import __graft_entry__

COUNTS = (0, 1, 7, 8, 9, 255, 256, 257)
# recorded from the library built at the parent of the commit that added this file
SIZES = {
    "hbrbc_g1_prepared_size": [0, 512, 1024, 1024, 1280, 24832, 24832, 25344],
    "hbrbc_g2_prepared_size": [0, 19968, 137472, 156928, 176640, 4994304, 5013760, 5033728],
    "hbrbc_g2_points_size": [0, 512, 1792, 1792, 2048, 49408, 49408, 49920],
    "hbrbc_pairing_workspace_size": [0, 1024, 4352, 4864, 5632, 147200, 147712, 148736],
}
COMBINE_CASES = ((0, 0), (1, 1), (22, 1), (257, 12))   # (total shares, groups)
COMBINE_SIZES = {
    "hbrbc_g1_combine_workspace_size": [0, 1024, 4608, 46336],
    "hbrbc_g2_combine_workspace_size": [0, 1280, 7680, 83456],
}


@pytest.fixture(scope="module")
def built():
    __graft_entry__.build()


def test_table_and_workspace_sizes_are_pinned(built):
    import hbbft_amd as hb
    L = hb.lib()
    for name, want in SIZES.items():
        assert [getattr(L, name)(c) for c in COUNTS] == want, name
    for name, want in COMBINE_SIZES.items():
        assert [getattr(L, name)(t, g) for t, g in COMBINE_CASES] == want, name


def test_sizes_follow_the_documented_layout(built):
    """Coordinates padded to 256 bytes, then a status byte per point padded to
    256 bytes: 96, 19,584 (68 lines of 72 words) and 192 coordinate bytes a point."""
    import hbbft_amd as hb
    L = hb.lib()

    def pad(x):
        return (x + 255) // 256 * 256

    for name, per_point in (("hbrbc_g1_prepared_size", 96), ("hbrbc_g2_prepared_size", 19584),
                            ("hbrbc_g2_points_size", 192), ("hbrbc_pairing_workspace_size", 576)):
        for c in COUNTS:
            assert getattr(L, name)(c) == pad(c * per_point) + pad(c), (name, c)


class _PastTheChecks(Exception):
    """Raised in place of the stream lookup: every assertion of a wrapper has passed
    and no entry has been called."""


def _stop(*_):
    raise _PastTheChecks()


def test_wrappers_require_the_exact_table_size_before_any_device(built, monkeypatch):
    import torch
    import hbbft_amd as hb
    from hbbft_amd import threshold as T
    L = hb.lib()
    monkeypatch.setattr(T, "_stream", _stop)
    count, key_points, points = 3, 2, 4

    def tab(size, delta=0):
        return torch.zeros(size + delta, dtype=torch.uint8)

    a_size, k_size = L.hbrbc_g1_prepared_size(count), L.hbrbc_g1_prepared_size(key_points)
    p_size, s_size = L.hbrbc_g2_prepared_size(points), L.hbrbc_g2_points_size(count)
    idx = torch.zeros(count, dtype=torch.int32)
    g1 = torch.zeros((2 * count, 96), dtype=torch.uint8)
    shares = torch.zeros((count, 96), dtype=torch.uint8)
    ws = torch.zeros(L.hbrbc_pairing_workspace_size(count), dtype=torch.uint8)

    def prepared(dp=0):
        return T.pairing_check_prepared(g1, tab(p_size, dp), points, idx, idx, ws)

    def prepared_keys(dk=0, dp=0):
        return T.pairing_check_prepared_keys(shares, tab(k_size, dk), key_points, idx,
                                             tab(p_size, dp), points, idx, idx, ws)

    def prepared_pts(da=0, dk=0, dp=0):
        return T.pairing_check_prepared_pts(tab(a_size, da), count, tab(k_size, dk), key_points,
                                            idx, tab(p_size, dp), points, idx, idx, ws)

    def sig(ds=0, dk=0, dp=0):
        return T.sig_check_prepared(tab(s_size, ds), count, tab(k_size, dk), key_points, idx,
                                    tab(p_size, dp), points, idx, ws)

    for call, tables in ((prepared, 1), (prepared_keys, 2), (prepared_pts, 3), (sig, 3)):
        with pytest.raises(_PastTheChecks):   # the exact sizes pass every check
            call()
        for k in range(tables):
            for delta in (1, 256, -1, -256):   # oversized, undersized
                deltas = [0] * tables
                deltas[k] = delta
                with pytest.raises(AssertionError):
                    call(*deltas)
                    pytest.fail("%s%r returned" % (call.__name__, deltas))
    # a table of the next count is as wrong as any other size
    with pytest.raises(AssertionError):
        T.pairing_check_prepared_pts(tab(L.hbrbc_g1_prepared_size(count + 6)), count, tab(k_size),
                                     key_points, idx, tab(p_size), points, idx, idx, ws)
    # the preparations allocate one byte for a table of no points: count 0 takes it
    none = torch.zeros(0, dtype=torch.int32)
    for empty in (tab(0), tab(1)):
        with pytest.raises(_PastTheChecks):
            T.pairing_check_prepared_pts(empty, 0, tab(k_size), key_points, none, tab(p_size),
                                         points, none, none, ws)
    with pytest.raises(AssertionError):
        T.pairing_check_prepared_pts(tab(2), 0, tab(k_size), key_points, none, tab(p_size),
                                     points, none, none, ws)
