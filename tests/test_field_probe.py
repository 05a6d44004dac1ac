"""The BLS12-381 field units of hbbft_amd/csrc/pairing.hip as field arithmetic:
every op of tests/hip/field_probe.hip on the operand classes of
tests/field_ref.py, byte-exact against Python integers.  The classes are the
crafted ones (value list, final subtraction taken, signed lane; proved on the
CPU in tests/test_field_cpu.py) and 4,096 seeded random items per op, as one
launch of 64 full blocks and a ragged one of 4,097."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import field_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# op -> (code, Fp (or Fr) operands in, result elements out, flag words, bytes per element)
OPS = {name: (code, nin, nout, flag, 32 if name.startswith("fr_") else 48)
       for code, (name, nin, nout, flag) in enumerate([
           ("fp_add", 2, 1, 0), ("fp_sub", 2, 1, 0), ("fp_neg", 2, 1, 0), ("fp_dbl", 2, 1, 0),
           ("fp_mul", 2, 1, 0), ("fp_sqr", 2, 1, 0), ("fp_inv", 1, 1, 0),
           ("fp2_mul", 4, 2, 0), ("fp2_sqr", 2, 2, 0), ("fp2_inv", 2, 2, 0), ("fp2_mul_xi", 2, 2, 0),
           ("fp6_mul", 12, 6, 0), ("fp12_mul_inl", 24, 12, 0), ("fp12_mul", 24, 12, 0),
           ("fp12_sqr_inl", 12, 12, 0), ("fp12_sqr", 12, 12, 0), ("fp12_mul_by_014", 18, 12, 0),
           ("fp12_cyclo_sqr", 12, 12, 0), ("fp12_frob1", 12, 12, 0), ("fp12_frob2", 12, 12, 0),
           ("fp12_frob3", 12, 12, 0), ("fp12_inv", 12, 12, 0), ("fp_sqrt", 1, 1, 1),
           ("fp2_sqrt", 2, 2, 1), ("fr_add", 2, 1, 0), ("fr_sub", 2, 1, 0), ("fr_mul", 2, 1, 0),
           ("fr_inv", 1, 1, 0)])}


@functools.lru_cache(None)
def _lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hip", "libfieldprobe.so"))
    lib.hbprobe_run.restype = ctypes.c_int
    lib.hbprobe_run.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_size_t, ctypes.c_void_p]
    return lib


def _pack(items, size):
    """rows of integers -> uint32 words, little-endian limbs, item-major"""
    raw = b"".join(v.to_bytes(size, "little") for row in items for v in row)
    return np.frombuffer(raw, np.uint32).reshape(len(items), -1)


def _run(name, items):
    import torch
    code, nin, nout, flag, size = OPS[name]
    assert items and all(len(row) == nin for row in items)
    src = torch.from_numpy(_pack(items, size).view(np.int32).copy()).to("cuda:0")
    dst = torch.zeros((len(items), nout * size // 4 + flag), dtype=torch.int32, device="cuda:0")
    rc = _lib().hbprobe_run(code, src.data_ptr(), dst.data_ptr(), len(items),
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return dst.cpu().numpy().view(np.uint32)


def _expect(name, rows):
    """reference rows ([elements..., flag?]) -> the words the probe must write"""
    _, _, nout, flag, size = OPS[name]
    out = _pack([row[:nout] for row in rows], size)
    if flag:
        out = np.concatenate([out, np.array([[row[nout]] for row in rows], np.uint32)], axis=1)
    return out


def _compare(name, items, rows, launches=None):
    want = _expect(name, rows)
    for n in launches or [len(items)]:
        got = _run(name, items[:n])
        bad = np.nonzero((got != want[:n]).any(axis=1))[0]
        assert bad.size == 0, "%s: %d of %d items differ, first %d: operands %s" % (
            name, bad.size, n, bad[0], [hex(v) for v in items[bad[0]]])


# ---------------------------------------------------------------- operands
def _pairs(t):
    return [(t[i], t[i + 1]) for i in range(0, len(t), 2)]


def _flat(ps):
    return [v for p in ps for v in p]


@functools.lru_cache(None)
def _value_pairs():
    v = F.fp_values()
    return [(a, b) for a in v for b in v]


@functools.lru_cache(None)
def _random_rows(n_el, seed, modulus=F.P):
    rng = random.Random(seed)
    return [tuple(rng.randrange(modulus) for _ in range(n_el)) for _ in range(4097)]


@functools.lru_cache(None)
def _value_rows(n_el):
    """tower operands drawn from the value list: every value at every coefficient"""
    v = F.fp_values()
    return [tuple(v[(i + 13 * j) % len(v)] for j in range(n_el)) for i in range(len(v))]


RAGGED = [4096, 4097]


def _both(name, n_el, ref, seed):
    """value-list rows in one launch, the random fill in 64 full blocks and 4,097"""
    rows = _value_rows(n_el)
    _compare(name, rows, [ref(r) for r in rows])
    rows = _random_rows(n_el, seed)
    _compare(name, rows, _random_ref(ref, n_el, seed), RAGGED)


@functools.lru_cache(None)
def _random_ref(ref, n_el, seed):
    return [ref(r) for r in _random_rows(n_el, seed)]


# references on flat rows of raw integers
def _r_fp2_mul(r):
    return F.fp2_mul(r[0:2], r[2:4])


def _r_fp6_mul(r):
    return _flat(F.fp6_mul(_pairs(r[:6]), _pairs(r[6:])))


def _r_fp12_mul(r):
    return _flat(F.fp12_mul(_pairs(r[:12]), _pairs(r[12:])))


def _r_fp12_sqr(r):
    return _flat(F.fp12_sqr(_pairs(r)))


def _r_014(r):
    c = _pairs(r[12:])
    return _flat(F.fp12_mul_by_014(_pairs(r[:12]), c[0], c[1], c[2]))


def _r_cyclo(r):
    return _flat(F.fp12_cyclo_sqr(_pairs(r)))


def _r_inv12(r):
    return _flat(F.fp12_inv(_pairs(r)))


def _r_frob(k):
    return {1: _r_frob1, 2: _r_frob2, 3: _r_frob3}[k]


def _r_frob1(r):
    return _flat(F.fp12_frob(_pairs(r), 1))


def _r_frob2(r):
    return _flat(F.fp12_frob(_pairs(r), 2))


def _r_frob3(r):
    return _flat(F.fp12_frob(_pairs(r), 3))


# ---------------------------------------------------------------- the entry
def test_entry_rejects_empty_and_unknown():
    import torch
    buf = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    assert _lib().hbprobe_run(0, buf.data_ptr(), buf.data_ptr(), 0, None) != 0
    assert _lib().hbprobe_run(len(OPS), buf.data_ptr(), buf.data_ptr(), 1, None) != 0
    assert _lib().hbprobe_run(0xFFFFFFFF, buf.data_ptr(), buf.data_ptr(), 1, None) != 0


# ---------------------------------------------------------------- Fp
@pytest.mark.parametrize("name", ["fp_add", "fp_sub", "fp_neg", "fp_dbl", "fp_mul", "fp_sqr"])
def test_fp_binary(name):
    ref = getattr(F, name)
    items = _value_pairs()                                      # class (a): all pairs
    _compare(name, items, [(ref(a, b),) for a, b in items])
    items = _random_rows(2, 0xD0)                               # class (d)
    _compare(name, items, [(ref(a, b),) for a, b in items], RAGGED)


def test_fp_mul_final_subtraction():
    """class (b): fp_mul's value before fp_reduce_once is p + d"""
    items = [(a, b) for a, b, _ in F.final_sub_fp_mul()]
    items += [(b, a) for a, b in items]
    _compare("fp_mul", items, [(F.fp_mul(a, b),) for a, b in items])
    # the same products as the t0 = a0 b0 and t1 = a1 b1 of an Fp2 product
    rows = [(a, 0, b, 0) for a, b in items] + [(0, a, 0, b) for a, b in items] + \
           [(a, a, b, b) for a, b in items]
    _compare("fp2_mul", rows, [_r_fp2_mul(r) for r in rows])


def test_fp_inv_on_values():
    v = F.fp_values()
    _compare("fp_inv", [(a,) for a in v], [(F.fp_inv(a),) for a in v])


def test_fp_sqrt():
    items = [(a,) for a in F.fp_values()] + _random_rows(1, 0xD1)
    _compare("fp_sqrt", items, [F.fp_sqrt(a) for a, in items])
    assert {F.fp_sqrt(a)[1] for a, in items} == {0, 1}


# ---------------------------------------------------------------- Fp2
def test_fp2_sqr_values_and_random():
    items = _value_pairs()                                      # all pairs of (c0, c1)
    _compare("fp2_sqr", items, [F.fp2_sqr(a) for a in items])
    items = _random_rows(2, 0xD2)
    _compare("fp2_sqr", items, [F.fp2_sqr(a) for a in items], RAGGED)


def test_fp2_sqr_final_subtraction():
    """class (b): c1, then c0, reach fp_from29 at p + d"""
    items = [c[:2] for c in F.final_sub_fp2_c1() + F.final_sub_fp2_c0()]
    _compare("fp2_sqr", items, [F.fp2_sqr(a) for a in items])


def test_fp2_sqr_signed_lane():
    """class (c): c0 negative before the reduction (-1 ... -2^329), exactly 0,
    and the operands with the largest columns"""
    items = [c[:2] for c in F.signed_lane_cases()] + F.column_extremes()
    _compare("fp2_sqr", items, [F.fp2_sqr(a) for a in items])


def test_fp2_mul():
    vp = _value_pairs()
    items = [vp[i] + vp[(i * 89 + 17) % len(vp)] for i in range(len(vp))]
    _compare("fp2_mul", items, [_r_fp2_mul(r) for r in items])
    items = _random_rows(4, 0xD3)
    _compare("fp2_mul", items, [_r_fp2_mul(r) for r in items], RAGGED)


def test_fp2_inv_and_mul_xi():
    items = _value_pairs()
    _compare("fp2_inv", items, [F.fp2_inv(a) for a in items])
    _compare("fp2_mul_xi", items, [F.fp2_mul_xi(a) for a in items])
    items = _random_rows(2, 0xD4)
    _compare("fp2_mul_xi", items, [F.fp2_mul_xi(a) for a in items], RAGGED)


def test_fp2_sqrt():
    vp = _value_pairs()
    items = vp[::7] + [(a, 0) for a in F.fp_values()] + _random_rows(2, 0xD5)
    # squares, so that both outcomes are well represented
    items += [F.fp2_sqr(a) for a in _random_rows(2, 0xD6)[:256]]
    rows = [F.fp2_sqrt(a) for a in items]
    _compare("fp2_sqrt", items, [y + (flag,) for y, flag in rows])
    for a, (y, flag) in zip(items, rows):
        assert not flag or F.fp2_sqr(y) == F.fp2_mul(a, (F.mont(1), 0))
    assert sum(flag for _, flag in rows) >= 256 and not all(flag for _, flag in rows)


# ---------------------------------------------------------------- Fp6, Fp12
def test_fp6_mul():
    _both("fp6_mul", 12, _r_fp6_mul, 0xD7)


@pytest.mark.parametrize("name", ["fp12_mul_inl", "fp12_mul"])
def test_fp12_mul(name):
    _both(name, 24, _r_fp12_mul, 0xD8)


@pytest.mark.parametrize("name", ["fp12_sqr_inl", "fp12_sqr"])
def test_fp12_sqr(name):
    _both(name, 12, _r_fp12_sqr, 0xD9)


def test_fp12_mul_by_014():
    _both("fp12_mul_by_014", 18, _r_014, 0xDA)


def test_fp12_cyclo_sqr():
    _both("fp12_cyclo_sqr", 12, _r_cyclo, 0xD9)
    # on the cyclotomic subgroup the formula is the square
    gs = [F.cyclotomic(_pairs(r)) for r in _random_rows(12, 0xD9)[:8]]
    rows = [tuple(_flat(g)) for g in gs]
    want = [_flat(F.fp12_sqr(g)) for g in gs]
    assert want == [_r_cyclo(r) for r in rows]
    _compare("fp12_cyclo_sqr", rows, want)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_fp12_frob(k):
    _both("fp12_frob%d" % k, 12, _r_frob(k), 0xD9)


def test_fp12_inv_on_values():
    rows = _value_rows(12)
    _compare("fp12_inv", rows, [_r_inv12(r) for r in rows])


# ---------------------------------------------------------------- Fr
@pytest.mark.parametrize("name", ["fr_add", "fr_sub", "fr_mul"])
def test_fr_binary(name):
    ref = getattr(F, name)
    v = F.fr_values()
    items = [(a, b) for a in v for b in v]                      # class (e): all pairs
    _compare(name, items, [(ref(a, b),) for a, b in items])
    items = _random_rows(2, 0xE0, F.RORD)
    _compare(name, items, [(ref(a, b),) for a, b in items], RAGGED)


def test_fr_inv_on_values():
    v = F.fr_values()
    _compare("fr_inv", [(a,) for a in v], [(F.fr_inv(a),) for a in v])
