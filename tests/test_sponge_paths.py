"""The SHA3 sponge kernels at the grids that reach each of their forms, and the
proof walk of the validate kernels.

The one-lane 8-byte-load kernels run from 2^18 sponges per launch, the
16-byte-load kernels from 16,384 up to 2^18, the pair-lane kernels below
that; so the shapes here are many instances of short shards.  The shard
lengths put zero to three full 136-byte blocks in front of an empty and a
non-empty last block; the tamperings hit every level of the walk at an even
and at an odd index, which is what a wrong operand order of the pair hash, a
sibling taken from the wrong slot or a skipped level handled wrongly would
fail.  Byte work: every comparison is exact."""
import hashlib

import numpy as np
import pytest

import hbbft_amd as hb
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def sibling_levels(n, j):
    """Levels of an n-leaf tree at which leaf j has a sibling (merkle.rs:44-63);
    an odd last node is promoted and adds no digest to the proof."""
    out, lvl, sz = [], 0, n
    while sz > 1:
        if (j ^ 1) < sz:
            out.append(lvl)
        j >>= 1
        sz = (sz + 1) // 2
        lvl += 1
    return out


def sample_instances(count, k=8):
    return sorted({0, count - 1} | {(t * 2654435761) % count for t in range(1, k - 1)})


def send(torch, n, f, S, count, seed):
    """frame + encode, merkle and proofs of `count` random payloads whose shards
    are S bytes: device tensors, and the payloads on the host."""
    rb = hb.RbcBatch(n, f, device=0)
    plen = rb.k * S - 4
    assert hb.shard_len(plen, rb.k) == S
    pay = np.random.default_rng(seed).integers(0, 256, (count, plen), dtype=np.uint8)
    payloads = torch.zeros((count, (plen + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
    payloads[:, :plen] = torch.from_numpy(pay).cuda()
    slab = rb.alloc_slab(count, S)
    slab.fill_(0x5A)
    nodes = rb.alloc_nodes(count)
    rb.frame(payloads, plen, slab)
    rb.encode(slab, S)
    del payloads
    rb.merkle(slab, S, nodes)
    digests = torch.zeros((count, n, max(rb.dslots, 1), 32), dtype=torch.uint8, device="cuda")
    ndig = torch.zeros((count, n), dtype=torch.uint8, device="cuda")
    rb.proofs(nodes, digests, ndig)
    return dict(rb=rb, n=n, f=f, S=S, plen=plen, count=count, pay=pay, slab=slab, nodes=nodes,
                digests=digests, ndig=ndig)


def check_samples_vs_oracle(r):
    """Leaves, tree and proofs of the sampled instances equal the oracle's."""
    n, f, S = r["n"], r["f"], r["S"]
    for i in sample_instances(r["count"]):
        sh, nd = orc.send_shards(n, f, r["pay"][i].tobytes())
        assert np.array_equal(r["slab"][i, :, :S].cpu().numpy(), sh), (S, i)
        assert np.array_equal(r["nodes"][i].cpu().numpy(), nd), (S, i)
        dg, ndg = r["digests"][i].cpu().numpy(), r["ndig"][i].cpu().numpy()
        for j in range(n):
            p = orc.merkle_proof(nd, n, j)
            assert ndg[j] == len(p) == len(sibling_levels(n, j)), (S, i, j)
            assert np.array_equal(dg[j, : len(p)], p), (S, i, j)


def check_pipeline(torch, n, count, S, seed):
    """run_pipeline of test_gpu_parity at a grid of count x n sponges: every
    proof valid, every instance decoded from n - f shards to its tree and its
    payload; sampled instances against the oracle."""
    f = (n - 1) // 3
    r = send(torch, n, f, S, count, seed)
    rb, slab, nodes, plen = r["rb"], r["slab"], r["nodes"], r["plen"]
    ok = torch.zeros((count, n), dtype=torch.uint8, device="cuda")
    rb.validate(slab, S, r["digests"], r["ndig"], nodes, ok)
    assert bool(ok.all()), (S, int((ok == 0).sum()))
    check_samples_vs_oracle(r)
    del r["digests"], r["ndig"]
    present = np.stack([orc.gen_present(seed + 1, i, n, f) for i in range(count)])
    pres_d = torch.from_numpy(present).cuda()
    roots = nodes[:, -1, :].clone()
    slab[pres_d == 0] = 0xA5   # the erased rows arrive as garbage; decoded in place
    nodes2 = rb.alloc_nodes(count)
    out = torch.zeros((count, (rb.k * S + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
    plen_out = torch.zeros(count, dtype=torch.int32, device="cuda")
    status = torch.zeros(count, dtype=torch.int32, device="cuda")
    rb.decode(slab, S, pres_d, roots, nodes2, out, plen_out, status)
    torch.cuda.synchronize()
    assert bool((status == 0).all()) and bool((plen_out == plen).all()), S
    assert torch.equal(nodes2, nodes), S
    assert np.array_equal(out[:, :plen].cpu().numpy(), r["pay"]), S


def check_rejections(torch, r, tamper):
    """Apply `tamper` (a list of (kind, instance, proof, ...)) to copies of the
    proofs of `r`: exactly the tampered proofs are rejected."""
    rb, n, S, count = r["rb"], r["n"], r["S"], r["count"]
    slab, digests, ndig = r["slab"].clone(), r["digests"].clone(), r["ndig"].clone()
    idx = torch.arange(n, dtype=torch.int32, device="cuda").repeat(count, 1)
    bad = set()
    for kind, i, j, *arg in tamper:
        assert (i, j) not in bad, "one tampering per proof"
        bad.add((i, j))
        if kind == "sibling":    # one bit of digest slot arg[0]
            assert arg[0] < int(ndig[i, j])
            digests[i, j, arg[0], (5 * i + j) % 32] ^= 1 << (i % 8)
        elif kind == "index":
            idx[i, j] = j ^ 1
        elif kind == "ndig":
            if arg[0] > 0:
                ndig[i, j] += arg[0]
            else:
                ndig[i, j] -= -arg[0]
        elif kind == "value":
            slab[i, j, arg[0]] ^= 0x10
    ok = torch.zeros((count, n), dtype=torch.uint8, device="cuda")
    rb.validate(slab, S, digests, ndig, r["nodes"], ok, indices=idx)
    torch.cuda.synchronize()
    want = np.ones((count, n), np.uint8)
    for i, j in bad:
        want[i, j] = 0
    got = ok.cpu().numpy()
    assert np.array_equal(got, want), sorted(set(zip(*np.nonzero(got != want))))[:8]


def level_flips(n, count, levels):
    """For each level: sibling of that level flipped in one proof whose index
    is even at the level and in one whose index is odd, in instances spread
    over the grid."""
    out = []
    for d in levels:
        i = (count // 7) * (d + 1) + d
        j = (37 + 5 * d) % n
        out.append(("sibling", i, j & ~(1 << d), d))
        out.append(("sibling", i + 1, j | (1 << d), d))
    return out


# one-lane, 8-byte loads: 4096 x 64 = 2^18 sponges per launch
@pytest.mark.parametrize("S", [135, 136, 137, 271, 272, 273, 409])
def test_pipeline_one_lane_kernels(torch_cuda, S):
    check_pipeline(torch_cuda, 64, 4096, S, seed=1000 + S)


def test_rejections_one_lane_kernels(torch_cuda):
    n, count, S = 64, 4096, 273
    r = send(torch_cuda, n, 21, S, count, seed=77)
    tamper = level_flips(n, count, range(6)) + [
        ("index", 100, 20), ("index", 101, 21),
        ("ndig", 2000, 33, -1), ("ndig", 2001, 34, +1),
        ("value", 3000, 63, S - 1), ("value", 3001, 0, 0)]
    check_rejections(torch_cuda, r, tamper)


# promoted nodes: lanes that skip a level while their neighbours hash
@pytest.mark.parametrize("n,count", [(100, 2688), (7, 37456)])
def test_odd_trees_one_lane_kernels(torch_cuda, n, count):
    torch = torch_cuda
    assert count * n >= 1 << 18
    f = (n - 1) // 3
    r = send(torch, n, f, 137, count, seed=n)
    ok = torch.zeros((count, n), dtype=torch.uint8, device="cuda")
    r["rb"].validate(r["slab"], r["S"], r["digests"], r["ndig"], r["nodes"], ok)
    assert bool(ok.all())
    check_samples_vs_oracle(r)
    depth = hb.max_proof_len(n)
    short = [j for j in range(n) if len(sibling_levels(n, j)) < depth]
    assert short, "the tree has promoted nodes"
    j = short[0]
    lv = sibling_levels(n, j)
    skipped = min(set(range(depth)) - set(lv))
    after = sum(1 for x in lv if x < skipped)        # the first slot used after the skip
    tamper = [("sibling", count // 3, j, min(after, len(lv) - 1)),
              ("sibling", count // 3 + 1, j, len(lv) - 1),
              ("sibling", count // 2, short[-1], 0),
              ("ndig", count // 2 + 1, j, +1),       # a spare slot is there: too many digests
              ("ndig", count // 2 + 2, j, -1),
              ("index", count - 2, short[-1]),
              ("sibling", 5, 0, depth - 1), ("sibling", 6, 1, 0)]
    check_rejections(torch, r, tamper)


# one lane, 16-byte loads: 512 x 64 = 32,768 sponges per launch
@pytest.mark.parametrize("S", [136, 273, 409])
def test_pipeline_and_rejections_wide_load_kernels(torch_cuda, S):
    n, count = 64, 512
    check_pipeline(torch_cuda, n, count, S, seed=2000 + S)
    r = send(torch_cuda, n, 21, S, count, seed=3000 + S)
    tamper = level_flips(n, count, [1, 4]) + [("index", 9, 20), ("ndig", 300, 33, -1),
                                               ("value", 511, 63, S - 1)]
    check_rejections(torch_cuda, r, tamper)


def test_lengths_differ_within_a_wave(torch_cuda):
    """merkle_ragged: the 7 rows of an instance share a length, and a wave
    holds nine instances, so its lanes run different numbers of full blocks."""
    torch = torch_cuda
    n, count = 7, 37456
    rb = hb.RbcBatch(n, device=0)
    gen = torch.Generator(device="cuda").manual_seed(9)
    slab = torch.randint(0, 256, (count, n, 608), dtype=torch.uint8, device="cuda", generator=gen)
    lens = 1 + np.arange(count, dtype=np.int64) % 600
    nodes = rb.alloc_nodes(count)
    rb.merkle_ragged(slab, torch.from_numpy(lens.astype(np.int32)).cuda(), nodes)
    torch.cuda.synchronize()
    # lengths around every block boundary, then instances spread over the grid
    picks = [L - 1 for L in (1, 7, 8, 135, 136, 137, 271, 272, 273, 407, 408, 409, 543, 544,
                             545, 600)]
    picks += [(t * 587 + 601) % count for t in range(64 - len(picks))]
    assert len(set(picks)) == 64
    for i in picks:
        rows, L = slab[i].cpu().numpy(), int(lens[i])
        vals = [rows[j, :L].tobytes() for j in range(n)]
        got = nodes[i].cpu().numpy()
        assert [got[j].tobytes() for j in range(n)] == \
            [hashlib.sha3_256(v).digest() for v in vals], (i, L)
        assert np.array_equal(got, orc.merkle_build(vals)), (i, L)


def test_ragged_values_every_length(torch_cuda):
    """MerkleTree.from_vec of 1,024 values of 0..1023 bytes: one lane each,
    64 different lengths in every wave."""
    vals = [bytes((11 * i + 3 * t + 1) & 0xFF for t in range(i)) for i in range(1024)]
    tree = hb.MerkleTree.from_vec(vals)
    assert tree.levels()[0] == [hashlib.sha3_256(v).digest() for v in vals]
