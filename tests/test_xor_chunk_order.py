"""Chunk order of the specialised XOR-network kernels (jit.hip gen_prologue):
workgroup b takes chunk (b % 8) * (grid / 8) + b / 8, so that each XCD walks
consecutive chunks; the grid's last grid % 8 workgroups keep their own index.
Any assignment of chunks to workgroups is bit-exact; this checks the map is a
bijection where it can go wrong: grids below 8, grids that are no multiple of
8, and several chunks per row, against the oracle and against the plain order
(HBRBC_JIT_XCD=0)."""
import numpy as np
import pytest

from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

N, F, K = 16, 5, 6
PLEN = K * 4112 - 4 - 3          # S = 4112: three 2 KB chunks a row, the last one 16 bytes


@pytest.fixture(scope="module")
def slabs(tmp_path_factory):
    """{(xcd, count): (twin's slab, encoder's slab)} for grids of 3, 9 and 111 workgroups."""
    import os
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import hbbft_amd as hb
    assert hb.shard_len(PLEN, K) == 4112
    out = {}
    old = {k: os.environ.get(k) for k in ("HBRBC_JIT_XCD", "HBRBC_JIT_DIR", "HBRBC_JIT")}
    try:
        for xcd in ("1", "0"):
            d = str(tmp_path_factory.mktemp("jit_xcd" + xcd))
            os.environ.update(HBRBC_JIT_XCD=xcd, HBRBC_JIT_DIR=d, HBRBC_JIT="load")
            hb.jit_build_encode(K, N - K, d)
            rb = hb.RbcBatch(N, F, device=0)
            for count in (1, 3, 37):
                pay = np.stack([orc.gen_payload(0x5843, i, PLEN) for i in range(count)])
                payloads = torch.zeros((count, (PLEN + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
                payloads[:, :PLEN] = torch.from_numpy(pay).cuda()
                slab = rb.alloc_slab(count, 4112)
                slab.fill_(0x5A)
                rb.frame_encode(payloads, PLEN, slab)
                slab2 = rb.alloc_slab(count, 4112)
                slab2.fill_(0xA5)
                rb.frame(payloads, PLEN, slab2)
                rb.encode(slab2, 4112)
                torch.cuda.synchronize()
                assert rb.coding.encode_kernel() == "specialised"
                out[(xcd, count)] = (slab.cpu().numpy()[:, :, :4112], slab2.cpu().numpy()[:, :, :4112])
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


@pytest.mark.parametrize("count", [1, 3, 37])
def test_chunk_order_is_bit_exact(slabs, count):
    ref = np.stack([orc.send_shards(N, F, orc.gen_payload(0x5843, i, PLEN).tobytes())[0]
                    for i in range(count)])
    for xcd in ("1", "0"):
        twin, enc = slabs[(xcd, count)]
        assert np.array_equal(twin, ref), "frame+encode twin, HBRBC_JIT_XCD=" + xcd
        assert np.array_equal(enc, ref), "encoder, HBRBC_JIT_XCD=" + xcd
