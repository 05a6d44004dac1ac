// hb_sim.hip -- phase 3 of a HoneyBadger round (include/hbrbc.h
// hbrbc_hb_round): the reference's honey_badger/epoch_state.rs, threshold_
// decrypt.rs as a message handler and the batch output of honey_badger.rs for
// every (instance, node), one epoch.  Phases 1 and 2 (hbrbc_sm_round with
// HBRBC_SM_SUBSET, hbrbc_subset_round) have run when this kernel starts: it
// reads phase 2's out_seq past a per-node cursor and phase 1's output_root (the
// delivered root slot names the ciphertext).  The host restatement hbbft_amd/
// honey_badger.py driven by tests/hb_net.py is the checker (tests/
// test_hb_sim.py); line numbers below are the reference's.
//
// One thread per (instance, node, proposer): a node's N ThresholdDecrypts are
// independent of each other but for the batch point, which is two reductions
// over the node's proposer threads in LDS.  A workgroup holds `nb` consecutive
// nodes (instance-major) times all n proposers, node the fast index of the
// thread id as it is of every table, so a wave's accesses are runs of nb
// consecutive elements and a share record byte is read by the nb threads of a
// (proposer, sender) pair at once.
//
// The batch point (honey_badger.rs:107-109, 172-185): a node's batch leaves at
// the first moment after Done at which every accepted proposer is Complete,
// and what arrives for the epoch after that is dropped.  The host handles a
// round's share records in (proposer, sender, emission) order, so when the
// batch leaves in step (b) it leaves at p*, the highest proposer whose
// decryption completes in this round, and the threads above p* must handle
// nothing.  Whether a decryption completes in (b) does not depend on the other
// proposers, so every thread first counts, without writing, the new valid
// shares of its records (the dry run); the reductions give "nobody waits
// after (a)", "nobody waits after (b)" and p*; then the records are handled.
#include "launchers.hpp"

#include <hip/hip_runtime.h>

namespace hbrbc {

namespace {

enum : uint32_t { HB_NS_DONE = 1u << 16, HB_NS_BATCH = 1u << 17 };
constexpr int HB_MAX_NB = 64;   // nodes of a workgroup

__global__ __launch_bounds__(512) void hb_round_kernel(hbrbc_hb_args a, int nb) {
    if (a.active && *a.active == 0u) return;   // quiescent (uniform: the whole block leaves)
    __shared__ uint32_t s_wait[HB_MAX_NB];     // bit 0: a proposer waits after (a), 1: after (b)
    __shared__ int s_pstar[HB_MAX_NB];
    __shared__ uint32_t s_total;
    const int n = (int)a.n, W = (n + 31) / 32, f = (n - 1) / 3;
    const uint32_t roots = a.roots;
    const int tid = (int)threadIdx.x;
    const int ln = tid % nb, p = tid / nb;
    const size_t gn = (size_t)blockIdx.x * nb + ln;      // the node, instance-major
    const bool in_range = gn < a.count * (size_t)n;       // (p < n: the block is nb x n)
    const size_t inst = in_range ? gn / n : 0;
    const int node = in_range ? (int)(gn - inst * n) : 0;
    const size_t b = inst * n + p;                        // the proposer's tables
    const size_t g = b * n + node;                        // this node's slot in them
    uint32_t bad = 0;

    uint32_t role = HBRBC_HB_ABSENT, ns = 0, ifl = 0;
    if (in_range) {
        role = a.role[gn];
        if (role > HBRBC_HB_ABSENT) {
            bad |= 1u;
            role = HBRBC_HB_ABSENT;
        }
        ns = a.node_state[gn];
        ifl = a.inst_flags[inst];
    }
    const bool live = in_range && role != HBRBC_HB_ABSENT;
    uint32_t cursor = ns & 0xFFFFu;
    bool done = ns & HB_NS_DONE;
    const bool was_batched = ns & HB_NS_BATCH;
    int done_round = (live && done) ? a.done_round[gn] : -1;
    uint32_t ds = live ? a.dstate[g] : 0u;
    uint32_t nfault = live ? a.fault_count[g] : 0u;
    uint16_t *flog = a.faults + g * (size_t)a.max_faults;
    auto fault = [&](int blamed, uint32_t kind) {
        if (nfault < a.max_faults) flog[nfault] = (uint16_t)(((uint32_t)blamed << 8) | kind);
        ++nfault;
    };
    uint32_t *mk = a.mask + b * (size_t)(2 * W) * n + node;   // word w at mk[w n]
    uint32_t rec = 0;   // this round's share record of (p, node)
    auto emit = [&](uint32_t var) {
        const uint32_t c = rec & 3u;
        if (c < 2u) rec = (rec & ~3u) | (c + 1u) | (var << (2u + c));
    };
    // share_ok of both variants against the ciphertext this node holds for p
    auto ok_table = [&]() -> const uint8_t * {
        const uint32_t slot = a.output_root[g];
        if (slot >= roots) {
            bad |= 1u;
            return nullptr;
        }
        return a.share_ok + ((b * roots + slot) * 2) * (size_t)n;
    };

    if (live && role == HBRBC_HB_STRAY && (a.round == 1 || (done && done_round + 1 == a.round)))
        emit(1u);

    // ---- (a) the Subset's new outputs (process_subset, epoch_state.rs:306-354)
    uint32_t len = live ? a.out_len[gn] : 0u;
    if (len > (uint32_t)n + 1u) {
        bad |= 2u;
        len = (uint32_t)n + 1u;
    }
    const uint8_t *seq = a.out_seq + gn * (size_t)(n + 1);
    const bool has_done = len > 0 && seq[len - 1] == HBRBC_SUBSET_DONE;
    if (live && !done && has_done) {
        done = true;
        done_round = a.round;
    }
    if (live && !was_batched) {
        // SubsetHandler::AllAtEnd (132-162) holds the contributions until Done
        const uint32_t end = ((ifl & HBRBC_HB_ALL_AT_END) && !has_done) ? cursor : len;
        for (uint32_t k = cursor; k < end; ++k) {
            const uint32_t v = seq[k];
            if (v == HBRBC_SUBSET_DONE) {   // 334-351: the other proposers' states go
                if (!(ds & HBRBC_HB_ACCEPTED) && (ds & 7u) != HBRBC_HB_DS_ABSENT) {
                    for (int w = 0; w < W; ++w) {   // td.sender_ids(), in id order
                        uint32_t bits = mk[(size_t)w * n];
                        while (bits) {
                            const int i = __ffs((int)bits) - 1;
                            bits &= bits - 1u;
                            fault(w * 32 + i, HBRBC_HB_UNEXPECTED_SHARE);
                        }
                    }
                    ds = HBRBC_HB_DS_REMOVED;
                }
            } else if (v >= (uint32_t)n) {
                bad |= 2u;
            } else if (v == (uint32_t)p) {
                if (!(ifl & HBRBC_HB_ENCRYPTED)) {   // 327-329
                    ds = HBRBC_HB_ACCEPTED | HBRBC_HB_DS_COMPLETE;
                    continue;
                }
                ds |= HBRBC_HB_ACCEPTED;   // send_decryption_share (375-394)
                const uint32_t slot = a.output_root[g];
                const uint32_t cs = slot < roots ? a.ct_state[b * roots + slot] : 3u;
                if (cs == 1u) {
                    fault(p, HBRBC_HB_DESERIALIZE_CT);
                } else if (cs == 2u) {   // (the entry exists before set_ciphertext fails)
                    fault(p, HBRBC_HB_INVALID_CT);
                    if ((ds & 7u) == HBRBC_HB_DS_ABSENT) ds |= HBRBC_HB_DS_NO_CIPHERTEXT;
                } else if (cs == 0u) {
                    const uint8_t *ok = a.share_ok + ((b * roots + slot) * 2) * (size_t)n;
                    uint32_t cnt = 0;
                    for (int w = 0; w < W; ++w) {   // remove_invalid_shares (204-217)
                        uint32_t keep = mk[(size_t)w * n], vm = mk[(size_t)(W + w) * n];
                        uint32_t bits = keep;
                        while (bits) {
                            const int i = __ffs((int)bits) - 1;
                            bits &= bits - 1u;
                            if (!ok[((vm >> i) & 1u) * n + w * 32 + i]) {
                                keep &= ~(1u << i);
                                fault(w * 32 + i, HBRBC_HB_UNVERIFIED_SHARE);
                            }
                        }
                        if (w == (node >> 5)) {   // our own share (160-167)
                            keep |= 1u << (node & 31);
                            mk[(size_t)(W + w) * n] = vm & ~(1u << (node & 31));
                        }
                        mk[(size_t)w * n] = keep;
                        cnt += (uint32_t)__popc(keep);
                    }
                    if (role == HBRBC_HB_BAD_SHARE) {
                        emit(1u);
                    } else if (role != HBRBC_HB_SILENT) {
                        emit(0u);
                        if (role == HBRBC_HB_TWICE) emit(0u);
                    }
                    ds = HBRBC_HB_ACCEPTED | (cnt > (uint32_t)f ? HBRBC_HB_DS_COMPLETE
                                                                : HBRBC_HB_DS_ONGOING);
                } else {
                    bad |= 1u;
                }
            }
        }
        cursor = end;
    }

    // ---- the batch point: dry run of (b), then the reductions over the node's threads
    if (tid < HB_MAX_NB) {
        s_wait[tid] = 0u;
        s_pstar[tid] = -1;
    }
    if (tid == 0) s_total = 0u;
    __syncthreads();
    const bool handles = live && !was_batched && a.round > 0;
    bool would = false;
    if (handles && done && (ds & 7u) == HBRBC_HB_DS_ONGOING) {
        if (const uint8_t *ok = ok_table()) {
            uint32_t cnt = 0;
            for (int w = 0; w < W; ++w) cnt += (uint32_t)__popc(mk[(size_t)w * n]);
            for (int s = 0; s < n && cnt <= (uint32_t)f; ++s) {
                if (s == node) continue;
                const uint32_t r = a.in[b * n + s];
                uint32_t k = r & 3u;
                if (!k) continue;
                if (k > 2u) k = 2u;
                bool have = (mk[(size_t)(s >> 5) * n] >> (s & 31)) & 1u;
                for (uint32_t c = 0; c < k; ++c)
                    if (!have && ok[((r >> (2u + c)) & 1u) * n + s]) {
                        have = true;
                        ++cnt;
                    }
            }
            would = cnt > (uint32_t)f;
        }
    }
    if (live && (ds & HBRBC_HB_ACCEPTED) && (ds & 7u) != HBRBC_HB_DS_COMPLETE)
        atomicOr(&s_wait[ln], would ? 1u : 3u);
    if (would) atomicMax(&s_pstar[ln], p);
    __syncthreads();
    const uint32_t wait = s_wait[ln];
    const int pstar = s_pstar[ln];
    const bool batch_a = live && !was_batched && done && !(wait & 1u);
    const bool batch_b = live && !was_batched && done && !batch_a && !(wait & 2u);

    // ---- (b) the share records (handle_message_content, 255-271; handle_message, 182-201)
    if (handles && !batch_a && !(batch_b && p > pstar)) {
        uint32_t st = ds & 7u, cnt = 0;
        const uint8_t *ok = nullptr;
        if (st == HBRBC_HB_DS_ONGOING) {
            ok = ok_table();
            for (int w = 0; w < W; ++w) cnt += (uint32_t)__popc(mk[(size_t)w * n]);
        }
        const bool unexpected = done && !(ds & HBRBC_HB_ACCEPTED);
        if (st != HBRBC_HB_DS_ONGOING || ok)
            for (int s = 0; s < n; ++s) {
                if (s == node) continue;
                const uint32_t r = a.in[b * n + s];
                uint32_t k = r & 3u;
                if (!k) continue;
                if (k > 2u) k = 2u;
                for (uint32_t c = 0; c < k; ++c) {
                    const uint32_t var = (r >> (2u + c)) & 1u;
                    if (unexpected) {   // 256-261
                        fault(s, HBRBC_HB_UNEXPECTED_SHARE);
                        continue;
                    }
                    if (st == HBRBC_HB_DS_COMPLETE) continue;   // 42, 183-185
                    if (st == HBRBC_HB_DS_ABSENT) st = HBRBC_HB_DS_NO_CIPHERTEXT;
                    if (st == HBRBC_HB_DS_ONGOING && !ok[var * n + s]) {
                        fault(s, HBRBC_HB_UNVERIFIED_SHARE);
                        continue;
                    }
                    uint32_t *mw = mk + (size_t)(s >> 5) * n, *vw = mk + (size_t)(W + (s >> 5)) * n;
                    const uint32_t bit = 1u << (s & 31), m = *mw, vm = *vw;
                    *mw = m | bit;   // (insert replaces the stored share)
                    *vw = var ? (vm | bit) : (vm & ~bit);
                    if (m & bit) {
                        fault(s, HBRBC_HB_MULTIPLE_SHARES);
                        continue;
                    }
                    ++cnt;   // try_output (232-252)
                    if (st == HBRBC_HB_DS_ONGOING && cnt > (uint32_t)f) st = HBRBC_HB_DS_COMPLETE;
                }
            }
        ds = (ds & ~7u) | st;
    }

    // ---- the batch (try_output_batch, 277-303)
    if ((batch_a || batch_b) && (ds & HBRBC_HB_ACCEPTED)) {
        const uint32_t slot = a.output_root[g];
        if (slot >= roots) bad |= 1u;
        else if (a.undeserialisable[b * roots + slot]) fault(p, HBRBC_HB_BATCH_DESERIALIZE);
    }

    if (live) {
        a.dstate[g] = (uint8_t)ds;
        a.fault_count[g] = nfault;
        if (rec) {
            a.out[g] = (uint8_t)rec;
            atomicAdd(&s_total, rec & 3u);
        }
        if (p == 0) {
            a.node_state[gn] = cursor | (done ? HB_NS_DONE : 0u) |
                               ((was_batched || batch_a || batch_b) ? HB_NS_BATCH : 0u);
            if (done) a.done_round[gn] = done_round;
            if (batch_a || batch_b) a.batch_round[gn] = a.round;
        }
    }
    if (bad) atomicOr(a.emitted + 1, bad);
    __syncthreads();
    if (tid == 0 && s_total) atomicAdd(a.emitted, s_total);
}

}  // namespace

hipError_t launch_hb_round(const hbrbc_hb_args &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    const int n = (int)a.n;
    const size_t total = a.count * (size_t)n;
    int nb = 512 / n;   // n <= 255: at least 2 nodes, at most 512 threads
    if (nb > HB_MAX_NB) nb = HB_MAX_NB;
    if ((size_t)nb > total) nb = (int)total;
    const unsigned blocks = (unsigned)((total + nb - 1) / nb);
    hipLaunchKernelGGL(hb_round_kernel, dim3(blocks), dim3((unsigned)(nb * n)), 0, s, a, nb);
    return hipGetLastError();
}

}  // namespace hbrbc
