// subset_sim.hip -- phase 2 of a Subset round (include/hbrbc.h
// hbrbc_subset_round): the reference's subset/subset.rs and subset/
// proposal_state.rs for every (instance, node), over the BinaryAgreement
// handlers of ba_node.hpp.  Phase 1 is hbrbc_sm_round (sim.hip) with
// HBRBC_SM_SUBSET over the count x n broadcast instances; it has run when this
// kernel starts, and its output_root is the coupling in both directions: a
// root slot there is a delivered broadcast, HBRBC_SM_DROPPED written here
// stops the broadcast of a rejected proposal.  The host restatement
// hbbft_amd/subset.py driven by tests/subset_net.py is the checker
// (tests/test_subset_sim.py); line numbers below are the reference's.
//
// One thread per (instance, node); the lanes of a wave are nodes of one
// instance (of few instances below n = 64).  A node's round is a work list of
// agreement calls, taken one per iteration of a single loop so that propose
// and handle_message are each inlined once:
//  1. proposers in order whose broadcast has an output_root (proposal_state.
//     rs:97-110): Ongoing -> HasValue and propose(true), whose BVal is the
//     first record of this round's outbox of that agreement; Accepted ->
//     Complete(true) with its output;
//  2. the agreement records addressed to the node in (proposer, sender,
//     emission) order (handle_agreement, 117-137);
//  3. whenever the accepted count is N - f after a call (Subset::try_output,
//     subset.rs:154-169): vote_false on every proposal in order, AT ONCE --
//     before the node's remaining records of the round, those of higher
//     proposers included, whose propose(false) so precedes their records.  The
//     reference repeats that loop on every later call while the count stays
//     N - f; each repeat is a no-op, since after the first every agreement left
//     has an estimate (propose, binary_agreement.rs:232-240, sets it; update_
//     epoch keeps one), so the node remembers that it voted.
// While lanes agree on where they are the accesses are the coalesced ones of
// ba_round_kernel<false> (the nodes of an instance are the fast index of every
// table); a lane inside its vote loop runs on its own for n iterations.
//
// A BaNode is opened per proposer visit and closed when another proposer is
// visited or the agreement decides: epoch and flags live in registers while
// it is open; the out count and the fault count live in global memory between
// visits, because vote_false appends to the outboxes of proposers visited
// before and after.  The global state form only: the cores of an instance's n
// agreements are n times those ba_round_kernel stages, past the LDS from n =
// 24 or so.
#include "launchers.hpp"

#include <hip/hip_runtime.h>

#include "ba_node.hpp"

namespace hbrbc {

namespace {

enum : uint32_t { NS_VOTED = 1u << 16, NS_DONE = 1u << 17 };

// At the compiler's register budget (256 VGPRs and 16 AGPRs, nothing spilled, one
// wave per SIMD): a launch has count x n threads, a wave or less per SIMD at the
// sizes measured, so residency buys nothing; at ba_round_w3_kernel's 3 waves per
// SIMD the kernel spilled 295 VGPRs.
__global__ __launch_bounds__(256) void subset_round_kernel(hbrbc_subset_args a, int ipb) {
    if (a.active && *a.active == 0u) return;   // quiescent (uniform: the whole block leaves)
    const int n = (int)a.n, Q = (int)a.queue_epochs, W = (n + 31) / 32, f = (n - 1) / 3;
    const int tid = (int)threadIdx.x;
    const int li = tid / n, local = tid - li * n;
    const size_t inst = (size_t)blockIdx.x * ipb + li;
    if (li >= ipb || inst >= a.count) return;
    const size_t b0 = inst * n;                  // the instance's first agreement
    const size_t gn = inst * n + local;          // this node
    const size_t cw = ba_core_words(n), ib = (size_t)n * ba_state_bytes(n, Q);
    const size_t icw = (size_t)n * cw;           // core words of an agreement instance
    const uint32_t rec = 1u + W;
    const int mw = 1 + (local >> 5);
    const uint32_t mb = 1u << (local & 31);
    // this node's slot of agreement p in the [count n][n] tables
    auto slot = [&](int p) { return (b0 + p) * n + local; };

    BaNode m;
    m.n = n;
    m.f = f;
    m.W = W;
    m.Q = Q;
    m.me = local;
    m.coins = a.coins;
    m.max_out = a.max_out;
    m.max_faults = a.max_faults;
    m.rec = rec;
    m.cs = (size_t)n;
    m.sout = 0;
    m.ts_out = false;
    m.pend = 0;
    m.sp = 0;
    int cur = -1;                  // the open agreement
    uint32_t cur_ovf = 0, total = 0, bad = 0;
    auto close = [&]() {
        if (cur < 0) return;
        const size_t g = slot(cur);
        m.core[0] = m.epoch;
        m.core[m.cs] = m.fl;
        a.out_count[g] = m.nout | (((m.bad & BA_BAD_OUT) || cur_ovf) ? 0x80000000u : 0u);
        a.fault_count[g] = m.nfault;
        bad |= m.bad;
        cur = -1;
    };
    auto open = [&](int p) {
        if (cur == p) return;
        close();
        const size_t b = b0 + p, g = b * n + local;
        m.role = a.role[g];
        m.ahead = a.ahead[b];
        m.flip = a.flip + b * W;
        m.sok = a.share_ok + b * a.coins * 2 * n;
        m.coinv = a.coin + b * a.coins;
        m.core = reinterpret_cast<uint32_t *>(a.state + b * ib) + local;
        m.ring = reinterpret_cast<uint16_t *>(a.state + b * ib + 4 * icw) + (size_t)local * n * Q;
        m.epoch = m.core[0];
        m.fl = m.core[m.cs];
        m.out = a.out + g * a.max_out * rec;
        const uint32_t oc = a.out_count[g];
        m.nout = oc & 0x7FFFFFFFu;
        cur_ovf = oc >> 31;
        m.faults = a.faults + g * a.max_faults;
        m.nfault = a.fault_count[g];
        m.bad = 0;
        m.decision = a.decision + g;
        m.decision_epoch = a.decision_epoch + g;
        cur = p;
    };

    uint32_t acc, comp;            // count_accepted (subset.rs:147-150), complete proposals
    bool voted, done;
    if (a.round == 0) {
        // epoch 0 of every agreement: CoinState::Decided(true) (ba_node_round);
        // the proposal states: Ongoing, or dropped where the caller preset
        // HBRBC_SM_DROPPED (a dead node)
        acc = comp = 0;
        voted = done = false;
        for (int p = 0; p < n; ++p) {
            const size_t g = slot(p);
            reinterpret_cast<uint32_t *>(a.state + (b0 + p) * ib)[(size_t)n + local] = BF_COIN_VAL;
            const bool dead = a.output_root[g] == HBRBC_SM_DROPPED;
            a.proposal[g] = dead ? HBRBC_SUBSET_COMPLETE_FALSE : HBRBC_SUBSET_ONGOING;
            comp += dead ? 1u : 0u;
        }
    } else {
        const uint32_t ns = a.node_state[gn];
        acc = ns & 0xFFu;
        comp = (ns >> 8) & 0xFFu;
        voted = ns & NS_VOTED;
        done = ns & NS_DONE;
    }
    for (int p = 0; p < n; ++p) a.out_count[slot(p)] = 0;   // this round's outboxes
    uint32_t olen = a.out_len[gn];
    uint8_t *seq = a.out_seq + gn * (size_t)(n + 1);
    auto output = [&](uint32_t v) {   // (at most n contributions and Done)
        if (olen < (uint32_t)n + 1u) seq[olen] = (uint8_t)v;
        ++olen;
    };

    int phase = 0, ap = 0;         // step 1 and its proposer cursor
    int cp = 0, cs = 0;            // step 2: proposer, sender, record, the sender's count
    uint32_t ce = 0, cc = 0;
    bool cc_ok = false;
    int vp = n;                    // step 3's proposer cursor (n: not voting)
    for (;;) {
        int p = -1, mode = 0, snd = 0;   // the call: 0 propose(false), 1 propose(true), 2 a record
        uint32_t h = 0;
        bool changed = false, vote_end = false;
        if (vp < n) {   // ProposalState::vote_false (86-88) on proposal vp
            const int q = vp++;
            const uint8_t st = a.proposal[slot(q)];
            if (st == HBRBC_SUBSET_ONGOING || st == HBRBC_SUBSET_HAS_VALUE) p = q;
            vote_end = vp == n;
        } else if (phase == 0) {   // handle_broadcast (91-113) with phase 1's outcome
            if (ap == n) {
                phase = 1;
                continue;
            }
            const int q = ap++;
            const size_t g = slot(q);
            if (a.output_root[g] < HBRBC_SM_DROPPED) {
                const uint8_t st = a.proposal[g];
                if (st == HBRBC_SUBSET_ONGOING) {
                    a.proposal[g] = HBRBC_SUBSET_HAS_VALUE;
                    p = q;
                    mode = 1;
                } else if (st == HBRBC_SUBSET_ACCEPTED) {
                    a.proposal[g] = HBRBC_SUBSET_COMPLETE_TRUE;
                    ++comp;
                    output((uint32_t)q);
                    changed = true;
                }
            }
        } else {   // the next agreement record
            if (cp == n || a.round == 0) break;   // (round 0 has no inbox)
            if (!cc_ok) {
                if (cs == 0) {   // an agreement that is gone stays gone: its records are no-ops
                    const uint8_t st = a.proposal[slot(cp)];
                    if (st != HBRBC_SUBSET_ONGOING && st != HBRBC_SUBSET_HAS_VALUE) {
                        ++cp;
                        continue;
                    }
                }
                const uint32_t c = a.in_count[(b0 + cp) * n + cs] & 0x7FFFFFFFu;
                cc = c < a.max_out ? c : a.max_out;
                ce = 0;
                cc_ok = true;
            }
            if (ce >= cc) {
                cc_ok = false;
                if (++cs == n) {
                    cs = 0;
                    ++cp;
                }
                continue;
            }
            const uint32_t *r = a.in + (((b0 + cp) * n + cs) * (size_t)a.max_out + ce) * rec;
            ++ce;
            // (a node's own records do not name it: all_but_me)
            if (cs != local && (r[mw] & mb)) {
                const uint8_t st = a.proposal[slot(cp)];
                // (Accepted, Complete: the agreement is gone, 135)
                if (st == HBRBC_SUBSET_ONGOING || st == HBRBC_SUBSET_HAS_VALUE) {
                    p = cp;
                    mode = 2;
                    snd = cs;
                    h = r[0];
                }
            }
        }
        if (p >= 0) {   // handle_agreement (117-137)
            open(p);
            const uint32_t n0 = m.nout;
            if (mode == 2) m.handle_message(snd, h);
            else m.propose((uint32_t)mode);
            total += m.nout - n0;
            if (m.fl & BF_DEC_HAS) {   // the agreement was there, so the decision is new
                const bool d = m.fl & BF_DEC_VAL;
                close();
                const size_t g = slot(p);
                if (a.proposal[g] == HBRBC_SUBSET_ONGOING) {
                    if (d) {
                        a.proposal[g] = HBRBC_SUBSET_ACCEPTED;
                    } else {   // the Broadcast is dropped with the agreement
                        a.proposal[g] = HBRBC_SUBSET_COMPLETE_FALSE;
                        a.output_root[g] = HBRBC_SM_DROPPED;
                        ++comp;
                    }
                } else {   // HasValue
                    a.proposal[g] = d ? HBRBC_SUBSET_COMPLETE_TRUE : HBRBC_SUBSET_COMPLETE_FALSE;
                    ++comp;
                    if (d) output((uint32_t)p);
                }
                acc += d ? 1u : 0u;
                changed = true;
            }
        }
        // Subset::try_output (154-169), not from inside its own vote loop
        if (vp < n || !(changed || vote_end) || done || acc < (uint32_t)(n - f)) continue;
        if (!vote_end && acc == (uint32_t)(n - f) && !voted) {
            voted = true;
            vp = 0;
            continue;   // (the Done test follows the loop)
        }
        if (comp == (uint32_t)n) {
            done = true;
            output(HBRBC_SUBSET_DONE);
        }
    }
    close();
    a.node_state[gn] = (acc & 0xFFu) | ((comp & 0xFFu) << 8) | (voted ? NS_VOTED : 0u) |
                       (done ? NS_DONE : 0u);
    a.out_len[gn] = olen;
    if (total) atomicAdd(a.emitted, total);
    if (bad) atomicOr(a.emitted + 1, bad);
}

}  // namespace

hipError_t launch_subset_round(const hbrbc_subset_args &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    const int n = (int)a.n;
    int ipb = n >= 128 ? 1 : 256 / n;
    if ((size_t)ipb > a.count) ipb = (int)a.count;
    const unsigned blocks = (unsigned)((a.count + ipb - 1) / ipb);
    hipLaunchKernelGGL(subset_round_kernel, dim3(blocks), dim3((unsigned)(ipb * n)), 0, s, a, ipb);
    return hipGetLastError();
}

}  // namespace hbrbc
