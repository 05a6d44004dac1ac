// ba_node.hpp -- one BinaryAgreement node of the batched state machine
// (ba_sim.hip): the handlers of the reference's binary_agreement.rs,
// sbv_broadcast.rs and threshold_sign.rs:127-270 restated one by one over the
// node's bit-mask state.  The host restatement hbbft_amd/binary_agreement.py
// is the checker (tests/test_ba_sim.py); line numbers below are the
// reference's.  Plain C++ (HB_HD is empty in a host build), so the handlers
// can be compiled for the CPU and stepped through there.
//
// No recursion.  The reference's handlers call each other recursively in
// three places; each is unrolled here:
//  * sbv send -> handle_message(our_id) -> send (sbv_broadcast.rs:140-147):
//    the inner handle_bval of our own BVal can only reach send_bval(b) with b
//    already in sent_bval, so it is a separate function without that call.
//  * ThresholdSign::try_output -> sign -> handle_message(our_id) (227-247):
//    `terminated` is already set, so the own share is sent and not handled.
//  * try_update_epoch -> update_epoch -> (queue replay) -> handle_message_
//    content -> ... -> try_update_epoch (binary_agreement.rs:416-435, 491-520):
//    try_update_epoch only RECORDS the update (`pend`); `drain` runs it after
//    the handler that asked for it has unwound.  Nothing in the reference
//    runs between the nested update_epoch's return and the unwinding except
//    (a) the outer update_epoch's replay loop, which returns because the
//    epoch moved (510-516: after a nested update from send_bval it re-reads
//    `self.epoch` and finds that epoch's queue already taken), (b) the second
//    try_update_epoch of try_finish_conf_round (481), a no-op then: whenever
//    a coin value and conf_values are both known, try_update_epoch has just
//    run and decided or moved the epoch, and (c) handle_term's handle_conf
//    (351), which DOES act on the new epoch's state: it is kept as a
//    continuation (sender, b) on a small stack and runs when the update it
//    waited for, with everything nested in it, is complete.  A continuation
//    is pushed at most once at the top level and once per replayed epoch
//    (the replay is abandoned at the first update), so the stack holds at
//    most queue_epochs + 1 entries.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hbrbc.h"

#ifndef HB_HD
#define HB_HD __host__ __device__ __forceinline__
#endif

namespace hbrbc {

// message kinds (binary_agreement/mod.rs:135-144, sbv_broadcast.rs:29-34)
enum { BA_BVAL = 0, BA_AUX = 1, BA_CONF = 2, BA_TERM = 3, BA_COIN = 4 };
// FaultKind (mod.rs:110-129), in declaration order; 5 = CoinFault(
// UnverifiedSignatureShareSender)
enum {
    BAF_DUPLICATE_BVAL = 0,
    BAF_DUPLICATE_AUX = 1,
    BAF_MULTIPLE_CONF = 2,
    BAF_MULTIPLE_TERM = 3,
    BAF_AGREEMENT_EPOCH = 4,
    BAF_COIN_FAULT = 5
};
// the node's sender masks, W words each
enum { BM_BVAL = 0, BM_AUX = 2, BM_CONF_F = 4, BM_CONF_T = 5, BM_TERM = 6, BM_COIN = 8 };
// flags word.  BoolSets are bool_set.rs's two bits: 1 = {false}, 2 = {true}.
enum : uint32_t {
    BF_EST_HAS = 1u << 0, BF_EST_VAL = 1u << 1,    // estimated
    BF_DEC_HAS = 1u << 2, BF_DEC_VAL = 1u << 3,    // decision
    BF_BIN_SHIFT = 4,                              // sbv bin_values
    BF_SENT_SHIFT = 6,                             // sbv sent_bval
    BF_SBV_TERM = 1u << 8,                         // sbv terminated
    BF_CONF_HAS = 1u << 9, BF_CONF_SHIFT = 10,     // conf_values
    BF_COIN_PROG = 1u << 12,                       // CoinState::InProgress (else Decided)
    BF_COIN_VAL = 1u << 13,                        // Decided(value)
    BF_TS_INPUT = 1u << 14, BF_TS_TERM = 1u << 15  // ThresholdSign had_input / terminated
};
// emitted[1] bits
enum : uint32_t { BA_BAD_OUT = 1u, BA_BAD_QUEUE = 2u, BA_BAD_COINS = 4u, BA_BAD_EPOCH = 8u,
                  BA_BAD_STACK = 16u };
// a ring entry: one sender's ReceivedMessages of one future epoch
// (binary_agreement.rs:46-57)
enum : uint32_t {
    BQ_BVAL_SHIFT = 0, BQ_AUX_SHIFT = 2, BQ_CONF_HAS = 1u << 4, BQ_CONF_SHIFT = 5,
    BQ_TERM_HAS = 1u << 7, BQ_TERM_VAL = 1u << 8, BQ_COIN_HAS = 1u << 9, BQ_COIN_TAMPER = 1u << 10
};
constexpr int kBaStack = 18;             // queue_epochs <= 16
constexpr uint32_t kBaMaxFuture = 1000;  // binary_agreement.rs:214

struct BaNode {
    // ---- the instance and the node
    int n, f, W, Q, me, role;
    uint32_t coins, ahead, max_out, max_faults, rec;
    const uint32_t *flip;   // [W]
    const uint8_t *sok;     // [coins][2][n]
    const uint8_t *coinv;   // [coins]
    // ---- state: masks M(k, w) at core[(2 + k * W + w) * cs]; epoch and flags
    // (words 0 and 1) live in registers for the round
    uint32_t *core;
    size_t cs;
    uint16_t *ring;         // [n][Q]
    uint32_t epoch, fl;
    // ---- the round's results
    uint32_t *out;
    uint32_t nout;
    uint16_t *faults;
    uint32_t nfault;
    uint32_t bad;
    uint8_t *decision;
    uint16_t *decision_epoch;
    // ---- between handlers
    uint32_t sout;          // the sbv step's output (a BoolSet, 0 none)
    bool ts_out;            // the ThresholdSign step has an output
    uint32_t pend;          // 1 + b: update_epoch(b) asked for
    uint16_t cstack[kBaStack];
    int sp;

    HB_HD uint32_t &M(int k, int w) { return core[(size_t)(2 + k * W + w) * cs]; }
    HB_HD bool test(int k, int s) { return (M(k, s >> 5) >> (s & 31)) & 1u; }
    HB_HD void set(int k, int s) { M(k, s >> 5) |= 1u << (s & 31); }
    HB_HD int count(int k) {
        int c = 0;
        for (int w = 0; w < W; ++w) c += __builtin_popcount(M(k, w));
        return c;
    }
    HB_HD static uint32_t bs(uint32_t b) { return b ? 2u : 1u; }   // BoolSet::from(bool)
    HB_HD uint32_t bin_values() const { return (fl >> BF_BIN_SHIFT) & 3u; }

    HB_HD void fault(int node, int kind) {
        if (nfault < max_faults) faults[nfault] = (uint16_t)((node << 8) | kind);
        ++nfault;
    }

    // ---- what leaves the node (Target::all(): every node but the sender)
    HB_HD uint32_t all_but_me(int w) const {
        const int fw = n >> 5;
        const uint32_t all = w < fw ? 0xFFFFFFFFu : (w == fw ? (1u << (n & 31)) - 1u : 0u);
        return all & ~((me >> 5) == w ? 1u << (me & 31) : 0u);
    }
    // one record; part: 0 every recipient, 1 those outside flip, 2 those inside
    HB_HD void put(uint32_t h, int part) {
        if (nout >= max_out) {
            bad |= BA_BAD_OUT;
            return;
        }
        uint32_t *r = out + (size_t)nout * rec;
        ++nout;
        r[0] = h;
        for (int w = 0; w < W; ++w) {
            const uint32_t m = all_but_me(w);
            r[1 + w] = part == 0 ? m : (part == 1 ? m & ~flip[w] : m & flip[w]);
        }
    }
    HB_HD void emit(uint32_t kind, uint32_t val, uint32_t tam, uint32_t ep) {
        if (role == HBRBC_BA_SILENT) return;
        if (role == HBRBC_BA_AHEAD || role == HBRBC_BA_REPLAY_AHEAD) ep += ahead;
        if (ep >= 0xFFFFu) {
            bad |= BA_BAD_EPOCH;
            ep = 0xFFFFu;
        }
        if (role == HBRBC_BA_BAD_COIN && kind == BA_COIN) tam = 1;
        const uint32_t h = kind | (val << 8) | (tam << 12) | (ep << 16);
        if (role == HBRBC_BA_TWO_FACED) {
            uint32_t v2 = val;
            if (kind == BA_CONF) v2 = (val == 1u || val == 2u) ? val ^ 3u : val;
            else if (kind != BA_COIN) v2 = val ^ 1u;
            put(h, 1);
            put(kind | (v2 << 8) | (tam << 12) | (ep << 16), 2);
        } else {
            put(h, 0);
            if (role == HBRBC_BA_REPLAY || role == HBRBC_BA_REPLAY_AHEAD) put(h, 0);
        }
    }

    // ---- sbv_broadcast.rs --------------------------------------------------
    HB_HD void sbv_try_output() {   // 158-186 (count_aux: `true` first)
        if (fl & BF_SBV_TERM) return;
        const uint32_t bin = bin_values();
        if (!bin) return;
        int cnt = 0;
        uint32_t vals = 0;
        for (int b = 1; b >= 0; --b) {
            if (!(bin & bs(b))) continue;
            const int c = count(BM_AUX + b);
            if (c) {
                vals |= bs(b);
                cnt += c;
            }
        }
        if (cnt < n - f) return;
        fl |= BF_SBV_TERM;
        if (!sout) sout = vals;
    }
    HB_HD void sbv_handle_aux(int s, uint32_t b) {   // 150-155
        if (test(BM_AUX + b, s)) {
            fault(s, BAF_DUPLICATE_AUX);
            return;
        }
        set(BM_AUX + b, s);
        sbv_try_output();
    }
    HB_HD void sbv_send_aux(uint32_t b) {   // send(Aux(b)), 140-147
        emit(BA_AUX, b, 0, epoch);
        sbv_handle_aux(me, b);
    }
    // handle_bval (114-137) up to the f + 1 test: true when count == f + 1
    HB_HD bool sbv_bval_core(int s, uint32_t b) {
        if (test(BM_BVAL + b, s)) {
            fault(s, BAF_DUPLICATE_BVAL);
            return false;
        }
        set(BM_BVAL + b, s);
        const int c = count(BM_BVAL + b);
        if (c == 2 * f + 1) {   // tested before f + 1; at f = 0 both fire
            fl |= bs(b) << BF_BIN_SHIFT;
            if (bin_values() != 3u) sbv_send_aux(b);   // first entry: Aux(b)
            else sbv_try_output();
        }
        return c == f + 1;
    }
    HB_HD void sbv_send_bval(uint32_t b) {   // 102-108
        if ((fl >> BF_SENT_SHIFT) & bs(b)) return;
        fl |= bs(b) << BF_SENT_SHIFT;
        emit(BA_BVAL, b, 0, epoch);
        // our own BVal: its send_bval(b) at f + 1 finds b in sent_bval
        sbv_bval_core(me, b);
    }
    HB_HD void sbv_handle_bval(int s, uint32_t b) {
        if (sbv_bval_core(s, b)) sbv_send_bval(b);
    }

    // ---- threshold_sign.rs:127-270, shares by reference --------------------
    HB_HD uint32_t slot() {   // coin slot q of epoch 3q + 2
        const uint32_t q = (epoch - 2u) / 3u;
        return q < coins ? q : coins - 1;   // (past the table: flagged in coin_state)
    }
    HB_HD void ts_try_output() {   // 227-247
        if (!(fl & BF_TS_TERM) && count(BM_COIN) > f) {
            fl |= BF_TS_TERM;
            // sign() after `terminated`: the share goes out, handle_message
            // (our_id) returns at once
            if (!(fl & BF_TS_INPUT)) {
                fl |= BF_TS_INPUT;
                emit(BA_COIN, 0, 0, epoch);
            }
            ts_out = true;
        }
    }
    HB_HD void ts_handle(int s, uint32_t t) {   // 181-197
        if (fl & BF_TS_TERM) return;
        if (!sok[((size_t)slot() * 2 + (t & 1u)) * n + s]) {   // is_share_valid, 216-225
            fault(s, BAF_COIN_FAULT);
            return;
        }
        set(BM_COIN, s);   // (stored shares are valid: remove_invalid_shares finds none)
        ts_try_output();
    }
    HB_HD void ts_sign() {   // 157-174
        if (fl & BF_TS_INPUT) return;
        fl |= BF_TS_INPUT;
        emit(BA_COIN, 0, 0, epoch);
        ts_handle(me, 0);
    }

    // ---- binary_agreement.rs -----------------------------------------------
    HB_HD void decide(uint32_t b) {   // 453-468: Term(b) with epoch + 1, not handled here
        if (fl & BF_DEC_HAS) return;
        fl |= BF_DEC_HAS | (b ? BF_DEC_VAL : 0u);
        *decision = (uint8_t)b;
        *decision_epoch = (uint16_t)epoch;
        emit(BA_TERM, b, 0, epoch + 1);
    }
    HB_HD void try_update_epoch() {   // 416-435
        if (fl & BF_DEC_HAS) return;
        if (fl & BF_COIN_PROG) return;
        if (!(fl & BF_CONF_HAS)) return;
        const uint32_t coin = (fl & BF_COIN_VAL) ? 1u : 0u;
        const uint32_t cv = (fl >> BF_CONF_SHIFT) & 3u;
        const bool def = cv == 1u || cv == 2u;
        const uint32_t dv = cv == 2u ? 1u : 0u;
        if (def && dv == coin) decide(coin);
        else pend = 1u + (def ? dv : coin);   // update_epoch, run by drain()
    }
    HB_HD void on_coin_step() {   // 397-408
        if (!ts_out) return;
        ts_out = false;
        fl &= ~(BF_COIN_PROG | BF_COIN_VAL);
        if (coinv[slot()]) fl |= BF_COIN_VAL;
        try_update_epoch();
    }
    HB_HD int count_conf() {   // 485-488: Confs that are subsets of bin_values
        const uint32_t bin = bin_values();
        int c = 0;
        for (int w = 0; w < W; ++w) {
            const uint32_t cf = M(BM_CONF_F, w), ct = M(BM_CONF_T, w);
            c += __builtin_popcount(bin == 3u ? (cf | ct) : (bin == 2u ? (ct & ~cf) : (bin == 1u ? (cf & ~ct) : 0u)));
        }
        return c;
    }
    HB_HD void try_finish_conf_round() {   // 471-482
        if (!(fl & BF_CONF_HAS) || count_conf() < n - f) return;
        if (!(fl & BF_COIN_PROG)) return;
        ts_sign();
        on_coin_step();
        if (!pend) try_update_epoch();   // (see the header: a no-op after an update)
    }
    HB_HD void handle_conf(int s, uint32_t v) {   // 331-334: a second Conf overwrites
        const uint32_t b = 1u << (s & 31);
        uint32_t &cf = M(BM_CONF_F, s >> 5), &ct = M(BM_CONF_T, s >> 5);
        cf = (v & 1u) ? (cf | b) : (cf & ~b);
        ct = (v & 2u) ? (ct | b) : (ct & ~b);
        try_finish_conf_round();
    }
    HB_HD void send_conf(uint32_t v) {   // 368-382, send 385-394
        if (fl & BF_CONF_HAS) return;
        fl |= BF_CONF_HAS | (v << BF_CONF_SHIFT);
        emit(BA_CONF, v, 0, epoch);
        handle_conf(me, v);
    }
    HB_HD void handle_sbvb_step() {   // 303-327
        const uint32_t o = sout;
        sout = 0;
        if (fl & BF_CONF_HAS) return;   // the Conf round has already started
        if (!o) return;
        if (!(fl & BF_COIN_PROG)) {
            fl |= BF_CONF_HAS | (o << BF_CONF_SHIFT);
            try_update_epoch();
        } else {
            send_conf(o);
        }
    }
    HB_HD void handle_term(int s, uint32_t b) {   // 339-353
        set(BM_TERM + b, s);
        if (fl & BF_DEC_HAS) return;
        if (count(BM_TERM + b) > f) {
            decide(b);
            return;
        }
        sbv_handle_bval(s, b);
        sbv_handle_aux(s, b);
        handle_sbvb_step();
        if (pend) {   // handle_conf runs on the state the update leaves (drain)
            if (sp < kBaStack) cstack[sp++] = (uint16_t)((s << 1) | b);
            else bad |= BA_BAD_STACK;
        } else {
            handle_conf(s, bs(b));
        }
    }
    HB_HD void handle_coin(int s, uint32_t t) {   // 357-365
        if (!(fl & BF_COIN_PROG)) return;
        ts_handle(s, t);
        on_coin_step();
    }
    HB_HD void handle_content(int s, uint32_t kind, uint32_t val, uint32_t tam) {   // 278-289
        switch (kind) {
            case BA_BVAL:
                sbv_handle_bval(s, val & 1u);
                handle_sbvb_step();
                break;
            case BA_AUX:
                sbv_handle_aux(s, val & 1u);
                handle_sbvb_step();
                break;
            case BA_CONF: handle_conf(s, val & 3u); break;
            case BA_TERM: handle_term(s, val & 1u); break;
            case BA_COIN: handle_coin(s, tam & 1u); break;
            default: break;
        }
    }
    // update_epoch (491-509) up to the replay
    HB_HD void update_epoch_head(uint32_t b) {
        for (int w = 0; w < W; ++w) {   // sbv.clear(received_term), received_conf from the Terms
            const uint32_t t0 = M(BM_TERM, w), t1 = M(BM_TERM + 1, w);
            M(BM_BVAL, w) = t0;
            M(BM_BVAL + 1, w) = t1;
            M(BM_AUX, w) = t0;
            M(BM_AUX + 1, w) = t1;
            M(BM_CONF_F, w) = t0 & ~t1;   // (`true` is inserted last)
            M(BM_CONF_T, w) = t1;
            M(BM_COIN, w) = 0;
        }
        fl &= BF_DEC_HAS | BF_DEC_VAL;
        ++epoch;
        const uint32_t m = epoch % 3u;   // coin_state (439-450): true, false, the coin
        if (m == 0) fl |= BF_COIN_VAL;
        else if (m == 2) {
            fl |= BF_COIN_PROG;
            if ((epoch - 2u) / 3u >= coins) bad |= BA_BAD_COINS;
        }
        fl |= BF_EST_HAS | (b ? BF_EST_VAL : 0u);
        sbv_send_bval(b);
        handle_sbvb_step();
    }
    // the pending update_epoch calls and handle_term continuations
    HB_HD void drain() {
        for (;;) {
            if (pend) {
                const uint32_t b = pend - 1u;
                pend = 0;
                update_epoch_head(b);
                if (pend) {
                    // our own BVal moved the epoch again (f = 0): the
                    // reference never looks at this epoch's queue again; the
                    // ring slot is wanted for a later epoch
                    for (int s = 0; s < n; ++s) ring[s * Q + (int)(epoch % (uint32_t)Q)] = 0;
                    continue;
                }
                // the queued messages of this epoch (510-518): senders in
                // ascending order, BVal(true), BVal(false), Aux(true),
                // Aux(false), Conf, Term, Coin each; the whole epoch is taken
                // out of the queue, the replay stops at a decision or update
                const int sl = (int)(epoch % (uint32_t)Q);
                bool stop = false;
                for (int s = 0; s < n; ++s) {
                    const uint32_t e = ring[s * Q + sl];
                    if (!e) continue;
                    ring[s * Q + sl] = 0;
                    if (stop) continue;
                    for (int i = 0; i < 7 && !stop; ++i) {
                        uint32_t kind, val = 0, tam = 0;
                        bool has;
                        if (i < 2) {
                            kind = BA_BVAL, val = 1u - i, has = (e >> BQ_BVAL_SHIFT) & bs(val);
                        } else if (i < 4) {
                            kind = BA_AUX, val = 3u - i, has = (e >> BQ_AUX_SHIFT) & bs(val);
                        } else if (i == 4) {
                            kind = BA_CONF, val = (e >> BQ_CONF_SHIFT) & 3u, has = e & BQ_CONF_HAS;
                        } else if (i == 5) {
                            kind = BA_TERM, val = (e & BQ_TERM_VAL) ? 1u : 0u, has = e & BQ_TERM_HAS;
                        } else {
                            kind = BA_COIN, tam = (e & BQ_COIN_TAMPER) ? 1u : 0u, has = e & BQ_COIN_HAS;
                        }
                        if (!has) continue;
                        handle_content(s, kind, val, tam);
                        if ((fl & BF_DEC_HAS) || pend) stop = true;
                    }
                }
                continue;
            }
            if (sp > 0) {
                const uint32_t c = cstack[--sp];
                handle_conf((int)(c >> 1), bs(c & 1u));
                continue;
            }
            break;
        }
    }
    // ReceivedMessages::insert (72-109)
    HB_HD void queue_insert(int s, uint32_t ep, uint32_t kind, uint32_t val, uint32_t tam) {
        uint16_t &q = ring[s * Q + (int)(ep % (uint32_t)Q)];
        uint32_t e = q;
        int fk = -1;
        switch (kind) {
            case BA_BVAL:
                if ((e >> BQ_BVAL_SHIFT) & bs(val & 1u)) fk = BAF_DUPLICATE_BVAL;
                else e |= bs(val & 1u) << BQ_BVAL_SHIFT;
                break;
            case BA_AUX:
                if ((e >> BQ_AUX_SHIFT) & bs(val & 1u)) fk = BAF_DUPLICATE_AUX;
                else e |= bs(val & 1u) << BQ_AUX_SHIFT;
                break;
            case BA_CONF:
                if (e & BQ_CONF_HAS) fk = BAF_MULTIPLE_CONF;
                else e |= BQ_CONF_HAS | ((val & 3u) << BQ_CONF_SHIFT);
                break;
            case BA_TERM:
                if (e & BQ_TERM_HAS) fk = BAF_MULTIPLE_TERM;
                else e |= BQ_TERM_HAS | ((val & 1u) ? BQ_TERM_VAL : 0u);
                break;
            case BA_COIN:
                if (e & BQ_COIN_HAS) fk = BAF_AGREEMENT_EPOCH;
                else e |= BQ_COIN_HAS | ((tam & 1u) ? BQ_COIN_TAMPER : 0u);
                break;
            default: return;
        }
        if (fk >= 0) fault(s, fk);
        else q = (uint16_t)e;
    }
    HB_HD void handle_message(int s, uint32_t h) {   // 245-269
        const uint32_t kind = h & 0xFFu, val = (h >> 8) & 0xFu, tam = (h >> 12) & 1u, ep = h >> 16;
        if ((fl & BF_DEC_HAS) || (ep < epoch && kind != BA_TERM)) return;   // obsolete
        if (ep > epoch + kBaMaxFuture) {
            fault(s, BAF_AGREEMENT_EPOCH);
            return;
        }
        if (ep > epoch) {
            if (ep - epoch > (uint32_t)Q) bad |= BA_BAD_QUEUE;   // beyond the ring: reject the run
            else queue_insert(s, ep, kind, val, tam);
            return;
        }
        handle_content(s, kind, val, tam);
        drain();
    }
    HB_HD void propose(uint32_t b) {   // 232-240
        if (epoch != 0 || (fl & BF_EST_HAS)) return;
        fl |= BF_EST_HAS | (b ? BF_EST_VAL : 0u);
        sbv_send_bval(b);
        handle_sbvb_step();
        drain();
    }
};

// One node's round: round 0 is propose(input), later rounds walk the
// instance's inbox sender by sender.  core: the node's word 0 (word i at
// core[i * cs]); ring: its future-epoch ring.  nout: records emitted; bad:
// the flags for emitted[1].
HB_HD void ba_node_round(const hbrbc_ba_args &a, size_t inst, int local, uint32_t *core, size_t cs,
                         uint16_t *ring, uint32_t &nout, uint32_t &bad) {
    const int n = (int)a.n, W = (n + 31) / 32;
    const size_t g = inst * n + local;
    const uint32_t rec = 1u + W;
    BaNode m;
    m.n = n;
    m.f = (n - 1) / 3;
    m.W = W;
    m.Q = (int)a.queue_epochs;
    m.me = local;
    m.role = a.role[g];
    m.coins = a.coins;
    m.ahead = a.ahead[inst];
    m.max_out = a.max_out;
    m.max_faults = a.max_faults;
    m.rec = rec;
    m.flip = a.flip + inst * W;
    m.sok = a.share_ok + inst * a.coins * 2 * n;
    m.coinv = a.coin + inst * a.coins;
    m.core = core;
    m.cs = cs;
    m.ring = ring;
    m.epoch = m.core[0];
    m.fl = m.core[m.cs];
    m.out = a.out + g * a.max_out * rec;
    m.nout = 0;
    m.faults = a.faults + g * a.max_faults;
    m.nfault = a.fault_count[g];
    m.bad = 0;
    m.decision = a.decision + g;
    m.decision_epoch = a.decision_epoch + g;
    m.sout = 0;
    m.ts_out = false;
    m.pend = 0;
    m.sp = 0;
    if (a.round == 0) {
        m.fl = BF_COIN_VAL;   // epoch 0: CoinState::Decided(true)
        const uint32_t inp = a.input[g];
        if (inp != HBRBC_BA_NONE) m.propose(inp & 1u);
    } else {
        const uint32_t *cnts = a.in_count + inst * n;
        const uint32_t *recs = a.in + inst * n * (size_t)a.max_out * rec;
        const int mw = 1 + (local >> 5);
        const uint32_t mb = 1u << (local & 31);
        for (int s = 0; s < n; ++s) {
            uint32_t c = cnts[s] & 0x7FFFFFFFu;
            c = c < a.max_out ? c : a.max_out;
            const uint32_t *r = recs + (size_t)s * a.max_out * rec;
            for (uint32_t e = 0; e < c; ++e, r += rec) {
                // (a node's own records do not name it: all_but_me)
                if (s != local && (r[mw] & mb)) m.handle_message(s, r[0]);
            }
        }
    }
    m.core[0] = m.epoch;
    m.core[m.cs] = m.fl;
    a.out_count[g] = m.nout | ((m.bad & BA_BAD_OUT) ? 0x80000000u : 0u);
    a.fault_count[g] = m.nfault;
    nout = m.nout;
    bad = m.bad;
}

}  // namespace hbrbc
