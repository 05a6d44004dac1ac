// api_pairing.hip -- the BLS12-381 entries of include/hbrbc.h: argument checks
// and launch sequencing over the typed table views of pairing_tables.hpp.
// Every group and field operation is computed by the kernels in pairing.hip
// (and hash_g2.hip, which is compiled with it).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/hbrbc.h"
#include "api_internal.hpp"
#include "pairing_tables.hpp"

using namespace hbrbc;

namespace {

// ---- threshold-decrypt share verification (pairing.hip) ----
int pairing_run(const uint8_t *g1, const uint8_t *g2, size_t n_pair, size_t n_out, int per_out,
                uint8_t *gt_out, uint8_t *ok_out, uint8_t *status_out, void *workspace,
                hipStream_t s) {
    if (int rc = have_device()) return rc;
    const PairWs ws = pair_ws(workspace, n_pair);
    const char *mm = getenv("HBRBC_PAIR_MULTI");   // 0: one lane per pairing (A/B)
    if (per_out == 2 && !(mm && !std::strcmp(mm, "0"))) {
        // checks: one lane per check, both Miller loops sharing f's squarings
        HB_HIP(launch_pairing_miller2(g1, g2, n_out, ws, s));
        HB_HIP(launch_pairing_final(ws, n_out, n_out, 1, gt_out, ok_out, s));
        return HBRBC_OK;
    }
    HB_HIP(launch_pairing_miller(g1, 96, g2, 192, n_pair, per_out == 2, ws, s));
    if (status_out)
        HB_HIP(hipMemcpyAsync(status_out, ws.status, n_pair, hipMemcpyDeviceToDevice, s));
    HB_HIP(launch_pairing_final(ws, n_pair, n_out, per_out, gt_out, ok_out, s));
    return HBRBC_OK;
}

// The five preparations: `count` encoded points into a table of that count.
template <class Kind>
int prepare_table(hipError_t (*launch)(const uint8_t *, TableOut<Kind>, hipStream_t),
                  const uint8_t *points, size_t count, void *table, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!points || !table) return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    HB_HIP(launch(points, view<Kind>(table, count), static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

// The tail of the prepared checks: the Miller launch's outcome, then one final
// exponentiation per check of `ws` into ok_out.
int check_final(hipError_t miller_launch, PairWs ws, size_t count, uint8_t *ok_out,
                hipStream_t s) {
    HB_HIP(miller_launch);
    HB_HIP(launch_pairing_final(ws, count, count, 1, nullptr, ok_out, s));
    return HBRBC_OK;
}

// ---- share combine (pairing.hip): the two groups of pairing_tables.hpp ------
hipError_t g1_reduce_encode_np(const uint32_t *ws, const uint8_t *pst, const uint32_t *offsets,
                               size_t groups, size_t total, const uint8_t *lst, uint8_t *out96,
                               uint8_t *out48, uint8_t *, uint8_t *status, hipStream_t s) {
    return launch_g1_reduce_encode(ws, pst, offsets, groups, total, lst, out96, out48, status, s);
}

const CombineGroup<G1Keys> kCombineG1 = {96, g1_point_words, hbrbc_g1_prepare,
                                         launch_g1_scalar_mul, g1_reduce_encode_np,
                                         "decrypt combine"};
const CombineGroup<G2Points> kCombineG2 = {192, g2_point_words, hbrbc_g2_points_prepare,
                                           launch_g2_scalar_mul, launch_g2_reduce_encode,
                                           "signature combine"};

// The share count is the last entry of the device-side prefix sum: one
// 4-byte read-back (and a wait for what precedes it on the stream) sizes the
// per-share launches; the kernels themselves are queued without waiting.
int combine_total(const uint32_t *offsets, size_t groups, hipStream_t s, size_t *total) {
    uint32_t v = 0;
    HB_HIP(hipMemcpyAsync(&v, offsets + groups, sizeof v, hipMemcpyDeviceToHost, s));
    HB_HIP(hipStreamSynchronize(s));
    *total = v;
    return HBRBC_OK;
}

// sum_j [k_j] T[rows[j]] per group, encoded.  The scalars are the caller's
// (`scalars`), or with `idx` the Lagrange coefficients at 0 of the node
// indices, computed into the workspace first.  `parity` is G2's alone.
template <class Kind>
int lincomb_run(const CombineGroup<Kind> &G, const void *table, size_t table_count,
                const int32_t *rows, const uint8_t *scalars, const uint32_t *idx,
                const uint32_t *offsets, size_t groups, uint8_t *out_u, uint8_t *out_c,
                uint8_t *parity, uint8_t *status_out, void *workspace, void *stream) {
    if (groups == 0) return HBRBC_OK;
    if (!table || !offsets || !out_u || !out_c || !status_out || !workspace)
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    size_t total = 0;
    if (int rc = combine_total(offsets, groups, s, &total)) return rc;
    if (total && (!rows || (!idx && !scalars)))
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    const CombineWs w = combine_ws(G, workspace, total);
    if (idx) {
        HB_HIP(hipMemsetAsync(w.lst, 0, groups, s));
        HB_HIP(launch_lagrange(idx, offsets, groups, total, w.coeffs, w.lst, s));
        scalars = w.coeffs;
    }
    HB_HIP(G.scalar_mul(view<Kind>(table, table_count), rows, scalars, total, w.pts, w.pst, s));
    HB_HIP(G.reduce_encode(w.pts, w.pst, offsets, groups, total, idx ? w.lst : nullptr, out_u,
                           out_c, parity, status_out, s));
    return HBRBC_OK;
}

// The per-call forms: one group of n shares with rows 0 .. n-1, prepared and
// combined in one device block; out gets the uncompressed encoding, the
// compressed one and the parity byte (3 G.enc / 2 + 1 bytes).
template <class Kind>
int combine_once(const CombineGroup<Kind> &G, const uint8_t *shares, const uint32_t *idx,
                 size_t n, uint8_t *out) {
    if (int rc = have_device()) return rc;
    // device block: shares | idx | rows | offsets | encodings, parity, status |
    // prepared table | workspace
    const size_t o_idx = round_up(n * G.enc, 256), o_rows = o_idx + round_up(n * 4, 256);
    const size_t o_off = o_rows + round_up(n * 4, 256), o_out = o_off + 256;
    const size_t o_tab = o_out + 512;
    const size_t o_ws = o_tab + table_size<Kind>(n);
    const size_t bytes = o_ws + combine_workspace_size(G, n, 1);
    const size_t o_par = G.enc * 3 / 2, o_st = o_par + 1;
    uint8_t *dev = nullptr;
    HB_HIP(hipMalloc(&dev, bytes));
    std::vector<uint8_t> host(o_tab, 0);   // the output block too: G1 writes no parity byte
    if (n) {
        memcpy(host.data(), shares, n * G.enc);
        memcpy(host.data() + o_idx, idx, n * 4);
    }
    for (size_t i = 0; i < n; ++i) {
        const int32_t r = (int32_t)i;
        memcpy(host.data() + o_rows + 4 * i, &r, 4);
    }
    const uint32_t offs[2] = {0, (uint32_t)n};
    memcpy(host.data() + o_off, offs, sizeof offs);
    uint8_t res[512] = {0};
    int rc = HBRBC_OK;
    hipError_t e = hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = G.prepare(dev, n, dev + o_tab, nullptr);
        if (rc == HBRBC_OK)
            rc = lincomb_run(G, dev + o_tab, n, reinterpret_cast<const int32_t *>(dev + o_rows),
                             nullptr, reinterpret_cast<const uint32_t *>(dev + o_idx),
                             reinterpret_cast<const uint32_t *>(dev + o_off), 1, dev + o_out,
                             dev + o_out + G.enc, dev + o_out + o_par, dev + o_out + o_st,
                             dev + o_ws, nullptr);
        if (rc == HBRBC_OK) e = hipMemcpy(res, dev + o_out, o_st + 1, hipMemcpyDeviceToHost);
    }
    (void)hipFree(dev);
    if (e != hipSuccess) return fail(HBRBC_E_DEVICE, "%s: %s", G.what, hipGetErrorString(e));
    if (rc != HBRBC_OK) return rc;
    if (res[o_st] == 3) return fail(HBRBC_E_INVALID_ARG, "duplicate share index");
    if (res[o_st] == 2) return fail(HBRBC_E_INVALID_ARG, "invalid curve point");
    memcpy(out, res, o_st);
    return HBRBC_OK;
}

}  // namespace

extern "C" {

// ---- table and workspace sizes (the layouts of pairing_tables.hpp) ---------
size_t hbrbc_g1_prepared_size(size_t points) { return table_size<G1Keys>(points); }
size_t hbrbc_g2_prepared_size(size_t points) { return table_size<G2Lines>(points); }
size_t hbrbc_g2_points_size(size_t points) { return table_size<G2Points>(points); }

size_t hbrbc_pairing_workspace_size(size_t pairings) {
    return pair_ws_status_offset(pairings) + round_up(pairings, 256);
}

size_t hbrbc_g1_combine_workspace_size(size_t total_shares, size_t groups) {
    return combine_workspace_size(kCombineG1, total_shares, groups);
}

size_t hbrbc_g2_combine_workspace_size(size_t total_shares, size_t groups) {
    return combine_workspace_size(kCombineG2, total_shares, groups);
}

// ---- threshold-decrypt share verification ----------------------------------
int hbrbc_pairing_batch(const uint8_t *g1, const uint8_t *g2, size_t count, uint8_t *gt_out,
                        uint8_t *status_out, void *workspace, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!g1 || !g2 || !gt_out || !workspace) return fail(HBRBC_E_INVALID_ARG, "null argument");
    return pairing_run(g1, g2, count, count, 1, gt_out, nullptr, status_out, workspace,
                       static_cast<hipStream_t>(stream));
}

int hbrbc_pairing_check_batch(const uint8_t *g1, const uint8_t *g2, size_t count,
                              uint8_t *ok_out, void *workspace, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!g1 || !g2 || !ok_out || !workspace) return fail(HBRBC_E_INVALID_ARG, "null argument");
    return pairing_run(g1, g2, 2 * count, count, 2, nullptr, ok_out, nullptr, workspace,
                       static_cast<hipStream_t>(stream));
}

int hbrbc_g2_prepare(const uint8_t *g2, size_t count, void *prepared, void *stream) {
    return prepare_table<G2Lines>(launch_g2_prepare, g2, count, prepared, stream);
}

int hbrbc_g1_prepare(const uint8_t *g1, size_t count, void *prepared, void *stream) {
    return prepare_table<G1Keys>(launch_g1_prepare, g1, count, prepared, stream);
}

int hbrbc_pairing_check_prepared(const uint8_t *g1, const void *prepared, size_t points,
                                 const uint32_t *idx_b, const uint32_t *idx_d, size_t count,
                                 uint8_t *ok_out, void *workspace, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!g1 || !prepared || !idx_b || !idx_d || !ok_out || !workspace)
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    if (points == 0) return fail(HBRBC_E_INVALID_ARG, "no prepared points");
    const PairWs ws = pair_ws(workspace, count);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return check_final(launch_pairing_miller_prepared(g1, view<G2Lines>(prepared, points), idx_b,
                                                      idx_d, count, ws, s),
                       ws, count, ok_out, s);
}

int hbrbc_pairing_check_prepared_keys(const uint8_t *g1_a, const void *keys, size_t key_points,
                                      const uint32_t *idx_c, const void *prepared, size_t points,
                                      const uint32_t *idx_b, const uint32_t *idx_d, size_t count,
                                      uint8_t *ok_out, void *workspace, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!g1_a || !keys || !idx_c || !prepared || !idx_b || !idx_d || !ok_out || !workspace)
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (points == 0) return fail(HBRBC_E_INVALID_ARG, "no prepared points");
    if (key_points == 0) return fail(HBRBC_E_INVALID_ARG, "no prepared keys");
    if (int rc = have_device()) return rc;
    const PairWs ws = pair_ws(workspace, count);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return check_final(
        launch_pairing_miller_prepared_keys(g1_a, view<G1Keys>(keys, key_points), idx_c,
                                            view<G2Lines>(prepared, points), idx_b, idx_d, count,
                                            ws, s),
        ws, count, ok_out, s);
}

int hbrbc_pairing_check_prepared_pts(const void *a_prepared, const void *keys, size_t key_points,
                                     const uint32_t *idx_c, const void *prepared, size_t points,
                                     const uint32_t *idx_b, const uint32_t *idx_d, size_t count,
                                     uint8_t *ok_out, void *workspace, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!a_prepared || !keys || !idx_c || !prepared || !idx_b || !idx_d || !ok_out || !workspace)
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (points == 0) return fail(HBRBC_E_INVALID_ARG, "no prepared points");
    if (key_points == 0) return fail(HBRBC_E_INVALID_ARG, "no prepared keys");
    if (int rc = have_device()) return rc;
    const PairWs ws = pair_ws(workspace, count);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return check_final(
        launch_pairing_miller_prepared_pts(view<G1Keys>(a_prepared, count),
                                           view<G1Keys>(keys, key_points), idx_c,
                                           view<G2Lines>(prepared, points), idx_b, idx_d, count,
                                           ws, s),
        ws, count, ok_out, s);
}

int hbrbc_pairing_check(const uint8_t a[96], const uint8_t b[192], const uint8_t c[96],
                        const uint8_t d[192], int *result) {
    if (!a || !b || !c || !d || !result) return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    const size_t ws_bytes = hbrbc_pairing_workspace_size(2);
    const size_t total = 2 * 96 + 2 * 192 + 16 + ws_bytes;
    uint8_t *dev = nullptr;
    HB_HIP(hipMalloc(&dev, total));
    std::vector<uint8_t> host(2 * 96 + 2 * 192);
    memcpy(host.data(), a, 96);
    memcpy(host.data() + 96, c, 96);
    memcpy(host.data() + 192, b, 192);
    memcpy(host.data() + 384, d, 192);
    uint8_t ok = 0;
    int rc = HBRBC_OK;
    hipError_t e = hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = pairing_run(dev, dev + 192, 2, 1, 2, nullptr, dev + 576, nullptr, dev + 592,
                         nullptr);
        if (rc == HBRBC_OK) e = hipMemcpy(&ok, dev + 576, 1, hipMemcpyDeviceToHost);
    }
    (void)hipFree(dev);
    if (e != hipSuccess) return fail(HBRBC_E_DEVICE, "pairing check: %s", hipGetErrorString(e));
    if (rc != HBRBC_OK) return rc;
    if (ok == 2) return fail(HBRBC_E_INVALID_ARG, "invalid curve point");
    *result = ok;
    return HBRBC_OK;
}

// ---- share combine: PublicKeySet::decrypt up to g --------------------------
int hbrbc_lagrange_coeffs(const uint32_t *idx, const uint32_t *offsets, size_t groups,
                          uint8_t *coeffs_out, uint8_t *status_out, void *stream) {
    if (groups == 0) return HBRBC_OK;
    if (!offsets || !status_out) return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    size_t total = 0;
    if (int rc = combine_total(offsets, groups, s, &total)) return rc;
    if (total && (!idx || !coeffs_out)) return fail(HBRBC_E_INVALID_ARG, "null argument");
    HB_HIP(hipMemsetAsync(status_out, 0, groups, s));
    HB_HIP(launch_lagrange(idx, offsets, groups, total, coeffs_out, status_out, s));
    return HBRBC_OK;
}

int hbrbc_g1_lincomb_prepared(const void *a_prepared, size_t prepared_count, const int32_t *rows,
                              const uint8_t *scalars, const uint32_t *offsets, size_t groups,
                              uint8_t *out96, uint8_t *out48, uint8_t *status_out,
                              void *workspace, void *stream) {
    return lincomb_run(kCombineG1, a_prepared, prepared_count, rows, scalars, nullptr, offsets,
                       groups, out96, out48, nullptr, status_out, workspace, stream);
}

int hbrbc_decrypt_combine_prepared(const void *a_prepared, size_t prepared_count,
                                   const int32_t *rows, const uint32_t *idx,
                                   const uint32_t *offsets, size_t groups, uint8_t *out96,
                                   uint8_t *out48, uint8_t *status_out, void *workspace,
                                   void *stream) {
    return lincomb_run(kCombineG1, a_prepared, prepared_count, rows, nullptr, idx, offsets,
                       groups, out96, out48, nullptr, status_out, workspace, stream);
}

int hbrbc_decrypt_combine(const uint8_t *shares, const uint32_t *idx, size_t n, uint8_t out96[96],
                          uint8_t out48[48]) {
    if (!out96 || !out48 || (n && (!shares || !idx)))
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    uint8_t out[145];
    if (int rc = combine_once(kCombineG1, shares, idx, n, out)) return rc;
    memcpy(out96, out, 96);
    memcpy(out48, out + 96, 48);
    return HBRBC_OK;
}

// ---- key generation (pairing.hip): SyncKeyGen's commitment evaluations ------
int hbrbc_g1_poly_eval_prepared(const void *a_prepared, size_t prepared_count, const int32_t *rows,
                                const uint32_t *offsets, size_t polys, const int32_t *poly,
                                const uint32_t *x, size_t evals, void *out_table, uint8_t *out96,
                                uint8_t *out48, uint8_t *status_out, void *stream) {
    if (evals == 0) return HBRBC_OK;
    if (!a_prepared || !rows || !offsets || !poly || !x || !out_table || !status_out)
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_g1_horner(view<G1Keys>(a_prepared, prepared_count), rows, offsets, polys, poly,
                            x, view<G1Keys>(out_table, evals), out96, out48, status_out,
                            static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

int hbrbc_g1_base_mul_check(const void *a_prepared, size_t prepared_count, const int32_t *rows,
                            const uint8_t *scalars, size_t count, uint8_t *ok_out, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!a_prepared || !rows || !scalars || !ok_out)
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_g1_base_mul_check(view<G1Keys>(a_prepared, prepared_count), rows, scalars, count,
                                    ok_out, static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

// ---- threshold signatures (pairing.hip): ThresholdSign, the coin ----------
int hbrbc_g2_points_prepare(const uint8_t *g2, size_t count, void *table, void *stream) {
    return prepare_table<G2Points>(launch_g2_points, g2, count, table, stream);
}

// ---- compressed wire encodings (pairing.hip) -------------------------------
int hbrbc_g1_prepare_compressed(const uint8_t *g1c, size_t count, void *prepared, void *stream) {
    return prepare_table<G1Keys>(launch_g1_prepare_compressed, g1c, count, prepared, stream);
}

int hbrbc_g2_points_prepare_compressed(const uint8_t *g2c, size_t count, void *table,
                                       void *stream) {
    return prepare_table<G2Points>(launch_g2_points_compressed, g2c, count, table, stream);
}

int hbrbc_g1_decompress(const uint8_t *g1c, size_t count, uint8_t *out96, uint8_t *status,
                        void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!g1c || !out96 || !status) return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_g1_decompress(g1c, count, out96, status, static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

int hbrbc_g2_decompress(const uint8_t *g2c, size_t count, uint8_t *out192, uint8_t *status,
                        void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!g2c || !out192 || !status) return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_g2_decompress(g2c, count, out192, status, static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

int hbrbc_sig_check_prepared(const void *sig_table, size_t sig_count, const void *keys,
                             size_t key_points, const uint32_t *idx_key, const void *prepared,
                             size_t points, const uint32_t *idx_h, size_t count, uint8_t *ok_out,
                             void *workspace, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!sig_table || !keys || !idx_key || !prepared || !idx_h || !ok_out || !workspace)
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (points == 0) return fail(HBRBC_E_INVALID_ARG, "no prepared points");
    if (key_points == 0) return fail(HBRBC_E_INVALID_ARG, "no prepared keys");
    if (sig_count == 0) return fail(HBRBC_E_INVALID_ARG, "no signature shares");
    if (int rc = have_device()) return rc;
    const PairWs ws = pair_ws(workspace, count);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return check_final(
        launch_pairing_miller_sig(view<G2Points>(sig_table, sig_count),
                                  view<G1Keys>(keys, key_points), idx_key,
                                  view<G2Lines>(prepared, points), idx_h, count, ws, s),
        ws, count, ok_out, s);
}

int hbrbc_g2_lincomb_prepared(const void *sig_table, size_t sig_count, const int32_t *rows,
                              const uint8_t *scalars, const uint32_t *offsets, size_t groups,
                              uint8_t *out192, uint8_t *out96, uint8_t *parity_out,
                              uint8_t *status_out, void *workspace, void *stream) {
    if (groups && !parity_out) return fail(HBRBC_E_INVALID_ARG, "null argument");
    return lincomb_run(kCombineG2, sig_table, sig_count, rows, scalars, nullptr, offsets, groups,
                       out192, out96, parity_out, status_out, workspace, stream);
}

int hbrbc_sig_combine_prepared(const void *sig_table, size_t sig_count, const int32_t *rows,
                               const uint32_t *idx, const uint32_t *offsets, size_t groups,
                               uint8_t *out192, uint8_t *out96, uint8_t *parity_out,
                               uint8_t *status_out, void *workspace, void *stream) {
    if (groups && !parity_out) return fail(HBRBC_E_INVALID_ARG, "null argument");
    return lincomb_run(kCombineG2, sig_table, sig_count, rows, nullptr, idx, offsets, groups,
                       out192, out96, parity_out, status_out, workspace, stream);
}

int hbrbc_sig_combine(const uint8_t *shares, const uint32_t *idx, size_t n, uint8_t out192[192],
                      uint8_t out96[96], uint8_t *parity) {
    if (!out192 || !out96 || !parity || (n && (!shares || !idx)))
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    uint8_t out[289];
    if (int rc = combine_once(kCombineG2, shares, idx, n, out)) return rc;
    memcpy(out192, out, 192);
    memcpy(out96, out + 192, 96);
    *parity = out[288];
    return HBRBC_OK;
}

// ---- share creation (pairing.hip): multiplications with a result, Fr --------
int hbrbc_g1_base_mul(const uint8_t *scalars, size_t count, void *out_table, uint8_t *out96,
                      uint8_t *out48, uint8_t *status_out, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!scalars || !out_table || !status_out) return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_g1_base_mul(scalars, view<G1Keys>(out_table, count), out96, out48, status_out,
                              static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

int hbrbc_g1_mul_prepared(const void *a_prepared, size_t prepared_count, const int32_t *rows,
                          const uint8_t *scalars, size_t nscalars, const int32_t *sidx,
                          size_t count, void *out_table, uint8_t *out96, uint8_t *out48,
                          uint8_t *status_out, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!a_prepared || !rows || !scalars || !out_table || !status_out)
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (!sidx && nscalars < count)
        return fail(HBRBC_E_INVALID_ARG, "without sidx every result needs a scalar of its own");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_g1_mul_table(view<G1Keys>(a_prepared, prepared_count), rows, scalars, nscalars,
                               sidx, view<G1Keys>(out_table, count), out96, out48, status_out,
                               static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

int hbrbc_g2_mul_prepared(const void *table, size_t table_count, const int32_t *rows,
                          const uint8_t *scalars, size_t nscalars, const int32_t *sidx,
                          size_t count, void *out_table, uint8_t *out192, uint8_t *out96,
                          uint8_t *status_out, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!table || !rows || !scalars || !out_table || !status_out)
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (!sidx && nscalars < count)
        return fail(HBRBC_E_INVALID_ARG, "without sidx every result needs a scalar of its own");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_g2_mul_table(view<G2Points>(table, table_count), rows, scalars, nscalars, sidx,
                               view<G2Points>(out_table, count), out192, out96, status_out,
                               static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

int hbrbc_fr_poly_eval(const uint8_t *scalars, size_t nscalars, const int32_t *rows,
                       const uint32_t *offsets, size_t polys, const int32_t *poly,
                       const uint32_t *x, size_t evals, uint8_t *out, uint8_t *status_out,
                       void *stream) {
    if (evals == 0) return HBRBC_OK;
    if (!scalars || !rows || !offsets || !poly || !x || !out || !status_out)
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_fr_horner(scalars, nscalars, rows, offsets, polys, poly, x, evals, out,
                            status_out, static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

int hbrbc_fr_dot(const uint8_t *a, const uint8_t *b, const uint32_t *offsets, size_t groups,
                 size_t total, uint8_t *out, uint8_t *status_out, void *stream) {
    if (groups == 0) return HBRBC_OK;
    if (!offsets || !out || !status_out || (total && (!a || !b)))
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_fr_dot(a, b, offsets, groups, total, out, status_out,
                         static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

// ---- hashes and the pad (hash_g2.hip) --------------------------------------
static int hash_g2_run(const uint8_t *u48, bool with_u, const uint8_t *msgs,
                       const uint32_t *offsets, size_t count, size_t total, void *out_table,
                       uint8_t *out192, uint8_t *out96, uint8_t *status_out, uint32_t *words_out,
                       void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!offsets || !out_table || !status_out || (with_u && !u48) || (total && !msgs))
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (total > 0xFFFFFFFFull) return fail(HBRBC_E_INVALID_ARG, "total exceeds 32-bit offsets");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_hash_g2(u48, msgs, offsets, total, view<G2Points>(out_table, count), out192,
                          out96, status_out, words_out, static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

int hbrbc_hash_g2_batch(const uint8_t *msgs, const uint32_t *offsets, size_t count, size_t total,
                        void *out_table, uint8_t *out192, uint8_t *out96, uint8_t *status_out,
                        uint32_t *words_out, void *stream) {
    return hash_g2_run(nullptr, false, msgs, offsets, count, total, out_table, out192, out96,
                       status_out, words_out, stream);
}

int hbrbc_hash_g1_g2_batch(const uint8_t *u48, const uint8_t *msgs, const uint32_t *offsets,
                           size_t count, size_t total, void *out_table, uint8_t *out192,
                           uint8_t *out96, uint8_t *status_out, uint32_t *words_out,
                           void *stream) {
    return hash_g2_run(u48, true, msgs, offsets, count, total, out_table, out192, out96,
                       status_out, words_out, stream);
}

size_t hbrbc_xor_with_hash_workspace_size(size_t count) { return round_up(count * 32, 256); }

int hbrbc_xor_with_hash_batch(const uint8_t *g48, const uint8_t *data, const uint32_t *offsets,
                              size_t count, size_t total, uint8_t *out, uint8_t *status_out,
                              void *workspace, void *stream) {
    if (count == 0) return HBRBC_OK;
    if (!g48 || !offsets || !status_out || !workspace || (total && (!data || !out)))
        return fail(HBRBC_E_INVALID_ARG, "null argument");
    if (total > 0xFFFFFFFFull) return fail(HBRBC_E_INVALID_ARG, "total exceeds 32-bit offsets");
    if (int rc = have_device()) return rc;
    HB_HIP(launch_xor_with_hash(g48, data, offsets, count, total, out, status_out,
                                static_cast<uint32_t *>(workspace),
                                static_cast<hipStream_t>(stream)));
    return HBRBC_OK;
}

}  // extern "C"
