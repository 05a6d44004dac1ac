// pairing_tables.hpp -- the host layer of pairing.hip: the layout of the
// prepared point tables and of the workspaces, as typed views, and the launch
// wrappers that take them.  Internal to libhbrbc.so; included by pairing.hip
// (with hash_g2.hip) and api_pairing.hip only.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "api_internal.hpp"

namespace hbrbc {

// ---- prepared tables ------------------------------------------------------
// A table of `count` points is Kind::words(count) 32-bit coordinate words,
// padded to 256 bytes, then one status byte per point (0 ok, 1 infinity,
// 2 invalid), padded to 256 bytes.  The three kinds (words per point are
// pairing.hip's):
size_t g1_key_words(size_t points);
size_t pairing_prepared_words(size_t points);
size_t g2_point_table_words(size_t points);
// hbrbc_g1_prepare*: affine G1 points
struct G1Keys { static size_t words(size_t n) { return g1_key_words(n); } };
// hbrbc_g2_prepare: the Miller-loop lines of G2 points
struct G2Lines { static size_t words(size_t n) { return pairing_prepared_words(n); } };
// hbrbc_g2_points_prepare*: affine G2 points
struct G2Points { static size_t words(size_t n) { return g2_point_table_words(n); } };

template <class Kind> size_t table_status_offset(size_t count) {
    return round_up(Kind::words(count) * 4, 256);
}
template <class Kind> size_t table_size(size_t count) {
    return table_status_offset<Kind>(count) + round_up(count, 256);
}

// `count` is the count the table was prepared with: it places `status`.
template <class Kind> struct Table { const uint32_t *words; const uint8_t *status; size_t count; };
template <class Kind> struct TableOut { uint32_t *words; uint8_t *status; size_t count; };

template <class Kind> Table<Kind> view(const void *table, size_t count) {
    return {static_cast<const uint32_t *>(table),
            static_cast<const uint8_t *>(table) + table_status_offset<Kind>(count), count};
}
template <class Kind> TableOut<Kind> view(void *table, size_t count) {
    return {static_cast<uint32_t *>(table),
            static_cast<uint8_t *>(table) + table_status_offset<Kind>(count), count};
}

// ---- Miller workspace -----------------------------------------------------
// The Miller values of `pairings` loops (limb-major, 576 bytes each), then
// one status byte per pairing.
struct PairWs { uint32_t *gt; uint8_t *status; };
inline size_t pair_ws_status_offset(size_t pairings) { return round_up(pairings * 576, 256); }
inline PairWs pair_ws(void *workspace, size_t pairings) {
    return {static_cast<uint32_t *>(workspace),
            static_cast<uint8_t *>(workspace) + pair_ws_status_offset(pairings)};
}

// BLS12-381 pairing checks (pairing.hip)
hipError_t launch_pairing_miller(const uint8_t *g1, size_t g1_stride, const uint8_t *g2,
                                 size_t g2_stride, size_t n, int pair_inputs, PairWs ws,
                                 hipStream_t s);
hipError_t launch_pairing_miller2(const uint8_t *g1, const uint8_t *g2, size_t count, PairWs ws,
                                  hipStream_t s);
hipError_t launch_g2_prepare(const uint8_t *g2, TableOut<G2Lines> prep, hipStream_t s);
hipError_t launch_pairing_miller_prepared(const uint8_t *g1, Table<G2Lines> prep,
                                          const uint32_t *ib, const uint32_t *id, size_t count,
                                          PairWs ws, hipStream_t s);
hipError_t launch_pairing_miller_prepared_pts(Table<G1Keys> a, Table<G1Keys> keys,
                                              const uint32_t *ic, Table<G2Lines> prep,
                                              const uint32_t *ib, const uint32_t *id, size_t count,
                                              PairWs ws, hipStream_t s);
hipError_t launch_g1_prepare(const uint8_t *g1, TableOut<G1Keys> keys, hipStream_t s);
hipError_t launch_pairing_miller_prepared_keys(const uint8_t *g1_a, Table<G1Keys> keys,
                                               const uint32_t *ic, Table<G2Lines> prep,
                                               const uint32_t *ib, const uint32_t *id, size_t count,
                                               PairWs ws, hipStream_t s);
hipError_t launch_pairing_final(PairWs ws, size_t n_miller, size_t n_out, int per_out,
                                uint8_t *gt_out, uint8_t *ok_out, hipStream_t s);
// decryption-share combine (pairing.hip): Lagrange coefficients, [k] P per
// share from a g1_prepare table into a limb-major workspace of
// g1_point_words(total) words, per-group sum and encodings
size_t g1_point_words(size_t shares);
hipError_t launch_lagrange(const uint32_t *idx, const uint32_t *offsets, size_t groups,
                           size_t total, uint8_t *coeffs, uint8_t *status, hipStream_t s);
hipError_t launch_g1_scalar_mul(Table<G1Keys> tab, const int32_t *rows, const uint8_t *scalars,
                                size_t total, uint32_t *ws, uint8_t *pst, hipStream_t s);
hipError_t launch_g1_reduce_encode(const uint32_t *ws, const uint8_t *pst, const uint32_t *offsets,
                                   size_t groups, size_t total, const uint8_t *lst, uint8_t *out96,
                                   uint8_t *out48, uint8_t *status, hipStream_t s);
// key generation (pairing.hip): ragged G1 polynomials over a g1_prepare table
// evaluated at small integers (Horner), out.count results in table form and
// optionally encoded; fixed-base checks [s] G1::one() == T[row]
hipError_t launch_g1_horner(Table<G1Keys> tab, const int32_t *rows, const uint32_t *offsets,
                            size_t polys, const int32_t *poly, const uint32_t *x,
                            TableOut<G1Keys> out, uint8_t *out96, uint8_t *out48, uint8_t *status,
                            hipStream_t s);
hipError_t launch_g1_base_mul_check(Table<G1Keys> tab, const int32_t *rows, const uint8_t *scalars,
                                    size_t count, uint8_t *ok, hipStream_t s);
// threshold signatures (pairing.hip): decoded G2 points (a g2_points table),
// the share check e(K, P) == e(G1::one(), S) with S from that table, [k] Q per
// share into a limb-major workspace of g2_point_words(total) words, per-group
// sum, encodings and parity
size_t g2_point_words(size_t shares);
hipError_t launch_g2_points(const uint8_t *g2, TableOut<G2Points> tab, hipStream_t s);
hipError_t launch_pairing_miller_sig(Table<G2Points> sig, Table<G1Keys> keys, const uint32_t *ic,
                                     Table<G2Lines> prep, const uint32_t *ih, size_t count,
                                     PairWs ws, hipStream_t s);
hipError_t launch_g2_scalar_mul(Table<G2Points> tab, const int32_t *rows, const uint8_t *scalars,
                                size_t total, uint32_t *ws, uint8_t *pst, hipStream_t s);
hipError_t launch_g2_reduce_encode(const uint32_t *ws, const uint8_t *pst, const uint32_t *offsets,
                                   size_t groups, size_t total, const uint8_t *lst,
                                   uint8_t *out192, uint8_t *out96, uint8_t *parity,
                                   uint8_t *status, hipStream_t s);
// share creation (pairing.hip): [scalars[sidx[j]]] T[rows[j]] over a g1_prepare
// / g2_points table and [s] G1::one(), out.count results in table form and
// optionally encoded; ragged Fr polynomials evaluated at 32-bit integers and
// ragged Fr dot products, 32 big-endian bytes per scalar
hipError_t launch_g1_mul_table(Table<G1Keys> tab, const int32_t *rows, const uint8_t *scalars,
                               size_t nscalars, const int32_t *sidx, TableOut<G1Keys> out,
                               uint8_t *out96, uint8_t *out48, uint8_t *status, hipStream_t s);
hipError_t launch_g2_mul_table(Table<G2Points> tab, const int32_t *rows, const uint8_t *scalars,
                               size_t nscalars, const int32_t *sidx, TableOut<G2Points> out,
                               uint8_t *out192, uint8_t *out96, uint8_t *status, hipStream_t s);
hipError_t launch_g1_base_mul(const uint8_t *scalars, TableOut<G1Keys> out, uint8_t *out96,
                              uint8_t *out48, uint8_t *status, hipStream_t s);
hipError_t launch_fr_horner(const uint8_t *scalars, size_t nscalars, const int32_t *rows,
                            const uint32_t *offsets, size_t polys, const int32_t *poly,
                            const uint32_t *x, size_t evals, uint8_t *out, uint8_t *status,
                            hipStream_t s);
hipError_t launch_fr_dot(const uint8_t *a, const uint8_t *b, const uint32_t *offsets,
                         size_t groups, size_t total, uint8_t *out, uint8_t *status,
                         hipStream_t s);
// compressed wire encodings (pairing.hip): the g1_prepare / g2_points tables
// from 48- / 96-byte points, and compressed to uncompressed bytes with a
// status byte per point (0 ok, 1 infinity, 2 invalid)
hipError_t launch_g1_prepare_compressed(const uint8_t *g1c, TableOut<G1Keys> keys, hipStream_t s);
hipError_t launch_g2_points_compressed(const uint8_t *g2c, TableOut<G2Points> tab, hipStream_t s);
hipError_t launch_g1_decompress(const uint8_t *g1c, size_t count, uint8_t *out96, uint8_t *status,
                                hipStream_t s);
hipError_t launch_g2_decompress(const uint8_t *g2c, size_t count, uint8_t *out192,
                                uint8_t *status, hipStream_t s);
// hashes and the pad (hash_g2.hip, compiled with pairing.hip): hash_g2 of the
// ragged messages msgs[offsets[i] .. offsets[i + 1]) (with u48: hash_g1_g2, 48
// bytes per item) into a g2_points table and optionally encoded, the stream
// words drawn per item (nullable); xor_with_hash of ragged rows with the
// stream of 48 bytes per row, `seeds` holding 8 words per row
hipError_t launch_hash_g2(const uint8_t *u48, const uint8_t *msgs, const uint32_t *offsets,
                          size_t total, TableOut<G2Points> out, uint8_t *out192, uint8_t *out96,
                          uint8_t *status, uint32_t *words, hipStream_t s);
hipError_t launch_xor_with_hash(const uint8_t *g48, const uint8_t *data, const uint32_t *offsets,
                                size_t count, size_t total, uint8_t *out, uint8_t *status,
                                uint32_t *seeds, hipStream_t s);

// ---- share combine: PublicKeySet::decrypt up to g in G1, combine_signatures
// in G2.  The two differ in table kind, sizes and launchers only:
template <class Kind> struct CombineGroup {
    size_t enc;                           // bytes of the uncompressed encoding (compressed: half)
    size_t (*point_words)(size_t);        // projective workspace points
    int (*prepare)(const uint8_t *, size_t, void *, void *);
    hipError_t (*scalar_mul)(Table<Kind>, const int32_t *, const uint8_t *, size_t, uint32_t *,
                             uint8_t *, hipStream_t);
    decltype(&launch_g2_reduce_encode) reduce_encode;   // G1 writes no parity byte
    const char *what;
};

// workspace: projective points (limb-major), per-share status, coefficients,
// per-group Lagrange status
struct CombineWs {
    uint32_t *pts;
    uint8_t *pst, *coeffs, *lst;
};

template <class Kind>
CombineWs combine_ws(const CombineGroup<Kind> &G, void *workspace, size_t total) {
    uint8_t *p = static_cast<uint8_t *>(workspace);
    CombineWs w;
    w.pts = reinterpret_cast<uint32_t *>(p);
    p += round_up(G.point_words(total) * 4, 256);
    w.pst = p;
    p += round_up(total, 256);
    w.coeffs = p;
    p += round_up(total * 32, 256);
    w.lst = p;
    return w;
}

template <class Kind>
size_t combine_workspace_size(const CombineGroup<Kind> &G, size_t total_shares, size_t groups) {
    return round_up(G.point_words(total_shares) * 4, 256) + round_up(total_shares, 256) +
           round_up(total_shares * 32, 256) + round_up(groups, 256);
}

}  // namespace hbrbc
