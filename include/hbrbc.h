/*
 * hbrbc.h -- C ABI of the MI355X Reliable-Broadcast data path (libhbrbc.so).
 *
 * Drop-in boundary for hbbft's `broadcast` data work (reference:
 * yangl1996/hbbft, /root/reference).  The reference has no FFI of its own:
 * its seam is the private enum `Coding` (src/broadcast/broadcast.rs:639-694)
 * and the crate-private module `merkle` (src/broadcast/merkle.rs, exported at
 * src/broadcast/mod.rs:224).  Every entry point below names the reference
 * item it replaces.  INTEGRATION.md shows the Rust `extern "C"` binding that
 * `Coding`/`MerkleTree`/`Proof` delegate to.
 *
 * Two layers:
 *  1. Per-call shims on HOST memory with exactly the reference semantics
 *     (same argument meaning, same rse::Error outcomes).  They stage through
 *     the device and run the same HIP kernels as the batched layer.
 *  2. Batched entry points on DEVICE memory for thousands of independent
 *     broadcast instances per call (the hot path).  All are asynchronous on
 *     the given stream (a hipStream_t; NULL = the HIP null stream) and
 *     never allocate, free or synchronise unless documented.
 *
 * Batched layout ("shard slab"): instance `i`, shard `j`, byte `b` lives at
 *   shards + i*inst_stride + j*shard_stride + b,
 * 0 <= b < shard_len.  Requirements: shard_stride % 16 == 0,
 * shard_stride >= shard_len, inst_stride % 16 == 0,
 * inst_stride >= n_shards*shard_stride, base 16-byte aligned.  Bytes in
 * [shard_len, round_up(shard_len,16)) of a row are padding: the coding
 * kernels read and write them, hashing never covers them.
 *
 * Merkle node slab: instance `i` owns `hbrbc_merkle_node_count(n)` 32-byte
 * nodes at nodes + i*node_inst_stride: level 0 (the n leaf digests), level 1
 * (ceil(n/2)), ..., the root last.  This is `MerkleTree::levels` plus
 * `root_hash` of merkle.rs:12-16 flattened.
 *
 * Errors: every function returns an `int` status.  No exception and no
 * abort crosses this ABI.  Ownership: the caller owns every buffer passed in.
 */
#ifndef HBRBC_H
#define HBRBC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------- */
/* 1..13 mirror reed_solomon_erasure::Error (4.0.x) in declaration order;  */
/* hbbft maps all of them to `Error::InvalidNodeCount` at construction      */
/* (broadcast.rs:101) and to `FaultKind::BroadcastDecoding` on reconstruct  */
/* (broadcast.rs:551-557, 569).                                             */
enum hbrbc_status {
    HBRBC_OK = 0,
    HBRBC_E_TOO_FEW_SHARDS = 1,
    HBRBC_E_TOO_MANY_SHARDS = 2,
    HBRBC_E_TOO_FEW_DATA_SHARDS = 3,
    HBRBC_E_TOO_MANY_DATA_SHARDS = 4,
    HBRBC_E_TOO_FEW_PARITY_SHARDS = 5,
    HBRBC_E_TOO_MANY_PARITY_SHARDS = 6,
    HBRBC_E_TOO_FEW_BUFFER_SHARDS = 7,
    HBRBC_E_TOO_MANY_BUFFER_SHARDS = 8,
    HBRBC_E_INCORRECT_SHARD_SIZE = 9,
    HBRBC_E_TOO_FEW_SHARDS_PRESENT = 10,
    HBRBC_E_EMPTY_SHARD = 11,
    HBRBC_E_INVALID_SHARD_FLAGS = 12,
    HBRBC_E_INVALID_INDEX = 13,
    /* decode outcomes of decode_from_shards (broadcast.rs:563-601) */
    HBRBC_E_SINGULAR_MATRIX = 64,
    HBRBC_E_ROOT_MISMATCH = 65,   /* mtree.root_hash() != root_hash (583-585) */
    HBRBC_E_NO_PAYLOAD_LEN = 66,  /* fewer than 4 data bytes (592-597)        */
    /* bincode deserialisation of a wire message (hbrbc_wire_decode_batch) */
    HBRBC_E_WIRE_TRUNCATED = 70,    /* bincode ErrorKind::Io(UnexpectedEof)     */
    HBRBC_E_WIRE_BAD_VARIANT = 71,  /* enum variant index > 4                   */
    HBRBC_E_WIRE_TOO_LARGE = 72,    /* value or digest list exceeds the batch's slots */
    /* library errors */
    HBRBC_E_INVALID_ARG = 100,
    HBRBC_E_DEVICE = 101,         /* a HIP call failed: see hbrbc_last_error() */
    HBRBC_E_NO_DEVICE = 102
};

typedef struct hbrbc_ctx hbrbc_ctx;

/* Message of the last failing call on this thread (static storage). */
const char *hbrbc_last_error(void);
/* Library version string ("hbrbc <semver> gfx950 src=<hash>"; the hash is
 * hbbft_amd/srchash.py over the sources the library was built from). */
const char *hbrbc_version(void);

/* ---- context = one `Coding` (broadcast.rs:639-655) --------------------- */
/* Replaces `Coding::new(data_shard_num, parity_shard_num)`
 * (broadcast.rs:648-655) -> rse `ReedSolomon::new` + `build_matrix`.
 * parity == 0 selects `Coding::Trivial`.  Errors: TOO_FEW_DATA_SHARDS
 * (data == 0), TOO_MANY_SHARDS (data + parity > 256), NO_DEVICE, DEVICE.
 * `device` < 0 uses the calling thread's current HIP device. */
int hbrbc_coding_new(size_t data_shards, size_t parity_shards, int device, hbrbc_ctx **out);
void hbrbc_coding_free(hbrbc_ctx *ctx);
/* `Coding::data_shard_count` / `parity_shard_count` (broadcast.rs:658-671). */
size_t hbrbc_data_shard_count(const hbrbc_ctx *ctx);
size_t hbrbc_parity_shard_count(const hbrbc_ctx *ctx);
/* The (data+parity) x data encoding matrix, row-major (rse `build_matrix`). */
int hbrbc_encoding_matrix(const hbrbc_ctx *ctx, uint8_t *out);
/* The context's own stream (a hipStream_t). */
void *hbrbc_stream(const hbrbc_ctx *ctx);

/* ---- layer 1: per-call shims, host memory, synchronous ------------------ */
/* `Coding::encode(&mut [&mut [u8]])` (broadcast.rs:674-679, called at 193):
 * shards[0..data) in, shards[data..n) overwritten with parity. */
int hbrbc_encode(hbrbc_ctx *ctx, uint8_t *const *shards, const size_t *lens, size_t n_shards);
/* `Coding::reconstruct_shards(&mut [Option<Box<[u8]>>])` (broadcast.rs:682-693,
 * called at 569).  present[i] != 0 marks Some(shard); absent slots must point
 * at writable buffers of the common shard length and are filled (rse
 * allocates them zeroed, then writes every byte). */
int hbrbc_reconstruct(hbrbc_ctx *ctx, uint8_t *const *shards, const size_t *lens,
                      const uint8_t *present, size_t n_shards);

/* Number of nodes in the flattened tree over n leaves (levels + root). */
size_t hbrbc_merkle_node_count(size_t n);
/* Depth bound: the largest digest count of any proof over n leaves. */
size_t hbrbc_merkle_max_proof_len(size_t n);
/* `MerkleTree::from_vec(Vec<T>)` (merkle.rs:20-33): leaf i = SHA3-256 of
 * values[i][0..lens[i]); nodes_out receives node_count(n)*32 bytes, the
 * root last.  Runs on the default device. */
int hbrbc_merkle_build(const uint8_t *const *values, const size_t *lens, size_t n,
                       uint8_t *nodes_out);
/* `MerkleTree::proof(index)` (merkle.rs:36-53): returns HBRBC_OK and fills
 * digests_out (32*ndig bytes, at most max_proof_len(n) digests), or
 * HBRBC_E_INVALID_INDEX for index >= n (`None`).  Pure data movement. */
int hbrbc_merkle_proof(const uint8_t *nodes, size_t n, size_t index, uint8_t *digests_out,
                       size_t *ndig_out);
/* `Proof::validate(n)` (merkle.rs:83-103): *valid_out = 1 iff the digests
 * form a branch from SHA3(value) at `index` to `root` in a tree of n leaves
 * (too few or too many digests -> 0). */
int hbrbc_proof_validate(const uint8_t *value, size_t len, size_t index, const uint8_t *digests,
                         size_t ndig, const uint8_t root[32], size_t n, int *valid_out);

/* ---- layer 2: batched, device memory, asynchronous on `stream` ---------- */
/* send_shards framing (broadcast.rs:174-189): payload p of instance i (bytes
 * payloads[i*payload_stride .. +payload_len)) -> data shards 0..data-1 of
 * the slab hold BE32(payload_len) ++ payload ++ zeros; padding zeroed.
 * payload_stride % 4 == 0 and >= round_up(payload_len, 4); shard_len must
 * equal hbrbc_shard_len(payload_len, data). */
size_t hbrbc_shard_len(size_t payload_len, size_t data_shards);
int hbrbc_frame_batch(hbrbc_ctx *ctx, const uint8_t *payloads, size_t payload_stride,
                      size_t payload_len, size_t count, uint8_t *shards, size_t shard_len,
                      size_t shard_stride, size_t inst_stride, void *stream);
/* Coding::encode over `count` instances (broadcast.rs:193): parity rows
 * data..n-1 of every instance written in place. */
int hbrbc_encode_batch(hbrbc_ctx *ctx, uint8_t *shards, size_t shard_len, size_t shard_stride,
                       size_t inst_stride, size_t count, void *stream);
/* send_shards' framing + Coding::encode in one pass (broadcast.rs:174-193):
 * with the specialised encoder loaded and shard_stride == round_up(shard_len,
 * 16) the data rows are framed straight from the payloads inside the encode
 * kernel (one read of the payload, no re-read of the data rows); otherwise
 * hbrbc_frame_batch then hbrbc_encode_batch.  Same arguments and result. */
int hbrbc_frame_encode_batch(hbrbc_ctx *ctx, const uint8_t *payloads, size_t payload_stride,
                             size_t payload_len, size_t count, uint8_t *shards, size_t shard_len,
                             size_t shard_stride, size_t inst_stride, void *stream);
/* ---- ragged batches: one launch per stage for proposals of any lengths ---- */
/* send_shards' framing + Coding::encode (broadcast.rs:174-193) for `count`
 * proposals of their own lengths, e.g. an epoch where every validator
 * proposes its contribution (honey_badger/epoch_state.rs:223-236,
 * subset/proposal_state.rs:69-113): instance i frames payload_lens[i]
 * (device uint32[count], each <= max_payload_len) bytes into shards of
 * ceil((payload_lens[i] + 4) / data) bytes; every row slot is written up to
 * shard_stride (>= round_up(shard_len(max_payload_len), 16)), zero past the
 * instance's shard, and the parity rows are encoded over that common length. */
int hbrbc_frame_encode_ragged(hbrbc_ctx *ctx, const uint8_t *payloads, size_t payload_stride,
                              const uint32_t *payload_lens, size_t max_payload_len, size_t count,
                              uint8_t *shards, size_t shard_stride, size_t inst_stride,
                              void *stream);
/* MerkleTree::from_vec of a ragged batch: leaf j of instance i hashes
 * shard_lens[i] (device uint32[count]) bytes of its row.  Each entry must be
 * <= shard_stride; the kernels clamp a larger one to shard_stride (they never
 * read past the row slot), so its digests then cover shard_stride bytes. */
int hbrbc_merkle_ragged(hbrbc_ctx *ctx, const uint8_t *shards, const uint32_t *shard_lens,
                        size_t shard_stride, size_t inst_stride, size_t count, uint8_t *nodes,
                        size_t node_inst_stride, void *stream);
/* MerkleTree::from_vec over the n = data+parity shards of every instance
 * (broadcast.rs:204, 580). */
int hbrbc_merkle_batch(hbrbc_ctx *ctx, const uint8_t *shards, size_t shard_len,
                       size_t shard_stride, size_t inst_stride, size_t count, uint8_t *nodes,
                       size_t node_inst_stride, void *stream);
/* MerkleTree::proof for every index of every instance (broadcast.rs:212-222).
 * proof (i, j): digests at digests + ((i*n + j)*max_proof_len(n))*32,
 * count in ndig[i*n + j]. */
int hbrbc_proofs_batch(hbrbc_ctx *ctx, const uint8_t *nodes, size_t node_inst_stride,
                       size_t count, uint8_t *digests, uint8_t *ndig, void *stream);
/* Proof::validate for `count` x `per_inst` proofs (broadcast.rs:254, 291,
 * 604-606).  Proof (i, j): value at values + i*value_inst_stride +
 * j*value_stride (value_len bytes, value_stride % 8 == 0), index
 * indices[i*per_inst + j] (NULL: index = j), digests/ndig laid out as
 * hbrbc_proofs_batch with digest slots = max_proof_len(tree_n), root at
 * roots + i*root_stride.  ok_out[i*per_inst + j] = 1 valid / 0 invalid. */
int hbrbc_validate_batch(hbrbc_ctx *ctx, const uint8_t *values, size_t value_len,
                         size_t value_stride, size_t value_inst_stride, size_t per_inst,
                         const uint32_t *indices, const uint8_t *digests, const uint8_t *ndig,
                         const uint8_t *roots, size_t root_stride, size_t tree_n, size_t count,
                         uint8_t *ok_out, void *stream);
/* Coding::reconstruct_shards over `count` instances (broadcast.rs:569):
 * present[i*n + j] != 0 marks shard j of instance i as received; missing
 * rows are overwritten in place (data from the first `data` present rows via
 * inv(M[valid]), parity from the rebuilt data: bit-identical to rse).
 * status_out[i] = HBRBC_OK or HBRBC_E_TOO_FEW_SHARDS_PRESENT.  Uses the
 * context's workspace (grown on demand, the only allocation on this path;
 * call hbrbc_reserve first to keep it out of a captured region). */
int hbrbc_reconstruct_batch(hbrbc_ctx *ctx, uint8_t *shards, size_t shard_len,
                            size_t shard_stride, size_t inst_stride, const uint8_t *present,
                            size_t count, int32_t *status_out, void *stream);
/* decode_from_shards (broadcast.rs:563-601): reconstruct, re-tree over all n
 * shards, compare with roots[i*root_stride..+32], unframe.  payload bytes of
 * instance i go to payload_out + i*payload_stride (payload_stride a multiple
 * of 4 and >= round_up(data*shard_len - 4, 16); every instance's row must
 * hold that many bytes, bytes past the payload are written 0), their length to payload_len_out[i] and
 * the outcome to status_out[i] (OK, TOO_FEW_SHARDS_PRESENT, ROOT_MISMATCH,
 * NO_PAYLOAD_LEN).  `nodes` (count x node_inst_stride) receives the
 * re-built trees.  Every byte of every instance's payload row up to
 * round_up(data*shard_len - 4, 16) is written: past the payload (all of it
 * for a failed instance) with 0. */
int hbrbc_decode_batch(hbrbc_ctx *ctx, uint8_t *shards, size_t shard_len, size_t shard_stride,
                       size_t inst_stride, const uint8_t *present, size_t count,
                       const uint8_t *roots, size_t root_stride, uint8_t *nodes,
                       size_t node_inst_stride, uint8_t *payload_out, size_t payload_stride,
                       uint32_t *payload_len_out, int32_t *status_out, void *stream);
/* Pre-size the reconstruct workspace (and the decode-matrix cache) for
 * `count` instances; growing it empties the cache. */
int hbrbc_reserve(hbrbc_ctx *ctx, size_t count);

/* ---- blocked row layouts (validator-sharded slabs) ----------------------- */
/* The *_rows variants take the same arguments as their *_batch forms plus a
 * row placement: row j of instance i lives at
 *   base + i*inst_stride + (j / rows_per_block)*block_stride
 *        + (j % rows_per_block)*shard_stride
 * rows_per_block == 0 or >= n is the plain layout above (row j at
 * j*shard_stride).  With rows_per_block < n (<= 255): inst_stride >=
 * rows_per_block*shard_stride and block_stride >= count*inst_stride, e.g.
 * the destination-major Value slab [rank][instance][rows_per_block][stride]
 * whose block d is the contiguous chunk an all-to-all sends to rank d, or the
 * Echo all-gather [validator rank][instance][rows_per_block][stride]. */
int hbrbc_frame_encode_rows(hbrbc_ctx *ctx, const uint8_t *payloads, size_t payload_stride,
                            size_t payload_len, size_t count, uint8_t *shards, size_t shard_len,
                            size_t shard_stride, size_t rows_per_block, size_t block_stride,
                            size_t inst_stride, void *stream);
int hbrbc_merkle_rows(hbrbc_ctx *ctx, const uint8_t *shards, size_t shard_len, size_t shard_stride,
                      size_t rows_per_block, size_t block_stride, size_t inst_stride, size_t count,
                      uint8_t *nodes, size_t node_inst_stride, void *stream);
/* Proof::validate (merkle.rs:83-103) for `count` x `per_inst` proofs: proof
 * (i, jj) checks value row r = rows[jj] (rows: device uint32[per_inst], the
 * same for every instance; NULL: r = jj) of instance i in the row layout
 * above, with claimed index indices[i*per_inst + jj] (NULL: r), digests and
 * ndig of proof slot i*digest_rows + r (rows given; every r < digest_rows) or
 * i*per_inst + jj, against roots + i*root_stride.  ok_out[i*per_inst + jj].
 * leaf_out (optional): SHA3-256 of the value -- the Merkle leaf -- to
 * leaf_out + i*leaf_inst_stride + r*32, e.g. level 0 of a node slab that a
 * later hbrbc_decode_rows(known_leaves = 1) completes. */
int hbrbc_validate_rows(hbrbc_ctx *ctx, const uint8_t *values, size_t value_len,
                        size_t value_stride, size_t rows_per_block, size_t block_stride,
                        size_t value_inst_stride, size_t per_inst, const uint32_t *rows,
                        const uint32_t *indices, const uint8_t *digests, const uint8_t *ndig,
                        size_t digest_rows, const uint8_t *roots, size_t root_stride,
                        size_t tree_n, size_t count, uint8_t *ok_out, uint8_t *leaf_out,
                        size_t leaf_inst_stride, void *stream);
int hbrbc_reconstruct_rows(hbrbc_ctx *ctx, uint8_t *shards, size_t shard_len, size_t shard_stride,
                           size_t rows_per_block, size_t block_stride, size_t inst_stride,
                           const uint8_t *present, size_t count, int32_t *status_out,
                           void *stream);
/* decode_from_shards in the row layout above.  known_leaves != 0: level 0 of
 * `nodes` already holds SHA3-256 of every PRESENT row of every instance (the
 * receiver hashed them when it validated their Echo proofs, broadcast.rs:291,
 * e.g. through hbrbc_validate_rows' leaf_out); only the rows reconstruct
 * rebuilds are hashed before the levels, root compare and unframe. */
int hbrbc_decode_rows(hbrbc_ctx *ctx, uint8_t *shards, size_t shard_len, size_t shard_stride,
                      size_t rows_per_block, size_t block_stride, size_t inst_stride,
                      const uint8_t *present, size_t count, const uint8_t *roots,
                      size_t root_stride, uint8_t *nodes, size_t node_inst_stride,
                      int known_leaves, uint8_t *payload_out, size_t payload_stride,
                      uint32_t *payload_len_out, int32_t *status_out, void *stream);

/* A receiver holds only the rows it got: every row of instance i with
 * present[i*n + j] == 0 (the shards decode_from_shards gets as None,
 * broadcast.rs:566-571) is overwritten with `fill` over its whole slot
 * (shard_stride bytes), in the plain or blocked layout.  A decode after it
 * rebuilds those rows from the others; the benchmark drops the erased rows
 * of every step this way so no timed decode starts from rows that still
 * hold the right bytes.  n <= 256. */
int hbrbc_drop_rows(hbrbc_ctx *ctx, uint8_t *shards, size_t shard_stride, size_t rows_per_block,
                    size_t block_stride, size_t inst_stride, const uint8_t *present, size_t count,
                    uint8_t fill, void *stream);

/* ---- decode-matrix cache (rse's per-pattern decode-matrix LRU) ----------- */
/* Every reconstruct/decode call looks each instance's present pattern up in a
 * device hash table: the first instance of a new pattern computes inv(M[first
 * k present]) and the recovery rows into a shared slot, every other instance
 * of that pattern -- in this call or a later one -- reuses them.  Shared
 * slots are flushed after about 4 x capacity insertions.  Calls on one
 * context must be stream-ordered (the cache is context state). */
int hbrbc_decode_cache_clear(hbrbc_ctx *ctx);
/* Shared slots claimed since the last flush (synchronises the device). */
int hbrbc_decode_cache_fill(hbrbc_ctx *ctx, uint32_t *patterns_out);
/* Pattern-specialised decoder: compile (hiprtc; or load from the code-object
 * cache) an XOR network for the erasure pattern `present` (host, n bytes)
 * in layouts with this rows_per_block (0: plain).  Later reconstruct/decode
 * calls in that layout run it for every instance of the pattern and the
 * generic kernel for the rest; one pattern per layout (a new call replaces
 * the previous one).  HBRBC_JIT=0 forbids compiling (cache only). */
int hbrbc_decoder_specialise(hbrbc_ctx *ctx, const uint8_t *present, size_t rows_per_block);

/* ---- wire format: bincode of broadcast::Message -------------------------- */
/* `Message::{Value, Echo}(Proof<Vec<u8>>)` (message.rs:13-24, merkle.rs:72-78) as
 * bincode 1.x `serialize` writes it (Cargo.toml:24; examples/simulation.rs:132,
 * examples/network/commst.rs:68): u32 LE variant (0 Value, 1 Echo, 2 Ready,
 * 3 CanDecode, 4 EchoHash), then for Value/Echo u64 LE value length, the value,
 * u64 LE index, u64 LE digest count, 32 bytes per digest, 32 root bytes;
 * for the digest variants 32 bytes.  Message g lives in a slot at
 * out + g*msg_stride (16-aligned, zero-padded past its length). */
size_t hbrbc_wire_proof_message_len(size_t value_len, size_t ndig);
/* Serialise the proofs laid out as for hbrbc_validate_batch (value (i, j) at
 * values + i*value_inst_stride + j*value_stride, 16-aligned rows; index
 * indices[i*per_inst + j] or j; digests/ndig as hbrbc_proofs_batch; root at
 * roots + i*root_stride) as Value (variant 0) or Echo (1) messages, message
 * g = i*per_inst + j; msg_len_out[g] = its length.  msg_stride >=
 * round_up(proof_message_len(value_len, max_proof_len(n)), 16). */
int hbrbc_wire_encode_batch(hbrbc_ctx *ctx, uint32_t variant, const uint8_t *values,
                            size_t value_len, size_t value_stride, size_t value_inst_stride,
                            size_t per_inst, const uint32_t *indices, const uint8_t *digests,
                            const uint8_t *ndig, const uint8_t *roots, size_t root_stride,
                            size_t count, uint8_t *out, size_t msg_stride, uint32_t *msg_len_out,
                            void *stream);
/* Deserialise `nmsg` messages of msg_len[g] bytes each (bincode `deserialize`;
 * trailing bytes ignored): variant_out[g]; for Value/Echo the value into
 * values + g*value_stride (zero-padded; longer than value_stride -> WIRE_TOO_LARGE),
 * value_len_out, index_out (saturated at 2^32-1), digests + g*max_proof_len(n)*32
 * and ndig_out (more than max_proof_len(n) -> WIRE_TOO_LARGE, since no tree over
 * n leaves has that many levels), roots + g*32; for Ready/CanDecode/EchoHash the
 * digest into roots.  status_out[g] = OK or a WIRE_* code. */
int hbrbc_wire_decode_batch(hbrbc_ctx *ctx, const uint8_t *msgs, size_t msg_stride,
                            const uint32_t *msg_len, size_t nmsg, uint8_t *values,
                            size_t value_stride, uint32_t *value_len_out, uint32_t *index_out,
                            uint8_t *digests, uint8_t *ndig_out, uint8_t *roots,
                            uint32_t *variant_out, int32_t *status_out, void *stream);

/* ---- specialised encoder ------------------------------------------------ */
/* Coding::encode runs either the generic bit-sliced GF kernel or, when a code
 * object for this (data, parity) matrix is cached under <lib dir>/jit (or
 * $HBRBC_JIT_DIR), a kernel generated for the matrix: a fixed XOR network on
 * bit planes (hbbft_amd/csrc/jit.hip), bit-identical output.  Returns
 * "specialised", "bitslice", "trivial" or "jit-failed". */
const char *hbrbc_encode_kernel(const hbrbc_ctx *ctx);
/* Generate and compile (hiprtc, gfx950, no device needed) the specialised
 * encoder for rse build_matrix(data, data + parity) into `dir` (NULL: the
 * default directory).  With HBRBC_JIT=1 a context compiles a missing one
 * itself; HBRBC_JIT=0 disables the specialised path. */
int hbrbc_jit_build_encode(size_t data_shards, size_t parity_shards, const char *dir);
/* Large matrices are split into parity-row groups, one code object each (a
 * program stays near 4096 coefficients, so hiprtc time stays near a minute);
 * these build them one at a time, e.g. in parallel processes. */
size_t hbrbc_jit_encode_groups(size_t data_shards, size_t parity_shards);
int hbrbc_jit_build_encode_group(size_t data_shards, size_t parity_shards, size_t group,
                                 const char *dir);
/* Cache file name (no directory) of group `group`'s code object under the
 * current generator settings; 0 and a NUL-terminated name in buf, or an error. */
int hbrbc_jit_file_name(size_t data_shards, size_t parity_shards, size_t group, char *buf,
                        size_t buf_len);
/* The same for the encoder of a blocked row layout (rows_per_block < n). */
int hbrbc_jit_build_encode_rows(size_t data_shards, size_t parity_shards, size_t group,
                                size_t rows_per_block, const char *dir);
int hbrbc_jit_encode_file_name(size_t data_shards, size_t parity_shards, size_t group,
                               size_t rows_per_block, char *buf, size_t buf_len);
/* Pattern-specialised decoders (hbrbc_decoder_specialise) built ahead of use:
 * groups of the pattern's program, one group's code object, its file name. */
size_t hbrbc_jit_decode_groups(size_t data_shards, size_t parity_shards, const uint8_t *present);
int hbrbc_jit_build_decode(size_t data_shards, size_t parity_shards, const uint8_t *present,
                           size_t rows_per_block, size_t group, const char *dir);
/* The same for the decoder's fused-unframe variant (fused_unframe != 0: the
 * programs also write the payload bytes of the data rows; a decode that
 * unframes in the reconstruct loads them on first use). */
int hbrbc_jit_build_decode_variant(size_t data_shards, size_t parity_shards,
                                   const uint8_t *present, size_t rows_per_block, size_t group,
                                   int fused_unframe, const char *dir);
int hbrbc_jit_decode_variant_file_name(size_t data_shards, size_t parity_shards,
                                       const uint8_t *present, size_t rows_per_block,
                                       size_t group, int fused_unframe, char *buf,
                                       size_t buf_len);
int hbrbc_jit_decode_file_name(size_t data_shards, size_t parity_shards, const uint8_t *present,
                               size_t rows_per_block, size_t group, char *buf, size_t buf_len);

/* ---- measurement hooks (bench.py) --------------------------------------- */
/* Stage ids for the per-stage device timers. */
enum hbrbc_stage {
    HBRBC_STAGE_FRAME = 0,
    HBRBC_STAGE_ENCODE = 1,
    HBRBC_STAGE_LEAF_HASH = 2,
    HBRBC_STAGE_TREE_LEVELS = 3,
    HBRBC_STAGE_PROOFS = 4,
    HBRBC_STAGE_VALIDATE = 5,
    HBRBC_STAGE_DECODE_MATRIX = 6,
    HBRBC_STAGE_RECONSTRUCT = 7,
    HBRBC_STAGE_UNFRAME = 8,
    HBRBC_STAGE_COUNT = 9
};
/* When enabled, every stage's kernels are bracketed by hipEvents recorded on
 * the stream they run on.  hbrbc_profile_read synchronises those events and
 * returns total milliseconds and launch count per stage since the last
 * reset. */
int hbrbc_profile_enable(hbrbc_ctx *ctx, int enable);
int hbrbc_profile_reset(hbrbc_ctx *ctx);
int hbrbc_profile_read(hbrbc_ctx *ctx, double *ms_out, uint64_t *launches_out);
const char *hbrbc_stage_name(int stage);

/* 1 if hbrbc_decode_batch / _rows on this context (row block rows_per_block,
 * 0 = plain layout) write the payload from the reconstruct kernel (fused
 * unframe, in the generic and the pattern-specialised decoders: shard_len
 * % 4 == 0, payload_stride % 16 == 0, HBRBC_UNFRAME_FUSED != 0), else 0.
 * Outputs are identical either way; this only tells where the bytes move. */
int hbrbc_unframe_fused(const hbrbc_ctx *ctx, size_t shard_len, size_t payload_stride,
                        size_t rows_per_block);

/* ---- threshold-decrypt share verification --------------- */
/* BLS12-381 pairings of the `pairing` crate as `threshold_crypto` (rev 624eeee,
 * Cargo.toml:36) uses them behind hbbft's ThresholdDecrypt:
 *   `Ciphertext::verify`                  (threshold_decrypt.rs:142)
 *       e(G1::one(), W) == e(U, hash_g1_g2(U, V))
 *   `PublicKeyShare::verify_decryption_share` (threshold_decrypt.rs:220-228)
 *       e(share, hash_g1_g2(U, V)) == e(pk_i, W)
 * Points use the crate's uncompressed encodings: G1 = 96 bytes x || y, G2 =
 * 192 bytes x.c1 || x.c0 || y.c1 || y.c0, big-endian, infinity = flag 0x40 in
 * byte 0 with every other bit zero.  Non-canonical coordinates (>= p), set
 * compression/sort flags, points off the curve and points outside the
 * order-r subgroup are rejected per item, as the crate's deserialisation
 * (`into_affine`) rejects them.
 * These entries take H = hash_g1_g2(U, V) as a G2 point; hbrbc_hash_g1_g2_batch
 * ("hashes and the pad" below) computes it on the device.
 *   `PublicKeySet::decrypt`               (threshold_decrypt.rs:232-252, try_output)
 *       g = sum_i lambda_i share_i, the Lagrange interpolation at 0 of more
 *       than num_faulty valid shares in G1 (x_i = node index + 1, lambda_i =
 *       prod_{j != i} x_j / (x_j - x_i) in the scalar field Fr), from the
 *       shares as hbrbc_g1_prepare left them on the device; the
 *       hbrbc_lagrange_coeffs .. hbrbc_decrypt_combine entries below.
 *       xor_with_hash(g, V), which turns g into the plaintext, is
 *       hbrbc_xor_with_hash_batch below; it hashes the compressed encoding of
 *       g. */
#define HBRBC_G1_BYTES 96
#define HBRBC_G2_BYTES 192
#define HBRBC_GT_BYTES 576
/* Device workspace bytes for `pairings` Miller loops. */
size_t hbrbc_pairing_workspace_size(size_t pairings);
/* `PEngine::pairing(g1[i], g2[i])` for i < count: gt_out + 576 i receives the
 * GT value (the crate's Fq12 after its final exponentiation, tower order
 * c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1, each coefficient 48 bytes
 * big-endian); status_out[i] = 0 ok, 2 invalid point (the value is then 1).
 * An infinity on either side gives 1.  Device memory, async on `stream`. */
int hbrbc_pairing_batch(const uint8_t *g1, const uint8_t *g2, size_t count, uint8_t *gt_out,
                        uint8_t *status_out, void *workspace, void *stream);
/* count checks e(a_i, b_i) == e(c_i, d_i): g1 holds a_0, c_0, a_1, c_1, ...
 * (2 count points), g2 holds b_0, d_0, b_1, d_1, ....  ok_out[i] = 1 if
 * equal, 0 if not, 2 if any of the four points is invalid.  For
 * verify_decryption_share: a = share, b = hash, c = pk_i, d = W; for
 * Ciphertext::verify: a = G1::one(), b = W, c = U, d = hash.
 * workspace >= hbrbc_pairing_workspace_size(2 count).  Device memory, async. */
int hbrbc_pairing_check_batch(const uint8_t *g1, const uint8_t *g2, size_t count,
                              uint8_t *ok_out, void *workspace, void *stream);
/* Prepared G2 points (the crate's G2Prepared): the 68 Miller-loop lines of
 * each point, computed once and shared by every check against it (hbbft:
 * the N decryption shares of a ciphertext are all checked against its H and
 * W).  `prepared` >= hbrbc_g2_prepared_size(count) bytes of device memory;
 * an invalid point is marked there and fails every check that uses it.
 *
 * Table layout, for all three kinds of prepared table (hbrbc_g2_prepare,
 * hbrbc_g1_prepare, hbrbc_g2_points_prepare and the entries that write their
 * results in one of these forms): the coordinates of the `points` entries,
 * padded to 256 bytes, then one status byte per entry.  The status bytes thus
 * sit at an offset that depends on the count the table was prepared with:
 * every entry that takes a table takes that count with it (`points`,
 * `key_points`, `prepared_count`, `sig_count`, `table_count`), whatever rows
 * the call uses. */
size_t hbrbc_g2_prepared_size(size_t points);
int hbrbc_g2_prepare(const uint8_t *g2, size_t count, void *prepared, void *stream);
/* count checks e(a_i, P[idx_b[i]]) == e(c_i, P[idx_d[i]]) against prepared
 * points P (`points` of them in `prepared`): g1 holds a_0, c_0, a_1, c_1, ...;
 * ok_out as hbrbc_pairing_check_batch (an index >= points makes that check 2).
 * Checks that share prepared points
 * should be adjacent (a wave then reads each line once).  workspace >=
 * hbrbc_pairing_workspace_size(count).  Device memory, async on `stream`. */
int hbrbc_pairing_check_prepared(const uint8_t *g1, const void *prepared, size_t points,
                                 const uint32_t *idx_b, const uint32_t *idx_d, size_t count,
                                 uint8_t *ok_out, void *workspace, void *stream);
/* Prepared G1 keys: hbbft checks each decryption share against its sender's
 * public key share pk_i, and the validator set's key shares are the same for
 * every ciphertext; `threshold_crypto` holds them as curve points, decoded and
 * checked once.  hbrbc_g1_prepare decodes and checks `count` G1 points once
 * (as any G1 input: canonical, on the curve, order r) into `prepared` >=
 * hbrbc_g1_prepared_size(count) bytes of device memory; an invalid point is
 * marked there and fails every check that uses it.  Device memory, async.
 * Table layout: see hbrbc_g2_prepared_size. */
size_t hbrbc_g1_prepared_size(size_t points);
int hbrbc_g1_prepare(const uint8_t *g1, size_t count, void *prepared, void *stream);
/* count checks e(a_i, P[idx_b[i]]) == e(K[idx_c[i]], P[idx_d[i]]) with K the
 * `key_points` prepared G1 keys and P the `points` prepared G2 points: g1_a
 * holds a_0, a_1, ... (count points); ok_out as hbrbc_pairing_check_batch
 * (an index past either table makes that check 2).  For
 * verify_decryption_share: a = share, K = the pk_i table, b = hash, d = W.
 * workspace >= hbrbc_pairing_workspace_size(count).  Device memory, async. */
int hbrbc_pairing_check_prepared_keys(const uint8_t *g1_a, const void *keys, size_t key_points,
                                      const uint32_t *idx_c, const void *prepared, size_t points,
                                      const uint32_t *idx_b, const uint32_t *idx_d, size_t count,
                                      uint8_t *ok_out, void *workspace, void *stream);
/* The same checks with the shares decoded beforehand too: `a_prepared` is
 * hbrbc_g1_prepare of the count shares (a_i = entry i), so their decoding
 * and order-r checks run as a launch of their own (e.g. beside
 * hbrbc_g2_prepare on another stream) and the Miller loops only load them.
 * Outcomes as hbrbc_pairing_check_prepared_keys. */
int hbrbc_pairing_check_prepared_pts(const void *a_prepared, const void *keys, size_t key_points,
                                     const uint32_t *idx_c, const void *prepared, size_t points,
                                     const uint32_t *idx_b, const uint32_t *idx_d, size_t count,
                                     uint8_t *ok_out, void *workspace, void *stream);
/* Per-call shim on host memory (one check, synchronous, current device):
 * *result = 1 if e(a, b) == e(c, d), 0 if not; HBRBC_E_INVALID_ARG for an
 * invalid point. */
int hbrbc_pairing_check(const uint8_t a[96], const uint8_t b[192], const uint8_t c[96],
                        const uint8_t d[192], int *result);
/* Combining decryption shares: batches of ragged groups.  Group g holds the
 * entries offsets[g] .. offsets[g + 1] - 1 of the flat per-share arrays
 * (offsets: groups + 1 entries, a prefix sum; offsets[groups] is the share
 * count, which each entry reads back from the device -- one 4-byte copy that
 * waits for the stream -- before it queues its kernels).  Per-group status:
 * 0 ok, 1 ok and the result is the point at infinity, 2 an invalid input in
 * the group (invalid table entry, row outside the table, scalar >= r), 3 two
 * equal indices in the group (the crate's DuplicateEntry).  Results come in
 * two encodings: out96 + 96 g the uncompressed one (as the inputs), out48 +
 * 48 g zkcrypto's G1Compressed (x big-endian with 0x80 set in byte 0, 0x20 set
 * iff y > p - y; infinity = 0xC0 and 47 zero bytes); for statuses 2 and 3
 * both are zero bytes, and a failed group never affects another.  An empty
 * group is the empty sum (status 1).  Device memory, async on `stream`. */
#define HBRBC_G1_COMPRESSED_BYTES 48
#define HBRBC_FR_BYTES 32
/* Device workspace bytes of the three entries below. */
size_t hbrbc_g1_combine_workspace_size(size_t total_shares, size_t groups);
/* lambda of every share: idx holds the node indices (x = idx + 1, formed in
 * 64 bits), coeffs_out + 32 j receives lambda_j as 32 big-endian bytes
 * (canonical, < r; zero bytes where the index repeats), status_out[g] = 0 or
 * 3.  Needs no workspace. */
int hbrbc_lagrange_coeffs(const uint32_t *idx, const uint32_t *offsets, size_t groups,
                          uint8_t *coeffs_out, uint8_t *status_out, void *stream);
/* Per group sum_j scalars[j] * T[rows[j]] over a table T of hbrbc_g1_prepare:
 * rows int32 per share, scalars 32 big-endian bytes per share.
 * `prepared_count` is the table's count (see hbrbc_g2_prepared_size).
 * A zero scalar and a table entry at infinity contribute the identity. */
int hbrbc_g1_lincomb_prepared(const void *a_prepared, size_t prepared_count, const int32_t *rows,
                              const uint8_t *scalars, const uint32_t *offsets, size_t groups,
                              uint8_t *out96, uint8_t *out48, uint8_t *status_out,
                              void *workspace, void *stream);
/* `PublicKeySet::decrypt` up to g: the two above in sequence, share j of a
 * group being T[rows[j]] from node idx[j]. */
int hbrbc_decrypt_combine_prepared(const void *a_prepared, size_t prepared_count,
                                   const int32_t *rows, const uint32_t *idx,
                                   const uint32_t *offsets, size_t groups, uint8_t *out96,
                                   uint8_t *out48, uint8_t *status_out, void *workspace,
                                   void *stream);
/* Per-call shim on host memory (one group of n shares, 96 bytes each, from
 * nodes idx[0..n); synchronous, current device): decodes and checks the
 * shares and combines them.  HBRBC_E_INVALID_ARG for an invalid share or a
 * repeated index (statuses 2 and 3); a result at infinity is returned in its
 * encodings. */
int hbrbc_decrypt_combine(const uint8_t *shares, const uint32_t *idx, size_t n, uint8_t out96[96],
                          uint8_t out48[48]);

/* ---- key generation: SyncKeyGen's commitment evaluations -----------------
 * `SyncKeyGen` (sync_key_gen.rs) checks each Part against `commit.row(our_idx
 * + 1)` (:557, :569) and each Ack against `commit.evaluate(our_idx + 1,
 * sender_idx + 1)` (:603), `generate` sums `commit.row(0)` over the complete
 * parts (:516-534), and `PublicKeySet::public_key_share(i)` is
 * `commit.evaluate(i + 1)`: G1 polynomials evaluated at small integers, and
 * comparisons with [s] G1::one().  Decrypting rows and values (`sec_key.decrypt`,
 * over hbrbc_xor_with_hash_batch) stays with the caller; scalars arrive as Fr.  Device memory, async on
 * `stream`; neither entry reads anything back.
 *
 * Evaluates ragged polynomials over a table T of hbrbc_g1_prepare with
 * `prepared_count` points: polynomial p has the coefficients
 * T[rows[offsets[p] .. offsets[p + 1])], constant term first (offsets: polys +
 * 1 entries, a prefix sum whose last entry is the length of rows; every range
 * is clamped to it).  Evaluation e is polynomial poly[e] at x[e], the raw
 * point (the crate's IntoFr of an integer; x = 0 gives the constant term, x =
 * 1 the sum of the coefficients; an empty polynomial is the identity), by
 * Horner's rule with double-and-add over the significant bits of x.
 * status_out[e]: 0 ok, 1 ok and the point at infinity, 2 an invalid table
 * entry, a row outside the table or poly[e] outside [0, polys).  Results go to
 * `out_table` (hbrbc_g1_prepared_size(evals) bytes) in the form of
 * hbrbc_g1_prepare over `evals` points, bit for bit -- every entry that takes
 * such a table takes it, this one included -- and, where the pointers are
 * non-null, to out96 + 96 e and out48 + 48 e in the encodings of the combine
 * above (zero bytes for status 2). */
int hbrbc_g1_poly_eval_prepared(const void *a_prepared, size_t prepared_count, const int32_t *rows,
                                const uint32_t *offsets, size_t polys, const int32_t *poly,
                                const uint32_t *x, size_t evals, void *out_table, uint8_t *out96,
                                uint8_t *out48, uint8_t *status_out, void *stream);
/* count checks [s_i] G1::one() == T[rows[i]] over a table T of hbrbc_g1_prepare
 * (or of the entry above) with `prepared_count` points: scalars + 32 i holds
 * s_i as 32 big-endian bytes.  ok_out[i]: 1 equal, 0 not, 2 an invalid table
 * entry, a row outside the table or s_i >= r.  A table entry at infinity
 * equals [0] G1::one(). */
int hbrbc_g1_base_mul_check(const void *a_prepared, size_t prepared_count, const int32_t *rows,
                            const uint8_t *scalars, size_t count, uint8_t *ok_out, void *stream);

/* ---- threshold signatures: ThresholdSign, the coin of BinaryAgreement ----
 * `ThresholdSign` (threshold_sign.rs; binary_agreement.rs:444-446 creates one
 * per coin round and :404 takes `sig.parity()` as the coin) checks every
 * received share with
 *   `PublicKeyShare::verify_g2`           e(pk_i, H) == e(G1::one(), share_i)
 * (:216-225, H = hash_g2(doc)) and, with more than num_faulty valid shares,
 * runs `combine_signatures` -- the Lagrange interpolation at 0 of the shares
 * in G2 -- and checks the result against the master public key (:249-270) in
 * the same form.  H arrives as a G2 point (hbrbc_hash_g2_batch below computes
 * hash_g2 on the device).  Shares arrive in the uncompressed
 * encoding (192 bytes) here, or as 96-byte wire shares through
 * hbrbc_g2_points_prepare_compressed below.
 *
 * The G2 point on the right of the check differs per share, so it is not a
 * prepared-lines point: the shares are decoded and checked once (canonical
 * coordinates, on the twist, order r) into a point table, which both the
 * check and the combine read.  Device memory, async on `stream`. */
#define HBRBC_G2_COMPRESSED_BYTES 96
/* Bytes of a table of `points` decoded G2 points (table layout: see
 * hbrbc_g2_prepared_size). */
size_t hbrbc_g2_points_size(size_t points);
/* Decodes g2 (count x 192 bytes) into `table` (hbrbc_g2_points_size(count)
 * bytes): affine coordinates and a status per point (invalid points are kept
 * as status, their coordinates zero). */
int hbrbc_g2_points_prepare(const uint8_t *g2, size_t count, void *table, void *stream);
/* count checks e(K[idx_key[i]], P[idx_h[i]]) == e(G1::one(), S[i]): S = a
 * hbrbc_g2_points_prepare table of exactly `sig_count` points (check i reads
 * entry i), K = `key_points` keys of hbrbc_g1_prepare, P = `points` points of
 * hbrbc_g2_prepare.  ok_out[i]: 1 equal, 0 not, 2 an invalid point, an index
 * outside its table or i >= sig_count.  An S[i] at infinity is a valid point
 * (the check then holds only if the left side is 1).  Workspace:
 * hbrbc_pairing_workspace_size(count). */
int hbrbc_sig_check_prepared(const void *sig_table, size_t sig_count, const void *keys,
                             size_t key_points, const uint32_t *idx_key, const void *prepared,
                             size_t points, const uint32_t *idx_h, size_t count, uint8_t *ok_out,
                             void *workspace, void *stream);
/* Combining signature shares: ragged groups and statuses as for the
 * decryption shares above.  Results per group: out192 + 192 g the uncompressed
 * encoding, out96 + 96 g zkcrypto's G2Compressed (x.c1 || x.c0 big-endian with
 * 0x80 set in byte 0, 0x20 set iff y is the larger of y and -y, c1 compared
 * first and c0 only when the c1 are equal; infinity = 0xC0 and 95 zero
 * bytes), parity_out[g] the XOR of all bits of the uncompressed encoding
 * (`Signature::parity()`, the coin).  For statuses 2 and 3 all three are zero
 * bytes.  Device workspace bytes of the two entries below: */
size_t hbrbc_g2_combine_workspace_size(size_t total_shares, size_t groups);
/* Per group sum_j scalars[j] * S[rows[j]] over a table S of
 * hbrbc_g2_points_prepare with exactly `sig_count` points: rows int32 per
 * share, scalars 32 big-endian bytes per share (>= r: status 2). */
int hbrbc_g2_lincomb_prepared(const void *sig_table, size_t sig_count, const int32_t *rows,
                              const uint8_t *scalars, const uint32_t *offsets, size_t groups,
                              uint8_t *out192, uint8_t *out96, uint8_t *parity_out,
                              uint8_t *status_out, void *workspace, void *stream);
/* `combine_signatures`: the Lagrange coefficients of idx (as
 * hbrbc_lagrange_coeffs) followed by the linear combination, share j of a
 * group being S[rows[j]] from node idx[j]; status 3 for a repeated index. */
int hbrbc_sig_combine_prepared(const void *sig_table, size_t sig_count, const int32_t *rows,
                               const uint32_t *idx, const uint32_t *offsets, size_t groups,
                               uint8_t *out192, uint8_t *out96, uint8_t *parity_out,
                               uint8_t *status_out, void *workspace, void *stream);
/* Per-call shim on host memory (one group of n shares, 192 bytes each, from
 * nodes idx[0..n); synchronous, current device): decodes and checks the
 * shares and combines them.  HBRBC_E_INVALID_ARG for an invalid share or a
 * repeated index (statuses 2 and 3); a result at infinity is returned in its
 * encodings. */
int hbrbc_sig_combine(const uint8_t *shares, const uint32_t *idx, size_t n, uint8_t out192[192],
                      uint8_t out96[96], uint8_t *parity);

/* ---- compressed wire encodings -------------------------------------------
 * hbbft's messages carry points in the crate's compressed form: 48 bytes for
 * G1 (DecryptionShare, PublicKeyShare, a ciphertext's U: x big-endian), 96 for
 * G2 (SignatureShare, a ciphertext's W: x.c1 || x.c0), with three flags in
 * byte 0: 0x80 compressed (must be set), 0x40 infinity (every other bit then
 * zero), 0x20 y is the larger of y and -y (as integers; in Fp2 c1 compared
 * first and c0 only when the c1 are equal).  The entries below decode as
 * G1Compressed::into_affine / G2Compressed::into_affine do: flags, x < p,
 * y = sqrt(x^3 + b) (no root: invalid) with the sign the flag names, order r.
 * Device memory, async on `stream`.
 *
 * hbrbc_g1_prepare / hbrbc_g2_points_prepare from compressed input: g1c holds
 * count x 48 bytes, g2c count x 96; the tables (hbrbc_g1_prepared_size /
 * hbrbc_g2_points_size bytes) are those of the uncompressed entries, bit for
 * bit, and every entry that takes such a table takes these. */
int hbrbc_g1_prepare_compressed(const uint8_t *g1c, size_t count, void *prepared, void *stream);
int hbrbc_g2_points_prepare_compressed(const uint8_t *g2c, size_t count, void *table,
                                       void *stream);
/* Compressed to uncompressed: out96 + 96 i (out192 + 192 i) receives point i
 * in the encoding the other entries take -- zero bytes for an invalid point,
 * 0x40 and zeros for infinity -- and status[i] 0 ok, 1 infinity, 2 invalid.
 * A ciphertext's W reaches hbrbc_g2_prepare this way, its U the pairing
 * checks. */
int hbrbc_g1_decompress(const uint8_t *g1c, size_t count, uint8_t *out96, uint8_t *status,
                        void *stream);
int hbrbc_g2_decompress(const uint8_t *g2c, size_t count, uint8_t *out192, uint8_t *status,
                        void *stream);

/* ---- share creation: what a node sends -----------------------------------
 * The entries above handle what a node receives; these make what it sends,
 * for a simulator or test network that hosts every node:
 *   `decrypt_share_no_verify`  [sk_i] U          (threshold_decrypt.rs:161)
 *   `sign_g2`                  [sk_i] H          (threshold_sign.rs:167)
 *   `Poly::commitment`, `BivarPoly::commitment`, `public_key_share`, the U of
 *   `PublicKey::encrypt`       [s] G1::one()
 *   `BivarPoly::row`, `Poly::evaluate`, and `generate`'s secret key share
 *   (sync_key_gen.rs:413-417, :459, :523-524), in the scalar field Fr.
 * Scalars are 32 big-endian bytes, canonical (< r).  Device memory, async on
 * `stream`; no entry reads anything back.  The multiplications branch on the
 * bits of the scalar: they are NOT constant-time and are meant for simulation
 * and test networks, not for a node whose secret key an observer could time.
 * hash_g1_g2, hash_g2 and xor_with_hash have entries of their own below
 * ("hashes and the pad"); `pk.encrypt` / `sec_key.decrypt` of rows and values
 * are built from them by the caller, and `BivarPoly::random` stays with the
 * caller.
 *
 * [s_i] G1::one() for i < count: result i goes to `out_table`
 * (hbrbc_g1_prepared_size(count) bytes) as entry i of a hbrbc_g1_prepare table
 * over `count` points, bit for bit, and, where the pointers are non-null, to
 * out96 + 96 i and out48 + 48 i in the encodings of the combine.
 * status_out[i]: 0 ok, 1 the point at infinity (s = 0), 2 s >= r (zero
 * bytes). */
int hbrbc_g1_base_mul(const uint8_t *scalars, size_t count, void *out_table, uint8_t *out96,
                      uint8_t *out48, uint8_t *status_out, void *stream);
/* Result j < count is [scalars[sidx[j]]] T[rows[j]]: T a table of
 * hbrbc_g1_prepare (hbrbc_g2_points_prepare) with exactly `prepared_count`
 * (`table_count`) points, `scalars` holds nscalars scalars, rows and sidx are
 * int32 per result.  A null sidx means sidx[j] = j, and nscalars must then be
 * >= count.  Lanes that share a scalar should be adjacent (sort the results by
 * sidx): a wave whose 64 lanes hold one scalar takes every branch as one.
 * Results go to `out_table` (hbrbc_g1_prepared_size(count) /
 * hbrbc_g2_points_size(count) bytes) in the form of hbrbc_g1_prepare /
 * hbrbc_g2_points_prepare over `count` points, bit for bit -- every entry
 * that reads such a table reads this one, and no second order-r check is due:
 * a multiple of a checked point is in the subgroup -- and, where the pointers
 * are non-null, to the uncompressed and compressed encodings (G1: out96 +
 * 96 j, out48 + 48 j; G2: out192 + 192 j, out96 + 96 j).  status_out[j]: 0
 * ok, 1 the point at infinity (a zero scalar or a table entry at infinity), 2
 * an invalid table entry, a row outside the table, sidx[j] outside [0,
 * nscalars) or a scalar >= r (zero bytes); an index out of range is a status,
 * never a read out of range. */
int hbrbc_g1_mul_prepared(const void *a_prepared, size_t prepared_count, const int32_t *rows,
                          const uint8_t *scalars, size_t nscalars, const int32_t *sidx,
                          size_t count, void *out_table, uint8_t *out96, uint8_t *out48,
                          uint8_t *status_out, void *stream);
int hbrbc_g2_mul_prepared(const void *table, size_t table_count, const int32_t *rows,
                          const uint8_t *scalars, size_t nscalars, const int32_t *sidx,
                          size_t count, void *out_table, uint8_t *out192, uint8_t *out96,
                          uint8_t *status_out, void *stream);
/* The Fr twin of hbrbc_g1_poly_eval_prepared, with the same ragged
 * description: polynomial p has the coefficients scalars[rows[offsets[p] ..
 * offsets[p + 1])], constant term first (offsets: polys + 1 entries, every
 * range clamped to the last one, which the kernel reads itself).  Evaluation
 * e is polynomial poly[e] at the raw x[e] (x = 0 gives the constant term, an
 * empty polynomial 0): out + 32 e.  status_out[e]: 0 ok, 2 a coefficient >= r,
 * a row outside [0, nscalars) or poly[e] outside [0, polys) (zero bytes).
 * `BivarPoly::row(x)`: coefficient j is the polynomial over the entries (0..t,
 * j) of the bivariate polynomial; `Poly::evaluate` directly. */
int hbrbc_fr_poly_eval(const uint8_t *scalars, size_t nscalars, const int32_t *rows,
                       const uint32_t *offsets, size_t polys, const int32_t *poly,
                       const uint32_t *x, size_t evals, uint8_t *out, uint8_t *status_out,
                       void *stream);
/* Per group g the sum of a_j b_j mod r over j in [offsets[g], offsets[g + 1])
 * (offsets: groups + 1 entries, every range clamped to `total`, the number of
 * scalars in a and in b): out + 32 g.  status_out[g]: 0 ok (an empty group is
 * 0), 2 an operand >= r (zero bytes).  With a = the coefficients of
 * hbrbc_lagrange_coeffs and b = the values a node received, this is the
 * `Poly::interpolate(..).evaluate(0)` of `generate`. */
int hbrbc_fr_dot(const uint8_t *a, const uint8_t *b, const uint32_t *offsets, size_t groups,
                 size_t total, uint8_t *out, uint8_t *status_out, void *stream);

/* ---- hashes and the pad: bytes to group elements and back -----------------
 * `threshold_crypto`'s hash_g2(doc) (the H of a signature, the coin's nonce),
 * hash_g1_g2(U, V) (the H of a ciphertext) and xor_with_hash(g, V) (the pad of
 * encrypt and decrypt).  The crate is not available to this project: the
 * definition is the one written out in hbbft_amd/csrc/hash_g2.hip and
 * tests/hash_ref.py (SHA3-256 seed, ChaCha20 word stream, rejection-sampled
 * Fq2 x, root y by a drawn flag, the full 507-bit cofactor of E'(Fp2)), and
 * its byte parity with the crate is NOT pinned.  One stated
 * deviation: a product with the cofactor at infinity (probability ~2^-255) is
 * status 3 here; the crate draws again.
 *
 * Ragged input: item i is msgs[offsets[i] .. offsets[i + 1]) (offsets: count +
 * 1 uint32 entries), `total` the bytes in msgs (<= 2^32 - 1); an item whose
 * range is reversed or ends past `total` is status 2 and nothing of it is
 * read.  hbrbc_hash_g1_g2_batch appends the 48 bytes at u48 + 48 i (a
 * ciphertext's U as it arrives on the wire; the bytes are hashed, not read as
 * a point) to the message, or to its SHA3-256 when it is longer than 64 bytes.
 * Result i goes to `out_table` (hbrbc_g2_points_size(count) bytes) as entry i
 * of a hbrbc_g2_points_prepare table over `count` points, bit for bit -- so
 * hbrbc_g2_mul_prepared and hbrbc_sig_check_prepared read it, and
 * hbrbc_g2_prepare makes Miller lines of out192 -- and, where the pointers are
 * non-null, to out192 + 192 i and out96 + 96 i.  status_out[i]: 0 ok, 2 an
 * invalid description (zero bytes), 3 the point at infinity after the
 * cofactor.  words_out[i] (nullable): the stream words the sampler drew (25
 * per attempt, 12 more per rejected Fq draw).  Device memory, async on
 * `stream`; two launches, nothing is read back. */
int hbrbc_hash_g2_batch(const uint8_t *msgs, const uint32_t *offsets, size_t count, size_t total,
                        void *out_table, uint8_t *out192, uint8_t *out96, uint8_t *status_out,
                        uint32_t *words_out, void *stream);
int hbrbc_hash_g1_g2_batch(const uint8_t *u48, const uint8_t *msgs, const uint32_t *offsets,
                           size_t count, size_t total, void *out_table, uint8_t *out192,
                           uint8_t *out96, uint8_t *status_out, uint32_t *words_out,
                           void *stream);
/* xor_with_hash: row i is data[offsets[i] .. offsets[i + 1]) (ranges as above,
 * offsets ascending), XORed with the low bytes of the stream words of
 * SHA3-256(g48 + 48 i) -- the compressed encoding of g -- into the same range
 * of `out` (out may be data; bytes outside the rows are not touched).  Its own
 * inverse.  One lane per 16 bytes of a row, so long rows spread over the
 * device.  status_out[i]: 0 ok, 2 an invalid range (neither read nor
 * written).  workspace >= hbrbc_xor_with_hash_workspace_size(count) bytes.
 * Device memory, async on `stream`; nothing is read back. */
size_t hbrbc_xor_with_hash_workspace_size(size_t count);
int hbrbc_xor_with_hash_batch(const uint8_t *g48, const uint8_t *data, const uint32_t *offsets,
                              size_t count, size_t total, uint8_t *out, uint8_t *status_out,
                              void *workspace, void *stream);

/* ---- the Broadcast state machine, batched --------------- */
/* Many instances x nodes of `Broadcast` (broadcast.rs:228-558) in synchronous
 * rounds: what a node emits in round t is delivered in round t + 1, each node
 * handling its inbox in (sender index, emission order).  Round 0 is the
 * proposers' broadcast().  A message is a record of 1 + W uint32 words
 * (W = ceil(n / 32)): word 0 = kind | root << 8 | index << 16 | tampered << 24
 * (kind: 0 Value, 1 Echo, 2 Ready, 3 CanDecode, 4 EchoHash, 5 the
 * ProposeAdversary's injected broadcasts), words 1..W = recipient bits.
 * Proofs travel by reference (root c = codeword slot of the instance, index
 * j, tampered copy or not): proof_ok holds Proof::validate of each (the
 * batched validate kernel), decode_ok decode_from_shards of each root (the
 * batched decode).  Nodes [node_lo, node_lo + nodes) are hosted here; the
 * previous round's records of every sender s sit in `in` at block s / R, row
 * s % R ([G][count][R][max_out][1 + W]); this round's go to `out`
 * ([count][nodes][max_out][1 + W]); out_count bit 31 flags an overflow.
 * Fault records: blamed node << 8 | FaultKind (error.rs:28-50 order). */
#define HBRBC_SM_NONE 0xFF
enum hbrbc_sm_role {            /* per instance and node */
    HBRBC_SM_HONEST = 0,
    HBRBC_SM_SILENT = 1,        /* emits nothing when handling a message (ProposeAdversary drop) */
    HBRBC_SM_CORRUPT_ECHO = 2,  /* its Echoes carry the tampered copy of its proof */
    HBRBC_SM_WITHHOLD_ECHO = 3  /* sends no Echo at all */
};
typedef struct hbrbc_sm_args {
    size_t count;                 /* instances */
    uint32_t node_lo, nodes;      /* hosted nodes */
    uint32_t rows_per_rank;       /* R of the `in` layout (n for one rank) */
    uint32_t roots;               /* codeword slots per instance, <= 8 */
    uint32_t max_out;             /* records per node per round */
    uint32_t max_faults;          /* fault records kept per node */
    int32_t round;
    const uint8_t *proposer;      /* [count] */
    const uint8_t *role;          /* [count][n] */
    const uint8_t *value_root;    /* [count][n]: root of the proposer's Value to node j, or NONE */
    const uint8_t *value_tamper;  /* [count][n]: that Value carries the tampered copy */
    const uint8_t *proof_ok;      /* [count][roots][2][n] */
    const uint8_t *decode_ok;     /* [count][roots] */
    const uint8_t *fake_from;     /* [count]: dispatcher of the injected broadcasts, or NONE */
    const uint8_t *fake_root;     /* [count]: their codeword slot */
    const uint32_t *fake_list;    /* [count][W]: the faulty nodes whose broadcasts are injected */
    const uint32_t *in;
    const uint32_t *in_count;     /* [G][count][R] */
    uint32_t *out;
    uint32_t *out_count;          /* [count][nodes] */
    uint8_t *state;               /* [count][nodes][hbrbc_sm_state_bytes], zeroed before round 0 */
    uint8_t *output_root;         /* [count][nodes]: decided root, NONE before */
    uint16_t *faults;             /* [count][nodes][max_faults] */
    uint32_t *fault_count;        /* [count][nodes] (may exceed max_faults) */
    uint32_t *emitted;            /* [2]: [0] += records emitted this round, [1] |= 1 if a
                                     node emitted more than max_out (out_count bit 31) */
    const uint32_t *active;       /* NULL, or: the round returns at once when *active == 0
                                     (every sender's previous round emitted nothing: the
                                     network is quiescent), so a host can enqueue several
                                     rounds and read the emitted counts back once */
    uint32_t flags;               /* HBRBC_SM_NO_FAKE: no instance has a fake_from node, so no
                                     inbox holds a Fake record and those of rounds >= 2 hold only
                                     Echo, EchoHash, Ready and CanDecode records: round 1 runs a
                                     kernel without the Fake handler, rounds >= 2 one without the
                                     Value handler too (a record of a kind left out, or a
                                     fake_from node, sets emitted[1] bit 1, the caller's error).
                                     HBRBC_SM_SUBSET: the instances are the broadcasts of Subset
                                     proposal states (see hbrbc_subset_round): a node that
                                     enters a round with output_root != NONE handles nothing
                                     (round 0 included), and a node that decides takes no
                                     further record of that round -- the ProposalState has
                                     dropped the Broadcast */
} hbrbc_sm_args;
#define HBRBC_SM_NO_FAKE 1u
#define HBRBC_SM_SUBSET 2u
/* output_root of a broadcast its proposal state dropped without an output:
 * written by hbrbc_subset_round for a rejected proposal, preset by the caller
 * for a dead node (root slots are < 8) */
#define HBRBC_SM_DROPPED 0xFE
size_t hbrbc_sm_state_bytes(size_t n, size_t roots);
/* One round for the hosted nodes of every instance (ctx gives n, f, k). */
int hbrbc_sm_round(hbrbc_ctx *ctx, const hbrbc_sm_args *args, void *stream);

/* ---- the BinaryAgreement state machine, batched ------------------------ */
/* Many instances x nodes of `BinaryAgreement` (binary_agreement.rs:206-521,
 * sbv_broadcast.rs:67-187, threshold_sign.rs:127-270) in the synchronous
 * rounds of hbrbc_sm_round: what a node emits in round t is delivered in
 * round t + 1, each node handling its inbox in (sender index, emission
 * order); round 0 is propose(input) of every node that has an input.  All n
 * nodes of an instance are hosted (one rank).  A message is a record of
 * 1 + W uint32 words (W = ceil(n / 32)): word 0 = kind | value << 8 |
 * tampered << 12 | epoch << 16 (kind: 0 BVal, 1 Aux, 2 Conf, 3 Term, 4 Coin;
 * value: a bool, or the two bits of a Conf's BoolSet, 1 = {false}, 2 =
 * {true}, 3 = both), words 1..W = recipient bits.  The coin travels by
 * reference: a Coin record names its sender's signature share of coin slot
 * q = (epoch - 2) / 3 (or a tampered copy); share_ok holds the outcome of the
 * share check of each, coin the parity of the slot's combined signature (a
 * BLS threshold signature is unique, so the parity does not depend on which
 * f + 1 valid shares a node combined).  Records of the previous round sit in
 * `in` ([count][n][max_out][1 + W], counts in in_count), this round's go to
 * `out`; out_count bit 31 flags an overflow.  Messages of a future epoch wait
 * in a ring of queue_epochs slots per sender; one beyond the ring sets
 * emitted[1] bit 1 (the run is to be rejected).  Fault records: blamed node
 * << 8 | FaultKind (binary_agreement/mod.rs:110-129 order, 5 = CoinFault(
 * UnverifiedSignatureShareSender)). */
#define HBRBC_BA_NONE 0xFF
enum hbrbc_ba_role {            /* per instance and node: what LEAVES the node */
    HBRBC_BA_HONEST = 0,
    HBRBC_BA_SILENT = 1,        /* nothing */
    HBRBC_BA_TWO_FACED = 2,     /* every record twice: as it is to the recipients outside the
                                   instance's flip mask, complemented (b -> !b, {false} <->
                                   {true}; both and Coin unchanged) to those inside */
    HBRBC_BA_BAD_COIN = 3,      /* its Coin records carry the tampered flag */
    HBRBC_BA_REPLAY = 4,        /* every record twice in a row */
    HBRBC_BA_AHEAD = 5,         /* every record's epoch raised by the instance's `ahead` */
    HBRBC_BA_REPLAY_AHEAD = 6   /* both: twice in a row, epoch raised (duplicates in the queue) */
};
enum hbrbc_ba_form {            /* hbrbc_ba_args.form */
    HBRBC_BA_FORM_AUTO = 0,     /* by n: STAGED below 128, STAGED_W3 from there while an
                                   instance's cores fit the LDS, GLOBAL beyond */
    HBRBC_BA_FORM_GLOBAL = 1,   /* state read and written where it lies; 3 waves per SIMD */
    HBRBC_BA_FORM_STAGED = 2,   /* epoch, flags and sender masks of a workgroup's instances in
                                   LDS for the round (the queue ring stays in global memory) */
    HBRBC_BA_FORM_STAGED_W3 = 3 /* the same at 3 waves per SIMD (fewer registers, more
                                   resident waves) */
};
typedef struct hbrbc_ba_args {
    size_t count;                 /* instances */
    uint32_t n;                   /* validators per instance, 1..255; f = (n - 1) / 3 */
    uint32_t max_out;             /* records per node per round */
    uint32_t max_faults;          /* fault records kept per node */
    uint32_t queue_epochs;        /* slots of the future-epoch ring per sender, 1..16 */
    uint32_t coins;               /* coin slots in share_ok / coin */
    int32_t round;
    uint32_t form;                /* enum hbrbc_ba_form */
    const uint8_t *input;         /* [count][n]: 0, 1 or NONE (no propose) */
    const uint8_t *role;          /* [count][n] */
    const uint32_t *flip;         /* [count][W]: the recipients a TWO_FACED node lies to */
    const uint16_t *ahead;        /* [count]: epochs an AHEAD node adds */
    const uint8_t *share_ok;      /* [count][coins][2][n]: share of node j (tampered copy) valid */
    const uint8_t *coin;          /* [count][coins]: parity of the slot's signature */
    const uint32_t *in;
    const uint32_t *in_count;     /* [count][n] */
    uint32_t *out;
    uint32_t *out_count;          /* [count][n] */
    uint8_t *state;               /* [count][n][hbrbc_ba_state_bytes], zeroed before round 0 */
    uint8_t *decision;            /* [count][n]: 0 / 1, NONE before */
    uint16_t *decision_epoch;     /* [count][n]: the epoch the node decided in */
    uint16_t *faults;             /* [count][n][max_faults] */
    uint32_t *fault_count;        /* [count][n] (may exceed max_faults) */
    uint32_t *emitted;            /* [2]: [0] += records emitted this round, [1] |= 1 a node
                                     emitted more than max_out, 2 a record for an epoch beyond
                                     the queue ring, 4 a node reached a coin slot >= coins,
                                     8 an epoch of 65535, 16 more than queue_epochs + 2
                                     pending Term continuations (not reachable) */
    const uint32_t *active;       /* NULL, or: the round returns at once when *active == 0 */
} hbrbc_ba_args;
size_t hbrbc_ba_state_bytes(size_t n, size_t queue_epochs);
/* One round for every node of every instance. */
int hbrbc_ba_round(const hbrbc_ba_args *args, void *stream);

/* ---- Subset, batched: N broadcasts and N agreements a node ------------- */
/* Many instances x nodes of `Subset` (subset/subset.rs:103-169, subset/
 * proposal_state.rs:30-173) in the synchronous rounds of the two state
 * machines above.  Per Subset instance i there are n broadcast and n
 * agreement instances, (i, p) at index i n + p.  A round is two launches:
 * phase 1, hbrbc_sm_round with HBRBC_SM_SUBSET over the count n broadcast
 * instances (proposer[i n + p] = p, all nodes hosted), handles every node's
 * broadcast records; phase 2, hbrbc_subset_round, one thread per (instance,
 * node), then
 *  1. for every proposer in order whose broadcast has an output_root: an
 *     Ongoing proposal becomes HasValue and calls propose(true) on its
 *     agreement, an Accepted one becomes Complete(true) and is output;
 *  2. handles the node's agreement records in (proposer, sender, emission)
 *     order with the handlers of hbrbc_ba_round; a `true` decision accepts the
 *     proposal (and outputs it if the value is there), a `false` one completes
 *     it and writes HBRBC_SM_DROPPED into the broadcast's output_root; at the
 *     record that takes the accepted count to N - f, propose(false) runs at
 *     once on every proposal that still has its agreement, in proposer order
 *     (those whose records of this round are still to come included); when
 *     every proposal is complete the node outputs Done.
 * Round 0 is Subset::propose of every live node: phase 1's round 0, then
 * phase 2 with empty inboxes (it initialises the agreements' epoch-0 coin
 * state and the proposal states: HBRBC_SM_DROPPED in output_root gives
 * Complete(false), the caller's preset for a dead node).  The agreement
 * tables keep the layouts of hbrbc_ba_args with count n instances.  The global
 * state form only. */
enum hbrbc_subset_proposal {    /* the proposal-state byte (proposal_state.rs:17-28) */
    HBRBC_SUBSET_ONGOING = 0,
    HBRBC_SUBSET_HAS_VALUE = 1,
    HBRBC_SUBSET_ACCEPTED = 2,
    HBRBC_SUBSET_COMPLETE_FALSE = 3,
    HBRBC_SUBSET_COMPLETE_TRUE = 4
};
#define HBRBC_SUBSET_DONE 0xFF   /* the Done marker of an output sequence */
typedef struct hbrbc_subset_args {
    size_t count;                 /* Subset instances */
    uint32_t n;                   /* validators per instance, 1..255; f = (n - 1) / 3 */
    uint32_t max_out;             /* agreement records per node, proposer and round */
    uint32_t max_faults;          /* agreement fault records kept per node and proposer */
    uint32_t queue_epochs;        /* slots of the future-epoch ring per sender, 1..16 */
    uint32_t coins;               /* coin slots in share_ok / coin */
    int32_t round;
    const uint8_t *role;          /* [count n][n]: enum hbrbc_ba_role */
    const uint32_t *flip;         /* [count n][W] */
    const uint16_t *ahead;        /* [count n] */
    const uint8_t *share_ok;      /* [count n][coins][2][n] */
    const uint8_t *coin;          /* [count n][coins] */
    const uint32_t *in;
    const uint32_t *in_count;     /* [count n][n] */
    uint32_t *out;
    uint32_t *out_count;          /* [count n][n]; every round clears the node's own counts */
    uint8_t *state;               /* [count n][n][hbrbc_ba_state_bytes], zeroed before round 0 */
    uint8_t *decision;            /* [count n][n]: 0 / 1, NONE before */
    uint16_t *decision_epoch;     /* [count n][n] */
    uint16_t *faults;             /* [count n][n][max_faults] */
    uint32_t *fault_count;        /* [count n][n], zeroed before round 0 */
    uint8_t *output_root;         /* [count n][n]: phase 1's; read, and HBRBC_SM_DROPPED written */
    uint8_t *proposal;            /* [count n][n]: enum hbrbc_subset_proposal of node j about
                                     proposer p at (i n + p) n + j; written in round 0 */
    uint32_t *node_state;         /* [count][n]: accepted count | complete count << 8 | voted
                                     false << 16 | Done << 17; written in round 0 */
    uint8_t *out_seq;             /* [count][n][n + 1]: the accepted proposers in output order,
                                     then HBRBC_SUBSET_DONE */
    uint32_t *out_len;            /* [count][n], zeroed before round 0 */
    uint32_t *emitted;            /* [2]: [0] += agreement records emitted this round, [1] |=
                                     the flag bits of hbrbc_ba_args.emitted */
    const uint32_t *active;       /* NULL, or: the round returns at once when *active == 0 (the
                                     records of both protocols in the previous round) */
} hbrbc_subset_args;
/* Phase 2 of one round for every node of every instance. */
int hbrbc_subset_round(const hbrbc_subset_args *args, void *stream);

/* ---- HoneyBadger, batched: one epoch, Subset then N decryptions a node -- */
/* One epoch of `HoneyBadger` (honey_badger/epoch_state.rs:195-395,
 * threshold_decrypt.rs:115-253 as a message handler, honey_badger.rs:100-116,
 * 172-185) for every node of `count` networks, in the rounds of the Subset
 * above.  A round is three launches: hbrbc_sm_round, hbrbc_subset_round, then
 * phase 3, hbrbc_hb_round, one thread per (instance, node, proposer).  A
 * node's phase 3 does, in this order,
 *  (a) the entries of phase 2's out_seq past the node's cursor, in sequence
 *      order (with HBRBC_HB_ALL_AT_END none before Done is there): a
 *      contribution of proposer p is Complete in a plain instance; in an
 *      encrypted one ct_state of the delivered root slot gives the fault that
 *      blames p or the ciphertext, then remove_invalid_shares logs its faults
 *      in sender order, the node's own share is stored and emitted, try_output
 *      runs.  Done fixes the accepted set and removes the decryption state of
 *      every other proposer, one UnexpectedDecryptionShare per stored sender;
 *  (b) the previous round's DecryptionShare records for p in (sender,
 *      emission) order (not the node's own).
 * The batch leaves at the first moment every accepted proposer is Complete
 * after Done; HoneyBadger drops what arrives for the epoch after that: when
 * the batch leaves in (a) no share record of the round is handled; when it
 * leaves in (b), at p* -- the highest proposer whose decryption completes in
 * this round -- the threads of proposers above p* handle none (a reduction
 * over the node's proposer threads); from the next round on the node handles
 * nothing.  BatchDeserializationFailed is logged with the batch.
 * Ciphertexts, shares and plaintexts travel by reference: a share record is
 * one byte per (instance, proposer, sender) and round,
 *   bits 0..1 the number of copies (0..2), bit 2 + c the variant of copy c
 *   (0 the sender's honest share, 1 its tampered one),
 * and share_ok holds `verify_decryption_share` of both variants against the
 * ciphertext of each root slot (g = sum lambda_i share_i does not depend on
 * which f + 1 valid shares are combined, so the plaintext is the slot's).
 * The simulation takes the outcome of Ciphertext::verify and of the bincode
 * of a Ciphertext from the caller (the hashes have entries of their own,
 * hbrbc_hash_g1_g2_batch), hence ct_state and undeserialisable are inputs.  Fault records:
 * blamed node << 8 | kind (enum hbrbc_hb_fault). */
enum hbrbc_hb_role {            /* per instance and node: the decryption layer's sending side */
    HBRBC_HB_HONEST = 0,
    HBRBC_HB_SILENT = 1,        /* sends no share */
    HBRBC_HB_BAD_SHARE = 2,     /* sends its variant-1 share */
    HBRBC_HB_TWICE = 3,         /* every share as two copies in one round */
    HBRBC_HB_STRAY = 4,         /* in round 1, and again in the round after it sees Done, a
                                   variant-1 share for every proposer, ahead of its own */
    HBRBC_HB_ABSENT = 5         /* a dead node: handles and sends nothing */
};
enum hbrbc_hb_fault {
    HBRBC_HB_UNEXPECTED_SHARE = 0,     /* UnexpectedDecryptionShare */
    HBRBC_HB_DESERIALIZE_CT = 1,       /* DeserializeCiphertext */
    HBRBC_HB_INVALID_CT = 2,           /* InvalidCiphertext */
    HBRBC_HB_BATCH_DESERIALIZE = 3,    /* BatchDeserializationFailed */
    HBRBC_HB_MULTIPLE_SHARES = 4,      /* DecryptionFault(MultipleDecryptionShares) */
    HBRBC_HB_UNVERIFIED_SHARE = 5      /* DecryptionFault(UnverifiedDecryptionShareSender) */
};
enum hbrbc_hb_decryption {      /* dstate bits 0..2; bit 3 (HBRBC_HB_ACCEPTED): p was output */
    HBRBC_HB_DS_ABSENT = 0,
    HBRBC_HB_DS_NO_CIPHERTEXT = 1,     /* Ongoing, shares waiting for the ciphertext */
    HBRBC_HB_DS_ONGOING = 2,           /* Ongoing with the ciphertext, own share sent */
    HBRBC_HB_DS_COMPLETE = 3,
    HBRBC_HB_DS_REMOVED = 4            /* removed at Done: the proposer was not accepted */
};
#define HBRBC_HB_ACCEPTED 8u
#define HBRBC_HB_ENCRYPTED 1u    /* inst_flags: require_decryption */
#define HBRBC_HB_ALL_AT_END 2u   /* inst_flags: SubsetHandlingStrategy::AllAtEnd */
#define HBRBC_HB_NO_BATCH (-1)
typedef struct hbrbc_hb_args {
    size_t count;                 /* networks (Subset instances) */
    uint32_t n;                   /* validators, 1..255; f = (n - 1) / 3; W = ceil(n / 32) */
    uint32_t roots;               /* root slots per broadcast in the tables, 1..8 */
    uint32_t max_faults;          /* fault records kept per node and proposer */
    int32_t round;
    const uint8_t *inst_flags;    /* [count]: HBRBC_HB_ENCRYPTED | HBRBC_HB_ALL_AT_END */
    const uint8_t *role;          /* [count][n]: enum hbrbc_hb_role */
    const uint8_t *ct_state;      /* [count n][roots]: 0 valid, 1 does not deserialise, 2 fails
                                     Ciphertext::verify */
    const uint8_t *undeserialisable; /* [count n][roots]: the contribution does not deserialise */
    const uint8_t *share_ok;      /* [count n][roots][2][n] */
    const uint8_t *output_root;   /* [count n][n]: phase 1's (the delivered root slot) */
    const uint8_t *out_seq;       /* [count][n][n + 1]: phase 2's */
    const uint32_t *out_len;      /* [count][n] */
    const uint8_t *in;            /* [count n][n]: the previous round's share records, by
                                     (proposer, sender) */
    uint8_t *out;                 /* [count n][n]: this round's; zeroed by the caller */
    uint32_t *node_state;         /* [count][n]: out_seq cursor | saw Done << 16 | batch out
                                     << 17; zeroed before round 0 */
    int32_t *done_round;          /* [count][n]: the round the node saw Done in */
    int32_t *batch_round;         /* [count][n]: HBRBC_HB_NO_BATCH before round 0 */
    uint8_t *dstate;              /* [count n][n]: enum hbrbc_hb_decryption | HBRBC_HB_ACCEPTED
                                     of node j about proposer p at (i n + p) n + j; zeroed */
    uint32_t *mask;               /* [count n][2 W][n]: words 0..W-1 the senders whose share is
                                     stored, W..2W-1 the stored shares' variants; zeroed */
    uint16_t *faults;             /* [count n][n][max_faults] */
    uint32_t *fault_count;        /* [count n][n] (may exceed max_faults); zeroed */
    uint32_t *emitted;            /* [2]: [0] += share records (copies) emitted this round,
                                     [1] |= 1 a root slot, ct_state or role out of range, 2 an
                                     out_seq entry or length out of range */
    const uint32_t *active;       /* NULL, or: the round returns at once when *active == 0 (the
                                     records of all three protocols in the previous round) */
} hbrbc_hb_args;
/* Phase 3 of one round for every node of every instance. */
int hbrbc_hb_round(const hbrbc_hb_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HBRBC_H */
