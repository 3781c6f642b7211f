/* bpgpu.h -- C ABI of the MI355X-native Bulletproofs verification engine
 * (libbpgpu.so).
 *
 * The reference (dalek-cryptography/bulletproofs, Rust) has no FFI layer: its
 * verification hot path is one call into a dependency,
 *     RistrettoPoint::optional_multiscalar_mul(scalars, points)
 * made at src/range_proof/mod.rs:421-445 (range proofs),
 * src/inner_product_proof.rs:308-319 (stand-alone inner-product proofs) and
 * src/r1cs/verifier.rs:459-491 (R1CS).  This header is the boundary a Rust
 * maintainer would bind with `extern "C"` to move that call -- and, one level
 * up, whole batches of RangeProof::verify_multiple -- onto the GPU.  Every
 * entry point below names the reference interface it replaces.  INTEGRATION.md
 * shows the Rust-side binding.
 *
 * Conventions
 *   - plain pointers and sizes only; caller owns every buffer; nothing is
 *     retained after a call returns (except what *_load / *_create upload).
 *   - scalars : 32 bytes little-endian, canonical (< l), as Scalar::as_bytes().
 *   - points  : 32 bytes, CompressedRistretto encodings (RFC 9496).
 *   - return  : BPGPU_OK or a negative BPGPU_ERR_* code; per-item results in
 *     status / verdict byte arrays.  The library never aborts the process.
 *   - entry points without suffix take HOST pointers and do H2D/D2H themselves;
 *     `_dev` twins take DEVICE pointers plus a hipStream_t (as void*; NULL =
 *     the context's own stream), enqueue asynchronously and return.
 *   - one context serves one device; calls on one context are serialised by an
 *     internal mutex (the reference's calls are &self and re-entrant; use one
 *     context per host thread for concurrency).  A context owns ONE set of device
 *     scratch buffers: work enqueued on it is ordered.  If consecutive `_dev` calls
 *     on one context name different streams, the library makes the later stream
 *     wait (hipStreamWaitEvent) for the earlier call's kernels, so results stay
 *     correct -- but only one context per stream gives overlap.
 *   - throughput: a batch is a chain of a few dependent launches, several of them
 *     narrow, so one stream cannot fill the device.  Keep many batches in flight:
 *     one context per HIP stream (the generator tables are shared by the contexts
 *     of a process), ~48 streams, and GPU_MAX_HW_QUEUES=16 in the environment
 *     (ROCm's default of 4 hardware queues serialises the streams).
 */
#ifndef BPGPU_H
#define BPGPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BPGPU_OK 0
#define BPGPU_ERR_INVALID_ARG (-1)
#define BPGPU_ERR_HIP (-2)         /* a HIP runtime call failed; see bpgpu_last_error */
#define BPGPU_ERR_NO_GENS (-3)     /* generators not loaded, or too few for the request */
#define BPGPU_ERR_NO_DEVICE (-4)
#define BPGPU_ERR_BAD_GENERATOR (-5) /* a generator encoding passed to bpgpu_gens_load does not decode */
#define BPGPU_ERR_HW_QUEUES (-6)   /* bpgpu_pool_create: GPU_MAX_HW_QUEUES is set to a value the pool's lanes cannot overlap on */

/* per-MSM status (msm entry points) */
#define BPGPU_MSM_OK 0
#define BPGPU_MSM_BAD_POINT 1      /* some point failed to decode: optional_multiscalar_mul -> None */
#define BPGPU_MSM_BAD_SCALAR 2     /* some scalar is not canonical */

/* per-proof verdicts: ProofError of src/errors.rs:12-54 */
#define BPGPU_VERDICT_OK 0
#define BPGPU_VERDICT_VERIFICATION_ERROR 1
#define BPGPU_VERDICT_FORMAT_ERROR 2
#define BPGPU_VERDICT_INVALID_BITSIZE 3
#define BPGPU_VERDICT_INVALID_GENERATORS_LENGTH 4

typedef struct bpgpu_ctx bpgpu_ctx;

/* ---- context ------------------------------------------------------------- */
int bpgpu_version(void);
/* device: HIP device ordinal.  Fails with BPGPU_ERR_NO_DEVICE when no GPU is usable
 * (there is no CPU fallback). */
int bpgpu_ctx_create(int device, bpgpu_ctx **out);
void bpgpu_ctx_destroy(bpgpu_ctx *ctx);
const char *bpgpu_last_error(bpgpu_ctx *ctx);
/* Tunables (set before bpgpu_gens_*):
 *   "fixed_window_bits"     window W of the generator tables, 2..20; 0 (default) = the W with the fewest windows whose
 *                           table (n_gens * ceil(255/W) * 2^(W-1) * 128 bytes) fits fixed_table_max_bytes
 *   "fixed_table_max_bytes" HBM budget of the tables (default 160 GiB of the MI355X's 288 GB; a context settles for a
 *                           smaller window when the allocation fails)
 *   "fixed_splits"          workgroups the generator terms of one proof block are split over (0 = auto)
 *   "bucket_min_terms"      variable-base terms per MSM from which the bucket (Pippenger) path is taken instead of the
 *                           table-lookup one (default 1536; the batch-combined check, one MSM over all proofs' terms,
 *                           switches at 32768 terms unless this option is set; a huge value disables the bucket
 *                           path, 1 forces it).  Results are bit-identical either way.
 *   "host_sync_blocking"    1: host-pointer entry points wait for their results on a blocking event (the calling
 *                           thread sleeps: right for many host threads, one context each); 0 (default): spin-wait
 *   "prover_constant_time"  1: the prover's secret-dependent commitments through the constant-time walk (bpgpu_rangeproof_prove_batch)
 *   "transcript_script"     0: byte-wise transcript replay instead of the per-shape script (csrc/rp_script.h; for A/B only)
 *   "horner_lanes"          lanes per Horner chain of the proof-specific terms in the range-proof path:
 *                           1 (one lane per proof: least work, longest chain; on chains of >= 2048 proofs it runs on the context's
 *                           second stream beside the table walk), 4 (a quad per proof: twice the instructions, half the latency),
 *                           64 (one wavefront per chain: lowest latency of a single small batch),
 *                           0 = auto (default): 64 up to 256 proofs (a small batch alone is a latency matter: 0.61 instead of 0.85 ms
 *                           for a single proof); 1 on chains of >= 8192 proofs, and on chains of >= 2048 when the pool knows that
 *                           other chains run beside them; 4 otherwise
 *   "a_outside"             1 (default): on chains of >= 2048 proofs A, whose coefficient is 1, is added after the Horner chain instead of
 *                           going through a table and the window sums; 0: like every other point (for A/B)
 *   "per_proof_radix"       radix of the proofs' own points: 0 / 16 (default), 32 (16-entry tables, 51 windows; takes effect on chains
 *                           of >= 2048 proofs; measured +1 % steady, -4 % on bursts)
 *   "split_stage3"          -1 (default): the window sums as their own launch on chains of >= 2048 proofs; 0 / 1: never / always
 *   "transcript_coop"       1 (default): launch chains of up to 256 proofs replay their transcripts 32 lanes per proof (Keccak-f[1600]
 *                           with one state word per lane: one blocking call of 1 proof 0.62 -> 0.53 ms); 0: one lane per proof everywhere
 *   narrow chains (up to 256 proofs: the crate's own call shape, the combining queue's small chains; round 6):
 *   "coop_split"            1 (default): launch 1 stages the proof, the script and its masks in LDS, the 5 + k challenges are reduced on
 *                           5 + k lanes, the k + 1 inversions run on k + 1 lanes at once, the basepoint coefficients are a role of launch 3;
 *                           0: the group's leader does all of it (k_rp_stage1_coop 227 -> 157 us for one proof)
 *   "exp_single"            1 (default): the generator-exponent role with one index per lane (launch 3: 73 -> 33 us); 0: as wide chains
 *   "narrow_chunk"          per-proof points per (chunk, window) lane of launch 3: 0 = 8 (default), 2 .. 32; 32 = one chunk
 *   "narrow_walk"           1 (default): the table walk with lane = split, a proof's partial sums folded inside launch 4 (finish 40 -> 5 us)
 *   "narrow_hi_max"         chains of up to this many proofs (default 32; 0: never) give every per-proof point a second table, of its
 *                           2^128 multiple (a wavefront per point, beside the transcript), and run a 32-window Horner chain
 *   "narrow_hi4_max"        chains of up to this many proofs (default 4; 0 = never) take THREE more tables per point (2^64 P, 2^128 P, 2^192 P) and a
 *                           16-window chain (one blocking call 0.315 -> 0.29 ms)
 *   "narrow_fused_finish"   1 (default): verdict-only calls, chains of 8 .. 256 proofs: the last workgroup of a proof in launch 4 adds up its pieces
 *                           and writes the verdict (no finish launch); 0: k_finish1
 *   "msm_narrow"            1 (default): bpgpu_msm_batch with at most 16 MSMs of at most 768 terms in all (the boundary function called from one
 *                           thread with a Straus-size MSM) runs three launches: decode beside a wavefront per term that builds the table of
 *                           2^128 P, window sums in ~sqrt(N) chunks, one tail (32-window Horner chain + encoding); 0: the batch form
 *   "msm_fork"              1 (default): bpgpu_msm_batch_shared's generator half on the context's second stream beside the per-MSM points; 0: one stream
 *   "bucket_chain"          0 (default): MSMs of up to 6144 variable-base terms take the fused bucket chain (csrc/bucket2.h: decode, one LDS
 *                           sort + accumulate workgroup per (MSM, window), one tail launch); 1: bucket.h's chain everywhere (for A/B)
 *   "bucket_lanes"          lanes of a (MSM, window) workgroup of the fused chain: 0 = by batch width (default), 64, 128, 256
 *   "bucket_fast_tail"      -1 (default): batches of fewer than 48 MSMs end with the short-chain tail (leaves of 4 buckets, shuffle sums);
 *                           0 / 1: never / always
 *   "exponent_pairs"        1 (default): the generator-exponent role handles index i together with nm-1-i (they share s_i and s_i^-1: -24 % of
 *                           the role's Montgomery products); 0: four consecutive indices per lane (for A/B)
 *   "fb_walk_waves"         wavefronts the generator half of a fused chain is cut into (0 = 2048)
 *   "r1cs_rlc_max_terms"    proof-specific terms of one combination of bpgpu_r1cs_verify_rlc (0 = 2^24, the most); more form several MSMs
 * get_option additionally answers "fixed_table_bytes" and the effective "fixed_window_bits".
 * Returns BPGPU_ERR_INVALID_ARG for unknown keys. */
int bpgpu_ctx_set_option(bpgpu_ctx *ctx, const char *key, int64_t value);
int bpgpu_ctx_get_option(bpgpu_ctx *ctx, const char *key, int64_t *value);
int bpgpu_synchronize(bpgpu_ctx *ctx);

/* ---- generators ------------------------------------------------------------
 * Replace BulletproofGens::new(gens_capacity, party_capacity)
 * (src/generators.rs:157-204) and PedersenGens::default() (generators.rs:44-53)
 * as held by a verifier.  Both build the fixed-base window tables in HBM. */
/* derive the generators on the device exactly as the reference does
 * (SHAKE256("GeneratorsChain" || 'G'/'H' || u32le(party)) -> from_uniform_bytes;
 *  B = basepoint, B_blinding = hash_from_bytes::<Sha3_512>(compress(B))). */
int bpgpu_gens_create(bpgpu_ctx *ctx, size_t gens_capacity, size_t party_capacity);
/* or load them from encodings the caller already has; G/H party-major:
 * G[(party * gens_capacity + i) * 32], as BulletproofGens::G_vec[party][i]. */
int bpgpu_gens_load(bpgpu_ctx *ctx, size_t gens_capacity, size_t party_capacity,
                    const uint8_t *G, const uint8_t *H, const uint8_t B[32], const uint8_t B_blinding[32]);
/* read back the encodings (any pointer may be NULL) */
int bpgpu_gens_export(bpgpu_ctx *ctx, uint8_t *G, uint8_t *H, uint8_t B[32], uint8_t B_blinding[32]);
/* A service that verifies TWO shapes (say m = 16 and m = 1 proofs) on one generator set: BulletproofGens::new(gens_capacity,
 * party_capacity) serves every n <= gens_capacity, m <= party_capacity (src/generators.rs:157-259), but the window table that replaces
 * the doublings is sized for the whole set -- at (64, 16) that is W = 16, and m = 1 proofs walked it 9 % slower than through their own
 * W = 20 table.  This adds a SECOND table over the sub-set (n2, m2) of the loaded generators and re-balances both windows under the
 * context's one budget ("fixed_table_max_bytes"): the pair minimising nwin(W1) / nwin(W1 alone) + nwin(W2) / nwin(W2 alone) -- under
 * 160 GiB, (64, 16) + (64, 1): W = 15 (73 GB) + W = 19 (61 GB).  Range proofs with n <= n2 and m <= m2 then walk the secondary table
 * (results are the same group elements: bit-identical verdicts and encodings).  Options (get): "secondary_window_bits",
 * "secondary_table_bytes", "secondary_shape_n" / "_m"; "fixed_window_bits" reports the re-balanced primary window.  Calling it again
 * replaces the secondary shape; bpgpu_gens_create / _load drop it. */
int bpgpu_gens_add_shape(bpgpu_ctx *ctx, size_t n2, size_t m2);

/* ---- multiscalar multiplication ---------------------------------------------
 * bpgpu_msm_batch: nbatch independent calls of
 *   RistrettoPoint::optional_multiscalar_mul(scalars_b, points_b.decompress())
 * (trait curve25519_dalek::traits::VartimeMultiscalarMul; call sites
 * range_proof/mod.rs:421, inner_product_proof.rs:308, r1cs/verifier.rs:459).
 *   n_terms[b]  : number of (scalar, point) pairs of MSM b (host array, may be 0)
 *   scalars     : sum(n_terms) x 32 bytes, MSM after MSM
 *   points      : sum(n_terms) x 32 bytes
 *   out         : nbatch x 32 bytes = compress(sum_i scalars[i] * points[i]);
 *                 all-zero when status[b] != 0
 *   status      : nbatch bytes, BPGPU_MSM_* */
int bpgpu_msm_batch(bpgpu_ctx *ctx, size_t nbatch, const uint32_t *n_terms,
                    const uint8_t *scalars, const uint8_t *points, uint8_t *out, uint8_t *status);
int bpgpu_msm_batch_dev(bpgpu_ctx *ctx, size_t nbatch, const uint32_t *n_terms_host,
                        const void *d_scalars, const void *d_points, void *d_out, void *d_status, void *stream);

/* bpgpu_msm_batch_shared: the verification "mega-check" shape
 * (range_proof/mod.rs:421-443): every MSM of the batch is
 *     sum_{g < 2nm+2} gen_scalars[b][g] * Gen_g  +  sum_{u < n_unique} uniq_scalars[b][u] * uniq_points[b][u]
 * with Gen = (B_blinding, B, G(n,m)..., H(n,m)...) taken from the loaded
 * generators in the reference's order (mod.rs:439-442).  The generator terms
 * use the precomputed tables; results are bit-identical to bpgpu_msm_batch on
 * the same terms.  Requires n <= gens_capacity, m <= party_capacity. */
int bpgpu_msm_batch_shared(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch, size_t n_unique,
                           const uint8_t *gen_scalars, const uint8_t *uniq_scalars, const uint8_t *uniq_points,
                           uint8_t *out, uint8_t *status);
int bpgpu_msm_batch_shared_dev(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch, size_t n_unique,
                               const void *d_gen_scalars, const void *d_uniq_scalars, const void *d_uniq_points,
                               void *d_out, void *d_status, void *stream);

/* ---- Merlin transcripts across the boundary ------------------------------------------
 * The reference's verifiers take `transcript: &mut Transcript` (range_proof/mod.rs:345-353,
 * inner_product_proof.rs:260-270): it may already hold application messages and is left advanced.
 * A transcript crosses this ABI as its 208-byte state, which is the in-memory image of merlin's
 * Strobe128 { state: [u8; 200] (align 8), pos: u8, pos_begin: u8, cur_flags: u8 }:
 *   [0,200) sponge bytes, [200] pos, [201] pos_begin, [202] cur_flags, [203,208) zero.
 * The three helpers run on the host (no GPU needed) and are Transcript::new / append_message /
 * challenge_bytes of src/transcript.rs's dependency (merlin 2.x) on that representation. */
#define BPGPU_TRANSCRIPT_BYTES 208
int bpgpu_transcript_new(const uint8_t *label, size_t label_len, uint8_t state[BPGPU_TRANSCRIPT_BYTES]);
int bpgpu_transcript_append_message(uint8_t state[BPGPU_TRANSCRIPT_BYTES], const uint8_t *label, size_t label_len,
                                    const uint8_t *msg, size_t msg_len);
int bpgpu_transcript_challenge_bytes(uint8_t state[BPGPU_TRANSCRIPT_BYTES], const uint8_t *label, size_t label_len,
                                     uint8_t *out, size_t out_len);

/* ---- batches of transcripts, built and bound on the GPU ------------------------------------
 * One SCRIPT of transcript operations applied to nbatch transcripts (rows) at once: the labels are shared, the messages are
 * per row and may have per-row lengths.  The states that come out are what every `_ts` entry point takes as `transcripts`
 * (and every `_ts_dev` entry point as `d_transcripts`, with no further step).
 *
 * Operations (kind), each with a label of label_len <= BPGPU_TS_MAX_LABEL bytes:
 *   BPGPU_TS_APPEND            Transcript::append_message(label, msg_row): data = the messages, stride = bytes between rows
 *                              (0: ONE message of len bytes for every row), len <= BPGPU_TS_MAX_LEN the message length; with
 *                              lens (nbatch values, optional) row r appends its leading lens[r] <= len bytes: of its own row, of
 *                              which no byte past lens[r] is read, or (stride 0) of the one message, whose len bytes must all be
 *                              there.  append_point / append_scalar / the domain separators of src/transcript.rs:44-73.
 *   BPGPU_TS_APPEND_U64        append_u64(label, x_row): data = uint64_t values, stride 8 (one per row) or 0 (one for all); len ignored
 *   BPGPU_TS_CHALLENGE         challenge_bytes(label, len) into data[r * stride .. + len): len <= BPGPU_TS_MAX_CHALLENGE, stride >= len
 *   BPGPU_TS_CHALLENGE_SCALAR  the crate's challenge_scalar (transcript.rs:89-95): challenge_bytes(label, 64) through
 *                              Scalar::from_bytes_mod_order_wide, 32 canonical bytes into data[r * stride .. + 32): stride >= 32
 * A challenge needs a non-zero stride (one output per row); lens is for BPGPU_TS_APPEND only.  A script has at most
 * BPGPU_TS_MAX_OPS operations (nops = 0 copies the start states).
 *
 * Start states, exactly one of:
 *   new_label (new_label_len <= BPGPU_TS_MAX_LABEL; may be empty but not NULL): Transcript::new(new_label) for every row
 *   states_in with stride_in = 0: one BPGPU_TRANSCRIPT_BYTES state shared by the rows; stride_in = BPGPU_TRANSCRIPT_BYTES: one per
 *   row, at any STROBE positions.
 * states_out: nbatch x BPGPU_TRANSCRIPT_BYTES.  It may be states_in itself when stride_in = BPGPU_TRANSCRIPT_BYTES.
 *
 * bpgpu_transcript_batch takes HOST pointers, inside the ops too, and returns when the outputs are written; a malformed start state
 * (pos >= 166 or pos_begin > 166) and a lens[r] > len are BPGPU_ERR_INVALID_ARG.  Messages may be secret: the staging is cleared on
 * every exit.  bpgpu_transcript_batch_dev takes DEVICE pointers for states_in / states_out (4-byte aligned) and for data / lens
 * (lens 4-byte aligned; data of any alignment) inside the ops, while the op array, the labels and new_label are host memory; it
 * enqueues on `stream` and reads nothing back: a malformed row starts at position 0, as in the other `_dev` calls, and a
 * lens[r] > len appends len bytes.  Neither needs generators.  nbatch = 0 is BPGPU_OK.
 *
 * Rate (tools/transcript_batch_rate.py, one MI355X): 64 Ki states of `new` + a 32-byte session id in 0.047 ms through the `_dev` form and
 * 1.10 ms through the host form, against 2.40 ms for one host thread looping over the three helpers above and copying the states to
 * the device; with a 16-byte challenge and a 40-byte append on top 0.093 ms, 1.47 ms and 50.0 ms.
 *
 * CONTRACT: for every row, states_out and every challenge are byte for byte what bpgpu_transcript_new /
 * bpgpu_transcript_append_message / bpgpu_transcript_challenge_bytes produce when applied to that row's start state op by op. */
#define BPGPU_TS_APPEND 1
#define BPGPU_TS_APPEND_U64 2
#define BPGPU_TS_CHALLENGE 3
#define BPGPU_TS_CHALLENGE_SCALAR 4
#define BPGPU_TS_MAX_OPS 32
#define BPGPU_TS_MAX_LABEL 255
#define BPGPU_TS_MAX_LEN 65536
#define BPGPU_TS_MAX_CHALLENGE 4096
typedef struct bpgpu_ts_op {
    uint32_t kind;
    const uint8_t *label;
    size_t label_len;
    void *data;
    size_t stride;
    size_t len;
    const uint32_t *lens;
} bpgpu_ts_op;
int bpgpu_transcript_batch(bpgpu_ctx *ctx, size_t nbatch, const uint8_t *new_label, size_t new_label_len, const uint8_t *states_in,
                           size_t stride_in, const bpgpu_ts_op *ops, size_t nops, uint8_t *states_out);
int bpgpu_transcript_batch_dev(bpgpu_ctx *ctx, size_t nbatch, const uint8_t *new_label, size_t new_label_len, const void *d_states_in,
                               size_t stride_in, const bpgpu_ts_op *ops, size_t nops, void *d_states_out, void *stream);

/* ---- range-proof verification ---------------------------------------------------
 * nbatch independent calls of
 *   RangeProof::from_bytes(proof)?.verify_multiple_with_rng(bp_gens, pc_gens,
 *        &mut Transcript::new(label), &commitments, n, rng)
 * (src/range_proof/mod.rs:345-452, 504-538) with all proofs of one shape (n, m).
 *   proofs       : nbatch x proof_len bytes, proof_len = 32*(9 + 2*lg(n*m)) for valid input
 *   commitments  : nbatch x m x 32 bytes (value commitments V_j)
 *   label        : Merlin transcript label shared by the batch
 *   rng64        : nbatch x 64 bytes = what the rng would hand Scalar::random for the
 *                  batching challenge c (mod.rs:396); NULL = the library's thread_rng(): ONE 32-byte key per launch chain from a
 *                  per-thread ChaCha20 generator keyed by the OS CSPRNG, expanded on the device -- proof p's 64 bytes are block p
 *                  of ChaCha20(key) (nothing per proof is drawn or copied on the host)
 *   verdict      : nbatch bytes, BPGPU_VERDICT_*  (Ok(()) == 0)
 *   msm_out      : optional nbatch x 32 bytes, compress(mega_check) for parity tests */
int bpgpu_rangeproof_verify_batch(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch,
                                  const uint8_t *proofs, size_t proof_len, const uint8_t *commitments,
                                  const uint8_t *label, size_t label_len, const uint8_t *rng64,
                                  uint8_t *verdict, uint8_t *msm_out);
int bpgpu_rangeproof_verify_batch_dev(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch,
                                      const void *d_proofs, size_t proof_len, const void *d_commitments,
                                      const uint8_t *label, size_t label_len, const void *d_rng64,
                                      void *d_verdict, void *d_msm_out, void *stream);

/* Asynchronous form of bpgpu_rangeproof_verify_batch for a host thread that keeps several contexts busy: the inputs are
 * staged (the caller may reuse its input buffers at once), the work is enqueued, the call returns.  `verdict` / `msm_out`
 * are filled by bpgpu_ctx_collect(ctx) -- or implicitly by the next call made on this context -- and must stay valid
 * until then.  One submitted call per context at a time.  A single thread cycling over ~32 contexts reaches the
 * throughput of one thread per context (tools/archive/host_api_rate.py --pipelined). */
int bpgpu_rangeproof_verify_batch_submit(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch,
                                         const uint8_t *proofs, size_t proof_len, const uint8_t *commitments,
                                         const uint8_t *label, size_t label_len, const uint8_t *rng64,
                                         uint8_t *verdict, uint8_t *msm_out);
int bpgpu_ctx_collect(bpgpu_ctx *ctx);

/* The same verification on caller-supplied transcripts (the full `&mut Transcript` semantics of mod.rs:345-353):
 *   transcripts       : transcript_stride == 0: ONE state (208 bytes) every proof of the batch starts from;
 *                       transcript_stride == BPGPU_TRANSCRIPT_BYTES: nbatch states, one per proof
 *   transcripts_out   : optional nbatch x 208 bytes: each proof's transcript as verify_multiple_with_rng leaves it
 *                       (after the last inner-product challenge).  A proof rejected by from_bytes or by the parameter
 *                       checks (FormatError, InvalidBitsize, InvalidGeneratorsLength) gets its input state back; a proof
 *                       with an identity A / S / T_1 / T_2 / L_i / R_i gets the state as of that message (nothing of it
 *                       absorbed: validate_and_append_point, transcript.rs:75-87); n m != 2^k leaves the state as of the
 *                       `w` challenge (verification_scalars, ipp.rs:203-211) -- on every path the reference's own state.
 * `_dev`: `shared_transcript` is a HOST pointer to one state (or NULL), `d_transcripts` a device pointer to nbatch
 * states (or NULL); exactly one of the two must be given. */
int bpgpu_rangeproof_verify_batch_ts(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch,
                                     const uint8_t *proofs, size_t proof_len, const uint8_t *commitments,
                                     const uint8_t *transcripts, size_t transcript_stride, const uint8_t *rng64,
                                     uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out);
int bpgpu_rangeproof_verify_batch_ts_dev(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch,
                                         const void *d_proofs, size_t proof_len, const void *d_commitments,
                                         const uint8_t *shared_transcript, const void *d_transcripts, const void *d_rng64,
                                         void *d_verdict, void *d_msm_out, void *d_transcripts_out, void *stream);

/* ---- batch-combined verification (ADDITIONAL entry point; not a call of the reference) ---------------
 * The reference verifies one proof per MSM (verify_multiple checks ONE aggregated proof: mod.rs:345-452).
 * For a batch of independent proofs the standard next step is a random linear combination:
 *     R = sum_i rho_i * MegaCheck_i ,  MegaCheck_i = the multiscalar multiplication of mod.rs:421-443 for proof i,
 * with one weight rho_i = Scalar::from_bytes_mod_order_wide(weights64[i]) per proof.  The 2nm+2 generator
 * coefficients of all proofs add up in the scalar field, so the table walk runs once per batch.  R is the
 * identity when every combined proof verifies; if one does not, R != identity except with probability ~2^-252
 * over the weights, which must be unpredictable to the provers (NULL = drawn by the library as for rng64: uniform 512-bit strings
 * expanded on the device from a per-chain key).  Weights a caller passes are valid at any width; SHORT ones (e.g. 128 bits,
 * zero-extended) give proof i's A term the bare weight as its coefficient, and those equal-length scalars crowd single buckets of
 * the combined MSM -- which the bucket stage handles (crowded buckets are summed 64 lanes at a time: +4 % per combination,
 * measured at 4096 proofs).
 *   verdict   : nbatch bytes.  Proofs rejected by the parser / point decoder get their BPGPU_VERDICT_* code and
 *               are left out of the combination.  The others get 0 when R is the identity.  Otherwise:
 *               - bpgpu_rangeproof_verify_rlc re-verifies the batch proof by proof (same rng64) and returns
 *                 exactly the verdicts of bpgpu_rangeproof_verify_batch;
 *               - the asynchronous _dev variant marks them BPGPU_VERDICT_UNDECIDED and leaves that to the caller.
 *   batch_out : optional 33 bytes: [0] = 0 if R is the identity else 1; [1..33) = compress(R) (parity tests) */
#define BPGPU_VERDICT_UNDECIDED 5
int bpgpu_rangeproof_verify_rlc(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch,
                                const uint8_t *proofs, size_t proof_len, const uint8_t *commitments,
                                const uint8_t *label, size_t label_len, const uint8_t *rng64,
                                const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out);
int bpgpu_rangeproof_verify_rlc_dev(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch,
                                    const void *d_proofs, size_t proof_len, const void *d_commitments,
                                    const uint8_t *label, size_t label_len, const void *d_rng64,
                                    const void *d_weights64, void *d_verdict, void *d_batch_out, void *stream);

/* The same combination over proofs of MIXED shapes in ONE check (ADDITIONAL entry point; not a call of the reference): a block of
 * aggregated proofs with m = 1, 2, 4, 8, 16 outputs and more than one bit size, group after group.  BulletproofGens::new(N, M)
 * serves every n <= N, m <= M from the same points (generators.rs:157-259), so the generator coefficients of all groups add up on the
 * rows of the call's (N, M) = (max n, max m) and the table walk runs once per call; the 4 + 2k + m proof-specific terms of every
 * proof form one list for one MSM.
 *   n, m, nbatch, proof_len : ngroups values each; nbatch[g] == 0 and ngroups == 0 are valid
 *   proofs      : group after group, nbatch[g] x proof_len[g] bytes
 *   commitments : group after group, nbatch[g] x m[g] x 32 bytes
 *   labels, label_lens : one Merlin label per group (Transcript::new(label), as bpgpu_rangeproof_verify_batch)
 *   rng64, weights64 : total x 64 bytes each, in call order (total = sum nbatch[g]); rho_i = from_bytes_mod_order_wide(weights64[i])
 *                 with i the proof's index within the CALL.  NULL = drawn by the library, expanded on the device from a per-call key,
 *                 block = the index within the call: no two proofs of a call share a weight, whichever groups they are in
 *   verdict     : total bytes, call order; every proof's verdict is the one bpgpu_rangeproof_verify_batch gives it in a call of its
 *                 own shape with the same rng64 bytes.  Proofs rejected by the parser / point decoder keep their BPGPU_VERDICT_* code
 *                 and are left out of R.  A group the per-shape call rejects as a whole (malformed proof_len, n not 8 / 16 / 32 / 64,
 *                 n > gens_capacity or m > party_capacity, n m != 2^k) gets that call's codes, contributes nothing and does not disturb
 *                 the others.  When R is not the identity (or does not decode) the call re-verifies group by group on the per-proof
 *                 path with the same rng64 and returns exactly its verdicts.
 *   batch_out   : optional 33 bytes, as bpgpu_rangeproof_verify_rlc: compress(R) as computed before any fallback
 * One call takes at most 2^24 proofs and 2^24 proof-specific terms. */
int bpgpu_rangeproof_verify_rlc_mixed(bpgpu_ctx *ctx, size_t ngroups, const size_t *n, const size_t *m, const size_t *nbatch,
                                      const size_t *proof_len, const uint8_t *proofs, const uint8_t *commitments,
                                      const uint8_t *const *labels, const size_t *label_lens, const uint8_t *rng64,
                                      const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out);

/* Both combined checks on the CALLERS' OWN transcripts (the full `&mut Transcript` of mod.rs:345-353, as bpgpu_rangeproof_verify_batch_ts;
 * ADDITIONAL entry points): every proof starts from a Merlin state the application has already bound to its transaction or session.
 *   transcripts, transcript_stride : as bpgpu_rangeproof_verify_batch_ts -- stride 0: ONE 208-byte state for the batch; stride
 *                 BPGPU_TRANSCRIPT_BYTES: nbatch states, which may sit at differing STROBE positions.  rangeproof_domain_sep(n, m) is
 *                 applied on the device to the caller's state.  A malformed state is BPGPU_ERR_INVALID_ARG before anything runs.
 *   transcripts_out : optional nbatch x 208 bytes, byte for byte what bpgpu_rangeproof_verify_batch_ts returns per proof (mod.rs:345-353:
 *                 the end state; the input state back for FormatError and the parameter rejections; the state at the stopping message for
 *                 an identity A / S / T_1 / T_2 / L_i / R_i; the state at `w` when n m != 2^k) -- whether R was the identity or the call
 *                 fell back to the per-proof path
 *   rng64, weights64, verdict, batch_out : as bpgpu_rangeproof_verify_rlc; the fallback re-verifies through the per-proof path with the
 *                 same transcripts and rng bytes, so the verdicts are exactly those of bpgpu_rangeproof_verify_batch_ts
 * With the states in host memory the call sees whether all of them sit at one (pos, pos_begin, cur_flags): then the per-shape script
 * (compiled for that position, with the domain separator) replays them and only the 50 sponge words differ per lane; else the byte-wise
 * replay does.  A single state equal to bpgpu_transcript_new(label) gives the R of the label entry point for the same rng64 / weights64.
 * `_dev`: `shared_transcript` is a HOST pointer to one state (or NULL), `d_transcripts` a device pointer to nbatch states (or NULL, byte-wise
 * replay); exactly one of the two, as bpgpu_rangeproof_verify_batch_ts_dev; undecided verdicts are BPGPU_VERDICT_UNDECIDED, as
 * bpgpu_rangeproof_verify_rlc_dev. */
int bpgpu_rangeproof_verify_rlc_ts(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch,
                                   const uint8_t *proofs, size_t proof_len, const uint8_t *commitments,
                                   const uint8_t *transcripts, size_t transcript_stride, const uint8_t *rng64,
                                   const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out);
int bpgpu_rangeproof_verify_rlc_ts_dev(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch,
                                       const void *d_proofs, size_t proof_len, const void *d_commitments,
                                       const uint8_t *shared_transcript, const void *d_transcripts, const void *d_rng64,
                                       const void *d_weights64, void *d_verdict, void *d_batch_out, void *d_transcripts_out,
                                       void *stream);
/* bpgpu_rangeproof_verify_rlc_mixed on the callers' own transcripts (mod.rs:345-353), group by group:
 *   transcript_stride : ngroups values: 0 = one state for group g, BPGPU_TRANSCRIPT_BYTES = nbatch[g] states
 *   transcripts     : group after group: 208 bytes where transcript_stride[g] == 0, else nbatch[g] x 208 (a group with nbatch[g] == 0
 *                     still has its one state, or none, in the buffer)
 *   transcripts_out : optional total x 208 bytes in call order, per proof what bpgpu_rangeproof_verify_batch_ts returns (above)
 *   rng64, weights64 : rows indexed by the proof's position in the CALL, NULL = drawn by the library, exactly as the label form
 *   verdict, batch_out : as the label form; the fallback, and the per-shape call of a group rejected as a whole, get the group's
 *                     transcripts: every verdict is the one bpgpu_rangeproof_verify_batch_ts gives, group by group, with the same rng64
 * The front end decides per group: one state, or states at one position -> the script for that position; positions that differ within
 * the group -> the byte-wise replay.  A group whose single state equals bpgpu_transcript_new(label) contributes to R exactly what it
 * does through bpgpu_rangeproof_verify_rlc_mixed.
 * Rate (profiles/rlc_ts_rate.json: tools/rlc_mixed_rate.py --transcripts per-proof, one MI355X, the three forms interleaved, medians of
 * 50 calls, two runs within 1.2 % on the block and 3.5 % on one shape): a block of 1 024 proofs at n = 64, m = 1 .. 16 -- the label form
 * 3.54 ms (0.29 M/s), this call with one state per proof at differing positions 8.9 ms (0.115 M/s), bpgpu_rangeproof_verify_batch_ts group
 * by group 9.6 ms (0.107 M/s); 4 096 proofs of (64, 1) -- 1.70 / 2.22 / 2.03 ms (2.41 / 1.84 / 2.02 M/s).  The byte-wise replay is what it
 * costs over the label form (2.5x, 1.3x); with one state per group there is none and the call costs what the label form costs.  Against
 * the per-proof path this call is 7 - 9 % ahead on the mixed block and 9 % behind on the one wide shape (6 % and 10 % behind with one
 * state per group): at these two sizes there is no block size from which it is ahead throughout, and what it saves is the table walk per
 * shape, not the transcript. */
int bpgpu_rangeproof_verify_rlc_mixed_ts(bpgpu_ctx *ctx, size_t ngroups, const size_t *n, const size_t *m, const size_t *nbatch,
                                         const size_t *proof_len, const uint8_t *proofs, const uint8_t *commitments,
                                         const uint8_t *transcripts, const size_t *transcript_stride, const uint8_t *rng64,
                                         const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out);

/* ---- stand-alone inner-product proofs -------------------------------------------
 * nbatch independent calls of
 *   InnerProductProof::from_bytes(proof)?.verify(n, &mut Transcript::new(label), G_factors, H_factors, &P, &Q, &G, &H)
 * (src/inner_product_proof.rs:260-326, 373-407), all of one size n.
 *   proofs     : nbatch x proof_len bytes, proof_len = 32*(2*lg(n) + 2) for valid input
 *   G_factors, H_factors : nbatch x n x 32 bytes (the iterators of verify())
 *   P, Q       : nbatch x 32 bytes; G, H : nbatch x n x 32 bytes (compressed points)
 *   verdict    : nbatch bytes, BPGPU_VERDICT_* (an undecodable point counts as VerificationError)
 *   msm_out    : optional nbatch x 32 bytes, compress(expect_P - P) for parity tests */
int bpgpu_ipp_verify_batch(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                           const uint8_t *label, size_t label_len, const uint8_t *G_factors, const uint8_t *H_factors,
                           const uint8_t *P, const uint8_t *Q, const uint8_t *G, const uint8_t *H,
                           uint8_t *verdict, uint8_t *msm_out);

/* Device-pointer variant.  bases_shared != 0: every proof of the batch uses the SAME generator vectors, as the
 * reference's callers do (G = bp_gens.G(n, m), H = bp_gens.H(n, m)): d_G and d_H then hold n x 32 bytes instead of
 * nbatch x n x 32.  transcript: shared_transcript (host, 208 bytes, may hold earlier messages) if not NULL, else
 * Transcript::new(label). */
int bpgpu_ipp_verify_batch_dev(bpgpu_ctx *ctx, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                               const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                               const void *d_G_factors, const void *d_H_factors, const void *d_P, const void *d_Q,
                               const void *d_G, const void *d_H, int bases_shared,
                               void *d_verdict, void *d_msm_out, void *stream);
/* Batch-combined InnerProductProof verification (ADDITIONAL entry point, as bpgpu_rangeproof_verify_rlc, bpgpu_r1cs_verify_rlc and
 * bpgpu_linear_verify_rlc; the reference's InnerProductProof has only create / verify).  proofs, G_factors, H_factors, P, Q and the
 * transcript are those of bpgpu_ipp_verify_batch_dev; G, H hold n x 32 bytes, shared by the batch (the bases_shared != 0 form, the only
 * one this call takes); msm_out is replaced by weights64 and batch_out; one n per call.
 *     R = sum_p rho_p * Check_p ,  rho_p = Scalar::from_bytes_mod_order_wide(weights64[p]),
 * over the proofs that reach the final check, Check_p being the multiscalar multiplication of bpgpu_ipp_verify_batch for proof p.
 * G and H are shared, so their 2n coefficients add up in the scalar field and only the 2 lg(n) + 2 points Q, L_j, R_j, P of every
 * proof cost point arithmetic: ONE multiscalar multiplication per call -- one walk of the window tables plus nbatch (2 lg(n) + 2) points
 * in generator-table mode, 2n + nbatch (2 lg(n) + 2) points with the caller's bases -- and no buffer of the call grows with nbatch x n
 * (the per-proof call stages nbatch (2n + 2 lg(n) + 2) terms and decodes G, H once per proof).  R is the identity when every combined
 * proof verifies; if one does not, R != identity except with probability ~2^-252 over the weights, which must be unpredictable to the
 * provers (NULL = drawn by the library: uniform 512-bit strings expanded on the device from a per-call key).  A zero weight leaves its
 * proof unchecked.
 *   G, H      : n x 32 bytes each.  G = H = NULL: generator-table mode -- the bases are the context's bp_gens.G(n / gens_m, gens_m) and
 *               bp_gens.H(n / gens_m, gens_m), chained in party order (range_proof/mod.rs:439-442), and their coefficients go through
 *               the fixed-base window tables instead of per-call point tables.  Exactly one of them NULL: BPGPU_ERR_INVALID_ARG
 *   gens_m    : generator-table mode only (ignored with explicit bases): >= 1 and a divisor of n, else BPGPU_ERR_INVALID_ARG;
 *               BPGPU_ERR_NO_GENS when no generators are loaded, n / gens_m > gens_capacity or gens_m > party_capacity
 *   weights64 : nbatch x 64 bytes, or NULL
 *   verdict   : ALWAYS what bpgpu_ipp_verify_batch_dev(..., bases_shared = 1, ...) returns for the same inputs and points.  A proof that
 *               stops in the front end (FormatError: non-canonical a / b; VerificationError: n != 2^lg_n, an identity L_j / R_j) gets
 *               that code and is left out of R; the others get 0 when R is the identity and every point decoded.  Otherwise the host
 *               entry point re-verifies the batch through the per-proof path (in generator-table mode on the generators' encodings)
 *               and returns those verdicts; the asynchronous _dev variant marks them BPGPU_VERDICT_UNDECIDED and leaves that to the
 *               caller.
 *   batch_out : optional 33 bytes: [0] = 0 when R is the identity and every point decoded, else 1; [1..33) = compress(R) as computed
 *               before any fallback, or zeros when a point (a shared G_i / H_i included) did not decode
 * A proof_len that is no InnerProductProof length gives FormatError for every proof (and batch_out = zeros); nbatch = 0 is BPGPU_OK.
 * One call takes at most 2^24 proofs and 2^24 proof-specific points (nbatch (2 lg(n) + 2)); larger calls return
 * BPGPU_ERR_INVALID_ARG.  This call has no per-proof transcripts and no transcripts_out (the per-proof call that defines its verdicts
 * has neither): bpgpu_ipp_verify_rlc_ts below has both.
 * The transcript replay stays per proof (k_ipp_vs_front: one lane per proof, serial over lg(n) rounds and one inversion) and sets the
 * floor of the call, 0.19 ... 0.31 ms; what the combination saves is the per-proof staging, the decodes of G, H per proof and the
 * per-proof multiscalar multiplications.  Measured on one MI355X (profiles/ipp_rlc_rate.json, n = 64 ... 1 024 against
 * bpgpu_ipp_verify_batch_dev with bases_shared = 1): faster at every shape measured -- 1.2x ... 1.4x at 64 proofs of n = 64, 1.6x ... 1.7x
 * at 1 024 and 3.0x ... 3.1x at 4 096; 2.8x ... 8.8x at n = 256; 6.3x ... 16.1x at n = 1 024 -- the caller's bases and the generator tables
 * within 1 ... 4 % of each other from 1 024 proofs on (11 % at 256 x 4 096) and the tables 11 ... 44 % slower at 64 proofs (the table
 * walk is a fixed cost).
 * The call never takes less than 0.74 ms (the one combined MSM alone is 0.5 ... 1.5 ms of kernels).  A failing batch costs this call
 * plus the per-proof one: 1.06x ... 1.82x the per-proof call alone. */
int bpgpu_ipp_verify_rlc(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                         const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                         const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *P, const uint8_t *Q,
                         const uint8_t *G, const uint8_t *H, size_t gens_m, const uint8_t *weights64,
                         uint8_t *verdict, uint8_t *batch_out);
int bpgpu_ipp_verify_rlc_dev(bpgpu_ctx *ctx, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                             const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                             const void *d_G_factors, const void *d_H_factors, const void *d_P, const void *d_Q,
                             const void *d_G, const void *d_H, size_t gens_m, const void *d_weights64,
                             void *d_verdict, void *d_batch_out, void *stream);

/* ---- linear proofs (LinearProof, `pub use` src/lib.rs:36) --------------------------------
 * nbatch independent calls of
 *   LinearProof::from_bytes(proof)?.verify(&mut transcript, &C, &G, &F, &B, b_vec)
 * (src/linear_proof.rs:175-236, 240-312, 350-394), all of one size n = G.len() = b_vec.len(): the proof that
 * <a, b> = c for a committed secret a and the public b.  The three multiscalar multiplications and the comparison of
 * verify() (:207-236) run as ONE multiscalar multiplication of n + 2 lg(n) + 4 terms per proof whose result must be
 * the identity; transcript replay, the fold of b and the subset products run on the device (csrc/linear.h).
 *   proofs  : nbatch x proof_len bytes, proof_len = 32*(2*lg(n) + 3) for valid input (L_j, R_j pairs, S, a, r)
 *   transcript : shared_transcript (host, 208 bytes, may hold earlier messages) if not NULL, else Transcript::new(label);
 *             every proof starts from it
 *   transcripts_out : optional nbatch x 208 bytes: each proof's transcript as verify() leaves it (after the x_star
 *             challenge, :208) when the proof reaches the final check; for proofs rejected earlier the state right after
 *             innerproduct_domain_sep(n) (:196)
 *   C       : nbatch x 32 bytes (compressed commitments)
 *   G       : n x 32 bytes, F, B : 32 bytes each -- compressed points shared by the batch (the reference's callers pass
 *             bp_gens.share(0).G(n), pedersen B and B_blinding: linear_proof.rs:405-411); the encodings given here are
 *             what the transcript absorbs (G_i.compress(), :201-205), so they must be canonical
 *             G = F = B = NULL: the bases are the context's generators -- G = bp_gens.share(0).G(n), F = pc_gens.B,
 *             B = pc_gens.B_blinding -- and their n + 2 coefficients go through the fixed-base window tables instead of
 *             per-call point tables (the fast path; needs bpgpu_gens_create / _load with gens_capacity >= n)
 *   b       : nbatch x n x 32 bytes canonical scalars, or n x 32 when b_shared != 0
 *   verdict : nbatch bytes, BPGPU_VERDICT_* (FormatError: proof length, non-canonical a, r or b_i; VerificationError:
 *             n != 2^lg_n, an identity L_j / R_j, an undecodable point, or expect_S != S)
 *   msm_out : optional nbatch x 32 bytes, compress(expect_S - S) for parity tests */
int bpgpu_linear_verify_batch(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                              const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                              const uint8_t *C, const uint8_t *G, const uint8_t *F, const uint8_t *B,
                              const uint8_t *b, int b_shared, uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out);
int bpgpu_linear_verify_batch_dev(bpgpu_ctx *ctx, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                                  const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                                  const void *d_C, const void *d_G, const void *d_F, const void *d_B,
                                  const void *d_b, int b_shared, void *d_verdict, void *d_msm_out, void *d_transcripts_out,
                                  void *stream);
/* Batch-combined LinearProof verification (ADDITIONAL entry point, as bpgpu_rangeproof_verify_rlc and bpgpu_r1cs_verify_rlc; the
 * reference's LinearProof has only create / verify).  Arguments are those of bpgpu_linear_verify_batch, with msm_out replaced by
 * weights64 and batch_out; one n per call.
 *     R = sum_p rho_p * Check_p ,  rho_p = Scalar::from_bytes_mod_order_wide(weights64[p]),
 * over the proofs that reach the final check, Check_p being the multiscalar multiplication of bpgpu_linear_verify_batch for proof p.
 * G, F, B are shared by the batch (the caller's points or, with G = F = B = NULL, the context's generators), so their n + 2
 * coefficients add up in the scalar field and only the 2 lg(n) + 2 points C, L_j, R_j, S of every proof cost point arithmetic: ONE
 * multiscalar multiplication per call -- one walk of the window tables plus nbatch (2 lg(n) + 2) points in generator-table mode,
 * (n + 2) + nbatch (2 lg(n) + 2) points with the caller's bases.  R is the identity when every combined proof verifies; if one does
 * not, R != identity except with probability ~2^-252 over the weights, which must be unpredictable to the provers (NULL = drawn by
 * the library: uniform 512-bit strings expanded on the device from a per-call key).  A zero weight leaves its proof unchecked.
 *   weights64       : nbatch x 64 bytes, or NULL
 *   verdict         : ALWAYS what bpgpu_linear_verify_batch returns for the same inputs.  A proof that stops in the front end
 *                     (FormatError; an identity L_j / R_j; n != 2^lg_n) gets that code and is left out of R; the others get 0 when R is
 *                     the identity and every point decoded.  Otherwise the host entry point re-verifies the batch through the per-proof
 *                     path and returns those verdicts; the asynchronous _dev variant marks them BPGPU_VERDICT_UNDECIDED and leaves
 *                     that to the caller.
 *   batch_out       : optional 33 bytes: [0] = 0 when R is the identity and every point decoded, else 1; [1..33) = compress(R) as
 *                     computed before any fallback, or zeros when a point did not decode
 *   transcripts_out : optional, as bpgpu_linear_verify_batch leaves them
 * Errors and shortcuts are those of bpgpu_linear_verify_batch: a proof_len that is no LinearProof length gives FormatError for every
 * proof (and batch_out = zeros), generators missing or smaller than n an error code, nbatch = 0 BPGPU_OK.  One call takes at most 2^24
 * proofs and 2^24 proof-specific points (nbatch (2 lg(n) + 2)); larger calls return BPGPU_ERR_INVALID_ARG.
 * The transcript replay stays per proof (C is absorbed first and is the proof's own), so the front end costs what it costs in the
 * per-proof call; what the combination saves is the multiscalar multiplication.  Measured on one MI355X (DESIGN 3.4,
 * profiles/linear_rlc_rate.json): faster than bpgpu_linear_verify_batch with the caller's bases from about 1 000 proofs on (1.5x ... 2.2x
 * at 4 096 proofs, n = 64 ... 1 024) and with the generator tables at 4 096 proofs and n >= 256 (1.2x); NOT faster (0.82x ... 1.03x) at 64
 * proofs and with the generator tables up to 1 024 proofs: the front end (k_lin_prepare) dominates both calls there and the one combined
 * MSM has a floor of 0.5 ... 1.5 ms.  A failing batch costs this call plus the per-proof one. */
int bpgpu_linear_verify_rlc(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                            const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                            const uint8_t *C, const uint8_t *G, const uint8_t *F, const uint8_t *B,
                            const uint8_t *b, int b_shared, const uint8_t *weights64,
                            uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out);
int bpgpu_linear_verify_rlc_dev(bpgpu_ctx *ctx, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                                const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                                const void *d_C, const void *d_G, const void *d_F, const void *d_B,
                                const void *d_b, int b_shared, const void *d_weights64,
                                void *d_verdict, void *d_batch_out, void *d_transcripts_out, void *stream);

/* ---- inner-product and linear proofs on the callers' OWN transcripts ---------------------------------------------------------
 * InnerProductProof and LinearProof are sub-protocols: a protocol that embeds one has bound its own Merlin transcript (label, session
 * id, earlier messages) before it calls create / verify, and that transcript differs from proof to proof.  The _ts entry points are
 * the calls above with `label, label_len, shared_transcript` replaced by the convention of bpgpu_rangeproof_verify_batch_ts /
 * bpgpu_rangeproof_prove_batch_ts; every other argument, error and shortcut is the sibling's.
 *   transcripts       : REQUIRED.  transcript_stride = 0: ONE 208-byte state, every proof starts from it;
 *                       transcript_stride = BPGPU_TRANSCRIPT_BYTES: nbatch states, one per proof.  The states are the callers' states
 *                       BEFORE innerproduct_domain_sep(n) (transcript.rs:50-53), at any STROBE position: the separator is applied per
 *                       proof on the device, byte by byte, also where it crosses the 166-byte rate boundary in its middle.
 *                       transcripts == NULL, any other stride or a malformed state (position bytes out of range) return
 *                       BPGPU_ERR_INVALID_ARG before anything is staged, the outputs untouched.  nbatch = 0 is BPGPU_OK.
 *   transcripts_out   : optional nbatch x 208 bytes.
 *       linear        : as bpgpu_linear_verify_batch documents them for shared_transcript = the proof's own state.
 *       inner product : what verification_scalars leaves in the caller's `&mut Transcript` (ipp.rs:203-222, transcript.rs:75-87): the
 *                       INPUT state for a proof that from_bytes or n != 2^lg_n rejects (the reference returns before the separator);
 *                       for an identity L_j / R_j the state as of that message -- separator and earlier rounds absorbed, nothing of
 *                       the identity point; the state after the last u challenge otherwise.
 *   _dev forms        : as bpgpu_rangeproof_verify_batch_ts_dev -- exactly one of shared_transcript (host, one state) and
 *                       d_transcripts (device, nbatch states, 4-byte aligned) is given; work is enqueued on `stream` (NULL: the
 *                       context's own).  Device states cannot be checked by the host: one whose position bytes are out of range is
 *                       started at position 0.  The _dev combined checks mark undecided verdicts BPGPU_VERDICT_UNDECIDED.
 * Contracts (tests/test_gpu_ipp_linear_ts.py):
 *   per proof     : every output of row p -- verdict / status, msm_out, proof bytes, transcripts_out -- equals the sibling called with
 *                   nbatch = 1 and shared_transcript = transcripts[p];
 *   shared state  : with transcript_stride = 0 the outputs equal the sibling's on the whole batch with that shared_transcript, byte
 *                   for byte (batch_out of the combined checks included, for equal weights64);
 *   combined      : verdict and transcripts_out of an _rlc_ts call ALWAYS equal those of the _verify_batch_ts call on the same inputs,
 *                   also with a failing proof in the batch and for proofs stopped in the front end.  The host forms' per-proof
 *                   fallback starts again from the callers' input states.
 * bpgpu_ipp_verify_batch_ts takes bases_shared like the _dev form (bpgpu_ipp_verify_batch does not): != 0, G and H hold n x 32 bytes.
 * The front ends do the work of their siblings plus one 208-byte load and the separator (at most two permutations) per proof.  Measured on
 * one MI355X (profiles/ipp_linear_ts_rate.json; 4 096 proofs, generator tables, blocking calls alternating, median): one state
 * per proof against one shared state 2.23 / 2.15 ms (n = 64) and 17.88 / 17.45 ms (n = 1 024) for bpgpu_linear_verify_batch_ts, 2.52 / 2.46
 * and 17.35 / 17.47 ms for bpgpu_ipp_verify_rlc_ts; the _dev forms 2.03 / 1.98, 17.51 / 17.12, 1.68 / 1.68 and 2.68 / 2.64 ms -- ratios of
 * 0.99 ... 1.04, each form's calls within 0.5 ... 4.3 % of its median (the host inner-product call at n = 1 024, which stages 268 MB: 9 ... 34 %). */
int bpgpu_ipp_verify_batch_ts(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                              const uint8_t *transcripts, size_t transcript_stride,
                              const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *P, const uint8_t *Q,
                              const uint8_t *G, const uint8_t *H, int bases_shared,
                              uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out);
int bpgpu_ipp_verify_batch_ts_dev(bpgpu_ctx *ctx, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                                  const uint8_t *shared_transcript, const void *d_transcripts,
                                  const void *d_G_factors, const void *d_H_factors, const void *d_P, const void *d_Q,
                                  const void *d_G, const void *d_H, int bases_shared,
                                  void *d_verdict, void *d_msm_out, void *d_transcripts_out, void *stream);
int bpgpu_ipp_verify_rlc_ts(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                            const uint8_t *transcripts, size_t transcript_stride,
                            const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *P, const uint8_t *Q,
                            const uint8_t *G, const uint8_t *H, size_t gens_m, const uint8_t *weights64,
                            uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out);
int bpgpu_ipp_verify_rlc_ts_dev(bpgpu_ctx *ctx, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                                const uint8_t *shared_transcript, const void *d_transcripts,
                                const void *d_G_factors, const void *d_H_factors, const void *d_P, const void *d_Q,
                                const void *d_G, const void *d_H, size_t gens_m, const void *d_weights64,
                                void *d_verdict, void *d_batch_out, void *d_transcripts_out, void *stream);
int bpgpu_linear_verify_batch_ts(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                 const uint8_t *transcripts, size_t transcript_stride,
                                 const uint8_t *C, const uint8_t *G, const uint8_t *F, const uint8_t *B,
                                 const uint8_t *b, int b_shared, uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out);
int bpgpu_linear_verify_batch_ts_dev(bpgpu_ctx *ctx, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                                     const uint8_t *shared_transcript, const void *d_transcripts,
                                     const void *d_C, const void *d_G, const void *d_F, const void *d_B,
                                     const void *d_b, int b_shared, void *d_verdict, void *d_msm_out, void *d_transcripts_out,
                                     void *stream);
int bpgpu_linear_verify_rlc_ts(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                               const uint8_t *transcripts, size_t transcript_stride,
                               const uint8_t *C, const uint8_t *G, const uint8_t *F, const uint8_t *B,
                               const uint8_t *b, int b_shared, const uint8_t *weights64,
                               uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out);
int bpgpu_linear_verify_rlc_ts_dev(bpgpu_ctx *ctx, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                                   const uint8_t *shared_transcript, const void *d_transcripts,
                                   const void *d_C, const void *d_G, const void *d_F, const void *d_B,
                                   const void *d_b, int b_shared, const void *d_weights64,
                                   void *d_verdict, void *d_batch_out, void *d_transcripts_out, void *stream);

/* ---- R1CS constraint-system proofs (r1cs::Verifier::verify, src/r1cs/verifier.rs:329-500) ----------------------------
 * The reference's verifier re-runs a gadget (closures) against its constraint system.  On the verifier side only
 * commit (verifier.rs:235-243) and challenge_scalar inside randomized callbacks (:177) touch the transcript; multiply,
 * allocate, allocate_multiplier and constrain only append constraints and count multipliers (:67-127).  So a gadget is
 * recorded ONCE as data -- a bpgpu_r1cs_circuit -- and verified on the device for any number of proofs.
 *   m          : committed variables (Verifier::commit calls)
 *   n1, n2     : multipliers before / after randomization (create_randomized_constraints, :300-321)
 *   two_phase  : 1 when a randomized callback was registered (r1cs-2phase, even with n2 = 0), else 0 (then n2 = 0, no challenges)
 *   labels     : the phase-2 challenge labels in draw order, concatenated; label_lens[j] bytes each
 *   constraints: CSR rows in the order the gadget added them: row_ptr[n_constraints + 1], and per term
 *                kind (BPGPU_R1CS_L/R/O: multiplier index < n1 + n2; _V: committed index < m; _ONE: index 0),
 *                challenge (BPGPU_R1CS_NO_CHALLENGE, or j < n_challenges), power (0 without a challenge, else 1..BPGPU_R1CS_MAX_POWER),
 *                coeff (32 bytes canonical): the term's coefficient is coeff * ch_j^power.  Terms are summed as
 *                flattened_constraints does (:260-298), with the reference's signs on V and ONE.
 * Host-only; every field is validated (BPGPU_ERR_INVALID_ARG otherwise).  The per-variable lists are uploaded to a device on
 * first use and cached there until destroy; a circuit may be used from several threads and contexts at once. */
typedef struct bpgpu_r1cs_circuit bpgpu_r1cs_circuit;
#define BPGPU_R1CS_L 0
#define BPGPU_R1CS_R 1
#define BPGPU_R1CS_O 2
#define BPGPU_R1CS_V 3
#define BPGPU_R1CS_ONE 4
#define BPGPU_R1CS_NO_CHALLENGE 0xffffffffu
#define BPGPU_R1CS_MAX_VARS 65536            /* m, n1 + n2 (padded_n <= 2^16) */
#define BPGPU_R1CS_MAX_CONSTRAINTS (1u << 22)
#define BPGPU_R1CS_MAX_TERMS (1u << 24)
#define BPGPU_R1CS_MAX_CHALLENGES 256
#define BPGPU_R1CS_MAX_LABEL 1024
#define BPGPU_R1CS_MAX_POWER 255
int bpgpu_r1cs_circuit_create(size_t m, size_t n1, size_t n2, int two_phase, size_t n_challenges, const uint8_t *labels,
                              const uint32_t *label_lens, size_t n_constraints, const uint32_t *row_ptr, size_t n_terms,
                              const uint8_t *term_kind, const uint32_t *term_index, const uint32_t *term_challenge,
                              const uint32_t *term_power, const uint8_t *term_coeff, bpgpu_r1cs_circuit **out);
void bpgpu_r1cs_circuit_destroy(bpgpu_r1cs_circuit *circuit);
/* padded_n = (n1 + n2).next_power_of_two() (0 -> 1) and the per-proof point count 11 + m + 2 lg(padded_n) of the mega-check */
int bpgpu_r1cs_circuit_shape(const bpgpu_r1cs_circuit *circuit, size_t *padded_n, size_t *n_unique);
/* nbatch proofs against one circuit; each as R1CSProof::from_bytes (src/r1cs/proof.rs:129-204), Verifier::new(transcript),
 * commit(V_i) for its m commitments, the recorded gadget, and verify(proof, pc_gens, bp_gens) with the context's generators.
 *   proofs            : nbatch x proof_stride bytes; proof_lens[b] <= proof_stride bytes of each are the proof (either
 *                       serialization: version 0 with A_I2 = A_O2 = S2 = identity, or version 1)
 *   commitments       : nbatch x m x 32 bytes
 *   transcripts       : the caller's transcript(s) BEFORE Verifier::new: one 208-byte state (transcript_stride 0) or nbatch
 *                       (stride BPGPU_TRANSCRIPT_BYTES)
 *   rng32             : nbatch x 32 bytes -- what TranscriptRngBuilder::finalize takes from thread_rng() (verifier.rs:448) -- or
 *                       NULL: the library's generator (ChaCha20 keyed from the OS per call)
 *   verdict           : nbatch bytes, BPGPU_VERDICT_* (R1CSError, errors.rs:125-167: FormatError, VerificationError -- an identity
 *                       validated point, an IPP of the wrong length, an undecodable point, a mega-check that is not the
 *                       identity -- or InvalidGeneratorsLength when padded_n > gens_capacity)
 *   msm_out           : optional nbatch x 32 bytes, the mega-check's encoding where the verdict came from it
 *   transcripts_out   : optional nbatch x 208 bytes, each transcript as the reference leaves it: unchanged after a from_bytes
 *                       failure; as of the message for an identity validated point (A_I1, A_O1, S1, T_*, L_i, R_i); after the
 *                       phase-2 challenges for InvalidGeneratorsLength; as of `w` for an IPP whose length is not lg(padded_n);
 *                       else after the last IPP challenge.
 * `_dev`: device pointers (proof_lens: nbatch uint32), `shared_transcript` a HOST pointer to one state or `d_transcripts` nbatch
 * states on the device (exactly one of the two). */
int bpgpu_r1cs_verify_batch_ts(bpgpu_ctx *ctx, const bpgpu_r1cs_circuit *circuit, size_t nbatch, const uint8_t *proofs,
                               size_t proof_stride, const uint32_t *proof_lens, const uint8_t *commitments,
                               const uint8_t *transcripts, size_t transcript_stride, const uint8_t *rng32,
                               uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out);
int bpgpu_r1cs_verify_batch_ts_dev(bpgpu_ctx *ctx, const bpgpu_r1cs_circuit *circuit, size_t nbatch, const void *d_proofs,
                                   size_t proof_stride, const void *d_proof_lens, const void *d_commitments,
                                   const uint8_t *shared_transcript, const void *d_transcripts, const void *d_rng32,
                                   void *d_verdict, void *d_msm_out, void *d_transcripts_out, void *stream);
/* Batch-combined R1CS verification (ADDITIONAL entry point, as bpgpu_rangeproof_verify_rlc; the reference's r1cs::Verifier has only
 * new / commit / verify).  One call takes ngroups groups; group g is what one bpgpu_r1cs_verify_batch_ts call takes: circuits[g] (the
 * same circuit may appear in several groups), nbatch[g] proofs (proofs[g], proof_stride[g], proof_lens[g]), commitments[g] and
 * transcripts[g] with transcript_stride[g] (0: one shared state, BPGPU_TRANSCRIPT_BYTES: one per proof).  The per-proof arrays rng32
 * (32 bytes), weights64 (64), verdict (1) and transcripts_out (208) run over all proofs, the groups' in order (sum(nbatch) entries).
 *     R = sum_i rho_i * MegaCheck_i ,  rho_i = Scalar::from_bytes_mod_order_wide(weights64[i]),
 * over the proofs that reach the mega-check.  Their generator coefficients add up in the scalar field on the generator rows of the
 * largest padded_n, so the table walk runs once per call; their own points (11 + m + 2k per proof) form one Pippenger MSM.  R is the
 * identity when every combined proof verifies; if one does not, R != identity except with probability ~2^-252 over the weights, which
 * must be unpredictable to the provers (NULL = drawn by the library: uniform 512-bit strings expanded on the device from a per-call key).
 * A zero weight leaves its proof unchecked.
 *   rng32           : as bpgpu_r1cs_verify_batch_ts, or NULL: each proof's 32 bytes are drawn ONCE as that call's seeded mode draws them
 *                     (ChaCha20 keyed from the OS per call) and serve both the combination and any fallback
 *   verdict         : ALWAYS what bpgpu_r1cs_verify_batch_ts returns for the proof's group with the same rng32 bytes.  A proof that
 *                     stops before the mega-check (FormatError, an identity validated point, InvalidGeneratorsLength, an IPP of the wrong
 *                     length) gets that code and is left out of R.  When R is not the identity, or a point of the combined MSM does not
 *                     decode, the call re-verifies every group through the per-proof pipeline and returns those verdicts.
 *   batch_out       : optional 33 bytes: [0] = 0 when R is the identity and every point decoded, else 1; [1..33) = compress(R), or zeros
 *                     when a point did not decode
 *   transcripts_out : optional, as bpgpu_r1cs_verify_batch_ts leaves them
 * ngroups = 0 or a NULL group array is BPGPU_ERR_INVALID_ARG; groups with nbatch[g] = 0 are skipped.  Context option
 * "r1cs_rlc_max_terms" caps the proof-specific terms of one MSM (default 2^24): above it the call forms several combinations and adds
 * their points before the identity test.  Memory stays bounded: groups are processed in slices of at most 1024 proofs, in the
 * combination and in the per-proof fallback alike (the combined term list itself holds at most r1cs_rlc_max_terms terms). */
int bpgpu_r1cs_verify_rlc(bpgpu_ctx *ctx, size_t ngroups, const bpgpu_r1cs_circuit *const *circuits, const size_t *nbatch,
                          const uint8_t *const *proofs, const size_t *proof_stride, const uint32_t *const *proof_lens,
                          const uint8_t *const *commitments, const uint8_t *const *transcripts, const size_t *transcript_stride,
                          const uint8_t *rng32, const uint8_t *weights64,
                          uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out);

/* ---- R1CS proof creation (r1cs::Prover::prove, src/r1cs/prover.rs:380-655) ------------------------------------------------
 * The prover's gadget also computes the witness: a_L, a_R, a_O of every multiplier.  Phase-2 multipliers may take inputs from
 * linear combinations that hold the phase-2 challenges, which exist only partway through the proof, so HOW each multiplier
 * gets its inputs is recorded -- a bpgpu_r1cs_witness, beside the circuit -- and evaluated per proof on the device.
 *   n_free     : free inputs per proof (the scalars the gadget assigned: allocate, allocate_multiplier)
 *   src_left, src_right : n1 + n2 entries each, where a_L[i] / a_R[i] comes from: BPGPU_R1CS_SRC_FREE | j (free input j, each
 *                used exactly once), an LC row index, or BPGPU_R1CS_SRC_ZERO (an allocate() pair left open: a_R = 0, so
 *                a_O = 0, as prover.rs:121-140 leaves it).  a_O[i] = a_L[i] a_R[i].
 *   rows       : CSR LC rows with the circuit's term encoding, evaluated as Prover::eval (prover.rs:340-356): plain sums, no
 *                sign flip on V / ONE.  A row used by multiplier i may reference L / R / O of multipliers < i only, and no
 *                challenge when i < n1.
 * Host-only; validated like the circuit (BPGPU_ERR_INVALID_ARG). */
typedef struct bpgpu_r1cs_witness bpgpu_r1cs_witness;
#define BPGPU_R1CS_SRC_ZERO 0xffffffffu
#define BPGPU_R1CS_SRC_FREE 0x80000000u
int bpgpu_r1cs_witness_create(const bpgpu_r1cs_circuit *circuit, size_t n_free, const uint32_t *src_left, const uint32_t *src_right,
                              size_t n_rows, const uint32_t *row_ptr, size_t n_terms, const uint8_t *term_kind,
                              const uint32_t *term_index, const uint32_t *term_challenge, const uint32_t *term_power,
                              const uint8_t *term_coeff, bpgpu_r1cs_witness **out);
void bpgpu_r1cs_witness_destroy(bpgpu_r1cs_witness *witness);
/* nbatch independent proofs of one recorded gadget: Prover::new(transcript), commit(v_j, v_blinding_j) for j < m, the gadget
 * with the free inputs, prove(bp_gens) with the context's generators.
 *   v, v_blinding     : nbatch x m x 32 bytes; free_inputs: nbatch x n_free x 32 bytes (canonical scalars)
 *   transcripts       : the caller's transcript(s) BEFORE Prover::new: one 208-byte state (transcript_stride 0) or nbatch
 *                       (stride BPGPU_TRANSCRIPT_BYTES)
 *   rng32             : nbatch x 32 bytes -- what TranscriptRngBuilder::finalize takes from thread_rng() (prover.rs:411) --
 *                       or NULL: the OS generator.  The TranscriptRng is rekeyed with every v_blinding first (merlin 2:
 *                       meta_ad(b"v_blinding"), meta_ad(u32le(32), more), KEY(v_blinding)); the draws follow prover.rs's order.
 *   proofs_out        : nbatch x proof_stride bytes, R1CSProof::to_bytes (proof.rs:83-108; version 0 exactly when A_I2, A_O2,
 *                       S2 are all the identity); proof_lens_out[p] its length.  proof_stride >= 1 + 32 (14 + 2 lg(padded_n) + 2)
 *                       (11 instead of 14 when n2 = 0).
 *   commitments_out   : nbatch x m x 32 bytes, the V_j = v_j B + v_blinding_j B_blinding
 *   status_out        : nbatch bytes, BPGPU_MSM_BAD_SCALAR for a non-canonical input scalar (that proof is void), else 0
 *   transcripts_out   : optional nbatch x 208 bytes, each transcript as prove leaves it (after the last IPP challenge)
 * BPGPU_ERR_NO_GENS when padded_n > gens_capacity (InvalidGeneratorsLength).  A witness that does not satisfy the constraints
 * still yields a proof, as in the reference; the verifier rejects it.  With the option prover_constant_time the V_j, A_I, A_O,
 * S and T_i commitments take the constant-time walk (byte-identical proofs).  Secrets at rest: as the other provers. */
int bpgpu_r1cs_prove_batch(bpgpu_ctx *ctx, const bpgpu_r1cs_circuit *circuit, const bpgpu_r1cs_witness *witness, size_t nbatch,
                           const uint8_t *v, const uint8_t *v_blinding, const uint8_t *free_inputs, const uint8_t *transcripts,
                           size_t transcript_stride, const uint8_t *rng32, uint8_t *proofs_out, size_t proof_stride,
                           uint32_t *proof_lens_out, uint8_t *commitments_out, uint8_t *status_out, uint8_t *transcripts_out);

/* ---- R1CS witness check: which constraint does a witness leave unsatisfied? (bellman's is_satisfied / which_is_unsatisfied) ----
 * Constraint q of proof p holds iff Prover::eval(lc_q) == 0 (prover.rs:340-356): the sum over its terms of
 * coeff * challenge^power * value, mod l, over the witness the witness program computes.  ADDITIONAL entry points: no other call
 * changes.  BPGPU_R1CS_UNSATISFIED is the next status byte after the BPGPU_MSM_* ones the provers' status_out carries. */
#define BPGPU_R1CS_SATISFIED 0xffffffffu
#define BPGPU_R1CS_UNSATISFIED 3
/* The stand-alone check of nbatch witnesses of one recorded gadget.  No generators, no transcript, no blindings: it works on a
 * context that never loaded generators.
 *   v           : nbatch x m x 32 bytes; free_inputs: nbatch x n_free x 32 bytes (canonical scalars)
 *   challenges  : nbatch x n_challenges x 32 bytes, canonical scalars: proof p's phase-2 challenge values in draw order; NULL
 *                 when the circuit has no challenges (ignored then).  A witness that is right satisfies every constraint under
 *                 any challenges; one that is wrong fails under almost all of them.
 *   first_out   : nbatch words, the lowest unsatisfied constraint index (in the order the gadget added them), or
 *                 BPGPU_R1CS_SATISFIED
 *   count_out   : optional nbatch words, how many constraints failed
 *   map_out     : optional nbatch x map_stride bytes, map_stride >= ceil(Q / 8): bit q % 8 of byte q / 8 is set iff constraint q
 *                 failed; every other bit is zero
 *   status_out  : nbatch bytes, BPGPU_MSM_BAD_SCALAR for a non-canonical v, free input or challenge -- that proof is not
 *                 checked (first = BPGPU_R1CS_SATISFIED, count 0, map zero) -- else 0
 * nbatch = 0 is BPGPU_OK.  BPGPU_ERR_INVALID_ARG: a witness program of another circuit, challenges == NULL for a circuit that
 * has some, map_stride too small.  v and the free inputs are secrets: staging and working set are cleared on every exit, as the
 * provers clear theirs.  The circuit's row form is built and uploaded at the first check (here or in the checked prover) and
 * freed by bpgpu_r1cs_circuit_destroy. */
int bpgpu_r1cs_witness_check(bpgpu_ctx *ctx, const bpgpu_r1cs_circuit *circuit, const bpgpu_r1cs_witness *witness, size_t nbatch,
                             const uint8_t *v, const uint8_t *free_inputs, const uint8_t *challenges, uint32_t *first_out,
                             uint32_t *count_out, uint8_t *map_out, size_t map_stride, uint8_t *status_out);
/* bpgpu_r1cs_prove_batch with the check run on each proof's OWN phase-2 challenges, after the last witness launch and before
 * the polynomials (bpgpu_r1cs_prove_batch is this function with the check off).  A proof whose witness satisfies every
 * constraint: every output equals bpgpu_r1cs_prove_batch's on the same inputs byte for byte, unsat_first_out[p] =
 * BPGPU_R1CS_SATISFIED.  Otherwise proof p is void: status_out[p] = BPGPU_R1CS_UNSATISFIED, unsat_first_out[p] the first failing
 * constraint, its proof bytes zero, proof_lens_out[p] = 0, transcripts_out[p] the input state unchanged; commitments_out still
 * holds its V_j (valid commitments).  A non-canonical input keeps BPGPU_MSM_BAD_SCALAR (and BPGPU_R1CS_SATISFIED): it takes
 * precedence.  The chain runs at full width; void proofs are blanked at the end. */
int bpgpu_r1cs_prove_batch_checked(bpgpu_ctx *ctx, const bpgpu_r1cs_circuit *circuit, const bpgpu_r1cs_witness *witness, size_t nbatch,
                                   const uint8_t *v, const uint8_t *v_blinding, const uint8_t *free_inputs, const uint8_t *transcripts,
                                   size_t transcript_stride, const uint8_t *rng32, uint8_t *proofs_out, size_t proof_stride,
                                   uint32_t *proof_lens_out, uint8_t *commitments_out, uint8_t *status_out, uint8_t *transcripts_out,
                                   uint32_t *unsat_first_out);

/* nbatch independent calls of
 *   LinearProof::create(&mut transcript, &mut rng, &C, r, a_vec, b_vec, G_vec, &F, &B).to_bytes()
 * (src/linear_proof.rs:40-173), all of one size n (a power of two) over the same G, F, B.  Per round the reference forms
 * L_j, R_j with two (n'+2)-term multiscalar multiplications (:104-117) and folds the generators with n' two-term ones
 * (:140-144); here all proofs advance round by round together and every L_j / R_j / S is one multiscalar
 * multiplication over the ORIGINAL points (csrc/linear_prover.h): the same group elements, so the proofs are
 * byte-identical to the reference algorithm's given the same transcript, inputs and randomness.  Variable time, like
 * the reference's own create() (vartime_multiscalar_mul).
 *   rng     : nbatch x 64*(2 lg n + 2) bytes: what the rng would yield to Scalar::random, 64 bytes per draw, in the
 *             reference's draw order (s_j, t_j per round, then s_star, t_star); NULL = the OS CSPRNG
 *   C, r    : nbatch x 32 bytes: the commitment (absorbed into the transcript as given) and its blinding factor
 *   a       : nbatch x n x 32 canonical scalars (secret); b : nbatch x n x 32, or n x 32 when b_shared != 0 (public)
 *   G       : n x 32 bytes; F, B : 32 bytes (compressed points, shared by the batch); G = F = B = NULL: the context's
 *             generators as in bpgpu_linear_verify_batch -- every L_j, R_j, S is then a pure window-table MSM
 *   proofs_out : nbatch x 32*(2 lg n + 3) bytes; status_out : nbatch bytes (BPGPU_MSM_OK, or why no proof was made:
 *             an undecodable point or a non-canonical scalar); transcripts_out : optional nbatch x 208 bytes, each
 *             proof's transcript as create() leaves it */
int bpgpu_linear_create_batch(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *label, size_t label_len,
                              const uint8_t *shared_transcript, const uint8_t *rng, const uint8_t *C, const uint8_t *r,
                              const uint8_t *a, const uint8_t *b, int b_shared, const uint8_t *G, const uint8_t *F,
                              const uint8_t *B, uint8_t *proofs_out, uint8_t *status_out, uint8_t *transcripts_out);

/* ---- the dealer's share audit of the multi-party range-proof protocol ---------------------------
 * nshares independent calls of
 *   ProofShare::audit_share(&self, bp_gens, pc_gens, j, &bit_commitment, &bit_challenge, &poly_commitment, &poly_challenge)
 * (src/range_proof/messages.rs:85-167): what Dealer::receive_shares runs for every party when the aggregated proof does
 * not verify (src/range_proof/dealer.rs:303-335), to name the parties whose shares are malformed.  Per share: the check
 * t_x == <l_vec, r_vec> and two multiscalar multiplications (2n + 3 and 5 terms, messages.rs:128-141, 149-160) whose
 * results must be the identity; generators are the context's (bpgpu_gens_create / _load).
 *   n           : bitsize of the shares (l_vec.len(): 8, 16, 32 or 64); n > gens_capacity fails every share (check_size)
 *   party_index : nshares x uint32, the party position j of each share (j >= party_capacity fails that share)
 *   shares      : nshares x 32*(3 + 2n) bytes: t_x, t_x_blinding, e_blinding, l_vec[n], r_vec[n] (canonical scalars;
 *                 a non-canonical one fails the share -- upstream they are Scalars by type)
 *   bit_commitments  : nshares x 96 bytes: V_j, A_j, S_j (compressed; A_j, S_j are RistrettoPoints upstream: an
 *                 undecodable encoding fails the share here)
 *   poly_commitments : nshares x 64 bytes: T_1_j, T_2_j
 *   challenges  : nshares x 96 bytes (y, z, x per share), or 96 bytes when challenges_shared != 0
 *   verdict     : nshares bytes: BPGPU_VERDICT_OK = Ok(()), BPGPU_VERDICT_VERIFICATION_ERROR = Err(())
 *   checks_out  : optional nshares x 64 bytes: compress(P_check), compress(t_check) (parity tests) */
int bpgpu_rangeproof_audit_shares(bpgpu_ctx *ctx, size_t n, size_t nshares, const uint32_t *party_index,
                                  const uint8_t *shares, const uint8_t *bit_commitments, const uint8_t *poly_commitments,
                                  const uint8_t *challenges, int challenges_shared, uint8_t *verdict, uint8_t *checks_out);

/* ---- batched inner-product-proof creation (prover side) --------------------------------
 * nbatch independent calls of
 *   InnerProductProof::create(&mut transcript, &Q, G_factors, H_factors, G_vec, H_vec, a_vec, b_vec).to_bytes()
 * (src/inner_product_proof.rs:38-193), all of one size n (a power of two): per round the reference forms L and R with
 * two (2n'+1)-term multiscalar multiplications (ipp.rs:87-113) and folds the generators with 2n' two-term ones
 * (ipp.rs:127-178); here all proofs advance round by round together and every L_j / R_j is one multiscalar
 * multiplication over the ORIGINAL points (csrc/ipp_prover.h), which yields the same group elements: proofs are
 * byte-identical to the reference algorithm's.
 *   transcript  : shared_transcript (host, 208 bytes, may hold earlier messages) if not NULL, else Transcript::new(label);
 *                 innerproduct_domain_sep(n) is applied here, as create() does
 *   Q           : nbatch x 32;  G_factors, H_factors, a, b : nbatch x n x 32 (canonical scalars)
 *   G, H        : nbatch x n x 32, or n x 32 when bases_shared != 0 (compressed points)
 *   proofs_out  : nbatch x 32 * (2 lg n + 2) bytes: L_1 R_1 ... L_k R_k a b   (InnerProductProof::to_bytes, ipp.rs:334-345)
 *   status      : nbatch bytes, BPGPU_MSM_* (a point that does not decode / a non-canonical scalar: that proof is void)
 * VARIABLE TIME in the secret vectors a, b -- as the reference's create(), which calls vartime_multiscalar_mul -- and
 * therefore no replacement for the constant-time commitments of the range-proof parties (party.rs:119-124). */
int bpgpu_ipp_create_batch(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *label, size_t label_len,
                           const uint8_t *shared_transcript, const uint8_t *Q, const uint8_t *G_factors,
                           const uint8_t *H_factors, const uint8_t *G, const uint8_t *H, int bases_shared,
                           const uint8_t *a, const uint8_t *b, uint8_t *proofs_out, uint8_t *status);

/* ---- creation on the callers' own transcripts ------------------------------------------------------------------------------
 * bpgpu_ipp_create_batch / bpgpu_linear_create_batch with `label, label_len, shared_transcript` replaced by `transcripts,
 * transcript_stride` -- the convention, errors and contracts of the _ts verifiers above (bpgpu_ipp_verify_batch_ts): the callers' states
 * before innerproduct_domain_sep(n), which the device applies per proof; every output of row p equals the sibling's with nbatch = 1
 * and shared_transcript = transcripts[p], and with transcript_stride = 0 the sibling's on the whole batch.
 *   transcripts_out : optional nbatch x 208 bytes: each proof's state as create() leaves it (inner product: after the last u
 *                     challenge; linear: after x_star) -- the state the matching _ts verifier leaves for the proof.
 * bpgpu_linear_create_batch_ts takes its randomness as ONE seed per proof:
 *   rng32 : nbatch x 32 bytes; the rng handed to create() is ChaChaRng::from_seed(rng32[p]) (rand_chacha: ChaCha20, 64-bit block
 *           counter, stream id 0).  Draw d is Scalar::from_bytes_mod_order_wide(keystream block d), in the reference's order
 *           (linear_proof.rs:103-104, 146-147): s_j = draw 2j, t_j = draw 2j + 1, s_star = draw 2 lg n, t_star = draw 2 lg n + 1 --
 *           the proof bpgpu_linear_create_batch makes from rng = keystream blocks 0 .. 2 lg n + 1 of the seed.  The draws are computed
 *           on the device by the lane that fills the chain's working set; no buffer of draws exists in the caller's memory or in
 *           staging.  NULL: 32 bytes per proof from the OS CSPRNG.  The seeds are secrets: they sit in the secret part of the staging
 *           block and are cleared with the working set on every exit, error paths included. */
int bpgpu_ipp_create_batch_ts(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *transcripts, size_t transcript_stride,
                              const uint8_t *Q, const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *G,
                              const uint8_t *H, int bases_shared, const uint8_t *a, const uint8_t *b, uint8_t *proofs_out,
                              uint8_t *status, uint8_t *transcripts_out);
int bpgpu_linear_create_batch_ts(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *transcripts, size_t transcript_stride,
                                 const uint8_t *rng32, const uint8_t *C, const uint8_t *r, const uint8_t *a, const uint8_t *b,
                                 int b_shared, const uint8_t *G, const uint8_t *F, const uint8_t *B, uint8_t *proofs_out,
                                 uint8_t *status_out, uint8_t *transcripts_out);

/* ---- batched range-proof creation (prover side) ------------------------------------------
 * nbatch independent calls of
 *   RangeProof::prove_multiple_with_rng(bp_gens, pc_gens, &mut transcript, &values, &blindings, n, rng)
 * (src/range_proof/mod.rs:234-288, running the dealer / party protocol of party.rs and dealer.rs in-line), all of one
 * shape (n, m = values per proof): every commitment (V_j, A, S, T_1, T_2, Q) is a multiscalar multiplication over the
 * generator tables, the inner-product argument is bpgpu_ipp_create_batch's (csrc/rp_prover.h).  Byte-identical to the
 * reference algorithm given the same random scalars.
 *   values      : nbatch x m u64 (each < 2^n);  blindings : nbatch x m x 32 bytes (Scalars, reduced mod l)
 *   transcript  : shared_transcript (host, 208 bytes, may hold earlier messages) if not NULL, else Transcript::new(label)
 *   rng         : nbatch x 64 * (m * (2n + 2) + 2m) bytes = what the rng would hand Scalar::random, in the order the
 *                 reference draws: per party j: a_blinding, s_blinding, s_L[0..n), s_R[0..n); then per party j:
 *                 t_1_blinding, t_2_blinding.  NULL = OS CSPRNG (the thread_rng() of prove_multiple).
 *   proofs_out  : nbatch x 32 * (9 + 2 lg(n m)) bytes (RangeProof::to_bytes);  commitments_out : nbatch x m x 32 bytes
 *   transcripts_out : optional nbatch x 208 bytes: each proof's transcript as the prover leaves it
 * Returns BPGPU_ERR_INVALID_ARG for the reference's InvalidBitsize / InvalidAggregation (m not a power of two) / a value
 * that does not fit n bits, BPGPU_ERR_NO_GENS for InvalidGeneratorsLength.
 * Timing: by default VARIABLE TIME in the secrets (values, blindings, s_L, s_R) -- the window-table walk is indexed by their
 * digits; for provers whose GPU an adversary cannot observe.  With the context option "prover_constant_time" = 1 the
 * secret-dependent commitments V_j, A, S, T_1, T_2 -- the ones the reference computes with its constant-time
 * multiscalar_mul (party.rs:99-124, 179-187; generators.rs:39-41) -- take a small-window table walk whose addresses and
 * instruction stream do not depend on the scalars (every (generator, window) pair reads all 8 table entries, selects by masks,
 * always adds; csrc/msm_fixed.h).  Proofs are byte-identical either way.  The inner-product rounds stay variable-time, as in the
 * reference (vartime_multiscalar_mul at ipp.rs:87-178).  Cost: ~2x the prover's time at (64, 1).
 * Secrets at rest: like the reference's parties (zeroize on Drop, party.rs:148-260), every prover entry point
 * (bpgpu_rangeproof_prove_batch, bpgpu_ipp_create_batch, bpgpu_linear_create_batch, bpgpu_r1cs_prove_batch) clears what it staged before it returns,
 * on success and on every error path: the context's device IO buffer, the provers' working sets and the MSM arena (window
 * digits of secret scalars) on the stream behind the last copy, then the secret part of the pinned host staging block.
 * Not cleared: the caller's own buffers. */
int bpgpu_rangeproof_prove_batch(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch, const uint64_t *values,
                                 const uint8_t *blindings, const uint8_t *label, size_t label_len,
                                 const uint8_t *shared_transcript, const uint8_t *rng,
                                 uint8_t *proofs_out, uint8_t *commitments_out, uint8_t *transcripts_out);

/* The same proofs on the callers' OWN transcripts, with the random scalars drawn on the device from one 32-byte seed per proof.
 *   transcripts : the callers' states BEFORE rangeproof_domain_sep(n, m), at any STROBE position: one 208-byte state shared by
 *                 every proof (transcript_stride = 0) or one per proof (transcript_stride = BPGPU_TRANSCRIPT_BYTES).  The separator is
 *                 applied per proof on the device.  transcripts_out (optional, nbatch x 208): each state as the prover leaves it --
 *                 what bpgpu_rangeproof_verify_batch_ts leaves for the same proof.
 *   rng32       : nbatch x 32 bytes, proof p's seed: the rng handed to prove_multiple_with_rng is rand_chacha's
 *                 ChaChaRng::from_seed(rng32[p]).  Draw d of proof p is Scalar::from_bytes_mod_order_wide of keystream block d of
 *                 ChaCha20 under that key (64-bit block counter d, stream id 0), d in the order of the `rng` buffer above:
 *                 party j: a_blinding j(2n+2), s_blinding j(2n+2)+1, s_L[i] j(2n+2)+2+i, s_R[i] j(2n+2)+2+n+i;
 *                 t_1_blinding_j m(2n+2)+2j, t_2_blinding_j m(2n+2)+2j+1.  Each draw is computed by the device lane that consumes it:
 *                 no buffer of draws exists in the caller's memory, in staging or on the device.
 *                 NULL = 32 bytes per proof from the OS-seeded CSPRNG of the library.
 * CONTRACT: for every p the three outputs equal bpgpu_rangeproof_prove_batch(nbatch = 1, shared_transcript = transcripts[p],
 * rng = keystream blocks 0 .. D-1 of rng32[p]) with D = m(2n+2) + 2m.
 * Errors: those of bpgpu_rangeproof_prove_batch, and BPGPU_ERR_INVALID_ARG for transcripts == NULL, a stride other than 0 or 208
 * and a malformed state (every state is checked before anything is staged).  nbatch = 0 is BPGPU_OK.  "prover_constant_time"
 * applies as above.  The seeds are secrets: staged in the secret part of the staging block and cleared with it on every exit.
 * The _dev form takes device pointers (4-byte aligned, values 8-byte) and enqueues on `stream` (NULL: the context's own) with the
 * conventions of the other _dev entry points; nothing is read back, so what the host form checks in the data is the caller's
 * to guarantee: values < 2^n (a proof of a larger value does not verify) and well-formed states (a state whose position bytes are
 * out of range is started at position 0).  The library's working sets and the MSM arena are cleared on that stream behind the last
 * kernel; the caller's buffers are the caller's.  With d_rng32 = NULL the library draws the seeds, uploads them through its own
 * staging and clears that once the copy has completed (the one wait of the _dev form). */
int bpgpu_rangeproof_prove_batch_ts(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch, const uint64_t *values,
                                    const uint8_t *blindings, const uint8_t *transcripts, size_t transcript_stride,
                                    const uint8_t *rng32, uint8_t *proofs_out, uint8_t *commitments_out,
                                    uint8_t *transcripts_out);
int bpgpu_rangeproof_prove_batch_ts_dev(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch, const void *d_values,
                                        const void *d_blindings, const void *d_transcripts, size_t transcript_stride,
                                        const void *d_rng32, void *d_proofs_out, void *d_commitments_out,
                                        void *d_transcripts_out, void *stream);

/* ---- rewindable range proofs: value, message and blinding back out of (proof, commitment, seed) ---------------
 * The wallet side of a confidential ledger: a wallet that restores from its key, or follows the chain, finds its own outputs by
 * rewinding every (proof, commitment) row under the seed it would have used, and gets value and blinding back from what the chain
 * stores.  Nothing in the reference defines this; the protocol is fixed here.  m = 1 ONLY (any other m: BPGPU_ERR_INVALID_ARG): in an
 * aggregated proof the blindings and values of the parties cannot be separated.  csrc/rewind.h.
 * Write d_k for draw k of the proof's seed exactly as bpgpu_rangeproof_prove_batch_ts defines draws; for m = 1: d_0 is a_blinding,
 * d_1 s_blinding, d_{2n+2} t_1_blinding, d_{2n+3} t_2_blinding.
 * REWINDABLE PROVING (bpgpu_rangeproof_prove_batch_rw[_dev]): let e = v + 2^64 msg, msg the caller's optional 16-byte message read as
 * a little-endian integer (0 where none is given), so e < 2^192.  The proof is the seeded prover's proof with
 * a_blinding = d_0 - e (mod l); every other draw is unchanged.  a_blinding stays uniform; the proof is an ordinary proof of the
 * reference's format and verifies under every existing verifier.
 *   arguments : those of bpgpu_rangeproof_prove_batch_ts[_dev], plus messages: nbatch x 16 bytes, or NULL (every message 0).
 *               rng32 is REQUIRED (NULL: BPGPU_ERR_INVALID_ARG): a proof made from a seed nobody holds cannot be rewound.
 *   CONTRACT  : for every p the outputs equal bpgpu_rangeproof_prove_batch(nbatch = 1, shared_transcript = transcripts[p], rng = ...)
 *               where rng is keystream blocks 0 .. 2n+3 of rng32[p] with block 0 replaced by the 32 canonical bytes of (d_0 - e) mod l,
 *               zero-extended to 64.
 *   "prover_constant_time" applies as before.  The messages are secrets like values, blindings and seeds: staged in the secret span
 *   and cleared with it on every exit.
 * REWINDING row p (bpgpu_rangeproof_rewind_batch[_dev]): inputs are the proof bytes, the commitment V, the caller's state BEFORE
 * rangeproof_domain_sep (any STROBE position; one shared state with transcript_stride = 0, or one per row with 208) and the seed.
 *   1. Parse: proof_len must be 32 * (9 + 2 lg n) (else BPGPU_ERR_INVALID_ARG for the call); a proof that RangeProof::from_bytes
 *      rejects -- one of t_x, t_x_blinding, e_blinding, a, b not canonical -- gets status BPGPU_REWIND_FORMAT.
 *   2. Replay the transcript to x: rangeproof_domain_sep(n, 1); append V; validate-and-append A and S; challenges y, z;
 *      validate-and-append T_1 and T_2; challenge x.  A, S, T_1 or T_2 of 32 zero bytes: BPGPU_REWIND_NOT_FOUND.
 *   3. e = d_0 + d_1 x - e_blinding (mod l).  e >= 2^192: BPGPU_REWIND_NOT_FOUND.
 *   4. gamma = (t_x_blinding - x (d_{2n+2} + x d_{2n+3})) z^-2;  v = e mod 2^64;  msg = e >> 64.
 *   5. compress(v B + gamma B_blinding) != V: BPGPU_REWIND_NOT_FOUND; otherwise BPGPU_REWIND_OK.
 *   status_out : nbatch bytes;  values_out : nbatch u64;  messages_out : nbatch x 16 bytes;  blindings_out : nbatch x 32 bytes.
 *   The three data outputs of a row are all zero unless its status is BPGPU_REWIND_OK.  rng32: nbatch x 32 bytes, required.
 * WHAT REWINDING IS NOT:
 *   - It does NOT verify the proof.  A changed e_blinding can change the recovered message and still pass step 5 (the message takes
 *     no part in the commitment), so a recovered message is only as good as the proof's verification: verify first.
 *   - Whoever holds a seed opens the output: value, message and blinding.
 *   - A SEED MUST NEVER SERVE TWO (COMMITMENT, TRANSCRIPT) PAIRS: the existing rule for seeds (two proofs from one set of nonces give
 *     away the secrets).  Derive it from (key, commitment), as below.
 *   - z is public: its inversion is the variable-time one, also under "prover_constant_time".
 *   - Scanning under many keys (bpgpu_rangeproof_scan_batch, below) decides a row by the LOWEST key whose candidate passes step 3, not
 *     by the first key that opens it: a key that passes step 3 and fails step 5 makes the row BPGPU_REWIND_NOT_FOUND even if a higher
 *     key would open it.  It verifies no more than rewinding does.
 *   - With value 0 and no message e = 0: bpgpu_rangeproof_prove_batch_ts's proof of the value 0 IS the rewindable proof and rewinds
 *     under its seed.  Every other proof of the seeded prover gives BPGPU_REWIND_NOT_FOUND under its own seed (e = l - v >= 2^192).
 * SEED DERIVATION (RangeProof.rewind_seeds of the bindings; fixed here so that C and Rust callers reproduce it): seed_i is
 *     t = Transcript::new(b"bpgpu rewind seed v1"); t.append_message(b"key", key32); t.append_message(b"C", commitment_i);
 *     t.challenge_bytes(b"seed", 32 bytes)
 * -- one bpgpu_transcript_batch call for a batch of commitments.
 * Timing and secrets: ONE launch, lane = row.  By default variable time: a row rejected by step 1, 2 or 3 computes no gamma and
 * skips the walk over the window tables (a scan is almost all such rows).  With "prover_constant_time" = 1 every row computes gamma
 * and walks the W = 4 mask-select table of bpgpu_pedersen_commit_batch; nothing branches on e (a row that the parse or the replay
 * rejected -- public -- walks zeros).  The seeds and the three data outputs are secrets: the host form stages them in the secret
 * span and clears staging, the device IO buffer and the working sets on every exit, as bpgpu_rangeproof_prove_batch documents.
 * nbatch = 0 is BPGPU_OK; states and lengths are checked before anything is staged; at most 2^26 rows per call; a context without
 * generators returns BPGPU_ERR_NO_GENS.  The _dev forms take device pointers (4-byte aligned, values 8-byte) and enqueue on `stream`
 * (NULL: the context's own) with the conventions of the other _dev entry points; nothing is read back, and a state whose position
 * bytes are out of range is started at position 0.
 * Measured on one MI355X (profiles/rewind_rate.json; n = 64, one state per row, medians): 4 096 rows through host pointers --
 * 0.60 ms when every row is the caller's, 0.41 ms when none is, 0.74 ms constant-time, against 1.44 ms for bpgpu_rangeproof_verify_batch_ts
 * on the same proofs; the launch alone (_dev, buffers on the device) 0.26 / 0.09 / 0.56 ms at 4 096 rows and 0.29 / 0.11 / 0.70 ms at
 * 65 536, where the host-pointer call (4.3 - 4.6 ms) is its staging of 944 bytes per row.  The two provers do not differ beyond their
 * spreads (11.3 ms for 4 096 proofs either way). */
#define BPGPU_REWIND_OK 0
#define BPGPU_REWIND_NOT_FOUND 1
#define BPGPU_REWIND_FORMAT 2
int bpgpu_rangeproof_prove_batch_rw(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch, const uint64_t *values,
                                    const uint8_t *blindings, const uint8_t *transcripts, size_t transcript_stride,
                                    const uint8_t *rng32, const uint8_t *messages, uint8_t *proofs_out, uint8_t *commitments_out,
                                    uint8_t *transcripts_out);
int bpgpu_rangeproof_prove_batch_rw_dev(bpgpu_ctx *ctx, size_t n, size_t m, size_t nbatch, const void *d_values,
                                        const void *d_blindings, const void *d_transcripts, size_t transcript_stride,
                                        const void *d_rng32, const void *d_messages, void *d_proofs_out, void *d_commitments_out,
                                        void *d_transcripts_out, void *stream);
int bpgpu_rangeproof_rewind_batch(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                  const uint8_t *commitments, const uint8_t *transcripts, size_t transcript_stride,
                                  const uint8_t *rng32, uint8_t *status_out, uint64_t *values_out, uint8_t *messages_out,
                                  uint8_t *blindings_out);
int bpgpu_rangeproof_rewind_batch_dev(bpgpu_ctx *ctx, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                                      const void *d_commitments, const void *d_transcripts, size_t transcript_stride,
                                      const void *d_rng32, void *d_status_out, void *d_values_out, void *d_messages_out,
                                      void *d_blindings_out, void *stream);

/* ---- scanning range proofs under many wallet keys: one transcript replay per row ----------------------------------
 * A wallet service, an exchange with sub-accounts or a wallet with rotated view keys holds nkeys keys and follows one chain.  With
 * bpgpu_rangeproof_rewind_batch it makes nkeys passes, each deriving its seeds and replaying every row's transcript again; the replay
 * does not depend on the key.  bpgpu_rangeproof_scan_batch[_dev] replays once per row and tests every key's candidate.  csrc/scan.h.
 *   keys32 : nkeys x 32 bytes, shared by every row.  For row p:
 *   1. Parse and replay to x: steps 1 and 2 of REWINDING above, unchanged (BPGPU_REWIND_FORMAT and the zero-point
 *      BPGPU_REWIND_NOT_FOUND keep their meaning).  m = 1 only.
 *   2. For j = 0 .. nkeys-1: seed_{p,j} = the SEED DERIVATION above of (keys32[j], commitment_p), and e_j = d_0 + d_1 x - e_blinding
 *      with the draws of seed_{p,j}.  j* is the LOWEST j with e_j < 2^192.  None: BPGPU_REWIND_NOT_FOUND.
 *   3. Steps 4 and 5 of REWINDING with seed_{p,j*}: the status is BPGPU_REWIND_OK iff compress(v B + gamma B_blinding) == V.
 *   status_out : nbatch bytes;  key_index_out : nbatch x u32, j* when the status is OK, else 0xFFFFFFFF;  values_out, messages_out,
 *   blindings_out as in rewinding: all zero unless the status is OK.
 * CONSEQUENCES:
 *   - If at most one key of a row passes step 2, row p equals the first BPGPU_REWIND_OK among the seed derivation +
 *     bpgpu_rangeproof_rewind_batch run once per key, with key_index that key.  Every honest input is such a row, up to probability
 *     about nkeys * 2^-61 (a wrong seed's e is uniform mod l ~ 2^252.6 and passes the 2^192 test with probability 2^-60.6).
 *   - A key listed twice reports the lower index.
 *   - A key that passes step 2 and fails step 3 makes the row BPGPU_REWIND_NOT_FOUND, EVEN IF A HIGHER KEY WOULD OPEN IT: e_blinding is
 *     absorbed after x, so whoever writes the proof bytes can make any one key pass step 2.  Like everything under WHAT REWINDING IS
 *     NOT: scanning does NOT verify, and a recovered message is only as good as the proof's verification.  Verify first; a row that
 *     verifies and was made by bpgpu_rangeproof_prove_batch_rw is an honest input.
 * Limits, checked before anything is staged: 1 <= nkeys <= 1024, nbatch <= 2^26, nbatch * nkeys <= 2^28, the proof_len,
 * transcript_stride and state checks of rewinding (BPGPU_ERR_INVALID_ARG); nbatch = 0 is BPGPU_OK; a context without generators
 * returns BPGPU_ERR_NO_GENS.
 * Timing and secrets: FOUR launches -- the keys' STROBE prefixes (lane = key), the replay (lane = row), the candidate test
 * (lane = (row, key)) and the open (lane = row).  A candidate's state stands at STROBE position 91 after the key; C and the challenge
 * take it to 144 < 166, so a candidate costs ONE Keccak-f, two ChaCha blocks and one scalar multiply-add.  Rows whose replay failed
 * spend nothing per key.  With "prover_constant_time" = 1 nothing branches on e or j* and no address depends on them: every
 * (row, key) lane of a replayed row does the same work, j*'s key is picked by mask-select over a loop across all keys, and every
 * replayed row derives one seed, computes one gamma and walks the W = 4 table (a row without a survivor walks a discarded candidate;
 * a row that the parse or the replay rejected -- public -- walks zeros); z's inversion stays the variable-time one.  Keys, derived
 * seeds, x-dependent candidates and the outputs (the key index included) are secrets: the host form stages keys and outputs in the
 * secret span and clears staging, the device IO buffer and every working set on every exit; the _dev form stages nothing, reads
 * nothing back and clears its working set on `stream` behind the last launch.  _dev: device pointers 4-byte aligned (values 8-byte),
 * enqueued on `stream` (NULL: the context's own) with the conventions of the other _dev entry points.
 * Measured on one MI355X (profiles/scan_rate.json; n = 64, one state per row, medians, _dev forms on device-resident buffers)
 * against the path it replaces, nkeys x (the seed derivation through bpgpu_transcript_batch_dev + bpgpu_rangeproof_rewind_batch_dev):
 * 4 096 rows x 16 keys 0.12 ms against 2.11 ms when no row is the caller's and 0.32 against 2.28 ms when every row belongs to the last
 * key; 4 096 x 256: 0.39 / 0.58 against 33.7 / 34.0 ms; 65 536 x 16: 0.44 / 0.76 against 2.58 / 2.76 ms; 65 536 x 256: 4.62 / 4.87 against
 * 41.5 / 41.6 ms (3.6 G candidates/s).  AT ONE KEY THE SCAN IS NOT FASTER: 0.32 against 0.30 ms at 4 096 rows that are all the caller's
 * (0.93 of the passes' speed) and 1.24 - 1.26 times bpgpu_rangeproof_rewind_batch_dev with ready seeds (0.26 ms): four launches and a
 * second derivation of the seed.  With one key, derive the seeds and rewind.  The kernel split (rocprofv3 --kernel-trace --stats,
 * 65 536 x 16): candidates 299 us, open 4 (none mine) to 360 us (all mine), replay 124 us, prefixes 11 us. */
int bpgpu_rangeproof_scan_batch(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                const uint8_t *commitments, const uint8_t *transcripts, size_t transcript_stride,
                                const uint8_t *keys32, size_t nkeys, uint8_t *status_out, uint32_t *key_index_out,
                                uint64_t *values_out, uint8_t *messages_out, uint8_t *blindings_out);
int bpgpu_rangeproof_scan_batch_dev(bpgpu_ctx *ctx, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                                    const void *d_commitments, const void *d_transcripts, size_t transcript_stride,
                                    const void *d_keys32, size_t nkeys, void *d_status_out, void *d_key_index_out,
                                    void *d_values_out, void *d_messages_out, void *d_blindings_out, void *stream);

/* ---- batches of Pedersen commitments and openings -----------------------------------------------
 * nbatch calls of PedersenGens::commit(value, blinding) = value B + blinding B_blinding (src/generators.rs:38-42) with the bases
 * the context holds, in ONE launch: a lane walks the window tables of the two bases that already sit in device memory (no point is
 * decoded, nothing is doubled), compresses its point and stores the 32 bytes (commit) or compares them with a given commitment
 * (open).  csrc/pedersen.h.
 *   values       : value_bytes = 8: nbatch u64; value_bytes = 32: nbatch x 32-byte scalars.  Anything else: BPGPU_ERR_INVALID_ARG.
 *   blindings    : nbatch x 32 bytes, with rng_seed32 == NULL and first_draw == 0 (else BPGPU_ERR_INVALID_ARG); or NULL, the
 *                  SEEDED mode: blinding i is draw first_draw + i of rand_chacha's ChaChaRng::from_seed(rng_seed32) -- ONE rng for
 *                  the batch, one Scalar::random per commitment: Scalar::from_bytes_mod_order_wide of keystream block
 *                  first_draw + i (64-bit block counter, stream id 0), exactly as documented for bpgpu_rangeproof_prove_batch_ts,
 *                  computed by the lane that consumes it.  rng_seed32 == NULL then means 32 bytes from the library's OS-seeded
 *                  generator, and blindings_out is required (BPGPU_ERR_INVALID_ARG if it is NULL).
 *   commitments_out : nbatch x 32 bytes
 *   blindings_out   : nbatch x 32 bytes: the blindings used (given or drawn); optional when the caller gave the seed or the blindings
 *   status_out      : nbatch bytes: BPGPU_MSM_OK, or BPGPU_MSM_BAD_SCALAR for a non-canonical value or blinding -- that row's
 *                     commitment is then 32 zero bytes (the status tells it from the commitment to (0, 0), which is 32 zero bytes
 *                     with BPGPU_MSM_OK); the other rows are unaffected.
 * CONTRACT: row i of the commit call equals bpgpu_msm_batch with the two terms (value_i, B), (blinding_i, B_blinding) -- what
 * BulletproofGens.commit of the Python package returns -- whatever "fixed_window_bits" and "prover_constant_time" are.
 * bpgpu_pedersen_open_batch: verdict_out, nbatch bytes of BPGPU_VERDICT_*: 0 = (value_i, blinding_i) opens commitments[i];
 * VerificationError = it does not, which includes a commitment that is no valid encoding (the encodings are compared, and the
 * encoder's output is canonical); FormatError = a non-canonical scalar.
 * nbatch = 0 is BPGPU_OK; a context without generators returns BPGPU_ERR_NO_GENS; one call takes at most 2^28 rows.
 * Timing: VARIABLE TIME in the scalars by default.  With the context option "prover_constant_time" = 1 the commit forms walk the
 * small-window table of the provers' constant-time path: every (generator, window) pair reads all 8 entries, selects by masks and
 * always adds, and the number of B windows follows from the value's type (u64 or scalar), never from its bits; the bytes are the
 * same.  The open forms are always variable time: their inputs are public to the verifier.
 * Secrets: values, blindings and seeds are staged through the provers' secret staging; staging, the device IO buffer and the working
 * sets are cleared on every exit, as bpgpu_rangeproof_prove_batch documents.  The _dev forms take device pointers (4-byte aligned)
 * and enqueue on `stream` (NULL: the context's own) with the conventions of the other _dev entry points; nothing is read back.
 * They clear what the library itself allocated (the slot of a library-drawn seed) on the stream behind the kernel; with
 * d_rng_seed32 = NULL and d_blindings = NULL the library draws the seed, uploads it through its own staging and clears that once
 * the copy has completed (the one wait of the _dev form). */
int bpgpu_pedersen_commit_batch(bpgpu_ctx *ctx, size_t nbatch, const void *values, size_t value_bytes,
                                const uint8_t *blindings, const uint8_t *rng_seed32, uint64_t first_draw,
                                uint8_t *commitments_out, uint8_t *blindings_out, uint8_t *status_out);
int bpgpu_pedersen_open_batch(bpgpu_ctx *ctx, size_t nbatch, const uint8_t *commitments, const void *values, size_t value_bytes,
                              const uint8_t *blindings, uint8_t *verdict_out);
int bpgpu_pedersen_commit_batch_dev(bpgpu_ctx *ctx, size_t nbatch, const void *d_values, size_t value_bytes,
                                    const void *d_blindings, const void *d_rng_seed32, uint64_t first_draw,
                                    void *d_commitments_out, void *d_blindings_out, void *d_status_out, void *stream);
int bpgpu_pedersen_open_batch_dev(bpgpu_ctx *ctx, size_t nbatch, const void *d_commitments, const void *d_values, size_t value_bytes,
                                  const void *d_blindings, void *d_verdict_out, void *stream);

/* ---- signed sums of Pedersen commitments, and the balance check over them ------------------------
 * What the commitments are for: a validator of confidential transactions checks, beside the range proofs, that inputs minus outputs
 * open to (fee, excess); a wallet or ledger updates a committed balance, C' = C + v B + r B_blinding.  csrc/pedersen_sum.h.
 * A call has nbatch rows.  Row r owns the terms [row_offsets[r], row_offsets[r + 1]) of ONE flat array of 32-byte Ristretto encodings.
 *   row_offsets : HOST array of nbatch + 1 uint32_t, non-decreasing, row_offsets[0] = 0 (also in the _dev forms: the launch geometry
 *                 follows from it, as from n_terms in bpgpu_msm_batch_dev).  A row may have no terms.  At most 2^28 rows and 2^28
 *                 terms per call.
 *   points      : row_offsets[nbatch] x 32 bytes
 *   signs       : one byte per term, 0 = add, 1 = subtract; NULL = every term is added
 *   values      : optional.  value_bytes = 8: nbatch u64; value_bytes = 32: nbatch x 32-byte scalars.  NULL = 0.
 *   blindings   : optional, nbatch x 32 bytes.  NULL = 0.
 * With S_r = sum_{sign 0} C_i - sum_{sign 1} C_i and O_r = values[r] B + blindings[r] B_blinding (the context's bases):
 * bpgpu_pedersen_sum_batch:     out[r] = compress(S_r + O_r), 32 bytes.  status_out[r] = BPGPU_MSM_OK, BPGPU_MSM_BAD_POINT when a term
 *   of the row does not decode, BPGPU_MSM_BAD_SCALAR when the value or the blinding is not canonical.  A rejected row's output is 32
 *   zero bytes; the other rows are unaffected.
 * bpgpu_pedersen_balance_batch: verdict_out[r] = BPGPU_VERDICT_OK iff S_r == O_r as Ristretto elements -- the signed sum opens to
 *   (value, blinding).  The test is the coset identity test (X == 0 or Y == 0) on S_r - O_r: nothing is compressed, no inversion is
 *   taken.  BPGPU_VERDICT_VERIFICATION_ERROR when the row does not balance or a term does not decode (a None of
 *   optional_multiscalar_mul in the verifiers); BPGPU_VERDICT_FORMAT_ERROR for a scalar that is not canonical.
 * In both a scalar that is not canonical takes precedence over a point that does not decode in the same row (as in
 * bpgpu_pedersen_open_batch).  nbatch = 0 is BPGPU_OK.  With values == NULL and blindings == NULL no generator is needed and the call
 * works on a context that never loaded any (as bpgpu_r1cs_witness_check does); otherwise such a context returns BPGPU_ERR_NO_GENS.
 * BPGPU_ERR_INVALID_ARG: a value_bytes other than 8 or 32 when values is given; offsets that decrease or do not start at 0; too many
 * rows or terms; in the host forms a sign byte above 1 (the _dev forms use bit 0 of the byte and read nothing back).
 * CONTRACTS: (a) row r of the sum call equals bpgpu_msm_batch on the terms (+-1, C_i) ..., (value, B), (blinding, B_blinding);
 * (b) a row without terms equals row r of bpgpu_pedersen_commit_batch; (c) a balance row with exactly one added term has the verdict
 * of bpgpu_pedersen_open_batch on the same (commitment, value, blinding) -- whatever "fixed_window_bits" and "prover_constant_time"
 * are.
 * Timing and secrets: the balance forms are VARIABLE TIME; their inputs are public to a verifier.  In the sum forms the commitments are
 * public, but (value, blinding) may be a wallet's secrets: the walk over B and B_blinding honours "prover_constant_time" exactly as
 * bpgpu_pedersen_commit_batch does (the bytes are the same either way), and a host form that is given a value or a blinding -- sum or
 * balance: an opening is shown to this verifier alone, as in bpgpu_pedersen_open_batch -- stages them through the provers' secret
 * staging: staging, the device IO buffer and the working sets are cleared on every exit, as bpgpu_rangeproof_prove_batch documents.
 * The _dev forms take device pointers for points, signs, values, blindings and outputs (4-byte aligned; signs at any alignment) and
 * enqueue on `stream` (NULL: the context's own) with the conventions of the other _dev entry points.  The only host -> device traffic
 * is the library's own plan table (a few words per row), through its staging; what the library allocated for the call (plan table,
 * row flags, partial sums) is cleared on the stream behind the last kernel. */
int bpgpu_pedersen_sum_batch(bpgpu_ctx *ctx, size_t nbatch, const uint32_t *row_offsets, const uint8_t *points, const uint8_t *signs,
                             const void *values, size_t value_bytes, const uint8_t *blindings, uint8_t *out, uint8_t *status_out);
int bpgpu_pedersen_balance_batch(bpgpu_ctx *ctx, size_t nbatch, const uint32_t *row_offsets, const uint8_t *points, const uint8_t *signs,
                                 const void *values, size_t value_bytes, const uint8_t *blindings, uint8_t *verdict_out);
int bpgpu_pedersen_sum_batch_dev(bpgpu_ctx *ctx, size_t nbatch, const uint32_t *row_offsets, const void *d_points, const void *d_signs,
                                 const void *d_values, size_t value_bytes, const void *d_blindings, void *d_out, void *d_status_out,
                                 void *stream);
int bpgpu_pedersen_balance_batch_dev(bpgpu_ctx *ctx, size_t nbatch, const uint32_t *row_offsets, const void *d_points, const void *d_signs,
                                     const void *d_values, size_t value_bytes, const void *d_blindings, void *d_verdict_out, void *stream);

/* ---- proofs of knowledge of commitment openings -------------------------------------------------
 * A validator of someone else's transactions never sees a blinding; it is handed a PROOF that the sender knows the opening of
 * C = v B + r B_blinding (the context's bases): the excess signature of a Mimblewimble kernel, the proof that goes with a committed
 * balance.  A sigma protocol, csrc/opening.h; nothing in the reference defines it.  A call has ONE form:
 *   BPGPU_OPENING_FULL     : v and r are secret.        proof = R | s_v | s_r, 96 bytes.
 *   BPGPU_OPENING_BLINDING : v is public, r is secret.  proof = R | s_r, 64 bytes.  With v = 0 a Schnorr signature under the key C on
 *                            the base B_blinding: the excess proof.
 * Transcript, in the style of src/transcript.rs, applied to the caller's own state at any STROBE position:
 *     append_message(b"dom-sep", b"openingproof v1"); append_u64(b"form", form); append_point(b"C", C);
 *     form 1 only: append_scalar(b"v", v)  -- a u64 value zero-extended to 32 bytes;
 *     validate_and_append_point(b"R", R)   -- 32 zero bytes: VerificationError, nothing of R absorbed;
 *     c = challenge_scalar(b"c").
 * Prover: nonces k_v (form 0 only) and k_r; R = k_v B + k_r B_blinding; s_v = k_v + c v; s_r = k_r + c r.
 * Verifier: s_v from the proof (form 0) or s_v = c v (form 1); s_v B + s_r B_blinding - c C - R must be the identity.
 * Arguments (the transcript arguments, the shared_transcript / d_transcripts pair of the _dev forms, malformed states, nbatch = 0 and
 * BPGPU_VERDICT_UNDECIDED are those of bpgpu_linear_verify_rlc_ts[_dev] above):
 *   form         : BPGPU_OPENING_FULL or BPGPU_OPENING_BLINDING; anything else is BPGPU_ERR_INVALID_ARG.
 *   proof_len    : 96 (form 0) or 64 (form 1); anything else is BPGPU_ERR_INVALID_ARG.
 *   commitments  : nbatch x 32 bytes.
 *   values       : value_bytes = 8: nbatch u64; 32: nbatch x 32-byte scalars; any other value_bytes with values given is BPGPU_ERR_INVALID_ARG.  Creation:
 *                  required in form 0; NULL in form 1 when every value is 0.  Verification: NULL in form 0 (the value is not public);
 *                  in form 1 the public values, NULL when every value is 0.
 *   blindings    : creation, nbatch x 32 bytes.
 *   rng32        : creation, ONE 32-byte seed per proof: ChaChaRng::from_seed(rng32[p]), as in bpgpu_linear_create_batch_ts.  Form 0:
 *                  k_v = draw 0, k_r = draw 1; form 1: k_r = draw 0.  NULL: the seeds come from the OS CSPRNG.  A SEED MUST NEVER BE
 *                  USED FOR TWO DIFFERENT STATEMENTS OR TRANSCRIPTS: two proofs with one nonce and different challenges give away r
 *                  (and v).  Fixed seeds are for tests and for derandomised signing under a seed derived from (secret, statement,
 *                  transcript).
 *   status       : creation, nbatch bytes: BPGPU_MSM_OK, or BPGPU_MSM_BAD_SCALAR for a value or blinding that is not canonical -- that
 *                  row's proof bytes are zero and its transcripts_out row is its input state; the other rows are unaffected.
 *   msm_out      : optional nbatch x 32 bytes, compress of the row's check (32 zero bytes for a row that verifies or that stopped
 *                  before the multiplication).
 *   weights64, batch_out, verdict of the combined forms: as bpgpu_linear_verify_rlc_ts.
 * Verdicts and transcripts_out of the verifiers:
 *   a scalar of the proof that is not canonical : FORMAT_ERROR,        the input state
 *   a public value that is not canonical        : FORMAT_ERROR,        the input state
 *   R of 32 zero bytes                          : VERIFICATION_ERROR,  the state as of that message (separator, form, C, v absorbed)
 *   C or R that does not decode, a failing check: VERIFICATION_ERROR,  the state after c
 *   a proof that verifies                       : OK,                  the state after c
 * CONTRACTS (tests/test_gpu_opening.py):
 *   (a) a row's msm_out equals bpgpu_msm_batch on (s_v, B), (s_r, B_blinding), (l - c, C), (l - 1, R), with c taken from
 *       bpgpu_transcript_batch running the script above;
 *   (b) verdict and transcripts_out of an _rlc_ts call ALWAYS equal those of the _verify_batch_ts call on the same inputs; the host
 *       form falls back to the per-proof path where the combination does not decide, the _dev form marks BPGPU_VERDICT_UNDECIDED;
 *   (c) a proof from bpgpu_opening_create_batch_ts verifies, and the transcripts_out of the two sides are equal.
 * Timing and secrets: creation is ONE launch, lane = proof; its walk over the window tables is variable time unless the context option
 * "prover_constant_time" is set (the W = 4 mask-select table of bpgpu_pedersen_commit_batch; the same bytes); a rejected row walks like
 * any other.  v (form 0), r and the seeds are staged in the secret span: staging, the device IO buffer and the working sets are cleared
 * on every exit, as bpgpu_rangeproof_prove_batch documents.  The verifiers are variable time.  The context needs generators
 * (bpgpu_gens_create / _load with n >= 1), else BPGPU_ERR_NO_GENS.
 * Measured on one MI355X (profiles/opening_rate.json; host pointers, one state per proof, medians): 4 096 proofs -- creation
 * 0.33 / 0.38 ms (form 1 / 0), _verify_batch_ts 0.81 ms, _verify_rlc_ts 0.93 ms, against 0.97 ms for bpgpu_transcript_batch + bpgpu_msm_batch
 * on the four terms per row; 65 536 proofs -- _verify_rlc_ts 3.1 ms, _verify_batch_ts 8.3 ms, the old route 11.1 ms. */
#define BPGPU_OPENING_FULL 0
#define BPGPU_OPENING_BLINDING 1
int bpgpu_opening_create_batch_ts(bpgpu_ctx *ctx, int form, size_t nbatch, const uint8_t *transcripts, size_t transcript_stride,
                                  const uint8_t *rng32, const uint8_t *commitments, const void *values, size_t value_bytes,
                                  const uint8_t *blindings, uint8_t *proofs_out, uint8_t *status, uint8_t *transcripts_out);
int bpgpu_opening_verify_batch_ts(bpgpu_ctx *ctx, int form, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                  const uint8_t *transcripts, size_t transcript_stride, const uint8_t *commitments,
                                  const void *values, size_t value_bytes, uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out);
int bpgpu_opening_verify_batch_ts_dev(bpgpu_ctx *ctx, int form, size_t nbatch, const void *d_proofs, size_t proof_len,
                                      const uint8_t *shared_transcript, const void *d_transcripts, const void *d_commitments,
                                      const void *d_values, size_t value_bytes, void *d_verdict, void *d_msm_out,
                                      void *d_transcripts_out, void *stream);
int bpgpu_opening_verify_rlc_ts(bpgpu_ctx *ctx, int form, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                const uint8_t *transcripts, size_t transcript_stride, const uint8_t *commitments,
                                const void *values, size_t value_bytes, const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out,
                                uint8_t *transcripts_out);
int bpgpu_opening_verify_rlc_ts_dev(bpgpu_ctx *ctx, int form, size_t nbatch, const void *d_proofs, size_t proof_len,
                                    const uint8_t *shared_transcript, const void *d_transcripts, const void *d_commitments,
                                    const void *d_values, size_t value_bytes, const void *d_weights64, void *d_verdict,
                                    void *d_batch_out, void *d_transcripts_out, void *stream);

/* ---- proofs of recorded linear relations between points -------------------------------------------
 * The sigma protocol of the opening proofs over ANY set of linear equations between points (csrc/sigma.h; nothing in the reference
 * defines it): "two commitments under different value bases hold the same amount", "a key and a tag share a discrete log" (DLEQ), "an
 * ElGamal pair encrypts what a commitment commits to", "I can open this vector commitment".  A relation is recorded once per context,
 * as a gadget is for R1CS (bpgpu_r1cs_circuit_create), and batches are proved and verified against the record.
 * THE RELATION: S secret scalars x_0 .. x_{S-1}, P instance-point slots per row, E equations, each of 1 .. 8; equation k reads
 *     slot[lhs_k] = sum_t x[sec_{k,t}] Base[base_{k,t}]     with 1 .. 8 terms, at most 32 terms in all.
 * A base id is 0 = B_blinding or 1 = B of the context's generators, 2 + i = G_i of party 0 (i < 8 and i < gens_capacity; custom shared
 * bases come in through bpgpu_gens_load), or 16 + p = instance slot p of the row.  An lhs is always 16 + p.  Public scalar coefficients
 * are out of scope: a caller folds them into an instance point (bpgpu_pedersen_sum_batch) before the call.
 * Canonical descriptor bytes:  u8 S, u8 P, u8 E,  then per equation  u8 lhs, u8 nterms,  then nterms x (u8 secret, u8 base).
 * bpgpu_sigma_relation_create returns BPGPU_ERR_INVALID_ARG when a count is out of range, an lhs is not an instance slot, a secret or a
 * slot index is out of range, a secret is used in no term, an instance slot is used nowhere, a G_i lies beyond the loaded generators,
 * or the bytes end early or late.  It stores digest = Transcript(b"sigma statement"), append_message(b"desc", bytes),
 * challenge_bytes(b"digest", 32).  The relation belongs to the context it was recorded on and may only be used there (another context, also a later one at the same
 * address, is BPGPU_ERR_INVALID_ARG).  bpgpu_sigma_relation_destroy waits for the device to drain before it frees the record, so it may
 * follow an asynchronous _dev call directly; it must not run concurrently with a call that uses the relation.  Destroying it after the
 * context is allowed.
 * Transcript, applied to the caller's own state at any STROBE position:
 *     append_message(b"dom-sep", b"sigmaproof v1"); append_message(b"stmt", digest);
 *     append_point(b"P", P_i) for the P instance points in slot order -- as given; the identity is allowed (a zero balance as an lhs);
 *     validate_and_append_point(b"T", T_k), k = 1 .. E -- 32 zero bytes: VerificationError, nothing of that T_k absorbed;
 *     c = challenge_scalar(b"c").
 * Prover: nonce k_j = draw j of ChaChaRng::from_seed(rng32[row]); T_k = sum_t k[sec] Base; s_j = k_j + c x_j.
 * proof = T_1 | .. | T_E | s_1 | .. | s_S, 32 (E + S) bytes.
 * Verifier, equation k: sum_t s[sec] Base - c slot[lhs_k] - T_k must be the identity.
 * Arguments (the transcript arguments, the shared_transcript / d_transcripts pair of the _dev forms, malformed states, nbatch = 0 and
 * BPGPU_VERDICT_UNDECIDED are those of bpgpu_opening_verify_*):
 *   proof_len    : 32 (E + S); anything else is BPGPU_ERR_INVALID_ARG.
 *   points       : nbatch x P x 32 bytes, slot order.      secrets : creation, nbatch x S x 32 bytes.
 *   rng32        : creation, ONE 32-byte seed per row; NULL: the seeds come from the OS CSPRNG.  A SEED MUST NEVER SERVE TWO DIFFERENT
 *                  STATEMENTS OR TRANSCRIPTS: two proofs with one nonce and different challenges give away the secrets.
 *   status       : creation, nbatch bytes: BPGPU_MSM_OK; BPGPU_MSM_BAD_SCALAR for a secret that is not canonical; BPGPU_MSM_BAD_POINT
 *                  for an instance BASE that does not decode.  Such a row walks like any other, its proof bytes are zero and its
 *                  transcripts_out row is its input state; the other rows are unaffected.
 *   msm_out      : optional nbatch x E x 32 bytes, compress of each equation's check (32 zero bytes where it holds or the row stopped).
 *   weights64    : the combined forms, nbatch x E x 64 bytes (one weight per proof and equation) or NULL: drawn by the library.
 *   nbatch (P + E) may not exceed 2^24 (the combined list): more is BPGPU_ERR_INVALID_ARG in every call of the family.
 * Verdicts and transcripts_out of the verifiers:
 *   an s_j that is not canonical                : FORMAT_ERROR,        the input state
 *   a T_k of 32 zero bytes                      : VERIFICATION_ERROR,  the state as of that message
 *   a point that does not decode, a failing check: VERIFICATION_ERROR, the state after c
 *   a proof that verifies                       : OK,                  the state after c
 * CONTRACTS (tests/test_gpu_sigma.py): (a) msm_out of (row, equation) equals bpgpu_msm_batch on that equation's terms with c from
 * bpgpu_transcript_batch running the script; (b) verdict and transcripts_out of an _rlc_ts call ALWAYS equal those of the
 * _verify_batch_ts call on the same inputs (the host form falls back to the per-proof path where the combination does not decide, the
 * _dev form marks BPGPU_VERDICT_UNDECIDED); (c) a created proof verifies and both sides' transcripts_out are equal.
 * Timing and secrets: creation is three launches (the per-lane variable-base products k P, the table walks with the encodings, the
 * transcripts).  Its walks are variable time unless the context option "prover_constant_time" is set; then the shared bases take the
 * W = 4 mask-select table and the product k P reads all 8 multiples of its point per window, selects by masks and applies the sign by
 * mask -- the nonce is as secret as the witness; the same bytes.  Secrets and seeds are staged in the secret span: staging, the device
 * IO buffer and the working sets are cleared on every exit.  The verifiers are variable time.  The context needs generators.
 * Measured on one MI355X (profiles/sigma_rate.json; host pointers, one state per row, medians; DLEQ / one amount under two
 * value bases): 65 536 rows -- _verify_rlc_ts 4.7 / 5.3 ms, _verify_batch_ts 15.4 / 16.2 ms, creation 5.1 / 6.0 ms, against 19.4 / 21.2 ms
 * (verification) and 16.8 / 18.2 ms (creation) for bpgpu_transcript_batch + bpgpu_msm_batch on the same terms.  4 096 rows -- creation
 * 1.43 / 2.15 ms is 7 % SLOWER than that route (1.34 / 2.01 ms), and at 64 rows 1.8 - 2.6 times slower: small batches are made faster the
 * old way. */
typedef struct bpgpu_sigma_relation bpgpu_sigma_relation;
/* the validation of bpgpu_sigma_relation_create alone, on the host, against gens_capacity generators; digest (optional): the 32 bytes */
int bpgpu_sigma_descriptor_check(const uint8_t *desc, size_t desc_len, size_t gens_capacity, uint8_t digest[32]);
int bpgpu_sigma_relation_create(bpgpu_ctx *ctx, const uint8_t *desc, size_t desc_len, bpgpu_sigma_relation **out);
void bpgpu_sigma_relation_destroy(bpgpu_sigma_relation *rel);
int bpgpu_sigma_relation_shape(const bpgpu_sigma_relation *rel, size_t *S, size_t *P, size_t *E, uint8_t digest[32]);
int bpgpu_sigma_create_batch_ts(bpgpu_ctx *ctx, const bpgpu_sigma_relation *rel, size_t nbatch, const uint8_t *transcripts,
                                size_t transcript_stride, const uint8_t *rng32, const uint8_t *points, const uint8_t *secrets,
                                uint8_t *proofs_out, uint8_t *status, uint8_t *transcripts_out);
int bpgpu_sigma_verify_batch_ts(bpgpu_ctx *ctx, const bpgpu_sigma_relation *rel, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                const uint8_t *transcripts, size_t transcript_stride, const uint8_t *points, uint8_t *verdict,
                                uint8_t *msm_out, uint8_t *transcripts_out);
int bpgpu_sigma_verify_batch_ts_dev(bpgpu_ctx *ctx, const bpgpu_sigma_relation *rel, size_t nbatch, const void *d_proofs,
                                    size_t proof_len, const uint8_t *shared_transcript, const void *d_transcripts, const void *d_points,
                                    void *d_verdict, void *d_msm_out, void *d_transcripts_out, void *stream);
int bpgpu_sigma_verify_rlc_ts(bpgpu_ctx *ctx, const bpgpu_sigma_relation *rel, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                              const uint8_t *transcripts, size_t transcript_stride, const uint8_t *points, const uint8_t *weights64,
                              uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out);
int bpgpu_sigma_verify_rlc_ts_dev(bpgpu_ctx *ctx, const bpgpu_sigma_relation *rel, size_t nbatch, const void *d_proofs, size_t proof_len,
                                  const uint8_t *shared_transcript, const void *d_transcripts, const void *d_points,
                                  const void *d_weights64, void *d_verdict, void *d_batch_out, void *d_transcripts_out, void *stream);

/* ---- the multi-party aggregation protocol: parties and dealer ------------------------------------
 * range_proof_mpc of the reference (src/range_proof/party.rs, dealer.rs, messages.rs; docs/aggregation-api.md) as six
 * batched, STATELESS calls: host pointers in and out, nothing retained after return.  bpgpu_rangeproof_prove_batch above
 * runs parties and dealer in-line for proofs whose secrets all sit in one process and never forms a message; these calls
 * are the protocol itself, for a service that acts as the party for many clients, a dealer that aggregates many sessions,
 * or values held by different owners.  What the reference keeps in its typestate structs travels as caller-held opaque
 * blobs of bpgpu_mpc_state1_bytes(n) / bpgpu_mpc_state2_bytes(n) bytes per party; their layout is private to the library
 * (csrc/mpc_party.h) and they hold the party's SECRETS: the caller zeroes them when done, as the reference zeroizes on
 * Drop (party.rs:148-260).  Messages have the layouts bpgpu_rangeproof_audit_shares reads.
 * Per-row status bytes: */
#define BPGPU_MPC_OK 0
#define BPGPU_MPC_MALICIOUS_DEALER 1 /* MPCError::MaliciousDealer: the poly challenge x is zero (party.rs:283-285) */
#define BPGPU_MPC_MALFORMED_SHARES 2 /* MPCError::MalformedProofShares { bad_shares } (dealer.rs:303-335) */
#define BPGPU_MPC_BAD_SCALAR 3       /* a challenge that is not a canonical scalar (upstream: Scalar by type) */
#define BPGPU_MPC_BAD_POINT 4        /* an A_j, S_j, T_1_j or T_2_j that does not decode (upstream: RistrettoPoint by type) */
/* Parameter errors are return codes: BPGPU_ERR_INVALID_ARG for InvalidBitsize (n not 8, 16, 32, 64), InvalidAggregation (m
 * not a power of two), n m beyond the prover's limit or a blob that is no state of the step; BPGPU_ERR_NO_GENS for
 * InvalidGeneratorsLength (n > gens_capacity, a position or m beyond party_capacity).
 *
 * PARTY SIDE.  Rows are independent parties of one bitsize n, each at its own position j: rows of many sessions with
 * different m share a call.  Every commitment is a multiscalar multiplication over B~, B and PARTY j's share G_j(n), H_j(n)
 * of the generator tables: 2n + 2 terms whatever j and party_capacity are; rows are grouped by position inside the call so
 * that a wavefront walks one sub-table (csrc/mpc_party.h) and results come back in the caller's order.  Timing: as
 * bpgpu_rangeproof_prove_batch -- variable time by default; with the context option "prover_constant_time" = 1 exactly
 * V_j, A_j, S_j, T_1_j, T_2_j (party.rs:99-124, 224-227, the reference's constant-time multiscalar_mul) take the
 * constant-time walk, byte-identical outputs.  Every call clears what it staged (prover_exit, see above).
 *
 * bpgpu_mpc_party_bit_commit: Party::new + PartyAwaitingPosition::assign_position_with_rng (party.rs:37-144).
 *   party_index : nparties x uint32, the position j of each row (j >= party_capacity: BPGPU_ERR_NO_GENS)
 *   values      : nparties x u64.  A value that does not fit n bits is ACCEPTED, as Party::new accepts it (only bits
 *                 0..n are committed): the reference's dishonest-party scenario (mod.rs:726-799) and the dealer's check
 *                 depend on that -- unlike bpgpu_rangeproof_prove_batch, which refuses such a value
 *   blindings   : nparties x 32 bytes (Scalars, reduced mod l)
 *   rng         : nparties x 64 (2n + 2) bytes in draw order a_blinding, s_blinding, s_L[0..n), s_R[0..n); NULL = OS CSPRNG
 *   bit_commitments : nparties x 96 bytes: V_j, A_j, S_j (BitCommitment);  state1 : nparties x bpgpu_mpc_state1_bytes(n) */
size_t bpgpu_mpc_state1_bytes(size_t n);
size_t bpgpu_mpc_state2_bytes(size_t n);
int bpgpu_mpc_party_bit_commit(bpgpu_ctx *ctx, size_t n, size_t nparties, const uint32_t *party_index, const uint64_t *values,
                               const uint8_t *blindings, const uint8_t *rng, uint8_t *bit_commitments, uint8_t *state1);
/* PartyAwaitingBitChallenge::apply_challenge_with_rng (party.rs:182-237).
 *   bit_challenges : nparties x 64 bytes (y, z per row), or 64 bytes when challenges_shared != 0 (BitChallenge)
 *   rng         : nparties x 128 bytes: t_1_blinding, t_2_blinding; NULL = OS CSPRNG
 *   poly_commitments : nparties x 64 bytes: T_1_j, T_2_j (PolyCommitment);  state2 : nparties x bpgpu_mpc_state2_bytes(n)
 *   status      : nparties bytes; a non-canonical y or z is BPGPU_MPC_BAD_SCALAR for that row (its outputs are zero) */
int bpgpu_mpc_party_poly_commit(bpgpu_ctx *ctx, size_t n, size_t nparties, const uint8_t *state1, const uint8_t *bit_challenges,
                                int challenges_shared, const uint8_t *rng, uint8_t *poly_commitments, uint8_t *state2,
                                uint8_t *status);
/* The SEEDED forms of the two steps that draw: "this party's rng is ChaChaRng::from_seed(s)", as bpgpu_rangeproof_prove_batch_ts
 * speaks of a proof's.  Every random scalar is a ChaCha20 block computed by the lane that consumes it: 32 + 8 bytes per party
 * cross the staging block in place of 64 (2n + 2) (or 128), and no buffer of draws exists on the host or the device.
 *   rng32       : nparties x 32 bytes; row p's rng is rand_chacha's ChaChaRng::from_seed(rng32[p]) -- ChaCha20 with a 64-bit
 *                 block counter and stream id 0 (see bpgpu_rangeproof_prove_batch_ts); draw d is
 *                 Scalar::from_bytes_mod_order_wide(keystream block d).  NULL: 32 bytes per row from the OS-seeded CSPRNG
 *   first_draw  : nparties x uint64, the block index of the row's first draw in this step: how far the client's rng has
 *                 advanced.  Bit commit consumes first_draw + 0: a_blinding, + 1: s_blinding, + 2 + i: s_L[i],
 *                 + 2 + n + i: s_R[i] (party.rs:87-118); poly commit first_draw + 0: t_1_blinding, + 1: t_2_blinding
 *                 (party.rs:224-227).  NULL: 0 for every row in bit commit, 2n + 2 in poly commit (one ChaChaRng carried
 *                 through both steps).  A party at position j of an m-party prove_multiple_with_rng sits at j (2n + 2) in
 *                 bit commit and at m (2n + 2) + 2j in poly commit.  A first_draw whose draws would run the counter past
 *                 2^64 - 1 (first_draw > 2^64 - (2n + 2) in bit commit, > 2^64 - 2 in poly commit): BPGPU_ERR_INVALID_ARG
 * CONTRACT: every output of every row equals what the unseeded call writes when its rng holds keystream blocks first_draw ...
 * of rng32[p]; state blobs keep their layout and size, so seeded and unseeded steps interoperate.  Parameter errors, per-row
 * status, "prover_constant_time" (byte-identical outputs) and the clearing of what was staged -- the seeds are in the secret
 * part of the staging block -- are those of the unseeded calls. */
int bpgpu_mpc_party_bit_commit_seeded(bpgpu_ctx *ctx, size_t n, size_t nparties, const uint32_t *party_index,
                                      const uint64_t *values, const uint8_t *blindings, const uint8_t *rng32,
                                      const uint64_t *first_draw, uint8_t *bit_commitments, uint8_t *state1);
int bpgpu_mpc_party_poly_commit_seeded(bpgpu_ctx *ctx, size_t n, size_t nparties, const uint8_t *state1,
                                       const uint8_t *bit_challenges, int challenges_shared, const uint8_t *rng32,
                                       const uint64_t *first_draw, uint8_t *poly_commitments, uint8_t *state2,
                                       uint8_t *status);
/* PartyAwaitingPolyChallenge::apply_challenge (party.rs:279-311).
 *   poly_challenges : nparties x 32 bytes (x per row), or 32 bytes when challenges_shared != 0 (PolyChallenge)
 *   shares      : nparties x 32 (3 + 2n) bytes: t_x, t_x_blinding, e_blinding, l_vec[n], r_vec[n] (ProofShare)
 *   status      : x == 0 is BPGPU_MPC_MALICIOUS_DEALER, a non-canonical x BPGPU_MPC_BAD_SCALAR; that row's share is zero */
int bpgpu_mpc_party_proof_share(bpgpu_ctx *ctx, size_t n, size_t nparties, const uint8_t *state2, const uint8_t *poly_challenges,
                                int challenges_shared, uint8_t *shares, uint8_t *status);
/* DEALER SIDE.  Rows are sessions of one shape (n, m); the messages of a session are its m parties' in position order.  The
 * dealer's state is its transcript (one 208-byte state per session, carried by the caller) and the messages it has seen.
 *
 * bpgpu_mpc_dealer_bit_challenge: Dealer::new + DealerAwaitingBitCommitments::receive_bit_commitments (dealer.rs:37-137):
 * rangeproof_domain_sep(n, m), every V_j appended AS GIVEN, A = sum A_j and S = sum S_j (decoded, added and compressed by
 * a kernel of their own), appended; y and z drawn.
 *   transcript  : transcripts == NULL: Transcript::new(label);  transcript_stride == 0: ONE 208-byte state shared by the
 *                 sessions;  == BPGPU_TRANSCRIPT_BYTES: one state per session.  This is the INITIAL transcript (what
 *                 Dealer::new clones for its final check): keep it for bpgpu_mpc_dealer_assemble
 *   bit_challenges : nsessions x 64 bytes: y, z;  sums_out (optional) : nsessions x 64 bytes: compress(A), compress(S)
 *   transcripts_out : nsessions x 208 bytes, the advanced transcripts
 *   status      : an A_j or S_j that does not decode is BPGPU_MPC_BAD_POINT for that session (outputs zero, transcript
 *                 as it came) */
int bpgpu_mpc_dealer_bit_challenge(bpgpu_ctx *ctx, size_t n, size_t m, size_t nsessions, const uint8_t *bit_commitments,
                                   const uint8_t *label, size_t label_len, const uint8_t *transcripts, size_t transcript_stride,
                                   uint8_t *bit_challenges, uint8_t *sums_out, uint8_t *transcripts_out, uint8_t *status);
/* DealerAwaitingPolyCommitments::receive_poly_commitments (dealer.rs:160-197): T_1 = sum T_1_j, T_2 = sum T_2_j appended, x drawn.
 *   transcripts : nsessions x 208 bytes, advanced in place;  poly_challenges : nsessions x 32 bytes: x
 *   sums_out (optional) : nsessions x 64 bytes: compress(T_1), compress(T_2) */
int bpgpu_mpc_dealer_poly_challenge(bpgpu_ctx *ctx, size_t m, size_t nsessions, const uint8_t *poly_commitments, uint8_t *transcripts,
                                    uint8_t *poly_challenges, uint8_t *sums_out, uint8_t *status);
/* DealerAwaitingProofShares::assemble_shares with receive_shares_with_rng (trusted == 0) or receive_trusted_shares
 * (trusted != 0) (dealer.rs:226-380): t_x, t_x_blinding, e_blinding summed and appended, w drawn, Q = w B, l_vec || r_vec in
 * party order, H_factors y^-i, the inner-product argument over G(n, m), H(n, m) (bpgpu_ipp_create_batch's rounds; variable
 * time, as upstream), the proof in RangeProof::to_bytes order.  Unless trusted, every assembled proof is verified with the
 * batched verifier on the INITIAL transcript and rng64, and the shares of the sessions that fail go through
 * bpgpu_rangeproof_audit_shares.
 *   challenges  : nsessions x 96 bytes: y, z, x;  transcripts : nsessions x 208 bytes as bpgpu_mpc_dealer_poly_challenge
 *                 left them, advanced in place to where the reference's dealer leaves its transcript
 *   initial_*   : the transcript convention of bpgpu_mpc_dealer_bit_challenge;  rng64 : nsessions x 64 bytes or NULL
 *   proofs_out  : nsessions x 32 (9 + 2 lg(n m)) bytes;  bad_shares : nsessions x m bytes, 1 = that party is named
 *   status      : BPGPU_MPC_MALFORMED_SHARES: the proof did not verify, or (also when trusted) a share scalar is not
 *                 canonical; proof bytes zero, bad_shares names the parties.  Other sessions of the call are unaffected. */
int bpgpu_mpc_dealer_assemble(bpgpu_ctx *ctx, size_t n, size_t m, size_t nsessions, const uint8_t *shares, const uint8_t *bit_commitments,
                              const uint8_t *poly_commitments, const uint8_t *challenges, uint8_t *transcripts,
                              const uint8_t *initial_label, size_t initial_label_len, const uint8_t *initial_transcripts,
                              size_t initial_stride, const uint8_t *rng64, int trusted, uint8_t *proofs_out, uint8_t *bad_shares,
                              uint8_t *status);

/* InnerProductProof::from_bytes + InnerProductProof::verification_scalars (src/inner_product_proof.rs:198-253, 373-407) for
 * nbatch proofs: what the R1CS verifier calls (src/r1cs/verifier.rs:401-404) before it builds ITS multiscalar multiplication
 * (r1cs/verifier.rs:459-491, served by bpgpu_msm_batch_shared), and what InnerProductProof::verify uses at ipp.rs:283.
 *   proofs      : nbatch x proof_len bytes, InnerProductProof::to_bytes (L_0 R_0 .. L_{k-1} R_{k-1} a b)
 *   transcript  : transcripts == NULL: Transcript::new(label);  transcript_stride == 0: ONE 208-byte state shared by the
 *                 batch;  == BPGPU_TRANSCRIPT_BYTES: one state per proof.  innerproduct_domain_sep(n) is applied by the call.
 *   u_sq, u_inv_sq : nbatch x k x 32 bytes (k = lg n): u_i^2 and u_i^-2 in creation order;  s : nbatch x n x 32 bytes
 *   transcripts_out (optional) : the advanced states of the proofs with status 0 (others: unspecified)
 *   status      : nbatch bytes: 0, BPGPU_VERDICT_VERIFICATION_ERROR (n != 2^k, or an identity L_i / R_i:
 *                 validate_and_append_point), BPGPU_VERDICT_FORMAT_ERROR (malformed length, a / b not canonical); the outputs
 *                 of a rejected proof are zero */
int bpgpu_ipp_verification_scalars(bpgpu_ctx *ctx, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                   const uint8_t *label, size_t label_len, const uint8_t *transcripts, size_t transcript_stride,
                                   uint8_t *u_sq, uint8_t *u_inv_sq, uint8_t *s, uint8_t *transcripts_out, uint8_t *status);

/* ---- pool: the scheduler (any number of proofs per call, any number of devices) ------------
 * The reference's call shape is ONE call for as many proofs as the caller has: a loop over
 * RangeProof::verify_multiple (src/range_proof/mod.rs:457-470), from one thread or many.  A bpgpu_ctx is one launch
 * chain on one stream and cannot fill a device by itself; a pool owns `lanes_per_device` contexts on each of `ndev`
 * devices (the generator tables are built once per device and shared by its lanes) and does the scheduling that the
 * benchmark used to do by hand:
 *   - bpgpu_pool_rangeproof_verify / bpgpu_pool_rangeproof_verify_ts (HOST pointers, blocking, any nbatch, ANY NUMBER OF THREADS AT
 *     ONCE): the requests go through the pool's combining queue (declared below): calls that arrive close together share launch
 *     chains, a large call spans several chains and -- proofs being independent units -- takes the contiguous shard
 *     [nbatch d / ndev, nbatch (d+1) / ndev) of every device; every piece's verdicts land at its offset of the caller's buffer: the
 *     "final gather" of SURVEY 8e is that host-side placement, no collective is involved.  Verdicts are exactly those of
 *     bpgpu_rangeproof_verify_batch[_ts] on the whole batch.  (Option "host_path_combining" = 0 restores round 3's path for the label
 *     form: one call at a time, slices staged by "host_workers" threads per device.)
 *   - bpgpu_pool_rangeproof_submit_dev (DEVICE pointers on device `dev_index` of the pool, asynchronous): the batch is
 *     queued; bpgpu_pool_flush -- or the pool itself once "auto_flush_items" batches wait (default: one per lane) --
 *     packs consecutive queued batches of one shape (n, m, proof_len, label) into coalesced launch chains of about
 *     "coalesce_proofs" proofs (default 5120) and issues them on the lanes round-robin.  A burst of small batches is
 *     thereby served as a few wide chains instead of many narrow ones (20 x 1024 proofs from an idle device: 4.1 M
 *     verifications/s as twenty chains, 5.9 - 6.2 M as two); every batch still gets its own verdict (and msm_out) buffer filled.
 *     Input buffers must be complete on the device when the batch is submitted and stay valid until bpgpu_pool_wait returns (the
 *     pool's streams are not ordered against the caller's) -- or use bpgpu_pool_rangeproof_submit_dev_ex below: a producer stream
 *     the chain waits for, and a ticket per batch.  Batches whose length or parameters are malformed are passed to
 *     bpgpu_rangeproof_verify_batch_dev unchanged, which reports them per proof.  When a chain cannot be issued, the verdict bytes
 *     of the batches it carried are set to BPGPU_VERDICT_UNDECIDED (never left at 0 = "verified") and the flush reports the error.
 * devices: HIP ordinals, one entry per shard (an ordinal may repeat: two shards on one GPU -- what the one-GPU tests
 * do).  lanes_per_device: 0 = 32 (plus the combining queue's own lanes: environment BPGPU_COMBINE_LANES, default 12).  More than 4
 * lanes need 8..16 hardware queues: export GPU_MAX_HW_QUEUES=16 before the process's FIRST HIP call (the ROCm runtime reads it
 * then).  libbpgpu sets the variable when it is loaded if it is unset -- which only helps when nothing initialised HIP earlier;
 * bpgpu_pool_create therefore returns BPGPU_ERR_HW_QUEUES when it finds another value, and, when the value is the library's own,
 * after timing sixteen single-wavefront kernels that spin 1 ms each on sixteen streams (~3 ms in all, best of three) and finding fewer than 6 of them overlapping.
 * bpgpu_pool_last_error is per calling thread: what the last pool call OF THAT THREAD reported.
 * Options (bpgpu_pool_set_option; one line each, every one of them is flipped by a test -- tests/test_abi_and_host.py::
 * test_every_pool_option_is_documented_and_settable, tests/cpu_pool):
 *   "coalesce_proofs"      5120   target width of a coalesced launch chain
 *   "max_chain_proofs"     16384  no chain wider than this (a lane's arena: ~55 KB per proof)
 *   "pair_limit_proofs"    24576  a flush of up to this many proofs is issued as at most two chains
 *   "latency_proofs"       6144   a host call, or a flush on an idle device, of up to this many proofs is alone: its chains take the latency forms
 *   "auto_flush_items"     0      flush by itself once this many items wait on a device (0 = the number of lanes)
 *   "auto_flush_proofs"    0      ... or once this many proofs wait (0 = off)
 *   "slice_proofs"         0      host-pointer calls of the round-3 host path: proofs per slice (0 = automatic)
 *   "host_workers"         0      ... and its worker threads (set before the first host-pointer call)
 *   "host_path_combining"  1      bpgpu_pool_rangeproof_verify through the combining queue (0 = the round-3 slicing workers)
 *   "rlc_isolate"          0      1 = a chain carries at most one batch-combined batch: a bad proof leaves only its own batch undecided
 *   "combine_wait_us"      100    a staging buffer leaves at the latest this long after its first request arrived ...
 *   "combine_quiet_us"     20     ... or when nothing has joined it for this long
 *   "combine_max_age_us"   1500   ... and no request waits longer than this for its chain to be issued
 *   "combine_inflight"     4      deadlines seal buffers only while fewer chains than this run: beyond, load widens the chains
 *   "combine_busy_chains"  2      a chain issued beside this many others takes the throughput forms
 *   "combine_max_open"     4      transcript-position classes with a staging buffer of their own
 *   "combine_mapped_out"   1024   chains up to this wide write their results straight into pinned host memory
 *   "combine_msm_bytes"    32 MiB staging block of a multiscalar-multiplication class: MSMs per chain = this / bytes per MSM
 *   "combine_trace"        0      ring size of the timeline records (bpgpu_pool_trace_dump)
 *   "stat_reset"           -      zero all statistics
 * Any other key is forwarded to every lane context (set those before bpgpu_pool_gens_*).  When a staging buffer leaves is decided per
 * kind of work, as measured (profiles/r05/combine_policy_ab.txt): range proofs by the deadlines above in two regimes, multiscalar multiplications and inner-product
 * proofs in cohorts (a buffer leaves when the group the last chain released is back); the constants of both policies are not options.
 * Removed in round 6 because their own A/B refuted them (the tables stay under profiles/r05/): "plan_by_work", "plan_min_chain_proofs",
 * "stagger_chains", "combine_policy", "combine_mapped_in"; context keys "split_stage1", "fork_early".
 * Read-only statistics (bpgpu_pool_get_option): "stat_chains", "stat_chain_proofs" (launch chains issued by flushes and the proofs they
 * carried), "stat_last_splits", "stat_combined_chains" / "_proofs" / "_requests", "stat_svc_issue_us" / "_complete_us" / "_polls" /
 * "_deliver_us" (the combining queue's service threads), "stat_active_calls", "combine_lanes". */
typedef struct bpgpu_pool bpgpu_pool;
int bpgpu_pool_create(const int *devices, int ndev, int lanes_per_device, bpgpu_pool **out);
void bpgpu_pool_destroy(bpgpu_pool *pool);
const char *bpgpu_pool_last_error(bpgpu_pool *pool);
int bpgpu_pool_set_option(bpgpu_pool *pool, const char *key, int64_t value);
int bpgpu_pool_get_option(bpgpu_pool *pool, const char *key, int64_t *value);
int bpgpu_pool_devices(bpgpu_pool *pool);
int bpgpu_pool_lanes(bpgpu_pool *pool);
/* lane `lane` of shard `dev_index` (for bpgpu_profile_*, bpgpu_ctx_get_option); owned by the pool */
bpgpu_ctx *bpgpu_pool_lane(bpgpu_pool *pool, int dev_index, int lane);
/* BulletproofGens::new / PedersenGens::default (or the caller's encodings) on every device of the pool */
int bpgpu_pool_gens_create(bpgpu_pool *pool, size_t gens_capacity, size_t party_capacity);
int bpgpu_pool_gens_load(bpgpu_pool *pool, size_t gens_capacity, size_t party_capacity, const uint8_t *G, const uint8_t *H,
                         const uint8_t B[32], const uint8_t B_blinding[32]);
/* bpgpu_gens_add_shape on every lane of every device (call it while the pool is idle) */
int bpgpu_pool_gens_add_shape(bpgpu_pool *pool, size_t n2, size_t m2);
/* arguments as bpgpu_rangeproof_verify_batch */
int bpgpu_pool_rangeproof_verify(bpgpu_pool *pool, size_t n, size_t m, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                 const uint8_t *commitments, const uint8_t *label, size_t label_len, const uint8_t *rng64,
                                 uint8_t *verdict, uint8_t *msm_out);
/* arguments as bpgpu_rangeproof_verify_batch_dev, without the stream */
int bpgpu_pool_rangeproof_submit_dev(bpgpu_pool *pool, int dev_index, size_t n, size_t m, size_t nbatch, const void *d_proofs,
                                     size_t proof_len, const void *d_commitments, const uint8_t *label, size_t label_len,
                                     const void *d_rng64, void *d_verdict, void *d_msm_out);
/* RangeProof::verify_multiple_with_rng in the reference's own call shape (src/range_proof/mod.rs:345-353, 455-470): a FEW proofs
 * per call -- one is fine --, each with its own `transcript: &mut Transcript`, BLOCKING, from ANY number of threads at once.
 * Calls that arrive close together share a launch chain (the pool's combining queue: one staging buffer per class of requests
 * -- shape and STROBE position of the transcripts --, which leaves as one chain when it is full ("coalesce_proofs"), when its
 * first proof has waited "combine_wait_us" (default 100) or when nothing joined it for "combine_quiet_us" (default 20); every
 * caller is woken when ITS proofs are done, not when the pool drains).  Arguments as bpgpu_rangeproof_verify_batch_ts:
 *   transcripts / transcript_stride : BPGPU_TRANSCRIPT_BYTES: one 208-byte state per proof (may have absorbed application data:
 *                 the normal use of Merlin); 0: ONE state shared by the nbatch proofs (e.g. bpgpu_transcript_new(label))
 *   transcripts_out (optional, nbatch x 208; may alias `transcripts` when the stride is 208): the advanced states, as
 *                 bpgpu_rangeproof_verify_batch_ts leaves them (a FormatError proof's state is handed back untouched)
 *   rng64 (optional): 64 bytes per proof for the batching challenge; NULL: drawn per calling thread from a ChaCha20 generator
 *                 keyed by the OS (the thread_rng() of verify_multiple)
 * Verdicts, encodings and states are bit-identical to bpgpu_rangeproof_verify_batch_ts on the same inputs.  Requests of any
 * size are accepted (a large one spans several chains and, on a multi-device pool, takes a contiguous shard per device).
 * bpgpu_pool_rangeproof_verify (label instead of transcripts) is the same call with Transcript::new(label) for every proof.
 * On a non-zero return no verdict byte of the call reads 0: proofs whose chain failed carry BPGPU_VERDICT_UNDECIDED.
 *
 * bpgpu_pool_rangeproof_submit_ts: the non-blocking form.  Returns once the inputs have been copied (they may be reused at
 * once); verdict / msm_out / transcripts_out must stay valid until bpgpu_pool_ticket_wait(ticket) has returned -- it blocks
 * until THIS request is complete (not the pool), returns the request's error code and frees the ticket; every ticket must be
 * waited for exactly once.  bpgpu_pool_ticket_done: 1 when wait would not block.  One thread can thereby keep thousands of
 * single-proof requests in flight. */
typedef struct bpgpu_ticket bpgpu_ticket;
int bpgpu_pool_rangeproof_verify_ts(bpgpu_pool *pool, size_t n, size_t m, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                    const uint8_t *commitments, const uint8_t *transcripts, size_t transcript_stride,
                                    const uint8_t *rng64, uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out);
int bpgpu_pool_rangeproof_submit_ts(bpgpu_pool *pool, size_t n, size_t m, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                    const uint8_t *commitments, const uint8_t *transcripts, size_t transcript_stride,
                                    const uint8_t *rng64, uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out,
                                    bpgpu_ticket **ticket);
int bpgpu_pool_ticket_done(bpgpu_pool *pool, bpgpu_ticket *ticket);
int bpgpu_pool_ticket_wait(bpgpu_pool *pool, bpgpu_ticket *ticket);
/* ---- the boundary function itself through the pool: one multiscalar multiplication (or a few) per call, from any thread ------------
 * SURVEY 8b's drop-in point is RistrettoPoint::optional_multiscalar_mul / vartime_multiscalar_mul as the crate calls it: ONE
 * multiscalar multiplication per call (src/range_proof/mod.rs:421-445, src/r1cs/verifier.rs:459-491, src/inner_product_proof.rs:308-319,
 * src/linear_proof.rs:217-225, src/range_proof/messages.rs:128-149), from whatever thread verifies.  One such call cannot fill a device
 * (bpgpu_msm_batch_shared on a context of its own: 0.77 ms per 6 179-term MSM, and threads do not add up beyond one context each), so
 * these go through the same combining queue as the range proofs: calls that arrive close together share a launch chain, every caller
 * is woken when ITS results are there.  BLOCKING, ANY NUMBER OF THREADS AT ONCE; results bit-identical to the bpgpu_msm_batch* /
 * bpgpu_ipp_verify_batch call on a context.
 *   bpgpu_pool_msm_batch_shared : arguments as bpgpu_msm_batch_shared (the mega-check shape: 2nm+2 generator scalars in the order of
 *                                 mod.rs:421-443 + n_unique (scalar, point) pairs per MSM); MSMs of one (n, m, n_unique) share chains
 *   bpgpu_pool_msm_batch_shared_submit : the non-blocking form; out / status must stay valid until bpgpu_pool_ticket_wait(ticket)
 *   bpgpu_pool_msm_batch        : arguments as bpgpu_msm_batch (ragged batch); MSMs of equal length share chains, so a call is placed
 *                                 stretch by stretch of equal n_terms; an MSM of 0 terms is the identity (encoding 0, status 0)
 *   bpgpu_pool_ipp_verify       : arguments as bpgpu_ipp_verify_batch (InnerProductProof::verify, ipp.rs:260-326); proofs of one
 *                                 (n, proof_len, label) share chains
 *   bpgpu_pool_msm_batch_shared_submit_dev : the same call for inputs that are already in HBM (device pointers, arguments as
 *                                 bpgpu_msm_batch_shared_dev): the batch leaves at once as ONE chain on the next lane of pool device
 *                                 `dev_index`, behind `producer_stream` if have_producer; ticket (optional) as for
 *                                 bpgpu_pool_rangeproof_submit_dev_ex; nothing is combined -- device-resident batches are as wide as
 *                                 their owner made them.  The pool's lanes are the (context, stream) pairs a caller would otherwise
 *                                 manage by hand.
 * On a non-zero return no status / verdict byte of the call reads 0: items whose chain failed carry BPGPU_VERDICT_UNDECIDED.
 * Option "combine_msm_bytes" (default 32 MiB): staging block per chain of a multiscalar-multiplication class -- items per chain =
 * that / input bytes per MSM (cfg5's shape, 263 KB per MSM: 127 per chain). */
int bpgpu_pool_msm_batch_shared(bpgpu_pool *pool, size_t n, size_t m, size_t nbatch, size_t n_unique, const uint8_t *gen_scalars,
                                const uint8_t *uniq_scalars, const uint8_t *uniq_points, uint8_t *out, uint8_t *status);
int bpgpu_pool_msm_batch_shared_submit(bpgpu_pool *pool, size_t n, size_t m, size_t nbatch, size_t n_unique, const uint8_t *gen_scalars,
                                       const uint8_t *uniq_scalars, const uint8_t *uniq_points, uint8_t *out, uint8_t *status,
                                       bpgpu_ticket **ticket);
int bpgpu_pool_msm_batch(bpgpu_pool *pool, size_t nbatch, const uint32_t *n_terms, const uint8_t *scalars, const uint8_t *points,
                         uint8_t *out, uint8_t *status);
int bpgpu_pool_msm_batch_shared_submit_dev(bpgpu_pool *pool, int dev_index, size_t n, size_t m, size_t nbatch, size_t n_unique,
                                           const void *d_gen_scalars, const void *d_uniq_scalars, const void *d_uniq_points, void *d_out,
                                           void *d_status, void *producer_stream, int have_producer, bpgpu_ticket **ticket);
int bpgpu_pool_ipp_verify(bpgpu_pool *pool, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *label,
                          size_t label_len, const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *P, const uint8_t *Q,
                          const uint8_t *G, const uint8_t *H, uint8_t *verdict, uint8_t *msm_out);
/* R1CS proofs through the pool (arguments as bpgpu_r1cs_verify_batch_ts): the whole call runs on the next device, blocking;
 * any thread may call it, with any circuit. */
int bpgpu_pool_r1cs_verify_ts(bpgpu_pool *pool, const bpgpu_r1cs_circuit *circuit, size_t nbatch, const uint8_t *proofs,
                              size_t proof_stride, const uint32_t *proof_lens, const uint8_t *commitments,
                              const uint8_t *transcripts, size_t transcript_stride, const uint8_t *rng32,
                              uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out);
/* bpgpu_r1cs_verify_rlc through the pool (same arguments): the whole call runs on the next device, blocking; any thread may call it. */
int bpgpu_pool_r1cs_verify_rlc(bpgpu_pool *pool, size_t ngroups, const bpgpu_r1cs_circuit *const *circuits, const size_t *nbatch,
                               const uint8_t *const *proofs, const size_t *proof_stride, const uint32_t *const *proof_lens,
                               const uint8_t *const *commitments, const uint8_t *const *transcripts, const size_t *transcript_stride,
                               const uint8_t *rng32, const uint8_t *weights64,
                               uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out);
/* bpgpu_rangeproof_verify_rlc_mixed through the pool (same arguments): the whole call runs on the next device, blocking; any thread
 * may call it. */
int bpgpu_pool_rangeproof_verify_rlc_mixed(bpgpu_pool *pool, size_t ngroups, const size_t *n, const size_t *m, const size_t *nbatch,
                                           const size_t *proof_len, const uint8_t *proofs, const uint8_t *commitments,
                                           const uint8_t *const *labels, const size_t *label_lens, const uint8_t *rng64,
                                           const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out);
/* bpgpu_rangeproof_verify_rlc_mixed_ts through the pool (same arguments; the callers' transcripts of mod.rs:345-353): the whole call runs
 * on the next device, blocking; any thread may call it. */
int bpgpu_pool_rangeproof_verify_rlc_mixed_ts(bpgpu_pool *pool, size_t ngroups, const size_t *n, const size_t *m, const size_t *nbatch,
                                              const size_t *proof_len, const uint8_t *proofs, const uint8_t *commitments,
                                              const uint8_t *transcripts, const size_t *transcript_stride, const uint8_t *rng64,
                                              const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out);
/* The combining queue's timeline (set option "combine_trace" = ring size first): one JSON object per line -- every launch chain (opened,
 * sealed, issue begin / end, completion seen, delivery begin / end, buffer free; CLOCK_MONOTONIC ns) and every eighth request per thread
 * (submitted, slots reserved, inputs written, delivered, woken).  tools/combine_timeline.py turns it into "where does a request wait". */
int bpgpu_pool_trace_dump(bpgpu_pool *pool, const char *path);
/* bpgpu_pool_rangeproof_submit_dev with a completion contract (a service that consumes batch k while batch k+1 is queued, with no
 * device-wide synchronisation anywhere):
 *   producer_stream / have_producer : have_producer != 0: the batch's input buffers are complete when the work queued so far on
 *                 `producer_stream` (a hipStream_t; NULL = the legacy default stream) is -- the chain that carries the batch waits
 *                 for exactly that point on the device (an event recorded there now); 0: complete at submission, as before
 *   ticket (optional): handle of THIS batch.  bpgpu_pool_ticket_stream_wait(pool, ticket, consumer_stream) makes a consumer stream
 *                 wait, on the device, until the batch's verdicts (and encodings) are written -- it issues the pending chains of
 *                 that device first if they have not left; bpgpu_pool_ticket_wait blocks the host until then, returns the
 *                 batch's error code and frees the ticket (required exactly once per ticket); bpgpu_pool_ticket_done polls.
 * On an error of the chain that carried (part of) the batch its verdict bytes read BPGPU_VERDICT_UNDECIDED, never 0. */
int bpgpu_pool_rangeproof_submit_dev_ex(bpgpu_pool *pool, int dev_index, size_t n, size_t m, size_t nbatch, const void *d_proofs,
                                        size_t proof_len, const void *d_commitments, const uint8_t *label, size_t label_len,
                                        const void *d_rng64, void *d_verdict, void *d_msm_out, void *producer_stream,
                                        int have_producer, bpgpu_ticket **ticket);
int bpgpu_pool_ticket_stream_wait(bpgpu_pool *pool, bpgpu_ticket *ticket, void *consumer_stream);
/* bpgpu_rangeproof_verify_rlc_dev through the pool (SURVEY 8f-3's ADDITIONAL batch-combined check, no counterpart in the crate): consecutive
 * submitted batches of one shape are combined by ONE identity check per launch chain (~coalesce_proofs proofs: from 32 768 per-proof terms
 * the bucket MSM) instead of one per batch -- a service with batches of 1 024 gets the rate of batches of 5 120.  Weights: drawn by the
 * library per chain (OS CSPRNG).  d_verdict: per proof 0 / the front end's status / BPGPU_VERDICT_UNDECIDED when the CHAIN's combination is
 * not the identity -- some proof of some batch of that chain fails; which one is for the caller to find by resubmitting the undecided
 * batches through bpgpu_pool_rangeproof_submit_dev[_ex].  d_batch_out (optional, 33 bytes, 4-byte aligned): the verdict byte and the
 * combined point of the chain that carried the batch.  producer_stream / have_producer / ticket as bpgpu_pool_rangeproof_submit_dev_ex. */
int bpgpu_pool_rangeproof_submit_rlc_dev(bpgpu_pool *pool, int dev_index, size_t n, size_t m, size_t nbatch, const void *d_proofs,
                                         size_t proof_len, const void *d_commitments, const uint8_t *label, size_t label_len,
                                         const void *d_rng64, void *d_verdict, void *d_batch_out, void *producer_stream,
                                         int have_producer, bpgpu_ticket **ticket);
/* The final gather for callers that keep verdicts on the devices (north star: "... only for the final identity-check gather"): the
 * verdict bytes of every shard -- part[d]: device memory on pool device d, bytes[d] bytes -- to ONE buffer d_dst on pool device `root`,
 * shard after shard, by peer copies (xGMI between the GPUs of a node), ordered on the device behind everything the pool has issued on the
 * source device so far (flush first).  Asynchronous on `stream` (hipStream_t of the root device, NULL = default stream).  Nothing else of
 * a verification ever crosses devices: proofs are independent units (src/range_proof/mod.rs:455-470 verifies them one by one). */
int bpgpu_pool_gather_dev(bpgpu_pool *pool, int root, const void *const *part, const size_t *bytes, void *d_dst, void *stream);
int bpgpu_pool_flush(bpgpu_pool *pool);   /* issue everything queued; returns without waiting */
int bpgpu_pool_wait(bpgpu_pool *pool);    /* flush, then wait until every lane is idle */

/* ---- instrumentation -----------------------------------------------------------
 * When enabled, every kernel launch is bracketed by HIP events on its stream;
 * bpgpu_profile_report writes one line per kernel: "name launches total_ms". */
int bpgpu_profile_enable(bpgpu_ctx *ctx, int on);
int bpgpu_profile_reset(bpgpu_ctx *ctx);
int bpgpu_profile_report(bpgpu_ctx *ctx, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
