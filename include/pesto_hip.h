/* pesto_hip.h - C ABI of libpesto_hip.so: PeSTo's geometric-transformer forward pass on MI355X (gfx950).
 *
 * The reference has NO native/FFI layer: its operator API for this path is the torch Module
 *     Model(config_model).load_state_dict(...); z = model(X, ids_topk, q0, M)
 * (reference model/model.py:7-52; call sites apply_model.ipynb:87-93,155, profiling.py:24-28,102,
 * interfaceome/apply_model.py:33-34,73).  Each entry point below names the reference interface it
 * replaces.  Plain pointers and sizes only; no torch types.  All functions return 0 on success and a
 * negative pesto_status on failure; pesto_last_error() gives the thread-local message.
 *
 * Conventions (identical to the reference tensors):
 *   X          float32 [N,3]        atom coordinates of the collated batch
 *   ids_topk   int64 or int32 [N,k] 1-based neighbour ids into the sink-augmented arrays, 0 = sink /
 *                                   padding, columns in ascending distance (k <= 64)
 *   q0         float32 [N,n0]       input features (one-hot in practice, any values accepted)
 *   res_of_atom int32 [N]           residue (column of the reference's mask M) each atom belongs to;
 *                                   the host layer derives it from M (exactly one 1 per row)
 *   z          float32 [R,n_out]    logits per residue
 */
#ifndef PESTO_HIP_H
#define PESTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PESTO_MAX_LAYERS 64
#define PESTO_MAX_K 64

typedef enum pesto_status {
    PESTO_OK = 0,
    PESTO_ERR_INVALID = -1,   /* bad argument / config / blob size */
    PESTO_ERR_HIP = -2,       /* a HIP runtime call failed */
    PESTO_ERR_NOMEM = -3,
    PESTO_ERR_STATE = -4,     /* debug entry point called out of order */
    PESTO_ERR_RANGE = -5      /* PESTO_PRECISION_F16_SPLIT only: an activation left the f16 range (z has been filled with NaN) */
} pesto_status;

/* Arithmetic of the state-update layers (the reference computes in fp32 throughout, src/model_operations.py:87-154).
 *   F16_SPLIT : every large GEMM as three v_mfma_f32_16x16x32_f16 products of f16 hi/lo pairs (x = hi + lo), fp32 accumulate:
 *               ~22-bit mantissa, but the f16 EXPONENT range - activations beyond +-65504 cannot be represented. The kernels
 *               detect that (range guard); the result is then NaN everywhere and, where the call synchronises, PESTO_ERR_RANGE.
 *   FP32      : everything on exact fp32 MFMA (v_mfma_f32_16x16x4_f32), no range limit, about half the speed.
 *   AUTO      : F16_SPLIT, and every STRUCTURE whose range guard fired is computed again on the FP32 kernels (the reference's trained
 *               i_v3_1, model/save/i_v3_1_2021-05-28_12-40, needs this: its states reach 4e5). Default.
 *               The guard is kept per structure of a launch (one word per member of a PESTO_BATCH_INDEPENDENT batch / per trajectory
 *               frame / per collated call): the repeat runs the exact kernels over the launch again but writes only the logits of
 *               the flagged structures; the others keep the logits of the split kernels. A structure's bits therefore do not depend
 *               on what shared its launch - bitwise independence of the grouping holds under AUTO as under F16_SPLIT / FP32 -
 *               and not on the handle's history either (no "fp32 first after one overflow" switch: a model that overflows on every
 *               input pays the repeat every time; pesto_get_status counts the structures repeated - use PESTO_PRECISION_FP32 for it).
 *               Host-pointer calls (which wait for their D2H copy anyway) repeat before they return. Device-pointer calls also
 *               CHECK BEFORE THEY RETURN: the flags word is final behind the last layer launch, is copied (4 bytes) in front of the
 *               pool kernels, and the call waits for THAT copy - not for the stream. When the call returns the verdict is known (bad
 *               inputs have raised, an overflowed structure has been queued again on the exact kernels), but the pool kernels may
 *               still be reading res_of_atom and writing z_out: z_out is final IN STREAM ORDER on `stream` (what a drop-in caller
 *               that goes on with further work on that stream needs), and the input / output buffers must stay valid - and must not
 *               be overwritten from the host or from another stream - until `stream` has passed the call (pesto_synchronize, or a
 *               stream / event wait of the caller's). pesto_set_async_auto(m, 1) trades the check for a fully asynchronous
 *               call: the flags word is copied to pinned memory behind the launch and looked at by the NEXT call on the handle (any
 *               forward, pesto_postprocess, pesto_get_status, pesto_set_precision, pesto_forward_batch_wait, pesto_synchronize):
 *               bad inputs are reported there (PESTO_ERR_INVALID), a range overflow queues the fp32 repeat of the remembered launch
 *               into the same z_out - the caller keeps the buffers of such a call valid until that next call / pesto_synchronize
 *               returns; until then the structures of an overflowed launch hold NaN logits (loud, never a plausible wrong number). */
typedef enum pesto_precision {
    PESTO_PRECISION_AUTO = 0,
    PESTO_PRECISION_F16_SPLIT = 1,
    PESTO_PRECISION_FP32 = 2
} pesto_precision;

/* replaces: the config dict consumed by Model.__init__ (model/model.py:7-30, model/config.py:25-63).
 * Ns=32, Nh=2, Nk=3, pool Nh=4, N1=32 are fixed (true for every run shipped with the reference). */
typedef struct pesto_config {
    int32_t n0;                    /* config["em"]["N0"]: 30 (i_v4_*) or 123 (i_v3_*) */
    int32_t n_layers;              /* len(config["sum"]) */
    int32_t nn[PESTO_MAX_LAYERS];  /* config["sum"][l]["nn"] in {8,16,32,64} */
    int32_t n_out;                 /* config["dm"]["N2"] */
    int32_t em_depth;              /* 3 = Linear-ELU-Linear-ELU-Linear (model/model.py:10-16); 1 = single Linear (i_v3_1) */
    int32_t dm_depth;              /* same for the decoder (model/model.py:24-30) */
    int32_t precision;             /* pesto_precision; no reference counterpart (torch computes in fp32) */
} pesto_config;

typedef struct pesto_model pesto_model;

enum { PESTO_PTR_HOST = 0, PESTO_PTR_DEVICE = 1 };
enum { PESTO_IDS_INT32 = 32, PESTO_IDS_INT64 = 64, PESTO_IDS_UINT16 = 16 /* pesto_forward_batch_submit only */,
       PESTO_IDS_NARROW = 0x100 /* pesto_forward_batch_submit only, OR-ed to INT32 / INT64: stage the table as uint16 (narrowed and range-checked
                                   while it is packed) when every structure has <= 65,536 atoms */ };

const char* pesto_last_error(void);

/* number of float32 values in the weight blob for this config (schema: pesto_amd/weights.py) */
int pesto_blob_size(const pesto_config* cfg, int64_t* n_floats);

/* replaces: Model(config) + load_state_dict + .to(device)  (apply_model.ipynb:87-93).
 * weights: HOST pointer to the flat blob (state_dict order, m_nn/sdk skipped). The library keeps its
 * own device copy (re-laid-out for the kernels). device: HIP device ordinal. */
int pesto_create(const pesto_config* cfg, const float* weights, int64_t n_weights, int device, pesto_model** out);
int pesto_destroy(pesto_model* m);

/* change the precision policy of an existing handle (takes effect with the next call) / read it back together with the number
 * of launch sequences run so far and how many STRUCTURES AUTO computed again on the fp32 kernels */
int pesto_set_precision(pesto_model* m, int32_t precision);
int pesto_get_status(const pesto_model* m, int32_t* precision, int64_t* n_forward, int64_t* n_fp32_rerun);
/* PESTO_PRECISION_AUTO's bill: structures (members of a batch, trajectory frames, collated calls) forwarded on the split kernels and how
 * many of them were computed again on the exact fp32 kernels. A model whose ratio stays near 1 - the reference's trained i_v3_1
 * (model/save/i_v3_1_2021-05-28_12-40: states of 4e5 from layer 13 on) repeats EVERY structure - pays split + exact on every call and
 * belongs on PESTO_PRECISION_FP32; the Python layer logs that once (logging "pesto_amd", WARNING). No reference counterpart. */
int pesto_get_auto_counters(const pesto_model* m, int64_t* n_structures, int64_t* n_repeated);
/* enabled != 0: device-pointer forwards under PESTO_PRECISION_AUTO return without synchronising; their range / input check is made by
 * the next call on the handle (see pesto_precision). Default 0: checked before the call returns. No reference counterpart. */
int pesto_set_async_auto(pesto_model* m, int32_t enabled);
/* Conditioning trigger of PESTO_PRECISION_AUTO (round 5; no reference counterpart - torch computes in fp32 throughout,
 * src/model_operations.py:109-152). The f16 hi/lo split drops a term of 2^-22 RELATIVE size per product, so the absolute error of the
 * logits grows with the magnitude of the states. A structure whose new state exceeds `limit` (max |q|, |p| of any atom) in any layer is
 * flagged like a range overflow and repeated on the exact fp32 kernels (counted by pesto_get_status). limit <= 0 switches the trigger
 * off; F16_SPLIT and FP32 ignore it.
 * Calibration (profiles/r05_state_limit.txt): the states of REAL structures reach 48 - 96 on a few of the 53 pdbs_test chains (three
 * chains above 48, one above 64 with the i_v4_1 architecture, none above 96) while their logits stay within 3e-5 of the reference, and the
 * two pinned ill-conditioned random clouds (tests/golden/fuzz_pins.npz, |p| ~ 50) sit BELOW that - state magnitude does not separate
 * them, so the default is a safety net between the sizes trained models produce and the f16 range (65,504), not a tuned detector:
 * 128 fires on none of the reference's test structures. (The pinned inputs themselves are at 8.3e-5 / 8.2e-5 from the reference's fp64
 * logits with the trigger off; a caller that wants the exact kernels on such inputs sets a lower limit or PESTO_PRECISION_FP32.) */
#define PESTO_AUTO_STATE_LIMIT_DEFAULT 128.0f
int pesto_set_auto_state_limit(pesto_model* m, float limit);
/* Second conditioning trigger of PESTO_PRECISION_AUTO, on by default: a structure with ZERO-PADDED neighbour slots - fewer than 64 atoms,
 * or a table of fewer than 64 columns (collate_batch_features pads with 0, src/dataset.py:100-109; unpack_state_features wraps those slots
 * to the last atom, src/model_operations.py:8) - is repeated on the exact fp32 kernels. Padded slots are where the forward is
 * ill-conditioned for any fp32 evaluation (the reference's own fp32 and fp64 runs differ by 1.15e-4 on the pinned 2-atom member of
 * tests/golden/fuzz_pins.npz; the split kernels by 0.8 - 1.4e-4 depending on summation order, the exact kernels by 2e-5); real structures
 * have none, so the repeat costs nothing where throughput matters. The repeat of AUTO runs the exact kernels over the WHOLE launch of a
 * flagged structure (it writes only that structure's logits): bulk callers give such structures launches of their own
 * (pesto_amd.sharding.forward_local and pesto_amd.apply.apply_model do). enabled == 0 switches it off. F16_SPLIT / FP32 ignore it. */
int pesto_set_auto_pad_trigger(pesto_model* m, int32_t enabled);

/* replaces: Model.forward(X, ids_topk, q0, M)  (model/model.py:32-52).
 * ptr_kind: PESTO_PTR_HOST (library stages H2D/D2H itself) or PESTO_PTR_DEVICE (all five buffers on
 * the model's device). stream: a hipStream_t. With device pointers the work is queued on exactly that stream
 * (NULL = HIP's default stream, which is what torch.cuda.current_stream() is by default). Under PESTO_PRECISION_AUTO the flags word
 * (bad ids / residue columns, range overflow) is read back behind the launch and the call returns once it has been checked
 * (pesto_set_async_auto(m, 1): returns at once, checked by the next call on the handle - see pesto_precision above); under
 * F16_SPLIT / FP32 the call returns at once and nothing is checked (bad inputs make every logit NaN, an overflow its structure's).
 * With host pointers NULL selects the model's own stream, the call returns after z has been copied back, and the checks
 * (PESTO_ERR_INVALID, the fp32 repeat under AUTO, PESTO_ERR_RANGE under F16_SPLIT) happen before it returns.
 * A handle owns ONE workspace: calls on different streams are ordered after one another through an event, never concurrent.
 * No allocation happens on this path once the grow-only workspace has seen a batch of this size. */
int pesto_forward(pesto_model* m, int64_t N, int64_t R, int32_t k,
                  const float* X, const void* ids_topk, int32_t ids_kind,
                  const float* q0, const int32_t* res_of_atom,
                  float* z_out, int32_t ptr_kind, void* stream);

/* replaces: the reference's bulk inference loops, which call Model.forward ONCE PER STRUCTURE (apply_model.ipynb:139-167,
 * interfaceome/apply_model.py:57-82, profiling.py:84-108), for n_struct structures laid out as one collated batch
 * (X, ids_topk, q0, res_of_atom exactly as for pesto_forward; ids_topk e.g. from pesto_knn_collate with the same offsets).
 * Structure s owns atoms [struct_offsets[s], struct_offsets[s+1]) (HOST array, n_struct + 1 entries). One launch sequence
 * for the whole batch, but the two places where the reference's forward couples the atoms of a call - the wrap-around of
 * zero-padded neighbour slots to the LAST atom and the global max(D) of the coincident-atom fix-up
 * (src/model_operations.py:8-12) - act per structure, so every structure gets the result of its own call, independent
 * of its batch mates. Pointer / stream / precision rules as pesto_forward. */
int pesto_forward_structures(pesto_model* m, int64_t N, int64_t R, int32_t k, int32_t n_struct, const int32_t* struct_offsets,
                             const float* X, const void* ids_topk, int32_t ids_kind,
                             const float* q0, const int32_t* res_of_atom,
                             float* z_out, int32_t ptr_kind, void* stream);

/* replaces: the per-frame loop of the reference's MD analysis (md_analysis/apply_model_md.ipynb cell 6):
 *     for i in frames: z_i = model(X_traj[:, i], ids_topk, q, M)        # ids_topk, q, M of frame 0 for every frame
 * n_frames coordinate sets of the SAME N atoms share ids_topk [N,k], q0 [N,n0] and res_of_atom [N]; frame f's atom i is at
 * X + f*x_frame_stride + i*x_atom_stride (strides in floats, xyz contiguous; the reference's [N, frames, 3] trajectory
 * tensor is x_frame_stride = 3, x_atom_stride = 3*frames). z_out is [n_frames, R, n_out]. Results are those of n_frames
 * separate pesto_forward calls (per-frame max(D) and wrap-around, src/model_operations.py:8-12), but frames_per_launch
 * frames (0 = choose: about 24.6k atoms, four full rounds of the layer kernels) run as ONE batch through every kernel. Pointer/stream rules as pesto_forward. */
int pesto_forward_frames(pesto_model* m, int64_t N, int64_t R, int32_t k, int64_t n_frames,
                         const float* X, int64_t x_frame_stride, int64_t x_atom_stride,
                         const void* ids_topk, int32_t ids_kind, const float* q0, const int32_t* res_of_atom,
                         float* z_out, int32_t frames_per_launch, int32_t ptr_kind, void* stream);

/* replaces: collate_batch_features (src/dataset.py:91-112) + Model.forward for a LIST of structures - the bulk drivers' loop
 * (apply_model.ipynb:139-167, interfaceome/apply_model.py:57-82) with several structures per launch.
 * HOST pointers, one entry per structure b: X[b] float32 [N_b,3]; ids_topk0[b] [N_b,k_b] 0-BASED within the structure, as
 * extract_topology returns them (k_b = min(64, N_b)); q0[b] [N_b,n0]; res_of_atom[b] int32 [N_b] (column of the structure's
 * own mask, R_b residues); z_out[b] float32 [R_b,n_out]. The arrays are copied back to back and collated ON THE DEVICE
 * (offset + 1-based ids zero-padded to 64 columns, residue columns offset). batch_mode:
 *   PESTO_BATCH_COLLATED    exactly the reference's forward on the collated batch (training-style batches, src/dataset.py:91-112):
 *                           ONE max(D) for the whole batch and zero-padded neighbour slots wrap to the LAST atom of the batch
 *                           (src/model_operations.py:8-12) - a structure's result depends on its batch mates when it has fewer
 *                           than 64 atoms or coincident atoms;
 *   PESTO_BATCH_INDEPENDENT each structure as in its own call, which is what the reference's bulk inference loops do (one
 *                           structure per forward): max(D) and the wrap target are per structure, so results do not depend on
 *                           how structures were grouped into launches (what sharding over GPUs relies on) - bit for bit under
 *                           every precision: under AUTO the range guard and its fp32 repeat are per structure (pesto_precision).
 * Returns after every z_out[b] is filled. */
enum { PESTO_BATCH_COLLATED = 0, PESTO_BATCH_INDEPENDENT = 1 };
int pesto_forward_batch(pesto_model* m, int32_t n_struct, const int64_t* N, const int64_t* R, const int32_t* k,
                        const float* const* X, const void* const* ids_topk0, int32_t ids_kind, const float* const* q0,
                        const int32_t* const* res_of_atom, float* const* z_out, int32_t batch_mode, void* stream);

/* replaces: the same bulk loop fed by DataLoader(num_workers = 8) (interfaceome/apply_model.py:50-82; SURVEY 8b, threading row: "host may
 * overlap H2D of structure t+1 with compute of t"). pesto_forward_batch in two halves, with TWO staging slots per handle:
 *   submit  packs the structures into the slot's PINNED host buffer, queues one H2D copy on the handle's copy stream and - behind it, on
 *           the handle's compute stream - the collate kernel, the forward and the D2H copy of the logits into pinned memory; returns at
 *           once with the slot as *ticket. A second submit may follow before the first is waited for: its packing and H2D copy overlap
 *           the first launch's kernels (PESTO_ERR_STATE if both slots are in flight).
 *   wait    blocks until the ticket's logits have arrived, reports bad inputs (PESTO_ERR_INVALID) / handles the range guard as
 *           pesto_forward_batch does (AUTO: the slot's inputs are still on the device, the launch is repeated on the fp32 kernels),
 *           and copies the logits into the z_out[b] arrays given at submit (which must stay valid until then; the input arrays may be
 *           reused as soon as submit returns).
 * Inputs as pesto_forward_batch, plus two compact forms that cut the H2D volume from 392 to 145 bytes per atom:
 *   ids_kind PESTO_IDS_UINT16  ids_topk0[b] as uint16 (0-based within the structure, N_b <= 65,536);
 *   q_index != NULL            instead of the dense one-hot q0[b]: uint8 [N_b, n_index] block-local indices, expanded on the GPU to
 *                              q0[i][index_offsets[c] + q_index[i][c]] = 1 (encode_features, src/data_encoding.py:78-84);
 *   q_index == NULL, n_index > 0   dense q0[b] AND the block offsets: the library looks for the indices itself while it reads the rows
 *                              for packing (every block of every row exactly one 1.0f, everything else 0.0f) and ships them as bytes; a
 *                              launch with one row that is not one-hot travels dense - same bits either way. */
int pesto_forward_batch_submit(pesto_model* m, int32_t n_struct, const int64_t* N, const int64_t* R, const int32_t* k,
                               const float* const* X, const void* const* ids_topk0, int32_t ids_kind,
                               const float* const* q0, const uint8_t* const* q_index, int32_t n_index, const int32_t* index_offsets,
                               const int32_t* const* res_of_atom, float* const* z_out, int32_t batch_mode, int32_t* ticket);
int pesto_forward_batch_wait(pesto_model* m, int32_t ticket);
/* test / measurement hook: enabled != 0 makes pesto_forward_batch_submit do its HOST half only (validation, one-hot detection, packing
 * into the pinned slot) and queue nothing on the GPU; the wait returns zero logits. profiles/host_packing.py uses it to measure the
 * packing rate one rank's CPU sustains with the GPU idle. */
int pesto_debug_host_only(pesto_model* m, int32_t enabled);

/* bytes of device workspace a batch of (N, R) needs (ownership: SURVEY 8b) */
int pesto_workspace_bytes(const pesto_model* m, int64_t N, int64_t R, int64_t* bytes);

/* wait for everything queued on the model's own stream; also runs the deferred check of the last asynchronous AUTO launch
 * (pesto_set_async_auto; its error code is returned; the structures of an overflowed launch are repeated on the fp32 kernels and waited for) */
int pesto_synchronize(pesto_model* m);

/* mean duration in milliseconds of the state-update kernels of the most recent pesto_forward, measured with
 * HIP events on the stream they ran on (bench.py's roofline leg); enable with pesto_set_timing(m, 1). */
int pesto_set_timing(pesto_model* m, int32_t enabled);
int pesto_get_timing(pesto_model* m, double* layers_ms, double* total_ms, int32_t* n_layer_launches);
/* pesto_set_timing(m, 2) additionally records one event between consecutive layer launches; this returns, for the most recent
 * forward, the summed duration and the launch count per kernel class: [0] node kernel, [1..4] edge kernel with nn = 8, 16, 32, 64
 * (bench.py's per-kernel roofline). The extra events serialise nothing but cost ~1 us each: not for timed throughput runs. */
int pesto_get_kernel_timing(pesto_model* m, double ms_sum[5], int32_t launches[5]);

/* replaces: extract_topology (src/data_encoding.py:87-102) + the index half of collate_batch_features (src/dataset.py:100-109)
 * for a concatenated batch: exact k nearest neighbours per atom WITHIN its structure, ascending distance, entries with
 * D < 1e-2 (self, coincident atoms) last, emitted as 1-based batch-global ids zero-padded to 64 columns. Distances are rounded
 * exactly as torch.norm rounds them (sqrt(fma(z, z, fma(y, y, x * x))), correctly rounded sqrt); two atoms at exactly the same float32
 * distance are ordered by index (the reference's torch.topk leaves that order undefined).
 * X [n_total,3] and ids_out [n_total,64] follow ptr_kind; struct_offsets [n_struct+1] is a HOST array (offsets[0] = 0,
 * offsets[n_struct] = n_total). */
int pesto_knn_collate(pesto_model* m, int64_t n_total, int32_t n_struct, const int32_t* struct_offsets, const float* X, int32_t k,
                      void* ids_out, int32_t ids_kind, int32_t ptr_kind, void* stream);

/* Companion of pesto_knn_collate, no reference counterpart: the reference takes whatever order torch.topk gives two neighbours at exactly
 * the same float32 distance (src/data_encoding.py:98-99); this library orders them by index. The tables agree as SETS per neighbourhood
 * unless such a tie straddles a layer's cut-off (ids_topk[:, :nn], src/model_operations.py:230): then one of two equally distant atoms is
 * inside the first 8 / 16 / 32 / 64 and the choice is as arbitrary in the reference as here - but logits can differ (0.03 observed on one
 * of 132,417 rows of the reference's pdbs_test set). This call reports those rows so that a caller can warn or pass its own table:
 * flags_out[i] bit 0 / 1 / 2 / 3 = a tie of row i straddles the cut after column 8 / 16 / 32 / 64 of `ids` (the [n_total, 64] table of
 * pesto_knn_collate for the same X / struct_offsets / k). One wave per row, one scan over the row's structure. */
int pesto_knn_tie_rows(pesto_model* m, int64_t n_total, int32_t n_struct, const int32_t* struct_offsets, const float* X, int32_t k,
                       const void* ids, int32_t ids_kind, uint8_t* flags_out, int32_t ptr_kind, void* stream);

/* replaces: the caller-side post-op p = sigmoid(z) (apply_model.ipynb:160, interfaceome/apply_model.py:76) and the
 * residue -> atom expansion of encode_bfactor (src/structure.py:208-218) for per-residue predictions.
 * z [R,n_out] -> p_out [R,n_out] (may be NULL) and bfactor_out [n_out,N] channel-major (may be NULL):
 * bfactor_out[c][i] = sigmoid(z[res_of_atom[i]][c]). With device pointers the call is asynchronous on `stream`, so a bulk
 * loop can keep every structure's result on the GPU and copy back once. */
int pesto_postprocess(pesto_model* m, int64_t N, int64_t R, const float* z, const int32_t* res_of_atom, float* p_out, float* bfactor_out,
                      int32_t ptr_kind, void* stream);

/* replaces: the dense residue mask argument M of Model.forward (model/model.py:32; built by encode_structure, src/data_encoding.py:73,
 * one 1 per row) for callers that hold M itself: M float32 [N,R] (0/1) -> res_of_atom_out int32 [N], the column of each row's single
 * member. One pass over M on the GPU (k_mask_to_segments). A row with zero or several members gives res_of_atom_out[i] = -1, an empty
 * residue column makes res_of_atom_out[0] = -1: the forward that consumes the array then fails its residue-column check
 * (PESTO_ERR_INVALID where the call synchronises, NaN logits otherwise) - SURVEY 8b's argument contract. With device pointers the call
 * is asynchronous on `stream`; with host pointers it returns PESTO_ERR_INVALID itself. */
int pesto_mask_to_segments(pesto_model* m, int64_t N, int64_t R, const float* M, int32_t* res_of_atom_out, int32_t ptr_kind, void* stream);

/* ---- evaluation: interface labels and scores (no GPU counterpart in the reference) ----
 * The two entry points below report their failures through pesto_eval_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). They use the handle for its device, after pesto_synchronize(m), and
 * allocate their buffers stream-ordered per call, so they share no workspace with the forward. */
const char* pesto_eval_last_error(void);

/* replaces: the label side of the reference's dataset build and loader - extract_all_contacts / locate_contacts (src/data_encoding.py:116-176,
 * one dense torch distance matrix per pair of subunits), contacts_types (processing/build_dataset.py:38-51) and load_interface_labels
 * OR-ed over a subunit's partners (model/save/i_v4_1_2021-09-07_11-21/data_handler.py:9-23, 100-126) - for n_struct assemblies in one launch.
 * Assembly s owns atoms [struct_offsets[s], struct_offsets[s+1]) (HOST array, n_struct + 1 entries). Per atom: X float32 [n_total,3],
 * subunit int32 (any id; atoms of one subunit share it), residue int32 (the batch-global label row of a receptor atom, in [0, n_res)),
 * receptor uint8 (!= 0: the atom's resname is one of l_types) and partner_mask uint32 (bit c: the resname is one of r_types[c]; 0 = never a
 * partner). Result: labels_out uint32 [n_res] (cleared by the call),
 *     labels_out[residue[a]] |= partner_mask[b]   for every receptor atom a and atom b of the same assembly, subunit[b] != subunit[a],
 *                                                 with the fp32 distance sqrt(fma(z,z, fma(y,y, x*x))) (torch.norm's rounding) < r_thr
 * and ties_out uint8 [n_total]: 1 where a receptor atom has such a partner at EXACTLY r_thr - the pairs on which a distance rounded another
 * way could decide the label. Cell grid (cells >= r_thr wide), one thread per atom in cell order; OR is order-free, so the result is
 * deterministic. Both paths synchronise `stream` (the offsets and the error word are host memory of the call); a receptor atom with a
 * residue outside [0, n_res) makes the call return PESTO_ERR_INVALID (with device pointers its contacts are skipped, nothing else). */
int pesto_interface_labels(pesto_model* m, int64_t n_total, int32_t n_struct, const int32_t* struct_offsets, const float* X,
                           const int32_t* subunit, const int32_t* residue, const uint8_t* receptor, const uint32_t* partner_mask,
                           int64_t n_res, float r_thr, uint32_t* labels_out, uint8_t* ties_out, int32_t ptr_kind, void* stream);

/* replaces: bc_scoring (src/scoring.py:77-96: torch counts and sklearn's roc_auc_score on the host, one structure at a time) for n_struct
 * structures in one launch. Structure s owns rows [res_offsets[s], res_offsets[s+1]) (HOST array, every structure >= 1 row) of
 * y uint8 [R,n_class] (0 / non-zero) and p float32 [R,n_class] (probabilities, finite). scores_out float32 [n_struct,8,n_class], rows
 * acc, ppv, npv, tpr, tnr, mcc, auc, std (bc_score_names): q = round(p) half to even; exact integer TP / TN / FP / FN; ppv NaN without
 * positives, npv NaN without negatives, +-inf -> NaN for tpr / tnr / mcc, 0/0 NaN; mcc in the reference's float32 operation order;
 * auc = Mann-Whitney U / (P N) with ties 1/2, 2U counted exactly over every (positive, negative) pair (NaN unless P > 0 and N > 0);
 * std = torch.std (unbiased, fp64 accumulation; NaN for one row). One workgroup per (structure, class). The call synchronises `stream`. */
int pesto_bc_scores(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const uint8_t* y, const float* p,
                    float* scores_out, int32_t ptr_kind, void* stream);

/* ---- ranking curves and pooled scores (what the reference's evaluation notebooks take from sklearn.metrics) ----
 * replaces: metrics.roc_curve, metrics.precision_recall_curve with metrics.auc, metrics.f1_score and the label-split confidence
 * histograms of interface_ppi_benchmark.ipynb, interface_type_evaluation.ipynb, interface_ppi_confidence.ipynb and
 * interfaceome/eukaryotic_protein_complexes_scoring_analysis.ipynb, on columns of 10^5 to 10^7 pooled residues.
 * Failures of the entry points below are reported through pesto_rank_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the evaluation group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`.
 *
 * The inputs are pesto_bc_scores': y uint8 [R,n_class] (0 / non-zero), p float32 [R,n_class], res_offsets int32 [n_struct+1] (HOST, every
 * segment >= 1 row), R * n_class <= 2^31 - 1, n_class <= 1024, n_struct * n_class <= PESTO_RANK_MAX_COLUMNS. A column is one (segment,
 * class) pair, col = s * n_class + c; pooled evaluation is n_struct = 1. A non-finite p (NaN, +-inf) makes the call return PESTO_ERR_INVALID (a device flag read back with the
 * outputs; sklearn refuses the same inputs). Every element becomes the key col << 33 | desc(p) << 1 | y (desc: the order-preserving map of
 * the float's bits, complemented, -0.0 taken as +0.0) and all columns are sorted at once by one LSD radix sort of 8-bit digits; the
 * distinct scores of a column in descending order are its thresholds, and with an integer scan of y the k-th has
 *     tps[k] = positives with p >= thr[k]      fps[k] = negatives with p >= thr[k]           (sklearn's _binary_clf_curve)
 * Everything below is exact integer arithmetic up to the final divisions, and bit-identical from call to call. */
const char* pesto_rank_last_error(void);

enum {
    PESTO_RANK_TILE = 2048,                   /* keys one workgroup handles per radix pass */
    PESTO_RANK_MAX_COLUMNS = (1 << 24) - 1    /* n_struct * n_class: a workgroup of 256 threads per column, below 2^32 threads per launch */
};

/* counts_out int64 [n_struct,6,n_class], rows P, N, TP, FP (q = round(p) half to even != 0, as pesto_bc_scores), K (distinct thresholds),
 * K_roc (the points roc_curve keeps with drop_intermediate, see pesto_rank_curves). scores_out float64 [n_struct,3,n_class], rows
 *     roc_auc = (double)u2 / (2.0 * P * N), u2 = sum_k (fps[k] - fps[k-1]) * (tps[k] + tps[k-1]) in uint64: the integer pesto_bc_scores
 *               counts over all pairs, so its float32 rounding equals that function's auc row bit for bit; NaN unless P > 0 and N > 0
 *     pr_auc  = the trapezoid of precision tps / (tps + fps) over recall tps / P on the points of precision_recall_curve including the
 *               closing point (recall 0, precision 1) - metrics.auc(recall, precision) - summed in float64 in a fixed order; NaN when
 *               P = 0 (sklearn then sets recall to 1 with a warning)
 *     f1      = 2 TP / (2 TP + FP + FN), 0.0 when the denominator is 0 */
int pesto_rank_scores(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const uint8_t* y, const float* p,
                      int64_t* counts_out, double* scores_out, int32_t ptr_kind, void* stream);

/* Column col owns the rows offsets_out[col] .. offsets_out[col+1] of thr_out float32 [capacity], tps_out int64 [capacity] and fps_out
 * int64 [capacity], thresholds descending. mode 0: every distinct threshold - the points of precision_recall_curve and of
 * roc_curve(drop_intermediate=False). mode 1: the first point, the last point and every point where the second difference of fps or of tps
 * is not zero - roc_curve's drop_intermediate=True, applied as sklearn applies it, before the (0, 0) point is prepended; the curve is
 * thinned on the device. offsets_out int64 [n_struct * n_class + 1]; sizes_out int64 [1] (HOST): K, the points of all columns. The capacity
 * protocol of pesto_frame_contacts (0 <= capacity < 2^31; thr_out, tps_out and fps_out may be NULL for 0): complete when K <= capacity,
 * otherwise only offsets_out and K are, nothing is emitted and the call must be repeated with the capacity K. */
int pesto_rank_curves(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const uint8_t* y, const float* p,
                      int32_t mode, int64_t capacity, int64_t* offsets_out, float* thr_out, int64_t* tps_out, int64_t* fps_out,
                      int64_t* sizes_out, int32_t ptr_kind, void* stream);

/* edges float32 [n_bins+1] (HOST), strictly increasing, no NaN; n_struct * n_class * n_bins < 2^31. counts_out int64
 * [n_struct,n_class,n_bins,2]: counts_out[s,c,:,v] = np.histogram(p[y == v], bins=edges) of the column - left-closed bins, the last one closed
 * on both sides - by binary search of every edge among the column's sorted thresholds. */
int pesto_rank_histogram(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const uint8_t* y, const float* p,
                         int32_t n_bins, const float* edges, int64_t* counts_out, int32_t ptr_kind, void* stream);

/* ---- surface-vertex benchmark scoring (masif-site_benchmark/masif_sppider_Intpred_comp.ipynb of the reference) ----
 * replaces: pyflann's nearest atom of every mesh vertex, pymesh's vertex_area, and the Python dictionaries that carry labels from vertices
 * to residues (is_res_iface, assign_labels_per_residue) and MaSIF's scores from vertices to residues (compute_pred_labels_per_residue).
 * Failures of the entry points below are reported through pesto_surface_last_error() (thread-local message of the last failing call of this
 * group; an invalid handle's message is copied there too). Like the evaluation group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`.
 *
 * A ragged batch of n_struct structures: v_offsets over V vertices, a_offsets over N atoms, r_offsets over R residues (int32 [n_struct+1],
 * HOST, every structure >= 1 entry) and f_offsets over F faces (non-decreasing: a structure may have no face). Face indices and
 * atom_residue are local to their structure; nearest-atom indices, and everything returned per vertex or per residue, are in batch order.
 * No entry point uses a floating-point atomic: every sum is a 64-bit integer sum, every output the same bits from call to call. */
const char* pesto_surface_last_error(void);

enum {
    PESTO_SURFACE_VERTEX_TILE = 256,          /* vertices one workgroup of the search owns */
    PESTO_SURFACE_ATOM_TILE = 256,            /* atoms it holds in LDS at a time */
    PESTO_SURFACE_SLAB = 512                  /* atoms of one structure one workgroup walks (slab = 0) */
};

/* vertices float32 [V,3], xyz float32 [N,3] -> index_out int32 [V] (batch atom index), distance_out float32 [V]. The key of a (vertex, atom)
 * pair of one structure is the float32 squared distance fmaf(rz, rz, fmaf(ry, ry, rx * rx)) of the float32 differences; a key that is not
 * finite (a NaN or infinite coordinate, an overflow) never matches; the smallest key wins, among equal keys the lowest atom index;
 * distance = sqrtf(key). A vertex without a match gets -1 and NaN. This is EXACT, where the reference asks FLANN for an approximate
 * neighbour in float64. slab: the atoms of one structure a workgroup walks, a multiple of PESTO_SURFACE_ATOM_TILE (0: PESTO_SURFACE_SLAB);
 * the result does not depend on it. Two launches and one memset. */
int pesto_surface_nearest(pesto_model* m, int32_t n_struct, const int32_t* v_offsets, const int32_t* a_offsets, const float* vertices,
                          const float* xyz, int32_t slab, int32_t* index_out, float* distance_out, int32_t ptr_kind, void* stream);

/* pymesh's vertex_area in fixed point: faces int32 [F,3] (local vertex indices) -> area_fixed_out int64 [V], the sum over the faces at a
 * vertex of llrint(area / 3 * 2^40), area = 0.5 * sqrt(cx cx + cy cy + cz cz) of the cross product of the edge vectors (corner 1 - corner 0,
 * corner 2 - corner 0) in float64 from the float32 coordinates, every operation rounded once as written and summed left to right. The
 * area is area_fixed * 2^-40. PESTO_ERR_INVALID when a face index lies outside its structure (nothing is read there) or a face's third is
 * not below 2^53 units (NaN included). One launch and two memsets. */
int pesto_surface_areas(pesto_model* m, int32_t n_struct, const int32_t* v_offsets, const int32_t* f_offsets, const float* vertices,
                        const int32_t* faces, int64_t* area_fixed_out, int32_t ptr_kind, void* stream);

/* Per residue, over the vertices whose nearest atom (nearest int32 [V], batch index or -1: no residue) belongs to it (atom_residue int32
 * [N], local): n_vertices_out int32 [R]; area_out and iface_area_out int64 [R], the sums of area_fixed int64 [V] over all of them and over
 * those with iface uint8 [V] != 0; label_out uint8 [R] = ia > 5.0 && ia / a > 0.04 with ia, a the two sums * 2^-40 in float64 (the
 * notebook's is_res_iface); max_score_out float32 [R], the maximum of vertex_score float32 [V] (both may be NULL), NaN for a residue
 * without a vertex, -0.0 reported as +0.0. PESTO_ERR_INVALID for a non-finite vertex_score, an index of nearest outside its structure's
 * atoms or an atom_residue outside its structure's residues. Two launches and up to five memsets. */
int pesto_surface_residues(pesto_model* m, int32_t n_struct, const int32_t* v_offsets, const int32_t* a_offsets, const int32_t* r_offsets,
                           const int32_t* nearest, const int32_t* atom_residue, const int64_t* area_fixed, const uint8_t* iface,
                           const float* vertex_score, int32_t* n_vertices_out, int64_t* area_out, int64_t* iface_area_out, uint8_t* label_out,
                           float* max_score_out, int32_t ptr_kind, void* stream);

/* out float32 [n_vertices] = p_atom[nearest[v]], NaN where nearest[v] == -1 (PESTO_ERR_INVALID for any other index outside [0, n_atoms)).
 * One launch. */
int pesto_surface_vertex_scores(pesto_model* m, int64_t n_vertices, int64_t n_atoms, const int32_t* nearest, const float* p_atom, float* out,
                                int32_t ptr_kind, void* stream);

/* The residues with n_vertices int32 [R] > 0 and valid uint8 [R] != 0 (NULL: all valid), per structure in residue order: offsets_out int64
 * [n_struct+1], residue_out int32 [capacity] (batch residue index), y_out uint8 [capacity] (label != 0), p_out float32 [capacity]
 * (p_res float32 [R]); sizes_out int64 [1] (HOST): K. The capacity protocol of pesto_frame_contacts (capacity R always fits). A structure
 * may come out empty. Three launches. */
int pesto_surface_scored(pesto_model* m, int32_t n_struct, const int32_t* r_offsets, const int32_t* n_vertices, const uint8_t* label, const float* p_res,
                         const uint8_t* valid, int64_t capacity, int64_t* offsets_out, int32_t* residue_out, uint8_t* y_out, float* p_out,
                         int64_t* sizes_out, int32_t ptr_kind, void* stream);

/* ---- interface patches (no GPU counterpart in the reference) ----
 * Failures of the entry point below are reported through pesto_patches_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the evaluation group it uses the handle for its device, after
 * pesto_synchronize(m), and allocates its buffers stream-ordered per call. */
const char* pesto_patches_last_error(void);

enum {
    PESTO_PATCHES_SMALL_MAX = 4096,       /* structures of at most this many rows: one workgroup per (structure, selection), all in LDS */
    PESTO_PATCHES_MAX_CLASSES = 1024,
    PESTO_PATCHES_MAX_SEL = 1024,
    PESTO_PATCHES_MAX_ROWS = 0x3ffffff0,
    PESTO_PATCHES_FORCE_LARGE = 1         /* flags bit: every structure takes the large-structure path (test hook) */
};

/* replaces: cluster_interfaces and cluster_multi_interfaces with follow_rabbit / follow_rabbits (interfaceome/cluster_interfaces.py:9-56,
 * interfaceome/cluster_multi_interfaces.py:9-61: a dense NumPy distance matrix and a set-based search per structure and selection) for
 * n_struct structures and n_sel selections in one call. Structure s owns rows [res_offsets[s], res_offsets[s+1]) (HOST array, n_struct + 1
 * entries, every structure >= 1 row; R = res_offsets[n_struct] <= PESTO_PATCHES_MAX_ROWS, R * n_class and R * n_sel < 2^31) of
 * xyz float32 [R,3] (the residue's CA), p float32 [R,n_class], afs float32 [R] (confidence, e.g. pLDDT; NULL: no confidence test) and
 * has_ca uint8 [R] (0: the residue has no CA and is never a node; NULL: every residue has one). sel int32 [n_sel,2] (HOST) lists the
 * class pairs (i, j), 0 <= i <= j < n_class <= PESTO_PATCHES_MAX_CLASSES, n_sel <= PESTO_PATCHES_MAX_SEL. For selection k = (i, j):
 *     node r      afs[r] > afs_thr && has_ca[r] && p[r,i] > p_thr && p[r,j] > p_thr      (float32, strict; NaN never passes)
 *     edge (a,b)  sqrt((dx*dx + dy*dy) + dz*dz) < d_thr, every operation rounded to float32 (NumPy's distance matrix); d_thr > 0 finite
 *     patches     the connected components, numbered 0, 1, ... in the order of their smallest member row (follow_rabbits' order)
 * Outputs: patch_of int32 [n_sel,R] (patch number of the row within its (structure, selection), -1 for rows that are not nodes),
 * n_patches int32 [n_struct,n_sel], patch_size int32 [n_sel,R] and patch_mean float32 [n_sel,R,2] (size and the mean of p[:,i], p[:,j] over
 * the members, summed in double, at each patch's smallest member row; 0 at every other row). Every output is bit-identical from call to
 * call. Structures of more than PESTO_PATCHES_SMALL_MAX rows spread their node-pair tiles over many workgroups. flags: 0 or
 * PESTO_PATCHES_FORCE_LARGE. The call synchronises `stream`. */
int pesto_interface_patches(pesto_model* m, int32_t n_struct, const int32_t* res_offsets, int32_t n_class, const float* xyz, const float* p,
                            const float* afs, const uint8_t* has_ca, int32_t n_sel, const int32_t* sel, float afs_thr, float p_thr, float d_thr,
                            int32_t* patch_of, int32_t* n_patches, int32_t* patch_size, float* patch_mean, int32_t flags, int32_t ptr_kind,
                            void* stream);

/* ---- dataset contacts (no GPU counterpart in the reference) ----
 * Failures of the entry point below are reported through pesto_contacts_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the evaluation group it uses the handle for its device, after
 * pesto_synchronize(m), and allocates its buffers stream-ordered per call; it keeps no state between calls. */
const char* pesto_contacts_last_error(void);

/* replaces: extract_all_contacts / locate_contacts (src/data_encoding.py:116-167, a dense torch distance matrix per pair of subunits) and
 * contacts_types + pack_contacts_data (processing/build_dataset.py:41-83, a dense [R0,R1,79,79] bool map per pair) for n_struct assemblies.
 * Assembly s owns atoms [struct_offsets[s], struct_offsets[s+1]) (HOST array). Per atom: X float32 [n_total,3]; subunit int32 in
 * [0, n_sub), n_sub <= 65535, ascending along the atoms (each subunit one contiguous run, in the reference's subunit order; a new id at
 * every assembly start); residue int32 in [0, 8192) (the column of encode_structure's M within the subunit); type int32 in [-1, n_types),
 * n_types <= 128 (the index of the atom's resname in molecule_ids, -1 for none).
 * Contacts: every (a, b) of one assembly with subunit[a] < subunit[b] and sqrt(fma(z,z, fma(y,y, x*x))) < r_thr (torch.norm's float32
 * rounding), grouped by (subunit[a], subunit[b]) ascending and within a group by a, then b - the reference's torch.where order.
 *   pairs_out int32 [cap_pairs,2] (batch atom indices a, b), d_out float32 [cap_pairs] (the distance)
 *   groups_out int32 [cap_groups,4]: per group (subunit i, subunit j, its first row of pairs_out, its number of typed keys)
 *   keys_out uint16 [cap_pairs,4]: per group in turn, torch.where of contacts_types' Y, sorted (r0, r1, t0, t1) rows. Y[r0, r1] is the
 *             [n_types, n_types] slab of the LAST pair (a, b) of the group, in the order above, with residue[a] = r0 and residue[b] = r1
 *             (the reference's index_put_ with repeated residue pairs): one row (r0, r1, type[a], type[b]) when both types are defined,
 *             none otherwise
 *   rkeys_out uint16 [cap_pairs,4]: the same rows for the swapped direction, (r1, r0, t1, t0) sorted (torch.where of Y.permute(1,0,3,2))
 *   T_out uint8 [cap_groups,n_types,n_types]: T[g][t0][t1] = 1 where group g has such a key (contacts_types' T)
 *   ties_out uint8 [n_total]: 1 where an atom of another subunit lies at EXACTLY r_thr (a differently rounded distance could decide it)
 *   sizes_out int64 [3] (HOST): K pairs, G groups, U typed keys (both directions have U). The outputs are complete when K <= cap_pairs and
 *             G <= cap_groups (cap_groups < 2^22); otherwise sizes_out holds what is known (K always; G and U -1 while K > cap_pairs) and the call must be
 *             repeated with larger capacities (the count is the one synchronisation of a call).
 * Cell grid (cells >= r_thr wide), count -> scan -> emit in (a, b) order, a stable radix regroup, stable radix sorts of packed 64-bit
 * keys: every output is bit-identical from call to call and between a batch and its assemblies one at a time. The call synchronises
 * `stream`; an id, residue or type outside its range makes it return PESTO_ERR_INVALID. */
int pesto_contacts(pesto_model* m, int64_t n_total, int32_t n_struct, const int32_t* struct_offsets, int32_t n_sub, const float* X,
                   const int32_t* subunit, const int32_t* residue, const int32_t* type, int32_t n_types, float r_thr, int64_t cap_pairs,
                   int64_t cap_groups, int32_t* pairs_out, float* d_out, int32_t* groups_out, uint16_t* keys_out, uint16_t* rkeys_out,
                   uint8_t* T_out, uint8_t* ties_out, int64_t* sizes_out, int32_t ptr_kind, void* stream);

/* ---- MD ensemble analysis (the reference's md_analysis/mdtraj_utils; its statistical contacts model is a per-frame torch loop) ----
 * Failures of the entry points below are reported through pesto_trajectory_last_error() (thread-local message of the last failing call
 * of this group; an invalid handle's message is copied there too). Like the evaluation group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`.
 * Trajectories are float32 [F,N,3] (mdtraj's xyz). Distances are the float32 ones of NumPy and torch,
 *     d = sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded, the root correctly rounded,
 * and every output is bit-identical from call to call (integer counts; floating-point sums in double in a fixed order). */
const char* pesto_trajectory_last_error(void);

enum {
    PESTO_TRAJECTORY_MAX_FRAMES = 1 << 24,    /* the reference counts frames in float32 */
    PESTO_TRAJECTORY_MAX_BINS = 128,          /* one LDS counter per (bin, thread) */
    PESTO_TRAJECTORY_MAX_MAP_ATOMS = 12288    /* Na + Nb of pesto_residue_contact_maps: one frame's atoms in LDS */
};

/* replaces: contacts_distribution (md_analysis/mdtraj_utils/statistical_contacts_model.py:7-30) for xyz_a [F,Na,3] against xyz_b [F,Nb,3]
 * (the same pointer for a trajectory against itself). edges: n_bins + 1 strictly increasing finite float64 values within the float32
 * range (HOST array), 1 <= n_bins <= PESTO_TRAJECTORY_MAX_BINS; F <= PESTO_TRAJECTORY_MAX_FRAMES; Na * Nb * n_bins < 2^31.
 *     counts_out uint32 [Na,Nb,n_bins]: the number of frames with edges[b] <= d < edges[b+1] (float32 d against the float64 edge;
 *                a NaN distance is in no bin)
 *     P_out float32 [Na,Nb,n_bins] or NULL: float32(count) / (float32(sum over b of count) + 1e-6f), the reference's normalisation
 * frame_splits: 0, or the number of frame ranges counted by separate workgroups and added as integers (test hook; the result does not
 * depend on it). */
int pesto_contact_counts(pesto_model* m, int64_t F, int64_t Na, int64_t Nb, const float* xyz_a, const float* xyz_b, int32_t n_bins,
                         const double* edges, uint32_t* counts_out, float* P_out, int32_t frame_splits, int32_t ptr_kind, void* stream);

/* replaces: StatisticalContactsModel.loglikelihood (statistical_contacts_model.py:47-75). Arguments as pesto_contact_counts; P float32
 * [Na,Nb,n_bins] is the fitted model. L_out float32 [F]: -mean over (i, j, b) of log(1 - PQ + floor(PQ)), PQ = P[i,j,b] where frame f puts
 * pair (i, j) into bin b and 0 elsewhere, evaluated in double from the float32 P. Device scratch: one double per 32 x 32 tile of pairs and
 * frame, at most 64 MB (or one 64-frame chunk of every tile, if larger): the frames go through in passes. */
int pesto_contact_loglik(pesto_model* m, int64_t F, int64_t Na, int64_t Nb, const float* xyz_a, const float* xyz_b, int32_t n_bins,
                         const double* edges, const float* P, float* L_out, int32_t ptr_kind, void* stream);

/* replaces: div_KL (statistical_contacts_model.py:78-81). P, Q float32 [n_pairs,n_bins], n_pairs * n_bins < 2^31; D_out float32 [n_pairs]:
 * -sum over b of P log(R), R = Q / (P + 1e-6f), R = 1 where R < 1e-6f, evaluated in double from the float32 inputs. */
int pesto_contact_div_kl(pesto_model* m, int64_t n_pairs, int32_t n_bins, const float* P, const float* Q, float* D_out, int32_t ptr_kind,
                         void* stream);

/* replaces: the residue-pair loop of fnat (md_analysis/mdtraj_utils/trajectory_utils.py:369-379). xyz_a [F,Na,3], xyz_b [F,Nb,3],
 * Na + Nb <= PESTO_TRAJECTORY_MAX_MAP_ATOMS. perm_a int32 [Na]: the atoms of A ordered by residue row; off_a int32 [Ra + 1]: residue r owns
 * perm_a[off_a[r] .. off_a[r+1]), every residue at least one atom (likewise perm_b, off_b). maps_out uint8 [F,Ra,Rb]: 1 where an atom
 * pair of the two residues has float32(d * scale) < r_thr (NumPy's float32 evaluation of pairwise_distance_matrix(...) < r_thr). */
int pesto_residue_contact_maps(pesto_model* m, int64_t F, int64_t Na, int64_t Nb, const float* xyz_a, const float* xyz_b, int32_t Ra, int32_t Rb,
                               const int32_t* perm_a, const int32_t* off_a, const int32_t* perm_b, const int32_t* off_b, float r_thr, float scale,
                               uint8_t* maps_out, int32_t ptr_kind, void* stream);

/* replaces: the numerator and denominator of fnat (trajectory_utils.py:386). maps uint8 [F,n], maps_ref uint8 [F_ref,n], F_ref = 1 or F.
 * native_out int64 [F]: the number of k with maps[f,k] and maps_ref[f or 0,k] set; ref_total_out int64 [1]: the number of set entries
 * of maps_ref. */
int pesto_native_contacts(pesto_model* m, int64_t F, int64_t F_ref, int64_t n, const uint8_t* maps_ref, const uint8_t* maps, int64_t* native_out,
                          int64_t* ref_total_out, int32_t ptr_kind, void* stream);

/* replaces: superpose_transform, the transform in superpose and the expression of rmsd (trajectory_utils.py:190-230, 308-325) for every
 * frame of xyz [F,N,3] onto xyz_ref [F_ref,N_ref,3], F_ref = 1 or F, fitted on n_sel >= 3 atoms: sel_ref / sel int32 [n_sel] atom
 * indices, or NULL for all atoms of that side (then n_sel equals its atom count). Per frame, in double: t, t_ref = means of the
 * selected atoms; U S V^T = svd((ref - t_ref)^T (xyz - t)) by one-sided Jacobi; R = V diag(1, 1, det(U) det(V)) U^T. A selection that
 * leaves R undetermined (collinear or coincident atoms) gets some proper rotation of the same fit, never NaN.
 *     t_out float32 [F,3], R_out float32 [F,3,3], t_ref_out float32 [F_ref,3]:  (xyz - t) R + t_ref lies on xyz_ref
 *     xyz_out float32 [F,N,3] or NULL: every atom transformed (from the double t, R, t_ref)
 *     rmsd_out float32 [F]: sqrt(mean over the selected atoms of the squared deviation from the reference's) * scale */
int pesto_superpose(pesto_model* m, int64_t F, int64_t F_ref, int64_t N_ref, int64_t N, int64_t n_sel, const float* xyz_ref, const float* xyz,
                    const int32_t* sel_ref, const int32_t* sel, double scale, float* t_out, float* R_out, float* t_ref_out, float* xyz_out,
                    float* rmsd_out, int32_t ptr_kind, void* stream);

/* replaces: Xp = X M / count at the end of md_analysis/apply_model_md.ipynb. X_frames [F,N,3]; perm int32 [N]: the atoms ordered by
 * residue row (ascending within a row); off int32 [R + 1]. out float32 [F,R,3]: the mean of each residue's atoms, summed in double in
 * atom order (NaN for a residue without atoms). */
int pesto_residue_centroids(pesto_model* m, int64_t F, int64_t N, int64_t R, const float* X_frames, const int32_t* perm, const int32_t* off,
                            float* out, int32_t ptr_kind, void* stream);

/* ---- pairwise RMSD and frame clustering (the clustering step of md_analysis/apply_model_with_clustering.ipynb and
 * clustering_analysis.ipynb; the notebooks' own clusterer is a third-party package that the reference does not contain) ----
 * Failures of the entry points below are reported through pesto_cluster_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the trajectory group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`. Every
 * output is bit-identical from call to call. */
const char* pesto_cluster_last_error(void);

enum {
    PESTO_CLUSTER_MAX_PAIRS = 1 << 28,        /* Fa * Fb of pesto_pairwise_rmsd: the matrix is indexed in 32 bits */
    PESTO_CLUSTER_MAX_FRAMES = 16384          /* F of pesto_gromos_clusters: F * F = PESTO_CLUSTER_MAX_PAIRS */
};

/* replaces: superpose_transform followed by the expression of rmsd (md_analysis/mdtraj_utils/trajectory_utils.py:190-207, 323), called
 * once per pair of frames. xyz_a [Fa,N,3], xyz_b [Fb,N,3] or NULL (xyz_a against itself, Fb = Fa); sel int32 [n_sel] atom indices or NULL
 * for all atoms (n_sel = N), used for the fit and for the measure; 1 <= n_sel <= N; Fa * Fb <= PESTO_CLUSTER_MAX_PAIRS.
 *     D_out float32 [Fa,Fb]: scale * sqrt(mean over the selected atoms of |R (b_j - t_b) - (a_i - t_a)|^2) at the optimal proper rotation
 *           (never a reflection), evaluated in double from the float32 coordinates as
 *           sqrt(max((G_a + G_b - 2 (s0 + s1 + sign(det H) s2)) / n_sel, 0)), G the centred sums of squares and s the singular values of
 *           the centred covariance H, rounded once.
 * Without xyz_b only the pairs i <= j are evaluated and mirrored: D is bitwise symmetric with a diagonal of exactly 0, and off the
 * diagonal it has the bits of the call with xyz_b = a copy of xyz_a. Device scratch: 16 bytes per frame and selected atom. */
int pesto_pairwise_rmsd(pesto_model* m, int64_t Fa, int64_t Fb, int64_t N, int64_t n_sel, const float* xyz_a, const float* xyz_b, const int32_t* sel,
                        double scale, float* D_out, int32_t ptr_kind, void* stream);

/* replaces: the clustering of the frames in md_analysis/clustering_analysis.ipynb, by the GROMOS method (Daura et al. 1999) over a
 * distance matrix. D float32 [F,F], 1 <= F <= PESTO_CLUSTER_MAX_FRAMES, bitwise symmetric (PESTO_ERR_INVALID otherwise; checked on the
 * device); cutoff finite. adj[i,j] = D[i,j] <= cutoff or i == j (a NaN compares false). While a frame is active: the centre is the active
 * frame with the most active neighbours (the lowest index on ties); it and its active neighbours get the next label and become inactive.
 *     labels_out int32 [F]; centers_out, sizes_out int32 [F], of which the first *n_clusters_out are filled (sizes never increase);
 *     n_clusters_out: one int32 in HOST memory. */
int pesto_gromos_clusters(pesto_model* m, int64_t F, const float* D, float cutoff, int32_t* labels_out, int32_t* centers_out, int32_t* sizes_out,
                          int32_t* n_clusters_out, int32_t ptr_kind, void* stream);

/* ---- density-peak clustering of frames by the centre of their predicted interface (steps 3 to 5 of the clustering in
 * md_analysis/apply_model_with_clustering.ipynb, cell lines 263-343, and clustering_analysis.ipynb) ----
 * The notebooks hand the interface centres to CLoNe, a third-party package that the reference does not contain. CLoNe is NOT reproduced:
 * what stands here is the published algorithm it derives from, density peaks (Rodriguez and Laio, Science 344, 2014). No equality with
 * CLoNe's results is claimed.
 * Failures of the entry points below are reported through pesto_peaks_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the cluster group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`. Every
 * output is bit-identical from call to call; a refused call writes nothing.
 *
 * The distance source of the two clustering entry points is exactly one of
 *     X float32 [F,d], 1 <= d <= PESTO_PEAKS_MAX_DIM, finite (PESTO_ERR_INVALID otherwise; checked on the device). The distance is
 *       float32 without contraction, the dimensions added in ascending order: s = dx0*dx0; s = s + dx1*dx1; ...; dist = sqrt_rn(s), every
 *       operation rounded to float32 (for d = 3 the trajectory group's squared distance and its root). Matrix-free: nothing of size
 *       [n,n] is allocated; n <= PESTO_PEAKS_MAX_POINTS.
 *     D float32 [F,F], F <= PESTO_CLUSTER_MAX_FRAMES, off the diagonal finite, >= 0 and bitwise symmetric (PESTO_ERR_INVALID otherwise;
 *       checked on the device); the diagonal is ignored. d is ignored.
 * idx int32 [n] selects rows (values in [0, F), else PESTO_ERR_INVALID) or is NULL (n = F); all indices below count the n selected rows. */
const char* pesto_peaks_last_error(void);

enum {
    PESTO_PEAKS_MAX_POINTS = 1 << 17,         /* n over points: seven all-pairs passes of 8.6e9 pairs stay a matter of seconds */
    PESTO_PEAKS_MAX_CLUSTERS = 1024,          /* n_clusters */
    PESTO_PEAKS_MAX_DIM = 8,                  /* d: a staged point is 8 floats */
    PESTO_PEAKS_MAX_FRAMES = 1 << 23          /* F of the interface centres: a workgroup per frame */
};
enum { PESTO_PEAKS_THRESHOLD = 0, PESTO_PEAKS_WEIGHTS = 1 };    /* mode of the interface centres */
enum { PESTO_PEAKS_CUTOFF = 0, PESTO_PEAKS_GAUSSIAN = 1 };      /* kernel of the density */

/* replaces: T = P > p_thr, Xc = sum_r(Xp T) / sum_r(T) and the interface radius r_int of apply_model_with_clustering.ipynb (cell lines
 * 263-343), for every frame at once; the clusterer that follows there is CLoNe, which is not reproduced. Xp float32 [F,R,3]; PW float32
 * [F,R]: the predictions P (PESTO_PEAKS_THRESHOLD: w_r = 1 where P > p_thr, a NaN compares false) or the weights themselves
 * (PESTO_PEAKS_WEIGHTS: w_r = PW; a negative or non-finite one makes the call return PESTO_ERR_INVALID). Per frame, in double in a fixed
 * order, terms of weight 0 skipped, each output rounded once:
 *     wsum_out double [F] = S = sum w_r; centers_out float32 [F,3] = c = sum w_r x_r / S; rg_out float32 [F] = sqrt(sum w_r |x_r - c|^2 / S)
 * A frame with S = 0 gets centers = rg = NaN. One workgroup per frame, two passes over its residues, no [F,R] intermediate. */
int pesto_weighted_centers(pesto_model* m, int64_t F, int64_t R, const float* Xp, const float* PW, int32_t mode, float p_thr, float* centers_out,
                           double* wsum_out, float* rg_out, int32_t ptr_kind, void* stream);

/* replaces: the choice of d_c from the percentile pdc inside the notebooks' clusterer (clustering_analysis.ipynb; CLoNe itself is not
 * reproduced). *dist_out (HOST memory): the k-th smallest (0-based) of the n (n - 1) / 2 distances over the pairs i < j of the selected
 * rows, n >= 2, 0 <= k < n (n - 1) / 2. Exact: a radix select over the bit patterns of the non-negative float32 distances in three passes
 * (digits of 11, 10 and 10 bits), each a histogram of integer counts (LDS bins per workgroup, 64-bit totals, integer atomics only); the
 * distances are recomputed in every pass and never stored. */
int pesto_pair_distance_rank(pesto_model* m, int64_t F, int32_t d, const float* X, const float* D, int64_t n, const int32_t* idx, int64_t k,
                             float* dist_out, int32_t ptr_kind, void* stream);

/* replaces: the clustering of the interface centres in apply_model_with_clustering.ipynb (cell lines 263-343) and
 * clustering_analysis.ipynb, by density peaks; CLoNe, the notebooks' clusterer, is not reproduced. dc finite and > 0. "Denser" is the total
 * order key(j) > key(i): rho_j > rho_i, or rho_j == rho_i and j < i.
 *     rho_out double [n]: PESTO_PEAKS_CUTOFF the number of j != i with d_ij < dc (strictly); PESTO_PEAKS_GAUSSIAN sum over j != i of
 *         exp(-(d_ij / dc)^2) in double from the float32 d_ij and dc, in a fixed order
 *     nh_out int32 [n], delta_out float32 [n]: the denser j with the smallest d_ij (the lowest j among equal distances) and that distance;
 *         for the densest point -1 and the largest d_ij (0 when n = 1)
 *     centres: the densest point always. n_clusters = K in 1 .. min(n, PESTO_PEAKS_MAX_CLUSTERS): it and the K - 1 others with the largest
 *         gamma_i = rho_i * (double)delta_i (the lower index first among equal ones). n_clusters = 0: it and every point with
 *         rho_i >= rho_min and delta_i >= delta_min. centers_out, sizes_out int32 [n], of which the first *n_clusters_out are filled: the
 *         centres from the densest to the least dense by key, and the members of each; n_clusters_out: one int32 in HOST memory
 *     labels_out int32 [n]: labels[centers[c]] = c, labels[i] = labels[nh[i]] otherwise (pointer jumping, at most ceil(log2 n) rounds)
 *     halo_out uint8 [n]: rho_i < rho_b[labels[i]], rho_b[c] the largest (rho_i + rho_j) / 2 over the pairs i in c, j not in c with
 *         d_ij < dc (0 without such a pair), taken by an integer atomic maximum on the bits of the non-negative double
 * All-pairs passes: density, nearest denser point, border density over the distances; two rankings without distances. */
int pesto_density_peaks(pesto_model* m, int64_t F, int32_t d, const float* X, const float* D, int64_t n, const int32_t* idx, float dc, int32_t kernel,
                        int32_t n_clusters, double rho_min, float delta_min, double* rho_out, float* delta_out, int32_t* nh_out, int32_t* labels_out,
                        uint8_t* halo_out, int32_t* centers_out, int32_t* sizes_out, int32_t* n_clusters_out, int32_t ptr_kind, void* stream);

/* ---- docking metrics and frame contacts (the remaining array functions of md_analysis/mdtraj_utils/trajectory_utils.py) ----
 * Failures of the entry points below are reported through pesto_docking_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the trajectory group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`.
 * Coordinates are float32 [F,N,3]. The distance is the trajectory group's float32 one times a scale, r_thr and scale being float32:
 *     d = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * scale, every operation rounded as written, the root correctly rounded;
 * r_thr finite, scale positive and finite. Every output is bit-identical from call to call. */
const char* pesto_docking_last_error(void);

enum {
    PESTO_DOCKING_MAX_FRAMES = 1 << 23,       /* a workgroup of 256 threads per frame, below 2^32 threads per launch */
    PESTO_DOCKING_MAX_MAP_WORDS = 1 << 28     /* F * ceil(Ra * Rb / 32) of pesto_frame_residue_contacts: two int32 of scratch per word */
};

/* replaces: the frame loop of contacts (trajectory_utils.py:408-423; per frame a dense [Na,Nb] torch matrix, torch.where and three
 * copies to the host). xyz_a [F,Na,3], xyz_b [F,Nb,3], Na * Nb < 2^31. Frame f owns the rows offsets_out[f] .. offsets_out[f+1] of
 *     pairs_out int32 [cap_pairs,2]: exactly the (i, j) with d < r_thr, i ascending, then j ascending (torch.where's order); a NaN
 *                distance is in no list
 *     d_out float32 [cap_pairs]: their d
 *     offsets_out int64 [F+1]; sizes_out int64 [1] (HOST): K, the number of contacts of all frames
 * The outputs are complete when K <= cap_pairs (1 <= cap_pairs < 2^30); otherwise only offsets_out and K are, and the call must be
 * repeated with a larger capacity (the count is the one synchronisation of a call). A tiled brute-force search, count -> scan -> emit;
 * the [Na,Nb] matrix is never stored. */
int pesto_frame_contacts(pesto_model* m, int64_t F, int64_t Na, int64_t Nb, const float* xyz_a, const float* xyz_b, float r_thr, float scale,
                         int64_t cap_pairs, int64_t* offsets_out, int32_t* pairs_out, float* d_out, int64_t* sizes_out, int32_t ptr_kind,
                         void* stream);

/* replaces: atoms_to_residue_contacts (trajectory_utils.py:233-264; np.unique and a Python loop per frame and residue pair). offsets int64
 * [F+1], pairs int32 [K,2], d float32 [K]: the lists of pesto_frame_contacts (0 <= K < 2^30; d non-negative, no NaN). res_a int32 [Na],
 * res_b int32 [Nb]: the residue row of each atom, in [0, Ra) and [0, Rb). Frame f owns the rows roffsets_out[f] .. roffsets_out[f+1] of
 *     rpairs_out int32 [cap_rpairs,2]: the distinct (res_a[i], res_b[j]) of the frame's contacts in lexicographic order (np.unique, axis 0)
 *     dmin_out float32 [cap_rpairs]: the smallest d among the contacts of each
 *     roffsets_out int64 [F+1]; sizes_out int64 [1] (HOST): U, the number of residue pairs of all frames
 * with the capacity protocol of pesto_frame_contacts (1 <= cap_rpairs < 2^30). A bit map of [Ra,Rb] per frame (at most
 * PESTO_DOCKING_MAX_MAP_WORDS words in all), its set bits emitted in index order, the minimum by an integer atomic on the bits of d: exact
 * and independent of the order of the threads. An atom index or residue row outside its range makes the call return PESTO_ERR_INVALID. */
int pesto_frame_residue_contacts(pesto_model* m, int64_t F, int64_t Na, int64_t Nb, int64_t K, const int64_t* offsets, const int32_t* pairs,
                                 const float* d, const int32_t* res_a, const int32_t* res_b, int32_t Ra, int32_t Rb, int64_t cap_rpairs,
                                 int64_t* roffsets_out, int32_t* rpairs_out, float* dmin_out, int64_t* sizes_out, int32_t ptr_kind, void* stream);

/* replaces: interface_residues_within (trajectory_utils.py:267-297; a dense distance matrix and an [N,residues] isclose matrix). xyz0
 * [N,3]: the reference frame; ids_a int32 [na], ids_b int32 [nb]: the atoms of the two subunits; res_of_atom int32 [N] in [0, R).
 * flags_out uint8 [2,N]: flags_out[0][n] = 1 where the residue of atom n holds an atom of ids_a with d <= r_thr to some atom of ids_b,
 * flags_out[1][n] likewise for ids_b against ids_a (every atom of such a residue, in ids_a or not; note <=, where the contacts have <).
 * An index or row outside its range makes the call return PESTO_ERR_INVALID. */
int pesto_interface_atoms(pesto_model* m, int64_t N, const float* xyz0, int64_t na, const int32_t* ids_a, int64_t nb, const int32_t* ids_b,
                          const int32_t* res_of_atom, int32_t R, float r_thr, float scale, uint8_t* flags_out, int32_t ptr_kind, void* stream);

/* replaces: interface_rigid_docking (trajectory_utils.py:474-499; two batched SVD superpositions, a transformed copy of the whole
 * trajectory between them, scipy's as_rotvec). xyz_ref [F_ref,N,3], F_ref = 1 or F; xyz [F,N,3]; sel_R int32 [n_R], sel_L int32 [n_L]:
 * the receptor's and the ligand's interface atoms (in [0, N), else PESTO_ERR_INVALID; at least 3 each). Per frame, in double from the float32
 * inputs: the fit of pesto_superpose on sel_R; the atoms of sel_L alone transformed by it; their fit onto the reference's sel_L, giving
 * t_cm, R2, t_ref2 (the same sums, order and rotation, degenerate selections included).
 *     t_out float32 [F,3] = t_ref2 - t_cm, in the coordinates' unit
 *     r_out float32 [F,3] = the rotation vector of R2 as scipy's Rotation.from_matrix(R2).as_rotvec() reads it: unit quaternion with
 *           w >= 0, angle = 2 atan2(|v|, w) in [0, pi], r = angle v / |v|, 0 for the identity. Near angle = pi the sign of the axis is
 *           decided by rounding, here as anywhere.
 * A selection that equals the reference's bit for bit is fitted by the identity itself (no rotation within rounding of it): a frame that
 * is the reference gives t = 0 and r = 0 exactly. One kernel, one workgroup per frame; no [F,N,3] intermediate. */
int pesto_rigid_docking(pesto_model* m, int64_t F, int64_t F_ref, int64_t N, const float* xyz_ref, const float* xyz, int64_t n_R,
                        const int32_t* sel_R, int64_t n_L, const int32_t* sel_L, float* t_out, float* r_out, int32_t ptr_kind, void* stream);

/* replaces: irmsd (trajectory_utils.py:328-338; interface selection, SVD superposition of copies of the trajectory, the rmsd expression)
 * once the interface's CA atoms are known: sel int32 [n_sel], n_sel >= 3, in [0, N) (else PESTO_ERR_INVALID), the same atoms of xyz_ref
 * [F_ref,N,3] and xyz [F,N,3]. rmsd_out float32 [F]: the rmsd_out of pesto_superpose fitted on sel on both sides, bit for bit (the same
 * kernel as pesto_rigid_docking, stopped after its first fit) - except that a selection equal to the reference's bit for bit is fitted by
 * the identity itself and gives exactly 0, where pesto_superpose leaves the rounding residue of its rotation (some 1e-15). */
int pesto_interface_rmsd(pesto_model* m, int64_t F, int64_t F_ref, int64_t N, const float* xyz_ref, const float* xyz, int64_t n_sel,
                         const int32_t* sel, double scale, float* rmsd_out, int32_t ptr_kind, void* stream);

/* ---- DockQ scoring of docking decoys against the bound complex (fnat, interface RMSD, ligand RMSD, DockQ, CAPRI class) ----
 * Failures of the entry points below are reported through pesto_dockq_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the docking group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`. The
 * distance and its tests are the docking group's; the RMSDs are evaluated in double from the float32 inputs and rounded once. No
 * floating-point atomics: every output is bit-identical from call to call. Every index is checked on the device before anything
 * dereferences it; a refused call returns PESTO_ERR_INVALID and writes nothing. */
const char* pesto_dockq_last_error(void);

enum {
    PESTO_DOCKQ_MAX_FRAMES = 1 << 23,         /* a workgroup of 256 threads per decoy, below 2^32 threads per launch */
    PESTO_DOCKQ_MAX_PAIRS = 1 << 24           /* native residue pairs of one call; each at most 2^31 - 1 atom pairs */
};

/* replaces, for F decoys of one complex at once: fnat through trajectory_utils.py's all-pairs residue maps of every frame (this
 * library's pesto_residue_contact_maps over the full sides and pesto_native_contacts), irmsd (trajectory_utils.py:328-338) once the
 * interface atoms are known, and what neither had: the ligand RMSD (a fit on one selection measured on another), the DockQ score (Basu and
 * Wallner 2016) and the CAPRI class. xyz_ref float32 [N,3]: the bound complex; xyz float32 [F,N,3]: the decoys, same atom order.
 *     pairs int32 [P,4], 1 <= P <= PESTO_DOCKQ_MAX_PAIRS: per native residue pair the ranges [a0, a1) and [b0, b1) of
 *         perm int32 [n_perm] that hold the atoms of its receptor residue and of its ligand residue (atom indices in [0, N); ranges
 *         non-empty, within [0, n_perm], (a1 - a0) (b1 - b0) < 2^31)
 *     sel_I int32 [n_I >= 3]: the interface's backbone atoms; sel_R int32 [n_R >= 3]: the receptor's; sel_L int32 [n_L >= 1]: the ligand's
 *     r_contact float32, scale > 0 (rounded to float32 for the distance test d < r_contact, used as given for the RMSDs)
 * Per decoy f:
 *     preserved_out int32 [F]: the pairs with an atom pair d < r_contact (a NaN distance passes no test)
 *     fnat_out float32 [F] = float32(double(preserved) / double(P))
 *     irmsd_out float32 [F]: the rmsd_out of pesto_interface_rmsd on sel_I, bit for bit
 *     lrmsd_out float32 [F] = float32(sqrt(sum over sel_L of |x' - y|^2 / n_L) scale), x' the atom moved by the fit of the decoy onto
 *         xyz_ref on sel_R (the first fit of pesto_rigid_docking, its identity short cut included: a decoy that is the reference gives 0)
 *     dockq_out float32 [F] = float32((fnat + 1 / (1 + (irmsd / 1.5)^2) + 1 / (1 + (lrmsd / 8.5)^2)) / 3), in double from the three float32
 *         values, every operation rounded as written
 *     capri_out uint8 [F]: 3 if 2 preserved >= P and (lrmsd <= 1 or irmsd <= 1); else 2 if 10 preserved >= 3 P and (lrmsd <= 5 or
 *         irmsd <= 2); else 1 if 10 preserved >= P and (lrmsd <= 10 or irmsd <= 4); else 0 - the fnat conditions on the integers
 * One launch behind the index check, one workgroup per decoy: a wave per native pair with an early exit at its first contact, then the
 * two fits. */
int pesto_dockq(pesto_model* m, int64_t F, int64_t N, const float* xyz_ref, const float* xyz, int64_t P, const int32_t* pairs, int64_t n_perm,
                const int32_t* perm, int64_t n_I, const int32_t* sel_I, int64_t n_R, const int32_t* sel_R, int64_t n_L, const int32_t* sel_L,
                float r_contact, double scale, float* fnat_out, int32_t* preserved_out, float* irmsd_out, float* lrmsd_out, float* dockq_out,
                uint8_t* capri_out, int32_t ptr_kind, void* stream);

/* replaces: the rmsd expression of trajectory_utils.py:328-338 behind a superposition on OTHER atoms than it measures, which neither the
 * reference's irmsd nor pesto_superpose offers (both fit and measure on one selection). xyz_ref [F_ref,N,3], F_ref = 1 or F; xyz [F,N,3];
 * sel_fit int32 [n_fit >= 3], sel_measure int32 [n_measure >= 1], in [0, N). rmsd_out float32 [F] = float32(sqrt(sum over sel_measure of
 * |x' - y|^2 / n_measure) scale), x' moved by the fit on sel_fit - the one fit of pesto_superpose, pesto_rigid_docking, pesto_interface_rmsd and pesto_dockq (pesto_fit.h),
 * so this is pesto_dockq's lrmsd_out bit for bit for sel_R, sel_L and pesto_interface_rmsd's rmsd_out for sel_measure = sel_fit. */
int pesto_fit_rmsd(pesto_model* m, int64_t F, int64_t F_ref, int64_t N, const float* xyz_ref, const float* xyz, int64_t n_fit, const int32_t* sel_fit,
                   int64_t n_measure, const int32_t* sel_measure, double scale, float* rmsd_out, int32_t ptr_kind, void* stream);

/* ---- rigid poses of a ligand on a receptor: scoring against the predicted interfaces, sliding to contact, ranking ----
 * Failures of the entry points below are reported through pesto_poses_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the docking group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`. The
 * definitions are this library's own. Pose f is (R_f = rotations[f] float32 [3,3] row-major, t_f = translations[f] float32 [3]), both
 * finite; R_f need not be orthonormal. Ligand atom x has, in pose f, the coordinates
 *     y_a = ((R[a,0]*x_0 + R[a,1]*x_1) + R[a,2]*x_2) + t_a        float32, every operation rounded as written, no contraction
 * and every function sees the ligand through this placement alone. The distance and its test are the docking group's: d =
 * fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * scale < r, a NaN distance passes no test. No floating-point atomics: every output is
 * bit-identical from call to call, between host and device pointers, and for a pose alone or inside a batch. Every index is checked
 * for its range, and every probability, pose and direction for its value, on the device before anything relies on it; a refused call
 * returns PESTO_ERR_INVALID and writes nothing. Coordinates may hold anything: a non-finite one gives its atom no pair. */
const char* pesto_poses_last_error(void);

enum {
    PESTO_POSES_MAX_FRAMES = 1 << 23,         /* a workgroup of 256 threads per pose, below 2^32 threads per launch */
    PESTO_POSES_MAX_RESIDUES = 4096,          /* residues of either side: a residue mask is at most 128 words of LDS */
    PESTO_POSES_MAX_PAIRS = 0x7fffffff,       /* N_R * N_L: a pose's contact count is an int32 */
    PESTO_POSES_MAX_PLACED = 0x7fffffff       /* F * (N_R + N_L) atoms written by pesto_poses_materialize */
};

/* how well each of F poses agrees with the two predicted interfaces. xyz_R float32 [N_R,3] (never moved), xyz_L float32 [N_L,3];
 * res_R int32 [N_R]: the residue row of every receptor atom, in [0, R_R); the ligand's atoms come ordered by residue: perm_L int32 [N_L]
 * (atom indices in [0, N_L); that they are distinct, a permutation, is the caller's contract and is NOT checked: an index named twice
 * is counted twice, nothing else) and off_L int32 [R_L + 1] (0 = off_L[0] < ... < off_L[R_L] = N_L: residue s owns
 * perm_L[off_L[s] .. off_L[s+1])); 1 <= R_R, R_L <= PESTO_POSES_MAX_RESIDUES; p_R float32 [R_R], p_L float32 [R_L]: the predicted interface
 * probability of every residue, finite and >= 0; 0 <= r_clash <= r_contact, scale > 0; N_R * N_L <= PESTO_POSES_MAX_PAIRS. Per pose f:
 *     n_contact_out int32 [F]: the atom pairs (receptor atom, placed ligand atom) with d < r_contact; n_clash_out: with d < r_clash
 *     n_res_R_out, n_res_L_out int32 [F]: the residues of either side with a contact pair, the pose's interfaces I_R, I_L
 *     n_pairs_out int32 [F]: the distinct residue pairs (r, s) with a contact pair, C
 *     w_R_out, w_L_out double [F] = sum over I_R of p_R[r], sum over I_L of p_L[s]; w_pair_out double [F] = sum over C of
 *         double(p_R[r]) * double(p_L[s]) (every product exact), each in double in an order that depends on the pose's sets alone
 *     score_out float32 [F] = float32((dice_R + dice_L) / 2), dice_R = 2 w_R / (n_res_R + P_R), P_R = sum of p_R in double, 0 where the
 *         denominator is 0; dice_L likewise: the soft Dice overlap of the predicted and the posed interface
 *     masks_out uint32 [F, ceil(R_R / 32) + ceil(R_L / 32)] or NULL: bit r % 32 of word r / 32 set for r in I_R, then the ligand's words
 * One cell grid over the receptor per call, one workgroup per pose, a wave per ligand residue; the frames are never stored and no pair
 * list is written. A receptor atom with a non-finite coordinate has no pair by the definition (its distances are NaN or infinite); the
 * grid is built on a copy in which such atoms sit on the first finite atom (the origin without one), and they are tested as NaN. */
int pesto_poses_scores(pesto_model* m, int64_t F, int64_t N_R, int64_t N_L, int32_t R_R, int32_t R_L, const float* xyz_R, const float* xyz_L,
                       const int32_t* res_R, const int32_t* perm_L, const int32_t* off_L, const float* rotations, const float* translations,
                       const float* p_R, const float* p_L, float r_contact, float r_clash, float scale, int32_t* n_contact_out, int32_t* n_clash_out,
                       int32_t* n_res_R_out, int32_t* n_res_L_out, int32_t* n_pairs_out, double* w_R_out, double* w_L_out, double* w_pair_out,
                       float* score_out, uint32_t* masks_out, int32_t ptr_kind, void* stream);

/* how far the ligand, placed with t = origins[f] and withdrawn along +u = directions[f] (float32 [F,3], used as given,
 * | |u|^2 - 1 | <= 1e-3 in double), can be pushed back until it first touches the receptor. In double, every operation rounded as
 * written, over every atom pair (i of the receptor, j of the ligand):
 *     w = double(y_j) - double(x_i);  b = (w0*u0 + w1*u1) + w2*u2;  c = ((w0*w0 + w1*w1) + w2*w2) - b*b
 *     rho = double(r_touch) / double(scale);  disc = rho*rho - c;  the pair counts where disc > 0;  s_ij = -b + sqrt(disc)
 * s_out double [F] = the maximum of s_ij; pair_out int32 [F,2] = the (i, j) that attains it, the smallest (i, then j) among ties;
 * translations_out float32 [F,3] = float32(double(origin) + s * u) per component. Where no pair counts (the ray misses; a non-finite
 * w counts for nothing): s and the translation are NaN and the pair is (-1, -1). r_touch >= 0, scale > 0, N_R * N_L <=
 * PESTO_POSES_MAX_PAIRS. All pairs, one workgroup per pose, receptor tiles in LDS; the maximum does not depend on the order. */
int pesto_poses_slide(pesto_model* m, int64_t F, int64_t N_R, int64_t N_L, const float* xyz_R, const float* xyz_L, const float* rotations,
                      const float* origins, const float* directions, float r_touch, float scale, double* s_out, float* translations_out,
                      int32_t* pair_out, int32_t ptr_kind, void* stream);

/* the placed frames, for the entry points that take frames: xyz_out float32 [F, N_R + N_L, 3], the receptor's rows first (copied;
 * N_R = 0 and xyz_R = NULL: the ligand alone), then the placement of every ligand atom, bit for bit. F * (N_R + N_L) <=
 * PESTO_POSES_MAX_PLACED. */
int pesto_poses_materialize(pesto_model* m, int64_t F, int64_t N_R, int64_t N_L, const float* xyz_R, const float* xyz_L, const float* rotations,
                            const float* translations, float* xyz_out, int32_t ptr_kind, void* stream);

/* the best poses: index_out int32 [min(k, F)], of which the first count_out[0] = min(k, eligible) are written (count_out: HOST int64
 * [1]). Eligible are the poses whose score float32 [F] is not a NaN and, with n_clash int32 [F] given (NULL: no filter), n_clash <=
 * max_clash; they come by score descending (-0.0 equals 0.0), ties by index ascending. k >= 0. One stable radix sort of 64-bit keys on
 * the score's 32 bits; no host sort. */
int pesto_poses_top(pesto_model* m, int64_t F, int64_t k, const float* score, const int32_t* n_clash, int32_t max_clash, int32_t* index_out,
                    int64_t* count_out, int32_t ptr_kind, void* stream);

/* ---- lDDT model-quality scoring (Mariani et al. 2013): superposition-free, per residue, over all frames ----
 * Failures of the entry points below are reported through pesto_lddt_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the docking group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`.
 *
 * Definition (this library's own; no equality with OpenStructure's lddt is claimed: there is no stereochemistry filter, no renaming of
 * symmetric side-chain atoms, no sequence separation and no periodic image). The distance is the docking group's,
 * d(a, b) = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * fl32(scale), and a NaN distance passes no test.
 *     reference pairs: the ordered pairs (i, j), i != j, of atoms of one structure, both selected (sel uint8 [N], NULL: all), with
 *         res_of_atom[i] != res_of_atom[j], d_ref(i, j) < r_incl in xyz_ref and, for mode 1 (inter), chain_of_atom[i] != chain_of_atom[j],
 *         for mode 2 (intra) the chains equal (mode 0, all: chain_of_atom may be NULL). K of them; an atom with a non-finite reference
 *         coordinate has none.
 *     total[r] int32: the pairs with i in residue r
 *     preserved[f,r,k] int32: those with fabsf(d_f(i, j) - d_ref(i, j)) < thresholds[k], the subtraction rounded once in float32
 *     residue[f,r] float32 = float32(double(sum_k preserved[f,r,k]) / double(T total[r])), NaN where total[r] = 0
 *     score[f,s] float32: the same quotient over the int64 sums over the residues of structure s, NaN for a structure without pairs
 * Every output is an integer count or one rounded quotient of integers: bit-identical from call to call. */
const char* pesto_lddt_last_error(void);

enum {
    PESTO_LDDT_MAX_FRAMES = 1 << 23,          /* frames of one call */
    PESTO_LDDT_MAX_ENTRIES = 1 << 30,         /* reference pairs (list entries) of one call */
    PESTO_LDDT_MAX_THRESHOLDS = 8
};

/* The reference list as CSR over the atoms: offsets_out int64 [N + 1], row i = offsets_out[i] .. offsets_out[i + 1] holds j_out int32 and
 * d_out float32 = d_ref(i, j) of atom i's pairs, in no particular order within a row (the cell grid's). xyz_ref float32 [N,3] holds
 * n_struct structures back to back (struct_offsets int32 [n_struct + 1], host memory; pairs never cross structures); res_of_atom int32
 * [N]: labels that are only compared, any value >= 0 (a negative one: PESTO_ERR_INVALID, found on the device); chain_of_atom int32 [N]
 * or NULL (mode 0); sel uint8 [N] or NULL; r_incl and scale positive and finite, rounded to float32.
 * *n_pairs_out (host memory) = K is written whenever the count pass ran; the offsets on success; the K entries only when K <= capacity
 * (capacity 0 with j_out = d_out = NULL asks for the count alone). K > PESTO_LDDT_MAX_ENTRIES: PESTO_ERR_INVALID, and nothing but
 * *n_pairs_out is written. The grid of pesto_interface_labels at r_incl /
 * scale, a count pass, a 64-bit scan and a fill pass; one synchronisation to read K. */
int pesto_lddt_pairs(pesto_model* m, int64_t N, int32_t n_struct, const int32_t* struct_offsets, const float* xyz_ref, const int32_t* res_of_atom,
                     const int32_t* chain_of_atom, const uint8_t* sel, int32_t mode, float r_incl, double scale, int64_t capacity,
                     int64_t* offsets_out, int32_t* j_out, float* d_out, int64_t* n_pairs_out, int32_t ptr_kind, void* stream);

/* lDDT of the F frames xyz float32 [F,N,3] against xyz_ref float32 [N,3] (same atom order; a missing atom has NaN coordinates).
 *     struct_offsets, res_struct_offsets int32 [n_struct + 1], host memory: the atoms and the residue rows of every structure (a ragged
 *         batch; one structure: {0, N} and {0, R})
 *     res_of_atom int32 [N] in [0, R); perm int32 [N]: the atoms ordered by residue row; res_offsets int32 [R + 1]: row r owns
 *         perm[res_offsets[r] .. res_offsets[r + 1]) (the atoms of a residue need not be adjacent)
 *     thresholds float32 [T], host memory, 1 <= T <= PESTO_LDDT_MAX_THRESHOLDS, positive and ascending
 *     offsets_in / j_in / d_in / K_in: the list of pesto_lddt_pairs, or offsets_in NULL: the list is built here from xyz_ref,
 *         chain_of_atom, sel, mode and r_incl (which are not read when a list is given), sized after its count pass and freed on return
 * Outputs: score_out float32 [F,n_struct], residue_out float32 [F,R], preserved_out int32 [F,R,T], total_out int32 [R] and n_pairs_out
 * int64 [n_struct] (host memory). Every index is checked for what the kernels dereference by it - res_of_atom in [0, R), res_offsets an
 * ordered split of [0, N], perm in [0, N) with each entry's atom in the residue whose range holds the entry, a residue's atoms inside its
 * structure, a given list's offsets ascending from 0 to K and its partners in [0, N) - by a kernel whose verdict is read before anything
 * else is launched: a refused call returns PESTO_ERR_INVALID and writes nothing. Not checked, because nothing is addressed by it: that
 * perm names every atom once (a repeated atom counts twice) and that a given list's partners lie in their atom's structure (the list of
 * pesto_lddt_pairs does). A list built here with K > PESTO_LDDT_MAX_ENTRIES: PESTO_ERR_INVALID with n_pairs_out[0] = K, nothing else
 * written. Then the list (unless given), one scoring launch over all frames - a wave per (frame, residue), its lanes across
 * a row's entries, integer counts in registers, no atomics - and one workgroup per (structure, frame) for the quotients. */
int pesto_lddt(pesto_model* m, int64_t F, int64_t N, int32_t n_struct, const int32_t* struct_offsets, const int32_t* res_struct_offsets,
               const float* xyz_ref, const float* xyz, int64_t R, const int32_t* res_of_atom, const int32_t* perm, const int32_t* res_offsets,
               const int32_t* chain_of_atom, const uint8_t* sel, int32_t mode, int32_t T, const float* thresholds, float r_incl, double scale,
               int64_t K_in, const int64_t* offsets_in, const int32_t* j_in, const float* d_in, float* score_out,
               float* residue_out, int32_t* preserved_out, int32_t* total_out, int64_t* n_pairs_out, int32_t ptr_kind, void* stream);

/* ---- TM-score and GDT of a model against its reference for a given residue correspondence (Zhang and Skolnick 2004) ----
 * Failures of the entry point below are reported through pesto_tmscore_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the DockQ group it uses the handle for its device, after
 * pesto_synchronize(m), allocates its buffers stream-ordered per call, keeps no state between calls and synchronises `stream`.
 * replaces: what the package lacked next to lDDT and the RMSDs - the global fold measures that the reference's model selection
 * (interfaceome/selecting_alphafold_models.ipynb) and its MD notebooks' single RMSD curve stand in for; outside the package, one run of
 * the TMscore program per pair. */
const char* pesto_tmscore_last_error(void);

enum {
    PESTO_TMSCORE_MAX_FRAMES = 1 << 23,       /* frames, or structures of a ragged batch, of one call */
    PESTO_TMSCORE_MAX_LENGTH = 4096,          /* selected atoms of a structure: 64 lanes of a wave times the 64 bits of a lane's word */
    PESTO_TMSCORE_MAX_ITER = 1024,            /* n_iter */
    PESTO_TMSCORE_MAX_RAISE = 4096            /* raises of d_cut by 0.5 behind one fit */
};

/* replaces: the superposition search of the TMscore program for F models of one structure (or one model each of n_struct structures) in
 * one call. xyz_ref float32 [N,3], xyz float32 [F,N,3] in the same atom order; sel int32 [sel_offsets[n_struct]]: the atoms scored, in
 * sequence order, structure after structure (sel_offsets int32 [n_struct + 1], host memory, from 0; 3 <= L <= PESTO_TMSCORE_MAX_LENGTH
 * atoms each; n_struct > 1 needs F = 1). norm_len, d0 double [n_struct], host memory, positive: L_norm and d0 of every structure (the
 * caller's choice; customarily L and max(0.5, 1.24 cbrt(max(L_norm - 15, 0)) - 1.8)).
 * Definition, in double from the float32 inputs: d_i = sqrt(|x'_i - y_i|^2) scale under a fit x' = (x - m) R + m_ref (pesto_fit.h, with
 * its identity short cut); TM(fit) = (sum_i 1 / (1 + (d_i / d0)^2)) / L_norm; count_c(fit) = |{i: d_i < c}|, c = 0.5, 1, 2, 4, 8.
 * Seeds: the windows of length L >> k (k = 0 .. 5, while above 4), then min(L, 4), at the starts 0, step, 2 step, ... <= L - n and
 * L - n, numbered length first, then start. A search: S = the window; up to n_iter times: fit on S (the fit is visited), S' = {i: d_i
 * < d_cut} with d_cut = min(8, max(4.5, d0)) raised by 0.5 while |S'| < 3 (at most PESTO_TMSCORE_MAX_RAISE times, then the seed
 * ends), stop if S' = S, else S = S'. Per unit u (frame, or structure):
 *     tm_out float32 [U]: the largest TM over all visited fits; seed_out int32 [U]: the lowest seed that attains it;
 *     rotation_out double [U,3,3], translation_out double [U,3]: that seed's first such fit as x' = x R + t, t = m_ref - m R
 *     counts_out int32 [U,5]: the largest count_c over all visited fits; gdt_ts_out = float32(double(c1 + c2 + c4 + c8) / double(4 L)),
 *     gdt_ha_out likewise over (0.5, 1, 2, 4)
 *     rmsd_out float32 [U]: pesto_fit_rmsd on sel for fit and measure, bit for bit (its kernel)
 * A unit with a non-finite selected coordinate (the frame's or the reference's): NaN scores and fit, zero counts, seed -1. sel is
 * checked on the device before anything dereferences it; a refused call returns PESTO_ERR_INVALID and writes nothing. A wave per seed,
 * the workgroups of a unit sharing its seeds out, and a second launch for the maximum over the shares: no atomics, and no output depends
 * on the sharing, so every output is bit-identical from call to call and between a frame alone and in a batch. */
int pesto_tmscore(pesto_model* m, int64_t F, int64_t N, int32_t n_struct, const int32_t* sel_offsets, const int32_t* sel, const float* xyz_ref,
                  const float* xyz, const double* norm_len, const double* d0, int32_t step, int32_t n_iter, double scale, float* tm_out,
                  float* gdt_ts_out, float* gdt_ha_out, int32_t* counts_out, float* rmsd_out, int32_t* seed_out, double* rotation_out,
                  double* translation_out, int32_t ptr_kind, void* stream);

/* ---- pairwise sequence alignment, the alignment itself, and clustering by identity (pesto_align.hip) ----
 * Failures of the entry points below are reported through pesto_align_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the TM-score group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`.
 * replaces: what the package lacked between its dataset and its training - the sequence clusters that the reference's
 * processing/split_dataset.ipynb downloads (RCSB's bc-30.out) - and a residue correspondence for two files numbered differently.
 *
 * Definition (pesto_amd/sequences.py states it in full). S sequences of codes in [0, A) lie back to back in codes uint8
 * [seq_offsets[S]] (seq_offsets int32 [S + 1], HOST memory, from 0, 1 to PESTO_ALIGN_MAX_LENGTH codes each); matrix int8 [A, A] and pairs
 * int32 [P, 2] (a before b, indices in [0, S)) are HOST memory too; PESTO_ALIGN_MAX_GAP >= gap_open >= gap_extend >= 0; unknown: a code that
 * never counts as identical, or -1. For a of m codes against b of n, per cell (i, j) three int32 states,
 *     D[i][j] = matrix[a[i-1]][b[j-1]] + max(D, U, L)[i-1][j-1]                          (mode 2, local: max(D, U, L, 0), a fresh start)
 *     U[i][j] = max(D[i-1][j] - gap_open, U[i-1][j] - gap_extend, L[i-1][j] - gap_open)
 *     L[i][j] = max(D[i][j-1] - gap_open, U[i][j-1] - gap_open, L[i][j-1] - gap_extend)
 * THE FIRST IN THE ORDER D, U, L (then the fresh start) BEING THE PREDECESSOR ON TIES. mode 0, global: D[0][0] = 0, U[i][0] = L[0][i] =
 * -(gap_open + (i - 1) gap_extend), the end at (m, n) in the best of D, U, L in that order. mode 1, overlap: D = 0 on both borders, the
 * end the largest D over the cells with i = m or j = n, ties to the smallest i, then the smallest j. mode 2, local: the end the largest D
 * over i, j >= 1 with the same rule; no positive D: the empty alignment (all zero). Everything else on the borders is minus infinity.
 * The canonical alignment is the path from the end through those predecessors. Per pair, all int32:
 *     score_out [P]; n_ident_out [P]: its D columns with equal codes other than `unknown`; n_aligned_out [P]: its D columns; n_cols_out
 *     [P]: all its columns; span_out [P, 4] = (i0, j0, i1, j1), the half-open ranges of a and of b that it covers.
 * Every output is an integer that depends on nothing but the pair: bit-identical from call to call. The codes are checked on the device
 * (all below A) by a kernel whose verdict is read before anything is written; a refused call returns PESTO_ERR_INVALID. */
const char* pesto_align_last_error(void);

enum {
    PESTO_ALIGN_MAX_LENGTH = 4096,            /* codes of a sequence: 13 bits for each count a state carries */
    PESTO_ALIGN_MAX_ALPHABET = 32,            /* A */
    PESTO_ALIGN_MAX_GAP = 127,                /* gap_open: with int8 scores every sum stays far inside int32 */
    PESTO_ALIGN_MAX_SEQUENCES = 1 << 20,      /* S */
    PESTO_ALIGN_MAX_PAIRS = 0x7fffffff,       /* P */
    PESTO_ALIGN_MAX_MAP_PAIRS = 1 << 20,      /* P of the entry point that stores the alignments */
    PESTO_ALIGN_MAPS_WORKSPACE = 1 << 28      /* bytes of predecessor choices (one per cell) held at a time; the list is run in chunks */
};

/* The five outputs of P pairs without any cell matrix: one wave per pair, lanes on strips of 8 columns skewed by a row, every state
 * carrying its path's counts; O(m + n) memory per pair. pairs NULL: all i < j in row-major order (P = S (S - 1) / 2), decoded from a
 * linear index - no list is made. labels_out int32 [S] or NULL: when given, the wave of a pair (a, b) links the two sequences as soon as
 *     n_ident * 10000 >= id_bp * denom  and  n_aligned * 10000 >= cov_bp * max(m, n)      (64-bit integers; denom > 0)
 * with denom by `over`: 0 = min(m, n), 1 = n_aligned, 2 = n_cols, and labels_out numbers the connected components in the order of their
 * smallest members; the five per-pair outputs may then all be NULL. */
int pesto_align_scores(pesto_model* m, int32_t S, const int32_t* seq_offsets, const uint8_t* codes, int32_t A, const int8_t* matrix, int32_t mode,
                       int32_t gap_open, int32_t gap_extend, int32_t unknown, int64_t P, const int32_t* pairs, int32_t* score_out,
                       int32_t* n_ident_out, int32_t* n_aligned_out, int32_t* n_cols_out, int32_t* span_out, int32_t id_bp, int32_t cov_bp,
                       int32_t over, int32_t* labels_out, int32_t ptr_kind, void* stream);

/* The same five outputs and the alignment of 1 <= P <= PESTO_ALIGN_MAX_MAP_PAIRS listed pairs: map_out int32 [sum of m over the list], per
 * residue of a the index in b it is aligned to, -1 where it faces a gap or lies outside the span; pair p's rows follow pair p - 1's. The
 * recursion stores one byte per cell (the three predecessor choices), the path is walked back on the device, and the counts are those met
 * on the walk. */
int pesto_align_maps(pesto_model* m, int32_t S, const int32_t* seq_offsets, const uint8_t* codes, int32_t A, const int8_t* matrix, int32_t mode,
                     int32_t gap_open, int32_t gap_extend, int32_t unknown, int64_t P, const int32_t* pairs, int32_t* score_out, int32_t* n_ident_out,
                     int32_t* n_aligned_out, int32_t* n_cols_out, int32_t* span_out, int32_t* map_out, int32_t ptr_kind, void* stream);

/* ---- structure-based alignment of CA traces: the alignment and the superposition found together (pesto_structalign.hip) ----
 * Failures of the entry point below are reported through pesto_structalign_last_error() (thread-local message of the last failing call
 * of this group; an invalid handle's message is copied there too). Like the align group it uses the handle for its device, after
 * pesto_synchronize(m), allocates its buffers stream-ordered per call, keeps no state between calls and synchronises `stream`.
 * replaces: what the package lacked for two chains whose residue correspondence is not known (a homologue, the two halves of a
 * duplicated domain): outside the package, one run of a structure alignment program per pair. This is the library's OWN definition;
 * no equality with the TM-align program is claimed.
 *
 * Definition (pesto_amd/structalign.py states it too). xyz float32 [offsets[S], 3]: the CA coordinates of S structures back to back
 * (offsets int32 [S + 1], HOST memory, from 0; PESTO_STRUCTALIGN_MIN_LENGTH to PESTO_STRUCTALIGN_MAX_LENGTH residues each); pairs int32
 * [P, 2], HOST memory: a of m residues is moved onto b of n residues; codes uint8 [offsets[S]] or NULL: residue codes, used only to count
 * identities; init int32 [sum of m over the pairs] or NULL, HOST memory: the caller's initial map of every pair (-1, or indices of b that ascend);
 * d0 double [P, 3], HOST memory: d0s of the pair (customarily the TM-score d0 of Lmin = min(m, n)), then the d0 of m and of n; scale
 * turns coordinates into angstroms.
 *   Cell score under a transform (R, t), in double from the float32 inputs: x'_i = x_i R + t, u = |x'_i - y_j|^2 scale^2 / d0s^2,
 *     s_ij = int32(floor(Q / (1 + u) + 0.5)), Q = PESTO_STRUCTALIGN_Q.
 *   DP(R, t, g): the recursion, ties D, U, L, end rule and canonical path of the align group in mode 1 (overlap), with s_ij in the place of
 *     the matrix lookup, gap_open = g and gap_extend = 0: integer throughout. Its result is a map, its score and its n_aligned.
 *   Initial alignments. I1, gapless threading: every offset k (a_i on b_(i+k)) whose overlap has at least max(3, ceil(Lmin / 2)) residues:
 *     one fit (pesto_fit.h) of the overlap, the sum of s over the overlap under it; the largest sum wins, ties to the smallest k; the
 *     alignment is the overlap. I2, fragments of f = min(Lmin, max(4, min(20, Lmin / 3))) residues starting at 0, stride, 2 stride, ...
 *     <= len - f, plus len - f, stride = max(1, ceil((len - f) / (frag_starts - 1))): for every pair of fragments the fit of a's onto
 *     b's, and the score of DP(fit, 0) of the whole chains; the largest score wins, ties to the lowest (start in a, start in b); the
 *     alignment is the map of that DP. I3: init, if given.
 *   Units. A unit is (initial alignment i, gap g) with g = round(gap_open Q), then 0: unit 2 i + (g == 0), 4 or 6 per pair. A unit whose
 *     alignment has fewer than 3 pairs is dead. In each of `rounds` rounds a live unit (1) runs the TM-score search of the tmscore group
 *     on its aligned pairs (a's residues onto b's, norm_len = Lmin, d0 = d0s, step = max(1, n_aligned >> 3), n_iter 20): tm_r, R, t;
 *     (2) runs DP(R, t, its gap): the new map; (3) is done if the new map equals the old one, dead if it aligns fewer than 3 pairs.
 *   The pair's result is the alignment SEARCHED in the (unit, round) with the largest tm_r (float32), ties to the lowest (unit, round).
 * Outputs per pair: map_out int32 [sum of m]: the index in b or -1; n_aligned_out, n_ident_out (aligned pairs with equal codes; 0 without
 * codes), dp_score_out (the score of the winning round's DP), unit_out, round_out int32 [P]; tm_out float32 [P, 2]: the winning pairs
 * scored by the tmscore group at step 1, normalised by m with d0[1] and by n with d0[2], bit for bit what pesto_tmscore gives for them;
 * rotation_out double [P, 3, 3], translation_out double [P, 3]: those of the search normalised by the shorter chain (the first with m =
 * n); rmsd_out float32 [P]: over the aligned pairs, as pesto_tmscore reports it; history_out double [P, units, rounds, 3] = (tm_r, the
 * score of the round's DP, n_aligned of the alignment searched), NaN where a unit did not run.
 * No unit ever alive: tm 0, n_aligned 0, map -1, the identity transform, rmsd NaN, unit and round -1. A non-finite coordinate in either
 * chain: NaN scores and transform, map -1, unit -1. Every argument is checked on the host before any launch; a refused call returns
 * PESTO_ERR_INVALID and writes nothing. No atomics, and nothing depends on how the work is shared over workgroups: every output is
 * bit-identical from call to call and between host and device inputs. The host reads every unit's n_aligned and done flag once per
 * round (8 bytes a unit) to lay out the next round's ragged batch. */
const char* pesto_structalign_last_error(void);

enum {
    PESTO_STRUCTALIGN_Q = 1024,               /* the score of two residues in the same place */
    PESTO_STRUCTALIGN_MIN_LENGTH = 3,         /* residues of a chain: a superposition needs three points */
    PESTO_STRUCTALIGN_MAX_LENGTH = 4096,      /* ... and the TM search keeps 64 points a lane */
    PESTO_STRUCTALIGN_MAX_STRUCTURES = 1 << 20,
    PESTO_STRUCTALIGN_MAX_PAIRS = 1 << 20,    /* P */
    PESTO_STRUCTALIGN_MAX_ROUNDS = 64,
    PESTO_STRUCTALIGN_MIN_FRAG_STARTS = 2,
    PESTO_STRUCTALIGN_MAX_FRAG_STARTS = 64,
    PESTO_STRUCTALIGN_WORKSPACE = 1 << 28     /* bytes of predecessor choices (one per cell) held at a time; the units run in chunks */
};

int pesto_structalign(pesto_model* m, int32_t S, const int32_t* offsets, const float* xyz, const uint8_t* codes, int64_t P, const int32_t* pairs,
                      const int32_t* init, const double* d0, double gap_open, int32_t rounds, int32_t frag_starts, double scale, int32_t* map_out,
                      int32_t* n_aligned_out, int32_t* n_ident_out, int32_t* dp_score_out, int32_t* unit_out, int32_t* round_out, float* tm_out,
                      double* rotation_out, double* translation_out, float* rmsd_out, double* history_out, int32_t ptr_kind, void* stream);

/* ---- chain mapping of oligomers: which model chain lies on which reference chain ----
 * Failures of the entry point below are reported through pesto_chainmap_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the TM-score group it uses the handle for its device, after
 * pesto_synchronize(m), allocates its buffers stream-ordered per call, keeps no state between calls and synchronises `stream`.
 * replaces: what the package lacked between its sequence matching and its scorers - the chain mapping step of OpenStructure's
 * ChainMapper, of DockQ v2 and of MM-align / US-align, which pair the copies of an entity by structure before anything is scored. */
const char* pesto_chainmap_last_error(void);

enum {
    PESTO_CHAINMAP_MAX_FRAMES = 1 << 23,      /* frames of one call */
    PESTO_CHAINMAP_MAX_CHAINS = 64,           /* chains of a side */
    PESTO_CHAINMAP_MAX_GROUP = 12,            /* chains of one group on a side: the assignment's table has 2^12 doubles */
    PESTO_CHAINMAP_MAX_GROUPS = 128,          /* group ids lie in [0, 128) */
    PESTO_CHAINMAP_MAX_LENGTH = 4096,         /* slots of a chain */
    PESTO_CHAINMAP_MAX_ITER = 64,             /* n_iter */
    PESTO_CHAINMAP_WORKSPACE = 1 << 28        /* bytes of gathered slot lists held at a time: it caps the shares of a frame's seeds, and the frames run in chunks */
};

/* replaces: one run of a chain mapper per decoy. xyz_ref float32 [Nr,3]: the reference's Cr chains back to back (ref_offsets int32
 * [Cr + 1], ref_group int32 [Cr]); xyz float32 [F,Nm,3]: F models with the chain layout offsets int32 [Cm + 1], group int32 [Cm]. The
 * four int32 arrays live where ptr_kind says, like the coordinates. All chains of a group, on both sides, have the same number of
 * slots L_g (3 .. PESTO_CHAINMAP_MAX_LENGTH) and slot r is the same residue in each; a residue a chain lacks has NaN coordinates.
 * norm_len, d0: positive (customarily the reference's finite residues and the TM-score d0 of that number).
 * Definition, in double from the float32 inputs. Under a fit x' = (x - m) R + m_ref (pesto_fit.h, with its identity short cut) the pair
 * sum of reference chain a and model chain b of one group is s(a, b) = sum_r 1 / (1 + (d_r / d0)^2) over the slots finite in both,
 * d_r = |x'_{b,r} - y_{a,r}| scale. The assignment under a fit pairs, in every group, min(n_r, n_m) chains one to one so that the sum
 * of s is the exact maximum (ties: the lowest set of chains used on the larger side, read as a bit mask; then, from the last chain of
 * the smaller side backwards, the lowest chain of the larger side). total = the sum over the groups in ascending id.
 * Seeds: seed a Cm + b for every pair (a, b) of one group with at least 3 common finite slots; its first fit is that of chain b onto
 * chain a on those slots. A search makes up to n_iter fits: the assignment and total under the fit (the fit is visited); stop if the
 * mapping equals that of the seed's previous fit; else fit all common slots of the mapped pairs together (fewer than 3: stop).
 * Per frame f: score_out float32 = max total / norm_len over all visited fits; seed_out the lowest seed that attains it, round_out the
 * first visit of that seed that does; mapping_out int32 [F,Cr] the model chain under every reference chain at that fit or -1;
 * chain_score_out float32 [F,Cr] = s(a, mapping[a]) / (finite slots of a), 0 where unmapped; n_mapped_out int32; rotation_out double
 * [F,3,3] and translation_out double [F,3]: x' = x R + t. A frame with an infinite coordinate (on either side) or without a seed: score
 * and transform NaN, chain_score 0, mapping, seed and round -1, n_mapped 0.
 * The scalar arguments are checked on the host, and so are offsets and groups (device arrays, at most 65 ints each, are copied to the
 * host on `stream` first), before anything is launched: a refused call returns PESTO_ERR_INVALID, launches nothing and writes nothing.
 * No atomics on the results: every output is bit-identical from call to call, between host and device pointers and between a frame
 * alone and in a batch. */
int pesto_chainmap(pesto_model* m, int64_t F, int64_t Nr, int64_t Nm, int32_t Cr, int32_t Cm, const int32_t* ref_offsets, const int32_t* ref_group,
                   const int32_t* offsets, const int32_t* group, const float* xyz_ref, const float* xyz, double norm_len, double d0, int32_t n_iter,
                   double scale, float* score_out, int32_t* mapping_out, float* chain_score_out, int32_t* n_mapped_out, int32_t* seed_out,
                   int32_t* round_out, double* rotation_out, double* translation_out, int32_t ptr_kind, void* stream);

/* ---- QS-score and interface contact score of assemblies, for a given chain mapping or for the mapping that maximises it ----
 * Failures of the entry points below are reported through pesto_qsscore_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the chain mapping group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`.
 * replaces: what the package lacked beside lDDT, TM-score and DockQ - the interface score of an assembly (QS-score, Bertoni et al. 2017,
 * in the form OpenStructure states it; ICS as CASP's assembly category defines it) and the QS-optimal chain mapping that OpenStructure's
 * ChainMapper searches for, one decoy per run.
 *
 * The layout is that of the chain mapping group (one point per residue, customarily CB, CA for glycine; all chains of a group share the
 * slots of the group; a residue a chain lacks is NaN), with its limits PESTO_CHAINMAP_MAX_*; the four int32 layout arrays live where ptr_kind
 * says, like the coordinates, and are checked as the chain mapping group checks them, by the same code and before anything is launched
 * (device arrays are copied to the host on `stream` first; the job lists are made there too). Definition, in double from the float32 inputs:
 *     w(d) = 1 for d <= 5, exp(-2 ((d - 5) / 4.28)^2) for 5 < d < 12, 0 for d >= 12 (angstroms after scale)
 *     a mapping m[a] = the model chain under reference chain a or -1, one to one, within groups; interface (a, a'), a < a', is mapped if
 *     both are; a slot pair (r, s) of it is common if y[a,r], y[a',s], x[b,r], x[b',s] are finite (b = m[a], b' = m[a']);
 *     d1 = |y[a,r] - y[a',s]| scale, d2 = |x[b,r] - x[b',s]| scale. Summed over the common slot pairs of a mapped interface:
 *     num = w(min(d1,d2)) (1 - |d1 - d2| / 12) and shared = w(min(d1,d2)) where d1 < 12 and d2 < 12; extra = w of the one distance below
 *     12 where exactly one is; mref = w(d1) where d1 < 12; mmdl = w(d2) where d2 < 12; n_shared = the pairs with d1 and d2 < contact_thr.
 *     Wref (Wmdl[f]) = the sum of w over ALL chain pairs of the reference (of frame f) and their finite slot pairs; n_ref (n_model) = the
 *     pairs among them below contact_thr.
 *     qs_best = sum num / sum (shared + extra) over the mapped interfaces; qs_global = sum num / (sum (shared + extra) + (Wref - sum mref)
 *     + (Wmdl - sum mmdl)); interface_qs[a,a'] = num / (shared + extra) of one mapped interface; a denominator that is not positive: NaN.
 *     ics = 2 n_shared / (n_ref + n_model), precision = n_shared / n_model, recall = n_shared / n_ref; 0 / 0: NaN.
 * Sums run in one order (a lane's slot pairs, the wave's butterfly, the waves, the blocks of 64 slots, the interfaces in ascending
 * (a, a')); no atomics on results: every output is bit-identical from call to call, between host and device pointers and between a
 * frame alone and in a batch. A frame with an infinite coordinate (on either side): NaN scores, counts -1 (mapping -1, n_mapped 0,
 * index -1). */
const char* pesto_qsscore_last_error(void);

enum {
    PESTO_QSSCORE_MAX_MAPPINGS = 1 << 20,     /* mappings pesto_qsmap enumerates: the product over the groups of max! / (max - min)! */
    PESTO_QSSCORE_WORKSPACE = 1 << 28         /* bytes of chain-pair tables and block sums held at a time: the frames run in chunks */
};

/* replaces: one run of a QS-score scorer per decoy. mapping int32 [mapping_rows, Cr], mapping_rows 1 (one mapping for all frames) or F,
 * lives where ptr_kind says and is checked by a kernel (model chains in [-1, Cm), each at most once, of the reference chain's group)
 * whose verdict is read before anything is written. qs_best_out, qs_global_out, ics_out, precision_out, recall_out float32 [F], each
 * rounded once; counts_out int32 [F,3] = n_ref, n_model, n_shared (exact; saturating at INT32_MAX); interface_qs_out float32 [F,Cr,Cr],
 * symmetric, NaN on the diagonal and for interfaces that are not mapped. A refused call returns PESTO_ERR_INVALID and writes nothing. */
int pesto_qsscore(pesto_model* m, int64_t F, int64_t Nr, int64_t Nm, int32_t Cr, int32_t Cm, const int32_t* ref_offsets, const int32_t* ref_group,
                  const int32_t* offsets, const int32_t* group, const float* xyz_ref, const float* xyz, const int32_t* mapping, int64_t mapping_rows,
                  double contact_thr, double scale, float* qs_best_out, float* qs_global_out, float* ics_out, float* precision_out, float* recall_out,
                  int32_t* counts_out, float* interface_qs_out, int32_t ptr_kind, void* stream);

/* replaces: the search of a chain mapper for the QS-optimal mapping, one decoy per run. Every mapping that maps min(n_r, n_m) chains in
 * every group present on both sides is scored from one table of chain-pair terms per frame; their number must not exceed
 * PESTO_QSSCORE_MAX_MAPPINGS (PESTO_ERR_INVALID). mapping_out int32 [F,Cr] = the mapping of the largest qs_global (ties: the larger
 * qs_best, then the lowest index), n_mapped_out int32 [F], index_out int64 [F] its number in the enumeration: a mixed-radix number over
 * the groups present on both sides, the lowest group id the least significant digit; a group's digit is mixed-radix over the chains of
 * its side with fewer chains (the reference's on a tie), the first the least significant, and the digit q of the k-th of them, in
 * [0, max - k), picks the q-th still free chain of the other side in ascending order. The other outputs are those of pesto_qsscore for
 * that mapping, bit for bit. A frame where no mapping has a qs_global: mapping -1, n_mapped 0, index -1. */
int pesto_qsmap(pesto_model* m, int64_t F, int64_t Nr, int64_t Nm, int32_t Cr, int32_t Cm, const int32_t* ref_offsets, const int32_t* ref_group,
                const int32_t* offsets, const int32_t* group, const float* xyz_ref, const float* xyz, double contact_thr, double scale, int32_t* mapping_out,
                int32_t* n_mapped_out, int64_t* index_out, float* qs_best_out, float* qs_global_out, float* ics_out, float* precision_out, float* recall_out,
                int32_t* counts_out, float* interface_qs_out, int32_t ptr_kind, void* stream);

/* ---- essential dynamics of MD frames: fluctuations, covariance, cross-correlation, principal components (Amadei et al. 1993) ----
 * Failures of the entry points below are reported through pesto_dynamics_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the cluster group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`.
 *
 * Definition (this library's own; the reference has none). xyz float32 [F,N,3]; sel int32 [n_sel] atom indices or NULL for all atoms
 * (n_sel = N); x_f the selected coordinates of frame f flattened to m = 3 n_sel values. All arithmetic in double from the float32 inputs:
 *     mean = (1/F) sum_f x_f        d_f = (double)x_f - mean (centred BEFORE multiplying)
 *     C    = scale^2 sum_f d_f d_f^T / (F - ddof), ddof 0 or 1, F - ddof >= 1
 * Every sum runs in an order fixed by the shapes alone (no floating-point atomics): every output is bit-identical from call to call. */
const char* pesto_dynamics_last_error(void);

enum {
    PESTO_DYNAMICS_MAX_FRAMES = 1 << 24,      /* F */
    PESTO_DYNAMICS_MAX_ATOMS = 1 << 24,       /* N */
    PESTO_DYNAMICS_MAX_COV = 1 << 27,         /* (3 n_sel)^2 of pesto_covariance and pesto_cross_correlation: 1 GiB of doubles */
    PESTO_DYNAMICS_MAX_COMPONENTS = 32        /* n_components of pesto_pca: half the solver's block of 64 vectors */
};

/* mean_out float32 [n_sel,3] = float32(mean), in the input's unit (unscaled); rmsf_out float32 [n_sel] =
 * float32(scale sqrt((1/F) sum_f |d_f,i|^2)), each rounded once. */
int pesto_fluctuations(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double scale, float* mean_out,
                       float* rmsf_out, int32_t ptr_kind, void* stream);

/* C_out float64 [3 n_sel, 3 n_sel] = C. One 64 x 64 tile per workgroup on v_mfma_f64_16x16x4_f64, the frames staged through LDS and
 * centred while staged; only the tiles i <= j are computed and mirrored, so C is bitwise symmetric. (3 n_sel)^2 <= PESTO_DYNAMICS_MAX_COV.
 * Device scratch: 4 bytes per frame and selected coordinate. */
int pesto_covariance(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double scale, int32_t ddof, double* C_out,
                     int32_t ptr_kind, void* stream);

/* dccm_out float32 [n_sel,n_sel] = float32(tr C_ij / sqrt(tr C_ii tr C_jj)) over the 3 x 3 blocks of C (scale and ddof cancel), rounded
 * once: bitwise symmetric, exactly 1 on the diagonal, 0 off the diagonal for an atom with zero variance (never NaN). C itself is device
 * scratch, so (3 n_sel)^2 <= PESTO_DYNAMICS_MAX_COV. */
int pesto_cross_correlation(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, float* dccm_out, int32_t ptr_kind,
                            void* stream);

/* The k = n_components leading eigenpairs of C, 1 <= k <= min(PESTO_DYNAMICS_MAX_COMPONENTS, 3 n_sel), by block subspace iteration with
 * Rayleigh-Ritz on 64 vectors, matrix-free (C is never formed: Y = D^T (D Q) scale^2 / (F - ddof) per iteration; any F against 3 n_sel).
 * The start block is a fixed counter hash; every block is orthonormalised twice through its 64 x 64 Gram matrix; the 64 x 64 eigenproblems
 * are a one-sided Jacobi in one workgroup. At most max_iter >= 1 iterations; the done flag is read every fourth.
 *     eig_out float64 [k]: the Ritz values theta, descending, >= 0
 *     comp_out float64 [k,n_sel,3]: orthonormal rows; in each the entry of largest magnitude is positive (the lowest index on ties)
 *     proj_out float32 [F,k] = float32(scale d_f . v_i)
 *     mean_out float32 [n_sel,3] as pesto_fluctuations
 *     resid_out float64 [k] = |C v_i - theta_i v_i|_2 as the iteration measures it (Y V - Q V Theta)
 *     total_variance_out: one double in HOST memory, tr C
 *     info_out int32 [4] in HOST memory: rank, iterations, converged, and the most sweeps any of the call's 64 x 64 Jacobi runs took
 *         (a diagnostic: 60 is the cap)
 * A direction i < k with theta_i <= 1e-12 theta_0 is a null direction: eigenvalue 0, residual 0, an all-zero component row; rank counts
 * the others, rank <= min(k, F - 1, 3 n_sel). converged = (max_i resid_i <= tol theta_0), tol >= 0; it is reported, never an error. */
int pesto_pca(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, int32_t n_components, double scale, int32_t ddof,
              double tol, int32_t max_iter, double* eig_out, double* comp_out, float* proj_out, float* mean_out, double* resid_out,
              double* total_variance_out, int32_t* info_out, int32_t ptr_kind, void* stream);

/* proj_out float32 [F,k] = float32(scale ((double)x_f - (double)mean) . v_i) for a given basis: mean float32 [n_sel,3], components float64
 * [k,n_sel,3], 1 <= k <= 64 (neither orthonormality nor a sign is required). The product of pesto_pca's projections. */
int pesto_project(pesto_model* m, int64_t F, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, int32_t k, const float* mean,
                  const double* components, double scale, float* proj_out, int32_t ptr_kind, void* stream);

/* ---- elastic-network normal modes of one structure: ANM (Atilgan et al. 2001) and GNM (Bahar et al. 1997) ----
 * Failures of the entry points below are reported through pesto_enm_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the dynamics group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`.
 *
 * Definition (this library's own; no equality with another package is claimed). xyz float32 [N,3]; sel int32 [n_sel] node indices in
 * [0, N) or NULL for all (n_sel = N); an index outside the range or a non-finite selected coordinate refuses the call on the device's
 * verdict (PESTO_ERR_INVALID) before any output is written. The springs are the ordered pairs (i, j), i != j, of selected nodes with
 *     fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * fl32(scale) < fl32(cutoff)   (strict; the distance of the lDDT group)   and dist2 > 0
 * with the stiffness k_ij = gamma |r|^-p, r = scale ((double)x_j - (double)x_i), p 0 or 2, gamma > 0 and finite, cutoff and scale
 * positive float32 values. dim = 3 (ANM): the Hessian, double [3 n_sel, 3 n_sel], H_ij = -k_ij r r^T / |r|^2 for a spring, H_ii =
 * -sum_j H_ij in ascending j. dim = 1 (GNM): the Kirchhoff matrix, Gamma_ij = -k_ij, Gamma_ii = sum_j k_ij. b = 2 max_i sum_j k_ij
 * bounds both spectra (Gershgorin for Gamma; H <= Gamma (x) I_3 because u u^T <= I for every spring). Every sum runs in an order fixed
 * by the shapes and the list alone (no floating-point atomics): every output is bit-identical from call to call. */
const char* pesto_enm_last_error(void);

enum {
    PESTO_ENM_MAX_NODES = 1 << 24,            /* N; also the frames of pesto_enm_deform */
    PESTO_ENM_MAX_SPRINGS = 1 << 27,          /* list entries (ordered pairs) of one call */
    PESTO_ENM_MAX_DENSE = 1 << 27,            /* (dim n_sel)^2 of pesto_enm_matrix, n^2 of the correlation: 1 GiB of doubles */
    PESTO_ENM_MAX_MODES = 32                  /* n_modes of pesto_enm_modes: half the solver's block of 64 vectors */
};

/* The spring list as a CSR over the selected nodes in the selection's numbering: offsets_out int64 [n_sel + 1]; j_out int32 and k_out
 * float64 [capacity], row i = offsets[i] .. offsets[i + 1] holds node i's partners j ascending with k_ij. n_springs_out (one int64 in
 * HOST memory) = K, the list's entries (every spring twice); bound_out (one double in HOST memory) = b. j_out and k_out are filled
 * where K <= capacity (0 <= capacity <= PESTO_ENM_MAX_SPRINGS; with 0 they may be NULL): call once for K, once more with room for it.
 * The cell grid of the contact searches at cutoff / scale, a count pass, the 64-bit scan and a fill pass; a wave per row sorts it by
 * ranking every entry against the whole row: d^2 / 64 comparisons a wave for a row of d entries, milliseconds for a protein's rows of
 * some hundred, but quadratic: a dense cloud whose rows hold about n entries costs n^3 / 64 in all and is not what the limits promise
 * to be quick. R of the modes call is orthonormalised by ONE workgroup in some 40 reductions over the 3 n_sel coordinates: linear in
 * n_sel, about a millisecond per 10^5 nodes a reduction, so seconds near PESTO_ENM_MAX_NODES. */
int pesto_enm_network(pesto_model* m, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double cutoff, double scale, double gamma, int32_t p,
                      int64_t capacity, int64_t* offsets_out, int32_t* j_out, double* k_out, int64_t* n_springs_out, double* bound_out, int32_t ptr_kind,
                      void* stream);

/* out float64 [dim n_sel, dim n_sel]: the Hessian (dim 3) or the Kirchhoff matrix (dim 1), cleared and filled from the list; bitwise
 * symmetric, every diagonal 3 x 3 block included. (dim n_sel)^2 <= PESTO_ENM_MAX_DENSE. */
int pesto_enm_matrix(pesto_model* m, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double cutoff, double scale, double gamma, int32_t p,
                     int32_t dim, double* out, int32_t ptr_kind, void* stream);

/* The k = n_modes lowest eigenpairs of the Hessian (dim 3, n_sel >= 3, k <= min(PESTO_ENM_MAX_MODES, 3 n_sel - 6)) or of the Kirchhoff
 * matrix (dim 1, n_sel >= 2, k <= min(PESTO_ENM_MAX_MODES, n_sel - 1)) restricted to the complement of R, the rigid-body basis: three
 * translations and three rotations about the centroid, orthonormalised in double with null directions dropped (dim 1: the constant
 * vector). Matrix-free: the operator walks the list, one wave per node with the 64 vectors of the block across its lanes. Solver:
 * Chebyshev-filtered subspace iteration (Zhou and Saad 2007) on min(64, dim n_sel - rank R) vectors with Rayleigh-Ritz through the
 * 64 x 64 one-sided Jacobi and the Gram orthonormalisation of the dynamics group; the filter damps [largest Ritz value of the block, b],
 * is scaled against the lowest Ritz value, and has the degree (at most 4096) that gains 1e3 on the k-th mode; the rigid motions are
 * projected out of every product and once after every filter. A block that spans the whole complement needs one Rayleigh-Ritz step and
 * no filter. At most max_iter >= 1 Rayleigh-Ritz steps; the host reads the Ritz values after each.
 *     eig_out float64 [k]: ascending; a Ritz value <= 1e-10 b is a floppy direction and is reported as exactly 0 (its mode is kept)
 *     modes_out float64 [k, n_sel, dim]: orthonormal rows; in each the entry of largest magnitude is positive (the lowest index on ties)
 *     resid_out float64 [k] = |(I - R R^T) H v_i - theta_i v_i|_2 as the iteration measures it
 *     bound_out: one double in HOST memory, b;   n_springs_out: one int64 in HOST memory, K
 *     info_out int32 [6] in HOST memory: n_zero (the floppy directions among the k), iterations, converged, applies (operator
 *         applications on the block), the most sweeps any of the call's Jacobi runs took, rank R
 * converged = (max_i resid_i <= tol b), tol >= 0; it is reported, never an error. */
int pesto_enm_modes(pesto_model* m, int64_t N, int64_t n_sel, const float* xyz, const int32_t* sel, double cutoff, double scale, double gamma, int32_t p,
                    int32_t dim, int32_t n_modes, double tol, int32_t max_iter, double* eig_out, double* modes_out, double* resid_out, double* bound_out,
                    int64_t* n_springs_out, int32_t* info_out, int32_t ptr_kind, void* stream);

/* From k modes (eig float64 [k], modes float64 [k, n, dim], 1 <= k <= 64), the sums running over eig_k > 0 in ascending k:
 *     fluct_out float64 [n] = factor sum_k |v_k,i|^2 / eig_k                                              (NULL: not wanted)
 *     corr_out float32 [n, n] = C_ij / sqrt(C_ii C_jj), C_ij = sum_k (v_k,i . v_k,j) / eig_k, rounded once; bitwise symmetric, exactly 1
 *         on the diagonal, 0 (never NaN) for a node without fluctuation; n^2 <= PESTO_ENM_MAX_DENSE        (NULL: not wanted) */
int pesto_enm_fluctuations(pesto_model* m, int64_t k, int64_t n, int32_t dim, const double* eig, const double* modes, double factor, double* fluct_out,
                           float* corr_out, int32_t ptr_kind, void* stream);

/* overlap_out float64 [ka, kb] = |a_i . b_j| for modes_a float64 [ka, len] and modes_b float64 [kb, len], 1 <= ka, kb <= 64; with
 * normalise_b every b_j is divided by its length first (a displacement between two conformers; a zero one gives 0). */
int pesto_enm_overlap(pesto_model* m, int64_t ka, int64_t kb, int64_t len, const double* modes_a, const double* modes_b, int32_t normalise_b,
                      double* overlap_out, int32_t ptr_kind, void* stream);

/* xyz_out float32 [F, N, 3] = fl32((double)x_a + sum_k A[f,k] v_k[node_of_atom[a]]), the sum in ascending k, in double, rounded once:
 * xyz float32 [N,3], modes float64 [k, n, 3] (1 <= k <= 64), amplitudes float64 [F, k], node_of_atom int32 [N] with values in [0, n)
 * (checked on the device before anything is written) or NULL with n = N: atoms are nodes. F N 3 <= 2^36. */
int pesto_enm_deform(pesto_model* m, int64_t F, int64_t N, int64_t n, int64_t k, const float* xyz, const double* modes, const double* amplitudes,
                     const int32_t* node_of_atom, float* xyz_out, int32_t ptr_kind, void* stream);

/* ---- hydrogen bonds and periodic unwrapping (hydrogen_bonds and unwrap_pbc of md_analysis/mdtraj_utils/trajectory_utils.py) ----
 * Failures of the entry points below are reported through pesto_hbonds_last_error() (thread-local message of the last failing call of
 * this group; an invalid handle's message is copied there too). Like the docking group they use the handle for its device, after
 * pesto_synchronize(m), allocate their buffers stream-ordered per call, keep no state between calls and synchronise `stream`.
 *
 * Definition (md.baker_hubbard's documented criterion in this library's arithmetic). xyz float32 [F,N,3]; dh int32 [P,2], rows (donor
 * atom, hydrogen atom); acc int32 [A], the acceptor atoms; every index in [0, N), else PESTO_ERR_INVALID (checked on the device). The
 * candidates are the triplets (dh[p,0], dh[p,1], acc[a]) with acc[a] != dh[p,0], in the order p ascending, then a ascending. With H, D, A
 * the float32 coordinates of a triplet in a frame:
 *     d  = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * scale between H and A, as in the docking group, and d < r_thr (r_thr, scale: float32,
 *          positive and finite)
 *     u = D - H, v = A - H, c = (ux*vx + uy*vy) + uz*vz, uu and vv likewise, in double, every operation rounded as written, and
 *          c < 0 && c*c > cos2_angle * (uu*vv)      cos2_angle = cos(angle)^2 in [0, 1) for a D-H-A angle threshold in [90, 180) degrees
 * make the triplet bonded in that frame; a NaN, uu = 0 or vv = 0 does not. Every output is bit-identical from call to call. */
const char* pesto_hbonds_last_error(void);

enum {
    PESTO_HBONDS_MAX_FRAMES = 1 << 23,        /* a workgroup per frame and donor tile, below 2^32 threads per launch */
    PESTO_HBONDS_MAX_PAIRS = 0x7fffffff,      /* P * A, the candidates of one frame */
    PESTO_HBONDS_MAX_LIST = (1 << 30) - 1,    /* entries of one list */
    PESTO_HBONDS_DONOR_TILE = 32              /* donor pairs of one workgroup */
};

/* replaces: the frame loop of hydrogen_bonds (trajectory_utils.py:441-471; md.baker_hubbard restarted for every frame, then np.isin
 * filters in Python). P * A <= PESTO_HBONDS_MAX_PAIRS and F * ceil(P / 32) < 2^24. Frame f owns the rows offsets_out[f] .. offsets_out[f+1] of
 *     triplets_out int32 [cap,3]: the bonded (donor, hydrogen, acceptor) atoms of the frame in candidate order
 *     d_out float32 [cap]: their d
 *     offsets_out int64 [F+1]; sizes_out int64 [1] (HOST): K, the number of bonds of all frames
 * with the capacity protocol of pesto_frame_contacts (1 <= cap < 2^30): complete when K <= cap, otherwise only offsets_out and K are and
 * nothing beyond cap is written. group int8 [N] or NULL: when given, only triplets whose donor and acceptor atoms carry different
 * non-zero groups are listed (0: in neither subunit). A tiled brute-force search, count -> scan -> emit; no [P,A] array is stored. */
int pesto_frame_hbonds(pesto_model* m, int64_t F, int64_t N, int64_t P, int64_t A, const float* xyz, const int32_t* dh, const int32_t* acc,
                       const int8_t* group, float r_thr, float scale, double cos2_angle, int64_t cap, int64_t* offsets_out, int32_t* triplets_out,
                       float* d_out, int64_t* sizes_out, int32_t ptr_kind, void* stream);

/* replaces: md.baker_hubbard over a whole trajectory, which hydrogen_bonds (trajectory_utils.py:441-471) restarts for every frame. n[p,a]
 * is the number of frames in which candidate (p, a) is bonded; it is listed iff (double)n / (double)F > freq (strict; freq finite, >= 0).
 *     triplets_out int32 [cap,3]: the listed triplets in candidate order;   counts_out int32 [cap]: their n
 *     sizes_out int64 [1] (HOST): k, their number
 * with the same capacity protocol. A workgroup owns 32 donor pairs x 64 acceptors and loops over the frames with the counts in registers;
 * the scratch is one int32 per (donor pair, 64 acceptors). */
int pesto_hbond_occupancy(pesto_model* m, int64_t F, int64_t N, int64_t P, int64_t A, const float* xyz, const int32_t* dh, const int32_t* acc,
                          float r_thr, float scale, double cos2_angle, double freq, int64_t cap, int32_t* triplets_out, int32_t* counts_out,
                          int64_t* sizes_out, int32_t ptr_kind, void* stream);

/* replaces: unwrap_pbc (trajectory_utils.py:28-64; a Python loop over chains and their 27 periodic images, a copy of the trajectory).
 * xyz [F,N,3]; unitcell_lengths float32 [F,3]; perm int32 [N]: the atoms ordered by molecule, a permutation of [0, N) (an index outside
 * [0, N) or named twice: PESTO_ERR_INVALID, checked on the device before anything is read through it);
 * mol_off int32 [M+1] (HOST): molecule m holds perm[mol_off[m] .. mol_off[m+1]), none empty; masses float64 [N]. In double:
 *     com[f,m] = sum(mass x) / sum(mass) over the molecule, in a fixed order
 *     for m >= 1, image k = 0 .. 26 is dV[k] = (g[(k/3)%3], g[k/9], g[k%3]), g = (0, 1, -1): y slowest, then x, then z
 *     dist[k] = sqrt((tx*tx + ty*ty) + tz*tz), t = (com[f,m] + L[f] * dV[k]) - com[f,0], every operation rounded as written
 *     image_out int32 [F,M] = the first k of minimum dist (0 for molecule 0)
 *     xyz_out float32 [F,N,3] = fl32((double)x + (double)L[f,c] * dV[k][c]) for every atom of m; molecule 0 is copied
 * A NaN in com[f,m], com[f,0] or L[f] gives k = 0 and a copy of that molecule's frame. xyz is never modified. */
int pesto_unwrap_pbc(pesto_model* m, int64_t F, int64_t N, int64_t M, const float* xyz, const float* unitcell_lengths, const int32_t* perm,
                     const int32_t* mol_off, const double* masses, float* xyz_out, int32_t* image_out, int32_t ptr_kind, void* stream);

/* ---- solvent-accessible surface area (the reference's two uses of md.shrake_rupley) ----
 * replaces: wrapper_solvent_accessible_surface_area (interfaceome/solvent_accessible_surface_area.py:27-31, one structure at a time in a
 * two-process pool) and sasa (md_analysis/mdtraj_utils/trajectory_utils.py:428-438, a Python loop over the frames).
 * Failures are reported through pesto_sasa_last_error() (thread-local; an invalid handle's message is copied there too). Like the
 * trajectory group the entry point uses the handle for its device, allocates its buffers stream-ordered per call, keeps no state between
 * calls and synchronises `stream`; pointers are host or device memory according to ptr_kind, struct_offsets is always HOST memory.
 *
 * Definition. X float32 [F,n_total,3]; radius float32 [n_total], the atomic plus the probe radius; points float32 [P,3], the sphere
 * points (finite; unit vectors for a meaningful area); the atoms struct_offsets[s] .. struct_offsets[s+1] form structure s and only meet
 * each other. Every operation below is rounded to float32 on its own, as written, without fused multiply-adds:
 *     t[c]          = X[f,i,c] + (radius[i] * points[k,c])              c = x, y, z
 *     d[c]          = t[c] - X[f,j,c]
 *     q(f,i,k,j)    = (d.x*d.x + d.y*d.y) + d.z*d.z
 *     buried(f,i,k) = some j != i of i's structure with finite X[f,j] and radius[j] has  q < radius[j]*radius[j]
 *     count[f,i]    = number of k in [0, P) that are not buried
 *     area[f,i]     = float32(((c0 * count) * radius[i]) * radius[i])    evaluated in double; the caller passes c0 = 4 pi / P
 *     group[f,g]    = float32(sum of the double areas of the atoms perm[group_off[g] .. group_off[g+1]), in that order)
 * This is mdtraj's Shrake-Rupley algorithm made exact: count is an integer that depends neither on the order in which occluders are
 * visited, nor on the other structures of the launch, nor on the pruning (a cell grid per frame and structure and a distance test, both
 * widened by a margin that covers the float32 rounding of t and q - the argument is at the top of pesto_sasa.hip). A comparison with a
 * NaN is false: an atom with a non-finite coordinate or radius buries nothing and has count = P. Coincident atoms are no error (mdtraj
 * exits on them). mdtraj evaluates the area in float32; this one may differ from it by a couple of units in the last place.
 * Limits: 1 <= P <= PESTO_SASA_MAX_POINTS; 1 <= F * n_total < 2^31; n_struct >= 1 with strictly increasing offsets from 0 to n_total;
 * group sums need 1 <= n_groups, F * n_groups < 2^31. They are checked before any launch (PESTO_ERR_INVALID).
 *     counts_out int32 [F,n_total] or NULL, area_out float32 [F,n_total] or NULL, group_out float32 [F,n_groups] or NULL (then perm,
 *     group_off and n_groups are not read); at least one of the three. Every output is bit-identical from call to call. */
const char* pesto_sasa_last_error(void);

enum { PESTO_SASA_MAX_POINTS = 8192 };

int pesto_sasa(pesto_model* m, int64_t F, int64_t n_total, int32_t n_struct, const int32_t* struct_offsets, const float* X, const float* radius,
               int32_t P, const float* points, double c0, int32_t* counts_out, float* area_out, int32_t n_groups, const int32_t* perm,
               const int32_t* group_off, float* group_out, int32_t ptr_kind, void* stream);

/* ---- DSSP secondary structure (Kabsch & Sander 1983) ----
 * replaces: wrapper_secondary_structure (interfaceome/secondary_structures.py:27-31: md.compute_dssp(traj, simplified=False) on one
 * structure at a time in a 12-process pool). Every frame of a trajectory and every structure of a ragged batch goes through one launch
 * sequence. Failures are reported through pesto_dssp_last_error() (thread-local; an invalid handle's message is copied there too). Like
 * the other analysis groups the entry point uses the handle for its device, allocates its buffers stream-ordered per call, keeps no state
 * between calls and synchronises `stream`; X and the outputs are host or device memory according to ptr_kind; the topology tables (res_offsets, bb_atoms, proline, chain) are
 * always HOST memory, so their limits are checked before anything is launched.
 *
 * Inputs. X float32 [F,n_atoms,3]; scale multiplies the coordinates to angstroms (in double). The residues res_offsets[s] ..
 * res_offsets[s+1] of the R_total rows form structure s and only meet each other. bb_atoms int32 [R_total,4]: the rows of X that hold
 * the N, CA, C and O of every residue, -1 for a missing atom (such a residue gets PESTO_DSSP_NA and takes part in nothing). proline
 * uint8 [R_total]: 1 for a proline (no N-H). chain int32 [R_total]: residues of different chain numbers are never consecutive.
 * The definition - hydrogen placement, the electrostatic energy in thousandths of kcal/mol, the best-two selection, bridges, ladders and
 * their bulge links, helices, turns and bends, all in double as written, without fused multiply-adds - is the module docstring of
 * pesto_amd/dssp.py; pesto_dssp.hip restates it above its kernels. Every output is an integer that depends neither on the other
 * structures of the launch nor on the order of the threads: bit-identical from call to call.
 *     codes_out uint8 [F,R_total] or NULL: enum pesto_dssp_code
 *     partners_out int32 [F,R_total,4] or NULL: per residue its two best acceptors (as N-H donor) and its two best donors (as C=O
 *         acceptor), as residue indices WITHIN ITS STRUCTURE, best first, -1 for none
 *     energies_out int32 [F,R_total,4] or NULL: their energies in thousandths of kcal/mol (negative; 0 for none)
 * at least one of codes_out and the pair partners_out / energies_out (either of the pair may be NULL on its own).
 * Limits, checked before any launch (PESTO_ERR_INVALID): 1 <= F, 1 <= n_atoms, F * n_atoms < 2^31; 1 <= n_struct, strictly increasing
 * offsets from 0 to R_total, at most PESTO_DSSP_MAX_RESIDUES per structure, F * R_total < 2^31 and F * n_struct < 2^31; finite scale;
 * every atom row in -1 .. n_atoms - 1. */
const char* pesto_dssp_last_error(void);

enum { PESTO_DSSP_MAX_RESIDUES = 65535 };
enum pesto_dssp_code {
    PESTO_DSSP_BLANK = 0, PESTO_DSSP_H = 1, PESTO_DSSP_B = 2, PESTO_DSSP_E = 3, PESTO_DSSP_G = 4, PESTO_DSSP_I = 5, PESTO_DSSP_T = 6,
    PESTO_DSSP_S = 7, PESTO_DSSP_NA = 8
};

int pesto_dssp(pesto_model* m, int64_t F, int64_t n_atoms, const float* X, double scale, int64_t R_total, int32_t n_struct,
               const int32_t* res_offsets, const int32_t* bb_atoms, const uint8_t* proline, const int32_t* chain, uint8_t* codes_out,
               int32_t* partners_out, int32_t* energies_out, int32_t ptr_kind, void* stream);

/* ---- test hooks ----
 * Debug twins of the shipped kernels, selected per handle (the parity tests run every stage through each of them):
 * layer_kernels 0 = shipped (hybrid first layer; arithmetic per the precision policy), 1 = reference-formulation fp32 VALU
 * kernel (LDS-tiled, no MFMA);
 * knn_brute_force != 0: pesto_knn_collate searches every structure by brute force instead of the cell grid. */
int pesto_debug_select(pesto_model* m, int32_t layer_kernels, int32_t knn_brute_force);
/* work decomposition of the shipped state-update kernel: 0 = chosen per launch (default), 1 = rendezvous mode (every wave of a workgroup
 * processes centres, the finish / prepare phase runs behind workgroup rendezvous), 2 = node-wave mode (four waves of twelve only
 * finish / prepare). Both run the same arithmetic in the same order: results must not depend on the choice (tests force each). */
int pesto_debug_edge_mode(pesto_model* m, int32_t mode);

/* ---- per-stage entry points (HOST pointers), used by tests/ to pin each stage against the oracle ----
 * replaces: em.forward (model/model.py:34) */
int pesto_stage_embed(pesto_model* m, int64_t N, const float* q0, float* q_out /*[N,32]*/);
/* replaces: unpack_state_features (src/model_operations.py:6-22); outputs include the sink row 0 */
int pesto_stage_unpack(pesto_model* m, int64_t N, int32_t k, const float* X, const void* ids_topk, int32_t ids_kind,
                       float* D_out /*[N+1,k]*/, float* R_out /*[N+1,k,3]*/);
/* replaces: StateUpdateLayer.forward (src/model_operations.py:225-242) for layer `layer`, using the geometry
 * left by the last pesto_stage_unpack; q [N+1,32] and p [N+1,3,32] updated in place */
int pesto_stage_layer(pesto_model* m, int32_t layer, float* q_io, float* p_io);
/* replaces: StatePoolLayer.forward + decoder (src/model_operations.py:197-213, model/model.py:46-50);
 * q [N,32], p [N,3,32] WITHOUT the sink row */
int pesto_stage_pool(pesto_model* m, int64_t N, int64_t R, const float* q, const float* p, const int32_t* res_of_atom,
                     float* qr_out /*[R,32]*/, float* pr_out /*[R,3,32]*/, float* z_out /*[R,n_out]*/);

/* ---- training step (pesto_train.hip) ----
 * replaces: eval_step + loss.backward() + optimizer.step() (model/main.py:42-58, 186-200) with torch.optim.Adam at its defaults, all in
 * float32: the forward runs on the exact fp32 layer kernel and keeps the input state of every layer ((n_layers + 1) x (N + 1) x 128
 * floats), the backward recomputes each layer from its inputs as the reference's checkpoint does (src/model_operations.py:234-236).
 * A trainer is a handle of its own (weights in blob order, Adam's m and v, pos_ratios and the plain section of the weight image on the
 * device); failures are reported through pesto_train_last_error() (thread-local). em_depth / dm_depth = 1 is rejected.
 * Sums that several workgroups add to (weight gradients, the scatter-add of the gather) are accumulated with 64-bit fixed-point atomics
 * (40 fractional bits; terms clamped to +-4e6, sums wrap beyond +-2^23): they do not depend on the order of the workgroups, so the
 * same step gives the same bits on every run. */
typedef struct pesto_trainer pesto_trainer;
const char* pesto_train_last_error(void);
/* pos_ratios = 0.5, global_step = 0 (model/main.py:134-136) */
int pesto_train_create(const pesto_config* cfg, const float* weights, int64_t n_weights, int device, float lr, float pos_weight_factor,
                       pesto_trainer** out);
int pesto_train_destroy(pesto_trainer* t);
/* One collated batch with pesto_forward's semantics (the call's last atom as wrap target, the call-global max(D)).
 * mode 0: eval_step (main.py:42-58; pos_ratios updated, no gradient); 1: the same plus the gradient of sum(losses) with respect to
 * every parameter, handed out in blob order (grads_out, n_weights floats); 2: global_step += 1, then mode 1 and the Adam update.
 * y [R,C] float 0/1 with C == n_out; losses_out, p_out (= sigmoid(z)) and z_out [R,C] may be NULL. ids in [0, N], res_of_atom in [0, R)
 * with no empty residue: checked on the device BEFORE any other kernel runs (PESTO_ERR_INVALID; the trainer's state is untouched). */
int pesto_train_step(pesto_trainer* t, int32_t mode, int64_t N, int64_t R, int32_t k, int32_t C, const float* X, const void* ids_topk,
                     int32_t ids_kind, const float* q0, const int32_t* res_of_atom, const float* y, float* losses_out, float* p_out,
                     float* z_out, float* grads_out, int32_t ptr_kind, void* stream);
/* ---- the same forward and backward for a caller's own loss and optimiser (pesto_amd.nn: a torch Module over this handle) ----
 * replaces: model.parameters() handed to an optimiser that updates them in place (model/main.py:159, 200), load_state_dict (:150).
 * The weights are taken from a blob in pesto_amd.weights order (host or device pointer, n_weights floats) and the plain section of the
 * weight image is refreshed from it; Adam's m / v, pos_ratios and global_step are untouched. */
int pesto_train_set_weights(pesto_trainer* t, const float* blob, int32_t ptr_kind, void* stream);
/* replaces: z = model.forward(X, ids_topk, q, M) (model/main.py:46, model/model.py:32-52) without a loss: the argument check and the
 * kernels of pesto_train_step's forward half, so z_out [R,n_out] has its bits; pos_ratios and global_step are untouched.
 * keep != 0 keeps the input state of every layer for one pesto_train_backward and hands out a ticket (*ticket_out: 1, 2, ... per handle);
 * keep == 0 runs on two alternating states (ticket_out may be NULL). A handle has ONE workspace: every later forward, training step,
 * stage call or weight update ends the ticket. With device pointers X, q0 and res_of_atom must stay alive and unchanged until the
 * backward has run (it reads them again); host arrays are copied. */
int pesto_train_forward(pesto_trainer* t, int32_t keep, int64_t N, int64_t R, int32_t k, const float* X, const void* ids_topk, int32_t ids_kind,
                        const float* q0, const int32_t* res_of_atom, float* z_out, int64_t* ticket_out, int32_t ptr_kind, void* stream);
/* replaces: z.backward(dz) (model/main.py:196-199 with a caller's loss; X.requires_grad_() / q.requires_grad_() for the input gradients).
 * dz [R,n_out]; grads_out: the parameter gradients in blob order (n_weights floats); dq0_out [N,n0] and dX_out [N,3]; each of the three
 * may be NULL and is then not computed. A ticket that is not the handle's last kept forward fails with PESTO_ERR_INVALID: a gradient of
 * another forward is never produced. The call may be repeated on the same ticket (retain_graph) and gives the same bits.
 * dX is the backward of unpack_state_features (src/model_operations.py:8-14) under every layer's use of D and R (:109-116, 131-136):
 * d|r|/dr = 0 at r = 0 as in torch; the fix-up mask (D < 1e-2) is the forward's own decision; the gradient of max(D) is split evenly over
 * the maximal edges, which for one edge or the two directions of one pair equals any other rule - other exact ties of the maximum are
 * undefined in the reference's gradient as well. */
int pesto_train_backward(pesto_trainer* t, int64_t ticket, const float* dz, float* grads_out, float* dq0_out, float* dX_out, int32_t ptr_kind,
                         void* stream);
/* torch.optim.Adam.step() (betas 0.9 / 0.999, eps 1e-8, bias correction) with a gradient given in blob order (host pointer) */
int pesto_train_adam(pesto_trainer* t, const float* grads);
/* host copies of the trainer's state; a NULL argument is skipped */
int pesto_train_get_state(pesto_trainer* t, float* weights_out, float* pos_ratios_out /*[n_out]*/, int64_t* global_step, float* lr);
int pesto_train_set_state(pesto_trainer* t, const float* pos_ratios /*[n_out]*/, const int64_t* global_step, const float* lr);
/* HIP-event times of the last pesto_train_step (ms): forward + loss, backward, Adam; enabled != 0 makes the steps record them */
int pesto_train_set_timing(pesto_trainer* t, int32_t enabled);
int pesto_train_get_timing(pesto_trainer* t, double* ms_out /*[3]*/);
/* per-stage backward entry points (HOST pointers), used by tests/: gradients in blob order (n_weights floats, zero outside the stage)
 * replaces: the backward of em.forward (model/model.py:34); dq [N,32] */
int pesto_train_stage_embed(pesto_trainer* t, int64_t N, const float* q0, const float* dq, float* grads_out);
/* replaces: the backward of StateUpdateLayer.forward (src/model_operations.py:225-242) of layer `layer`: states and their gradients
 * [N+1,32] / [N+1,3,32] with the sink row, whose output gradient is multiplied by 0 (:239-240) */
int pesto_train_stage_layer(pesto_trainer* t, int32_t layer, int64_t N, int32_t k, const float* X, const void* ids_topk, int32_t ids_kind,
                            const float* q_in, const float* p_in, const float* dq_out, const float* dp_out, float* dq_in, float* dp_in,
                            float* grads_out);
/* replaces: the backward of StatePoolLayer.forward + decoder (src/model_operations.py:197-213, model/model.py:46-50); q [N,32],
 * p [N,3,32] without the sink row, dz [R,n_out] */
int pesto_train_stage_head(pesto_trainer* t, int64_t N, int64_t R, const float* q, const float* p, const int32_t* res_of_atom,
                           const float* dz, float* dq, float* dp, float* grads_out);

#ifdef __cplusplus
}
#endif
#endif /* PESTO_HIP_H */
