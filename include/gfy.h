/* gfy.h — C ABI of the MI355X (gfx950) GINE encode / embedding-distance library.
 *
 * This is the drop-in boundary for the hot path of nicoaira/GINFINITY.  The
 * reference has no FFI: its boundary is the Python seam
 *     Ginfinity._run_graph_shard(shard, embedding_dtype)      src/ginfinity/api.py:232-260
 * called from encode_graphs (api.py:227-228).  Every entry point below names
 * the reference lines it replaces.  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; all array arguments are DEVICE pointers unless the
 *     name ends in _host; the caller owns every buffer it passes in;
 *   - every function that launches work takes a hipStream_t as `void* stream`
 *     and only ENQUEUES: no hidden synchronisation, no allocation (graph-
 *     capturable); scratch memory is caller-provided (`workspace`), sized by
 *     the matching *_workspace_bytes query;
 *   - return value: 0 = GFY_OK, otherwise an error code; the message is kept
 *     per host thread and read with gfy_last_error().  The library never
 *     aborts.  (Python shim maps codes to ValueError / RuntimeError —
 *     reference error conventions: api.py:70-76,197-210.)
 *   - a gfy_encoder handle is not thread-safe ("a loaded instance is safe for
 *     serialized inference", docs/OPERATIONS.md:43-47).
 */
#ifndef GFY_H_
#define GFY_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFY_ABI_VERSION 4

enum gfy_status {
  GFY_OK = 0,
  GFY_ERR_INVALID = 1,     /* bad argument / malformed weight pack            */
  GFY_ERR_UNSUPPORTED = 2, /* architecture not compiled in (hidden != 128 …) */
  GFY_ERR_HIP = 3,         /* a HIP runtime call failed                       */
  GFY_ERR_WORKSPACE = 4    /* workspace too small                             */
};

enum gfy_dtype { GFY_F16 = 0, GFY_F32 = 1, GFY_F64 = 2 };

enum gfy_metric { GFY_L2 = 0, GFY_COSINE = 1 };

typedef struct gfy_encoder gfy_encoder;

/* Last error message of the calling host thread ("" if none). */
const char* gfy_last_error(void);
int gfy_abi_version(void);

/* ---- weight pack -----------------------------------------------------------
 * One little-endian blob: a 32-byte header followed by float32 tensors in
 * checkpoint order, row-major as torch stores them ([out_features][in_features]).
 *
 *   uint32 magic 'GFY1' (0x31594647), uint32 version (1), uint32 in_dim (7),
 *   uint32 hidden (128), uint32 layers (4), uint32 edge_dim (10),
 *   uint32 out_dim (128), uint32 flags (bit0 = residual)
 *   input.weight[hidden][in_dim]  input.bias[hidden]
 *   for l in 0..layers-1:
 *     convs.l.eps[1]
 *     convs.l.edge_lin.weight[hidden][edge_dim]  convs.l.edge_lin.bias[hidden]
 *     convs.l.mlp.0.weight[2h][h]  convs.l.mlp.0.bias[2h]
 *     convs.l.mlp.1.weight[2h] .bias[2h] .running_mean[2h] .running_var[2h]
 *     convs.l.mlp.4.weight[h][2h]  convs.l.mlp.4.bias[h]
 *     norms.l.weight[h]  norms.l.bias[h]
 *   head.0.weight[h][h] head.0.bias[h] head.2.weight[out][h] head.2.bias[out]
 * (reference: src/ginfinity/_model.py:29-63). */
size_t gfy_weight_pack_bytes(uint32_t in_dim, uint32_t hidden, uint32_t layers,
                             uint32_t edge_dim, uint32_t out_dim);

/* Build an encoder on HIP device `device` from a HOST weight pack.
 * model_dtype = GFY_F16 reproduces `model.half()` (api.py:111-112: parameters
 * and BatchNorm buffers rounded to fp16, fp16 activations with fp32 internals);
 * GFY_F32 is `full_precision=True`.  Replaces api.py:101-112 (module build,
 * .to(device), .half()).  Synchronous (uploads weights). */
int gfy_encoder_create(const void* weight_pack_host, size_t bytes,
                       int model_dtype, int device, gfy_encoder** out);
void gfy_encoder_destroy(gfy_encoder* encoder);

/* ---- records -> graph arrays (MI355X-side extension of the path's caller) ---------
 * GraphBuilder._build_full for every unsliced record of a micro-batch, concatenated as
 * GraphShard.from_graphs does (src/ginfinity/graph.py:494-561 — node features 496-514,
 * typed edges 516-546, pair table 737-747; concatenation 346-412).  Integer / one-hot
 * work, bit-identical to the reference's arrays including the edge order.
 *   bases, marks   uint8 [N]     the records' sequence / dot-bracket text, concatenated
 *                                (A C G U and ( . ) only — RNA.__post_init__ guarantees it)
 *   node_ptr       int64 [R+1]   record r owns nodes node_ptr[r]-node_ptr[0] ..
 *   edge_ptr       int64 [R+1]   and edges edge_ptr[r]-edge_ptr[0] ..; the caller computes
 *                                it: 2(L-1) + 2 pairs + (skip2 ? 2 max(L-2,0) : 0) per record
 *   struct_states  1: one "paired" flag (struct_feature "A"); 3: one-hot ( . )  ("B")
 *   positional     float32 [N][positional_columns] or NULL: the reference's host numpy
 *                  float32 sin/cos columns, copied into the feature rows unchanged
 *   node_features  float32 [N][4 + struct_states + positional_columns]   out
 *   edge_index     int32 [2][E], edge_types uint8 [E]                     out
 *   first_invalid  int32 [1] out: -1, or the first record whose text is not a balanced
 *                  structure over the alphabet, disagrees with edge_ptr, or nests deeper
 *                  than 2,048 levels (the reference caps records at 4,096 nt,
 *                  _validation.py MAXIMUM_LENGTH_NT); its rows are then unspecified,
 *                  nothing is written out of bounds.  No workspace.                 */
int gfy_build_graphs(const uint8_t* bases, const uint8_t* marks,
                     const int64_t* node_ptr, const int64_t* edge_ptr,
                     int64_t n_records, int64_t n_nodes, int64_t n_edges,
                     int struct_states, int positional_columns, int skip2,
                     const float* positional, float* node_features,
                     int32_t* edge_index, uint8_t* edge_types,
                     int32_t* first_invalid, void* stream);

/* ---- windowed (sliced) records -> graph arrays ---------------------------------------
 * GraphBuilder._slice_graph on top of _build_full (src/ginfinity/graph.py:608-695) for every
 * record of a list, WITHOUT building a window's whole molecule: the chosen positions of a
 * record (the window, and with keep_paired_neighbours the partners of its paired bases plus
 * context_hops - 1 further hops along the whole molecule's edges, stopping when a hop adds
 * nothing) are a 4,096-bit map per record, and every array follows from the map.  The arrays
 * are the reference's bit for bit: nodes ascending by position, the whole molecule's edges with
 * both ends chosen, in the whole molecule's order, renumbered to the new node ranks.  An
 * unsliced record is the window [0, L) and comes out as gfy_build_graphs writes it.
 *   bases, marks   uint8 [molecule_nt]  text of the DISTINCT molecules, concatenated: windows
 *                                       of one transcript share one copy and one pair table
 *   mol_ptr        int64 [M+1]          molecule m owns mol_ptr[m]-mol_ptr[0] .. ; 1..4,096 nt
 *   rec_mol, rec_start, rec_end  int32 [R]   record r is the window [start, end) of molecule
 *                                       rec_mol[r], 0 <= start < end <= its length
 * Two calls with ONE copy to the host between them, because node_ptr / edge_ptr (and so the
 * micro-batches) depend on how much context every window drew in:
 *   gfy_window_select   pair table of every molecule, then per record the chosen map into the
 *                       workspace and  counts int32 [R][2] = (nodes, edges)  out
 *   gfy_window_emit     records [first_record, first_record + batch_records) — one micro-batch —
 *                       from the maps the select call left in the SAME workspace:
 *     node_ptr, edge_ptr  int64 [batch_records+1]  prefix sums of the counts (any base: the
 *                         kernels subtract the first entry), n_nodes / n_edges their totals
 *     core_ptr       int64 [batch_records+1] prefix sums of end - start, n_core its total;
 *                    read only when out_rows is given
 *     struct_states, positional_columns, skip2   as for gfy_build_graphs
 *     positional     float32 [molecule_nt][positional_columns] or NULL: the reference's host
 *                    numpy sin/cos columns of the WHOLE molecules (a window keeps its
 *                    molecule's values)
 *     node_features  float32 [n_nodes][4 + struct_states + positional_columns]    out
 *     edge_index     int32 [2][n_edges], edge_types uint8 [n_edges]                  out
 *     residue_index  int32 [n_nodes] position in the molecule; node_roles uint8 [n_nodes]
 *                    0 = core (inside the window), 1 = context                     out
 *     out_rows       int32 [n_nodes] or NULL: row of the micro-batch's output for a core
 *                    node, -1 for a context node — the out_rows argument of the encode calls
 *   first_invalid  int32 [1] out of either call: -1, or the first record (index into the whole
 *                  list) that names no molecule, whose window leaves its molecule, whose
 *                  molecule is not 1..4,096 nt of balanced structure over the alphabet, or —
 *                  emit — whose node_ptr / edge_ptr / core_ptr entries disagree with its map.
 *                  Its counts are then 0 and its rows unspecified; every value read from the
 *                  inputs is range-checked and nothing is written out of bounds.
 *   workspace      gfy_window_workspace_bytes(); select writes it, emit reads it.  Returns
 *                  GFY_ERR_WORKSPACE when it is too small, GFY_ERR_INVALID for bad arguments. */
size_t gfy_window_workspace_bytes(int64_t n_molecules, int64_t molecule_nt, int64_t n_records);
int gfy_window_select(const uint8_t* bases, const uint8_t* marks, const int64_t* mol_ptr,
                      int64_t n_molecules, int64_t molecule_nt, const int32_t* rec_mol,
                      const int32_t* rec_start, const int32_t* rec_end, int64_t n_records,
                      int keep_paired_neighbours, int context_hops, int skip2,
                      int32_t* counts, int32_t* first_invalid, void* workspace,
                      size_t workspace_bytes, void* stream);
int gfy_window_emit(const uint8_t* bases, const uint8_t* marks, const int64_t* mol_ptr,
                    int64_t n_molecules, int64_t molecule_nt, const int32_t* rec_mol,
                    const int32_t* rec_start, const int32_t* rec_end, int64_t n_records,
                    int64_t first_record, int64_t batch_records, const int64_t* node_ptr,
                    const int64_t* edge_ptr, const int64_t* core_ptr, int64_t n_nodes,
                    int64_t n_edges, int64_t n_core, int struct_states,
                    int positional_columns, int skip2, const float* positional,
                    float* node_features, int32_t* edge_index, uint8_t* edge_types,
                    int32_t* residue_index, uint8_t* node_roles, int32_t* out_rows,
                    int32_t* first_invalid, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ---- COO -> CSR ------------------------------------------------------------
 * Destination-major CSR of a shard's edges, edges of one destination kept in
 * their COO order (a stable counting sort; integer work, bit-exact, run-to-run
 * deterministic).  Replaces the int64 widening + index_select/index_add_
 * addressing of api.py:239-242 and _model.py:41-45.
 *   edge_index  int32 [2][E]   row 0 = source, row 1 = destination (graph.py:306-308)
 *   edge_types  uint8 [E]
 *   row_ptr     int32 [N+1]    out
 *   col         int32 [E]      out: source node of each in-edge
 *   typ         uint8 [E]      out: edge type of each in-edge                */
/* Limit of the COO entry points (gfy_build_csr, gfy_encode_coo, gfy_encode_coo_batch): the node
 * count of a call, rounded up to whole 32-row tiles (a batch: the sum over its shards), must be
 * below 16,777,215 — GFY_ERR_UNSUPPORTED otherwise, before anything is launched.  (The counting
 * kernel keeps an edge's source row in 24 bits.)  gfy_encode with a caller-built CSR takes up to
 * 16,777,216 nodes.  The reference's micro-batches hold 60,000 (api.py:147-148). */
size_t gfy_csr_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int gfy_build_csr(const int32_t* edge_index, const uint8_t* edge_types,
                  int64_t n_nodes, int64_t n_edges, int32_t* row_ptr,
                  int32_t* col, uint8_t* typ, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ---- encode ------------------------------------------------------------------
 * GINEEncoder.forward (+ optional float64 L2 normalise) for one micro-batch:
 * input Linear, `layers` x (GINE message/aggregate/update, BatchNorm MLP,
 * LayerNorm, residual), 2-layer head.  Replaces api.py:237-252 and
 * _model.py:39-46,65-72.
 *   node_features float32 [N][in_dim]          (graph.py:302-305)
 *   (edge values are the caller's to validate, as GraphShard does: graph.py:318-323.  The device
 *   entry points never read outside the arrays for any VALUE in them: an edge whose source is
 *   outside [0, N) or whose type is >= edge_dim is IGNORED — it contributes no message —; the
 *   host entry point gfy_host_encode returns GFY_ERR_INVALID for such an edge)
 *   row_ptr/col/typ                            from gfy_build_csr
 *   out_rows      int32 [N] or NULL: output row of node i, -1 = drop the node
 *                 (context nodes of sliced graphs, api.py:253-260); NULL = i
 *   out           [n_out_rows][out_dim] of out_dtype (f16 / f32 / f64)
 *   normalise     1: out = o / max(||o||_2, 1e-12) computed in float64 and
 *                 rounded once to out_dtype (api.py:250-252,258-259);
 *                 0: raw head output o
 * Output dtypes of the fp16 model are separate code paths: out_dtype f16 runs head + normalise
 * inside the last layer launch, f32 / f64 run the stand-alone head kernel, and the two sum the
 * head's 128-deep dot products in different k orders (fp32 accumulation either way).  Each is
 * deterministic and within 1e-3 of the reference, but an f32 result rounded to fp16 is NOT
 * guaranteed to be the f16 call's bytes: fewer than 2e-3 of the elements differ, by at most
 * 2.5e-4 (tests/test_gpu_parity.py::test_fused_head_equals_standalone_head).                */
size_t gfy_encode_workspace_bytes(const gfy_encoder* encoder, int64_t n_nodes,
                                  int64_t n_edges);
int gfy_encode(gfy_encoder* encoder, const float* node_features,
               const int32_t* row_ptr, const int32_t* col, const uint8_t* typ,
               int64_t n_nodes, int64_t n_edges, const int32_t* out_rows,
               void* out, int out_dtype, int normalise, void* workspace,
               size_t workspace_bytes, void* stream);

/* The whole seam in one call: COO in, embeddings out — Ginfinity._run_graph_shard
 * (api.py:236-252) for one micro-batch.  Same result as gfy_build_csr + gfy_encode with fewer
 * launches: the last stage of the CSR build runs inside the encoder's setup launch and no
 * counter is zeroed per call (3 + layers launches instead of 6 + layers for the fp16 model).
 *   edge_index / edge_types   as for gfy_build_csr; the other arguments as for gfy_encode
 *   workspace                 gfy_encode_coo_workspace_bytes(); its first
 *                             gfy_encode_coo_clear_bytes(n_nodes) bytes must be ZERO when the
 *                             call starts and are zero again when it has run: clear a new
 *                             workspace once with gfy_encode_coo_prepare (or hipMemset the
 *                             whole of it) and again whenever n_nodes / n_edges change or
 *                             anything else has written to it.                             */
size_t gfy_encode_coo_workspace_bytes(const gfy_encoder* encoder, int64_t n_nodes,
                                      int64_t n_edges);
size_t gfy_encode_coo_clear_bytes(int64_t n_nodes);
int gfy_encode_coo_prepare(void* workspace, size_t workspace_bytes, int64_t n_nodes,
                           void* stream);
int gfy_encode_coo(gfy_encoder* encoder, const float* node_features,
                   const int32_t* edge_index, const uint8_t* edge_types, int64_t n_nodes,
                   int64_t n_edges, const int32_t* out_rows, void* out, int out_dtype,
                   int normalise, void* workspace, size_t workspace_bytes, void* stream);

/* A BATCH of shards in one sequence of launches: what encode_graphs does micro-batch after
 * micro-batch (api.py:211-230 calling _run_graph_shard, api.py:232-260) for up to
 * GFY_MAX_BATCH_SHARDS micro-batches at once.  Shards never share edges (graph.py:392-395), so the
 * kernels treat the batch as one graph in which every shard starts on a 32-row tile boundary; the
 * result of every shard is bit-identical to gfy_encode_coo on that shard alone (the per-node
 * arithmetic does not depend on what else is in the launch).  Why: a 60,000-node shard gives each
 * of the 256 CUs less than one round of tiles, so a launch is mostly ramp, fill and drain; a
 * batch runs the persistent-rounds layer kernel (GFY_OPT_LAYER_KERNEL) and pays those once.
 *   shards_host   HOST array of n_shards descriptors; the pointers in them are DEVICE pointers
 *                 with the meaning of the gfy_encode_coo arguments of the same name
 *   workspace     gfy_encode_coo_batch_workspace_bytes(); its first
 *                 gfy_encode_coo_batch_clear_bytes() bytes must be ZERO when the call starts and
 *                 are zero again when it has run (hipMemset once; again when the shards' sizes
 *                 change or anything else has written to it)                                  */
#define GFY_MAX_BATCH_SHARDS 16
typedef struct gfy_shard {
  const float* node_features;
  const int32_t* edge_index;
  const uint8_t* edge_types;
  const int32_t* out_rows;   /* or NULL */
  void* out;
  int64_t n_nodes, n_edges;
  /* Optional (ABI 4): the shard's record boundaries as GraphShard keeps them (graph.py:268-271),
   * DEVICE arrays of n_records + 1 ascending int64 — record r owns the nodes
   * [node_ptr[r] - node_ptr[0], node_ptr[r + 1] - node_ptr[0]) and the edges
   * [edge_ptr[r] - edge_ptr[0], ...) of this shard.  When EVERY shard of a call has them,
   * COO -> tile plans runs without global atomics (csrc/csr_records.inc: one launch instead of
   * two; a workgroup scans only the edges of the records that overlap its rows).  NULL / 0: the
   * counting kernel, as before.
   * PRECONDITION, the CALLER's to check: no edge leaves its record — both ends of every edge
   * lie in the node range of the record whose edge range holds it (what GraphShard.from_graphs
   * builds, graph.py:392-395; the kernel needs it of the destination).  The library does not
   * look: an edge whose destination lies in another record is not found by that record's
   * workgroups and is DROPPED without an error, unless both records happen to overlap one range
   * of rows.  Such an edge is legal input (the reference validates edges against the shard's
   * node range only, graph.py:318-321, and honours them): pass a shard that has one WITHOUT
   * boundaries.  gfy_pack_microbatch makes this check while it copies the edges and leaves the
   * boundaries out (counts[2] = 0); ginfinity_amd does the same wherever it attaches them
   * (engine.py, records_closed).  With the precondition met, results are identical either way.
   * Pass them only where a record's edge list is short against the shard (every workgroup of
   * a record reads the record's whole edge list).                                            */
  const int64_t* node_ptr;
  const int64_t* edge_ptr;
  int64_t n_records;
} gfy_shard;
size_t gfy_encode_coo_batch_workspace_bytes(const gfy_encoder* encoder,
                                            const gfy_shard* shards_host, int n_shards);
size_t gfy_encode_coo_batch_clear_bytes(const gfy_shard* shards_host, int n_shards);
int gfy_encode_coo_batch(gfy_encoder* encoder, const gfy_shard* shards_host, int n_shards,
                         int out_dtype, int normalise, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Debug/parity tap: copy the hidden state after `stage` into `out`
 * ([N][hidden] in the model dtype): stage 0 = input Linear, l+1 = after layer l.
 * Same arguments as gfy_encode; used by the stage-by-stage parity tests. */
int gfy_encode_hidden(gfy_encoder* encoder, const float* node_features,
                      const int32_t* row_ptr, const int32_t* col,
                      const uint8_t* typ, int64_t n_nodes, int64_t n_edges,
                      int stage, void* out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Debug/parity tap of ONE GINE layer (GINEConv + LayerNorm + residual, _model.py:39-46,69-71)
 * run on a GIVEN hidden state — e.g. the reference's own recorded tensor, so that every layer
 * and every phase is pinned by itself instead of through the layers before it:
 *   hidden_in  fp16 [N][hidden], natural channel order (h of the previous layer, or h0)
 *   tap        GFY_TAP_H: h' = R(h + y) [N][hidden];  GFY_TAP_Z: z = R(R(s h) + agg) after the
 *              gather;  GFY_TAP_V: v = relu(R(BN(u))) [N][2 hidden];  GFY_TAP_W: w = R(v W1^T + b1);
 *              GFY_TAP_Y: y = R(LayerNorm(w))
 *   out        fp16, natural channel order.  fp16 model with the residual architecture only;
 *              runs the persistent-rounds kernel's tap instantiation (same code otherwise).   */
enum gfy_layer_tap { GFY_TAP_H = 0, GFY_TAP_Z = 1, GFY_TAP_V = 2, GFY_TAP_W = 3, GFY_TAP_Y = 4 };
size_t gfy_debug_layer_workspace_bytes(const gfy_encoder* encoder, int64_t n_nodes,
                                       int64_t n_edges);
int gfy_debug_layer(gfy_encoder* encoder, int layer, const void* hidden_in,
                    const int32_t* row_ptr, const int32_t* col, const uint8_t* typ,
                    int64_t n_nodes, int64_t n_edges, int tap, void* out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* Per-kernel device timing of gfy_encode (diagnostics; bench.py's roofline
 * figure).  While enabled, gfy_encode brackets each kernel with hipEvents on the
 * caller's stream (do not enable under graph capture).  enable = 2 leaves out the
 * events BETWEEN layer launches 1 .. layers-1 and reports their mean: an event between
 * two dependent kernels adds ~2.5 us of stream time that a profiler's kernel duration
 * does not contain.  enable = 3 (fp16 model) records no events: every layer launch notes the
 * device clock of its first workgroup start and last workgroup end, and
 * gfy_encoder_get_timing returns those `layers` kernel durations (10 ns resolution) — what a
 * profiler reports, also when other streams' kernels run between two events of this stream.
 * gfy_encoder_get_timing
 * waits for the last gfy_encode and writes milliseconds to ms_host:
 * [0] per-encode setup (tile plans + input Linear), [1..layers] GINE layer
 * launches, [layers+1] stand-alone head+normalise (fp16-model fp16 output: the
 * last layer's launch runs the head too and this entry is ~0);
 * *count receives layers+2. */
int gfy_encoder_set_timing(gfy_encoder* encoder, int enable);
int gfy_encoder_get_timing(gfy_encoder* encoder, float* ms_host, int capacity,
                           int* count);

/* Diagnostic options of one encoder (no reference counterpart; results within the stated
 * tolerances for every setting).  Set between encodes, never read from the environment.
 *   GFY_OPT_SEPARATE_HEAD  1: head + normalise as its own launch even for fp16 output
 *   GFY_OPT_LAYER_KERNEL   -1 (default): by the launch — several rounds of tiles per CU (a batch,
 *                          a large micro-batch) run the windowed kernel (two 4-wave workgroups per
 *                          CU, weights streamed; edge_dim <= 12, else persistent rounds), one
 *                          round the one-round kernel whose last launch carries the head;
 *                          1 / 3 / 4 force one-round / persistent rounds / windowed
 *   GFY_OPT_STAGGER        rounds kernels: start offset between the workgroups of an XCD in
 *                          shader cycles; -1 (default): 500 (windowed: 250) from three rounds up
 *   GFY_OPT_PRIORITY       windowed kernel: s_setprio level of a CU's first (bits 1:0) / second
 *                          (bits 3:2) workgroup while it multiplies, of the second one elsewhere
 *                          (bits 5:4); -1 (default): 4                                            */
enum gfy_option { GFY_OPT_SEPARATE_HEAD = 2, GFY_OPT_LAYER_KERNEL = 3, GFY_OPT_STAGGER = 4,
                  GFY_OPT_PRIORITY = 6 };
int gfy_encoder_set_option(gfy_encoder* encoder, int option, int value);
/* Which layer kernel the encoder's last fp16-model encode launched (the values of
 * GFY_OPT_LAYER_KERNEL: 1 one round, 3 persistent rounds, 4 windowed; 0: none yet): lets a
 * caller — and the tests — see that a call took the batched path. */
int gfy_encoder_last_layer_kernel(const gfy_encoder* encoder);

/* ---- host (CPU) implementation --------------------------------------------------------
 * The reference's default device is the CPU (api.py:64-76: Ginfinity.load(device="cpu")); these
 * entry points serve it: the same rounding-point model in plain C++ (csrc/gine_host.cpp),
 * threads over node blocks, no HIP call.  For the drop-in surface on a box without a GPU
 * (BASELINE configs[0]) — not a fallback: a gfy_encoder never routes here.  ALL pointers are
 * HOST pointers; gfy_host_encode returns when the result is written.  Arguments as
 * gfy_encode_coo; `threads` <= 1 runs on the calling thread.                                */
typedef struct gfy_host_encoder gfy_host_encoder;
int gfy_host_encoder_create(const void* weight_pack_host, size_t bytes, int model_dtype,
                            gfy_host_encoder** out);
void gfy_host_encoder_destroy(gfy_host_encoder* encoder);
int gfy_host_encode(const gfy_host_encoder* encoder, const float* node_features,
                    const int32_t* edge_index, const uint8_t* edge_types, int64_t n_nodes,
                    int64_t n_edges, const int32_t* out_rows, void* out, int out_dtype,
                    int normalise, int threads);

/* ---- host-side packing of one micro-batch (no HIP call; exported by both libraries) ------
 * Records [start, stop) of a host shard -> one staging block, laid out as the device arrays of a
 * gfy_shard: what Ginfinity.encode_graphs does per micro-batch with GraphShard.slice
 * (api.py:211-230, graph.py:414-444: node rows cut, edge_index rebased by -node_ptr[start],
 * ptr arrays cut) plus the core-row map of api.py:253-257 — in ONE call that holds no
 * interpreter lock, so a pool of packer threads scales (the numpy form of it kept the packers of
 * 128 micro-batches behind one lock: 19-24 ms for 561 MB).
 *   slot + base      where the block starts (page-locked staging memory; base % 256 == 0)
 *   offsets[6]       out: byte offsets FROM `slot` of node_features, edge_index (2 x edges),
 *                    edge_types, out_rows (int32, -1 = dropped row; absent when every node is a
 *                    core node), node_ptr, edge_ptr (absent unless with_records, every
 *                    record has <= 65,536 edges and both ends of every edge lie in the node
 *                    range of the record whose edge range holds it: the precondition of
 *                    gfy_shard.node_ptr, checked here - an edge that joins two records of the
 *                    range is no error); -1 = absent; every array starts at a multiple of 256
 *   counts[4]        out: nodes, edges, records (0 = boundaries absent), kept rows
 * Returns GFY_ERR_INVALID (gfy_last_error: which) for an edge that leaves the records' node range
 * — the check of GraphShard.slice (graph.py:318-321).                                          */
int gfy_pack_microbatch(const float* node_features, int feature_dim, const int32_t* edge_index,
                        int64_t edges_total, const uint8_t* edge_types,
                        const uint8_t* node_roles, const int64_t* node_ptr,
                        const int64_t* edge_ptr, int64_t start, int64_t stop, int with_records,
                        void* slot, int64_t base, int64_t* offsets, int64_t* counts);

/* ---- one packed group of micro-batches -> the device (libgfy.so only) ---------------------
 * What follows gfy_pack_microbatch in the micro-batch loop of Ginfinity.encode_graphs
 * (api.py:211-230: `batch.to(device)`).  A gfy_upload_ring owns one event per staging slot of
 * its caller (`slots` of them, 1..64; made on the device that is current at creation).
 * gfy_upload_async: `bytes` of page-locked staging memory (slot `slot`) go up by ONE
 * asynchronous copy on `copy_stream`, and `consumer_stream` — the stream gfy_encode_coo_batch
 * of that group is issued on — waits for it; nothing blocks the host.  gfy_upload_wait returns
 * when the last upload from `slot` has left it, i.e. when a packer may write into it again (at
 * once if there was none).  One call per group instead of a copy, two event records, a stream
 * wait and a stream switch in the caller's interpreter (encode_shards_device: ~140 us of ~400
 * per group of the launching thread, which is what bounds a rank fed from host arrays).  A ring
 * is used by one thread at a time.                                                           */
typedef struct gfy_upload_ring gfy_upload_ring;
int gfy_upload_ring_create(int slots, gfy_upload_ring** ring_out);
void gfy_upload_ring_destroy(gfy_upload_ring* ring);
int gfy_upload_async(gfy_upload_ring* ring, int slot, void* device_dst, const void* pinned_src,
                     size_t bytes, void* copy_stream, void* consumer_stream);
int gfy_upload_wait(gfy_upload_ring* ring, int slot);

/* ---- all-pairs distance over 128-d embeddings ----------------------------------
 * No reference symbol (the aligner lives in the external `ginfinity-sw`;
 * only parameters are exported: api.py:47-50, data/alignment.json:6) — defined
 * here as D_ij = sqrt(max(|a_i|^2 + |b_j|^2 - 2 a_i.b_j, 0)) (GFY_L2) or
 * S_ij = a_i.b_j / (|a_i||b_j|) (GFY_COSINE); fp16 inputs, fp32 accumulation
 * on the matrix cores.
 *   a [n][128] fp16, b [m][128] fp16.                                           */

size_t gfy_pairwise_workspace_bytes(int64_t n, int64_t m);

/* Dense block: out float32 [n][m]  (small blocks only: n*m*4 bytes). */
int gfy_pairwise_dense(const void* a, int64_t n, const void* b, int64_t m,
                       int metric, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Fused row reduction, the N x M matrix is never materialised:
 *   best_val float32 [n], best_idx int32 [n]: nearest b-row of each a-row
 *   (smallest distance for GFY_L2, largest similarity for GFY_COSINE; ties ->
 *   lowest index).  exclude_offset >= 0 skips the pair (i, i + exclude_offset)
 *   — "self" when b is a with a row offset; -1 excludes nothing.
 *   An a-row whose every candidate is excluded (m = 1 and that row skipped; in
 *   gfy_pairwise_nearest_window a row whose only candidate is itself) gets
 *   best_idx = -1 and best_val = +inf (GFY_L2) / -inf (GFY_COSINE).            */
int gfy_pairwise_nearest(const void* a, int64_t n, const void* b, int64_t m,
                         int metric, int64_t exclude_offset, float* best_val,
                         int32_t* best_idx, void* workspace,
                         size_t workspace_bytes, void* stream);

/* The same when b IS the rows [window_first, window_first + m) of a (one rank's own piece in
 * the chunked cross-shard search): every a-row skips itself, i.e. the pair (window_first + j, j)
 * is excluded for every j — rows in front of the window, inside it and behind it in ONE call. */
int gfy_pairwise_nearest_window(const void* a, int64_t n, const void* b, int64_t m,
                                int metric, int64_t window_first, float* best_val,
                                int32_t* best_idx, void* workspace, size_t workspace_bytes,
                                void* stream);

/* Exact top-k, the N x M matrix is never materialised.  For every a-row the k best b-rows,
 * smallest distance first (GFY_L2) / largest similarity first (GFY_COSINE):
 *   top_val float32 [n][k], top_idx int32 [n][k], row-major.
 *   Order: by (the kernel's fp32 key of the pair, b-row index) — among equal keys the lowest
 *   index comes first; no index appears twice in a row.  The key is the one
 *   gfy_pairwise_nearest minimises, computed the same way, so column 0 is its answer bit for
 *   bit, the first j columns of a call with k >= j are the call with k = j bit for bit, and a
 *   row's result does not depend on which other rows the call holds.
 *   1 <= k <= GFY_PAIRWISE_TOPK_MAX; anything else is GFY_ERR_INVALID before any launch.
 *   exclude_offset as in gfy_pairwise_nearest, window_first as in gfy_pairwise_nearest_window:
 *   an excluded pair appears in no column.
 *   A row with fewer than k candidates (m < k, or one fewer after an exclusion) fills its
 *   trailing columns with top_idx = -1 and top_val = +inf (GFY_L2) / -inf (GFY_COSINE).
 *   The workspace has its own size, which grows with k.                                   */
#define GFY_PAIRWISE_TOPK_MAX 16
size_t gfy_pairwise_topk_workspace_bytes(int64_t n, int64_t m, int k);
int gfy_pairwise_topk(const void* a, int64_t n, const void* b, int64_t m, int metric, int k,
                      int64_t exclude_offset, float* top_val, int32_t* top_idx,
                      void* workspace, size_t workspace_bytes, void* stream);
int gfy_pairwise_topk_window(const void* a, int64_t n, const void* b, int64_t m, int metric,
                             int k, int64_t window_first, float* top_val, int32_t* top_idx,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The same with a half-open range of b-rows excluded per a-row — in a self-search over rows
 * grouped in records, each row's own record: the pair (i, j) is excluded iff
 * skip_lo[i] <= j < skip_hi[i].
 *   skip_lo, skip_hi int32 [n], device memory; NULL is GFY_ERR_INVALID before any launch.
 *   They may hold any value: lo >= hi excludes nothing, and bounds below 0 or above m are
 *   clipped by the comparison itself.  The ranges of different rows are independent: they need
 *   not be sorted, nested or disjoint, and a row's result depends neither on the other rows of
 *   the call nor on their ranges.
 *   Everything else — keys, order by (key, b-row index), no index twice, -1 and +inf / -inf
 *   behind the last candidate, the prefix property, the argument checks, the workspace and its
 *   size (gfy_pairwise_topk_workspace_bytes) — is that of gfy_pairwise_topk.  skip_lo[i] = i + c,
 *   skip_hi[i] = i + c + 1 is exclude_offset = c (window_first = -c) bit for bit.
 *   Cost: a workgroup (128 a-rows) takes the unchanged path in every b-tile that does not meet
 *   the union [min lo, max hi) of its rows' non-empty ranges, and masks in the tiles that do.
 *   Rows sorted by record in a self-search mask in the few tiles under their own records;
 *   arbitrary ranges may mask in every tile, which is correct and not meant to be fast.       */
int gfy_pairwise_topk_ranges(const void* a, int64_t n, const void* b, int64_t m, int metric, int k,
                             const int32_t* skip_lo, const int32_t* skip_hi,
                             float* top_val, int32_t* top_idx,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The same with at most one hit per record of b: the k best rows that lie in k DIFFERENT
 * records — in a library of records, the records that resemble a row instead of k neighbouring
 * rows of one of them.  b's rows are grouped in contiguous records; the record of b-row j is the
 * half-open range [group_lo[j], group_hi[j]).
 *   For every record R, its representative for a-row i is the non-excluded row of R that is
 *   first in the order (the kernel's fp32 key, then b-row index).  The result for a-row i is
 *   the k best representatives, ordered by (key, b-row index).  A record whose every row is
 *   excluded has no representative.  No two columns of a row lie in one record.
 *   skip_lo, skip_hi int32 [n] as in gfy_pairwise_topk_ranges (the single-pair exclusions are
 *   ranges of one row: skip_lo[i] = i + c, skip_hi[i] = i + c + 1; lo >= hi excludes nothing).
 *   group_lo, group_hi int32 [m], device memory.  Precondition: they describe a partition of
 *   [0, m) into contiguous ranges, group_lo[j] <= j < group_hi[j], the same pair for every row
 *   of a range (gfy_pairwise_topk_ranges' bounds of a self-search over records are such a pair).
 *   The values are only ever compared, never used as addresses: a violated precondition gives
 *   unspecified columns and never an access outside the caller's buffers.
 *   Keys, the value formulas, -1 with +inf / -inf behind the last candidate (a row with fewer
 *   than k records that have a representative), the prefix property, independence of the other
 *   rows of the call, the workspace and its size are those of gfy_pairwise_topk.  With every
 *   record one row long the result is that of gfy_pairwise_topk_ranges bit for bit.
 *   1 <= k <= GFY_PAIRWISE_TOPK_DISTINCT_MAX.  NULL pointers (a NULL group pointer is named as
 *   "group_lo or group_hi"), k, n, m, metric and a short workspace are refused before any
 *   launch, with the codes of gfy_pairwise_topk_ranges.                                        */
#define GFY_PAIRWISE_TOPK_DISTINCT_MAX 16
int gfy_pairwise_topk_distinct(const void* a, int64_t n, const void* b, int64_t m, int metric, int k,
                               const int32_t* skip_lo, const int32_t* skip_hi,
                               const int32_t* group_lo, const int32_t* group_hi,
                               float* top_val, int32_t* top_idx,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Record-to-record best-match scores: how well does record q of a match record r of b, for every
 * pair of records — the cheap, exact, dense ranking by which a caller decides which pairs of
 * records are worth aligning.  The N x M matrix is never materialised.
 *   The rows of b are grouped in records_b contiguous records and the rows of a in records_a:
 *   ptr_b int32 [records_b + 1] and ptr_a int32 [records_a + 1], device memory, are the running
 *   sums of the records' row counts (ptr[0] = 0, ascending, ptr_b[records_b] = m,
 *   ptr_a[records_a] = n); record r of b is the rows [ptr_b[r], ptr_b[r + 1]).  Counts of zero
 *   are allowed.
 *   The key and the value of a pair are those of gfy_pairwise_nearest / gfy_pairwise_topk,
 *   computed the same way (the folded start values for GFY_L2, the fma key form for GFY_COSINE,
 *   the same per-row terms, the same value formulas).
 *   Row level (gfy_pairwise_record_best): out_best float32 [n][records_b], row-major;
 *   best[i][r] is the value of the best pair (i, j) with j in record r — smallest distance
 *   (GFY_L2) / largest similarity (GFY_COSINE).  A record of zero rows gives +inf / -inf.
 *   Column r is gfy_pairwise_nearest(a, the rows of record r)'s best_val bit for bit.  (Only a
 *   zero keeps no promise of its sign: a maximum does not tell +0 from -0.)
 *   Record level (gfy_pairwise_record_scores): out_scores float32 [records_a][records_b];
 *   score[q][r] is the mean over the rows i of record q of best[i][r]: summed in float64 in
 *   ascending row order, divided by the record's row count, rounded to float32 once.  A record
 *   of a with zero rows gives a row of NaN; a record of b with zero rows gives +inf / -inf
 *   through the mean.  The score is directional (a onto b): the symmetric form is two calls.
 *   Nothing is excluded: in a self-search the pairs (i, i) are simply the best ones.
 *   An entry of best or of score depends neither on the other records and rows of the call nor
 *   on how the call is cut into workgroups and chunks, and is the same from run to run, bit for
 *   bit: per (a-row, record) the sweep keeps a maximum, which does not depend on the order of
 *   its operands (integer atomic max on an order-preserving image of the fp32 value), and the
 *   mean is summed in one fixed order without atomics.
 *   Workspace: gfy_pairwise_record_workspace_bytes(n, m, records_a, records_b), the same for both
 *   calls (records_a is ignored); it holds the row-level intermediate, n * records_b words, so
 *   a caller with many rows walks a in blocks of whole records, one call per block into the
 *   rows of one out_scores.  gfy_pairwise_record_chunks(n, m) tells into how many chunks a call
 *   of that shape cuts b (its own query: the split is a copy of the top-k launcher's today and
 *   need not stay one).
 *   Cost (by reasoning, not measured): the MFMA work of gfy_pairwise_nearest with a lighter
 *   epilogue, plus per (128 a-rows, record) at most one 64-lane atomic per wave that met the
 *   record — up to 8 against about 1.3 us of MFMA work for a record of 200 rows.  Records of one
 *   row each degrade to a dense write through atomics, which is correct and not meant to be fast.
 *   ptr_b is only compared and ptr_a clipped to [0, n]: arrays that are no running sums give
 *   unspecified values and no access outside the caller's buffers.
 *   A NULL pointer (named in gfy_last_error), n or m outside 1..2^31 - 2, records_b outside
 *   1..GFY_PAIRWISE_RECORDS_MAX, records_a < 1 and an unknown metric are GFY_ERR_INVALID, a short
 *   workspace is GFY_ERR_WORKSPACE; all of it before any launch and without a device.          */
#define GFY_PAIRWISE_RECORDS_MAX 2097120   /* 65,535 x 32: the grid of the transposing finish */
size_t gfy_pairwise_record_workspace_bytes(int64_t n, int64_t m, int64_t records_a,
                                           int64_t records_b);
int gfy_pairwise_record_chunks(int64_t n, int64_t m);
int gfy_pairwise_record_best(const void* a, int64_t n, const void* b, int64_t m, int metric,
                             const int32_t* ptr_b, int64_t records_b, float* out_best,
                             void* workspace, size_t workspace_bytes, void* stream);
int gfy_pairwise_record_scores(const void* a, int64_t n, const void* b, int64_t m, int metric,
                               const int32_t* ptr_a, int64_t records_a,
                               const int32_t* ptr_b, int64_t records_b, float* out_scores,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Radius search: for every a-row EVERY b-row that is at least as close as a threshold — a result
 * whose length varies per row, where top-k stops at k.  The N x M matrix is never materialised.
 *   The key and the value of a pair are those of gfy_pairwise_nearest / gfy_pairwise_topk,
 *   computed the same way (the folded start values for GFY_L2, the fma key form for GFY_COSINE,
 *   the same per-row terms, the same value formulas): value_ij is bit for bit what
 *   gfy_pairwise_topk reports for the pair.  threshold is a float32 and is compared in float32:
 *     GFY_L2      the pair (i, j) is a hit iff value_ij <= threshold
 *     GFY_COSINE  the pair (i, j) is a hit iff value_ij >= threshold
 *   So the hit set of a row depends neither on the other rows of the call nor on how the call
 *   is cut into blocks and chunks, is the same from run to run bit for bit, is for m <= 16 the
 *   entries of gfy_pairwise_topk(k = m) that pass the comparison with the same value bits, and
 *   is nested in a monotone threshold (raising a GFY_L2 threshold never loses a hit).
 *   skip_lo, skip_hi int32 [n], device memory, both or both NULL (none): the pair (i, j) is
 *   excluded iff skip_lo[i] <= j < skip_hi[i], with the meaning, the clipping and the cost of
 *   gfy_pairwise_topk_ranges.  An excluded pair is never a hit and never counted.  Padded rows
 *   of the ragged last tile are never hits.
 *   gfy_pairwise_within_count: counts int32 [n], the number of hits of every a-row.
 *   gfy_pairwise_within_fill: offsets int64 [n + 1], device memory — for a call with the same
 *   arguments the running sums of the counts (offsets[0] = 0, offsets[n] = the entries that
 *   indices and values hold).  Row i's hits go to [offsets[i], offsets[i + 1]) of indices int32
 *   and values float32, in ASCENDING b-row order, the value next to its index.  The fill never
 *   writes outside that segment whatever offsets holds: a segment is clipped to ascending order
 *   and to [0, offsets[n]], a hit that does not fit is dropped, and *status (int32, one word,
 *   device memory, zeroed by the call) is set non-zero — also when a row has fewer hits than
 *   its segment is long.  Stale or wrong offsets are a reported error, never a stray store; the
 *   entries of a segment longer than its row's hits are left as they were.
 *   Cost: two sweeps, each the MFMA work of gfy_pairwise_nearest at 128 a-rows per workgroup
 *   with a lighter epilogue (the count: one comparison per pair; the fill: one maximum per 16
 *   pairs and the stores of the hits), one integer atomic per wave and a-row; then one wave per
 *   a-row orders its segment — in registers up to 64 hits, in LDS up to 2,048, beyond that in
 *   place in global memory, which is correct and not meant to be fast.  Measured once
 *   (tools/bench_within.py, 262,144 x 262,144 unit rows, about 10 hits per row): the count 1.3 x
 *   the time of gfy_pairwise_nearest, count + offsets + fill + order 2.7 x; nothing else is.
 *   Workspace: gfy_pairwise_within_workspace_bytes(n, m), the same for both calls.
 *   gfy_pairwise_within_chunks(n, m) tells into how many chunks a call of that shape cuts b.
 *   The checks are those of gfy_pairwise_topk; besides, n above 2^31 - 2, a threshold that is
 *   not finite and one skip pointer without the other are GFY_ERR_INVALID before any launch.  */
size_t gfy_pairwise_within_workspace_bytes(int64_t n, int64_t m);
int gfy_pairwise_within_chunks(int64_t n, int64_t m);
int gfy_pairwise_within_count(const void* a, int64_t n, const void* b, int64_t m, int metric,
                              float threshold, const int32_t* skip_lo, const int32_t* skip_hi,
                              int32_t* counts, void* workspace, size_t workspace_bytes,
                              void* stream);
int gfy_pairwise_within_fill(const void* a, int64_t n, const void* b, int64_t m, int metric,
                             float threshold, const int32_t* skip_lo, const int32_t* skip_hi,
                             const int64_t* offsets, int32_t* indices, float* values,
                             int32_t* status, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Batched local alignment of record pairs: Smith-Waterman with affine gaps (Gotoh) over the
 * cosine of the records' rows, the step behind the ranking of gfy_pairwise_record_scores.  The
 * L_q x L_r matrix of a pair is never written to memory.
 *   No reference symbol: the reference delegates alignment to an external package that is not in
 *   its tree and holds parameter names without a formula.  The semantics are defined here; this
 *   is NOT that package, reproduces none of its scores, and none of the reference's alignment
 *   parameters maps onto an argument of this call.
 *   Rows of a ([n][128] fp16) are grouped in records_a contiguous records by ptr_a, rows of b in
 *   records_b by ptr_b (int32 running sums, device memory, as gfy_pairwise_record_scores takes
 *   them).  pairs int32 [P][2], device memory: pair p = (q, r) aligns A = the L_q rows of record
 *   q of a with B = the L_r rows of record r of b.
 *   Cosine      C[i][j] is gfy_pairwise_dense(A, B, GFY_COSINE)[i][j] bit for bit (the same
 *               multiply, key and value).
 *   Substitution  s[i][j] = fl32(fl32(C[i][j] * match_scale) + match_shift): two rounded fp32
 *               operations, never contracted.
 *   Recurrences, all fp32, every + and - one rounded operation, max exact:
 *               E[i][j] = max(E[i][j-1] - gap_extend, H[i][j-1] - gap_open)
 *               F[i][j] = max(F[i-1][j] - gap_extend, H[i-1][j] - gap_open)
 *               H[i][j] = max(0, H[i-1][j-1] + s[i][j], E[i][j], F[i][j])
 *               H = 0 and E = F = -inf outside the matrix; gap_open is the cost of a gap's first
 *               position.  A cell is a fixed expression of its three predecessors: the result
 *               depends neither on the schedule, nor on the other pairs of the call, nor on the
 *               run.
 *   Result      out_score[p] = max H; out_end[p] = (i, j), 0-based inside the two records, the
 *               first cell in the order (i ascending, then j ascending) with H == score.  A score
 *               of 0 (no positive cell, a record of zero rows) gives end = (-1, -1); only a zero
 *               keeps no promise of its sign.
 *   Limits      a record has at most GFY_ALIGN_ROWS_MAX rows; 0 <= gap_extend <= gap_open, the
 *               four parameters finite; 1 <= P < 2^31.  Rows holding inf / NaN give unspecified
 *               values.  The start cell is gfy_align_local_span's and the aligned path
 *               gfy_align_trace's; global and query-in-target alignment are gfy_align_global's;
 *               alignment inside a band of diagonals is gfy_align_local_band's; what a raw score
 *               means against shuffled targets is gfy_align_local_null's.
 *   Workspace   gfy_align_workspace_bytes(pairs, max_rows_b), max_rows_b the longest b-record any
 *               pair names: the last row of a 64-row strip of A, per wave in flight.
 *   ptr_a, ptr_b and pairs are device arrays, which the kernel only compares and clips.  A pair
 *   whose record index is out of range, or whose record is longer than GFY_ALIGN_ROWS_MAX, or
 *   whose b-record is longer than the max_rows_b the workspace holds, gets score = NaN and end =
 *   (-2, -2), and causes no access outside the caller's buffers.
 *   A NULL pointer (named in gfy_last_error), n or m outside 1..2^31 - 2, a record count outside
 *   1..2^31 - 2, P outside 1..2^31 - 1, a non-finite parameter and gap_extend outside
 *   [0, gap_open] are GFY_ERR_INVALID, a workspace shorter than gfy_align_workspace_bytes(P, 0)
 *   is GFY_ERR_WORKSPACE; all of it before any launch and without a device.
 *   Cost: not measured.                                                                       */
#define GFY_ALIGN_ROWS_MAX 4096
size_t gfy_align_workspace_bytes(int64_t pairs, int64_t max_rows_b);
int gfy_align_local(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                    const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                    const int32_t* pairs /* [P][2] device */, int64_t P,
                    float match_scale, float match_shift, float gap_open, float gap_extend,
                    float* out_score /* [P] */, int32_t* out_end /* [P][2] */,
                    void* workspace, size_t workspace_bytes, void* stream);

/* gfy_align_local with the START cell of every alignment: the stretch start..end of both records
 * is what takes part.  C, s, E, F, H, out_score and out_end are those of gfy_align_local, bit for
 * bit; the origin of the best path is carried through the same recurrences, so the L_q x L_r
 * matrix is still never written.
 *   Origins     every E, F and H that is > 0 has an origin (i0, j0), the first matched cell of
 *               the path that produced it:
 *               H[i][j]  the origin of the first candidate, in the order diagonal, then E, then
 *                        F, whose value equals H[i][j].  The diagonal candidate H[i-1][j-1] +
 *                        s[i][j] carries the origin of H[i-1][j-1] if that value is > 0, and
 *                        (i, j) itself otherwise (a predecessor that is 0 of either sign, or
 *                        outside the matrix: the alignment starts here).
 *               E[i][j]  the origin of H[i][j-1] if H[i][j-1] - gap_open >= E[i][j-1] -
 *                        gap_extend (opening wins a tie), else that of E[i][j-1].
 *               F[i][j]  the same rule with the row above.
 *               A value <= 0 has no origin; what is carried for it is unspecified and never
 *               reaches a positive H, since a positive E or F descends from a positive H.
 *   Result      out_start[p] = the origin of H at out_end[p]; (-1, -1) with a score of 0, (-2, -2)
 *               for a pair that is refused, as out_end.  An origin is a fixed function of the
 *               three predecessors: a pair's start depends neither on the other pairs of the call
 *               nor on the run, bit for bit.
 *   It follows  start <= end in both coordinates; s[start] == H[start] > 0; and the same
 *               recurrences run on the box start..end alone reach, at the box's last cell,
 *               exactly out_score, bit for bit (rounded addition and max are monotone and the
 *               path's own operations are unchanged).  gfy_align_trace only has to revisit
 *               that box.
 *   Workspace   gfy_align_span_workspace_bytes(pairs, max_rows_b): a strip's last row carries
 *               (H, F, origin of H, origin of F), 16 bytes per column, twice gfy_align_local's.
 *   Arguments, clipping of what the device arrays hold and error codes are those of
 *   gfy_align_local; a NULL out_start is GFY_ERR_INVALID and named.
 *   The aligned path itself is gfy_align_trace's; global alignment is gfy_align_global's; a band
 *   is gfy_align_local_span_band's; null scores are gfy_align_local_null's.                   */
size_t gfy_align_span_workspace_bytes(int64_t pairs, int64_t max_rows_b);
int gfy_align_local_span(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                         const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                         const int32_t* pairs /* [P][2] device */, int64_t P,
                         float match_scale, float match_shift, float gap_open, float gap_extend,
                         float* out_score /* [P] */, int32_t* out_start /* [P][2] */,
                         int32_t* out_end /* [P][2] */,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The aligned PATH of every pair: the walk back from out_end by the origin rules of
 * gfy_align_local_span, nothing new.  starts and ends (int32 [P][2], device memory) are what that
 * call returned for the same a, b, pairs and parameters.
 *   Walk        a state is H, E or F at a cell; the walk starts in H at end.
 *               H at (i, j)  if H == H[i-1][j-1] + s[i][j]: op 0 (row i of A matched with row j of
 *                            B); then, if H[i-1][j-1] > 0, on in H at (i-1, j-1), else stop (this
 *                            cell is start).  Else if H == E[i][j]: E at the same cell.  Else F at
 *                            the same cell.
 *               E at (i, j)  op 1 (row j of B faces a gap); on at (i, j-1), in H if H[i][j-1] -
 *                            gap_open >= E[i][j-1] - gap_extend (opening wins a tie), else in E.
 *               F at (i, j)  op 2 (row i of A faces a gap); on at (i-1, j) by the same rule with
 *                            the row above.
 *   Result      out_ops[op_ptr[p] ..]: the ops in FORWARD order, start to end, out_len[p] of them,
 *               one byte each.  The first and the last op are 0; the ops 0 and 2 number end_i -
 *               start_i + 1, the ops 0 and 1 end_j - start_j + 1; out_len <= rows + cols - 1 of
 *               the box.  A start of (-1, -1) (a score of 0) has out_len = 0.  Re-scoring the ops
 *               (h = 0; op 0: h = fl32(h + s[i][j]); the first op of a run of equal gap ops: g =
 *               fl32(h - gap_open), each further one g = fl32(g - gap_extend); after the run h =
 *               g) gives out_score bit for bit: a run that re-opens inside needs gap_open ==
 *               gap_extend, and then both readings round alike.
 *   The box     the kernel runs the recurrences on the box start..end ALONE (a-rows from start_i,
 *               b-rows from start_j), keeps 4 direction bits per cell and walks them.  That walk
 *               equals the walk on the full matrix.  By induction from start along the chosen
 *               path, every cell ON the path has the same H, E or F in both: its value is that
 *               of a candidate whose predecessor lies on the path and is equal by hypothesis (for
 *               start itself the predecessor is the 0 outside the box); every other candidate is
 *               formed in the box from values that are <= the full matrix's (rounded + and max
 *               are monotone, and what the box lacks counts as 0 or -inf, never more than what
 *               the matrix holds there), so it can only become smaller and the maximum stays.
 *               Every tie rule prefers the candidate on the path: a candidate that lost to it in
 *               the full matrix, strictly or by the rule, still loses when it shrinks.  So every
 *               direction bit the walk reads is the same, and so are the ops.
 *   The call also serves any box inside the two records: its result is then the walk of the
 *   recurrences on that box from the box's last cell (out_len = 0 where H there is not > 0).
 *   The walk emits at most rows + cols - 1 ops and stops on leaving the box.
 *   Slots       op_ptr int64 [P + 1], device memory: pair p owns out_ops[op_ptr[p] ..
 *               op_ptr[p + 1]), at least rows + cols - 1 bytes of it; the ops fill its front, the
 *               rest is left as it was.
 *   Workspace   gfy_align_trace_workspace_bytes(pairs, max_box_rows, max_box_cols): per wave of
 *               the full grid two carry buffers of max_box_cols entries and a region of max_box_rows
 *               x ceil(max_box_cols / 8) direction words (8 MB at 4096 x 4096) — the first thing
 *               proportional to L_q x L_r this library writes, for the box only.  The call takes
 *               the same max_box_rows and max_box_cols (they say how the workspace is cut; they
 *               come from starts and ends, which the caller has to read back to size the slots
 *               anyway).  Any workspace that holds one wave's part is accepted: as many waves as
 *               fit are used and take the pairs in turn, the others return at once.  A smaller
 *               one is GFY_ERR_WORKSPACE.
 *   Refused     out_len[p] = -2 and nothing written to the slot: a record index out of range or a
 *               record longer than GFY_ALIGN_ROWS_MAX (as gfy_align_local), a box not inside its
 *               records (start > end, end past the record, a negative start other than (-1, -1)),
 *               a box of more columns than max_box_cols or of more direction words than a wave's
 *               region, a slot shorter than rows + cols - 1.  starts, ends and the records are
 *               compared and clipped, never followed unchecked.
 *   Arguments and error codes are those of gfy_align_local, with out_ops and out_len in place of
 *   out_score and out_end; NULL starts, ends, op_ptr, out_ops or out_len is GFY_ERR_INVALID and
 *   named, and so is a negative max_box_rows or max_box_cols; all before any launch and without a
 *   device.
 *   Cost: DESIGN.md §4.                                                                       */
size_t gfy_align_trace_workspace_bytes(int64_t pairs, int64_t max_box_rows, int64_t max_box_cols);
int gfy_align_trace(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                    const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                    const int32_t* pairs /* [P][2] device */, int64_t P,
                    float match_scale, float match_shift, float gap_open, float gap_extend,
                    const int32_t* starts /* [P][2] */, const int32_t* ends /* [P][2] */,
                    const int64_t* op_ptr /* [P + 1] */, uint8_t* out_ops, int32_t* out_len /* [P] */,
                    int64_t max_box_rows, int64_t max_box_cols,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Local alignment INSIDE A BAND of diagonals per pair (seed and extend): gfy_align_local,
 * gfy_align_local_span and gfy_align_trace with `bands` (int32 [P][2], device memory) behind
 * gap_extend.  A seed hit (i, j) of a nearest-row search says on which diagonal j - i the common
 * stretch lies; a band around it asks for the best local alignment NEAR THAT SEED, which is
 * another question than the best one anywhere in the pair, and costs the band's cells only.
 *   Band        bands[p] = (lo, hi), lo <= hi: diagonals d = j - i in the coordinates of the two
 *               records, both ends inclusive.  THE BAND IS THE MATRIX: a cell whose diagonal lies
 *               outside [lo, hi] is outside the matrix in the sense of gfy_align_local, H = 0, E =
 *               F = -inf, no origin.  Nothing else changes: s[i][j], the recurrences, every
 *               rounded operation, the order that names out_end, the origin rules, the tie rules
 *               of the walk and the op codes are those of the calls without a band.
 *   It follows  - a band that covers the matrix (lo <= -(L_q - 1) and hi >= L_r - 1) gives the
 *                 results of the call without a band, bit for bit.
 *               - every operation is monotone and an outside cell holds the least values a cell
 *                 can have, so widening a band never lowers a pair's score, exactly, in fp32
 *                 comparison.
 *               - a band that meets no cell of the matrix gives score 0, start and end (-1, -1)
 *                 and out_len 0.
 *               - lo == hi is gapless extension along one diagonal.
 *               - the span property holds with the band shifted: the recurrences run on the box
 *                 start..end alone, under the band (lo - (start_j - start_i), hi - (start_j -
 *                 start_i)), reach exactly out_score at the box's last cell (the argument of
 *                 gfy_align_trace: what the box lacks counts as 0 or -inf, as what the band
 *                 lacks does).  The path is the walk inside that box; a path cell has a positive
 *                 value, so the walk never leaves the band.
 *               - re-scoring the ops gives out_score bit for bit, as without a band.
 *   Clipping    the kernel reads lo and hi per pair like the pair itself and clips them into
 *               [-GFY_ALIGN_ROWS_MAX, GFY_ALIGN_ROWS_MAX], which covers any matrix.  A pair with
 *               lo > hi is refused like a pair out of range: NaN, (-2, -2), out_len -2.
 *   Trace       gfy_align_trace_band takes the SAME bands as the span call, in the records'
 *               coordinates, and shifts each into its box itself.  A box whose last cell lies
 *               outside the band has out_len 0.
 *   Work        what lies outside the band is not done, not masked: of a 64-row strip from row
 *               i0, only the columns c_lo = max(0, i0 + lo) .. c_hi = min(L_r - 1, i0 + rows - 1 +
 *               hi) are loaded, multiplied and stepped over, c_hi - (c_lo & ~31) + rows steps
 *               against L_r + rows - 1, and a strip without a band cell is skipped (arithmetic
 *               from the loop bounds; no time is claimed).
 *   Workspace   the sizers, the cut and the acceptance of the calls without a band; the trace's
 *               region stays sized for the whole box.
 *   Arguments, checks and error codes are those of the counterpart; a NULL bands is
 *   GFY_ERR_INVALID, named, with a pointer to the call without a band.  Out of scope: a band on
 *   gfy_align_global and gfy_align_global_trace (borders that leave the band, pairs with no
 *   admissible path), band-only storage of the direction words.
 *   Cost: not measured.                                                                       */
int gfy_align_local_band(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                         const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                         const int32_t* pairs /* [P][2] device */, int64_t P,
                         float match_scale, float match_shift, float gap_open, float gap_extend,
                         const int32_t* bands /* [P][2] device */,
                         float* out_score /* [P] */, int32_t* out_end /* [P][2] */,
                         void* workspace, size_t workspace_bytes, void* stream);
int gfy_align_local_span_band(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                              const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                              const int32_t* pairs /* [P][2] device */, int64_t P,
                              float match_scale, float match_shift, float gap_open,
                              float gap_extend, const int32_t* bands /* [P][2] device */,
                              float* out_score /* [P] */, int32_t* out_start /* [P][2] */,
                              int32_t* out_end /* [P][2] */,
                              void* workspace, size_t workspace_bytes, void* stream);
int gfy_align_trace_band(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                         const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                         const int32_t* pairs /* [P][2] device */, int64_t P,
                         float match_scale, float match_shift, float gap_open, float gap_extend,
                         const int32_t* bands /* [P][2] device */,
                         const int32_t* starts /* [P][2] */, const int32_t* ends /* [P][2] */,
                         const int64_t* op_ptr /* [P + 1] */, uint8_t* out_ops,
                         int32_t* out_len /* [P] */, int64_t max_box_rows, int64_t max_box_cols,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Local alignment INSIDE A BOX of rows per pair: gfy_align_local_band and
 * gfy_align_local_span_band with `boxes` (int32 [P][4], device memory) behind `bands`.  A band
 * says on which diagonals a seed lies, not where on them: two conserved regions of one record
 * pair at the same offset share their band, and a banded call returns the stronger one for
 * both.  A box around each region gives each its own answer, and costs the box's strips only.
 *   Box         boxes[p] = (i_lo, i_hi, j_lo, j_hi), i_lo <= i_hi and j_lo <= j_hi: rows of the
 *               a-record and of the b-record, 0-based inside the two records, both ends
 *               inclusive.  THE BOX IS THE MATRIX, exactly as the band is: a cell outside the box
 *               is outside the matrix in the sense of gfy_align_local, H = 0, E = F = -inf, no
 *               origin.  Nothing else changes: s[i][j], the recurrences, every rounded operation,
 *               the order that names out_end, the origin rules, the tie rules of the walk and the
 *               op codes are those of the calls without a box.
 *   Band        bands keeps its meaning, diagonals d = j - i in the RECORDS' coordinates, and
 *               combines with the box by intersection.  bands may be NULL: no band.
 *   Results     out_start and out_end stay in the records' coordinates.
 *   Clipping    the kernel reads the four values per pair like the band, clips them into
 *               [-GFY_ALIGN_ROWS_MAX, GFY_ALIGN_ROWS_MAX] and then into the two records.  A box
 *               that holds no cell after clipping gives what a band that meets no cell gives:
 *               score 0, start and end (-1, -1).  A pair with i_lo > i_hi or j_lo > j_hi as given
 *               is refused like a band with lo > hi: NaN and (-2, -2).
 *   It follows  - a box that covers both records gives the results of the call without a box,
 *                 bit for bit.
 *               - a boxed call equals, bit for bit, the call without a box on rows i_lo..i_hi of
 *                 A and j_lo..j_hi of B taken as two records of their own, under the band (lo -
 *                 (j_lo - i_lo), hi - (j_lo - i_lo)), with (i_lo, j_lo) added to its cells (the
 *                 clipped box's i_lo and j_lo).  That is how the kernel does it.
 *               - every operation is monotone and an outside cell holds the least values a cell
 *                 can have, so enlarging a box never lowers a pair's score, exactly, in fp32
 *                 comparison.
 *               - re-scoring the ops gives out_score bit for bit.
 *               - a pair's result depends neither on the other pairs of the call nor on the run.
 *   Trace       there is no boxed trace call and none is needed.  The span property holds inside
 *               the box as it does inside the band: what the box lacks counts as 0 or -inf, so
 *               the recurrences on start..end alone reach out_score at end.  start..end lies
 *               inside the caller's box, so every cell of start..end is a cell of the boxed
 *               matrix, and gfy_align_trace_band (gfy_align_trace where bands is NULL) on
 *               start..end, with the band in the records' coordinates, walks the same path.
 *   Work        the strips follow the box, not the record: ceil(box rows / 64) strips of at most
 *               box columns + 63 steps, the first at the box's first row.  A 150-row chain
 *               with a margin of 16 in two 4,096-row records under a band of 9 diagonals: a box
 *               of 182 rows, 3 strips (4 from a margin of 22 on) against the 64 strips of the
 *               a-record that the band meets (arithmetic from the loop bounds; no time is
 *               claimed).
 *   Workspace   the sizers of the calls without a box, gfy_align_workspace_bytes and
 *               gfy_align_span_workspace_bytes, with the widest box's columns (after clipping)
 *               for max_rows_b; a pair whose box has more columns than the workspace holds is
 *               refused: NaN and (-2, -2).
 *   Arguments, checks and error codes are those of the banded counterpart but for bands; a NULL
 *   boxes is GFY_ERR_INVALID, named, with a pointer to the call without a box.  A box on the
 *   global modes is gfy_align_global_box's.  Out of scope: band-only or box-only storage of the
 *   direction words, boxes that are not rectangles.
 *   Cost: DESIGN.md §4.                                                                        */
int gfy_align_local_box(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                        const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                        const int32_t* pairs /* [P][2] device */, int64_t P,
                        float match_scale, float match_shift, float gap_open, float gap_extend,
                        const int32_t* bands /* [P][2] device, or NULL */,
                        const int32_t* boxes /* [P][4] device */,
                        float* out_score /* [P] */, int32_t* out_end /* [P][2] */,
                        void* workspace, size_t workspace_bytes, void* stream);
int gfy_align_local_span_box(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                             const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                             const int32_t* pairs /* [P][2] device */, int64_t P,
                             float match_scale, float match_shift, float gap_open,
                             float gap_extend, const int32_t* bands /* [P][2] device, or NULL */,
                             const int32_t* boxes /* [P][4] device */,
                             float* out_score /* [P] */, int32_t* out_start /* [P][2] */,
                             int32_t* out_end /* [P][2] */,
                             void* workspace, size_t workspace_bytes, void* stream);

/* NULL SCORES of local alignment: every pair aligned `shuffles` times against its own b-side with
 * the rows in another order each time, in one launch and without writing a shuffled row.  A raw
 * local score grows with the two lengths and depends on the four parameters and on how ordinary
 * the two records' rows are; there is no scoring matrix here to look a lambda and a K up for.
 * The answer is empirical: the real score against the scores of the same pair with the target's
 * rows in random order.  The arguments are gfy_align_local_box's with `shuffles`, `order` and
 * `order_ptr` behind `boxes`, and without out_end.
 *   B-side      of pair p: the rows of its b-record, or with a box rows j_lo .. j_hi of it after
 *               clipping (gfy_align_local_box).  It has columns_p rows, whatever the a-side holds.
 *   Orders      order is int32, order_ptr int64 [P + 1], both in device memory.  The `shuffles`
 *               orders of pair p lie back to back from order[order_ptr[p]] on, columns_p entries
 *               each.  In run k COLUMN j OF THE PAIR'S MATRIX HOLDS ROW order[order_ptr[p] + k *
 *               columns_p + j] OF THE B-SIDE; entries are relative to the b-side, 0 .. columns_p -
 *               1.  Nothing else changes: the a-side, s[i][j] (the cosine of row i with the row
 *               that the column holds, its 1/|b| taken from that row), the recurrences, every
 *               rounded operation, the band (diagonals of the matrix as it stands, in the records'
 *               coordinates) and the box.  Entries need not be a permutation: repeats are legal
 *               (a bootstrap of the target's rows).
 *   Result      out_score[p][k], [P][shuffles] row-major, the local score of run k.  There is no
 *               end: a cell of a shuffled matrix names no row of the record.
 *   Identity    out_score[p][k] equals, bit for bit, gfy_align_local (or _band / _box) of the pair
 *               with the b-side replaced by the rows order[...] copied out in that order.  A cell
 *               is a fixed expression of its predecessors, and a cosine is a fixed function of
 *               its two rows.  The order 0, 1, .. columns_p - 1 gives gfy_align_local_box's score.
 *   bands, boxes  each may be NULL: the covering band, the covering box.  Band, box, both or
 *               neither are one kernel.
 *   Refusals    order and order_ptr are device arrays, which the kernel only compares and clips,
 *               as it does pairs.  A pair with order_ptr[p] < 0 or order_ptr[p + 1] - order_ptr[p]
 *               != shuffles * columns_p gets NaN in all its runs; a run with an entry outside 0 ..
 *               columns_p - 1 gets NaN, and the other runs are not affected; a pair that
 *               gfy_align_local_box refuses gets NaN in all its runs.  The range test comes before
 *               an entry becomes an address: a refused run causes no access outside the caller's
 *               buffers.  (order_ptr is trusted to lie inside order, as op_ptr is inside out_ops.)
 *   Workspace   gfy_align_workspace_bytes(P * shuffles, max columns_p): the launch runs over the
 *               virtual pairs v = p * shuffles + k, one wave each, by the grid and carry rules of
 *               the score calls.
 *   Orders for a null: ginfinity_amd.align.shuffle_orders makes them, a fixed function of (seed,
 *               v, j) that anything with 64-bit integers reproduces.  With mix(z): z ^= z >> 30;
 *               z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 (all
 *               modulo 2^64, >> logical) and G = 0x9E3779B97F4A7C15,
 *                   key(seed, v, j) = mix(mix(seed + (v + 1) * G) + (j + 1) * G) >> 32,
 *               and the order of virtual pair v is 0 .. columns - 1 sorted by (key, j).
 *   What the scores become (z-score, Gumbel fit, p-value) is host arithmetic on [P][shuffles]
 *   numbers: ginfinity_amd.align.significance states its formulas.
 *   A NULL a, b, ptr_a, ptr_b, pairs, order, order_ptr, out_score or workspace (named in
 *   gfy_last_error), shuffles < 1, P * shuffles outside 1..2^31 - 1 and what gfy_align_local
 *   refuses are GFY_ERR_INVALID, a workspace shorter than gfy_align_workspace_bytes(P * shuffles,
 *   0) is GFY_ERR_WORKSPACE; all of it before any launch and without a device.  Out of scope:
 *   nulls for the global and query-in-target modes, orders of the a-side, start, end or path of a
 *   run, an E-value calibrated over a whole database search.
 *   Cost: DESIGN.md §4.                                                                        */
int gfy_align_local_null(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                         const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                         const int32_t* pairs /* [P][2] device */, int64_t P,
                         float match_scale, float match_shift, float gap_open, float gap_extend,
                         const int32_t* bands /* [P][2] device, or NULL */,
                         const int32_t* boxes /* [P][4] device, or NULL */,
                         int64_t shuffles, const int32_t* order /* device */,
                         const int64_t* order_ptr /* [P + 1] device */,
                         float* out_score /* [P][shuffles] */,
                         void* workspace, size_t workspace_bytes, void* stream);

/* GLOBAL and QUERY-IN-TARGET alignment of record pairs: the recurrences of gfy_align_local with
 * charged borders and without the 0 candidate.  within = 0 aligns both records end to end
 * (Needleman-Wunsch with affine gaps): unrelated flanks are charged for, not ignored.  within = 1
 * aligns ALL of the a-record inside the b-record ("fit"): the b-record's rows in front of and
 * behind the alignment are free, so a window cannot silently take part with a piece of itself.
 * A, B, C, s[i][j], the four parameters and their checks are gfy_align_local's; every + and - is
 * one rounded fp32 operation, max is exact, nothing is contracted.
 *   Recurrences E[i][j] = max(E[i][j-1] - gap_extend, H[i][j-1] - gap_open)
 *               F[i][j] = max(F[i-1][j] - gap_extend, H[i-1][j] - gap_open)
 *               H[i][j] = max(H[i-1][j-1] + s[i][j], E[i][j], F[i][j])           (no 0 candidate)
 *   Borders     the same recurrences carried onto row -1 and column -1, so a border is an
 *               ITERATED sum and not a closed form.  H[-1][-1] = 0.
 *               Left, both modes:  F[i][-1] = max(F[i-1][-1] - gap_extend, H[i-1][-1] - gap_open),
 *                        H[i][-1] = F[i][-1], E[i][-1] = -inf, with F[-1][-1] = -inf: H[0][-1] =
 *                        fl32(0 - gap_open), H[i][-1] = fl32(H[i-1][-1] - gap_extend).
 *               Top, within = 0:  the mirror image, H[-1][j] = E[-1][j] iterated along j and
 *                        F[-1][j] = -inf.
 *               Top, within = 1:  H[-1][j] = 0 and E[-1][j] = F[-1][j] = -inf for every j: the
 *                        leading rows of B are free.
 *   Result      within = 0: out_score = H[L_q-1][L_r-1], out_end = (L_q-1, L_r-1).
 *               within = 1: out_score = max over 0 <= j < L_r of H[L_q-1][j], out_end = (L_q-1, j)
 *               for the first such j.  Scores may be negative, and only a zero keeps no promise
 *               of its sign.  A pair with a record of zero rows on either side is "nothing to
 *               align": score 0, end (-1, -1) (and an empty path), as in the local mode, not the
 *               cost of a gap.  A pair that is refused gets NaN and (-2, -2), as
 *               gfy_align_local's: the same clipping of ptr_a, ptr_b and pairs, the same limits.
 *   Ordering    every operation is monotone in its inputs and the modes differ only in
 *               candidates added, so for any pair and parameters, exactly, in fp32 comparison:
 *               score(within = 0) <= score(within = 1) <= gfy_align_local's score.
 *   Workspace   gfy_align_workspace_bytes(pairs, max_rows_b), used as gfy_align_local uses it.
 *   Arguments and error codes are those of gfy_align_local; a within other than 0 or 1 is
 *   GFY_ERR_INVALID.  A box of rows on these modes is gfy_align_global_box's.  Out of scope: a
 *   band on these modes (the gfy_align_*_band calls are local only), free ends on the a-side, a
 *   span-only call for these modes, null scores for these modes (gfy_align_local_null is local
 *   only).
 *   Cost: DESIGN.md §4.                                                                       */
int gfy_align_global(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                     const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                     const int32_t* pairs /* [P][2] device */, int64_t P,
                     float match_scale, float match_shift, float gap_open, float gap_extend,
                     int within, float* out_score /* [P] */, int32_t* out_end /* [P][2] */,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The aligned PATH of gfy_align_global.  ends (int32 [P][2], device memory) is what that call
 * returned for the same a, b, pairs, parameters and within.
 *   Walk        from H at end by the tie rules of gfy_align_trace: in H the diagonal first, then
 *               E, then F; in E and F opening wins a tie.  Ops 0, 1 and 2 as there, reported in
 *               FORWARD order.  There is no "starts here" rule: the walk ends on a border, which
 *               it always reaches in H (a gap that meets a border opened there).
 *               At (-1, -1) it stops.  At (i, -1) it emits i + 1 ops 2: the left border is a
 *               charged gap.  At (-1, j) it emits j + 1 ops 1 with within = 0 and stops with
 *               within = 1: those rows of B are free.
 *   Result      out_ops[op_ptr[p] ..], out_len[p] of them, at most L_q + L_r (a path of gaps
 *               alone; one more than the local bound).  out_start[p] = (first row of A consumed,
 *               first row of B consumed): start_i = 0 always, start_j = 0 with within = 0, and
 *               with within = 1 start_j = end_j + 1 - #(ops != 2), which is end_j + 1 where no row
 *               of B is consumed.  The ops 0 and 2 number L_q, the ops 0 and 1 end_j + 1 -
 *               start_j.  An end of (-1, -1) has out_len = 0 and start (-1, -1).  Re-scoring the
 *               ops by the rule of gfy_align_trace (h = 0; ...) gives out_score bit for bit: this
 *               is why the borders are iterated.
 *   The box     rows 0 .. L_q - 1, columns 0 .. end_j.  Its top-left corner is the matrix's own, so
 *               every value in it is the full matrix's by construction and no argument is needed.
 *               4 direction bits per cell as gfy_align_trace keeps them (which candidate H took:
 *               1, 2 or 3; 0 is unused).
 *   Slots       op_ptr int64 [P + 1], device memory: pair p owns out_ops[op_ptr[p] ..
 *               op_ptr[p + 1]), at least L_q + end_j + 1 bytes of it (L_q + L_r always serves).
 *   Workspace   gfy_align_global_trace_workspace_bytes(pairs, max_rows_a, max_rows_b), cut and
 *               accepted as gfy_align_trace's is, for boxes of up to max_rows_a x max_rows_b.
 *   Refused     out_len[p] = -2, out_start[p] = (-2, -2) and nothing written to the slot: what
 *               gfy_align_global refuses, an end other than (-1, -1) that it cannot have named
 *               (end_i != L_q - 1, end_j outside the b-record, with within = 0 end_j != L_r - 1),
 *               a box of more columns than max_rows_b or of more direction words than a wave's
 *               region, a slot shorter than L_q + end_j + 1.
 *   Arguments and error codes are those of gfy_align_trace, with ends, op_ptr, out_ops, out_len
 *   and out_start named when NULL; a within other than 0 or 1 is GFY_ERR_INVALID.            */
size_t gfy_align_global_trace_workspace_bytes(int64_t pairs, int64_t max_rows_a,
                                              int64_t max_rows_b);
int gfy_align_global_trace(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                           const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                           const int32_t* pairs /* [P][2] device */, int64_t P,
                           float match_scale, float match_shift, float gap_open, float gap_extend,
                           int within, const int32_t* ends /* [P][2] */,
                           const int64_t* op_ptr /* [P + 1] */, uint8_t* out_ops,
                           int32_t* out_len /* [P] */, int32_t* out_start /* [P][2] */,
                           int64_t max_rows_a, int64_t max_rows_b,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Global and query-in-target alignment INSIDE A BOX of rows per pair (fill between anchors):
 * gfy_align_global and gfy_align_global_trace with `boxes` (int32 [P][4], device memory) behind
 * `within`.  A chain of seeds has a first and a last cell; the stretch between them aligned END
 * TO END, unrelated linkers included, is the global alignment of that stretch, which a local
 * alignment (it keeps the best piece) does not give.  within = 1 with a box asks where a WINDOW
 * of the a-record (the box's a-rows) lies inside a REGION of the b-record (the box's b-rows).
 *   Box         boxes[p] = (i_lo, i_hi, j_lo, j_hi) as gfy_align_local_box takes it: rows of the
 *               a-record and of the b-record, 0-based inside the two records, both ends
 *               inclusive.  THE BOX IS THE MATRIX: row -1 and column -1 of gfy_align_global's
 *               definition are the rows just outside the box.  The left border is the charged
 *               gap iterated in fp32, the top border is charged (within = 0) or free (within =
 *               1), exactly as without a box.  Nothing else changes: s[i][j], the recurrences,
 *               every rounded operation, the tie rules of the walk and the op codes.
 *   Results     stay in the RECORDS' coordinates.  within = 0: out_end = (i_hi, j_hi) of the
 *               clipped box and out_start = (i_lo, j_lo).  within = 1: out_end = (i_hi, j) for the
 *               first best j in j_lo .. j_hi and out_start = (i_lo, start_j), start_j = end_j + 1
 *               where no row of B is consumed.
 *   Clipping    the kernel reads the four values per pair like the pair itself, clips them into
 *               [-GFY_ALIGN_ROWS_MAX, GFY_ALIGN_ROWS_MAX] and then into the two records.  A box
 *               that holds no cell after clipping is "nothing to align", like a record of zero
 *               rows: score 0, start and end (-1, -1), out_len 0.  A pair with i_lo > i_hi or j_lo
 *               > j_hi as given is refused as gfy_align_local_box refuses it: NaN, (-2, -2),
 *               out_len -2.
 *   It follows  - a box that covers both records gives the results of gfy_align_global and
 *                 gfy_align_global_trace bit for bit: scores, starts, ends and ops.
 *               - a boxed call equals, bit for bit, the call without a box on rows i_lo..i_hi of
 *                 A and j_lo..j_hi of B taken as two records of their own, with (i_lo, j_lo) (the
 *                 clipped box's) added to its cells.  That is how the kernel does it.
 *               - re-scoring the ops by the rule of gfy_align_trace gives out_score bit for bit.
 *               - in one and the same box, score(within = 0) <= score(within = 1) <=
 *                 gfy_align_local_box's score (bands NULL), exactly: the ordering of
 *                 gfy_align_global on the sliced rows.
 *               - a pair's result depends neither on the other pairs of the call, nor on the
 *                 run, nor on the workspace.
 *   Widening    within = 1: widening the box on the b-side (a lower j_lo, a higher j_hi, the same
 *               a-rows) never lowers out_score, exactly, in fp32 comparison.  A higher j_hi only
 *               adds candidates to the max over the last row (columns do not depend on the
 *               columns to their right).  A lower j_lo: compare the narrow matrix N (columns from
 *               j_lo) with the wide one W (columns from j_lo' < j_lo) column by column.  In W,
 *               column j_lo - 1 is a real column whose cells satisfy H_W[i][j_lo - 1] >=
 *               F_W[i][j_lo - 1], and F_W there is >= the charged left border of N by induction
 *               over rows: F_W[0] = H_W[-1] - gap_open = 0 - gap_open = N's border at row 0 (the
 *               top border of within is 0 in every column), and F_W[i] >= F_W[i-1] - gap_extend
 *               >= border[i-1] - gap_extend = border[i], subtraction being monotone.  E of that
 *               column is >= -inf = E of N's border.  So every input of N's first column is <=
 *               its counterpart in W, every operation (rounded +, rounded -, max) is monotone,
 *               and by induction over columns and rows every H, E and F of N is <= W's at the
 *               same cell; so is the max over the last row.  within = 0 has NO such property: a
 *               wider box must also pay for the rows it adds.
 *   Trace       gfy_align_global_trace_box takes the SAME boxes as the score call and the ends
 *               that call returned, in the records' coordinates.  The box is applied first; the
 *               trace's own box is then rows 0 .. box rows - 1 and columns 0 .. end_j - j_lo of
 *               it, whose top-left corner is the boxed matrix's own.  Refused (out_len -2, start
 *               (-2, -2)): what the score call refuses, an end other than (-1, -1) that it cannot
 *               have named for that box (end_i != i_hi, end_j outside j_lo .. j_hi, with within =
 *               0 end_j != j_hi, all after clipping), a box of more columns than max_rows_b or of
 *               more direction words than a wave's region, a slot shorter than box rows + end_j -
 *               j_lo + 1.
 *   Slots       pair p owns at least box rows + box columns bytes of out_ops (after clipping).
 *   Work        the strips follow the box: ceil(box rows / 64) strips of at most box columns + 63
 *               steps.  A 150-row chain in two 4,096-row records: 3 strips against the 64 of
 *               gfy_align_global on the whole records (arithmetic from the loop bounds; no time
 *               is claimed here).
 *   Workspace   no sizers of their own: gfy_align_workspace_bytes(pairs, widest box columns) and
 *               gfy_align_global_trace_workspace_bytes(pairs, max box rows, max box columns),
 *               sizes after clipping; max_rows_a and max_rows_b of the trace are the largest BOX
 *               sizes.  A pair whose box has more columns than the workspace holds is refused.
 *   Arguments, checks and error codes are those of the counterpart; a NULL boxes is
 *   GFY_ERR_INVALID, named, with a pointer to the call without a box.  Out of scope: a BAND on
 *   these modes (borders that leave the band, pairs with no admissible path at all), boxes that
 *   are not rectangles, free ends on the a-side.
 *   Cost: DESIGN.md §4.                                                                        */
int gfy_align_global_box(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                         const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                         const int32_t* pairs /* [P][2] device */, int64_t P,
                         float match_scale, float match_shift, float gap_open, float gap_extend,
                         int within, const int32_t* boxes /* [P][4] device */,
                         float* out_score /* [P] */, int32_t* out_end /* [P][2] */,
                         void* workspace, size_t workspace_bytes, void* stream);
int gfy_align_global_trace_box(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                               const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                               const int32_t* pairs /* [P][2] device */, int64_t P,
                               float match_scale, float match_shift, float gap_open,
                               float gap_extend, int within,
                               const int32_t* boxes /* [P][4] device */,
                               const int32_t* ends /* [P][2] */,
                               const int64_t* op_ptr /* [P + 1] */, uint8_t* out_ops,
                               int32_t* out_len /* [P] */, int32_t* out_start /* [P][2] */,
                               int64_t max_rows_a, int64_t max_rows_b,
                               void* workspace, size_t workspace_bytes, void* stream);

/* The VALUES ALONG given paths: per op the cosine of its cell and the running score behind it, per
 * path the score, the counts and the sum that a normalisation of scores starts from.  The dense
 * L_q x L_r cosine matrix of a pair is not written to read a few hundred of its cells.
 *   Paths       a, b, the records, pairs and the four parameters are those of gfy_align_local.
 *               starts int32 [P][2], op_ptr int64 [P + 1], ops uint8 [n_ops], device memory: pair
 *               p's path is ops[op_ptr[p] .. op_ptr[p + 1]), one byte per op, and starts at cell
 *               starts[p] in the records' coordinates.  Op 0 consumes cell (i, j) and moves to
 *               (i + 1, j + 1), op 1 moves to (i, j + 1), op 2 to (i + 1, j).  This is what
 *               gfy_align_trace and gfy_align_global_trace (and their band and box forms) return
 *               once the slots are compacted; any other path in that form is served as well.
 *   Per op      out_cosine float32 [n_ops]: at an op 0 at cell (i, j) C[i][j], which is
 *               gfy_pairwise_dense(A, B, GFY_COSINE)[i][j] bit for bit (the same eight MFMA steps
 *               from 0, the same norms, key and value); NaN ("no value") at a gap op.
 *               out_running float32 [n_ops]: h behind that op under the re-scoring rule of
 *               gfy_align_trace: h = 0; op 0: h = fl32(h + s[i][j]) with s = fl32(fl32(C *
 *               match_scale) + match_shift); the first op of a run of equal gap ops: fl32(h -
 *               gap_open), each further one of the run fl32(. - gap_extend) (inside a run the entry
 *               is the running g).  Every operation is rounded once and never contracted.
 *   Per path    out_score float32 [P]: the last running value, 0 for an empty path.
 *               out_counts int32 [P][4]: the ops 0, the runs of op 1, the runs of op 2 (op 1 behind
 *               op 2 starts a run, and the other way round), and a status: 0, or -2 refused.
 *               out_cosine_sum float64 [P]: the matched cosines, each widened to float64 and added
 *               one at a time in path order from 0: a fixed function of the path.
 *   It follows  for a path that an alignment call of this library returned for the same rows,
 *               pairs and parameters, out_score[p] is that call's out_score[p] bit for bit (local,
 *               band, box, global and within; only the sign of a zero is not promised): the
 *               re-scoring promise of gfy_align_trace, kept on the device.  A path's values depend
 *               neither on the other paths of the call, nor on their order, nor on max_waves.
 *   Refused     status -2, every per-op value of the path NaN, score and sum NaN, the counts 0: a
 *               record index out of range, a record longer than GFY_ALIGN_ROWS_MAX, a start with
 *               a negative coordinate other than (-1, -1) (where only an empty path may start),
 *               an op byte above 2, a path that names a cell outside its two records (start_i +
 *               #(ops 0 and 2) > L_q or start_j + #(ops 0 and 1) > L_r), op_ptr[p] > op_ptr[p + 1]
 *               or a slot outside [0, n_ops] (then no per-op value is written).  The kernel decides
 *               this from a counting pass over the ops before it follows any cell; what the
 *               device arrays hold is compared and clipped, never followed unchecked, and nothing
 *               outside the caller's buffers is read.  A refusal is not an error of the call.
 *   No workspace.  One wave per path; max_waves = 0 leaves the number of waves to the library,
 *   max_waves > 0 bounds it, and the waves take the paths in turn.
 *   A NULL pointer (named in gfy_last_error), n, m, the record counts or P out of gfy_align_local's
 *   ranges, a non-finite parameter, gap_extend outside [0, gap_open] and a negative n_ops or
 *   max_waves are GFY_ERR_INVALID, before any launch and without a device.
 *   Cost: DESIGN.md §4.                                                                        */
int gfy_align_path_values(const void* a, int64_t n, const int32_t* ptr_a, int64_t records_a,
                          const void* b, int64_t m, const int32_t* ptr_b, int64_t records_b,
                          const int32_t* pairs /* [P][2] device */, int64_t P,
                          float match_scale, float match_shift, float gap_open, float gap_extend,
                          const int32_t* starts /* [P][2] */, const int64_t* op_ptr /* [P + 1] */,
                          const uint8_t* ops /* [n_ops] */, int64_t n_ops,
                          float* out_cosine /* [n_ops] */, float* out_running /* [n_ops] */,
                          float* out_score /* [P] */, int32_t* out_counts /* [P][4] */,
                          double* out_cosine_sum /* [P] */, int64_t max_waves, void* stream);

/* Seeds from radius-search hits: the MAXIMAL DIAGONAL RUNS of the hits of
 * gfy_pairwise_within_fill, the step between that search and the gfy_align_*_band calls.  A
 * stretch that two records share is one hit per row on one diagonal; this call collapses every
 * such stretch into one seed with the evidence behind it.
 *   Hits        offsets int64 [n + 1], indices int32 [hits], values float32 [hits], device
 *               memory, as gfy_pairwise_within_fill leaves them: row i's hits are the b-rows
 *               indices[offsets[i] .. offsets[i + 1]), STRICTLY ASCENDING (a precondition; a
 *               segment in another order gives runs of no meaning and no stray access),
 *               offsets[0] = 0, offsets non-decreasing, offsets[n] = hits, 0 <= indices < m.
 *   Records     rows of a in records_a contiguous records by ptr_a (int32 running sums,
 *               [records_a + 1], device memory, ptr_a[records_a] = n), rows of b in records_b by
 *               ptr_b (ptr_b[records_b] = m), as the alignment calls take them.  A row at a
 *               boundary belongs to the record that starts there; a record of zero rows owns
 *               nothing.  For a hit (i, j) let q, r be the records of i and j.
 *   Runs        The predecessor of (i, j) is (i - 1, j - 1); it counts only if it is a hit, i - 1
 *               >= ptr_a[q] and j - 1 >= ptr_b[r], so that it lies in the same two records.  A
 *               hit without a predecessor is a HEAD.  The run of a head is the hits (i + t, j +
 *               t), t = 0 .. L - 1, for the largest L for which all of them are hits inside
 *               records q and r.  Every hit belongs to exactly one run, and a run never crosses a
 *               record boundary on either side.
 *   gfy_hit_runs_mark   marks int32 [hits]: L at a head, 0 at every other hit.  The float64 sums
 *               of the heads go to the workspace.
 *   gfy_hit_runs_emit   slots int64 [hits], device memory: the running sums of (marks[h] >=
 *               min_length), the entry of h included; runs = slots[hits - 1] >= 1; min_length >=
 *               1.  The head h with marks[h] >= min_length is run s = slots[h] - 1 — the runs come
 *               in the order of their heads, i ascending, then j ascending — and gets
 *                 out_pairs[s]   = (q, r)                               int32 [runs][2]
 *                 out_cells[s]   = (i - ptr_a[q], j - ptr_b[r])         int32 [runs][2]: the head
 *                                  inside the two records; its diagonal is the run's
 *                 out_lengths[s] = L                                    int32 [runs]
 *                 out_weights[s] = the sum of the run's L values, accumulated in float64 in
 *                                  ascending t, each addition one rounded operation, rounded to
 *                                  float32 once (the rule of gfy_pairwise_record_scores)
 *               with the SAME workspace, untouched since the mark call on the same hits.
 *   It follows  A run is a function of the hits and the records alone: it depends neither on how
 *               the call is cut into workgroups nor on the run of the program, bit for bit.  The
 *               lengths of all runs sum to hits at min_length = 1, and min_length = k gives the
 *               runs of min_length = 1 with L >= k, in the same order.
 *   Safety      *status (int32, one word, device memory, zeroed by each call) is set non-zero
 *               when offsets, indices or the pointers contradict the sizes of the call, or slots
 *               does not number the kept heads: every index read from memory is clipped or
 *               checked in front of its use, so whatever the arrays hold, no access leaves them
 *               and a hit that does not fit is left out.
 *   Cost        one lane per hit and binary searches: a hit finds its a-row in offsets, its
 *               records in ptr_a / ptr_b, its predecessor in the row above; a head then walks
 *               its diagonal with one binary search per step, so a run of L hits is L serial
 *               steps of one lane (no pointer jumping).  No atomics on the results, no sort.
 *               Measured cost: DESIGN.md §4.
 *   Workspace   gfy_hit_runs_workspace_bytes(hits): one float64 per hit.
 *   A NULL pointer, n, m or hits outside 1..2^31 - 2, records_a or records_b outside
 *   1..GFY_PAIRWISE_RECORDS_MAX, min_length < 1 and runs outside 1..hits are GFY_ERR_INVALID, a
 *   short workspace is GFY_ERR_WORKSPACE; all of it before any launch and without a device.   */
size_t gfy_hit_runs_workspace_bytes(int64_t hits);
int gfy_hit_runs_mark(const int64_t* offsets /* [n + 1] */, int64_t n,
                      const int32_t* indices /* [hits] */, const float* values /* [hits] */,
                      int64_t hits, const int32_t* ptr_a, int64_t records_a,
                      const int32_t* ptr_b, int64_t records_b, int64_t m,
                      int32_t* marks /* [hits] */, int32_t* status,
                      void* workspace, size_t workspace_bytes, void* stream);
int gfy_hit_runs_emit(const int64_t* offsets /* [n + 1] */, int64_t n,
                      const int32_t* indices /* [hits] */, const float* values /* [hits] */,
                      int64_t hits, const int32_t* ptr_a, int64_t records_a,
                      const int32_t* ptr_b, int64_t records_b, int64_t m,
                      const int32_t* marks /* [hits] */, const int64_t* slots /* [hits] */,
                      int min_length, int64_t runs,
                      int32_t* out_pairs /* [runs][2] */, int32_t* out_cells /* [runs][2] */,
                      int32_t* out_lengths /* [runs] */, float* out_weights /* [runs] */,
                      int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Chains of runs: the runs of gfy_hit_runs_emit LINKED ACROSS NEIGHBOURING DIAGONALS.  A run is a
 * gapless stretch on one diagonal, so a region that two records share with one inserted or
 * deleted row is two runs on two diagonals; this call joins such pieces into one chain and gives
 * the band of diagonals that holds all of it, which is what the gfy_align_*_band calls take.  It
 * is a fixed function of the runs and two integers, bit for bit, and needs no counts.
 *   Inputs      runs = (pairs int32 [S][2], cells int32 [S][2], lengths int32 [S], weights
 *               float32 [S]), device memory, in the order gfy_hit_runs_emit writes them: the key
 *               (q, cell_i, r, cell_j) is strictly ascending lexicographically from run to run
 *               (this follows from "i ascending, then j ascending" over contiguous records).  A
 *               subset of the runs in their order keeps this property; a permutation does not.
 *   Terms       Run s has pair (q_s, r_s), head (i_s, j_s), length L_s >= 1 and diagonal d_s =
 *               j_s - i_s.  Its tail is the cell (i_s + L_s - 1, j_s + L_s - 1).
 *   Linking     s may precede t (s -> t) if and only if all of these hold: the pairs are equal;
 *               gi = i_t - (i_s + L_s) >= 0; gj = j_t - (j_s + L_s) >= 0; max(gi, gj) <= max_gap;
 *               |d_t - d_s| = |gj - gi| <= max_shift.  There is no overlap in either coordinate,
 *               and s -> t implies s < t in the order of the runs.
 *   Forward     C[t] = L_t + max(0, max over s -> t of C[s]), computed in int64.  pred[t] is the s
 *               that attains the maximum; ties go to the smallest |d_t - d_s|, then to the largest
 *               s; pred[t] = -1 when no s precedes t.
 *   Backward    The mirror image: D[s] = L_s + max(0, max over s -> t of D[t]).  succ[s] is the t
 *               that attains the maximum; ties go to the smallest |d_t - d_s|, then to the
 *               smallest t; succ[s] = -1 when s precedes no t.
 *   Chains      A link s - t is kept if and only if pred[t] == s and succ[s] == t: both ends must
 *               choose each other.  Every run therefore has at most one kept predecessor and at
 *               most one kept successor.  The chains are the maximal paths; every run belongs to
 *               exactly one chain, and a chain lies in one record pair.  The rule was chosen
 *               because it is symmetric (the runs read backwards give the same chains) and needs
 *               no serial "take the best chain, remove its runs, repeat" step: two passes and a
 *               comparison decide every link.  What it guarantees: where a record pair's
 *               maximum-hit chain is unique, including all its prefixes and suffixes, that chain
 *               is one of the chains returned.
 *   Output      Chains come in the order of their first runs; chain c gets
 *                 out_pairs[c]     = (q, r)                             int32 [chains][2]
 *                 out_starts[c]    = the head of the first run          int32 [chains][2]
 *                 out_ends[c]      = the tail of the last run           int32 [chains][2]
 *                 out_diagonals[c] = (min d, max d) over its runs       int32 [chains][2]
 *                 out_counts[c]    = the number of its runs             int32 [chains]
 *                 out_lengths[c]   = the sum of L: the number of hits   int32 [chains]
 *                 out_weights[c]   = the runs' float32 weights added in float64 in chain order,
 *                                    each addition one rounded operation, rounded to float32 once
 *               and every run s out_members[s] = its chain (int32 [S]): a chain's runs are the s
 *               with out_members[s] == c, ascending.
 *   It follows  max_gap = 0 links nothing, because two such runs would have been one maximal run:
 *               then chains == S, starts == cells, the lengths are equal, the weights are the same
 *               bytes and members[s] == s.  The counts sum to S and the lengths to the sum of the
 *               runs' lengths, whatever the two integers.
 *   Calls       The caller sorts the runs by record pair with a STABLE sort (any key that is
 *               equal exactly where the pairs are: q * 2^31 + r in int64 cannot overflow) and
 *               passes order int64 [S], the permutation, and bounds int64 [groups + 1], ascending
 *               from 0 to S: group g is order[bounds[g] .. bounds[g + 1]), the runs of one pair.
 *               gfy_chain_runs_link writes marks int32 [S]: the count of its chain at a chain's
 *               first run, 0 at every other run; everything else goes to the workspace.
 *               gfy_chain_runs_emit takes slots int64 [S], the running sums of (marks > 0), the
 *               entry of s included, chains = slots[S - 1] >= 1, and the SAME workspace, untouched
 *               since the link call on the same runs.
 *   Safety      The preconditions that need the data (L >= 1, cells >= 0, pairs >= 0, the sum of L
 *               and every i + L, j + L at most 2^31 - 1 resp. 2^31, the ascending key) are the
 *               caller's; without them the chains have no meaning, and still no access leaves an
 *               array and no loop runs on.  *status (int32, one word, device memory, zeroed by
 *               each call) is set non-zero when order, bounds, a group that mixes pairs, or slots
 *               contradict the sizes of the call: every index read from memory is clipped or
 *               checked in front of its use, and a walk along a chain only moves forward.
 *   Cost        One wave per record pair.  A pass is serial in its runs; the 64 lanes share the
 *               candidates of one run, and because a pair's runs ascend in i a lane stops at the
 *               first one too far away to link, so a step costs the runs within max_gap + the
 *               pair's longest run of rows, not the pair.  plain != 0 scans every candidate; the
 *               result is the same (it exists to show that).  A group of up to 1,024 runs is
 *               held in LDS, a larger one in the workspace, by the same code.  A chain is walked
 *               by one lane.  Measured cost: DESIGN.md §4.
 *   Workspace   gfy_chain_runs_workspace_bytes(runs): 64 bytes per run.
 *   A NULL pointer, runs outside 1..2^31 - 2, groups or chains outside 1..runs and max_gap or
 *   max_shift outside 0..2^31 - 1 are GFY_ERR_INVALID, a short workspace is GFY_ERR_WORKSPACE; all
 *   of it before any launch and without a device.  Not built: overlapping runs, a gap or shift
 *   penalty in the chain score, chains across record pairs or shards, a host path.            */
size_t gfy_chain_runs_workspace_bytes(int64_t runs);
int gfy_chain_runs_link(const int32_t* pairs /* [runs][2] */, const int32_t* cells /* [runs][2] */,
                        const int32_t* lengths /* [runs] */, const float* weights /* [runs] */,
                        int64_t runs, const int64_t* order /* [runs] */,
                        const int64_t* bounds /* [groups + 1] */, int64_t groups,
                        int64_t max_gap, int64_t max_shift, int plain,
                        int32_t* marks /* [runs] */, int32_t* status,
                        void* workspace, size_t workspace_bytes, void* stream);
int gfy_chain_runs_emit(const int32_t* pairs /* [runs][2] */, const int32_t* cells /* [runs][2] */,
                        const int32_t* lengths /* [runs] */, const float* weights /* [runs] */,
                        int64_t runs, const int32_t* marks /* [runs] */,
                        const int64_t* slots /* [runs] */, int64_t chains,
                        int32_t* out_pairs /* [chains][2] */, int32_t* out_starts /* [chains][2] */,
                        int32_t* out_ends /* [chains][2] */,
                        int32_t* out_diagonals /* [chains][2] */,
                        int32_t* out_counts /* [chains] */, int32_t* out_lengths /* [chains] */,
                        float* out_weights /* [chains] */, int32_t* out_members /* [runs] */,
                        int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GFY_H_ */
