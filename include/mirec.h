/*
 * mirec.h — C ABI of libmirec.so, the MI355X (gfx950) engine for the
 * LightGCN propagation + BPR training hot path of
 * HiromasaYamanishi/furusato_recommend.
 *
 * Every entry point is extern "C", takes plain pointers and sizes, returns an
 * int status (0 = MIREC_OK) and never allocates device memory: the caller
 * (PyTorch's caching allocator on the Python side) owns every buffer and
 * passes scratch space explicitly.  Device entry points are stream-ordered on
 * the hipStream_t passed as `stream` (NULL = the legacy default stream), do
 * not synchronise the host and are safe to capture into a hipGraph.
 *
 * Reference interfaces each group replaces (paths under the reference repo):
 *   mirec_csr_*            model/lgcn.py:53-61 (symmetric edge list) and the
 *                          gcn_norm degree pass PyG's LGConv runs per call
 *                          (called at model/lgcn.py:66,82); restated in-repo
 *                          by model/radj.py:28-36.
 *   mirec_propagate        LGConv()(x, edge_index) at model/lgcn.py:82,
 *                          model/radj.py:39-44 (gather / scale / scatter-sum),
 *                          the layer mean of model/lgcn.py:78-86 and the
 *                          autograd backward of both.
 *   mirec_bpr_*            LightGCN.bpr_loss model/lgcn.py:98-118 + its
 *                          backward (stageOne, model/lgcn.py:127-133).
 *   mirec_adam_*           torch.optim.Adam created at model/lgcn.py:63,
 *                          stepped at model/lgcn.py:132.
 *   mirec_bpr_sample       UniformSample, negative_sample.py:98-134.
 */
#ifndef MIREC_H
#define MIREC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Still 1: mirec_csr_t gained a trailing field (`val`, the per-entry edge
 * weights) after the version was set; a binding checks its mirror of the
 * struct with mirec_struct_sizes, and a NULL `val` is the earlier behaviour.
 * Likewise mirec_prop_t's trailing scale_src / scale_dst / scale_next: NULL
 * (each on its own) means csr->dinv, the earlier behaviour.  Edge dropout
 * left both structs alone: it has a struct and an entry point of its own
 * (mirec_drop_t, mirec_propagate_drop). */
#define MIREC_ABI_VERSION 1

enum mirec_status {
  MIREC_OK = 0,
  MIREC_ERR_ARG = 1,       /* null pointer / negative size / bad enum        */
  MIREC_ERR_DIM = 2,       /* embedding dim not in {4,8,16,32,64,128,256}    */
  MIREC_ERR_HIP = 3,       /* a HIP runtime call failed (mirec_last_hip_error) */
  MIREC_ERR_WORKSPACE = 4, /* caller-provided scratch space too small         */
  MIREC_ERR_RANGE = 5      /* an index is outside [0, n)                     */
};

typedef void *mirec_stream_t; /* hipStream_t */

const char *mirec_strerror(int code);
int mirec_abi_version(void);
int mirec_last_hip_error(void);
/* sizeof(mirec_csr_t), sizeof(mirec_prop_t), sizeof(mirec_adam_hparams_t):
 * lets FFI bindings verify their struct mirrors. */
int mirec_struct_sizes(size_t *csr, size_t *prop, size_t *adam_hparams);

/* ------------------------------------------------------------------------ */
/* Graph (host side, once per graph)                                         */
/* ------------------------------------------------------------------------ */

/* Destination-major CSR of the symmetric user–item graph of
 * model/lgcn.py:53-61: node ids are users [0, n_users) then items
 * n_users + [0, m_items).  Row u lists its items in edge order, row
 * n_users+i lists its users in edge order (stable, duplicates kept as
 * multi-edges exactly like the reference edge list).  dinv[v] =
 * deg(v)^-1/2, 0 for isolated nodes (gcn_norm, add_self_loops=False).
 * rowptr: [n_users+m_items+1], col: [2*n_edges], dinv: [n_users+m_items]. */
int mirec_csr_bipartite(const int64_t *train_user, const int64_t *train_item,
                        int64_t n_edges, int64_t n_users, int64_t m_items,
                        int64_t *rowptr, int32_t *col, float *dinv);

/* Generic stable CSR by destination from a COO edge list (edge_index[0] =
 * source, edge_index[1] = destination, the LGConv convention).  dinv (may
 * be NULL) = in-degree^-1/2 of every node (gcn_norm on `col`). */
int mirec_csr_from_coo(const int64_t *src, const int64_t *dst, int64_t nnz,
                       int64_t n_nodes, int64_t *rowptr, int32_t *col,
                       float *dinv);

/* The entry order of mirec_csr_from_coo: perm[k] is the index in the COO
 * list of CSR entry k (the stable sort of the edges by destination), so
 * per-edge data w goes into CSR order as val[k] = w[perm[k]].  For
 * mirec_csr_bipartite pass the doubled edge list's destinations
 * (n_users + train_item, then train_user): edge e of the doubled list is
 * interaction e mod n_edges.  perm: [nnz].  MIREC_ERR_RANGE for a
 * destination outside [0, n_nodes). */
int mirec_csr_entry_order(const int64_t *dst, int64_t nnz, int64_t n_nodes,
                          int64_t *perm);

/* Long-row schedule for load balance: rows with more than `split` entries
 * are cut into segments of `split` entries.  Call once with NULL outputs
 * to get the counts, then again with arrays of those sizes:
 * long_rows[n_long], long_segptr[n_long+1], seg_row[n_seg], seg_beg[n_seg]. */
int mirec_csr_long_rows(const int64_t *rowptr, int64_t n_rows, int32_t split,
                        int64_t *n_long, int64_t *n_seg, int32_t *long_rows,
                        int64_t *long_segptr, int32_t *seg_row,
                        int64_t *seg_beg);

/* Ingest (dataloader.py:93-150): parse an interaction file held in memory,
 * one line per user "uid i1 i2 ..." (spaces / tabs; empty lines skipped;
 * a line with only a uid counts as a line without items).  If stop_uid >= 0
 * parsing ends after the first line whose uid == stop_uid (the reference's
 * test-mode cut).  Call once with line_uid == NULL to get the counts and
 * maxima (-1 if none), then with line_uid[n_lines], line_off[n_lines + 1],
 * items[n_items]: line k has uid line_uid[k] and items
 * items[line_off[k] .. line_off[k+1]), in file order.  n_threads host
 * threads (buffers under 1 MiB use one).  MIREC_ERR_ARG on a malformed
 * token. */
int mirec_parse_interactions(const char *buf, int64_t len, int64_t stop_uid,
                             int32_t n_threads, int64_t *n_lines, int64_t *n_items,
                             int64_t *max_uid, int64_t *max_item, int64_t *line_uid,
                             int64_t *line_off, int64_t *items);

/* Device-resident CSR descriptor (all pointers are device pointers). */
typedef struct mirec_csr {
  const int64_t *rowptr;      /* [n_rows+1] */
  const int32_t *col;         /* [nnz] source node of each entry */
  const float *dinv;          /* [n_rows] deg^-1/2 (0 if deg == 0) */
  int64_t n_rows;
  int64_t nnz;
  int32_t split;              /* long-row threshold, 0 = none */
  int32_t _pad;
  int64_t n_long;
  int64_t n_seg;
  const int32_t *long_rows;   /* [n_long] */
  const int64_t *long_segptr; /* [n_long+1] */
  const int32_t *seg_row;     /* [n_seg] */
  const int64_t *seg_beg;     /* [n_seg] */
  /* optional (NULL = none): rows [0, n_sorted) with each row's entries sorted
   * ascending, entry rowptr[r] + j of the CSR at index rowptr[r] - rowptr[0]
   * + j (mirec_csr_sort_rows); the samplers' membership tests binary-search
   * them (the user rows of a bipartite graph) */
  const int32_t *col_sorted;
  int64_t n_sorted;
  /* appended (see MIREC_ABI_VERSION): the matrix is A_ij = sum of val over
   * the entries (j -> i) instead of their count, and dinv comes from the
   * weighted degree (the caller's choice: gcn_norm's sum of the weights into
   * i, or all ones).  Read by mirec_propagate and mirec_edge_dot's callers
   * only; samplers, frontier and GraphSAGE use the structure alone. */
  const float *val; /* [nnz] per-entry weight, NULL = all ones */
} mirec_csr_t;

/* Host: rows [0, n_rows) of (rowptr, col) with each row sorted ascending into
 * col_sorted [rowptr[n_rows] - rowptr[0]] (the csr's col_sorted). */
int mirec_csr_sort_rows(const int64_t *rowptr, const int32_t *col, int64_t n_rows,
                        int32_t *col_sorted);

/* ------------------------------------------------------------------------ */
/* Propagation: one LightGCN layer (CSR segment-gather SpMM + epilogue)      */
/* ------------------------------------------------------------------------ */

enum mirec_in_mode {
  MIREC_IN_PRESCALED = 0, /* x_in rows are already x~_j = dinv_j * x_j        */
  MIREC_IN_RAW = 1,       /* x_in rows are x_j; the kernel applies dinv_j     */
  MIREC_IN_SPARSE = 2,    /* input row j = seed_in[slot[j]] (0 if slot[j]<0),
                             kernel applies dinv_j                            */
  MIREC_IN_NONE = 3       /* no gather: y = 0 (epilogue only; L = 0 / MF)    */
};

typedef struct mirec_adam_hparams {
  float one_minus_beta1; /* 1 - beta1                      */
  float beta2;
  float one_minus_beta2; /* 1 - beta2                      */
  float neg_step_size;   /* -lr / (1 - beta1^t)            */
  float bc2_sqrt;        /* sqrt(1 - beta2^t)              */
  float eps;
} mirec_adam_hparams_t;

/* For every row i of the CSR:
 *   y_i   = dinv_i * sum_{j in row i} xin~_j                (Â x, fp32)
 *           with csr->val: sum_{e = (j -> i)} val_e * xin~_j, the terms in
 *           the same (CSR) order; every in_mode, mask and row list applies
 *   z_i   = y_i + seed[slot_i]               (if seed != NULL and slot_i >= 0)
 *   xs_out_i = dinv_i * z_i                  (if xs_out != NULL; next layer)
 *   o_i   = (z_i + addend_i) / divisor + seed2[slot_i]
 *   out_i = o_i                 (if out != NULL and out_mask_i != 0)
 *   Adam(param_i, exp_avg_i, exp_avg_sq_i; grad = o_i)   (if param != NULL;
 *       then xs_out_i = dinv_i * param_i after the update)
 * `partial` is scratch of csr->n_seg * dim floats (may be NULL if n_seg==0).
 * Summation order per row is fixed by the CSR: results are deterministic.
 *
 * csr->dinv stands in three places above; scale_src / scale_dst / scale_next
 * (optional, [n_rows] each, NULL = csr->dinv) replace it one place at a time:
 *   xin~_j   = scale_src_j * x_j          (MIREC_IN_RAW, MIREC_IN_SPARSE)
 *   y_i      = scale_dst_i * sum ...
 *   xs_out_i = scale_next_i * z_i        (with Adam: scale_next_i * param_i)
 * which gives D^-(1-r) A D^-r (rAdjConv, model/radj.py:28-44) and its
 * transpose on the one symmetric CSR.  Every launch form honours them and
 * the sweep still qualifies; with csr->val they are refused (MIREC_ERR_ARG). */
typedef struct mirec_prop {
  int32_t dim;
  int32_t in_mode;
  const float *x_in;    /* [n_rows, dim] (modes 0/1) */
  const int32_t *slot;  /* [n_rows] seed slot map, -1 = none */
  const float *seed_in; /* [*, dim] mode-2 input rows indexed by slot */
  const float *seed;    /* [*, dim] */
  const float *addend;  /* [n_rows, dim] */
  const float *seed2;   /* [*, dim] */
  float divisor;
  float _pad;
  float *out;           /* [n_rows, dim] */
  float *xs_out;        /* [n_rows, dim] */
  float *param;         /* fused Adam: [n_rows, dim] each */
  float *exp_avg;
  float *exp_avg_sq;
  mirec_adam_hparams_t adam;
  float *partial;       /* [n_seg, dim] scratch */
  const uint8_t *row_mask;  /* [n_rows] byte map: rows with byte 0 are
                               skipped (nothing written); NULL = all rows */
  const uint8_t *in_mask;   /* byte map over source nodes: only neighbours
                               with byte != 0 contribute (others are exact
                               zeros).  MIREC_IN_SPARSE filters by
                               slot[j] >= 0 when in_mask is NULL, else by
                               the byte map first (must cover the seeded
                               nodes; fewer slot reads when many neighbours
                               are seeded) */
  const uint8_t *out_mask;  /* byte map: rows with byte 0 skip the `out`
                               write and the addend read (their xs_out is
                               still written); ignored with fused Adam */
  const int32_t *row_list;  /* optional deduplicated row list (device); the
                               rows processed are row_list[0 .. *row_count);
                               needs row_mask = the same set (long rows) */
  const int32_t *row_count; /* device pointer to the list length */
  int64_t row_list_cap;     /* host upper bound of *row_count (grid size) */
  int32_t narrow_max;       /* rows of degree <= narrow_max are gathered one
                               per lane group (latency-bound short rows);
                               longer ones one per wave.  0 = always wave */
  int32_t adam_stream;      /* != 0: fused Adam reads and writes param and its
                               moments non-temporally (streams touched once a
                               step), where the launch's kernel has such a
                               form; results do not depend on it */
  const int32_t *wide_list; /* optional second list (with row_list): rows
                               wide_list[0 .. *wide_count) are gathered by a
                               whole 256-thread workgroup each (4 waves split
                               the row, combined in LDS in a fixed order), so
                               a short list of long rows is not latency-bound */
  const int32_t *wide_count;
  /* appended (see MIREC_ABI_VERSION); NULL = csr->dinv */
  const float *scale_src;   /* [n_rows] scale of a gathered neighbour (modes 1/2) */
  const float *scale_dst;   /* [n_rows] scale of the row sum */
  const float *scale_next;  /* [n_rows] scale of z (or the updated param) for xs_out */
} mirec_prop_t;

int mirec_propagate(const mirec_csr_t *csr, const mirec_prop_t *p,
                    mirec_stream_t stream);

/* Edge dropout (the reference's LightGCN.__dropout_x, model/MF.py:158-176):
 * while training, every entry of the normalised adjacency is kept with
 * probability keep_prob and the kept ones are divided by keep_prob.  Here the
 * mask is a pure function of (seed, destination, source), evaluated inside
 * the propagation kernel for the row it walks and the column it has loaded,
 * so no mask or value array exists and the transposed matrix (the backward)
 * needs no second CSR: it is the same function with i and j swapped.  With
 *   mix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *             x = (x ^ (x >> 27)) * 0x94D049BB133111EB; return x ^ (x >> 31)
 *             (uint64 arithmetic, the splitmix64 finaliser)
 *   key = mix64(seed ^ 0xD6E8FEB86659FD93)
 *   t   = floor((double)keep_prob * 2^32), clamped to [1, 2^32]
 * entry (j -> i) (source j = col[e], destination i = its row) is kept iff
 *   mirec_edge_keep(seed, i, j) := (mix64(key ^ ((uint64)i << 32 | j)) >> 32) < t.
 * keep(seed, i, j) and keep(seed, j, i) are independent draws: the dropped
 * matrix is not symmetric.  Multi-edges (several entries with the same i and
 * j) share ONE draw: all are kept or all dropped, as in the reference, whose
 * coalesced sparse tensor holds one value per (i, j).  keep_prob must lie in
 * (0, 1]; 1 keeps every entry (t = 2^32 is compared without wrapping).
 *
 * Host: keep[e] = mirec_edge_keep(seed, i, col[e]) for every entry e of every
 * row i of a host CSR; transposed != 0: keep[e] = mirec_edge_keep(seed,
 * col[e], i), the mask a launch with drop->transposed applies.  keep: [nnz]
 * bytes (0 / 1).  MIREC_ERR_ARG for keep_prob outside (0, 1] or NaN. */
int mirec_edge_keep_mask(const int64_t *rowptr, const int32_t *col, int64_t n_rows,
                         uint64_t seed, float keep_prob, int32_t transposed,
                         uint8_t *keep);

/* Element dropout (dropout_p / seed of the GraphSAGE hop means, the table
 * gradient's mean groups and the SASRec row tail): a pure function of (seed,
 * element index), so nothing is stored and a backward given the same seed
 * recomputes the forward's mask.  With mix64 as above (uint64 arithmetic):
 *   key    = mix64(seed ^ 0xA24BAED4963EE407)
 *   thresh = floor((double)dropout_p * 65536 + 0.5), raised to 1 when
 *            dropout_p > 0 gives 0, capped at 65535; dropout_p = 0: no mask
 *   scale  = 1.0f / (1.0f - dropout_p) in float (1 when dropout_p = 0)
 * element idx is kept iff
 *   ((mix64(key + (idx >> 2)) >> (16 * (idx & 3))) & 0xffff) >= thresh
 * (key + (idx >> 2) wraps mod 2^64; the four elements of an aligned quad are
 * the four 16-bit slices of one hash).  A kept element is multiplied by scale,
 * a dropped one is 0.  dropout_p must lie in [0, 1) (MIREC_ERR_ARG otherwise,
 * NaN included).  Element index:
 *   (t*k + c) * dim + col   mirec_fanout_mean and its backward,
 *                           mirec_fanout_mean_gather and both its backwards,
 *                           the mean groups of mirec_table_grad_*,
 *                           mirec_fanout_resmean_gather, mirec_fanout_resmean
 *                           and mirec_fanout_resmean_bwd: column col of child
 *                           c of target t
 *   row * d + col           mirec_resnorm_fwd / _bwd, mirec_gemm_resnorm,
 *                           mirec_gemm_nn_resnorm_bwd
 * seed_base (row tail only; device, may be NULL): when given, the launch uses
 * key' = mix64(key ^ *seed_base), read when the kernel runs, in place of key;
 * NULL uses key itself, so *seed_base = 0 is not the same as NULL. */

/* The dropout of one launch.  All zero (or a NULL pointer) = no dropout. */
typedef struct mirec_drop {
  float keep_prob;     /* in (0, 1]; 0 = off */
  int32_t transposed;  /* != 0: the mask of the transposed matrix */
  uint64_t seed;
} mirec_drop_t;

size_t mirec_drop_sizeof(void);

/* mirec_propagate on the edge-dropped matrix: the sum over row i runs over
 * the entries (j -> i) with mirec_edge_keep(seed, i, j) (drop->transposed:
 * (seed, j, i)) only, in CSR order, and is multiplied by 1 / keep_prob; dinv
 * and the epilogue are those of the full graph.  Every in_mode, mask, row
 * list, long-row segments and the fused Adam apply; a dropped neighbour's row
 * is not read.  drop == NULL or drop->keep_prob == 0 is exactly
 * mirec_propagate.  Refused (MIREC_ERR_ARG, nothing launched) with csr->val,
 * with any scale vector of `p`, and for keep_prob outside (0, 1] or NaN.
 * The launch always runs the row kernel: there is no swept form. */
int mirec_propagate_drop(const mirec_csr_t *csr, const mirec_prop_t *p,
                         const mirec_drop_t *drop, mirec_stream_t stream);

/* Column-sweep layout of a block of CSR rows (the item rows of a bipartite
 * graph), built once per graph on the host (csrc/graph.cpp) and read by the
 * sweep kernel of csrc/sweep.hip.  The rows [row0, row0 + n_rows) are cut
 * into n_tiles tiles of tile_rows consecutive rows (the last one shorter),
 * one workgroup each; a tile's rows are cut into `groups` runs of group_rows
 * consecutive rows, one lane group each.  Stream s = tile * groups + group
 * holds the entries of its rows as (source column, row index inside the
 * tile) pairs at ent[2 * e], ent[2 * e + 1], e in [gptr[s], gptr[s + 1]),
 * sorted by column, stable: every row's entries appear in ascending column
 * order with duplicate edges in CSR order, which is the order the kernel
 * sums them in.  Every column lies in [0, n_src) (the source block, a
 * bipartite graph's user rows); the kernel paces its walk over it in bands
 * of band_rows columns.  All pointers are device pointers. */
typedef struct mirec_sweep {
  int64_t row0;
  int64_t n_rows;
  int64_t n_src;
  int32_t tile_rows;
  int32_t group_rows;
  int32_t groups;
  int32_t n_tiles;
  int32_t band_rows;
  int32_t _pad;
  const int64_t *gptr; /* [n_tiles * groups + 1] */
  const int32_t *ent;  /* [2 * (rowptr[row0 + n_rows] - rowptr[row0])] */
} mirec_sweep_t;

size_t mirec_sweep_sizeof(void);

/* Host: n_tiles = ceil(n_rows / tile_rows) and groups = ceil(tile_rows /
 * group_rows) of a layout with these parameters (array sizes for
 * mirec_sweep_build). */
int mirec_sweep_shape(int64_t n_rows, int32_t tile_rows, int32_t group_rows,
                      int32_t *n_tiles, int32_t *groups);

/* Host: fill gptr [n_tiles * groups + 1] and ent [2 * entries] (host arrays)
 * from the host CSR.  MIREC_ERR_RANGE if an entry's column is outside
 * [0, n_src) (the rows do not gather from the source block only). */
int mirec_sweep_build(const int64_t *rowptr, const int32_t *col, int64_t row0,
                      int64_t n_rows, int64_t n_src, int32_t tile_rows,
                      int32_t group_rows, int64_t *gptr, int32_t *ent);

/* Lane groups a sweep workgroup has at this width (the layout's `groups`
 * may not exceed it), 0 if the sweep kernel is not built for the width. */
int mirec_sweep_groups(int32_t dim);

/* mirec_propagate with the rows of `sw` gathered by the sweep kernel and the
 * rows [0, sw->row0) by the row kernel, on the same stream, when the launch
 * qualifies: in_mode PRESCALED, no in_mask / row_mask / row list, no long-row
 * segments (csr->n_seg == 0), no entry values (csr->val == NULL), sw->row0 + sw->n_rows == csr->n_rows and the
 * width has a sweep kernel.  Anything else (sw == NULL included) is exactly
 * mirec_propagate.  Per row the sum runs in ascending source column. */
int mirec_propagate_sweep(const mirec_csr_t *csr, const mirec_prop_t *p,
                          const mirec_sweep_t *sw, mirec_stream_t stream);

/* Per-wave form of the column-sweep layout, for a block of CSR rows [row0,
 * row0 + n_rows) whose columns all lie in the source block [src0, src0 +
 * n_src) (a bipartite graph's item rows: src0 = 0; its user rows: src0 =
 * n_users).  Tiles of tile_rows consecutive rows as in mirec_sweep_t; a
 * tile's rows are cut into MIREC_SWEEP_WAVES runs of wave_rows = ceil(tile_rows
 * / MIREC_SWEEP_WAVES) consecutive rows, one wave of the workgroup each.
 * Stream s = tile * MIREC_SWEEP_WAVES + wave occupies slot[wptr[s], wptr[s + 1])
 * and holds all entries of its rows merged in (column, CSR position) order as
 * 8-byte slots (local row << 32) | column (column as in the CSR, local row
 * inside the tile).  Slots come in steps of 4 (one per 16-lane group) and
 * batches of 4 steps; a stream is a whole number of batches.  The slots of a
 * step name different rows or are padding: local row -1 and the column of
 * the real slot before it.  Steps are filled greedily from the merged order:
 * a step takes, among the pending entries less than MIREC_SWEEP_LOOKAHEAD
 * merged positions past the oldest pending one, the earliest whose row the
 * step does not hold yet, so an entry never overtakes an earlier entry of
 * its row and per row the columns ascend with duplicate edges in CSR order.
 * `grid` workgroups take the tiles b, b + grid, ... in turn.  All pointers
 * are device pointers. */
#define MIREC_SWEEP_WAVES 8
#define MIREC_SWEEP_LOOKAHEAD 16
#define MIREC_SWEEP_BATCH 16 /* slots: 4 steps of 4 */

typedef struct mirec_sweep_wave {
  int64_t row0;
  int64_t n_rows;
  int64_t src0;
  int64_t n_src;
  int64_t n_slots; /* wptr[n_tiles * MIREC_SWEEP_WAVES], > 0 */
  int32_t tile_rows;
  int32_t wave_rows;
  int32_t n_tiles;
  int32_t band_rows;
  int32_t grid; /* workgroups launched, 1 .. n_tiles */
  int32_t row_bits; /* 0: `slot` holds the 8-byte slots above; > 0: the 4-byte
                       packed slots of mirec_sweep_wave_pack with this width
                       of the row field */
  const int64_t *wptr; /* [n_tiles * MIREC_SWEEP_WAVES + 1], in slots */
  const int64_t *slot; /* [n_slots] 8-byte, or [n_slots] 4-byte (row_bits > 0) */
} mirec_sweep_wave_t;

size_t mirec_sweep_wave_sizeof(void);

/* Host: fill wptr [ceil(n_rows / tile_rows) * MIREC_SWEEP_WAVES + 1] and
 * *n_slots (the padded length, which depends on the data) from the host CSR,
 * and slot[0, *n_slots) when slot_cap >= *n_slots.  MIREC_ERR_WORKSPACE if
 * slot_cap is smaller (wptr and *n_slots are valid: call again with room;
 * slot may be NULL with slot_cap 0 as a size query); MIREC_ERR_RANGE if an
 * entry's column is outside [src0, src0 + n_src). */
int mirec_sweep_wave_build(const int64_t *rowptr, const int32_t *col, int64_t row0,
                           int64_t n_rows, int64_t src0, int64_t n_src,
                           int32_t tile_rows, int64_t *wptr, int64_t *slot,
                           int64_t slot_cap, int64_t *n_slots);

/* Host: the 4-byte packed form of the slots mirec_sweep_wave_build wrote (or
 * of any run of them).  *row_bits = the smallest number of bits b with
 * tile_rows < 2^b; slot4[i] = (local row field << (32 - b)) | (column - src0),
 * the all-ones row field standing for the padding row -1.  Half the bytes of
 * the slot stream; the kernel decodes the same (local row, column) pairs, so
 * a launch computes bit for bit what it computes from the 8-byte slots.
 * MIREC_ERR_RANGE, before any array is touched, if the source block does not
 * fit the column field (n_src > 2^(32 - b)), and if a slot's column lies
 * outside [src0, src0 + n_src) or its row outside -1 .. tile_rows - 1. */
int mirec_sweep_wave_pack(const int64_t *slot8, int64_t n_slots, int64_t src0, int64_t n_src,
                          int32_t tile_rows, uint32_t *slot4, int32_t *row_bits);

/* mirec_propagate_sweep with the per-wave layout `items` (the tail rows of
 * the CSR, as `sw` there).  The rows [0, items->row0) go through the row
 * kernel, or, when `users` is a layout of exactly these rows, through the
 * sweep kernel too (a second launch on the same stream; no row kernel runs).
 * Same qualifying rule; anything else (items == NULL included) is exactly
 * mirec_propagate.  Per row the sum runs in ascending source column, one
 * term at a time: for the rows of `items` bitwise equal to
 * mirec_propagate_sweep's. */
int mirec_propagate_sweep_wave(const mirec_csr_t *csr, const mirec_prop_t *p,
                               const mirec_sweep_wave_t *items,
                               const mirec_sweep_wave_t *users, mirec_stream_t stream);

/* Per-XCD pacing of the per-wave sweep.  Index 0 of each array is the item
 * launch's, index 1 the user launch's; every[b] == 0 leaves that launch
 * unpaced.  One wave per workgroup, on every every[b]-th band advance and
 * before the band's barrier, adds its advances to its XCD's sum and naps
 * (nap[b] units of 512 clocks, 0 .. 16) while its own count of advances
 * leads the XCD's mean by more than lead_bands[b]; it polls a fixed number
 * of times at most and never waits until anything, so a launch ends whatever
 * `ws` holds.  Results do not depend on the pacing by a bit.  `ws`: device
 * memory of mirec_sweep_pace_ws_bytes() bytes, zeroed once by the caller; the
 * last workgroup of a launch to leave zeroes its region again (the two
 * launches use separate regions). */
typedef struct mirec_sweep_pace {
  void *ws;
  int32_t lead_bands[2];
  int32_t every[2];
  int32_t nap[2];
} mirec_sweep_pace_t;

size_t mirec_sweep_pace_sizeof(void);
size_t mirec_sweep_pace_ws_bytes(void);

/* mirec_propagate_sweep_wave with its sweep launches paced.  Same qualifying
 * rule; pace == NULL is exactly mirec_propagate_sweep_wave. */
int mirec_propagate_sweep_wave_paced(const mirec_csr_t *csr, const mirec_prop_t *p,
                                     const mirec_sweep_wave_t *items,
                                     const mirec_sweep_wave_t *users,
                                     const mirec_sweep_pace_t *pace, mirec_stream_t stream);

/* mirec_propagate_sweep_wave_paced for a launch WITH p->in_mask (a pruned
 * step's second backward launch: every row gathers from the frontier only).
 * `blocks` names the blocks of rows to run through the masked form of the
 * sweep; the other block's rows run the row kernel on their row range.  The
 * masked form needs what the full sweep needs (dim 64, PRESCALED, no values,
 * no row_mask / row_list, no segments) and no scale vectors;
 * a launch without in_mask, with blocks == 0 or that does not qualify is
 * exactly mirec_propagate_sweep_wave_paced (which runs an in_mask launch as
 * mirec_propagate does).
 * A masked-out slot becomes padding: its term is dropped and its load reads
 * the block's first source row instead, so masked-out rows of x_in are never
 * read.  Bands, barriers and pacing are decided from the layout's static
 * columns, as in the unmasked launch, whatever the mask holds.  Per row the
 * passing terms are added in ascending source column: bitwise the unmasked
 * sweep of an x_in whose masked-out rows are +0.0. */
#define MIREC_SWEEP_MASKED_ITEMS 1
#define MIREC_SWEEP_MASKED_USERS 2
int mirec_propagate_sweep_wave_masked(const mirec_csr_t *csr, const mirec_prop_t *p,
                                      const mirec_sweep_wave_t *items,
                                      const mirec_sweep_wave_t *users,
                                      const mirec_sweep_pace_t *pace, int32_t blocks,
                                      mirec_stream_t stream);

/* A measurement, not a propagation entry: the sweep launch of ONE block
 * (`layout`, items or users) with wave 0 of every workgroup noting
 * wall_clock64() at the tile's start, at each band advance and at the tile's
 * end.  stamps: [n_tiles][n_bands + 1] (n_bands = ceil(n_src / band_rows),
 * stamps_len >= that many elements), meta: [n_tiles][2] = workgroup index and
 * XCC id of the workgroup that ran the tile.  The launch must qualify
 * (MIREC_ERR_ARG otherwise); rows outside the block are not written. */
int mirec_sweep_wave_stamp(const mirec_csr_t *csr, const mirec_prop_t *p,
                           const mirec_sweep_wave_t *layout, int64_t *stamps,
                           int64_t stamps_len, int32_t *meta, mirec_stream_t stream);

/* out[e] = sum_c a[row(e), c] * b[col[e], c] for every entry e of the CSR, in
 * CSR order (row(e) = the row whose range holds e): with a = dL/dy and b = x
 * the gradient of y = A x with respect to the entry values (csr->val itself
 * and dinv are not read).  a: [n_rows, dim], b: [>= max col + 1, dim],
 * out: [nnz].  Work is split by entries, not rows; every entry is written
 * once, no atomics, a fixed summation order. */
int mirec_edge_dot(const mirec_csr_t *csr, const float *a, const float *b,
                   int32_t dim, float *out, mirec_stream_t stream);

/* out = dinv ⊙ x row-wise (the pre-scaled layer-0 input x~_0). */
int mirec_prescale(const float *x, const float *dinv, int64_t n_rows,
                   int32_t dim, float *out, mirec_stream_t stream);

/* Row shards of the data-parallel `sharded` exchange (csrc/shard.hip;
 * replaces the reference's never-synchronised DDP, ddp_lgcn.py:663-673).
 * Rank r of W owns rows i ≡ r (mod W); slot s of rank r is row r + s·W; a
 * block of slots [slot0, slot0 + n_slots) is all-gathered through a
 * [W][n_slots][dim] staging buffer.  pack: stage_rank[s] = table[rank +
 * (slot0 + s)·W] (rows past n_rows give zero rows).  unpack: table[w +
 * (slot0 + s)·W] = stage[w][s] for every w != rank (rows past n_rows
 * skipped) and, with x0s (and dinv), x0s[row] = dinv[row] · stage[w][s]. */
int mirec_shard_pack(const float *table, int64_t n_rows, int32_t dim, int32_t world,
                     int32_t rank, int64_t slot0, int64_t n_slots, float *stage_rank,
                     mirec_stream_t stream);
int mirec_shard_unpack(const float *stage, int64_t n_rows, int32_t dim, int32_t world,
                       int32_t rank, int64_t slot0, int64_t n_slots, const float *dinv,
                       float *table, float *x0s, mirec_stream_t stream);

/* Frontier bitmaps of a key set S (keys[n_keys], entries outside [0, n_rows)
 * ignored; or, if keys == NULL, the 3*batch nodes of the triples users[b],
 * n_users+pos[b], n_users+neg[b]):  bm_self = S, bm_hop = S ∪ N(S).  Both
 * are byte maps of ceil(n_rows/4)*4 bytes (4-byte aligned), cleared first
 * (with one memset when bm_hop starts right after bm_self's 16-byte-rounded
 * size).  If self_list
 * is given it receives the distinct nodes of S (in no particular order) and
 * *self_count their number (capacity: n_keys or 3*batch).  zero_counts[0 ..
 * n_zero_counts) (<= 256, may be NULL / 0) are set to 0 with the maps — the
 * counters of the mirec_mask_compact calls that follow (counts_zeroed = 1):
 * adjacent, 16-byte aligned maps, S count and counters clear in one launch. */
int mirec_frontier(const mirec_csr_t *csr, const int32_t *keys, int64_t n_keys,
                   const int32_t *users, const int32_t *pos, const int32_t *neg,
                   int64_t batch, int64_t n_users, uint8_t *bm_self,
                   uint8_t *bm_hop, int32_t *self_list, int32_t *self_count,
                   int32_t *zero_counts, int32_t n_zero_counts, mirec_stream_t stream);

/* Bit forms of a seed set S for the first backward layer's LDS prefilter
 * (mirec_propagate_seeded).  The nodes [0, split) and [split, n_rows) (users
 * and items of a bipartite graph) have an array each, range 0 first: bit
 * (node - range base) >> shift[r] of range r is set iff some node of S maps
 * to it, so shift 0 is S itself and a larger shift a superset of it.
 * `bits`: words[0] + words[1] device words, 4-byte aligned; words[r] * 32
 * bits must cover range r at shift[r] (MIREC_ERR_ARG otherwise). */
typedef struct mirec_seed_bits {
  uint32_t *bits;
  int64_t split;
  int32_t shift[2];
  int32_t words[2];
} mirec_seed_bits_t;

size_t mirec_seed_bits_sizeof(void);

/* mirec_frontier that also fills `sb` for the same S, with no launch more:
 * the words are cleared with the maps (by the one clear launch when sb->bits
 * starts right after bm_hop's 16-byte-rounded size and words[0] + words[1] is
 * a multiple of 4) and set with integer atomicOr by the lanes that set
 * bm_self.  sb == NULL is exactly mirec_frontier. */
int mirec_frontier_bits(const mirec_csr_t *csr, const int32_t *keys, int64_t n_keys,
                        const int32_t *users, const int32_t *pos, const int32_t *neg,
                        int64_t batch, int64_t n_users, uint8_t *bm_self,
                        uint8_t *bm_hop, int32_t *self_list, int32_t *self_count,
                        int32_t *zero_counts, int32_t n_zero_counts,
                        const mirec_seed_bits_t *sb, mirec_stream_t stream);

/* mirec_propagate for the list launch of the first backward layer (in_mode =
 * MIREC_IN_SPARSE with row lists, no in_mask), bit for bit: a persistent grid
 * whose workgroups hold `filter`'s bits in LDS, test every column against
 * them and read slot[col] of the passing ones only; the terms of a row are
 * the columns with slot >= 0, in mirec_propagate's order.  `filter` must
 * hold a superset of {v : slot[v] >= 0} (mirec_frontier_bits of the keys the
 * seeds were made from).  A launch of any other shape (another in_mode, no
 * row lists, an in_mask, edge values, scale vectors, long-row segments, bit
 * arrays beyond 64 KB) or filter == NULL runs mirec_propagate itself. */
int mirec_propagate_seeded(const mirec_csr_t *csr, const mirec_prop_t *p,
                           const mirec_seed_bits_t *filter, mirec_stream_t stream);

/* mirec_mask_compact of two byte maps in one launch (the step's S and F1 =
 * S ∪ N(S)), the degree split read from wide_bits (bit v of word v / 32:
 * degree of node v > narrow_max; built once per graph) instead of rowptr:
 * list_a / wide_a get map a's narrow / wide nodes, list_b / wide_b map b's;
 * counts[0..3] = their lengths (a narrow, a wide, b narrow, b wide), which
 * must be 0 on entry (mirec_frontier's zero_counts).  Lists ascending
 * within runs of 8 192 nodes; 16-byte aligned maps of >= n_rows bytes. */
int mirec_mask_compact_pair(const uint8_t *bm_a, const uint8_t *bm_b, const uint32_t *wide_bits,
                            int64_t n_rows, int32_t *list_a, int32_t *wide_a, int32_t *list_b,
                            int32_t *wide_b, int32_t *counts, mirec_stream_t stream);

/* Stable sort of n <= 8 192 (int32 key >= 0, int32 value) pairs: ascending
 * keys, equal keys in input order — bit for bit a stable radix sort's
 * result; vals_in NULL = the identity.  Two launches: every (key, index)
 * composite's rank counted over a grid of 256-entry blocks x 256-entry
 * chunks, then each pair written at its rank.  The sort of the BPR seed
 * grouping (mirec_bpr_seed: 3B node keys) and of small table-gradient
 * steps (mirec_table_grad_sorted); workspace: mirec_small_sort_workspace
 * bytes (ceil(n / 256) x n int32). */
int mirec_small_sort_workspace(int64_t n, size_t *bytes);
int mirec_small_sort_pairs(const int32_t *keys_in, const int32_t *vals_in, int32_t *keys_out,
                           int32_t *vals_out, int64_t n, void *workspace, size_t workspace_bytes,
                           mirec_stream_t stream);

/* Row lists of the nodes whose byte in the byte map bm[csr->n_rows] is
 * non-zero (16-byte aligned map): nodes of degree <= narrow_max (or all, if
 * wide_list is NULL) go to list[0 .. *count), the others to
 * wide_list[0 .. *wide_count); each list is ascending within runs of 4096
 * nodes, runs in no particular order (the result of a propagation does not
 * depend on list order).  Capacity: n_rows each.  Feeds the row_list /
 * wide_list of mirec_prop_t for the frontier-pruned launches.  The counts
 * are cleared first unless counts_zeroed (already 0 on this stream). */
int mirec_mask_compact(const mirec_csr_t *csr, const uint8_t *bm,
                       int32_t narrow_max, int32_t *list, int32_t *count,
                       int32_t *wide_list, int32_t *wide_count, int32_t counts_zeroed,
                       mirec_stream_t stream);

/* The ascending distinct ids of ids[0 .. n) that lie in [0, n_rows) and
 * outside [lo, hi) -> out[0 .. *count) (capacity n_rows): the rows a
 * data-parallel rank fetches from their owners before a GraphSAGE forward
 * (the fetch exchange of dist.DenseGradDataParallel; replaces torch.unique
 * of ddp-time bookkeeping, ddp_sage.py:754-878 has no exchange).  Byte map +
 * per-block counts + scan + ordered writes: no sort.  Workspace (16-byte
 * aligned): mirec_distinct_rows_workspace(n_rows) bytes. */
int64_t mirec_distinct_rows_workspace(int64_t n_rows);
int mirec_distinct_rows(const int32_t *ids, int64_t n, int64_t n_rows, int64_t lo,
                        int64_t hi, int32_t *out, int32_t *count, void *workspace,
                        size_t workspace_bytes, mirec_stream_t stream);
/* The same, skipping the ids whose byte in have[0 .. n_rows) is set, and
 * setting it for every id written: the pipelined exchange's read set of
 * micro-batch k without the rows fetched for micro-batches 0 .. k-1 (one
 * launch chain instead of a mask, a gather and a boolean compaction). */
int mirec_distinct_rows_unseen(const int32_t *ids, int64_t n, int64_t n_rows, int64_t lo,
                            int64_t hi, uint8_t *have, int32_t *out, int32_t *count,
                            void *workspace, size_t workspace_bytes, mirec_stream_t stream);

/* The rows r in [0, n_rows) with stamp[r] == gen (the rows a table gradient
 * of the sorted form wrote) ascending -> rows[0 .. counts[0]) (capacity
 * n_rows), and counts[1 + q] = those in owner block q of `parts` contiguous
 * blocks of n_rows / parts rows (the last to n_rows) — all on the device, no
 * host round trip: the pipelined fetch exchange's export of a micro-batch's
 * table-gradient rows (dist.DenseGradDataParallel; replaces torch.nonzero +
 * bincount).  Workspace: mirec_distinct_rows_workspace(n_rows) bytes. */
int mirec_stamped_rows(const int32_t *stamp, int64_t n_rows, int32_t gen, int32_t parts,
                       int32_t *rows, int32_t *counts, void *workspace,
                       size_t workspace_bytes, mirec_stream_t stream);

/* dst[ids[i], :] = src[i, :] for i < n (ids distinct; ids < 0 skipped);
 * dim % 4 == 0, src and dst 16-byte aligned: the install of the rows a rank
 * fetched into its local table (replaces index_copy_). */
int mirec_scatter_rows(const float *src, const int32_t *ids, int64_t n, int32_t dim,
                       float *dst, mirec_stream_t stream);

/* One source block of rows for mirec_owner_sum: ids[0 .. n) distinct,
 * rows [n, dim]. */
typedef struct mirec_row_block {
  const int32_t *ids;
  const float *rows;
  int64_t n;
} mirec_row_block_t;

/* out[r - lo, :] = sum over the blocks, IN BLOCK ORDER, of rows[i, :] where
 * ids[i] == r, for every r of the own block [lo, lo + n_own) (0 where no
 * block has r; ids outside the block ignored) — bitwise the sequence of
 * index_add_ launches it replaces (the owner side of the data-parallel
 * table-gradient exchange, dist.DenseGradDataParallel._owner_adam), in one
 * pass per 64 blocks.  Workspace: mirec_owner_sum_workspace(n_blocks, n_own)
 * bytes. */
int64_t mirec_owner_sum_workspace(int32_t n_blocks, int64_t n_own);
int mirec_owner_sum(const mirec_row_block_t *blocks, int32_t n_blocks, int64_t lo,
                    int64_t n_own, int32_t dim, void *workspace, size_t workspace_bytes,
                    float *out, mirec_stream_t stream);

/* out[i, :] = src[rows[i], :] for i < *count, the count read on the device
 * (capacity rows of out); dim % 4 == 0, src and out 16-byte aligned. */
int mirec_gather_rows_counted(const float *src, const int32_t *rows, const int32_t *count,
                              int64_t capacity, int32_t dim, float *out,
                              mirec_stream_t stream);

/* Capacity-bounded routing of a read set (the pipelined fetch exchange's
 * planner; replaces the per-read-set count read of ddp_sage.py:800-806's
 * exchange).  mirec_route_pack: ids ascending int32, *count (device) of them
 * valid, capacity = the ids buffer's length; writes one block per owner q
 * (contiguous row blocks of n_rows / parts, the last to n_rows) at
 * blocks + q*stride: blocks[q*stride] = the count of owner q's ids, then up
 * to cap of them (stride >= cap + 1; a count above cap is written as it is,
 * its ids past cap dropped: the host checks counts <= cap).  parts <= 256.
 * mirec_gather_rows_routed: the owner side over received blocks of that
 * layout: out[Σ_{p<q} min(c_p, cap) + j, :] = table[id_{q,j}, :], in source
 * order; out holds parts*cap rows of dim floats (ids outside [0, n_rows)
 * give zero rows). */
int mirec_route_pack(const int32_t *ids, const int32_t *count, int64_t capacity, int64_t n_rows,
                     int32_t parts, int32_t cap, int64_t stride, int32_t *blocks,
                     mirec_stream_t stream);
int mirec_gather_rows_routed(const float *table, int64_t n_rows, const int32_t *blocks,
                             int32_t parts, int32_t cap, int64_t stride, int32_t dim, float *out,
                             mirec_stream_t stream);

/* ------------------------------------------------------------------------ */
/* BPR (model/lgcn.py:98-133)                                                */
/* ------------------------------------------------------------------------ */

/* Scores of B triples from the layer-mean embeddings `out` [N, dim] and the
 * ego embeddings `emb` [N, dim] (users are rows [0, n_users), item ids are
 * offset by n_users).  Writes, per triple t:
 *   softplus[t] = softplus(<u,n> - <u,p>)          (torch threshold 20)
 *   coef[t]     = grad_scale * d mean(softplus) / d(neg - pos)
 *   reg[t]      = 1/2 (|u0|^2 + |p0|^2 + |n0|^2)
 * and the 3B seed keys/values (node id, occurrence index) consumed by
 * mirec_bpr_seed. */
int mirec_bpr_forward(const float *out, const float *emb, int64_t n_nodes,
                      int64_t n_users, int32_t dim, int64_t batch,
                      const int32_t *users, const int32_t *pos,
                      const int32_t *neg, float grad_scale, float *coef,
                      float *softplus, float *reg, int32_t *keys,
                      int32_t *vals, mirec_stream_t stream);

/* loss = mean(softplus) + decay * sum(reg) / B, written to loss_out[0];
 * if loss_accum != NULL also loss_accum[0] += loss (OneEpoch's aver_loss). */
int mirec_bpr_loss(const float *softplus, const float *reg, int64_t batch,
                   float decay, float *loss_out, float *loss_accum,
                   mirec_stream_t stream);

/* Scratch bytes mirec_bpr_seed needs for a batch of `batch` triples over a
 * graph of n_nodes nodes. */
int mirec_bpr_seed_workspace(int64_t batch, int64_t n_nodes, size_t *bytes);

/* Gradient seeds of the backward pass.  Sorts the 3B (node, occurrence)
 * pairs stably (mirec_small_sort_pairs up to 8 192 pairs, the device
 * library's radix sort above), marks the first position q of every distinct
 * node in `slot` (slot[node] = q; slot must be all -1 on entry) and writes
 *   seed_p[q] = (sum over the node's occurrences of dLoss/d out_node) / (L+1)
 *   seed_e[q] = decay * (#occurrences) * emb[node] / B   (reg term)
 * summed in occurrence order (deterministic).  keys_sorted[3B] keeps the
 * sorted node ids for mirec_bpr_seed_reset. */
int mirec_bpr_seed(const float *out, const float *emb, int64_t n_nodes,
                   int64_t n_users, int32_t dim, int64_t batch,
                   const int32_t *users, const int32_t *pos,
                   const int32_t *neg, const float *coef,
                   const int32_t *keys, const int32_t *vals, float decay,
                   float grad_scale, int32_t n_layers, int32_t *slot, float *seed_p,
                   float *seed_e, int32_t *keys_sorted, void *workspace,
                   size_t workspace_bytes, mirec_stream_t stream);

/* slot[keys_sorted[q]] = -1 for q in [0, n) (negative keys are skipped). */
int mirec_bpr_seed_reset(int32_t *slot, const int32_t *keys_sorted, int64_t n,
                         mirec_stream_t stream);

/* Dense pre-scaled seed rows: dense[v] = dinv[v] * seed[slot[v]] for the
 * listed nodes v = list[i], i < *count (device count, host bound cap), or
 * zeros when clear != 0 (restoring an all-zero table).  Feeds the first
 * backward layer as a PRESCALED input filtered by the S byte map. */
int mirec_seed_dense(const int32_t *list, const int32_t *count, int64_t cap,
                     const int32_t *slot, const float *dinv, const float *seed,
                     int32_t dim, float *dense, int32_t clear, mirec_stream_t stream);

/* Data-parallel sparse gradient exchange (dist.py).  The backward pass is
 * linear in the seeds, so the union batch's gradient is the backward of the
 * SUM of every rank's seeds: ranks all-gather their (node, seed_p, seed_e)
 * rows (3B each) instead of all-reducing the dense [N, D] gradient.
 * pack: keys_packed[q] = keys_sorted[q] at head positions, n_nodes elsewhere. */
int mirec_seed_pack(const int32_t *keys_sorted, int64_t n, int64_t n_nodes,
                    int32_t *keys_packed, mirec_stream_t stream);

int mirec_seed_merge_workspace(int64_t n, int64_t n_nodes, size_t *bytes);

/* merge: n gathered (key, row_p, row_e) entries (key == n_nodes: empty) →
 * per distinct node the sum of its rows in gathered order (deterministic,
 * identical on every rank), written at the node's first sorted position q;
 * slot[node] = q (slot must be all -1 on entry); keys_sorted[n] keeps the
 * sorted keys (-1 for empty entries) for mirec_bpr_seed_reset. */
int mirec_seed_merge(const int32_t *keys_packed, const float *rows_p,
                     const float *rows_e, int64_t n, int32_t dim,
                     int64_t n_nodes, int32_t *slot, float *seed_p,
                     float *seed_e, int32_t *keys_sorted, void *workspace,
                     size_t workspace_bytes, mirec_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Sampled softmax: K = n_neg negatives per positive (csrc/ssm.hip; the      */
/* intent of model/lgcnssm.py's softmax_loss; K = 1, temp = 1 is BPR)        */
/* ------------------------------------------------------------------------ */

/* Pair t = (users[t], pos[t]) has the negatives neg[t * n_neg + k] (item
 * ids without the n_users offset), temp > 0 is the temperature.  With
 * s+ = <out_u, out_p> / temp and s_k = <out_u, out_nk> / temp:
 *   terms[t]     = logsumexp(s+, s_0 .. s_{K-1}) - s+   (max-subtracted)
 *   reg[t]       = 1/2 (|e_u|^2 + |e_p|^2 + sum_k |e_nk|^2)  (a negative
 *                  drawn twice counts twice)
 *   coef[t*K+k]  = grad_scale * softmax weight of negative k / (B temp)
 *   coef_pos[t]  = sum_k coef[t*K+k]
 *   g_u[t, :]    = sum_k coef[t*K+k] out_nk - coef_pos[t] out_p  (the user
 *                  row's gradient, summed k = 0 .. K-1, then the positive)
 * and the (2 + K) B seed keys / values (node id, occurrence index) of
 * mirec_ssm_seed: occurrence t is the user of pair t, B + t its positive,
 * 2B + t K + k its negative k.  The loss is mirec_bpr_loss(terms, reg).
 * MIREC_ERR_ARG: a NULL pointer, batch < 1, n_neg < 1, temp <= 0 or not
 * finite, an unsupported dim, (2 + K) B >= 2^31. */
int mirec_ssm_forward(const float *out, const float *emb, int64_t n_nodes,
                      int64_t n_users, int32_t dim, int64_t batch, int32_t n_neg,
                      const int32_t *users, const int32_t *pos, const int32_t *neg,
                      float temp, float grad_scale, float *coef, float *coef_pos,
                      float *terms, float *reg, float *g_u, int32_t *keys,
                      int32_t *vals, mirec_stream_t stream);

/* The keys of mirec_ssm_forward alone (keys[(2 + K) B]: users, n_users +
 * pos, n_users + neg): the batch's node list for mirec_frontier's key form,
 * which a pruned forward needs before the scores exist. */
int mirec_ssm_keys(const int32_t *users, const int32_t *pos, const int32_t *neg,
                   int64_t batch, int32_t n_neg, int64_t n_users, int32_t *keys,
                   mirec_stream_t stream);

/* Scratch bytes mirec_ssm_seed needs. */
int mirec_ssm_seed_workspace(int64_t batch, int32_t n_neg, int64_t n_nodes, size_t *bytes);

/* Gradient seeds from mirec_ssm_forward's outputs, laid out as
 * mirec_bpr_seed's: stable sort of the (2 + K) B pairs (the small sort up to
 * 8 192 pairs, the radix sort above), slot[node] = q at the first position
 * of every distinct node (slot all -1 on entry), and
 *   seed_p[q] = (sum over the node's occurrences, in occurrence order, of
 *                1 * g_u[t] | -coef_pos[t] * out_u | coef[t*K+k] * out_u
 *                for a user | positive | negative occurrence) / (L+1)
 *   seed_e[q] = decay * (#occurrences) * emb[node] / B * grad_scale
 * keys_sorted[(2 + K) B] feeds mirec_bpr_seed_reset.  Deterministic: one
 * fixed summation order, no float atomics. */
int mirec_ssm_seed(const float *out, const float *emb, int64_t n_nodes, int64_t n_users,
                   int32_t dim, int64_t batch, int32_t n_neg, const int32_t *users,
                   const float *coef, const float *coef_pos, const float *g_u,
                   const int32_t *keys, const int32_t *vals, float decay,
                   float grad_scale, int32_t n_layers, int32_t *slot, float *seed_p,
                   float *seed_e, int32_t *keys_sorted, void *workspace,
                   size_t workspace_bytes, mirec_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Sampled softmax with one set of m negatives per batch, shared by all B   */
/* pairs (csrc/ssm_shared.hip)                               */
/* ------------------------------------------------------------------------ */

/* Pairs (users[t], pos[t]), t < B, and the shared item ids shared[j], j < m
 * (no n_users offset; drawn with replacement, a repeated id counts twice
 * everywhere).  Occurrence t is the user of pair t, B + t its positive,
 * 2B + j shared slot j: keys[2B + m] = users, n_users + pos, n_users +
 * shared — the batch's node list for mirec_frontier's key form.
 * Every entry point of this section returns MIREC_ERR_ARG for a NULL
 * pointer, batch < 1, m < 1, B m >= 2^31 or 2B + m >= 2^31 (the forward also
 * for temp <= 0 or not finite and an unsupported dim) and then writes
 * nothing. */
int mirec_ssm_shared_keys(const int32_t *users, const int32_t *pos, const int32_t *shared,
                          int64_t batch, int64_t m, int64_t n_users, int32_t *keys,
                          mirec_stream_t stream);

/* mask[t * m + j] = 1 iff shared[j] is a training positive of users[t] (an
 * entry of CSR row users[t]: binary search in csr->col_sorted when the CSR
 * carries it for the user rows, else a scan of the row, as the samplers
 * test a negative) or shared[j] == pos[t]; else 0.  A masked candidate is
 * left out of pair t's softmax. */
int mirec_ssm_shared_mask(const mirec_csr_t *csr, const int32_t *users, int64_t batch,
                          const int32_t *pos, const int32_t *shared, int64_t m,
                          int64_t n_users, uint8_t *mask, mirec_stream_t stream);

/* With s+ = <out_u, out_p> / temp, s_j = <out_u, out_nj> / temp and the
 * softmax of pair t taken over s+ and its unmasked s_j (max-subtracted):
 *   terms[t]      = logsumexp - s+      (exactly 0 when every j is masked)
 *   coef[t*m + j] = grad_scale * weight of candidate j / (B temp), exactly 0
 *                   when masked;  coef_pos[t] = sum_j coef[t*m + j]
 *   reg[t]        = 1/2 (|e_u|^2 + |e_p|^2);  reg_shared[j] = 1/2 |e_nj|^2
 *   g[t, :]       = sum_j coef[t*m + j] out_nj - coef_pos[t] out_p   (t < B)
 *   g[B + j, :]   = sum_t coef[t*m + j] out_u_t                      (j < m)
 * and the 2B + m seed (keys, vals) = (node id, occurrence index).  Every
 * sum has one fixed order (scores: d ascending; the row sums over j: lane l
 * of 64 takes j = l, l + 64, .., then a xor tree; g: j, resp. t, ascending,
 * then the positive), none depends on the launch shape or on the other
 * pairs of the batch; no float atomics.  The loss is mirec_ssm_shared_loss. */
int mirec_ssm_shared_forward(const float *out, const float *emb, int64_t n_nodes,
                             int64_t n_users, int32_t dim, int64_t batch, int64_t m,
                             const int32_t *users, const int32_t *pos, const int32_t *shared,
                             const uint8_t *mask, float temp, float grad_scale, float *coef,
                             float *coef_pos, float *terms, float *reg, float *reg_shared,
                             float *g, int32_t *keys, int32_t *vals, mirec_stream_t stream);

/* loss_out[0] = sum_t terms[t] / B + decay * (sum_t reg[t] + sum_j
 * reg_shared[j]) / B (one workgroup, fixed partition and tree); if
 * loss_accum != NULL also loss_accum[0] += that.  A shared row's norm counts
 * once per slot, not once per pair: with m = 1 this is not mirec_bpr_loss's
 * reg, which counts the negative's norm B times. */
int mirec_ssm_shared_loss(const float *terms, const float *reg, const float *reg_shared,
                          int64_t batch, int64_t m, float decay, float *loss_out,
                          float *loss_accum, mirec_stream_t stream);

/* Scratch bytes mirec_ssm_shared_seed needs. */
int mirec_ssm_shared_seed_workspace(int64_t batch, int64_t m, int64_t n_nodes, size_t *bytes);

/* Gradient seeds from mirec_ssm_shared_forward's outputs, laid out as
 * mirec_ssm_seed's: stable sort of the 2B + m pairs (the small sort up to
 * 8 192 pairs, the radix sort above), slot[node] = q at the head of every
 * run (slot all -1 on entry), and
 *   seed_p[q] = (sum over the node's occurrences, in occurrence order, of
 *                1 * g[t] | -coef_pos[t] * out_u | 1 * g[B + j]
 *                for a user | positive | shared occurrence) / (L+1)
 *   seed_e[q] = decay * (#occurrences) * emb[node] / B * grad_scale
 * keys_sorted[2B + m] feeds mirec_bpr_seed_reset.  MIREC_ERR_WORKSPACE on a
 * short workspace. */
int mirec_ssm_shared_seed(const float *out, const float *emb, int64_t n_nodes, int64_t n_users,
                          int32_t dim, int64_t batch, int64_t m, const int32_t *users,
                          const float *coef_pos, const float *g, const int32_t *keys,
                          const int32_t *vals, float decay, float grad_scale, int32_t n_layers,
                          int32_t *slot, float *seed_p, float *seed_e, int32_t *keys_sorted,
                          void *workspace, size_t workspace_bytes, mirec_stream_t stream);

/* n_sets shared sets of m item ids: out[b * m + j] uniform over [0,
 * m_items), with replacement and without rejection.  Element b * m + j is
 * one draw of the stream keyed by (seed, the sampler's own domain tag,
 * offset) at counter b * m + j: set b does not depend on n_sets or the
 * launch shape, and calls with different offsets are independent.
 * MIREC_ERR_ARG: out NULL, m_items < 1, n_sets < 1, m < 1, n_sets m >= 2^31. */
int mirec_shared_sample(int64_t m_items, int64_t n_sets, int64_t m, uint64_t seed,
                        uint64_t offset, int32_t *out, mirec_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Adam (torch.optim.Adam, amsgrad=False, weight_decay=0)                   */
/* ------------------------------------------------------------------------ */

int mirec_adam_dense(float *param, const float *grad, float *exp_avg,
                     float *exp_avg_sq, int64_t n,
                     const mirec_adam_hparams_t *h, mirec_stream_t stream);

/* Multi-tensor form for the small parameters of a model sharing one step
 * count: count (param, grad, exp_avg, exp_avg_sq, numel) tensors given as
 * host arrays of device pointers, one launch per 32 tensors.  Same update
 * as mirec_adam_dense. */
int mirec_adam_multi(int32_t count, float *const *params, const float *const *grads,
                     float *const *exp_avg, float *const *exp_avg_sq,
                     const int64_t *numel, const mirec_adam_hparams_t *hp,
                     mirec_stream_t stream);

/* The same two updates with the hyper-parameters read from DEVICE memory
 * when the kernel runs (h_device: one mirec_adam_hparams_t), so a captured
 * HIP graph replays each step with the scalars the host wrote there for
 * that step (bias corrections change every step). */
int mirec_adam_dense_dev(float *param, const float *grad, float *exp_avg,
                         float *exp_avg_sq, int64_t n,
                         const mirec_adam_hparams_t *h_device, mirec_stream_t stream);
int mirec_adam_multi_dev(int32_t count, float *const *params, const float *const *grads,
                         float *const *exp_avg, float *const *exp_avg_sq,
                         const int64_t *numel, const mirec_adam_hparams_t *h_device,
                         mirec_stream_t stream);

/* ------------------------------------------------------------------------ */
/* On-device BPR sampler (negative_sample.py:98-134 semantics)               */
/* ------------------------------------------------------------------------ */

/* Draws `batch` triples: u uniform over the users of shard `shard` (users
 * u with u % n_shards == shard; n_shards = 1 → all users), users with no
 * positives are redrawn, p uniform over u's CSR row (allPos order), n
 * uniform over [0, m_items) rejected while n is a positive of u.  Counter-
 * based: triple t of a call uses stream (seed, offset + t), so a batch is
 * reproducible and independent of the launch shape.  Item ids are returned
 * without the n_users offset.  err[0] is set to 1 if a draw exhausted its
 * retry budget (a user with every item as a positive). */
int mirec_bpr_sample(const mirec_csr_t *csr, int64_t n_users, int64_t m_items,
                     int64_t batch, uint64_t seed, uint64_t offset,
                     int32_t shard, int32_t n_shards, int32_t *users,
                     int32_t *pos, int32_t *neg, int32_t *err,
                     mirec_stream_t stream);

/* The ddp_lgcn.py epoch sampler (ddp_lgcn.py:33-35, 541-582): n_candidates
 * users drawn uniformly from the shard (users without positives are
 * skipped), a uniform positive each, and a candidate kept only if fewer than
 * `cap` earlier candidates (draw order) with the same positive item were kept
 * (POSITIVE_NUM_LIMIT = 3000); the kept ones (in draw order) draw a negative
 * not among the user's positives.  users / pos / neg: capacity n_candidates;
 * count[0] (device) = kept triples.  cand_u / cand_p (optional, [n]): every
 * candidate's user and positive (-1 = skipped).  Workspace:
 * mirec_bpr_sample_capped_workspace bytes. */
int mirec_bpr_sample_capped_workspace(int64_t n_candidates, int64_t m_items, size_t *bytes);

/* The same two samplers with per-user positive probabilities (the sample_pow
 * option of UniformSampling.sample_parallel, negative_sample.py:53-56:
 * np.random.choice(len(allPos[u]), p=probs[u])): pos_cdf[e - rowptr[0]]
 * is the inclusive cumulative probability of entry e within its user row
 * (rows 0 .. n_users - 1 of the CSR, i.e. the allPos order), non-decreasing
 * in the row, its last entry exactly 1.0, in float64 (mirec_pos_cdf_build makes
 * it on the host).  The positive is the first entry whose cumulative
 * probability exceeds a uniform draw on the 2^-53 grid (numpy's searchsorted
 * 'right' over its float64 CDF);
 * with pos_cdf = NULL they are the functions above (bit for bit). */
/* Host: cdf from probs[e - rowptr[0]] (float64, per user-row entry, each
 * non-empty row non-negative with a positive sum; normalised per row in
 * float64 as numpy's choice does).  MIREC_ERR_ARG on a negative / NaN entry
 * or a zero row. */
int mirec_pos_cdf_build(const int64_t *rowptr, int64_t n_users, const double *probs,
                        double *cdf);
int mirec_bpr_sample_ex(const mirec_csr_t *csr, const double *pos_cdf, int64_t n_users,
                        int64_t m_items, int64_t batch, uint64_t seed, uint64_t offset,
                        int32_t shard, int32_t n_shards, int32_t *users, int32_t *pos,
                        int32_t *neg, int32_t *err, mirec_stream_t stream);
int mirec_bpr_sample_capped(const mirec_csr_t *csr, int64_t n_users, int64_t m_items,
                            int64_t n_candidates, int32_t cap, uint64_t seed, uint64_t offset,
                            int32_t shard, int32_t n_shards, int32_t *users, int32_t *pos,
                            int32_t *neg, int32_t *count, int32_t *err, int32_t *cand_u,
                            int32_t *cand_p, void *workspace, size_t workspace_bytes,
                            mirec_stream_t stream);
int mirec_bpr_sample_capped_ex(const mirec_csr_t *csr, const double *pos_cdf, int64_t n_users,
                               int64_t m_items, int64_t n_candidates, int32_t cap,
                               uint64_t seed, uint64_t offset, int32_t shard, int32_t n_shards,
                               int32_t *users, int32_t *pos, int32_t *neg, int32_t *count,
                               int32_t *err, int32_t *cand_u, int32_t *cand_p, void *workspace,
                               size_t workspace_bytes, mirec_stream_t stream);

/* mirec_bpr_sample_ex with n_neg >= 1 negatives per pair (sampled softmax):
 * pair t draws from the same stream (seed, offset + t) the same user,
 * positive and first negative, then continues it for negatives 1 .. n_neg-1,
 * each uniform over [0, m_items) and rejected while it is a positive of u
 * (with replacement among themselves).  neg is [batch, n_neg] row-major;
 * with n_neg = 1 the output is mirec_bpr_sample_ex's bit for bit. */
int mirec_ssm_sample(const mirec_csr_t *csr, const double *pos_cdf, int64_t n_users,
                     int64_t m_items, int64_t batch, int32_t n_neg, uint64_t seed,
                     uint64_t offset, int32_t shard, int32_t n_shards, int32_t *users,
                     int32_t *pos, int32_t *neg, int32_t *err, mirec_stream_t stream);

/* ------------------------------------------------------------------------ */
/* GraphSAGE hop ops (model/graphsage.py:311-324, neighbor_sampling.py)      */
/* ------------------------------------------------------------------------ */

/* Fixed-fanout sampling WITH replacement (neighbor_sampling.py:14-30):
 * children[t*k + c] = a uniform entry of the CSR row of nodes[t]
 * (counter RNG keyed by (seed, offset + t*k + c)); -1 if the row is empty. */
int mirec_sample_fanout(const mirec_csr_t *csr, const int32_t *nodes, int64_t n,
                        int32_t k, uint64_t seed, uint64_t offset,
                        int32_t *children, mirec_stream_t stream);

/* out[0, B) = users, out[B, 2B) = n_users + pos, out[2B, 3B) = n_users + neg
 * (the seed node ids of a BPR batch in a [users ; items] id table). */
int mirec_pack_seed_nodes(const int32_t *users, const int32_t *pos, const int32_t *neg,
                          int64_t batch, int64_t n_users, int32_t *out, mirec_stream_t stream);

/* Fixed-fanout sampling WITHOUT replacement (PyG NeighborSampler, the
 * sampler of model/graphsage.py:342-365): a node with at most k entries keeps
 * all of them in row order and -1 in the remaining slots; otherwise k
 * distinct entries of its row, uniformly (Floyd's algorithm on counter RNG
 * (seed, offset + t*k + j)).  Nodes without neighbours get k x -1 (their
 * mean is 0, as PyG's scatter-mean over no edges). */
int mirec_sample_fanout_norep(const mirec_csr_t *csr, const int32_t *nodes, int64_t n,
                              int32_t k, uint64_t seed, uint64_t offset, int32_t *children,
                              mirec_stream_t stream);

/* out[i, :] = table[ids[i], :] (zeros for ids[i] < 0); dim % 4 == 0. */
int mirec_gather_rows(const float *table, const int32_t *ids, int64_t n,
                      int32_t dim, float *out, mirec_stream_t stream);

/* table_grad[ids[i], :] += grad[i, :] (float atomics; ids < 0 skipped). */
int mirec_scatter_add_rows(const float *grad, const int32_t *ids, int64_t n,
                           int32_t dim, float *table_grad, mirec_stream_t stream);

/* out[t] = mean over the children c in [0,k) with valid[t*k+c] >= 0 (all if
 * valid == NULL) of dropout_p-dropout(x[t*k + c]); 0 if no valid child.
 * Dropout keeps an element with probability 1-p and scales it by 1/(1-p);
 * the mask is the element dropout stated above (after mirec_edge_keep_mask)
 * at element index (t*k + c)*dim + col, so the backward recomputes it.
 * dim % 4 == 0. */
int mirec_fanout_mean(const float *x, const int32_t *valid, int64_t n_targets,
                      int32_t k, int32_t dim, float dropout_p, uint64_t seed,
                      float *out, mirec_stream_t stream);

/* Backward of mirec_fanout_mean: grad_x[t*k + c] (written, not added). */
int mirec_fanout_mean_bwd(const float *grad_out, const int32_t *valid,
                          int64_t n_targets, int32_t k, int32_t dim,
                          float dropout_p, uint64_t seed, float *grad_x,
                          mirec_stream_t stream);

/* Fused leaf hop: out[t] = mean over the children c in [0,k) with
 * ids[t*k+c] >= 0 of dropout_p-dropout(table[ids[t*k+c]]) — the row gather
 * and mirec_fanout_mean in one pass (same dropout mask as gathering first
 * and calling mirec_fanout_mean).  The backward adds mask * grad_out[t] /
 * cnt into table_grad[ids[t*k+c]] (float atomics; k <= 64).  dim % 4 == 0. */
int mirec_fanout_mean_gather(const float *table, const int32_t *ids, int64_t n_targets,
                             int32_t k, int32_t dim, float dropout_p, uint64_t seed,
                             float *out, mirec_stream_t stream);
int mirec_fanout_mean_gather_bwd(const float *grad_out, const int32_t *ids,
                                 int64_t n_targets, int32_t k, int32_t dim,
                                 float dropout_p, uint64_t seed, float *table_grad,
                                 mirec_stream_t stream);

/* Deterministic form of mirec_fanout_mean_gather_bwd: the entries are
 * radix-sorted by child id and each id's contributions are summed in entry
 * order and added to its row once (no float atomics).  n_rows = rows of the
 * table (child ids < n_rows); workspace: ..._sorted_workspace bytes. */
int mirec_fanout_mean_gather_bwd_sorted_workspace(int64_t n_targets, int32_t k, int32_t n_rows,
                                                  size_t *bytes);
int mirec_fanout_mean_gather_bwd_sorted(const float *grad_out, const int32_t *ids,
                                        int64_t n_targets, int32_t k, int32_t dim,
                                        float dropout_p, uint64_t seed, int32_t n_rows,
                                        float *table_grad, void *workspace,
                                        size_t workspace_bytes, mirec_stream_t stream);

/* LightSAGE hop (model/lightsage.py:274-290: no weights, no ReLU): for target
 * t with the k child slots t*k .. t*k + k - 1,
 *   out[t] = self_t + (1 / cnt_t) * sum over the valid slots c, in slot order,
 *            of dropout(child row of slot t*k + c)
 * cnt_t = the number of valid slots; a target without one gets self_t.  The
 * dropout is the element dropout stated above at element index (t*k + c)*dim
 * + col.  dim % 4 == 0, k >= 1, float rows 16-byte aligned; bad arguments
 * (dropout_p outside [0, 1), NaN included) return MIREC_ERR_ARG and launch
 * nothing.
 * _gather (the first layer, nothing materialised): self_t = table[self_ids[t]]
 * (a zero row for an id < 0), slot e is valid iff child_ids[e] >= 0 and its
 * row is table[child_ids[e]].
 * The plain form: self_t = x_self[t], slot e's row is x_child[e], valid iff
 * valid[e] >= 0 (all valid if valid == NULL).  On x_child = the gathered
 * table rows and x_self = the gathered self rows the two forms give the same
 * bits. */
int mirec_fanout_resmean_gather(const float *table, const int32_t *self_ids,
                                const int32_t *child_ids, int64_t n_targets, int32_t k,
                                int32_t dim, float dropout_p, uint64_t seed, float *out,
                                mirec_stream_t stream);
int mirec_fanout_resmean(const float *x_self, const float *x_child, const int32_t *valid,
                         int64_t n_targets, int32_t k, int32_t dim, float dropout_p,
                         uint64_t seed, float *out, mirec_stream_t stream);

/* Backward of both forms: grad_self[t] = grad_out[t]; grad_child[t*k + c] =
 * mask * scale * grad_out[t] / cnt_t, a zero row for an invalid slot.  Both
 * outputs are written, not added to. */
int mirec_fanout_resmean_bwd(const float *grad_out, const int32_t *valid, int64_t n_targets,
                             int32_t k, int32_t dim, float dropout_p, uint64_t seed,
                             float *grad_self, float *grad_child, mirec_stream_t stream);

/* Graph-attention hop (PyG GATConv, concat=True, add_self_loops=True, no
 * attention dropout; model/gnn.py:196-206) on the same fixed-fanout tree.
 * Rows are the projected features z = x Wᵀ, D = heads * ch floats, head h
 * the columns [h ch, (h + 1) ch).  For target t and head h, over the slots j
 * = the children c with valid[t*k + c] >= 0 (all if valid == NULL; a repeated
 * id counts once per slot) and the self slot, which is always present:
 *   s_j = <z_j,h, att_src_h> + <z_t,h, att_dst_h>
 *   e_j = s_j > 0 ? s_j : slope * s_j
 *   alpha_j = exp(e_j - max e) / sum exp(e - max e)
 *   out[t, h] = sum_j alpha_j z_j,h  (+ bias if not NULL)
 * A target without a valid child gives z_self (+ bias) exactly.  alpha, if
 * not NULL, receives [n_targets, k + 1, heads] with slot k the self slot and
 * exactly 0 in the invalid slots.  Every child row is read once.
 * Shapes: ch % 4 == 0, 1 <= heads <= 8, heads * ch <= 256, 1 <= k <= 64, row
 * pointers 16-byte aligned; anything else is MIREC_ERR_ARG, nothing launched. */
int mirec_fanout_gat(const float *z_child, const float *z_self, const int32_t *valid,
                     const float *att_src, const float *att_dst, const float *bias,
                     int64_t n_targets, int32_t k, int32_t heads, int32_t ch, float slope,
                     float *out, float *alpha, mirec_stream_t stream);

/* Backward of mirec_fanout_gat from the kept alpha, per head with g =
 * grad_out[t, h]:  dalpha_j = <g, z_j>,  de_j = alpha_j (dalpha_j - sum_m
 * alpha_m dalpha_m),  ds_j = de_j (s_j > 0 ? 1 : slope)  (s_j recomputed),
 *   grad_z_child[t*k + c] = alpha_c g + ds_c att_src  (0 for an invalid slot)
 *   grad_z_self[t] = alpha_self g + ds_self att_src + (sum_j ds_j) att_dst
 *   grad_att_src = sum_t sum_j ds_j z_j,  grad_att_dst = sum_t (sum_j ds_j) z_t
 * All four are written, not added to.  The parameter sums are per-block
 * partial sums in work (mirec_fanout_gat_bwd_work_floats floats; -1 for a
 * shape the kernels do not take) added in block order by a final launch: no
 * float atomics, the same bits from run to run.  The child rows are read
 * twice.  Same shape limits as the forward. */
int64_t mirec_fanout_gat_bwd_work_floats(int64_t n_targets, int32_t k, int32_t heads,
                                         int32_t ch);
int mirec_fanout_gat_bwd(const float *grad_out, const float *z_child, const float *z_self,
                         const int32_t *valid, const float *att_src, const float *att_dst,
                         const float *alpha, int64_t n_targets, int32_t k, int32_t heads,
                         int32_t ch, float slope, float *grad_z_child, float *grad_z_self,
                         float *grad_att_src, float *grad_att_dst, float *work,
                         mirec_stream_t stream);

/* The same forward over every row of a CSR graph (full-graph inference):
 * row r attends over its col entries (a multi-edge once per entry) and its
 * self loop; a row without entries gives z_r (+ bias).  Reads rowptr and col
 * only (dinv, val and the split arrays are ignored); entries outside [0,
 * n_rows) are skipped.  logits: [n_rows, 2 * heads] scratch, written by a
 * first launch (<z_r,h, att_src_h> then <z_r,h, att_dst_h>).  Any degree: one
 * lane group walks a row.  heads / ch limits as mirec_fanout_gat. */
int mirec_csr_gat(const mirec_csr_t *csr, const float *z, const float *att_src,
                  const float *att_dst, const float *bias, int32_t heads, int32_t ch,
                  float slope, float *out, float *logits, mirec_stream_t stream);

/* Dot-product attention hop (PyG TransformerConv, concat=True, beta=False, no
 * edge features, no attention dropout, root_weight=True; model/tgrec.py:
 * 161-171) on the same fixed-fanout tree.  Rows are projected features of D =
 * heads * ch floats, head h the columns [h ch, (h + 1) ch): query / skip rows
 * of the targets at stride ld_q, key / value rows of the children at stride
 * ld_kv (strides in floats, so q | skip and k | v may be the halves of one
 * [n, 2D] GEMM output).  For target t and head h, over the slots j = the
 * children c with valid[t*k + c] >= 0 (all if valid == NULL; a repeated id
 * counts once per slot; there is NO self slot):
 *   s_j = <query[t],h, key[t*k + j],h> * scale
 *   alpha_j = exp(s_j - max s) / sum exp(s - max s)
 *   out[t, h] = sum_j alpha_j value[t*k + j],h  (+ skip[t],h if skip != NULL)
 * A target without a valid child gives its skip row exactly as stored (zeros
 * without skip) and alpha slots of exactly 0.  out is contiguous [n_targets,
 * D]; alpha, if not NULL, receives [n_targets, k, heads] with exactly 0 in
 * the invalid slots.  Every key row and every value row is read once.
 * Shapes: ch % 4 == 0, 1 <= heads <= 8, heads * ch <= 256, 1 <= k <= 64,
 * every stride >= D and a multiple of 4, every pointer 16-byte aligned,
 * scale not NaN; anything else is MIREC_ERR_ARG, nothing launched (checked
 * before any device call).  n_targets == 0 is MIREC_OK.  The rows must be
 * finite and their logits too: a logit of -inf (a dot that overflowed) has
 * weight 0, and a target whose valid slots all have it divides 0 by 0. */
int mirec_fanout_tattn(const float *query, const float *skip, int64_t ld_q,
                       const float *key, const float *value, int64_t ld_kv,
                       const int32_t *valid, int64_t n_targets, int32_t k,
                       int32_t heads, int32_t ch, float scale,
                       float *out, float *alpha, mirec_stream_t stream);

/* Backward of mirec_fanout_tattn from the kept alpha [n_targets, k, heads],
 * per head with g = grad_out[t, h] (grad_out contiguous [n_targets, D]):
 *   dalpha_j = <g, value_j>,  ds_j = alpha_j (dalpha_j - sum_m alpha_m dalpha_m)
 *   grad_value[t*k + j] = alpha_j g          (0 for an invalid slot)
 *   grad_key[t*k + j]   = ds_j scale query[t] (0 for an invalid slot)
 *   grad_query[t] = sum_j ds_j scale key[t*k + j]
 *   grad_skip[t]  = g                         (if grad_skip != NULL)
 * grad_query / grad_skip rows lie at stride ld_gq, grad_key / grad_value rows
 * at stride ld_gkv.  Every child row has one parent, so all four are plain
 * stores: written, not added to; no atomics, no workspace, the same bits from
 * run to run.  The value rows are read twice, the key rows once.  Same shape,
 * stride and alignment limits as the forward. */
int mirec_fanout_tattn_bwd(const float *grad_out, const float *query, int64_t ld_q,
                           const float *key, const float *value, int64_t ld_kv,
                           const int32_t *valid, const float *alpha,
                           int64_t n_targets, int32_t k, int32_t heads, int32_t ch, float scale,
                           float *grad_query, float *grad_skip, int64_t ld_gq,
                           float *grad_key, float *grad_value, int64_t ld_gkv,
                           mirec_stream_t stream);

/* The same forward over every row of a CSR graph (full-graph inference): row
 * r attends with query[r] over the key / value rows of its col entries (a
 * multi-edge once per entry; no self loop); a row without entries gives its
 * skip row.  query / skip / key / value hold one row per graph row.  Reads
 * rowptr and col only; entries outside [0, n_rows) are skipped.  Any degree:
 * one lane group walks a row.  Limits as mirec_fanout_tattn. */
int mirec_csr_tattn(const mirec_csr_t *csr, const float *query, const float *skip, int64_t ld_q,
                    const float *key, const float *value, int64_t ld_kv,
                    int32_t heads, int32_t ch, float scale, float *out, mirec_stream_t stream);

/* GRU gate of the gated graph hop (PyG GatedGraphConv(d, num_layers=1,
 * aggr='mean'), model/gnn.py conv = 'ggnn': a GRUCell on (mean of the
 * projected children, the node's own row)).  gi = a W_ihᵀ + b_ih and gh = h
 * W_hhᵀ + b_hh are finished pre-activations, [n_rows, 3 dim] with the thirds
 * in the order r, z, n (the biases are the GEMMs' business); h [n_rows, dim]:
 *   r = sigmoid(gi_r + gh_r)   z = sigmoid(gi_z + gh_z)
 *   n = tanh(gi_n + r gh_n)    out = (1 - z) n + z h   (max(., 0) if relu)
 * sigmoid and tanh saturate: every finite pre-activation gives a finite out.
 * All tensors contiguous, dim % 4 == 0, 4 <= dim <= 1024, every pointer
 * 16-byte aligned; anything else is MIREC_ERR_ARG, nothing launched.  n_rows
 * == 0 is MIREC_OK. */
int mirec_gru_gate(const float *gi, const float *gh, const float *h, int64_t n_rows,
                   int32_t dim, int32_t relu, float *out, mirec_stream_t stream);

/* Backward of mirec_gru_gate.  The gates are recomputed from gi, gh, h; out
 * (the forward's output) is read only for the ReLU mask, g = grad_out where
 * out > 0 and 0 elsewhere — NULL if the forward ran without relu.
 *   dn = g (1 - z)   dz = g (h - n)   pn = dn (1 - n^2)
 *   grad_gi_n = pn   grad_gh_n = pn r   dr = pn gh_n
 *   grad_gi_r = grad_gh_r = dr r (1 - r)   grad_gi_z = grad_gh_z = dz z (1 - z)
 *   grad_h = g z     (the direct path only; the one through gh is the GEMM's)
 * All three are plain stores, written, not added to: no atomics, the same
 * bits from run to run.  The bias gradients are the column sums of grad_gi
 * and grad_gh (mirec_col_sums).  Limits as the forward. */
int mirec_gru_gate_bwd(const float *grad_out, const float *gi, const float *gh, const float *h,
                       const float *out, int64_t n_rows, int32_t dim, float *grad_gi,
                       float *grad_gh, float *grad_h, mirec_stream_t stream);

/* Deterministic id-table gradient (model/graphsage.py:311-337) and the Adam
 * step that consumes it (graphsage.py:388-397).  The table gradient of one
 * step is G[r] = c[slice(r)] * table[r] + S[r]: c = (c_user, c_item) the
 * norm-term coefficients dL/d|slice| / |slice| (device, 2 floats; rows
 * [0, n_user) are the user slice), S the sum of the tree's row
 * contributions, given as up to MIREC_TABLE_GRAD_MAX_GROUPS groups: entry
 * t*k + c of a group adds w_t * dropout(grad_out[t]) to row ids[t*k + c]
 * (ids < 0 skipped), with w_t = 1/(valid children of t) for a mean group
 * (the leaf hop's dropout-mean; mask element (t*k + c)*dim + col as in
 * mirec_fanout_mean_gather) and 1 otherwise (a plain row gather: k = 1,
 * dropout_p = 0). */
#define MIREC_TABLE_GRAD_MAX_GROUPS 8
typedef struct mirec_row_grad_group {
  const int32_t *ids;       /* [n_targets * k] row ids, -1 = none */
  const float *grad_out;    /* [n_targets, dim] */
  int64_t n_targets;
  int32_t k;
  int32_t mean;             /* 1: w_t = 1/cnt_t, 0: w_t = 1 */
  float dropout_p;
  int32_t _pad;
  uint64_t seed;
} mirec_row_grad_group_t;

/* sizeof(mirec_row_grad_group_t), for FFI struct-mirror checks. */
int64_t mirec_row_grad_group_size(void);

/* S for every touched row: the entries of all groups sorted by row id
 * (stable: mirec_small_sort_pairs up to 8 192 entries, the device library's
 * radix sort above), each id's contributions summed in entry order (runs longer than
 * a 64-entry chunk: per-chunk partials added in chunk order) — no float
 * atomics, bitwise repeatable.  Writes acc[r] = S[r] and stamp[r] = gen for
 * the touched rows only (nothing is cleared: a row belongs to this step iff
 * stamp[r] == gen).  acc [n_rows, dim], stamp [n_rows]; workspace:
 * mirec_table_grad_workspace bytes. */
int mirec_table_grad_workspace(const mirec_row_grad_group_t *groups, int32_t n_groups,
                               int32_t n_rows, int32_t dim, size_t *bytes);
int mirec_table_grad_sorted(const mirec_row_grad_group_t *groups, int32_t n_groups,
                            int32_t n_rows, int32_t dim, float *acc, int32_t *stamp, int32_t gen,
                            void *workspace, size_t workspace_bytes, mirec_stream_t stream);

/* The same S packed (the data-parallel exchanges' export): rows[j] = the
 * j-th touched row id ascending and vals[j] its row of S, j < counts[0];
 * counts[1 + p] = the touched rows in owner block p (rows [p N/P, (p + 1)
 * N/P), the last block to N = n_rows, P = parts) — all on the device, no
 * host sync.  The same sums bit for bit as mirec_table_grad_sorted; acc /
 * stamp are not touched.  rows / vals hold at least min(entries, n_rows)
 * rows; the workspace is mirec_table_grad_workspace's.  Replaces the
 * stamped-row scan + gather of the dense form for a routed step
 * (reference: the gradient all-reduce of ddp_sage.py:800-806). */
int mirec_table_grad_sorted_rows(const mirec_row_grad_group_t *groups, int32_t n_groups,
                                 int32_t n_rows, int32_t dim, int32_t parts, int32_t *rows,
                                 float *vals, int32_t *counts, void *workspace,
                                 size_t workspace_bytes, mirec_stream_t stream);

/* The same S in the atomic form, for plain groups only (k = 1, mean = 0,
 * dropout_p = 0): touched rows stamped and zeroed, then every gradient row
 * added with float atomics — two launches, no workspace; the summation
 * order of a repeated id is not fixed. */
int mirec_table_grad_atomic(const mirec_row_grad_group_t *groups, int32_t n_groups,
                            int32_t n_rows, int32_t dim, float *acc, int32_t *stamp, int32_t gen,
                            mirec_stream_t stream);

/* grad = G materialised (coef may be NULL = 0), [n_rows, dim]. */
int mirec_table_grad_dense(const float *table, const float *coef, int64_t n_user,
                           const float *acc, const int32_t *stamp, int32_t gen, int64_t n_rows,
                           int32_t dim, float *grad, mirec_stream_t stream);

/* Adam (torch.optim.Adam, as mirec_adam_dense) of the whole table with G
 * formed on the fly: param / exp_avg / exp_avg_sq read and written once,
 * the dense gradient never stored.  If sumsq and norms are given (sumsq:
 * mirec_adam_table_sumsq_floats floats), norms[0..1] = the L2 norms of the
 * UPDATED user / item slices (the next step's norm term), fixed order. */
int64_t mirec_adam_table_sumsq_floats(int64_t n_rows, int32_t dim);
int mirec_adam_table(float *param, float *exp_avg, float *exp_avg_sq, const float *coef,
                     int64_t n_user, const float *acc, const int32_t *stamp, int32_t gen,
                     int64_t n_rows, int32_t dim, const mirec_adam_hparams_t *h, float *sumsq,
                     float *norms, mirec_stream_t stream);
/* The owner's step of the data-parallel exchanges in one pass: S of the own
 * row block [lo, lo + n_own) from the source blocks exactly as
 * mirec_owner_sum forms it (block order), then mirec_adam_table on those
 * rows with every row stamped (param / exp_avg / exp_avg_sq point at row lo;
 * n_user = the block's user rows; sumsq / norms as there, sumsq of
 * mirec_adam_table_sumsq_floats(n_own, dim) floats) — S is never stored.
 * Bitwise the same parameters, moments and norms as mirec_owner_sum +
 * mirec_adam_table.  At most 64 blocks.  Workspace:
 * mirec_owner_sum_workspace(n_blocks, n_own) bytes.  (Reference: the Adam
 * step of the synchronised table gradient, ddp_sage.py:800-806.) */
int mirec_owner_adam(const mirec_row_block_t *blocks, int32_t n_blocks, int64_t lo,
                     int64_t n_own, int32_t dim, float *param, float *exp_avg,
                     float *exp_avg_sq, const float *coef, int64_t n_user,
                     const mirec_adam_hparams_t *h, float *sumsq, float *norms, void *workspace,
                     size_t workspace_bytes, mirec_stream_t stream);
/* mirec_adam_table with the hyper-parameters read from device memory when
 * the kernel runs (capturable in a HIP graph). */
int mirec_adam_table_dev(float *param, float *exp_avg, float *exp_avg_sq, const float *coef,
                         int64_t n_user, const float *acc, const int32_t *stamp, int32_t gen,
                         int64_t n_rows, int32_t dim, const mirec_adam_hparams_t *h_device,
                         float *sumsq, float *norms, mirec_stream_t stream);

/* coef[i] = norm[i*norm_stride] > 0 ? g[i*g_stride] / norm[i*norm_stride] : 0
 * for i < n (<= 1024): a table gradient's norm-term coefficients. */
int mirec_norm_coef(const float *g, int32_t g_stride, const float *norm, int32_t norm_stride,
                    int32_t n, float *coef, mirec_stream_t stream);

/* ------------------------------------------------------------------------ */
/* SASRec causal self-attention (model/sasrec.py:385-397), f32 MFMA          */
/* ------------------------------------------------------------------------ */

/* qkv: the packed in-projection output [batch, T, 3*heads*head_dim] (q | k |
 * v, head h = columns h*head_dim ..); out: [batch, T, heads*head_dim] =
 * softmax(q kᵀ / sqrt(head_dim) + causal mask) v per head.  T <= 64,
 * 1 <= head_dim <= 64. */
int mirec_attention_fwd(const float *qkv, int64_t batch, int32_t T, int32_t heads,
                        int32_t head_dim, float *out, mirec_stream_t stream);

/* Backward: dqkv [batch, T, 3*heads*head_dim] (written) from dout. */
int mirec_attention_bwd(const float *qkv, const float *dout, int64_t batch, int32_t T,
                        int32_t heads, int32_t head_dim, float *dqkv,
                        mirec_stream_t stream);

/* Packed (variable-length) form: sequence b is rows offsets[b] ..
 * offsets[b+1]-1 of qkv [n_tok, 3*heads*head_dim] / out / dout / dqkv
 * [n_tok, ...]; offsets (device, int32, batch+1 entries, non-decreasing)
 * with every length <= 64 (longer sequences are cut to their first 64
 * rows).  Padding positions past a sequence's length never influence its
 * earlier positions under the causal mask, so the padded and the packed
 * forms agree on every real row; the packed one skips the padding. */
int mirec_attention_varlen_fwd(const float *qkv, const int32_t *offsets, int64_t batch,
                               int32_t heads, int32_t head_dim, float *out,
                               mirec_stream_t stream);
int mirec_attention_varlen_bwd(const float *qkv, const float *dout, const int32_t *offsets,
                               int64_t batch, int32_t heads, int32_t head_dim,
                               float *dqkv, mirec_stream_t stream);

/* Packed form with the sequences ordered by length bucket: bucket_end (HOST
 * array of 4 non-decreasing counts; batch = bucket_end[3]) says sequences
 * [bucket_end[k-1], bucket_end[k]) have at most 16*(k+1) positions.  Each
 * bucket runs on a kernel whose workgroup holds only 16*(k+1) rows (one
 * wave per 16-row block, LDS sized to match), so short sequences neither
 * idle three waves nor reserve a 64-row LDS image.  A longer sequence placed
 * in a bucket is cut to the bucket's rows (an input error). */
int mirec_attention_bucketed_fwd(const float *qkv, const int32_t *offsets,
                                 const int64_t *bucket_end, int32_t heads, int32_t head_dim,
                                 float *out, mirec_stream_t stream);
int mirec_attention_bucketed_bwd(const float *qkv, const float *dout, const int32_t *offsets,
                                 const int64_t *bucket_end, int32_t heads, int32_t head_dim,
                                 float *dqkv, mirec_stream_t stream);

/* Backward with short sequences sharing a workgroup (one wave per 16-row
 * block, up to 4 blocks per workgroup): packs from
 * mirec_attention_length_order; head_dim % 4 == 0, <= 64.  Rows
 * [offsets[batch], n_rows) of dqkv (capacity padding) are zeroed. */
int mirec_attention_packed_bwd(const float *qkv, const float *dout, const int32_t *offsets,
                               const int32_t *packs, int64_t batch, int32_t heads,
                               int32_t head_dim, float *dqkv, int64_t n_rows,
                               mirec_stream_t stream);
/* The packed backward given the forward's statistic: lse [n, heads] as
 * mirec_attention_wave_fwd wrote it (base 2).  P = exp2(S scale log2 e -
 * lse) directly, with no max / sum reductions in the kernel.  Same packs,
 * layout and padding rows as mirec_attention_packed_bwd. */
int mirec_attention_packed_bwd_lse(const float *qkv, const float *lse, const float *dout,
                                   const int32_t *offsets, const int32_t *packs, int64_t batch,
                                   int32_t heads, int32_t head_dim, float *dqkv, int64_t n_rows,
                                   mirec_stream_t stream);

/* Packed form with the workgroups in a given sequence order (device int32
 * [batch], e.g. mirec_attention_length_order: longest first). */
int mirec_attention_ordered_fwd(const float *qkv, const int32_t *offsets, const int32_t *order,
                                int64_t batch, int32_t heads, int32_t head_dim, float *out,
                                mirec_stream_t stream);
int mirec_attention_ordered_bwd(const float *qkv, const float *dout, const int32_t *offsets,
                                const int32_t *order, int64_t batch, int32_t heads,
                                int32_t head_dim, float *dqkv, mirec_stream_t stream);

/* One wave per (sequence, head) (csrc/attn_wave.hip): no LDS, no barriers,
 * every operand loaded straight into its MFMA lane layout; head_dim 16, 32
 * or 64 (mirec_attention_wave_supported).  offsets == NULL: uniform batch
 * [batch, T, ...] (1 <= T <= 64); else packed as in the varlen form.  The
 * forward also writes lse [n_rows, heads] (BASE-2 log-sum-exp of each query's
 * scaled scores: log2 sum_k 2^(s_k * scale * log2 e), i.e. the natural lse times
 * log2 e); the backward takes out and lse from it and writes dqkv and delta
 * [n_rows, heads] (rowsum(dout ⊙ out), scratch), in two launches.  order
 * (optional, packed form): the sequences in the order their units run, from
 * mirec_attention_length_order (longest first, device int32 [batch]; the
 * forward with offsets and n_rows > 0 also zeroes out's rows [offsets[batch],
 * n_rows) (capacity padding); with
 * packs (optional, int32 [4 + 8 batch], 16-byte aligned) it also groups
 * that order into packs of at most 4 blocks of 16 positions for
 * mirec_attention_packed_bwd: packs[0] = count, packs[4 + 8p + 2s] and
 * packs[5 + 8p + 2s] = (first row, length) of the sequence in slot s of
 * pack p, (0, 0) when empty); with zero_buf it
 * also zeroes rows [offsets[batch], zero_rows) of that [zero_rows,
 * zero_width] buffer (the capacity padding of a packed batch's output). */
int mirec_attention_wave_supported(int32_t head_dim);
int mirec_attention_length_order(const int32_t *offsets, int64_t batch, int32_t *order,
                                 int32_t *packs, float *zero_buf, int64_t zero_rows,
                                 int32_t zero_width, mirec_stream_t stream);
int mirec_attention_wave_fwd(const float *qkv, const int32_t *offsets, const int32_t *order,
                             int64_t batch, int32_t T, int32_t heads, int32_t head_dim, float *out,
                             float *lse, int64_t n_rows, mirec_stream_t stream);
int mirec_attention_wave_bwd(const float *qkv, const float *out, const float *lse,
                             const float *dout, const int32_t *offsets, const int32_t *order,
                             int64_t batch, int32_t T, int32_t heads, int32_t head_dim,
                             float *dqkv, float *delta, mirec_stream_t stream);

/* Masked mean pool of the SASRec user tower (model/sasrec.py:399-413) on
 * packed sequences: out[b] = Σ_{r in [offsets[b], offsets[b+1])} x[r] /
 * length[b] (rows summed in a fixed order), x [n, d], out [B, d], d % 4 == 0,
 * d <= 1024.  Backward: grad_x[t] = grad_out[seg[t]] / length[seg[t]] for
 * the n_rows rows (0 where seg[t] is outside [0, B): capacity padding). */
int mirec_segment_mean(const float *x, const int32_t *offsets, const int64_t *length, int64_t B,
                       int32_t d, float *out, mirec_stream_t stream);
int mirec_segment_mean_bwd(const float *grad_out, const int64_t *seg, const int64_t *length,
                           int64_t n_rows, int64_t B, int32_t d, float *grad_x,
                           mirec_stream_t stream);

/* BPR loss on embedding rows (model/sasrec.py:423-435): x_r = <u_r, n_r> -
 * <u_r, p_r> (written to x_out[0..B); x_out holds 2B floats, the second half
 * scratch), loss[0] = mean_r softplus(x_r) + coef * extra[0] (extra: a
 * device scalar such as the embedding-norm term, or NULL); u, p, n [B, d].
 * Fixed summation order (deterministic).  Backward:
 * with g = g_loss[0] (device) and s_r = g sigmoid(x_r) / B: du = s (n - p),
 * dp = -s u, dn = s u, and g_extra[0] = g coef (if g_extra != NULL). */
int mirec_bpr_rows_loss(const float *u, const float *p, const float *n, int64_t B, int32_t d,
                        const float *extra, float coef, float *x_out, float *loss,
                        mirec_stream_t stream);
int mirec_bpr_rows_loss_bwd(const float *u, const float *p, const float *n, const float *x,
                            int64_t B, int32_t d, const float *g_loss, float coef, float *du,
                            float *dp, float *dn, float *g_extra, mirec_stream_t stream);

/* L2 norms of x[0, split) and x[split, n) -> norms[0], norms[1] (the
 * parameter-norm terms of model/graphsage.py:326-337 / model/sasrec.py:
 * 423-435 over an id table's user / item slices; split = n for one norm).
 * n % 4 == 0, split % 4 == 0, x 16-byte aligned; work:
 * mirec_slice_norms_work_floats() floats.  Fixed summation order. */
int64_t mirec_slice_norms_work_floats(void);
int mirec_slice_norms(const float *x, int64_t n, int64_t split, float *work, float *norms,
                      mirec_stream_t stream);

/* Weighted parameter-norm term (model/graphsage.py:326-337: all_param = 2
 * all_param + |p| over the parameters = Σ_k 2^(K-1-k) |p_k|):
 * total[0] = Σ_j extra_w[j] * extra[j] + Σ_k weights[k] * |xs[k]|₂ (extra:
 * norms already on the device, e.g. the id table's slices; xs: count small
 * device tensors of numel[k] floats, host array of pointers; weights /
 * extra_w: host arrays), norms[k] = |xs[k]|₂.  Fixed summation order.
 * Backward: grads[k] = g * weights[k] * xs[k] / |xs[k]| (written; 0 where the
 * norm is 0) and extra_grad[j] = g * extra_w[j], with g = g_total[0]
 * (device).  count, n_extra <= MIREC_NORM_TERMS_MAX. */
#define MIREC_NORM_TERMS_MAX 16
int mirec_norm_terms(const float *const *xs, const int64_t *numel, const float *weights,
                     int32_t count, const float *extra, const float *extra_w, int32_t n_extra,
                     float *norms, float *total, mirec_stream_t stream);
int mirec_norm_terms_bwd(const float *const *xs, float *const *grads, const int64_t *numel,
                         const float *weights, int32_t count, const float *norms,
                         const float *g_total, const float *extra_w, int32_t n_extra,
                         float *extra_grad, mirec_stream_t stream);
/* The same small-tensor gradients ADDED to grads[k] (the gradients the rest
 * of the backward already accumulated there): g_k += g * weights[k] * xs[k] /
 * |xs[k]|.  Run once the backward is done, so a parameter used by several
 * nodes is not summed by a separate elementwise kernel per use. */
int mirec_norm_terms_bwd_acc(const float *const *xs, float *const *grads, const int64_t *numel,
                             const float *weights, int32_t count, const float *norms,
                             const float *g_total, mirec_stream_t stream);

/* Per-step (positive, negative) pairs of a sequence batch: out[j] = a
 * uniform element of user users[j]'s sequence items[u][0, length[u]) (0 for
 * an empty one), out[B + j] = a uniform item in [0, m_items); counter-based
 * (seed, offset + j). */
int mirec_seq_sample(const int64_t *users, int64_t B, const int32_t *items, int32_t max_len,
                     const int64_t *length, int64_t m_items, uint64_t seed, uint64_t offset,
                     int64_t *out, mirec_stream_t stream);

/* Pack a SASRec batch into a fixed token capacity (the graph-captured step,
 * model/sasrec.py:449-455's pad_sequence without the padding): users [B]
 * (device int64), items [n_users, max_len] (int32, each user's last items),
 * length_tab [n_users] (int64), pos / neg [B] (int64).  Writes length[b] =
 * length_tab[users[b]], offsets[B+1] = the prefix sums clamped to capacity
 * (int32), ids_all[capacity + 2B] (int32) = the item id of every token row
 * (-1 past the last sequence) followed by pos and neg, and seg[capacity]
 * (int64) = the sequence of every row (B past the last sequence). */
int mirec_seq_pack(const int64_t *users, int64_t B, const int32_t *items, int32_t max_len,
                   const int64_t *length_tab, const int64_t *pos, const int64_t *neg,
                   int64_t capacity, int32_t *offsets, int64_t *length, int32_t *ids_all,
                   int64_t *seg, mirec_stream_t stream);

/* Zero rows [offsets[B], n_rows) of buf [n_rows, row_floats] (offsets on the
 * device): the capacity-padding rows of a packed batch, which the packed
 * attention kernels do not write. */
int mirec_zero_tail_rows(float *buf, const int32_t *offsets, int64_t B, int64_t n_rows,
                         int32_t row_floats, mirec_stream_t stream);

/* f32 MFMA GEMMs of the Linear layers on token rows (model/sasrec.py:385-421,
 * model/graphsage.py:311-324).  Row-major, device pointers, 16-byte aligned.
 *
 * Arithmetic (default build, MIREC_GEMM_X6): every f32 operand is split
 * exactly into three bf16 terms and each product is formed from the six
 * largest term products on bf16 MFMA with f32 accumulation — the error of
 * one f32 rounding per product.  Edge semantics differ from
 * an fp32 FMA chain: an infinite or NaN operand gives NaN (inf - inf in the
 * split), so an overflowed input yields NaN where fp32 would give +-inf; and
 * operands below ~2^-110 lose low-order bits (the third term underflows
 * bf16's range) — far below anything a finite, non-overflowing training step
 * feeds these GEMMs.  Building with -DMIREC_GEMM_X6=0 selects exact f32
 * v_mfma_f32_32x32x2_f32 products.
 *
 * C[n, No] = A[n, Kr] · B[No, Kr]ᵀ (+ bias[No] if bias != NULL): the forward
 * y = x Wᵀ + b, and the input gradient dX = dY W with B = Wᵀ (a [K, N] copy
 * of the weight).  Kr % 32 == 0, No % 128 == 0. */
int mirec_gemm_nt(const float *A, const float *B, const float *bias, float *C, int64_t n,
                  int32_t Kr, int32_t No, mirec_stream_t stream);

/* C[M, No] = A[n, M]ᵀ · B[n, No] summed over the n rows, and (if colsum !=
 * NULL) colsum[M] = Σ_rows A: the weight gradient dW = dYᵀ X and the bias
 * gradient db = Σ dY in one pass over dY.  M % 128 == 0, No % 128 == 0;
 * work: mirec_gemm_tn_work_floats(n, M, No) floats (per-slice partial
 * sums, added in a fixed order: deterministic). */
int64_t mirec_gemm_tn_work_floats(int64_t n, int32_t M, int32_t No);

/* out[c] = Σ_r A[r, c] over the n rows of a row-major [n, m] matrix, summed
 * in a fixed order (deterministic, capturable): the bias gradient db = Σ dY
 * of a Linear whose width the GEMM tiles do not take (nn.Linear backward,
 * model/sasrec.py:385-421), and the slice sum of the split weight gradient.
 * work: mirec_col_sums_work_floats(n, m) floats. */
int64_t mirec_col_sums_work_floats(int64_t n, int32_t m);
int mirec_col_sums(const float *A, int64_t n, int32_t m, float *out, float *work,
                   mirec_stream_t stream);
int mirec_gemm_tn(const float *A, const float *B, float *C, float *colsum, int64_t n, int32_t M,
                  int32_t No, float *work, mirec_stream_t stream);

/* Fused forms of the two GEMMs (the GraphSAGE hop h = relu(W [x ; aggr] + b),
 * model/graphsage.py:314-315, without materialising the concatenation):
 *   gemm_nt_ex: A2 != NULL: the A row is [A[r, 0:Ks) | A2[r, 0:Kr-Ks)] (row
 *     strides Ks and Kr-Ks; Ks % 32 == 0); Amask != NULL (single A only): A
 *     elements whose Amask element (same layout) is <= 0 read as 0 (the ReLU
 *     backward dY * (y > 0)); C2 != NULL: output columns [0, Ns) go to C (row
 *     stride Ns) and [Ns, No) to C2 (stride No-Ns; Ns % 128 == 0); relu != 0:
 *     max(., 0) after the bias.
 *   gemm_tn_ex: Amask as above on A; B2 != NULL: the B row is [B[r, 0:Ns) |
 *     B2[r, 0:No-Ns)] (Ns % 128 == 0); colsum = Σ of the masked A. */
int mirec_gemm_nt_ex(const float *A, const float *A2, int32_t Ks, const float *Amask,
                     const float *B, const float *bias, float *C, float *C2, int32_t Ns,
                     int32_t relu, int64_t n, int32_t Kr, int32_t No, mirec_stream_t stream);
/* C = A B with B [Kr, No] row-major (the input gradient dX = dY W of a
 * Linear, W used as stored: no transposed copy); Amask and the C / C2 split
 * as in gemm_nt_ex. */
int mirec_gemm_nn_ex(const float *A, const float *Amask, const float *B, float *C, float *C2,
                     int32_t Ns, int64_t n, int32_t Kr, int32_t No, mirec_stream_t stream);
int mirec_gemm_tn_ex(const float *A, const float *Amask, const float *B, const float *B2,
                     int32_t Ns, float *C, float *colsum, int64_t n, int32_t M, int32_t No,
                     float *work, mirec_stream_t stream);

/* Row tail of the SASRec block (model/sasrec.py:385-397 — the dropout,
 * residual add, ReLU and LayerNorm around the attention and the FFN), one
 * pass over the n x d token rows (d % 4 == 0, 4 <= d <= 1024):
 *   pre = (res ? res : 0) + dropout_p-dropout(z + (bias ? bias : 0))
 *   out = relu ? max(pre, 0) : pre                         (written if out)
 *   y   = (out - mean) * rstd * (gamma ? gamma : 1) + (beta ? beta : 0),
 *         rstd = 1 / sqrt(biased var + eps)                (written if y;
 *         mean / rstd [n] then required)
 * out may be NULL only when it equals z (no res / bias / relu / dropout).
 * The dropout mask is the element dropout stated above (after
 * mirec_edge_keep_mask) at element index row * d + col — the same seed
 * recomputes it in the backward.  seed_base (device, may be NULL): when
 * given, the key becomes mix64(key ^ *seed_base) when the kernel runs, so a
 * captured HIP graph draws a fresh mask on every replay (the host writes a
 * new base before each replay; the backward reads the same base). */
int mirec_resnorm_fwd(const float *res, const float *z, const float *bias, const float *gamma,
                      const float *beta, int64_t n, int32_t d, int32_t relu, float dropout_p,
                      uint64_t seed, const uint64_t *seed_base, float eps, float *out, float *y,
                      float *mean, float *rstd, mirec_stream_t stream);

/* mirec_resnorm_fwd with z = A Wᵀ computed in the same kernel (A [n, Kr],
 * W [d, Kr] row-major, d = 128, Kr % 32 == 0): the Linear before a block
 * stage's row tail (model/sasrec.py:385-397 — attention out-projection and
 * FFN, their biases passed as `bias`), z never written.  out is required;
 * every other argument and output as in mirec_resnorm_fwd (identical
 * values: same per-row arithmetic); the backward is mirec_resnorm_bwd
 * followed by the Linear's gradients (mirec_gemm_nn_ex / mirec_gemm_tn). */
int mirec_gemm_resnorm(const float *A, const float *W, int64_t n, int32_t Kr, int32_t d,
                       const float *res, const float *bias, const float *gamma, const float *beta,
                       int32_t relu, float dropout_p, uint64_t seed, const uint64_t *seed_base,
                       float eps, float *out, float *y, float *mean, float *rstd,
                       mirec_stream_t stream);

/* Backward counterpart of mirec_gemm_resnorm: g_y = A W computed in the
 * kernel (A [n, Kr], W [Kr, d] row-major as stored — the input gradient of
 * the Linear that consumed this row tail's y — d = 128, Kr % 32 == 0), then
 * mirec_resnorm_bwd(g_y, g_out, out, mean, rstd, gamma, ...) (the same
 * per-row expressions; d_gamma / d_beta / d_bias, each optional, summed per 64-row
 * tile and then in tile order (work: mirec_gemm_nn_resnorm_bwd_work_floats
 * floats when any sum is asked).  g_y is never written. */
int64_t mirec_gemm_nn_resnorm_bwd_work_floats(int64_t n, int32_t d);
int mirec_gemm_nn_resnorm_bwd(const float *A, const float *W, int64_t n, int32_t Kr, int32_t d,
                              const float *g_out, const float *out, const float *mean,
                              const float *rstd, const float *gamma, int32_t relu,
                              float dropout_p, uint64_t seed, const uint64_t *seed_base,
                              float *d_res, float *d_z, float *work, float *d_gamma,
                              float *d_beta, float *d_bias, mirec_stream_t stream);
/* The fixed-order sum of [parts][3][d] column partials into d_gamma /
 * d_beta / d_bias (each optional): the second pass of the row-tail
 * backwards. */
int mirec_resnorm_reduce_partials(const float *work, int64_t parts, int32_t d, float *d_gamma,
                                  float *d_beta, float *d_bias, mirec_stream_t stream);

/* Floats of scratch mirec_resnorm_bwd needs for parameter gradients. */
int64_t mirec_resnorm_work_floats(int64_t n, int32_t d);

/* Backward of mirec_resnorm_fwd.  out: the forward's out (or z when out
 * was omitted); g_y / g_out: gradients of y / out (either may be NULL =
 * zero).  Writes d_res = d(pre) and d_z = d(z) = d(bias) per row (each
 * optional), and the column sums d_gamma = Σ g_y·x̂, d_beta = Σ g_y,
 * d_bias = Σ d_z (each optional; work then needs
 * mirec_resnorm_work_floats floats).  Sums are added in a fixed order. */
int mirec_resnorm_bwd(const float *g_y, const float *g_out, const float *out, const float *mean,
                      const float *rstd, const float *gamma, int64_t n, int32_t d, int32_t relu,
                      float dropout_p, uint64_t seed, const uint64_t *seed_base, float *d_res,
                      float *d_z, float *work, float *d_gamma, float *d_beta, float *d_bias,
                      mirec_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Evaluation (trainer.py:130-138)                                           */
/* ------------------------------------------------------------------------ */

/* scores [n_eval, m_items] row-major (a GEMM of user and item embeddings,
 * model/lgcn.py:124).  If csr != NULL, row b's train positives (the CSR row
 * of user users[b]: node ids n_users + item) are set to -1024 in place
 * (trainer.py:132-137).  Then the k best items of every row (score
 * descending, ties to the lower item id) go to topk_idx[b*k ..] and, if
 * topk_val != NULL, their scores to topk_val.  1 <= k <= 64. */
int mirec_topk_masked(float *scores, int64_t n_eval, int64_t m_items,
                      const int32_t *users, const mirec_csr_t *csr,
                      int64_t n_users, int32_t k, int32_t *topk_idx,
                      float *topk_val, mirec_stream_t stream);

/* Streaming evaluation: the top-k of user_emb[b] · item_embᵀ
 * per evaluated user b, the user's train positives (csr row users[b],
 * entries n_users + item) scoring -1024, WITHOUT materialising the
 * [n_eval, m_items] scores: MFMA score tiles are filtered into per-user
 * candidate lists as they are produced (two launches).  user_emb [n_eval,
 * dim], item_emb [m_items, dim], dim in {16, 32, 64, 128}, 1 <= k <= 32;
 * same order and ties as mirec_topk_masked.  workspace:
 * mirec_score_topk_workspace bytes. */
int64_t mirec_score_topk_workspace(int64_t n_eval, int64_t m_items, int32_t k);
int mirec_score_topk(const float *user_emb, int64_t n_eval, const float *item_emb,
                     int64_t m_items, int32_t dim, const int32_t *users, const mirec_csr_t *csr,
                     int64_t n_users, int32_t k, int32_t *topk_idx, float *topk_val,
                     void *workspace, size_t workspace_bytes, mirec_stream_t stream);

/* Streamed full-rank evaluation: the exact position of every
 * held-out (user, item) pair among the user's non-train items, as integer
 * counts, WITHOUT materialising the scores.  User slot r (row r of user_emb,
 * user id users[r]) owns the pairs tptr[r] .. tptr[r + 1] - 1 of `targets`
 * (item ids, distinct per user; tptr[0] = 0, non-decreasing).  With s_j =
 * <user_emb[r], item_emb[j]> — bitwise mirec_score_topk's score of the same
 * (row, item) — and J the items that are not train positives of users[r]
 * (csr row users[r], entries n_users + item; csr == NULL: every item), pair
 * t of slot r gets
 *   score    = s_t
 *   masked   = 1 if t is not in J (or not an item id); its counts are then
 *              unspecified
 *   gt       = #{j in J : s_j >  s_t}
 *   eq       = #{j in J : s_j == s_t}          (t itself included: >= 1)
 *   eq_lower = #{j in J, j < t : s_j == s_t}
 * so 1 + gt + eq_lower is t's rank in mirec_score_topk's order (score
 * descending, ties to the lower item id).  dim in {16, 32, 64, 128, 256}.
 * tptr is a HOST array [n_eval + 1] (the pair count tptr[n_eval] sizes the
 * launches; the call copies the array to the workspace on `stream`, so a
 * pinned tptr must stay unchanged until the stream has passed the call);
 * every other pointer is a device pointer, the outputs [tptr[n_eval]] each.
 * No pairs: returns at once, reading and launching nothing.  workspace:
 * mirec_score_rank_workspace bytes, 16-byte aligned. */
int64_t mirec_score_rank_workspace(int64_t n_eval, int64_t n_targets, int64_t m_items,
                                   int32_t dim);
int mirec_score_rank(const float *user_emb, int64_t n_eval, const float *item_emb,
                     int64_t m_items, int32_t dim, const int32_t *users, const int64_t *tptr,
                     const int32_t *targets, const mirec_csr_t *csr, int64_t n_users,
                     float *score, int32_t *gt, int32_t *eq, int32_t *eq_lower, uint8_t *masked,
                     void *ws, size_t ws_bytes, mirec_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Host (CPU) path of configuration C1 (model/MF.py BPR, "CPU single-process", */
/* BASELINE configs[0]): host pointers, no stream, n_threads worker threads.  */
/* ------------------------------------------------------------------------ */

/* mirec_bpr_sample on the host: the same counter streams, so the triples are
 * the device sampler's bit for bit (col_sorted / pos_cdf optional, as in
 * mirec_csr_t / mirec_bpr_sample_ex).  Replaces UniformSample,
 * negative_sample.py:98-134, for a CPU model. */
int mirec_cpu_bpr_sample(const int64_t *rowptr, const int32_t *col, const int32_t *col_sorted,
                         const double *pos_cdf, int64_t n_users, int64_t m_items, int64_t batch,
                         uint64_t seed, uint64_t offset, int32_t shard, int32_t n_shards,
                         int32_t *users, int32_t *pos, int32_t *neg, int32_t *err,
                         int32_t n_threads);

/* mirec_ssm_sample on the host: the same streams, the same output bit for
 * bit, whatever n_threads. */
int mirec_cpu_ssm_sample(const int64_t *rowptr, const int32_t *col, const int32_t *col_sorted,
                         const double *pos_cdf, int64_t n_users, int64_t m_items, int64_t batch,
                         int32_t n_neg, uint64_t seed, uint64_t offset, int32_t shard,
                         int32_t n_shards, int32_t *users, int32_t *pos, int32_t *neg,
                         int32_t *err, int32_t n_threads);

/* mirec_shared_sample on the host: the same streams, the same output bit for
 * bit, whatever n_threads. */
int mirec_cpu_shared_sample(int64_t m_items, int64_t n_sets, int64_t m, uint64_t seed,
                            uint64_t offset, int32_t *out, int32_t n_threads);

/* mirec_bpr_sample_capped_ex on the host (the ddp_lgcn.py epoch sampler for
 * a CPU model): the same candidate streams, so users / pos / neg (capacity
 * n_candidates), *count and the optional cand_u / cand_p equal the device
 * sampler's bit for bit; the keep decision is the reference's sequential
 * per-item count (ddp_lgcn.py:571-572).  *err = 1 if a negative draw
 * exhausted its retries.  No workspace. */
int mirec_cpu_bpr_sample_capped(const int64_t *rowptr, const int32_t *col,
                                const int32_t *col_sorted, const double *pos_cdf, int64_t n_users,
                                int64_t m_items, int64_t n_candidates, int32_t cap, uint64_t seed,
                                uint64_t offset, int32_t shard, int32_t n_shards, int32_t *users,
                                int32_t *pos, int32_t *neg, int32_t *count, int32_t *err,
                                int32_t *cand_u, int32_t *cand_p, int32_t n_threads);

/* One MF stageOne (model/MF.py:62-94: BPR loss + decay x reg, backward,
 * torch.optim.Adam over the whole table) on a [n_rows, dim] host table whose
 * item rows start at item_offset (= n_users): grad is a [n_rows, dim]
 * workspace; *loss_out = loss + decay reg (the value stageOne returns).
 * MIREC_ERR_RANGE if an id is outside its table slice. */
int mirec_cpu_bpr_step(float *table, float *exp_avg, float *exp_avg_sq, float *grad,
                       int64_t n_rows, int32_t dim, int64_t item_offset, const int32_t *users,
                       const int32_t *pos, const int32_t *neg, int64_t batch, float decay,
                       const mirec_adam_hparams_t *h, float *loss_out, int32_t n_threads);

/* The two halves of mirec_cpu_bpr_step (bitwise the same arithmetic): the
 * dense gradient of one batch's loss + decay reg, multiplied by grad_scale
 * (1 / world_size under data parallelism; 1 = the step's), into grad
 * (*loss_out unscaled); then torch.optim.Adam over n elements. */
int mirec_cpu_bpr_grad(const float *table, float *grad, int64_t n_rows, int32_t dim,
                       int64_t item_offset, const int32_t *users, const int32_t *pos,
                       const int32_t *neg, int64_t batch, float decay, float grad_scale,
                       float *loss_out, int32_t n_threads);
int mirec_cpu_adam(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                   const mirec_adam_hparams_t *h, int32_t n_threads);

#ifdef __cplusplus
}
#endif

#endif /* MIREC_H */
