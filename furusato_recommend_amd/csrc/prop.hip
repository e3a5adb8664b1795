// LightGCN propagation on gfx950: CSR segment-gather SpMM with a fused
// layer epilogue.
//
// Replaces PyG LGConv (model/lgcn.py:66,82) / rAdjConv (model/radj.py:28-44):
//   out[i] = sum_{(j -> i)} x[j] / sqrt(deg_i * deg_j)
// which the reference evaluates as a [nnz, D] gather, a scale and an atomic
// scatter-add.  A wave owns G = 64/LPR consecutive rows (LPR = D/4 lanes read
// one neighbour row as float4s: D=64 -> 16 lanes x 16 B = one 256-B row).
// Short rows (degree <= narrow_max) are gathered one per lane group; a wave
// with a longer row walks its rows one at a time with the whole wave: the
// row's column indices are read once, coalesced (64 per load), broadcast
// with ds_bpermute, and G x UNROLL neighbour rows are in flight per
// instruction; groups hold disjoint neighbour subsets in registers and are
// combined with a xor-butterfly.  No atomics, a fixed summation order per
// row (deterministic).
//
// Masks (byte maps over nodes, optional; 1.1 MB at C2, L2-resident):
//   row_mask  rows whose byte is 0 are skipped entirely (nothing written);
//             with frontier row lists the rows come from the lists instead
//             (narrow rows G per wave, wide rows one workgroup each);
//   in_mask   neighbours whose byte is 0 contribute exactly 0 and are not
//             read: the 64 candidates of a chunk are tested at once and the
//             valid ones compacted to the front with ds_permute.
// Frontier pruning uses them to compute only the rows the BPR loss depends
// on; skipped terms are exact zeros, so results equal the dense pass up to
// fp32 summation order (the compaction regroups the surviving neighbours).
//
// Rows longer than csr->split are cut into segments processed by extra waves
// of the same launch (partial sums to scratch) and summed in segment order by
// a finalize launch, so a Zipf-skewed item cannot serialise the grid (the
// row phase leaves them to their segments entirely).
//
// Edge weights (csr->val, optional): prop_kernel<.., MODE + kWeighted, ..> is
// the same walk with every term multiplied by its entry's value (A_ij = sum
// of val over the entries j -> i); the unweighted instantiations are the
// earlier ones, instruction for instruction.
// mirec_edge_dot gives the gradient with respect to the values.
//
// Scales (mirec_prop_t scale_src / scale_dst / scale_next, optional): dinv
// plays three roles, the scale of a gathered neighbour (RAW, SPARSE), of the
// row sum, and of the row written for the next layer; a launch that names any
// of them runs the kScaled instantiations, which read the three from their
// own vectors (D^-(1-r) A D^-r and its transpose, model/radj.py:28-44).  The
// other instantiations are the earlier ones, instruction for instruction.
//
// Edge dropout (mirec_propagate_drop, the reference's __dropout_x,
// model/MF.py:158-176): the kDropout instantiations keep entry (j -> i) iff
// edge_keep(key, i, j) (common.h; a hash of the ordered pair, multi-edges
// share the draw), decided by the lane that has just loaded the column; the
// dropped ones leave through the in_mask compaction, which a launch without
// another filter runs for them alone, so their rows are never gathered.  The
// transposed mask (backward) swaps the two hash arguments on the same CSR.
// The other instantiations are the earlier ones, instruction for instruction.
//
// Epilogue (per row, LPR lanes): z = dinv_i * sum + seed[slot_i];
// xs_out = dinv_i * z (next layer's pre-scaled input);
// o = (z + addend)/divisor + seed2[slot_i]; out = o or Adam(param; grad=o).
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>

#include "common.h"

namespace mirec {

struct PropK {
  const int64_t *rowptr;
  const int32_t *col;
  const float *dinv;
  int64_t n_rows;
  int64_t n_seg;
  const int32_t *seg_row;
  const int64_t *seg_beg;
  int32_t split;
  const float *x_in;
  const int32_t *slot;
  const float *seed_in;
  const float *seed;
  const float *addend;
  const float *seed2;
  float divisor;
  float *out;
  float *xs_out;
  float *param;
  float *m;
  float *v;
  mirec_adam_hparams_t adam;
  float *partial;
  const uint8_t *row_mask;
  const uint8_t *in_mask;
  const uint8_t *out_mask;   // rows whose `out` (and addend read) is skipped when 0
  const int32_t *row_list;   // rows to process (deduplicated), or NULL = all rows
  const int32_t *row_count;  // device count of row_list entries
  int64_t row_waves;         // waves of the row phase (host upper bound)
  int32_t narrow_max;        // rows up to this degree are gathered group-per-row
  const int32_t *wide_list;  // rows gathered by a whole workgroup each (list mode)
  const int32_t *wide_count;
  // A DROPOUT launch (edge dropout, common.h edge_keep) has neither values nor
  // scales of its own (refused by the host), so its four scalars live in the
  // storage of those three pointers: PropK, and with it the argument block of
  // every other instantiation, keeps its size and its offsets.
  union {
    const float *val;        // [nnz] per-entry weight (WEIGHTED instantiations only)
    uint64_t drop_key;       // DROPOUT: edge_drop_key(seed)
  };
  // SCALED instantiations only (there `dinv` above is the row sum's scale):
  union {
    const float *scale_src;  // [n_rows] scale of a gathered neighbour (RAW, SPARSE)
    struct {
      uint32_t drop_thresh_m1;  // DROPOUT: edge_drop_thresh(keep_prob) - 1
      int32_t drop_transposed;  // DROPOUT: entry (j -> i) is masked by keep(j, i)
    };
  };
  union {
    const float *scale_next;  // [n_rows] scale of the row written to xs_out
    float drop_scale;         // DROPOUT: 1 / keep_prob, applied once to a gathered sum
  };
};

// prop_kernel's MODE argument with this bit set is the edge-weighted walk
// (the unweighted instantiations keep their names: MODE 0..3).
constexpr int kWeighted = 4;
// ... and with this bit the three scales come from their own vectors
// (never together with kWeighted: refused by the host).
constexpr int kScaled = 8;
// ... and with this bit every entry is kept or dropped by edge_keep (edge
// dropout; never together with kWeighted or kScaled: refused by the host).
constexpr int kDropout = 16;
// ... and with this bit fused Adam streams its table and moments
// (row_epilogue's STREAM; full unmasked PRESCALED launches at d = 64 only).
constexpr int kStream = 32;

__device__ __forceinline__ bool bit_set(const uint8_t *bm, int64_t i) { return bm[i] != 0; }

// Sum of the input rows listed in col[beg, end) (pre-scaled / raw x dinv_j /
// sparse seeds x dinv_j), restricted to in_mask when MASKED.  One walk in two
// shapes: the lanes that share a row read its entries W at a time (one
// coalesced col load per chunk), filter and compact them, and broadcast them
// to gather UNROLL float4 row loads per lane at a time.
//   !NARROW  the whole wave walks one row: W = 64, the G lane groups take
//            disjoint neighbours of a chunk (G x UNROLL rows in flight) and
//            the caller adds their partials (combine_groups);
//   NARROW   each LPR-lane group walks a row of its own: W = LPR, control flow
//            is group-uniform and shuffles stay inside the group.  G rows
//            progress per wave, so latency-bound short rows get G x the
//            memory-level parallelism of the wave-per-row shape, which would
//            leave most of a 64-entry chunk empty.
// Returns this lane's partial (!NARROW: a disjoint subset of the neighbours;
// NARROW: its group's row sum).
// WEIGHTED: entry e's term is multiplied by val[e]; the value is loaded next
// to its column and follows it through the compaction, and the per-neighbour
// weight becomes val (PRESCALED, which then takes the fma form) or
// val * dinv_j (RAW, SPARSE).  Same order of terms as the unweighted sum.
// SCALED: the neighbour's scale is scale_src_j instead of dinv_j.
// DROPOUT: the lane that holds a column evaluates edge_keep for (row, column)
// ((column, row) in a transposed launch); the result joins the filter of the
// compaction, or is the whole filter of a launch without one, so a dropped
// neighbour's row is never read; the sum of the kept ones, in CSR order, is
// scaled by 1 / keep_prob once.  `row` is the destination row of [beg, end)
// (NARROW: of this lane's group); the other instantiations ignore it.
template <int D, int UNROLL, int MODE, bool MASKED, bool WEIGHTED, bool NARROW,
          bool SCALED = false, bool DROPOUT = false>
__device__ __forceinline__ float4 gather(const PropK &a, int64_t beg, int64_t end, int lane,
                                         int32_t row = 0) {
  constexpr int LPR = D / 4;
  constexpr int G = 64 / LPR;
  constexpr int W = NARROW ? LPR : 64;  // entries per chunk = lanes sharing it
  const int grp = lane / LPR;
  const int sub = lane % LPR;
  const int l0 = NARROW ? grp * LPR : 0;  // first of the lanes sharing the chunk
  const int me = NARROW ? sub : lane;     // this lane's position among them
  float4 acc = f4_zero();
  if (MODE == MIREC_IN_NONE) return acc;
  const float *src = (MODE == MIREC_IN_SPARSE) ? a.seed_in : a.x_in;
  for (int64_t base = beg; base < end; base += W) {
    int cnt = (int)min((int64_t)W, end - base);
    int myc = me < cnt ? a.col[base + me] : 0;
    float myv = 1.f;
    if constexpr (WEIGHTED) myv = me < cnt ? a.val[base + me] : 0.f;
    // SPARSE: the seed-row slot itself is the filter (slot >= 0 <=> node in
    // S), one dependent load less than a byte-map test followed by the slot
    // (with an in_mask, SPARSE tests the byte map first and reads the slot
    // of the hits only: fewer slot reads when many neighbours are seeded)
    const bool slot_filter = MODE == MIREC_IN_SPARSE && a.in_mask == nullptr;
    int myr = slot_filter ? (me < cnt ? a.slot[myc] : -1) : myc;
    if (MASKED || DROPOUT) {
      bool ok = me < cnt;
      if (MASKED) ok = me < cnt && (slot_filter ? myr >= 0 : bit_set(a.in_mask, myc));
      if constexpr (DROPOUT) {
        const uint32_t r = (uint32_t)row, c = (uint32_t)myc;
        ok = ok && edge_keep(a.drop_key, a.drop_transposed ? c : r, a.drop_transposed ? r : c,
                             a.drop_thresh_m1);
      }
      const unsigned long long bal = __ballot(ok);
      const unsigned long long m = (W == 64) ? bal : ((bal >> l0) & ((1ull << W) - 1ull));
      const int nv = __popcll(m);
      if (nv == 0) continue;  // uniform over the lanes sharing the chunk
      if (nv < cnt) {  // compact the valid entries to the front
        const int below = __popcll(m & ((1ull << me) - 1ull));
        const int dst = l0 + (ok ? below : nv + (me - below));
        myc = __builtin_amdgcn_ds_permute(dst << 2, myc);
        if (slot_filter) myr = __builtin_amdgcn_ds_permute(dst << 2, myr);
        if (WEIGHTED)
          myv = __int_as_float(__builtin_amdgcn_ds_permute(dst << 2, __float_as_int(myv)));
      }
      cnt = nv;
    }
    if (MODE != MIREC_IN_SPARSE) myr = myc;
    else if (!slot_filter) myr = me < cnt ? a.slot[myc] : 0;
    float myw = 1.f;
    if (MODE == MIREC_IN_RAW || MODE == MIREC_IN_SPARSE) {
      if (me < cnt) myw = SCALED ? a.scale_src[myc] : a.dinv[myc];
    }
    if (WEIGHTED) myw = me < cnt ? myv * myw : 0.f;
    if (MODE == MIREC_IN_SPARSE && myr < 0) {  // byte map set without a seed row
      myr = 0;
      myw = 0.f;
    }
    for (int k = 0; k < cnt; k += (NARROW ? 1 : G) * UNROLL) {
      float4 v[UNROLL];
      float w[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int idx = NARROW ? k + u : k + u * G + grp;
        const int srcl = l0 + (idx & (W - 1));
        const int j = __shfl(myr, srcl);
        w[u] = (MODE != MIREC_IN_PRESCALED || WEIGHTED) ? __shfl(myw, srcl) : 1.f;
        if (idx < cnt)
          v[u] = ld4(src + (int64_t)j * D + sub * 4);
        else
          v[u] = f4_zero();
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        if (MODE != MIREC_IN_PRESCALED || WEIGHTED)
          acc = f4_fma(w[u], v[u], acc);
        else
          acc = f4_add(acc, v[u]);
      }
    }
  }
  if constexpr (DROPOUT) acc = f4_scale(a.drop_scale, acc);
  return acc;
}

// Combine the G group partials: afterwards every group holds the row sum.
template <int D>
__device__ __forceinline__ float4 combine_groups(float4 s) {
  constexpr int LPR = D / 4;
#pragma unroll
  for (int m = LPR; m < 64; m <<= 1) s = f4_add(s, f4_shfl_xor(s, m));
  return s;
}

// Non-temporal forms of ld4 / st4, for streams touched once per step.
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4_nt(const float *p) {
  const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t *>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4_nt(float *p, float4 v) {
  const f32x4_t t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<f32x4_t *>(p));
}

// SCALED: a.dinv is the row sum's scale (set so by the host) and the row
// written to xs_out is scaled by scale_next instead.
// STREAM (mirec_prop_t.adam_stream): fused Adam reads and writes the table
// and its two moments non-temporally: 6 streams touched once per step, which
// otherwise pass through the caches that hold the gathered rows.  xs_out (the
// next step's gathered input), out, addend and the seed rows stay as they are.
template <int D, bool SCALED = false, bool STREAM = false>
__device__ __forceinline__ void row_epilogue(const PropK &a, int64_t row, float4 s, int sub) {
  const float di = a.dinv[row];
  float dn = di;
  if (SCALED && a.xs_out != nullptr) dn = a.scale_next[row];
  const int64_t off = row * D + sub * 4;
  float4 z = f4_scale(di, s);
  int sl = -1;
  if (a.slot != nullptr && (a.seed != nullptr || a.seed2 != nullptr)) sl = a.slot[row];
  if (a.seed != nullptr && sl >= 0) z = f4_add(z, ld4(a.seed + (int64_t)sl * D + sub * 4));
  if (a.xs_out != nullptr && a.param == nullptr) st4(a.xs_out + off, f4_scale(dn, z));
  if (a.out == nullptr && a.param == nullptr) return;
  if (a.out_mask != nullptr && a.param == nullptr && a.out_mask[row] == 0) return;
  float4 o = z;
  if (a.addend != nullptr) o = f4_add(o, ld4(a.addend + off));
  if (a.divisor != 1.f) o = f4_div(o, a.divisor);
  if (a.seed2 != nullptr && sl >= 0) o = f4_add(o, ld4(a.seed2 + (int64_t)sl * D + sub * 4));
  if (a.param != nullptr) {
    float4 p, m, v;
    if constexpr (STREAM) {
      p = ld4_nt(a.param + off), m = ld4_nt(a.m + off), v = ld4_nt(a.v + off);
    } else {
      p = ld4(a.param + off), m = ld4(a.m + off), v = ld4(a.v + off);
    }
    // torch.optim.Adam single-tensor path (torch/optim/adam.py:457-547):
    // exp_avg.lerp_(g, 1-b1); exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2);
    // denom = sqrt(v)/sqrt(bc2) + eps; p.addcdiv_(m, denom, -lr/bc1) — the
    // shared expression of every Adam kernel (common.h)
    adam1(p.x, m.x, v.x, o.x, a.adam);
    adam1(p.y, m.y, v.y, o.y, a.adam);
    adam1(p.z, m.z, v.z, o.z, a.adam);
    adam1(p.w, m.w, v.w, o.w, a.adam);
    if constexpr (STREAM) {
      st4_nt(a.param + off, p);
      st4_nt(a.m + off, m);
      st4_nt(a.v + off, v);
    } else {
      st4(a.param + off, p);
      st4(a.m + off, m);
      st4(a.v + off, v);
    }
    if (a.out != nullptr) st4(a.out + off, o);
    // with Adam, xs_out receives the pre-scaled UPDATED parameter
    if (a.xs_out != nullptr) st4(a.xs_out + off, f4_scale(dn, p));
  } else {
    st4(a.out + off, o);
  }
}

constexpr int kWavesPerBlock = 4;

// Row phase: wave w takes the G rows w*G .. w*G+G-1 (of the row list if
// given).  If all of them have degree <= narrow_max each group gathers its
// own row (gather's NARROW shape); otherwise the wave walks them one by one
// with the whole wave per row.  Segment phase: wave row_waves + s
// gathers segment s of a long row into `partial`.
// With a row list the list length is known only on the device: the grid is
// capped (kListBlocks) and blocks stride over the list's work items, so a
// short list does not pay for its host-side capacity in empty waves.
// MASKED = in_mask filter on neighbours, ROWMASK = row_mask filter on rows
// (separate instantiations so profiles tell full and pruned launches apart).
template <int D, int UNROLL, int MODE, bool MASKED, bool ROWMASK, bool WEIGHTED, bool SCALED,
          bool DROPOUT, bool STREAM = false>
__device__ __forceinline__ void prop_work(const PropK &a, int64_t w, int64_t nrows,
                                          int64_t row_waves) {
  constexpr int LPR = D / 4;
  constexpr int G = 64 / LPR;
  constexpr int NARROW_UNROLL = UNROLL < 4 ? 4 : UNROLL;
  const int lane = threadIdx.x & 63;
  const int sub = lane % LPR;
  const int grp = lane / LPR;
  if (w < row_waves) {
    const int64_t idx = w * G + grp;
    bool have = idx < nrows;
    int32_t row = 0;
    if (have) row = (ROWMASK && a.row_list != nullptr) ? a.row_list[idx] : (int32_t)idx;
    if (ROWMASK && have) have = bit_set(a.row_mask, row);
    int64_t beg = 0, end = 0;
    if (have) {
      beg = a.rowptr[row];
      end = a.rowptr[row + 1];
      if (a.split > 0 && end - beg > a.split) {  // segments handle it
        have = false;
        beg = end = 0;  // the narrow gather must not walk the long row
      }
    }
    const int64_t deg = have ? end - beg : 0;
    if (G > 1 && __ballot(deg > a.narrow_max) == 0ull) {
      float4 s = gather<D, NARROW_UNROLL, MODE, MASKED, WEIGHTED, true, SCALED, DROPOUT>(
          a, beg, end, lane, row);
      if (have) row_epilogue<D, SCALED, STREAM>(a, row, s, sub);
      return;
    }
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      const int src = g * LPR;
      if (!__shfl((int)have, src)) continue;  // wave-uniform
      const int32_t r = __shfl(row, src);
      const int64_t rb = __shfl((long long)beg, src);
      const int64_t re = __shfl((long long)end, src);
      float4 s =
          gather<D, UNROLL, MODE, MASKED, WEIGHTED, false, SCALED, DROPOUT>(a, rb, re, lane, r);
      s = combine_groups<D>(s);
      if (lane < LPR) row_epilogue<D, SCALED, STREAM>(a, r, s, sub);
    }
  } else {
    const int64_t sg = w - row_waves;
    if (sg >= a.n_seg) return;
    const int64_t row = a.seg_row[sg];
    if (ROWMASK && !bit_set(a.row_mask, row)) return;
    const int64_t beg = a.seg_beg[sg];
    const int64_t end = min(beg + (int64_t)a.split, a.rowptr[row + 1]);
    float4 s =
        gather<D, UNROLL, MODE, MASKED, WEIGHTED, false, SCALED, DROPOUT>(a, beg, end, lane,
                                                                          (int32_t)row);
    s = combine_groups<D>(s);
    if (lane < LPR) st4(a.partial + sg * D + sub * 4, s);
  }
}

// One row gathered by the whole 256-thread workgroup: wave q takes the q-th
// quarter of the row's entries, the four wave sums are added in wave order
// through LDS (deterministic), wave 0 runs the epilogue.  Block-uniform
// control flow (contains barriers).
template <int D, int UNROLL, int MODE, bool MASKED, bool WEIGHTED, bool SCALED, bool DROPOUT>
__device__ __forceinline__ void block_row(const PropK &a, int32_t row) {
  constexpr int LPR = D / 4;
  __shared__ float4 red[kWavesPerBlock - 1][LPR];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int sub = lane % LPR;
  const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
  if (a.split > 0 && end - beg > a.split) return;  // segments handle it (uniform)
  const int64_t q = (end - beg + kWavesPerBlock - 1) / kWavesPerBlock;
  const int64_t wb = min(beg + wid * q, end), we = min(wb + q, end);
  float4 s =
      gather<D, UNROLL, MODE, MASKED, WEIGHTED, false, SCALED, DROPOUT>(a, wb, we, lane, row);
  s = combine_groups<D>(s);
  if (wid > 0 && lane < LPR) red[wid - 1][sub] = s;
  __syncthreads();
  if (wid == 0 && lane < LPR) {
#pragma unroll
    for (int k = 0; k < kWavesPerBlock - 1; ++k) s = f4_add(s, red[k][sub]);
    row_epilogue<D, SCALED>(a, row, s, sub);
  }
  __syncthreads();  // red[] is reused by the block's next row
}

// One row gathered by one wave.
template <int D, int UNROLL, int MODE, bool MASKED, bool WEIGHTED, bool SCALED, bool DROPOUT>
__device__ __forceinline__ void wave_row(const PropK &a, int32_t row) {
  constexpr int LPR = D / 4;
  const int lane = threadIdx.x & 63;
  const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
  if (a.split > 0 && end - beg > a.split) return;  // segments handle it
  float4 s =
      gather<D, UNROLL, MODE, MASKED, WEIGHTED, false, SCALED, DROPOUT>(a, beg, end, lane, row);
  s = combine_groups<D>(s);
  if (lane < LPR) row_epilogue<D, SCALED>(a, row, s, lane % LPR);
}

// Grid of the list launches (their row counts live on the device): 4x the
// waves resident at 8 per SIMD.  4096 -> 8192: the row-masked launches
// 0.366 -> 0.357 ms, the SPARSE one 0.224 -> 0.208 ms, C2 4.666 -> 4.630
// ms per step (profiles/round6_ab_list_blocks.txt; 2048: 4.79, 16384: 4.63).
constexpr int64_t kListBlocks = 8192;

// Occupancy floor (waves per SIMD): keeps the register allocator at <= 72
// VGPRs so 7-8 waves per SIMD keep enough gathers in flight.
// MODE_W = in_mode, + kWeighted for an edge-weighted launch (csr->val), or
// + kScaled for a launch with scale vectors of its own, or + kDropout for an
// edge-dropout launch.
template <int D, int UNROLL, int MODE_W, bool MASKED, bool ROWMASK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 8)))
MIREC_NO_PK_F32 void prop_kernel(PropK a) {
  constexpr int MODE = MODE_W & 3;
  constexpr bool WEIGHTED = (MODE_W & kWeighted) != 0;
  constexpr bool SCALED = (MODE_W & kScaled) != 0;
  constexpr bool DROPOUT = (MODE_W & kDropout) != 0;
  constexpr bool STREAM = (MODE_W & kStream) != 0;
  constexpr int G = 64 / (D / 4);
  // wave index made provably uniform (SGPR): loop control stays scalar
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (!ROWMASK || a.row_list == nullptr) {
    prop_work<D, UNROLL, MODE, MASKED, ROWMASK, WEIGHTED, SCALED, DROPOUT, STREAM>(
        a, (int64_t)blockIdx.x * kWavesPerBlock + wid, a.n_rows, a.row_waves);
    return;
  }
  // List mode: the list lengths are known only on the device, so the grid
  // is capped (kListBlocks) and blocks stride over the work: first one
  // block per wide row, then G rows per wave of the narrow list, then the
  // long-row segments.
  // SPARSE launches mostly scan indices (few seeded neighbours): a wave
  // per wide row is enough there; gathering launches use a workgroup.
  constexpr int WPB = (MODE == MIREC_IN_SPARSE) ? kWavesPerBlock : 1;  // wide rows / block
  const int64_t n_wide = a.wide_list != nullptr ? (int64_t)*a.wide_count : 0;
  const int64_t wide_blocks = (n_wide + WPB - 1) / WPB;
  const int64_t nrows = *a.row_count;
  const int64_t row_waves = (nrows + G - 1) / G;
  const int64_t waves = row_waves + a.n_seg;
  const int64_t total = wide_blocks + (waves + kWavesPerBlock - 1) / kWavesPerBlock;
#pragma unroll 1
  for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
    if (b < wide_blocks) {
      if constexpr (WPB == 1) {
        block_row<D, UNROLL, MODE, MASKED, WEIGHTED, SCALED, DROPOUT>(a, a.wide_list[b]);
      } else {
        const int64_t i = b * WPB + wid;
        if (i < n_wide)
          wave_row<D, UNROLL, MODE, MASKED, WEIGHTED, SCALED, DROPOUT>(a, a.wide_list[i]);
      }
    } else {
      const int64_t w = (b - wide_blocks) * kWavesPerBlock + wid;
      if (w < waves)
        prop_work<D, UNROLL, MODE, MASKED, ROWMASK, WEIGHTED, SCALED, DROPOUT>(a, w, nrows,
                                                                               row_waves);
    }
  }
}

// ---- the seeded list launch (mirec_propagate_seeded): prop_kernel's list
// mode for in_mode SPARSE without an in_mask, i.e. the first backward layer,
// whose rows F1 = S ∪ N(S) hold ~23 entries per seeded one at C2.  There
// prop_kernel is a chain of dependent loads per work item (list entry,
// rowptr, col, slot[col], dinv[col] + seed row; the last four per chunk)
// whose slot[col] test reads a 4.4 MB array for a 6 K-node set.  Here
//   - the grid is the resident workgroups only, and each holds the bit forms
//     of S (mirec_seed_bits_t, exact or coarsened: a superset) in LDS;
//   - a work item issues its list entry's rowptr pair and row_mask byte
//     together, then NR chunks of column loads back to back;
//   - every column is tested against the LDS bits, and slot[col] and
//     dinv[col] are loaded for the passing lanes only (the others read
//     element 0 and drop it: every index-side load is unconditional), all
//     chunks in one round;
//   - the exact filter stays slot >= 0, and from there on a chunk is
//     gather<.., SPARSE, MASKED, ..>'s: the same compaction inside the chunk
//     of W entries, the same (k, u, grp) per compacted hit, the same fma
//     order, combine_groups and row_epilogue, so the launch is bitwise
//     prop_kernel's.
// No waits on other workgroups, no atomics; work items in prop_kernel's
// order (wide rows one per wave, then G narrow rows per wave).
struct SeededK {
  SeedBitsK bits;
  int64_t last;  // nnz - 1 >= 0: column loads past a row's end are clamped to it
};

// Chunks per round (bounded by the registers the column, slot and dinv loads
// of a round hold next to UNROLL float4 rows): 64-entry chunks of a wide row,
// LPR-entry chunks of a narrow one.
template <int D>
constexpr int seeded_wide_chunks() {
  return D >= 256 ? 2 : 4;
}
template <int D>
constexpr int seeded_narrow_chunks() {
  constexpr int n = 64 / (D / 4);
  return n < 2 ? 2 : (n > 4 ? 4 : n);
}

// One chunk of gather<D, UNROLL, SPARSE, true, false, NARROW>: `cnt` entries,
// this lane's entry being a hit iff myr (its slot) >= 0, myw = dinv of its
// column.  Control flow is uniform over the lanes sharing the chunk.
template <int D, int UNROLL, bool NARROW>
__device__ __forceinline__ float4 seeded_chunk(const PropK &a, float4 acc, int cnt, int myr,
                                               float myw, int lane) {
  constexpr int LPR = D / 4;
  constexpr int G = 64 / LPR;
  constexpr int W = NARROW ? LPR : 64;
  const int grp = lane / LPR;
  const int sub = lane % LPR;
  const int l0 = NARROW ? grp * LPR : 0;
  const int me = NARROW ? sub : lane;
  const bool ok = myr >= 0;
  const unsigned long long bal = __ballot(ok);
  const unsigned long long m = (W == 64) ? bal : ((bal >> l0) & ((1ull << (W & 63)) - 1ull));
  const int nv = __popcll(m);
  if (nv == 0) return acc;
  if (nv < cnt) {  // compact the hits to the front
    const int below = __popcll(m & ((1ull << me) - 1ull));
    const int dst = l0 + (ok ? below : nv + (me - below));
    myr = __builtin_amdgcn_ds_permute(dst << 2, myr);
    myw = __int_as_float(__builtin_amdgcn_ds_permute(dst << 2, __float_as_int(myw)));
  }
  if (myr < 0) {  // a lane past the hits: never gathered, its weight multiplies a zero row
    myr = 0;
    myw = 0.f;
  }
  for (int k = 0; k < nv; k += (NARROW ? 1 : G) * UNROLL) {
    float4 v[UNROLL];
    float w[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int idx = NARROW ? k + u : k + u * G + grp;
      const int srcl = l0 + (idx & (W - 1));
      const int j = __shfl(myr, srcl);
      w[u] = __shfl(myw, srcl);
      if (idx < nv)
        v[u] = ld4(a.seed_in + (int64_t)j * D + sub * 4);
      else
        v[u] = f4_zero();
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) acc = f4_fma(w[u], v[u], acc);
  }
  return acc;
}

// The `deg` entries from `beg` of a row (NARROW: of this lane group's row) in
// `rounds` rounds of NR chunks (wave-uniform; rounds * NR chunks cover the
// longest row of the wave).  Offsets into the row are 32-bit; a column load
// past the row's end is clamped to the CSR's last entry and dropped.
template <int D, int UNROLL, bool NARROW, int NR>
__device__ __forceinline__ float4 gather_seeded(const PropK &a, const SeededK &f,
                                                const uint32_t *bits, int64_t beg, int deg,
                                                int rounds, int lane) {
  constexpr int LPR = D / 4;
  constexpr int W = NARROW ? LPR : 64;
  const int me = NARROW ? lane % LPR : lane;
  const int32_t *cp = a.col + beg;
  const int lim = (int)min(f.last - beg, (int64_t)0x7fffffff);  // (-1: col[beg - 1] = col[last])
  float4 acc = f4_zero();
#pragma unroll 1
  for (int it = 0, off = me; it < rounds; ++it, off += NR * W) {
    int c[NR], s[NR];
    float w[NR];
    bool pass[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) c[r] = cp[min(off + r * W, lim)];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const uint32_t pos = seed_bit_pos(f.bits, c[r]);
      pass[r] = off + r * W < deg && ((bits[pos >> 5] >> (pos & 31u)) & 1u) != 0u;
      const int j = pass[r] ? c[r] : 0;
      s[r] = a.slot[j];
      w[r] = a.dinv[j];
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int cnt = max(0, min(W, deg - (off - me + r * W)));
      acc = seeded_chunk<D, UNROLL, NARROW>(a, acc, cnt, pass[r] ? s[r] : -1, w[r], lane);
    }
  }
  return acc;
}

// One row by one wave (prop_kernel's wave_row / the walk of a wave that holds
// a long row).
template <int D, int UNROLL>
__device__ __forceinline__ void seeded_wave_row(const PropK &a, const SeededK &f,
                                                const uint32_t *bits, int32_t row, int64_t beg,
                                                int deg, int lane) {
  constexpr int LPR = D / 4;
  constexpr int NRW = seeded_wide_chunks<D>();
  const int rounds = __builtin_amdgcn_readfirstlane((deg + NRW * 64 - 1) / (NRW * 64));
  float4 s = gather_seeded<D, UNROLL, false, NRW>(a, f, bits, beg, deg, rounds, lane);
  s = combine_groups<D>(s);
  if (lane < LPR) row_epilogue<D>(a, row, s, lane % LPR);
}

// (the body is a separate always-inline function, as the sweep kernels': the
// shuffle and ballot wrappers inline into it, and it into the kernel)
template <int D, int UNROLL>
__device__ __forceinline__ void seeded_work(const PropK &a, const SeededK &f) {
  constexpr int LPR = D / 4;
  constexpr int G = 64 / LPR;
  constexpr int NARROW_UNROLL = UNROLL < 4 ? 4 : UNROLL;
  constexpr int NRN = seeded_narrow_chunks<D>();
  extern __shared__ uint32_t seeded_bits[];
  const int n_words = f.bits.words0 + f.bits.words1;
  for (int i = threadIdx.x; i < n_words; i += 256) seeded_bits[i] = f.bits.bits[i];
  __syncthreads();
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_wide = a.wide_list != nullptr ? (int64_t)*a.wide_count : 0;
  const int64_t wide_blocks = (n_wide + kWavesPerBlock - 1) / kWavesPerBlock;
  const int64_t nrows = *a.row_count;
  const int64_t row_waves = (nrows + G - 1) / G;
  const int64_t total = wide_blocks + (row_waves + kWavesPerBlock - 1) / kWavesPerBlock;
#pragma unroll 1
  for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
    // The lane index is made opaque per work item: everything derived from it
    // (lane masks, the per-lane offsets into a dozen operand pointers) is then
    // recomputed here instead of being hoisted out of the loop, where those
    // values held more registers across a work item than the file has
    // (spills to scratch).
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    lane &= 63;  // (its range, known again: the shuffles' operands keep their known bits)
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    if (b < wide_blocks) {
      const int64_t i = b * kWavesPerBlock + wid;
      if (i >= n_wide) continue;  // wave-uniform
      const int32_t row = a.wide_list[i];
      const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
      seeded_wave_row<D, UNROLL>(a, f, seeded_bits, row, beg, (int)(end - beg), lane);
      continue;
    }
    const int64_t w = (b - wide_blocks) * kWavesPerBlock + wid;
    if (w >= row_waves) continue;  // wave-uniform
    const int64_t idx = w * G + grp;
    bool have = idx < nrows;
    const int32_t row = a.row_list[have ? idx : 0];
    const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
    have = have && a.row_mask[row] != 0;
    const int deg = have ? (int)(end - beg) : 0;
    if (G > 1 && __ballot(deg > a.narrow_max) == 0ull) {
      int rounds = (deg + NRN * LPR - 1) / (NRN * LPR);
#pragma unroll
      for (int m = LPR; m < 64; m <<= 1) rounds = max(rounds, __shfl_xor(rounds, m));
      rounds = __builtin_amdgcn_readfirstlane(rounds);
      float4 s = gather_seeded<D, NARROW_UNROLL, true, NRN>(a, f, seeded_bits, beg, deg, rounds,
                                                            lane);
      if (have) row_epilogue<D>(a, row, s, sub);
    } else {
#pragma unroll 1
      for (int g = 0; g < G; ++g) {
        const int src = g * LPR;
        if (!__shfl((int)have, src)) continue;  // wave-uniform
        seeded_wave_row<D, UNROLL>(a, f, seeded_bits, __shfl(row, src),
                                   __shfl((long long)beg, src), __shfl(deg, src), lane);
      }
    }
  }
}

template <int D, int UNROLL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 8)))
MIREC_NO_PK_F32 void prop_seeded_kernel(PropK a, SeededK f) {
  seeded_work<D, UNROLL>(a, f);
}

// One workgroup per long row: its NG = 256 / LPR lane groups sum the
// segments sg0 + k, sg0 + k + NG, ... (group k, 4 partial rows in flight),
// then group 0 adds the NG group sums in order and runs the epilogue.  A
// fixed two-level order (deterministic); a Zipf hub row of 800 segments is
// 50 loads deep per group instead of a serial walk of 800 dependent loads
// (258 -> ~15 us per launch on the C2 Zipf graph).
template <int D, bool SCALED>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void prop_finalize(PropK a, const int32_t *long_rows,
                                                     const int64_t *long_segptr, int64_t n_long) {
  constexpr int LPR = D / 4;
  constexpr int NG = 256 / LPR;
  constexpr int kF = 4;  // partial rows in flight per group
  __shared__ float4 red[NG][LPR];
  const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
  const int64_t li = blockIdx.x;
  if (li >= n_long) return;
  const int64_t row = long_rows[li];
  if (a.row_mask != nullptr && !bit_set(a.row_mask, row)) return;
  const int64_t s0 = long_segptr[li], s1 = long_segptr[li + 1];
  float4 s = f4_zero();
  for (int64_t sg = s0 + grp; sg < s1; sg += (int64_t)kF * NG) {
    float4 x[kF];
#pragma unroll
    for (int u = 0; u < kF; ++u) {
      const int64_t q = sg + (int64_t)u * NG;
      x[u] = q < s1 ? ld4(a.partial + q * D + sub * 4) : f4_zero();
    }
#pragma unroll
    for (int u = 0; u < kF; ++u)
      if (sg + (int64_t)u * NG < s1) s = f4_add(s, x[u]);
  }
  red[grp][sub] = s;
  __syncthreads();
  if (grp != 0) return;
  float4 t = red[0][sub];
#pragma unroll
  for (int k = 1; k < NG; ++k) t = f4_add(t, red[k][sub]);
  row_epilogue<D, SCALED>(a, row, t, sub);
}

// ---- column sweep (mirec_sweep_t): the item rows of a full PRESCALED launch.
// A uniformly gathered 256 MB user block gets nothing from an XCD's 4 MB L2:
// every neighbour row comes over the fabric.  Here a workgroup owns a tile of
// consecutive rows, accumulators in LDS, and walks the tile's entries in
// ascending SOURCE column; every workgroup sweeps the user block in the same
// direction at about the same pace, so the rows being gathered at any moment
// are a window of a few MB, which an XCD fetches once and then serves from
// its L2.  Each LPR-lane group owns a run of the tile's rows and a stream of
// their entries sorted by column (built on the host): no row is shared, no
// atomics, no reduction, one fixed summation order per row (ascending column,
// duplicate edges in CSR order).
//
// Pacing: the column range is cut into bands; a wave passes from band b to
// b + 1 through a bare s_barrier (no counter wait: it orders when loads are
// ISSUED, nothing is handed over through memory), so a workgroup's waves stay
// within a band of each other while row loads stay in flight across the band
// boundary.  Every wave executes exactly n_bands - 1 barriers whatever its
// streams hold.  Workgroups never wait for each other and nothing depends on
// which of them are resident; nothing holds them together either (measured,
// they drift tens of bands apart: the per-wave form below has an optional
// per-XCD pacing for that).
constexpr int kSweepThreads = 512;
// (80 KB: two workgroups fill a CU's 160 KB; the group form's tiles stay
// within the 64 KB a launch gets without asking)
constexpr int kSweepLdsMax = 80 * 1024;
constexpr int kSweepLdsDefault = 64 * 1024;  // dynamic LDS of a launch that asks for no more

struct SweepK {
  const int64_t *gptr;
  const long long *ent;  // (lrow << 32) | col per entry
  int64_t row0;
  int64_t n_rows;
  int32_t tile_rows;
  int32_t group_rows;
  int32_t groups;
  int32_t band_rows;
  int32_t n_bands;
};

template <int D, int U, bool SCALED>
__device__ __forceinline__ void sweep_work(const PropK &a, const SweepK &s) {
  constexpr int LPR = D / 4;
  static_assert(LPR % U == 0 && LPR <= 64, "a chunk of LPR entries is U-row batches");
  extern __shared__ float4 sweep_acc[];  // [tile_rows][LPR]
  const int lane = threadIdx.x & 63;
  const int sub = threadIdx.x % LPR;
  const int grp = threadIdx.x / LPR;  // lane group of the workgroup
  const int gbase = (lane / LPR) * LPR;
  const int64_t tile_row0 = (int64_t)blockIdx.x * s.tile_rows;
  const int tile_len = (int)min((int64_t)s.tile_rows, s.n_rows - tile_row0);
  const bool active = grp < s.groups;
  const int lr0 = active ? min(grp * s.group_rows, tile_len) : 0;
  const int lr1 = active ? min(lr0 + s.group_rows, tile_len) : 0;
  for (int lr = lr0; lr < lr1; ++lr) sweep_acc[lr * LPR + sub] = f4_zero();
  int64_t pos = 0, end = 0;
  if (active) {
    const int64_t sidx = (int64_t)blockIdx.x * s.groups + grp;
    pos = s.gptr[sidx];
    end = s.gptr[sidx + 1];
  }
  // entries past the stream's end read as column INT32_MAX (beyond every band)
  constexpr long long kNone = 0x7fffffffll;
  // Every global load below is unconditional (a clamped address, the value
  // dropped by a select): with loads under branches the compiler cannot
  // count them and waits for ALL outstanding loads at each use, which
  // serialises the batches.
  const int64_t last = max(end - 1, (int64_t)0);  // ent holds >= 1 entry
  long long cur = __builtin_nontemporal_load(s.ent + min(pos + sub, last));
  if (pos + sub >= end) cur = kNone;
  int band = 0;  // wave-uniform
  int64_t hi = s.band_rows;
  float4 pv[U];
  int pr[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    pv[u] = f4_zero();
    pr[u] = -1;
  }
  // chunks of the wave's longest stream (wave-uniform trip count)
  int n_chunks = (int)((end - pos + LPR - 1) / LPR);
#pragma unroll
  for (int m = LPR; m < 64; m <<= 1) n_chunks = max(n_chunks, __shfl_xor(n_chunks, m));
  n_chunks = __builtin_amdgcn_readfirstlane(n_chunks);
#pragma unroll 1
  for (int c = 0; c < n_chunks; ++c) {
    // the next chunk's entries, one chunk ahead
    long long nxt = __builtin_nontemporal_load(s.ent + min(pos + LPR + sub, last));
    if (pos + LPR + sub >= end) nxt = kNone;
    const int ccol = (int)(cur & 0xffffffffll);
    const int crow = (int)(cur >> 32);
#pragma unroll
    for (int k = 0; k < LPR; k += U) {
      // the wave enters the next band once none of its groups has an entry
      // of the current one left to issue
      const int nc = __shfl(ccol, gbase + k);
      while (band + 1 < s.n_bands && __ballot((int64_t)nc < hi) == 0ull) {
        __builtin_amdgcn_s_barrier();
        ++band;
        hi += s.band_rows;
      }
      float4 v[U];
      int r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = __shfl(ccol, gbase + k + u);
        const int rr = __shfl(crow, gbase + k + u);
        const bool ok = pos + k + u < end;
        r[u] = ok ? rr : -1;  // a slot past the end reads row 0 and is dropped
        v[u] = ld4(a.x_in + (int64_t)(ok ? j : 0) * D + sub * 4);
      }
      // add the PREVIOUS batch (its loads were issued a batch ago) while
      // this one is in flight; a row's terms are added in stream order
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (pr[u] >= 0) {
          float4 *p = &sweep_acc[pr[u] * LPR + sub];
          *p = f4_add(*p, pv[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pv[u] = v[u];
        pr[u] = r[u];
      }
    }
    pos += LPR;
    cur = nxt;
  }
  while (band + 1 < s.n_bands) {  // every wave executes the same number of barriers
    __builtin_amdgcn_s_barrier();
    ++band;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (pr[u] >= 0) {
      float4 *p = &sweep_acc[pr[u] * LPR + sub];
      *p = f4_add(*p, pv[u]);
    }
  }
  // rows are private to their group (same lanes wrote and read them)
  for (int lr = lr0; lr < lr1; ++lr)
    row_epilogue<D, SCALED>(a, s.row0 + tile_row0 + lr, sweep_acc[lr * LPR + sub], sub);
}

// (the body is a separate always-inline function: the shuffle and ballot
// wrappers inline into it, and it into the kernel, across the kernel's
// packed-f32 target attribute)
template <int D, int U, bool SCALED>
__global__ __launch_bounds__(kSweepThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
MIREC_NO_PK_F32 void prop_sweep_kernel(PropK a, SweepK s) {
  sweep_work<D, U, SCALED>(a, s);
}

// ---- per-wave form of the sweep (mirec_sweep_wave_t).  The four lane groups
// of a wave above walk four private streams in lockstep per ENTRY, so their
// column positions drift apart; here a wave walks ONE stream, its rows'
// entries merged by column and cut on the host into steps of 4 slots that
// name 4 different rows (or padding): one cursor per wave, and the 4 groups
// add into different LDS rows in the same instruction.  Slot k*16 + u*4 + g
// of a 64-slot chunk (one coalesced 512-B load, the next chunk prefetched)
// goes to lane group g as step u of batch k.  A pad slot carries a column
// of the stream (its load hits a line just used) and local row -1 (dropped),
// so every row load is unconditional and unclamped.  Same mechanics
// otherwise: two register buffers, the previous batch added while the next
// is in flight, a row's terms added one at a time in stream order (for the
// item rows bitwise what prop_sweep_kernel gives), bare s_barrier per band,
// decided from the first slot of a batch: the oldest pending entry, no
// later slot has a smaller column.  Every wave executes exactly n_bands - 1
// of them per tile.
// Passes: workgroup b takes the tiles b, b + grid, ...; nothing waits across
// workgroups and nothing depends on which of them are resident.
struct SweepWaveK {
  const int64_t *wptr;
  const long long *slot;  // (lrow << 32) | col per slot; lrow -1 = padding (PACKED: below)
  int64_t n_slots;
  int64_t row0;
  int64_t n_rows;
  int64_t src0;
  int32_t tile_rows;
  int32_t wave_rows;
  int32_t n_tiles;
  int32_t band_rows;
  int32_t n_bands;
  int32_t row_bits;  // PACKED: the row field's width (in the struct's tail padding)
};

// PACKED (mirec_sweep_wave_pack): `slot` holds 4-byte slots, the local row in
// the top row_bits bits (all ones = padding), the column relative to src0
// below them: one 256-B load per 64-slot chunk.  A chunk is decoded once into
// the same (absolute column, local row or -1) pair per lane; everything after
// that is the 8-byte form's code.
//
// Two optional instantiations beside the production one (AUX = kAuxNone,
// whose code they leave as it is):
//
// kAuxPace, per-XCD pacing.  Between workgroups nothing holds the window of
// source rows together; here wave 0 of a workgroup, at its band advance and
// before the band's s_barrier, adds to its XCD's sum of advances and naps
// while its own count leads the XCD's mean (sum / registered workgroups) by
// more than `lead` bands.  The nap loop runs at most kPaceMaxNaps times: no
// workgroup ever waits UNTIL anything, so a launch ends whatever the
// workspace holds and whichever workgroups are resident; a stale or wrong
// figure costs time only.  The workspace is touched with non-returning
// vector atomics and read through the scalar data cache (lgkmcnt), so the
// row loads' vmcnt waits never see it.  A leaving workgroup takes its share
// out of the sum and the count; the last one to leave zeroes the region.
//
// kAuxStamp, a measurement: wave 0 notes wall_clock64() in LDS at the tile's
// start, at every band advance and at the tile's end, and writes the notes
// out after the tile's epilogue with the workgroup's index and XCC id.
constexpr int kAuxNone = 0, kAuxPace = 1, kAuxStamp = 2;
constexpr int kPaceLabels = 8;          // XCC ids
constexpr int kPaceLineWords = 32;      // one 128-B line per counter
constexpr int kPaceRegionWords = (2 * kPaceLabels + 1) * kPaceLineWords;
constexpr int kPaceMaxNaps = 8;         // polls (and naps) per paced advance
constexpr int kPaceMaxNapUnits = 16;    // s_sleep 8 (512 clocks) per nap, at most
constexpr int kXccIdReg = 20 | (3 << 11);  // hwreg(HW_REG_XCC_ID, 0, 4)

struct SweepAuxK {
  unsigned *ws;        // kAuxPace: this launch's region, kPaceRegionWords words
  int32_t lead;
  int32_t every;
  int32_t nap;
  long long *stamps;   // kAuxStamp: [n_tiles][n_bands + 1]
  int32_t *meta;       // kAuxStamp: [n_tiles][2] = workgroup, XCC id
};

// One dword through the scalar data cache, bypassing it (glc): served by the
// L2, counted by lgkmcnt.
__device__ __forceinline__ unsigned pace_read(const unsigned *p) {
  unsigned v;
  asm volatile("s_load_dword %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(v)
               : "s"(p)
               : "memory");
  return v;
}

//
// INMASK (mirec_propagate_sweep_wave_masked; unscaled, no STREAM):
// the sweep of a launch with an in_mask.  Each lane tests the column of its
// slot against the byte map; a failing lane turns its slot into padding
// (local row -1: the term is dropped by the pr[u] >= 0 test below) and names
// the block's first source row src0 as its LOAD column, a valid row that
// stays in L1 and whose contents are never added.  The byte of chunk i + 1 is
// loaded in the middle of chunk i, once its slot has arrived (the add of
// batch 0 has waited for it already) and two batches before it is used: no
// row load waits for a byte requested in its own iteration.  Every row load
// stays unconditional and unclamped.
// The band decision reads the STATIC column of a batch's first slot, before
// any redirection, so the bands a wave walks, the number of s_barrier it
// executes per tile (n_bands - 1) and its calls of pace() are those of the
// unmasked launch of the same layout whatever the mask holds: no wave can
// miss a barrier that the others of its workgroup execute.  There is no
// other wait, flag or dependence between workgroups.  A row's passing terms
// are added in stream order: the sum is bitwise the unmasked sweep's of an
// input whose masked-out rows are +0.0.
template <int D, int U, bool SCALED, int AUX = kAuxNone, bool PACKED = false,
          bool STREAM = false, bool INMASK = false>
__device__ __forceinline__ void sweep_wave_work(const PropK &a, const SweepWaveK &s,
                                                const SweepAuxK &x = SweepAuxK{}) {
  constexpr int LPR = D / 4;
  constexpr int G = 64 / LPR;          // lane groups = slots per step
  constexpr int NB = 64 / (U * G);     // batches per 64-slot chunk
  static_assert(G == 4 && U * G == MIREC_SWEEP_BATCH && kSweepThreads / 64 == MIREC_SWEEP_WAVES,
                "the host layout's steps, batches and waves");
  static_assert(!INMASK || (!SCALED && !STREAM && AUX != kAuxStamp && NB >= 3),
                "the masked forms a step uses");
  extern __shared__ float4 sweep_acc[];  // [tile_rows][LPR]
  const int lane = threadIdx.x & 63;
  const int sub = lane % LPR;
  const int g = lane / LPR;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  using Slot = typename std::conditional<PACKED, unsigned, long long>::type;
  const Slot *slots = reinterpret_cast<const Slot *>(s.slot);
  [[maybe_unused]] const int col_bits = 32 - s.row_bits;
  const Slot kPadRow = PACKED ? (Slot)(~0u << col_bits) : (Slot)0xffffffff00000000ull;
  const int64_t last = s.n_slots - 1;  // >= 0 (checked by the host)
  // a slot's absolute column (INMASK: the byte map's index)
  [[maybe_unused]] auto slot_col = [&](Slot v) -> int64_t {
    if constexpr (PACKED) return s.src0 + (int64_t)(v & ~kPadRow);
    return (int64_t)(v & 0xffffffffll);
  };
  // kAuxPace (wave 0): band advances of this workgroup since the kernel's
  // start, how many of them the XCD's sum holds, advances until the next poll
  int adv = 0, told = 0, due = 0;
  unsigned *pace_reg = nullptr, *pace_sum = nullptr;
  if constexpr (AUX == kAuxPace) {
    const int label = (int)__builtin_amdgcn_s_getreg(kXccIdReg) & (kPaceLabels - 1);
    pace_reg = x.ws + (2 * label) * kPaceLineWords;
    pace_sum = pace_reg + kPaceLineWords;
    due = x.every;
    if (wid == 0 && lane == 0)
      (void)__hip_atomic_fetch_add(pace_reg, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // wave 0, before the barrier of a band advance
  auto pace = [&]() {
    if constexpr (AUX == kAuxPace) {
      if (wid != 0) return;
      ++adv;
      if (--due != 0) return;
      due = x.every;
      if (lane == 0)
        (void)__hip_atomic_fetch_add(pace_sum, (unsigned)(adv - told), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
      told = adv;
#pragma unroll 1
      for (int i = 0; i < kPaceMaxNaps; ++i) {  // a constant trip count: never a wait-until
        const long long sum = pace_read(pace_sum), reg = pace_read(pace_reg);
        if ((long long)(adv - x.lead) * reg <= sum) break;  // lead <= x.lead (or no count yet)
#pragma unroll 1
        for (int j = 0; j < x.nap; ++j) __builtin_amdgcn_s_sleep(8);
      }
    }
  };
  [[maybe_unused]] long long *stamp_lds = nullptr;
  if constexpr (AUX == kAuxStamp)
    stamp_lds = reinterpret_cast<long long *>(sweep_acc + (int64_t)s.tile_rows * LPR);
  auto stamp = [&](int i) {
    if constexpr (AUX == kAuxStamp) {
      if (wid == 0 && lane == 0) stamp_lds[i] = (long long)wall_clock64();
    }
  };
#pragma unroll 1
  for (int tile = blockIdx.x; tile < s.n_tiles; tile += gridDim.x) {
    stamp(0);
    const int64_t tile_row0 = (int64_t)tile * s.tile_rows;
    const int tile_len = (int)min((int64_t)s.tile_rows, s.n_rows - tile_row0);
    const int lr0 = min(wid * s.wave_rows, tile_len);
    const int lr1 = min(lr0 + s.wave_rows, tile_len);
    for (int lr = lr0 + g; lr < lr1; lr += G) sweep_acc[lr * LPR + sub] = f4_zero();
    int64_t pos = s.wptr[(int64_t)tile * MIREC_SWEEP_WAVES + wid];
    const int64_t end = s.wptr[(int64_t)tile * MIREC_SWEEP_WAVES + wid + 1];
    const int n_batches = __builtin_amdgcn_readfirstlane((int)((end - pos) / (U * G)));
    // slots past the stream's end are padding (their column: a slot of the
    // layout, inside the source block)
    Slot cur = __builtin_nontemporal_load(slots + min(pos + lane, last));
    if (lane >= n_batches * (U * G)) cur |= kPadRow;
    // INMASK: the byte of this lane's slot of `cur` (every slot's column lies
    // inside the source block, padding and slots past the end included)
    [[maybe_unused]] int cmask = 1, nmask = 1;
    if constexpr (INMASK) {
      cmask = a.in_mask[slot_col(cur)];
      // (the byte's wait stands here, before the loop, and the next chunk's
      // at the loop's end: at the loop's head no byte is pending on either
      // path, so the compiler puts no wait for one before the row loads)
      asm volatile("" : "+v"(cmask));
    }
    int band = 0;
    int64_t hi = s.src0 + s.band_rows;
    float4 pv[U];
    int pr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      pv[u] = f4_zero();
      pr[u] = -1;
    }
#pragma unroll 1
    for (int b0 = 0; b0 < n_batches; b0 += NB) {
      Slot nxt = __builtin_nontemporal_load(slots + min(pos + 64 + lane, last));
      if (b0 * (U * G) + 64 + lane >= n_batches * (U * G)) nxt |= kPadRow;
      int ccol, crow;
      if constexpr (PACKED) {
        ccol = (int)s.src0 + (int)(cur & ~kPadRow);
        crow = cur >= kPadRow ? -1 : (int)(cur >> col_bits);
      } else {
        ccol = (int)(cur & 0xffffffffll);
        crow = (int)(cur >> 32);
      }
      // the column a lane's row load names: its own, or src0 when masked out
      // (ccol itself keeps deciding the bands)
      int lcol = ccol;
      if constexpr (INMASK) {
        if (cmask == 0) {
          crow = -1;
          lcol = (int)s.src0;
        }
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        // the wave enters the next band once its oldest pending entry lies
        // beyond the current one (batches past the end decide nothing)
        const int nc = __builtin_amdgcn_readlane(ccol, k * U * G);
        while (b0 + k < n_batches && band + 1 < s.n_bands && (int64_t)nc >= hi) {
          pace();
          __builtin_amdgcn_s_barrier();
          ++band;
          hi += s.band_rows;
          stamp(band);
        }
        if constexpr (INMASK) {
          // the next chunk's bytes: its slots arrived before batch 0 was added
          if (k == 2) nmask = a.in_mask[slot_col(nxt)];
        }
        float4 v[U];
        int r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int src = k * U * G + u * G + g;
          const int j = __shfl(lcol, src);
          r[u] = __shfl(crow, src);
          v[u] = ld4(a.x_in + (int64_t)j * D + sub * 4);
        }
        // add the PREVIOUS batch while this one is in flight; the G slots of
        // a step name different rows, so the groups do not race
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (pr[u] >= 0) {
            float4 *p = &sweep_acc[pr[u] * LPR + sub];
            *p = f4_add(*p, pv[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          pv[u] = v[u];
          pr[u] = r[u];
        }
      }
      pos += 64;
      cur = nxt;
      if constexpr (INMASK) {
        // a counted wait: the two batches of row loads issued after the byte
        // stay in flight
        asm volatile("" : "+v"(nmask));
        cmask = nmask;
      }
    }
    while (band + 1 < s.n_bands) {  // every wave executes the same number of barriers
      pace();
      __builtin_amdgcn_s_barrier();
      ++band;
      stamp(band);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (pr[u] >= 0) {
        float4 *p = &sweep_acc[pr[u] * LPR + sub];
        *p = f4_add(*p, pv[u]);
      }
    }
    // rows are private to their wave
    for (int lr = lr0 + g; lr < lr1; lr += G)
      row_epilogue<D, SCALED, STREAM>(a, s.row0 + tile_row0 + lr, sweep_acc[lr * LPR + sub],
                                      sub);
    if constexpr (AUX == kAuxStamp) {
      stamp(s.n_bands);
      if (wid == 0) {  // (a wave's LDS instructions complete in order)
        long long *o = x.stamps + (int64_t)tile * (s.n_bands + 1);
        for (int b = lane; b <= s.n_bands; b += 64) o[b] = stamp_lds[b];
        if (lane == 0) {
          x.meta[2 * tile] = (int32_t)blockIdx.x;
          x.meta[2 * tile + 1] = (int32_t)__builtin_amdgcn_s_getreg(kXccIdReg);
        }
      }
    }
    __syncthreads();  // the accumulators are reused by the workgroup's next tile
  }
  if constexpr (AUX == kAuxPace) {
    // leave: take this workgroup out of its XCD's mean; the last workgroup
    // of the launch to leave zeroes the region for the next launch
    if (wid == 0 && lane == 0) {
      (void)__hip_atomic_fetch_add(pace_sum, 0u - (unsigned)told, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(pace_reg, 0u - 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's adds are done
      unsigned *done = x.ws + 2 * kPaceLabels * kPaceLineWords;
      const unsigned left = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
      if (left == gridDim.x - 1) {
        for (int i = 0; i <= 2 * kPaceLabels; ++i)
          __hip_atomic_store(x.ws + i * kPaceLineWords, 0u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

template <int D, int U, bool SCALED, bool PACKED = false, bool STREAM = false>
__global__ __launch_bounds__(kSweepThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
MIREC_NO_PK_F32 void prop_sweep_wave_kernel(PropK a, SweepWaveK s) {
  sweep_wave_work<D, U, SCALED, kAuxNone, PACKED, STREAM>(a, s);
}

template <int D, int U, bool SCALED, int AUX, bool PACKED = false, bool STREAM = false>
__global__ __launch_bounds__(kSweepThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
MIREC_NO_PK_F32 void prop_sweep_wave_aux_kernel(PropK a, SweepWaveK s, SweepAuxK x) {
  sweep_wave_work<D, U, SCALED, AUX, PACKED, STREAM>(a, s, x);
}

// The in_mask forms (sweep_wave_work's INMASK): kernels of their own, so the
// ones above keep their names and their code.
template <int D, int U, bool PACKED>
__global__ __launch_bounds__(kSweepThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
MIREC_NO_PK_F32 void prop_sweep_wave_masked_kernel(PropK a, SweepWaveK s) {
  sweep_wave_work<D, U, false, kAuxNone, PACKED, false, true>(a, s);
}

template <int D, int U, int AUX, bool PACKED>
__global__ __launch_bounds__(kSweepThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
MIREC_NO_PK_F32 void prop_sweep_wave_masked_aux_kernel(PropK a, SweepWaveK s, SweepAuxK x) {
  sweep_wave_work<D, U, false, AUX, PACKED, false, true>(a, s, x);
}

using PropFn = void (*)(PropK);

// The prop_kernel instantiation of a launch.  SPARSE exists only MASKED (it
// always filters: by slot >= 0 without an in_mask), NONE only unmasked and
// unweighted (it reads no neighbours).  The cases stand in the order the
// kernels have in the code object, which follows their first use here.
// The kScaled cases come after all the earlier ones, so those keep their
// places; scaled and weighted never meet (refused in propagate()).  The
// kDropout cases follow them in turn (dropout meets neither; a NONE launch
// gathers nothing, so it has no dropout form).
template <int D, int UNROLL>
static PropFn prop_kernel_for(int mode, bool masked, bool rowmask, bool weighted, bool scaled,
                              bool dropout) {
  if (mode == MIREC_IN_SPARSE) masked = true;
  if (mode == MIREC_IN_NONE) weighted = dropout = false;
#define MIREC_PROP_CASE(MODE_W, MASKED)                               \
  case (MODE_W) * 2 + (MASKED):                                       \
    return rowmask ? prop_kernel<D, UNROLL, (MODE_W), MASKED, true>   \
                   : prop_kernel<D, UNROLL, (MODE_W), MASKED, false>;
  switch ((mode | (weighted ? kWeighted : 0) | (scaled ? kScaled : 0) |
           (dropout ? kDropout : 0)) * 2 + masked) {
    MIREC_PROP_CASE(MIREC_IN_PRESCALED | kWeighted, false)
    MIREC_PROP_CASE(MIREC_IN_PRESCALED, false)
    MIREC_PROP_CASE(MIREC_IN_PRESCALED | kWeighted, true)
    MIREC_PROP_CASE(MIREC_IN_PRESCALED, true)
    MIREC_PROP_CASE(MIREC_IN_RAW | kWeighted, false)
    MIREC_PROP_CASE(MIREC_IN_RAW, false)
    MIREC_PROP_CASE(MIREC_IN_RAW | kWeighted, true)
    MIREC_PROP_CASE(MIREC_IN_RAW, true)
    MIREC_PROP_CASE(MIREC_IN_SPARSE | kWeighted, true)
    MIREC_PROP_CASE(MIREC_IN_SPARSE, true)
    MIREC_PROP_CASE(MIREC_IN_PRESCALED | kScaled, false)
    MIREC_PROP_CASE(MIREC_IN_PRESCALED | kScaled, true)
    MIREC_PROP_CASE(MIREC_IN_RAW | kScaled, false)
    MIREC_PROP_CASE(MIREC_IN_RAW | kScaled, true)
    MIREC_PROP_CASE(MIREC_IN_SPARSE | kScaled, true)
    MIREC_PROP_CASE(MIREC_IN_NONE | kScaled, false)
    MIREC_PROP_CASE(MIREC_IN_PRESCALED | kDropout, false)
    MIREC_PROP_CASE(MIREC_IN_PRESCALED | kDropout, true)
    MIREC_PROP_CASE(MIREC_IN_RAW | kDropout, false)
    MIREC_PROP_CASE(MIREC_IN_RAW | kDropout, true)
    MIREC_PROP_CASE(MIREC_IN_SPARSE | kDropout, true)
    default:  // in_mask is refused with NONE (mirec_propagate_sweep)
    MIREC_PROP_CASE(MIREC_IN_NONE, false)
  }
#undef MIREC_PROP_CASE
}

template <int D, int UNROLL>
static int launch_prop(const mirec_csr_t *c, PropK k, int64_t list_cap, int mode,
                       hipStream_t st, bool dropout = false, bool stream = false) {
  constexpr int G = 64 / (D / 4);
  const int64_t rows = k.row_list != nullptr ? list_cap : c->n_rows;
  k.row_waves = (rows + G - 1) / G;
  const int64_t work = k.row_waves + c->n_seg;
  const bool scaled = !dropout && k.scale_next != nullptr;  // (shared storage, PropK)
  int64_t blocks = (work + kWavesPerBlock - 1) / kWavesPerBlock;
  if (k.row_list != nullptr) {
    if (k.wide_list != nullptr) blocks += list_cap;
    blocks = std::min(blocks, kListBlocks);
  }
  if (blocks > 0) {
    PropFn kernel =
        prop_kernel_for<D, UNROLL>(mode, k.in_mask != nullptr, k.row_mask != nullptr,
                                   !dropout && k.val != nullptr, scaled, dropout);
    if constexpr (D == 64) {
      // a full launch with streaming Adam (the other shapes have no such form:
      // the flag is a cache hint)
      if (stream && k.param != nullptr && mode == MIREC_IN_PRESCALED && k.in_mask == nullptr &&
          k.row_mask == nullptr && k.val == nullptr && !dropout)
        kernel = scaled
                     ? prop_kernel<D, UNROLL, MIREC_IN_PRESCALED | kScaled | kStream, false, false>
                     : prop_kernel<D, UNROLL, MIREC_IN_PRESCALED | kStream, false, false>;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, k);
    MIREC_LAUNCH_CHECK();
  }
  if (c->n_long > 0) {
    const auto fin = scaled ? prop_finalize<D, true> : prop_finalize<D, false>;
    hipLaunchKernelGGL(fin, dim3((unsigned)c->n_long), dim3(256), 0, st, k, c->long_rows,
                       c->long_segptr, c->n_long);
    MIREC_LAUNCH_CHECK();
  }
  return MIREC_OK;
}

// The seeded list launch: as many workgroups as stay resident with the bit
// arrays in LDS (asked of the runtime once per array size), or fewer when
// the lists cannot hold that much work.
constexpr size_t kSeededLdsMax = 64 * 1024;

template <int D, int UNROLL>
static int launch_seeded(PropK k, const mirec_seed_bits_t *sb, int64_t nnz, int64_t list_cap,
                         hipStream_t st) {
  constexpr int G = 64 / (D / 4);
  SeededK f;
  f.bits = seed_bits_k(sb);
  f.last = nnz - 1;
  const size_t lds = 4 * ((size_t)f.bits.words0 + (size_t)f.bits.words1);
  const auto kernel = prop_seeded_kernel<D, UNROLL>;
  static thread_local size_t cached_lds = 0;
  static thread_local int64_t cached_resident = 0;
  if (cached_resident == 0 || cached_lds != lds) {
    int dev = 0, cus = 0, per_cu = 0;
    MIREC_HIP(hipGetDevice(&dev));
    MIREC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    MIREC_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, reinterpret_cast<const void *>(kernel), 256, lds));
    cached_resident = (int64_t)std::max(per_cu, 1) * std::max(cus, 1);
    cached_lds = lds;
  }
  const int64_t row_waves = (list_cap + G - 1) / G;
  int64_t blocks = (row_waves + kWavesPerBlock - 1) / kWavesPerBlock;
  if (k.wide_list != nullptr) blocks += (list_cap + kWavesPerBlock - 1) / kWavesPerBlock;
  blocks = std::min(blocks, cached_resident);
  if (blocks > 0) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, st, k, f);
    MIREC_LAUNCH_CHECK();
  }
  return MIREC_OK;
}

// x~ = dinv ⊙ x (row scale), float4.
__global__ __launch_bounds__(256) void prescale_kernel(const float *__restrict__ x,
                                                       const float *__restrict__ dinv, int64_t n4,
                                                       int32_t d4, float *__restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
    st4(out + 4 * i, f4_scale(dinv[i / d4], ld4(x + 4 * i)));
}

// ---- per-entry dot (mirec_edge_dot): out[e] = <a[row(e)], b[col[e]]> for
// every CSR entry, the gradient of y = A x with respect to the entry values
// (a = dL/dy, b = x).  Balanced by ENTRIES: a wave owns kDotChunk consecutive
// entries whatever rows they belong to, so a hub row is spread over many
// waves and no wave's work depends on the maximum degree.  The rows of the
// chunk's first and last entries are found by binary search in rowptr (the
// last row r with rowptr[r] <= e: empty rows are stepped over); a lane then
// finds the row of its own entry inside that range, which is a single row
// for a chunk inside a hub.  Like the wave-per-row gather, 64 columns are read per
// coalesced load and broadcast; an LPR-lane group takes one entry at a time
// (one float4 of each row per lane), reduces the products inside the group
// and hands the sum to the lane that holds the entry, so the 64 results are
// stored coalesced.  Every entry is written once; no atomics.
constexpr int kDotChunk = 256;

__device__ __forceinline__ int32_t row_of_entry(const int64_t *rowptr, int32_t lo, int32_t hi,
                                                int64_t e) {
  while (lo < hi) {  // invariant: rowptr[lo] <= e, the answer lies in [lo, hi]
    const int32_t mid = lo + (hi - lo + 1) / 2;
    if (rowptr[mid] <= e)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

template <int D, int UNROLL>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void edge_dot_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n_rows,
    int64_t nnz, const float *__restrict__ a, const float *__restrict__ b,
    float *__restrict__ out) {
  constexpr int LPR = D / 4;
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR;
  const int sub = lane % LPR;
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t e0 = wave * kDotChunk;
  if (e0 >= nnz) return;  // wave-uniform
  const int64_t e1 = min(e0 + (int64_t)kDotChunk, nnz);
  const int32_t r_lo = row_of_entry(rowptr, 0, (int32_t)(n_rows - 1), e0);
  const int32_t r_hi = row_of_entry(rowptr, r_lo, (int32_t)(n_rows - 1), e1 - 1);
  for (int64_t base = e0; base < e1; base += 64) {
    const int cnt = (int)min((int64_t)64, e1 - base);
    const int myc = lane < cnt ? col[base + lane] : 0;
    const int myrow = lane < cnt ? row_of_entry(rowptr, r_lo, r_hi, base + lane) : r_lo;
    float res = 0.f;
    for (int k = 0; k < cnt; k += G * UNROLL) {
      float4 va[UNROLL], vb[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int idx = k + u * G + grp;
        const int j = __shfl(myc, idx & 63);
        const int r = __shfl(myrow, idx & 63);
        if (idx < cnt) {
          va[u] = ld4(a + (int64_t)r * D + sub * 4);
          vb[u] = ld4(b + (int64_t)j * D + sub * 4);
        } else {
          va[u] = f4_zero();
          vb[u] = f4_zero();
        }
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const float d = group_sum<LPR>(f4_dot(va[u], vb[u]));
        // entry k + u*G + g was summed by group g: lane k + u*G + g takes it
        const float t = __shfl(d, (lane & (G - 1)) * LPR);
        if (lane >= k + u * G && lane < k + (u + 1) * G) res = t;
      }
    }
    if (lane < cnt) out[base + lane] = res;
  }
}

template <int D, int UNROLL>
static int launch_edge_dot(const mirec_csr_t *c, const float *a, const float *b, float *out,
                           hipStream_t st) {
  const int64_t waves = (c->nnz + kDotChunk - 1) / kDotChunk;
  const int64_t blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL((edge_dot_kernel<D, UNROLL>), dim3((unsigned)blocks), dim3(256), 0, st,
                     c->rowptr, c->col, c->n_rows, c->nnz, a, b, out);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

// The sweep path's qualifying rule; the graph-side part
// (bipartite, enough rows, a source block larger than L2) is decided where
// the layout is built.  First the launch-side part, shared by both forms.
// `in_mask_ok`: the caller has a masked form for the launch (the wave form
// only, and only where mirec_propagate_sweep_wave_masked asks for it).
static bool sweep_launch_qualifies(const mirec_csr_t *c, const mirec_prop_t *p,
                                   bool in_mask_ok = false) {
  if (p->dim != 64) return false;
  if (c->val != nullptr) return false;  // the sweep layouts carry no values
  if (p->in_mode != MIREC_IN_PRESCALED) return false;
  if (p->in_mask != nullptr && !in_mask_ok) return false;
  if (p->row_mask != nullptr || p->row_list != nullptr) return false;
  return c->n_seg == 0;
}

static bool sweep_qualifies(const mirec_csr_t *c, const mirec_prop_t *p, const mirec_sweep_t *sw) {
  if (sw == nullptr || !sweep_launch_qualifies(c, p)) return false;
  if (sw->gptr == nullptr || sw->ent == nullptr || sw->n_rows <= 0 || sw->n_tiles <= 0)
    return false;
  if (sw->row0 < 0 || sw->row0 + sw->n_rows != c->n_rows || sw->n_src > c->n_rows) return false;
  if (sw->tile_rows <= 0 || sw->group_rows <= 0 || sw->band_rows <= 0) return false;
  if (sw->groups <= 0 || sw->groups > kSweepThreads / (64 / 4)) return false;
  if ((int64_t)sw->groups * sw->group_rows < sw->tile_rows) return false;
  if ((int64_t)sw->n_tiles * sw->tile_rows < sw->n_rows) return false;
  if ((int64_t)sw->tile_rows * 64 * 4 > kSweepLdsDefault) return false;
  return true;
}

// Rows [0, row0) of a launch whose other rows were swept: the row kernel.
template <int D, int UNROLL>
static int launch_head(const mirec_csr_t *c, const PropK &k, int64_t row0, hipStream_t st) {
  mirec_csr_t head = *c;
  head.n_rows = row0;
  head.n_long = 0;  // (no segments in a launch that qualifies: nothing to finalize)
  PropK kh = k;
  kh.n_rows = row0;  // the last wave's groups past row0 - 1 stay idle
  return launch_prop<D, UNROLL>(&head, kh, 0, MIREC_IN_PRESCALED, st);
}

// Rows [row0, n_rows) of a PRESCALED launch by the row kernel: the same launch
// on a CSR that begins at row0 (what a row indexes is shifted; x_in, in_mask
// and the seed rows, which columns and slots index, are not).
template <int D, int UNROLL>
static int launch_tail(const mirec_csr_t *c, const PropK &k, int64_t row0, hipStream_t st) {
  mirec_csr_t tail = *c;
  tail.n_rows = c->n_rows - row0;
  // (a launch that reaches here has no long-row segments, sweep_launch_qualifies;
  // their lists name absolute rows and would not fit the shifted pointers)
  if (c->n_seg != 0 || c->n_long != 0) return MIREC_ERR_ARG;
  PropK kt = k;
  kt.n_rows = tail.n_rows;
  kt.rowptr += row0;
  kt.dinv += row0;
  if (kt.slot != nullptr) kt.slot += row0;
  if (kt.out_mask != nullptr) kt.out_mask += row0;
  const int64_t off = row0 * D;
  if (kt.out != nullptr) kt.out += off;
  if (kt.xs_out != nullptr) kt.xs_out += off;
  if (kt.addend != nullptr) kt.addend += off;
  if (kt.param != nullptr) kt.param += off, kt.m += off, kt.v += off;
  return launch_prop<D, UNROLL>(&tail, kt, 0, MIREC_IN_PRESCALED, st);
}

// Item rows by the sweep kernel, rows [0, row0) by the row kernel.
template <int D, int UNROLL>
static int launch_sweep(const mirec_csr_t *c, const PropK &k, const mirec_sweep_t *sw,
                        hipStream_t st) {
  SweepK s;
  s.gptr = sw->gptr;
  s.ent = reinterpret_cast<const long long *>(sw->ent);
  s.row0 = sw->row0;
  s.n_rows = sw->n_rows;
  s.tile_rows = sw->tile_rows;
  s.group_rows = sw->group_rows;
  s.groups = sw->groups;
  s.band_rows = sw->band_rows;
  s.n_bands = (int32_t)std::max<int64_t>(1, (sw->n_src + sw->band_rows - 1) / sw->band_rows);
  const size_t lds = (size_t)sw->tile_rows * D * sizeof(float);
  const auto kernel =
      k.scale_next != nullptr ? prop_sweep_kernel<D, 4, true> : prop_sweep_kernel<D, 4, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)sw->n_tiles), dim3(kSweepThreads), lds, st, k, s);
  MIREC_LAUNCH_CHECK();
  if (sw->row0 == 0) return MIREC_OK;
  return launch_head<D, UNROLL>(c, k, sw->row0, st);
}

// A well-formed per-wave layout of the rows [row0, row0 + n_rows) of `c`.
static bool sweep_wave_valid(const mirec_csr_t *c, const mirec_sweep_wave_t *w, int64_t row0,
                             int64_t n_rows) {
  if (w == nullptr || w->wptr == nullptr || w->slot == nullptr || w->n_slots <= 0) return false;
  if (w->row0 != row0 || w->n_rows != n_rows || n_rows <= 0 || w->n_tiles <= 0) return false;
  if (w->src0 < 0 || w->n_src <= 0 || w->src0 + w->n_src > c->n_rows) return false;
  if (w->tile_rows <= 0 || w->wave_rows <= 0 || w->band_rows <= 0) return false;
  if ((int64_t)w->wave_rows * MIREC_SWEEP_WAVES < w->tile_rows) return false;
  if ((int64_t)w->n_tiles * w->tile_rows < n_rows) return false;
  if ((int64_t)(w->n_tiles - 1) * w->tile_rows >= n_rows) return false;
  if ((int64_t)w->tile_rows * 64 * 4 > kSweepLdsMax) return false;
  if (w->row_bits != 0) {  // packed slots: both fields hold what the layout names
    if (w->row_bits < 1 || w->row_bits > 31) return false;
    if ((int64_t)w->tile_rows >= ((int64_t)1 << w->row_bits)) return false;
    if (w->n_src > ((int64_t)1 << (32 - w->row_bits))) return false;
  }
  return w->grid > 0 && w->grid <= w->n_tiles;
}

// A launch with more dynamic LDS than the default limit needs the kernel's
// limit raised first: once per kernel and device.
static int sweep_lds_allow(const void *kernel, size_t lds) {
  if (lds <= (size_t)kSweepLdsDefault) return MIREC_OK;
  static std::mutex mu;
  static std::set<std::pair<const void *, int>> raised;
  int dev = 0;
  MIREC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (raised.count({kernel, dev}) != 0) return MIREC_OK;
  MIREC_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                kSweepLdsMax));
  raised.insert({kernel, dev});
  return MIREC_OK;
}

// The stamping launch's buffers (mirec_sweep_wave_stamp).
struct SweepStamp {
  const mirec_sweep_wave_t *layout;
  int64_t *stamps;
  int64_t stamps_len;
  int32_t *meta;
};

static int32_t sweep_wave_bands(const mirec_sweep_wave_t *w) {
  return (int32_t)std::max<int64_t>(1, (w->n_src + w->band_rows - 1) / w->band_rows);
}

// `pace` with block = 0 (items) or 1 (users): that block's region and
// parameters (every == 0: the block runs unpaced); `stamp`: the measurement;
// `masked`: the in_mask forms (unscaled: checked by the caller).
template <int D>
static int launch_sweep_wave(const PropK &k, const mirec_sweep_wave_t *w, hipStream_t st,
                             const mirec_sweep_pace_t *pace = nullptr, int block = 0,
                             const SweepStamp *stamp = nullptr, bool stream = false,
                             bool masked = false) {
  SweepWaveK s;
  s.wptr = w->wptr;
  s.slot = reinterpret_cast<const long long *>(w->slot);
  s.n_slots = w->n_slots;
  s.row0 = w->row0;
  s.n_rows = w->n_rows;
  s.src0 = w->src0;
  s.tile_rows = w->tile_rows;
  s.wave_rows = w->wave_rows;
  s.n_tiles = w->n_tiles;
  s.band_rows = w->band_rows;
  s.n_bands = sweep_wave_bands(w);
  s.row_bits = w->row_bits;
  size_t lds = (size_t)w->tile_rows * D * sizeof(float);
  const bool scaled = k.scale_next != nullptr;
  const bool packed = w->row_bits != 0;
  // streaming Adam has packed forms only (a cache hint: 8-byte layouts run without it)
  stream = stream && packed && k.param != nullptr;
  if (masked && (scaled || stamp != nullptr || k.in_mask == nullptr))
    return MIREC_ERR_ARG;
  if (masked && pace != nullptr && pace->every[block] > 0) {
    SweepAuxK x = {};
    x.ws = reinterpret_cast<unsigned *>(pace->ws) + block * kPaceRegionWords;
    x.lead = pace->lead_bands[block];
    x.every = pace->every[block];
    x.nap = pace->nap[block];
    const auto kernel = packed ? prop_sweep_wave_masked_aux_kernel<D, 4, kAuxPace, true>
                               : prop_sweep_wave_masked_aux_kernel<D, 4, kAuxPace, false>;
    const int rc = sweep_lds_allow(reinterpret_cast<const void *>(kernel), lds);
    if (rc != MIREC_OK) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)w->grid), dim3(kSweepThreads), lds, st, k, s, x);
  } else if (masked) {
    const auto kernel = packed ? prop_sweep_wave_masked_kernel<D, 4, true>
                               : prop_sweep_wave_masked_kernel<D, 4, false>;
    const int rc = sweep_lds_allow(reinterpret_cast<const void *>(kernel), lds);
    if (rc != MIREC_OK) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)w->grid), dim3(kSweepThreads), lds, st, k, s);
  } else if (stamp != nullptr) {
    SweepAuxK x = {};
    x.stamps = reinterpret_cast<long long *>(stamp->stamps);
    x.meta = stamp->meta;
    lds += (size_t)(s.n_bands + 1) * sizeof(long long);
    if (packed) return MIREC_ERR_ARG;  // the stamping kernel reads 8-byte slots
    const auto kernel = scaled ? prop_sweep_wave_aux_kernel<D, 4, true, kAuxStamp>
                               : prop_sweep_wave_aux_kernel<D, 4, false, kAuxStamp>;
    if (lds > (size_t)kSweepLdsDefault &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return MIREC_ERR_HIP;
    hipLaunchKernelGGL(kernel, dim3((unsigned)w->grid), dim3(kSweepThreads), lds, st, k, s, x);
  } else if (pace != nullptr && pace->every[block] > 0) {
    SweepAuxK x = {};
    x.ws = reinterpret_cast<unsigned *>(pace->ws) + block * kPaceRegionWords;
    x.lead = pace->lead_bands[block];
    x.every = pace->every[block];
    x.nap = pace->nap[block];
    auto kernel = scaled ? prop_sweep_wave_aux_kernel<D, 4, true, kAuxPace>
                         : prop_sweep_wave_aux_kernel<D, 4, false, kAuxPace>;
    if (packed)
      kernel = scaled ? prop_sweep_wave_aux_kernel<D, 4, true, kAuxPace, true>
                      : prop_sweep_wave_aux_kernel<D, 4, false, kAuxPace, true>;
    if (stream)
      kernel = scaled ? prop_sweep_wave_aux_kernel<D, 4, true, kAuxPace, true, true>
                      : prop_sweep_wave_aux_kernel<D, 4, false, kAuxPace, true, true>;
    const int rc = sweep_lds_allow(reinterpret_cast<const void *>(kernel), lds);
    if (rc != MIREC_OK) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)w->grid), dim3(kSweepThreads), lds, st, k, s, x);
  } else {
    auto kernel = scaled ? prop_sweep_wave_kernel<D, 4, true> : prop_sweep_wave_kernel<D, 4, false>;
    if (packed)
      kernel = scaled ? prop_sweep_wave_kernel<D, 4, true, true>
                      : prop_sweep_wave_kernel<D, 4, false, true>;
    if (stream)
      kernel = scaled ? prop_sweep_wave_kernel<D, 4, true, true, true>
                      : prop_sweep_wave_kernel<D, 4, false, true, true>;
    const int rc = sweep_lds_allow(reinterpret_cast<const void *>(kernel), lds);
    if (rc != MIREC_OK) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)w->grid), dim3(kSweepThreads), lds, st, k, s);
  }
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

}  // namespace mirec

extern "C" int mirec_sweep_groups(int32_t dim) {
  return dim == 64 ? mirec::kSweepThreads / (64 / 4) : 0;
}

namespace mirec {

// The one body of the three propagate entries: at most one of `sw` (group
// form) and `wi` (wave form, `wu` optional beside it) is given.
static int propagate(const mirec_csr_t *c, const mirec_prop_t *p, const mirec_sweep_t *sw,
                     const mirec_sweep_wave_t *wi, const mirec_sweep_wave_t *wu,
                     mirec_stream_t stream, const mirec_drop_t *drop = nullptr,
                     const mirec_sweep_pace_t *pace = nullptr,
                     const SweepStamp *stamp = nullptr,
                     const mirec_seed_bits_t *seeded = nullptr, int32_t masked_blocks = 0) {
  MIREC_CHECK_ARG(c != nullptr && p != nullptr);
  MIREC_CHECK_ARG((masked_blocks & ~(MIREC_SWEEP_MASKED_ITEMS | MIREC_SWEEP_MASKED_USERS)) == 0);
  if (pace != nullptr) {
    MIREC_CHECK_ARG(pace->ws != nullptr);
    for (int b = 0; b < 2; ++b)
      MIREC_CHECK_ARG(pace->every[b] >= 0 && pace->lead_bands[b] >= 0 && pace->nap[b] >= 0 &&
                      pace->nap[b] <= kPaceMaxNapUnits);
  }
  MIREC_CHECK_ARG(c->rowptr != nullptr && c->dinv != nullptr && c->n_rows >= 0);
  MIREC_CHECK_ARG(c->nnz == 0 || c->col != nullptr);
  if (!dim_supported(p->dim)) return MIREC_ERR_DIM;
  MIREC_CHECK_ARG(p->in_mode >= 0 && p->in_mode <= 3);
  if (p->in_mode == MIREC_IN_SPARSE)
    MIREC_CHECK_ARG(p->slot != nullptr && p->seed_in != nullptr);
  else if (p->in_mode != MIREC_IN_NONE)
    MIREC_CHECK_ARG(p->x_in != nullptr);
  MIREC_CHECK_ARG(p->in_mode != MIREC_IN_NONE || p->in_mask == nullptr);
  MIREC_CHECK_ARG((p->seed == nullptr && p->seed2 == nullptr) || p->slot != nullptr);
  MIREC_CHECK_ARG(p->param == nullptr || (p->exp_avg != nullptr && p->exp_avg_sq != nullptr));
  MIREC_CHECK_ARG(p->divisor != 0.f);
  MIREC_CHECK_ARG(p->row_list == nullptr ||
                  (p->row_count != nullptr && p->row_list_cap >= 0 && p->row_mask != nullptr));
  MIREC_CHECK_ARG(p->wide_list == nullptr || (p->row_list != nullptr && p->wide_count != nullptr));
  if (c->n_seg > 0) {
    MIREC_CHECK_ARG(c->split > 0 && c->seg_row && c->seg_beg && c->long_rows && c->long_segptr);
    if (p->partial == nullptr) return MIREC_ERR_WORKSPACE;
  }
  PropK k;
  k.rowptr = c->rowptr;
  k.col = c->col;
  k.dinv = c->dinv;
  k.n_rows = c->n_rows;
  k.n_seg = c->n_seg;
  k.seg_row = c->seg_row;
  k.seg_beg = c->seg_beg;
  k.split = c->n_seg > 0 ? c->split : 0;
  k.x_in = p->x_in;
  k.slot = p->slot;
  k.seed_in = p->seed_in;
  k.seed = p->seed;
  k.addend = p->addend;
  k.seed2 = p->seed2;
  k.divisor = p->divisor;
  k.out = p->out;
  k.xs_out = p->xs_out;
  k.param = p->param;
  k.m = p->exp_avg;
  k.v = p->exp_avg_sq;
  k.adam = p->adam;
  k.partial = p->partial;
  k.row_mask = p->row_mask;
  k.in_mask = p->in_mask;
  k.out_mask = p->out_mask;
  k.row_list = p->row_list;
  k.row_count = p->row_count;
  k.row_waves = 0;
  k.narrow_max = p->narrow_max;
  k.wide_list = p->wide_list;
  k.wide_count = p->wide_count;
  k.val = c->val;
  // A launch that names any scale runs the kScaled instantiations with all
  // three resolved (NULL = csr->dinv); they carry no edge weights.
  const bool scaled =
      p->scale_src != nullptr || p->scale_dst != nullptr || p->scale_next != nullptr;
  MIREC_CHECK_ARG(!scaled || c->val == nullptr);
  k.scale_src = k.scale_next = nullptr;
  if (scaled) {
    k.scale_src = p->scale_src != nullptr ? p->scale_src : c->dinv;
    k.dinv = p->scale_dst != nullptr ? p->scale_dst : c->dinv;
    k.scale_next = p->scale_next != nullptr ? p->scale_next : c->dinv;
  }
  // Edge dropout (mirec_propagate_drop, keep_prob != 0) runs the kDropout
  // instantiations: no edge weights, no scales of its own, keep_prob in (0, 1]
  // (a NaN fails too); it comes without sweep layouts (the sweep kernels have
  // no mask), so it runs the row kernel below.
  const bool dropout = drop != nullptr && drop->keep_prob != 0.f;
  if (dropout) {
    uint32_t thresh_m1 = 0;
    MIREC_CHECK_ARG(edge_drop_thresh(drop->keep_prob, &thresh_m1));
    MIREC_CHECK_ARG(c->val == nullptr && !scaled);
    k.drop_key = edge_drop_key(drop->seed);  // (the storage of val and the scales)
    k.drop_thresh_m1 = thresh_m1;
    k.drop_transposed = drop->transposed != 0;
    k.scale_next = nullptr;  // (all 8 bytes of the storage drop_scale shares)
    k.drop_scale = 1.f / drop->keep_prob;
  }
  const int64_t cap = p->row_list_cap;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool nt = p->adam_stream != 0 && p->param != nullptr;
  if (stamp != nullptr) {
    // the measurement: one block's launch, nothing else (its other rows stay unwritten)
    const mirec_sweep_wave_t *w = stamp->layout;
    MIREC_CHECK_ARG(w != nullptr && stamp->stamps != nullptr && stamp->meta != nullptr);
    MIREC_CHECK_ARG(sweep_launch_qualifies(c, p) && w->row0 >= 0 && w->n_rows > 0 &&
                    w->row0 + w->n_rows <= c->n_rows &&
                    sweep_wave_valid(c, w, w->row0, w->n_rows));
    MIREC_CHECK_ARG(stamp->stamps_len >= (int64_t)w->n_tiles * (sweep_wave_bands(w) + 1));
    return launch_sweep_wave<64>(k, w, st, nullptr, 0, stamp);
  }
  if (sweep_qualifies(c, p, sw)) return launch_sweep<64, 4>(c, k, sw, st);
  if (wi != nullptr && sweep_launch_qualifies(c, p) &&
      sweep_wave_valid(c, wi, wi->row0, c->n_rows - wi->row0)) {
    const int rc = launch_sweep_wave<64>(k, wi, st, pace, 0, nullptr, nt);
    if (rc != MIREC_OK || wi->row0 == 0) return rc;
    if (sweep_wave_valid(c, wu, 0, wi->row0))
      return launch_sweep_wave<64>(k, wu, st, pace, 1, nullptr, nt);
    return launch_head<64, 4>(c, k, wi->row0, st);
  }
  // A launch with an in_mask whose caller asks for the masked sweep of a block
  // (mirec_propagate_sweep_wave_masked): that block by the masked form of the
  // wave sweep (no scales of its own), the other block's rows
  // by the row kernel.  Everything else falls through to the row kernel.
  if (masked_blocks != 0 && p->in_mask != nullptr && !scaled && wi != nullptr &&
      sweep_launch_qualifies(c, p, true) &&
      sweep_wave_valid(c, wi, wi->row0, c->n_rows - wi->row0)) {
    const bool mi = (masked_blocks & MIREC_SWEEP_MASKED_ITEMS) != 0;
    const bool mu = (masked_blocks & MIREC_SWEEP_MASKED_USERS) != 0 && wi->row0 > 0 &&
                    sweep_wave_valid(c, wu, 0, wi->row0);
    if (mi || mu) {
      const int rc = mi ? launch_sweep_wave<64>(k, wi, st, pace, 0, nullptr, false, true)
                        : launch_tail<64, 4>(c, k, wi->row0, st);
      if (rc != MIREC_OK || wi->row0 == 0) return rc;
      return mu ? launch_sweep_wave<64>(k, wu, st, pace, 1, nullptr, false, true)
                : launch_head<64, 4>(c, k, wi->row0, st);
    }
  }
  if (seeded != nullptr) {  // (a launch of the seeded shape: mirec_propagate_seeded)
    switch (p->dim) {
      case 4: return launch_seeded<4, 1>(k, seeded, c->nnz, cap, st);
      case 8: return launch_seeded<8, 1>(k, seeded, c->nnz, cap, st);
      case 16: return launch_seeded<16, 1>(k, seeded, c->nnz, cap, st);
      case 32: return launch_seeded<32, 2>(k, seeded, c->nnz, cap, st);
      case 64: return launch_seeded<64, 4>(k, seeded, c->nnz, cap, st);
      case 128: return launch_seeded<128, 4>(k, seeded, c->nnz, cap, st);
      // (UNROLL batches the row loads only: hit idx of a chunk goes to group
      // idx % G and a group adds its hits in ascending idx whatever UNROLL is;
      // 4 rows per batch keep the 256-wide kernel free of spills)
      case 256: return launch_seeded<256, 4>(k, seeded, c->nnz, cap, st);
    }
    return MIREC_ERR_DIM;
  }
  switch (p->dim) {
    case 4: return launch_prop<4, 1>(c, k, cap, p->in_mode, st, dropout);
    case 8: return launch_prop<8, 1>(c, k, cap, p->in_mode, st, dropout);
    case 16: return launch_prop<16, 1>(c, k, cap, p->in_mode, st, dropout);
    case 32: return launch_prop<32, 2>(c, k, cap, p->in_mode, st, dropout);
    case 64: return launch_prop<64, 4>(c, k, cap, p->in_mode, st, dropout, nt);
    case 128: return launch_prop<128, 4>(c, k, cap, p->in_mode, st, dropout);
    case 256: return launch_prop<256, 8>(c, k, cap, p->in_mode, st, dropout);
  }
  return MIREC_ERR_DIM;
}

}  // namespace mirec

extern "C" int mirec_propagate(const mirec_csr_t *c, const mirec_prop_t *p,
                               mirec_stream_t stream) {
  return mirec_propagate_sweep(c, p, nullptr, stream);
}

extern "C" int mirec_propagate_sweep(const mirec_csr_t *c, const mirec_prop_t *p,
                                     const mirec_sweep_t *sw, mirec_stream_t stream) {
  return mirec::propagate(c, p, sw, nullptr, nullptr, stream);
}

extern "C" int mirec_propagate_sweep_wave(const mirec_csr_t *c, const mirec_prop_t *p,
                                          const mirec_sweep_wave_t *items,
                                          const mirec_sweep_wave_t *users,
                                          mirec_stream_t stream) {
  return mirec::propagate(c, p, nullptr, items, users, stream);
}

extern "C" size_t mirec_sweep_pace_sizeof(void) { return sizeof(mirec_sweep_pace_t); }

extern "C" size_t mirec_sweep_pace_ws_bytes(void) {
  return 2 * (size_t)mirec::kPaceRegionWords * sizeof(unsigned);
}

extern "C" int mirec_propagate_sweep_wave_paced(const mirec_csr_t *c, const mirec_prop_t *p,
                                                const mirec_sweep_wave_t *items,
                                                const mirec_sweep_wave_t *users,
                                                const mirec_sweep_pace_t *pace,
                                                mirec_stream_t stream) {
  return mirec::propagate(c, p, nullptr, items, users, stream, nullptr, pace);
}

extern "C" int mirec_propagate_sweep_wave_masked(const mirec_csr_t *c, const mirec_prop_t *p,
                                                 const mirec_sweep_wave_t *items,
                                                 const mirec_sweep_wave_t *users,
                                                 const mirec_sweep_pace_t *pace,
                                                 int32_t blocks, mirec_stream_t stream) {
  return mirec::propagate(c, p, nullptr, items, users, stream, nullptr, pace, nullptr, nullptr,
                          blocks);
}

extern "C" int mirec_sweep_wave_stamp(const mirec_csr_t *c, const mirec_prop_t *p,
                                      const mirec_sweep_wave_t *layout, int64_t *stamps,
                                      int64_t stamps_len, int32_t *meta, mirec_stream_t stream) {
  const mirec::SweepStamp s = {layout, stamps, stamps_len, meta};
  return mirec::propagate(c, p, nullptr, nullptr, nullptr, stream, nullptr, nullptr, &s);
}

extern "C" size_t mirec_drop_sizeof(void) { return sizeof(mirec_drop_t); }

extern "C" int mirec_propagate_drop(const mirec_csr_t *c, const mirec_prop_t *p,
                                    const mirec_drop_t *drop, mirec_stream_t stream) {
  return mirec::propagate(c, p, nullptr, nullptr, nullptr, stream, drop);
}

extern "C" int mirec_propagate_seeded(const mirec_csr_t *c, const mirec_prop_t *p,
                                      const mirec_seed_bits_t *filter, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(c != nullptr && p != nullptr);
  const bool shape = filter != nullptr && p->in_mode == MIREC_IN_SPARSE &&
                     p->row_list != nullptr && p->in_mask == nullptr && c->val == nullptr &&
                     c->n_seg == 0 && c->nnz > 0 && p->scale_src == nullptr &&
                     p->scale_dst == nullptr && p->scale_next == nullptr;
  if (!shape) return mirec_propagate(c, p, stream);
  MIREC_CHECK_ARG(seed_bits_valid(filter, c->n_rows));
  const size_t lds = 4 * ((size_t)filter->words[0] + (size_t)filter->words[1]);
  if (lds == 0 || lds > kSeededLdsMax) return mirec_propagate(c, p, stream);
  return propagate(c, p, nullptr, nullptr, nullptr, stream, nullptr, nullptr, nullptr, filter);
}

extern "C" int mirec_edge_keep_mask(const int64_t *rowptr, const int32_t *col, int64_t n_rows,
                                    uint64_t seed, float keep_prob, int32_t transposed,
                                    uint8_t *keep) {
  using namespace mirec;
  MIREC_CHECK_ARG(rowptr != nullptr && n_rows >= 0);
  uint32_t thresh_m1 = 0;
  MIREC_CHECK_ARG(edge_drop_thresh(keep_prob, &thresh_m1));
  if (n_rows == 0 || rowptr[n_rows] == rowptr[0]) return MIREC_OK;
  MIREC_CHECK_ARG(col != nullptr && keep != nullptr);
  const uint64_t key = edge_drop_key(seed);
  for (int64_t i = 0; i < n_rows; ++i) {
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const uint32_t r = (uint32_t)i, c = (uint32_t)col[e];
      keep[e] = edge_keep(key, transposed ? c : r, transposed ? r : c, thresh_m1) ? 1 : 0;
    }
  }
  return MIREC_OK;
}

extern "C" int mirec_edge_dot(const mirec_csr_t *c, const float *a, const float *b, int32_t dim,
                              float *out, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(c != nullptr && c->rowptr != nullptr && c->n_rows >= 0 && c->nnz >= 0);
  if (!dim_supported(dim)) return MIREC_ERR_DIM;
  if (c->nnz == 0) return MIREC_OK;
  MIREC_CHECK_ARG(c->n_rows > 0 && c->col != nullptr && a != nullptr && b != nullptr &&
                  out != nullptr);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (dim) {
    case 4: return launch_edge_dot<4, 1>(c, a, b, out, st);
    case 8: return launch_edge_dot<8, 1>(c, a, b, out, st);
    case 16: return launch_edge_dot<16, 1>(c, a, b, out, st);
    case 32: return launch_edge_dot<32, 2>(c, a, b, out, st);
    case 64: return launch_edge_dot<64, 4>(c, a, b, out, st);
    case 128: return launch_edge_dot<128, 4>(c, a, b, out, st);
    case 256: return launch_edge_dot<256, 4>(c, a, b, out, st);
  }
  return MIREC_ERR_DIM;
}

extern "C" int mirec_prescale(const float *x, const float *dinv, int64_t n_rows, int32_t dim,
                              float *out, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(x && dinv && out && n_rows >= 0);
  if (!dim_supported(dim)) return MIREC_ERR_DIM;
  const int64_t n4 = n_rows * dim / 4;
  if (n4 == 0) return MIREC_OK;
  const int64_t blocks = std::min<int64_t>((n4 + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(prescale_kernel, dim3(blocks), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, dinv, n4, dim / 4, out);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}
