// Dot-product attention hop (PyG TransformerConv, concat=True, beta=False, no
// edge features, no attention dropout, root_weight=True; model/tgrec.py:161-171)
// on the fixed-fanout tree of sage.hip and on the full CSR graph.  The four
// projections q = lin_query(x), skip = lin_skip(x) of the targets and k =
// lin_key(x), v = lin_value(x) of the children come from the MFMA GEMMs
// before these kernels; per target i and head h, over the slots j in S(i)
// (children with valid >= 0, a repeated id once per slot, NO self slot):
//   s_j = <q_i,h, k_j,h> * scale,  alpha_j = softmax_j s_j
//   out_i,h = Σ_j alpha_j v_j,h (+ skip_i,h)
//
//   mirec_fanout_tattn      forward on the tree; keeps alpha if asked
//   mirec_fanout_tattn_bwd  ∂q, ∂skip, ∂k, ∂v from alpha
//   mirec_csr_tattn         forward over every CSR row (full-graph inference)
//
// Rows are addressed through a stride in floats, so q | skip and k | v may be
// the two halves of one [n, 2D] GEMM output (and the gradients the two halves
// of the buffer the GEMM's backward reads): no copy either way.
//
// Layout: headrow.h's (shared with gat.hip) — one group of lanes per target,
// a float4 column per lane, a head's dot summed inside the lanes that own it.
//
// Forward: every k row and every v row is read once.  There is no self slot
// to seed the online softmax, so it starts empty (headrow.h, softmax_empty)
// and a target without a valid child is decided by the state's flag, not by
// a division: it gets its skip row as loaded, bit for bit, and alpha slots
// of exactly 0.  Children come in batches of 8: flags, then 8 k rows and 8 v
// rows in flight, the 8 head dots, one rescale per batch.  When alpha is kept
// the raw s_j go to the alpha buffer and the lane that wrote them normalises
// them in place once the final (max, sum) is known.
//
// Backward: two passes over a target's v rows (the second one a cache hit),
// one over its k rows.  Pass 1 reads v_j and sums S = Σ_m alpha_m dalpha_m,
// dalpha_j = <g, v_j>; pass 2 reads v_j again and k_j, recomputes the same
// f32 dalpha_j, forms ds_j = alpha_j (dalpha_j - S) and writes ∂v_j = alpha_j
// g, ∂k_j = ds_j scale q_i and, after the loop, ∂q_i = Σ_j ds_j scale k_j.
// S and ds_j are kept in double: with a saturated softmax dalpha_j - S is Σ_m
// alpha_m (dalpha_j - dalpha_m), orders below its terms, and ∂q / ∂k are
// built from it; both passes form the same f32 dalpha_j, so its rounding
// cancels exactly (gat.hip).  Every child row has one
// parent, so all four outputs are plain stores: no atomics, no partial sums,
// no workspace, one lane group per target and no grid-stride loop.
#include "headrow.h"

namespace mirec {

// out row of a finished state: the aggregate (none for a childless target:
// no division) plus the skip row, which a childless target gets as loaded.
__device__ __forceinline__ void tat_store(const SoftmaxState &S, const float *skip_row,
                                          float *out_row) {
  float4 o = S.any ? f4_scale(1.f / S.l, S.acc) : f4_zero();
  if (skip_row != nullptr) {
    const float4 sk = ld4(skip_row);
    o = S.any ? f4_add(o, sk) : sk;
  }
  st4(out_row, o);
}

template <bool POW2>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void fanout_tattn_kernel(
    const float *__restrict__ q, const float *__restrict__ skip, int64_t ld_q,
    const float *__restrict__ key, const float *__restrict__ val, int64_t ld_kv,
    const int32_t *__restrict__ valid, int64_t n_t, int32_t k, int32_t heads, int32_t d4,
    int32_t g, int32_t lg, float scale, float *__restrict__ out, float *alpha) {
  const HeadLane L = head_lane(lg, d4, g);
  const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lg;
  const bool live = t < n_t;
  const bool act = live && L.col;
  const int64_t D = (int64_t)d4 * 4;
  const float4 qv = act ? ld4(q + t * ld_q + 4 * L.sub) : f4_zero();
  SoftmaxState S = softmax_empty();
  const bool keep_a = alpha != nullptr && live && L.lead;
  float *arow = alpha != nullptr && live ? alpha + (t * k) * heads + L.h : nullptr;
  for (int c0 = 0; c0 < k; c0 += kHeadBatch) {
    bool ok[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u)
      ok[u] = live && c0 + u < k && (valid == nullptr || valid[t * k + c0 + u] >= 0);
    float4 kr[kHeadBatch], vr[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      const int64_t off = (t * k + c0 + u) * ld_kv + 4 * L.sub;
      kr[u] = (act && ok[u]) ? ld4(key + off) : f4_zero();
      vr[u] = (act && ok[u]) ? ld4(val + off) : f4_zero();
    }
    float s[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      s[u] = head_sum<POW2>(f4_dot_fma(qv, kr[u]), g, L.hb) * scale;
      if (keep_a && c0 + u < k) arow[(int64_t)(c0 + u) * heads] = ok[u] ? s[u] : 0.f;
    }
    softmax_fold(S, s, vr, ok);
  }
  if (act)
    tat_store(S, skip != nullptr ? skip + t * ld_q + 4 * L.sub : nullptr, out + t * D + 4 * L.sub);
  if (keep_a && S.any) {
    // the lane that wrote the raw s_j turns them into alpha_j
    const float inv = 1.f / S.l;
    for (int c = 0; c < k; ++c) {
      float *p = arow + (int64_t)c * heads;
      if (valid == nullptr || valid[t * k + c] >= 0) *p = exp2_hw((*p - S.m) * kLog2e) * inv;
    }
  }
}

template <bool POW2>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void fanout_tattn_bwd_kernel(
    const float *__restrict__ grad_out, const float *__restrict__ q, int64_t ld_q,
    const float *__restrict__ key, const float *__restrict__ val, int64_t ld_kv,
    const int32_t *__restrict__ valid, const float *__restrict__ alpha, int64_t n_t, int32_t k,
    int32_t heads, int32_t d4, int32_t g, int32_t lg, float scale, float *__restrict__ gq,
    float *__restrict__ gskip, int64_t ld_gq, float *__restrict__ gk, float *__restrict__ gv,
    int64_t ld_gkv) {
  const HeadLane L = head_lane(lg, d4, g);
  const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lg;
  const bool live = t < n_t;
  const bool act = live && L.col;
  const int64_t D = (int64_t)d4 * 4;
  const float4 gg = act ? ld4(grad_out + t * D + 4 * L.sub) : f4_zero();
  const float4 qv = act ? ld4(q + t * ld_q + 4 * L.sub) : f4_zero();
  const float *arow = alpha + (t * k) * heads + L.h;  // read for valid slots of live targets only
  // pass 1: S = Σ_m alpha_m dalpha_m, children in slot order
  double S = 0.0;
  for (int c0 = 0; c0 < k; c0 += kHeadBatch) {
    float al[kHeadBatch];
    float4 v[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      const bool ok = live && c0 + u < k && (valid == nullptr || valid[t * k + c0 + u] >= 0);
      al[u] = ok ? arow[(int64_t)(c0 + u) * heads] : 0.f;
      v[u] = (act && ok) ? ld4(val + (t * k + c0 + u) * ld_kv + 4 * L.sub) : f4_zero();
    }
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u)
      S = fma((double)al[u], (double)head_sum<POW2>(f4_dot_fma(gg, v[u]), g, L.hb), S);
  }
  // pass 2: ds_j, ∂v_j, ∂k_j and this lane's columns of ∂q
  float4 gqa = f4_zero();
  for (int c0 = 0; c0 < k; c0 += kHeadBatch) {
    float al[kHeadBatch];
    float4 v[kHeadBatch], kr[kHeadBatch];
    bool ok[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      ok[u] = live && c0 + u < k && (valid == nullptr || valid[t * k + c0 + u] >= 0);
      al[u] = ok[u] ? arow[(int64_t)(c0 + u) * heads] : 0.f;
      const int64_t off = (t * k + c0 + u) * ld_kv + 4 * L.sub;
      v[u] = (act && ok[u]) ? ld4(val + off) : f4_zero();
      kr[u] = (act && ok[u]) ? ld4(key + off) : f4_zero();
    }
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      const float da = head_sum<POW2>(f4_dot_fma(gg, v[u]), g, L.hb);
      const float ds = ok[u] ? (float)((double)al[u] * ((double)da - S) * (double)scale) : 0.f;
      gqa = f4_fma(ds, kr[u], gqa);
      if (act && c0 + u < k) {
        const int64_t off = (t * k + c0 + u) * ld_gkv + 4 * L.sub;
        st4(gk + off, ok[u] ? f4_scale(ds, qv) : f4_zero());
        st4(gv + off, ok[u] ? f4_scale(al[u], gg) : f4_zero());
      }
    }
  }
  if (act) {
    st4(gq + t * ld_gq + 4 * L.sub, gqa);
    if (gskip != nullptr) st4(gskip + t * ld_gq + 4 * L.sub, gg);
  }
}

// One lane group per CSR row, walking its entries in batches of 8 with the
// forward's online softmax.  The logit of an entry is the head dot of the
// row's q with the entry's k row, so the lanes of a head exchange inside the
// loop: no lane leaves early (a dead group and the idle lanes of a live one
// run the loop with zeros), and the trip count is the row's, the same for
// every lane of the group — the only lanes a lane exchanges with.  Any
// degree; a hub row is a long loop of its group.
template <bool POW2>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void csr_tattn_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ q, const float *__restrict__ skip, int64_t ld_q,
    const float *__restrict__ key, const float *__restrict__ val, int64_t ld_kv, int64_t n_rows,
    int32_t d4, int32_t g, int32_t lg, float scale, float *__restrict__ out) {
  const HeadLane L = head_lane(lg, d4, g);
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lg;
  const bool live = r < n_rows;
  const bool act = live && L.col;
  const int64_t D = (int64_t)d4 * 4;
  const float4 qv = act ? ld4(q + r * ld_q + 4 * L.sub) : f4_zero();
  const int64_t beg = live ? rowptr[r] : 0, end = live ? rowptr[r + 1] : 0;
  SoftmaxState S = softmax_empty();
  for (int64_t j0 = beg; j0 < end; j0 += kHeadBatch) {
    bool ok[kHeadBatch];
    float4 kr[kHeadBatch], vr[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      const int32_t src = j0 + u < end ? col[j0 + u] : -1;
      ok[u] = src >= 0 && src < n_rows;
      const int64_t off = (int64_t)src * ld_kv + 4 * L.sub;
      kr[u] = (L.col && ok[u]) ? ld4(key + off) : f4_zero();
      vr[u] = (L.col && ok[u]) ? ld4(val + off) : f4_zero();
    }
    float s[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u)
      s[u] = head_sum<POW2>(f4_dot_fma(qv, kr[u]), g, L.hb) * scale;
    softmax_fold(S, s, vr, ok);
  }
  if (act)
    tat_store(S, skip != nullptr ? skip + r * ld_q + 4 * L.sub : nullptr, out + r * D + 4 * L.sub);
}

}  // namespace mirec

extern "C" int mirec_fanout_tattn(const float *query, const float *skip, int64_t ld_q,
                                  const float *key, const float *value, int64_t ld_kv,
                                  const int32_t *valid, int64_t n_targets, int32_t k,
                                  int32_t heads, int32_t ch, float scale, float *out,
                                  float *alpha, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(n_targets >= 0 && head_shape_ok(k, heads, ch) && scale == scale);
  const int D = heads * ch;
  MIREC_CHECK_ARG(head_stride_ok(ld_q, D) && head_stride_ok(ld_kv, D));
  if (n_targets == 0) return MIREC_OK;
  MIREC_CHECK_ARG(query && key && value && out);
  MIREC_CHECK_ARG(aligned16(query) && aligned16(skip) && aligned16(key) && aligned16(value) &&
                  aligned16(out) && aligned16(alpha));
  const int d4 = D / 4, g = ch / 4, lg = row_lg(d4);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MIREC_HEADROW_LAUNCH(fanout_tattn_kernel, head_blocks(n_targets, lg), g, st, query, skip, ld_q,
                       key, value, ld_kv, valid, n_targets, k, heads, d4, g, lg, scale, out,
                       alpha);
  return MIREC_OK;
}

extern "C" int mirec_fanout_tattn_bwd(const float *grad_out, const float *query, int64_t ld_q,
                                      const float *key, const float *value, int64_t ld_kv,
                                      const int32_t *valid, const float *alpha,
                                      int64_t n_targets, int32_t k, int32_t heads, int32_t ch,
                                      float scale, float *grad_query, float *grad_skip,
                                      int64_t ld_gq, float *grad_key, float *grad_value,
                                      int64_t ld_gkv, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(n_targets >= 0 && head_shape_ok(k, heads, ch) && scale == scale);
  const int D = heads * ch;
  MIREC_CHECK_ARG(head_stride_ok(ld_q, D) && head_stride_ok(ld_kv, D) &&
                  head_stride_ok(ld_gq, D) && head_stride_ok(ld_gkv, D));
  if (n_targets == 0) return MIREC_OK;
  MIREC_CHECK_ARG(grad_out && query && key && value && alpha && grad_query && grad_key &&
                  grad_value);
  MIREC_CHECK_ARG(aligned16(grad_out) && aligned16(query) && aligned16(key) &&
                  aligned16(value) && aligned16(alpha) && aligned16(grad_query) &&
                  aligned16(grad_skip) && aligned16(grad_key) && aligned16(grad_value));
  const int d4 = D / 4, g = ch / 4, lg = row_lg(d4);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MIREC_HEADROW_LAUNCH(fanout_tattn_bwd_kernel, head_blocks(n_targets, lg), g, st, grad_out,
                       query, ld_q, key, value, ld_kv, valid, alpha, n_targets, k, heads, d4, g,
                       lg, scale, grad_query, grad_skip, ld_gq, grad_key, grad_value, ld_gkv);
  return MIREC_OK;
}

extern "C" int mirec_csr_tattn(const mirec_csr_t *csr, const float *query, const float *skip,
                               int64_t ld_q, const float *key, const float *value, int64_t ld_kv,
                               int32_t heads, int32_t ch, float scale, float *out,
                               mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(csr && csr->n_rows >= 0 && head_shape_ok(1, heads, ch) && scale == scale);
  const int D = heads * ch;
  MIREC_CHECK_ARG(head_stride_ok(ld_q, D) && head_stride_ok(ld_kv, D));
  if (csr->n_rows == 0) return MIREC_OK;
  MIREC_CHECK_ARG(csr->rowptr && csr->col && query && key && value && out);
  MIREC_CHECK_ARG(aligned16(query) && aligned16(skip) && aligned16(key) && aligned16(value) &&
                  aligned16(out));
  const int d4 = D / 4, g = ch / 4, lg = row_lg(d4);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MIREC_HEADROW_LAUNCH(csr_tattn_kernel, head_blocks(csr->n_rows, lg), g, st, csr->rowptr,
                       csr->col, query, skip, ld_q, key, value, ld_kv, csr->n_rows, d4, g, lg,
                       scale, out);
  return MIREC_OK;
}
