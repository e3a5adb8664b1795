// Graph-attention hop (PyG GATConv, concat=True, add_self_loops=True, no
// attention dropout; model/gnn.py:196-206) on the fixed-fanout tree of
// sage.hip and on the full CSR graph.  z = x Wᵀ is projected by the MFMA GEMM
// before these kernels; per target i and head h, over the slots j in S(i) ∪
// {i} (children with valid >= 0, a repeated id once per slot, then the self
// slot, always present):
//   s_j = <z_j,h, att_src_h> + <z_i,h, att_dst_h>,  e_j = leaky_relu(s_j)
//   alpha_j = softmax_j e_j,  out_i,h = Σ_j alpha_j z_j,h (+ bias)
//
//   mirec_fanout_gat      forward on the tree; keeps alpha if asked
//   mirec_fanout_gat_bwd  ∂z_child, ∂z_self, ∂att_src, ∂att_dst from alpha
//   mirec_csr_gat         forward over every CSR row (full-graph inference)
//
// Layout: headrow.h's (shared with tattn.hip) — one group of lanes per
// target, a float4 column per lane, a head's dot summed inside the lanes that
// own it.
//
// Forward: every child row is read once.  The running (max, sum, acc) of an
// online softmax starts from the self slot (max = e_self, sum = 1, acc =
// z_self), so the maximum is finite from the start and a target without a
// valid child leaves z_self untouched (no division).  Children come in
// batches of 8: flags, then 8 rows in flight, one rescale per batch — the
// step headrow.h has as softmax_fold, written out in the two forward kernels
// here because they measured slower with the call.  When
// alpha is kept the raw e_j go to the alpha buffer and the lane that wrote
// them normalises them in place once the final (max, sum) is known.
// Exponentials are exp2 of the log2(e)-scaled argument (common.h).
//
// Backward: two passes over a target's child rows (the second one a cache
// hit): pass 1 sums Σ_m alpha_m dalpha_m, pass 2 recomputes dalpha_j and s_j
// (dots over the row it reads anyway) and writes ∂z_j.  The per-head scalars
// S = Σ alpha dalpha, de_j = alpha_j (dalpha_j - S), ds_j and Σ_j ds_j are
// kept in double: with a saturated softmax (one alpha ~ 1) Σ_j de_j is S (1 -
// Σ alpha), seven orders below its terms, and ∂z_self / ∂att_dst are built
// from it; both passes form the same f32 dalpha_j, so it cancels exactly.
// A handful of f64 operations per child row and lane, beside the row's load.
// ∂att_src / ∂att_dst
// are sums over all targets: every lane accumulates its columns over the
// targets its block walks (a grid-stride loop, the grid a function of the
// shape alone), the block adds its groups in group order into `work`, and a
// final launch adds the blocks' partials in block order: no float atomics,
// bitwise the same from run to run.
#include "headrow.h"

namespace mirec {

constexpr int kGatMaxBlocks = 1024;  // partial sums of the backward

__device__ __forceinline__ float leaky(float s, float slope) { return s > 0.f ? s : slope * s; }

template <bool POW2>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void fanout_gat_kernel(
    const float *__restrict__ zc, const float *__restrict__ zs, const int32_t *__restrict__ valid,
    const float *__restrict__ att_src, const float *__restrict__ att_dst,
    const float *__restrict__ bias, int64_t n_t, int32_t k, int32_t heads, int32_t d4, int32_t g,
    int32_t lg, float slope, float *__restrict__ out, float *alpha) {
  const HeadLane L = head_lane(lg, d4, g);
  const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lg;
  const bool live = t < n_t;
  const bool act = live && L.col;
  const int64_t D = (int64_t)d4 * 4;
  const float4 a_s = L.col ? ld4(att_src + 4 * L.sub) : f4_zero();
  const float4 a_d = L.col ? ld4(att_dst + 4 * L.sub) : f4_zero();
  const float4 zself = act ? ld4(zs + t * D + 4 * L.sub) : f4_zero();
  const float sd = head_sum<POW2>(f4_dot_fma(zself, a_d), g, L.hb);
  const float e_self = leaky(head_sum<POW2>(f4_dot_fma(zself, a_s), g, L.hb) + sd, slope);
  float m = e_self, l = 1.f;
  float4 acc = zself;
  bool any = false;
  const bool keep_a = alpha != nullptr && live && L.lead;
  float *arow = alpha != nullptr && live ? alpha + (t * (k + 1)) * heads + L.h : nullptr;
  for (int c0 = 0; c0 < k; c0 += kHeadBatch) {
    bool ok[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u)
      ok[u] = live && c0 + u < k && (valid == nullptr || valid[t * k + c0 + u] >= 0);
    float4 v[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u)
      v[u] = (act && ok[u]) ? ld4(zc + (t * k + c0 + u) * D + 4 * L.sub) : f4_zero();
    // headrow.h's softmax_fold, inline: with the fold as a call (and the
    // alpha store beside it) two of the three measured shapes ran slower
    // 
    float e[kHeadBatch];
    float mb = m;
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      e[u] = leaky(head_sum<POW2>(f4_dot_fma(v[u], a_s), g, L.hb) + sd, slope);
      if (ok[u]) mb = fmaxf(mb, e[u]);
    }
    const float r = exp2_hw((m - mb) * kLog2e);  // 1 when the maximum stays
    l *= r;
    acc = f4_scale(r, acc);
    m = mb;
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      if (ok[u]) {
        const float p = exp2_hw((e[u] - mb) * kLog2e);
        l += p;
        acc = f4_fma(p, v[u], acc);
        any = true;
      }
      if (keep_a && c0 + u < k) arow[(int64_t)(c0 + u) * heads] = ok[u] ? e[u] : 0.f;
    }
  }
  const float inv = 1.f / l;
  if (act) {
    float4 o = any ? f4_scale(inv, acc) : zself;
    if (bias != nullptr) o = f4_add(o, ld4(bias + 4 * L.sub));
    st4(out + t * D + 4 * L.sub, o);
  }
  if (keep_a) {
    // the lane that wrote the raw e_j turns them into alpha_j
    for (int c = 0; c < k; ++c) {
      float *p = arow + (int64_t)c * heads;
      if (valid == nullptr || valid[t * k + c] >= 0) *p = exp2_hw((*p - m) * kLog2e) * inv;
    }
    arow[(int64_t)k * heads] = exp2_hw((e_self - m) * kLog2e) * inv;
  }
}

// work[(b * 2 + which) * D + col]: block b's sums of ds_j z_j (which = 0) and
// (Σ_j ds_j) z_i (which = 1) over the targets it walked.
template <bool POW2>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void fanout_gat_bwd_kernel(
    const float *__restrict__ grad_out, const float *__restrict__ zc,
    const float *__restrict__ zs, const int32_t *__restrict__ valid,
    const float *__restrict__ att_src, const float *__restrict__ att_dst,
    const float *__restrict__ alpha, int64_t n_t, int32_t k, int32_t heads, int32_t d4,
    int32_t g, int32_t lg, float slope, float *__restrict__ gzc, float *__restrict__ gzs,
    float *__restrict__ work) {
  __shared__ float4 red[2][256];
  const HeadLane L = head_lane(lg, d4, g);
  const int gpb = 256 >> lg;  // targets per block and round
  const int64_t D = (int64_t)d4 * 4;
  const float4 a_s = L.col ? ld4(att_src + 4 * L.sub) : f4_zero();
  const float4 a_d = L.col ? ld4(att_dst + 4 * L.sub) : f4_zero();
  float4 gsrc = f4_zero(), gdst = f4_zero();
  for (int64_t t0 = (int64_t)blockIdx.x * gpb; t0 < n_t; t0 += (int64_t)gridDim.x * gpb) {
    const int64_t t = t0 + (threadIdx.x >> lg);
    const bool live = t < n_t;
    const bool act = live && L.col;
    const float4 gg = act ? ld4(grad_out + t * D + 4 * L.sub) : f4_zero();
    const float4 zself = act ? ld4(zs + t * D + 4 * L.sub) : f4_zero();
    const float *arow = alpha + (t * (k + 1)) * heads + L.h;
    const float sd = head_sum<POW2>(f4_dot_fma(zself, a_d), g, L.hb);
    const float s_self = head_sum<POW2>(f4_dot_fma(zself, a_s), g, L.hb) + sd;
    const float da_self = head_sum<POW2>(f4_dot_fma(gg, zself), g, L.hb);
    const float al_self = live ? arow[(int64_t)k * heads] : 0.f;
    // pass 1: S = Σ_m alpha_m dalpha_m (children in slot order, then self)
    double S = 0.0;
    for (int c0 = 0; c0 < k; c0 += kHeadBatch) {
      float al[kHeadBatch];
      float4 v[kHeadBatch];
#pragma unroll
      for (int u = 0; u < kHeadBatch; ++u) {
        const bool ok = live && c0 + u < k && (valid == nullptr || valid[t * k + c0 + u] >= 0);
        al[u] = ok ? arow[(int64_t)(c0 + u) * heads] : 0.f;
        v[u] = (act && ok) ? ld4(zc + (t * k + c0 + u) * D + 4 * L.sub) : f4_zero();
      }
#pragma unroll
      for (int u = 0; u < kHeadBatch; ++u)
        S = fma((double)al[u], (double)head_sum<POW2>(f4_dot_fma(gg, v[u]), g, L.hb), S);
    }
    S = fma((double)al_self, (double)da_self, S);
    // pass 2: ds_j, ∂z_j, and this lane's columns of the parameter sums
    double sum_dsd = 0.0;
    for (int c0 = 0; c0 < k; c0 += kHeadBatch) {
      float al[kHeadBatch];
      float4 v[kHeadBatch];
      bool ok[kHeadBatch];
#pragma unroll
      for (int u = 0; u < kHeadBatch; ++u) {
        ok[u] = live && c0 + u < k && (valid == nullptr || valid[t * k + c0 + u] >= 0);
        al[u] = ok[u] ? arow[(int64_t)(c0 + u) * heads] : 0.f;
        v[u] = (act && ok[u]) ? ld4(zc + (t * k + c0 + u) * D + 4 * L.sub) : f4_zero();
      }
#pragma unroll
      for (int u = 0; u < kHeadBatch; ++u) {
        const float da = head_sum<POW2>(f4_dot_fma(gg, v[u]), g, L.hb);
        const float s = head_sum<POW2>(f4_dot_fma(v[u], a_s), g, L.hb) + sd;
        const double dsd =
            ok[u] ? (double)al[u] * ((double)da - S) * (s > 0.f ? 1.0 : (double)slope) : 0.0;
        sum_dsd += dsd;
        const float ds = (float)dsd;
        gsrc = f4_fma(ds, v[u], gsrc);
        if (act && c0 + u < k)
          st4(gzc + (t * k + c0 + u) * D + 4 * L.sub,
              ok[u] ? f4_fma(ds, a_s, f4_scale(al[u], gg)) : f4_zero());
      }
    }
    const double ds_selfd =
        (double)al_self * ((double)da_self - S) * (s_self > 0.f ? 1.0 : (double)slope);
    const float ds_self = (float)ds_selfd;
    const float sum_ds = (float)(sum_dsd + ds_selfd);
    gsrc = f4_fma(ds_self, zself, gsrc);
    gdst = f4_fma(sum_ds, zself, gdst);
    if (act)
      st4(gzs + t * D + 4 * L.sub,
          f4_fma(sum_ds, a_d, f4_fma(ds_self, a_s, f4_scale(al_self, gg))));
  }
  red[0][threadIdx.x] = gsrc;
  red[1][threadIdx.x] = gdst;
  __syncthreads();
  if ((int)threadIdx.x < 2 * d4) {  // 2 d4 <= 128 threads: one (which, column) each
    const int which = (int)threadIdx.x >= d4 ? 1 : 0;
    const int c = (int)threadIdx.x - which * d4;
    float4 s = f4_zero();
    for (int q = 0; q < gpb; ++q) s = f4_add(s, red[which][(q << lg) + c]);
    st4(work + ((int64_t)blockIdx.x * 2 + which) * D + 4 * c, s);
  }
}

// out[which][col] = Σ_b work[(b * 2 + which) * D + col] in block order: one
// wave per output float, lane l adding blocks l, l + 64, ..., then the
// butterfly.
__global__ __launch_bounds__(256) void gat_param_sum_kernel(const float *__restrict__ work,
                                                            int32_t n_blocks, int32_t D,
                                                            float *__restrict__ g_src,
                                                            float *__restrict__ g_dst) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);  // (which, col), e < 2 D
  if (e >= 2 * D) return;
  const int which = e >= D ? 1 : 0, c = e - which * D;
  float s = 0.f;
  for (int b = lane; b < n_blocks; b += 64) s += work[((int64_t)b * 2 + which) * D + c];
  s = group_sum<64>(s);
  if (lane == 0) (which ? g_dst : g_src)[c] = s;
}

// logits[r * 2H + h] = <z_r,h, att_src_h>, logits[r * 2H + H + h] = <z_r,h,
// att_dst_h>
template <bool POW2>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void csr_gat_logits_kernel(
    const float *__restrict__ z, const float *__restrict__ att_src,
    const float *__restrict__ att_dst, int64_t n_rows, int32_t heads, int32_t d4, int32_t g,
    int32_t lg, float *__restrict__ logits) {
  const HeadLane L = head_lane(lg, d4, g);
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lg;
  const bool act = r < n_rows && L.col;
  const float4 x = act ? ld4(z + r * d4 * 4 + 4 * L.sub) : f4_zero();
  const float4 a_s = L.col ? ld4(att_src + 4 * L.sub) : f4_zero();
  const float4 a_d = L.col ? ld4(att_dst + 4 * L.sub) : f4_zero();
  const float ss = head_sum<POW2>(f4_dot_fma(x, a_s), g, L.hb);
  const float sd = head_sum<POW2>(f4_dot_fma(x, a_d), g, L.hb);
  if (r < n_rows && L.lead) {
    logits[r * 2 * heads + L.h] = ss;
    logits[r * 2 * heads + heads + L.h] = sd;
  }
}

// One lane group per CSR row, walking its entries in batches of 8 with the
// online softmax of the forward (started from the self loop); the logits are
// read, so no lane exchange: every lane of a head repeats its head's scalar
// work.  Any degree; a long row is a long loop of its group.
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void csr_gat_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ z, const float *__restrict__ logits,
    const float *__restrict__ bias, int64_t n_rows, int32_t heads, int32_t d4, int32_t g,
    int32_t lg, float slope, float *__restrict__ out) {
  const HeadLane L = head_lane(lg, d4, g);
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lg;
  if (r >= n_rows || !L.col) return;  // no lane exchange below
  const int64_t D = (int64_t)d4 * 4;
  const int H2 = 2 * heads;
  const float sd = logits[r * H2 + heads + L.h];
  const float4 zself = ld4(z + r * D + 4 * L.sub);
  float m = leaky(logits[r * H2 + L.h] + sd, slope), l = 1.f;
  float4 acc = zself;
  const int64_t beg = rowptr[r], end = rowptr[r + 1];
  for (int64_t j0 = beg; j0 < end; j0 += kHeadBatch) {
    int32_t src[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) src[u] = j0 + u < end ? col[j0 + u] : -1;
    float e[kHeadBatch];
    float4 v[kHeadBatch];
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      const bool ok = src[u] >= 0 && src[u] < n_rows;
      e[u] = ok ? logits[(int64_t)src[u] * H2 + L.h] : 0.f;
      v[u] = ok ? ld4(z + (int64_t)src[u] * D + 4 * L.sub) : f4_zero();
      if (!ok) src[u] = -1;
    }
    // headrow.h's softmax_fold, inline (the valid flag is src[u] >= 0): as a
    // call it measured slower
    float mb = m;
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      e[u] = leaky(e[u] + sd, slope);
      if (src[u] >= 0) mb = fmaxf(mb, e[u]);
    }
    const float rs = exp2_hw((m - mb) * kLog2e);
    l *= rs;
    acc = f4_scale(rs, acc);
    m = mb;
#pragma unroll
    for (int u = 0; u < kHeadBatch; ++u) {
      if (src[u] >= 0) {
        const float p = exp2_hw((e[u] - mb) * kLog2e);
        l += p;
        acc = f4_fma(p, v[u], acc);
      }
    }
  }
  float4 o = end > beg ? f4_scale(1.f / l, acc) : zself;
  if (bias != nullptr) o = f4_add(o, ld4(bias + 4 * L.sub));
  st4(out + r * D + 4 * L.sub, o);
}

static int gat_bwd_blocks(int64_t n_targets, int lg) {
  const int64_t b = head_blocks(n_targets, lg);
  return (int)(b < kGatMaxBlocks ? b : kGatMaxBlocks);
}

}  // namespace mirec

extern "C" int mirec_fanout_gat(const float *z_child, const float *z_self, const int32_t *valid,
                                const float *att_src, const float *att_dst, const float *bias,
                                int64_t n_targets, int32_t k, int32_t heads, int32_t ch,
                                float slope, float *out, float *alpha, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(n_targets >= 0 && head_shape_ok(k, heads, ch) && slope == slope);
  if (n_targets == 0) return MIREC_OK;
  MIREC_CHECK_ARG(z_child && z_self && att_src && att_dst && out);
  MIREC_CHECK_ARG(aligned16(z_child) && aligned16(z_self) && aligned16(att_src) &&
                  aligned16(att_dst) && aligned16(bias) && aligned16(out));
  const int d4 = heads * ch / 4, g = ch / 4, lg = row_lg(d4);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MIREC_HEADROW_LAUNCH(fanout_gat_kernel, head_blocks(n_targets, lg), g, st, z_child, z_self,
                       valid, att_src, att_dst, bias, n_targets, k, heads, d4, g, lg, slope, out,
                       alpha);
  return MIREC_OK;
}

extern "C" int64_t mirec_fanout_gat_bwd_work_floats(int64_t n_targets, int32_t k, int32_t heads,
                                                    int32_t ch) {
  using namespace mirec;
  if (n_targets < 0 || !head_shape_ok(k, heads, ch)) return -1;
  const int d4 = heads * ch / 4;
  return (int64_t)gat_bwd_blocks(n_targets, row_lg(d4)) * 2 * d4 * 4;
}

extern "C" int mirec_fanout_gat_bwd(const float *grad_out, const float *z_child,
                                    const float *z_self, const int32_t *valid,
                                    const float *att_src, const float *att_dst,
                                    const float *alpha, int64_t n_targets, int32_t k,
                                    int32_t heads, int32_t ch, float slope, float *grad_z_child,
                                    float *grad_z_self, float *grad_att_src, float *grad_att_dst,
                                    float *work, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(n_targets >= 0 && head_shape_ok(k, heads, ch) && slope == slope);
  MIREC_CHECK_ARG(grad_att_src && grad_att_dst);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int D = heads * ch, d4 = D / 4, g = ch / 4, lg = row_lg(d4);
  if (n_targets == 0) {
    MIREC_HIP(hipMemsetAsync(grad_att_src, 0, sizeof(float) * D, st));
    MIREC_HIP(hipMemsetAsync(grad_att_dst, 0, sizeof(float) * D, st));
    return MIREC_OK;
  }
  MIREC_CHECK_ARG(grad_out && z_child && z_self && att_src && att_dst && alpha && grad_z_child &&
                  grad_z_self && work);
  MIREC_CHECK_ARG(aligned16(grad_out) && aligned16(z_child) && aligned16(z_self) &&
                  aligned16(att_src) && aligned16(att_dst) && aligned16(grad_z_child) &&
                  aligned16(grad_z_self) && aligned16(work));
  const int blocks = gat_bwd_blocks(n_targets, lg);
  MIREC_HEADROW_LAUNCH(fanout_gat_bwd_kernel, blocks, g, st, grad_out, z_child, z_self, valid,
                       att_src, att_dst, alpha, n_targets, k, heads, d4, g, lg, slope,
                       grad_z_child, grad_z_self, work);
  hipLaunchKernelGGL(gat_param_sum_kernel, dim3((2 * D + 3) / 4), dim3(256), 0, st, work, blocks,
                     D, grad_att_src, grad_att_dst);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

extern "C" int mirec_csr_gat(const mirec_csr_t *csr, const float *z, const float *att_src,
                             const float *att_dst, const float *bias, int32_t heads, int32_t ch,
                             float slope, float *out, float *logits, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(csr && csr->n_rows >= 0 && head_shape_ok(1, heads, ch) && slope == slope);
  if (csr->n_rows == 0) return MIREC_OK;
  MIREC_CHECK_ARG(csr->rowptr && csr->col && z && att_src && att_dst && out && logits);
  MIREC_CHECK_ARG(aligned16(z) && aligned16(att_src) && aligned16(att_dst) && aligned16(bias) &&
                  aligned16(out));
  const int d4 = heads * ch / 4, g = ch / 4, lg = row_lg(d4);
  const int64_t blocks = head_blocks(csr->n_rows, lg);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MIREC_HEADROW_LAUNCH(csr_gat_logits_kernel, blocks, g, st, z, att_src, att_dst, csr->n_rows,
                       heads, d4, g, lg, logits);
  hipLaunchKernelGGL(csr_gat_kernel, dim3((unsigned)blocks), dim3(256), 0, st, csr->rowptr,
                     csr->col, z, logits, bias, csr->n_rows, heads, d4, g, lg, slope, out);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}
