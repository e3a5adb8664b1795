// Sampled-softmax loss / gradient seeds for LightGCN: K negatives per
// positive (the intent of model/lgcnssm.py's softmax_loss, restated: the
// reference body is unfinished; with K = 1 and temperature 1 this is
// model/lgcn.py:98-118, softplus(neg - pos)).
//
// Pair t = (u, p) with negatives n_0 .. n_{K-1}, temperature tau:
//   s+ = <out_u, out_p> / tau, s_k = <out_u, out_nk> / tau
//   m = max(s+, s_.), e+ = exp(s+ - m), e_k = exp(s_k - m), Z = e+ + sum_k e_k
//   term = logsumexp(s+, s_.) - s+   (log1p(sum_k e_k) when m == s+)
//   reg  = 1/2 (|e_u|^2 + |e_p|^2 + sum_k |e_nk|^2)          (ego rows)
//   coef[t, k] = grad_scale * e_k / (Z B tau), coef_pos[t] = their sum C_t
//   g_u[t] = sum_k coef[t, k] out_nk - C_t out_p   (k = 0 .. K-1, then p)
// Forward: one LPR-lane group per pair, three passes over the K rows (the
// maximum; the exponentials, their sum and the unnormalised g_u; the scaling
// of coef).  Loss: mirec_bpr_loss on (term, reg).
// Seeds: the (2 + K) B (node, occurrence) pairs — occurrence t the user,
// B + t the positive, 2B + tK + k negative k of pair t — are sorted stably;
// the head position q of every distinct node owns the node's gradient row
// and sums the node's occurrences in occurrence order, each one row times
// one coefficient:
//   user occurrence:   1 * g_u[t]
//   pos  occurrence:  -C_t * out_u
//   neg  occurrence:   coef[t, k] * out_u
// seed_p[q] = that / (L+1), seed_e[q] = decay * (#occurrences) e_node / B *
// grad_scale, slot[node] = q — bpr.hip's seed rows, for PropagationEngine's
// backward.  No float atomics: every sum has one fixed order.
#include <cmath>

#include "common.h"
#include "seedrun.h"

namespace mirec {

__global__ __launch_bounds__(256) void ssm_keys_kernel(const int32_t *__restrict__ users,
                                                       const int32_t *__restrict__ pos,
                                                       const int32_t *__restrict__ neg,
                                                       int64_t batch, int64_t n_neg,
                                                       int32_t n_users, int32_t *keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (2 + n_neg) * batch) return;
  keys[i] = i < batch ? users[i]
                      : i < 2 * batch ? n_users + pos[i - batch] : n_users + neg[i - 2 * batch];
}

template <int D>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void ssm_forward_kernel(
    const float *__restrict__ out, const float *__restrict__ emb, int64_t n_users, int64_t batch,
    int32_t n_neg, const int32_t *__restrict__ users, const int32_t *__restrict__ pos,
    const int32_t *__restrict__ neg, float temp, float grad_scale, float *coef, float *coef_pos,
    float *terms, float *reg, float *g_u, int32_t *keys, int32_t *vals) {
  constexpr int LPR = D / 4;
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int sub = lane % LPR;
  const int64_t t = ((int64_t)blockIdx.x * kSeedWaves + (threadIdx.x >> 6)) * G + lane / LPR;
  const bool live = t < batch;
  const int64_t tt = live ? t : 0;
  const int K = n_neg;
  const int64_t u = users[tt];
  const int64_t p = n_users + pos[tt];
  const int32_t *ng = neg + tt * K;
  const float4 ou = ld4(out + u * D + sub * 4);
  const float4 op = ld4(out + p * D + sub * 4);
  const float4 eu = ld4(emb + u * D + sub * 4);
  const float4 ep = ld4(emb + p * D + sub * 4);
  const float ps = group_sum<LPR>(f4_dot(ou, op)) / temp;
  // pass 1: the maximum, the reg term and the negatives' keys
  float m = ps;
  float rr = f4_dot(eu, eu) + f4_dot(ep, ep);
  const int64_t kbase = 2 * batch + t * K;
  for (int k = 0; k < K; ++k) {
    const int64_t n = n_users + ng[k];
    const float4 on = ld4(out + n * D + sub * 4);
    const float4 en = ld4(emb + n * D + sub * 4);
    const float s = group_sum<LPR>(f4_dot(ou, on)) / temp;
    m = fmaxf(m, s);
    rr += f4_dot(en, en);
    if (live && sub == (k & (LPR - 1))) {
      keys[kbase + k] = (int32_t)n;
      vals[kbase + k] = (int32_t)(kbase + k);
    }
  }
  const float r = group_sum<LPR>(rr);
  // pass 2: e_k = exp(s_k - m) (the dots again, bit for bit), their sum and
  // the unnormalised sum_k e_k out_nk, all in the order k = 0 .. K-1; lane
  // k mod LPR of the group keeps e_k in coef[t, k] for pass 3
  const float e_pos = expf(ps - m);
  float s_neg = 0.f;
  float4 acc = f4_zero();
  for (int k = 0; k < K; ++k) {
    const int64_t n = n_users + ng[k];
    const float4 on = ld4(out + n * D + sub * 4);
    const float s = group_sum<LPR>(f4_dot(ou, on)) / temp;
    const float e = expf(s - m);
    s_neg += e;
    acc = f4_fma(e, on, acc);
    if (live && sub == (k & (LPR - 1))) coef[t * K + k] = e;
  }
  const float z = e_pos + s_neg;
  float scale = 1.f / (z * (float)batch * temp);
  if (grad_scale != 1.f) scale *= grad_scale;
  const float cpos = scale * s_neg;
  if (!live) return;
  // pass 3: every lane scales the e_k it stored itself
  for (int k = sub; k < K; k += LPR) coef[t * K + k] = scale * coef[t * K + k];
  // g_u = sum_k c_k out_nk - C out_p
  float4 g = f4_scale(scale, acc);
  g = f4_fma(-cpos, op, g);
  st4(g_u + t * D + sub * 4, g);
  if (sub == 0) {
    terms[t] = m == ps ? log1pf(s_neg) : (m - ps) + logf(z);
    coef_pos[t] = cpos;
    reg[t] = 0.5f * r;
    keys[t] = (int32_t)u;
    keys[batch + t] = (int32_t)p;
    vals[t] = (int32_t)t;
    vals[batch + t] = (int32_t)(batch + t);
  }
}

// seedrun.h's run walk with this loss's decode: every occurrence is one source
// row times one coefficient, a row of `out` (index >= 0) or row t of g_u
// (stored as ~t).
template <int D>
__global__ __launch_bounds__(256) void ssm_seed_accum_kernel(
    const float *__restrict__ out, const float *__restrict__ emb, int64_t batch, int32_t n_neg,
    const int32_t *__restrict__ users, const float *__restrict__ coef,
    const float *__restrict__ coef_pos, const float *__restrict__ g_u,
    const int32_t *__restrict__ keys_sorted, const int32_t *__restrict__ vals_sorted, float decay,
    float grad_scale, float layer_div, float *seed_p, float *seed_e) {
  const int64_t n = (2 + (int64_t)n_neg) * batch;
  const int64_t q = seed_run_pos<D>();
  if (q >= n) return;
  const int32_t node = keys_sorted[q];
  if (q > 0 && keys_sorted[q - 1] == node) return;  // not the head of its run
  seed_run_walk<D, 1>(
      q, node, n, batch, emb, keys_sorted, vals_sorted, decay, grad_scale, layer_div, seed_p,
      seed_e,
      [=](int64_t occ, int32_t(&row)[1], float(&w)[1]) {
        if (occ < batch) {
          row[0] = ~(int32_t)occ;
          w[0] = 1.f;
        } else if (occ < 2 * batch) {
          row[0] = users[occ - batch];
          w[0] = -coef_pos[occ - batch];
        } else {
          const int64_t j = occ - 2 * batch;
          row[0] = users[j / n_neg];
          w[0] = coef[j];
        }
      },
      [=](int32_t r) { return r >= 0 ? out + (int64_t)r * D : g_u + (int64_t)(~r) * D; });
}

template <int D>
static int launch_ssm_forward(const float *out, const float *emb, int64_t n_users, int64_t batch,
                              int32_t n_neg, const int32_t *users, const int32_t *pos,
                              const int32_t *neg, float temp, float grad_scale, float *coef,
                              float *coef_pos, float *terms, float *reg, float *g_u,
                              int32_t *keys, int32_t *vals, hipStream_t st) {
  constexpr int G = 64 / (D / 4);
  const int64_t per_block = (int64_t)kSeedWaves * G;
  const int64_t blocks = (batch + per_block - 1) / per_block;
  hipLaunchKernelGGL((ssm_forward_kernel<D>), dim3(blocks), dim3(256), 0, st, out, emb, n_users,
                     batch, n_neg, users, pos, neg, temp, grad_scale, coef, coef_pos, terms, reg,
                     g_u, keys, vals);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

// (2 + n_neg) * batch as a count of int32-indexed pairs, or false
static bool ssm_pairs(int64_t batch, int32_t n_neg, int64_t *n) {
  if (batch <= 0 || n_neg < 1 || batch >= INT32_MAX) return false;
  const int64_t t = (2 + (int64_t)n_neg) * batch;
  if (t >= INT32_MAX) return false;
  *n = t;
  return true;
}

}  // namespace mirec

extern "C" int mirec_ssm_keys(const int32_t *users, const int32_t *pos, const int32_t *neg,
                              int64_t batch, int32_t n_neg, int64_t n_users, int32_t *keys,
                              mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(users && pos && neg && keys);
  int64_t n = 0;
  MIREC_CHECK_ARG(ssm_pairs(batch, n_neg, &n) && n_users > 0 && n_users < INT32_MAX);
  hipLaunchKernelGGL(ssm_keys_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), users, pos, neg, batch,
                     (int64_t)n_neg, (int32_t)n_users, keys);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

extern "C" int mirec_ssm_forward(const float *out, const float *emb, int64_t n_nodes,
                                 int64_t n_users, int32_t dim, int64_t batch, int32_t n_neg,
                                 const int32_t *users, const int32_t *pos, const int32_t *neg,
                                 float temp, float grad_scale, float *coef, float *coef_pos,
                                 float *terms, float *reg, float *g_u, int32_t *keys,
                                 int32_t *vals, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(out && emb && users && pos && neg && coef && coef_pos && terms && reg && g_u &&
                  keys && vals);
  int64_t n = 0;
  MIREC_CHECK_ARG(ssm_pairs(batch, n_neg, &n));
  MIREC_CHECK_ARG(n_users > 0 && n_nodes > n_users && n_nodes < INT32_MAX);
  MIREC_CHECK_ARG(std::isfinite(temp) && temp > 0.f);
  if (!dim_supported(dim)) return MIREC_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (dim) {
#define C(DD) \
  case DD:    \
    return launch_ssm_forward<DD>(out, emb, n_users, batch, n_neg, users, pos, neg, temp, grad_scale, coef, coef_pos, terms, reg, g_u, keys, vals, st);
    C(4) C(8) C(16) C(32) C(64) C(128) C(256)
#undef C
  }
  return MIREC_ERR_ARG;
}

extern "C" int mirec_ssm_seed_workspace(int64_t batch, int32_t n_neg, int64_t n_nodes,
                                        size_t *bytes) {
  using namespace mirec;
  int64_t n = 0;
  MIREC_CHECK_ARG(bytes != nullptr && n_nodes > 0 && ssm_pairs(batch, n_neg, &n));
  size_t tb = 0;
  return seed_ws_layout(n, n_nodes, &tb, bytes);
}

extern "C" int mirec_ssm_seed(const float *out, const float *emb, int64_t n_nodes, int64_t n_users,
                              int32_t dim, int64_t batch, int32_t n_neg, const int32_t *users,
                              const float *coef, const float *coef_pos, const float *g_u,
                              const int32_t *keys, const int32_t *vals, float decay,
                              float grad_scale, int32_t n_layers, int32_t *slot, float *seed_p,
                              float *seed_e, int32_t *keys_sorted, void *workspace,
                              size_t workspace_bytes, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(out && emb && users && coef && coef_pos && g_u && keys && vals && slot &&
                  seed_p && seed_e && keys_sorted && workspace);
  int64_t n = 0;
  MIREC_CHECK_ARG(ssm_pairs(batch, n_neg, &n));
  MIREC_CHECK_ARG(n_layers >= 0 && n_users > 0 && n_nodes > n_users && n_nodes < INT32_MAX);
  if (!dim_supported(dim)) return MIREC_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int32_t *vals_sorted = nullptr;
  int rc = seed_sort_heads(keys, vals, n, n_nodes, workspace, workspace_bytes, keys_sorted,
                           &vals_sorted, slot, st);
  if (rc != MIREC_OK) return rc;
  const float layer_div = (float)(n_layers + 1);
  switch (dim) {
#define C(DD) \
  case DD:    \
    return launch_seed_accum<DD>(ssm_seed_accum_kernel<DD>, n, st, out, emb, batch, n_neg, users, coef, coef_pos, g_u, keys_sorted, vals_sorted, decay, grad_scale, layer_div, seed_p, seed_e);
    C(4) C(8) C(16) C(32) C(64) C(128) C(256)
#undef C
  }
  return MIREC_ERR_ARG;
}
