// LightSAGE hops on gfx950 (model/lightsage.py:274-290): no weights, each hop
// is x_t <- x_t + mean_c dropout(x_c) on the fixed-fanout tree of sage.hip.
//
//   mirec_fanout_resmean_gather  out[t] = row(self_ids[t]) + mean over valid c
//                                of dropout(table[child_ids[t*k + c]]): layer
//                                0, self and child rows read from the table by
//                                id, nothing materialised
//   mirec_fanout_resmean         the same on materialised rows (layers >= 1)
//   mirec_fanout_resmean_bwd     grad_self[t] = grad_out[t]; grad_child[t*k+c]
//                                = mask * scale * grad_out[t] / cnt_t (0 for an
//                                invalid slot); plain stores
// Layer 0's backward is three row groups of the sorted table gradient
// (tablegrad.hip).  The dropout mask is the counter hash of common.h at
// element index (t*k + c)*dim + col, recomputed in the backward.
#include "common.h"

namespace mirec {

// one thread per (target, float4 column), fanout_mean_kernel's shape.  GATHER:
// self row = table[self_ids[t]] (0 for an id < 0), child rows =
// table[valid[child]], xs = xc = table; else self row = xs[t], child rows =
// xc[child].  The mean is the sum in child order divided by cnt (the same
// arithmetic in both forms: they agree bitwise on xc = table[ids]), then the
// self row is added.
template <bool GATHER>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void fanout_resmean_kernel(
    const float *__restrict__ xs, const int32_t *__restrict__ self_ids,
    const float *__restrict__ xc, const int32_t *__restrict__ valid, int64_t n_targets, int32_t k,
    int32_t d4, uint64_t key, uint32_t thresh, float scale, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_targets * d4) return;
  const int64_t t = i / d4;
  const int64_t c4 = i - t * d4;
  const int64_t d = (int64_t)d4 * 4;
  // the self row's load goes out with the first batch of child rows
  int64_t srow = t;
  if (GATHER) srow = (int64_t)self_ids[t];
  float4 self = f4_zero();
  float4 acc = f4_zero();
  int cnt = 0;
  constexpr int kBatch = 8;
  for (int c0 = 0; c0 < k; c0 += kBatch) {
    int32_t vid[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u)
      vid[u] = (c0 + u < k && valid != nullptr) ? valid[t * k + c0 + u] : 0;
    if (c0 == 0 && srow >= 0) self = ld4(xs + srow * d + c4 * 4);
    float4 v[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int64_t child = t * k + c0 + u;
      const bool ok = c0 + u < k && vid[u] >= 0;
      const int64_t row = GATHER ? (int64_t)vid[u] : child;
      v[u] = ok ? ld4(xc + row * d + c4 * 4) : f4_zero();
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int64_t child = t * k + c0 + u;
      if (c0 + u < k && vid[u] >= 0) {
        ++cnt;
        float4 w = v[u];
        if (thresh != 0u) w = drop4(w, key, (uint64_t)(child * d + c4 * 4), thresh, scale);
        acc = f4_add(acc, w);
      }
    }
  }
  st4(out + i * 4, cnt > 0 ? f4_add(f4_div(acc, (float)cnt), self) : self);
}

// one thread per (slot, float4 column), slot = t*(k+1) + j: j = 0 copies
// grad_out[t] to grad_self[t], j = c + 1 writes child c's row.  cnt as in
// fanout_mean_bwd_kernel: the d4 lanes of a slot read the k flags of their
// target d4 at a time and count them by ballot (d4 a power of two <= 64, so
// the lane groups are aligned inside the wave and whole groups leave together
// at the end of the grid), else every lane loops over the flags.
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void fanout_resmean_bwd_kernel(
    const float *__restrict__ grad_out, const int32_t *__restrict__ valid, int64_t n_targets,
    int32_t k, int32_t d4, uint64_t key, uint32_t thresh, float scale,
    float *__restrict__ grad_self, float *__restrict__ grad_child) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (slot, float4)
  const int64_t k1 = (int64_t)k + 1;
  if (i >= n_targets * k1 * d4) return;
  const int64_t slot = i / d4;
  const int64_t c4 = i - slot * d4;
  const int64_t t = slot / k1;
  const int j = (int)(slot - t * k1);
  const int64_t d = (int64_t)d4 * 4;
  const float4 g = ld4(grad_out + t * d + c4 * 4);
  int cnt = k;
  if (valid != nullptr) {
    cnt = 0;
    if (d4 <= 64 && (d4 & (d4 - 1)) == 0) {
      const int lane = threadIdx.x & 63;
      const int gbase = lane & ~(d4 - 1);
      const unsigned long long gmask = (d4 == 64 ? ~0ull : ((1ull << d4) - 1ull)) << gbase;
      for (int j0 = 0; j0 < k; j0 += d4) {
        const int jj = j0 + (int)c4;
        cnt += __popcll(__ballot(jj < k && valid[t * k + jj] >= 0) & gmask);
      }
    } else {
      for (int c = 0; c < k; ++c) cnt += valid[t * k + c] >= 0 ? 1 : 0;
    }
  }
  if (j == 0) {
    st4(grad_self + t * d + c4 * 4, g);
    return;
  }
  const int64_t child = t * k + (j - 1);
  float4 r = f4_zero();
  if (valid == nullptr || valid[child] >= 0) {
    r = f4_div(g, (float)cnt);
    if (thresh != 0u) r = drop4(r, key, (uint64_t)(child * d + c4 * 4), thresh, scale);
  }
  st4(grad_child + child * d + c4 * 4, r);
}

}  // namespace mirec

extern "C" int mirec_fanout_resmean_gather(const float *table, const int32_t *self_ids,
                                           const int32_t *child_ids, int64_t n_targets, int32_t k,
                                           int32_t dim, float dropout_p, uint64_t seed, float *out,
                                           mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(table && self_ids && child_ids && out && n_targets >= 0 && k > 0 && dim > 0 &&
                  dim % 4 == 0);
  MIREC_CHECK_ARG(((uintptr_t)table & 15u) == 0 && ((uintptr_t)out & 15u) == 0);
  uint64_t key;
  uint32_t thresh;
  float scale;
  MIREC_CHECK_ARG(dropout_params(dropout_p, seed, &key, &thresh, &scale));
  if (n_targets == 0) return MIREC_OK;
  const int64_t tot = n_targets * (dim / 4);
  MIREC_CHECK_ARG((tot + 255) / 256 <= INT32_MAX);
  hipLaunchKernelGGL(fanout_resmean_kernel<true>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), table, self_ids, table, child_ids,
                     n_targets, k, dim / 4, key, thresh, scale, out);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

extern "C" int mirec_fanout_resmean(const float *x_self, const float *x_child, const int32_t *valid,
                                    int64_t n_targets, int32_t k, int32_t dim, float dropout_p,
                                    uint64_t seed, float *out, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(x_self && x_child && out && n_targets >= 0 && k > 0 && dim > 0 && dim % 4 == 0);
  MIREC_CHECK_ARG(((uintptr_t)x_self & 15u) == 0 && ((uintptr_t)x_child & 15u) == 0 &&
                  ((uintptr_t)out & 15u) == 0);
  uint64_t key;
  uint32_t thresh;
  float scale;
  MIREC_CHECK_ARG(dropout_params(dropout_p, seed, &key, &thresh, &scale));
  if (n_targets == 0) return MIREC_OK;
  const int64_t tot = n_targets * (dim / 4);
  MIREC_CHECK_ARG((tot + 255) / 256 <= INT32_MAX);
  hipLaunchKernelGGL(fanout_resmean_kernel<false>, dim3((unsigned)((tot + 255) / 256)), dim3(256),
                     0, reinterpret_cast<hipStream_t>(stream), x_self, nullptr, x_child, valid,
                     n_targets, k, dim / 4, key, thresh, scale, out);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

extern "C" int mirec_fanout_resmean_bwd(const float *grad_out, const int32_t *valid,
                                        int64_t n_targets, int32_t k, int32_t dim, float dropout_p,
                                        uint64_t seed, float *grad_self, float *grad_child,
                                        mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(grad_out && grad_self && grad_child && n_targets >= 0 && k > 0 && dim > 0 &&
                  dim % 4 == 0);
  MIREC_CHECK_ARG(((uintptr_t)grad_out & 15u) == 0 && ((uintptr_t)grad_self & 15u) == 0 &&
                  ((uintptr_t)grad_child & 15u) == 0);
  uint64_t key;
  uint32_t thresh;
  float scale;
  MIREC_CHECK_ARG(dropout_params(dropout_p, seed, &key, &thresh, &scale));
  if (n_targets == 0) return MIREC_OK;
  const int64_t tot = n_targets * ((int64_t)k + 1) * (dim / 4);
  MIREC_CHECK_ARG((tot + 255) / 256 <= INT32_MAX);
  hipLaunchKernelGGL(fanout_resmean_bwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), grad_out, valid, n_targets, k, dim / 4,
                     key, thresh, scale, grad_self, grad_child);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}
