// The seed pipeline shared by the LightGCN losses (bpr.hip, ssm.hip,
// ssm_shared.hip).  A loss hands over n (node, occurrence)
// pairs; the pipeline sorts them stably, publishes slot[node] = the head
// position q of the node's run, and the head of every run sums the run's
// occurrences in occurrence order:
//   seed_p[q] = sum / (L+1)
//   seed_e[q] = decay * (#occurrences) / B * grad_scale * emb[node]
// A loss supplies its keys, its n and the decode of one occurrence.  The host
// functions are defined once, in bpr.hip; the device side is templates, so
// every loss file instantiates its own accumulate kernel (the library is
// built without relocatable device code).
#pragma once

#include "common.h"

namespace mirec {

constexpr int kSeedWaves = 4;  // waves per 256-thread block of the row-group kernels

// Workspace of a sort of n pairs with keys below n_nodes: the sort's own
// temporary (*sort_bytes; smallsort.hip up to kSmallSortMax pairs, the device
// library's radix sort above it), then the sorted values, each block rounded
// up to 256 bytes (*total).
int seed_ws_layout(int64_t n, int64_t n_nodes, size_t *sort_bytes, size_t *total);

// MIREC_ERR_WORKSPACE unless ws holds seed_ws_layout's total; then the
// stable sort of (keys, vals) into keys_sorted and *vals_sorted (inside ws)
// and slot[node] = head position of the node's run, on stream st.
int seed_sort_heads(const int32_t *keys, const int32_t *vals, int64_t n, int64_t n_nodes,
                    void *ws, size_t ws_bytes, int32_t *keys_sorted, int32_t **vals_sorted,
                    int32_t *slot, hipStream_t st);

// The sorted position of this lane's LPR-lane group (one group per pair).
template <int D>
__device__ __forceinline__ int64_t seed_run_pos() {
  constexpr int LPR = D / 4;
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  return ((int64_t)blockIdx.x * kSeedWaves + (threadIdx.x >> 6)) * G + lane / LPR;
}

// The run of `node` from its head q, walked LPR entries per round: lane j
// decodes entry q0 + j — decode(occ, row, w) fills the entry's NSRC source
// rows and coefficients, a source past the first staying -1 when the entry
// has none — then the group loads the rows 8 at a time (row_of(index) is a
// row's pointer) and adds them in entry order, source 0 before source 1
// inside an entry: the serial walk's exact sequence of fmas (bitwise equal)
// without one dependent index chain per entry (a Zipf-popular item is
// hundreds of entries of a batch).  Then the two seed rows of q.
template <int D, int NSRC, class Decode, class RowOf>
__device__ __forceinline__ void seed_run_walk(
    int64_t q, int32_t node, int64_t n, int64_t batch, const float *__restrict__ emb,
    const int32_t *__restrict__ keys_sorted, const int32_t *__restrict__ vals_sorted, float decay,
    float grad_scale, float layer_div, float *seed_p, float *seed_e, Decode decode,
    RowOf row_of) {
  constexpr int LPR = D / 4;
  const int lane = threadIdx.x & 63;
  const int sub = lane % LPR;
  const int base = lane - sub;
  const unsigned long long low = LPR == 64 ? ~0ull : ((1ull << LPR) - 1ull);
  const unsigned long long gmask = low << base;
  float4 gp = f4_zero();
  int cnt = 0;
  for (int64_t q0 = q;; q0 += LPR) {
    const int64_t qj = q0 + sub;
    const bool in = qj < n && keys_sorted[qj] == node;
    int32_t row[NSRC];
    float w[NSRC];
#pragma unroll
    for (int s = 0; s < NSRC; ++s) row[s] = -1, w[s] = 0.f;
    if (in) decode((int64_t)vals_sorted[qj], row, w);
    const unsigned long long bal = (__ballot(in) & gmask) >> base;
    const int m = bal == low ? LPR : (int)__builtin_ctzll(~bal);
    for (int u0 = 0; u0 < m; u0 += 8) {
      float4 x[NSRC][8];
      float c[NSRC][8];
      bool has[NSRC][8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int src = base + ((u0 + u) & (LPR - 1));
        int32_t r[NSRC];
#pragma unroll
        for (int s = 0; s < NSRC; ++s) r[s] = __shfl(row[s], src);
#pragma unroll
        for (int s = 0; s < NSRC; ++s) c[s][u] = __shfl(w[s], src);
#pragma unroll
        for (int s = 0; s < NSRC; ++s) {
          has[s][u] = u0 + u < m && (s == 0 || r[s] >= 0);
          x[s][u] = has[s][u] ? ld4(row_of(r[s]) + sub * 4) : f4_zero();
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (u0 + u >= m) break;
#pragma unroll
        for (int s = 0; s < NSRC; ++s)
          if (s == 0 || has[s][u]) gp = f4_fma(c[s][u], x[s][u], gp);
      }
    }
    cnt += m;
    if (m < LPR) break;
  }
  const float4 e = ld4(emb + (int64_t)node * D + sub * 4);
  float re = decay * ((float)cnt / (float)batch);
  if (grad_scale != 1.f) re *= grad_scale;
  st4(seed_p + q * D + sub * 4, f4_div(gp, layer_div));
  st4(seed_e + q * D + sub * 4, f4_scale(re, e));
}

// One LPR-lane group per sorted pair, kSeedWaves waves per block.
template <int D, class Kernel, class... Args>
static int launch_seed_accum(Kernel kernel, int64_t n, hipStream_t st, Args... args) {
  constexpr int G = 64 / (D / 4);
  const int64_t per_block = (int64_t)kSeedWaves * G;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), 0, st,
                     args...);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

}  // namespace mirec
