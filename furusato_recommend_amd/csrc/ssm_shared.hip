// Sampled-softmax loss / gradient seeds for LightGCN with ONE set of M
// negatives per batch, shared by all B pairs (ssm.hip is the
// per-pair form, K negatives each).
//
// Pairs (u_t, p_t), t < B; shared item ids n_0 .. n_{M-1} (drawn with
// replacement: a repeated id counts twice everywhere); temperature tau:
//   mask[t, j] = 1 iff n_j is a training positive of u_t or n_j == p_t
//                (mirec_ssm_shared_mask, sampler.hip)
//   s+_t = <out_u, out_p> / tau, s_tj = <out_u, out_nj> / tau
//   m = max(s+, unmasked s_t.), e+ = exp(s+ - m), e_j = exp(s_tj - m) (0 when
//   masked), Z = e+ + sum_j e_j
//   terms[t] = logsumexp - s+   (log1p(sum_j e_j) when m == s+)
//   coef[t, j] = grad_scale * e_j / (Z B tau), coef_pos[t] = their sum C_t
//   g[t]     = sum_j coef[t, j] out_nj - C_t out_p        (user rows)
//   g[B + j] = sum_t coef[t, j] out_u_t                   (shared rows)
//   reg[t] = 1/2 (|e_u|^2 + |e_p|^2), reg_shared[j] = 1/2 |e_nj|^2
// Three launches, the B x M block `coef` carried between them in memory:
//   scores  coef[t, j] = s_tj: 64 x 64 tiles through LDS, every dot product
//           one fmaf chain d = 0 .. D-1
//   rows    one wave per pair: the maximum, the exponentials and their sum
//           (lane l sums j = l, l + 64, .. in that order, then the xor tree
//           over the 64 lanes), the scaling; one wave per shared slot: its reg
//           term and key
//   g       [B, M] x [M, D] and its transpose [M, B] x [B, D] in one launch:
//           tiles through LDS, every element one fmaf chain k = 0 .. M-1
//           (B-1), then the positive's term
// Each output element has one summation order that depends on (B, M, D)
// alone, never on a tile's position: a pair's terms and weights are the same
// bits in any batch.  No float atomics.
// Seeds: the 2B + M (node, occurrence) pairs — occurrence t the user of pair
// t, B + t its positive, 2B + j shared slot j — sorted stably; the head q of
// every distinct node sums its occurrences in occurrence order:
//   user occurrence:    1 * g[t]
//   pos  occurrence:   -C_t * out_u
//   shared occurrence:  1 * g[B + j]
// seed_p[q] = that / (L+1), seed_e[q] = decay * (#occurrences) e_node / B *
// grad_scale, slot[node] = q: ssm.hip's seed rows.
#include <cmath>

#include "common.h"
#include "seedrun.h"

namespace mirec {

constexpr int kShTile = 64;  // scores: pairs x slots per workgroup
constexpr int kShUnroll = 8;  // rows: elements per lane and round

__global__ __launch_bounds__(256) void ssh_keys_kernel(const int32_t *__restrict__ users,
                                                       const int32_t *__restrict__ pos,
                                                       const int32_t *__restrict__ shared,
                                                       int64_t batch, int64_t m, int32_t n_users,
                                                       int32_t *keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * batch + m) return;
  keys[i] = i < batch ? users[i]
                      : i < 2 * batch ? n_users + pos[i - batch] : n_users + shared[i - 2 * batch];
}

// coef[t, j] = <out_u_t, out_nj> / temp.  Thread (ty, tx) owns pairs
// t0 + 4 ty .. + 3 and slots j0 + 4 tx .. + 3; the operands pass through LDS
// KC columns at a time, stored [k][row] so that a thread's four rows are one
// 16-byte read.
template <int D>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void ssh_scores_kernel(
    const float *__restrict__ out, int64_t n_users, int64_t batch, int64_t m,
    const int32_t *__restrict__ users, const int32_t *__restrict__ shared, float temp,
    float *__restrict__ coef) {
  constexpr int KC = D < 32 ? D : 32;
  constexpr int T = kShTile;
  __shared__ __attribute__((aligned(16))) float as[KC][T];
  __shared__ __attribute__((aligned(16))) float bs[KC][T];
  __shared__ int64_t arow[T];
  __shared__ int64_t brow[T];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t t0 = (int64_t)blockIdx.y * T, j0 = (int64_t)blockIdx.x * T;
  if (tid < T) {
    const int64_t t = t0 + tid;
    arow[tid] = t < batch ? (int64_t)users[t] : -1;
  } else if (tid < 2 * T) {
    const int64_t j = j0 + tid - T;
    brow[tid - T] = j < m ? n_users + (int64_t)shared[j] : -1;
  }
  __syncthreads();
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  for (int k0 = 0; k0 < D; k0 += KC) {
    for (int i = tid; i < T * (KC / 4); i += 256) {
      const int row = i % T, kq = i / T;
      const int64_t ra = arow[row], rb = brow[row];
      const float4 a = ra >= 0 ? ld4(out + ra * D + k0 + kq * 4) : f4_zero();
      const float4 b = rb >= 0 ? ld4(out + rb * D + k0 + kq * 4) : f4_zero();
      as[kq * 4 + 0][row] = a.x, as[kq * 4 + 1][row] = a.y;
      as[kq * 4 + 2][row] = a.z, as[kq * 4 + 3][row] = a.w;
      bs[kq * 4 + 0][row] = b.x, bs[kq * 4 + 1][row] = b.y;
      bs[kq * 4 + 2][row] = b.z, bs[kq * 4 + 3][row] = b.w;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < KC; ++k) {
      const float4 a = ld4(&as[k][ty * 4]);
      const float4 b = ld4(&bs[k][tx * 4]);
      const float av[4] = {a.x, a.y, a.z, a.w};
      const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(av[r], bv[c], acc[r][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t t = t0 + ty * 4 + r;
    if (t >= batch) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t j = j0 + tx * 4 + c;
      if (j < m) coef[t * m + j] = acc[r][c] / temp;
    }
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v = fmaxf(v, __shfl_xor(v, s));
  return v;
}

// One wave per item i: i < B is pair i (its row of scores in `coef` becomes
// its row of coefficients), B + j is shared slot j (reg term, key, value).
template <int D>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void ssh_rows_kernel(
    const float *__restrict__ out, const float *__restrict__ emb, int64_t n_users, int64_t batch,
    int64_t m, const int32_t *__restrict__ users, const int32_t *__restrict__ pos,
    const int32_t *__restrict__ shared, const uint8_t *__restrict__ mask, float temp,
    float grad_scale, float *coef, float *coef_pos, float *terms, float *reg, float *reg_shared,
    int32_t *keys, int32_t *vals) {
  constexpr int LPR = D / 4;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kSeedWaves + (threadIdx.x >> 6);
  if (i >= batch + m) return;
  const bool has = lane < LPR;
  if (i >= batch) {
    const int64_t j = i - batch;
    const int64_t n = n_users + shared[j];
    const float4 e = has ? ld4(emb + n * D + lane * 4) : f4_zero();
    const float r = wave_sum(f4_dot(e, e));
    if (lane == 0) {
      reg_shared[j] = 0.5f * r;
      keys[2 * batch + j] = (int32_t)n;
      vals[2 * batch + j] = (int32_t)(2 * batch + j);
    }
    return;
  }
  const int64_t t = i;
  const int64_t u = users[t];
  const int64_t p = n_users + pos[t];
  float dot = 0.f, rr = 0.f;
  if (has) {
    const float4 ou = ld4(out + u * D + lane * 4);
    const float4 op = ld4(out + p * D + lane * 4);
    const float4 eu = ld4(emb + u * D + lane * 4);
    const float4 ep = ld4(emb + p * D + lane * 4);
    dot = f4_dot(ou, op);
    rr = f4_dot(eu, eu) + f4_dot(ep, ep);
  }
  const float ps = wave_sum(dot) / temp;
  const float r = wave_sum(rr);
  float *row = coef + t * m;
  const uint8_t *mk = mask + t * m;
  // (both passes take kShUnroll elements per lane and round, all loads of a
  // round issued before their use; the order of a lane's sum stays j = l,
  // l + 64, ..)
  // pass 1: the maximum over the positive and the unmasked candidates
  float mx = ps;
  for (int64_t j0 = lane; j0 < m; j0 += 64 * kShUnroll) {
    float v[kShUnroll];
    uint8_t k[kShUnroll];
#pragma unroll
    for (int q = 0; q < kShUnroll; ++q) {
      const int64_t j = j0 + 64 * q;
      k[q] = j < m ? mk[j] : (uint8_t)1;
      v[q] = j < m ? row[j] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < kShUnroll; ++q)
      if (!k[q]) mx = fmaxf(mx, v[q]);
  }
  mx = wave_max(mx);
  // pass 2: e_j (exactly 0 when masked) and their sum
  float part = 0.f;
  for (int64_t j0 = lane; j0 < m; j0 += 64 * kShUnroll) {
    float v[kShUnroll];
    uint8_t k[kShUnroll];
#pragma unroll
    for (int q = 0; q < kShUnroll; ++q) {
      const int64_t j = j0 + 64 * q;
      k[q] = j < m ? mk[j] : (uint8_t)1;
      v[q] = j < m ? row[j] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < kShUnroll; ++q) {
      const int64_t j = j0 + 64 * q;
      if (j < m) {
        const float e = k[q] ? 0.f : expf(v[q] - mx);
        row[j] = e;
        part += e;
      }
    }
  }
  const float s_neg = wave_sum(part);
  const float e_pos = expf(ps - mx);
  const float z = e_pos + s_neg;
  float scale = 1.f / (z * (float)batch * temp);
  if (grad_scale != 1.f) scale *= grad_scale;
  // pass 3: every lane scales the e_j it stored itself
  for (int64_t j = lane; j < m; j += 64) row[j] = scale * row[j];
  if (lane == 0) {
    terms[t] = mx == ps ? log1pf(s_neg) : (mx - ps) + logf(z);
    coef_pos[t] = scale * s_neg;
    reg[t] = 0.5f * r;
    keys[t] = (int32_t)u;
    keys[batch + t] = (int32_t)p;
    vals[t] = (int32_t)t;
    vals[batch + t] = (int32_t)(batch + t);
  }
}

// g[r, :] = sum_k w(r, k) out[src(k), :], k = 0 .. n_k - 1 in that order (one
// fmaf chain per element).  Workgroups below nb_user own user rows: w(r, k) =
// coef[r, k], src(k) = shared slot k, n_k = M, then - coef_pos[r] out_p.  The
// others own shared rows: w(r, k) = coef[k, r], src(k) = user of pair k, n_k
// = B.  One launch for both, so that the two chains of n_k / KC dependent
// rounds run side by side; a workgroup owns 2 RT rows x TC columns, a thread
// 2 rows x 4 columns, and the operands of round i + 1 (and the row ids of
// round i + 2) are fetched into registers while round i is computed from LDS.
template <int D>
__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void ssh_g_kernel(
    const float *__restrict__ out, int64_t n_users, int64_t batch, int64_t m,
    const int32_t *__restrict__ users, const int32_t *__restrict__ pos,
    const int32_t *__restrict__ shared, const float *__restrict__ coef,
    const float *__restrict__ coef_pos, int nb_user, float *__restrict__ g) {
  constexpr int TC = D < 64 ? D : 64;
  constexpr int CT = TC / 4;
  constexpr int RT = 256 / CT;
  constexpr int TR = 2 * RT;
  constexpr int KC = TR > 128 ? 16 : 32;
  constexpr int NW = KC * TR / 256;          // coefficients fetched per thread and round
  constexpr int NX = (KC * CT + 255) / 256;  // float4 of rows per thread and round
  __shared__ float ws[KC][TR + 1];
  __shared__ __attribute__((aligned(16))) float xs[KC][TC];
  const int tid = threadIdx.x;
  const int tx = tid % CT, ty = tid / CT;
  const bool trans = (int)blockIdx.x >= nb_user;
  const int64_t n_r = trans ? m : batch, n_k = trans ? batch : m;
  const int64_t r0 = (int64_t)(trans ? blockIdx.x - nb_user : blockIdx.x) * TR;
  const int c0 = blockIdx.y * TC;
  const int32_t *__restrict__ idx = trans ? users : shared;  // the rows summed over
  const int64_t idx_off = trans ? 0 : n_users;
  float wreg[NW];
  float4 xreg[NX];
  int32_t srcn[NX];  // ids of the rows of the round after the next (clamped: always valid)
  float4 acc[2] = {f4_zero(), f4_zero()};
  // round k0 (from 0 on): registers -> LDS, fetch round k0 + KC, compute; the
  // round at -KC only fetches
  for (int64_t k0 = -KC; k0 < n_k; k0 += KC) {
    if (k0 >= 0) {
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        const int i = tid + q * 256;
        const int kk = trans ? i / TR : i % KC, rr = trans ? i % TR : i / KC;
        ws[kk][rr] = (r0 + rr < n_r && k0 + kk < n_k) ? wreg[q] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < NX; ++q) {
        const int i = tid + q * 256;
        if (i < KC * CT)
          st4(&xs[i / CT][(i % CT) * 4], k0 + i / CT < n_k ? xreg[q] : f4_zero());
      }
      __syncthreads();
    }
    if (k0 + KC < n_k) {
      const int64_t kn = k0 + KC;
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        const int i = tid + q * 256;
        // coef[k, r] (trans): consecutive r are adjacent; coef[r, k]: consecutive k
        const int kk = trans ? i / TR : i % KC, rr = trans ? i % TR : i / KC;
        const int64_t r = r0 + rr, k = kn + kk;
        // (every load below is unconditional, on a clamped address, and its
        // value is not looked at before the next round moves it to LDS: a
        // branch around a load, or a select on its value, makes the wave
        // wait for the loads in flight before it computes)
        const bool ok = r < n_r && k < n_k;
        wreg[q] = coef[ok ? (trans ? k * m + r : r * m + k) : 0];
      }
      // the rows' ids were loaded a round earlier (the first round's here),
      // so that a row load never waits for its id inside the loop
      if (k0 < 0) {
#pragma unroll
        for (int q = 0; q < NX; ++q) {
          const int i = tid + q * 256;
          const int64_t k = kn + i / CT;
          srcn[q] = idx[k < n_k ? k : n_k - 1];
        }
      }
#pragma unroll
      for (int q = 0; q < NX; ++q) {
        const int cq = (tid + q * 256) % CT;
        xreg[q] = ld4(out + (idx_off + srcn[q]) * D + c0 + cq * 4);
      }
#pragma unroll
      for (int q = 0; q < NX; ++q) {
        const int i = tid + q * 256;
        const int64_t k = kn + KC + i / CT;
        srcn[q] = idx[k < n_k ? k : n_k - 1];
      }
    }
    if (k0 >= 0) {
#pragma unroll
      for (int kk = 0; kk < KC; ++kk) {
        const float4 x = ld4(&xs[kk][tx * 4]);
        const float w0 = ws[kk][ty * 2], w1 = ws[kk][ty * 2 + 1];
        acc[0] = f4_fma(w0, x, acc[0]);
        acc[1] = f4_fma(w1, x, acc[1]);
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int64_t r = r0 + ty * 2 + q;
    if (r >= n_r) continue;
    float4 v = acc[q];
    if (!trans) {
      const int64_t p = n_users + pos[r];
      v = f4_fma(-coef_pos[r], ld4(out + p * D + c0 + tx * 4), v);
    }
    st4(g + ((trans ? batch : 0) + r) * D + c0 + tx * 4, v);
  }
}

// Single workgroup, fixed partition and tree (bpr.hip's loss kernel with the
// shared rows' reg terms as a third sum).
__global__ __launch_bounds__(1024) void ssh_loss_kernel(const float *terms, const float *reg,
                                                        const float *reg_shared, int64_t batch,
                                                        int64_t m, float decay, float *loss_out,
                                                        float *loss_accum) {
  __shared__ float s_t[1024];
  __shared__ float s_r[1024];
  __shared__ float s_s[1024];
  float a = 0.f, b = 0.f, c = 0.f;
  for (int64_t i = threadIdx.x; i < batch; i += 1024) {
    a += terms[i];
    b += reg[i];
  }
  for (int64_t j = threadIdx.x; j < m; j += 1024) c += reg_shared[j];
  s_t[threadIdx.x] = a;
  s_r[threadIdx.x] = b;
  s_s[threadIdx.x] = c;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      s_t[threadIdx.x] += s_t[threadIdx.x + s];
      s_r[threadIdx.x] += s_r[threadIdx.x + s];
      s_s[threadIdx.x] += s_s[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float fb = (float)batch;
    const float loss = s_t[0] / fb + decay * ((s_r[0] + s_s[0]) / fb);
    loss_out[0] = loss;
    if (loss_accum != nullptr) loss_accum[0] += loss;
  }
}

// seedrun.h's run walk with this loss's decode: every occurrence is one source
// row times one coefficient, a row of `out` (index >= 0) or row r of g
// (stored as ~r).
template <int D>
__global__ __launch_bounds__(256) void ssh_seed_accum_kernel(
    const float *__restrict__ out, const float *__restrict__ emb, int64_t batch, int64_t m,
    const int32_t *__restrict__ users, const float *__restrict__ coef_pos,
    const float *__restrict__ g, const int32_t *__restrict__ keys_sorted,
    const int32_t *__restrict__ vals_sorted, float decay, float grad_scale, float layer_div,
    float *seed_p, float *seed_e) {
  const int64_t n = 2 * batch + m;
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
          row[0] = ~(int32_t)(occ - batch);  // g[B + j], j = occ - 2B
          w[0] = 1.f;
        }
      },
      [=](int32_t r) { return r >= 0 ? out + (int64_t)r * D : g + (int64_t)(~r) * D; });
}

// batch, m >= 1 with B M and 2B + M below 2^31; *n = 2B + M
static bool ssh_shape(int64_t batch, int64_t m, int64_t *n) {
  if (batch < 1 || m < 1 || batch >= INT32_MAX || m >= INT32_MAX) return false;
  if (batch * m >= INT32_MAX || 2 * batch + m >= INT32_MAX) return false;
  *n = 2 * batch + m;
  return true;
}

template <int D>
static int launch_ssh_forward(const float *out, const float *emb, int64_t n_users, int64_t batch,
                              int64_t m, const int32_t *users, const int32_t *pos,
                              const int32_t *shared, const uint8_t *mask, float temp,
                              float grad_scale, float *coef, float *coef_pos, float *terms,
                              float *reg, float *reg_shared, float *g, int32_t *keys,
                              int32_t *vals, hipStream_t st) {
  const dim3 sg((unsigned)((m + kShTile - 1) / kShTile), (unsigned)((batch + kShTile - 1) / kShTile));
  hipLaunchKernelGGL((ssh_scores_kernel<D>), sg, dim3(256), 0, st, out, n_users, batch, m, users,
                     shared, temp, coef);
  MIREC_LAUNCH_CHECK();
  const dim3 rg((unsigned)((batch + m + kSeedWaves - 1) / kSeedWaves));
  hipLaunchKernelGGL((ssh_rows_kernel<D>), rg, dim3(256), 0, st, out, emb, n_users, batch, m,
                     users, pos, shared, mask, temp, grad_scale, coef, coef_pos, terms, reg,
                     reg_shared, keys, vals);
  MIREC_LAUNCH_CHECK();
  constexpr int TC = D < 64 ? D : 64;
  constexpr int TR = 2 * (256 / (TC / 4));
  const int nb_user = (int)((batch + TR - 1) / TR), nb_shared = (int)((m + TR - 1) / TR);
  hipLaunchKernelGGL((ssh_g_kernel<D>), dim3((unsigned)(nb_user + nb_shared), D / TC), dim3(256),
                     0, st, out, n_users, batch, m, users, pos, shared, coef, coef_pos, nb_user,
                     g);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

}  // namespace mirec

extern "C" int mirec_ssm_shared_keys(const int32_t *users, const int32_t *pos,
                                     const int32_t *shared, int64_t batch, int64_t m,
                                     int64_t n_users, int32_t *keys, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(users && pos && shared && keys);
  int64_t n = 0;
  MIREC_CHECK_ARG(ssh_shape(batch, m, &n) && n_users > 0 && n_users < INT32_MAX);
  hipLaunchKernelGGL(ssh_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), users, pos, shared, batch, m,
                     (int32_t)n_users, keys);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

extern "C" int mirec_ssm_shared_forward(const float *out, const float *emb, int64_t n_nodes,
                                        int64_t n_users, int32_t dim, int64_t batch, int64_t m,
                                        const int32_t *users, const int32_t *pos,
                                        const int32_t *shared, const uint8_t *mask, float temp,
                                        float grad_scale, float *coef, float *coef_pos,
                                        float *terms, float *reg, float *reg_shared, float *g,
                                        int32_t *keys, int32_t *vals, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(out && emb && users && pos && shared && mask && coef && coef_pos && terms &&
                  reg && reg_shared && g && keys && vals);
  int64_t n = 0;
  MIREC_CHECK_ARG(ssh_shape(batch, m, &n));
  MIREC_CHECK_ARG(n_users > 0 && n_nodes > n_users && n_nodes < INT32_MAX);
  MIREC_CHECK_ARG(std::isfinite(temp) && temp > 0.f);
  if (!dim_supported(dim)) return MIREC_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (dim) {
#define C(DD) \
  case DD:    \
    return launch_ssh_forward<DD>(out, emb, n_users, batch, m, users, pos, shared, mask, temp, grad_scale, coef, coef_pos, terms, reg, reg_shared, g, keys, vals, st);
    C(4) C(8) C(16) C(32) C(64) C(128) C(256)
#undef C
  }
  return MIREC_ERR_ARG;
}

extern "C" int mirec_ssm_shared_loss(const float *terms, const float *reg,
                                     const float *reg_shared, int64_t batch, int64_t m,
                                     float decay, float *loss_out, float *loss_accum,
                                     mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(terms && reg && reg_shared && loss_out && batch >= 1 && m >= 1);
  hipLaunchKernelGGL(ssh_loss_kernel, dim3(1), dim3(1024), 0,
                     reinterpret_cast<hipStream_t>(stream), terms, reg, reg_shared, batch, m,
                     decay, loss_out, loss_accum);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

extern "C" int mirec_ssm_shared_seed_workspace(int64_t batch, int64_t m, int64_t n_nodes,
                                               size_t *bytes) {
  using namespace mirec;
  int64_t n = 0;
  MIREC_CHECK_ARG(bytes != nullptr && n_nodes > 0 && ssh_shape(batch, m, &n));
  size_t tb = 0;
  return seed_ws_layout(n, n_nodes, &tb, bytes);
}

extern "C" int mirec_ssm_shared_seed(const float *out, const float *emb, int64_t n_nodes,
                                     int64_t n_users, int32_t dim, int64_t batch, int64_t m,
                                     const int32_t *users, const float *coef_pos, const float *g,
                                     const int32_t *keys, const int32_t *vals, float decay,
                                     float grad_scale, int32_t n_layers, int32_t *slot,
                                     float *seed_p, float *seed_e, int32_t *keys_sorted,
                                     void *workspace, size_t workspace_bytes,
                                     mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(out && emb && users && coef_pos && g && keys && vals && slot && seed_p &&
                  seed_e && keys_sorted && workspace);
  int64_t n = 0;
  MIREC_CHECK_ARG(ssh_shape(batch, m, &n));
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
    return launch_seed_accum<DD>(ssh_seed_accum_kernel<DD>, n, st, out, emb, batch, m, users, coef_pos, g, keys_sorted, vals_sorted, decay, grad_scale, layer_div, seed_p, seed_e);
    C(4) C(8) C(16) C(32) C(64) C(128) C(256)
#undef C
  }
  return MIREC_ERR_ARG;
}
