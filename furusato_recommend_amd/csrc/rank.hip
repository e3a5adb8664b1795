// Streamed full-rank evaluation: for every held-out (user,
// item) pair the exact position of the item among the user's non-train
// items, as three integer counts over the scores s_j = <user, item j> —
// gt = #{s_j > s_t}, eq = #{s_j == s_t}, eq_lower = #{j < t, s_j == s_t} —
// so rank = 1 + gt + eq_lower is the item's place in mirec_score_topk's
// order (score descending, ties to the lower item id).  A count, not a
// selection: no candidate buffers, no sort, any cut-off k.
//
// The scores are the f32 MFMA chain of score_topk_kernel (topk.hip):
// v_mfma_f32_32x32x2_f32, lane (i, h) supplying column i's dims h·D/2 + s at
// step s = 0 .. D/2 - 1, accumulator from zero.  An output element of that
// chain depends on its own row, its own column and the step order only, so
// one (user row, item row) score is reproduced bit for bit by running the
// chain with the pair in column / row i and reading the diagonal
// (pair_score) — that is where a pair's threshold s_t and the scores of a
// user's train positives come from.
//
// Three launches on one stream:
//  1. rank_thr_kernel: pair -> user slot (binary search in tptr), the
//     threshold s_t, the counts zeroed.
//  2. rank_count_kernel: workgroup (64 pairs, one chunk of the items); a
//     pair's user row stays in registers as the B operand, item tiles of 32
//     stream through LDS (double-buffered); per score one compare and one
//     add, the j < t term only on equality; no mask test.  The chunks'
//     partial counts meet in integer atomics on the zeroed outputs (any
//     order gives the same integers).
//  3. rank_mask_kernel (csr given): one wave per pair walks the user's CSR
//     row, scores each distinct train positive through pair_score and takes
//     it out of the counts it entered in launch 2; a target that is itself a
//     train positive is flagged `masked`.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace mirec {
namespace {

constexpr int kRkPairs = 64;  // pairs per workgroup of the count kernel (2 waves of 32)
constexpr int kRkTile = 32;   // items per MFMA tile

__device__ __forceinline__ f32x16 mfma32x2(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// x of lane (lane ^ 32): v_permlane32_swap, each lane taking the half it lacks
__device__ __forceinline__ int swap_half(int x) {
  const auto r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
  return (int)((threadIdx.x & 32) ? r[0] : r[1]);
}

// <urow, irow> of the pair in column i, through the stream's chain: lane
// (i, h) feeds both operands' dims h·D/2 + s, so row i x column i of the
// product — accumulator register (i & 3) + 4 (i >> 3) of lane half
// (i >> 2) & 1 — is the pair's score; both lanes of the column get it.
// Every lane of the wave calls this with readable rows.
template <int D>
__device__ __forceinline__ float pair_score(const float *__restrict__ urow,
                                            const float *__restrict__ irow, int i, int h) {
  constexpr int KS = D / 2;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
  for (int s4 = 0; s4 < KS / 4; ++s4) {
    const float4 a = ld4(irow + h * KS + 4 * s4), b = ld4(urow + h * KS + 4 * s4);
    acc = mfma32x2(a.x, b.x, acc);
    acc = mfma32x2(a.y, b.y, acc);
    acc = mfma32x2(a.z, b.z, acc);
    acc = mfma32x2(a.w, b.w, acc);
  }
  const int r = (i & 3) + 4 * (i >> 3);
  float v = acc[0];
#pragma unroll
  for (int q = 1; q < 16; ++q) v = r == q ? acc[q] : v;
  const float o = __int_as_float(swap_half(__float_as_int(v)));
  return h == ((i >> 2) & 1) ? v : o;
}

template <int D>
__global__ __launch_bounds__(64) void rank_thr_kernel(
    const float *__restrict__ U, int64_t n_eval, const float *__restrict__ I, int64_t m_items,
    const int64_t *__restrict__ tptr, const int32_t *__restrict__ targets, int64_t n_targets,
    int32_t *__restrict__ pslot, float *__restrict__ score, int32_t *__restrict__ gt,
    int32_t *__restrict__ eq, int32_t *__restrict__ eql, uint8_t *__restrict__ masked) {
  const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
  const int64_t p = (int64_t)blockIdx.x * 32 + i;
  const bool ok = p < n_targets;
  // the slot r with tptr[r] <= p < tptr[r + 1] (slots without targets are
  // stepped over: the last r whose tptr[r] <= p)
  int64_t lo = 0, hi = n_eval - 1;
  if (ok) {
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (tptr[mid] <= p) lo = mid;
      else hi = mid - 1;
    }
  }
  const int64_t t = ok ? (int64_t)targets[p] : 0;
  const bool tok = t >= 0 && t < m_items;  // an id outside the items: flagged masked
  const float s = pair_score<D>(U + lo * D, I + (tok ? t : 0) * D, i, h);
  if (ok && h == 0) {
    pslot[p] = (int32_t)lo;
    score[p] = s;
    gt[p] = 0;
    eq[p] = 0;
    eql[p] = 0;
    masked[p] = tok ? 0 : 1;
  }
}

template <int D>
__global__ __launch_bounds__(128) void rank_count_kernel(
    const float *__restrict__ U, const float *__restrict__ I, int64_t m_items,
    const int32_t *__restrict__ pslot, const int32_t *__restrict__ targets,
    const float *__restrict__ score, int64_t n_targets, int64_t chunk, int32_t *__restrict__ gt,
    int32_t *__restrict__ eq, int32_t *__restrict__ eql) {
  constexpr int LD = D + 4;   // row stride: a read phase's 16 lanes hit distinct 4-bank groups
  constexpr int KS = D / 2;   // MFMA steps
  constexpr int kSI = kRkTile * LD;
  __shared__ __attribute__((aligned(16))) float sI[2][kSI];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int64_t p = (int64_t)blockIdx.x * kRkPairs + 32 * w + i;
  const bool ok = p < n_targets;
  const int64_t it0 = (int64_t)blockIdx.y * chunk;
  const int64_t it1 = min(m_items, it0 + chunk);
  const int64_t slot = ok ? pslot[p] : 0;
  const float thr = ok ? score[p] : INFINITY;
  const int tgt = ok ? targets[p] : -1;
  // the pair's user row as the B operand: ue[s] = U[slot][h D/2 + s]
  float ue[KS];
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4) {
    const float4 x = ok ? ld4(U + slot * D + h * KS + 4 * s4) : f4_zero();
    ue[4 * s4] = x.x, ue[4 * s4 + 1] = x.y, ue[4 * s4 + 2] = x.z, ue[4 * s4 + 3] = x.w;
  }
  // item tile loader: 32 rows x D floats, float4 per thread; rows past the
  // chunk are staged as zeros and never counted
  constexpr int PER = (kRkTile * D / 4 + 127) / 128;
  auto load = [&](int64_t base, float4 (&r)[PER]) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = t + 128 * q, row = e / (D / 4), c4 = e % (D / 4);
      r[q] = (e < kRkTile * D / 4 && base + row < it1) ? ld4(I + (base + row) * D + 4 * c4)
                                                        : f4_zero();
    }
  };
  auto stage = [&](int buf, const float4 (&r)[PER]) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = t + 128 * q, row = e / (D / 4), c4 = e % (D / 4);
      if (e >= kRkTile * D / 4) continue;
      st4(sI[buf] + row * LD + 4 * c4, r[q]);
    }
  };
  int cg = 0, ce = 0, cl = 0;
  float4 rg[PER];
  int cur = 0;
  if (it0 < it1) {
    load(it0, rg);
    stage(0, rg);
  }
  __syncthreads();
  for (int64_t base = it0; base < it1; base += kRkTile) {
    const bool more = base + kRkTile < it1;
    if (more) load(base + kRkTile, rg);  // in flight during the products
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float *arow = sI[cur] + i * LD + h * KS;
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      const float4 a = ld4(arow + 4 * s4);
      acc = mfma32x2(a.x, ue[4 * s4], acc);
      acc = mfma32x2(a.y, ue[4 * s4 + 1], acc);
      acc = mfma32x2(a.z, ue[4 * s4 + 2], acc);
      acc = mfma32x2(a.w, ue[4 * s4 + 3], acc);
    }
    // acc[r] = score of item base + 4 h + (r & 3) + 8 (r >> 2) for the pair
    const int ib = (int)base + 4 * h;
    unsigned ebits = 0u;
    if (base + kRkTile <= it1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        cg += acc[r] > thr ? 1 : 0;
        ebits |= (unsigned)(acc[r] == thr) << r;
      }
    } else {
      const int lim = (int)(it1 - base) - 4 * h;  // ragged last tile
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool in = (r & 3) + 8 * (r >> 2) < lim;
        cg += (in && acc[r] > thr) ? 1 : 0;
        ebits |= (unsigned)(in && acc[r] == thr) << r;
      }
    }
    if (ebits) {
      ce += __builtin_popcount(ebits);
#pragma unroll
      for (int r = 0; r < 16; ++r)
        cl += ((ebits >> r) & 1u) && ib + (r & 3) + 8 * (r >> 2) < tgt ? 1 : 0;
    }
    if (more) stage(cur ^ 1, rg);
    __syncthreads();  // the next tile staged; this tile's reads done
    cur ^= 1;
  }
  cg += swap_half(cg);
  ce += swap_half(ce);
  cl += swap_half(cl);
  if (ok && h == 0) {
    if (cg) atomicAdd(gt + p, cg);
    if (ce) atomicAdd(eq + p, ce);
    if (cl) atomicAdd(eql + p, cl);
  }
}

template <int D>
__global__ __launch_bounds__(64) void rank_mask_kernel(
    const float *__restrict__ U, const float *__restrict__ I, int64_t m_items,
    const int32_t *__restrict__ users, const int64_t *__restrict__ rowptr,
    const int32_t *__restrict__ col, const int32_t *__restrict__ sorted, int64_t n_sorted,
    int64_t n_users, const int32_t *__restrict__ pslot, const int32_t *__restrict__ targets,
    const float *__restrict__ score, int32_t *__restrict__ gt, int32_t *__restrict__ eq,
    int32_t *__restrict__ eql, uint8_t *__restrict__ masked) {
  const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
  const int64_t p = blockIdx.x;
  const int64_t slot = pslot[p];
  const int64_t u = users[slot];
  const float thr = score[p];
  const int64_t tgt = targets[p];
  const int64_t beg = rowptr[u], end = rowptr[u + 1];
  // distinct entries only (multi-edges repeat an item): in the sorted copy
  // of the row a repeat follows its twin, else the row's earlier entries
  // are scanned
  const int32_t *row = col + beg;
  const bool srt = sorted != nullptr && u < n_sorted;
  if (srt) row = sorted + (beg - rowptr[0]);
  const int64_t deg = end - beg;
  int above = 0, tie = 0, low = 0, self = 0;
  for (int64_t e0 = 0; e0 < deg; e0 += 32) {
    const int64_t e = e0 + i;
    bool valid = e < deg;
    int64_t q = 0;
    if (valid) {
      const int32_t node = row[e];
      q = (int64_t)node - n_users;
      valid = q >= 0 && q < m_items;
      if (valid) {
        if (srt) {
          valid = e == 0 || row[e - 1] != node;
        } else {
          for (int64_t f = 0; f < e; ++f) valid &= row[f] != node;
        }
      }
    }
    const float s = pair_score<D>(U + slot * D, I + (valid ? q : 0) * D, i, h);
    valid &= h == 0;
    above += __popcll(__ballot(valid && s > thr));
    tie += __popcll(__ballot(valid && s == thr));
    low += __popcll(__ballot(valid && s == thr && q < tgt));
    self += __popcll(__ballot(valid && q == tgt));
  }
  if (lane == 0) {
    if (above) gt[p] -= above;
    if (tie) eq[p] -= tie;
    if (low) eql[p] -= low;
    if (self) masked[p] = 1;
  }
}

// Workgroups of rank_count_kernel<D> resident on the chip at once, from the
// runtime, once per width.
template <int D>
int64_t rk_slots_of() {
  static int64_t slots = -1;
  if (slots < 0) {
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, rank_count_kernel<D>, 128, 0) !=
            hipSuccess)
      return 1024;
    slots = (int64_t)cus * std::max(per, 1);
  }
  return slots;
}

int64_t rk_slots(int D) {
  switch (D) {
    case 16: return rk_slots_of<16>();
    case 32: return rk_slots_of<32>();
    case 64: return rk_slots_of<64>();
    case 128: return rk_slots_of<128>();
    default: return rk_slots_of<256>();
  }
}

// Items per workgroup of the count kernel.  Chunks serve parallelism only
// (ids are 32-bit): as st_chunks of topk.hip, the chunk count that minimises
// rounds x (tiles per chunk + a chunk's fixed cost, ~4 tiles of prologue and
// atomics), at least 8 tiles per chunk, fewest chunks on a tie.
void rk_chunks(int64_t n_targets, int64_t m_items, int D, int64_t *chunk, int64_t *n_chunks) {
  const int64_t groups = (n_targets + kRkPairs - 1) / kRkPairs;
  const int64_t slots = std::max<int64_t>(1, rk_slots(D));
  const int64_t tiles_all = (m_items + kRkTile - 1) / kRkTile;
  const int64_t max_n = std::min<int64_t>(std::max<int64_t>(1, tiles_all / 8), 4096);
  int64_t best_n = 1, best_cost = -1;
  for (int64_t n = 1; n <= max_n; ++n) {
    const int64_t tiles = (tiles_all + n - 1) / n;
    const int64_t rounds = (groups * n + slots - 1) / slots;
    const int64_t cost = rounds * (tiles + 4);
    if (best_cost < 0 || cost < best_cost) {
      best_cost = cost;
      best_n = n;
    }
  }
  const int64_t c = (tiles_all + best_n - 1) / best_n * kRkTile;
  *chunk = c;
  *n_chunks = (m_items + c - 1) / c;
}

bool rk_dim(int d) { return d == 16 || d == 32 || d == 64 || d == 128 || d == 256; }

int64_t rk_tptr_bytes(int64_t n_eval) { return ((n_eval + 1) * 8 + 15) / 16 * 16; }

}  // namespace
}  // namespace mirec

extern "C" int64_t mirec_score_rank_workspace(int64_t n_eval, int64_t n_targets, int64_t m_items,
                                              int32_t dim) {
  using namespace mirec;
  if (n_eval < 0 || n_targets < 0 || n_targets >= INT32_MAX || m_items <= 0 ||
      m_items >= INT32_MAX || !rk_dim(dim))
    return -1;
  // the device copy of tptr, then the pairs' user slots
  return rk_tptr_bytes(n_eval) + n_targets * (int64_t)sizeof(int32_t);
}

extern "C" int mirec_score_rank(const float *user_emb, int64_t n_eval, const float *item_emb,
                                int64_t m_items, int32_t dim, const int32_t *users,
                                const int64_t *tptr, const int32_t *targets,
                                const mirec_csr_t *csr, int64_t n_users, float *score,
                                int32_t *gt, int32_t *eq, int32_t *eq_lower, uint8_t *masked,
                                void *ws, size_t ws_bytes, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(n_eval >= 0 && m_items > 0 && m_items < INT32_MAX && tptr != nullptr);
  MIREC_CHECK_ARG(rk_dim(dim));
  MIREC_CHECK_ARG(csr == nullptr || (users && csr->rowptr && csr->col));
  MIREC_CHECK_ARG(tptr[0] == 0);
  for (int64_t r = 0; r < n_eval; ++r) MIREC_CHECK_ARG(tptr[r] <= tptr[r + 1]);
  const int64_t n_targets = tptr[n_eval];
  MIREC_CHECK_ARG(n_targets < INT32_MAX);
  if (n_targets == 0) return MIREC_OK;  // nothing is read, nothing launched
  MIREC_CHECK_ARG(user_emb && item_emb && targets && score && gt && eq && eq_lower && masked &&
                  ws);
  MIREC_CHECK_ARG(((uintptr_t)user_emb | (uintptr_t)item_emb | (uintptr_t)ws) % 16 == 0);
  if ((int64_t)ws_bytes < mirec_score_rank_workspace(n_eval, n_targets, m_items, dim))
    return MIREC_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int64_t *d_tptr = static_cast<int64_t *>(ws);
  int32_t *pslot = reinterpret_cast<int32_t *>(static_cast<char *>(ws) + rk_tptr_bytes(n_eval));
  MIREC_HIP(hipMemcpyAsync(d_tptr, tptr, (size_t)(n_eval + 1) * sizeof(int64_t),
                           hipMemcpyHostToDevice, st));
  int64_t chunk, n_chunks;
  rk_chunks(n_targets, m_items, dim, &chunk, &n_chunks);
  const dim3 g_thr((unsigned)((n_targets + 31) / 32));
  const dim3 g_cnt((unsigned)((n_targets + kRkPairs - 1) / kRkPairs), (unsigned)n_chunks);
  const dim3 g_msk((unsigned)n_targets);
  const int64_t *rp = csr ? csr->rowptr : nullptr;
  const int32_t *cl = csr ? csr->col : nullptr;
  const int32_t *so = csr ? csr->col_sorted : nullptr;
  const int64_t ns = csr ? csr->n_sorted : 0;
#define MIREC_RK_CASE(DD)                                                                        \
  case DD:                                                                                       \
    hipLaunchKernelGGL((rank_thr_kernel<DD>), g_thr, dim3(64), 0, st, user_emb, n_eval,          \
                       item_emb, m_items, d_tptr, targets, n_targets, pslot, score, gt, eq,      \
                       eq_lower, masked);                                                        \
    hipLaunchKernelGGL((rank_count_kernel<DD>), g_cnt, dim3(128), 0, st, user_emb, item_emb,     \
                       m_items, pslot, targets, score, n_targets, chunk, gt, eq, eq_lower);      \
    if (csr != nullptr)                                                                          \
      hipLaunchKernelGGL((rank_mask_kernel<DD>), g_msk, dim3(64), 0, st, user_emb, item_emb,     \
                         m_items, users, rp, cl, so, ns, n_users, pslot, targets, score, gt, eq, \
                         eq_lower, masked);                                                      \
    break;
  switch (dim) {
    MIREC_RK_CASE(16)
    MIREC_RK_CASE(32)
    MIREC_RK_CASE(64)
    MIREC_RK_CASE(128)
    MIREC_RK_CASE(256)
  }
#undef MIREC_RK_CASE
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}
