// The layout and the online softmax shared by the head-grouped row kernels
// (gat.hip, tattn.hip).
//
// Layout.  A row of D = H·C floats is D/4 float4 columns; a target is owned
// by a group of LPT = 2^lg >= D/4 consecutive lanes (64 / LPT targets per
// wave, lanes past D/4 idle), lane `sub` holding columns 4 sub .. 4 sub + 3,
// all of head sub / (C/4) because C % 4 == 0.  A head's dot is summed inside
// the C/4 lanes that own it: an xor butterfly when C/4 is a power of two
// (the head groups are then aligned), else every lane adds its head's lanes
// in lane order — both fixed orders.  The kernels are templates on that
// choice (POW2) and MIREC_HEADROW_LAUNCH picks the instance.
#pragma once

#include <float.h>

#include "common.h"

namespace mirec {

constexpr int kHeadBatch = 8;  // (logit, value row) pairs in flight per lane

struct HeadLane {
  int sub;    // float4 column of this lane inside its target group
  int h;      // its head (0 for an idle lane)
  int hb;     // wave lane of the head's first lane
  bool col;   // sub < D/4
  bool lead;  // first lane of its head
};

__device__ __forceinline__ HeadLane head_lane(int lg, int d4, int g) {
  HeadLane L;
  const int lane = threadIdx.x & 63;
  L.sub = lane & ((1 << lg) - 1);
  L.col = L.sub < d4;
  L.h = L.col ? L.sub / g : 0;
  L.hb = (lane - L.sub) + L.h * g;
  L.lead = L.col && L.sub == L.h * g;
  return L;
}

// Sum of v over the g lanes of the caller's head (every lane that can reach
// the call calls it; idle lanes pass 0 and are read by nobody).
template <bool POW2>
__device__ __forceinline__ float head_sum(float v, int g, int hb) {
  if (POW2) {
    for (int m = 1; m < g; m <<= 1) v += __shfl_xor(v, m);
    return v;
  }
  float s = 0.f;
  for (int j = 0; j < g; ++j) s += __shfl(v, hb + j);
  return s;
}

// A lane's part of a head dot, fused.  Not common.h's f4_dot, which sums the
// four products without fma: the two round differently.
__device__ __forceinline__ float f4_dot_fma(float4 a, float4 b) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}

// The running state of one lane's online softmax and the step that folds a
// batch of up to 8 (logit, value row) pairs into it.  A softmax with a slot
// that is always present starts from it, {logit, 1, row, false}; one without
// starts from softmax_empty(): the running maximum is -FLT_MAX (a finite
// number: the first rescale is exp2 of a large negative argument, 0, times
// l = 0 and acc = 0, never inf - inf), and whether anything was folded is
// told by `any`, not by a division.
struct SoftmaxState {
  float m, l;
  float4 acc;
  bool any;  // a batch slot was folded in
};

__device__ __forceinline__ SoftmaxState softmax_empty() {
  return SoftmaxState{-FLT_MAX, 0.f, f4_zero(), false};
}

__device__ __forceinline__ void softmax_fold(SoftmaxState &S, const float (&s)[kHeadBatch],
                                             const float4 (&v)[kHeadBatch],
                                             const bool (&ok)[kHeadBatch]) {
  float mb = S.m;
#pragma unroll
  for (int u = 0; u < kHeadBatch; ++u)
    if (ok[u]) mb = fmaxf(mb, s[u]);
  // 1 when the maximum stays; 0 (times l = 0, acc = 0) on the first batch
  // with a valid slot of a state that began empty, where m is still -FLT_MAX
  const float r = exp2_hw((S.m - mb) * kLog2e);
  S.l *= r;
  S.acc = f4_scale(r, S.acc);
  S.m = mb;
#pragma unroll
  for (int u = 0; u < kHeadBatch; ++u) {
    if (ok[u]) {
      const float p = exp2_hw((s[u] - mb) * kLog2e);
      S.l += p;
      S.acc = f4_fma(p, v[u], S.acc);
      S.any = true;
    }
  }
}

// ---- host side: the entry points' argument checks and the launch
static inline bool head_shape_ok(int32_t k, int32_t heads, int32_t ch) {
  return heads >= 1 && heads <= 8 && ch >= 4 && ch % 4 == 0 && heads * ch <= 256 && k >= 1 &&
         k <= 64;
}

// a row stride in floats: rows of D floats, float4-addressable
static inline bool head_stride_ok(int64_t ld, int32_t D) { return ld >= D && ld % 4 == 0; }

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// 256-thread blocks for n rows, one group of 1 << lg lanes each
static inline int64_t head_blocks(int64_t n, int lg) {
  const int64_t gpb = 256 >> lg;
  return (n + gpb - 1) / gpb;
}

// kernel<C/4 is a power of two> on `blocks` blocks of 256 threads; inside an
// entry point (returns its error codes).
#define MIREC_HEADROW_LAUNCH(kernel, blocks, g, stream, ...)                                  \
  do {                                                                                        \
    const int64_t nb_ = (blocks);                                                             \
    MIREC_CHECK_ARG(nb_ < ((int64_t)1 << 31));                                                \
    if (((g) & ((g)-1)) == 0)                                                                 \
      hipLaunchKernelGGL(kernel<true>, dim3((unsigned)nb_), dim3(256), 0, stream,             \
                         __VA_ARGS__);                                                        \
    else                                                                                      \
      hipLaunchKernelGGL(kernel<false>, dim3((unsigned)nb_), dim3(256), 0, stream,            \
                         __VA_ARGS__);                                                        \
    MIREC_LAUNCH_CHECK();                                                                     \
  } while (0)

}  // namespace mirec
