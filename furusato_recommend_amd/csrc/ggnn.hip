// GRU gate of the gated graph hop (PyG GatedGraphConv(d, num_layers=1,
// aggr='mean'): a torch.nn.GRUCell on (mean of the projected children, the
// node's own row); model/gnn.py:185-232, conv = 'ggnn').  The three GEMMs run
// before these kernels — a = (mean_j x_j) W, gi = a W_ihᵀ + b_ih, gh = x W_hhᵀ
// + b_hh, the biases added in the GEMM epilogue — so the gate reads finished
// pre-activations; thirds of a [3d] row in the order r, z, n:
//   r = σ(gi_r + gh_r)   z = σ(gi_z + gh_z)   n = tanh(gi_n + r gh_n)
//   out = (1 - z) n + z h        (ReLU fused if asked)
//
//   mirec_gru_gate      forward
//   mirec_gru_gate_bwd  ∂gi, ∂gh and the direct ∂h from grad_out; the gates
//                       are recomputed, `out` is only read for the ReLU mask
//
// Layout: the row movers' (common.h) — 1 << lg lanes per row, lg = ceil log2
// (d / 4), one float4 column per lane, lanes past d / 4 idle; no lane talks to
// another.  The grid is capped at kGruMaxBlocks blocks of 256 >> lg rows and
// strides over the rows.  Both kernels are memory-bound (forward 7 d floats
// read and d written per row, backward 9 d read and 7 d written); every access
// is a 16-byte load or store, all of a thread's loads issued before its math.
//
// σ and tanh saturate instead of overflowing: σ(x) = 1 / (1 + 2^(-x log2 e)),
// tanh(x) = 1 - 2 / (1 + 2^(2 x log2 e)); an exponential that overflows gives
// 1 / inf = 0, one that underflows 1 / 1, so every finite pre-activation gives
// a finite gate.  One v_exp_f32 and one v_rcp_f32 per gate.
#include "common.h"

namespace mirec {

constexpr int kGruMaxBlocks = 2048;
constexpr int kGruMaxDim = 1024;  // 256 >> lg rows per block must be >= 1

__device__ __forceinline__ float rcp_hw(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float sigmoid_hw(float x) {
  return rcp_hw(1.f + exp2_hw(-kLog2e * x));
}
__device__ __forceinline__ float tanh_hw(float x) {
  return fmaf(-2.f, rcp_hw(1.f + exp2_hw((2.f * kLog2e) * x)), 1.f);
}

struct Gates {
  float r, z, n;
};
__device__ __forceinline__ Gates gru_gates(float gi_r, float gi_z, float gi_n, float gh_r,
                                           float gh_z, float gh_n) {
  Gates q;
  q.r = sigmoid_hw(gi_r + gh_r);
  q.z = sigmoid_hw(gi_z + gh_z);
  q.n = tanh_hw(fmaf(q.r, gh_n, gi_n));
  return q;
}
__device__ __forceinline__ float gru_out(const Gates &q, float h) {
  return fmaf(q.z, h - q.n, q.n);
}

__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void gru_gate_kernel(
    const float *__restrict__ gi, const float *__restrict__ gh, const float *__restrict__ h,
    int64_t n, int32_t d4, int32_t lg, int32_t relu, float *__restrict__ out) {
  const int c = threadIdx.x & ((1 << lg) - 1);
  if (c >= d4) return;
  const int rpb = 256 >> lg;
  const int64_t D = (int64_t)d4 * 4;
  for (int64_t r = (int64_t)blockIdx.x * rpb + (threadIdx.x >> lg); r < n;
       r += (int64_t)gridDim.x * rpb) {
    const float *pi = gi + r * 3 * D + 4 * c, *ph = gh + r * 3 * D + 4 * c;
    const float4 ir = ld4(pi), iz = ld4(pi + D), in = ld4(pi + 2 * D);
    const float4 hr = ld4(ph), hz = ld4(ph + D), hn = ld4(ph + 2 * D);
    const float4 x = ld4(h + r * D + 4 * c);
    float4 o;
    o.x = gru_out(gru_gates(ir.x, iz.x, in.x, hr.x, hz.x, hn.x), x.x);
    o.y = gru_out(gru_gates(ir.y, iz.y, in.y, hr.y, hz.y, hn.y), x.y);
    o.z = gru_out(gru_gates(ir.z, iz.z, in.z, hr.z, hz.z, hn.z), x.z);
    o.w = gru_out(gru_gates(ir.w, iz.w, in.w, hr.w, hz.w, hn.w), x.w);
    if (relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
    st4(out + r * D + 4 * c, o);
  }
}

// One element of the backward: g is the gradient after the ReLU mask.
struct GruGrad {
  float i_r, i_z, i_n, h_n, h;  // ∂gh_r = ∂gi_r, ∂gh_z = ∂gi_z
};
__device__ __forceinline__ GruGrad gru_bwd1(float g, float gi_r, float gi_z, float gi_n,
                                            float gh_r, float gh_z, float gh_n, float h) {
  const Gates q = gru_gates(gi_r, gi_z, gi_n, gh_r, gh_z, gh_n);
  GruGrad o;
  o.h = g * q.z;
  const float dn = g * (1.f - q.z);
  const float dz = g * (h - q.n);
  const float pn = dn * fmaf(-q.n, q.n, 1.f);
  o.i_n = pn;
  o.h_n = pn * q.r;
  const float dr = pn * gh_n;
  o.i_r = dr * (q.r * (1.f - q.r));
  o.i_z = dz * (q.z * (1.f - q.z));
  return o;
}

__global__ __launch_bounds__(256) MIREC_NO_PK_F32 void gru_gate_bwd_kernel(
    const float *__restrict__ grad_out, const float *__restrict__ gi,
    const float *__restrict__ gh, const float *__restrict__ h, const float *__restrict__ out,
    int64_t n, int32_t d4, int32_t lg, float *__restrict__ d_gi, float *__restrict__ d_gh,
    float *__restrict__ d_h) {
  const int c = threadIdx.x & ((1 << lg) - 1);
  if (c >= d4) return;
  const int rpb = 256 >> lg;
  const int64_t D = (int64_t)d4 * 4;
  for (int64_t r = (int64_t)blockIdx.x * rpb + (threadIdx.x >> lg); r < n;
       r += (int64_t)gridDim.x * rpb) {
    const int64_t o1 = r * D + 4 * c, o3 = r * 3 * D + 4 * c;
    const float *pi = gi + o3, *ph = gh + o3;
    float4 g = ld4(grad_out + o1);
    const float4 ir = ld4(pi), iz = ld4(pi + D), in = ld4(pi + 2 * D);
    const float4 hr = ld4(ph), hz = ld4(ph + D), hn = ld4(ph + 2 * D);
    const float4 x = ld4(h + o1);
    if (out != nullptr) {  // the fused ReLU passed the gradient where out > 0
      const float4 y = ld4(out + o1);
      g = make_float4(y.x > 0.f ? g.x : 0.f, y.y > 0.f ? g.y : 0.f, y.z > 0.f ? g.z : 0.f,
                      y.w > 0.f ? g.w : 0.f);
    }
    const GruGrad a = gru_bwd1(g.x, ir.x, iz.x, in.x, hr.x, hz.x, hn.x, x.x);
    const GruGrad b = gru_bwd1(g.y, ir.y, iz.y, in.y, hr.y, hz.y, hn.y, x.y);
    const GruGrad e = gru_bwd1(g.z, ir.z, iz.z, in.z, hr.z, hz.z, hn.z, x.z);
    const GruGrad f = gru_bwd1(g.w, ir.w, iz.w, in.w, hr.w, hz.w, hn.w, x.w);
    const float4 pr = make_float4(a.i_r, b.i_r, e.i_r, f.i_r);
    const float4 pz = make_float4(a.i_z, b.i_z, e.i_z, f.i_z);
    st4(d_gi + o3, pr);
    st4(d_gi + o3 + D, pz);
    st4(d_gi + o3 + 2 * D, make_float4(a.i_n, b.i_n, e.i_n, f.i_n));
    st4(d_gh + o3, pr);
    st4(d_gh + o3 + D, pz);
    st4(d_gh + o3 + 2 * D, make_float4(a.h_n, b.h_n, e.h_n, f.h_n));
    st4(d_h + o1, make_float4(a.h, b.h, e.h, f.h));
  }
}

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

static inline bool gru_dim_ok(int32_t dim) { return dim >= 4 && dim % 4 == 0 && dim <= kGruMaxDim; }

static unsigned gru_blocks(int64_t n_rows, int lg) {
  const int64_t rpb = 256 >> lg;
  const int64_t b = (n_rows + rpb - 1) / rpb;
  return (unsigned)(b < kGruMaxBlocks ? b : kGruMaxBlocks);
}

}  // namespace mirec

extern "C" int mirec_gru_gate(const float *gi, const float *gh, const float *h, int64_t n_rows,
                              int32_t dim, int32_t relu, float *out, mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(n_rows >= 0 && gru_dim_ok(dim));
  if (n_rows == 0) return MIREC_OK;
  MIREC_CHECK_ARG(gi && gh && h && out);
  MIREC_CHECK_ARG(aligned16(gi) && aligned16(gh) && aligned16(h) && aligned16(out));
  const int d4 = dim / 4, lg = row_lg(d4);
  hipLaunchKernelGGL(gru_gate_kernel, dim3(gru_blocks(n_rows, lg)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), gi, gh, h, n_rows, d4, lg,
                     relu ? 1 : 0, out);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}

extern "C" int mirec_gru_gate_bwd(const float *grad_out, const float *gi, const float *gh,
                                  const float *h, const float *out, int64_t n_rows, int32_t dim,
                                  float *grad_gi, float *grad_gh, float *grad_h,
                                  mirec_stream_t stream) {
  using namespace mirec;
  MIREC_CHECK_ARG(n_rows >= 0 && gru_dim_ok(dim));
  if (n_rows == 0) return MIREC_OK;
  MIREC_CHECK_ARG(grad_out && gi && gh && h && grad_gi && grad_gh && grad_h);
  MIREC_CHECK_ARG(aligned16(grad_out) && aligned16(gi) && aligned16(gh) && aligned16(h) &&
                  aligned16(out) && aligned16(grad_gi) && aligned16(grad_gh) &&
                  aligned16(grad_h));
  const int d4 = dim / 4, lg = row_lg(d4);
  hipLaunchKernelGGL(gru_gate_bwd_kernel, dim3(gru_blocks(n_rows, lg)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), grad_out, gi, gh, h, out, n_rows, d4,
                     lg, grad_gi, grad_gh, grad_h);
  MIREC_LAUNCH_CHECK();
  return MIREC_OK;
}
