// Training-mode BatchNorm2d (NCHW) with optional fused ReLU, plus frozen-BN
// fused apply. fp32/bf16 input, fp32 statistics and running stats.
//
// Reference call sites: nn.BatchNorm2d in every conv net
// (classification/resnet/models/networks.py:45), FrozenBatchNorm2d
// (detection/fasterRcnn/models/backbone/resnet50_fpn.py:5, FPN/fpn_model.py:8).
// The fused ReLU covers the conv->bn->relu chain that dominates ResNet.
#include "common.h"
#include "vec.h"

namespace dla {

// ---- pass 1: per-channel sum / sumsq ---------------------------------------
template <typename dev_t>
__global__ void bn_stats_kernel(const dev_t* __restrict__ x, float* __restrict__ sums,
                                int N, int C, int64_t HW) {
  __shared__ float smem[16];
  const int c = blockIdx.x;
  const int64_t total = (int64_t)N * HW;
  float sum = 0.f, sumsq = 0.f;
  for (int64_t m = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; m < total;
       m += (int64_t)gridDim.y * blockDim.x) {
    const int64_t n = m / HW, hw = m % HW;
    const float f = to_f32(x[(n * C + c) * HW + hw]);
    sum += f;
    sumsq += f * f;
  }
  sum = block_reduce_sum(sum, smem);
  sumsq = block_reduce_sum(sumsq, smem);
  if (threadIdx.x == 0) {
    atomicAdd(&sums[c], sum);
    atomicAdd(&sums[C + c], sumsq);
  }
}

// ---- finalize: mean/rstd + running-stat update + scale/shift ---------------
__device__ __forceinline__ void bn_finalize_channel(
    int c, float sum, float sumsq, const float* __restrict__ weight,
    const float* __restrict__ bias, float* __restrict__ mean,
    float* __restrict__ rstd, float* __restrict__ running_mean,
    float* __restrict__ running_var, float* __restrict__ scale,
    float* __restrict__ shift, float count, float eps, float momentum) {
  const float mu = sum / count;
  const float var = fmaxf(sumsq / count - mu * mu, 0.f);
  const float rs = rsqrtf(var + eps);
  mean[c] = mu;
  rstd[c] = rs;
  if (running_mean != nullptr && momentum > 0.f) {
    const float unbiased = var * count / fmaxf(count - 1.f, 1.f);
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
  const float sc = weight[c] * rs;
  scale[c] = sc;
  shift[c] = bias[c] - mu * sc;
}

__global__ void bn_finalize_kernel(const float* __restrict__ sums,
                                   const float* __restrict__ weight,
                                   const float* __restrict__ bias,
                                   float* __restrict__ mean, float* __restrict__ rstd,
                                   float* __restrict__ running_mean,
                                   float* __restrict__ running_var,
                                   float* __restrict__ scale, float* __restrict__ shift,
                                   int C, float count, float eps, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  bn_finalize_channel(c, sums[c], sums[C + c], weight, bias, mean, rstd,
                      running_mean, running_var, scale, shift, count, eps,
                      momentum);
}

// Finalize straight from the conv epilogue's [n_parts, 2C] per-block partial
// slab: each block owns kFinCh channels and sums the slab rows with kFinRows
// row lanes (fixed-order LDS tree, so the result is deterministic), then one
// lane per channel finalizes. Replaces a separate reduce launch per conv.
constexpr int kFinCh = 16, kFinRows = 64;

__global__ void __launch_bounds__(kFinCh * kFinRows)
bn_finalize_parts_kernel(const float* __restrict__ parts, int n_parts,
                         const float* __restrict__ weight,
                         const float* __restrict__ bias,
                         float* __restrict__ mean, float* __restrict__ rstd,
                         float* __restrict__ running_mean,
                         float* __restrict__ running_var,
                         float* __restrict__ scale, float* __restrict__ shift,
                         int C, float count, float eps, float momentum) {
  __shared__ float ls[2][kFinRows][kFinCh + 1];
  const int cl = threadIdx.x % kFinCh, rl = threadIdx.x / kFinCh;
  const int c = blockIdx.x * kFinCh + cl;
  float s = 0.f, q = 0.f;
  if (c < C) {
#pragma unroll 4
    for (int r = rl; r < n_parts; r += kFinRows) {
      const float* p = parts + (int64_t)r * 2 * C;
      s += p[c];
      q += p[C + c];
    }
  }
  ls[0][rl][cl] = s;
  ls[1][rl][cl] = q;
  __syncthreads();
  for (int h = kFinRows / 2; h > 0; h >>= 1) {
    if (rl < h) {
      ls[0][rl][cl] += ls[0][rl + h][cl];
      ls[1][rl][cl] += ls[1][rl + h][cl];
    }
    __syncthreads();
  }
  if (rl == 0 && c < C)
    bn_finalize_channel(c, ls[0][0][cl], ls[1][0][cl], weight, bias, mean,
                        rstd, running_mean, running_var, scale, shift, count,
                        eps, momentum);
}

// ---- pass 2 (also frozen-BN apply): y = x*scale[c] + shift[c] (+ReLU) ------
template <typename dev_t, int V, bool RELU>
__global__ void bn_apply_kernel(const dev_t* __restrict__ x,
                                const float* __restrict__ scale,
                                const float* __restrict__ shift,
                                dev_t* __restrict__ y, int C, int64_t HW,
                                int64_t n_total) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * V;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
       i < n_total; i += stride) {
    const int c = (int)((i / HW) % C);  // V divides HW, so one channel per vec
    const float sc = scale[c], sh = shift[c];
    Vec<dev_t, V> xv = vload<dev_t, V>(x + i);
    Vec<dev_t, V> yv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float f = to_f32(xv.v[j]) * sc + sh;
      yv.v[j] = from_f32<dev_t>(RELU ? fmaxf(f, 0.f) : f);
    }
    vstore<dev_t, V>(y + i, yv);
  }
}

// ---- backward pass 1: per-channel sum(dy), sum(dy * xhat) ------------------
template <typename dev_t, bool RELU>
__global__ void bn_bwd_stats_kernel(const dev_t* __restrict__ dy,
                                    const dev_t* __restrict__ x,
                                    const dev_t* __restrict__ y,  // for ReLU mask
                                    const float* __restrict__ mean,
                                    const float* __restrict__ rstd,
                                    float* __restrict__ sums,
                                    int N, int C, int64_t HW) {
  __shared__ float smem[16];
  const int c = blockIdx.x;
  const float mu = mean[c], rs = rstd[c];
  const int64_t total = (int64_t)N * HW;
  float s_dy = 0.f, s_dyxh = 0.f;
  for (int64_t m = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; m < total;
       m += (int64_t)gridDim.y * blockDim.x) {
    const int64_t n = m / HW, hw = m % HW;
    const int64_t idx = (n * C + c) * HW + hw;
    float g = to_f32(dy[idx]);
    if (RELU && to_f32(y[idx]) <= 0.f) g = 0.f;
    const float xh = (to_f32(x[idx]) - mu) * rs;
    s_dy += g;
    s_dyxh += g * xh;
  }
  s_dy = block_reduce_sum(s_dy, smem);
  s_dyxh = block_reduce_sum(s_dyxh, smem);
  if (threadIdx.x == 0) {
    atomicAdd(&sums[c], s_dy);
    atomicAdd(&sums[C + c], s_dyxh);
  }
}

// ---- backward pass 2: dx -----------------------------------------------------
template <typename dev_t, bool RELU>
__global__ void bn_bwd_dx_kernel(const dev_t* __restrict__ dy,
                                 const dev_t* __restrict__ x,
                                 const dev_t* __restrict__ y,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ rstd,
                                 const float* __restrict__ weight,
                                 const float* __restrict__ sums,
                                 dev_t* __restrict__ dx, int C, int64_t HW,
                                 int64_t n_total, float inv_count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_total;
       i += stride) {
    const int c = (int)((i / HW) % C);
    const float mu = mean[c], rs = rstd[c];
    float g = to_f32(dy[i]);
    if (RELU && to_f32(y[i]) <= 0.f) g = 0.f;
    const float xh = (to_f32(x[i]) - mu) * rs;
    const float m_dy = sums[c] * inv_count;
    const float m_dyxh = sums[C + c] * inv_count;
    dx[i] = from_f32<dev_t>(weight[c] * rs * (g - m_dy - xh * m_dyxh));
  }
}

// ======================= NHWC (channels_last) variants =======================
// NHWC is the fast layout on MI355X (MIOpen conv prefers it; BN reductions are
// column sums over a [N*H*W, C] row-major matrix -> fully coalesced).

// NHWC kernels share one thread mapping: flat thread t -> (c0 = (t %
// lanes_per_row)*V, row = t / lanes_per_row), rows strided by
// used_threads/lanes_per_row. Adjacent lanes read adjacent 16B channel chunks
// (fully coalesced); per-channel parameters load ONCE per thread (c0 is
// loop-invariant). Stats kernels block-reduce through LDS (ds_add_f32) and
// issue 2*C global atomics per block.

inline int64_t nhwc_used_threads(int lanes_per_row, int64_t rows,
                                 int64_t target_lanes) {
  int64_t k = target_lanes / lanes_per_row;
  if (k > rows) k = rows;
  if (k < 1) k = 1;
  return (int64_t)lanes_per_row * k;
}

template <typename dev_t, int V>
__global__ void bn_stats_nhwc_kernel(const dev_t* __restrict__ x,
                                     float* __restrict__ sums, int C,
                                     int64_t rows, int64_t used) {
  extern __shared__ float ls[];  // 2*C floats
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) ls[i] = 0.f;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lanes_per_row = C / V;
  if (t < used) {
    const int c0 = (int)(t % lanes_per_row) * V;
    const int64_t rstride = used / lanes_per_row;
    float s[V], q[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { s[j] = 0.f; q[j] = 0.f; }
    for (int64_t r = t / lanes_per_row; r < rows; r += rstride) {
      Vec<dev_t, V> xv = vload<dev_t, V>(x + r * C + c0);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float f = to_f32(xv.v[j]);
        s[j] += f;
        q[j] += f * f;
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      atomicAdd(&ls[c0 + j], s[j]);
      atomicAdd(&ls[C + c0 + j], q[j]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x)
    atomicAdd(&sums[i], ls[i]);
}

template <typename dev_t, int V, bool RELU>
__global__ void bn_apply_nhwc_kernel(const dev_t* __restrict__ x,
                                     const float* __restrict__ scale,
                                     const float* __restrict__ shift,
                                     dev_t* __restrict__ y, int C, int64_t rows,
                                     int64_t used) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= used) return;
  const int lanes_per_row = C / V;
  const int c0 = (int)(t % lanes_per_row) * V;
  const int64_t rstride = used / lanes_per_row;
  float sc[V], sh[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { sc[j] = scale[c0 + j]; sh[j] = shift[c0 + j]; }
  for (int64_t r = t / lanes_per_row; r < rows; r += rstride) {
    Vec<dev_t, V> xv = vload<dev_t, V>(x + r * C + c0);
    Vec<dev_t, V> yv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float f = to_f32(xv.v[j]) * sc[j] + sh[j];
      yv.v[j] = from_f32<dev_t>(RELU ? fmaxf(f, 0.f) : f);
    }
    vstore<dev_t, V>(y + r * C + c0, yv);
  }
}

template <typename dev_t, int V, bool RELU>
__global__ void bn_bwd_stats_nhwc_kernel(const dev_t* __restrict__ dy,
                                         const dev_t* __restrict__ x,
                                         const dev_t* __restrict__ y,
                                         const float* __restrict__ mean,
                                         const float* __restrict__ rstd,
                                         float* __restrict__ sums, int C,
                                         int64_t rows, int64_t used) {
  extern __shared__ float ls[];
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) ls[i] = 0.f;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lanes_per_row = C / V;
  if (t < used) {
    const int c0 = (int)(t % lanes_per_row) * V;
    const int64_t rstride = used / lanes_per_row;
    float mu[V], rs[V], s_dy[V], s_dyxh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      mu[j] = mean[c0 + j];
      rs[j] = rstd[c0 + j];
      s_dy[j] = 0.f;
      s_dyxh[j] = 0.f;
    }
    for (int64_t r = t / lanes_per_row; r < rows; r += rstride) {
      const int64_t base = r * C + c0;
      Vec<dev_t, V> dyv = vload<dev_t, V>(dy + base);
      Vec<dev_t, V> xv = vload<dev_t, V>(x + base);
      Vec<dev_t, V> yv;
      if (RELU) yv = vload<dev_t, V>(y + base);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float g = to_f32(dyv.v[j]);
        if (RELU && to_f32(yv.v[j]) <= 0.f) g = 0.f;
        const float xh = (to_f32(xv.v[j]) - mu[j]) * rs[j];
        s_dy[j] += g;
        s_dyxh[j] += g * xh;
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      atomicAdd(&ls[c0 + j], s_dy[j]);
      atomicAdd(&ls[C + c0 + j], s_dyxh[j]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x)
    atomicAdd(&sums[i], ls[i]);
}

template <typename dev_t, int V, bool RELU>
__global__ void bn_bwd_dx_nhwc_kernel(const dev_t* __restrict__ dy,
                                      const dev_t* __restrict__ x,
                                      const dev_t* __restrict__ y,
                                      const float* __restrict__ mean,
                                      const float* __restrict__ rstd,
                                      const float* __restrict__ weight,
                                      const float* __restrict__ sums,
                                      dev_t* __restrict__ dx, int C,
                                      int64_t rows, int64_t used,
                                      float inv_count) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= used) return;
  const int lanes_per_row = C / V;
  const int c0 = (int)(t % lanes_per_row) * V;
  const int64_t rstride = used / lanes_per_row;
  float mu[V], rs[V], wr[V], m_dy[V], m_dyxh[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = mean[c0 + j];
    rs[j] = rstd[c0 + j];
    wr[j] = weight[c0 + j] * rs[j];
    m_dy[j] = sums[c0 + j] * inv_count;
    m_dyxh[j] = sums[C + c0 + j] * inv_count;
  }
  for (int64_t r = t / lanes_per_row; r < rows; r += rstride) {
    const int64_t base = r * C + c0;
    Vec<dev_t, V> dyv = vload<dev_t, V>(dy + base);
    Vec<dev_t, V> xv = vload<dev_t, V>(x + base);
    Vec<dev_t, V> yv;
    if (RELU) yv = vload<dev_t, V>(y + base);
    Vec<dev_t, V> dxv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float g = to_f32(dyv.v[j]);
      if (RELU && to_f32(yv.v[j]) <= 0.f) g = 0.f;
      const float xh = (to_f32(xv.v[j]) - mu[j]) * rs[j];
      dxv.v[j] = from_f32<dev_t>(wr[j] * (g - m_dy[j] - xh * m_dyxh[j]));
    }
    vstore<dev_t, V>(dx + r * C + c0, dxv);
  }
}

// ---- fused residual join: out = relu(bn(x) + identity) ----------------------
// DUAL: the identity is itself a raw conv output with its own BN (first block
// of a stage): out = relu(x*sc + sh + xd*scd + shd). fp32 arithmetic, one
// rounding to the output type; the BN output is never materialised.
template <typename dev_t, int V, bool DUAL>
__global__ void bn_add_relu_nhwc_kernel(const dev_t* __restrict__ x,
                                        const float* __restrict__ scale,
                                        const float* __restrict__ shift,
                                        const dev_t* __restrict__ idn,
                                        const float* __restrict__ scale_d,
                                        const float* __restrict__ shift_d,
                                        dev_t* __restrict__ out, int C,
                                        int64_t rows, int64_t used) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= used) return;
  const int lanes_per_row = C / V;
  const int c0 = (int)(t % lanes_per_row) * V;
  const int64_t rstride = used / lanes_per_row;
  float sc[V], sh[V], scd[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sc[j] = scale[c0 + j];
    sh[j] = shift[c0 + j];
    if (DUAL) {
      scd[j] = scale_d[c0 + j];
      sh[j] += shift_d[c0 + j];
    }
  }
  for (int64_t r = t / lanes_per_row; r < rows; r += rstride) {
    const int64_t base = r * C + c0;
    Vec<dev_t, V> xv = vload<dev_t, V>(x + base);
    Vec<dev_t, V> iv = vload<dev_t, V>(idn + base);
    Vec<dev_t, V> ov;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float f = to_f32(xv.v[j]) * sc[j] + sh[j];
      f += DUAL ? to_f32(iv.v[j]) * scd[j] : to_f32(iv.v[j]);
      ov.v[j] = from_f32<dev_t>(fmaxf(f, 0.f));
    }
    vstore<dev_t, V>(out + base, ov);
  }
}

// Join backward pass 1: g = dy * [out > 0] is written once (it is the
// identity gradient and the input of pass 2), and sum(g), sum(g*xhat)
// (DUAL: also sum(g*xhat_d)) reduce per channel through LDS.
// sums layout: {sum g [C], sum g*xhat [C], sum g*xhat_d [C] (DUAL)}.
template <typename dev_t, int V, bool DUAL>
__global__ void bn_join_bwd_stats_nhwc_kernel(
    const dev_t* __restrict__ dy, const dev_t* __restrict__ out,
    const dev_t* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const dev_t* __restrict__ xd,
    const float* __restrict__ mean_d, const float* __restrict__ rstd_d,
    dev_t* __restrict__ g_out, float* __restrict__ sums, int C, int64_t rows,
    int64_t used) {
  constexpr int NS = DUAL ? 3 : 2;
  extern __shared__ float ls[];  // NS*C floats
  for (int i = threadIdx.x; i < NS * C; i += blockDim.x) ls[i] = 0.f;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lanes_per_row = C / V;
  if (t < used) {
    const int c0 = (int)(t % lanes_per_row) * V;
    const int64_t rstride = used / lanes_per_row;
    float mu[V], rs[V], mud[V], rsd[V], s_g[V], s_gxh[V], s_gxhd[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      mu[j] = mean[c0 + j];
      rs[j] = rstd[c0 + j];
      mud[j] = DUAL ? mean_d[c0 + j] : 0.f;
      rsd[j] = DUAL ? rstd_d[c0 + j] : 0.f;
      s_g[j] = 0.f;
      s_gxh[j] = 0.f;
      s_gxhd[j] = 0.f;
    }
    for (int64_t r = t / lanes_per_row; r < rows; r += rstride) {
      const int64_t base = r * C + c0;
      Vec<dev_t, V> dyv = vload<dev_t, V>(dy + base);
      Vec<dev_t, V> ov = vload<dev_t, V>(out + base);
      Vec<dev_t, V> xv = vload<dev_t, V>(x + base);
      Vec<dev_t, V> xdv;
      if (DUAL) xdv = vload<dev_t, V>(xd + base);
      Vec<dev_t, V> gv;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const bool on = to_f32(ov.v[j]) > 0.f;
        gv.v[j] = on ? dyv.v[j] : from_f32<dev_t>(0.f);
        const float g = on ? to_f32(dyv.v[j]) : 0.f;
        s_g[j] += g;
        s_gxh[j] += g * ((to_f32(xv.v[j]) - mu[j]) * rs[j]);
        if (DUAL) s_gxhd[j] += g * ((to_f32(xdv.v[j]) - mud[j]) * rsd[j]);
      }
      vstore<dev_t, V>(g_out + base, gv);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      atomicAdd(&ls[c0 + j], s_g[j]);
      atomicAdd(&ls[C + c0 + j], s_gxh[j]);
      if (DUAL) atomicAdd(&ls[2 * C + c0 + j], s_gxhd[j]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NS * C; i += blockDim.x)
    atomicAdd(&sums[i], ls[i]);
}

// Dual join backward pass 2: one read of g feeds both BNs' dx.
// (The single join reuses bn_bwd_dx_nhwc_kernel<.., false> with dy = g.)
template <typename dev_t, int V>
__global__ void bn_join_bwd_dx_dual_nhwc_kernel(
    const dev_t* __restrict__ g, const dev_t* __restrict__ x,
    const dev_t* __restrict__ xd, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ weight,
    const float* __restrict__ mean_d, const float* __restrict__ rstd_d,
    const float* __restrict__ weight_d, const float* __restrict__ sums,
    dev_t* __restrict__ dx, dev_t* __restrict__ dxd, int C, int64_t rows,
    int64_t used, float inv_count) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= used) return;
  const int lanes_per_row = C / V;
  const int c0 = (int)(t % lanes_per_row) * V;
  const int64_t rstride = used / lanes_per_row;
  float mu[V], rs[V], wr[V], mud[V], rsd[V], wrd[V], m_g[V], m_gxh[V],
      m_gxhd[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = mean[c0 + j];
    rs[j] = rstd[c0 + j];
    wr[j] = weight[c0 + j] * rs[j];
    mud[j] = mean_d[c0 + j];
    rsd[j] = rstd_d[c0 + j];
    wrd[j] = weight_d[c0 + j] * rsd[j];
    m_g[j] = sums[c0 + j] * inv_count;
    m_gxh[j] = sums[C + c0 + j] * inv_count;
    m_gxhd[j] = sums[2 * C + c0 + j] * inv_count;
  }
  for (int64_t r = t / lanes_per_row; r < rows; r += rstride) {
    const int64_t base = r * C + c0;
    Vec<dev_t, V> gv = vload<dev_t, V>(g + base);
    Vec<dev_t, V> xv = vload<dev_t, V>(x + base);
    Vec<dev_t, V> xdv = vload<dev_t, V>(xd + base);
    Vec<dev_t, V> dxv, dxdv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float gg = to_f32(gv.v[j]) - m_g[j];
      const float xh = (to_f32(xv.v[j]) - mu[j]) * rs[j];
      const float xhd = (to_f32(xdv.v[j]) - mud[j]) * rsd[j];
      dxv.v[j] = from_f32<dev_t>(wr[j] * (gg - xh * m_gxh[j]));
      dxdv.v[j] = from_f32<dev_t>(wrd[j] * (gg - xhd * m_gxhd[j]));
    }
    vstore<dev_t, V>(dx + base, dxv);
    vstore<dev_t, V>(dxd + base, dxdv);
  }
}

inline bool is_nhwc(const torch::Tensor& t) {
  return t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast) &&
         !t.is_contiguous();
}

struct BnFinalized {
  torch::Tensor mean, rstd, scale, shift;
};

// Launch the finalize step on `sums`: either the [2C] {sum, sumsq} vector or
// the conv epilogue's [n_parts, 2C] partial slab (summed inside the kernel).
inline BnFinalized bn_finalize_launch(
    const torch::Tensor& sums, const torch::Tensor& weight,
    const torch::Tensor& bias, c10::optional<torch::Tensor>& running_mean,
    c10::optional<torch::Tensor>& running_var, int C, int64_t rows,
    double momentum, double eps) {
  TORCH_CHECK(sums.is_cuda() && sums.scalar_type() == torch::kFloat &&
                  sums.is_contiguous(),
              "bn sums must be a contiguous fp32 GPU tensor");
  TORCH_CHECK((sums.dim() == 1 && sums.size(0) == 2 * C) ||
                  (sums.dim() == 2 && sums.size(0) >= 1 &&
                   sums.size(1) == 2 * C),
              "bn sums must be [2C] or [n_parts, 2C]");
  TORCH_CHECK(weight.numel() == C && bias.numel() == C,
              "bn weight/bias must have C elements");
  auto opts_f = sums.options();
  BnFinalized f{torch::empty({C}, opts_f), torch::empty({C}, opts_f),
                torch::empty({C}, opts_f), torch::empty({C}, opts_f)};
  auto w32 = weight.to(torch::kFloat).contiguous();
  auto b32 = bias.to(torch::kFloat).contiguous();
  float* rm = running_mean.has_value() ? running_mean->data_ptr<float>() : nullptr;
  float* rv = running_var.has_value() ? running_var->data_ptr<float>() : nullptr;
  const int n_parts = sums.dim() == 2 ? (int)sums.size(0) : 1;
  if (n_parts > 1) {
    hipLaunchKernelGGL(bn_finalize_parts_kernel, dim3((C + kFinCh - 1) / kFinCh),
                       dim3(kFinCh * kFinRows), 0, stream(),
                       sums.data_ptr<float>(), n_parts, w32.data_ptr<float>(),
                       b32.data_ptr<float>(), f.mean.data_ptr<float>(),
                       f.rstd.data_ptr<float>(), rm, rv,
                       f.scale.data_ptr<float>(), f.shift.data_ptr<float>(), C,
                       (float)rows, (float)eps, (float)momentum);
  } else {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0,
                       stream(), sums.data_ptr<float>(), w32.data_ptr<float>(),
                       b32.data_ptr<float>(), f.mean.data_ptr<float>(),
                       f.rstd.data_ptr<float>(), rm, rv,
                       f.scale.data_ptr<float>(), f.shift.data_ptr<float>(), C,
                       (float)rows, (float)eps, (float)momentum);
  }
  return f;
}

// dweight / dbias as views of the backward sums buffer: no device copy when
// the parameter is fp32, one conversion otherwise.
inline torch::Tensor bn_param_grad(const torch::Tensor& sums, int64_t offset,
                                   int C, const torch::Tensor& weight) {
  return sums.narrow(0, offset, C).to(weight.scalar_type());
}

inline bool is_nhwc_rows(const torch::Tensor& t) {
  return t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast);
}

}  // namespace dla

// Returns {y, save_mean, save_rstd}. Updates running stats in-place when given.
std::vector<torch::Tensor> batchnorm_fwd(torch::Tensor x, torch::Tensor weight,
                                         torch::Tensor bias,
                                         c10::optional<torch::Tensor> running_mean,
                                         c10::optional<torch::Tensor> running_var,
                                         double momentum, double eps, bool relu) {
  DLA_CHECK_CUDA(x);
  TORCH_CHECK(x.dim() == 4, "batchnorm_fwd expects a 4D tensor");
  const bool nhwc = dla::is_nhwc(x);
  TORCH_CHECK(nhwc || x.is_contiguous(), "batchnorm_fwd: x must be contiguous "
              "(NCHW or channels_last)");
  const int N = (int)x.size(0), C = (int)x.size(1);
  const int64_t HW = x.size(2) * x.size(3);
  auto opts_f = x.options().dtype(torch::kFloat);
  auto sums = torch::zeros({2 * C}, opts_f);
  auto mean = torch::empty({C}, opts_f);
  auto rstd = torch::empty({C}, opts_f);
  auto scale = torch::empty({C}, opts_f);
  auto shift = torch::empty({C}, opts_f);
  auto y = torch::empty_like(x);
  auto w32 = weight.to(torch::kFloat);
  auto b32 = bias.to(torch::kFloat);

  const int64_t rows = (int64_t)N * HW;
  const int ysplit = (int)std::min<int64_t>((rows + 65535) / 65536 + 1,
                                            std::max(1, 2048 / C));
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "batchnorm_fwd", [&] {
    if (nhwc) {
      constexpr int VM = 16 / (int)sizeof(dev_t);
      auto stats = [&](auto vtag) {
        constexpr int V = decltype(vtag)::value;
        const int lanes = C / V;
        const int64_t used = dla::nhwc_used_threads(lanes, rows, 262144);
        const int lds = 2 * C * sizeof(float);
        hipLaunchKernelGGL((dla::bn_stats_nhwc_kernel<dev_t, V>),
                           dim3((int)((used + 255) / 256)), dim3(256), lds,
                           dla::stream(), (const dev_t*)x.data_ptr(),
                           sums.data_ptr<float>(), C, rows, used);
      };
      if (C % VM == 0) stats(std::integral_constant<int, VM>{});
      else if (C % 2 == 0) stats(std::integral_constant<int, 2>{});
      else stats(std::integral_constant<int, 1>{});
    } else {
      hipLaunchKernelGGL((dla::bn_stats_kernel<dev_t>), dim3(C, ysplit), dim3(256), 0,
                         dla::stream(), (const dev_t*)x.data_ptr(),
                         sums.data_ptr<float>(), N, C, HW);
    }
    hipLaunchKernelGGL(dla::bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0,
                       dla::stream(), sums.data_ptr<float>(), w32.data_ptr<float>(),
                       b32.data_ptr<float>(), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(),
                       running_mean.has_value() ? running_mean->data_ptr<float>() : nullptr,
                       running_var.has_value() ? running_var->data_ptr<float>() : nullptr,
                       scale.data_ptr<float>(), shift.data_ptr<float>(), C,
                       (float)rows, (float)eps, (float)momentum);
    const int64_t n_total = x.numel();
    constexpr int VMAX = 16 / (int)sizeof(dev_t);
    auto launch = [&](auto vtag, auto rtag) {
      constexpr int V = decltype(vtag)::value;
      constexpr bool R = decltype(rtag)::value;
      if (nhwc) {
        const int lanes = C / V;
        const int64_t used = dla::nhwc_used_threads(lanes, rows, 524288);
        hipLaunchKernelGGL((dla::bn_apply_nhwc_kernel<dev_t, V, R>),
                           dim3((int)((used + 255) / 256)), dim3(256), 0,
                           dla::stream(), (const dev_t*)x.data_ptr(),
                           scale.data_ptr<float>(), shift.data_ptr<float>(),
                           (dev_t*)y.data_ptr(), C, rows, used);
        return;
      }
      const int grid = dla::grid_1d((n_total + V - 1) / V, 256);
      if (false) ;
      else
        hipLaunchKernelGGL((dla::bn_apply_kernel<dev_t, V, R>), dim3(grid), dim3(256),
                           0, dla::stream(), (const dev_t*)x.data_ptr(),
                           scale.data_ptr<float>(), shift.data_ptr<float>(),
                           (dev_t*)y.data_ptr(), C, HW, n_total);
    };
    const bool vec_ok = nhwc ? (C % VMAX == 0) : (HW % VMAX == 0);
    if (vec_ok) {
      if (relu) launch(std::integral_constant<int, VMAX>{}, std::true_type{});
      else launch(std::integral_constant<int, VMAX>{}, std::false_type{});
    } else {
      if (relu) launch(std::integral_constant<int, 1>{}, std::true_type{});
      else launch(std::integral_constant<int, 1>{}, std::false_type{});
    }
  });
  HIP_CHECK_ERR();
  return {y, mean, rstd};
}

// Train-mode BN forward with the stats pass ALREADY DONE by the producing
// kernel (conv1x1_fwd's fused sum/sumsq epilogue): finalize + apply only —
// saves one full read pass over x vs batchnorm_fwd. sums layout matches
// bn_stats: [2C] = {sum[c], sumsq[C+c]}, or the conv epilogue's per-block
// [n_parts, 2C] slab, which the finalize kernel sums itself.
std::vector<torch::Tensor> batchnorm_fwd_from_sums(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor sums, c10::optional<torch::Tensor> running_mean,
    c10::optional<torch::Tensor> running_var, double momentum, double eps,
    bool relu) {
  DLA_CHECK_CUDA(x);
  TORCH_CHECK(x.dim() == 4, "batchnorm_fwd_from_sums expects a 4D tensor");
  const bool nhwc = dla::is_nhwc(x);
  TORCH_CHECK(nhwc || x.is_contiguous(),
              "batchnorm_fwd_from_sums: x must be contiguous");
  const int N = (int)x.size(0), C = (int)x.size(1);
  const int64_t HW = x.size(2) * x.size(3);
  auto y = torch::empty_like(x);
  const int64_t rows = (int64_t)N * HW;
  auto fin = dla::bn_finalize_launch(sums, weight, bias, running_mean,
                                     running_var, C, rows, momentum, eps);
  auto& mean = fin.mean;
  auto& rstd = fin.rstd;
  auto& scale = fin.scale;
  auto& shift = fin.shift;
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "batchnorm_fwd_from_sums", [&] {
    const int64_t n_total = x.numel();
    constexpr int VMAX = 16 / (int)sizeof(dev_t);
    auto launch = [&](auto vtag, auto rtag) {
      constexpr int V = decltype(vtag)::value;
      constexpr bool R = decltype(rtag)::value;
      if (nhwc) {
        const int lanes = C / V;
        const int64_t used = dla::nhwc_used_threads(lanes, rows, 524288);
        hipLaunchKernelGGL((dla::bn_apply_nhwc_kernel<dev_t, V, R>),
                           dim3((int)((used + 255) / 256)), dim3(256), 0,
                           dla::stream(), (const dev_t*)x.data_ptr(),
                           scale.data_ptr<float>(), shift.data_ptr<float>(),
                           (dev_t*)y.data_ptr(), C, rows, used);
        return;
      }
      const int grid = dla::grid_1d((n_total + V - 1) / V, 256);
      hipLaunchKernelGGL((dla::bn_apply_kernel<dev_t, V, R>), dim3(grid),
                         dim3(256), 0, dla::stream(),
                         (const dev_t*)x.data_ptr(), scale.data_ptr<float>(),
                         shift.data_ptr<float>(), (dev_t*)y.data_ptr(), C, HW,
                         n_total);
    };
    const bool vec_ok = nhwc ? (C % VMAX == 0) : (HW % VMAX == 0);
    if (vec_ok) {
      if (relu) launch(std::integral_constant<int, VMAX>{}, std::true_type{});
      else launch(std::integral_constant<int, VMAX>{}, std::false_type{});
    } else {
      if (relu) launch(std::integral_constant<int, 1>{}, std::true_type{});
      else launch(std::integral_constant<int, 1>{}, std::false_type{});
    }
  });
  HIP_CHECK_ERR();
  return {y, mean, rstd};
}

// Frozen/eval BN apply (+optional ReLU): per-channel scale/shift precomputed host-side.
torch::Tensor bn_apply(torch::Tensor x, torch::Tensor scale, torch::Tensor shift,
                       bool relu) {
  DLA_CHECK_CUDA(x);
  TORCH_CHECK(x.dim() == 4, "bn_apply expects a 4D tensor");
  const bool nhwc = dla::is_nhwc(x);
  TORCH_CHECK(nhwc || x.is_contiguous(), "bn_apply: x must be contiguous");
  const int C = (int)x.size(1);
  const int64_t HW = x.size(2) * x.size(3);
  auto y = torch::empty_like(x);
  auto sc = scale.to(torch::kFloat).contiguous();
  auto sh = shift.to(torch::kFloat).contiguous();
  const int64_t n_total = x.numel();
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "bn_apply", [&] {
    constexpr int VMAX = 16 / (int)sizeof(dev_t);
    auto launch = [&](auto vtag, auto rtag) {
      constexpr int V = decltype(vtag)::value;
      constexpr bool R = decltype(rtag)::value;
      if (nhwc) {
        const int64_t rows = n_total / C;
        const int lanes = C / V;
        const int64_t used = dla::nhwc_used_threads(lanes, rows, 524288);
        hipLaunchKernelGGL((dla::bn_apply_nhwc_kernel<dev_t, V, R>),
                           dim3((int)((used + 255) / 256)), dim3(256), 0,
                           dla::stream(), (const dev_t*)x.data_ptr(),
                           sc.data_ptr<float>(), sh.data_ptr<float>(),
                           (dev_t*)y.data_ptr(), C, rows, used);
        return;
      }
      const int grid = dla::grid_1d((n_total + V - 1) / V, 256);
      if (false) ;
      else
        hipLaunchKernelGGL((dla::bn_apply_kernel<dev_t, V, R>), dim3(grid), dim3(256),
                           0, dla::stream(), (const dev_t*)x.data_ptr(),
                           sc.data_ptr<float>(), sh.data_ptr<float>(),
                           (dev_t*)y.data_ptr(), C, HW, n_total);
    };
    const bool vec_ok = nhwc ? (C % VMAX == 0) : (HW % VMAX == 0);
    if (vec_ok) {
      if (relu) launch(std::integral_constant<int, VMAX>{}, std::true_type{});
      else launch(std::integral_constant<int, VMAX>{}, std::false_type{});
    } else {
      if (relu) launch(std::integral_constant<int, 1>{}, std::true_type{});
      else launch(std::integral_constant<int, 1>{}, std::false_type{});
    }
  });
  HIP_CHECK_ERR();
  return y;
}

// Returns {dx, dweight, dbias}. y is required when relu=true (mask source).
std::vector<torch::Tensor> batchnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         c10::optional<torch::Tensor> y,
                                         torch::Tensor weight, torch::Tensor mean,
                                         torch::Tensor rstd, bool relu) {
  DLA_CHECK_CUDA(dy); DLA_CHECK_CUDA(x);
  const bool nhwc = dla::is_nhwc(x);
  TORCH_CHECK(nhwc || x.is_contiguous(), "batchnorm_bwd: x must be contiguous");
  if (nhwc && !dla::is_nhwc(dy)) dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  if (!nhwc) dy = dy.contiguous();
  const int N = (int)x.size(0), C = (int)x.size(1);
  const int64_t HW = x.size(2) * x.size(3);
  const int64_t rows = (int64_t)N * HW;
  auto opts_f = x.options().dtype(torch::kFloat);
  auto sums = torch::zeros({2 * C}, opts_f);
  auto dx = torch::empty_like(x);
  auto w32 = weight.to(torch::kFloat);
  const int ysplit = (int)std::min<int64_t>((rows + 65535) / 65536 + 1,
                                            std::max(1, 2048 / C));
  TORCH_CHECK(!relu || y.has_value(), "batchnorm_bwd: relu mask needs y");
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "batchnorm_bwd", [&] {
    const dev_t* yp = y.has_value() ? (const dev_t*)y->data_ptr() : nullptr;
    auto launch_stats = [&](auto rtag) {
      constexpr bool R = decltype(rtag)::value;
      if (nhwc) {
        constexpr int VM = 16 / (int)sizeof(dev_t);
        auto stats = [&](auto vtag) {
          constexpr int V = decltype(vtag)::value;
          const int lanes = C / V;
          const int64_t used = dla::nhwc_used_threads(lanes, rows, 262144);
          const int lds = 2 * C * sizeof(float);
          hipLaunchKernelGGL((dla::bn_bwd_stats_nhwc_kernel<dev_t, V, R>),
                             dim3((int)((used + 255) / 256)), dim3(256), lds,
                             dla::stream(), (const dev_t*)dy.data_ptr(),
                             (const dev_t*)x.data_ptr(), yp, mean.data_ptr<float>(),
                             rstd.data_ptr<float>(), sums.data_ptr<float>(), C,
                             rows, used);
        };
        if (C % VM == 0) stats(std::integral_constant<int, VM>{});
        else if (C % 2 == 0) stats(std::integral_constant<int, 2>{});
        else stats(std::integral_constant<int, 1>{});
      } else {
        hipLaunchKernelGGL((dla::bn_bwd_stats_kernel<dev_t, R>), dim3(C, ysplit),
                           dim3(256), 0, dla::stream(), (const dev_t*)dy.data_ptr(),
                           (const dev_t*)x.data_ptr(), yp, mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), sums.data_ptr<float>(), N, C, HW);
      }
    };
    if (relu) launch_stats(std::true_type{});
    else launch_stats(std::false_type{});

    const int64_t n_total = x.numel();
    const float inv_count = 1.f / (float)rows;
    constexpr int VMAX = 16 / (int)sizeof(dev_t);
    auto launch_dx = [&](auto vtag, auto rtag) {
      constexpr int V = decltype(vtag)::value;
      constexpr bool R = decltype(rtag)::value;
      if (nhwc) {
        const int lanes = C / V;
        const int64_t used = dla::nhwc_used_threads(lanes, rows, 524288);
        hipLaunchKernelGGL((dla::bn_bwd_dx_nhwc_kernel<dev_t, V, R>),
                           dim3((int)((used + 255) / 256)), dim3(256), 0,
                           dla::stream(), (const dev_t*)dy.data_ptr(),
                           (const dev_t*)x.data_ptr(), yp, mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), w32.data_ptr<float>(),
                           sums.data_ptr<float>(), (dev_t*)dx.data_ptr(), C,
                           rows, used, inv_count);
      } else {
        hipLaunchKernelGGL((dla::bn_bwd_dx_kernel<dev_t, R>), dim3(dla::grid_1d(n_total, 256)),
                           dim3(256), 0, dla::stream(), (const dev_t*)dy.data_ptr(),
                           (const dev_t*)x.data_ptr(), yp, mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), w32.data_ptr<float>(),
                           sums.data_ptr<float>(), (dev_t*)dx.data_ptr(), C, HW,
                           n_total, inv_count);
      }
    };
    const bool vec_ok = nhwc && (C % VMAX == 0);
    if (vec_ok) {
      if (relu) launch_dx(std::integral_constant<int, VMAX>{}, std::true_type{});
      else launch_dx(std::integral_constant<int, VMAX>{}, std::false_type{});
    } else {
      if (relu) launch_dx(std::integral_constant<int, 1>{}, std::true_type{});
      else launch_dx(std::integral_constant<int, 1>{}, std::false_type{});
    }
  });
  HIP_CHECK_ERR();
  return {dx, dla::bn_param_grad(sums, C, C, weight),
          dla::bn_param_grad(sums, 0, C, weight)};
}

// ---- fused residual join ----------------------------------------------------
namespace dla {

inline void join_check(const torch::Tensor& x, const torch::Tensor& other,
                       const char* what) {
  TORCH_CHECK(other.is_cuda() && other.scalar_type() == x.scalar_type() &&
                  other.sizes() == x.sizes() && is_nhwc_rows(other),
              "bn join: ", what, " must match x (shape, dtype, channels_last)");
}

inline int join_vec(const torch::Tensor& x) {
  const int vmax = 16 / (int)x.element_size();
  TORCH_CHECK(x.size(1) % vmax == 0,
              "bn join: C must be a multiple of ", vmax);
  return vmax;
}

}  // namespace dla

// out = relu(bn(x) + identity), BN finalized from the conv-fused sums
// ([2C] or [n_parts, 2C]). Returns {out, save_mean, save_rstd}.
std::vector<torch::Tensor> bn_add_relu_fwd_from_sums(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor sums, c10::optional<torch::Tensor> running_mean,
    c10::optional<torch::Tensor> running_var, double momentum, double eps,
    torch::Tensor identity) {
  DLA_CHECK_CUDA(x);
  TORCH_CHECK(dla::is_nhwc_rows(x), "bn_add_relu: x must be channels_last");
  dla::join_check(x, identity, "identity");
  dla::join_vec(x);
  const int C = (int)x.size(1);
  const int64_t rows = x.numel() / C;
  auto fin = dla::bn_finalize_launch(sums, weight, bias, running_mean,
                                     running_var, C, rows, momentum, eps);
  auto out = torch::empty_like(x);
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "bn_add_relu_fwd_from_sums", [&] {
    constexpr int V = 16 / (int)sizeof(dev_t);
    const int64_t used = dla::nhwc_used_threads(C / V, rows, 524288);
    hipLaunchKernelGGL((dla::bn_add_relu_nhwc_kernel<dev_t, V, false>),
                       dim3((int)((used + 255) / 256)), dim3(256), 0,
                       dla::stream(), (const dev_t*)x.data_ptr(),
                       fin.scale.data_ptr<float>(), fin.shift.data_ptr<float>(),
                       (const dev_t*)identity.data_ptr(), nullptr, nullptr,
                       (dev_t*)out.data_ptr(), C, rows, used);
  });
  HIP_CHECK_ERR();
  return {out, fin.mean, fin.rstd};
}

// out = relu(bn(x) + bn_d(xd)): both operands are raw conv outputs.
// Returns {out, mean, rstd, mean_d, rstd_d}.
std::vector<torch::Tensor> bn_add_relu_dual_fwd_from_sums(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor sums, c10::optional<torch::Tensor> running_mean,
    c10::optional<torch::Tensor> running_var, double momentum, double eps,
    torch::Tensor xd, torch::Tensor weight_d, torch::Tensor bias_d,
    torch::Tensor sums_d, c10::optional<torch::Tensor> running_mean_d,
    c10::optional<torch::Tensor> running_var_d, double momentum_d,
    double eps_d) {
  DLA_CHECK_CUDA(x);
  TORCH_CHECK(dla::is_nhwc_rows(x), "bn_add_relu_dual: x must be channels_last");
  dla::join_check(x, xd, "xd");
  dla::join_vec(x);
  const int C = (int)x.size(1);
  const int64_t rows = x.numel() / C;
  auto fin = dla::bn_finalize_launch(sums, weight, bias, running_mean,
                                     running_var, C, rows, momentum, eps);
  auto fd = dla::bn_finalize_launch(sums_d, weight_d, bias_d, running_mean_d,
                                    running_var_d, C, rows, momentum_d, eps_d);
  auto out = torch::empty_like(x);
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "bn_add_relu_dual_fwd_from_sums", [&] {
    constexpr int V = 16 / (int)sizeof(dev_t);
    const int64_t used = dla::nhwc_used_threads(C / V, rows, 524288);
    hipLaunchKernelGGL((dla::bn_add_relu_nhwc_kernel<dev_t, V, true>),
                       dim3((int)((used + 255) / 256)), dim3(256), 0,
                       dla::stream(), (const dev_t*)x.data_ptr(),
                       fin.scale.data_ptr<float>(), fin.shift.data_ptr<float>(),
                       (const dev_t*)xd.data_ptr(), fd.scale.data_ptr<float>(),
                       fd.shift.data_ptr<float>(), (dev_t*)out.data_ptr(), C,
                       rows, used);
  });
  HIP_CHECK_ERR();
  return {out, fin.mean, fin.rstd, fd.mean, fd.rstd};
}

// Backward of the single join. Returns {g, dx, dweight, dbias}; g = dy*[out>0]
// is the identity gradient itself (not a copy).
std::vector<torch::Tensor> bn_add_relu_bwd(torch::Tensor dy, torch::Tensor out,
                                           torch::Tensor x, torch::Tensor weight,
                                           torch::Tensor mean,
                                           torch::Tensor rstd) {
  DLA_CHECK_CUDA(x);
  TORCH_CHECK(dla::is_nhwc_rows(x), "bn_add_relu_bwd: x must be channels_last");
  dla::join_check(x, out, "out");
  if (!dla::is_nhwc_rows(dy)) dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  dla::join_check(x, dy, "dy");
  dla::join_vec(x);
  const int C = (int)x.size(1);
  const int64_t rows = x.numel() / C;
  TORCH_CHECK(mean.numel() == C && rstd.numel() == C && weight.numel() == C,
              "bn_add_relu_bwd: per-channel tensors must have C elements");
  auto sums = torch::zeros({2 * C}, x.options().dtype(torch::kFloat));
  auto g = torch::empty_like(x);
  auto dx = torch::empty_like(x);
  auto w32 = weight.to(torch::kFloat).contiguous();
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "bn_add_relu_bwd", [&] {
    constexpr int V = 16 / (int)sizeof(dev_t);
    const int lanes = C / V;
    const int64_t used_s = dla::nhwc_used_threads(lanes, rows, 262144);
    hipLaunchKernelGGL((dla::bn_join_bwd_stats_nhwc_kernel<dev_t, V, false>),
                       dim3((int)((used_s + 255) / 256)), dim3(256),
                       2 * C * sizeof(float), dla::stream(),
                       (const dev_t*)dy.data_ptr(), (const dev_t*)out.data_ptr(),
                       (const dev_t*)x.data_ptr(), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), nullptr, nullptr, nullptr,
                       (dev_t*)g.data_ptr(), sums.data_ptr<float>(), C, rows,
                       used_s);
    const int64_t used = dla::nhwc_used_threads(lanes, rows, 524288);
    hipLaunchKernelGGL((dla::bn_bwd_dx_nhwc_kernel<dev_t, V, false>),
                       dim3((int)((used + 255) / 256)), dim3(256), 0,
                       dla::stream(), (const dev_t*)g.data_ptr(),
                       (const dev_t*)x.data_ptr(), nullptr,
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       w32.data_ptr<float>(), sums.data_ptr<float>(),
                       (dev_t*)dx.data_ptr(), C, rows, used,
                       1.f / (float)rows);
  });
  HIP_CHECK_ERR();
  return {g, dx, dla::bn_param_grad(sums, C, C, weight),
          dla::bn_param_grad(sums, 0, C, weight)};
}

// Backward of the dual join. Returns {dx, dxd, dweight, dbias, dweight_d,
// dbias_d}; sum g is shared, so dbias_d holds the same values as dbias.
std::vector<torch::Tensor> bn_add_relu_dual_bwd(
    torch::Tensor dy, torch::Tensor out, torch::Tensor x, torch::Tensor weight,
    torch::Tensor mean, torch::Tensor rstd, torch::Tensor xd,
    torch::Tensor weight_d, torch::Tensor mean_d, torch::Tensor rstd_d) {
  DLA_CHECK_CUDA(x);
  TORCH_CHECK(dla::is_nhwc_rows(x), "bn_add_relu_dual_bwd: x must be channels_last");
  dla::join_check(x, out, "out");
  dla::join_check(x, xd, "xd");
  if (!dla::is_nhwc_rows(dy)) dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  dla::join_check(x, dy, "dy");
  dla::join_vec(x);
  const int C = (int)x.size(1);
  const int64_t rows = x.numel() / C;
  TORCH_CHECK(mean.numel() == C && rstd.numel() == C && weight.numel() == C &&
                  mean_d.numel() == C && rstd_d.numel() == C &&
                  weight_d.numel() == C,
              "bn_add_relu_dual_bwd: per-channel tensors must have C elements");
  auto sums = torch::zeros({3 * C}, x.options().dtype(torch::kFloat));
  auto g = torch::empty_like(x);
  auto dx = torch::empty_like(x);
  auto dxd = torch::empty_like(x);
  auto w32 = weight.to(torch::kFloat).contiguous();
  auto wd32 = weight_d.to(torch::kFloat).contiguous();
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "bn_add_relu_dual_bwd", [&] {
    constexpr int V = 16 / (int)sizeof(dev_t);
    const int lanes = C / V;
    const int64_t used_s = dla::nhwc_used_threads(lanes, rows, 262144);
    hipLaunchKernelGGL((dla::bn_join_bwd_stats_nhwc_kernel<dev_t, V, true>),
                       dim3((int)((used_s + 255) / 256)), dim3(256),
                       3 * C * sizeof(float), dla::stream(),
                       (const dev_t*)dy.data_ptr(), (const dev_t*)out.data_ptr(),
                       (const dev_t*)x.data_ptr(), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), (const dev_t*)xd.data_ptr(),
                       mean_d.data_ptr<float>(), rstd_d.data_ptr<float>(),
                       (dev_t*)g.data_ptr(), sums.data_ptr<float>(), C, rows,
                       used_s);
    const int64_t used = dla::nhwc_used_threads(lanes, rows, 524288);
    hipLaunchKernelGGL((dla::bn_join_bwd_dx_dual_nhwc_kernel<dev_t, V>),
                       dim3((int)((used + 255) / 256)), dim3(256), 0,
                       dla::stream(), (const dev_t*)g.data_ptr(),
                       (const dev_t*)x.data_ptr(), (const dev_t*)xd.data_ptr(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       w32.data_ptr<float>(), mean_d.data_ptr<float>(),
                       rstd_d.data_ptr<float>(), wd32.data_ptr<float>(),
                       sums.data_ptr<float>(), (dev_t*)dx.data_ptr(),
                       (dev_t*)dxd.data_ptr(), C, rows, used,
                       1.f / (float)rows);
  });
  HIP_CHECK_ERR();
  // sum g serves both biases, but two parameters must not share gradient
  // storage (optimizers update .grad in place): the second gets a copy
  auto dbias = dla::bn_param_grad(sums, 0, C, weight);
  return {dx, dxd, dla::bn_param_grad(sums, C, C, weight), dbias,
          dla::bn_param_grad(sums, 2 * C, C, weight_d),
          dbias.to(weight_d.scalar_type()).clone()};
}
