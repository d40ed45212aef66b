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

// bn_pre (the BN pre-activation, shared with the conv1x1 dgrad epilogue) lives
// in common.h.

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
      const float f = bn_pre(to_f32(xv.v[j]), sc, sh);
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
// loop-invariant). That is the mapping of the apply and dx kernels
// (used_threads is nhwc_used_threads of common.h); the per-channel reduction
// kernels have their own, below.

// ---- NHWC per-channel reductions: no atomics, one slab row per block -------
// The reduction kernels (stats, backward stats, join backward stats, stem
// backward stats) run on a grid of (channel chunks, row splits). A block owns
// `bl` <= kRedLanes adjacent V-wide lanes of the row and rb = 256 / bl
// row-lanes; thread (rl, lane) sums rows split*rb + rl, + splits*rb, ... in
// registers. The block then sums its row-lanes per channel in ascending order
// through LDS and stores the result to row `split` of a [splits, NS*C] slab
// with plain stores: every slab element is written by exactly one block,
// whatever (rows, C), because the column ranges of the chunks partition
// [0, C) and every (chunk, split) block stores its whole range, zeros when it
// had no rows. A second small kernel (bn_slab_reduce_kernel, or the finalize
// kernel in forward) sums the slab rows in a fixed order, so every BN result
// is bit-reproducible.
constexpr int kRedThreads = 256;
constexpr int kRedLanes = 32;      // widest channel chunk of a block, in lanes
constexpr int kRedBlocks = 2048;   // grid target: 8 blocks per CU
constexpr int kRedMaxParts = 512;  // most slab rows
constexpr int kRedMinRows = 8;     // stop splitting below 8 rows per thread
// Rows in flight per thread: about eight 16-byte loads, whatever the number
// of tensors a kernel reads per row.
constexpr int red_unroll(int tensors) { return tensors <= 2 ? 4 : 2; }

// Four waves per SIMD is the occupancy these kernels are written for: with a
// 128-register budget hipcc keeps the unrolled rows' loads together; asked
// for more waves it sinks every load to its first use to save registers.
#define DLA_RED_KERNEL \
  __launch_bounds__(dla::kRedThreads) __attribute__((amdgpu_waves_per_eu(1, 4)))

struct NhwcRedTile {
  int bl, rb, chunks, parts;
};

inline NhwcRedTile nhwc_red_tile(int lanes_per_row, int64_t rows,
                                 int blocks = kRedBlocks,
                                 int max_parts = kRedMaxParts) {
  NhwcRedTile t;
  t.chunks = (lanes_per_row + kRedLanes - 1) / kRedLanes;
  t.bl = (lanes_per_row + t.chunks - 1) / t.chunks;  // chunks*bl >= lanes
  t.rb = kRedThreads / t.bl;
  const int64_t per_part = (int64_t)t.rb * kRedMinRows;
  const int64_t by_rows = (rows + per_part - 1) / per_part;
  const int64_t p = std::min<int64_t>(
      std::min<int64_t>(blocks / t.chunks, max_parts), by_rows);
  t.parts = (int)std::max<int64_t>(p, 1);
  return t;
}

struct NhwcRedPos {
  int c0;           // first channel of this thread
  int64_t row;      // first row
  int64_t rstride;  // row step
  bool active;      // false: a lane past C or a row-lane past rb
};

template <int V>
__device__ __forceinline__ NhwcRedPos nhwc_red_pos(int C, int bl, int rb) {
  const int lane = threadIdx.x % bl, rl = threadIdx.x / bl;
  const int gl = blockIdx.x * bl + lane;
  NhwcRedPos p;
  p.c0 = gl * V;
  p.row = (int64_t)blockIdx.y * rb + rl;
  p.rstride = (int64_t)gridDim.y * rb;
  p.active = rl < rb && gl < C / V;
  return p;
}

// add(r, load(r)) for this thread's rows in ascending order. load(r) returns
// the row's vectors; U rows are loaded before the first is added, so
// that their loads are in flight together (hipcc does not hoist them itself).
template <int U, typename L, typename A>
__device__ __forceinline__ void nhwc_red_rows(const NhwcRedPos& p,
                                              int64_t rows, L&& load, A&& add) {
  if (!p.active) return;
  using D = decltype(load(int64_t{}));
  int64_t r = p.row;
  for (; r + (U - 1) * p.rstride < rows; r += U * p.rstride) {
    D d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) d[u] = load(r + u * p.rstride);
#pragma unroll
    for (int u = 0; u < U; ++u) add(r + u * p.rstride, d[u]);
  }
  for (; r < rows; r += p.rstride) add(r, load(r));
}

// The shared tail: acc[s][j] is this thread's partial of sum s for channel
// c0 + j (zero in inactive threads). Every thread of the block must call it.
template <int V, int NS>
__device__ __forceinline__ void nhwc_red_tail(const float (&acc)[NS][V],
                                              float* __restrict__ slab, int C,
                                              int bl, int rb) {
  __shared__ __attribute__((aligned(16))) float ls[kRedThreads * V];
  const int W = bl * V;  // channels of this block, <= kRedLanes * V
  const int cbase = blockIdx.x * W;
  float* out = slab + (int64_t)blockIdx.y * NS * C;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s) __syncthreads();  // the previous sum's reads are done
    if ((int)threadIdx.x < bl * rb) {  // (rl, lane) sits at rl*W + lane*V
#pragma unroll
      for (int j = 0; j < V; ++j) ls[threadIdx.x * V + j] = acc[s][j];
    }
    __syncthreads();
    for (int col = threadIdx.x; col < W; col += kRedThreads) {
      if (cbase + col < C) {
        float sum = 0.f;
        for (int r = 0; r < rb; ++r) sum += ls[r * W + col];
        out[s * C + cbase + col] = sum;
      }
    }
  }
}

// Sums the rows of a [n_parts, n_cols] slab per column into sums[n_cols]:
// row-lane rl adds rows rl, rl + kSlabRows, ... in ascending order, then a
// fixed tree over the row-lanes.
constexpr int kSlabCols = 32, kSlabRows = 32;

__global__ void __launch_bounds__(kSlabCols * kSlabRows)
bn_slab_reduce_kernel(const float* __restrict__ slab, int n_parts, int n_cols,
                      float* __restrict__ sums) {
  __shared__ float ls[kSlabRows][kSlabCols + 1];
  const int cl = threadIdx.x % kSlabCols, rl = threadIdx.x / kSlabCols;
  const int c = blockIdx.x * kSlabCols + cl;
  float s = 0.f;
  if (c < n_cols) {
#pragma unroll 4
    for (int r = rl; r < n_parts; r += kSlabRows)
      s += slab[(int64_t)r * n_cols + c];
  }
  ls[rl][cl] = s;
  __syncthreads();
  for (int h = kSlabRows / 2; h > 0; h >>= 1) {
    if (rl < h) ls[rl][cl] += ls[rl + h][cl];
    __syncthreads();
  }
  if (rl == 0 && c < n_cols) sums[c] = ls[0][cl];
}

// First stage for deep slabs (the conv dgrad epilogue leaves one row per 128
// GEMM rows: 6272 at 56x56, batch 256): block (x, y) sums the kSlabGroup rows
// of group y for its kSlabCols columns into row y of a [groups, n_cols] slab,
// in the same order as above; bn_slab_reduce_kernel then sums the groups.
// groups * n_cols / 32 blocks pull the slab, not n_cols / 32.
constexpr int kSlabGroup = 128;     // slab rows per first-stage block
// Slabs deeper than any reduction kernel's own (kRedMaxParts) take two stages.
constexpr int kSlabDeep = kRedMaxParts;

__global__ void __launch_bounds__(kSlabCols * kSlabRows)
bn_slab_group_reduce_kernel(const float* __restrict__ slab, int n_parts,
                            int n_cols, float* __restrict__ groups) {
  __shared__ float ls[kSlabRows][kSlabCols + 1];
  const int cl = threadIdx.x % kSlabCols, rl = threadIdx.x / kSlabCols;
  const int c = blockIdx.x * kSlabCols + cl;
  const int r0 = blockIdx.y * kSlabGroup;
  const int r1 = r0 + kSlabGroup < n_parts ? r0 + kSlabGroup : n_parts;
  float s = 0.f;
  if (c < n_cols) {
#pragma unroll 4
    for (int r = r0 + rl; r < r1; r += kSlabRows)
      s += slab[(int64_t)r * n_cols + c];
  }
  ls[rl][cl] = s;
  __syncthreads();
  for (int h = kSlabRows / 2; h > 0; h >>= 1) {
    if (rl < h) ls[rl][cl] += ls[rl + h][cl];
    __syncthreads();
  }
  if (rl == 0 && c < n_cols) groups[(int64_t)blockIdx.y * n_cols + c] = ls[0][cl];
}

template <typename dev_t, int V>
__global__ void DLA_RED_KERNEL
bn_stats_nhwc_kernel(const dev_t* __restrict__ x, float* __restrict__ slab,
                     int C, int64_t rows, int bl, int rb) {
  const NhwcRedPos p = nhwc_red_pos<V>(C, bl, rb);
  float acc[2][V];  // sum, sumsq
#pragma unroll
  for (int j = 0; j < V; ++j) { acc[0][j] = 0.f; acc[1][j] = 0.f; }
  nhwc_red_rows<red_unroll(1)>(
      p, rows, [&](int64_t r) { return vload<dev_t, V>(x + r * C + p.c0); },
      [&](int64_t, const Vec<dev_t, V>& xv) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float f = to_f32(xv.v[j]);
          acc[0][j] += f;
          acc[1][j] += f * f;
        }
      });
  nhwc_red_tail<V, 2>(acc, slab, C, bl, rb);
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
      const float f = bn_pre(to_f32(xv.v[j]), sc[j], sh[j]);
      yv.v[j] = from_f32<dev_t>(RELU ? fmaxf(f, 0.f) : f);
    }
    vstore<dev_t, V>(y + r * C + c0, yv);
  }
}

// RELU backward kernels take the mask from x (MASK_Y = false: g = 0 where
// bn_pre(x, scale, shift) is not > 0; y is neither passed nor loaded) or, for
// A/B runs and callers of the old entry point, from the stored y (MASK_Y).
template <typename dev_t, int V, bool RELU, bool MASK_Y = false>
__global__ void DLA_RED_KERNEL
bn_bwd_stats_nhwc_kernel(const dev_t* __restrict__ dy,
                         const dev_t* __restrict__ x,
                         const dev_t* __restrict__ y,
                         const float* __restrict__ scale,
                         const float* __restrict__ shift,
                         const float* __restrict__ mean,
                         const float* __restrict__ rstd,
                         float* __restrict__ slab, int C, int64_t rows, int bl,
                         int rb) {
  const NhwcRedPos p = nhwc_red_pos<V>(C, bl, rb);
  float mu[V], rs[V], sc[V], sh[V];
  float acc[2][V];  // sum dy, sum dy*xhat
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = p.active ? mean[p.c0 + j] : 0.f;
    rs[j] = p.active ? rstd[p.c0 + j] : 0.f;
    sc[j] = (p.active && RELU && !MASK_Y) ? scale[p.c0 + j] : 0.f;
    sh[j] = (p.active && RELU && !MASK_Y) ? shift[p.c0 + j] : 0.f;
    acc[0][j] = 0.f;
    acc[1][j] = 0.f;
  }
  struct Row {
    Vec<dev_t, V> dy, x, y;
  };
  nhwc_red_rows<red_unroll(MASK_Y ? 3 : 2)>(
      p, rows,
      [&](int64_t r) {
        const int64_t base = r * C + p.c0;
        Row d;
        d.dy = vload<dev_t, V>(dy + base);
        d.x = vload<dev_t, V>(x + base);
        if (RELU && MASK_Y) d.y = vload<dev_t, V>(y + base);
        return d;
      },
      [&](int64_t, const Row& d) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          float g = to_f32(d.dy.v[j]);
          const float xf = to_f32(d.x.v[j]);
          if (RELU && MASK_Y && to_f32(d.y.v[j]) <= 0.f) g = 0.f;
          if (RELU && !MASK_Y && !(bn_pre(xf, sc[j], sh[j]) > 0.f)) g = 0.f;
          const float xh = (xf - mu[j]) * rs[j];
          acc[0][j] += g;
          acc[1][j] += g * xh;
        }
      });
  nhwc_red_tail<V, 2>(acc, slab, C, bl, rb);
}

template <typename dev_t, int V, bool RELU, bool MASK_Y = false>
__global__ void bn_bwd_dx_nhwc_kernel(const dev_t* __restrict__ dy,
                                      const dev_t* __restrict__ x,
                                      const dev_t* __restrict__ y,
                                      const float* __restrict__ scale,
                                      const float* __restrict__ shift,
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
  float mu[V], rs[V], wr[V], sc[V], sh[V], m_dy[V], m_dyxh[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = mean[c0 + j];
    rs[j] = rstd[c0 + j];
    wr[j] = weight[c0 + j] * rs[j];
    sc[j] = (RELU && !MASK_Y) ? scale[c0 + j] : 0.f;
    sh[j] = (RELU && !MASK_Y) ? shift[c0 + j] : 0.f;
    m_dy[j] = sums[c0 + j] * inv_count;
    m_dyxh[j] = sums[C + c0 + j] * inv_count;
  }
  for (int64_t r = t / lanes_per_row; r < rows; r += rstride) {
    const int64_t base = r * C + c0;
    Vec<dev_t, V> dyv = vload<dev_t, V>(dy + base);
    Vec<dev_t, V> xv = vload<dev_t, V>(x + base);
    Vec<dev_t, V> yv;
    if (RELU && MASK_Y) yv = vload<dev_t, V>(y + base);
    Vec<dev_t, V> dxv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float g = to_f32(dyv.v[j]);
      const float xf = to_f32(xv.v[j]);
      if (RELU && MASK_Y && to_f32(yv.v[j]) <= 0.f) g = 0.f;
      if (RELU && !MASK_Y && !(bn_pre(xf, sc[j], sh[j]) > 0.f)) g = 0.f;
      const float xh = (xf - mu[j]) * rs[j];
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
__global__ void DLA_RED_KERNEL
bn_join_bwd_stats_nhwc_kernel(
    const dev_t* __restrict__ dy, const dev_t* __restrict__ out,
    const dev_t* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const dev_t* __restrict__ xd,
    const float* __restrict__ mean_d, const float* __restrict__ rstd_d,
    dev_t* __restrict__ g_out, float* __restrict__ slab, int C, int64_t rows,
    int bl, int rb) {
  constexpr int NS = DUAL ? 3 : 2;
  const NhwcRedPos p = nhwc_red_pos<V>(C, bl, rb);
  float mu[V], rs[V], mud[V], rsd[V];
  float acc[NS][V];  // sum g, sum g*xhat, (DUAL) sum g*xhat_d
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = p.active ? mean[p.c0 + j] : 0.f;
    rs[j] = p.active ? rstd[p.c0 + j] : 0.f;
    mud[j] = (p.active && DUAL) ? mean_d[p.c0 + j] : 0.f;
    rsd[j] = (p.active && DUAL) ? rstd_d[p.c0 + j] : 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s][j] = 0.f;
  }
  struct Row {
    Vec<dev_t, V> dy, out, x, xd;
  };
  nhwc_red_rows<red_unroll(DUAL ? 4 : 3)>(
      p, rows,
      [&](int64_t r) {
        const int64_t base = r * C + p.c0;
        Row d;
        d.dy = vload<dev_t, V>(dy + base);
        d.out = vload<dev_t, V>(out + base);
        d.x = vload<dev_t, V>(x + base);
        if (DUAL) d.xd = vload<dev_t, V>(xd + base);
        return d;
      },
      [&](int64_t r, const Row& d) {
        Vec<dev_t, V> gv;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const bool on = to_f32(d.out.v[j]) > 0.f;
          gv.v[j] = on ? d.dy.v[j] : from_f32<dev_t>(0.f);
          const float g = on ? to_f32(d.dy.v[j]) : 0.f;
          acc[0][j] += g;
          acc[1][j] += g * ((to_f32(d.x.v[j]) - mu[j]) * rs[j]);
          if (DUAL)
            acc[NS - 1][j] += g * ((to_f32(d.xd.v[j]) - mud[j]) * rsd[j]);
        }
        vstore<dev_t, V>(g_out + r * C + p.c0, gv);
      });
  nhwc_red_tail<V, NS>(acc, slab, C, bl, rb);
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

// ============================== host layer ===================================
// Every kernel is launched from ONE host function: a bn_*_launch below, or for
// the stem kernels their one entry point. A launcher owns its kernel's grid
// rule, its choice of vector width and the tensors the kernel produces. The
// bound entry points are compositions: bn_geom and the other checks, the
// parameter conversions, launchers, the packaging of the result.

// Two layout predicates; both meanings are in use.
// Any channels-last-contiguous 4-D tensor, [N, C, 1, 1] and [N, 1, H, W]
// (NCHW-contiguous as well) included: the joins, the dx-only entries and the
// stem, whose kernels see a [rows, C] matrix and nothing else.
inline bool is_nhwc_rows(const torch::Tensor& t) {
  return t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast);
}

// Channels-last and NOT NCHW-contiguous: batchnorm_fwd,
// batchnorm_fwd_from_sums, bn_apply and batchnorm_bwd_ex route on this one, so
// a tensor that is both takes their NCHW kernels.
inline bool is_nhwc_not_nchw(const torch::Tensor& t) {
  return is_nhwc_rows(t) && !t.is_contiguous();
}

template <typename dev_t>
constexpr int kVecMax = 16 / (int)sizeof(dev_t);  // 16-byte vectors

struct BnGeom {
  bool nhwc;  // x takes the NHWC kernels
  int N, C, H, W;
  int64_t HW, rows;  // rows = N * H * W
};

enum class BnLayout {
  kNchwOrNhwc,  // NHWC kernels iff is_nhwc_not_nchw, else NCHW-contiguous
  kNhwcRows,    // is_nhwc_rows, full-width vectors only
};

// The checks every entry makes on x (device, dtype, 4-D, layout) and x's
// geometry. The joins, the dx-only entries and the stem (kNhwcRows) have
// kernels for V = VMAX alone, so they require C % VMAX == 0.
inline BnGeom bn_geom(const torch::Tensor& x, const char* fn, BnLayout layout) {
  TORCH_CHECK(x.is_cuda(), fn, ": x must be a GPU tensor");
  TORCH_CHECK(x.dim() == 4, fn, " expects a 4D tensor");
  const auto st = x.scalar_type();
  TORCH_CHECK(st == torch::kFloat || st == torch::kBFloat16 ||
                  st == torch::kHalf, fn, ": unsupported dtype ", st);
  BnGeom geo;
  if (layout == BnLayout::kNhwcRows) {
    const int vmax = 16 / (int)x.element_size();
    TORCH_CHECK(is_nhwc_rows(x), fn, ": x must be channels_last");
    TORCH_CHECK(x.size(1) % vmax == 0, fn, ": C must be a multiple of ", vmax);
    geo.nhwc = true;
  } else {
    geo.nhwc = is_nhwc_not_nchw(x);
    TORCH_CHECK(geo.nhwc || x.is_contiguous(), fn,
                ": x must be contiguous (NCHW or channels_last)");
  }
  geo.N = (int)x.size(0), geo.C = (int)x.size(1);
  geo.H = (int)x.size(2), geo.W = (int)x.size(3);
  geo.HW = x.size(2) * x.size(3);
  geo.rows = (int64_t)geo.N * geo.HW;
  return geo;
}

// Per-channel tensors have C elements; where the entry hands their pointers
// to a kernel unconverted (fp32_contig) they are contiguous fp32 GPU tensors.
inline void bn_check_channels(std::initializer_list<const torch::Tensor*> ts,
                              int C, const char* fn, bool fp32_contig = false) {
  for (const auto* t : ts) {
    TORCH_CHECK(t->numel() == C, fn,
                ": per-channel tensors must have C elements");
    TORCH_CHECK(!fp32_contig ||
                    (t->is_cuda() && t->scalar_type() == torch::kFloat &&
                     t->is_contiguous()),
                fn, ": per-channel tensors must be contiguous fp32 [C]");
  }
}

// Grid of the NHWC elementwise kernels (apply, dx, join, stem dx): `used`
// threads in whole rows of C / V lanes, in blocks of 256.
constexpr int64_t kNhwcLaneTarget = 524288;

struct NhwcGrid {
  int64_t used;
  int blocks;
};

inline NhwcGrid nhwc_grid(int lanes_per_row, int64_t rows) {
  const int64_t used = nhwc_used_threads(lanes_per_row, rows, kNhwcLaneTarget);
  return {used, (int)((used + 255) / 256)};
}

// gridDim.y of the NCHW reduction kernels (gridDim.x = C).
inline int nchw_ysplit(const BnGeom& geo) {
  return (int)std::min<int64_t>((geo.rows + 65535) / 65536 + 1,
                                std::max(1, 2048 / geo.C));
}

// f(integral_constant V). The NHWC reduction kernels (forward and backward
// statistics) take V = VMAX, 2 or 1, whichever divides C.
template <typename dev_t, typename F>
inline void bn_red_vec(int C, F&& f) {
  if (C % kVecMax<dev_t> == 0) f(std::integral_constant<int, kVecMax<dev_t>>{});
  else if (C % 2 == 0) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 1>{});
}

// The elementwise kernels (apply, dx) take V = VMAX or 1, never 2.
template <typename dev_t, typename F>
inline void bn_elt_vec(bool vec_ok, F&& f) {
  if (vec_ok) f(std::integral_constant<int, kVecMax<dev_t>>{});
  else f(std::integral_constant<int, 1>{});
}

// Forward pass 1. NCHW: the [2C] {sum, sumsq} vector, zeroed because
// bn_stats_kernel adds into it. NHWC: the kernel's [n_parts, 2C] slab, which
// the finalize kernel sums.
inline torch::Tensor bn_stats_launch(const torch::Tensor& x, const BnGeom& geo) {
  const auto opts_f = x.options().dtype(torch::kFloat);
  const int C = geo.C;
  torch::Tensor sums;
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "bn_stats", [&] {
    if (!geo.nhwc) {
      sums = torch::zeros({2 * C}, opts_f);
      hipLaunchKernelGGL((bn_stats_kernel<dev_t>), dim3(C, nchw_ysplit(geo)),
                         dim3(256), 0, stream(), (const dev_t*)x.data_ptr(),
                         sums.data_ptr<float>(), geo.N, C, geo.HW);
      return;
    }
    bn_red_vec<dev_t>(C, [&](auto vtag) {
      constexpr int V = decltype(vtag)::value;
      const auto t = nhwc_red_tile(C / V, geo.rows);
      sums = torch::empty({t.parts, 2 * C}, opts_f);
      hipLaunchKernelGGL((bn_stats_nhwc_kernel<dev_t, V>),
                         dim3(t.chunks, t.parts), dim3(kRedThreads), 0,
                         stream(), (const dev_t*)x.data_ptr(),
                         sums.data_ptr<float>(), C, geo.rows, t.bl, t.rb);
    });
  });
  return sums;
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

// y = x * scale[c] + shift[c] (+ReLU); scale and shift contiguous fp32 [C].
// NHWC vectorises along C. NCHW vectorises along HW (HW % VMAX, not C), where
// a vector stays inside one channel.
inline torch::Tensor bn_apply_launch(const torch::Tensor& x, const BnGeom& geo,
                                     const torch::Tensor& scale,
                                     const torch::Tensor& shift, bool relu) {
  auto y = torch::empty_like(x);
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "bn_apply", [&] {
    const bool vec_ok = (geo.nhwc ? geo.C : geo.HW) % kVecMax<dev_t> == 0;
    bn_elt_vec<dev_t>(vec_ok, [&](auto vtag) {
      constexpr int V = decltype(vtag)::value;
      auto launch = [&](auto rtag) {
        constexpr bool R = decltype(rtag)::value;
        if (geo.nhwc) {
          const auto grid = nhwc_grid(geo.C / V, geo.rows);
          hipLaunchKernelGGL((bn_apply_nhwc_kernel<dev_t, V, R>),
                             dim3(grid.blocks), dim3(256), 0, stream(),
                             (const dev_t*)x.data_ptr(), scale.data_ptr<float>(),
                             shift.data_ptr<float>(), (dev_t*)y.data_ptr(),
                             geo.C, geo.rows, grid.used);
        } else {
          const int64_t n_total = x.numel();
          hipLaunchKernelGGL((bn_apply_kernel<dev_t, V, R>),
                             dim3(grid_1d((n_total + V - 1) / V, 256)),
                             dim3(256), 0, stream(), (const dev_t*)x.data_ptr(),
                             scale.data_ptr<float>(), shift.data_ptr<float>(),
                             (dev_t*)y.data_ptr(), geo.C, geo.HW, n_total);
        }
      };
      if (relu) launch(std::true_type{});
      else launch(std::false_type{});
    });
  });
  return y;
}

// dweight / dbias as views of the backward sums buffer: no device copy when
// the parameter is fp32, one conversion otherwise.
inline torch::Tensor bn_param_grad(const torch::Tensor& sums, int64_t offset,
                                   int C, const torch::Tensor& weight) {
  return sums.narrow(0, offset, C).to(weight.scalar_type());
}

// Backward: the [n_parts, NS*C] slab of a reduction kernel summed into a
// fresh [NS*C] tensor, which the dx kernels read and bn_param_grad views.
inline torch::Tensor bn_slab_reduce_launch(const torch::Tensor& slab) {
  const int n_parts = (int)slab.size(0), n_cols = (int)slab.size(1);
  if (n_parts > kSlabDeep) {  // two stages, both in a fixed order
    const int groups = (n_parts + kSlabGroup - 1) / kSlabGroup;
    auto part = torch::empty({groups, n_cols}, slab.options());
    hipLaunchKernelGGL(bn_slab_group_reduce_kernel,
                       dim3((n_cols + kSlabCols - 1) / kSlabCols, groups),
                       dim3(kSlabCols * kSlabRows), 0, stream(),
                       slab.data_ptr<float>(), n_parts, n_cols,
                       part.data_ptr<float>());
    return bn_slab_reduce_launch(part);
  }
  auto sums = torch::empty({n_cols}, slab.options());
  hipLaunchKernelGGL(bn_slab_reduce_kernel,
                     dim3((n_cols + kSlabCols - 1) / kSlabCols),
                     dim3(kSlabCols * kSlabRows), 0, stream(),
                     slab.data_ptr<float>(), n_parts, n_cols,
                     sums.data_ptr<float>());
  return sums;
}

// What a backward reads of one BN: its input, the saved statistics and the
// weight in fp32.
struct BnSaved {
  torch::Tensor x, mean, rstd, w32;
};

// Where the ReLU mask of a BN(+ReLU) backward comes from: the stored y
// (MASK_Y), or x through the forward's scale and shift. All null without ReLU.
struct BnMask {
  const void* y = nullptr;
  const float* scale = nullptr;
  const float* shift = nullptr;
};

// Backward pass 1: the [2C] {sum g, sum g*xhat}. NCHW adds into a zeroed
// vector and has no mask-from-x variant; NHWC sums its slab in a fixed order.
template <bool R, bool MY>
inline torch::Tensor bn_bwd_stats_launch(const torch::Tensor& dy, const BnSaved& bn,
                                         const BnMask& mask, const BnGeom& geo) {
  const auto opts_f = bn.x.options().dtype(torch::kFloat);
  const int C = geo.C;
  torch::Tensor sums;
  DLA_DISPATCH_FLOAT_TYPES(bn.x.scalar_type(), "bn_bwd_stats", [&] {
    if (geo.nhwc) {
      bn_red_vec<dev_t>(C, [&](auto vtag) {
        constexpr int V = decltype(vtag)::value;
        const auto t = nhwc_red_tile(C / V, geo.rows);
        auto slab = torch::empty({t.parts, 2 * C}, opts_f);
        hipLaunchKernelGGL((bn_bwd_stats_nhwc_kernel<dev_t, V, R, MY>),
                           dim3(t.chunks, t.parts), dim3(kRedThreads), 0,
                           stream(), (const dev_t*)dy.data_ptr(),
                           (const dev_t*)bn.x.data_ptr(), (const dev_t*)mask.y,
                           mask.scale, mask.shift, bn.mean.data_ptr<float>(),
                           bn.rstd.data_ptr<float>(), slab.data_ptr<float>(), C,
                           geo.rows, t.bl, t.rb);
        sums = bn_slab_reduce_launch(slab);
      });
    } else if constexpr (!R || MY) {
      sums = torch::zeros({2 * C}, opts_f);
      hipLaunchKernelGGL((bn_bwd_stats_kernel<dev_t, R>),
                         dim3(C, nchw_ysplit(geo)), dim3(256), 0, stream(),
                         (const dev_t*)dy.data_ptr(),
                         (const dev_t*)bn.x.data_ptr(), (const dev_t*)mask.y,
                         bn.mean.data_ptr<float>(), bn.rstd.data_ptr<float>(),
                         sums.data_ptr<float>(), geo.N, C, geo.HW);
    }
  });
  return sums;
}

// Backward pass 2: dx from dy (or from the masked g, with R = false) and the
// [2C] sums.
template <bool R, bool MY>
inline torch::Tensor bn_bwd_dx_launch(const torch::Tensor& dy, const BnSaved& bn,
                                      const BnMask& mask,
                                      const torch::Tensor& sums,
                                      const BnGeom& geo) {
  auto dx = torch::empty_like(bn.x);
  const float inv_count = 1.f / (float)geo.rows;
  DLA_DISPATCH_FLOAT_TYPES(bn.x.scalar_type(), "bn_bwd_dx", [&] {
    if (geo.nhwc) {
      bn_elt_vec<dev_t>(geo.C % kVecMax<dev_t> == 0, [&](auto vtag) {
        constexpr int V = decltype(vtag)::value;
        const auto grid = nhwc_grid(geo.C / V, geo.rows);
        hipLaunchKernelGGL((bn_bwd_dx_nhwc_kernel<dev_t, V, R, MY>),
                           dim3(grid.blocks), dim3(256), 0, stream(),
                           (const dev_t*)dy.data_ptr(),
                           (const dev_t*)bn.x.data_ptr(), (const dev_t*)mask.y,
                           mask.scale, mask.shift, bn.mean.data_ptr<float>(),
                           bn.rstd.data_ptr<float>(), bn.w32.data_ptr<float>(),
                           sums.data_ptr<float>(), (dev_t*)dx.data_ptr(),
                           geo.C, geo.rows, grid.used, inv_count);
      });
    } else if constexpr (!R || MY) {
      const int64_t n_total = bn.x.numel();
      hipLaunchKernelGGL((bn_bwd_dx_kernel<dev_t, R>),
                         dim3(grid_1d(n_total, 256)), dim3(256), 0, stream(),
                         (const dev_t*)dy.data_ptr(),
                         (const dev_t*)bn.x.data_ptr(), (const dev_t*)mask.y,
                         bn.mean.data_ptr<float>(), bn.rstd.data_ptr<float>(),
                         bn.w32.data_ptr<float>(), sums.data_ptr<float>(),
                         (dev_t*)dx.data_ptr(), geo.C, geo.HW, n_total,
                         inv_count);
    }
  });
  return dx;
}

// {dx, dweight, dbias} of one BN from its dx and [2C] sums.
inline std::vector<torch::Tensor> bn_grads(const torch::Tensor& dx,
                                           const torch::Tensor& sums, int C,
                                           const torch::Tensor& weight) {
  return {dx, bn_param_grad(sums, C, C, weight),
          bn_param_grad(sums, 0, C, weight)};
}

}  // namespace dla

// Returns {y, save_mean, save_rstd, scale, shift}; scale/shift are the
// per-channel fp32 coefficients of the apply pass, which the backward's
// mask-from-x route needs again. Updates running stats in-place when given.
std::vector<torch::Tensor> batchnorm_fwd(torch::Tensor x, torch::Tensor weight,
                                         torch::Tensor bias,
                                         c10::optional<torch::Tensor> running_mean,
                                         c10::optional<torch::Tensor> running_var,
                                         double momentum, double eps, bool relu) {
  const auto geo = dla::bn_geom(x, "batchnorm_fwd", dla::BnLayout::kNchwOrNhwc);
  // converted here, ahead of the statistics kernel as before; the finalize
  // launcher's own conversion is then a no-op
  auto w32 = weight.to(torch::kFloat);
  auto b32 = bias.to(torch::kFloat);
  auto sums = dla::bn_stats_launch(x, geo);
  auto fin = dla::bn_finalize_launch(sums, w32, b32, running_mean, running_var,
                                     geo.C, geo.rows, momentum, eps);
  auto y = dla::bn_apply_launch(x, geo, fin.scale, fin.shift, relu);
  HIP_CHECK_ERR();
  return {y, fin.mean, fin.rstd, fin.scale, fin.shift};
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
  const auto geo = dla::bn_geom(x, "batchnorm_fwd_from_sums",
                                dla::BnLayout::kNchwOrNhwc);
  auto fin = dla::bn_finalize_launch(sums, weight, bias, running_mean,
                                     running_var, geo.C, geo.rows, momentum, eps);
  auto y = dla::bn_apply_launch(x, geo, fin.scale, fin.shift, relu);
  HIP_CHECK_ERR();
  return {y, fin.mean, fin.rstd, fin.scale, fin.shift};
}

// Frozen/eval BN apply (+optional ReLU): per-channel scale/shift precomputed host-side.
torch::Tensor bn_apply(torch::Tensor x, torch::Tensor scale, torch::Tensor shift,
                       bool relu) {
  const auto geo = dla::bn_geom(x, "bn_apply", dla::BnLayout::kNchwOrNhwc);
  auto y = dla::bn_apply_launch(x, geo, scale.to(torch::kFloat).contiguous(),
                                shift.to(torch::kFloat).contiguous(), relu);
  HIP_CHECK_ERR();
  return y;
}

// The one rule for where the ReLU mask of a BN(+ReLU) backward comes from:
// channels-last x takes it from x (bn_pre(x, scale, shift) > 0, no y read);
// NCHW x keeps reading the stored y. The Python autograd functions ask this
// same function in forward to decide whether y has to be saved.
bool bn_relu_mask_from_x(torch::Tensor x) { return dla::is_nhwc_not_nchw(x); }

// Returns {dx, dweight, dbias}. relu=true needs a mask source: the forward's
// scale and shift (channels-last only, see bn_relu_mask_from_x), or else y.
// When y is given it is used, so the old signature keeps its meaning.
std::vector<torch::Tensor> batchnorm_bwd_ex(
    torch::Tensor dy, torch::Tensor x, c10::optional<torch::Tensor> y,
    torch::Tensor weight, torch::Tensor mean, torch::Tensor rstd,
    c10::optional<torch::Tensor> scale, c10::optional<torch::Tensor> shift,
    bool relu) {
  DLA_CHECK_CUDA(dy);
  const auto geo = dla::bn_geom(x, "batchnorm_bwd", dla::BnLayout::kNchwOrNhwc);
  if (geo.nhwc && !dla::is_nhwc_not_nchw(dy))
    dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  if (!geo.nhwc) dy = dy.contiguous();
  auto w32 = weight.to(torch::kFloat);
  const dla::BnSaved bn{x, mean, rstd, w32};
  const bool mask_y = relu && y.has_value();
  dla::BnMask mask;
  if (relu && !mask_y) {
    TORCH_CHECK(bn_relu_mask_from_x(x) && scale.has_value() && shift.has_value(),
                "batchnorm_bwd: the relu mask needs y, or channels_last x "
                "with the forward's scale and shift");
    dla::bn_check_channels({&*scale, &*shift}, geo.C, "batchnorm_bwd", true);
    mask.scale = scale->data_ptr<float>();
    mask.shift = shift->data_ptr<float>();
  }
  if (mask_y) {
    TORCH_CHECK(y->scalar_type() == x.scalar_type() && y->sizes() == x.sizes() &&
                    (geo.nhwc ? dla::is_nhwc_not_nchw(*y) : y->is_contiguous()),
                "batchnorm_bwd: y must match x (shape, dtype, layout)");
    mask.y = y->data_ptr();
  }
  torch::Tensor sums, dx;
  // (RELU, MASK_Y) as compile-time tags: (false,false), (true,false), (true,true)
  auto run = [&](auto rtag, auto mtag) {
    constexpr bool R = decltype(rtag)::value;
    constexpr bool MY = decltype(mtag)::value;
    sums = dla::bn_bwd_stats_launch<R, MY>(dy, bn, mask, geo);
    dx = dla::bn_bwd_dx_launch<R, MY>(dy, bn, mask, sums, geo);
  };
  if (!relu) run(std::false_type{}, std::false_type{});
  else if (mask_y) run(std::true_type{}, std::true_type{});
  else run(std::true_type{}, std::false_type{});
  HIP_CHECK_ERR();
  return dla::bn_grads(dx, sums, geo.C, weight);
}

// Today's signature: the mask comes from y.
std::vector<torch::Tensor> batchnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         c10::optional<torch::Tensor> y,
                                         torch::Tensor weight, torch::Tensor mean,
                                         torch::Tensor rstd, bool relu) {
  TORCH_CHECK(!relu || y.has_value(), "batchnorm_bwd: relu mask needs y");
  return batchnorm_bwd_ex(dy, x, relu ? y : c10::nullopt, weight, mean, rstd,
                          c10::nullopt, c10::nullopt, relu);
}

// ---- fused residual join ----------------------------------------------------
namespace dla {

inline void join_check(const torch::Tensor& x, const torch::Tensor& other,
                       const char* what) {
  TORCH_CHECK(other.is_cuda() && other.scalar_type() == x.scalar_type() &&
                  other.sizes() == x.sizes() && is_nhwc_rows(other),
              "bn join: ", what, " must match x (shape, dtype, channels_last)");
}

// out = relu(bn(x) + other). fd null: other is the identity as it is; else
// other is a raw conv output and fd its finalized BN (the dual join).
inline torch::Tensor bn_add_relu_launch(const torch::Tensor& x,
                                        const BnFinalized& fin,
                                        const torch::Tensor& other,
                                        const BnFinalized* fd,
                                        const BnGeom& geo) {
  auto out = torch::empty_like(x);
  const float* scd = fd ? fd->scale.data_ptr<float>() : nullptr;
  const float* shd = fd ? fd->shift.data_ptr<float>() : nullptr;
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "bn_add_relu", [&] {
    constexpr int V = kVecMax<dev_t>;
    const auto grid = nhwc_grid(geo.C / V, geo.rows);
    auto launch = [&](auto dtag) {
      hipLaunchKernelGGL(
          (bn_add_relu_nhwc_kernel<dev_t, V, decltype(dtag)::value>),
          dim3(grid.blocks), dim3(256), 0, stream(), (const dev_t*)x.data_ptr(),
          fin.scale.data_ptr<float>(), fin.shift.data_ptr<float>(),
          (const dev_t*)other.data_ptr(), scd, shd, (dev_t*)out.data_ptr(),
          geo.C, geo.rows, grid.used);
    };
    if (fd) launch(std::true_type{});
    else launch(std::false_type{});
  });
  return out;
}

// Join backward pass 1: writes g = dy * [out > 0] and returns the [NS*C] sums
// {sum g, sum g*xhat, (dual) sum g*xhat_d}. bnd is the second BN of a dual
// join, null for the single join.
inline torch::Tensor bn_join_bwd_stats_launch(const torch::Tensor& dy,
                                              const torch::Tensor& out,
                                              const BnSaved& bn,
                                              const BnSaved* bnd,
                                              torch::Tensor& g,
                                              const BnGeom& geo) {
  const int C = geo.C;
  torch::Tensor sums;
  DLA_DISPATCH_FLOAT_TYPES(bn.x.scalar_type(), "bn_join_bwd_stats", [&] {
    constexpr int V = kVecMax<dev_t>;
    const dev_t* xd = bnd ? (const dev_t*)bnd->x.data_ptr() : nullptr;
    const float* mean_d = bnd ? bnd->mean.data_ptr<float>() : nullptr;
    const float* rstd_d = bnd ? bnd->rstd.data_ptr<float>() : nullptr;
    const auto t = nhwc_red_tile(C / V, geo.rows);
    auto slab = torch::empty({t.parts, (bnd ? 3 : 2) * C},
                             bn.x.options().dtype(torch::kFloat));
    auto launch = [&](auto dtag) {
      hipLaunchKernelGGL(
          (bn_join_bwd_stats_nhwc_kernel<dev_t, V, decltype(dtag)::value>),
          dim3(t.chunks, t.parts), dim3(kRedThreads), 0, stream(),
          (const dev_t*)dy.data_ptr(), (const dev_t*)out.data_ptr(),
          (const dev_t*)bn.x.data_ptr(), bn.mean.data_ptr<float>(),
          bn.rstd.data_ptr<float>(), xd, mean_d, rstd_d, (dev_t*)g.data_ptr(),
          slab.data_ptr<float>(), C, geo.rows, t.bl, t.rb);
    };
    if (bnd) launch(std::true_type{});
    else launch(std::false_type{});
    sums = bn_slab_reduce_launch(slab);
  });
  return sums;
}

// Dual join backward pass 2: {dx, dxd} from one read of g and the [3C] sums.
inline std::pair<torch::Tensor, torch::Tensor> bn_join_dual_dx_launch(
    const torch::Tensor& g, const BnSaved& bn, const BnSaved& bnd,
    const torch::Tensor& sums, const BnGeom& geo) {
  auto dx = torch::empty_like(bn.x);
  auto dxd = torch::empty_like(bn.x);
  DLA_DISPATCH_FLOAT_TYPES(bn.x.scalar_type(), "bn_join_dual_dx", [&] {
    constexpr int V = kVecMax<dev_t>;
    const auto grid = nhwc_grid(geo.C / V, geo.rows);
    hipLaunchKernelGGL((bn_join_bwd_dx_dual_nhwc_kernel<dev_t, V>),
                       dim3(grid.blocks), dim3(256), 0, stream(),
                       (const dev_t*)g.data_ptr(), (const dev_t*)bn.x.data_ptr(),
                       (const dev_t*)bnd.x.data_ptr(), bn.mean.data_ptr<float>(),
                       bn.rstd.data_ptr<float>(), bn.w32.data_ptr<float>(),
                       bnd.mean.data_ptr<float>(), bnd.rstd.data_ptr<float>(),
                       bnd.w32.data_ptr<float>(), sums.data_ptr<float>(),
                       (dev_t*)dx.data_ptr(), (dev_t*)dxd.data_ptr(), geo.C,
                       geo.rows, grid.used, 1.f / (float)geo.rows);
  });
  return {dx, dxd};
}

// {dx, dxd, dweight, dbias, dweight_d, dbias_d} of a dual join from its [3C]
// sums. sum g serves both biases, but two parameters must not share gradient
// storage (optimizers update .grad in place): the second gets a copy.
inline std::vector<torch::Tensor> dual_grads(
    const std::pair<torch::Tensor, torch::Tensor>& dxs,
    const torch::Tensor& sums, int C, const torch::Tensor& weight,
    const torch::Tensor& weight_d) {
  auto dbias = bn_param_grad(sums, 0, C, weight);
  return {dxs.first, dxs.second, bn_param_grad(sums, C, C, weight), dbias,
          bn_param_grad(sums, 2 * C, C, weight_d),
          dbias.to(weight_d.scalar_type()).clone()};
}

}  // namespace dla

// out = relu(bn(x) + identity), BN finalized from the conv-fused sums
// ([2C] or [n_parts, 2C]). Returns {out, save_mean, save_rstd}.
std::vector<torch::Tensor> bn_add_relu_fwd_from_sums(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor sums, c10::optional<torch::Tensor> running_mean,
    c10::optional<torch::Tensor> running_var, double momentum, double eps,
    torch::Tensor identity) {
  const auto geo = dla::bn_geom(x, "bn_add_relu", dla::BnLayout::kNhwcRows);
  dla::join_check(x, identity, "identity");
  auto fin = dla::bn_finalize_launch(sums, weight, bias, running_mean,
                                     running_var, geo.C, geo.rows, momentum, eps);
  auto out = dla::bn_add_relu_launch(x, fin, identity, nullptr, geo);
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
  const auto geo = dla::bn_geom(x, "bn_add_relu_dual", dla::BnLayout::kNhwcRows);
  dla::join_check(x, xd, "xd");
  auto fin = dla::bn_finalize_launch(sums, weight, bias, running_mean,
                                     running_var, geo.C, geo.rows, momentum, eps);
  auto fd = dla::bn_finalize_launch(sums_d, weight_d, bias_d, running_mean_d,
                                    running_var_d, geo.C, geo.rows, momentum_d,
                                    eps_d);
  auto out = dla::bn_add_relu_launch(x, fin, xd, &fd, geo);
  HIP_CHECK_ERR();
  return {out, fin.mean, fin.rstd, fd.mean, fd.rstd};
}

// Backward of the single join. Returns {g, dx, dweight, dbias}; g = dy*[out>0]
// is the identity gradient itself (not a copy).
std::vector<torch::Tensor> bn_add_relu_bwd(torch::Tensor dy, torch::Tensor out,
                                           torch::Tensor x, torch::Tensor weight,
                                           torch::Tensor mean,
                                           torch::Tensor rstd) {
  const auto geo = dla::bn_geom(x, "bn_add_relu_bwd", dla::BnLayout::kNhwcRows);
  dla::join_check(x, out, "out");
  if (!dla::is_nhwc_rows(dy)) dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  dla::join_check(x, dy, "dy");
  dla::bn_check_channels({&mean, &rstd, &weight}, geo.C, "bn_add_relu_bwd");
  auto g = torch::empty_like(x);
  auto w32 = weight.to(torch::kFloat).contiguous();
  const dla::BnSaved bn{x, mean, rstd, w32};
  auto sums = dla::bn_join_bwd_stats_launch(dy, out, bn, nullptr, g, geo);
  // the mask is in g already: the plain dx pass without ReLU
  auto dx = dla::bn_bwd_dx_launch<false, false>(g, bn, {}, sums, geo);
  HIP_CHECK_ERR();
  return {g, dx, dla::bn_param_grad(sums, geo.C, geo.C, weight),
          dla::bn_param_grad(sums, 0, geo.C, weight)};
}

// Backward of the dual join. Returns {dx, dxd, dweight, dbias, dweight_d,
// dbias_d}; sum g is shared, so dbias_d holds the same values as dbias.
std::vector<torch::Tensor> bn_add_relu_dual_bwd(
    torch::Tensor dy, torch::Tensor out, torch::Tensor x, torch::Tensor weight,
    torch::Tensor mean, torch::Tensor rstd, torch::Tensor xd,
    torch::Tensor weight_d, torch::Tensor mean_d, torch::Tensor rstd_d) {
  const auto geo = dla::bn_geom(x, "bn_add_relu_dual_bwd",
                                dla::BnLayout::kNhwcRows);
  dla::join_check(x, out, "out");
  dla::join_check(x, xd, "xd");
  if (!dla::is_nhwc_rows(dy)) dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  dla::join_check(x, dy, "dy");
  dla::bn_check_channels({&mean, &rstd, &weight, &mean_d, &rstd_d, &weight_d},
                         geo.C, "bn_add_relu_dual_bwd");
  auto g = torch::empty_like(x);
  auto w32 = weight.to(torch::kFloat).contiguous();
  auto wd32 = weight_d.to(torch::kFloat).contiguous();
  const dla::BnSaved bn{x, mean, rstd, w32}, bnd{xd, mean_d, rstd_d, wd32};
  auto sums = dla::bn_join_bwd_stats_launch(dy, out, bn, &bnd, g, geo);
  auto dxs = dla::bn_join_dual_dx_launch(g, bn, bnd, sums, geo);
  HIP_CHECK_ERR();
  return dla::dual_grads(dxs, sums, geo.C, weight, weight_d);
}

// ---- dx-only backward: pass 1 ran in the conv1x1 dgrad epilogue -------------
// g is the masked gradient that epilogue stored and slab its [n_parts, NS*C]
// partial sums (conv1x1_dgrad_bwdstats), so what is left is the slab reduce
// and the dx pass. Serves BatchNorm(+ReLU) and the single join alike: with the
// mask already in g both are bn_bwd_dx_nhwc_kernel<.., false>. The epilogue
// is bf16, so these entries are bf16 with V = 8.
namespace dla {

inline void dx_only_check(const torch::Tensor& x, const torch::Tensor& g,
                          const torch::Tensor& slab, int ns) {
  join_check(x, g, "g");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "bn dx-only: bf16 only");
  TORCH_CHECK(slab.is_cuda() && slab.scalar_type() == torch::kFloat &&
                  slab.dim() == 2 && slab.is_contiguous() &&
                  slab.size(0) >= 1 && slab.size(1) == ns * x.size(1),
              "bn dx-only: slab must be fp32 [n_parts, ", ns, "*C]");
}

}  // namespace dla

// The fixed-order column sum of a [n_parts, n_cols] fp32 slab on its own
// (what the dx-only entries run first), for tests and timing.
torch::Tensor bn_slab_reduce(torch::Tensor slab) {
  TORCH_CHECK(slab.is_cuda() && slab.scalar_type() == torch::kFloat &&
                  slab.dim() == 2 && slab.is_contiguous() && slab.size(0) >= 1,
              "bn_slab_reduce: slab must be a contiguous fp32 [n_parts, n_cols] "
              "GPU tensor");
  auto sums = dla::bn_slab_reduce_launch(slab);
  HIP_CHECK_ERR();
  return sums;
}

// Returns {dx, dweight, dbias}.
std::vector<torch::Tensor> bn_bwd_dx_from_slab(torch::Tensor g,
                                               torch::Tensor slab,
                                               torch::Tensor x,
                                               torch::Tensor weight,
                                               torch::Tensor mean,
                                               torch::Tensor rstd) {
  const auto geo = dla::bn_geom(x, "bn_bwd_dx_from_slab",
                                dla::BnLayout::kNhwcRows);
  dla::dx_only_check(x, g, slab, 2);
  dla::bn_check_channels({&mean, &rstd, &weight}, geo.C, "bn_bwd_dx_from_slab");
  auto w32 = weight.to(torch::kFloat).contiguous();
  auto sums = dla::bn_slab_reduce_launch(slab);
  auto dx = dla::bn_bwd_dx_launch<false, false>(g, {x, mean, rstd, w32}, {},
                                                sums, geo);
  HIP_CHECK_ERR();
  return dla::bn_grads(dx, sums, geo.C, weight);
}

// Dual join. Returns {dx, dxd, dweight, dbias, dweight_d, dbias_d}.
std::vector<torch::Tensor> bn_join_dual_bwd_dx_from_slab(
    torch::Tensor g, torch::Tensor slab, torch::Tensor x, torch::Tensor weight,
    torch::Tensor mean, torch::Tensor rstd, torch::Tensor xd,
    torch::Tensor weight_d, torch::Tensor mean_d, torch::Tensor rstd_d) {
  const auto geo = dla::bn_geom(x, "bn_join_dual_bwd_dx_from_slab",
                                dla::BnLayout::kNhwcRows);
  dla::dx_only_check(x, g, slab, 3);
  dla::join_check(x, xd, "xd");
  dla::bn_check_channels({&mean, &rstd, &weight, &mean_d, &rstd_d, &weight_d},
                         geo.C, "bn_join_dual_bwd_dx_from_slab");
  auto w32 = weight.to(torch::kFloat).contiguous();
  auto wd32 = weight_d.to(torch::kFloat).contiguous();
  auto sums = dla::bn_slab_reduce_launch(slab);
  auto dxs = dla::bn_join_dual_dx_launch(g, {x, mean, rstd, w32},
                                         {xd, mean_d, rstd_d, wd32}, sums, geo);
  HIP_CHECK_ERR();
  return dla::dual_grads(dxs, sums, geo.C, weight, weight_d);
}

// ---- fused stem: BN apply + ReLU + 3x3 / stride 2 / pad 1 max-pool ----------
// pooled = max_pool(T(relu(bn_pre(x)))) over the raw conv output x (NHWC), T
// the rounding to the storage type. The BN output y is never written: rounding
// and ReLU are monotone, so the maximum of the rounded values is the value the
// unfused route pools, bit for bit. Instead of aten's int64 indices the kernel
// keeps one uint8 slot (kh*3 + kw, 0..8) per pooled element: the first maximum
// in row-major window order wins (aten's `val > maxval`), padding positions
// never take part.
namespace dla {

constexpr int kPoolRun = 8;  // consecutive output rows of one image per block

// One block owns kPoolRun consecutive output rows of one image, so the input
// rows that neighbouring windows share are re-read from this CU's caches and
// only the one row shared with the next run is fetched twice.
template <typename dev_t, int V>
__global__ void __launch_bounds__(256)
bn_relu_maxpool_fwd_nhwc_kernel(const dev_t* __restrict__ x,
                                const float* __restrict__ scale,
                                const float* __restrict__ shift,
                                dev_t* __restrict__ out,
                                uint8_t* __restrict__ slots, int C, int H,
                                int W, int OH, int OW, int runs_per_img) {
  const int n = blockIdx.x / runs_per_img;
  const int oh0 = (blockIdx.x % runs_per_img) * kPoolRun;
  const int oh1 = min(oh0 + kPoolRun, OH);
  const int lanes = C / V;
  const int items = (oh1 - oh0) * OW * lanes;
  const dev_t* xn = x + (int64_t)n * H * W * C;
  const int64_t obase = ((int64_t)n * OH + oh0) * OW * C;
  for (int i = threadIdx.x; i < items; i += blockDim.x) {
    const int c0 = (i % lanes) * V;
    const int p = i / lanes;  // output pixel within the run
    const int ow = p % OW, oh = oh0 + p / OW;
    float sc[V], sh[V], best[V];
    int slot[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      sc[j] = scale[c0 + j];
      sh[j] = shift[c0 + j];
      best[j] = -INFINITY;
      slot[j] = 4;  // the window centre is always inside the image
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = 2 * oh - 1 + kh;
      if (ih < 0 || ih >= H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = 2 * ow - 1 + kw;
        if (iw < 0 || iw >= W) continue;
        Vec<dev_t, V> xv =
            vload<dev_t, V>(xn + ((int64_t)ih * W + iw) * C + c0);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float f = bn_pre(to_f32(xv.v[j]), sc[j], sh[j]);
          const float y = to_f32(from_f32<dev_t>(fmaxf(f, 0.f)));
          if (y > best[j]) {
            best[j] = y;
            slot[j] = kh * 3 + kw;
          }
        }
      }
    }
    Vec<dev_t, V> ov;
    Vec<uint8_t, V> sv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      ov.v[j] = from_f32<dev_t>(best[j]);  // exact: best is a dev_t value
      sv.v[j] = (uint8_t)slot[j];
    }
    const int64_t o = obase + (int64_t)p * C + c0;
    vstore<dev_t, V>(out + o, ov);
    vstore<uint8_t, V>(slots + o, sv);
  }
}

// Gradient reaching the BN output at input position (n, h, w), channels
// c0..c0+V-1, in fp32: the dpool values of the at most four windows that
// cover (h, w) and whose slot points at it, summed in the fixed order (oh, ow)
// ascending, then zeroed under the ReLU mask taken from x. Both backward
// kernels gather through this function, so neither writes a full-size g and
// nothing is scattered with atomics.
template <typename dev_t, int V>
__device__ __forceinline__ void stem_pool_grad(
    const dev_t* __restrict__ dpool, const uint8_t* __restrict__ slots,
    const Vec<dev_t, V>& xv, const float* sc, const float* sh, int n, int h,
    int w, int c0, int C, int OH, int OW, float* g) {
#pragma unroll
  for (int j = 0; j < V; ++j) g[j] = 0.f;
  // rows/columns 2k are covered by window k only, 2k+1 by windows k and k+1
  const int oh_hi = min((h + 1) >> 1, OH - 1);
  const int ow_hi = min((w + 1) >> 1, OW - 1);
  for (int oh = h >> 1; oh <= oh_hi; ++oh) {
    const int kh = h - 2 * oh + 1;
    for (int ow = w >> 1; ow <= ow_hi; ++ow) {
      const int want = kh * 3 + (w - 2 * ow + 1);
      const int64_t o = (((int64_t)n * OH + oh) * OW + ow) * C + c0;
      Vec<uint8_t, V> sv = vload<uint8_t, V>(slots + o);
      Vec<dev_t, V> dv = vload<dev_t, V>(dpool + o);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if ((int)sv.v[j] == want) g[j] += to_f32(dv.v[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j)
    if (!(bn_pre(to_f32(xv.v[j]), sc[j], sh[j]) > 0.f)) g[j] = 0.f;
}

// Backward pass 1: sum g, sum g*xhat per channel; thread mapping and the
// slab tail are bn_bwd_stats_nhwc_kernel's. The gathers of stem_pool_grad
// depend on one another, so this kernel waits on latency, not on bandwidth:
// no row unroll and no occupancy cap (fewer registers, more waves), and a
// grid of kStemRedBlocks blocks.
constexpr int kStemRedBlocks = 1024;

template <typename dev_t, int V>
__global__ void __launch_bounds__(kRedThreads)
bn_relu_maxpool_bwd_stats_nhwc_kernel(
    const dev_t* __restrict__ dpool, const uint8_t* __restrict__ slots,
    const dev_t* __restrict__ x, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ slab, int C, int H,
    int W, int OH, int OW, int64_t rows, int bl, int rb) {
  const NhwcRedPos p = nhwc_red_pos<V>(C, bl, rb);
  float mu[V], rs[V], sc[V], sh[V];
  float acc[2][V];  // sum g, sum g*xhat
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = p.active ? mean[p.c0 + j] : 0.f;
    rs[j] = p.active ? rstd[p.c0 + j] : 0.f;
    sc[j] = p.active ? scale[p.c0 + j] : 0.f;
    sh[j] = p.active ? shift[p.c0 + j] : 0.f;
    acc[0][j] = 0.f;
    acc[1][j] = 0.f;
  }
  nhwc_red_rows<1>(
      p, rows, [&](int64_t r) { return vload<dev_t, V>(x + r * C + p.c0); },
      [&](int64_t r, const Vec<dev_t, V>& xv) {
        const uint32_t r32 = (uint32_t)r;  // rows < 2^31 (checked by the host)
        const uint32_t q = r32 / (uint32_t)W;
        const int w = (int)(r32 - q * (uint32_t)W);
        const int n = (int)(q / (uint32_t)H);
        const int h = (int)(q - (uint32_t)n * (uint32_t)H);
        float g[V];
        stem_pool_grad<dev_t, V>(dpool, slots, xv, sc, sh, n, h, w, p.c0, C,
                                 OH, OW, g);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float xh = (to_f32(xv.v[j]) - mu[j]) * rs[j];
          acc[0][j] += g[j];
          acc[1][j] += g[j] * xh;
        }
      });
  nhwc_red_tail<V, 2>(acc, slab, C, bl, rb);
}

// Backward pass 2: dx = weight*rstd*(g - mean(g) - xhat*mean(g*xhat)).
template <typename dev_t, int V>
__global__ void bn_relu_maxpool_bwd_dx_nhwc_kernel(
    const dev_t* __restrict__ dpool, const uint8_t* __restrict__ slots,
    const dev_t* __restrict__ x, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ weight,
    const float* __restrict__ sums, dev_t* __restrict__ dx, int C, int H,
    int W, int OH, int OW, int64_t rows, int64_t used, float inv_count) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= used) return;
  const int lanes_per_row = C / V;
  const int c0 = (int)(t % lanes_per_row) * V;
  const int64_t rstride = used / lanes_per_row;
  float mu[V], rs[V], wr[V], sc[V], sh[V], m_g[V], m_gxh[V], g[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = mean[c0 + j];
    rs[j] = rstd[c0 + j];
    wr[j] = weight[c0 + j] * rs[j];
    sc[j] = scale[c0 + j];
    sh[j] = shift[c0 + j];
    m_g[j] = sums[c0 + j] * inv_count;
    m_gxh[j] = sums[C + c0 + j] * inv_count;
  }
  for (int64_t r = t / lanes_per_row; r < rows; r += rstride) {
    const uint32_t r32 = (uint32_t)r;  // rows < 2^31 (checked by the host)
    const uint32_t q = r32 / (uint32_t)W;
    const int w = (int)(r32 - q * (uint32_t)W);
    const int n = (int)(q / (uint32_t)H);
    const int h = (int)(q - (uint32_t)n * (uint32_t)H);
    Vec<dev_t, V> xv = vload<dev_t, V>(x + r * C + c0);
    stem_pool_grad<dev_t, V>(dpool, slots, xv, sc, sh, n, h, w, c0, C, OH, OW,
                             g);
    Vec<dev_t, V> dxv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float xh = (to_f32(xv.v[j]) - mu[j]) * rs[j];
      dxv.v[j] = from_f32<dev_t>(wr[j] * (g[j] - m_g[j] - xh * m_gxh[j]));
    }
    vstore<dev_t, V>(dx + r * C + c0, dxv);
  }
}

// x of a stem entry (the stem kernels index rows with 32 bits).
inline BnGeom stem_geom(const torch::Tensor& x, const char* fn) {
  const auto geo = bn_geom(x, fn, BnLayout::kNhwcRows);
  TORCH_CHECK(x.numel() > 0 && geo.rows < (int64_t(1) << 31), fn,
              ": N*H*W must be in [1, 2^31)");
  return geo;
}

}  // namespace dla

// Train-mode stem. Returns {pooled, slots (uint8), mean, rstd, scale, shift};
// running stats are updated in place when given.
std::vector<torch::Tensor> bn_relu_maxpool_fwd(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    c10::optional<torch::Tensor> running_mean,
    c10::optional<torch::Tensor> running_var, double momentum, double eps) {
  const auto geo = dla::stem_geom(x, "bn_relu_maxpool_fwd");
  const int N = geo.N, C = geo.C, H = geo.H, W = geo.W;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  auto out_opts = x.options().memory_format(at::MemoryFormat::ChannelsLast);
  auto pooled = torch::empty({N, C, OH, OW}, out_opts);
  auto slots = torch::empty({N, C, OH, OW}, out_opts.dtype(torch::kByte));
  const int runs = (OH + dla::kPoolRun - 1) / dla::kPoolRun;
  TORCH_CHECK((int64_t)N * runs < (int64_t(1) << 31),
              "bn_relu_maxpool_fwd: too many blocks");
  auto sums = dla::bn_stats_launch(x, geo);
  auto fin = dla::bn_finalize_launch(sums, weight, bias, running_mean,
                                     running_var, C, geo.rows, momentum, eps);
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "bn_relu_maxpool_fwd", [&] {
    constexpr int V = dla::kVecMax<dev_t>;
    hipLaunchKernelGGL((dla::bn_relu_maxpool_fwd_nhwc_kernel<dev_t, V>),
                       dim3(N * runs), dim3(256), 0, dla::stream(),
                       (const dev_t*)x.data_ptr(), fin.scale.data_ptr<float>(),
                       fin.shift.data_ptr<float>(), (dev_t*)pooled.data_ptr(),
                       slots.data_ptr<uint8_t>(), C, H, W, OH, OW, runs);
  });
  HIP_CHECK_ERR();
  return {pooled, slots, fin.mean, fin.rstd, fin.scale, fin.shift};
}

// Returns {dx, dweight, dbias} as batchnorm_bwd does.
std::vector<torch::Tensor> bn_relu_maxpool_bwd(
    torch::Tensor dpool, torch::Tensor x, torch::Tensor slots,
    torch::Tensor weight, torch::Tensor mean, torch::Tensor rstd,
    torch::Tensor scale, torch::Tensor shift) {
  const char* fn = "bn_relu_maxpool_bwd";
  const auto geo = dla::stem_geom(x, fn);
  const int N = geo.N, C = geo.C, H = geo.H, W = geo.W;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const int64_t rows = geo.rows;
  DLA_CHECK_CUDA(dpool);
  if (!dla::is_nhwc_rows(dpool))
    dpool = dpool.contiguous(at::MemoryFormat::ChannelsLast);
  const std::vector<int64_t> pshape{N, C, OH, OW};
  TORCH_CHECK(dpool.scalar_type() == x.scalar_type() &&
                  dpool.sizes() == at::IntArrayRef(pshape),
              fn, ": dpool must be [N, C, OH, OW] of x's dtype");
  TORCH_CHECK(slots.is_cuda() && slots.scalar_type() == torch::kByte &&
                  slots.sizes() == at::IntArrayRef(pshape) &&
                  dla::is_nhwc_rows(slots),
              fn, ": slots must be channels_last uint8 [N, C, OH, OW]");
  dla::bn_check_channels({&mean, &rstd, &scale, &shift}, C, fn, true);
  dla::bn_check_channels({&weight}, C, fn);
  torch::Tensor sums;
  auto dx = torch::empty_like(x);
  auto w32 = weight.to(torch::kFloat).contiguous();
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "bn_relu_maxpool_bwd", [&] {
    constexpr int V = dla::kVecMax<dev_t>;
    const auto t = dla::nhwc_red_tile(C / V, rows, dla::kStemRedBlocks,
                                      dla::kStemRedBlocks);
    auto slab = torch::empty({t.parts, 2 * C},
                             x.options().dtype(torch::kFloat));
    hipLaunchKernelGGL((dla::bn_relu_maxpool_bwd_stats_nhwc_kernel<dev_t, V>),
                       dim3(t.chunks, t.parts), dim3(dla::kRedThreads), 0,
                       dla::stream(), (const dev_t*)dpool.data_ptr(),
                       slots.data_ptr<uint8_t>(), (const dev_t*)x.data_ptr(),
                       scale.data_ptr<float>(), shift.data_ptr<float>(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       slab.data_ptr<float>(), C, H, W, OH, OW, rows, t.bl,
                       t.rb);
    sums = dla::bn_slab_reduce_launch(slab);
    const auto grid = dla::nhwc_grid(C / V, rows);
    hipLaunchKernelGGL((dla::bn_relu_maxpool_bwd_dx_nhwc_kernel<dev_t, V>),
                       dim3(grid.blocks), dim3(256), 0, dla::stream(),
                       (const dev_t*)dpool.data_ptr(), slots.data_ptr<uint8_t>(),
                       (const dev_t*)x.data_ptr(), scale.data_ptr<float>(),
                       shift.data_ptr<float>(), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), w32.data_ptr<float>(),
                       sums.data_ptr<float>(), (dev_t*)dx.data_ptr(), C, H, W,
                       OH, OW, rows, grid.used, 1.f / (float)rows);
  });
  HIP_CHECK_ERR();
  return dla::bn_grads(dx, sums, C, weight);
}
