// Fused per-pixel cross-entropy for dense prediction (segmentation):
// logits [B, C, *spatial] (P pixels per image), int64 target [B, *spatial],
// optional per-class weight, ignore_index, reduction none / sum / mean.
//
//   forward : one pass over the logits -> lse per pixel (fp32, saved) and
//             loss = w[t] * (lse - z_t)
//   backward: one pass -> dlogits = w[t] * (softmax - onehot) * g, written in
//             the logits' dtype and memory layout
//
// Two native layouts, no layout copy:
//   NCHW ([B, C, P] contiguous): a lane owns V adjacent pixels and walks the C
//     planes with an online max/sum; adjacent lanes read adjacent pixels. V
//     is the widest of 16/8/4-byte accesses that P and the pointers allow
//     (every plane start is then aligned); V = 1 is the scalar path.
//   channels_last ([B, P, C]): a block stages TP pixels x C contiguous
//     elements with 16-byte coalesced loads into LDS, one lane then reads its
//     pixel's row. The LDS row stride is padded to an odd number of dwords so
//     the lane-per-pixel ds_read_b32 are conflict-free. Backward writes the
//     row back in place and the block streams the tile out the same way.
//
// A target equal to ignore_index or outside [0, C) contributes nothing and
// gets a zero gradient; a label is range-checked before it indexes anything.
//
// sum / mean: every block stores {loss_sum, weight_sum} into its own row of
// an uninitialised slab and a one-block kernel adds the rows in a fixed
// order: no atomics, no zero fill, bit-reproducible. mean divides by the
// summed weight of the valid pixels (0 -> loss 0, gradient 0). Backward
// reads the upstream grad and that denominator from device memory, so there
// is no host synchronisation and the op can be captured into a hipGraph.
#include <cfloat>
#include <climits>
#include <type_traits>

#include "common.h"
#include "vec.h"

namespace dla {

constexpr int kDceBlock = 256;
constexpr int kDceMaxClNhwc = 256;

enum DceReduction { kDceNone = 0, kDceSum = 1, kDceMean = 2 };

// One step of the online log-sum-exp with a single exp per element: the
// running sum s is kept relative to the running max m. m starts at -FLT_MAX
// (not -inf) so a leading -inf logit gives d = -inf, e = 0 and not inf - inf.
__device__ __forceinline__ void dce_lse_step(float z, float& m, float& s) {
  const float d = z - m;
  const float e = __expf(-fabsf(d));
  s = d > 0.f ? fmaf(s, e, 1.f) : s + e;
  m = fmaxf(m, z);
}

// class id if the label takes part in the loss, -1 otherwise
__device__ __forceinline__ int dce_label(int64_t t, int C, int64_t ignore) {
  return (t >= 0 && t < (int64_t)C && t != ignore) ? (int)t : -1;
}

// V consecutive elements through accesses of at most 16 bytes. p must be
// aligned to min(16, V * sizeof(T)) bytes.
template <typename T, int V>
__device__ __forceinline__ void dce_load_run(const T* p, T (&out)[V]) {
  constexpr int K = (V * sizeof(T) > 16) ? 16 / (int)sizeof(T) : V;
#pragma unroll
  for (int i = 0; i < V / K; ++i) {
    const Vec<T, K> v = vload<T, K>(p + i * K);
#pragma unroll
    for (int k = 0; k < K; ++k) out[i * K + k] = v.v[k];
  }
}

template <typename T, int V>
__device__ __forceinline__ void dce_store_run(T* p, const T (&in)[V]) {
  constexpr int K = (V * sizeof(T) > 16) ? 16 / (int)sizeof(T) : V;
#pragma unroll
  for (int i = 0; i < V / K; ++i) {
    Vec<T, K> v;
#pragma unroll
    for (int k = 0; k < K; ++k) v.v[k] = in[i * K + k];
    vstore<T, K>(p + i * K, v);
  }
}

// this block's {loss_sum, weight_sum} -> its slab row, plain stores
__device__ __forceinline__ void dce_store_partial(float* slab, float ls,
                                                  float ws, float* smem) {
  ls = block_reduce_sum(ls, smem);
  ws = block_reduce_sum(ws, smem);
  if (threadIdx.x == 0) {
    slab[2 * (int64_t)blockIdx.x + 0] = ls;
    slab[2 * (int64_t)blockIdx.x + 1] = ws;
  }
}

// stats = {loss, denominator}; rows added in a fixed order by one block
__global__ __launch_bounds__(kDceBlock)
void dce_finalize_kernel(const float* __restrict__ slab, int rows,
                         float* __restrict__ stats, int mean) {
  __shared__ float smem[16];
  float ls = 0.f, ws = 0.f;
  for (int r = threadIdx.x; r < rows; r += kDceBlock) {
    ls += slab[2 * r + 0];
    ws += slab[2 * r + 1];
  }
  ls = block_reduce_sum(ls, smem);
  ws = block_reduce_sum(ws, smem);
  if (threadIdx.x == 0) {
    stats[0] = mean ? (ws > 0.f ? ls / ws : 0.f) : ls;
    stats[1] = ws;
  }
}

// grad scale of the reduced losses, read from device memory
__device__ __forceinline__ float dce_scalar_grad(const float* gin,
                                                 const float* stats, int mean) {
  float g = gin[0];
  if (mean) {
    const float d = stats[1];
    g = d > 0.f ? g / d : 0.f;
  }
  return g;
}

// ---- NCHW --------------------------------------------------------------------
// item = V adjacent pixels of one image; V divides P.
template <typename dev_t, int V>
__global__ __launch_bounds__(kDceBlock)
void dce_fwd_nchw_kernel(const dev_t* __restrict__ logits,
                         const int64_t* __restrict__ target,
                         const float* __restrict__ weight,
                         float* __restrict__ lse_out,
                         float* __restrict__ loss_out,  // none only
                         float* __restrict__ slab,      // sum / mean only
                         int64_t B, int C, int64_t P, int64_t ignore) {
  __shared__ float smem[16];
  const int64_t G = P / V;
  const int64_t items = B * G;
  float ls = 0.f, ws = 0.f;
  for (int64_t it = (int64_t)blockIdx.x * kDceBlock + threadIdx.x; it < items;
       it += (int64_t)gridDim.x * kDceBlock) {
    const int64_t b = it / G;
    const int64_t p0 = (it - b * G) * V;
    const int64_t n0 = b * P + p0;
    int64_t traw[V];
    dce_load_run<int64_t, V>(target + n0, traw);
    int tt[V];
    float m[V], s[V], zt[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      tt[j] = dce_label(traw[j], C, ignore);
      m[j] = -FLT_MAX;
      s[j] = 0.f;
      zt[j] = 0.f;
    }
    const dev_t* src = logits + b * (int64_t)C * P + p0;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
      const Vec<dev_t, V> zv = vload<dev_t, V>(src + (int64_t)c * P);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float z = to_f32(zv.v[j]);
        dce_lse_step(z, m[j], s[j]);
        if (c == tt[j]) zt[j] = z;
      }
    }
    float lse[V], loss[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float lg = __logf(s[j]);
      lse[j] = m[j] + lg;
      const bool valid = tt[j] >= 0;
      const float w = valid ? (weight != nullptr ? weight[tt[j]] : 1.f) : 0.f;
      // (m - z_t) + log(s): no cancellation against a large lse
      loss[j] = valid ? w * ((m[j] - zt[j]) + lg) : 0.f;
      ls += loss[j];
      ws += w;
    }
    dce_store_run<float, V>(lse_out + n0, lse);
    if (loss_out != nullptr) dce_store_run<float, V>(loss_out + n0, loss);
  }
  if (slab != nullptr) dce_store_partial(slab, ls, ws, smem);
}

template <typename dev_t, int V, bool PER_PIXEL>
__global__ __launch_bounds__(kDceBlock)
void dce_bwd_nchw_kernel(const dev_t* __restrict__ logits,
                         const int64_t* __restrict__ target,
                         const float* __restrict__ weight,
                         const float* __restrict__ lse,
                         const float* __restrict__ gin,    // [1] or per pixel
                         const float* __restrict__ stats,  // mean only
                         dev_t* __restrict__ dlogits, int64_t B, int C,
                         int64_t P, int64_t ignore, int mean) {
  const int64_t G = P / V;
  const int64_t items = B * G;
  const float gs = PER_PIXEL ? 0.f : dce_scalar_grad(gin, stats, mean);
  for (int64_t it = (int64_t)blockIdx.x * kDceBlock + threadIdx.x; it < items;
       it += (int64_t)gridDim.x * kDceBlock) {
    const int64_t b = it / G;
    const int64_t p0 = (it - b * G) * V;
    const int64_t n0 = b * P + p0;
    int64_t traw[V];
    dce_load_run<int64_t, V>(target + n0, traw);
    float l[V], g[V];
    dce_load_run<float, V>(lse + n0, l);
    if (PER_PIXEL) dce_load_run<float, V>(gin + n0, g);
    int tt[V];
    float coef[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      tt[j] = dce_label(traw[j], C, ignore);
      const float w =
          tt[j] >= 0 ? (weight != nullptr ? weight[tt[j]] : 1.f) : 0.f;
      coef[j] = w * (PER_PIXEL ? g[j] : gs);
    }
    const int64_t off = b * (int64_t)C * P + p0;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
      const Vec<dev_t, V> zv = vload<dev_t, V>(logits + off + (int64_t)c * P);
      Vec<dev_t, V> out;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float p = __expf(to_f32(zv.v[j]) - l[j]);
        const float d = coef[j] * (p - (c == tt[j] ? 1.f : 0.f));
        out.v[j] = from_f32<dev_t>(tt[j] >= 0 ? d : 0.f);
      }
      vstore<dev_t, V>(dlogits + off + (int64_t)c * P, out);
    }
  }
}

// ---- channels_last -----------------------------------------------------------
// Tile = TP pixels x C elements, contiguous in global memory; in LDS row r
// starts at element r * Cp. A 16-byte chunk may straddle rows, so elements
// are placed one by one while (row, col) is stepped along the chunk.
template <typename dev_t, int TP>
__device__ __forceinline__ void dce_tile_in(const dev_t* __restrict__ src,
                                            dev_t* tile, int nE, int C, int Cp,
                                            bool vec_ok) {
  constexpr int VL = 16 / (int)sizeof(dev_t);
  const int nchunks = (nE + VL - 1) / VL;
  for (int ch = threadIdx.x; ch < nchunks; ch += TP) {
    const int e = ch * VL;
    dev_t vals[VL];
    if (vec_ok && e + VL <= nE) {
      const Vec<dev_t, VL> v = vload<dev_t, VL>(src + e);
#pragma unroll
      for (int k = 0; k < VL; ++k) vals[k] = v.v[k];
    } else {
#pragma unroll
      for (int k = 0; k < VL; ++k)
        vals[k] = e + k < nE ? src[e + k] : from_f32<dev_t>(0.f);
    }
    int row = e / C;
    int col = e - row * C;
#pragma unroll
    for (int k = 0; k < VL; ++k) {
      if (e + k < nE) tile[row * Cp + col] = vals[k];
      if (++col == C) {
        col = 0;
        ++row;
      }
    }
  }
}

template <typename dev_t, int TP>
__device__ __forceinline__ void dce_tile_out(dev_t* __restrict__ dst,
                                             const dev_t* tile, int nE, int C,
                                             int Cp, bool vec_ok) {
  constexpr int VL = 16 / (int)sizeof(dev_t);
  const int nchunks = (nE + VL - 1) / VL;
  for (int ch = threadIdx.x; ch < nchunks; ch += TP) {
    const int e = ch * VL;
    int row = e / C;
    int col = e - row * C;
    Vec<dev_t, VL> v;
#pragma unroll
    for (int k = 0; k < VL; ++k) {
      v.v[k] = e + k < nE ? tile[row * Cp + col] : from_f32<dev_t>(0.f);
      if (++col == C) {
        col = 0;
        ++row;
      }
    }
    if (vec_ok && e + VL <= nE) {
      vstore<dev_t, VL>(dst + e, v);
    } else {
#pragma unroll
      for (int k = 0; k < VL; ++k)
        if (e + k < nE) dst[e + k] = v.v[k];
    }
  }
}

// N = B * P pixels, row n of C elements at logits + n * C. TP threads work on
// tiles of tile_pix <= TP pixels (a multiple of 32, so tiles start 16-byte
// aligned).
template <typename dev_t, int TP>
__global__ __launch_bounds__(TP)
void dce_fwd_nhwc_kernel(const dev_t* __restrict__ logits,
                         const int64_t* __restrict__ target,
                         const float* __restrict__ weight,
                         float* __restrict__ lse_out,
                         float* __restrict__ loss_out,
                         float* __restrict__ slab, int64_t N, int C, int Cp,
                         int tile_pix, int vec_ok, int64_t ignore) {
  extern __shared__ __attribute__((aligned(16))) char dce_lds[];
  dev_t* tile = reinterpret_cast<dev_t*>(dce_lds);
  __shared__ float smem[16];
  constexpr int EPD = 4 / (int)sizeof(dev_t);  // elements per LDS dword
  const int64_t ntiles = (N + tile_pix - 1) / tile_pix;
  float ls = 0.f, ws = 0.f;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t pix0 = t * tile_pix;
    const int npix = (int)(N - pix0 < tile_pix ? N - pix0 : tile_pix);
    dce_tile_in<dev_t, TP>(logits + pix0 * C, tile, npix * C, C, Cp,
                           vec_ok != 0);
    __syncthreads();
    if ((int)threadIdx.x < npix) {
      const int64_t n = pix0 + threadIdx.x;
      const int tt = dce_label(target[n], C, ignore);
      const dev_t* row = tile + threadIdx.x * Cp;
      float m = -FLT_MAX, s = 0.f, zt = 0.f;
#pragma unroll 4
      for (int c0 = 0; c0 < C; c0 += EPD) {
        const Vec<dev_t, EPD> zv = vload<dev_t, EPD>(row + c0);
#pragma unroll
        for (int j = 0; j < EPD; ++j) {
          if (c0 + j < C) {
            const float z = to_f32(zv.v[j]);
            dce_lse_step(z, m, s);
            if (c0 + j == tt) zt = z;
          }
        }
      }
      const float lg = __logf(s);
      const bool valid = tt >= 0;
      const float w = valid ? (weight != nullptr ? weight[tt] : 1.f) : 0.f;
      const float loss = valid ? w * ((m - zt) + lg) : 0.f;
      lse_out[n] = m + lg;
      if (loss_out != nullptr) loss_out[n] = loss;
      ls += loss;
      ws += w;
    }
    __syncthreads();  // the next tile overwrites the rows
  }
  if (slab != nullptr) dce_store_partial(slab, ls, ws, smem);
}

template <typename dev_t, int TP, bool PER_PIXEL>
__global__ __launch_bounds__(TP)
void dce_bwd_nhwc_kernel(const dev_t* __restrict__ logits,
                         const int64_t* __restrict__ target,
                         const float* __restrict__ weight,
                         const float* __restrict__ lse,
                         const float* __restrict__ gin,
                         const float* __restrict__ stats,
                         dev_t* __restrict__ dlogits, int64_t N, int C, int Cp,
                         int tile_pix, int vec_ok, int64_t ignore, int mean) {
  extern __shared__ __attribute__((aligned(16))) char dce_lds[];
  dev_t* tile = reinterpret_cast<dev_t*>(dce_lds);
  constexpr int EPD = 4 / (int)sizeof(dev_t);
  const int64_t ntiles = (N + tile_pix - 1) / tile_pix;
  const float gs = PER_PIXEL ? 0.f : dce_scalar_grad(gin, stats, mean);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t pix0 = t * tile_pix;
    const int npix = (int)(N - pix0 < tile_pix ? N - pix0 : tile_pix);
    dce_tile_in<dev_t, TP>(logits + pix0 * C, tile, npix * C, C, Cp,
                           vec_ok != 0);
    __syncthreads();
    if ((int)threadIdx.x < npix) {
      const int64_t n = pix0 + threadIdx.x;
      const int tt = dce_label(target[n], C, ignore);
      const bool valid = tt >= 0;
      const float l = lse[n];
      const float w = valid ? (weight != nullptr ? weight[tt] : 1.f) : 0.f;
      const float coef = w * (PER_PIXEL ? gin[n] : gs);
      dev_t* row = tile + threadIdx.x * Cp;
#pragma unroll 4
      for (int c0 = 0; c0 < C; c0 += EPD) {
        Vec<dev_t, EPD> zv = vload<dev_t, EPD>(row + c0);
#pragma unroll
        for (int j = 0; j < EPD; ++j) {
          const float p = __expf(to_f32(zv.v[j]) - l);
          const float d = coef * (p - (c0 + j == tt ? 1.f : 0.f));
          zv.v[j] = from_f32<dev_t>(valid ? d : 0.f);
        }
        vstore<dev_t, EPD>(row + c0, zv);
      }
    }
    __syncthreads();
    dce_tile_out<dev_t, TP>(dlogits + pix0 * C, tile, npix * C, C, Cp,
                            vec_ok != 0);
    __syncthreads();
  }
}

// LDS row stride in elements: an odd number of dwords, >= C
inline int dce_row_stride(int C, int esize) {
  if (esize == 4) return C | 1;
  int cp = (C + 1) & ~1;         // even
  if ((cp & 3) == 0) cp += 2;    // cp / 2 odd
  return cp;
}

// Block size and pixels per tile: the largest of 256/128 whose tile stays
// within 32 KiB (several blocks per CU keep loads in flight across the
// barriers), else 64; the widest fp32 rows (C = 256) fit the 64 KiB of LDS
// only 32 at a time.
struct DceTile {
  int threads, pixels, lds;
};
inline DceTile dce_tile(int Cp, int esize) {
  for (int tp : {256, 128}) {
    if (tp * Cp * esize <= 32768) return {tp, tp, tp * Cp * esize};
  }
  const int pix = 64 * Cp * esize <= 65536 - 64 ? 64 : 32;
  return {64, pix, pix * Cp * esize};
}

inline bool dce_aligned(const void* p, int bytes) {
  return (reinterpret_cast<uintptr_t>(p) % bytes) == 0;
}

struct DceShape {
  int64_t B, P, N;
  int C;
};

inline DceShape dce_check(const torch::Tensor& logits,
                          const torch::Tensor& target,
                          const c10::optional<torch::Tensor>& weight,
                          bool channels_last) {
  DLA_CHECK_CUDA(logits);
  DLA_CHECK_INPUT(target);
  TORCH_CHECK(logits.dim() >= 3, "dense_ce: logits must be [B, C, *spatial]");
  TORCH_CHECK(target.scalar_type() == at::kLong, "dense_ce: target must be int64");
  DceShape s;
  s.B = logits.size(0);
  TORCH_CHECK(logits.size(1) <= INT_MAX, "dense_ce: too many classes");
  s.C = (int)logits.size(1);
  TORCH_CHECK(s.B > 0 && s.C > 0 && logits.numel() > 0,
              "dense_ce: empty logits");
  s.P = logits.numel() / (s.B * s.C);
  s.N = s.B * s.P;
  TORCH_CHECK(target.dim() == logits.dim() - 1 && target.numel() == s.N &&
                  target.size(0) == s.B,
              "dense_ce: target must be [B, *spatial] of the logits");
  for (int d = 1; d < target.dim(); ++d)
    TORCH_CHECK(target.size(d) == logits.size(d + 1),
                "dense_ce: target must be [B, *spatial] of the logits");
  if (channels_last) {
    TORCH_CHECK(logits.dim() == 4 &&
                    logits.is_contiguous(at::MemoryFormat::ChannelsLast),
                "dense_ce: logits are not channels_last");
    TORCH_CHECK(s.C <= kDceMaxClNhwc, "dense_ce: channels_last needs C <= ",
                kDceMaxClNhwc);
  } else {
    DLA_CHECK_CONTIG(logits);
  }
  if (weight.has_value()) {
    DLA_CHECK_INPUT(*weight);
    TORCH_CHECK(weight->scalar_type() == at::kFloat && weight->numel() == s.C,
                "dense_ce: weight must be fp32 [C]");
  }
  return s;
}

// widest V (elements per lane) the NCHW kernels may use
inline int dce_nchw_width(int64_t P, int esize, bool ptrs_aligned16,
                          const void* logits) {
  if (!ptrs_aligned16) return 1;
  for (int v = 16 / esize; v > 1; v >>= 1) {
    if (P % v == 0 && dce_aligned(logits, v * esize)) return v;
  }
  return 1;
}

}  // namespace dla

#define DCE_DISPATCH_V16(V, ...)                                               \
  [&] {                                                                        \
    switch (V) {                                                               \
      case 8: { constexpr int kV = 8; return __VA_ARGS__(); }                  \
      case 4: { constexpr int kV = 4; return __VA_ARGS__(); }                  \
      case 2: { constexpr int kV = 2; return __VA_ARGS__(); }                  \
      default: { constexpr int kV = 1; return __VA_ARGS__(); }                 \
    }                                                                          \
  }()

#define DCE_DISPATCH_TP(TP, ...)                                               \
  [&] {                                                                        \
    switch (TP) {                                                              \
      case 256: { constexpr int kTP = 256; return __VA_ARGS__(); }             \
      case 128: { constexpr int kTP = 128; return __VA_ARGS__(); }             \
      default: { constexpr int kTP = 64; return __VA_ARGS__(); }               \
    }                                                                          \
  }()

// Returns {result, lse[N] fp32}. result is the fp32 per-pixel loss in the
// target's shape for reduction none, else stats[2] = {loss, denominator}.
std::vector<torch::Tensor> dense_ce_fwd(torch::Tensor logits,
                                        torch::Tensor target,
                                        c10::optional<torch::Tensor> weight,
                                        int64_t ignore_index, int64_t reduction,
                                        bool channels_last) {
  const dla::DceShape s = dla::dce_check(logits, target, weight, channels_last);
  TORCH_CHECK(reduction >= 0 && reduction <= 2, "dense_ce: bad reduction");
  const auto opts_f = logits.options().dtype(torch::kFloat);
  auto lse = torch::empty({s.N}, opts_f);
  const bool none = reduction == dla::kDceNone;
  const float* wp = weight.has_value() ? weight->data_ptr<float>() : nullptr;
  const int64_t* tp = target.data_ptr<int64_t>();
  const int esize = (int)logits.element_size();

  int grid, V = 1, Cp = 0;
  dla::DceTile tile{64, 64, 0};
  if (channels_last) {
    Cp = dla::dce_row_stride(s.C, esize);
    tile = dla::dce_tile(Cp, esize);
    grid = (int)std::min<int64_t>((s.N + tile.pixels - 1) / tile.pixels,
                                  dla::kMaxGrid);
  } else {
    V = dla::dce_nchw_width(s.P, esize,
                            dla::dce_aligned(tp, 16) &&
                                dla::dce_aligned(lse.data_ptr(), 16),
                            logits.data_ptr());
    const int64_t items = s.B * (s.P / V);
    grid = (int)std::min<int64_t>(
        (items + dla::kDceBlock - 1) / dla::kDceBlock, dla::kMaxGrid);
  }

  torch::Tensor result, slab;
  float *loss_p = nullptr, *slab_p = nullptr;
  if (none) {
    result = torch::empty(target.sizes(), opts_f);
    loss_p = result.data_ptr<float>();
    if (!dla::dce_aligned(loss_p, 16)) V = 1;
  } else {
    result = torch::empty({2}, opts_f);
    slab = torch::empty({grid, 2}, opts_f);
    slab_p = slab.data_ptr<float>();
  }

  DLA_DISPATCH_FLOAT_TYPES(logits.scalar_type(), "dense_ce_fwd", [&] {
    const dev_t* lp = (const dev_t*)logits.data_ptr();
    if (channels_last) {
      const int vec_ok = dla::dce_aligned(lp, 16) ? 1 : 0;
      DCE_DISPATCH_TP(tile.threads, [&] {
        hipLaunchKernelGGL((dla::dce_fwd_nhwc_kernel<dev_t, kTP>), dim3(grid),
                           dim3(kTP), tile.lds, dla::stream(), lp, tp, wp,
                           lse.data_ptr<float>(), loss_p, slab_p, s.N, s.C, Cp,
                           tile.pixels, vec_ok, ignore_index);
      });
    } else {
      DCE_DISPATCH_V16(V, [&] {
        if constexpr (kV * sizeof(dev_t) <= 16) {
          hipLaunchKernelGGL((dla::dce_fwd_nchw_kernel<dev_t, kV>), dim3(grid),
                             dim3(dla::kDceBlock), 0, dla::stream(), lp, tp, wp,
                             lse.data_ptr<float>(), loss_p, slab_p, s.B, s.C,
                             s.P, ignore_index);
        }
      });
    }
  });
  HIP_CHECK_ERR();
  if (!none) {
    hipLaunchKernelGGL(dla::dce_finalize_kernel, dim3(1), dim3(dla::kDceBlock),
                       0, dla::stream(), slab_p, grid,
                       result.data_ptr<float>(),
                       reduction == dla::kDceMean ? 1 : 0);
    HIP_CHECK_ERR();
  }
  return {result, lse};
}

// grad_out: fp32, one element for sum / mean (stats = the forward's result,
// read for the mean's denominator), one per pixel for none.
torch::Tensor dense_ce_bwd(torch::Tensor logits, torch::Tensor target,
                           c10::optional<torch::Tensor> weight,
                           torch::Tensor lse, int64_t ignore_index,
                           int64_t reduction, bool channels_last,
                           torch::Tensor grad_out,
                           c10::optional<torch::Tensor> stats) {
  const dla::DceShape s = dla::dce_check(logits, target, weight, channels_last);
  TORCH_CHECK(reduction >= 0 && reduction <= 2, "dense_ce: bad reduction");
  const bool none = reduction == dla::kDceNone;
  const bool mean = reduction == dla::kDceMean;
  DLA_CHECK_INPUT(lse);
  DLA_CHECK_INPUT(grad_out);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == s.N,
              "dense_ce_bwd: lse must be fp32 [N]");
  TORCH_CHECK(grad_out.scalar_type() == at::kFloat &&
                  grad_out.numel() == (none ? s.N : 1),
              "dense_ce_bwd: grad_out must be fp32, per pixel for none, else "
              "one element");
  const float* stats_p = nullptr;
  if (mean) {
    TORCH_CHECK(stats.has_value(), "dense_ce_bwd: mean needs stats");
    DLA_CHECK_INPUT(*stats);
    TORCH_CHECK(stats->scalar_type() == at::kFloat && stats->numel() == 2,
                "dense_ce_bwd: stats must be fp32 [2]");
    stats_p = stats->data_ptr<float>();
  }
  auto dlogits = torch::empty_like(logits);
  const float* wp = weight.has_value() ? weight->data_ptr<float>() : nullptr;
  const int64_t* tp = target.data_ptr<int64_t>();
  const float* gp = grad_out.data_ptr<float>();
  const float* lsp = lse.data_ptr<float>();
  const int esize = (int)logits.element_size();

  DLA_DISPATCH_FLOAT_TYPES(logits.scalar_type(), "dense_ce_bwd", [&] {
    const dev_t* lp = (const dev_t*)logits.data_ptr();
    dev_t* dp = (dev_t*)dlogits.data_ptr();
    if (channels_last) {
      const int Cp = dla::dce_row_stride(s.C, esize);
      const dla::DceTile tile = dla::dce_tile(Cp, esize);
      const int grid = (int)std::min<int64_t>(
          (s.N + tile.pixels - 1) / tile.pixels, dla::kMaxGrid);
      const int vec_ok =
          dla::dce_aligned(lp, 16) && dla::dce_aligned(dp, 16) ? 1 : 0;
      DCE_DISPATCH_TP(tile.threads, [&] {
        auto launch = [&](auto per_pixel) {
          constexpr bool kPP = decltype(per_pixel)::value;
          hipLaunchKernelGGL((dla::dce_bwd_nhwc_kernel<dev_t, kTP, kPP>),
                             dim3(grid), dim3(kTP), tile.lds, dla::stream(),
                             lp, tp, wp, lsp, gp, stats_p, dp, s.N, s.C, Cp,
                             tile.pixels, vec_ok, ignore_index, mean ? 1 : 0);
        };
        if (none) launch(std::true_type{});
        else launch(std::false_type{});
      });
    } else {
      const bool al = dla::dce_aligned(tp, 16) && dla::dce_aligned(lsp, 16) &&
                      (!none || dla::dce_aligned(gp, 16));
      int V = dla::dce_nchw_width(s.P, esize, al, lp);
      if (!dla::dce_aligned(dp, V * esize)) V = 1;
      const int64_t items = s.B * (s.P / V);
      const int grid = (int)std::min<int64_t>(
          (items + dla::kDceBlock - 1) / dla::kDceBlock, dla::kMaxGrid);
      DCE_DISPATCH_V16(V, [&] {
        if constexpr (kV * sizeof(dev_t) <= 16) {
          auto launch = [&](auto per_pixel) {
            constexpr bool kPP = decltype(per_pixel)::value;
            hipLaunchKernelGGL((dla::dce_bwd_nchw_kernel<dev_t, kV, kPP>),
                               dim3(grid), dim3(dla::kDceBlock), 0,
                               dla::stream(), lp, tp, wp, lsp, gp, stats_p, dp,
                               s.B, s.C, s.P, ignore_index, mean ? 1 : 0);
          };
          if (none) launch(std::true_type{});
          else launch(std::false_type{});
        }
      });
    }
  });
  HIP_CHECK_ERR();
  return dlogits;
}
