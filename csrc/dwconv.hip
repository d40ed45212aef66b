// Depthwise 2-D convolution, NHWC (channels_last), forward + dgrad + wgrad.
//
// Supported: square odd K in {3,5,7}, stride in {1,2}, padding (K-1)/2,
// dilation 1, groups == Cin == Cout. bf16 / fp16 / fp32 storage, fp32
// accumulation. There is no channel contraction, so this is a stencil, not a
// GEMM: each lane owns one 16-byte channel vector (V channels) and a strip of
// TW neighbouring outputs along W.
//
//  forward / dgrad(s1): register sliding window. Per tap row the lane loads
//    the (TW-1)*S+K input vectors of its strip once, converts each to fp32
//    once and feeds it to every output of the strip that uses it, so K=7 does
//    13/7 loads per output and tap row instead of 7. The fp32 weights (and
//    bias) of the block's channel tile sit in LDS; dgrad at stride 1 is the
//    same kernel with the taps flipped while they are staged.
//  dgrad(s2): gather over the strip's dx positions; the column parity of every
//    (output, tap) pair is resolved at compile time (strips start on even
//    columns), the row parity is a per-row test. No scatter, no atomics.
//  wgrad: one tap row ky per wave with K*V accumulators per lane; dbias rides
//    along in wave 0. Lanes of a wave that share a channel vector are summed
//    through LDS in slot order, each block stores one fp32 partial slab row
//    set and a finalize kernel sums the slabs in a fixed tree - no float
//    atomics, so dW / dbias are bit-reproducible.
//
// Grids are capped (kMaxGrid) with grid-stride loops over (b, row, strip).
#include "common.h"
#include "vec.h"

namespace dla {

namespace {

constexpr int kDwBlock = 256;
constexpr int kDwMaxCtv = 16;  // channel vectors per block tile (LDS: 25 KiB)

// channel vectors per tile: maximise (useful lanes) x (useful tile columns)
inline int dw_pick_ctv(int CV, int lanes) {
  int best = 1;
  double best_eff = 0.0;
  for (int t = 1; t <= std::min(CV, kDwMaxCtv); ++t) {
    const int tiles = (CV + t - 1) / t;
    const double eff = (double)CV / (double)(tiles * t) *
                       (double)(t * (lanes / t)) / (double)lanes;
    if (eff >= best_eff) {
      best_eff = eff;
      best = t;
    }
  }
  return best;
}

// Stage the block's fp32 weights [KK][ctc] (+ bias [ctc]) in LDS. fp32
// parameters next to 16-bit activations are rounded to the activation type on
// the way, which is the cast autocast would make, without its launch.
template <typename T, int KK>
__device__ __forceinline__ void dw_stage_weights(
    float* __restrict__ wl, const void* __restrict__ w, bool w_f32,
    const void* __restrict__ bias, bool b_f32, int C, int c_base, int ctc,
    bool flip) {
  for (int i = threadIdx.x; i < (KK + 1) * ctc; i += blockDim.x) {
    const int tap = i / ctc, c = c_base + i % ctc;
    float v = 0.f;
    if (c < C) {
      if (tap < KK) {
        const int64_t src = (int64_t)c * KK + (flip ? KK - 1 - tap : tap);
        v = w_f32 ? to_f32(from_f32<T>(static_cast<const float*>(w)[src]))
                  : to_f32(static_cast<const T*>(w)[src]);
      } else if (bias != nullptr) {
        v = b_f32 ? to_f32(from_f32<T>(static_cast<const float*>(bias)[c]))
                  : to_f32(static_cast<const T*>(bias)[c]);
      }
    }
    wl[i] = v;
  }
}

template <typename T, int V>
__device__ __forceinline__ void dw_load_f32(const T* __restrict__ p,
                                            float (&f)[V]) {
  const Vec<T, V> v = vload<T, V>(p);
#pragma unroll
  for (int e = 0; e < V; ++e) f[e] = to_f32(v.v[e]);
}

// y[b,oh,ow,c] = bias[c] + sum_{ky,kx} x[b, oh*S-P+ky, ow*S-P+kx, c] * w[c,ky,kx]
template <typename T, int K, int S, int TW>
__global__ void __launch_bounds__(kDwBlock)
dw_fwd_kernel(const T* __restrict__ x, const void* __restrict__ w, bool w_f32,
              const void* __restrict__ bias, bool b_f32, T* __restrict__ y,
              int C, int H, int W, int OH, int OW, int ctv, int64_t items,
              bool flip) {
  constexpr int V = VecWidth<T>::value;
  constexpr int KK = K * K, P = (K - 1) / 2, NIN = (TW - 1) * S + K;
  extern __shared__ float wl[];
  const int ctc = ctv * V;
  const int c_base = blockIdx.y * ctc;
  dw_stage_weights<T, KK>(wl, w, w_f32, bias, b_f32, C, c_base, ctc, flip);
  __syncthreads();

  const int slots = kDwBlock / ctv;
  const int cvl = threadIdx.x % ctv, slot = threadIdx.x / ctv;
  const int c = c_base + cvl * V;
  if (slot >= slots || c >= C) return;  // no barrier below
  const float* wlc = wl + cvl * V;
  const int strips = (OW + TW - 1) / TW;

  for (int64_t it = (int64_t)blockIdx.x * slots + slot; it < items;
       it += (int64_t)gridDim.x * slots) {
    const uint32_t it32 = (uint32_t)it;  // items <= B*OH*OW < 2^31
    const int st = (int)(it32 % (uint32_t)strips);
    const uint32_t r = it32 / (uint32_t)strips;
    const int oh = (int)(r % (uint32_t)OH);
    const int64_t b = r / (uint32_t)OH;
    const int ow0 = st * TW, iw0 = ow0 * S - P;

    float acc[TW][V];
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[t][e] = wlc[KK * ctc + e];

#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int ih = oh * S - P + ky;
      if (ih < 0 || ih >= H) continue;
      const T* xrow = x + ((b * H + ih) * W) * C + c;
      float wr[K][V];
#pragma unroll
      for (int kx = 0; kx < K; ++kx)
#pragma unroll
        for (int e = 0; e < V; ++e) wr[kx][e] = wlc[(ky * K + kx) * ctc + e];
#pragma unroll
      for (int j = 0; j < NIN; ++j) {
        const int iw = iw0 + j;
        if (iw >= 0 && iw < W) {
          float xf[V];
          dw_load_f32<T, V>(xrow + (int64_t)iw * C, xf);
#pragma unroll
          for (int t = 0; t < TW; ++t) {
            const int kx = j - t * S;
            if (kx >= 0 && kx < K) {
#pragma unroll
              for (int e = 0; e < V; ++e)
                acc[t][e] = fmaf(xf[e], wr[kx][e], acc[t][e]);
            }
          }
        }
      }
    }

    T* yrow = y + ((b * OH + oh) * OW) * C + c;
#pragma unroll
    for (int t = 0; t < TW; ++t) {
      if (ow0 + t < OW) {
        Vec<T, V> o;
#pragma unroll
        for (int e = 0; e < V; ++e) o.v[e] = from_f32<T>(acc[t][e]);
        vstore<T, V>(yrow + (int64_t)(ow0 + t) * C, o);
      }
    }
  }
}

// Stride-2 dgrad as a gather:
// dx[b,ih,iw,c] = sum over (ky,kx) with (ih+P-ky), (iw+P-kx) even and in range
//                 of dy[b,(ih+P-ky)/2,(iw+P-kx)/2,c] * w[c,ky,kx]
// TW is even, so a strip starts on an even iw and column parity is static.
template <typename T, int K, int TW>
__global__ void __launch_bounds__(kDwBlock)
dw_dgrad_s2_kernel(const T* __restrict__ dy, const void* __restrict__ w,
                   bool w_f32, T* __restrict__ dx, int C, int H, int W, int OH,
                   int OW, int ctv, int64_t items) {
  static_assert(TW % 2 == 0, "strips must start on even columns");
  constexpr int V = VecWidth<T>::value;
  constexpr int KK = K * K, P = (K - 1) / 2;
  // u = t + P - kx spans [-P, TW-1+P]; even u = 2m with m in [M_LO, M_HI]
  constexpr int M_LO = -(P / 2), M_HI = (TW - 1 + P) / 2;
  extern __shared__ float wl[];
  const int ctc = ctv * V;
  const int c_base = blockIdx.y * ctc;
  dw_stage_weights<T, KK>(wl, w, w_f32, nullptr, false, C, c_base, ctc, false);
  __syncthreads();

  const int slots = kDwBlock / ctv;
  const int cvl = threadIdx.x % ctv, slot = threadIdx.x / ctv;
  const int c = c_base + cvl * V;
  if (slot >= slots || c >= C) return;  // no barrier below
  const float* wlc = wl + cvl * V;
  const int strips = (W + TW - 1) / TW;

  for (int64_t it = (int64_t)blockIdx.x * slots + slot; it < items;
       it += (int64_t)gridDim.x * slots) {
    const uint32_t it32 = (uint32_t)it;  // items <= B*H*W < 2^31
    const int st = (int)(it32 % (uint32_t)strips);
    const uint32_t r = it32 / (uint32_t)strips;
    const int ih = (int)(r % (uint32_t)H);
    const int64_t b = r / (uint32_t)H;
    const int iw0 = st * TW, owb = iw0 / 2;

    float acc[TW][V];
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[t][e] = 0.f;

#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int u = ih + P - ky;
      if (u < 0 || (u & 1)) continue;
      const int oh = u >> 1;
      if (oh >= OH) continue;
      const T* grow = dy + ((b * OH + oh) * OW) * C + c;
      float wr[K][V];
#pragma unroll
      for (int kx = 0; kx < K; ++kx)
#pragma unroll
        for (int e = 0; e < V; ++e) wr[kx][e] = wlc[(ky * K + kx) * ctc + e];
#pragma unroll
      for (int m = M_LO; m <= M_HI; ++m) {
        const int ow = owb + m;
        if (ow >= 0 && ow < OW) {
          float gf[V];
          dw_load_f32<T, V>(grow + (int64_t)ow * C, gf);
#pragma unroll
          for (int t = 0; t < TW; ++t) {
            const int kx = t + P - 2 * m;
            if (kx >= 0 && kx < K) {
#pragma unroll
              for (int e = 0; e < V; ++e)
                acc[t][e] = fmaf(gf[e], wr[kx][e], acc[t][e]);
            }
          }
        }
      }
    }

    T* xrow = dx + ((b * H + ih) * W) * C + c;
#pragma unroll
    for (int t = 0; t < TW; ++t) {
      if (iw0 + t < W) {
        Vec<T, V> o;
#pragma unroll
        for (int e = 0; e < V; ++e) o.v[e] = from_f32<T>(acc[t][e]);
        vstore<T, V>(xrow + (int64_t)(iw0 + t) * C, o);
      }
    }
  }
}

// wgrad partials. Block = K waves, wave ky owns tap row ky. Per block:
// parts[blockIdx.x][ky*K+kx][c] = sum over the block's (b,oh,ow) of
// dy[b,oh,ow,c] * x[b,oh*S-P+ky,ow*S-P+kx,c], and parts[.][KK][c] = sum dy.
template <typename T, int K, int S, int TW>
__global__ void __launch_bounds__(K * 64)
dw_wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                float* __restrict__ parts, int C, int H, int W, int OH, int OW,
                int ctv, int64_t items) {
  constexpr int V = VecWidth<T>::value;
  constexpr int KK = K * K, P = (K - 1) / 2, NIN = (TW - 1) * S + K;
  __shared__ float red[K][64][V];
  const int ky = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slots = 64 / ctv;
  const int cvl = lane % ctv, slot = lane / ctv;
  const int c = blockIdx.y * ctv * V + cvl * V;
  const bool active = slot < slots && c < C;
  const int strips = (OW + TW - 1) / TW;

  float acc[K][V], bacc[V];
#pragma unroll
  for (int kx = 0; kx < K; ++kx)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[kx][e] = 0.f;
#pragma unroll
  for (int e = 0; e < V; ++e) bacc[e] = 0.f;

  if (active) {
    for (int64_t it = (int64_t)blockIdx.x * slots + slot; it < items;
         it += (int64_t)gridDim.x * slots) {
      const uint32_t it32 = (uint32_t)it;  // items <= B*OH*OW < 2^31
      const int st = (int)(it32 % (uint32_t)strips);
      const uint32_t r = it32 / (uint32_t)strips;
      const int oh = (int)(r % (uint32_t)OH);
      const int64_t b = r / (uint32_t)OH;
      const int ow0 = st * TW, iw0 = ow0 * S - P;
      const int ih = oh * S - P + ky;
      const bool row_ok = ih >= 0 && ih < H;
      if (!row_ok && ky != 0) continue;

      const T* grow = dy + ((b * OH + oh) * OW) * C + c;
      float gf[TW][V];
#pragma unroll
      for (int t = 0; t < TW; ++t) {
        if (ow0 + t < OW) {
          dw_load_f32<T, V>(grow + (int64_t)(ow0 + t) * C, gf[t]);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) gf[t][e] = 0.f;
        }
      }
      if (ky == 0) {
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
          for (int e = 0; e < V; ++e) bacc[e] += gf[t][e];
      }
      if (!row_ok) continue;
      const T* xrow = x + ((b * H + ih) * W) * C + c;
#pragma unroll
      for (int j = 0; j < NIN; ++j) {
        const int iw = iw0 + j;
        if (iw >= 0 && iw < W) {
          float xf[V];
          dw_load_f32<T, V>(xrow + (int64_t)iw * C, xf);
#pragma unroll
          for (int t = 0; t < TW; ++t) {
            const int kx = j - t * S;
            if (kx >= 0 && kx < K) {
#pragma unroll
              for (int e = 0; e < V; ++e)
                acc[kx][e] = fmaf(gf[t][e], xf[e], acc[kx][e]);
            }
          }
        }
      }
    }
  }

  // lanes of a wave that share a channel vector: sum in slot order via LDS
  float* pblk = parts + (int64_t)blockIdx.x * (KK + 1) * C;
#pragma unroll
  for (int kx = 0; kx <= K; ++kx) {  // pass K carries dbias (wave 0 only)
#pragma unroll
    for (int e = 0; e < V; ++e)
      red[ky][lane][e] = kx < K ? acc[kx < K ? kx : 0][e] : bacc[e];
    __syncthreads();
    if (active && slot == 0 && (kx < K || ky == 0)) {
      float s[V];
#pragma unroll
      for (int e = 0; e < V; ++e) s[e] = red[ky][cvl][e];
      for (int sl = 1; sl < slots; ++sl)
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] += red[ky][sl * ctv + cvl][e];
      const int row = kx < K ? ky * K + kx : KK;
#pragma unroll
      for (int e = 0; e < V; ++e) pblk[(int64_t)row * C + c + e] = s[e];
    }
    __syncthreads();
  }
}

// dW[c,tap] / dbias[c] = sum over slabs, fixed order (kDwFinRows row lanes,
// LDS tree): deterministic. Writes the parameter dtype directly.
constexpr int kDwFinCols = 16, kDwFinRows = 16;

template <typename OutT>
__global__ void __launch_bounds__(kDwFinCols * kDwFinRows)
dw_wgrad_finalize_kernel(const float* __restrict__ parts, int n_parts,
                         OutT* __restrict__ dW, OutT* __restrict__ db, int C,
                         int KK) {
  __shared__ float ls[kDwFinRows][kDwFinCols + 1];
  const int cl = threadIdx.x % kDwFinCols, rl = threadIdx.x / kDwFinCols;
  const int n_out = (KK + 1) * C;
  const int j = blockIdx.x * kDwFinCols + cl;
  float s = 0.f;
  if (j < n_out) {
#pragma unroll 4
    for (int r = rl; r < n_parts; r += kDwFinRows)
      s += parts[(int64_t)r * n_out + j];
  }
  ls[rl][cl] = s;
  __syncthreads();
  for (int h = kDwFinRows / 2; h > 0; h >>= 1) {
    if (rl < h) ls[rl][cl] += ls[rl + h][cl];
    __syncthreads();
  }
  if (rl == 0 && j < n_out) {
    const int row = j / C, c = j % C;
    if (row < KK)
      dW[(int64_t)c * KK + row] = from_f32<OutT>(ls[0][cl]);
    else
      db[c] = from_f32<OutT>(ls[0][cl]);
  }
}

inline bool dw_is_nhwc(const torch::Tensor& t) {
  return t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast);
}

struct DwGeom {
  int B, C, H, W, OH, OW, K, S;
};

inline void dw_check_act(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(dw_is_nhwc(t), name, " must be a channels_last 4-D tensor");
  TORCH_CHECK(t.numel() > 0, name, " must not be empty");
  const auto st = t.scalar_type();
  TORCH_CHECK(st == at::kBFloat16 || st == at::kHalf || st == at::kFloat, name,
              " must be bf16, fp16 or fp32");
  TORCH_CHECK(t.size(1) % (16 / t.element_size()) == 0, name,
              ": C must be a multiple of the 16-byte vector");
  TORCH_CHECK(t.size(0) * t.size(2) * t.size(3) < (int64_t(1) << 31), name,
              ": B*H*W must be below 2^31");
}

inline void dw_check_kernel(int64_t K, int64_t stride) {
  TORCH_CHECK(K == 3 || K == 5 || K == 7, "dwconv: kernel size must be 3, 5 or 7");
  TORCH_CHECK(stride == 1 || stride == 2, "dwconv: stride must be 1 or 2");
}

// weight [C,1,K,K] (or bias [C]) in fp32 or the activation dtype
inline void dw_check_param(const torch::Tensor& p, const torch::Tensor& act,
                           const char* name) {
  TORCH_CHECK(p.is_cuda() && p.is_contiguous(), name,
              " must be a contiguous GPU tensor");
  TORCH_CHECK(p.scalar_type() == at::kFloat ||
                  p.scalar_type() == act.scalar_type(),
              name, " must be fp32 or the activation dtype");
}

inline int64_t dw_weight_k(const torch::Tensor& w, int64_t C) {
  TORCH_CHECK(w.dim() == 4 && w.size(0) == C && w.size(1) == 1 &&
                  w.size(2) == w.size(3),
              "dwconv: weight must be [C,1,K,K] (groups == Cin == Cout)");
  return w.size(2);
}

inline dim3 dw_grid(int64_t items, int slots, int n_ctile) {
  const int64_t want = (items + slots - 1) / slots;
  const int64_t cap = std::max<int64_t>(1, kMaxGrid / n_ctile);
  return dim3((unsigned)std::min(want, cap), (unsigned)n_ctile);
}

template <typename T, int K, int S, int TW>
void dw_launch_fwd(const torch::Tensor& x, const torch::Tensor& w,
                   const c10::optional<torch::Tensor>& bias, torch::Tensor& y,
                   const DwGeom& g, bool flip) {
  constexpr int V = VecWidth<T>::value;
  const int CV = g.C / V;
  const int ctv = dw_pick_ctv(CV, kDwBlock);
  const int n_ctile = (CV + ctv - 1) / ctv;
  const int64_t items = (int64_t)g.B * g.OH * ((g.OW + TW - 1) / TW);
  const size_t lds = (size_t)(K * K + 1) * ctv * V * sizeof(float);
  const void* bp = bias.has_value() ? bias->data_ptr() : nullptr;
  const bool b_f32 = bias.has_value() && bias->scalar_type() == at::kFloat;
  hipLaunchKernelGGL((dw_fwd_kernel<T, K, S, TW>),
                     dw_grid(items, kDwBlock / ctv, n_ctile), dim3(kDwBlock),
                     lds, stream(), static_cast<const T*>(x.data_ptr()),
                     w.data_ptr(), w.scalar_type() == at::kFloat, bp, b_f32,
                     static_cast<T*>(y.data_ptr()), g.C, g.H, g.W, g.OH, g.OW,
                     ctv, items, flip);
  HIP_CHECK_ERR();
}

template <typename T, int K>
void dw_launch_dgrad_s2(const torch::Tensor& dy, const torch::Tensor& w,
                        torch::Tensor& dx, const DwGeom& g) {
  constexpr int V = VecWidth<T>::value, TW = 4;
  const int CV = g.C / V;
  const int ctv = dw_pick_ctv(CV, kDwBlock);
  const int n_ctile = (CV + ctv - 1) / ctv;
  const int64_t items = (int64_t)g.B * g.H * ((g.W + TW - 1) / TW);
  const size_t lds = (size_t)(K * K + 1) * ctv * V * sizeof(float);
  hipLaunchKernelGGL((dw_dgrad_s2_kernel<T, K, TW>),
                     dw_grid(items, kDwBlock / ctv, n_ctile), dim3(kDwBlock),
                     lds, stream(), static_cast<const T*>(dy.data_ptr()),
                     w.data_ptr(), w.scalar_type() == at::kFloat,
                     static_cast<T*>(dx.data_ptr()), g.C, g.H, g.W, g.OH, g.OW,
                     ctv, items);
  HIP_CHECK_ERR();
}

template <typename T, int K, int S>
torch::Tensor dw_launch_wgrad(const torch::Tensor& dy, const torch::Tensor& x,
                              const DwGeom& g, int* n_parts_out) {
  constexpr int V = VecWidth<T>::value, TW = 4;
  const int CV = g.C / V;
  const int ctv = dw_pick_ctv(CV, 64);
  const int n_ctile = (CV + ctv - 1) / ctv;
  const int slots = 64 / ctv;
  const int64_t items = (int64_t)g.B * g.OH * ((g.OW + TW - 1) / TW);
  // >= 8 loop trips per lane before another slab is worth its traffic
  const int64_t want = (items + (int64_t)slots * 8 - 1) / ((int64_t)slots * 8);
  const int64_t cap = std::max<int64_t>(1, 512 / n_ctile);
  const int n_parts = (int)std::max<int64_t>(1, std::min(want, cap));
  auto parts = torch::empty({n_parts, K * K + 1, g.C},
                            x.options().dtype(torch::kFloat)
                                .memory_format(at::MemoryFormat::Contiguous));
  hipLaunchKernelGGL((dw_wgrad_kernel<T, K, S, TW>), dim3(n_parts, n_ctile),
                     dim3(K * 64), 0, stream(),
                     static_cast<const T*>(dy.data_ptr()),
                     static_cast<const T*>(x.data_ptr()),
                     parts.data_ptr<float>(), g.C, g.H, g.W, g.OH, g.OW, ctv,
                     items);
  HIP_CHECK_ERR();
  *n_parts_out = n_parts;
  return parts;
}

#define DLA_DW_DISPATCH_K(K_, ...)                                             \
  [&] {                                                                        \
    switch (K_) {                                                              \
      case 3: { constexpr int kK = 3; return __VA_ARGS__(); }                  \
      case 5: { constexpr int kK = 5; return __VA_ARGS__(); }                  \
      default: { constexpr int kK = 7; return __VA_ARGS__(); }                 \
    }                                                                          \
  }()

// forward template on `src` (x, or dy for the stride-1 dgrad)
void dw_run_fwd(const torch::Tensor& src, const torch::Tensor& w,
                const c10::optional<torch::Tensor>& bias, torch::Tensor& dst,
                const DwGeom& g, bool flip) {
  DLA_DISPATCH_FLOAT_TYPES(src.scalar_type(), dwconv_fwd, [&] {
    DLA_DW_DISPATCH_K(g.K, [&] {
      if (g.S == 1) {
        // TW = 7 divides every ConvNeXt width (56, 28, 14, 7)
        constexpr int kTW = kK == 7 ? 7 : 4;
        dw_launch_fwd<dev_t, kK, 1, kTW>(src, w, bias, dst, g, flip);
      } else {
        dw_launch_fwd<dev_t, kK, 2, 4>(src, w, bias, dst, g, flip);
      }
    });
  });
}

}  // namespace

}  // namespace dla

using namespace dla;

torch::Tensor dwconv_fwd(torch::Tensor x, torch::Tensor weight,
                         c10::optional<torch::Tensor> bias, int64_t stride) {
  dw_check_act(x, "x");
  const int64_t C = x.size(1);
  const int64_t K = dw_weight_k(weight, C);
  dw_check_kernel(K, stride);
  dw_check_param(weight, x, "weight");
  if (bias.has_value()) {
    dw_check_param(*bias, x, "bias");
    TORCH_CHECK(bias->dim() == 1 && bias->size(0) == C, "dwconv: bias must be [C]");
  }
  const int64_t P = (K - 1) / 2;
  DwGeom g{(int)x.size(0), (int)C, (int)x.size(2), (int)x.size(3),
           (int)((x.size(2) + 2 * P - K) / stride + 1),
           (int)((x.size(3) + 2 * P - K) / stride + 1), (int)K, (int)stride};
  auto y = torch::empty({g.B, g.C, g.OH, g.OW},
                        x.options().memory_format(at::MemoryFormat::ChannelsLast));
  dw_run_fwd(x, weight, bias, y, g, /*flip=*/false);
  return y;
}

torch::Tensor dwconv_dgrad(torch::Tensor dy, torch::Tensor weight, int64_t H,
                           int64_t W, int64_t stride) {
  dw_check_act(dy, "dy");
  const int64_t C = dy.size(1);
  const int64_t K = dw_weight_k(weight, C);
  dw_check_kernel(K, stride);
  dw_check_param(weight, dy, "weight");
  const int64_t P = (K - 1) / 2;
  TORCH_CHECK(H >= 1 && W >= 1 &&
                  dy.size(2) == (H + 2 * P - K) / stride + 1 &&
                  dy.size(3) == (W + 2 * P - K) / stride + 1,
              "dwconv_dgrad: dy does not match the H x W input at this stride");
  TORCH_CHECK(dy.size(0) * H * W < (int64_t(1) << 31),
              "dwconv_dgrad: B*H*W must be below 2^31");
  auto dx = torch::empty({dy.size(0), C, H, W},
                         dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (stride == 1) {
    // forward on dy with flipped taps; "input" and "output" are both H x W
    DwGeom g{(int)dy.size(0), (int)C, (int)H, (int)W, (int)H, (int)W, (int)K, 1};
    dw_run_fwd(dy, weight, c10::nullopt, dx, g, /*flip=*/true);
  } else {
    DwGeom g{(int)dy.size(0), (int)C, (int)H, (int)W, (int)dy.size(2),
             (int)dy.size(3), (int)K, 2};
    DLA_DISPATCH_FLOAT_TYPES(dy.scalar_type(), dwconv_dgrad, [&] {
      DLA_DW_DISPATCH_K(g.K, [&] {
        dw_launch_dgrad_s2<dev_t, kK>(dy, weight, dx, g);
      });
    });
  }
  return dx;
}

// returns {dW [C,1,K,K], dbias [C]} in fp32 (out_f32) or the activation dtype,
// whichever the parameters are stored in
std::vector<torch::Tensor> dwconv_wgrad(torch::Tensor dy, torch::Tensor x,
                                        int64_t K, int64_t stride,
                                        bool out_f32) {
  dw_check_act(dy, "dy");
  dw_check_act(x, "x");
  dw_check_kernel(K, stride);
  TORCH_CHECK(dy.scalar_type() == x.scalar_type(),
              "dwconv_wgrad: dy and x must have the same dtype");
  const int64_t C = x.size(1), P = (K - 1) / 2;
  TORCH_CHECK(dy.size(0) == x.size(0) && dy.size(1) == C &&
                  dy.size(2) == (x.size(2) + 2 * P - K) / stride + 1 &&
                  dy.size(3) == (x.size(3) + 2 * P - K) / stride + 1,
              "dwconv_wgrad: dy does not match x at this kernel / stride");
  const at::ScalarType out_dtype = out_f32 ? at::kFloat : x.scalar_type();
  DwGeom g{(int)x.size(0), (int)C, (int)x.size(2), (int)x.size(3),
           (int)dy.size(2), (int)dy.size(3), (int)K, (int)stride};
  int n_parts = 0;
  torch::Tensor parts = DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), dwconv_wgrad, [&] {
    return DLA_DW_DISPATCH_K(g.K, [&] {
      return g.S == 1 ? dw_launch_wgrad<dev_t, kK, 1>(dy, x, g, &n_parts)
                      : dw_launch_wgrad<dev_t, kK, 2>(dy, x, g, &n_parts);
    });
  });
  auto opts = x.options().dtype(out_dtype).memory_format(at::MemoryFormat::Contiguous);
  auto dW = torch::empty({C, 1, K, K}, opts);
  auto db = torch::empty({C}, opts);
  const int KK = (int)(K * K);
  const int n_out = (KK + 1) * (int)C;
  DLA_DISPATCH_FLOAT_TYPES(out_dtype, dwconv_wgrad_finalize, [&] {
    hipLaunchKernelGGL((dw_wgrad_finalize_kernel<dev_t>),
                       dim3((n_out + kDwFinCols - 1) / kDwFinCols),
                       dim3(kDwFinCols * kDwFinRows), 0, stream(),
                       parts.data_ptr<float>(), n_parts,
                       static_cast<dev_t*>(dW.data_ptr()),
                       static_cast<dev_t*>(db.data_ptr()), (int)C, KK);
  });
  HIP_CHECK_ERR();
  return {dW, db};
}
