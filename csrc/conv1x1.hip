// 1x1 convolution as an implicit-GEMM MFMA kernel (gfx950 / CDNA4), the
// north-star conv path of BASELINE.json: NHWC conv1x1 IS the GEMM
//   C[M,N] = A[M,K] @ B[N,K]^T,  M = batch*H*W, K = Cin, N = Cout,
// with the weight consumed in its native [Cout][Cin] layout (B^T), so the
// SAME kernel serves forward (A=x, B=W) and data-grad (A=dy, B=W^T).
//
// Replaces the reference's nn.Conv2d 1x1 call sites
// (classification/resnet/models/networks.py:27-35 Bottleneck conv1/conv3 and
// downsample) with a hand-written CDNA4 kernel:
//  - 128xBN tile (BN 64/128), BK=64, 4 waves, mfma_f32_16x16x32_bf16
//  - global->LDS staging via __builtin_amdgcn_global_load_lds (16B pieces),
//    double-buffered, one barrier per K-step (guide §5 step-3 structure)
//  - XOR-swizzled LDS image (guide T2 / G4: byte ^= (row&7)<<4 applied on the
//    glds SOURCE address and again on the ds_read_b128 fragment reads)
//  - fused epilogue: optional per-channel bias / scale+shift (eval-mode BN) /
//    residual add / ReLU, and optional per-channel sum+sumsq accumulation so
//    train-mode BatchNorm needs NO separate stats pass over the output
//    (sums layout matches batchnorm.hip: sums[c], sums[C+c])
//  - epilogue stores go through an LDS f32 transpose so global writes are
//    row-major 8B/lane coalesced (fragment layout is column-per-lane)
//
// wgrad: dW[N][K] = sum_m dy[m][n] * x[m][k] — separate kernels contracting
// over M. 1x1: conv1x1_wgrad2_kernel (row-major glds staging, transposed
// ds_read_b64_tr_b16 fragment reads, per-split slab + fixed-order finalize).
// 3x3 and the DLA_C1X1_WGRAD_V1=1 A/B route: conv1x1_wgrad_kernel (scatter
// ds_write staging into transposed images, fp32 atomicAdd over M-splits).
#include <cstdlib>

#include "common.h"
#include "vec.h"

namespace dla {

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

using bf16 = __hip_bfloat16;

// global->LDS direct copy, 16 bytes per lane (guide §5: the 16B width is the
// fast variant; dest must be wave-uniform base + lane*16).
__device__ __forceinline__ void glds16(const bf16* gsrc, bf16* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)gsrc,
      (__attribute__((address_space(3))) unsigned int*)lds_dst, 16, 0, 0);
}

// ---------------------------------------------------------------------------
// conv1x1 forward / dgrad kernel: C[M,N] = A[M,K] @ B[N,K]^T (bf16 in/out,
// fp32 accumulate). K % 64 == 0, N % BN == 0.
// ---------------------------------------------------------------------------
// TAPS=1: plain 1x1 GEMM. TAPS=9: 3x3 stride-1 pad-1 implicit GEMM —
// K = 9*Cin tap-major, each BK k-step lies inside ONE (ky,kx) tap plane
// (Cin % 64 == 0), the A row for output position m is the tap-shifted
// input row with zero predication at the image boundary; everything else
// (B staging from the wrapper-pre-permuted [Co][9Ci] weight, MFMA loop,
// stats/bias/scale/relu/residual epilogue, store transpose) is shared.
//
// BWD != BWD_NONE (dgrad only): the store pass also does pass 1 of the BN
// backward whose output gradient this GEMM produces. v is the bf16 value the
// plain kernel would store (after the residual add and its rounding):
//   BWD_RELU_X     g = bn_pre(x, scale, shift) > 0 ? v : 0   (BN + ReLU)
//   BWD_JOIN       g = out > 0 ? v : 0                       (residual join)
//   BWD_JOIN_DUAL  as JOIN, with the second BN's x-hat
// g is stored in place of v, and sum g, sum g*xhat (DUAL: sum g*xhat_d) of
// the block's rows go to row blockIdx.y of a [gridDim.y, NS*N] slab, layout
// {sum g [N], sum g*xhat [N], (DUAL) sum g*xhat_d [N]} as the BN reduction
// kernels write it. Every (m-block, n-block) stores its [NS*BN] slice once:
// no atomics, no zero fill, fixed summation order.
enum BwdMode { BWD_NONE = 0, BWD_RELU_X = 1, BWD_JOIN = 2, BWD_JOIN_DUAL = 3 };

struct BwdEpi {
  const bf16* out;      // [M,N] join output (JOIN, JOIN_DUAL)
  const bf16* x;        // [M,N] raw input of the BN
  const bf16* xd;       // [M,N] raw input of the second BN (JOIN_DUAL)
  const float* scale;   // [N] forward scale / shift of the BN (RELU_X)
  const float* shift;
  const float* mean;    // [N]
  const float* rstd;
  const float* mean_d;  // [N] (JOIN_DUAL)
  const float* rstd_d;
  float* slab;          // [gridDim.y, NS*N]
};

template <int BN, bool STATS, int BK = 64, int TAPS = 1, int RING = 0,
          int BWD = BWD_NONE>
// The backward-stats modes ask for the 3 waves per SIMD the plain BN=128
// dgrad runs at: left alone, their extra epilogue state costs a block per CU
// (the allocator then spends the accumulator registers as well: 138-168
// unified, no spill). BWD_NONE asks for nothing (1 is the default minimum).
// They are built for BN 64 and 128 only: the 8-wave BN=256 variant has 128
// registers per lane, spilled and measured slower than the separate pass.
__global__ __launch_bounds__((BN == 256) ? 512 : 256)
__attribute__((amdgpu_waves_per_eu(BWD == BWD_NONE ? 1 : 3))) void
conv1x1_nt_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B,
    bf16* __restrict__ C, const bf16* __restrict__ residual,  // [M,N] | null
    const float* __restrict__ bias,                           // [N] | null
    const float* __restrict__ scale,                          // [N] | null
    const float* __restrict__ shift,                          // [N] | null
    float* __restrict__ sums,  // [gridDim.x, 2N] per-block partials | null
    int64_t M, int K, int N, bool relu, int imgH = 0, int imgW = 0,
    BwdEpi be = BwdEpi{}) {
  static_assert(BWD == BWD_NONE || (!STATS && TAPS == 1 && BN != 256),
                "the backward-stats epilogue belongs to the 1x1 dgrad");
  constexpr int BM = 128;
  constexpr int NWAVES = (BN == 256) ? 8 : 4;
  constexpr int WAVES_M = (BN == 64) ? 4 : 2;
  constexpr int WAVES_N = NWAVES / WAVES_M;  // 4 / 2 / 1
  constexpr int WM = BM / WAVES_M;  // 64 or 32
  constexpr int WN = BN / WAVES_N;  // 64
  constexpr int MFR = WM / 16, NFR = WN / 16;
  constexpr int ROWB = BK * 2;  // LDS row bytes (128)

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // grid (gy=n, gx=m) with n fastest: the N/BN blocks of one M-strip are
  // dispatched together, so they share the strip's A tile through L2/L3
  // instead of re-fetching it a full grid-pass later
  const int64_t m0 = (int64_t)blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;

  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  bf16* const lds16 = (bf16*)lds_raw;
  const int nk = K / BK;
  // direct-global A fragments measured SLOWER than LDS staging at nk==1
  // (latency-exposed loads, no glds prefetch): keep the staged path.
  const bool direct_a = false;
  // RING>0: R-slot glds ring, stage 2 ahead (guide "pipelining across
  // barriers": raw s_barrier + counted vmcnt leaves 2 stages in flight)
  const int nbuf = RING > 0 ? RING : (nk > 1 ? 2 : 1);
  auto a_lds = [&](int buf) { return lds16 + buf * (BM * BK); };
  auto b_lds = [&](int buf) {
    return (direct_a ? lds16 : lds16 + nbuf * BM * BK) + buf * (BN * BK);
  };

  // stage one K-step of A[BM][BK] and B[BN][BK] into buffer `buf`.
  // LDS image is row-major with the read-side XOR swizzle baked into the
  // SOURCE address (rule 21: linear dest + inverse-swizzled source).
  // A 1KB piece covers 1024/ROWB rows; swizzle granularity shrinks with the
  // row size (BK=64: byte ^= (row&7)<<4 over 16B slots; BK=32: (row&3)<<4).
  constexpr int RPP = 1024 / (BK * 2);       // rows per 1KB piece (8 or 16)
  constexpr int LPR = 64 / RPP;              // lanes per row (8 or 4)
  // BK=64 (128B rows): byte ^= (row&7)<<4 spreads a 16-lane column read
  // over 8 slots. BK=32 (64B rows): rows alias every 4, so fold row>>2 in:
  // ((row ^ row>>2)&3)<<4 gives 4 distinct slots per alias class.
  auto swz = [&](int row) {
    return BK == 64 ? (row & 7) << 4 : ((row ^ (row >> 2)) & 3) << 4;
  };
  const int CinK = K / TAPS;  // physical A row length (elements)
  auto stage = [&](int buf, int kt) {
    const int k0b_all = kt * BK * 2;
    // tap plane + byte offset within the tap's Cin slice
    const int tap = TAPS == 1 ? 0 : (kt * BK) / CinK;
    const int k0b = TAPS == 1 ? k0b_all : ((kt * BK) % CinK) * 2;
    const int ky = tap / 3 - 1, kx = tap % 3 - 1;  // -1..1 (TAPS==9)
    if (!direct_a) {
#pragma unroll
      for (int pp = 0; pp < (BM / RPP) / NWAVES; ++pp) {
        const int p = wave + pp * NWAVES;
        const int row = p * RPP + lane / LPR;
        const int b = (lane % LPR) * 16;
        if (TAPS == 1) {
          const int64_t rg = m0 + row < M ? m0 + row : M - 1;
          const char* src = (const char*)A + rg * (int64_t)CinK * 2 + k0b +
                            (b ^ swz(row));
          glds16((const bf16*)src, a_lds(buf) + p * 512);
        } else {
          // per-row tap shift + boundary predication: a 128-row strip
          // nearly always crosses a W boundary for kx != 0, so this path
          // stages by predicated 16B loads + LDS vector stores
          const int64_t m = m0 + row < M ? m0 + row : M - 1;
          const int64_t img = m / ((int64_t)imgH * imgW);
          const int r = (int)(m - img * imgH * imgW);
          const int oh = r / imgW, ow = r % imgW;
          const int ih = oh + ky, iw = ow + kx;
          const bool valid = (unsigned)ih < (unsigned)imgH &&
                             (unsigned)iw < (unsigned)imgW &&
                             m0 + row < M;
          Vec<bf16, 8> v;
          if (valid) {
            const int64_t in_row = (img * imgH + ih) * imgW + iw;
            v = *(const Vec<bf16, 8>*)((const char*)A +
                                       in_row * (int64_t)CinK * 2 + k0b +
                                       (b ^ swz(row)));
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v.v[j] = from_f32<bf16>(0.f);
          }
          vstore<bf16, 8>(a_lds(buf) + p * 512 + (lane % LPR) * 8 +
                              (lane / LPR) * (BK),
                          v);
        }
      }
    }
#pragma unroll
    for (int pp = 0; pp < (BN / RPP) / NWAVES; ++pp) {
      const int p = wave + pp * NWAVES;
      const int row = p * RPP + lane / LPR;
      const int b = (lane % LPR) * 16;
      const char* src = (const char*)B + (int64_t)(n0 + row) * K * 2 +
                        k0b_all + (b ^ swz(row));
      glds16((const bf16*)src, b_lds(buf) + p * 512);
    }
  };

  const int wm_off = (wave / WAVES_N) * WM;
  const int wn_off = (wave % WAVES_N) * WN;

  f32x4 acc[MFR][NFR];
#pragma unroll
  for (int mi = 0; mi < MFR; ++mi)
#pragma unroll
    for (int ni = 0; ni < NFR; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute_step = [&](const char* ab, const char* bb) {
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      const int kbyte = (ks * 32 + (lane >> 4) * 8) * 2;
      bf16x8 af[MFR], bfr[NFR];
#pragma unroll
      for (int mi = 0; mi < MFR; ++mi) {
        const int row = wm_off + mi * 16 + (lane & 15);
        if (direct_a) {
          const int64_t rg = m0 + row < M ? m0 + row : M - 1;
          af[mi] = *(const bf16x8*)((const char*)A + rg * (int64_t)K * 2 +
                                    kbyte);
        } else {
          af[mi] =
              *(const bf16x8*)(ab + row * ROWB + (kbyte ^ swz(row)));
        }
      }
#pragma unroll
      for (int ni = 0; ni < NFR; ++ni) {
        const int row = wn_off + ni * 16 + (lane & 15);
        bfr[ni] = *(const bf16x8*)(bb + row * ROWB + (kbyte ^ swz(row)));
      }
#pragma unroll
      for (int mi = 0; mi < MFR; ++mi)
#pragma unroll
        for (int ni = 0; ni < NFR; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
    }
  };

  if constexpr (RING == 0) {
    stage(0, 0);
    __syncthreads();  // drains the glds (vmcnt0 inside the barrier)
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
      compute_step((const char*)a_lds(cur), (const char*)b_lds(cur));
      __syncthreads();
      cur ^= 1;
    }
  } else {
    // 4-slot ring, stage 2 ahead. Slot s is overwritten by stage(s+RING)
    // issued 2 iterations after its readers' barrier (R >= D+2 bounds the
    // wave skew: issue at iteration j implies all computes <= j-2 done).
    // Counted vmcnt before a RAW barrier per the guide: __syncthreads()
    // would drain every in-flight glds to vmcnt(0).
    static_assert(RING == 4, "ring depth fixed at 4 (stage 2 ahead)");
    constexpr int G = ((BM / RPP) / NWAVES) + ((BN / RPP) / NWAVES);
    stage(0, 0);
    if (nk > 1) stage(1, 1);
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 2 < nk) {
        stage((kt + 2) % RING, kt + 2);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * G) : "memory");
      } else if (kt + 1 < nk) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      compute_step((const char*)a_lds(kt % RING),
                   (const char*)b_lds(kt % RING));
    }
    __syncthreads();  // all glds drained: bare barrier before LDS reuse
  }

  // ---- stats from registers (fp32-exact, before the bf16 rounding) -------
  // fragment layout: lane's channel for n-tile ni is col = ni*16 + (lane&15);
  // its 4*MFR values per ni are rows of that channel. Padded rows (gm >= M)
  // must not contribute.
  if (STATS) {
    // per-block partial sums -> slab row sums[m-block * 2N + ...], NO
    // global atomics (a 6k-deep atomic chain per channel measured 6x the
    // whole GEMM); the [2C] reduction happens in one torch sum downstream.
    float* sbuf = (float*)lds_raw;  // [WAVES_M][2*BN] (staging LDS is free)
    const int wm = wave / WAVES_N;
#pragma unroll
    for (int ni = 0; ni < NFR; ++ni) {
      const int c = wn_off + ni * 16 + (lane & 15);  // channel within block
      const float b = bias != nullptr ? bias[n0 + c] : 0.f;
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int mi = 0; mi < MFR; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t gm = m0 + wm_off + mi * 16 + (lane >> 4) * 4 + r;
          if (gm < M) {
            const float raw = acc[mi][ni][r] + b;
            s += raw;
            q += raw * raw;
          }
        }
      // lanes l, l+16, l+32, l+48 hold the same channel (different rows)
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      q += __shfl_xor(q, 16, 64);
      q += __shfl_xor(q, 32, 64);
      if (lane < 16) {
        sbuf[wm * (2 * BN) + c] = s;
        sbuf[wm * (2 * BN) + BN + c] = q;
      }
    }
    __syncthreads();
    float* slab = sums + (int64_t)blockIdx.y * (2 * N);  // m-block row
    for (int t = threadIdx.x; t < 2 * BN; t += NWAVES * 64) {
      float tot = 0.f;
#pragma unroll
      for (int wmi = 0; wmi < WAVES_M; ++wmi) tot += sbuf[wmi * (2 * BN) + t];
      const int c = t < BN ? t : t - BN;
      slab[(t < BN ? 0 : N) + n0 + c] = tot;
    }
    __syncthreads();  // sbuf is about to be reused by the store transpose
  }

  // ---- epilogue: LDS bf16 transpose -> row-major 16B stores --------------
  // chunked over m-halves so the scratch stays at half a wave-tile (keeps
  // the K=64 single-buffer path at 3 blocks/CU)
  constexpr int EROW = WN + 8;  // +8 bf16 pad keeps b128 reads 16B-aligned
  constexpr int EPC = (MFR >= 4) ? 2 : 1;   // epilogue chunks
  constexpr int MFC = MFR / EPC;            // m-frags per chunk
  bf16* ep = (bf16*)lds_raw + wave * (MFC * 16) * EROW;
  const int c0 = (lane & 7) * 8;           // channel chunk in wave tile
  const int ng0 = n0 + wn_off + c0;        // global channel of chunk start
  const bool has_ss = scale != nullptr;
  float sc[8], sh[8];
  if (has_ss) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = scale[ng0 + j]; sh[j] = shift[ng0 + j]; }
  }
  float bcol[NFR];
#pragma unroll
  for (int ni = 0; ni < NFR; ++ni)
    bcol[ni] = bias != nullptr ? bias[n0 + wn_off + ni * 16 + (lane & 15)]
                               : 0.f;
  // backward-stats state: this lane's 8 channels, summed over its rows
  constexpr bool BDUAL = BWD == BWD_JOIN_DUAL;
  constexpr int BNS = BWD == BWD_NONE ? 1 : (BDUAL ? 3 : 2);
  float bacc[BNS][8], bmu[8], brs[8], bmud[8], brsd[8], bsc[8], bsh[8];
  if constexpr (BWD != BWD_NONE) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bmu[j] = be.mean[ng0 + j];
      brs[j] = be.rstd[ng0 + j];
      if constexpr (BDUAL) {
        bmud[j] = be.mean_d[ng0 + j];
        brsd[j] = be.rstd_d[ng0 + j];
      }
      if constexpr (BWD == BWD_RELU_X) {
        bsc[j] = be.scale[ng0 + j];
        bsh[j] = be.shift[ng0 + j];
      }
#pragma unroll
      for (int s = 0; s < BNS; ++s) bacc[s][j] = 0.f;
    }
  }
#pragma unroll
  for (int h = 0; h < EPC; ++h) {
#pragma unroll
    for (int mc = 0; mc < MFC; ++mc) {
      const int mi = h * MFC + mc;
#pragma unroll
      for (int ni = 0; ni < NFR; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = mc * 16 + (lane >> 4) * 4 + r;
          const int col = ni * 16 + (lane & 15);
          ep[row * EROW + col] = from_f32<bf16>(acc[mi][ni][r] + bcol[ni]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < (MFC * 16) / 8; ++i) {
      const int r = (lane >> 3) + 8 * i;
      const int64_t gm = m0 + wm_off + h * (MFC * 16) + r;
      if (gm < M) {
        Vec<bf16, 8> v = vload<bf16, 8>(ep + r * EROW + c0);
        Vec<bf16, 8> res;
        if (residual != nullptr)
          res = vload<bf16, 8>(residual + gm * N + ng0);
        Vec<bf16, 8> bo, bx, bxd;  // mask source and x-hat inputs
        if constexpr (BWD == BWD_JOIN || BDUAL)
          bo = vload<bf16, 8>(be.out + gm * N + ng0);
        if constexpr (BWD != BWD_NONE)
          bx = vload<bf16, 8>(be.x + gm * N + ng0);
        if constexpr (BDUAL) bxd = vload<bf16, 8>(be.xd + gm * N + ng0);
        Vec<bf16, 8> out;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float y = to_f32(v.v[j]);
          if (has_ss) y = y * sc[j] + sh[j];
          if (residual != nullptr) y += to_f32(res.v[j]);
          if (relu) y = fmaxf(y, 0.f);
          out.v[j] = from_f32<bf16>(y);
          if constexpr (BWD != BWD_NONE) {
            // mask and sum the rounded value, as the separate pass 1 does
            const float xf = to_f32(bx.v[j]);
            const bool on = BWD == BWD_RELU_X
                                ? bn_pre(xf, bsc[j], bsh[j]) > 0.f
                                : to_f32(bo.v[j]) > 0.f;
            if (!on) out.v[j] = from_f32<bf16>(0.f);
            const float g = on ? to_f32(out.v[j]) : 0.f;
            bacc[0][j] += g;
            bacc[1][j] += g * ((xf - bmu[j]) * brs[j]);
            if constexpr (BDUAL)
              bacc[2][j] += g * ((to_f32(bxd.v[j]) - bmud[j]) * brsd[j]);
          }
        }
        vstore<bf16, 8>(C + gm * N + ng0, out);
      }
    }
    if (h + 1 < EPC) __syncthreads();
  }

  if constexpr (BWD != BWD_NONE) {
    // lanes l, l^8, l^16, l^32 hold the same 8 channels (different rows):
    // fixed xor order, then the WAVES_M waves of a column through LDS in
    // ascending order, as the forward STATS epilogue does
#pragma unroll
    for (int s = 0; s < BNS; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = bacc[s][j];
        t += __shfl_xor(t, 8, 64);
        t += __shfl_xor(t, 16, 64);
        t += __shfl_xor(t, 32, 64);
        bacc[s][j] = t;
      }
    __syncthreads();  // every wave is done with its transpose scratch
    float* sbuf = (float*)lds_raw;  // [WAVES_M][BNS * BN]
    const int wm = wave / WAVES_N;
    if (lane < 8) {
#pragma unroll
      for (int s = 0; s < BNS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          sbuf[wm * (BNS * BN) + s * BN + wn_off + c0 + j] = bacc[s][j];
    }
    __syncthreads();
    float* row = be.slab + (int64_t)blockIdx.y * (BNS * N);  // m-block row
    for (int t = threadIdx.x; t < BNS * BN; t += NWAVES * 64) {
      float tot = 0.f;
#pragma unroll
      for (int wmi = 0; wmi < WAVES_M; ++wmi)
        tot += sbuf[wmi * (BNS * BN) + t];
      row[(t / BN) * N + n0 + (t % BN)] = tot;
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad kernel: dW[N][K] += sum_m dy[m][n] * x[m][k] (fp32 atomics).
// Both operands staged TRANSPOSED in LDS ([ch][m+pad], scatter b16 writes
// with an m-XOR so the channel-group writes spread over banks), fragments
// then read m-contiguous b128. 64x64 output tile, 4 waves (32x32 each).
// ---------------------------------------------------------------------------
// TAPS=9: dW[co][tap*Ci+ci] = sum_m dy[m][co] * x[shift_tap(m)][ci]
// (3x3 s1 p1 wgrad) — the x tile is staged from tap-shifted rows with
// zero predication at the image boundary, everything else unchanged.
template <int BCO, int BCI, int TAPS = 1>
__global__ __launch_bounds__((BCO * BCI >= 8192) ? 512 : 256) void conv1x1_wgrad_kernel(
    const bf16* __restrict__ dy,  // [M,N]
    const bf16* __restrict__ x,   // [M,Cin] (K = TAPS*Cin)
    float* __restrict__ dW,       // [N,K] pre-zeroed
    int64_t M, int K, int N, int64_t chunk, int imgH = 0, int imgW = 0) {
  constexpr int KM = 64;   // m per step
  constexpr int TR = 72;   // LDS row length (elements) for [ch][KM] image
  constexpr int NW = (BCO * BCI >= 8192) ? 8 : 4;
  constexpr int WGC = (BCO >= 128 && BCI == 64) ? 4 : 2;  // wave grid over co
  constexpr int WGI = NW / WGC;        // wave grid over ci
  constexpr int WCO = BCO / WGC;       // 64 or 32
  constexpr int WCI = BCI / WGI;       // 32
  constexpr int FCO = WCO / 16, FCI = WCI / 16;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * BCO;  // co tile
  const int k0 = blockIdx.y * BCI;  // ci tile
  const int64_t m_begin = (int64_t)blockIdx.z * chunk;
  const int64_t m_end = m_begin + chunk < M ? m_begin + chunk : M;

  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  bf16* const lds16 = (bf16*)lds_raw;
  auto dyt = [&](int buf) { return lds16 + buf * (BCO * TR); };
  auto xt = [&](int buf) { return lds16 + 2 * BCO * TR + buf * (BCI * TR); };

  // transposed scatter-stage of a [KM m][BCH ch] global chunk into
  // lds[ch][m ^ mswz(ch)] (mswz spreads the 8 channel-groups over banks).
  // tap >= 0 (TAPS==9): rows are tap-shifted with boundary zeros.
  auto stage_t = [&](bf16* lds, const bf16* g, int stride_elems, int ch0g,
                     int64_t mt, int tap, auto bch_tag) {
    constexpr int BCH = decltype(bch_tag)::value;
#pragma unroll
    for (int it = 0; it < (KM * BCH / 8) / (NW * 64); ++it) {
      const int idx = (int)threadIdx.x + it * (NW * 64);
      const int m = idx / (BCH / 8);            // 0..63
      const int ch = (idx % (BCH / 8)) * 8;
      Vec<bf16, 8> v;
      bool valid = mt + m < m_end;
      int64_t src_row = mt + m;
      if (TAPS != 1 && tap >= 0 && valid) {
        const int ky = tap / 3 - 1, kx = tap % 3 - 1;
        const int64_t img = src_row / ((int64_t)imgH * imgW);
        const int r = (int)(src_row - img * imgH * imgW);
        const int oh = r / imgW, ow = r % imgW;
        const int ih = oh + ky, iw = ow + kx;
        valid = (unsigned)ih < (unsigned)imgH &&
                (unsigned)iw < (unsigned)imgW;
        src_row = (img * imgH + ih) * imgW + iw;
      }
      if (valid) {
        v = vload<bf16, 8>(g + src_row * (int64_t)stride_elems + ch0g + ch);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v.v[j] = from_f32<bf16>(0.f);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = ch + j;
        lds[c * TR + (m ^ (((c >> 3) & 7) << 3))] = v.v[j];
      }
    }
  };

  // TAPS==9: one block owns a ky ROW of taps (3 of them) for its
  // (co, ci) tile, so dy is staged ONCE per m-step instead of once per
  // tap (the all-tap-tiles grid re-read dy ~9x: ~1.8 GB/call at the
  // 56x56x64 shape). The kx taps loop inside over alternating x buffers.
  constexpr int KXN = (TAPS == 1) ? 1 : 3;
  f32x4 acc[KXN][FCO][FCI];
#pragma unroll
  for (int kx = 0; kx < KXN; ++kx)
#pragma unroll
    for (int mi = 0; mi < FCO; ++mi)
#pragma unroll
      for (int ni = 0; ni < FCI; ++ni)
        acc[kx][mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int wco = (wave / WGI) * WCO;
  const int wci = (wave % WGI) * WCI;

  const int CinK = K / TAPS;
  const int ky_idx = TAPS == 1 ? 0 : k0 / CinK;     // ky row of this block
  const int ci0 = TAPS == 1 ? k0 : k0 % CinK;       // offset within x row
  auto tap_of = [&](int kx) { return TAPS == 1 ? -1 : ky_idx * 3 + kx; };

  stage_t(dyt(0), dy, N, n0, m_begin, -1, std::integral_constant<int, BCO>{});
  stage_t(xt(0), x, CinK, ci0, m_begin, tap_of(0),
          std::integral_constant<int, BCI>{});
  __syncthreads();
  int xbuf = 0, dybuf = 0;
  for (int64_t mt = m_begin; mt < m_end; mt += KM) {
#pragma unroll
    for (int kx = 0; kx < KXN; ++kx) {
      // prefetch the next x tile (next tap, or next m-step's first tap)
      if (kx + 1 < KXN) {
        stage_t(xt(xbuf ^ 1), x, CinK, ci0, mt, tap_of(kx + 1),
                std::integral_constant<int, BCI>{});
      } else if (mt + KM < m_end) {
        stage_t(xt(xbuf ^ 1), x, CinK, ci0, mt + KM, tap_of(0),
                std::integral_constant<int, BCI>{});
        stage_t(dyt(dybuf ^ 1), dy, N, n0, mt + KM, -1,
                std::integral_constant<int, BCO>{});
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int mm = ks * 32 + (lane >> 4) * 8;
        bf16x8 af[FCO], bfr[FCI];
#pragma unroll
        for (int mi = 0; mi < FCO; ++mi) {
          const int c = wco + mi * 16 + (lane & 15);
          af[mi] = *(const bf16x8*)(dyt(dybuf) + c * TR +
                                    (mm ^ (((c >> 3) & 7) << 3)));
        }
#pragma unroll
        for (int ni = 0; ni < FCI; ++ni) {
          const int c = wci + ni * 16 + (lane & 15);
          bfr[ni] = *(const bf16x8*)(xt(xbuf) + c * TR +
                                     (mm ^ (((c >> 3) & 7) << 3)));
        }
#pragma unroll
        for (int mi = 0; mi < FCO; ++mi)
#pragma unroll
          for (int ni = 0; ni < FCI; ++ni)
            acc[kx][mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[mi], bfr[ni], acc[kx][mi][ni], 0, 0, 0);
      }
      __syncthreads();
      xbuf ^= 1;
    }
    dybuf ^= 1;
  }

#pragma unroll
  for (int kx = 0; kx < KXN; ++kx)
#pragma unroll
    for (int mi = 0; mi < FCO; ++mi)
#pragma unroll
      for (int ni = 0; ni < FCI; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = n0 + wco + mi * 16 + (lane >> 4) * 4 + r;
          const int ci_local = wci + ni * 16 + (lane & 15);
          const int kg = TAPS == 1
              ? k0 + ci_local
              : (ky_idx * 3 + kx) * CinK + ci0 + ci_local;
          atomicAdd(&dW[(int64_t)co * K + kg], acc[kx][mi][ni][r]);
        }
}

// ---------------------------------------------------------------------------
// wgrad v2 (1x1 only): dW[N][K] = sum_m dy[m][n] * x[m][k], no atomics.
//  - both operands are staged exactly as they lie in memory, as row-major
//    [KM m][BC ch] LDS images, 16 B per lane straight from global
//    (glds16), double-buffered with one barrier per 64-row step
//  - the transpose happens in the fragment read: two ds_read_b64_tr_b16 per
//    16ch x 32m operand fragment (guide T10). Group g of 16 lanes reads rows
//    8g..8g+3 then 8g+4..8g+7 of the k-step, so lane (g, i) ends up with
//    channel i, m = 8g + j in element j: the MFMA's natural k order, for
//    both operands alike
//  - a 32-lane half touches 8 rows (q = 0..3 of two blocks 8 rows apart),
//    32 B each; wg_swz XORs the 16-byte chunk index so they fall on 8
//    different bank octets (bank = (byte/4) % 64). The XOR never touches
//    chunk bit 0, so the 32 bytes of one block row stay contiguous. It is
//    applied to the glds SOURCE address (linear LDS destination) and again
//    on the fragment read
//  - the last, partial step of a chunk stages through registers with zero
//    fill into the same image; rows at or past m_end are never read
//  - splits > 1: each split stores its fp32 tile into out[split][N][K] and
//    wgrad_finalize_kernel sums the splits in fixed order; splits == 1
//    stores dW directly
//  - the 1-D grid is remapped so the tiles of one m-chunk run on one XCD
//    (ids congruent mod 8 share an XCD) and share the chunk through its L2;
//    only speed depends on that placement
// ---------------------------------------------------------------------------
using bf16x4 = __attribute__((ext_vector_type(4))) short;

template <int BC>
__device__ __forceinline__ int wg_swz(int row) {
  static_assert(BC == 64 || BC == 128, "128 B or 256 B rows");
  // 128 B rows: odd rows already sit in the other half of the 256 B bank row
  if (BC == 64) return (((row >> 1) & 1) << 2) | (((row >> 3) & 1) << 1);
  return ((row & 3) << 2) | (((row >> 3) & 1) << 1);
}

template <int BCO, int BCI>
__global__ __launch_bounds__(256) void conv1x1_wgrad2_kernel(
    const bf16* __restrict__ dy,  // [M,N]
    const bf16* __restrict__ x,   // [M,K]
    float* __restrict__ out,      // [splits][N][K] (dW itself at splits == 1)
    int64_t M, int K, int N, int64_t chunk, int tiles, int total) {
  constexpr int KM = 64;  // m rows per step
  constexpr int WGC = 2, WGI = 2;  // 4 waves, 2 over co x 2 over ci
  constexpr int WCO = BCO / WGC, WCI = BCI / WGI;
  constexpr int FCO = WCO / 16, FCI = WCI / 16;
  constexpr int IMG = KM * (BCO + BCI) * 2;  // bytes of one buffer
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  // XCD-aware id remap: XCD i runs logical ids [i*per, (i+1)*per)
  const int per = (int)gridDim.x >> 3;
  const int logical = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);
  if (logical >= total) return;
  const int split = logical / tiles;
  const int tile = logical - split * tiles;
  const int n0 = (tile % (N / BCO)) * BCO;
  const int k0 = (tile / (N / BCO)) * BCI;
  const int64_t m_begin = (int64_t)split * chunk;
  const int64_t m_end = m_begin + chunk < M ? m_begin + chunk : M;
  const int nfull = (int)((m_end - m_begin) / KM);
  const int nsteps = (int)((m_end - m_begin + KM - 1) / KM);

  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  auto dy_img = [&](int buf) { return lds_raw + buf * IMG; };
  auto x_img = [&](int buf) { return lds_raw + buf * IMG + KM * BCO * 2; };

  // stage rows [mt, mt+KM) of g[:, ch0 : ch0+BC] into a [KM][BC] image
  auto stage_op = [&](char* img, const bf16* g, int stride, int ch0,
                      int64_t mt, bool full, auto bc_tag) {
    constexpr int BC = decltype(bc_tag)::value;
    constexpr int LPR = BC / 8;    // 16 B chunks (lanes) per row
    constexpr int RPP = 64 / LPR;  // rows per 1 KB piece
    const char* base = (const char*)(g + mt * (int64_t)stride + ch0);
    if (full) {
#pragma unroll
      for (int pp = 0; pp < (KM / RPP) / 4; ++pp) {
        const int p = wave + pp * 4;
        const int row = p * RPP + lane / LPR;
        const int ch = (lane % LPR) ^ wg_swz<BC>(row);
        glds16((const bf16*)(base + (int64_t)row * stride * 2 + ch * 16),
               (bf16*)(img + p * 1024));
      }
    } else {
#pragma unroll
      for (int it = 0; it < (KM * LPR) / 256; ++it) {
        const int idx = (int)threadIdx.x + it * 256;
        const int row = idx / LPR;
        const int ch = (idx % LPR) ^ wg_swz<BC>(row);
        Vec<bf16, 8> v;
        if (mt + row < m_end) {
          v = vload<bf16, 8>(
              (const bf16*)(base + (int64_t)row * stride * 2 + ch * 16));
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v.v[j] = from_f32<bf16>(0.f);
        }
        vstore<bf16, 8>((bf16*)(img + idx * 16), v);
      }
    }
  };
  auto stage = [&](int buf, int s) {
    const int64_t mt = m_begin + (int64_t)s * KM;
    const bool full = s < nfull;  // block-uniform
    stage_op(dy_img(buf), dy, N, n0, mt, full,
             std::integral_constant<int, BCO>{});
    stage_op(x_img(buf), x, K, k0, mt, full,
             std::integral_constant<int, BCI>{});
  };

  // per-lane fragment read offsets: lane 4q+p of group g supplies the
  // address of row 8g+q (+32ks +4h as an immediate), columns 4p..4p+3 of the
  // fragment's 16 channels. wg_swz depends only on (q, g) for those rows.
  const int fg = lane >> 4, fq = (lane >> 2) & 3, fp = lane & 3;
  const int frow = 8 * fg + fq;
  int offa[FCO], offb[FCI];
#pragma unroll
  for (int mi = 0; mi < FCO; ++mi) {
    const int chunk16 = ((wave / WGI) * WCO + mi * 16) / 8 + (fp >> 1);
    offa[mi] = frow * (BCO * 2) + ((chunk16 ^ wg_swz<BCO>(frow)) << 4) +
               8 * (fp & 1);
  }
#pragma unroll
  for (int ni = 0; ni < FCI; ++ni) {
    const int chunk16 = ((wave % WGI) * WCI + ni * 16) / 8 + (fp >> 1);
    offb[ni] = frow * (BCI * 2) + ((chunk16 ^ wg_swz<BCI>(frow)) << 4) +
               8 * (fp & 1);
  }
  auto tr_frag = [&](const char* p, int rowb) {
    using lds_v4 = __attribute__((address_space(3))) bf16x4;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)p);
    const bf16x4 hi =
        __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(p + 4 * rowb));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  };

  f32x4 acc[FCO][FCI];
#pragma unroll
  for (int mi = 0; mi < FCO; ++mi)
#pragma unroll
    for (int ni = 0; ni < FCI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  for (int s = 0; s < nsteps; ++s) {
    // step s has landed (vmcnt(0) in the barrier) and every wave is done
    // reading the other buffer
    __syncthreads();
    if (s + 1 < nsteps) stage((s + 1) & 1, s + 1);
    const char* da = dy_img(s & 1);
    const char* xa = x_img(s & 1);
#pragma unroll
    for (int ks = 0; ks < KM / 32; ++ks) {
      bf16x8 af[FCO], bfr[FCI];
#pragma unroll
      for (int mi = 0; mi < FCO; ++mi)
        af[mi] = tr_frag(da + ks * 32 * (BCO * 2) + offa[mi], BCO * 2);
#pragma unroll
      for (int ni = 0; ni < FCI; ++ni)
        bfr[ni] = tr_frag(xa + ks * 32 * (BCI * 2) + offb[ni], BCI * 2);
#pragma unroll
      for (int mi = 0; mi < FCO; ++mi)
#pragma unroll
        for (int ni = 0; ni < FCI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
    }
  }

  float* o = out + (int64_t)split * N * K;
  const int wco = (wave / WGI) * WCO, wci = (wave % WGI) * WCI;
#pragma unroll
  for (int mi = 0; mi < FCO; ++mi)
#pragma unroll
    for (int ni = 0; ni < FCI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = n0 + wco + mi * 16 + (lane >> 4) * 4 + r;
        const int ci = k0 + wci + ni * 16 + (lane & 15);
        o[(int64_t)co * K + ci] = acc[mi][ni][r];
      }
}

// dW = sum over splits of slab[split], in an order fixed by (splits, G):
// thread (g, o) sums the splits [g*per, (g+1)*per) of float4 output o in
// ascending order, then the G group sums are added in ascending g. G > 1
// gives a small weight with many splits enough threads to pull the slab.
// G is a power of two <= 64; n4 = N*K/4 is a multiple of 256.
__global__ __launch_bounds__(256) void wgrad_finalize_kernel(
    const float* __restrict__ slab, float* __restrict__ dW, int n4,
    int splits, int G, int per) {
  __shared__ f32x4 part[256];
  const int outs = 256 / G;  // float4 outputs per block
  const int g = threadIdx.x / outs, o = threadIdx.x % outs;
  const int i = blockIdx.x * outs + o;
  const f32x4* p = (const f32x4*)slab + i;
  const int z0 = g * per;
  const int z1 = z0 + per < splits ? z0 + per : splits;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int z = z0; z < z1; ++z) s += p[(int64_t)z * n4];
  if (G == 1) {  // block-uniform
    ((f32x4*)dW)[i] = s;
    return;
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if (g == 0) {
    for (int j = 1; j < G; ++j) s += part[j * outs + o];
    ((f32x4*)dW)[i] = s;
  }
}

}  // namespace dla

// A [M,K] bf16, B [N,K] bf16 -> C = A @ B^T [M,N] bf16, with fused epilogue.
// Returns {C, sums}: the [gx, 2N] forward stats slab with want_stats, the
// [gx, NS*N] backward-stats slab with bwd != BWD_NONE (be.slab is set here),
// else empty. Tile selection is the same for every mode.
static std::vector<torch::Tensor> conv1x1_run(
    torch::Tensor a, torch::Tensor b, c10::optional<torch::Tensor> bias,
    c10::optional<torch::Tensor> scale, c10::optional<torch::Tensor> shift,
    c10::optional<torch::Tensor> residual, bool relu, bool want_stats,
    int bwd, dla::BwdEpi be) {
  DLA_CHECK_INPUT(a);
  DLA_CHECK_INPUT(b);
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 &&
                  b.scalar_type() == torch::kBFloat16,
              "conv1x1_fwd: bf16 only");
  const int64_t M = a.size(0);
  const int K = (int)a.size(1), N = (int)b.size(0);
  TORCH_CHECK((int)b.size(1) == K, "conv1x1_fwd: K mismatch");
  TORCH_CHECK(K % 64 == 0 && N % 64 == 0, "conv1x1_fwd: K,N must be %64");
  TORCH_CHECK(bwd == dla::BWD_NONE || !want_stats,
              "conv1x1: forward and backward stats do not combine");
  auto C = torch::empty({M, N}, a.options());
  auto opts_f = a.options().dtype(torch::kFloat);
  const int gx = (int)((M + 127) / 128);
  // per-block stats partials (fully written by the kernel; reduced to [2N]
  // by the caller with one torch sum — no global atomics)
  auto sums = want_stats ? torch::empty({gx, 2 * N}, opts_f)
                         : torch::empty({0}, opts_f);
  if (bwd != dla::BWD_NONE) {
    sums = torch::empty({gx, (bwd == dla::BWD_JOIN_DUAL ? 3 : 2) * N}, opts_f);
    be.slab = sums.data_ptr<float>();
  }
  const dla::bf16* res_p =
      residual.has_value() ? (const dla::bf16*)residual->data_ptr() : nullptr;
  const float* bias_p = bias.has_value() ? bias->data_ptr<float>() : nullptr;
  const float* scale_p = scale.has_value() ? scale->data_ptr<float>() : nullptr;
  const float* shift_p = shift.has_value() ? shift->data_ptr<float>() : nullptr;
  float* sums_p = want_stats ? sums.data_ptr<float>() : nullptr;

  const int nk = K / 64;
  auto launch_mode = [&](auto bntag, auto stag, auto bktag, auto modetag) {
    constexpr int BN = decltype(bntag)::value;
    constexpr bool ST = decltype(stag)::value;
    constexpr int BKT = decltype(bktag)::value;
    constexpr int MODE = decltype(modetag)::value;
    constexpr int NW = (BN == 256) ? 8 : 4;
    constexpr int WM = (BN == 64) ? 32 : 64;
    // single staging buffer suffices when there is only one K-step; with one
    // K-step A skips LDS entirely (direct-global fragments)
    const int nbuf = K / BKT > 1 ? 2 : 1;
    const int lds_stage = (128 * BKT + BN * BKT) * 2 * nbuf;
    // chunked transpose scratch: half a wave-tile when MFR >= 4
    const int lds_ep = NW * (WM >= 64 ? WM / 2 : WM) * (64 + 8) * 2;
    const int lds_st = ST ? ((BN == 64) ? 4 : 2) * 2 * BN * 4 : 0;
    const int lds = std::max(std::max(lds_stage, lds_ep), lds_st);
    if (lds > 65536) {
      static bool done[2] = {false, false};
      if (!done[ST]) {
        (void)hipFuncSetAttribute(
            (const void*)&dla::conv1x1_nt_kernel<BN, ST, BKT, 1, 0, MODE>,
            hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
        done[ST] = true;
      }
    }
    hipLaunchKernelGGL((dla::conv1x1_nt_kernel<BN, ST, BKT, 1, 0, MODE>),
                       dim3(N / BN, gx), dim3(NW * 64), lds, dla::stream(),
                       (const dla::bf16*)a.data_ptr(),
                       (const dla::bf16*)b.data_ptr(),
                       (dla::bf16*)C.data_ptr(), res_p, bias_p, scale_p,
                       shift_p, sums_p, M, K, N, relu, 0, 0, be);
  };
  auto launch = [&](auto bntag, auto stag, auto bktag) {
    using std::integral_constant;
    if constexpr (decltype(stag)::value || decltype(bntag)::value == 256) {
      launch_mode(bntag, stag, bktag, integral_constant<int, dla::BWD_NONE>{});
    } else {
      switch (bwd) {
        case dla::BWD_RELU_X:
          launch_mode(bntag, stag, bktag,
                      integral_constant<int, dla::BWD_RELU_X>{});
          break;
        case dla::BWD_JOIN:
          launch_mode(bntag, stag, bktag,
                      integral_constant<int, dla::BWD_JOIN>{});
          break;
        case dla::BWD_JOIN_DUAL:
          launch_mode(bntag, stag, bktag,
                      integral_constant<int, dla::BWD_JOIN_DUAL>{});
          break;
        default:
          launch_mode(bntag, stag, bktag,
                      integral_constant<int, dla::BWD_NONE>{});
      }
    }
  };
  // BK=32 halves the staging LDS (4 blocks/CU): measured +5% at K=128
  // (nk==2, the exposed-drain case), neutral/negative deeper — default it
  // only there (DLA_C1X1_BK32=1 forces it for all BN=128 shapes).
  static const bool bk32_force = []{
    const char* e = std::getenv("DLA_C1X1_BK32");
    return e != nullptr && e[0] == '1';
  }();
  // 4-slot glds ring (BK=32, 64KB LDS, 2 blocks/CU) — opt-in pending A/B
  // on the wait-bound fat-N shapes (ROADMAP item 2; guide "3-buf span +83%")
  static const bool ring_on = []{
    const char* e = std::getenv("DLA_C1X1_RING");
    return e != nullptr && e[0] == '1';
  }();
  const bool bk32 = bk32_force || nk == 2;
  auto launch_ring = [&](auto stag) {
    constexpr bool ST = decltype(stag)::value;
    constexpr int lds = 4 * (128 * 32 + 128 * 32) * 2;  // 64 KB
    hipLaunchKernelGGL((dla::conv1x1_nt_kernel<128, ST, 32, 1, 4>),
                       dim3(N / 128, gx), dim3(256), lds, dla::stream(),
                       (const dla::bf16*)a.data_ptr(),
                       (const dla::bf16*)b.data_ptr(),
                       (dla::bf16*)C.data_ptr(), res_p, bias_p, scale_p,
                       shift_p, sums_p, M, K, N, relu);
  };
  auto pick = [&](auto bntag) {
    constexpr int BNv = decltype(bntag)::value;
    if (BNv == 128 && ring_on && bwd == dla::BWD_NONE && K % 32 == 0 &&
        K / 32 >= 4) {
      if (want_stats) launch_ring(std::true_type{});
      else launch_ring(std::false_type{});
      return;
    }
    if (BNv == 128 && bk32 && nk >= 2) {
      if (want_stats) launch(bntag, std::true_type{},
                             std::integral_constant<int, 32>{});
      else launch(bntag, std::false_type{}, std::integral_constant<int, 32>{});
      return;
    }
    if (want_stats) launch(bntag, std::true_type{},
                           std::integral_constant<int, 64>{});
    else launch(bntag, std::false_type{}, std::integral_constant<int, 64>{});
  };
  // BN=256 (512 threads, single A pass) wins only at nk==1 where the LDS
  // fits 3 blocks/CU; at nk>=2 its 96KB double-buffer drops occupancy to
  // 1 block/CU and BN=128 (2 blocks/CU) measures faster.
  // The backward-stats modes take BN=128 there: 0.35 ms at 802816x64x256
  // (the byte floor) against 0.51 ms for a BN=256 variant
  // (profiles/bwdstats_epilogue_ab.txt).
  if (N % 256 == 0 && nk == 1 && bwd == dla::BWD_NONE)
    pick(std::integral_constant<int, 256>{});
  else if (N % 128 == 0) pick(std::integral_constant<int, 128>{});
  else pick(std::integral_constant<int, 64>{});
  HIP_CHECK_ERR();
  return {C, sums};
}

std::vector<torch::Tensor> conv1x1_fwd(torch::Tensor a, torch::Tensor b,
                                       c10::optional<torch::Tensor> bias,
                                       c10::optional<torch::Tensor> scale,
                                       c10::optional<torch::Tensor> shift,
                                       c10::optional<torch::Tensor> residual,
                                       bool relu, bool want_stats) {
  return conv1x1_run(a, b, bias, scale, shift, residual, relu, want_stats,
                     dla::BWD_NONE, dla::BwdEpi{});
}

// dgrad with the backward-stats epilogue: dy [M,K] bf16, wt [N,K] bf16 (the
// transposed weight), optional residual [M,N] (the identity gradient).
//   mode 1 (RELU_X):    x, scale, shift, mean, rstd
//   mode 2 (JOIN):      out, x, mean, rstd
//   mode 3 (JOIN_DUAL): out, x, mean, rstd, xd, mean_d, rstd_d
// out / x / xd are [M,N] bf16 rows (NHWC tensors pass as they are), the
// per-channel tensors fp32 [N]. Returns {g [M,N] bf16, slab [ceil(M/128),
// NS*N] fp32}; g is the masked dgrad output, bit for bit what pass 1 of the
// BN backward would write from the plain dgrad output.
std::vector<torch::Tensor> conv1x1_dgrad_bwdstats(
    torch::Tensor dy, torch::Tensor wt, c10::optional<torch::Tensor> residual,
    int64_t mode, c10::optional<torch::Tensor> out, torch::Tensor x,
    c10::optional<torch::Tensor> scale, c10::optional<torch::Tensor> shift,
    torch::Tensor mean, torch::Tensor rstd, c10::optional<torch::Tensor> xd,
    c10::optional<torch::Tensor> mean_d, c10::optional<torch::Tensor> rstd_d) {
  TORCH_CHECK(mode >= dla::BWD_RELU_X && mode <= dla::BWD_JOIN_DUAL,
              "conv1x1_dgrad_bwdstats: mode must be 1, 2 or 3");
  const int64_t M = dy.size(0), N = wt.size(0);
  auto rows_ok = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
           t.numel() == M * N &&
           (t.dim() == 2 ? t.is_contiguous() && t.size(1) == N
                         : t.dim() == 4 && t.size(1) == N &&
                               t.is_contiguous(at::MemoryFormat::ChannelsLast));
  };
  auto chan_ok = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.scalar_type() == torch::kFloat &&
           t.is_contiguous() && t.numel() == N;
  };
  TORCH_CHECK(rows_ok(x), "conv1x1_dgrad_bwdstats: x must be [M,N] bf16 rows");
  TORCH_CHECK(chan_ok(mean) && chan_ok(rstd),
              "conv1x1_dgrad_bwdstats: mean/rstd must be fp32 [N]");
  TORCH_CHECK(!residual.has_value() ||
                  (rows_ok(*residual) && residual->dim() == 2),
              "conv1x1_dgrad_bwdstats: residual must be [M,N] bf16");
  dla::BwdEpi be{};
  be.x = (const dla::bf16*)x.data_ptr();
  be.mean = mean.data_ptr<float>();
  be.rstd = rstd.data_ptr<float>();
  if (mode == dla::BWD_RELU_X) {
    TORCH_CHECK(scale.has_value() && shift.has_value() && chan_ok(*scale) &&
                    chan_ok(*shift),
                "conv1x1_dgrad_bwdstats: RELU_X needs fp32 [N] scale/shift");
    be.scale = scale->data_ptr<float>();
    be.shift = shift->data_ptr<float>();
  } else {
    TORCH_CHECK(out.has_value() && rows_ok(*out),
                "conv1x1_dgrad_bwdstats: JOIN needs out as [M,N] bf16 rows");
    be.out = (const dla::bf16*)out->data_ptr();
  }
  if (mode == dla::BWD_JOIN_DUAL) {
    TORCH_CHECK(xd.has_value() && rows_ok(*xd) && mean_d.has_value() &&
                    rstd_d.has_value() && chan_ok(*mean_d) && chan_ok(*rstd_d),
                "conv1x1_dgrad_bwdstats: JOIN_DUAL needs xd, mean_d, rstd_d");
    be.xd = (const dla::bf16*)xd->data_ptr();
    be.mean_d = mean_d->data_ptr<float>();
    be.rstd_d = rstd_d->data_ptr<float>();
  }
  return conv1x1_run(dy, wt, c10::nullopt, c10::nullopt, c10::nullopt,
                     residual, false, false, (int)mode, be);
}

// 3x3 stride-1 pad-1 conv as tap-major implicit GEMM (TAPS=9 variant of
// the kernel above). a: x flattened NHWC [M=B*H*W, Cin]; w9: weight
// pre-permuted to [Co, 9*Cin] (tap-major: permute(0,2,3,1) of the torch
// [Co,Ci,3,3] layout). Returns {y [M,Co], stats partials}.
std::vector<torch::Tensor> conv3x3_fwd(torch::Tensor a, torch::Tensor w9,
                                       int64_t imgH, int64_t imgW,
                                       c10::optional<torch::Tensor> bias,
                                       c10::optional<torch::Tensor> scale,
                                       c10::optional<torch::Tensor> shift,
                                       c10::optional<torch::Tensor> residual,
                                       bool relu, bool want_stats) {
  DLA_CHECK_INPUT(a);
  DLA_CHECK_INPUT(w9);
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 &&
                  w9.scalar_type() == torch::kBFloat16,
              "conv3x3_fwd: bf16 only");
  const int64_t M = a.size(0);
  const int Cin = (int)a.size(1), N = (int)w9.size(0);
  const int K = 9 * Cin;
  TORCH_CHECK((int)w9.size(1) == K, "conv3x3_fwd: weight must be [Co, 9*Ci]");
  TORCH_CHECK(Cin % 64 == 0 && N % 64 == 0, "conv3x3_fwd: C must be %64");
  TORCH_CHECK(M % (imgH * imgW) == 0, "conv3x3_fwd: M != B*H*W");
  auto C = torch::empty({M, N}, a.options());
  auto opts_f = a.options().dtype(torch::kFloat);
  const int gx = (int)((M + 127) / 128);
  auto sums = want_stats ? torch::empty({gx, 2 * N}, opts_f)
                         : torch::empty({0}, opts_f);
  const dla::bf16* res_p =
      residual.has_value() ? (const dla::bf16*)residual->data_ptr() : nullptr;
  const float* bias_p = bias.has_value() ? bias->data_ptr<float>() : nullptr;
  const float* scale_p = scale.has_value() ? scale->data_ptr<float>() : nullptr;
  const float* shift_p = shift.has_value() ? shift->data_ptr<float>() : nullptr;
  float* sums_p = want_stats ? sums.data_ptr<float>() : nullptr;
  auto launch = [&](auto bntag, auto stag) {
    constexpr int BN = decltype(bntag)::value;
    constexpr bool ST = decltype(stag)::value;
    const int lds_stage = (128 * 64 + BN * 64) * 2 * 2;
    const int lds_ep = 4 * ((BN == 64) ? 32 : 64) / ((BN == 64) ? 1 : 2) *
                       (64 + 8) * 2;
    const int lds_st = ST ? ((BN == 64) ? 4 : 2) * 2 * BN * 4 : 0;
    const int lds = std::max(std::max(lds_stage, lds_ep), lds_st);
    hipLaunchKernelGGL((dla::conv1x1_nt_kernel<BN, ST, 64, 9>),
                       dim3(N / BN, gx), dim3(256), lds, dla::stream(),
                       (const dla::bf16*)a.data_ptr(),
                       (const dla::bf16*)w9.data_ptr(),
                       (dla::bf16*)C.data_ptr(), res_p, bias_p, scale_p,
                       shift_p, sums_p, M, K, N, relu, (int)imgH, (int)imgW);
  };
  auto pick = [&](auto bntag) {
    if (want_stats) launch(bntag, std::true_type{});
    else launch(bntag, std::false_type{});
  };
  if (N % 128 == 0) pick(std::integral_constant<int, 128>{});
  else pick(std::integral_constant<int, 64>{});
  HIP_CHECK_ERR();
  return {C, sums};
}

// wgrad v2 launcher: tile choice, M-split count, slab + finalize.
static torch::Tensor conv1x1_wgrad_v2(const torch::Tensor& dy,
                                      const torch::Tensor& x, int64_t M,
                                      int K, int N) {
  auto opts_f = x.options().dtype(torch::kFloat);
  if (M == 0) return torch::zeros({N, K}, opts_f);
  auto dW = torch::empty({N, K}, opts_f);
  auto launch = [&](auto cotag, auto citag) {
    constexpr int BCO = decltype(cotag)::value;
    constexpr int BCI = decltype(citag)::value;
    constexpr int lds = 2 * 64 * (BCO + BCI) * 2;
    constexpr int bpc = std::min(4, 163840 / lds);  // resident blocks per CU
    const int tiles = (N / BCO) * (K / BCI);
    // enough splits for one resident wave of blocks on 256 CUs, but chunks
    // of at least 4 steps, and slab traffic (write + read, 8 B per output
    // and split) no more than the operand bytes 2*M*(N+K)
    int64_t s = std::max<int64_t>(1, (256 * bpc) / tiles);
    s = std::min<int64_t>(s, std::max<int64_t>(1, M / 256));
    s = std::min<int64_t>(
        s, std::max<int64_t>(1, M * (N + K) / (4 * (int64_t)N * K)));
    const int64_t chunk = (((M + s - 1) / s + 63) / 64) * 64;
    const int splits = (int)((M + chunk - 1) / chunk);
    const int total = tiles * splits;
    torch::Tensor slab;
    float* out = dW.data_ptr<float>();
    if (splits > 1) {
      slab = torch::empty({splits, N, K}, opts_f);
      out = slab.data_ptr<float>();
    }
    static_assert(lds <= 65536, "needs hipFuncSetAttribute above 64 KB");
    hipLaunchKernelGGL((dla::conv1x1_wgrad2_kernel<BCO, BCI>),
                       dim3(((total + 7) / 8) * 8), dim3(256), lds,
                       dla::stream(), (const dla::bf16*)dy.data_ptr(),
                       (const dla::bf16*)x.data_ptr(), out, M, K, N, chunk,
                       tiles, total);
    if (splits > 1) {
      const int n4 = N * K / 4;
      // split groups per output: enough for ~64 K threads to pull the slab,
      // while each group still sums at least 4 splits
      int G = 1;
      while (G < 64 && n4 * G < 65536 && splits >= 8 * G) G *= 2;
      hipLaunchKernelGGL(dla::wgrad_finalize_kernel, dim3(n4 / (256 / G)),
                         dim3(256), 0, dla::stream(), (const float*)out,
                         dW.data_ptr<float>(), n4, splits, G,
                         (splits + G - 1) / G);
    }
  };
  using std::integral_constant;
  const bool n128 = N % 128 == 0, k128 = K % 128 == 0;
  // 128x128 measured best wherever it divides; a whole-weight 256x64 /
  // 64x256 tile and 64x128 / 128x64 at the fat weights were no faster
  // (profiles/wgrad_v2_ab.txt)
  if (n128 && k128)
    launch(integral_constant<int, 128>{}, integral_constant<int, 128>{});
  else if (k128)
    launch(integral_constant<int, 64>{}, integral_constant<int, 128>{});
  else if (n128)
    launch(integral_constant<int, 128>{}, integral_constant<int, 64>{});
  else
    launch(integral_constant<int, 64>{}, integral_constant<int, 64>{});
  HIP_CHECK_ERR();
  return dW;
}

// dW[N,K] fp32 = dy[M,N]^T @ x[M,K]
torch::Tensor conv1x1_wgrad(torch::Tensor dy, torch::Tensor x) {
  DLA_CHECK_INPUT(dy);
  DLA_CHECK_INPUT(x);
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
                  x.scalar_type() == torch::kBFloat16,
              "conv1x1_wgrad: bf16 only");
  const int64_t M = x.size(0);
  const int K = (int)x.size(1), N = (int)dy.size(1);
  TORCH_CHECK(dy.size(0) == M, "conv1x1_wgrad: M mismatch");
  TORCH_CHECK(K % 64 == 0 && N % 64 == 0, "conv1x1_wgrad: K,N must be %64");
  // DLA_C1X1_WGRAD_V1=1: the scatter-staged, atomicAdd kernel (same-build A/B)
  const char* v1 = std::getenv("DLA_C1X1_WGRAD_V1");
  if (v1 == nullptr || v1[0] != '1') return conv1x1_wgrad_v2(dy, x, M, K, N);
  auto dW = torch::zeros({N, K}, x.options().dtype(torch::kFloat));
  auto launch = [&](auto cotag, auto citag) {
    constexpr int BCO = decltype(cotag)::value;
    constexpr int BCI = decltype(citag)::value;
    const int tiles = (N / BCO) * (K / BCI);
    int splits = (int)std::min<int64_t>(
        std::max<int64_t>(1, 1024 / tiles),
        (M + 2047) / 2048);
    const int64_t chunk0 = (M + splits - 1) / splits;
    const int64_t chunk = ((chunk0 + 63) / 64) * 64;  // multiple of KM
    splits = (int)((M + chunk - 1) / chunk);
    const int lds = 2 * (BCO + BCI) * 72 * 2;
    if (lds > 65536) {
      static bool done = false;
      if (!done) {
        (void)hipFuncSetAttribute(
            (const void*)&dla::conv1x1_wgrad_kernel<BCO, BCI>,
            hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
        done = true;
      }
    }
    hipLaunchKernelGGL((dla::conv1x1_wgrad_kernel<BCO, BCI>),
                       dim3(N / BCO, K / BCI, splits),
                       dim3(BCO * BCI >= 8192 ? 512 : 256), lds,
                       dla::stream(), (const dla::bf16*)dy.data_ptr(),
                       (const dla::bf16*)x.data_ptr(), dW.data_ptr<float>(),
                       M, K, N, chunk);
  };
  // pick the instantiated tile minimizing re-read traffic; (256,64) measured
  // slower than (128,64) (1 block/CU, staging-bound) so 128 caps BCO
  const bool n128 = N % 128 == 0, k128 = K % 128 == 0;
  if (n128 && k128)
    launch(std::integral_constant<int, 128>{}, std::integral_constant<int, 128>{});
  else if (k128)
    launch(std::integral_constant<int, 64>{}, std::integral_constant<int, 128>{});
  else if (n128)
    launch(std::integral_constant<int, 128>{}, std::integral_constant<int, 64>{});
  else
    launch(std::integral_constant<int, 64>{}, std::integral_constant<int, 64>{});
  HIP_CHECK_ERR();
  return dW;
}

// dW9 [Co, 9*Ci] fp32 = 3x3 s1 p1 wgrad (tap-major k, same order the
// conv3x3_fwd weight uses)
torch::Tensor conv3x3_wgrad(torch::Tensor dy, torch::Tensor x, int64_t imgH,
                            int64_t imgW) {
  DLA_CHECK_INPUT(dy);
  DLA_CHECK_INPUT(x);
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
                  x.scalar_type() == torch::kBFloat16,
              "conv3x3_wgrad: bf16 only");
  const int64_t M = x.size(0);
  const int Cin = (int)x.size(1), N = (int)dy.size(1);
  const int K = 9 * Cin;
  TORCH_CHECK(dy.size(0) == M, "conv3x3_wgrad: M mismatch");
  TORCH_CHECK(Cin % 64 == 0 && N % 64 == 0, "conv3x3_wgrad: C must be %64");
  auto dW = torch::zeros({N, K}, x.options().dtype(torch::kFloat));
  auto launch = [&](auto cotag, auto citag) {
    constexpr int BCO = decltype(cotag)::value;
    constexpr int BCI = decltype(citag)::value;
    const int tiles = (N / BCO) * (3 * Cin / BCI);  // ky-row-merged grid
    int splits = (int)std::min<int64_t>(
        std::max<int64_t>(1, 1024 / tiles),
        (M + 2047) / 2048);
    const int64_t chunk0 = (M + splits - 1) / splits;
    const int64_t chunk = ((chunk0 + 63) / 64) * 64;
    splits = (int)((M + chunk - 1) / chunk);
    const int lds = 2 * (BCO + BCI) * 72 * 2;
    if (lds > 65536) {
      static bool done = false;
      if (!done) {
        (void)hipFuncSetAttribute(
            (const void*)&dla::conv1x1_wgrad_kernel<BCO, BCI, 9>,
            hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
        done = true;
      }
    }
    hipLaunchKernelGGL((dla::conv1x1_wgrad_kernel<BCO, BCI, 9>),
                       dim3(N / BCO, 3 * Cin / BCI, splits),
                       dim3(BCO * BCI >= 8192 ? 512 : 256), lds,
                       dla::stream(), (const dla::bf16*)dy.data_ptr(),
                       (const dla::bf16*)x.data_ptr(), dW.data_ptr<float>(),
                       M, K, N, chunk, (int)imgH, (int)imgW);
  };
  // BCI must divide Cin so a ci tile stays inside one tap plane
  const bool n128 = N % 128 == 0, ci128 = Cin % 128 == 0;
  if (n128 && ci128)
    launch(std::integral_constant<int, 128>{}, std::integral_constant<int, 128>{});
  else if (ci128)
    launch(std::integral_constant<int, 64>{}, std::integral_constant<int, 128>{});
  else if (n128)
    launch(std::integral_constant<int, 128>{}, std::integral_constant<int, 64>{});
  else
    launch(std::integral_constant<int, 64>{}, std::integral_constant<int, 64>{});
  HIP_CHECK_ERR();
  return dW;
}
