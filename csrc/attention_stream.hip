// Streaming fused attention for CDNA4 (gfx950): the plain (no bias, no mask,
// no cosine) path of csrc/attention.hip for sequences that do not fit its
// resident kernels (N > 256: ViT-B/16 at 384^2 has N = 577, 448^2 has 785).
//
// The resident kernels keep all of K and V^T of one (b, h) in LDS and a whole
// score row in s_acc[16]. Here a block owns 128 rows (8 waves x 16) of one
// (b, h) and LOOPS over panels of the other sequence axis, staging one panel
// at a time into LDS and running the resident kernels' per-panel body on it:
//  - forward: key panels of PANEL keys; a running (m, l) per row and an
//    online rescale of o_acc carry the softmax across panels;
//  - backward kv: each wave owns 16 keys, loops over 64-query panels;
//  - backward q : each wave owns 16 queries, loops over 64-key panels.
// Every output element is produced by exactly one wave and written once: no
// atomics, no zero fill, no workspace, bit-reproducible. No [B,H,N,N] tensor
// reaches HBM; backward recomputes P from the forward's (m, l) stats, which
// have the resident kernels' [2,B,H,N] layout, so either backward can consume
// either forward's stats.
//
// Fragment conventions, LDS strides and the same-wave LDS visibility fences
// are those of csrc/attention.hip (16x16x32 bf16 MFMA; C/D row =
// (lane>>4)*4 + reg, col = lane&15).
// Shape domain: bf16, d in {32, 64}, 1 <= N <= 4096.
#include "common.h"
#include "vec.h"

namespace dla {
namespace attn_stream {

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int KPAD = 72;         // LDS row stride of row-major tiles (bf16)
constexpr int CHUNK = 64;        // keys/queries per P-staging chunk (4 tiles)
constexpr int PBUF = 16 * KPAD;  // per-wave P chunk buffer elems
constexpr int NWAVES = 8;
constexpr int ROWS = NWAVES * 16;  // rows of the owned axis per block
// Rows of the streamed axis per backward panel. 64 keeps both backward
// kernels under 80 KB of LDS (two blocks per CU): measured 0.85 ms against
// 1.29 ms for 128-row panels (one block per CU) at B64 N577 H12 d64, with
// bit-identical dqkv (profiles/attn_stream_ab.txt).
constexpr int BWD_PANEL = 64;

// LDS bytes of the three kernels (host launch code and docs/KERNELS.md)
constexpr int fwd_lds_bytes(int D, int panel) {
  return (panel * KPAD + D * (panel + 8) + NWAVES * 2 * PBUF) * 2;
}
constexpr int bwd_kv_lds_bytes(int D) {
  return (2 * BWD_PANEL * KPAD + 2 * D * (BWD_PANEL + 8) +
          NWAVES * 2 * PBUF) * 2;
}
constexpr int bwd_q_lds_bytes(int D) {
  return (2 * BWD_PANEL * KPAD + D * (BWD_PANEL + 8) + NWAVES * 2 * PBUF) * 2;
}

// Stage rows [n0, n0 + npad) of a strided bf16 [N][D] source into LDS
// row-major (row stride KPAD) and/or transposed (dst_t[d][VROW]); panel-local
// rows >= nvalid are zero-filled, never read from global.
template <int D>
__device__ void stage_panel(const __hip_bfloat16* src, int64_t row_stride,
                            __hip_bfloat16* dst_rows, __hip_bfloat16* dst_t,
                            int n0, int nvalid, int npad, int VROW) {
  for (int n = threadIdx.x / (D / 4); n < npad;
       n += blockDim.x / (D / 4)) {
    const int d0 = (threadIdx.x % (D / 4)) * 4;
    Vec<__hip_bfloat16, 4> v;
    if (n < nvalid) {
      v = vload<__hip_bfloat16, 4>(src + (int64_t)(n0 + n) * row_stride + d0);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v.v[j] = __hip_bfloat16(0.f);
    }
    if (dst_rows) vstore<__hip_bfloat16, 4>(&dst_rows[n * KPAD + d0], v);
    if (dst_t) {
#pragma unroll
      for (int j = 0; j < 4; ++j) dst_t[(d0 + j) * VROW + n] = v.v[j];
    }
  }
}

// ---------------------------------------------------------------- forward --
// grid (B*H, ceil(N/128)), 512 threads. PANEL in {128, 256} keys per panel.
template <int D, int PANEL>
__global__ __launch_bounds__(512)
void attn_fwd_stream_kernel(const __hip_bfloat16* __restrict__ qkv,  // [B,N,3,H,D]
                            __hip_bfloat16* __restrict__ out,        // [B,N,H*D]
                            float* __restrict__ stats,  // [2,B,H,N]|null
                            int B, int N, int H, float scale) {
  constexpr int KSLICES = D / 32;
  constexpr int NT = PANEL / 16;  // key tiles per panel
  constexpr int VROW = PANEL + 8;
  const int b = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // A wave whose rows lie at or past N still walks every panel (it must
  // reach each barrier); it computes on a clamped row and stores nothing.
  const int q0 = blockIdx.y * ROWS + wave * 16;

  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  __hip_bfloat16* k_lds = (__hip_bfloat16*)lds_raw;  // [PANEL][KPAD]
  __hip_bfloat16* vt_lds = k_lds + PANEL * KPAD;     // [D][VROW]
  __hip_bfloat16* p_lds = vt_lds + D * VROW;         // [NWAVES][2*PBUF]
  __hip_bfloat16* p_buf = p_lds + wave * 2 * PBUF;   // double-buffered

  const int64_t bh_stride = (int64_t)3 * H * D;
  const __hip_bfloat16* q_src = qkv + (int64_t)b * N * 3 * H * D +
                                (int64_t)h * D;
  const __hip_bfloat16* k_src = q_src + (int64_t)H * D;
  const __hip_bfloat16* v_src = q_src + (int64_t)2 * H * D;

  bf16x8 q_frag[KSLICES];
  {
    const int row = q0 + (lane & 15);
    const int srow = row < N ? row : N - 1;
#pragma unroll
    for (int sl = 0; sl < KSLICES; ++sl) {
      const int d0 = sl * 32 + (lane >> 4) * 8;
      q_frag[sl] = *(const bf16x8*)(q_src + (int64_t)srow * bh_stride + d0);
    }
  }

  const int col = lane & 15;
  float m_run[4], l_run[4];
  f32x4 o_acc[D / 16];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -INFINITY;
    l_run[r] = 0.f;
  }
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) o_acc[dt] = {0.f, 0.f, 0.f, 0.f};

  for (int p0 = 0; p0 < N; p0 += PANEL) {
    const int pn = N - p0 < PANEL ? N - p0 : PANEL;  // valid keys, >= 1
    const int n_ktiles = (pn + 15) >> 4;
    const int pnpad = n_ktiles * 16;
    // the previous panel's K/V^T may still be read by a slower wave
    if (p0 > 0) __syncthreads();
    stage_panel<D>(k_src, bh_stride, k_lds, nullptr, p0, pn, pnpad, VROW);
    stage_panel<D>(v_src, bh_stride, nullptr, vt_lds, p0, pn, pnpad, VROW);
    __syncthreads();

    // S = Q K^T over the panel's key tiles (kept in VGPRs)
    f32x4 s_acc[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      if (kt < n_ktiles) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sl = 0; sl < KSLICES; ++sl) {
          const int key = kt * 16 + (lane & 15);
          const int d0 = sl * 32 + (lane >> 4) * 8;
          bf16x8 k_frag = *(const bf16x8*)(&k_lds[key * KPAD + d0]);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[sl], k_frag,
                                                        acc, 0, 0, 0);
        }
        s_acc[kt] = acc;
      }
    }

    // panel softmax, kt-outer so the 4 rows' chains interleave. Keys past
    // the panel's valid count get -inf; every panel holds a real key, so
    // the panel max (and from panel 0 on the running max) is finite and
    // -inf - m never meets -inf.
    float row_sum[4], mx[4], alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mx[r] = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      if (kt < n_ktiles) {
        const int key = kt * 16 + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sv = s_acc[kt][r] * scale;
          if (key >= pn) sv = -INFINITY;
          s_acc[kt][r] = sv;
          mx[r] = fmaxf(mx[r], sv);
        }
      }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], off, 64));
    // online rescale: alpha = exp(m_old - m_new); 0 on panel 0 (m_old=-inf)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float m_new = fmaxf(m_run[r], mx[r]);
      alpha[r] = __expf(m_run[r] - m_new);
      m_run[r] = m_new;
      row_sum[r] = 0.f;
    }
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      if (kt < n_ktiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __expf(s_acc[kt][r] - m_run[r]);
          s_acc[kt][r] = p;
          row_sum[r] += p;
        }
      }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        row_sum[r] += __shfl_xor(row_sum[r], off, 64);
#pragma unroll
    for (int r = 0; r < 4; ++r) l_run[r] = l_run[r] * alpha[r] + row_sum[r];
    // o_acc shares s_acc's C/D row mapping: alpha[r] applies per register
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) o_acc[dt][r] *= alpha[r];

    // O += P V through the per-wave P buffer, software-pipelined over two
    // buffers: chunk c+1's LDS writes are issued before chunk c's reads.
    auto write_pchunk = [&](int c) {
      const int t0 = c * 4;
      const int nt = n_ktiles - t0 < 4 ? n_ktiles - t0 : 4;
      __hip_bfloat16* pb = p_buf + (c & 1) * PBUF;
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        if (tt < nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            pb[((lane >> 4) * 4 + r) * KPAD + tt * 16 + col] =
                __hip_bfloat16(s_acc[tt + (c << 2)][r]);
        }
      }
    };
    write_pchunk(0);
#pragma unroll
    for (int c = 0; c < NT / 4; ++c) {  // chunks of 4 key tiles (64 keys)
      const int t0 = c * 4;
      if (t0 < n_ktiles) {
        const int nt = n_ktiles - t0 < 4 ? n_ktiles - t0 : 4;
        if (c + 1 < NT / 4 && (c + 1) * 4 < n_ktiles) write_pchunk(c + 1);
        const __hip_bfloat16* pb = p_buf + (c & 1) * PBUF;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          if (kk * 32 < nt * 16) {
            const int k0 = kk * 32 + (lane >> 4) * 8;
            const bool valid = k0 < nt * 16;
            bf16x8 p_frag{};
            if (valid)
              p_frag = *(const bf16x8*)(&pb[(lane & 15) * KPAD + k0]);
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) {
              const int d = dt * 16 + (lane & 15);
              bf16x8 v_frag{};
              if (valid)
                v_frag = *(const bf16x8*)(&vt_lds[d * VROW + c * CHUNK + k0]);
              o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  p_frag, v_frag, o_acc[dt], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  if (stats != nullptr && col == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0 + (lane >> 4) * 4 + r;
      if (qrow < N) {
        stats[((int64_t)b * H + h) * N + qrow] = m_run[r];
        stats[((int64_t)(B + b) * H + h) * N + qrow] = l_run[r];
      }
    }
  }

  // normalise once and store O through an LDS transpose (p_buf scratch):
  // coalesced 16-byte row stores instead of 2-byte column stores
  {
    float rinv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rinv[r] = 1.f / l_run[r];
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        p_buf[((lane >> 4) * 4 + r) * KPAD + dt * 16 + (lane & 15)] =
            __hip_bfloat16(o_acc[dt][r] * rinv[r]);
    // same-wave cross-lane LDS visibility: drain, and fence the reads
    // below from being hoisted above the drain
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < (16 * D / 8) / 64; ++i) {
      const int t = lane + 64 * i;
      const int row = t / (D / 8);
      const int c8 = t % (D / 8);
      const int qrow = q0 + row;
      if (qrow < N) {
        Vec<__hip_bfloat16, 8> v =
            vload<__hip_bfloat16, 8>(&p_buf[row * KPAD + c8 * 8]);
        vstore<__hip_bfloat16, 8>(
            out + ((int64_t)b * N + qrow) * H * D + h * D + c8 * 8, v);
      }
    }
  }
}

// --------------------------------------------------------------- backward --
// dV = P^T dO ; dP = dO V^T ; dS = P*(dP - D_row) ; dQ = scale*dS K ;
// dK = scale*dS^T Q.  P recomputed from (m, l); D_row precomputed by host.

// dK and dV. grid (B*H, ceil(N/128)); each wave owns 16 keys (k/v fragments
// in registers) and accumulates over 64-query panels of Q, dO, Q^T, dO^T.
template <int D>
__global__ __launch_bounds__(512)
void attn_bwd_kv_stream_kernel(const __hip_bfloat16* __restrict__ qkv,
                               const __hip_bfloat16* __restrict__ dout,
                               const float* __restrict__ stats,
                               const float* __restrict__ drow,
                               __hip_bfloat16* __restrict__ dqkv,
                               int B, int N, int H, float scale) {
  constexpr int KSLICES = D / 32;
  constexpr int QP = BWD_PANEL;
  constexpr int VROW = QP + 8;
  const int b = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int key0 = blockIdx.y * ROWS + wave * 16;  // may be >= N: no stores

  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  __hip_bfloat16* q_lds = (__hip_bfloat16*)lds_raw;  // [QP][KPAD]
  __hip_bfloat16* do_lds = q_lds + QP * KPAD;        // [QP][KPAD]
  __hip_bfloat16* qt_lds = do_lds + QP * KPAD;       // [D][VROW]
  __hip_bfloat16* dot_lds = qt_lds + D * VROW;       // [D][VROW]
  __hip_bfloat16* p_lds = dot_lds + D * VROW;        // [NWAVES][2*PBUF]
  __hip_bfloat16* p_buf = p_lds + wave * 2 * PBUF;   // P^T | dS^T buffers

  const int64_t bh_stride = (int64_t)3 * H * D;
  const __hip_bfloat16* q_src = qkv + (int64_t)b * N * 3 * H * D +
                                (int64_t)h * D;
  const __hip_bfloat16* k_src = q_src + (int64_t)H * D;
  const __hip_bfloat16* v_src = q_src + (int64_t)2 * H * D;
  const __hip_bfloat16* do_src = dout + (int64_t)b * N * H * D +
                                 (int64_t)h * D;
  const float* m_arr = stats + ((int64_t)b * H + h) * N;
  const float* l_arr = stats + ((int64_t)(B + b) * H + h) * N;
  const float* d_arr = drow + ((int64_t)b * H + h) * N;

  bf16x8 k_frag[KSLICES], v_frag[KSLICES];
  {
    const int key = key0 + (lane & 15);
    const int skey = key < N ? key : N - 1;
#pragma unroll
    for (int sl = 0; sl < KSLICES; ++sl) {
      const int d0 = sl * 32 + (lane >> 4) * 8;
      k_frag[sl] = *(const bf16x8*)(k_src + (int64_t)skey * bh_stride + d0);
      v_frag[sl] = *(const bf16x8*)(v_src + (int64_t)skey * bh_stride + d0);
    }
  }
  f32x4 dv_acc[D / 16], dk_acc[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    dv_acc[dt] = {0.f, 0.f, 0.f, 0.f};
    dk_acc[dt] = {0.f, 0.f, 0.f, 0.f};
  }

  for (int p0 = 0; p0 < N; p0 += QP) {
    const int pn = N - p0 < QP ? N - p0 : QP;  // valid queries in the panel
    const int n_qtiles = (pn + 15) >> 4;
    const int pnpad = n_qtiles * 16;
    if (p0 > 0) __syncthreads();  // slower waves still read the last panel
    stage_panel<D>(q_src, bh_stride, q_lds, qt_lds, p0, pn, pnpad, VROW);
    stage_panel<D>(do_src, (int64_t)H * D, do_lds, dot_lds, p0, pn, pnpad,
                   VROW);
    __syncthreads();

#pragma unroll
    for (int c = 0; c < QP / CHUNK; ++c) {  // 64-query chunks
      const int t0 = c * 4;
      if (t0 < n_qtiles) {
        const int nt = n_qtiles - t0 < 4 ? n_qtiles - t0 : 4;
        f32x4 st[4], dpt[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          if (tt < nt) {
            f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sl = 0; sl < KSLICES; ++sl) {
              const int q = (t0 + tt) * 16 + (lane & 15);
              const int d0 = sl * 32 + (lane >> 4) * 8;
              bf16x8 qb = *(const bf16x8*)(&q_lds[q * KPAD + d0]);
              bf16x8 db = *(const bf16x8*)(&do_lds[q * KPAD + d0]);
              sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k_frag[sl], qb,
                                                             sacc, 0, 0, 0);
              dacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v_frag[sl], db,
                                                             dacc, 0, 0, 0);
            }
            st[tt] = sacc;
            dpt[tt] = dacc;
          }
        }
        // P^T and scale*dS^T for this chunk; stage both, accumulate dV
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          if (tt < nt) {
            const int q = (t0 + tt) * 16 + (lane & 15);  // panel-local
            const float m = q < pn ? m_arr[p0 + q] : 0.f;
            const float li = q < pn ? 1.f / l_arr[p0 + q] : 0.f;
            const float dr = q < pn ? d_arr[p0 + q] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float pt = __expf(st[tt][r] * scale - m) * li;
              st[tt][r] = pt;
              dpt[tt][r] = pt * (dpt[tt][r] - dr) * scale;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
              p_buf[((lane >> 4) * 4 + r) * KPAD + tt * 16 + (lane & 15)] =
                  __hip_bfloat16(st[tt][r]);
            // dS^T goes to the SECOND buffer up-front: no WAR wait between
            // the dV reads of P^T and the dS^T writes
#pragma unroll
            for (int r = 0; r < 4; ++r)
              p_buf[PBUF + ((lane >> 4) * 4 + r) * KPAD + tt * 16 +
                    (lane & 15)] = __hip_bfloat16(dpt[tt][r]);
          }
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          if (kk * 32 < nt * 16) {
            const int k0 = kk * 32 + (lane >> 4) * 8;
            const bool valid = k0 < nt * 16;
            bf16x8 pt_frag{};
            if (valid)
              pt_frag = *(const bf16x8*)(&p_buf[(lane & 15) * KPAD + k0]);
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) {
              const int d = dt * 16 + (lane & 15);
              bf16x8 dob{};
              if (valid)
                dob = *(const bf16x8*)(&dot_lds[d * VROW + c * CHUNK + k0]);
              dv_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  pt_frag, dob, dv_acc[dt], 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          if (kk * 32 < nt * 16) {
            const int k0 = kk * 32 + (lane >> 4) * 8;
            const bool valid = k0 < nt * 16;
            bf16x8 ds_frag{};
            if (valid)
              ds_frag =
                  *(const bf16x8*)(&p_buf[PBUF + (lane & 15) * KPAD + k0]);
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) {
              const int d = dt * 16 + (lane & 15);
              bf16x8 qb{};
              if (valid)
                qb = *(const bf16x8*)(&qt_lds[d * VROW + c * CHUNK + k0]);
              dk_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  ds_frag, qb, dk_acc[dt], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // dK/dV stores through an LDS transpose (p_buf scratch)
  auto store_t = [&](bool is_v) {
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        p_buf[((lane >> 4) * 4 + r) * KPAD + dt * 16 + (lane & 15)] =
            __hip_bfloat16(is_v ? dv_acc[dt][r] : dk_acc[dt][r]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __hip_bfloat16* dst = dqkv + (int64_t)(is_v ? 2 : 1) * H * D +
                          (int64_t)h * D;
#pragma unroll
    for (int i = 0; i < (16 * D / 8) / 64; ++i) {
      const int t = lane + 64 * i;
      const int row = t / (D / 8);
      const int c8 = t % (D / 8);
      const int key = key0 + row;
      if (key < N) {
        Vec<__hip_bfloat16, 8> v =
            vload<__hip_bfloat16, 8>(&p_buf[row * KPAD + c8 * 8]);
        vstore<__hip_bfloat16, 8>(
            dst + (((int64_t)b * N + key) * 3) * H * D + c8 * 8, v);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  store_t(false);
  store_t(true);
}

// dQ. grid (B*H, ceil(N/128)); each wave owns 16 queries (q/dO fragments in
// registers) and accumulates over 64-key panels of K, V and K^T.
template <int D>
__global__ __launch_bounds__(512)
void attn_bwd_q_stream_kernel(const __hip_bfloat16* __restrict__ qkv,
                              const __hip_bfloat16* __restrict__ dout,
                              const float* __restrict__ stats,
                              const float* __restrict__ drow,
                              __hip_bfloat16* __restrict__ dqkv,
                              int B, int N, int H, float scale) {
  constexpr int KSLICES = D / 32;
  constexpr int KP = BWD_PANEL;
  constexpr int VROW = KP + 8;
  const int b = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q0 = blockIdx.y * ROWS + wave * 16;  // may be >= N: no stores

  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  __hip_bfloat16* k_lds = (__hip_bfloat16*)lds_raw;  // [KP][KPAD]
  __hip_bfloat16* v_lds = k_lds + KP * KPAD;         // [KP][KPAD]
  __hip_bfloat16* kt_lds = v_lds + KP * KPAD;        // [D][VROW]
  __hip_bfloat16* p_lds = kt_lds + D * VROW;         // [NWAVES][2*PBUF]
  __hip_bfloat16* p_buf = p_lds + wave * 2 * PBUF;   // chunk-alternating

  const int64_t bh_stride = (int64_t)3 * H * D;
  const __hip_bfloat16* q_src = qkv + (int64_t)b * N * 3 * H * D +
                                (int64_t)h * D;
  const __hip_bfloat16* k_src = q_src + (int64_t)H * D;
  const __hip_bfloat16* v_src = q_src + (int64_t)2 * H * D;
  const __hip_bfloat16* do_src = dout + (int64_t)b * N * H * D +
                                 (int64_t)h * D;
  const float* m_arr = stats + ((int64_t)b * H + h) * N;
  const float* l_arr = stats + ((int64_t)(B + b) * H + h) * N;
  const float* d_arr = drow + ((int64_t)b * H + h) * N;

  bf16x8 q_frag[KSLICES], do_frag[KSLICES];
  {
    const int row = q0 + (lane & 15);
    const int srow = row < N ? row : N - 1;
#pragma unroll
    for (int sl = 0; sl < KSLICES; ++sl) {
      const int d0 = sl * 32 + (lane >> 4) * 8;
      q_frag[sl] = *(const bf16x8*)(q_src + (int64_t)srow * bh_stride + d0);
      do_frag[sl] = *(const bf16x8*)(do_src + (int64_t)srow * H * D + d0);
    }
  }
  float mr[4], lr[4], drr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + (lane >> 4) * 4 + r;
    mr[r] = qrow < N ? m_arr[qrow] : 0.f;
    lr[r] = qrow < N ? 1.f / l_arr[qrow] : 0.f;
    drr[r] = qrow < N ? d_arr[qrow] : 0.f;
  }
  f32x4 dq_acc[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) dq_acc[dt] = {0.f, 0.f, 0.f, 0.f};

  for (int p0 = 0; p0 < N; p0 += KP) {
    const int pn = N - p0 < KP ? N - p0 : KP;  // valid keys in the panel
    const int n_ktiles = (pn + 15) >> 4;
    const int pnpad = n_ktiles * 16;
    if (p0 > 0) __syncthreads();  // slower waves still read the last panel
    stage_panel<D>(k_src, bh_stride, k_lds, kt_lds, p0, pn, pnpad, VROW);
    stage_panel<D>(v_src, bh_stride, v_lds, nullptr, p0, pn, pnpad, VROW);
    __syncthreads();

#pragma unroll
    for (int c = 0; c < KP / CHUNK; ++c) {  // 64-key chunks
      const int t0 = c * 4;
      if (t0 < n_ktiles) {
        const int nt = n_ktiles - t0 < 4 ? n_ktiles - t0 : 4;
        f32x4 st[4], dpt[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          if (tt < nt) {
            f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sl = 0; sl < KSLICES; ++sl) {
              const int key = (t0 + tt) * 16 + (lane & 15);
              const int d0 = sl * 32 + (lane >> 4) * 8;
              bf16x8 kb = *(const bf16x8*)(&k_lds[key * KPAD + d0]);
              bf16x8 vb = *(const bf16x8*)(&v_lds[key * KPAD + d0]);
              sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[sl], kb,
                                                             sacc, 0, 0, 0);
              dacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(do_frag[sl], vb,
                                                             dacc, 0, 0, 0);
            }
            st[tt] = sacc;
            dpt[tt] = dacc;
          }
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          if (tt < nt) {
            const int key = (t0 + tt) * 16 + (lane & 15);  // panel-local
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float pv =
                  key < pn ? __expf(st[tt][r] * scale - mr[r]) * lr[r] : 0.f;
              st[tt][r] = pv * (dpt[tt][r] - drr[r]) * scale;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
              p_buf[(c & 1) * PBUF +
                    ((lane >> 4) * 4 + r) * KPAD + tt * 16 + (lane & 15)] =
                  __hip_bfloat16(st[tt][r]);  // alternate buffers: no WAR
          }
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          if (kk * 32 < nt * 16) {
            const int k0 = kk * 32 + (lane >> 4) * 8;
            const bool valid = k0 < nt * 16;
            bf16x8 ds_frag{};
            if (valid)
              ds_frag = *(const bf16x8*)(&p_buf[(c & 1) * PBUF +
                                                (lane & 15) * KPAD + k0]);
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) {
              const int d = dt * 16 + (lane & 15);
              bf16x8 kb{};
              if (valid)
                kb = *(const bf16x8*)(&kt_lds[d * VROW + c * CHUNK + k0]);
              dq_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  ds_frag, kb, dq_acc[dt], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // dQ store through an LDS transpose (p_buf scratch): coalesced 16B rows
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      p_buf[((lane >> 4) * 4 + r) * KPAD + dt * 16 + (lane & 15)] =
          __hip_bfloat16(dq_acc[dt][r]);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < (16 * D / 8) / 64; ++i) {
    const int t = lane + 64 * i;
    const int row = t / (D / 8);
    const int c8 = t % (D / 8);
    const int qrow = q0 + row;
    if (qrow < N) {
      Vec<__hip_bfloat16, 8> v =
          vload<__hip_bfloat16, 8>(&p_buf[row * KPAD + c8 * 8]);
      vstore<__hip_bfloat16, 8>(
          dqkv + (((int64_t)b * N + qrow) * 3) * H * D + (int64_t)h * D +
              c8 * 8,
          v);
    }
  }
}

// Forward key-panel size. 128 keys per panel (73 KB of LDS at d = 64, two
// blocks per CU) is the measured default: 0.31 ms against 0.47 ms for 256
// (107 KB, one block per CU) at B64 N577 H12 d64
// (profiles/attn_stream_ab.txt). DLA_ATTN_STREAM_PANEL=256 selects the
// larger panel for A/B runs.
inline int fwd_panel() {
  const char* e = std::getenv("DLA_ATTN_STREAM_PANEL");
  return (e != nullptr && std::atoi(e) == 256) ? 256 : 128;
}

}  // namespace attn_stream
}  // namespace dla

namespace {

struct AttnDims {
  int B, N, H, D;
};

AttnDims stream_dims(const torch::Tensor& qkv, int64_t num_heads,
                     const char* who) {
  TORCH_CHECK(qkv.is_cuda(), who, " wants a GPU tensor");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, who, " wants bf16 qkv");
  TORCH_CHECK(qkv.is_contiguous(), who, " wants contiguous qkv");
  TORCH_CHECK(qkv.dim() >= 2 && num_heads >= 1, who, " wants [B,N,3*H*d]");
  AttnDims s;
  s.B = (int)qkv.size(0);
  s.N = (int)qkv.size(1);
  s.H = (int)num_heads;
  TORCH_CHECK(s.B >= 1 && s.N >= 1, who, " wants a non-empty qkv");
  const int64_t inner = qkv.numel() / ((int64_t)s.B * s.N);
  s.D = (int)(inner / (3 * s.H));
  TORCH_CHECK(inner == (int64_t)3 * s.H * s.D, "qkv inner dim mismatch");
  TORCH_CHECK(s.D == 32 || s.D == 64, who, " supports head_dim 32/64, got ",
              s.D);
  TORCH_CHECK(s.N <= 4096, who, " supports N <= 4096, got ", s.N);
  return s;
}

}  // namespace

std::vector<torch::Tensor> attn_fwd_stream(torch::Tensor qkv,
                                           int64_t num_heads, double scale,
                                           bool save_stats) {
  namespace as = dla::attn_stream;
  const AttnDims s = stream_dims(qkv, num_heads, "attn_fwd_stream");
  auto out = torch::empty({s.B, s.N, (int64_t)s.H * s.D}, qkv.options());
  torch::Tensor stats;
  if (save_stats)
    stats = torch::empty({2, s.B, s.H, s.N},
                         qkv.options().dtype(torch::kFloat));
  dim3 grid(s.B * s.H, (s.N + as::ROWS - 1) / as::ROWS);
  dim3 block(as::NWAVES * 64);
  const int panel = as::fwd_panel();
  auto launch = [&](auto dtag, auto ptag) {
    constexpr int DD = decltype(dtag)::value;
    constexpr int PP = decltype(ptag)::value;
    hipLaunchKernelGGL((as::attn_fwd_stream_kernel<DD, PP>), grid, block,
                       as::fwd_lds_bytes(DD, PP), dla::stream(),
                       (const __hip_bfloat16*)qkv.data_ptr(),
                       (__hip_bfloat16*)out.data_ptr(),
                       save_stats ? stats.data_ptr<float>() : nullptr, s.B,
                       s.N, s.H, (float)scale);
  };
  using D64 = std::integral_constant<int, 64>;
  using D32 = std::integral_constant<int, 32>;
  using P256 = std::integral_constant<int, 256>;
  using P128 = std::integral_constant<int, 128>;
  if (s.D == 64) panel == 256 ? launch(D64{}, P256{}) : launch(D64{}, P128{});
  else panel == 256 ? launch(D32{}, P256{}) : launch(D32{}, P128{});
  HIP_CHECK_ERR();
  std::vector<torch::Tensor> res = {out};
  if (save_stats) res.push_back(stats);
  return res;
}

std::vector<torch::Tensor> attn_bwd_stream(torch::Tensor qkv,
                                           torch::Tensor dout,
                                           torch::Tensor stats,
                                           torch::Tensor drow,
                                           int64_t num_heads, double scale) {
  namespace as = dla::attn_stream;
  const AttnDims s = stream_dims(qkv, num_heads, "attn_bwd_stream");
  TORCH_CHECK(dout.is_cuda() && dout.is_contiguous() &&
                  dout.scalar_type() == at::kBFloat16 &&
                  dout.numel() == (int64_t)s.B * s.N * s.H * s.D,
              "attn_bwd_stream wants contiguous bf16 dout [B,N,H*d]");
  TORCH_CHECK(stats.is_cuda() && stats.is_contiguous() &&
                  stats.scalar_type() == at::kFloat &&
                  stats.numel() == (int64_t)2 * s.B * s.H * s.N,
              "attn_bwd_stream wants contiguous fp32 stats [2,B,H,N]");
  TORCH_CHECK(drow.is_cuda() && drow.is_contiguous() &&
                  drow.scalar_type() == at::kFloat &&
                  drow.numel() == (int64_t)s.B * s.H * s.N,
              "attn_bwd_stream wants contiguous fp32 drow [B,H,N]");
  auto dqkv = torch::empty_like(qkv);
  dim3 grid(s.B * s.H, (s.N + as::ROWS - 1) / as::ROWS);
  dim3 block(as::NWAVES * 64);
  auto run = [&](auto dtag) {
    constexpr int DD = decltype(dtag)::value;
    hipLaunchKernelGGL((as::attn_bwd_kv_stream_kernel<DD>), grid, block,
                       as::bwd_kv_lds_bytes(DD), dla::stream(),
                       (const __hip_bfloat16*)qkv.data_ptr(),
                       (const __hip_bfloat16*)dout.data_ptr(),
                       stats.data_ptr<float>(), drow.data_ptr<float>(),
                       (__hip_bfloat16*)dqkv.data_ptr(), s.B, s.N, s.H,
                       (float)scale);
    hipLaunchKernelGGL((as::attn_bwd_q_stream_kernel<DD>), grid, block,
                       as::bwd_q_lds_bytes(DD), dla::stream(),
                       (const __hip_bfloat16*)qkv.data_ptr(),
                       (const __hip_bfloat16*)dout.data_ptr(),
                       stats.data_ptr<float>(), drow.data_ptr<float>(),
                       (__hip_bfloat16*)dqkv.data_ptr(), s.B, s.N, s.H,
                       (float)scale);
  };
  if (s.D == 64) run(std::integral_constant<int, 64>{});
  else run(std::integral_constant<int, 32>{});
  HIP_CHECK_ERR();
  return {dqkv};
}
