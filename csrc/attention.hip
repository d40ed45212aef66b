// Fused multi-head attention forward + backward for CDNA4 (gfx950).
//
// Replaces the eager softmax(Q K^T / sqrt(d) + bias + mask) V chain in
// ViT (classification/vision_transformer/vit_model.py:88-113), Swin window
// attention (classification/swin_transformer/models/swin_transformer.py:118-151),
// and MAE with ONE kernel launch per tensor (TransFG's part-selection blocks
// need the full attention maps and keep their eager code):
//  - consumes the packed qkv projection [B, N, 3, H, d] directly (no permute
//    copies, no [B,H,N,N] fp32 score tensor, no separate softmax kernels);
//  - writes O in [B, N, H*d] (the layout the output projection wants);
//  - backward recomputes P in-LDS from saved per-row softmax stats (m, l) —
//    no [B,H,N,N] tensor ever reaches HBM (optionally saves P in bf16 for
//    the bias-gradient fallback path).
//
// Shape domain: d in {32, 64}, N <= 256 (ViT 197, Swin windows 49, MAE 50);
// the backward kernels additionally need their LDS to fit 160 KiB, which at
// d = 64 holds for N <= 224 (attn_bwd_lds_bytes). Longer sequences, and the
// backward of d = 64 with 225 <= N <= 256, run the streaming kernels of
// csrc/attention_stream.hip (plain path only).
// Design notes (rocprof-driven):
//  - one workgroup per (b, h); 8 waves (4 for small N), each owning 16
//    output rows at a time;
//  - K staged in LDS [Npad][72] (72*2B = 36-dword row stride: 16-lane
//    B-fragment reads hit 16 distinct banks), V transposed in LDS [d][Npad+8];
//  - P/dS round-trips through a tiny per-wave LDS chunk (16x72) and the
//    O/dV/dK MFMAs accumulate chunk-by-chunk, keeping LDS small enough for
//    multiple waves per SIMD;
//  - every accumulator loop is fully unrolled with compile-time bounds:
//    a runtime-indexed register array spills to scratch (measured 60x).
#include "common.h"
#include "vec.h"

namespace dla {

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int KPAD = 72;         // K/Q/dO LDS row stride (bf16 elems)
constexpr int CHUNK = 64;        // keys/queries per P-staging chunk (4 tiles)
constexpr int PBUF = 16 * KPAD;  // per-wave P chunk buffer elems

__device__ __forceinline__ float wave16_max(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ float wave16_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Stage rows [N][D] of a (possibly strided) bf16 source into LDS row-major
// (row stride KPAD) and/or transposed (dst_t[d][VROW]).
template <int D>
__device__ void stage_rows(const __hip_bfloat16* src, int64_t row_stride,
                           __hip_bfloat16* dst_rows, __hip_bfloat16* dst_t,
                           int N, int Npad, int VROW) {
  for (int n = threadIdx.x / (D / 4); n < Npad;
       n += blockDim.x / (D / 4)) {
    const int d0 = (threadIdx.x % (D / 4)) * 4;
    Vec<__hip_bfloat16, 4> v;
    if (n < N) {
      v = vload<__hip_bfloat16, 4>(src + n * row_stride + d0);
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
// COSINE (Swin-v2): S = logit_scale[h] * cos(q, k) instead of scale * q.k —
// per-row q/k inverse norms are computed in-kernel; `scale` is unused and
// `lscale` carries the per-head clamped-exp logit scales. Training uses
// this forward with SAVE_P; the cosine chain rule (incl. logit_scale and
// CPB-bias grads) runs from the saved P in the Python wrapper
// (ops/attention._AttnCosineFn).
template <int D, bool HAS_BIAS, bool HAS_MASK, bool SAVE_P, bool COSINE = false>
__global__ __launch_bounds__(512)
void attn_fwd_kernel(const __hip_bfloat16* __restrict__ qkv,  // [B,N,3,H,D]
                     const float* __restrict__ bias,          // [H,N,N]|null
                     const float* __restrict__ mask,          // [nW,N,N]|null
                     __hip_bfloat16* __restrict__ out,        // [B,N,H*D]
                     __hip_bfloat16* __restrict__ p_out,      // [B,H,N,N]|null
                     float* __restrict__ stats,               // [2,B,H,N]|null
                     const float* __restrict__ lscale,        // [H]|null
                     int B, int N, int H, int n_win, float scale,
                     int ablate = 0) {  // phase-ablation probe (0 = full)
  constexpr int KSLICES = D / 32;
  const int b = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  const int Npad = (N + 15) & ~15;
  const int n_ktiles = Npad / 16;

  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  __hip_bfloat16* k_lds = (__hip_bfloat16*)lds_raw;       // [Npad][KPAD]
  __hip_bfloat16* vt_lds = k_lds + Npad * KPAD;           // [D][VROW]
  const int VROW = Npad + 8;
  __hip_bfloat16* p_lds = vt_lds + D * VROW;              // [nwaves][2*PBUF]

  float* kinv = (float*)(p_lds + nwaves * 2 * PBUF);  // [Npad] (COSINE only)

  const int64_t bh_stride = (int64_t)3 * H * D;
  stage_rows<D>(qkv + ((int64_t)b * N * 3 + 1) * H * D + (int64_t)h * D,
                bh_stride, k_lds, nullptr, N, Npad, VROW);
  stage_rows<D>(qkv + ((int64_t)b * N * 3 + 2) * H * D + (int64_t)h * D,
                bh_stride, nullptr, vt_lds, N, Npad, VROW);
  __syncthreads();
  if (COSINE) {
    for (int key = threadIdx.x; key < Npad; key += blockDim.x) {
      float sum = 0.f;
      for (int d = 0; d < D; ++d) {
        const float v = to_f32(k_lds[key * KPAD + d]);
        sum += v * v;
      }
      kinv[key] = rsqrtf(fmaxf(sum, 1e-12f));
    }
    __syncthreads();
  }
  if (ablate >= 4) return;  // ablation: staging only
  const float ls = COSINE ? lscale[h] : scale;

  const __hip_bfloat16* q_src = qkv + (int64_t)b * N * 3 * H * D +
                                (int64_t)h * D;
  __hip_bfloat16* p_buf = p_lds + wave * 2 * PBUF;  // double-buffered
  const int n_qblocks = (N + 15) / 16;

  for (int qb = wave; qb < n_qblocks; qb += nwaves) {
    const int q0 = qb * 16;
    bf16x8 q_frag[KSLICES];
    {
      const int row = q0 + (lane & 15);
      const int srow = row < N ? row : N - 1;
#pragma unroll
      for (int sl = 0; sl < KSLICES; ++sl) {
        const int d0 = sl * 32 + (lane >> 4) * 8;
        q_frag[sl] = *(const bf16x8*)(q_src + srow * bh_stride + d0);
      }
    }
    float q_inv = 1.f;  // per A-fragment row (lane&15); COSINE only
    if (COSINE) {
      float qs = 0.f;
#pragma unroll
      for (int sl = 0; sl < KSLICES; ++sl)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          __hip_bfloat16 hv;
          short sv = q_frag[sl][j];
          __builtin_memcpy(&hv, &sv, sizeof(hv));
          const float v = to_f32(hv);
          qs += v * v;
        }
      // row total lives across lanes {r, r+16, r+32, r+48}
      qs += __shfl_xor(qs, 16, 64);
      qs += __shfl_xor(qs, 32, 64);
      q_inv = rsqrtf(fmaxf(qs, 1e-12f));
    }
    __shared__ float qn_sh[8][16];  // per wave: qinv by row-in-block
    if (COSINE) {
      qn_sh[wave][lane & 15] = q_inv;  // lanes of a row write the same value
    }

    // S = Q K^T over all key tiles (kept in VGPRs)
    f32x4 s_acc[16];
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) {
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

    if (ablate >= 3) continue;  // ablation: QK^T only
    // softmax rows (C/D: col = key = lane&15, row = (lane>>4)*4 + reg).
    // kt-outer loops keep the 4 rows' max/exp/sum chains INDEPENDENT so
    // they interleave (the row-outer form serialized a 16-deep fmax chain,
    // 4 dependent shuffle reductions and a 16-deep exp+add chain per row:
    // ablation measured the whole softmax phase at 95 us of a 336 us
    // kernel before this restructure).
    const int col = lane & 15;
    float row_sum[4], mx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mx[r] = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) {
      if (kt < n_ktiles) {
        const int key = kt * 16 + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qrow = q0 + (lane >> 4) * 4 + r;
          float sv = COSINE
              ? s_acc[kt][r] * ls * qn_sh[wave][(lane >> 4) * 4 + r] *
                    kinv[key]
              : s_acc[kt][r] * scale;
          if ((HAS_BIAS || HAS_MASK) && key < N && qrow < N) {
            if (HAS_BIAS) sv += bias[((int64_t)h * N + qrow) * N + key];
            if (HAS_MASK)
              sv += mask[((int64_t)(b % n_win) * N + qrow) * N + key];
          }
          if (key >= N) sv = -INFINITY;
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
#pragma unroll
    for (int r = 0; r < 4; ++r) row_sum[r] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) {
      if (kt < n_ktiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __expf(s_acc[kt][r] - mx[r]);
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
    if (stats != nullptr && col == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = q0 + (lane >> 4) * 4 + r;
        if (qrow < N) {
          stats[((int64_t)b * H + h) * N + qrow] = mx[r];
          stats[((int64_t)(B + b) * H + h) * N + qrow] = row_sum[r];
        }
      }
    }
    if (SAVE_P) {
#pragma unroll
      for (int kt = 0; kt < 16; ++kt) {
        if (kt < n_ktiles) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qrow = q0 + (lane >> 4) * 4 + r;
            const int key = kt * 16 + col;
            if (qrow < N && key < N)
              p_out[(((int64_t)b * H + h) * N + qrow) * N + key] =
                  __hip_bfloat16(s_acc[kt][r] / row_sum[r]);
          }
        }
      }
    }

    if (ablate >= 2) continue;  // ablation: no PV / p_buf
    // O = P V through the per-wave P buffer, software-pipelined over two
    // buffers: chunk c+1's LDS writes are issued BEFORE chunk c's fragment
    // reads, so the write->read drain of a chunk hides under the previous
    // chunk's MFMAs (ablation: the serialized form cost 67 us of 336).
    f32x4 o_acc[D / 16];
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) o_acc[dt] = {0.f, 0.f, 0.f, 0.f};
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
    for (int c = 0; c < 4; ++c) {  // chunks of 4 key tiles (64 keys)
      const int t0 = c * 4;
      if (t0 < n_ktiles) {
        const int nt = n_ktiles - t0 < 4 ? n_ktiles - t0 : 4;
        if ((c + 1) * 4 < n_ktiles) write_pchunk(c + 1);
        const __hip_bfloat16* pb = p_buf + (c & 1) * PBUF;
        // MFMA over the chunk: pairs of tiles = 32-key K-steps
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

    if (ablate == 1) continue;  // ablation: no O store
    // O store through an LDS transpose (p_buf reused as scratch): the
    // fragment layout is column-per-lane, so direct stores were 16 scalar
    // 2-byte globals per lane (ablation: 64 us of 336); the transpose
    // turns them into coalesced 16-byte row stores.
    {
      float rinv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) rinv[r] = 1.f / row_sum[r];
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          p_buf[((lane >> 4) * 4 + r) * KPAD + dt * 16 + (lane & 15)] =
              __hip_bfloat16(o_acc[dt][r] * rinv[r]);
      // same-wave cross-lane LDS visibility: drain, and fence the reads
      // below from being hoisted above the drain (guide rule 18)
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
              (__hip_bfloat16*)out + ((int64_t)b * N + qrow) * H * D +
                  h * D + c8 * 8,
              v);
        }
      }
    }
  }
}

// --------------------------------------------------------------- backward --
// dV = P^T dO ; dP = dO V^T ; dS = P*(dP - D_row) ; dQ = scale*dS K ;
// dK = scale*dS^T Q.  P recomputed from (m, l); D_row precomputed by host.

// Kernel A: dK and dV. Each wave owns 16 keys; S^T / dP^T computed per
// 64-query chunk and pushed through the small P buffer into the dV / dK
// MFMA accumulators.
template <int D>
__global__ __launch_bounds__(512)
void attn_bwd_kv_kernel(const __hip_bfloat16* __restrict__ qkv,
                        const __hip_bfloat16* __restrict__ dout,  // [B,N,H*D]
                        const float* __restrict__ stats,
                        const float* __restrict__ drow,
                        __hip_bfloat16* __restrict__ dqkv,
                        int B, int N, int H, float scale) {
  constexpr int KSLICES = D / 32;
  const int b = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  const int Npad = (N + 15) & ~15;
  const int n_qtiles = Npad / 16;

  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  __hip_bfloat16* q_lds = (__hip_bfloat16*)lds_raw;       // [Npad][KPAD]
  __hip_bfloat16* do_lds = q_lds + Npad * KPAD;           // [Npad][KPAD]
  const int VROW = Npad + 8;
  __hip_bfloat16* qt_lds = do_lds + Npad * KPAD;          // [D][VROW]
  __hip_bfloat16* dot_lds = qt_lds + D * VROW;            // [D][VROW]
  __hip_bfloat16* p_lds = dot_lds + D * VROW;             // [nwaves][2*PBUF]

  const int64_t bh_stride = (int64_t)3 * H * D;
  stage_rows<D>(qkv + (int64_t)b * N * 3 * H * D + (int64_t)h * D,
                bh_stride, q_lds, qt_lds, N, Npad, VROW);
  stage_rows<D>(dout + (int64_t)b * N * H * D + (int64_t)h * D,
                (int64_t)H * D, do_lds, dot_lds, N, Npad, VROW);
  __syncthreads();

  const float* m_arr = stats + ((int64_t)b * H + h) * N;
  const float* l_arr = stats + ((int64_t)(B + b) * H + h) * N;
  const float* d_arr = drow + ((int64_t)b * H + h) * N;
  const __hip_bfloat16* k_src = qkv + ((int64_t)b * N * 3 + 1) * H * D +
                                (int64_t)h * D;
  const __hip_bfloat16* v_src = qkv + ((int64_t)b * N * 3 + 2) * H * D +
                                (int64_t)h * D;
  __hip_bfloat16* p_buf = p_lds + wave * 2 * PBUF;  // P^T | dS^T split buffers

  for (int kt = wave; kt < (N + 15) / 16; kt += nwaves) {
    const int key0 = kt * 16;
    bf16x8 k_frag[KSLICES], v_frag[KSLICES];
    {
      const int key = key0 + (lane & 15);
      const int skey = key < N ? key : N - 1;
#pragma unroll
      for (int sl = 0; sl < KSLICES; ++sl) {
        const int d0 = sl * 32 + (lane >> 4) * 8;
        k_frag[sl] = *(const bf16x8*)(k_src + skey * bh_stride + d0);
        v_frag[sl] = *(const bf16x8*)(v_src + skey * bh_stride + d0);
      }
    }
    f32x4 dv_acc[D / 16], dk_acc[D / 16];
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      dv_acc[dt] = {0.f, 0.f, 0.f, 0.f};
      dk_acc[dt] = {0.f, 0.f, 0.f, 0.f};
    }

#pragma unroll
    for (int c = 0; c < 4; ++c) {  // 64-query chunks
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
        // P^T and scale*dS^T for this chunk; stage P^T, accumulate dV
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          if (tt < nt) {
            const int q = (t0 + tt) * 16 + (lane & 15);
            const float m = q < N ? m_arr[q] : 0.f;
            const float li = q < N ? 1.f / l_arr[q] : 0.f;
            const float dr = q < N ? d_arr[q] : 0.f;
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
            // dS^T staged to the SECOND buffer up-front: no WAR wait
            // between the dV reads of P^T and the dS^T writes
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
        // accumulate dK from the second buffer
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

    // dK/dV stores through an LDS transpose (p_buf scratch): fragment
    // layout is column-per-lane, direct stores were 32 scalar 2B globals
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
              dst + ((int64_t)(b * N + key) * 3) * H * D + c8 * 8, v);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    };
    store_t(false);
    store_t(true);
  }
}

// Kernel B: dQ. Each wave owns 16 queries; per 64-key chunk: S and dP
// recomputed, dS staged, dQ accumulated.
template <int D>
__global__ __launch_bounds__(512)
void attn_bwd_q_kernel(const __hip_bfloat16* __restrict__ qkv,
                       const __hip_bfloat16* __restrict__ dout,
                       const float* __restrict__ stats,
                       const float* __restrict__ drow,
                       __hip_bfloat16* __restrict__ dqkv,
                       int B, int N, int H, float scale) {
  constexpr int KSLICES = D / 32;
  const int b = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  const int Npad = (N + 15) & ~15;
  const int n_ktiles = Npad / 16;

  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  __hip_bfloat16* k_lds = (__hip_bfloat16*)lds_raw;       // [Npad][KPAD]
  __hip_bfloat16* v_lds = k_lds + Npad * KPAD;            // [Npad][KPAD]
  const int VROW = Npad + 8;
  __hip_bfloat16* kt_lds = v_lds + Npad * KPAD;           // [D][VROW]
  __hip_bfloat16* p_lds = kt_lds + D * VROW;              // [nwaves][PBUF]

  const int64_t bh_stride = (int64_t)3 * H * D;
  stage_rows<D>(qkv + ((int64_t)b * N * 3 + 1) * H * D + (int64_t)h * D,
                bh_stride, k_lds, kt_lds, N, Npad, VROW);
  stage_rows<D>(qkv + ((int64_t)b * N * 3 + 2) * H * D + (int64_t)h * D,
                bh_stride, v_lds, nullptr, N, Npad, VROW);
  __syncthreads();

  const float* m_arr = stats + ((int64_t)b * H + h) * N;
  const float* l_arr = stats + ((int64_t)(B + b) * H + h) * N;
  const float* d_arr = drow + ((int64_t)b * H + h) * N;
  const __hip_bfloat16* q_src = qkv + (int64_t)b * N * 3 * H * D +
                                (int64_t)h * D;
  const __hip_bfloat16* do_src = dout + (int64_t)b * N * H * D +
                                 (int64_t)h * D;
  __hip_bfloat16* p_buf = p_lds + wave * 2 * PBUF;  // chunk-alternating

  for (int qb = wave; qb < (N + 15) / 16; qb += nwaves) {
    const int q0 = qb * 16;
    bf16x8 q_frag[KSLICES], do_frag[KSLICES];
    {
      const int row = q0 + (lane & 15);
      const int srow = row < N ? row : N - 1;
#pragma unroll
      for (int sl = 0; sl < KSLICES; ++sl) {
        const int d0 = sl * 32 + (lane >> 4) * 8;
        q_frag[sl] = *(const bf16x8*)(q_src + srow * bh_stride + d0);
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

#pragma unroll
    for (int c = 0; c < 4; ++c) {  // 64-key chunks
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
            const int key = (t0 + tt) * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float pv =
                  key < N ? __expf(st[tt][r] * scale - mr[r]) * lr[r] : 0.f;
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
            dqkv + ((int64_t)(b * N + qrow) * 3) * H * D + (int64_t)h * D +
                c8 * 8,
            v);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  }
}

// numerics probe: D[16,16] = A[16,32] @ B[32,16] via one mfma, to pin the
// fragment layout on real hardware (guide: A=I with asymmetric B).
__global__ void mfma_probe_kernel(const __hip_bfloat16* A,
                                  const __hip_bfloat16* B, float* D_out) {
  const int lane = threadIdx.x & 63;
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = lane & 15, k = (lane >> 4) * 8 + j;
    a[j] = ((const short*)A)[row * 32 + k];
    const int col = lane & 15;
    b[j] = ((const short*)B)[k * 16 + col];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = (lane >> 4) * 4 + r, col = lane & 15;
    D_out[row * 16 + col] = acc[r];
  }
}

}  // namespace dla

std::vector<torch::Tensor> attn_fwd(torch::Tensor qkv, int64_t num_heads,
                                    double scale,
                                    c10::optional<torch::Tensor> bias,
                                    c10::optional<torch::Tensor> mask,
                                    bool save_p, bool save_stats) {
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, "attn_fwd wants bf16 qkv");
  TORCH_CHECK(qkv.is_contiguous(), "attn_fwd wants contiguous qkv");
  const int B = (int)qkv.size(0);
  const int N = (int)qkv.size(1);
  const int H = (int)num_heads;
  const int64_t inner = qkv.numel() / ((int64_t)B * N);
  const int D = (int)(inner / (3 * H));
  TORCH_CHECK(inner == (int64_t)3 * H * D, "qkv inner dim mismatch");
  TORCH_CHECK(D == 32 || D == 64, "attn_fwd supports head_dim 32/64, got ", D);
  TORCH_CHECK(N <= 256, "attn_fwd supports N <= 256, got ", N);

  auto out = torch::empty({B, N, (int64_t)H * D}, qkv.options());
  torch::Tensor p, stats;
  if (save_p) p = torch::empty({B, H, N, N}, qkv.options());
  if (save_stats)
    stats = torch::empty({2, B, H, N}, qkv.options().dtype(torch::kFloat));

  int n_win = 1;
  const float* bias_ptr = nullptr;
  const float* mask_ptr = nullptr;
  torch::Tensor bias_f, mask_f;
  if (bias.has_value()) {
    bias_f = bias->to(torch::kFloat).contiguous();
    TORCH_CHECK(bias_f.dim() == 3 && bias_f.size(1) == N,
                "bias must be [H,N,N]");
    bias_ptr = bias_f.data_ptr<float>();
  }
  if (mask.has_value()) {
    mask_f = mask->to(torch::kFloat).contiguous();
    TORCH_CHECK(mask_f.dim() == 3 && mask_f.size(1) == N,
                "mask must be [nW,N,N]");
    n_win = (int)mask_f.size(0);
    TORCH_CHECK(B % n_win == 0, "batch (", B,
                ") must be a multiple of the window count (", n_win, ")");
    mask_ptr = mask_f.data_ptr<float>();
  }

  const int Npad = (N + 15) & ~15;
  const int nwaves = N > 96 ? 8 : 4;  // small-N: 4 waves cover all q blocks
  const int lds = (Npad * dla::KPAD + D * (Npad + 8) + nwaves * 2 * dla::PBUF) *
                  (int)sizeof(__hip_bfloat16);
  dim3 grid(B * H), block(nwaves * 64);

  const char* abl_env = std::getenv("DLA_ATTN_ABLATE");
  const int ablate = abl_env ? std::atoi(abl_env) : 0;
  auto launch = [&](auto dtag, auto btag, auto mtag, auto ptag) {
    constexpr int DD = decltype(dtag)::value;
    constexpr bool BB = decltype(btag)::value;
    constexpr bool MM = decltype(mtag)::value;
    constexpr bool PP = decltype(ptag)::value;
    hipLaunchKernelGGL((dla::attn_fwd_kernel<DD, BB, MM, PP>), grid, block,
                       lds, dla::stream(),
                       (const __hip_bfloat16*)qkv.data_ptr(), bias_ptr,
                       mask_ptr, (__hip_bfloat16*)out.data_ptr(),
                       save_p ? (__hip_bfloat16*)p.data_ptr() : nullptr,
                       save_stats ? stats.data_ptr<float>() : nullptr,
                       nullptr, B, N, H, n_win, (float)scale, ablate);
  };
  auto d3 = [&](auto dtag) {
    using T = std::true_type;
    using F = std::false_type;
    const bool bb = bias_ptr != nullptr, mm = mask_ptr != nullptr;
    if (bb && mm) save_p ? launch(dtag, T{}, T{}, T{})
                          : launch(dtag, T{}, T{}, F{});
    else if (bb) save_p ? launch(dtag, T{}, F{}, T{})
                         : launch(dtag, T{}, F{}, F{});
    else if (mm) save_p ? launch(dtag, F{}, T{}, T{})
                         : launch(dtag, F{}, T{}, F{});
    else save_p ? launch(dtag, F{}, F{}, T{})
                 : launch(dtag, F{}, F{}, F{});
  };
  if (D == 64) d3(std::integral_constant<int, 64>{});
  else d3(std::integral_constant<int, 32>{});
  HIP_CHECK_ERR();
  std::vector<torch::Tensor> res = {out};
  if (save_p) res.push_back(p);
  if (save_stats) res.push_back(stats);
  return res;
}

// Dynamic LDS bytes {kv kernel, q kernel} that attn_bwd launches with.
// ops/attention._attn_route mirrors this arithmetic to keep shapes that do
// not fit 160 KiB per CU off the resident backward.
std::vector<int64_t> attn_bwd_lds_bytes(int64_t N, int64_t D) {
  const int64_t Npad = (N + 15) & ~(int64_t)15;
  const int64_t nwaves = N > 96 ? 8 : 4;
  const int64_t lds_kv = (2 * Npad * dla::KPAD + 2 * D * (Npad + 8) +
                          nwaves * 2 * dla::PBUF) * 2;
  const int64_t lds_q = (2 * Npad * dla::KPAD + D * (Npad + 8) +
                         nwaves * 2 * dla::PBUF) * 2;
  return {lds_kv, lds_q};
}

std::vector<torch::Tensor> attn_bwd(torch::Tensor qkv, torch::Tensor dout,
                                    torch::Tensor stats, torch::Tensor drow,
                                    int64_t num_heads, double scale) {
  TORCH_CHECK(qkv.is_contiguous() && dout.is_contiguous());
  const int B = (int)qkv.size(0);
  const int N = (int)qkv.size(1);
  const int H = (int)num_heads;
  const int D = (int)(qkv.numel() / ((int64_t)B * N * 3 * H));
  TORCH_CHECK(D == 32 || D == 64);
  auto dqkv = torch::empty_like(qkv);
  const int nwaves = N > 96 ? 8 : 4;
  dim3 grid(B * H), block(nwaves * 64);
  const std::vector<int64_t> lds = attn_bwd_lds_bytes(N, D);
  const int lds_kv = (int)lds[0];
  const int lds_q = (int)lds[1];
  TORCH_CHECK(lds_kv <= 163840 && lds_q <= 163840, "attn_bwd: N = ", N,
              ", d = ", D, " needs ", lds_kv, " B of LDS (limit 163840); "
              "use attn_bwd_stream");
  auto run = [&](auto dtag) {
    constexpr int DD = decltype(dtag)::value;
    hipLaunchKernelGGL((dla::attn_bwd_kv_kernel<DD>), grid, block, lds_kv,
                       dla::stream(), (const __hip_bfloat16*)qkv.data_ptr(),
                       (const __hip_bfloat16*)dout.data_ptr(),
                       stats.data_ptr<float>(), drow.data_ptr<float>(),
                       (__hip_bfloat16*)dqkv.data_ptr(), B, N, H,
                       (float)scale);
    hipLaunchKernelGGL((dla::attn_bwd_q_kernel<DD>), grid, block, lds_q,
                       dla::stream(), (const __hip_bfloat16*)qkv.data_ptr(),
                       (const __hip_bfloat16*)dout.data_ptr(),
                       stats.data_ptr<float>(), drow.data_ptr<float>(),
                       (__hip_bfloat16*)dqkv.data_ptr(), B, N, H,
                       (float)scale);
  };
  if (D == 64) run(std::integral_constant<int, 64>{});
  else run(std::integral_constant<int, 32>{});
  HIP_CHECK_ERR();
  return {dqkv};
}

torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B) {
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 &&
              B.scalar_type() == at::kBFloat16);
  auto D = torch::zeros({16, 16}, A.options().dtype(torch::kFloat));
  hipLaunchKernelGGL(dla::mfma_probe_kernel, dim3(1), dim3(64), 0,
                     dla::stream(), (const __hip_bfloat16*)A.data_ptr(),
                     (const __hip_bfloat16*)B.data_ptr(),
                     D.data_ptr<float>());
  HIP_CHECK_ERR();
  return {D};
}


// Swin-v2 cosine attention forward. logit_scale: [H] fp32 =
// clamp(exp(param), max=100). save_p additionally returns the softmax
// probabilities P [B,H,N,N] bf16 for the training backward (the Python
// wrapper runs the cosine chain rule from P — same split as the v1
// bias path).
std::vector<torch::Tensor> attn_fwd_cosine(torch::Tensor qkv,
                              int64_t num_heads,
                              torch::Tensor logit_scale,
                              c10::optional<torch::Tensor> bias,
                              c10::optional<torch::Tensor> mask,
                              bool save_p) {
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 && qkv.is_contiguous());
  const int B = (int)qkv.size(0);
  const int N = (int)qkv.size(1);
  const int H = (int)num_heads;
  const int D = (int)(qkv.numel() / ((int64_t)B * N * 3 * H));
  TORCH_CHECK(D == 32 || D == 64);
  TORCH_CHECK(N <= 256);
  auto ls = logit_scale.to(torch::kFloat).contiguous();
  TORCH_CHECK(ls.numel() == H, "logit_scale must be [H]");
  auto out = torch::empty({B, N, (int64_t)H * D}, qkv.options());
  torch::Tensor pten;
  if (save_p) pten = torch::empty({B, H, N, N}, qkv.options());

  int n_win = 1;
  const float* bias_ptr = nullptr;
  const float* mask_ptr = nullptr;
  torch::Tensor bias_f, mask_f;
  if (bias.has_value()) {
    bias_f = bias->to(torch::kFloat).contiguous();
    bias_ptr = bias_f.data_ptr<float>();
  }
  if (mask.has_value()) {
    mask_f = mask->to(torch::kFloat).contiguous();
    n_win = (int)mask_f.size(0);
    mask_ptr = mask_f.data_ptr<float>();
  }
  const int Npad = (N + 15) & ~15;
  const int nwaves = N > 96 ? 8 : 4;
  const int lds = (Npad * dla::KPAD + D * (Npad + 8) + nwaves * 2 * dla::PBUF) *
                      (int)sizeof(__hip_bfloat16) +
                  Npad * (int)sizeof(float);  // + kinv
  dim3 grid(B * H), block(nwaves * 64);
  auto run = [&](auto dtag, auto btag, auto mtag, auto ptag) {
    constexpr int DD = decltype(dtag)::value;
    constexpr bool BB = decltype(btag)::value;
    constexpr bool MM = decltype(mtag)::value;
    constexpr bool PP = decltype(ptag)::value;
    hipLaunchKernelGGL(
        (dla::attn_fwd_kernel<DD, BB, MM, PP, true>), grid, block, lds,
        dla::stream(), (const __hip_bfloat16*)qkv.data_ptr(), bias_ptr,
        mask_ptr, (__hip_bfloat16*)out.data_ptr(),
        save_p ? (__hip_bfloat16*)pten.data_ptr() : nullptr, nullptr,
        ls.data_ptr<float>(), B, N, H, n_win, 1.0f);
  };
  using T = std::true_type;
  using F = std::false_type;
  auto d2 = [&](auto dtag) {
    const bool bb = bias_ptr != nullptr, mm = mask_ptr != nullptr;
    if (bb && mm) save_p ? run(dtag, T{}, T{}, T{}) : run(dtag, T{}, T{}, F{});
    else if (bb) save_p ? run(dtag, T{}, F{}, T{}) : run(dtag, T{}, F{}, F{});
    else if (mm) save_p ? run(dtag, F{}, T{}, T{}) : run(dtag, F{}, T{}, F{});
    else save_p ? run(dtag, F{}, F{}, T{}) : run(dtag, F{}, F{}, F{});
  };
  if (D == 64) d2(std::integral_constant<int, 64>{});
  else d2(std::integral_constant<int, 32>{});
  HIP_CHECK_ERR();
  std::vector<torch::Tensor> res = {out};
  if (save_p) res.push_back(pten);
  return res;
}
