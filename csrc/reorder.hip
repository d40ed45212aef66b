// Data-movement helpers for the conv1x1 path (gfx950):
//  - transpose2d: [N,K] -> [K,N] bf16 via LDS-tiled coalesced transpose
//    (replaces torch's strided copy: 45us -> ~3us for a 2MB weight)
//  - stride2_gather / stride2_scatter: NHWC row gather/scatter for 1x1
//    stride-2 convs (replaces ~700us torch strided elementwise with a
//    coalesced row-copy; scatter writes zeros to unsampled rows in the same
//    pass, so no separate zero-fill of dx is needed)
#include "common.h"
#include "vec.h"

namespace dla {

using bf16 = __hip_bfloat16;

// 32x32 bf16 tiles through LDS, +1-element pad kills write bank conflicts.
__global__ __launch_bounds__(256) void transpose2d_kernel(
    const bf16* __restrict__ src, bf16* __restrict__ dst, int R, int C) {
  __shared__ bf16 tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32x8
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + i * 8;
    const int c = c0 + tx;
    if (r < R && c < C) tile[ty + i * 8][tx] = src[(int64_t)r * C + c];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = c0 + ty + i * 8;  // row of dst = col of src
    const int c = r0 + tx;
    if (r < C && c < R) dst[(int64_t)r * R + c] = tile[tx][ty + i * 8];
  }
}

// NHWC-flat row indices: input row m_in = (b*IH + ih)*IW + iw,
// output row m_out = (b*OH + oh)*OW + ow with oh=ih/2, ow=iw/2,
// OH=ceil(IH/2), OW=ceil(IW/2).

// dst[M_out, C] <- src[row(m)] (the stride-2 subsample forward)
template <typename dev_t, int V>
__global__ void stride2_gather_kernel(const dev_t* __restrict__ src,
                                      dev_t* __restrict__ dst, int C, int IH,
                                      int IW, int OH, int OW, int64_t M_out,
                                      int64_t used) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= used) return;
  const int lanes = C / V;
  const int c0 = (int)(t % lanes) * V;
  const int64_t rstride = used / lanes;
  for (int64_t m = t / lanes; m < M_out; m += rstride) {
    const int64_t bo = m / ((int64_t)OH * OW);
    const int64_t r = m - bo * OH * OW;
    const int oh = (int)(r / OW), ow = (int)(r % OW);
    const int64_t src_row = (bo * (int64_t)IH + oh * 2) * IW + ow * 2;
    vstore<dev_t, V>(dst + m * C + c0,
                     vload<dev_t, V>(src + src_row * C + c0));
  }
}

// dst[M_in, C]: rows with even (ih, iw) get src rows, all others zero
// (single pass: no separate zero-fill of the full-size gradient).
template <typename dev_t, int V>
__global__ void stride2_scatter_kernel(const dev_t* __restrict__ src,
                                       dev_t* __restrict__ dst, int C, int IH,
                                       int IW, int OH, int OW, int64_t M_in,
                                       int64_t used) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= used) return;
  const int lanes = C / V;
  const int c0 = (int)(t % lanes) * V;
  const int64_t rstride = used / lanes;
  for (int64_t m = t / lanes; m < M_in; m += rstride) {
    const int64_t bi = m / ((int64_t)IH * IW);
    const int64_t r = m - bi * IH * IW;
    const int ih = (int)(r / IW), iw = (int)(r % IW);
    Vec<dev_t, V> v;
    if ((ih & 1) == 0 && (iw & 1) == 0) {
      const int64_t src_row =
          (bi * (int64_t)OH + (ih >> 1)) * OW + (iw >> 1);
      v = vload<dev_t, V>(src + src_row * C + c0);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) v.v[j] = from_f32<dev_t>(0.f);
    }
    vstore<dev_t, V>(dst + m * C + c0, v);
  }
}

}  // namespace dla

torch::Tensor transpose2d(torch::Tensor src) {
  DLA_CHECK_INPUT(src);
  TORCH_CHECK(src.dim() == 2 && src.scalar_type() == torch::kBFloat16,
              "transpose2d: 2D bf16");
  const int R = (int)src.size(0), C = (int)src.size(1);
  auto dst = torch::empty({C, R}, src.options());
  hipLaunchKernelGGL(dla::transpose2d_kernel,
                     dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0,
                     dla::stream(), (const dla::bf16*)src.data_ptr(),
                     (dla::bf16*)dst.data_ptr(), R, C);
  HIP_CHECK_ERR();
  return dst;
}

// x4d [B,C,IH,IW] channels_last -> [B,C,OH,OW] channels_last (stride-2 1x1
// conv input subsample)
torch::Tensor stride2_gather(torch::Tensor x) {
  DLA_CHECK_CUDA(x);
  TORCH_CHECK(x.dim() == 4, "stride2_gather: 4D");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "stride2_gather: channels_last");
  const int B = (int)x.size(0), C = (int)x.size(1);
  const int IH = (int)x.size(2), IW = (int)x.size(3);
  const int OH = (IH + 1) / 2, OW = (IW + 1) / 2;
  auto y = torch::empty({B, C, OH, OW},
                        x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int64_t M_out = (int64_t)B * OH * OW;
  DLA_DISPATCH_FLOAT_TYPES(x.scalar_type(), "stride2_gather", [&] {
    constexpr int VM = 16 / (int)sizeof(dev_t);
    const int V = (C % VM == 0) ? VM : 1;
    auto run = [&](auto vtag) {
      constexpr int VV = decltype(vtag)::value;
      const int lanes = C / VV;
      const int64_t used = dla::nhwc_used_threads(lanes, M_out, 262144);
      hipLaunchKernelGGL((dla::stride2_gather_kernel<dev_t, VV>),
                         dim3((unsigned)((used + 255) / 256)),
                         dim3(256), 0, dla::stream(),
                         (const dev_t*)x.data_ptr(), (dev_t*)y.data_ptr(), C,
                         IH, IW, OH, OW, M_out, used);
    };
    if (V == VM) run(std::integral_constant<int, VM>{});
    else run(std::integral_constant<int, 1>{});
  });
  HIP_CHECK_ERR();
  return y;
}

// dy_s [B,C,OH,OW] channels_last -> dx [B,C,IH,IW] channels_last (zeros on
// unsampled positions)
torch::Tensor stride2_scatter(torch::Tensor dy, int64_t IH, int64_t IW) {
  DLA_CHECK_CUDA(dy);
  TORCH_CHECK(dy.dim() == 4, "stride2_scatter: 4D");
  TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast),
              "stride2_scatter: channels_last");
  const int B = (int)dy.size(0), C = (int)dy.size(1);
  const int OH = (int)dy.size(2), OW = (int)dy.size(3);
  auto dx = torch::empty({B, C, IH, IW},
                         dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int64_t M_in = (int64_t)B * IH * IW;
  DLA_DISPATCH_FLOAT_TYPES(dy.scalar_type(), "stride2_scatter", [&] {
    constexpr int VM = 16 / (int)sizeof(dev_t);
    auto run = [&](auto vtag) {
      constexpr int VV = decltype(vtag)::value;
      const int lanes = C / VV;
      const int64_t used = dla::nhwc_used_threads(lanes, M_in, 524288);
      hipLaunchKernelGGL((dla::stride2_scatter_kernel<dev_t, VV>),
                         dim3((unsigned)((used + 255) / 256)), dim3(256), 0,
                         dla::stream(), (const dev_t*)dy.data_ptr(),
                         (dev_t*)dx.data_ptr(), C, (int)IH, (int)IW, OH, OW,
                         M_in, used);
    };
    if (C % VM == 0) run(std::integral_constant<int, VM>{});
    else run(std::integral_constant<int, 1>{});
  });
  HIP_CHECK_ERR();
  return dx;
}
