// nn.PixelShuffle(2) on NHWC memory: the depth-to-space step of a sub-pixel convolution (the reference's second up-sampling form,
// src/models/layer/elic_layers.py:16-20) and its autograd.  x is [N][H][W] pixels of 4C channels in torch's order ch = 4c + 2i + j, y is
// [N][2H][2W] pixels of C channels: y[n][2h+i][2w+j][c] = x[n][h][w][4c+2i+j].
//
// Pure data movement: no LDS, no atomics, bit exact.  One thread owns output channels c..c+3 of one input pixel -- 64 contiguous bytes of the
// input row (four channels x four phases): four 16-byte loads, a 4x4 transpose in registers, four 16-byte stores, one to each of the four
// output pixels.  Consecutive lanes take consecutive channel quads, so a wave's loads are one contiguous run along the row(s) and its stores
// four contiguous runs.  The backward is the same thread shape mirrored.  C == 3 (the image layer): the 12-float input row of a pixel is
// three quads, the output is the image layout (pixel stride 4, zero fourth lane); one thread per input pixel.  Grid-stride over a capped
// grid, 64-bit element offsets, strides in floats (channel slices of wider NHWC tensors).
#include <algorithm>

#include "common.hpp"

namespace crdr {

struct PsArgs {
  const float* src;   // forward: x, backward: dy
  float* dst;         // forward: y, backward: dx
  int64_t total;      // threads: N H W Q
  int H, W, Q;        // input pixels, channel quads per OUTPUT pixel (1 for the RGB form)
  int ldx, ldy;       // pixel strides of the 4C side and of the C side
};

// (input pixel p = (n, h, w), phase k = 2i + j) -> element offset of output pixel (n, 2h+i, 2w+j)
__device__ __forceinline__ int64_t ps_out_pixel(int64_t n, int h, int w, int k, int H, int W) {
  return (n * (2 * H) + (2 * h + (k >> 1))) * (int64_t)(2 * W) + (2 * w + (k & 1));
}

template <bool BWD>
__global__ __launch_bounds__(256) void pixel_shuffle_kernel(const PsArgs a) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < a.total; t += (int64_t)gridDim.x * 256) {
    const int q = (int)(t % a.Q);
    int64_t p = t / a.Q;
    const int w = (int)(p % a.W);
    const int64_t nh = p / a.W;
    const int h = (int)(nh % a.H);
    const int64_t n = nh / a.H;
    const int64_t xo = p * a.ldx + 16 * q;
    f32x4 v[4], o[4];
    if (!BWD) {
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = *reinterpret_cast<const f32x4*>(a.src + xo + 4 * c);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[k] = f32x4{v[0][k], v[1][k], v[2][k], v[3][k]};
        *reinterpret_cast<f32x4*>(a.dst + ps_out_pixel(n, h, w, k, a.H, a.W) * a.ldy + 4 * q) = o[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = *reinterpret_cast<const f32x4*>(a.src + ps_out_pixel(n, h, w, k, a.H, a.W) * a.ldy + 4 * q);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        v[c] = f32x4{o[0][c], o[1][c], o[2][c], o[3][c]};
        *reinterpret_cast<f32x4*>(a.dst + xo + 4 * c) = v[c];
      }
    }
  }
}

// C == 3: x rows of 12 floats, y in the image layout [c0, c1, c2, 0]
template <bool BWD>
__global__ __launch_bounds__(256) void pixel_shuffle_rgb_kernel(const PsArgs a) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.total; p += (int64_t)gridDim.x * 256) {
    const int w = (int)(p % a.W);
    const int64_t nh = p / a.W;
    const int h = (int)(nh % a.H);
    const int64_t n = nh / a.H;
    const int64_t xo = p * a.ldx;
    f32x4 v[3], o[4];
    if (!BWD) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const f32x4*>(a.src + xo + 4 * c);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[k] = f32x4{v[0][k], v[1][k], v[2][k], 0.f};
        *reinterpret_cast<f32x4*>(a.dst + ps_out_pixel(n, h, w, k, a.H, a.W) * a.ldy) = o[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = *reinterpret_cast<const f32x4*>(a.src + ps_out_pixel(n, h, w, k, a.H, a.W) * a.ldy);
#pragma unroll
      for (int c = 0; c < 3; ++c) {   // the fourth lane of dy is not read into anything
        v[c] = f32x4{o[0][c], o[1][c], o[2][c], o[3][c]};
        *reinterpret_cast<f32x4*>(a.dst + xo + 4 * c) = v[c];
      }
    }
  }
}

namespace {

constexpr int PS_MAX_GRID = 2048;   // workgroups of 256 threads: eight per CU, the rest of the tensor by the grid-stride loop

int pixel_shuffle_launch(const char* what, bool bwd, const float* src, float* dst, int N, int H, int W, int C, int ldx, int ldy, crdr_stream_t s) {
  CRDR_REQUIRE(src && dst, "%s: null pointer", what);
  CRDR_REQUIRE(N >= 0 && H >= 1 && W >= 1, "%s: N %d H %d W %d", what, N, H, W);
  CRDR_REQUIRE(C == 3 || (C >= 4 && C % 4 == 0), "%s: C must be 3 or a multiple of 4 (got %d)", what, C);
  CRDR_REQUIRE(C <= (1 << 24) && H <= (1 << 29) && W <= (1 << 29), "%s: tensor too large", what);
  const int cy = round_up(C, 4);
  CRDR_REQUIRE(ldx % 4 == 0 && ldx >= 4 * C, "%s: the pixel stride of the 4C-channel side is %d (needs a multiple of 4, >= %d)", what, ldx, 4 * C);
  CRDR_REQUIRE(ldy % 4 == 0 && ldy >= cy, "%s: the pixel stride of the C-channel side is %d (needs a multiple of 4, >= %d)", what, ldy, cy);
  CRDR_REQUIRE(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0, "%s: operands must be 16-byte aligned", what);
  PsArgs a;
  a.src = src; a.dst = dst; a.H = H; a.W = W; a.Q = C == 3 ? 1 : C / 4; a.ldx = ldx; a.ldy = ldy;
  a.total = (int64_t)N * H * W * a.Q;
  if (a.total == 0) return 0;
  CRDR_REQUIRE(a.total < ((int64_t)1 << 40), "%s: tensor too large", what);
  const int grid = (int)std::min<int64_t>(cdiv64(a.total, 256), PS_MAX_GRID);
  hipStream_t st = as_stream(s);
  if (C == 3) {
    if (bwd) hipLaunchKernelGGL(pixel_shuffle_rgb_kernel<true>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(pixel_shuffle_rgb_kernel<false>, dim3(grid), dim3(256), 0, st, a);
  } else {
    if (bwd) hipLaunchKernelGGL(pixel_shuffle_kernel<true>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(pixel_shuffle_kernel<false>, dim3(grid), dim3(256), 0, st, a);
  }
  CRDR_CHECK_LAUNCH(what);
  return 0;
}

}  // namespace
}  // namespace crdr

using namespace crdr;

extern "C" int crdr_pixel_shuffle_fwd(const float* x, int ldx, int N, int H, int W, int C, float* y, int ldy, crdr_stream_t s) {
  return pixel_shuffle_launch("pixel_shuffle_fwd", false, x, y, N, H, W, C, ldx, ldy, s);
}

extern "C" int crdr_pixel_shuffle_bwd(const float* dy, int lddy, int N, int H, int W, int C, float* dx, int lddx, crdr_stream_t s) {
  return pixel_shuffle_launch("pixel_shuffle_bwd", true, dy, dx, N, H, W, C, lddx, lddy, s);
}
