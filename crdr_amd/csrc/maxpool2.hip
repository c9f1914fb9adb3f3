// nn.MaxPool2d(kernel_size=2, stride=2) on NHWC fp32 memory and its autograd: the four pools between the conv groups of LPIPS-VGG
// (lpips 0.1.4 pretrained_networks.vgg16 / torchvision vgg16.features indices 4, 9, 16, 23).
//   y[n][oh][ow][c] = max over i,j in {0,1} of x[n][2oh+i][2ow+j][c],  OH = H / 2, OW = W / 2 (an odd last row / column is dropped)
//   dx[n][2oh+i][2ow+j][c] = dy[n][oh][ow][c] at the window's FIRST maximum in the scan order (0,0), (0,1), (1,0), (1,1) -- a later
//   value replaces the running best only when it is strictly greater (or a NaN), torch's own rule -- and 0 everywhere else, the
//   pixels of a dropped odd row / column included.
//
// Bandwidth kernels: no LDS, no atomics, no index tensor (the backward recomputes the argmax from x), every element of y / dx written
// exactly once.  One lane owns one channel quad (16-byte loads and stores) of one output pixel; the block is (channel quads, pixels)
// = (min(Q, 256), 256 / that) threads, so consecutive lanes walk the channels of a pixel and then the next pixel of the same output
// row and a wave reads contiguous runs of the two input rows.  The image and the output row are the block's z and y indices: no
// integer division anywhere.  The backward's grid covers ceil(H/2) x ceil(W/2) windows; the partial windows of an odd edge store
// their zeros in the same pass and read nothing.  Element offsets are 64-bit; strides are in floats (channel slices of wider
// NHWC tensors).
#include <algorithm>

#include "common.hpp"

namespace crdr {

struct Mp2Args {
  const float* x;
  const float* dy;    // backward only
  float* out;         // forward: y, backward: dx
  int H, W;           // input pixels
  int OH, OW;         // output pixels (H / 2, W / 2)
  int Q;              // channel quads
  int ldx, ldy, ldo;  // pixel strides of x, of dy (backward) and of `out`
};

__device__ __forceinline__ f32x4 mp2_ld(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void mp2_st(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
// torch's replacement rule (aten/src/ATen/native/cpu/MaxPoolKernel.cpp): strictly greater, or a NaN
__device__ __forceinline__ bool mp2_takes(float v, float best) { return v > best || v != v; }

__global__ __launch_bounds__(256) void maxpool2s2_fwd_kernel(const Mp2Args a) {
  const int ow = blockIdx.x * blockDim.y + threadIdx.y;
  if (ow >= a.OW) return;
  const int oh = blockIdx.y;
  const int64_t n = blockIdx.z;
  const int64_t row = (int64_t)a.W * a.ldx;
  const float* r0 = a.x + (n * a.H + 2 * oh) * row + (int64_t)(2 * ow) * a.ldx;   // rows 2oh, 2oh+1 < H and columns 2ow, 2ow+1 < W
  const float* r1 = r0 + row;
  float* yo = a.out + ((n * a.OH + oh) * (int64_t)a.OW + ow) * a.ldo;
  for (int q = threadIdx.x; q < a.Q; q += blockDim.x) {
    const f32x4 v[4] = {mp2_ld(r0 + 4 * q), mp2_ld(r0 + a.ldx + 4 * q), mp2_ld(r1 + 4 * q), mp2_ld(r1 + a.ldx + 4 * q)};
    f32x4 best = v[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 4; ++c) best[c] = mp2_takes(v[k][c], best[c]) ? v[k][c] : best[c];
    mp2_st(yo + 4 * q, best);
  }
}

__global__ __launch_bounds__(256) void maxpool2s2_bwd_kernel(const Mp2Args a) {
  const int ww = blockIdx.x * blockDim.y + threadIdx.y;   // window column, < ceil(W / 2)
  if (2 * ww >= a.W) return;
  const int wh = blockIdx.y;                              // window row, < ceil(H / 2): pixel (2wh, 2ww) always exists
  const int64_t n = blockIdx.z;
  const bool row1 = 2 * wh + 1 < a.H, col1 = 2 * ww + 1 < a.W;
  const int64_t in_px = (n * a.H + 2 * wh) * (int64_t)a.W + 2 * ww;
  const float* r0 = a.x + in_px * a.ldx;
  const float* r1 = r0 + (int64_t)a.W * a.ldx;
  float* d0 = a.out + in_px * a.ldo;
  float* d1 = d0 + (int64_t)a.W * a.ldo;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (row1 && col1) {   // a whole window: wh < OH and ww < OW
    const float* g = a.dy + ((n * a.OH + wh) * (int64_t)a.OW + ww) * a.ldy;
    for (int q = threadIdx.x; q < a.Q; q += blockDim.x) {
      const f32x4 v[4] = {mp2_ld(r0 + 4 * q), mp2_ld(r0 + a.ldx + 4 * q), mp2_ld(r1 + 4 * q), mp2_ld(r1 + a.ldx + 4 * q)};
      const f32x4 gy = mp2_ld(g + 4 * q);
      f32x4 o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float best = v[0][c];
        int at = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k)
          if (mp2_takes(v[k][c], best)) { best = v[k][c]; at = k; }
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k][c] = at == k ? gy[c] : 0.f;
      }
      mp2_st(d0 + 4 * q, o[0]);
      mp2_st(d0 + a.ldo + 4 * q, o[1]);
      mp2_st(d1 + 4 * q, o[2]);
      mp2_st(d1 + a.ldo + 4 * q, o[3]);
    }
  } else {              // the dropped odd row / column: no window, zero gradient
    for (int q = threadIdx.x; q < a.Q; q += blockDim.x) {
      mp2_st(d0 + 4 * q, zero);
      if (col1) mp2_st(d0 + a.ldo + 4 * q, zero);
      if (row1) mp2_st(d1 + 4 * q, zero);
    }
  }
}

namespace {

constexpr int MP2_MAX_GRID_YZ = 65535;

// the checks both directions share; fills the block and the common fields of the arguments
int maxpool2_plan(const char* what, int N, int H, int W, int C, int ldx, int ldy, Mp2Args* a, dim3* block) {
  CRDR_REQUIRE(N >= 0 && H >= 2 && W >= 2, "%s: N %d H %d W %d (needs H >= 2 and W >= 2)", what, N, H, W);
  CRDR_REQUIRE(C >= 4 && C % 4 == 0, "%s: C must be a multiple of 4 (got %d)", what, C);
  CRDR_REQUIRE(ldx % 4 == 0 && ldx >= C, "%s: the input's pixel stride is %d (needs a multiple of 4, >= %d)", what, ldx, C);
  CRDR_REQUIRE(ldy % 4 == 0 && ldy >= C, "%s: the output's pixel stride is %d (needs a multiple of 4, >= %d)", what, ldy, C);
  CRDR_REQUIRE(N <= MP2_MAX_GRID_YZ && (H + 1) / 2 <= MP2_MAX_GRID_YZ && W <= (1 << 29) && ldx <= (1 << 24) && ldy <= (1 << 24),
               "%s: tensor too large", what);
  a->H = H; a->W = W; a->OH = H / 2; a->OW = W / 2; a->Q = C / 4;
  const int bx = std::min(a->Q, 256);
  *block = dim3(bx, 256 / bx);
  return 0;
}

}  // namespace
}  // namespace crdr

using namespace crdr;

extern "C" int crdr_maxpool2s2_fwd(const float* x, int ldx, int N, int H, int W, int C, float* y, int ldy, crdr_stream_t s) {
  const char* what = "maxpool2s2_fwd";
  Mp2Args a;
  dim3 block;
  if (int rc = maxpool2_plan(what, N, H, W, C, ldx, ldy, &a, &block)) return rc;
  CRDR_REQUIRE(x && y, "%s: null pointer", what);
  CRDR_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0, "%s: operands must be 16-byte aligned", what);
  if (N == 0) return 0;
  a.x = x; a.dy = nullptr; a.out = y; a.ldx = ldx; a.ldy = 0; a.ldo = ldy;
  hipLaunchKernelGGL(maxpool2s2_fwd_kernel, dim3(cdiv(a.OW, (int)block.y), a.OH, N), block, 0, as_stream(s), a);
  CRDR_CHECK_LAUNCH(what);
  return 0;
}

extern "C" int crdr_maxpool2s2_bwd(const float* x, int ldx, const float* dy, int lddy, int N, int H, int W, int C, float* dx, int lddx,
                                   crdr_stream_t s) {
  const char* what = "maxpool2s2_bwd";
  Mp2Args a;
  dim3 block;
  if (int rc = maxpool2_plan(what, N, H, W, C, ldx, lddy, &a, &block)) return rc;
  CRDR_REQUIRE(lddx % 4 == 0 && lddx >= C && lddx <= (1 << 24), "%s: the pixel stride of dx is %d (needs a multiple of 4, >= %d)", what, lddx, C);
  CRDR_REQUIRE(x && dy && dx, "%s: null pointer", what);
  CRDR_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0,
               "%s: operands must be 16-byte aligned", what);
  if (N == 0) return 0;
  a.x = x; a.dy = dy; a.out = dx; a.ldx = ldx; a.ldy = lddy; a.ldo = lddx;
  hipLaunchKernelGGL(maxpool2s2_bwd_kernel, dim3(cdiv((W + 1) / 2, (int)block.y), (H + 1) / 2, N), block, 0, as_stream(s), a);
  CRDR_CHECK_LAUNCH(what);
  return 0;
}
