// x16 up-sampling of a latent-resolution condition fused with the concatenation behind the image: the input stage of the reference's
// CLIC21GVAELatentConditionalDiscriminator (src/models/discriminator/clic21_gvae_discriminator.py:65-68),
//   out = torch.cat((img, F.interpolate(cond, scale_factor=16, mode=..., align_corners=False)), dim=1),
// and its autograd.  img is [N][16h][16w] pixels of 3 channels (pixel stride >= 4), cond is [N][h][w] pixels of Cc channels, out is
// [N][16h][16w] pixels of ld = Cc + 4 floats: lanes [img0 img1 img2 | cond_0 .. cond_{Cc-1} | 0].
//
// Per axis, output index o reads the sources f0 - E .. f0 - E + T - 1 (clamped to the grid, clamped taps keep their weights) with
//   s = o + 8,  f0 = s / 16 - 1,  u = s % 16,  t = (u + 0.5) / 16          (t is exact in fp32)
//   nearest   source f0 + (u >= 8), weight 1
//   bilinear  E = 0, T = 2, weights 1 - t, t
//   bicubic   E = 1, T = 4, Keys weights with A = -0.75: c2(t + 1), c1(t), c1(1 - t), c2(2 - t)
// which is torch's source coordinate (o + 0.5) / 16 - 0.5 split into its 16 phases.  So all the outputs with one s / 16 share their
// sources, and the tiles are cut in s, not in o: a workgroup owns one band of 16 output rows (s_y / 16 = band, band = 0 .. h: the first
// and the last band are half bands) and UP_TILE_W output columns (s_x / UP_TILE_W = ct) of one image.  Such a tile reads R = 2 + 2E
// condition rows and NS = UP_TC + 1 + 2E condition columns; they are staged in LDS ALREADY CLAMPED and in the OUTPUT's lane order (three
// empty lanes in front, the zero pad lane behind), so that the 3-float offset of the condition inside the pixel is paid once per staged
// element and the hot loop reads and writes whole aligned 16-byte quads.
//
//   forward   up16_fwd_kernel     thread = (output column, quad j of the pixel), consecutive lanes consecutive quads: the row-interpolated
//                                 quads of the R staged rows once (registers), then 16 output rows, each one 16-byte store per lane and
//                                 1 KiB contiguous per wave.  Lanes with j == 0 bring the image quad in; the last quad's pad lane is 0.
//   backward  up16_bwd_kernel     the same thread shape mirrored: 16 rows of dout are read once and folded onto the R source rows in
//                                 registers (rows in order), lanes with j == 0 write dimg; the R x UP_TILE_W column sums meet in LDS and
//                                 one thread per (source row, source column slot, quad) folds its <= 16 T columns in column order
//                                 -> part[n][band][r][ct][slot][ld]
//             up16_gather_kernel  one thread per dcond element adds the partials of the tiles that reach it: bands in order, rows in
//                                 order, column tiles in order, slots in order (clamped taps of the edges fold here)
//             up16_dimg_kernel    dimg alone (generator phase: the discriminator is frozen)
// No float atomics: which thread adds what and in which order follows from the descriptor alone.
#include <algorithm>

#include "common.hpp"

namespace crdr {

constexpr int UP_THREADS = 256;
constexpr int UP_TC = 8;                 // condition columns whose 16 phases one tile covers
constexpr int UP_TILE_W = 16 * UP_TC;    // output columns of a tile
constexpr int UP_MAX_CC = 64;
constexpr int UP_MAX_LD = UP_MAX_CC + 4;
constexpr int UP_MAX_GRID = 2048;        // dimg alone: grid-stride above this many workgroups

template <int MODE>
struct UpGeom {
  static constexpr int E = MODE == 2 ? 1 : 0;   // extra taps on either side
  static constexpr int T = MODE == 2 ? 4 : 2;   // staged sources an output reads per axis (nearest: one of two)
  static constexpr int R = 2 + 2 * E;           // staged rows of a band
  static constexpr int NS = UP_TC + 1 + 2 * E;  // staged column slots of a tile
};

struct UpArgs {
  const float *img, *cond, *dout;
  float *out, *dimg, *dcond, *part;
  int N, h, w, Cc, Q, ldi, ldc, ldo, nct;
};

__device__ __forceinline__ float up_c1(float x) { return ((1.25f * x - 2.25f) * x) * x + 1.f; }               // |x| <= 1, A = -0.75
__device__ __forceinline__ float up_c2(float x) { return ((-0.75f * x + 3.75f) * x - 6.f) * x + 3.f; }        // 1 < |x| < 2

// weight of tap tx at phase u (nearest: 1 for the tap it reads, 0 for the other -- used as a selector, never as a factor)
template <int MODE>
__device__ __forceinline__ float up_w(int u, int tx) {
  const float t = ((float)u + 0.5f) * 0.0625f;
  if (MODE == 0) return ((u >= 8) == (tx == 1)) ? 1.f : 0.f;
  if (MODE == 1) return tx == 0 ? 1.f - t : t;
  const float x = tx == 0 ? t + 1.f : (tx == 1 ? t : (tx == 2 ? 1.f - t : 2.f - t));
  return (tx == 0 || tx == 3) ? up_c2(x) : up_c1(x);
}

__device__ __forceinline__ int up_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

struct UpTile {
  int64_t n;
  int band, ct;
};

__device__ __forceinline__ UpTile up_tile(const UpArgs& a) {
  UpTile t;
  const int64_t b = blockIdx.x;
  t.ct = (int)(b % a.nct);
  t.band = (int)((b / a.nct) % (a.h + 1));
  t.n = b / ((int64_t)a.nct * (a.h + 1));
  return t;
}

template <int MODE>
__global__ __launch_bounds__(UP_THREADS) void up16_fwd_kernel(const UpArgs a) {
  using G = UpGeom<MODE>;
  __shared__ __attribute__((aligned(16))) float L[G::R * G::NS * UP_MAX_LD];
  const UpTile tl = up_tile(a);
  const int ld = 4 * a.Q;   // floats of a staged pixel = lanes of an output pixel
  for (int idx = threadIdx.x; idx < G::R * G::NS * ld; idx += UP_THREADS) {
    const int lane = idx % ld, slot = (idx / ld) % G::NS, r = idx / (ld * G::NS);
    const int row = up_clamp(tl.band - 1 - G::E + r, a.h), col = up_clamp(UP_TC * tl.ct - 1 - G::E + slot, a.w);
    const int ch = lane - 3;
    L[idx] = (ch >= 0 && ch < a.Cc) ? a.cond[((tl.n * a.h + row) * a.w + col) * a.ldc + ch] : 0.f;
  }
  __syncthreads();
  const int H = 16 * a.h, W = 16 * a.w;
  for (int it = threadIdx.x; it < UP_TILE_W * a.Q; it += UP_THREADS) {
    const int lx = it / a.Q, j = it - lx * a.Q;
    const int ox = UP_TILE_W * tl.ct + lx - 8;
    if (ox < 0 || ox >= W) continue;
    const int g = lx >> 4, u = lx & 15;
    f32x4 hq[G::R];
#pragma unroll
    for (int r = 0; r < G::R; ++r) {
      const float* row = L + (r * G::NS + g) * ld + 4 * j;
      if (MODE == 0) {
        hq[r] = *reinterpret_cast<const f32x4*>(row + (u >= 8 ? ld : 0));
      } else {
        f32x4 acc = up_w<MODE>(u, 0) * *reinterpret_cast<const f32x4*>(row);
#pragma unroll
        for (int tx = 1; tx < G::T; ++tx) acc += up_w<MODE>(u, tx) * *reinterpret_cast<const f32x4*>(row + tx * ld);
        hq[r] = acc;
      }
    }
#pragma unroll
    for (int ly = 0; ly < 16; ++ly) {
      const int oy = 16 * tl.band + ly - 8;
      if (oy < 0 || oy >= H) continue;   // the half bands at the top and the bottom (the same in every lane)
      f32x4 v;
      if (MODE == 0) {
        v = hq[ly >= 8 ? 1 : 0];
      } else {
        v = up_w<MODE>(ly, 0) * hq[0];
#pragma unroll
        for (int ty = 1; ty < G::T; ++ty) v += up_w<MODE>(ly, ty) * hq[ty];
      }
      const int64_t pix = (tl.n * H + oy) * W + ox;
      if (j == 0) {
        const f32x4 im = *reinterpret_cast<const f32x4*>(a.img + pix * a.ldi);
        v[0] = im[0]; v[1] = im[1]; v[2] = im[2];
      }
      if (j == a.Q - 1) v[3] = 0.f;
      *reinterpret_cast<f32x4*>(a.out + pix * a.ldo + 4 * j) = v;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(UP_THREADS) void up16_bwd_kernel(const UpArgs a) {
  using G = UpGeom<MODE>;
  extern __shared__ __attribute__((aligned(16))) float S[];   // [R][UP_TILE_W][ld]: the column sums of the band, folded onto the source rows
  const UpTile tl = up_tile(a);
  const int ld = 4 * a.Q;
  const int H = 16 * a.h, W = 16 * a.w;
  for (int it = threadIdx.x; it < UP_TILE_W * a.Q; it += UP_THREADS) {
    const int lx = it / a.Q, j = it - lx * a.Q;
    const int ox = UP_TILE_W * tl.ct + lx - 8;
    f32x4 v[G::R];
#pragma unroll
    for (int r = 0; r < G::R; ++r) v[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ox >= 0 && ox < W) {
#pragma unroll
      for (int ly = 0; ly < 16; ++ly) {
        const int oy = 16 * tl.band + ly - 8;
        if (oy < 0 || oy >= H) continue;
        const int64_t pix = (tl.n * H + oy) * W + ox;
        const f32x4 d = *reinterpret_cast<const f32x4*>(a.dout + pix * a.ldo + 4 * j);
        if (j == 0 && a.dimg) *reinterpret_cast<f32x4*>(a.dimg + pix * a.ldi) = f32x4{d[0], d[1], d[2], 0.f};
        if (MODE == 0) {
          v[ly >= 8 ? 1 : 0] += d;
        } else {
#pragma unroll
          for (int ty = 0; ty < G::T; ++ty) v[ty] += up_w<MODE>(ly, ty) * d;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < G::R; ++r) *reinterpret_cast<f32x4*>(S + ((size_t)(r * UP_TILE_W + lx) * ld + 4 * j)) = v[r];
  }
  __syncthreads();
  // fold the columns onto the source column slots: slot cs takes tap tx = cs - g of the 16 phases of group g, groups and phases in order
  for (int idx = threadIdx.x; idx < G::R * G::NS * a.Q; idx += UP_THREADS) {
    const int j = idx % a.Q, cs = (idx / a.Q) % G::NS, r = idx / (a.Q * G::NS);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tx = G::T - 1; tx >= 0; --tx) {   // g = cs - tx ascending
      const int g = cs - tx;
      if (g < 0 || g >= UP_TC) continue;
      const float* col = S + ((size_t)(r * UP_TILE_W + 16 * g) * ld + 4 * j);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        if (MODE == 0) {
          if ((u >= 8) == (tx == 1)) acc += *reinterpret_cast<const f32x4*>(col + u * ld);
        } else {
          acc += up_w<MODE>(u, tx) * *reinterpret_cast<const f32x4*>(col + u * ld);
        }
      }
    }
    const int64_t slot = (((tl.n * (a.h + 1) + tl.band) * G::R + r) * a.nct + tl.ct) * G::NS + cs;
    *reinterpret_cast<f32x4*>(a.part + slot * ld + 4 * j) = acc;
  }
}

template <int MODE>
__global__ __launch_bounds__(UP_THREADS) void up16_gather_kernel(const UpArgs a, int64_t total) {
  using G = UpGeom<MODE>;
  const int64_t e = (int64_t)blockIdx.x * UP_THREADS + threadIdx.x;
  if (e >= total) return;
  const int ch = (int)(e % a.Cc);
  const int k = (int)((e / a.Cc) % a.w);
  const int i = (int)((e / ((int64_t)a.Cc * a.w)) % a.h);
  const int64_t n = e / ((int64_t)a.Cc * a.w * a.h);
  const int ld = 4 * a.Q;
  // the bands and column tiles whose staged (clamped) sources can be row i / column k
  const int b0 = i - G::E < 0 ? 0 : i - G::E, b1 = i + 1 + G::E > a.h ? a.h : i + 1 + G::E;
  const int num = k - UP_TC + 1 - G::E;
  const int c0 = num <= 0 ? 0 : (num + UP_TC - 1) / UP_TC;
  const int c1 = (k == a.w - 1 || (k + 1 + G::E) / UP_TC > a.nct - 1) ? a.nct - 1 : (k + 1 + G::E) / UP_TC;
  float acc = 0.f;
  for (int b = b0; b <= b1; ++b)
    for (int r = 0; r < G::R; ++r) {
      if (up_clamp(b - 1 - G::E + r, a.h) != i) continue;
      for (int ct = c0; ct <= c1; ++ct)
        for (int cs = 0; cs < G::NS; ++cs) {
          if (up_clamp(UP_TC * ct - 1 - G::E + cs, a.w) != k) continue;
          const int64_t slot = (((n * (a.h + 1) + b) * G::R + r) * a.nct + ct) * G::NS + cs;
          acc += a.part[slot * ld + 3 + ch];
        }
    }
  a.dcond[((n * a.h + i) * a.w + k) * a.ldc + ch] = acc;
}

__global__ __launch_bounds__(UP_THREADS) void up16_dimg_kernel(const float* dout, int lddo, float* dimg, int lddi, int64_t pixels) {
  for (int64_t p = (int64_t)blockIdx.x * UP_THREADS + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * UP_THREADS) {
    const f32x4 d = *reinterpret_cast<const f32x4*>(dout + p * lddo);
    *reinterpret_cast<f32x4*>(dimg + p * lddi) = f32x4{d[0], d[1], d[2], 0.f};
  }
}

namespace {

struct UpShape {
  int nct, R, NS, ld;
  int64_t blocks;
  size_t part_floats, lds_bytes;
};

UpShape up_shape(const crdr_upsample16_desc* d) {
  UpShape s;
  const int E = d->mode == 2 ? 1 : 0;
  s.R = 2 + 2 * E;
  s.NS = UP_TC + 1 + 2 * E;
  s.ld = d->Cc + 4;
  s.nct = (16 * d->w + 7) / UP_TILE_W + 1;   // s_x = o_x + 8 runs over [8, 16 w + 8)
  s.blocks = (int64_t)d->N * (d->h + 1) * s.nct;
  s.part_floats = (size_t)s.blocks * s.R * s.NS * s.ld;
  s.lds_bytes = (size_t)s.R * UP_TILE_W * s.ld * sizeof(float);
  return s;
}

inline bool up_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int up_check(const crdr_upsample16_desc* d, const char* what) {
  CRDR_REQUIRE(d, "%s: null descriptor", what);
  CRDR_REQUIRE(d->mode >= 0 && d->mode <= 2, "%s: mode = %d (0 nearest, 1 bilinear, 2 bicubic)", what, d->mode);
  CRDR_REQUIRE(d->N >= 0 && d->N <= (1 << 20) && d->h >= 1 && d->w >= 1 && d->h <= (1 << 20) && d->w <= (1 << 20), "%s: N = %d, latent grid %d x %d", what, d->N, d->h,
               d->w);
  CRDR_REQUIRE(d->Cc >= 4 && d->Cc % 4 == 0 && d->Cc <= UP_MAX_CC, "%s: the condition's channel count must be a multiple of 4 in [4, %d] (got %d)",
               what, UP_MAX_CC, d->Cc);
  CRDR_REQUIRE(d->ldi % 4 == 0 && d->ldi >= 4, "%s: the image's pixel stride is %d (needs a multiple of 4, >= 4: 3 channels and a pad lane)", what,
               d->ldi);
  CRDR_REQUIRE(d->ldc % 4 == 0 && d->ldc >= d->Cc, "%s: the condition's pixel stride is %d (needs a multiple of 4, >= %d)", what, d->ldc, d->Cc);
  CRDR_REQUIRE(d->ldo % 4 == 0 && d->ldo >= d->Cc + 4, "%s: the output's pixel stride is %d (needs a multiple of 4, >= %d)", what, d->ldo, d->Cc + 4);
  CRDR_REQUIRE(up_shape(d).blocks < ((int64_t)1 << 30), "%s: tensor too large", what);
  return 0;
}

UpArgs up_args(const crdr_upsample16_desc* d, const UpShape& s) {
  UpArgs a = {};
  a.N = d->N; a.h = d->h; a.w = d->w; a.Cc = d->Cc; a.Q = s.ld / 4; a.ldi = d->ldi; a.ldc = d->ldc; a.ldo = d->ldo; a.nct = s.nct;
  return a;
}

std::atomic<bool> g_up_lds_done{false};

}  // namespace
}  // namespace crdr

using namespace crdr;

extern "C" size_t crdr_upsample16_cat_workspace(const crdr_upsample16_desc* d) {
  if (up_check(d, "upsample16_cat_workspace") || d->N == 0) return 0;
  return up_shape(d).part_floats * sizeof(float);
}

extern "C" int crdr_upsample16_cat_fwd(const crdr_upsample16_desc* d, const float* img, const float* cond, float* out, crdr_stream_t s) {
  if (int rc = up_check(d, "upsample16_cat_fwd")) return rc;
  CRDR_REQUIRE(img && cond && out, "upsample16_cat_fwd: null pointer");
  CRDR_REQUIRE(up_aligned16(img) && up_aligned16(cond) && up_aligned16(out), "upsample16_cat_fwd: operands must be 16-byte aligned");
  if (d->N == 0) return 0;
  const UpShape sh = up_shape(d);
  UpArgs a = up_args(d, sh);
  a.img = img; a.cond = cond; a.out = out;
  const dim3 grid((unsigned)sh.blocks), block(UP_THREADS);
  hipStream_t st = as_stream(s);
  if (d->mode == 0) hipLaunchKernelGGL(up16_fwd_kernel<0>, grid, block, 0, st, a);
  else if (d->mode == 1) hipLaunchKernelGGL(up16_fwd_kernel<1>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(up16_fwd_kernel<2>, grid, block, 0, st, a);
  CRDR_CHECK_LAUNCH("upsample16_cat_fwd");
  return 0;
}

extern "C" int crdr_upsample16_cat_bwd(const crdr_upsample16_desc* d, const float* dout, float* dimg, float* dcond, void* ws, size_t ws_bytes,
                                       crdr_stream_t s) {
  if (int rc = up_check(d, "upsample16_cat_bwd")) return rc;
  CRDR_REQUIRE(dout, "upsample16_cat_bwd: null pointer");
  CRDR_REQUIRE(up_aligned16(dout) && up_aligned16(dimg) && up_aligned16(dcond) && up_aligned16(ws),
               "upsample16_cat_bwd: operands must be 16-byte aligned");
  if (d->N == 0 || (!dimg && !dcond)) return 0;
  const UpShape sh = up_shape(d);
  hipStream_t st = as_stream(s);
  if (!dcond) {
    const int64_t pixels = (int64_t)d->N * 16 * d->h * 16 * d->w;
    const int grid = (int)std::min<int64_t>(cdiv64(pixels, UP_THREADS), UP_MAX_GRID);
    hipLaunchKernelGGL(up16_dimg_kernel, dim3(grid), dim3(UP_THREADS), 0, st, dout, d->ldo, dimg, d->ldi, pixels);
    CRDR_CHECK_LAUNCH("upsample16_cat_dimg");
    return 0;
  }
  CRDR_REQUIRE(ws && ws_bytes >= sh.part_floats * sizeof(float), "upsample16_cat_bwd: workspace too small (%zu < %zu)", ws_bytes,
               sh.part_floats * sizeof(float));
  using BwdKernel = void (*)(const UpArgs);
  static const BwdKernel bwd[3] = {up16_bwd_kernel<0>, up16_bwd_kernel<1>, up16_bwd_kernel<2>};
  allow_full_lds(g_up_lds_done, bwd, 3);
  UpArgs a = up_args(d, sh);
  a.dout = dout; a.dimg = dimg; a.dcond = dcond; a.part = (float*)ws;
  hipLaunchKernelGGL(bwd[d->mode], dim3((unsigned)sh.blocks), dim3(UP_THREADS), sh.lds_bytes, st, a);
  CRDR_CHECK_LAUNCH("upsample16_cat_bwd");
  const int64_t total = (int64_t)d->N * d->h * d->w * d->Cc;
  const dim3 ggrid((unsigned)cdiv64(total, UP_THREADS)), block(UP_THREADS);
  if (d->mode == 0) hipLaunchKernelGGL(up16_gather_kernel<0>, ggrid, block, 0, st, a, total);
  else if (d->mode == 1) hipLaunchKernelGGL(up16_gather_kernel<1>, ggrid, block, 0, st, a, total);
  else hipLaunchKernelGGL(up16_gather_kernel<2>, ggrid, block, 0, st, a, total);
  CRDR_CHECK_LAUNCH("upsample16_cat_gather");
  return 0;
}
