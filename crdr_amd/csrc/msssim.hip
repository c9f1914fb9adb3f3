// MS-SSIM forward and backward (pytorch_msssim 1.0.0 `ms_ssim`, called at src/losses/distortion_loss.py:61-70 and
// src/utils/img_utils.py:135-162).  Images are NHWC with a pixel stride of 4 floats (<= 4 channels; lanes >= C are
// zeroed on load and get a zero gradient), so one pixel is one 16-byte access and every channel rides in a f32x4.
//
// Per level (5 levels), one launch of msssim_level_fwd: a 16 x 16 tile of the *valid* 11 x 11 Gaussian-filtered maps,
// its 26 x 26 input tile of X and Y in LDS, a vertical then a horizontal pass over the five moments (G*X, G*Y, G*X^2,
// G*Y^2, G*XY), the cs / ssim maps, per-tile partial sums per channel, and -- same launch, an 8 x 8 block per
// workgroup -- the 2 x 2 average-pooled images of the next level.  msssim_stats sums the partials in a fixed order into
// CS_l and S_4; msssim_final forms v = prod relu(CS_l)^w_l relu(S_4)^w_4 and the mean over (n, c).  No float atomics: two identical
// calls give identical bits.
//
// Backward (store, not recompute): the forward writes, per output pixel, the four maps A_x, A_y, B, C such that with
// k = dL/d(per-pixel cs or ssim) -- a per-(n, c) constant -- the adjoints of (G*X, G*Y, G*X^2 = G*Y^2, G*XY) carried
// through sigma = E - mu^2 are k (A_x, A_y, B, C).  Then, with G^T the full (zero-padded by 10) correlation,
//   dX_l = k (G^T A_x + 2 X G^T B + Y G^T C) + pool^T(dX_{l+1}),   dY_l = k (G^T A_y + 2 Y G^T B + X G^T C) + pool^T(dY_{l+1}),
// coarsest level first, one launch of msssim_level_bwd per level.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace crdr {
namespace {

constexpr int MS_LEVELS = 5;
constexpr int K = 11, HALO = K - 1;
constexpr int T = 16;          // output tile side (forward), input-gradient tile side (backward)
constexpr int TI = T + HALO;   // 26: the tile plus the window's reach
constexpr int PT = T / 2;      // side of the pooled block a forward workgroup writes
constexpr float MS_WEIGHTS[MS_LEVELS] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};

struct Geometry {
  int H[MS_LEVELS], W[MS_LEVELS];     // level image sizes
  int gx[MS_LEVELS], gy[MS_LEVELS];   // forward grid (tiles) per level
  size_t img[MS_LEVELS], maps[MS_LEVELS], part[MS_LEVELS], stat, total;   // float offsets into the state buffer
  size_t grad[MS_LEVELS], grad_total;                                     // float offsets into the backward workspace
};

size_t align16(size_t v) { return (v + 15) / 16 * 16; }   // 64-byte sections

void geometry(int N, int H, int W, bool maps, Geometry& g) {
  size_t off = 0, goff = 0;
  for (int l = 0; l < MS_LEVELS; ++l) {
    g.H[l] = l ? (g.H[l - 1] + 1) / 2 : H;   // 2 x 2 average pooling, stride 2, padding side % 2: 2k -> k, 2k + 1 -> k + 1
    g.W[l] = l ? (g.W[l - 1] + 1) / 2 : W;
  }
  for (int l = 0; l < MS_LEVELS; ++l) {
    const int OH = g.H[l] - HALO, OW = g.W[l] - HALO;
    g.gy[l] = cdiv(OH, T);
    g.gx[l] = cdiv(OW, T);
    if (l + 1 < MS_LEVELS) {   // the pooled blocks of the next level ride on the same grid
      g.gy[l] = std::max(g.gy[l], cdiv(g.H[l + 1], PT));
      g.gx[l] = std::max(g.gx[l], cdiv(g.W[l + 1], PT));
    }
    const size_t pix = (size_t)N * g.H[l] * g.W[l] * 4;
    g.img[l] = off;
    if (l) off += align16(2 * pix);   // X then Y of levels 1..4 (level 0 is the caller's input)
    g.maps[l] = off;
    if (maps) off += align16((size_t)N * OH * OW * 16);
    g.part[l] = off;
    off += align16((size_t)N * g.gx[l] * g.gy[l] * 8);
    g.grad[l] = goff;
    if (l) goff += align16(2 * pix);
  }
  g.stat = off;           // [6][N][4]: CS_0..CS_3, S_4, v
  off += align16((size_t)6 * N * 4);
  g.total = off;
  g.grad_total = goff;
}

struct MsFwdArgs {
  const float* x;
  const float* y;
  int ldx, ldy, H, W, C, quant, last;
  float c1, c2;
  float g[K];
  float* px;    // next level's images (ld 4), nullptr at the last level
  float* py;
  int PH, PW, padh, padw;
  float* maps;  // [N][OH][OW][4 maps][4 lanes] or nullptr
  float* part;  // [N][tiles][cs, ssim][4 lanes]
};

// quant: 0 as is; 1 truncate (`.int().float()`); 2 (x + 1) / 2 * 255 then truncate (cvt_range_to_255 first)
__device__ __forceinline__ f32x4 ms_load(const float* p, int ld, int64_t pix, int C, int quant) {
  f32x4 v = *reinterpret_cast<const f32x4*>(p + pix * ld);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float e = v[j];
    if (quant == 2) e = (e + 1.f) / 2.f * 255.f;
    if (quant) e = truncf(e);
    v[j] = j < C ? e : 0.f;
  }
  return v;
}

__device__ __forceinline__ f32x4 wave_sum4(f32x4 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += __shfl_down(v[j], o, 64);
  return v;
}

__global__ __launch_bounds__(256) void msssim_level_fwd(const MsFwdArgs a) {
  __shared__ f32x4 sx[TI][TI], sy[TI][TI];   // 21.1 KiB
  __shared__ f32x4 sv[5][T][TI];             // 32.5 KiB: the five moments after the vertical pass
  __shared__ f32x4 red[2][4];
  const int n = blockIdx.z, tid = threadIdx.x;
  const int H = a.H, W = a.W, OH = H - HALO, OW = W - HALO;
  const int oy0 = blockIdx.y * T, ox0 = blockIdx.x * T;
  const int64_t base = (int64_t)n * H * W;

  for (int e = tid; e < TI * TI; e += 256) {
    const int r = e / TI, c = e - r * TI, gy = oy0 + r, gx = ox0 + c;
    f32x4 vx = {0.f, 0.f, 0.f, 0.f}, vy = vx;
    if (gy < H && gx < W) {   // taps beyond the image only feed outputs beyond the valid map
      vx = ms_load(a.x, a.ldx, base + (int64_t)gy * W + gx, a.C, a.quant);
      vy = ms_load(a.y, a.ldy, base + (int64_t)gy * W + gx, a.C, a.quant);
    }
    sx[r][c] = vx;
    sy[r][c] = vy;
  }
  // 2 x 2 average pooling (stride 2, padding (H % 2, W % 2), pad counted in the divisor): the pooled 8 x 8 block this workgroup owns,
  // summed in torch's window order and divided by 4 whatever the pad
  if (a.px && tid < 2 * PT * PT) {
    const int img = tid / (PT * PT), q = tid % (PT * PT);
    const int i = blockIdx.y * PT + q / PT, j = blockIdx.x * PT + q % PT;
    if (i < a.PH && j < a.PW) {
      const float* src = img ? a.y : a.x;
      const int ld = img ? a.ldy : a.ldx;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int r = 2 * i - a.padh + dy, c = 2 * j - a.padw + dx;   // r <= H - 1, c <= W - 1 by the pooled size
          if (r >= 0 && c >= 0) s += ms_load(src, ld, base + (int64_t)r * W + c, a.C, a.quant);
        }
      float* dst = img ? a.py : a.px;
      *reinterpret_cast<f32x4*>(dst + ((int64_t)n * a.PH * a.PW + (int64_t)i * a.PW + j) * 4) = s * 0.25f;
    }
  }
  __syncthreads();
  for (int e = tid; e < T * TI; e += 256) {
    const int r = e / TI, c = e - r * TI;
    f32x4 m0 = {0.f, 0.f, 0.f, 0.f}, m1 = m0, m2 = m0, m3 = m0, m4 = m0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const f32x4 u = sx[r + t][c], v = sy[r + t][c];
      const float w = a.g[t];
      m0 += w * u;
      m1 += w * v;
      m2 += w * (u * u);
      m3 += w * (v * v);
      m4 += w * (u * v);
    }
    sv[0][r][c] = m0;
    sv[1][r][c] = m1;
    sv[2][r][c] = m2;
    sv[3][r][c] = m3;
    sv[4][r][c] = m4;
  }
  __syncthreads();
  const int r = tid / T, c = tid % T, oy = oy0 + r, ox = ox0 + c;
  f32x4 cs = {0.f, 0.f, 0.f, 0.f}, ss = cs;
  if (oy < OH && ox < OW) {
    f32x4 mx = cs, my = cs, exx = cs, eyy = cs, exy = cs;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const float w = a.g[t];
      mx += w * sv[0][r][c + t];
      my += w * sv[1][r][c + t];
      exx += w * sv[2][r][c + t];
      eyy += w * sv[3][r][c + t];
      exy += w * sv[4][r][c + t];
    }
    const f32x4 mxx = mx * mx, myy = my * my, mxy = mx * my;
    const f32x4 sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
    const f32x4 B = sxx + syy + a.c2;
    cs = (2.f * sxy + a.c2) / B;
    const f32x4 B1 = mxx + myy + a.c1;
    const f32x4 lum = (2.f * mxy + a.c1) / B1;
    ss = lum * cs;
    if (a.maps) {
      f32x4 Ax, Ay, Bm, Cm;
      if (!a.last) {   // adjoint of cs
        Ax = 2.f * (mx * cs - my) / B;
        Ay = 2.f * (my * cs - mx) / B;
        Bm = -cs / B;
        Cm = 2.f / B;
      } else {         // adjoint of ssim = lum * cs
        Ax = 2.f * cs * (my - lum * mx) / B1 + 2.f * lum * (mx * cs - my) / B;
        Ay = 2.f * cs * (mx - lum * my) / B1 + 2.f * lum * (my * cs - mx) / B;
        Bm = -lum * cs / B;
        Cm = 2.f * lum / B;
      }
      f32x4* m = reinterpret_cast<f32x4*>(a.maps + (((int64_t)n * OH + oy) * OW + ox) * 16);
      m[0] = Ax;
      m[1] = Ay;
      m[2] = Bm;
      m[3] = Cm;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j >= a.C) cs[j] = ss[j] = 0.f;
  }
  cs = wave_sum4(cs);
  ss = wave_sum4(ss);
  const int lane = tid & 63, wv = tid >> 6;
  if (lane == 0) {
    red[0][wv] = cs;
    red[1][wv] = ss;
  }
  __syncthreads();
  if (tid < 2) {
    const f32x4 s = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
    const int64_t tile = (int64_t)n * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x;
    *reinterpret_cast<f32x4*>(a.part + (tile * 2 + tid) * 4) = s;
  }
}

struct MsFinalArgs {
  const float* part[MS_LEVELS];
  int tiles[MS_LEVELS];
  float count[MS_LEVELS];   // output pixels per level
  float w[MS_LEVELS];
  float* stat;              // [6][N][4]
  float* out;
  int N, C;
};

// CS_l (l < 4) from the cs partials, S_4 from the ssim partials: one workgroup per (level, n), one wave per lane, a fixed order
__global__ __launch_bounds__(256) void msssim_stats(const MsFinalArgs a) {
  const int l = blockIdx.x / a.N, n = blockIdx.x - l * a.N, lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int tiles = a.tiles[l], which = l == MS_LEVELS - 1;
  const float* part = a.part[l];
  float s = 0.f;
  for (int t = lane; t < tiles; t += 64) s += part[(((int64_t)n * tiles + t) * 2 + which) * 4 + j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (lane == 0) a.stat[(l * a.N + n) * 4 + j] = s / a.count[l];
}

__global__ __launch_bounds__(256) void msssim_final(const MsFinalArgs a) {
  const int tid = threadIdx.x, N4 = a.N * 4;
  for (int p = tid; p < N4; p += 256) {
    float v = 0.f;
    if ((p & 3) < a.C) {
      v = 1.f;
#pragma unroll
      for (int l = 0; l < MS_LEVELS; ++l) v *= powf(fmaxf(a.stat[l * N4 + p], 0.f), a.w[l]);
    }
    a.stat[MS_LEVELS * N4 + p] = v;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int n = 0; n < a.N; ++n)
      for (int j = 0; j < a.C; ++j) s += a.stat[MS_LEVELS * N4 + n * 4 + j];
    a.out[0] = s / (float)(a.N * a.C);
  }
}

struct MsBwdArgs {
  const float* x;
  const float* y;
  int ldx, ldy, H, W, C, N, level;
  float g[K];
  const float* maps;   // this level's [N][OH][OW][16]
  const float* stat;   // [6][N][4]
  const float* gout;   // dL/d(mean ms-ssim)
  float w, denom;      // the level's weight; N * C * OH * OW
  const float* dxp;    // next level's image gradients (ld 4), nullptr at the last level
  const float* dyp;
  int PH, PW, padh, padw;
  float* dx;           // may be nullptr
  float* dy;
  int lddx, lddy;
};

__global__ __launch_bounds__(256) void msssim_level_bwd(const MsBwdArgs a) {
  __shared__ f32x4 sm[TI][TI];       // 10.6 KiB: one map's tile, output rows / columns [i0 - 10, i0 + 16)
  __shared__ f32x4 sv[4][T][TI];     // 26 KiB: the four maps after the vertical pass
  const int n = blockIdx.z, tid = threadIdx.x;
  const int H = a.H, W = a.W, OH = H - HALO, OW = W - HALO;
  const int iy0 = blockIdx.y * T, ix0 = blockIdx.x * T;
  const float* mp = a.maps + (int64_t)n * OH * OW * 16;
  for (int m = 0; m < 4; ++m) {
    for (int e = tid; e < TI * TI; e += 256) {
      const int r = e / TI, c = e - r * TI, oy = iy0 - HALO + r, ox = ix0 - HALO + c;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (oy >= 0 && oy < OH && ox >= 0 && ox < OW) v = *reinterpret_cast<const f32x4*>(mp + ((int64_t)oy * OW + ox) * 16 + m * 4);
      sm[r][c] = v;
    }
    __syncthreads();
    for (int e = tid; e < T * TI; e += 256) {
      const int r = e / TI, c = e - r * TI;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < K; ++t) s += a.g[t] * sm[r + HALO - t][c];   // input row i takes output rows i - t
      sv[m][r][c] = s;
    }
    __syncthreads();
  }
  const int r = tid / T, c = tid % T, iy = iy0 + r, ix = ix0 + c;
  if (iy >= H || ix >= W) return;
  f32x4 hA = {0.f, 0.f, 0.f, 0.f}, hB = hA, hC = hA, hD = hA;
#pragma unroll
  for (int t = 0; t < K; ++t) {
    const float w = a.g[t];
    hA += w * sv[0][r][c + HALO - t];
    hB += w * sv[1][r][c + HALO - t];
    hC += w * sv[2][r][c + HALO - t];
    hD += w * sv[3][r][c + HALO - t];
  }
  // k = gout * dv/dstat / (N C P) = gout v w / stat / (N C P) where stat > 0 (relu: zero gradient otherwise)
  const int N4 = a.N * 4;
  const float go = a.gout[0];
  f32x4 k;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float st = a.stat[a.level * N4 + n * 4 + j], v = a.stat[MS_LEVELS * N4 + n * 4 + j];
    k[j] = (j < a.C && st > 0.f) ? go * v * a.w / st / a.denom : 0.f;
  }
  const int64_t pix = (int64_t)n * H * W + (int64_t)iy * W + ix;
  const f32x4 X = *reinterpret_cast<const f32x4*>(a.x + pix * a.ldx);
  const f32x4 Y = *reinterpret_cast<const f32x4*>(a.y + pix * a.ldy);
  const int64_t par = a.dxp || a.dyp ? ((int64_t)n * a.PH + ((iy + a.padh) >> 1)) * a.PW + ((ix + a.padw) >> 1) : 0;
  if (a.dx) {
    f32x4 d = k * (hA + 2.f * X * hC + Y * hD);
    if (a.dxp) d += 0.25f * *reinterpret_cast<const f32x4*>(a.dxp + par * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j >= a.C) d[j] = 0.f;
    *reinterpret_cast<f32x4*>(a.dx + pix * a.lddx) = d;
  }
  if (a.dy) {
    f32x4 d = k * (hB + 2.f * Y * hC + X * hD);
    if (a.dyp) d += 0.25f * *reinterpret_cast<const f32x4*>(a.dyp + par * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j >= a.C) d[j] = 0.f;
    *reinterpret_cast<f32x4*>(a.dy + pix * a.lddy) = d;
  }
}

// pytorch_msssim _fspecial_gauss_1d(11, 1.5), in fp32
void window(float (&g)[K]) {
  float s = 0.f;
  for (int t = 0; t < K; ++t) {
    const float d = (float)(t - K / 2);
    g[t] = std::exp(-(d * d) / (2.f * 1.5f * 1.5f));
    s += g[t];
  }
  for (int t = 0; t < K; ++t) g[t] /= s;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" size_t crdr_msssim_workspace(int N, int H, int W, int which) {
  if (N < 1 || std::min(H, W) <= HALO << 4) return 0;
  Geometry g;
  geometry(N, H, W, which == 1, g);
  return (which == 2 ? g.grad_total : g.total) * sizeof(float);
}

extern "C" int crdr_msssim_fwd(const float* x, int ldx, const float* y, int ldy, int N, int H, int W, int C, float data_range,
                               int quant, float* state, size_t state_bytes, int with_maps, float* out, crdr_stream_t s) {
  CRDR_REQUIRE(x && y && state && out, "msssim_fwd: null pointer");
  CRDR_REQUIRE(N >= 1 && C >= 1 && C <= 4 && ldx == 4 && ldy == 4 && aligned16(x) && aligned16(y) && aligned16(state),
               "msssim_fwd: NHWC images of <= 4 channels with a 16-byte aligned pixel stride of 4 (C %d, ld %d / %d)", C, ldx, ldy);
  CRDR_REQUIRE(std::min(H, W) > HALO << 4, "msssim_fwd: image size should be larger than %d (got %d x %d)", HALO << 4, H, W);
  CRDR_REQUIRE(quant >= 0 && quant <= 2 && !(quant && with_maps), "msssim_fwd: quant %d (no gradient through the truncation)", quant);
  Geometry g;
  geometry(N, H, W, with_maps != 0, g);
  CRDR_REQUIRE(state_bytes >= g.total * sizeof(float), "msssim_fwd: state buffer too small");
  hipStream_t st = as_stream(s);
  MsFwdArgs a;
  window(a.g);
  a.c1 = (0.01f * data_range) * (0.01f * data_range);
  a.c2 = (0.03f * data_range) * (0.03f * data_range);
  a.C = C;
  MsFinalArgs f;
  for (int l = 0; l < MS_LEVELS; ++l) {
    const bool last = l == MS_LEVELS - 1;
    a.x = l ? state + g.img[l] : x;
    a.y = l ? state + g.img[l] + (size_t)N * g.H[l] * g.W[l] * 4 : y;
    a.ldx = a.ldy = 4;
    a.H = g.H[l];
    a.W = g.W[l];
    a.quant = l ? 0 : quant;   // the pooled images already hold quantised values
    a.last = last;
    a.px = last ? nullptr : state + g.img[l + 1];
    a.py = last ? nullptr : a.px + (size_t)N * g.H[l + 1] * g.W[l + 1] * 4;
    a.PH = last ? 0 : g.H[l + 1];
    a.PW = last ? 0 : g.W[l + 1];
    a.padh = g.H[l] % 2;
    a.padw = g.W[l] % 2;
    a.maps = with_maps ? state + g.maps[l] : nullptr;
    a.part = state + g.part[l];
    hipLaunchKernelGGL(msssim_level_fwd, dim3(g.gx[l], g.gy[l], N), dim3(256), 0, st, a);
    CRDR_CHECK_LAUNCH("msssim_level_fwd");
    f.part[l] = a.part;
    f.tiles[l] = g.gx[l] * g.gy[l];
    f.count[l] = (float)(g.H[l] - HALO) * (float)(g.W[l] - HALO);
    f.w[l] = MS_WEIGHTS[l];
  }
  f.stat = state + g.stat;
  f.out = out;
  f.N = N;
  f.C = C;
  hipLaunchKernelGGL(msssim_stats, dim3(MS_LEVELS * N), dim3(256), 0, st, f);
  CRDR_CHECK_LAUNCH("msssim_stats");
  hipLaunchKernelGGL(msssim_final, dim3(1), dim3(256), 0, st, f);
  CRDR_CHECK_LAUNCH("msssim_final");
  return 0;
}

extern "C" int crdr_msssim_bwd(const float* x, int ldx, const float* y, int ldy, int N, int H, int W, int C, const float* state,
                               const float* gout, float* dx, int lddx, float* dy, int lddy, void* ws, size_t ws_bytes,
                               crdr_stream_t s) {
  CRDR_REQUIRE(x && y && state && gout && ws && (dx || dy), "msssim_bwd: null pointer");
  CRDR_REQUIRE(N >= 1 && C >= 1 && C <= 4 && ldx == 4 && ldy == 4 && (!dx || lddx == 4) && (!dy || lddy == 4) && aligned16(x) &&
                   aligned16(y) && aligned16(state) && aligned16(ws) && (!dx || aligned16(dx)) && (!dy || aligned16(dy)),
               "msssim_bwd: NHWC images of <= 4 channels with a 16-byte aligned pixel stride of 4");
  CRDR_REQUIRE(std::min(H, W) > HALO << 4, "msssim_bwd: image size should be larger than %d", HALO << 4);
  Geometry g;
  geometry(N, H, W, true, g);
  CRDR_REQUIRE(ws_bytes >= g.grad_total * sizeof(float), "msssim_bwd: workspace too small");
  float* gw = static_cast<float*>(ws);
  hipStream_t st = as_stream(s);
  MsBwdArgs a;
  window(a.g);
  a.C = C;
  a.N = N;
  a.stat = state + g.stat;
  a.gout = gout;
  for (int l = MS_LEVELS - 1; l >= 0; --l) {
    const size_t npix = (size_t)N * g.H[l] * g.W[l] * 4;
    const bool last = l == MS_LEVELS - 1;
    a.x = l ? state + g.img[l] : x;
    a.y = l ? state + g.img[l] + npix : y;
    a.ldx = a.ldy = 4;
    a.H = g.H[l];
    a.W = g.W[l];
    a.level = l;
    a.maps = state + g.maps[l];
    a.w = MS_WEIGHTS[l];
    a.denom = (float)N * (float)C * (float)(g.H[l] - HALO) * (float)(g.W[l] - HALO);
    const size_t nnext = last ? 0 : (size_t)N * g.H[l + 1] * g.W[l + 1] * 4;
    a.dxp = last || !dx ? nullptr : gw + g.grad[l + 1];
    a.dyp = last || !dy ? nullptr : gw + g.grad[l + 1] + nnext;
    a.PH = last ? 0 : g.H[l + 1];
    a.PW = last ? 0 : g.W[l + 1];
    a.padh = g.H[l] % 2;
    a.padw = g.W[l] % 2;
    a.dx = !dx ? nullptr : l ? gw + g.grad[l] : dx;
    a.dy = !dy ? nullptr : l ? gw + g.grad[l] + npix : dy;
    a.lddx = l ? 4 : lddx;
    a.lddy = l ? 4 : lddy;
    hipLaunchKernelGGL(msssim_level_bwd, dim3(cdiv(g.W[l], T), cdiv(g.H[l], T), N), dim3(256), 0, st, a);
    CRDR_CHECK_LAUNCH("msssim_level_bwd");
  }
  return 0;
}

}  // namespace crdr
