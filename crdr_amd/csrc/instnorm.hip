// InstanceNorm (moments per (image, channel) over the H x W plane, nn.InstanceNorm2d without running statistics): the norm of the reference's
// rate-aware discriminators (src/models/discriminator/multirate_clic21_gvae_discriminator.py:12-24, norm_type IN) with the LeakyReLU that
// follows it fused.
//
// Tensors are NHWC, so the moments are COLUMN sums across pixels -- the opposite of ChannelNorm (chnorm.hip), whose row lives in one lane
// group.  A workgroup of 256 threads owns one slab of IN_SLAB pixels of one image and one tile of QT channel quads (QT = the power of two
// that covers min(C / 4, 64)): thread t holds quad t % QT and walks the pixels t / QT, t / QT + 256 / QT, ... of the slab, so that a
// wave-instruction reads whole contiguous runs of the pixel rows (1 KiB per wave at C >= 256).  The 256 / QT row partials of a quad meet
// in LDS in a fixed tree.
//
//   forward   in_stats_kernel    per slab: the slab's mean, then (second walk over the slab, which the first left in L2) the sum of the
//                                squares CENTRED on that mean, and the mean's own rounding taken out -> part[n][slab][2][C] = (mean, M2)
//             in_merge_kernel    one thread per (n, c) merges the slabs in slab order with Chan's formula -> stats[n][2][C] = (mu, rstd)
//             in_apply_kernel    y = act(gamma (x - mu) rstd + beta): x read once, y written once
//   backward  in_bsum_kernel     per slab: sum dz xhat and sum dz (z and xhat recomputed by in_xhat / in_z, the forward's own expressions,
//                                so the activation mask is the forward's) -> part[n][slab][2][C]
//             in_bmerge_kernel   one thread per (n, c) adds the slabs in slab order -> sums[n][2][C]
//             in_bparam_kernel   dgamma[c] += sum_n sums[n][0][c], dbeta[c] += sum_n sums[n][1][c], n in order (only with a gradient slot)
//             in_bapply_kernel   dx = rstd (gh - mean gh - xhat mean(gh xhat)), gh = gamma dz
// No float atomics: which thread adds which element and the order in which partials meet follow from the descriptor alone.
#include <algorithm>

#include "common.hpp"

namespace crdr {

constexpr int IN_THREADS = 256;
constexpr int IN_SLAB = 512;   // pixels of one image per workgroup

struct InArgs {
  const float *x, *gamma, *beta, *stats, *dy, *sums;
  float *y, *dx, *part;
  int64_t HW;
  int C, Q, lq, ntile, nslab, ldx, ldy, lddy, lddx, act;
  float slope, inv_hw;
};

// where a thread works: image n, first pixel p0 and pixel count cnt of its slab, channel quad q (on: q exists), row r of R
struct InWhere {
  int64_t n, p0;
  int sl, cnt, q, r, R;
  bool on;
};

// pixels in slab sl of a plane of HW (the last slab is ragged)
__device__ __forceinline__ int in_slab_count(int64_t HW, int sl) {
  const int64_t left = HW - (int64_t)sl * IN_SLAB;
  return left < IN_SLAB ? (int)left : IN_SLAB;
}

__device__ __forceinline__ InWhere in_where(const InArgs& a) {
  InWhere w;
  const int64_t b = blockIdx.x;
  const int tile = (int)(b % a.ntile);
  w.sl = (int)((b / a.ntile) % a.nslab);
  w.n = b / ((int64_t)a.ntile * a.nslab);
  w.p0 = (int64_t)w.sl * IN_SLAB;
  w.cnt = in_slab_count(a.HW, w.sl);
  w.q = (tile << a.lq) + (threadIdx.x & ((1 << a.lq) - 1));
  w.r = threadIdx.x >> a.lq;
  w.R = IN_THREADS >> a.lq;
  w.on = w.q < a.Q;
  return w;
}

// the sum over the R rows of every quad of the tile, the same bits in every thread of a quad's column; fixed tree, whatever the values
__device__ __forceinline__ f32x4 in_block_sum(f32x4 v, f32x4* red, const InWhere& w, int lq) {
  red[threadIdx.x] = v;   // threadIdx.x == r * QT + quad
  __syncthreads();
  for (int s = w.R >> 1; s >= 1; s >>= 1) {
    if (w.r < s) red[threadIdx.x] += red[threadIdx.x + (s << lq)];
    __syncthreads();
  }
  const f32x4 t = red[threadIdx.x & ((1 << lq) - 1)];
  __syncthreads();   // red is reused by the next sum
  return t;
}

__device__ __forceinline__ f32x4 in_ld(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// the ONE expression of xhat and of z, shared by forward and backward: (x - mu) * rstd cannot contract, the affine step is an explicit fma
__device__ __forceinline__ float in_xhat(float x, float mu, float rstd) { return (x - mu) * rstd; }
__device__ __forceinline__ float in_z(float xhat, float g, float b) { return __fmaf_rn(g, xhat, b); }

__global__ __launch_bounds__(IN_THREADS) void in_stats_kernel(const InArgs a) {
  __shared__ f32x4 red[IN_THREADS];
  const InWhere w = in_where(a);
  const float* xp = a.x + (w.n * a.HW + w.p0) * a.ldx + 4 * w.q;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (w.on) {
#pragma unroll 4
    for (int i = w.r; i < w.cnt; i += w.R) s += in_ld(xp + (int64_t)i * a.ldx);
  }
  const float inv_cnt = 1.f / (float)w.cnt;
  f32x4 mean = in_block_sum(s, red, w, a.lq) * inv_cnt;
  // second walk: squares centred on that mean, and the sum of the centred values themselves -- what the rounding of the first walk's long sum
  // left in the mean (up to a few ulp under a common offset), taken out of both moments below
  f32x4 m2 = {0.f, 0.f, 0.f, 0.f}, sd = {0.f, 0.f, 0.f, 0.f};
  if (w.on) {
#pragma unroll 4
    for (int i = w.r; i < w.cnt; i += w.R) {
      const f32x4 d = in_ld(xp + (int64_t)i * a.ldx) - mean;
      sd += d;
      m2 += d * d;
    }
  }
  sd = in_block_sum(sd, red, w, a.lq);
  m2 = in_block_sum(m2, red, w, a.lq);
  const f32x4 corr = sd * inv_cnt;
  mean += corr;
  m2 -= sd * corr;   // sum (x - mean - corr)^2 = sum (x - mean)^2 - cnt corr^2
#pragma unroll
  for (int e = 0; e < 4; ++e) m2[e] = fmaxf(m2[e], 0.f);   // (a constant plane: the difference of two roundings may come out below zero)
  if (w.on && w.r == 0) {
    float* o = a.part + (w.n * a.nslab + w.sl) * 2 * a.C + 4 * w.q;
    *reinterpret_cast<f32x4*>(o) = mean;
    *reinterpret_cast<f32x4*>(o + a.C) = m2;
  }
}

// Chan, Golub, LeVeque: (na, mean, M2) + (nb, mb, Mb) -> (na + nb, mean + d nb / n, M2 + Mb + d^2 na nb / n), d = mb - mean; slabs in order
__global__ __launch_bounds__(IN_THREADS) void in_merge_kernel(const float* part, int64_t NC, int C, int nslab, int64_t HW, float eps, float* stats) {
  const int64_t i = (int64_t)blockIdx.x * IN_THREADS + threadIdx.x;
  if (i >= NC) return;
  const int64_t n = i / C;
  const int c = (int)(i % C);
  const float* p = part + n * nslab * 2 * C + c;
  float mean = p[0], m2 = p[C], na = (float)in_slab_count(HW, 0);
  for (int s = 1; s < nslab; ++s) {
    const float nb = (float)in_slab_count(HW, s);
    const float mb = p[(int64_t)s * 2 * C], Mb = p[(int64_t)s * 2 * C + C];
    const float d = mb - mean, nt = na + nb;
    mean += d * (nb / nt);
    m2 += Mb + d * d * (na * nb / nt);
    na = nt;
  }
  stats[n * 2 * C + c] = mean;
  stats[n * 2 * C + C + c] = rsqrtf(m2 / (float)HW + eps);   // biased variance (nn.InstanceNorm2d)
}

__global__ __launch_bounds__(IN_THREADS) void in_apply_kernel(const InArgs a) {
  const InWhere w = in_where(a);
  if (!w.on) return;
  const float* st = a.stats + w.n * 2 * a.C + 4 * w.q;
  const f32x4 mu = in_ld(st), rstd = in_ld(st + a.C);
  const f32x4 g = a.gamma ? in_ld(a.gamma + 4 * w.q) : f32x4{1.f, 1.f, 1.f, 1.f};
  const f32x4 b = a.beta ? in_ld(a.beta + 4 * w.q) : f32x4{0.f, 0.f, 0.f, 0.f};
  const float* xp = a.x + (w.n * a.HW + w.p0) * a.ldx + 4 * w.q;
  float* yp = a.y + (w.n * a.HW + w.p0) * a.ldy + 4 * w.q;
#pragma unroll 4
  for (int i = w.r; i < w.cnt; i += w.R) {
    const f32x4 v = in_ld(xp + (int64_t)i * a.ldx);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float z = in_z(in_xhat(v[e], mu[e], rstd[e]), g[e], b[e]);
      o[e] = a.act == 1 ? (z > 0.f ? z : 0.f) : a.act == 2 ? (z > 0.f ? z : a.slope * z) : z;
    }
    *reinterpret_cast<f32x4*>(yp + (int64_t)i * a.ldy) = o;
  }
}

// dz = act'(z) dy with z recomputed
__device__ __forceinline__ float in_dz(float z, float dy, int act, float slope) {
  return act == 1 ? (z > 0.f ? dy : 0.f) : act == 2 ? (z > 0.f ? dy : slope * dy) : dy;
}

__global__ __launch_bounds__(IN_THREADS) void in_bsum_kernel(const InArgs a) {
  __shared__ f32x4 red[IN_THREADS];
  const InWhere w = in_where(a);
  f32x4 sx = {0.f, 0.f, 0.f, 0.f}, sd = {0.f, 0.f, 0.f, 0.f};
  if (w.on) {
    const float* st = a.stats + w.n * 2 * a.C + 4 * w.q;
    const f32x4 mu = in_ld(st), rstd = in_ld(st + a.C);
    const f32x4 g = a.gamma ? in_ld(a.gamma + 4 * w.q) : f32x4{1.f, 1.f, 1.f, 1.f};
    const f32x4 b = a.beta ? in_ld(a.beta + 4 * w.q) : f32x4{0.f, 0.f, 0.f, 0.f};
    const float* xp = a.x + (w.n * a.HW + w.p0) * a.ldx + 4 * w.q;
    const float* dp = a.dy + (w.n * a.HW + w.p0) * a.lddy + 4 * w.q;
#pragma unroll 4
    for (int i = w.r; i < w.cnt; i += w.R) {
      const f32x4 v = in_ld(xp + (int64_t)i * a.ldx), dyv = in_ld(dp + (int64_t)i * a.lddy);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = in_xhat(v[e], mu[e], rstd[e]);
        const float dz = in_dz(in_z(xh, g[e], b[e]), dyv[e], a.act, a.slope);
        sx[e] += dz * xh;
        sd[e] += dz;
      }
    }
  }
  sx = in_block_sum(sx, red, w, a.lq);
  sd = in_block_sum(sd, red, w, a.lq);
  if (w.on && w.r == 0) {
    float* o = a.part + (w.n * a.nslab + w.sl) * 2 * a.C + 4 * w.q;
    *reinterpret_cast<f32x4*>(o) = sx;
    *reinterpret_cast<f32x4*>(o + a.C) = sd;
  }
}

// sums[n][which][c] = sum over the slabs, in slab order, of part[n][slab][which][c]
__global__ __launch_bounds__(IN_THREADS) void in_bmerge_kernel(const float* part, int64_t N2C, int C, int nslab, float* sums) {
  const int64_t i = (int64_t)blockIdx.x * IN_THREADS + threadIdx.x;
  if (i >= N2C) return;
  const int64_t n = i / (2 * C);
  const int j = (int)(i % (2 * C));
  const float* p = part + n * nslab * 2 * C + j;
  float s = 0.f;
  for (int sl = 0; sl < nslab; ++sl) s += p[(int64_t)sl * 2 * C];
  sums[i] = s;
}

// dgamma[c] += sum_n sums[n][0][c], dbeta[c] += sum_n sums[n][1][c], images in order
__global__ __launch_bounds__(IN_THREADS) void in_bparam_kernel(const float* sums, int N, int C, float* dgamma, float* dbeta) {
  const int j = blockIdx.x * IN_THREADS + threadIdx.x;
  if (j >= 2 * C) return;
  float* dst = j < C ? dgamma : dbeta;
  if (!dst) return;
  float s = 0.f;
  for (int n = 0; n < N; ++n) s += sums[(int64_t)n * 2 * C + j];
  dst[j < C ? j : j - C] += s;
}

__global__ __launch_bounds__(IN_THREADS) void in_bapply_kernel(const InArgs a) {
  const InWhere w = in_where(a);
  if (!w.on) return;
  const float* st = a.stats + w.n * 2 * a.C + 4 * w.q;
  const f32x4 mu = in_ld(st), rstd = in_ld(st + a.C);
  const f32x4 g = a.gamma ? in_ld(a.gamma + 4 * w.q) : f32x4{1.f, 1.f, 1.f, 1.f};
  const f32x4 b = a.beta ? in_ld(a.beta + 4 * w.q) : f32x4{0.f, 0.f, 0.f, 0.f};
  const float* sm = a.sums + w.n * 2 * a.C + 4 * w.q;
  const f32x4 mgx = g * in_ld(sm) * a.inv_hw;          // mean_hw(gh xhat)
  const f32x4 mg = g * in_ld(sm + a.C) * a.inv_hw;     // mean_hw gh
  const float* xp = a.x + (w.n * a.HW + w.p0) * a.ldx + 4 * w.q;
  const float* dp = a.dy + (w.n * a.HW + w.p0) * a.lddy + 4 * w.q;
  float* op = a.dx + (w.n * a.HW + w.p0) * a.lddx + 4 * w.q;
#pragma unroll 4
  for (int i = w.r; i < w.cnt; i += w.R) {
    const f32x4 v = in_ld(xp + (int64_t)i * a.ldx), dyv = in_ld(dp + (int64_t)i * a.lddy);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = in_xhat(v[e], mu[e], rstd[e]);
      const float dz = in_dz(in_z(xh, g[e], b[e]), dyv[e], a.act, a.slope);
      o[e] = rstd[e] * (g[e] * dz - mg[e] - xh * mgx[e]);
    }
    *reinterpret_cast<f32x4*>(op + (int64_t)i * a.lddx) = o;
  }
}

namespace {

constexpr int IN_MAX_C = 1024;

bool in_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// slabs per image, channel tiles, log2 of the tile's quads, workgroups
struct InShape {
  int nslab, ntile, lq;
  int64_t blocks;
};

InShape in_shape(const crdr_instance_norm_desc* d) {
  InShape s;
  const int Q = d->C / 4;
  s.lq = 0;
  while ((1 << s.lq) < std::min(Q, 64)) ++s.lq;
  s.ntile = cdiv(Q, 1 << s.lq);
  s.nslab = (int)cdiv64(d->HW, IN_SLAB);
  s.blocks = (int64_t)d->N * s.nslab * s.ntile;
  return s;
}

size_t in_part_floats(const crdr_instance_norm_desc* d, const InShape& s) { return (size_t)d->N * s.nslab * 2 * d->C; }
size_t in_ws_bytes(const crdr_instance_norm_desc* d, const InShape& s) {
  return (in_part_floats(d, s) + (size_t)d->N * 2 * d->C) * sizeof(float);   // slab partials, then the backward's sums[n][2][C]
}

int in_check(const crdr_instance_norm_desc* d, const char* what) {
  CRDR_REQUIRE(d, "%s: null descriptor", what);
  CRDR_REQUIRE(d->N >= 0 && d->HW >= 0 && d->HW < ((int64_t)1 << 31), "%s: N = %d, HW = %lld", what, d->N, (long long)d->HW);
  CRDR_REQUIRE(d->HW >= 2, "%s: more than one value per channel is needed (H W = %lld); torch refuses it in training mode too", what,
               (long long)d->HW);
  CRDR_REQUIRE(d->C >= 4 && d->C % 4 == 0 && d->C <= IN_MAX_C, "%s: the channel count must be a multiple of 4 in [4, %d] (got %d)", what, IN_MAX_C,
               d->C);
  CRDR_REQUIRE(d->ldx % 4 == 0 && d->ldx >= d->C, "%s: ldx = %d (C = %d)", what, d->ldx, d->C);
  CRDR_REQUIRE(d->act >= 0 && d->act <= 2, "%s: act = %d (0 none, 1 ReLU, 2 LeakyReLU)", what, d->act);
  CRDR_REQUIRE(in_shape(d).blocks < ((int64_t)1 << 31), "%s: tensor too large", what);
  return 0;
}

InArgs in_args(const crdr_instance_norm_desc* d, const InShape& s) {
  InArgs a = {};
  a.HW = d->HW; a.C = d->C; a.Q = d->C / 4; a.lq = s.lq; a.ntile = s.ntile; a.nslab = s.nslab; a.ldx = d->ldx; a.ldy = d->ldy; a.act = d->act;
  a.slope = d->slope; a.inv_hw = 1.f / (float)d->HW;
  return a;
}

}  // namespace
}  // namespace crdr

using namespace crdr;

extern "C" size_t crdr_instance_norm_workspace(const crdr_instance_norm_desc* d) {
  if (in_check(d, "instance_norm_workspace") || d->N == 0) return 0;
  return in_ws_bytes(d, in_shape(d));
}

extern "C" int crdr_instance_norm_fwd(const crdr_instance_norm_desc* d, const float* x, const float* gamma, const float* beta, float* y, float* stats,
                                      void* ws, size_t ws_bytes, crdr_stream_t s) {
  if (int rc = in_check(d, "instance_norm_fwd")) return rc;
  CRDR_REQUIRE(x && y && stats, "instance_norm_fwd: null pointer");
  CRDR_REQUIRE(d->ldy % 4 == 0 && d->ldy >= d->C, "instance_norm_fwd: ldy = %d (C = %d)", d->ldy, d->C);
  CRDR_REQUIRE(in_aligned16(x) && in_aligned16(y) && in_aligned16(gamma) && in_aligned16(beta) && in_aligned16(stats) && in_aligned16(ws),
               "instance_norm_fwd: operands must be 16-byte aligned");
  if (d->N == 0) return 0;
  const InShape sh = in_shape(d);
  CRDR_REQUIRE(ws && ws_bytes >= in_ws_bytes(d, sh), "instance_norm_fwd: workspace too small (%zu < %zu)", ws_bytes, in_ws_bytes(d, sh));
  InArgs a = in_args(d, sh);
  a.x = x; a.gamma = gamma; a.beta = beta; a.y = y; a.stats = stats; a.part = (float*)ws;
  const int64_t NC = (int64_t)d->N * d->C;
  hipLaunchKernelGGL(in_stats_kernel, dim3((unsigned)sh.blocks), dim3(IN_THREADS), 0, as_stream(s), a);
  CRDR_CHECK_LAUNCH("instance_norm_stats");
  hipLaunchKernelGGL(in_merge_kernel, dim3((unsigned)cdiv64(NC, IN_THREADS)), dim3(IN_THREADS), 0, as_stream(s), (const float*)ws, NC, d->C, sh.nslab,
                     d->HW, d->eps, stats);
  CRDR_CHECK_LAUNCH("instance_norm_merge");
  hipLaunchKernelGGL(in_apply_kernel, dim3((unsigned)sh.blocks), dim3(IN_THREADS), 0, as_stream(s), a);
  CRDR_CHECK_LAUNCH("instance_norm_apply");
  return 0;
}

extern "C" int crdr_instance_norm_bwd(const crdr_instance_norm_desc* d, const float* x, const float* gamma, const float* beta, const float* stats,
                                      const float* dy, int lddy, float* dx, int lddx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                                      crdr_stream_t s) {
  if (int rc = in_check(d, "instance_norm_bwd")) return rc;
  CRDR_REQUIRE(x && stats && dy && dx, "instance_norm_bwd: null pointer");
  CRDR_REQUIRE(lddy % 4 == 0 && lddy >= d->C && lddx % 4 == 0 && lddx >= d->C, "instance_norm_bwd: lddy = %d, lddx = %d (C = %d)", lddy, lddx, d->C);
  CRDR_REQUIRE(in_aligned16(x) && in_aligned16(dy) && in_aligned16(dx) && in_aligned16(gamma) && in_aligned16(beta) && in_aligned16(stats) &&
                   in_aligned16(ws),
               "instance_norm_bwd: operands must be 16-byte aligned");
  CRDR_REQUIRE((reinterpret_cast<uintptr_t>(dgamma) & 3) == 0 && (reinterpret_cast<uintptr_t>(dbeta) & 3) == 0,
               "instance_norm_bwd: gradient slots must be float aligned");
  if (d->N == 0) return 0;
  const InShape sh = in_shape(d);
  CRDR_REQUIRE(ws && ws_bytes >= in_ws_bytes(d, sh), "instance_norm_bwd: workspace too small (%zu < %zu)", ws_bytes, in_ws_bytes(d, sh));
  InArgs a = in_args(d, sh);
  float* sums = (float*)ws + in_part_floats(d, sh);
  a.x = x; a.gamma = gamma; a.beta = beta; a.stats = stats; a.dy = dy; a.lddy = lddy; a.dx = dx; a.lddx = lddx; a.part = (float*)ws; a.sums = sums;
  const int64_t N2C = (int64_t)d->N * 2 * d->C;
  hipLaunchKernelGGL(in_bsum_kernel, dim3((unsigned)sh.blocks), dim3(IN_THREADS), 0, as_stream(s), a);
  CRDR_CHECK_LAUNCH("instance_norm_bsum");
  hipLaunchKernelGGL(in_bmerge_kernel, dim3((unsigned)cdiv64(N2C, IN_THREADS)), dim3(IN_THREADS), 0, as_stream(s), (const float*)ws, N2C, d->C,
                     sh.nslab, sums);
  CRDR_CHECK_LAUNCH("instance_norm_bmerge");
  if (dgamma || dbeta) {
    hipLaunchKernelGGL(in_bparam_kernel, dim3(cdiv(2 * d->C, IN_THREADS)), dim3(IN_THREADS), 0, as_stream(s), (const float*)sums, d->N, d->C, dgamma,
                       dbeta);
    CRDR_CHECK_LAUNCH("instance_norm_bparam");
  }
  hipLaunchKernelGGL(in_bapply_kernel, dim3((unsigned)sh.blocks), dim3(IN_THREADS), 0, as_stream(s), a);
  CRDR_CHECK_LAUNCH("instance_norm_bapply");
  return 0;
}
