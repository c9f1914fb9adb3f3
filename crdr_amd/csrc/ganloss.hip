// GAN objectives on discriminator logits (crdr_hip.h, "losses": crdr_gan_loss_fwd / crdr_gan_loss_bwd).
//
//   x_i = p_i - r_i,  r_i = q_i (paired) | mean(q) (centred: RaGAN) | 0 (no q)
//   kind 0: max(x,0) - x t + log1p(exp(-|x|))   kind 1: max(1 - sgn x, 0)   kind 2: -x
//   out[0] = sum_i m_i l(x_i)
//
// Every sum here is two-stage like the reductions of eltwise.hip: a capped grid of 256-thread blocks, each thread adds its
// grid-stride terms one after the other, the 64 lanes of a wave combine in a shuffle tree, the 4 wave sums in a fixed order, one block
// then sums the block partials the same way.  No atomics: the order of the additions depends on (n, nq) alone, so two calls on the
// same data give the same bits.  mean(q) is reduced first and stays in device memory (stats[0]); the loss pass and the backward read
// it from there, so nothing here synchronises with the host and a captured graph replays with the data it finds.
// Element offsets are 64-bit throughout.
#include <algorithm>

#include "common.hpp"

using namespace crdr;

namespace {

enum { GL_BCE = 0, GL_HINGE_D = 1, GL_HINGE_G = 2 };
enum { GL_NOQ = 0, GL_PAIRED = 1, GL_CENTRED = 2 };

__device__ __forceinline__ float gl_block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) red[w] = v;
  __syncthreads();
  const float r = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return r;
}

// grid of a sum over n elements: one block per 1024 elements, at most 1024 blocks (the second stage is one block of 256 threads)
int gl_blocks(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(cdiv64(n, 1024), 1), 1024); }

template <int KIND>
__device__ __forceinline__ float gl_loss(float x, float target, float sgn) {
  if (KIND == GL_BCE) return fmaxf(x, 0.f) - x * target + log1pf(expf(-fabsf(x)));
  if (KIND == GL_HINGE_D) return fmaxf(1.f - sgn * x, 0.f);
  return -x;
}
// dl/dx; the hinge takes torch's relu'(0) = 0
template <int KIND>
__device__ __forceinline__ float gl_slope(float x, float target, float sgn) {
  if (KIND == GL_BCE) return 1.f / (1.f + expf(-x)) - target;
  if (KIND == GL_HINGE_D) return (1.f - sgn * x > 0.f) ? -sgn : 0.f;
  return -1.f;
}

__global__ __launch_bounds__(256) void gl_sum_kernel(const float* __restrict__ q, int64_t nq, float* __restrict__ partial) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < nq; e += gridDim.x * 256ll) s += q[e];
  s = gl_block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// total[0] = sum of the nb partials; scaled[0] = that sum / denom (each when asked for)
__global__ __launch_bounds__(256) void gl_final_kernel(const float* __restrict__ partial, int nb, float* __restrict__ total,
                                                       float* __restrict__ scaled, float denom) {
  __shared__ float red[4];
  float s = 0.f;
  for (int e = threadIdx.x; e < nb; e += 256) s += partial[e];
  s = gl_block_sum(s, red);
  if (threadIdx.x == 0) {
    if (total) total[0] = s;
    if (scaled) scaled[0] = s / denom;
  }
}

template <int KIND, int FORM>
__global__ __launch_bounds__(256) void gl_fwd_kernel(const float* __restrict__ p, const float* __restrict__ q,
                                                     const float* __restrict__ mask, const float* __restrict__ stats, int64_t n,
                                                     float target, float sgn, float* __restrict__ partial) {
  __shared__ float red[4];
  const float mean = FORM == GL_CENTRED ? stats[0] : 0.f;
  float s = 0.f;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < n; e += gridDim.x * 256ll) {
    const float x = FORM == GL_PAIRED ? p[e] - q[e] : FORM == GL_CENTRED ? p[e] - mean : p[e];
    const float l = gl_loss<KIND>(x, target, sgn);
    s += mask ? mask[e] * l : l;
  }
  s = gl_block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// dp_i = k m_i l'(x_i); paired: dq_i = -dp_i; centred: the block sums of dp_i go to `partial` (when given) for dq = -(sum dp) / nq
template <int KIND, int FORM>
__global__ __launch_bounds__(256) void gl_bwd_kernel(const float* __restrict__ p, const float* __restrict__ q,
                                                     const float* __restrict__ mask, const float* __restrict__ stats, int64_t n,
                                                     float target, float sgn, const float* __restrict__ g, float gscale,
                                                     float* __restrict__ dp, float* __restrict__ dq, float* __restrict__ partial) {
  __shared__ float red[4];
  const float k = gscale * g[0];
  const float mean = FORM == GL_CENTRED ? stats[0] : 0.f;
  float s = 0.f;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < n; e += gridDim.x * 256ll) {
    const float x = FORM == GL_PAIRED ? p[e] - q[e] : FORM == GL_CENTRED ? p[e] - mean : p[e];
    const float km = mask ? k * mask[e] : k;
    const float d = km * gl_slope<KIND>(x, target, sgn);
    if (dp) dp[e] = d;
    if (FORM == GL_PAIRED && dq) dq[e] = -d;
    s += d;
  }
  if (FORM == GL_CENTRED && partial) {   // (uniform over the grid: every thread of every block reaches the barriers)
    s = gl_block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
  }
}

// dq_j = -(sum_i dp_i) / nq for every j
__global__ __launch_bounds__(256) void gl_fill_kernel(const float* __restrict__ total, float nqf, float* __restrict__ dq, int64_t nq) {
  const float v = -(total[0] / nqf);
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < nq; e += gridDim.x * 256ll) dq[e] = v;
}

struct GlPlan {
  int form, nb, nbq;
};

bool gl_aligned(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 3) == 0; }

// the checks both directions share; -> 0, or -1 with the error set
int gl_plan(const crdr_gan_loss_desc* d, const float* p, const float* q, const float* mask, const void* ws, size_t ws_bytes,
            const char* what, GlPlan* plan) {
  CRDR_REQUIRE(d && p, "%s: null desc / p", what);
  CRDR_REQUIRE(d->n >= 1, "%s: n = %lld", what, (long long)d->n);
  CRDR_REQUIRE(d->kind >= GL_BCE && d->kind <= GL_HINGE_G, "%s: kind %d (0 BCE, 1 hinge D, 2 hinge G)", what, d->kind);
  CRDR_REQUIRE(d->kind != GL_HINGE_D || d->sgn == 1.f || d->sgn == -1.f, "%s: hinge sgn %f (+1 real, -1 fake)", what, d->sgn);
  CRDR_REQUIRE(d->center == 0 || d->center == 1, "%s: center %d", what, d->center);
  CRDR_REQUIRE(!d->center || q, "%s: the centred form needs q", what);
  CRDR_REQUIRE(!q || (d->center ? d->nq >= 1 : d->nq == d->n), "%s: q has %lld elements for n = %lld (center %d)", what,
               (long long)d->nq, (long long)d->n, d->center);
  CRDR_REQUIRE(gl_aligned(p) && gl_aligned(q) && gl_aligned(mask) && gl_aligned(ws), "%s: misaligned pointer", what);
  plan->form = !q ? GL_NOQ : d->center ? GL_CENTRED : GL_PAIRED;
  plan->nb = gl_blocks(d->n);
  plan->nbq = plan->form == GL_CENTRED ? gl_blocks(d->nq) : 0;
  CRDR_REQUIRE(ws && ws_bytes >= crdr_gan_loss_workspace(d->n, q ? d->nq : 0), "%s: workspace too small (%zu bytes)", what, ws_bytes);
  return 0;
}

template <int KIND>
void gl_launch_fwd(int form, int nb, hipStream_t st, const float* p, const float* q, const float* mask, const float* stats, int64_t n,
                   float target, float sgn, float* partial) {
  if (form == GL_NOQ) hipLaunchKernelGGL((gl_fwd_kernel<KIND, GL_NOQ>), dim3(nb), dim3(256), 0, st, p, q, mask, stats, n, target, sgn, partial);
  if (form == GL_PAIRED) hipLaunchKernelGGL((gl_fwd_kernel<KIND, GL_PAIRED>), dim3(nb), dim3(256), 0, st, p, q, mask, stats, n, target, sgn, partial);
  if (form == GL_CENTRED) hipLaunchKernelGGL((gl_fwd_kernel<KIND, GL_CENTRED>), dim3(nb), dim3(256), 0, st, p, q, mask, stats, n, target, sgn, partial);
}
template <int KIND>
void gl_launch_bwd(int form, int nb, hipStream_t st, const float* p, const float* q, const float* mask, const float* stats, int64_t n,
                   float target, float sgn, const float* g, float gscale, float* dp, float* dq, float* partial) {
  if (form == GL_NOQ) hipLaunchKernelGGL((gl_bwd_kernel<KIND, GL_NOQ>), dim3(nb), dim3(256), 0, st, p, q, mask, stats, n, target, sgn, g, gscale, dp, dq, partial);
  if (form == GL_PAIRED) hipLaunchKernelGGL((gl_bwd_kernel<KIND, GL_PAIRED>), dim3(nb), dim3(256), 0, st, p, q, mask, stats, n, target, sgn, g, gscale, dp, dq, partial);
  if (form == GL_CENTRED) hipLaunchKernelGGL((gl_bwd_kernel<KIND, GL_CENTRED>), dim3(nb), dim3(256), 0, st, p, q, mask, stats, n, target, sgn, g, gscale, dp, dq, partial);
}

}  // namespace

// [gl_blocks(n) partials of the sum over p][gl_blocks(nq) partials of the sum over q][1 total of the backward's sum dp]
extern "C" size_t crdr_gan_loss_workspace(int64_t n, int64_t nq) {
  return (size_t)(gl_blocks(n) + (nq > 0 ? gl_blocks(nq) : 0) + 1) * sizeof(float);
}

extern "C" int crdr_gan_loss_fwd(const crdr_gan_loss_desc* d, const float* p, const float* q, const float* mask, float* out,
                                 float* stats, void* ws, size_t ws_bytes, crdr_stream_t s) {
  GlPlan pl;
  if (int rc = gl_plan(d, p, q, mask, ws, ws_bytes, "gan_loss_fwd", &pl)) return rc;
  CRDR_REQUIRE(out && stats && gl_aligned(out) && gl_aligned(stats), "gan_loss_fwd: null or misaligned out / stats");
  hipStream_t st = as_stream(s);
  float* part = (float*)ws;
  float* partq = part + pl.nb;
  if (pl.form == GL_CENTRED) {   // stats = {mean(q), sum(q)}
    hipLaunchKernelGGL(gl_sum_kernel, dim3(pl.nbq), dim3(256), 0, st, q, d->nq, partq);
    hipLaunchKernelGGL(gl_final_kernel, dim3(1), dim3(256), 0, st, (const float*)partq, pl.nbq, stats + 1, stats, (float)d->nq);
    CRDR_CHECK_LAUNCH("gan_loss_fwd");
  }
  if (d->kind == GL_BCE) gl_launch_fwd<GL_BCE>(pl.form, pl.nb, st, p, q, mask, stats, d->n, d->target, d->sgn, part);
  if (d->kind == GL_HINGE_D) gl_launch_fwd<GL_HINGE_D>(pl.form, pl.nb, st, p, q, mask, stats, d->n, d->target, d->sgn, part);
  if (d->kind == GL_HINGE_G) gl_launch_fwd<GL_HINGE_G>(pl.form, pl.nb, st, p, q, mask, stats, d->n, d->target, d->sgn, part);
  CRDR_CHECK_LAUNCH("gan_loss_fwd");
  hipLaunchKernelGGL(gl_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, pl.nb, out, (float*)nullptr, 1.f);
  CRDR_CHECK_LAUNCH("gan_loss_fwd");
  return 0;
}

extern "C" int crdr_gan_loss_bwd(const crdr_gan_loss_desc* d, const float* p, const float* q, const float* mask, const float* stats,
                                 const float* g, float gscale, float* dp, float* dq, void* ws, size_t ws_bytes, crdr_stream_t s) {
  GlPlan pl;
  if (int rc = gl_plan(d, p, q, mask, ws, ws_bytes, "gan_loss_bwd", &pl)) return rc;
  CRDR_REQUIRE(g && stats && gl_aligned(g) && gl_aligned(stats), "gan_loss_bwd: null or misaligned g / stats");
  CRDR_REQUIRE(gl_aligned(dp) && gl_aligned(dq), "gan_loss_bwd: misaligned dp / dq");
  CRDR_REQUIRE(!dq || q, "gan_loss_bwd: dq without q");
  if (!dp && !dq) return 0;
  hipStream_t st = as_stream(s);
  float* part = (float*)ws;
  float* total = part + pl.nb + pl.nbq;
  float* psum = (pl.form == GL_CENTRED && dq) ? part : nullptr;
  if (d->kind == GL_BCE) gl_launch_bwd<GL_BCE>(pl.form, pl.nb, st, p, q, mask, stats, d->n, d->target, d->sgn, g, gscale, dp, dq, psum);
  if (d->kind == GL_HINGE_D) gl_launch_bwd<GL_HINGE_D>(pl.form, pl.nb, st, p, q, mask, stats, d->n, d->target, d->sgn, g, gscale, dp, dq, psum);
  if (d->kind == GL_HINGE_G) gl_launch_bwd<GL_HINGE_G>(pl.form, pl.nb, st, p, q, mask, stats, d->n, d->target, d->sgn, g, gscale, dp, dq, psum);
  CRDR_CHECK_LAUNCH("gan_loss_bwd");
  if (psum) {
    hipLaunchKernelGGL(gl_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, pl.nb, total, (float*)nullptr, 1.f);
    hipLaunchKernelGGL(gl_fill_kernel, dim3(gl_blocks(d->nq)), dim3(256), 0, st, (const float*)total, (float)d->nq, dq, d->nq);
    CRDR_CHECK_LAUNCH("gan_loss_bwd");
  }
  return 0;
}
