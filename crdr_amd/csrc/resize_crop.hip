// PilRandomResize -> RandomCrop(pad_if_needed, reflect) -> HFlip -> ToTensor -> Normalize(0.5, 0.5) (data_transform.py:19-73) over the
// device image pool: one launch cuts a whole batch of crops out of images that are never resized as a whole.  Only the crop window of
// the resized image is computed, with the integer arithmetic of PIL's 8-bit resampler (Resample.c: horizontal pass, uint8 in between,
// vertical pass; 22-bit fixed-point coefficients, 32-bit accumulators), so a crop is bit-equal to PIL's.
//
// The host (crdr_amd/dataset/device_pipeline.py) builds, per sample and per axis, a table over the crop positions: position j reads the
// source samples lo[j] .. lo[j] + cnt[j] - 1 with the weights k[0 .. cnt[j]) [j].  Reflect padding of the resized image and the flip are
// already resolved into the order of the entries, and a pass PIL skips (output length == input length) is cnt = 1, k = 2^22, which
// reproduces the byte.  So this file holds no filter, no reflect and no flip code:
//   mid[y][c][ch] = clip8((2^21 + sum_i kh[i][c] * src[y][xlo[c] + i][ch]) >> 22)
//   b[r][c][ch]   = clip8((2^21 + sum_j kv[j][r] * mid[ylo[r] + j][c][ch]) >> 22)
//   out[r][c][ch] = ((float)b / 255.0f - 0.5f) / 0.5f          (the expression of crop_flip_normalize_kernel), lane 3 = 0
//
// A workgroup of 256 threads owns one sample and a tile of 32 output rows x 32 output columns.  It copies the tile's slices of the two
// tables to LDS, takes ymin = min ylo and ymax = max (ylo + cnt) over the tile's rows, filters the source rows [ymin, ymax) horizontally
// for the tile's 32 columns into LDS (phase one, one packed 4-byte pixel per item), and filters those vertically (phase two, one
// 16-byte store per lane, 32 consecutive pixels = 512 B per half wave).  An intermediate byte is computed once per tile; neighbouring row
// tiles recompute the 2 x support rows they share.  Where rows are reflected the ylo of a tile are not monotonic: the reflected rows fold
// back onto rows the tile needs anyway, so [ymin, ymax) -- a min and a max, no assumption on order -- only gets shorter.
//
// LDS: RC_SPAN = 288 rows x 32 columns x 4 B = 36,864 B of intermediates + 2 x 19 x 32 x 4 B = 4,864 B of tables = 41,728 B per
// workgroup, three workgroups in a CU's 160 KiB.  288 rows cover the worst case RC_KMAX = 17 taps admit: taps <= 17 means
// support < 8.5 source samples, i.e. at most a 8.5 x bilinear (4.25 x bicubic) down-scale, whose 32 output rows span at most
// 31 * 8.5 + 17 + 2 = 283 source rows.
//
// The tables are data, so every index they yield is clamped once per entry (never per tap) before use: cnt to [0, min(ktaps, side)], lo
// to [0, side - cnt], and the row offset into the LDS image to RC_SPAN - cnt.  For tables the host builder makes the clamps change
// nothing; for any other content they keep every read inside the image and the LDS array.  Stores go by output index alone.
#include <algorithm>

#include "common.hpp"

namespace crdr {

constexpr int RC_KMAX = 17;      // taps per table entry; device_pipeline.KMAX
constexpr int RC_TILE = 32;      // output rows and columns per workgroup
constexpr int RC_SPAN = 288;     // source rows a tile may need
constexpr int RC_BITS = 22;      // PIL's PRECISION_BITS = 32 - 8 - 2

struct RcArgs {
  const uint8_t* pool;
  const int32_t* items;  // [N][4]  {pool byte offset low 32 bits, high 32 bits, H, W}
  const int32_t* tabs;   // [N] { [2 + kt][cw] columns, [2 + kt][ch] rows };  rows of an axis table: lo, cnt, k[0], ..., k[kt - 1]
  float* out;
  int ch, cw, kt, ldo;
};

__device__ __forceinline__ uint32_t rc_clip8(uint32_t acc) {
  const int v = (int)acc >> RC_BITS;   // arithmetic shift, as PIL's
  return (uint32_t)min(max(v, 0), 255);
}

__global__ __launch_bounds__(256) void resize_crop_flip_normalize_kernel(const RcArgs a) {
  __shared__ uint32_t mid[RC_SPAN * RC_TILE];
  __shared__ int32_t htab[(2 + RC_KMAX) * RC_TILE];
  __shared__ int32_t vtab[(2 + RC_KMAX) * RC_TILE];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int c0 = blockIdx.x * RC_TILE, r0 = blockIdx.y * RC_TILE;
  const int nc = min(RC_TILE, a.cw - c0), nr = min(RC_TILE, a.ch - r0);
  const int32_t* it = a.items + (size_t)n * 4;
  const size_t off = (size_t)(uint32_t)it[0] | ((size_t)(uint32_t)it[1] << 32);
  const int H = it[2], W = it[3];
  const int rows = 2 + a.kt;
  const int32_t* th = a.tabs + (size_t)n * rows * (a.cw + a.ch);
  const int32_t* tv = th + (size_t)rows * a.cw;

  for (int e = tid; e < rows * RC_TILE; e += 256) {
    const int row = e >> 5, j = e & 31;
    htab[e] = j < nc ? th[(size_t)row * a.cw + c0 + j] : 0;   // a ragged tile's missing entries: cnt = 0
    vtab[e] = j < nr ? tv[(size_t)row * a.ch + r0 + j] : 0;
  }
  __syncthreads();
  if (tid < 2 * RC_TILE) {   // one lane per entry
    int32_t* t = tid < RC_TILE ? htab : vtab;
    const int j = tid & 31, side = tid < RC_TILE ? W : H;
    const int cnt = min(max(t[RC_TILE + j], 0), min(a.kt, side));
    t[RC_TILE + j] = cnt;
    t[j] = max(0, min(t[j], side - cnt));
  }
  __syncthreads();
  int ymin = H, ymax = 0;
  for (int j = 0; j < nr; ++j) {   // the same LDS words for every lane: broadcast reads
    const int lo = vtab[j], cnt = vtab[RC_TILE + j];
    if (cnt > 0) { ymin = min(ymin, lo); ymax = max(ymax, lo + cnt); }
  }
  const int span = min(ymax - ymin, RC_SPAN);

  // phase one: source rows [ymin, ymin + span) filtered horizontally for the tile's columns
  const uint8_t* img = a.pool + off;
  for (int item = tid; item < span * RC_TILE; item += 256) {
    const int c = item & 31, y = ymin + (item >> 5);
    const int cnt = htab[RC_TILE + c];
    const uint8_t* p = img + ((size_t)y * W + htab[c]) * 3;
    uint32_t s0 = 1u << (RC_BITS - 1), s1 = s0, s2 = s0;
    for (int i = 0; i < cnt; ++i) {
      const uint32_t k = (uint32_t)htab[(2 + i) * RC_TILE + c];
      s0 += k * p[3 * i];
      s1 += k * p[3 * i + 1];
      s2 += k * p[3 * i + 2];
    }
    mid[item] = rc_clip8(s0) | (rc_clip8(s1) << 8) | (rc_clip8(s2) << 16);
  }
  __syncthreads();

  // phase two: the vertical pass, normalise, store
  const int c = tid & 31;
  if (c >= nc) return;
  for (int r = tid >> 5; r < nr; r += 8) {
    const int cnt = vtab[RC_TILE + r];
    const int rel = min(vtab[r] - ymin, RC_SPAN - cnt);   // >= 0 wherever cnt > 0
    uint32_t s0 = 1u << (RC_BITS - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < cnt; ++j) {
      const uint32_t k = (uint32_t)vtab[(2 + j) * RC_TILE + r];
      const uint32_t m = mid[(rel + j) * RC_TILE + c];
      s0 += k * (m & 255u);
      s1 += k * ((m >> 8) & 255u);
      s2 += k * (m >> 16);
    }
    f32x4 v;
    v[0] = ((float)rc_clip8(s0) / 255.0f - 0.5f) / 0.5f;
    v[1] = ((float)rc_clip8(s1) / 255.0f - 0.5f) / 0.5f;
    v[2] = ((float)rc_clip8(s2) / 255.0f - 0.5f) / 0.5f;
    v[3] = 0.f;
    *reinterpret_cast<f32x4*>(a.out + (((size_t)n * a.ch + r0 + r) * a.cw + c0 + c) * a.ldo) = v;
  }
}

}  // namespace crdr

using namespace crdr;

extern "C" int crdr_resize_crop_flip_normalize(const uint8_t* pool, const int32_t* items, const int32_t* tabs, int N, int ktaps, int crop_h,
                                               int crop_w, float* out, int ldo, crdr_stream_t s) {
  const char* what = "resize_crop_flip_normalize";
  CRDR_REQUIRE(pool && items && tabs && out, "%s: null pointer", what);
  CRDR_REQUIRE(ldo >= 4 && ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0, "%s: out must be 16-byte aligned rows", what);
  CRDR_REQUIRE(((reinterpret_cast<uintptr_t>(items) | reinterpret_cast<uintptr_t>(tabs)) & 3) == 0, "%s: items / tabs must be 4-byte aligned", what);
  CRDR_REQUIRE(ktaps >= 1 && ktaps <= RC_KMAX, "%s: %d taps per table entry (1..%d supported: cnt <= KMAX)", what, ktaps, RC_KMAX);
  CRDR_REQUIRE(N >= 0 && N <= 65535 && crop_h >= 0 && crop_w >= 0 && cdiv(crop_h, RC_TILE) <= 65535,
               "%s: N %d crop %d x %d out of range", what, N, crop_h, crop_w);
  if (N == 0 || crop_h == 0 || crop_w == 0) return 0;
  RcArgs a;
  a.pool = pool; a.items = items; a.tabs = tabs; a.out = out; a.ch = crop_h; a.cw = crop_w; a.kt = ktaps; a.ldo = ldo;
  hipLaunchKernelGGL(resize_crop_flip_normalize_kernel, dim3(cdiv(crop_w, RC_TILE), cdiv(crop_h, RC_TILE), N), dim3(256), 0, as_stream(s), a);
  CRDR_CHECK_LAUNCH("resize_crop_flip_normalize_kernel");
  return 0;
}
