// Winograd F(2x2, 3x3) path of crdr_conv2d (wino.hip), planned and launched from igemm.hip.
#pragma once
#include <algorithm>

#include "common.hpp"
#include "igemm_args.hpp"

namespace crdr {

// The tap table of a k x k stride-1 convolution (plain or transposed) as a window: win[dh * k + dw] = weight-pack index of the tap `dh` rows and
// `dw` columns from the window's first tap (-1: no such tap), *dmin = the first tap's offset from the output pixel.  `who` names the kernel in
// the refusals.
inline int tap_window(const IgemmTaps& taps, int k, const char* who, bool complete, int* win, int* dmin) {
  *dmin = 127;
  for (int t = 0; t < k * k; ++t) *dmin = std::min(*dmin, (int)(signed char)(taps.packed[t] & 0xff));
  for (int t = 0; t < k * k; ++t) win[t] = -1;
  for (int t = 0; t < k * k; ++t) {
    const int v = taps.packed[t];
    const int dh = (int)(signed char)(v & 0xff) - *dmin, dw = (int)(signed char)((v >> 8) & 0xff) - *dmin;
    CRDR_REQUIRE(dh >= 0 && dh < k && dw >= 0 && dw < k, "conv2d: %s: tap offsets are not a %dx%d window", who, k, k);
    win[dh * k + dw] = v >> 16;
  }
  for (int t = 0; complete && t < k * k; ++t) CRDR_REQUIRE(win[t] >= 0, "conv2d: %s: incomplete %dx%d window", who, k, k);
  return 0;
}

// What both Winograd kernels ask of a launch beyond its shape: no gate / pre-add / split-bf16 epilogue, no epilogue operand that a grouped launch
// cannot take per problem, and an input tensor (with the 8 rows a patch may reach past it) that one 2 GiB buffer descriptor spans.  The outputs'
// extents are checked per kernel: the two base their descriptors differently.
inline bool wino_admits(const crdr_conv_desc* d, int G) {
  if (d->flags & (CRDR_EPI_GATE | CRDR_EPI_PREADD | CRDR_CONV_BF16X3)) return false;
  if (G > 1 && (d->flags & (CRDR_EPI_VEC2 | CRDR_EPI_AFFINE | CRDR_EPI_MASKOFF))) return false;
  return ((long long)d->N * d->H + 8) * d->W * d->ldx * 4 < (1ll << 31);
}

// the Winograd kernel of a plan (igemm.hip: Plan::wino)
enum class WinoKernel { None, F2, F2Pairs, F4 };

bool wino_eligible(const crdr_conv_desc* d, int G);
size_t wino_workspace(const crdr_conv_desc* d, int G);   // bytes of transformed filters
int wino_colsum_rows(const crdr_conv_desc* d);
bool wino_pairs_ok(const crdr_conv_desc* d);   // the pair-tile variant applies
int wino_launch(const crdr_conv_desc* d, bool pairs, IgemmArgs a, const IgemmTaps& taps, const IgemmGroup& grp, int G, float* u, hipStream_t s);

// Winograd F(4x4, 3x3) path (wino4.hip): the third of the forced Winograd ids.  vec_ok: every operand row is 16-byte aligned (known at
// launch; planning passes true)
bool wino4_eligible(const crdr_conv_desc* d, int G, bool vec_ok);
size_t wino4_workspace(const crdr_conv_desc* d, int G, int nsplit);   // bytes of transformed filters (+ the partial tiles of a K-split launch)
bool wino4_split_ok(const crdr_conv_desc* d, int G, int nsplit);      // nsplit K splits per tile (forced id: bits 8..11 = nsplit - 1)
int wino4_colsum_rows(const crdr_conv_desc* d);
int wino4_filter_item(const crdr_conv_desc* d, const IgemmTaps& taps, int G, crdr_w4_filter_item* it);   // crdr_conv2d_filter_item
int wino4_filters_batched(const crdr_w4_filter_item* items, const long long* prefix, const long long* meta, hipStream_t s);
int wino4_launch(const crdr_conv_desc* d, IgemmArgs a, const IgemmTaps& taps, const IgemmGroup& grp, int G, float* u, float* slabs, int nsplit,
                 bool filters_ready, hipStream_t s);

}  // namespace crdr
