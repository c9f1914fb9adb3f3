// The forced-algorithm id (crdr_conv_desc.reserved, the low 16 bits of crdr_wgrad_desc.algo): the one place in the library that takes it apart
// or puts it together.  Its layout is ABI (the tuner's database, bench.py, the tools and the tests hold raw ids); include/crdr_hip.h has the table.
//   bits 0..7   0: the library chooses; else 1 + an index into the kernel families laid end to end (`sizes`, below)
//   bits 8..11  log2(splits) for the tiled conv kernels and every wgrad kernel, but splits - 1 for the F(4x4) conv kernel (its K range divides
//               into any number of parts up to 16); the streaming and F(2x2) conv kernels have no split and refuse anything but 0
// crdr_conv2d_wgrad_num_configs() counts the F(2x2) slab kernel and ..._num_wino_configs() = 2 counts it again: hence the F(4x4) slab id is
// num_configs() + 1 wherever a caller computes it.
#pragma once

namespace crdr {

enum AlgoFamily { kAlgoBuiltIn, kAlgoTiled /* wgrad: direct */, kAlgoStream, kAlgoWino2, kAlgoWino4, kAlgoBeyond /* names no kernel */ };
struct AlgoId {
  AlgoFamily family;
  int index;   // inside the family (kAlgoBeyond: the low byte - 1, what the planners report as the config out of range)
  int split;   // bits 8..11 as they stand
};

// sizes: members of the families kAlgoTiled .. kAlgoWino4, in id order
inline AlgoId algo_decode(int id, const int (&sizes)[4]) {
  const int base = id & 0xff, split = (id >> 8) & 0xf;
  for (int f = 0, first = 1; id != 0 && f < 4; first += sizes[f++])
    if (base >= first && base < first + sizes[f]) return {AlgoFamily(kAlgoTiled + f), base - first, split};
  return {id == 0 ? kAlgoBuiltIn : kAlgoBeyond, base - 1, split};
}
inline AlgoId conv_algo_decode(int reserved, int ntiled, int nstream) { return algo_decode(reserved, {ntiled, nstream, 2, 1}); }
inline AlgoId wgrad_algo_decode(int algo, int ndirect) { return algo_decode(algo & 0xffff, {ndirect, 0, 1, 1}); }   // (bits 16..: mode flags)

inline int conv_algo_splits(const AlgoId& id) { return id.family == kAlgoWino4 ? id.split + 1 : 1 << id.split; }
inline int wgrad_algo_splits(const AlgoId& id) { return 1 << id.split; }

inline int conv_algo_encode(AlgoFamily family, int index, int nsplit, int ntiled, int nstream) {
  const int first[] = {1, 1 + ntiled, 1 + ntiled + nstream, 1 + ntiled + nstream + 2};
  int ls = 0;
  while ((1 << ls) < nsplit) ++ls;
  return (first[family - kAlgoTiled] + index) | ((family == kAlgoWino4 ? nsplit - 1 : ls) << 8);
}

}  // namespace crdr
