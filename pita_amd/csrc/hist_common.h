// The bin rule shared by every histogram kernel of the library (pita_histogram, pita_weighted_histogram,
// pita_pair_distance_histogram, pita_dihedral_histogram2d per axis): numpy.histogram's.
#pragma once
#include "common.h"

namespace pita {

constexpr int HIST_MAX_BINS = 1024;

// Bin of x over the ascending edges e[0 .. nbins] (an LDS copy), lo = e[0], hi = e[nbins], inv = nbins / (hi - lo):
// bin i = [e[i], e[i + 1]), the last bin closed on the right; -1 for a value outside [lo, hi] or a NaN (not counted).
// A guessed bin from the uniform spacing is corrected against the edges, so that the result is numpy's bin for bin on
// uniform and non-uniform edges alike.
__device__ __forceinline__ int hist_bin(float x, const float* e, int nbins, float lo, float hi, float inv) {
  if (!(x >= lo && x <= hi)) return -1;  // out of range or NaN
  int i = (int)((x - lo) * inv);
  i = i < 0 ? 0 : (i > nbins - 1 ? nbins - 1 : i);
  while (i > 0 && x < e[i]) --i;
  while (i < nbins - 1 && x >= e[i + 1]) ++i;
  return i;
}

}  // namespace pita
