// Layouts of the resident histogram's handle scratch (hist_resident.hip).  Pure host code.
#pragma once

#include "carve.h"

namespace aiy {

constexpr int kHcCtrStride = 32;                   // uints between cluster counters (128 B)
constexpr int kHcRedRec = 16;                      // 8-byte words per (parity, workgroup) record of `dist`

// One launch of `cals` calibration clusters of G workgroups with `cap` doubles per slab.
// Counters and reduction records are 128-byte units and are packed at that alignment.
struct HcScratch {
  double* slab;     // [cals][G][2][cap]
  int* span;        // [cals][G][32][4]
  unsigned* ctr;    // [cals][kHcCtrStride]
  double* dist;     // [cals][2][G][kHcRedRec]
  unsigned* err;
  size_t ctr_bytes, dist_bytes, bytes;
};
inline HcScratch hc_scratch(Carve c, int cals, int G, int cap) {
  constexpr size_t kUnit = kHcCtrStride * sizeof(unsigned);
  static_assert(kUnit == kHcRedRec * sizeof(double), "counter stride = reduction record");
  HcScratch L;
  L.ctr_bytes = (size_t)cals * kHcCtrStride * sizeof(unsigned);
  L.dist_bytes = (size_t)cals * 2 * G * kHcRedRec * sizeof(double);
  L.slab = c.take<double>((size_t)cals * G * 2 * cap);
  L.span = c.take<int>((size_t)cals * G * 32 * 4);
  L.ctr = c.take<unsigned>((size_t)cals * kHcCtrStride, kUnit);
  L.dist = c.take<double>((size_t)cals * 2 * G * kHcRedRec, kUnit);
  L.err = c.take<unsigned>(256 / sizeof(unsigned), kUnit);
  L.bytes = c.bytes();
  return L;
}

// The vectors a solve keeps in HBM (Aitken: stored differences; BiCGSTAB: the p rows, v
// blocks or r, p, v, t of the pull form), then the pull forms' inverse lottery.
struct HcdScratch {
  double* vec;
  int* ainv;
  size_t bytes;
};
inline HcdScratch hcd_scratch(Carve c, size_t vec_doubles, size_t ainv_ints) {
  HcdScratch L;
  L.vec = c.take<double>(vec_doubles);
  L.ainv = c.take<int>(ainv_ints);
  L.bytes = c.bytes();
  return L;
}

}  // namespace aiy
