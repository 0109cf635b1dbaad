// Host driver of tests/test_carve.py: csrc/carve.h and the resident histogram's scratch layout
// (csrc/hist_scratch.h) on heap blocks of exactly the measured size, under the host sanitizers.
// A plain C++ program: the two headers include nothing from HIP.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../aiyagari_hark_amd/csrc/hist_scratch.h"

using aiy::Carve;

static int g_fail = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);      \
      ++g_fail;                                                       \
    }                                                                 \
  } while (0)

struct Region {
  char* p;
  size_t bytes, align;
};

// Regions in layout order inside [base, base + total): aligned relative to the base, ascending,
// disjoint, the last one ending within the block; first and last byte of each written.
static void check_regions(char* base, size_t total, const std::vector<Region>& rs) {
  size_t end = 0;
  for (const Region& r : rs) {
    const size_t at = (size_t)(r.p - base);
    CHECK(at % r.align == 0);
    CHECK(at >= end);
    if (r.bytes == 0) continue;
    end = at + r.bytes;
    CHECK(end <= total);
    if (end > total) return;
    r.p[0] = 1;
    r.p[r.bytes - 1] = 2;
  }
}

struct Mixed {
  double* a;
  int* b;
  char* c;
  uint16_t* empty;
  unsigned long long* d;
  char* e;
  size_t bytes;
};
static const size_t kMixedCount[6] = {37, 65, 1, 0, 3, 256};
static Mixed mixed(Carve c) {
  Mixed L;
  L.a = c.take<double>(kMixedCount[0]);
  L.b = c.take<int>(kMixedCount[1]);
  L.c = c.take<char>(kMixedCount[2]);
  L.empty = c.take<uint16_t>(kMixedCount[3]);
  L.d = c.take<unsigned long long>(kMixedCount[4]);
  L.e = c.take<char>(kMixedCount[5]);
  L.bytes = c.bytes();
  return L;
}

static void test_mixed() {
  const Mixed m = mixed(Carve());
  CHECK(!m.a && !m.b && !m.c && !m.empty && !m.d && !m.e);   // measuring binds nothing
  CHECK(m.bytes % 256 == 0);
  // 296 -> 512, 260 -> 512, 1 -> 256, 0 -> 0, 24 -> 256, 256 -> 256
  CHECK(m.bytes == 512 + 512 + 256 + 0 + 256 + 256);
  char* base = static_cast<char*>(std::malloc(m.bytes));
  const Mixed L = mixed(Carve(base));
  CHECK(L.bytes == m.bytes);
  CHECK((char*)L.a == base);
  check_regions(base, m.bytes,
                {{(char*)L.a, 37 * sizeof(double), 256}, {(char*)L.b, 65 * sizeof(int), 256}, {L.c, 1, 256},
                 {(char*)L.empty, 0, 256}, {(char*)L.d, 3 * sizeof(unsigned long long), 256}, {L.e, 256, 256}});
  // the empty region consumed nothing: the next region starts where it does
  CHECK((char*)L.empty == (char*)L.d);
  CHECK((size_t)((char*)L.d - base) == 512 + 512 + 256);
  std::free(base);
  // a cursor that took only empty regions has handed out nothing
  Carve z;
  z.take<double>(0);
  z.take<int>(0);
  CHECK(z.bytes() == 0);
}

// hc_scratch's closed form before the layout was carved
static size_t hc_closed_form(int cals, int G, int cap) {
  return (size_t)cals * G * 2 * cap * sizeof(double) + (size_t)cals * G * 32 * 4 * sizeof(int) +
         (size_t)cals * aiy::kHcCtrStride * sizeof(unsigned) + (size_t)cals * 2 * G * aiy::kHcRedRec * sizeof(double) +
         256;
}

static void test_hc(int cals, int G, int cap) {
  const aiy::HcScratch m = aiy::hc_scratch(Carve(), cals, G, cap);
  std::printf("hc_scratch(%d, %d, %d) = %zu (closed form %zu)\n", cals, G, cap, m.bytes, hc_closed_form(cals, G, cap));
  CHECK(m.bytes == hc_closed_form(cals, G, cap));
  char* base = static_cast<char*>(std::malloc(m.bytes));
  const aiy::HcScratch L = aiy::hc_scratch(Carve(base), cals, G, cap);
  CHECK(L.bytes == m.bytes);
  CHECK(L.ctr_bytes == (size_t)cals * aiy::kHcCtrStride * sizeof(unsigned));
  CHECK(L.dist_bytes == (size_t)cals * 2 * G * aiy::kHcRedRec * sizeof(double));
  check_regions(base, m.bytes,
                {{(char*)L.slab, (size_t)cals * G * 2 * cap * sizeof(double), 256},
                 {(char*)L.span, (size_t)cals * G * 32 * 4 * sizeof(int), 256},
                 {(char*)L.ctr, L.ctr_bytes, 128},
                 {(char*)L.dist, L.dist_bytes, 128},
                 {(char*)L.err, 256, 128}});
  std::free(base);
}

static void test_hcd() {
  const size_t vec = 3 * 7 * 41 + 5, ainv = 3 * 7 * 42;
  for (const size_t n_ainv : {ainv, (size_t)0}) {
    const aiy::HcdScratch m = aiy::hcd_scratch(Carve(), vec, n_ainv);
    CHECK(m.bytes % 256 == 0);
    char* base = static_cast<char*>(std::malloc(m.bytes));
    const aiy::HcdScratch L = aiy::hcd_scratch(Carve(base), vec, n_ainv);
    check_regions(base, m.bytes, {{(char*)L.vec, vec * sizeof(double), 256}, {(char*)L.ainv, n_ainv * sizeof(int), 256}});
    std::free(base);
  }
}

int main() {
  test_mixed();
  test_hc(1, 1, 512);
  test_hc(3, 10, 18000);
  test_hc(24, 10, 19456);
  test_hcd();
  std::printf(g_fail ? "FAILED %d\n" : "OK\n", g_fail);
  return g_fail ? 1 : 0;
}
