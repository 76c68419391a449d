// plan_check.cpp — the first level's host planner (csrc/srs_plan.hip) alone,
// built for the host with -fsanitize=address,undefined (plan.mk): histograms
// at the planner's edges, for 32- and 64-bit keys, with the properties the
// sort relies on (tests/test_table_plan.py) asserted here. Exit code 0 and
// "plan_check ok" on success; a sanitizer report aborts the program.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "srs_plan.h"

using namespace srs;

static int g_failures = 0;
static std::string g_case;

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      g_failures++;                                                              \
      fprintf(stderr, "FAIL %s: %s (line %d)\n", g_case.c_str(), #cond, __LINE__); \
    }                                                                            \
  } while (0)

using Hist = std::vector<uint32_t>;

// the group of every 16-bit bin's first key, as pass_digit computes it
static std::vector<int> groups_of_bins(const TablePlan& P) {
  std::vector<int> g(65536);
  for (int b = 0; b < 65536; b++) {
    if (P.mode == 1) {
      g[b] = P.lut16[b];
    } else {  // split table: first group | lg << 16, by the top 9 bits
      const int e = P.tab3[b >> 7], lg = e >> 16;
      g[b] = (e & 0xFFFF) + (lg <= 7 ? (b & 127) >> (7 - lg) : (b & 127) << (lg - 7));
    }
  }
  return g;
}

static void check_table(const Hist& h, int64_t n, int key_bits, const char* force) {
  TablePlan P;
  plan_table(h, n, key_bits, force, &P);
  const int before = g_failures;
  CHECK(P.mode == 0 || P.mode == 1 || P.mode == 3);
  if (P.mode == 0) return;
  CHECK(P.groups >= 1 && P.groups <= 512);
  CHECK((int)P.rbits.size() == kGroups);
  CHECK(P.mode != 1 || P.lut16.size() == 65536);
  CHECK(P.mode != 3 || P.tab3.size() == 512);
  if (g_failures != before) return;  // (the tables below would be read out of bounds)
  for (int r : P.rbits) CHECK(r >= 0 && r <= key_bits);
  if (P.mode == 3)
    for (int t = 0; t < 512; t++) {
      const int lg = P.tab3[t] >> 16, g0 = P.tab3[t] & 0xFFFF;
      CHECK(lg >= 0 && lg <= 9);
      CHECK(g0 + (1 << lg) <= 512);  // (every entry below the group count's limit)
    }
  const std::vector<int> g = groups_of_bins(P);
  int prev = 0;
  for (int b = 0; b < 65536; b++) {
    // (below the 512 groups the tables are built for; TablePlan::groups counts
    // the groups in use, and a 16-bit table's ids may skip some)
    CHECK(g[b] >= 0 && g[b] < kGroups);
    CHECK(g[b] >= prev);  // group ids never decrease with the bin
    prev = g[b];
  }
}

static void check_ranges(const Hist& h, int key_bits) {
  std::vector<KeyCluster> cl;
  const bool ok = find_clusters(h, &cl);
  if (!ok) {
    CHECK(cl.empty());
    return;
  }
  CHECK((int)cl.size() <= kMaxRanges);
  for (size_t c = 0; c < cl.size(); c++) {
    CHECK(cl[c].b0 <= cl[c].b1 && cl[c].b1 - cl[c].b0 < kClusterSpan && cl[c].cnt > 0);
    if (c) CHECK(cl[c].b0 - cl[c - 1].b1 > kClusterGap);
  }
  if (cl.empty()) return;
  uint64_t hi[kMaxRanges];
  range_splits(cl, key_bits, hi);
  for (size_t c = 0; c + 1 < cl.size(); c++) CHECK(hi[c] < hi[c + 1] || hi[c + 1] == ~0ull);
  // the exact pass's answer: every cluster's keys fill its sampled bins (and,
  // a second time, sit on one value each)
  const int low = key_bits - 16;
  for (int single = 0; single < 2; single++) {
    uint64_t got[2 * kMaxRanges];
    for (int c = 0; c < kMaxRanges; c++) {
      got[2 * c] = ~0ull;
      got[2 * c + 1] = 0;
    }
    for (size_t c = 0; c < cl.size(); c++) {
      got[2 * c] = (uint64_t)cl[c].b0 << low;
      got[2 * c + 1] = single ? got[2 * c] : (((uint64_t)cl[c].b1 + 1) << low) - 1;
    }
    RangePlan P;
    plan_ranges(cl, hi, got, key_bits, &P);
    if (P.one_value) {
      CHECK(single && cl.size() == 1 && !P.use);
      continue;
    }
    CHECK(P.use);
    CHECK(P.nranges == (int)cl.size());
    CHECK(P.shift >= 0 && P.shift <= key_bits);
    CHECK(P.final_lvl == (P.shift == 0));
    CHECK(P.used >= 1 && P.used <= 512);  // the used buckets
    for (int c = 0; c < P.nranges; c++) {
      CHECK(P.base[c] >= 0 && P.base[c] < 512);
      if (c) CHECK(P.base[c] > P.base[c - 1]);  // the bases increase
      // the bucket of the range's smallest key is its base
      const uint64_t lo = P.shift >= 64 ? 0 : P.mn[c] >> P.shift;
      CHECK((uint32_t)((uint32_t)lo + P.rng_adj[c]) == (uint32_t)P.base[c]);
    }
  }
}

static void run(const char* name, const Hist& h, int64_t n) {
  for (int key_bits : {32, 64}) {
    g_case = std::string(name) + (key_bits == 32 ? " (32)" : " (64)");
    for (const char* force : {(const char*)nullptr, "1", "3"}) check_table(h, n, key_bits, force);
    check_ranges(h, key_bits);
  }
}

int main() {
  const int64_t n = int64_t(1) << 30;
  {
    Hist h(65536, 64);
    run("flat", h, n);
  }
  {
    Hist h(65536, 0);
    h[12345] = 1u << 22;
    run("one bin", h, n);
  }
  {
    Hist h(65536, 0);
    h[777] = 1;
    run("n = 1", h, 1);
  }
  {
    Hist h(65536, 0);
    for (int b = 100; b < 140; b++) h[b] = 50000;
    for (int b = 100 + 4097 + 39; b < 100 + 4097 + 80; b++) h[b] = 50000;
    run("two clusters", h, n);
  }
  {
    Hist h(65536, 0);
    for (int b = 30000; b < 30000 + 256; b++) h[b] = 16384;
    run("cluster of 256 bins", h, n);
  }
  {
    Hist h(65536, 0);
    for (int b = 30000; b < 30000 + 257; b++) h[b] = 16384;
    run("cluster of 257 bins", h, n);
  }
  {
    // float keys in [-1, 1), transformed: negatives below 0x8000 (bins count
    // down from -0.0 = 0x7FFF), non-negatives from 0x8000 up to 1.0 = 0xBF80;
    // each exponent (128 bins) holds half the keys of the one above it
    Hist h(65536, 0);
    for (int e = 0; e < 24; e++) {
      const uint32_t per_bin = (1u << 21 >> e) / 128 + 1;
      for (int j = 0; j < 128; j++) {
        h[0xBF80 - 128 * (e + 1) + j] = per_bin;      // [2^-(e+1), 2^-e)
        h[0x407F + 128 * e + 1 + j] = per_bin;        // (-2^-e, -2^-(e+1)]
      }
    }
    run("floats in [-1, 1)", h, n);
  }
  {
    Hist h(65536, 3);
    for (int j = 0; j < 128; j++) h[200 * 128 + j] = 30000;
    run("all bins, one heavy top-9-bit bin", h, n);
  }
  {
    Hist h(65536, 1);
    h[65535] = 1u << 22;
    run("last bin heavy", h, n);
  }
  {
    Hist h(65536, 0);
    h[65535] = 1u << 22;
    run("last bin only", h, n);
  }
  if (g_failures) {
    printf("plan_check: %d failures\n", g_failures);
    return 1;
  }
  printf("plan_check ok\n");
  return 0;
}
