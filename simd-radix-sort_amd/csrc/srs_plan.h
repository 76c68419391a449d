// srs_plan.h — the first level's host-side planning (srs_plan.hip): plain
// arithmetic on the sampled 16-bit histogram and on the clusters' exact
// min / max keys. No workspace, no stream, no HIP call: the driver
// (srs_api.hip) runs the device passes and hands their results in, and
// tests/cpp/plan_check.cpp runs this unit alone under the sanitizers.
#pragma once

#include <stdint.h>

#include <vector>

#include "srs_common.h"

namespace srs {

constexpr int kGroups = kMaxBins;

// The digit table of a balanced first level, planned from the sampled
// 16-bit histogram h of the transformed keys (n input keys): mode 0 (no
// table: it would not beat the plain digit), 1 (16-bit bins -> groups,
// lut16) or 3 (split table, tab3), each group's rbits, and the predicted
// keys the next level leaves above the LDS capacity (over; over_other for
// the table not taken). srs_debug_plan_table exposes it. force: the
// SRS_TABLE knob ("1" or "3" forces the table kind; NULL or empty: chosen).
struct TablePlan {
  int mode = 0;
  std::vector<int32_t> lut16, tab3, rbits;
  int groups = 0;
  double over = 0, over_other = 0;
};
void plan_table(const std::vector<uint32_t>& h, int64_t n, int key_bits, const char* force,
                TablePlan* P);

// The sampled keys' clusters (SoA only): at most kMaxRanges clusters of at
// most kClusterSpan adjacent 16-bit bins each (e.g. the reference's Gaussian
// keys: one cluster around 0 for signed keys, two at both ends of the range
// for unsigned ones): a range level decides (plan_ranges), no digit table.
// find_clusters: false, and none, when there are more or one is wider.
struct KeyCluster {
  int b0, b1;    // first and last sampled 16-bit bin
  uint64_t cnt;  // sampled keys
};
constexpr int kClusterGap = 4096;  // bins between two clusters
constexpr int kClusterSpan = 256;  // bins a cluster may cover
bool find_clusters(const std::vector<uint32_t>& h, std::vector<KeyCluster>* cl);

// Range level, host half. range_splits: the split points
// halfway between the clusters (range c's keys: u in (hi[c-1], hi[c]]) for
// the exact min / max pass. plan_ranges: from that pass's got[2c], got[2c + 1]
// (min > max: no key), the one shift that fits every non-empty range into
// the level's buckets, SortDesc's rng_hi / rng_adj, each range's first bucket.
struct RangePlan {
  bool use = false;        // a range level runs
  bool final_lvl = false;  // every bucket holds one key value (shift 0)
  bool one_value = false;  // all keys are equal
  int shift = 0;
  int nranges = 0;    // the non-empty ranges, in key order: their exact
  uint64_t mn[kMaxRanges], mx[kMaxRanges];  // smallest and largest key,
  int base[kMaxRanges];                     // their first bucket
  uint32_t used = 0;  // buckets taken
  uint64_t rng_hi[kMaxRanges];
  uint32_t rng_adj[kMaxRanges];
};
void range_splits(const std::vector<KeyCluster>& cl, int key_bits, uint64_t hi[kMaxRanges]);
void plan_ranges(const std::vector<KeyCluster>& cl, const uint64_t hi[kMaxRanges],
                 const uint64_t got[2 * kMaxRanges], int key_bits, RangePlan* P);

}  // namespace srs
