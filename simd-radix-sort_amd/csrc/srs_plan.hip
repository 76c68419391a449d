// srs_plan.hip — the first level's host-side planning: the digit table of a
// balanced first level, the key clusters of the sample, the range level's
// bucket arithmetic. Host code only (srs_plan.h); the GPU waits while it runs.
#include "srs_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

namespace srs {

// The balanced first level's table (plan_balanced_level in srs_api.hip says
// when): 512 key-range groups of ~equal size through a digit table (the
// multi-GPU partition's LUT digit). Each group's children start below the
// key prefix its bins share.
void plan_table(const std::vector<uint32_t>& h, int64_t n, int key_bits, const char* force,
                TablePlan* P) {
  *P = TablePlan();
  // (host time here is GPU idle time: every pass below looks only at the
  // non-empty bins or is a plain integer sweep)
  std::vector<uint64_t> ct(512, 0);
  std::vector<int32_t> nz;  // the non-empty bins
  nz.reserve(8192);
  for (int b0 = 0; b0 < 65536; b0 += 16) {  // (skips empty runs 16 bins at a time)
    uint64_t any = 0;
    for (int j = 0; j < 16; j++) any |= h[b0 + j];
    if (!any) continue;
    for (int b = b0; b < b0 + 16; b++)
      if (h[b]) {
        nz.push_back(b);
        ct[b >> 7] += h[b];
      }
  }
  uint64_t total = 0;
  for (uint64_t c : ct) total += c;
  if (total == 0) return;
  // Bins -> groups. Candidate groupings of the 16-bit bins into 512 key-range
  // groups; the one whose next level is predicted to leave the fewest keys in
  // buckets above the LDS capacity wins (a group's next digit splits its key
  // range evenly, so a group that mixes bins of different key density, e.g.
  // two float exponents, overfills the buckets of the denser one: C2 had 2101
  // such buckets, 5 % of its keys, taking a third and fourth level):
  //  * cumulative: group of bin b = floor(G * (keys before b + half of b) / total);
  //  * bin-aligned: a top-9-bit bin worth at least one group gets groups of its
  //    own, cut at 16-bit bins by key counts; bins worth less share groups of
  //    at most one share.
  const double to_n = (double)n / (double)total;  // sample -> input keys
  // predicted keys the next level leaves in buckets above kLocalCap (keys
  // uniform inside a 16-bit bin), or that need two more levels
  std::vector<double> qsum(kMaxBins, 0.0);
  auto overflow = [&](const std::vector<int32_t>& L) -> double {
    // a group's bins are one run of the (monotone) table
    std::vector<int32_t> fst(kGroups, -1), lst(kGroups, -1), nz0(kGroups, 0), nz1(kGroups, 0);
    std::vector<uint64_t> cnt(kGroups, 0);
    // each group's run of the (monotone) table: one forward sweep that
    // gallops over each run instead of stepping through 65,536 entries
    for (int b = 0; b < 65536;) {
      const int g = L[b];
      int step = 1;
      while (b + step < 65536 && L[b + step] == g) step <<= 1;
      int lo = b + (step >> 1), hi = std::min(b + step, 65536);  // last g in [lo, hi)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (L[mid] == g) lo = mid;
        else hi = mid;
      }
      fst[g] = b;
      lst[g] = lo;
      b = lo + 1;
    }
    for (size_t i = 0; i < nz.size(); i++) {  // the group's non-empty bins: nz[nz0, nz1)
      const int g = L[nz[i]];
      if (!cnt[g]) nz0[g] = (int32_t)i;
      nz1[g] = (int32_t)i + 1;
      cnt[g] += h[nz[i]];
    }
    double over = 0;
    for (int g = 0; g < kGroups; g++) {
      const double len = (double)cnt[g] * to_n;
      if (len <= kLocalCap) continue;
      int bl = 0;
      while ((1 << bl) <= (fst[g] ^ lst[g])) bl++;
      int need;
      if (levels_for((int64_t)len, kLocalCapTarget, &need) > 1) {
        over += len;
        continue;
      }
      const int bits = choose_bits((int64_t)len, key_bits - (16 - bl));
      if (bits >= bl) {  // each bin splits into 2^(bits - bl) buckets
        const double lim = (double)kLocalCap * (double)(1 << (bits - bl)) / to_n;
        const double lim3 = lim + 3.0 * std::sqrt(lim);  // (sample noise)
        for (int i = nz0[g]; i < nz1[g]; i++)
          if ((double)h[nz[i]] > lim3) over += h[nz[i]] * to_n;
      } else {  // each bucket spans 2^(bl - bits) bins of the aligned range
        const int sh = bl - bits, b0 = fst[g] & ~((1 << bl) - 1);
        int qlo = kMaxBins, qhi = -1;
        for (int i = nz0[g]; i < nz1[g]; i++) {
          const int q = (nz[i] - b0) >> sh;
          qsum[q] += h[nz[i]];
          qlo = std::min(qlo, q);
          qhi = std::max(qhi, q);
        }
        const double lim = (double)kLocalCap / to_n, lim3 = lim + 3.0 * std::sqrt(lim);
        for (int q = qlo; q <= qhi; q++) {
          if (qsum[q] > lim3) over += qsum[q] * to_n;
          qsum[q] = 0;
        }
      }
    }
    return over;
  };
  // The 16-bit-table candidates (DigitLut mode 1, below) are planned only
  // when the split table's predicted overflow is not already zero (they cost
  // ~0.3 ms of host time, during which the GPU waits).
  std::vector<int32_t> lut(65536), first(kGroups, -1), last(kGroups, -1), rbits(kGroups);
  double over_best = -1;  // (-1: not evaluated)
  int buckets_used = 0, groups_used = 0;
  for (int t = 0; t < 512; t++) buckets_used += ct[t] != 0;
  // false: no table pays
  auto plan_mode1 = [&]() -> bool {
    {  // (an empty bin takes the group before it)
      double before = 0;
      int g = 0, at = 0;
      for (int b : nz) {
        std::fill(lut.begin() + at, lut.begin() + b, g);
        const int x = (int)((before + 0.5 * h[b]) * kGroups / (double)total);
        g = std::min(std::max(x, g), kGroups - 1);
        lut[b] = g;
        at = b + 1;
        before += h[b];
      }
      std::fill(lut.begin() + at, lut.end(), g);
    }
    over_best = overflow(lut);
    {
      std::vector<int32_t> la(65536, 0);
      std::vector<double> x(512);
      for (int t = 0; t < 512; t++) x[t] = (double)kGroups * (double)ct[t] / (double)total;
      for (double sc = 1.0; sc > 0.5; sc -= 0.005) {
        std::vector<int> nt(512, 0);
        int S = 0;
        double acc = 0;
        bool open = false;
        for (int t = 0; t < 512; t++) {
          if (!ct[t]) continue;
          if (x[t] < 1.0) {
            if (!open || acc + x[t] > 1.0) {
              S++;
              open = true;
              acc = 0;
            }
            acc += x[t];
            continue;
          }
          open = false;
          nt[t] = std::min(128, std::max(1, (int)std::lround(x[t] * sc)));
          S += nt[t];
        }
        if (S > kGroups) continue;
        int g = -1;
        acc = 0;
        open = false;
        for (int t = 0; t < 512; t++) {
          if (!ct[t] || x[t] < 1.0) {
            if (ct[t] && (!open || acc + x[t] > 1.0)) {
              g++;
              open = true;
              acc = 0;
            }
            acc += x[t];
            for (int j = 0; j < 128; j++) la[t * 128 + j] = std::max(g, 0);
            continue;
          }
          open = false;
          const int base = g + 1;
          double before = 0;
          int prev = 0;
          for (int j = 0; j < 128; j++) {
            const double hj = h[t * 128 + j];
            int k = (int)((before + 0.5 * hj) * nt[t] / (double)ct[t]);
            k = std::min(std::max(k, prev), nt[t] - 1);
            prev = k;
            la[t * 128 + j] = base + k;
            before += hj;
          }
          g = base + nt[t] - 1;
        }
        const double o = overflow(la);
        if (o <= over_best) {
          over_best = o;
          lut.swap(la);
        }
        break;
      }
    }
    for (int b = 0; b < 65536; b++) {
      const int g = lut[b];
      if (first[g] < 0) first[g] = b;
      last[g] = b;
    }
    // the table only pays when its groups outnumber the plain digit's
    // non-empty buckets (Gaussian int64 keys fill two 16-bit bins: both ways
    // give two buckets, and the table pass is the slower one)
    {
      std::vector<uint8_t> has(kGroups, 0);
      for (int b : nz) has[lut[b]] = 1;
      for (int g = 0; g < kGroups; g++) groups_used += has[g];
    }
    if (groups_used < 2 * buckets_used) return false;
    for (int g = 0; g < kGroups; g++) {
      const int diff = first[g] < 0 ? 0xFFFF : (first[g] ^ last[g]);
      int bl = 0;
      while ((1 << bl) <= diff) bl++;
      rbits[g] = key_bits - (16 - bl);  // the group's keys share 16 - bl top bits
    }
    return true;
  };
  // Split table (DigitLut mode 3), when its next level overflows no more:
  // each top-9-bit bin t gets 2^lg_t consecutive groups, the next lg_t key
  // bits (no group spans two bins unless both are worth less than a group).
  // One 2 KB table and one lookup per key instead of the two-level 16-bit
  // table (up to 24 KB staged per tile, two dependent lookups).
  {
    const int kb = key_bits;
    // A group's rbits bounds every key code the table sends it, so a group
    // that takes a run of empty bins, or bins of different key density (two
    // float exponents), gets a next digit that splits the keys it holds
    // badly: C2's first group took the 128 empty bins below -1.0 (rbits 31)
    // and left 1.95 M keys in one bucket, its shared tail group put one
    // exponent's keys into a sixteenth of its buckets. When they fit, every
    // non-empty bin gets groups of its own and every run of empty bins one
    // group (which stays empty unless the sample missed keys). Otherwise bins
    // worth less than one group share groups (consecutive, at most one share
    // each) and empty bins join the group before them.
    std::vector<int> lg(512, -1);     // own groups 2^lg; -1: none
    std::vector<int> share(512, -1);  // >= 0: index of the shared group it joins
    int S = 0;
    int nonempty = 0, empty_runs = 0;
    for (int t = 0; t < 512; t++) {
      nonempty += ct[t] != 0;
      empty_runs += !ct[t] && (t == 0 || ct[t - 1]);
    }
    const bool own = nonempty + empty_runs <= 512;
    if (own) {
      S = empty_runs;
      for (int t = 0; t < 512; t++) {
        if (!ct[t]) continue;
        const double x = 512.0 * (double)ct[t] / (double)total;
        int l = 0;
        while (l < 9 && (double)(2 << l) <= x * 1.4142) l++;  // (nearest power of two)
        lg[t] = l;
        S += 1 << l;
      }
    } else {
      double acc = 0;
      int nsh = 0;
      bool open = false;
      for (int t = 0; t < 512; t++) {
        if (!ct[t]) continue;
        const double x = 512.0 * (double)ct[t] / (double)total;
        if (x < 1.0) {
          if (!open || acc + x > 1.0) {
            nsh++;
            S++;
            open = true;
            acc = 0;
          }
          share[t] = nsh - 1;
          acc += x;
          continue;
        }
        open = false;
        int l = 0;
        while (l < 9 && (double)(2 << l) <= x * 1.4142) l++;  // (nearest power of two)
        lg[t] = l;
        S += 1 << l;
      }
    }
    auto gsize = [&](int t, int l) { return (double)ct[t] / (double)(1 << l); };
    {  // over budget: halve where the resulting groups stay smallest (min-heap)
      std::priority_queue<std::pair<double, int>, std::vector<std::pair<double, int>>,
                          std::greater<std::pair<double, int>>> q;
      for (int t = 0; t < 512; t++)
        if (lg[t] > 0) q.push({gsize(t, lg[t] - 1), t});
      while (S > 512 && !q.empty()) {
        const int t = q.top().second;
        q.pop();
        S -= 1 << (lg[t] - 1);
        lg[t]--;
        if (lg[t] > 0) q.push({gsize(t, lg[t] - 1), t});
      }
    }
    {  // spare budget: split the largest groups that still fit (max-heap; a
       // bin whose doubling does not fit now never will: the budget only shrinks)
      std::priority_queue<std::pair<double, int>> q;
      for (int t = 0; t < 512; t++)
        if (lg[t] >= 0 && lg[t] < 9) q.push({gsize(t, lg[t]), t});
      while (!q.empty()) {
        const int t = q.top().second;
        q.pop();
        if (S + (1 << lg[t]) > 512) continue;
        S += 1 << lg[t];
        lg[t]++;
        if (lg[t] < 9) q.push({gsize(t, lg[t]), t});
      }
    }
    // the same grouping at 16-bit resolution (representable while lg <= 7)
    bool repr = S <= 512;
    std::vector<int32_t> l3(65536, 0);
    {
      int run = 0, cur_share = -1;
      for (int t = 0; t < 512 && repr; t++) {
        if (lg[t] < 0) {
          int g;
          if (own) {  // (an empty bin: its run's group)
            g = (t == 0 || ct[t - 1]) ? run++ : run - 1;
          } else if (share[t] >= 0 && share[t] != cur_share) {
            cur_share = share[t];
            g = run++;
          } else {
            g = run > 0 ? run - 1 : 0;
          }
          for (int j = 0; j < 128; j++) l3[t * 128 + j] = g;
          continue;
        }
        if (lg[t] > 7) {
          repr = false;
          break;
        }
        for (int j = 0; j < 128; j++) l3[t * 128 + j] = run + (j >> (7 - lg[t]));
        run += 1 << lg[t];
      }
    }
    const double over3 = repr ? overflow(l3) : 1e300;
    const bool forced = force && *force;
    const bool early = !forced && repr && over3 == 0 &&
                       S - (own ? empty_runs : 0) >= 2 * buckets_used;
    if (!early && !plan_mode1()) return;
    const bool take3 = forced ? (*force == '3' && repr) : (early || (repr && over3 <= over_best));
    if (take3) {
      // entry t: first group (bits 0..15) | lg (16..23); shared and empty
      // bins: the group (lg 0)
      std::vector<int32_t> tab(512);
      std::vector<uint64_t> glo(kGroups, ~0ull), ghi(kGroups, 0);
      const int unit = kb - 9;  // key bits below the top 9
      for (int t = 0; t < 512; t++) {
        const uint64_t t0 = (uint64_t)t << unit;
        const int l = lg[t] < 0 ? 0 : lg[t];
        const int g0 = l3[t * 128];
        tab[t] = g0 | (l << 16);
        const int sub = unit - l;
        for (int j = 0; j < (1 << l); j++) {
          const uint64_t a0 = t0 + ((uint64_t)j << sub);
          glo[g0 + j] = std::min(glo[g0 + j], a0);
          ghi[g0 + j] = std::max(ghi[g0 + j], a0 + ((uint64_t(1) << sub) - 1));
        }
      }
      for (int g = 0; g < kGroups; g++) {
        if (glo[g] > ghi[g]) {
          rbits[g] = kb;  // (no keys)
          continue;
        }
        const uint64_t x = glo[g] ^ ghi[g];
        rbits[g] = x ? 64 - __builtin_clzll(x) : 0;
      }
      P->mode = 3;
      P->tab3 = tab;
      P->rbits = rbits;
      P->groups = S;
      P->over = over3;
      P->over_other = over_best;
      return;
    }
    P->over_other = over3;
  }
  P->mode = 1;
  P->lut16 = lut;
  P->rbits = rbits;
  P->groups = groups_used;
  P->over = over_best;
}

bool find_clusters(const std::vector<uint32_t>& h, std::vector<KeyCluster>* clusters) {
  clusters->clear();
  std::vector<KeyCluster> cl;
  bool ok = true;
  for (int b = 0; b < 65536 && ok; b++) {  // (stops at the first cluster too many or too wide)
    if (!h[b]) continue;
    if (cl.empty() || b - cl.back().b1 > kClusterGap) cl.push_back(KeyCluster{b, b, 0});
    cl.back().b1 = b;
    cl.back().cnt += h[b];
    ok = (int)cl.size() <= kMaxRanges && cl.back().b1 - cl.back().b0 < kClusterSpan;
  }
  if (ok) *clusters = cl;
  return ok;
}

void range_splits(const std::vector<KeyCluster>& cl, int key_bits, uint64_t hi[kMaxRanges]) {
  const int K = (int)cl.size();
  for (int c = 0; c < kMaxRanges; c++) hi[c] = ~0ull;
  for (int k = 0; k + 1 < K; k++) {  // split halfway between the sampled clusters
    const uint64_t mid_bin = ((uint64_t)cl[k].b1 + (uint64_t)cl[k + 1].b0 + 1) / 2;
    hi[k] = (mid_bin << (key_bits - 16)) - 1;
  }
}

void plan_ranges(const std::vector<KeyCluster>& cl, const uint64_t hi[kMaxRanges],
                 const uint64_t got[2 * kMaxRanges], int key_bits, RangePlan* P) {
  *P = RangePlan();
  const int kb = key_bits;
  const int K = (int)cl.size();
  // the non-empty ranges (a range's keys: u in (hi[c-1], hi[c]])
  struct Rg {
    uint64_t mn, mx, cnt, hi;
  };
  std::vector<Rg> rg;
  for (int c = 0; c < K; c++) {
    if (got[2 * c] > got[2 * c + 1]) continue;  // no key fell into this range
    rg.push_back(Rg{got[2 * c], got[2 * c + 1], std::max<uint64_t>(cl[c].cnt, 1), hi[c]});
  }
  if (rg.empty()) return;
  if (rg.size() == 1 && rg[0].mn == rg[0].mx) {
    P->one_value = true;
    return;
  }
  // one shift for every range: the smallest that fits all of them into the
  // level's buckets (ranges keep their order: dense bucket bases)
  const int R_ = (int)rg.size();
  auto shr = [](uint64_t x, int s) { return s >= 64 ? 0 : x >> s; };
  auto span = [&](int s) {
    uint64_t t = 0;
    for (const Rg& r : rg) t += shr(r.mx, s) - shr(r.mn, s) + 1;
    return t;
  };
  int s = 0;
  while (s < kb && span(s) > (uint64_t)kMaxBins) s++;
  uint32_t used = 0;
  for (int c = 0; c < kMaxRanges; c++) {
    P->rng_hi[c] = ~0ull;
    P->rng_adj[c] = 0;
  }
  for (int c = 0; c < R_; c++) {
    P->rng_hi[c] = c + 1 < R_ ? rg[c].hi : ~0ull;
    P->base[c] = (int)used;
    P->rng_adj[c] = used - (uint32_t)shr(rg[c].mn, s);  // (wrapping)
    used += (uint32_t)(shr(rg[c].mx, s) - shr(rg[c].mn, s) + 1);
    P->mn[c] = rg[c].mn;
    P->mx[c] = rg[c].mx;
  }
  P->nranges = R_;
  P->used = used;
  P->shift = s;
  P->use = true;
  P->final_lvl = s == 0;
}

}  // namespace srs
