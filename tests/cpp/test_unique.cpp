// test_unique.cpp — device::unique of include/simd_sort/radix_sort.hpp on n
// records of a few hundred distinct keys with two payload pairs, up and down,
// with every optional output and with none; the sorted arrays, the indices,
// the unique keys, the offsets and the inverse checked against
// std::stable_sort plus a run scan on the host, the slots past U against the
// fill.
// usage: test_unique [n [distinct]]
#include <hip/hip_runtime.h>
#include <simd_sort/radix_sort.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#define CK(x)                                                               \
  do {                                                                      \
    int rc_ = (int)(x);                                                     \
    if (rc_ != 0) {                                                         \
      fprintf(stderr, "%s:%d %s -> %d\n", __FILE__, __LINE__, #x, rc_);     \
      return 1;                                                             \
    }                                                                       \
  } while (0)

namespace dv = simd_sort::radix_sort::device;

static uint64_t splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

template <typename T>
static int upload(const std::vector<T>& h, T** d) {
  CK(hipMalloc((void**)d, h.size() * sizeof(T)));
  CK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

template <typename T>
static int refill(T* d, const std::vector<T>& h) {
  CK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

template <typename T>
static int download(std::vector<T>& h, const T* d) {
  CK(hipMemcpy(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost));
  return 0;
}

template <bool Up>
static int run(int64_t n, int64_t distinct) {
  std::vector<int32_t> keys(n);
  std::vector<uint64_t> p0(n);
  std::vector<uint16_t> p1(n);
  for (int64_t i = 0; i < n; i++) {
    keys[i] = (int32_t)(splitmix(i) % (uint64_t)distinct) * 7 - 1000;
    p0[i] = (uint64_t)i * 3;
    p1[i] = (uint16_t)splitmix(i ^ 77);
  }
  // the expectation: the stable sort, then a scan of its runs
  std::vector<int64_t> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
    return Up ? keys[x] < keys[y] : keys[x] > keys[y];
  });
  std::vector<int32_t> want_u;
  std::vector<int64_t> want_offs, want_inv(n);
  for (int64_t j = 0; j < n; j++) {
    if (j == 0 || keys[order[j]] != keys[order[j - 1]]) {
      want_u.push_back(keys[order[j]]);
      want_offs.push_back(j);
    }
    want_inv[order[j]] = (int64_t)want_u.size() - 1;
  }
  want_offs.push_back(n);
  const int64_t U = (int64_t)want_u.size();

  const std::vector<int32_t> fill_k(n, 0x5A5A5A5A);
  const std::vector<uint64_t> fill_p0(n, 0x5A5A5A5A5A5A5A5Aull);
  const std::vector<uint16_t> fill_p1(n, 0x5A5A);
  const std::vector<int64_t> fill_i(n + 1, -7);
  int32_t *dk, *dks, *du;
  uint64_t *dp0, *dp0s;
  uint16_t *dp1, *dp1s;
  int64_t *doffs, *dinv, *didx;
  CK(upload(keys, &dk));
  CK(upload(p0, &dp0));
  CK(upload(p1, &dp1));
  CK(upload(fill_k, &dks));
  CK(upload(fill_k, &du));
  CK(upload(fill_p0, &dp0s));
  CK(upload(fill_p1, &dp1s));
  CK(upload(fill_i, &doffs));
  CK(upload(fill_i, &dinv));
  CK(upload(fill_i, &didx));
  std::vector<int32_t> ks(n), uq(n);
  std::vector<uint64_t> p0s(n);
  std::vector<uint16_t> p1s(n);
  std::vector<int64_t> offs(n + 1), inv(n + 1), idx(n + 1);
  for (int with = 0; with < 2; with++) {  // every optional output, or none
    CK(refill(du, fill_k));
    CK(refill(doffs, fill_i));
    CK(refill(dinv, fill_i));
    CK(refill(didx, fill_i));
    const simd_sort::SortIndex got =
        with ? dv::unique<Up>(nullptr, n, (const int32_t*)dk, du, doffs, dinv, dks, didx,
                              std::pair<const uint64_t*, uint64_t*>(dp0, dp0s),
                              std::pair<const uint16_t*, uint16_t*>(dp1, dp1s))
             : dv::unique<Up>(nullptr, n, (const int32_t*)dk, du, (int64_t*)nullptr,
                              (int64_t*)nullptr, (int32_t*)nullptr, (int64_t*)nullptr);
    CK(hipDeviceSynchronize());
    if ((int64_t)got != U) {
      fprintf(stderr, "up=%d with=%d: %lld unique keys, expected %lld\n", (int)Up, with,
              (long long)got, (long long)U);
      return 1;
    }
    CK(download(uq, (const int32_t*)du));
    CK(download(offs, (const int64_t*)doffs));
    CK(download(inv, (const int64_t*)dinv));
    CK(download(idx, (const int64_t*)didx));
    for (int64_t j = 0; j < n; j++) {
      if (uq[j] != (j < U ? want_u[j] : fill_k[j])) {
        fprintf(stderr, "up=%d with=%d: unique_out[%lld] differs\n", (int)Up, with, (long long)j);
        return 1;
      }
    }
    for (int64_t j = 0; j <= n; j++) {
      const int64_t wo = with && j <= U ? want_offs[j] : -7;
      const int64_t wi = with && j < n ? want_inv[j] : -7;
      const int64_t wx = with && j < n ? order[j] : -7;
      if (offs[j] != wo || inv[j] != wi || idx[j] != wx) {
        fprintf(stderr, "up=%d with=%d: offsets / inverse / indices slot %lld differs\n", (int)Up,
                with, (long long)j);
        return 1;
      }
    }
    if (!with) continue;
    CK(download(ks, (const int32_t*)dks));
    CK(download(p0s, (const uint64_t*)dp0s));
    CK(download(p1s, (const uint16_t*)dp1s));
    for (int64_t j = 0; j < n; j++) {
      const int64_t o = order[j];
      if (ks[j] != keys[o] || p0s[j] != p0[o] || p1s[j] != p1[o]) {
        fprintf(stderr, "up=%d: sorted record %lld differs\n", (int)Up, (long long)j);
        return 1;
      }
    }
  }
  std::vector<int32_t> back(n);
  CK(download(back, (const int32_t*)dk));
  if (back != keys) {
    fprintf(stderr, "the input was written\n");
    return 1;
  }
  CK(hipFree(dk)); CK(hipFree(dp0)); CK(hipFree(dp1)); CK(hipFree(dks)); CK(hipFree(du));
  CK(hipFree(dp0s)); CK(hipFree(dp1s)); CK(hipFree(doffs)); CK(hipFree(dinv)); CK(hipFree(didx));
  return 0;
}

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 100000;
  const int64_t distinct = argc > 2 ? atoll(argv[2]) : 300;
  if (n < 1 || distinct < 1) {
    fprintf(stderr, "usage: test_unique [n [distinct]]\n");
    return 2;
  }
  if (run<true>(n, distinct) || run<false>(n, distinct)) return 1;
  printf("unique ok: n=%lld distinct=%lld\n", (long long)n, (long long)distinct);
  return 0;
}
