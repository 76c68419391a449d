// test_topk.cpp — device::top_k of include/simd_sort/radix_sort.hpp, both
// forms (separate arrays with payload pairs, DataElement records), up and
// down, checked against std::stable_sort of the same data on the host.
// usage: test_topk [n [k]]
#include <hip/hip_runtime.h>
#include <simd_sort/radix_sort.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

template <bool Up>
static int run_separate(int64_t n, int64_t k) {
  std::vector<int32_t> keys(n);
  std::vector<uint64_t> p0(n);
  std::vector<uint16_t> p1(n);
  for (int64_t i = 0; i < n; i++) {
    keys[i] = (int32_t)(splitmix(i) % 2001) - 1000;  // many ties
    p0[i] = (uint64_t)i;
    p1[i] = (uint16_t)splitmix(i ^ 77);
  }
  std::vector<int64_t> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
    return Up ? keys[a] < keys[b] : keys[a] > keys[b];
  });
  int32_t *dk, *dko;
  uint64_t *dp0, *dp0o;
  uint16_t *dp1, *dp1o;
  CK(upload(keys, &dk));
  CK(upload(p0, &dp0));
  CK(upload(p1, &dp1));
  CK(hipMalloc((void**)&dko, k * sizeof(int32_t)));
  CK(hipMalloc((void**)&dp0o, k * sizeof(uint64_t)));
  CK(hipMalloc((void**)&dp1o, k * sizeof(uint16_t)));
  dv::top_k<Up>(nullptr, k, n, (const int32_t*)dk, dko,
                std::pair<const uint64_t*, uint64_t*>(dp0, dp0o),
                std::pair<const uint16_t*, uint16_t*>(dp1, dp1o));
  CK(hipDeviceSynchronize());
  std::vector<int32_t> ko(k);
  std::vector<uint64_t> p0o(k);
  std::vector<uint16_t> p1o(k);
  CK(hipMemcpy(ko.data(), dko, k * sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(hipMemcpy(p0o.data(), dp0o, k * sizeof(uint64_t), hipMemcpyDeviceToHost));
  CK(hipMemcpy(p1o.data(), dp1o, k * sizeof(uint16_t), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < k; i++) {
    const int64_t o = order[i];
    if (ko[i] != keys[o] || p0o[i] != p0[o] || p1o[i] != p1[o]) {
      fprintf(stderr, "separate up=%d: record %lld differs\n", (int)Up, (long long)i);
      return 1;
    }
  }
  std::vector<int32_t> back(n);
  CK(hipMemcpy(back.data(), dk, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (back != keys) {
    fprintf(stderr, "separate: the input was written\n");
    return 1;
  }
  CK(hipFree(dk)); CK(hipFree(dp0)); CK(hipFree(dp1));
  CK(hipFree(dko)); CK(hipFree(dp0o)); CK(hipFree(dp1o));
  return 0;
}

template <bool Up>
static int run_combined(int64_t n, int64_t k) {
  using E = simd_sort::DataElement<double, uint32_t, uint32_t>;
  static_assert(sizeof(E) == 16, "record layout");
  std::vector<E> el(n);
  for (int64_t i = 0; i < n; i++) {
    el[i].key = (double)((int64_t)(splitmix(i * 3) % 4001) - 2000) * 0.25;
    std::get<0>(el[i].payloads) = (uint32_t)i;
    std::get<1>(el[i].payloads) = (uint32_t)splitmix(i);
  }
  std::vector<E> want = el;
  std::stable_sort(want.begin(), want.end(), [](const E& a, const E& b) {
    return Up ? a.key < b.key : a.key > b.key;
  });
  E *d, *dout;
  CK(hipMalloc((void**)&d, n * sizeof(E)));
  CK(hipMemcpy(d, el.data(), n * sizeof(E), hipMemcpyHostToDevice));
  CK(hipMalloc((void**)&dout, k * sizeof(E)));
  dv::top_k<Up>(nullptr, k, n, (const E*)d, dout);
  CK(hipDeviceSynchronize());
  std::vector<E> got(k);
  CK(hipMemcpy((void*)got.data(), dout, k * sizeof(E), hipMemcpyDeviceToHost));
  if (memcmp((const void*)got.data(), (const void*)want.data(), k * sizeof(E)) != 0) {
    fprintf(stderr, "combined up=%d: records differ\n", (int)Up);
    return 1;
  }
  CK(hipFree(d));
  CK(hipFree(dout));
  return 0;
}

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 10000;
  const int64_t k = argc > 2 ? atoll(argv[2]) : 100;
  if (n < 1 || k < 1 || k > n) {
    fprintf(stderr, "usage: test_topk [n [k <= n]]\n");
    return 2;
  }
  if (run_separate<true>(n, k) || run_separate<false>(n, k)) return 1;
  if (run_combined<true>(n, k) || run_combined<false>(n, k)) return 1;
  printf("top_k ok: n=%lld k=%lld\n", (long long)n, (long long)k);
  return 0;
}
