// test_sort_rows.cpp — device::sort_rows of include/simd_sort/radix_sort.hpp
// on one small matrix with padded rows and two payload pairs, up and down,
// checked against std::stable_sort of every row on the host.
// usage: test_sort_rows [rows [row_len]]
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

template <bool Up>
static int run(int64_t rows, int64_t len) {
  const int64_t stride = len + 3, cells = rows * stride, recs = rows * len;
  std::vector<int32_t> keys(cells);
  std::vector<uint64_t> p0(cells);
  std::vector<uint16_t> p1(cells);
  for (int64_t i = 0; i < cells; i++) {
    keys[i] = (int32_t)(splitmix(i) % 2001) - 1000;  // many ties
    p0[i] = (uint64_t)i;
    p1[i] = (uint16_t)splitmix(i ^ 77);
  }
  int32_t *dk, *dko;
  uint64_t *dp0, *dp0o;
  uint16_t *dp1, *dp1o;
  CK(upload(keys, &dk));
  CK(upload(p0, &dp0));
  CK(upload(p1, &dp1));
  CK(hipMalloc((void**)&dko, recs * sizeof(int32_t)));
  CK(hipMalloc((void**)&dp0o, recs * sizeof(uint64_t)));
  CK(hipMalloc((void**)&dp1o, recs * sizeof(uint16_t)));
  dv::sort_rows<Up>(nullptr, rows, len, stride, (const int32_t*)dk, dko,
                    std::pair<const uint64_t*, uint64_t*>(dp0, dp0o),
                    std::pair<const uint16_t*, uint16_t*>(dp1, dp1o));
  CK(hipDeviceSynchronize());
  std::vector<int32_t> ko(recs);
  std::vector<uint64_t> p0o(recs);
  std::vector<uint16_t> p1o(recs);
  CK(hipMemcpy(ko.data(), dko, recs * sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(hipMemcpy(p0o.data(), dp0o, recs * sizeof(uint64_t), hipMemcpyDeviceToHost));
  CK(hipMemcpy(p1o.data(), dp1o, recs * sizeof(uint16_t), hipMemcpyDeviceToHost));
  std::vector<int64_t> order(len);
  for (int64_t r = 0; r < rows; r++) {
    std::iota(order.begin(), order.end(), r * stride);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
      return Up ? keys[a] < keys[b] : keys[a] > keys[b];
    });
    for (int64_t j = 0; j < len; j++) {
      const int64_t o = order[j], at = r * len + j;
      if (ko[at] != keys[o] || p0o[at] != p0[o] || p1o[at] != p1[o]) {
        fprintf(stderr, "up=%d: row %lld record %lld differs\n", (int)Up, (long long)r,
                (long long)j);
        return 1;
      }
    }
  }
  std::vector<int32_t> back(cells);
  CK(hipMemcpy(back.data(), dk, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (back != keys) {
    fprintf(stderr, "the input was written\n");
    return 1;
  }
  CK(hipFree(dk)); CK(hipFree(dp0)); CK(hipFree(dp1));
  CK(hipFree(dko)); CK(hipFree(dp0o)); CK(hipFree(dp1o));
  return 0;
}

int main(int argc, char** argv) {
  const int64_t rows = argc > 1 ? atoll(argv[1]) : 37;
  const int64_t len = argc > 2 ? atoll(argv[2]) : 1000;
  if (rows < 1 || len < 1) {
    fprintf(stderr, "usage: test_sort_rows [rows [row_len]]\n");
    return 2;
  }
  if (run<true>(rows, len) || run<false>(rows, len)) return 1;
  printf("sort_rows ok: rows=%lld row_len=%lld\n", (long long)rows, (long long)len);
  return 0;
}
