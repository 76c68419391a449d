// test_sort_ragged.cpp — device::sort_ragged of include/simd_sort/radix_sort.hpp
// on segments of 0 .. max_len records plus one long segment, with a gap before
// the first and after the last, two payload pairs, up and down, every segment
// checked against std::stable_sort on the host.
// usage: test_sort_ragged [segments [max_len [long_len]]]
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
static int run(int64_t nseg, int64_t max_len, int64_t long_len) {
  const int64_t head = 5, tail = 9;
  std::vector<int64_t> offs(nseg + 2);
  offs[0] = head;
  for (int64_t s = 0; s <= nseg; s++) {
    const int64_t len = s == nseg / 2 ? long_len : (int64_t)(splitmix(s ^ 1234) % (max_len + 1));
    offs[s + 1] = offs[s] + len;
  }
  const int64_t segs = nseg + 1, num = offs[segs] + tail;
  std::vector<int32_t> keys(num);
  std::vector<uint64_t> p0(num);
  std::vector<uint16_t> p1(num);
  for (int64_t i = 0; i < num; i++) {
    keys[i] = (int32_t)(splitmix(i) % 2001) - 1000;  // many ties
    p0[i] = (uint64_t)i;
    p1[i] = (uint16_t)splitmix(i ^ 77);
  }
  const std::vector<int32_t> fill_k(num, 0x5A5A5A5A);
  int32_t *dk, *dko;
  uint64_t *dp0, *dp0o;
  uint16_t *dp1, *dp1o;
  int64_t *doffs, *didx;
  CK(upload(keys, &dk));
  CK(upload(p0, &dp0));
  CK(upload(p1, &dp1));
  CK(upload(offs, &doffs));
  CK(upload(fill_k, &dko));
  CK(hipMalloc((void**)&dp0o, num * sizeof(uint64_t)));
  CK(hipMalloc((void**)&dp1o, num * sizeof(uint16_t)));
  CK(hipMalloc((void**)&didx, num * sizeof(int64_t)));
  std::vector<int32_t> ko(num);
  std::vector<uint64_t> p0o(num);
  std::vector<uint16_t> p1o(num);
  std::vector<int64_t> idx(num);
  std::vector<int64_t> order;
  for (int with_idx = 0; with_idx < 2; with_idx++) {
    CK(hipMemcpy(dko, fill_k.data(), num * sizeof(int32_t), hipMemcpyHostToDevice));
    if (with_idx)
      dv::sort_ragged<Up>(nullptr, num, segs, (const int64_t*)doffs, (const int32_t*)dk, dko, didx,
                          std::pair<const uint64_t*, uint64_t*>(dp0, dp0o),
                          std::pair<const uint16_t*, uint16_t*>(dp1, dp1o));
    else
      dv::sort_ragged<Up>(nullptr, num, segs, (const int64_t*)doffs, (const int32_t*)dk, dko,
                          std::pair<const uint64_t*, uint64_t*>(dp0, dp0o),
                          std::pair<const uint16_t*, uint16_t*>(dp1, dp1o));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(ko.data(), dko, num * sizeof(int32_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(p0o.data(), dp0o, num * sizeof(uint64_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(p1o.data(), dp1o, num * sizeof(uint16_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(idx.data(), didx, num * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int64_t s = 0; s < segs; s++) {
      const int64_t a = offs[s], len = offs[s + 1] - a;
      order.resize(len);
      std::iota(order.begin(), order.end(), a);
      std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        return Up ? keys[x] < keys[y] : keys[x] > keys[y];
      });
      for (int64_t j = 0; j < len; j++) {
        const int64_t o = order[j], at = a + j;
        if (ko[at] != keys[o] || p0o[at] != p0[o] || p1o[at] != p1[o] ||
            (with_idx && idx[at] != o - a)) {
          fprintf(stderr, "up=%d indices=%d: segment %lld (len %lld) record %lld differs\n",
                  (int)Up, with_idx, (long long)s, (long long)len, (long long)j);
          return 1;
        }
      }
    }
    for (int64_t i = 0; i < num; i++) {
      if ((i < head || i >= offs[segs]) && ko[i] != 0x5A5A5A5A) {
        fprintf(stderr, "record %lld outside the segments was written\n", (long long)i);
        return 1;
      }
    }
  }
  std::vector<int32_t> back(num);
  CK(hipMemcpy(back.data(), dk, num * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (back != keys) {
    fprintf(stderr, "the input was written\n");
    return 1;
  }
  CK(hipFree(dk)); CK(hipFree(dp0)); CK(hipFree(dp1)); CK(hipFree(doffs)); CK(hipFree(didx));
  CK(hipFree(dko)); CK(hipFree(dp0o)); CK(hipFree(dp1o));
  return 0;
}

int main(int argc, char** argv) {
  const int64_t nseg = argc > 1 ? atoll(argv[1]) : 1000;
  const int64_t max_len = argc > 2 ? atoll(argv[2]) : 600;
  const int64_t long_len = argc > 3 ? atoll(argv[3]) : 9000;
  if (nseg < 1 || max_len < 0 || long_len < 0) {
    fprintf(stderr, "usage: test_sort_ragged [segments [max_len [long_len]]]\n");
    return 2;
  }
  if (run<true>(nseg, max_len, long_len) || run<false>(nseg, max_len, long_len)) return 1;
  printf("sort_ragged ok: segments=%lld max_len=%lld long_len=%lld\n", (long long)nseg,
         (long long)max_len, (long long)long_len);
  return 0;
}
