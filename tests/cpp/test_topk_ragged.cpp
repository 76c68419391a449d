// test_topk_ragged.cpp — device::top_k_ragged of include/simd_sort/radix_sort.hpp
// on segments of 0 .. max_len records plus one long segment, with a gap before
// the first and after the last, two payload pairs, up and down, with and
// without indices and counts, k = 10 (the kernels) and k = 3000 (the sort
// route); every segment's head checked against std::stable_sort on the host,
// every other output slot against the fill.
// usage: test_topk_ragged [segments [max_len [long_len]]]
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
static int run(int64_t nseg, int64_t max_len, int64_t long_len, int64_t k) {
  const int64_t head = 5, tail = 9;
  std::vector<int64_t> offs(nseg + 2);
  offs[0] = head;
  for (int64_t s = 0; s <= nseg; s++) {
    const int64_t len = s == nseg / 2 ? long_len : (int64_t)(splitmix(s ^ 1234) % (max_len + 1));
    offs[s + 1] = offs[s] + len;
  }
  const int64_t segs = nseg + 1, num = offs[segs] + tail, slots = segs * k;
  std::vector<int32_t> keys(num);
  std::vector<uint64_t> p0(num);
  std::vector<uint16_t> p1(num);
  for (int64_t i = 0; i < num; i++) {
    keys[i] = (int32_t)(splitmix(i) % 2001) - 1000;  // many ties
    p0[i] = (uint64_t)i;
    p1[i] = (uint16_t)splitmix(i ^ 77);
  }
  const std::vector<int32_t> fill_k(slots, 0x5A5A5A5A);
  const std::vector<uint64_t> fill_p0(slots, 0x5A5A5A5A5A5A5A5Aull);
  const std::vector<uint16_t> fill_p1(slots, 0x5A5A);
  const std::vector<int64_t> fill_idx(slots, -7), fill_cnt(segs, -7);
  int32_t *dk, *dko;
  uint64_t *dp0, *dp0o;
  uint16_t *dp1, *dp1o;
  int64_t *doffs, *didx, *dcnt;
  CK(upload(keys, &dk));
  CK(upload(p0, &dp0));
  CK(upload(p1, &dp1));
  CK(upload(offs, &doffs));
  CK(upload(fill_k, &dko));
  CK(upload(fill_p0, &dp0o));
  CK(upload(fill_p1, &dp1o));
  CK(upload(fill_idx, &didx));
  CK(upload(fill_cnt, &dcnt));
  std::vector<int32_t> ko(slots);
  std::vector<uint64_t> p0o(slots);
  std::vector<uint16_t> p1o(slots);
  std::vector<int64_t> idx(slots), cnt(segs);
  std::vector<int64_t> order;
  for (int with = 0; with < 2; with++) {  // with indices and counts, or neither
    CK(refill(dko, fill_k));
    CK(refill(dp0o, fill_p0));
    CK(refill(dp1o, fill_p1));
    CK(refill(didx, fill_idx));
    CK(refill(dcnt, fill_cnt));
    dv::top_k_ragged<Up>(nullptr, k, num, segs, (const int64_t*)doffs, (const int32_t*)dk, dko,
                         with ? didx : nullptr, with ? dcnt : nullptr,
                         std::pair<const uint64_t*, uint64_t*>(dp0, dp0o),
                         std::pair<const uint16_t*, uint16_t*>(dp1, dp1o));
    CK(hipDeviceSynchronize());
    CK(download(ko, dko));
    CK(download(p0o, dp0o));
    CK(download(p1o, dp1o));
    CK(download(idx, didx));
    CK(download(cnt, dcnt));
    for (int64_t s = 0; s < segs; s++) {
      const int64_t a = offs[s], len = offs[s + 1] - a, c = std::min(k, len);
      order.resize(len);
      std::iota(order.begin(), order.end(), a);
      std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        return Up ? keys[x] < keys[y] : keys[x] > keys[y];
      });
      if (cnt[s] != (with ? c : -7)) {
        fprintf(stderr, "up=%d k=%lld with=%d: count of segment %lld is %lld\n", (int)Up,
                (long long)k, with, (long long)s, (long long)cnt[s]);
        return 1;
      }
      for (int64_t j = 0; j < k; j++) {
        const int64_t at = s * k + j;
        bool ok;
        if (j < c) {
          const int64_t o = order[j];
          ok = ko[at] == keys[o] && p0o[at] == p0[o] && p1o[at] == p1[o] &&
               idx[at] == (with ? o - a : -7);
        } else {
          ok = ko[at] == fill_k[at] && p0o[at] == fill_p0[at] && p1o[at] == fill_p1[at] &&
               idx[at] == -7;
        }
        if (!ok) {
          fprintf(stderr, "up=%d k=%lld with=%d: segment %lld (len %lld) slot %lld differs\n",
                  (int)Up, (long long)k, with, (long long)s, (long long)len, (long long)j);
          return 1;
        }
      }
    }
  }
  std::vector<int32_t> back(num);
  CK(download(back, (const int32_t*)dk));
  if (back != keys) {
    fprintf(stderr, "the input was written\n");
    return 1;
  }
  CK(hipFree(dk)); CK(hipFree(dp0)); CK(hipFree(dp1)); CK(hipFree(doffs)); CK(hipFree(didx));
  CK(hipFree(dko)); CK(hipFree(dp0o)); CK(hipFree(dp1o)); CK(hipFree(dcnt));
  return 0;
}

int main(int argc, char** argv) {
  const int64_t nseg = argc > 1 ? atoll(argv[1]) : 1000;
  const int64_t max_len = argc > 2 ? atoll(argv[2]) : 600;
  const int64_t long_len = argc > 3 ? atoll(argv[3]) : 9000;
  if (nseg < 1 || max_len < 0 || long_len < 0) {
    fprintf(stderr, "usage: test_topk_ragged [segments [max_len [long_len]]]\n");
    return 2;
  }
  for (int64_t k : {10, 3000})
    if (run<true>(nseg, max_len, long_len, k) || run<false>(nseg, max_len, long_len, k)) return 1;
  printf("topk_ragged ok: segments=%lld max_len=%lld long_len=%lld\n", (long long)nseg,
         (long long)max_len, (long long)long_len);
  return 0;
}
