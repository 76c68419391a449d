// test_merge.cpp — both forms of device::merge of
// include/simd_sort/radix_sort.hpp on two sorted sets of na and nb float keys
// of a few hundred distinct values (-0.0 and +0.0 among them) with two
// payloads (8 and 2 bytes), up and down: the form with source_out and the
// form without; every output checked against std::stable_sort of A followed
// by B on the transformed keys.
// usage: test_merge [na [nb [distinct]]]
#include <hip/hip_runtime.h>
#include <simd_sort/radix_sort.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <tuple>
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

// the unsigned image of the float order (total order; descending: complemented)
template <bool Up>
static uint32_t image(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  const uint32_t u = (b & 0x80000000u) ? ~b : b ^ 0x80000000u;
  return Up ? u : ~u;
}

template <typename T>
static int upload(const std::vector<T>& h, T** d) {
  CK(hipMalloc((void**)d, std::max<size_t>(h.size(), 1) * sizeof(T)));
  CK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

template <typename T>
static int download(std::vector<T>& h, const T* d) {
  CK(hipMemcpy(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost));
  return 0;
}

static float value(uint64_t r, int64_t distinct) {
  const int64_t v = (int64_t)(r % (uint64_t)distinct);
  if (v == 0) return -0.0f;
  if (v == 1) return 0.0f;
  return (float)(v - distinct / 2) * 0.75f;
}

template <typename T>
static bool same(const std::vector<T>& x, const std::vector<T>& y) {
  return x.size() == y.size() && memcmp(x.data(), y.data(), x.size() * sizeof(T)) == 0;
}

template <bool Up>
static int run(int64_t na, int64_t nb, int64_t distinct) {
  const int64_t n = na + nb;
  auto less = [](float x, float y) { return image<Up>(x) < image<Up>(y); };
  // A followed by B: keys (each side sorted), an 8-byte and a 2-byte payload
  std::vector<float> keys(n);
  std::vector<uint64_t> p8(n);
  std::vector<uint16_t> p2(n);
  for (int64_t i = 0; i < n; i++) keys[i] = value(splitmix(i), distinct);
  std::sort(keys.begin(), keys.begin() + na, less);
  std::sort(keys.begin() + na, keys.end(), less);
  for (int64_t i = 0; i < n; i++) {
    p8[i] = splitmix(i ^ 0xABCDEF);
    p2[i] = (uint16_t)splitmix(i * 31);
  }
  std::vector<int64_t> order(n);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int64_t x, int64_t y) { return image<Up>(keys[x]) < image<Up>(keys[y]); });
  std::vector<float> wkeys(n);
  std::vector<uint64_t> w8(n);
  std::vector<uint16_t> w2(n);
  for (int64_t i = 0; i < n; i++) {
    wkeys[i] = keys[order[i]];
    w8[i] = p8[order[i]];
    w2[i] = p2[order[i]];
  }

  float *dkeys, *dkout;
  uint64_t *d8, *d8out;
  uint16_t *d2, *d2out;
  int64_t* dsrc;
  CK(upload(keys, &dkeys));
  CK(upload(p8, &d8));
  CK(upload(p2, &d2));
  const std::vector<float> fk(n, -7.0f);
  const std::vector<uint64_t> f8(n, 7);
  const std::vector<uint16_t> f2(n, 7);
  const std::vector<int64_t> fs(n, -7);
  CK(upload(fk, &dkout));
  CK(upload(f8, &d8out));
  CK(upload(f2, &d2out));
  CK(upload(fs, &dsrc));
  using P8 = std::tuple<const uint64_t*, const uint64_t*, uint64_t*>;
  using P2 = std::tuple<const uint16_t*, const uint16_t*, uint16_t*>;
  std::vector<float> gk(n);
  std::vector<uint64_t> g8(n);
  std::vector<uint16_t> g2(n);
  std::vector<int64_t> gs(n);

  for (int form = 0; form < 2; form++) {
    CK(hipMemcpy(dkout, fk.data(), n * sizeof(float), hipMemcpyHostToDevice));
    CK(hipMemcpy(d8out, f8.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
    CK(hipMemcpy(d2out, f2.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice));
    if (form == 0)
      dv::merge<Up>(nullptr, na, (const float*)dkeys, nb, (const float*)(dkeys + na), dkout, dsrc,
                    P8(d8, d8 + na, d8out), P2(d2, d2 + na, d2out));
    else
      dv::merge<Up>(nullptr, na, (const float*)dkeys, nb, (const float*)(dkeys + na), dkout,
                    P8(d8, d8 + na, d8out), P2(d2, d2 + na, d2out));
    CK(hipDeviceSynchronize());
    CK(download(gk, (const float*)dkout));
    CK(download(g8, (const uint64_t*)d8out));
    CK(download(g2, (const uint16_t*)d2out));
    CK(download(gs, (const int64_t*)dsrc));
    if (!same(gk, wkeys) || !same(g8, w8) || !same(g2, w2) || !same(gs, order)) {
      fprintf(stderr, "up=%d form=%d: keys %d, 8-byte payload %d, 2-byte payload %d, source %d\n",
              (int)Up, form, (int)same(gk, wkeys), (int)same(g8, w8), (int)same(g2, w2),
              (int)same(gs, order));
      return 1;
    }
  }
  std::vector<float> back(n);
  CK(download(back, (const float*)dkeys));
  if (!same(back, keys)) {
    fprintf(stderr, "the inputs were written\n");
    return 1;
  }
  CK(hipFree(dkeys)); CK(hipFree(d8)); CK(hipFree(d2)); CK(hipFree(dkout));
  CK(hipFree(d8out)); CK(hipFree(d2out)); CK(hipFree(dsrc));
  return 0;
}

int main(int argc, char** argv) {
  const int64_t na = argc > 1 ? atoll(argv[1]) : 100000;
  const int64_t nb = argc > 2 ? atoll(argv[2]) : 60000;
  const int64_t distinct = argc > 3 ? atoll(argv[3]) : 300;
  if (na < 1 || nb < 1 || distinct < 3) {
    fprintf(stderr, "usage: test_merge [na [nb [distinct]]]\n");
    return 2;
  }
  if (run<true>(na, nb, distinct) || run<false>(na, nb, distinct)) return 1;
  printf("merge ok: na=%lld nb=%lld distinct=%lld\n", (long long)na, (long long)nb,
         (long long)distinct);
  return 0;
}
