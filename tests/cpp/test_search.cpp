// test_search.cpp — both forms of device::search_sorted of
// include/simd_sort/radix_sort.hpp on a table of n float keys of a few hundred
// distinct values (-0.0 and +0.0 among them) and nq queries, up and down: the
// flat form with and without the hint, the segmented form over four segments
// with some bad segment ids; every bound checked against std::lower_bound and
// std::upper_bound on the transformed keys.
// usage: test_search [n [distinct [nq]]]
#include <hip/hip_runtime.h>
#include <simd_sort/radix_sort.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

template <bool Up>
static int run(int64_t n, int64_t distinct, int64_t nq) {
  std::vector<float> table(n), queries(nq);
  for (int64_t i = 0; i < n; i++) table[i] = value(splitmix(i), distinct);
  // queries: values of the table's law and values between them
  for (int64_t j = 0; j < nq; j++)
    queries[j] = value(splitmix(j ^ 0xABCDEF), distinct + 40) + ((j % 3) == 0 ? 0.25f : 0.0f);
  auto less = [](float x, float y) { return image<Up>(x) < image<Up>(y); };
  // four segments, each sorted on its own; the flat table is sorted whole
  const int64_t nseg = 4;
  const std::vector<int64_t> offs = {0, n / 5, n / 5, n / 2, n};
  std::vector<float> flat = table, ragged = table;
  std::sort(flat.begin(), flat.end(), less);
  for (int64_t s = 0; s < nseg; s++) std::sort(ragged.begin() + offs[s], ragged.begin() + offs[s + 1], less);
  std::vector<int64_t> qseg(nq);
  for (int64_t j = 0; j < nq; j++) qseg[j] = (int64_t)(splitmix(j * 31) % 6) - 1;  // -1 .. 4

  float *dflat, *dragged, *dq;
  int64_t *doffs, *dqseg, *dlo, *dhi, *dbad;
  const std::vector<int64_t> fill(nq, -7), one(1, -7);
  CK(upload(flat, &dflat));
  CK(upload(ragged, &dragged));
  CK(upload(queries, &dq));
  CK(upload(offs, &doffs));
  CK(upload(qseg, &dqseg));
  CK(upload(fill, &dlo));
  CK(upload(fill, &dhi));
  CK(upload(one, &dbad));
  std::vector<int64_t> lo(nq), hi(nq), bad(1);

  for (int hint = 0; hint < 2; hint++) {
    dv::search_sorted<Up>(nullptr, n, (const float*)dflat, nq, (const float*)dq, dlo, dhi,
                          hint ? SRS_SEARCH_QUERIES_SORTED : 0);
    CK(hipDeviceSynchronize());
    CK(download(lo, (const int64_t*)dlo));
    CK(download(hi, (const int64_t*)dhi));
    for (int64_t j = 0; j < nq; j++) {
      const int64_t wl = std::lower_bound(flat.begin(), flat.end(), queries[j], less) - flat.begin();
      const int64_t wh = std::upper_bound(flat.begin(), flat.end(), queries[j], less) - flat.begin();
      if (lo[j] != wl || hi[j] != wh) {
        fprintf(stderr, "up=%d hint=%d: query %lld gives [%lld, %lld), expected [%lld, %lld)\n",
                (int)Up, hint, (long long)j, (long long)lo[j], (long long)hi[j], (long long)wl,
                (long long)wh);
        return 1;
      }
    }
  }

  dv::search_sorted<Up>(nullptr, n, (const float*)dragged, nseg, (const int64_t*)doffs, nq,
                        (const float*)dq, (const int64_t*)dqseg, dlo, dhi, dbad);
  CK(hipDeviceSynchronize());
  CK(download(lo, (const int64_t*)dlo));
  CK(download(hi, (const int64_t*)dhi));
  CK(download(bad, (const int64_t*)dbad));
  int64_t want_bad = 0;
  for (int64_t j = 0; j < nq; j++) {
    int64_t wl = -1, wh = -1;
    const int64_t s = qseg[j];
    if (s >= 0 && s < nseg) {
      const auto b = ragged.begin() + offs[s], e = ragged.begin() + offs[s + 1];
      wl = std::lower_bound(b, e, queries[j], less) - b;
      wh = std::upper_bound(b, e, queries[j], less) - b;
    } else {
      want_bad++;
    }
    if (lo[j] != wl || hi[j] != wh) {
      fprintf(stderr, "up=%d segmented: query %lld of segment %lld gives [%lld, %lld), expected "
              "[%lld, %lld)\n", (int)Up, (long long)j, (long long)s, (long long)lo[j],
              (long long)hi[j], (long long)wl, (long long)wh);
      return 1;
    }
  }
  if (bad[0] != want_bad || want_bad == 0) {
    fprintf(stderr, "up=%d segmented: %lld bad queries counted, expected %lld\n", (int)Up,
            (long long)bad[0], (long long)want_bad);
    return 1;
  }
  std::vector<float> back(n);
  CK(download(back, (const float*)dflat));
  if (memcmp(back.data(), flat.data(), n * sizeof(float)) != 0) {
    fprintf(stderr, "the table was written\n");
    return 1;
  }
  CK(hipFree(dflat)); CK(hipFree(dragged)); CK(hipFree(dq)); CK(hipFree(doffs));
  CK(hipFree(dqseg)); CK(hipFree(dlo)); CK(hipFree(dhi)); CK(hipFree(dbad));
  return 0;
}

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 100000;
  const int64_t distinct = argc > 2 ? atoll(argv[2]) : 300;
  const int64_t nq = argc > 3 ? atoll(argv[3]) : 50000;
  if (n < 1 || distinct < 3 || nq < 1) {
    fprintf(stderr, "usage: test_search [n [distinct [nq]]]\n");
    return 2;
  }
  if (run<true>(n, distinct, nq) || run<false>(n, distinct, nq)) return 1;
  printf("search ok: n=%lld distinct=%lld queries=%lld\n", (long long)n, (long long)distinct,
         (long long)nq);
  return 0;
}
