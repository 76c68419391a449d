// simd_sort/radix_sort.hpp — drop-in replacement for jonicho/simd-radix-sort's
// radixSort.hpp on AMD Instinct MI355X.
//
// Same namespace, same overloads, same semantics as the reference
// (radixSort.hpp:1761-1783, src/radix_sort.hpp:297-337):
//
//   simd_sort::radix_sort::sort(num, keyArray, payloadArrays...);
//   simd_sort::radix_sort::sort<false>(num, keyArray, payloadArrays...);
//   simd_sort::radix_sort::sort(num, (simd_sort::DataElement<K, Ps...>*) combined);
//   simd_sort::radix_sort::sort<Up, BitSorter, CmpSorter>(cmpSortThreshold, num, ...);
//   simd_sort::radix_sort::sort(cmpSortThreshold, num, ...);   // defaulted, :1761-1763
//
// BitSorter may be spelled as in radixSort.hpp (`BitSorterSIMD`, a plain
// name) or as in src/radix_sort.hpp:109 (`BitSorterSIMD<>`,
// `BitSorterSIMD<false>`, `BitSorterSIMD<true>` = OneReg).
//
// The arrays are sorted in place. Instead of the AVX-512 partition the work
// runs as HIP kernels on the GPU through the C ABI in srs_c_api.h
// (link with -lsrs_amd). Unlike the reference this header needs no AVX-512
// and compiles with any C++17 compiler.
//
// Error behaviour: the reference returns void and cannot fail at run time;
// unsupported type combinations fail at compile time (static_assert), as
// there. A run-time failure of the GPU path (no device, out of memory)
// prints the library's message and calls std::abort(): there is no silent
// CPU fallback.
#pragma once

#include <sys/types.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>

#include "../srs_c_api.h"

namespace simd_sort {

// src/common.hpp:14
using SortIndex = ssize_t;

// src/common.hpp:105-106
template <std::size_t X>
inline constexpr bool is_power_of_two = X > 0 && (X & (X - 1)) == 0;

// Combined key + payload element, layout-identical to the reference's
// (radixSort.hpp:180-195): the key at offset 0, payloads in a std::tuple.
template <typename K, typename... Ps>
struct DataElement {
  K key;
  std::tuple<Ps...> payloads;
  bool operator<(const DataElement& other) const { return key < other.key; }
  bool operator>(const DataElement& other) const { return key > other.key; }
};

template <typename K>
struct DataElement<K> {
  K key;
  bool operator<(const DataElement& other) const { return key < other.key; }
  bool operator>(const DataElement& other) const { return key > other.key; }
};

// Leaf sorter selectors. The reference's CmpSorterInsertionSort
// (radixSort.hpp:159-178) becomes the GPU's LDS-resident leaf; the name is
// kept so that existing call sites compile unchanged.
struct CmpSorterInsertionSort {};
// src/cmp_sorters.hpp:66-78: the recursion stops at leaves of <=
// cmpSortThreshold elements and leaves them in partition order, so each
// element ends within cmpSortThreshold of its sorted position (thesis
// 3113-3124). On the GPU the local pass skips its in-bucket rank when every
// bucket holds <= cmpSortThreshold keys (SRS_LEAF_UNSORTED); every leaf holds
// exactly the elements a full sort puts there. The order inside a leaf is
// unspecified and may differ between runs.
struct CmpSorterNoSort {};
// src/cmp_sorters.hpp:40-63 (needs the vendored bramas sorters there): the
// leaves are sorted (as here); the reference's type restrictions are kept
// as compile-time errors below.
struct CmpSorterBramasSmallSort {};

namespace radix_sort {

// Bit-sorter selectors. src/radix_sort.hpp:109 declares
// `template <bool OneReg = false> struct BitSorterSIMD` (OneReg: one
// register per payload vector, :119-121); radixSort.hpp:1583 has the plain
// `struct BitSorterSIMD`. Here it is the class template, and the sort()
// overloads below also take the template itself as a template-template
// argument, so both spellings compile. BitSorterSequential is
// src/radix_sort.hpp:66. All produce the same key order; on the GPU all run
// the same multi-bit digit passes.
template <bool OneReg = false>
struct BitSorterSIMD {
  static std::string name() { return OneReg ? "BitSorterSIMD<OneReg>" : "BitSorterSIMD"; }
};
struct BitSorterSequential {
  static std::string name() { return "BitSorterSequential"; }
};

namespace detail {

template <typename K>
constexpr int key_kind() {
  if constexpr (std::is_same_v<K, uint8_t>) return SRS_KEY_U8;
  else if constexpr (std::is_same_v<K, int8_t>) return SRS_KEY_I8;
  else if constexpr (std::is_same_v<K, uint16_t>) return SRS_KEY_U16;
  else if constexpr (std::is_same_v<K, int16_t>) return SRS_KEY_I16;
  else if constexpr (std::is_same_v<K, uint32_t>) return SRS_KEY_U32;
  else if constexpr (std::is_same_v<K, int32_t>) return SRS_KEY_I32;
  else if constexpr (std::is_same_v<K, uint64_t>) return SRS_KEY_U64;
  else if constexpr (std::is_same_v<K, int64_t>) return SRS_KEY_I64;
  else if constexpr (std::is_same_v<K, float>) return SRS_KEY_F32;
  else if constexpr (std::is_same_v<K, double>) return SRS_KEY_F64;
  else if constexpr (std::is_same_v<K, char> && std::is_signed_v<char>) return SRS_KEY_I8;
  else if constexpr (std::is_same_v<K, char>) return SRS_KEY_U8;
  else if constexpr (std::is_same_v<K, long> && sizeof(long) == 8) return SRS_KEY_I64;
  else if constexpr (std::is_same_v<K, unsigned long> && sizeof(long) == 8) return SRS_KEY_U64;
  else if constexpr (std::is_same_v<K, long long>) return SRS_KEY_I64;
  else if constexpr (std::is_same_v<K, unsigned long long>) return SRS_KEY_U64;
  else return -1;
}

template <typename CmpSorter>
inline constexpr bool known_cmp_sorter = std::is_same_v<CmpSorter, CmpSorterInsertionSort> ||
                                         std::is_same_v<CmpSorter, CmpSorterNoSort> ||
                                         std::is_same_v<CmpSorter, CmpSorterBramasSmallSort>;

template <typename CmpSorter>
inline constexpr int leaf_mode =
    std::is_same_v<CmpSorter, CmpSorterNoSort> ? SRS_LEAF_UNSORTED : SRS_LEAF_SORTED;

template <typename BitSorter>
inline constexpr bool known_bit_sorter = std::is_same_v<BitSorter, BitSorterSIMD<false>> ||
                                         std::is_same_v<BitSorter, BitSorterSIMD<true>> ||
                                         std::is_same_v<BitSorter, BitSorterSequential>;

// src/cmp_sorters.hpp:47-61
template <bool Up, typename CmpSorter, typename K, typename... Ps>
constexpr void check_cmp_sorter() {
  static_assert(known_cmp_sorter<CmpSorter>,
                "CmpSorter must be CmpSorterInsertionSort, CmpSorterNoSort or "
                "CmpSorterBramasSmallSort (a user-defined leaf sorter cannot run on the GPU)");
  if constexpr (std::is_same_v<CmpSorter, CmpSorterBramasSmallSort>) {
    static_assert(std::is_same_v<K, double> || std::is_same_v<K, int>,
                  "BramasSmallSort only supports int and double");
    static_assert(Up, "BramasSmallSort only supports sorting up");
    static_assert(sizeof...(Ps) <= 1, "BramasSmallSort only supports one or zero payloads");
    static_assert(((std::is_same_v<K, Ps>) && ...), "key and payload must have the same type");
  }
}

template <typename T>
inline constexpr bool valid_payload =
    std::is_trivially_copyable_v<T> &&
    (sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8);

inline void check(int rc, const char* what) {
  if (rc != SRS_OK) {
    std::fprintf(stderr, "simd_sort::radix_sort::%s failed (%d): %s\n", what, rc,
                 srs_last_error());
    std::abort();
  }
}

}  // namespace detail

// sort(cmpSortThreshold, num, keys, payloads...) — radixSort.hpp:1761-1768
// (defaults as there: Up = true, BitSorterSIMD, CmpSorterInsertionSort)
template <bool Up = true, typename BitSorter = BitSorterSIMD<>,
          typename CmpSorter = CmpSorterInsertionSort, typename K, typename... Ps>
void sort(SortIndex cmpSortThreshold, const SortIndex num, K* const keys,
          Ps* const... payloads) {
  static_assert(detail::known_bit_sorter<BitSorter>,
                "BitSorter must be BitSorterSIMD or BitSorterSequential");
  detail::check_cmp_sorter<Up, CmpSorter, K, Ps...>();
  static_assert(detail::key_kind<K>() >= 0,
                "key type must be one of u8/i8/u16/i16/u32/i32/u64/i64/float/double");
  static_assert((detail::valid_payload<Ps> && ...),
                "payload element sizes must be 1, 2, 4 or 8 bytes");
  static_assert(sizeof...(Ps) <= SRS_MAX_PAYLOADS, "too many payload arrays");
  void* pays[sizeof...(Ps) + 1] = {(void*)payloads..., nullptr};
  uint32_t sizes[sizeof...(Ps) + 1] = {(uint32_t)sizeof(Ps)..., 0};
  detail::check(srs_sort_soa_leaf((int64_t)num, detail::key_kind<K>(), Up ? 1 : 0,
                                  (int64_t)cmpSortThreshold, detail::leaf_mode<CmpSorter>,
                                  (void*)keys, (int32_t)sizeof...(Ps), pays, sizes),
                "sort");
}

// sort(cmpSortThreshold, num, DataElement<K, Ps...>*) — radixSort.hpp:1770-1778
// (the reference also reaches it through the defaulted SoA form with
// K = DataElement; partial ordering picks this overload for both)
template <bool Up = true, typename BitSorter = BitSorterSIMD<>,
          typename CmpSorter = CmpSorterInsertionSort, typename K, typename... Ps>
void sort(SortIndex cmpSortThreshold, const SortIndex num,
          DataElement<K, Ps...>* const elements) {
  static_assert(detail::known_bit_sorter<BitSorter>,
                "BitSorter must be BitSorterSIMD or BitSorterSequential");
  static_assert(detail::known_cmp_sorter<CmpSorter>,
                "CmpSorter must be CmpSorterInsertionSort, CmpSorterNoSort or "
                "CmpSorterBramasSmallSort (a user-defined leaf sorter cannot run on the GPU)");
  static_assert(is_power_of_two<sizeof(DataElement<K, Ps...>)>,
                "size of DataElement<K, Ps...> must be a power of two");
  static_assert(sizeof(DataElement<K, Ps...>) <= 64, "DataElement larger than 64 bytes");
  static_assert(detail::key_kind<K>() >= 0,
                "key type must be one of u8/i8/u16/i16/u32/i32/u64/i64/float/double");
  detail::check(srs_sort_aos_leaf((int64_t)num, detail::key_kind<K>(), Up ? 1 : 0,
                                  (int64_t)cmpSortThreshold, detail::leaf_mode<CmpSorter>,
                                  (void*)elements, (uint32_t)sizeof(DataElement<K, Ps...>)),
                "sort");
}

// The radixSort.hpp spelling sort<Up, BitSorterSIMD, CmpSorter>(...): the
// bit sorter named without template arguments (radixSort.hpp:1583, 1764).
template <bool Up, template <bool> class BitSorter, typename CmpSorter = CmpSorterInsertionSort,
          typename K, typename... Ps>
void sort(SortIndex cmpSortThreshold, const SortIndex num, K* const keys,
          Ps* const... payloads) {
  sort<Up, BitSorter<false>, CmpSorter>(cmpSortThreshold, num, keys, payloads...);
}

template <bool Up, template <bool> class BitSorter, typename CmpSorter = CmpSorterInsertionSort,
          typename K, typename... Ps>
void sort(SortIndex cmpSortThreshold, const SortIndex num,
          DataElement<K, Ps...>* const elements) {
  sort<Up, BitSorter<false>, CmpSorter>(cmpSortThreshold, num, elements);
}

// sort<Up>(num, keys, payloads...) — radixSort.hpp:1780-1783 (threshold 16)
template <bool Up = true, typename K, typename... Ps>
void sort(const SortIndex num, K* const keys, Ps* const... payloads) {
  sort<Up, BitSorterSIMD<>, CmpSorterInsertionSort>(16, num, keys, payloads...);
}

// ---- device-resident extension (no reference counterpart) ----------------
// Same semantics on arrays already in HBM, enqueued on `stream` (a
// hipStream_t, nullptr = default stream).
namespace device {

template <bool Up = true, typename K, typename... Ps>
void sort(void* stream, const SortIndex num, K* const keys, Ps* const... payloads) {
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  static_assert((detail::valid_payload<Ps> && ...), "payload sizes must be 1, 2, 4 or 8");
  void* pays[sizeof...(Ps) + 1] = {(void*)payloads..., nullptr};
  uint32_t sizes[sizeof...(Ps) + 1] = {(uint32_t)sizeof(Ps)..., 0};
  detail::check(srs_sort_soa_device((int64_t)num, detail::key_kind<K>(), Up ? 1 : 0, 16,
                                    (void*)keys, (int32_t)sizeof...(Ps), pays, sizes, nullptr,
                                    nullptr, stream),
                "device::sort");
}

template <bool Up = true, typename K, typename... Ps>
void sort(void* stream, const SortIndex num, DataElement<K, Ps...>* const elements) {
  static_assert(is_power_of_two<sizeof(DataElement<K, Ps...>)>,
                "size of DataElement<K, Ps...> must be a power of two");
  detail::check(srs_sort_aos_device((int64_t)num, detail::key_kind<K>(), Up ? 1 : 0, 16,
                                    (void*)elements, (uint32_t)sizeof(DataElement<K, Ps...>),
                                    nullptr, stream),
                "device::sort");
}

// top_k: the first min(k, num) records of the stable sort of the input
// (srs_topk_soa_device: Up the k smallest ascending, !Up the k largest
// descending, equal keys in input order), written to keys_out and to the
// second array of every payload pair {payload, payload_out}. The inputs are
// not written; the outputs must not overlap them.
template <bool Up = true, typename K, typename... Ps>
void top_k(void* stream, const SortIndex k, const SortIndex num, const K* const keys,
           K* const keys_out, std::pair<const Ps*, Ps*>... payloads) {
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  static_assert((detail::valid_payload<Ps> && ...), "payload sizes must be 1, 2, 4 or 8");
  static_assert(sizeof...(Ps) <= SRS_MAX_PAYLOADS, "too many payload arrays");
  const void* pays[sizeof...(Ps) + 1] = {(const void*)payloads.first..., nullptr};
  void* pays_out[sizeof...(Ps) + 1] = {(void*)payloads.second..., nullptr};
  uint32_t sizes[sizeof...(Ps) + 1] = {(uint32_t)sizeof(Ps)..., 0};
  detail::check(srs_topk_soa_device((int64_t)num, (int64_t)k, detail::key_kind<K>(), Up ? 1 : 0,
                                    (const void*)keys, (int32_t)sizeof...(Ps), pays, sizes,
                                    (void*)keys_out, pays_out, nullptr, stream),
                "device::top_k");
}

template <bool Up = true, typename K, typename... Ps>
void top_k(void* stream, const SortIndex k, const SortIndex num,
           const DataElement<K, Ps...>* const elements, DataElement<K, Ps...>* const elements_out) {
  static_assert(is_power_of_two<sizeof(DataElement<K, Ps...>)>,
                "size of DataElement<K, Ps...> must be a power of two");
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  detail::check(srs_topk_aos_device((int64_t)num, (int64_t)k, detail::key_kind<K>(), Up ? 1 : 0,
                                    (const void*)elements, (uint32_t)sizeof(DataElement<K, Ps...>),
                                    (void*)elements_out, nullptr, stream),
                "device::top_k");
}

// top_k_rows: top_k on every row of a matrix in one call
// (srs_topk_rows_soa_device). Record i of row r of every input array is at
// [r * row_stride + i] (row_stride >= row_len, in records); result j of row r
// at [r * min(k, row_len) + j] of keys_out and of every payload_out.
template <bool Up = true, typename K, typename... Ps>
void top_k_rows(void* stream, const SortIndex k, const SortIndex rows, const SortIndex row_len,
                const SortIndex row_stride, const K* const keys, K* const keys_out,
                std::pair<const Ps*, Ps*>... payloads) {
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  static_assert((detail::valid_payload<Ps> && ...), "payload sizes must be 1, 2, 4 or 8");
  static_assert(sizeof...(Ps) <= SRS_MAX_PAYLOADS, "too many payload arrays");
  const void* pays[sizeof...(Ps) + 1] = {(const void*)payloads.first..., nullptr};
  void* pays_out[sizeof...(Ps) + 1] = {(void*)payloads.second..., nullptr};
  uint32_t sizes[sizeof...(Ps) + 1] = {(uint32_t)sizeof(Ps)..., 0};
  detail::check(srs_topk_rows_soa_device((int64_t)rows, (int64_t)row_len, (int64_t)row_stride,
                                         (int64_t)k, detail::key_kind<K>(), Up ? 1 : 0,
                                         (const void*)keys, (int32_t)sizeof...(Ps), pays, sizes,
                                         (void*)keys_out, pays_out, nullptr, stream),
                "device::top_k_rows");
}

// sort_rows: every row of a matrix sorted in one call, out of place
// (srs_sort_rows_soa_device). Record i of row r of every input array is at
// [r * row_stride + i] (row_stride >= row_len, in records); record j of row
// r's stable sort at [r * row_len + j] of keys_out and of every payload_out.
template <bool Up = true, typename K, typename... Ps>
void sort_rows(void* stream, const SortIndex rows, const SortIndex row_len,
               const SortIndex row_stride, const K* const keys, K* const keys_out,
               std::pair<const Ps*, Ps*>... payloads) {
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  static_assert((detail::valid_payload<Ps> && ...), "payload sizes must be 1, 2, 4 or 8");
  static_assert(sizeof...(Ps) <= SRS_MAX_PAYLOADS, "too many payload arrays");
  const void* pays[sizeof...(Ps) + 1] = {(const void*)payloads.first..., nullptr};
  void* pays_out[sizeof...(Ps) + 1] = {(void*)payloads.second..., nullptr};
  uint32_t sizes[sizeof...(Ps) + 1] = {(uint32_t)sizeof(Ps)..., 0};
  detail::check(srs_sort_rows_soa_device((int64_t)rows, (int64_t)row_len, (int64_t)row_stride,
                                         detail::key_kind<K>(), Up ? 1 : 0, (const void*)keys,
                                         (int32_t)sizeof...(Ps), pays, sizes, (void*)keys_out,
                                         pays_out, nullptr, stream),
                "device::sort_rows");
}

// sort_ragged: every segment [offsets[i], offsets[i + 1]) of dense arrays of
// num records sorted in one call, out of place (srs_sort_ragged_soa_device).
// offsets: num_segments + 1 non-decreasing int64 values in DEVICE memory,
// within [0, num]; record j of segment i's stable sort lands at
// [offsets[i] + j] of keys_out and of every payload_out. The second form
// also writes every record's position inside its segment to indices_out.
template <bool Up = true, typename K, typename... Ps>
void sort_ragged(void* stream, const SortIndex num, const SortIndex num_segments,
                 const int64_t* const offsets, const K* const keys, K* const keys_out,
                 int64_t* const indices_out, std::pair<const Ps*, Ps*>... payloads) {
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  static_assert((detail::valid_payload<Ps> && ...), "payload sizes must be 1, 2, 4 or 8");
  static_assert(sizeof...(Ps) <= SRS_MAX_PAYLOADS, "too many payload arrays");
  const void* pays[sizeof...(Ps) + 1] = {(const void*)payloads.first..., nullptr};
  void* pays_out[sizeof...(Ps) + 1] = {(void*)payloads.second..., nullptr};
  uint32_t sizes[sizeof...(Ps) + 1] = {(uint32_t)sizeof(Ps)..., 0};
  detail::check(srs_sort_ragged_soa_device((int64_t)num, (int64_t)num_segments, offsets,
                                           detail::key_kind<K>(), Up ? 1 : 0, (const void*)keys,
                                           (int32_t)sizeof...(Ps), pays, sizes, (void*)keys_out,
                                           pays_out, indices_out, stream),
                "device::sort_ragged");
}
template <bool Up = true, typename K, typename... Ps>
void sort_ragged(void* stream, const SortIndex num, const SortIndex num_segments,
                 const int64_t* const offsets, const K* const keys, K* const keys_out,
                 std::pair<const Ps*, Ps*>... payloads) {
  sort_ragged<Up>(stream, num, num_segments, offsets, keys, keys_out, (int64_t*)nullptr,
                  payloads...);
}

// top_k_ragged: the first min(k, len) records of every segment [offsets[i],
// offsets[i + 1]) of dense arrays of num records in one call
// (srs_topk_ragged_soa_device). offsets is sort_ragged's; result j of
// segment i lands at [i * k + j] of keys_out, of every payload_out and of
// indices_out (positions inside the segment; may be null), slots from
// min(k, len) on are not written; counts_out (device, num_segments entries;
// may be null) receives min(k, len) per segment.
template <bool Up = true, typename K, typename... Ps>
void top_k_ragged(void* stream, const SortIndex k, const SortIndex num,
                  const SortIndex num_segments, const int64_t* const offsets,
                  const K* const keys, K* const keys_out, int64_t* const indices_out,
                  int64_t* const counts_out, std::pair<const Ps*, Ps*>... payloads) {
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  static_assert((detail::valid_payload<Ps> && ...), "payload sizes must be 1, 2, 4 or 8");
  static_assert(sizeof...(Ps) <= SRS_MAX_PAYLOADS, "too many payload arrays");
  const void* pays[sizeof...(Ps) + 1] = {(const void*)payloads.first..., nullptr};
  void* pays_out[sizeof...(Ps) + 1] = {(void*)payloads.second..., nullptr};
  uint32_t sizes[sizeof...(Ps) + 1] = {(uint32_t)sizeof(Ps)..., 0};
  detail::check(srs_topk_ragged_soa_device((int64_t)num, (int64_t)num_segments, offsets,
                                           (int64_t)k, detail::key_kind<K>(), Up ? 1 : 0,
                                           (const void*)keys, (int32_t)sizeof...(Ps), pays, sizes,
                                           (void*)keys_out, pays_out, indices_out, counts_out,
                                           stream),
                "device::top_k_ragged");
}

// unique: the distinct keys of an array, where each group of equal keys
// starts and which group every record fell into, in one call
// (srs_unique_soa_device). With S the stable sort of the input and U its
// number of runs of equal keys: unique_out[0, U) receives every run's first
// key (num slots), offsets_out[0, U] every run's start in S and num (num + 1
// slots; sort_ragged's and top_k_ragged's offsets over the sorted arrays),
// inverse_out[i] the run number of input record i, keys_sorted_out and every
// payload's second array S itself, indices_out S's input positions. All but
// unique_out may be null (keys_sorted_out and the payload outputs together;
// null only without payloads). Returns U, after one read-back behind the
// call's kernels.
template <bool Up = true, typename K, typename... Ps>
SortIndex unique(void* stream, const SortIndex num, const K* const keys, K* const unique_out,
                 int64_t* const offsets_out, int64_t* const inverse_out,
                 K* const keys_sorted_out, int64_t* const indices_out,
                 std::pair<const Ps*, Ps*>... payloads) {
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  static_assert((detail::valid_payload<Ps> && ...), "payload sizes must be 1, 2, 4 or 8");
  static_assert(sizeof...(Ps) <= SRS_MAX_PAYLOADS, "too many payload arrays");
  const void* pays[sizeof...(Ps) + 1] = {(const void*)payloads.first..., nullptr};
  void* pays_out[sizeof...(Ps) + 1] = {(void*)payloads.second..., nullptr};
  uint32_t sizes[sizeof...(Ps) + 1] = {(uint32_t)sizeof(Ps)..., 0};
  int64_t num_unique = 0;
  detail::check(srs_unique_soa_device((int64_t)num, detail::key_kind<K>(), Up ? 1 : 0,
                                      (const void*)keys, (int32_t)sizeof...(Ps), pays, sizes,
                                      (void*)keys_sorted_out,
                                      keys_sorted_out ? pays_out : nullptr, indices_out,
                                      (void*)unique_out, offsets_out, inverse_out, nullptr,
                                      &num_unique, stream),
                "device::unique");
  return (SortIndex)num_unique;
}

// search_sorted: the lower and upper bounds of query keys in a sorted array
// (srs_search_sorted_device), in the sort's key order (Up = false: an array
// sorted descending; floats in the total order). lower_out[j] receives the
// number of keys before queries[j], upper_out[j] the number before or equal
// to it (int64, device; either may be null, not both). flags:
// SRS_SEARCH_QUERIES_SORTED, a hint. The call does not wait for the device.
template <bool Up = true, typename K>
void search_sorted(void* stream, const SortIndex num, const K* const sorted_keys,
                   const SortIndex num_queries, const K* const queries,
                   int64_t* const lower_out, int64_t* const upper_out, const int32_t flags = 0) {
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  detail::check(srs_search_sorted_device((int64_t)num, detail::key_kind<K>(), Up ? 1 : 0,
                                         (const void*)sorted_keys, 0, nullptr,
                                         (int64_t)num_queries, (const void*)queries, nullptr,
                                         lower_out, upper_out, nullptr, flags, stream),
                "device::search_sorted");
}

// The segmented form: offsets is sort_ragged's (num_segments + 1 device
// values), every segment sorted on its own; queries[j] is searched in segment
// query_segments[j] (device) and the results are positions inside it. A
// query with a bad id or a segment with bad offsets receives -1 and is
// counted in *num_bad_dev (device; may be null), which is not read back.
template <bool Up = true, typename K>
void search_sorted(void* stream, const SortIndex num, const K* const sorted_keys,
                   const SortIndex num_segments, const int64_t* const offsets,
                   const SortIndex num_queries, const K* const queries,
                   const int64_t* const query_segments, int64_t* const lower_out,
                   int64_t* const upper_out, int64_t* const num_bad_dev) {
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  detail::check(srs_search_sorted_device((int64_t)num, detail::key_kind<K>(), Up ? 1 : 0,
                                         (const void*)sorted_keys, (int64_t)num_segments, offsets,
                                         (int64_t)num_queries, (const void*)queries,
                                         query_segments, lower_out, upper_out, num_bad_dev, 0,
                                         stream),
                "device::search_sorted");
}

// merge: two sorted record sets (num_a records in keys_a, num_b in keys_b,
// both in the sort's key order; Up = false: both sorted descending) merged
// stably into keys_out and every payload's third array, num_a + num_b records
// (srs_merge_soa_device): the stable sort of A followed by B, A's records
// first among equal keys. Every payload is (A's array, B's array, the output
// array). source_out (device, num_a + num_b int64; may be null) receives
// every output record's position in that concatenation. Out of place; the
// call does not wait for the device. The second form has no source_out.
template <bool Up = true, typename K, typename... Ps>
void merge(void* stream, const SortIndex num_a, const K* const keys_a, const SortIndex num_b,
           const K* const keys_b, K* const keys_out, int64_t* const source_out,
           std::tuple<const Ps*, const Ps*, Ps*>... payloads) {
  static_assert(detail::key_kind<K>() >= 0, "unsupported key type");
  static_assert((detail::valid_payload<Ps> && ...), "payload sizes must be 1, 2, 4 or 8");
  static_assert(sizeof...(Ps) <= SRS_MAX_PAYLOADS, "too many payload arrays");
  const void* pays_a[sizeof...(Ps) + 1] = {(const void*)std::get<0>(payloads)..., nullptr};
  const void* pays_b[sizeof...(Ps) + 1] = {(const void*)std::get<1>(payloads)..., nullptr};
  void* pays_out[sizeof...(Ps) + 1] = {(void*)std::get<2>(payloads)..., nullptr};
  uint32_t sizes[sizeof...(Ps) + 1] = {(uint32_t)sizeof(Ps)..., 0};
  detail::check(srs_merge_soa_device((int64_t)num_a, (int64_t)num_b, detail::key_kind<K>(),
                                     Up ? 1 : 0, (const void*)keys_a, (const void*)keys_b,
                                     (int32_t)sizeof...(Ps), pays_a, pays_b, sizes,
                                     (void*)keys_out, pays_out, source_out, stream),
                "device::merge");
}
template <bool Up = true, typename K, typename... Ps>
void merge(void* stream, const SortIndex num_a, const K* const keys_a, const SortIndex num_b,
           const K* const keys_b, K* const keys_out,
           std::tuple<const Ps*, const Ps*, Ps*>... payloads) {
  merge<Up>(stream, num_a, keys_a, num_b, keys_b, keys_out, (int64_t*)nullptr, payloads...);
}

}  // namespace device
}  // namespace radix_sort
}  // namespace simd_sort
