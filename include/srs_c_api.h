/*
 * srs_c_api.h — C ABI of the MI355X-native MSB radix sort (libsrs_amd.so).
 *
 * This is the drop-in boundary for the reference's hot path. Every entry point
 * takes plain pointers and sizes; there are no C++ or torch types in the
 * signatures, so cgo / ctypes / JNI / N-API can bind it directly.
 *
 * Reference interfaces replaced (jonicho/simd-radix-sort, /root/reference):
 *   srs_sort_soa     <- simd_sort::radix_sort::sort(num, keys, payloads...)
 *                       radixSort.hpp:1780-1783, and the thresholded form
 *                       sort<Up,BitSorter,CmpSorter>(cmpSortThreshold, num,
 *                       keys, payloads...) radixSort.hpp:1761-1768
 *                       (src/radix_sort.hpp:297-312, :334-337)
 *   srs_sort_aos     <- sort<Up,BitSorter,CmpSorter>(cmpSortThreshold, num,
 *                       DataElement<K,Ps...>* elements) radixSort.hpp:1770-1778
 *                       (src/radix_sort.hpp:314-332)
 *   *_device         <- same semantics on arrays already resident in HBM,
 *                       enqueued on a caller-provided hipStream_t.
 *
 * Semantics (identical to the reference):
 *   - In place: on return the caller's arrays hold the sorted data.
 *   - Key order is the reference's per-bit direction order
 *     (bitDirUp, radixSort.hpp:1568-1581): unsigned ascending, two's
 *     complement signed, IEEE floats by value with -0.0 before +0.0 (n >
 *     cmp_sort_threshold) or -0.0 == +0.0 kept in input order (n <=
 *     cmp_sort_threshold, the reference's insertion-sort leaf,
 *     radixSort.hpp:159-178 / :1743). up == 0 reverses the order.
 *   - num <= 1 is a no-op (radixSort.hpp:1740). num < 0 is a no-op.
 *   - Payload order inside a run of equal keys: the GPU sort is STABLE
 *     (input order). The reference is unstable there; see DESIGN.md §5 for
 *     what parity means for equal keys.
 *   - NaN keys are outside the contract (the reference's leaf never moves
 *     them; its output depends on leaf boundaries).
 *
 * Error convention: every function returns SRS_OK (0) or a negative
 * srs_status; srs_last_error() returns a thread-local message. The reference
 * API is void (no error channel); the C++ drop-in header
 * (include/simd_sort/radix_sort.hpp) turns a non-zero status into
 * std::abort() with the message, i.e. it fails loudly. There is NO CPU
 * fallback inside the library.
 */
#ifndef SRS_C_API_H_
#define SRS_C_API_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Key kinds: the ten key types the reference supports and tests
 * (src/test.cpp:156-169). Values are part of the ABI. */
typedef enum srs_key_kind {
  SRS_KEY_U8 = 0,
  SRS_KEY_I8 = 1,
  SRS_KEY_U16 = 2,
  SRS_KEY_I16 = 3,
  SRS_KEY_U32 = 4,
  SRS_KEY_I32 = 5,
  SRS_KEY_U64 = 6,
  SRS_KEY_I64 = 7,
  SRS_KEY_F32 = 8,
  SRS_KEY_F64 = 9
} srs_key_kind;

typedef enum srs_status {
  SRS_OK = 0,
  SRS_ERR_INVALID_ARG = -1,
  SRS_ERR_UNSUPPORTED = -2,
  SRS_ERR_HIP = -3,
  SRS_ERR_OUT_OF_MEMORY = -4,
  SRS_ERR_NO_DEVICE = -5,
  SRS_ERR_INTERNAL = -6
} srs_status;

/* Maximum number of payload columns per call (the reference's test uses up
 * to 63 one-byte payloads, src/test.cpp:125-134). */
#define SRS_MAX_PAYLOADS 64

/* ---- host-pointer drop-in entry points (synchronous) -------------------- */

/* Sort `num` keys (kind `key_kind`) and `num_payloads` payload columns in
 * place. payload_sizes[i] is the element size in bytes of column i
 * (1, 2, 4 or 8). cmp_sort_threshold is the reference's cmpSortThreshold
 * (16 in the two-argument sort()). Host memory; copies through HBM. */
int srs_sort_soa(int64_t num, int key_kind, int up, int64_t cmp_sort_threshold,
                 void* keys, int32_t num_payloads, void* const* payloads,
                 const uint32_t* payload_sizes);

/* Sort `num` combined elements of `elem_size` bytes (a power of two, 1..64,
 * >= the key size) whose key of kind `key_kind` sits at byte offset 0
 * (simd_sort::DataElement<K, Ps...>). The payload bytes are opaque and move
 * with their key. */
int srs_sort_aos(int64_t num, int key_kind, int up, int64_t cmp_sort_threshold,
                 void* elements, uint32_t elem_size);

/* Leaf handling: the reference's CmpSorter template argument
 * (src/cmp_sorters.hpp). SRS_LEAF_SORTED = CmpSorterInsertionSort (and
 * CmpSorterBramasSmallSort): leaves of <= cmp_sort_threshold keys are sorted,
 * so the output is fully sorted. SRS_LEAF_UNSORTED = CmpSorterNoSort
 * (src/cmp_sorters.hpp:66-78, thesis:3113-3124): the recursion stops at
 * leaves of <= cmp_sort_threshold keys and leaves them in partition order.
 * Every leaf then holds exactly the keys (and their payloads) a full sort
 * puts there, so each element ends within cmp_sort_threshold - 1 places of
 * its sorted slot; num <= cmp_sort_threshold leaves the input untouched.
 * The order inside a leaf is unspecified and may differ from run to run (the
 * GPU's bucket pass places a leaf's elements with LDS atomics); only the
 * leaf's contents are guaranteed, as for the reference's no-op leaf. */
#define SRS_LEAF_SORTED 0
#define SRS_LEAF_UNSORTED 1

/* srs_sort_soa / srs_sort_aos with the leaf handling chosen by leaf_mode:
 * sort<Up, BitSorter, CmpSorter>(cmpSortThreshold, num, ...) for every
 * CmpSorter of src/cmp_sorters.hpp (radixSort.hpp:1761-1778). */
int srs_sort_soa_leaf(int64_t num, int key_kind, int up, int64_t cmp_sort_threshold,
                      int leaf_mode, void* keys, int32_t num_payloads, void* const* payloads,
                      const uint32_t* payload_sizes);
int srs_sort_aos_leaf(int64_t num, int key_kind, int up, int64_t cmp_sort_threshold,
                      int leaf_mode, void* elements, uint32_t elem_size);

/* ---- device-pointer entry points (asynchronous on `stream`) ------------- */

/* Same as srs_sort_soa on device pointers. `stream` is a hipStream_t (NULL =
 * the default stream). If keys_out/payloads_out are NULL the sort is in place;
 * otherwise the inputs are left untouched and the result is written to the
 * *_out arrays (which must not alias the inputs). The call enqueues work and
 * may block briefly on small control read-backs; results are ready when the
 * stream completes. By size: num <= 8192 is one launch and no host wait;
 * 8192 < num <= 2^20 (no segment list) is one launch with its own grid
 * barriers, and the call waits until that kernel has posted its first
 * level's bucket sizes to host memory (a skewed input then continues on the
 * general levels); larger sorts read back a small counter block once per
 * global level. */
int srs_sort_soa_device(int64_t num, int key_kind, int up,
                        int64_t cmp_sort_threshold, void* keys,
                        int32_t num_payloads, void* const* payloads,
                        const uint32_t* payload_sizes, void* keys_out,
                        void* const* payloads_out, void* stream);

int srs_sort_aos_device(int64_t num, int key_kind, int up,
                        int64_t cmp_sort_threshold, void* elements,
                        uint32_t elem_size, void* elements_out, void* stream);

/* The device forms with the leaf handling chosen by leaf_mode (see above). */
int srs_sort_soa_device_leaf(int64_t num, int key_kind, int up, int64_t cmp_sort_threshold,
                             int leaf_mode, void* keys, int32_t num_payloads,
                             void* const* payloads, const uint32_t* payload_sizes,
                             void* keys_out, void* const* payloads_out, void* stream);
int srs_sort_aos_device_leaf(int64_t num, int key_kind, int up, int64_t cmp_sort_threshold,
                             int leaf_mode, void* elements, uint32_t elem_size,
                             void* elements_out, void* stream);

/* Sorts each segment [segment_bounds[i], segment_bounds[i+1]) of a device
 * key column and its payload columns independently, in place, as sub-ranges
 * of one sort (no n <= threshold rule per segment). segment_bounds is a HOST
 * array of num_segments + 1 non-decreasing offsets within [0, num]; elements
 * outside every segment are untouched. known_top_bits: the caller guarantees
 * that inside each segment all keys agree on their top known_top_bits
 * transformed bits (0 = no knowledge); those bits are not examined again.
 * Asynchronous on `stream` (returns once the work is queued). Replaces
 * calling radix_sort::sort (radixSort.hpp:1780) once per sub-range; the
 * multi-GPU shard sorts its receive groups with it. */
int srs_sort_segments_device(int64_t num, int key_kind, int up, void* keys,
                             int32_t num_payloads, void* const* payloads,
                             const uint32_t* payload_sizes, int64_t num_segments,
                             const int64_t* segment_bounds, int32_t known_top_bits,
                             void* stream);

/* Top-k: writes the first min(k, num) records of the stable sort of the
 * input (by the key order above; up == 0 reversed, so up = 1 gives the k
 * smallest ascending and up = 0 the k largest descending) to the *_out
 * arrays, without sorting the rest. Equal keys keep their input order, so the
 * result is unique: bit-equal to the head of srs_sort_soa_device with
 * num > cmp_sort_threshold. Float keys follow the total order (-0.0 before
 * +0.0 ascending) at every size; NaN keys are outside the contract. The
 * inputs are never written; the outputs hold min(k, num) records and must
 * not overlap any input (SRS_ERR_INVALID_ARG, checked before any device
 * access). k <= 0 or num <= 0 is a no-op; k >= num is the out-of-place sort.
 * indices_out (device int64, may be NULL) receives each output record's
 * position in the input (ascending within a run of equal keys); it travels
 * as one more 8-byte column, so with it at most SRS_MAX_PAYLOADS - 1 = 63
 * payload columns are allowed (SRS_ERR_UNSUPPORTED). The reference has no
 * counterpart (its callers sort everything and keep the head).
 * The call enqueues work on `stream` and blocks on a small pinned read-back
 * once per select pass (a 12-bit digit histogram of the keys that share the
 * prefix found so far; one to three passes for most inputs, and none when
 * k > num / 2 or num <= 8192: those calls sort everything into a workspace
 * buffer and copy the head); the finishing sort of the selected records
 * reads back as srs_sort_soa_device does for its size. Results are ready
 * when the stream completes. */
int srs_topk_soa_device(int64_t num, int64_t k, int key_kind, int up,
                        const void* keys, int32_t num_payloads,
                        const void* const* payloads, const uint32_t* payload_sizes,
                        void* keys_out, void* const* payloads_out,
                        int64_t* indices_out, void* stream);
/* The same on combined elements (srs_sort_aos_device's layout). */
int srs_topk_aos_device(int64_t num, int64_t k, int key_kind, int up,
                        const void* elements, uint32_t elem_size,
                        void* elements_out, int64_t* indices_out, void* stream);

/* Row-wise top-k: srs_topk_soa_device on every row of a matrix in one call.
 * Record i of row r of a column of width w is at base + (r * row_stride + i)
 * * w; row_stride is in records, the same for every input column, and at
 * least row_len (a row may start at any element: base pointers need only
 * their element alignment). The outputs are dense: with kk = min(k, row_len),
 * result j of row r is at r * kk + j of every *_out column. Each row's result
 * is exactly srs_topk_soa_device's (stable, total order for floats);
 * indices_out (may be NULL) receives positions inside the row, 0 .. row_len -
 * 1. The inputs are never written and the records between row_len and
 * row_stride are never selected. Checked before any device access:
 * key_kind, payload sizes, NULL or misaligned pointers, 64 payloads with
 * indices (as for top-k), row_stride < row_len, rows * row_stride overflowing
 * int64, and any output over any input column (an input column spans
 * ((rows - 1) * row_stride + row_len) * w bytes, an output rows * kk * w).
 * rows <= 0, row_len <= 0 or k <= 0 is a no-op.
 * Rows of at most 8192 records, and longer rows with kk <= 2048
 * (srs_topk_rows_max_k), take ONE launch with one workgroup per row and no
 * read-back; other shapes (and a few rows of many millions of records) run
 * srs_topk_soa_device's select row by row, with its read-backs
 * (DESIGN.md §12). */
int srs_topk_rows_soa_device(int64_t rows, int64_t row_len, int64_t row_stride, int64_t k,
                             int key_kind, int up, const void* keys, int32_t num_payloads,
                             const void* const* payloads, const uint32_t* payload_sizes,
                             void* keys_out, void* const* payloads_out,
                             int64_t* indices_out, void* stream);
/* The largest min(k, row_len) the one-launch route takes for rows longer
 * than 8192 records (kTopkRowsMaxK). */
int64_t srs_topk_rows_max_k(void);

/* Row-wise sort: every row of a matrix sorted in one call, out of place.
 * Addressing is srs_topk_rows_soa_device's: record i of row r of a column of
 * width w is at base + (r * row_stride + i) * w, row_stride in records, the
 * same for every input column and at least row_len. The outputs are dense:
 * record j of row r is at r * row_len + j of every *_out column. Each row's
 * result is the stable sort by transformed key (equal keys keep their input
 * order; floats in the total order at every size, -0.0 before +0.0; NaN keys
 * are outside the contract; up == 0 reverses the key order), bit-equal to
 * srs_topk_rows_soa_device with k = row_len wherever that call runs in one
 * launch. indices_out (may be NULL) receives positions inside the row; it
 * travels as one more 8-byte column, so 64 payload columns with indices
 * return SRS_ERR_UNSUPPORTED. The inputs are never written. There is no
 * in-place form: every output must be clear of every input column.
 * Checked before any device access, exactly as for row-wise top-k with k =
 * row_len: key_kind, payload sizes, NULL or misaligned pointers, row_stride <
 * row_len, rows * row_stride overflowing int64, and any output (indices
 * included) over any input column. rows <= 0 or row_len <= 0 is a no-op;
 * row_len == 1 copies the rows (and writes index 0).
 * Rows of up to 8192 records take no host read-back: one launch with a
 * workgroup per row (short rows), or the sort's LDS pass over a device-built
 * list of one segment per row. Longer rows run the sort's global levels
 * breadth-first over all rows, with a level's read-backs. */
int srs_sort_rows_soa_device(int64_t rows, int64_t row_len, int64_t row_stride,
                             int key_kind, int up, const void* keys, int32_t num_payloads,
                             const void* const* payloads, const uint32_t* payload_sizes,
                             void* keys_out, void* const* payloads_out,
                             int64_t* indices_out, void* stream);

/* Ragged sort: segments given by a DEVICE array of offsets, every segment
 * sorted in one call, out of place. offsets holds num_segments + 1 int64
 * values in device memory, non-decreasing, with 0 <= offsets[0] and
 * offsets[num_segments] <= num; segment i is records [offsets[i],
 * offsets[i + 1]) of every column. Columns are dense and num records long;
 * the outputs have the inputs' shape: record j of segment i's result is at
 * offsets[i] + j of every *_out column. Each segment's result is the stable
 * sort by transformed key (equal keys keep their input order; floats in the
 * total order at every length, -0.0 before +0.0; NaN keys are outside the
 * contract; up == 0 reverses the key order), bit-equal to
 * srs_sort_rows_soa_device when the offsets are uniform. indices_out (may be
 * NULL) receives positions inside the segment, 0 .. len - 1; it travels as
 * one more 8-byte column, so 64 payload columns with indices return
 * SRS_ERR_UNSUPPORTED. The inputs and offsets are never written, and records
 * outside [offsets[0], offsets[num_segments]) are neither read nor written
 * in the outputs. Empty segments are legal; a segment of one record is
 * copied (index 0). There is no in-place form: every output must be clear of
 * every input column and of the offsets (srs_sort_segments_device stays the
 * in-place call, with host bounds).
 * Checked before any device access: key_kind, payload sizes, NULL or
 * misaligned pointers (offsets: 8-byte aligned), num_segments + 1
 * overflowing, and any output (indices included) over any input column or
 * the offsets array. num <= 0 or num_segments <= 0 is a no-op.
 * Bad offsets (a decreasing pair, a negative start, an end beyond num) are
 * seen on the device only: no kernel of the call reads or writes a column
 * outside [0, num) whatever offsets holds, a segment with a bad bound is
 * skipped and counted, and when the count comes back non-zero the call
 * returns SRS_ERR_INVALID_ARG (srs_last_error() names the count); the
 * outputs are then unspecified.
 * Host waits: ONE pinned read-back of the segment counters after the
 * classify pass (segments of at most 256 records are sorted by a kernel
 * queued behind that copy, a wave per segment, and never wait for it); after
 * that, only what the sort's global levels need for segments of more than
 * 8192 records, two read-backs a level. */
int srs_sort_ragged_soa_device(int64_t num, int64_t num_segments, const int64_t* offsets,
                               int key_kind, int up, const void* keys, int32_t num_payloads,
                               const void* const* payloads, const uint32_t* payload_sizes,
                               void* keys_out, void* const* payloads_out,
                               int64_t* indices_out, void* stream);

/* Ragged top-k: the first k records of every segment of a DEVICE array of
 * offsets, in one call. The inputs are srs_sort_ragged_soa_device's: dense
 * columns of num records, offsets holding num_segments + 1 int64 values in
 * device memory; the inputs and the offsets are never written. The outputs
 * hold num_segments * k records each, a fixed stride of k slots per segment:
 * with c_i = min(k, len_i), result j < c_i of segment i is at i * k + j of
 * every *_out column and of indices_out (may be NULL; positions inside the
 * segment); slots j >= c_i are NOT written. counts_out (device int64,
 * num_segments entries, may be NULL) receives c_i for every valid segment, 0
 * for an empty one. Each segment's result is the first c_i records of its
 * stable sort by transformed key (equal keys keep their input order; floats
 * in the total order at every length; NaN keys are outside the contract; up
 * == 0 gives the largest, descending): unique, and bit-equal to the head of
 * srs_sort_ragged_soa_device's segment and to srs_topk_rows_soa_device when
 * the offsets are uniform.
 * Checked before any device access: key_kind, payload sizes, NULL or
 * misaligned pointers (offsets, indices_out and counts_out: 8-byte aligned),
 * num_segments + 1, num_segments * k and that product times a column width
 * overflowing int64, 64 payload columns with indices (SRS_ERR_UNSUPPORTED),
 * and any output (indices and counts included) over any input column or over
 * the offsets array. num <= 0, num_segments <= 0 or k <= 0 is a no-op.
 * Bad offsets behave as in srs_sort_ragged_soa_device: every kernel tests a
 * segment's two offsets itself, a segment with a bad bound is skipped and
 * counted, and when the count comes back non-zero the call returns
 * SRS_ERR_INVALID_ARG (srs_last_error() names the count); the outputs are
 * then unspecified. No column is accessed outside [0, num), no output
 * outside its num_segments * k records.
 * k <= 2048 (srs_topk_rows_max_k) with num < 2^31 takes three kernels, a wave
 * per segment of up to 256 records and a workgroup per longer one, and ONE
 * pinned read-back of the counters behind all of them. Other shapes run the
 * ragged sort into workspace columns of num records (with its host waits)
 * and copy the heads. */
int srs_topk_ragged_soa_device(int64_t num, int64_t num_segments, const int64_t* offsets,
                               int64_t k, int key_kind, int up, const void* keys,
                               int32_t num_payloads, const void* const* payloads,
                               const uint32_t* payload_sizes, void* keys_out,
                               void* const* payloads_out, int64_t* indices_out,
                               int64_t* counts_out, void* stream);

/* Unique: the distinct keys, where each group of equal keys starts, and
 * which group every input record fell into, in one call. Let S be the stable
 * sort of the input by transformed key (srs_sort_soa_device out of place
 * with num > cmp_sort_threshold: floats in the total order at every size, so
 * -0.0 and +0.0 are two keys; NaN keys are outside the contract; up == 0
 * reversed), and U the number of runs of bit-equal keys in S. The inputs are
 * never written.
 * unique_out (required, num slots of the key type): slots [0, U) receive the
 * first key of every run, in S's order; slots from U on are NOT written.
 * offsets_out (may be NULL, num + 1 int64): slots [0, U] receive every run's
 * start in S and offsets_out[U] = num, directly usable as the offsets of
 * srs_sort_ragged_soa_device / srs_topk_ragged_soa_device over the sorted
 * columns; the counts are its differences. Slots past U are NOT written.
 * keys_sorted_out / payloads_sorted_out: S itself, num records each; a set,
 * or both NULL (num_payloads must then be 0, else SRS_ERR_INVALID_ARG; S
 * lives in the workspace only).
 * indices_out (may be NULL, num int64): the input position of every record
 * of S (the argsort); the sort is stable, so indices_out[offsets_out[j]] is
 * the first occurrence of unique key j in the input.
 * inverse_out (may be NULL, num int64): inverse_out[i] is the run number,
 * 0 .. U-1, of input record i: unique_out[inverse_out[i]] is bit-equal to
 * keys[i].
 * num_unique_dev (device int64) and num_unique_host (host int64) may each be
 * NULL; they receive U.
 * Host waits: with num_unique_host, ONE pinned read-back of U behind all
 * kernels, and the call returns after it; without it the unique stage (three
 * launches in stream order: the run tally, the scan of the tile counts, the
 * write) adds no host wait to what the sort does for its
 * size.
 * Checked before any device access: key_kind, payload sizes, NULL or
 * misaligned pointers (the int64 arrays: 8-byte aligned), num + 1
 * overflowing, 64 payload columns with an index column (it travels whenever
 * indices_out or inverse_out is given; SRS_ERR_UNSUPPORTED), and any output
 * over any input column or over another output. num <= 0 is a no-op that
 * writes 0 to *num_unique_host if given; num == 1 gives U = 1 and offsets
 * {0, 1}. No output is accessed outside the slot counts above. SoA only. */
int srs_unique_soa_device(int64_t num, int key_kind, int up, const void* keys,
                          int32_t num_payloads, const void* const* payloads,
                          const uint32_t* payload_sizes, void* keys_sorted_out,
                          void* const* payloads_sorted_out, int64_t* indices_out,
                          void* unique_out, int64_t* offsets_out, int64_t* inverse_out,
                          int64_t* num_unique_dev, int64_t* num_unique_host, void* stream);

/* Search-sorted: the lower and upper bounds of query keys in a sorted key
 * column, in one call. Let T be the key transform of (key_kind, up) (unsigned
 * keys as they are, signed keys with the sign bit flipped, floats in the
 * total order so that -0.0 comes before +0.0; up == 0 complements, which
 * reverses the order). sorted_keys holds num keys of key_kind with T
 * non-decreasing: what srs_sort_soa_device writes with num >
 * cmp_sort_threshold, what every total-order call writes (top-k, the
 * row-wise and the ragged calls), and what unique_out and keys_sorted_out of
 * srs_unique_soa_device hold. up == 0 therefore means a table sorted
 * descending. NaN keys are outside the contract, as elsewhere. Neither the
 * table nor the queries are written.
 * Flat form (offsets == NULL and query_segments == NULL; num_segments is
 * ignored): queries holds num_queries keys of the same kind; lower_out[j]
 * receives the number of table keys t with T(t) < T(q_j), upper_out[j] the
 * number with T(t) <= T(q_j), both int64. Either output may be NULL, not
 * both. upper - lower is the number of table keys equal to the query (the
 * multiplicity of a sort-merge join; non-zero: the key is present); with
 * unique_out as the table, lower is the group number of a query that is
 * present (the inverse_out of keys that were not in the unique call).
 * Segmented form (offsets and query_segments both given, num_segments >= 1;
 * either one alone is SRS_ERR_INVALID_ARG): offsets is the ragged calls'
 * array, num_segments + 1 int64 values in device memory, and every segment
 * [offsets[s], offsets[s + 1]) is sorted on its own, as
 * srs_sort_ragged_soa_device leaves it. query_segments[j] (device int64,
 * num_queries entries) names the segment query j is searched in, and the
 * results are positions inside that segment, 0 .. len. A query is BAD when
 * its segment id is outside [0, num_segments) or its segment's two offsets
 * are bad (decreasing, negative, beyond num): it receives -1 in every output
 * given and is counted in *num_bad_dev (device int64, may be NULL; written
 * by the call, 0 when there is none). The good queries of the same call are
 * answered as usual. The kernel tests the id and both offsets itself: no key
 * outside [0, num) is read whatever the two arrays hold. The call does NOT
 * read the count back: a lookup has no other host wait and does not gain
 * one. The flat form writes 0 to *num_bad_dev if it is given.
 * A table that is not sorted gives unspecified results inside [0, num] ([0,
 * len] for a segment); nothing outside the columns is accessed.
 * flags: SRS_SEARCH_QUERIES_SORTED says that the caller believes the queries
 * are themselves in T order (the output of a sort, for example). It is a
 * hint for the route only: the kernel then runs on the caller's queries and
 * narrows every tile of SRS_SEARCH_QUERY_TILE queries to the table range
 * between the tile's smallest and largest query, so a wrong hint never
 * changes a result. Without it, many queries against a large table are
 * first sorted by the call, with an index column, searched in order and
 * written back through the index (DESIGN.md §17 has the rule).
 * num_queries <= 0 is a no-op. num <= 0 with queries writes 0 to every
 * output given; in the segmented form every query is then bad unless its
 * segment is a valid empty one.
 * Checked before any device access: key_kind; NULL sorted_keys with num > 0,
 * NULL queries, both outputs NULL; misaligned pointers (keys to their element
 * size, the int64 arrays to 8 bytes); num, num_queries * 8 or num_segments +
 * 1 overflowing; unknown flags bits; offsets without query_segments or the
 * reverse, num_segments < 1 with them; and every output (num_bad_dev
 * included) over every input (sorted_keys, queries, offsets, query_segments)
 * and over every other output.
 * Host waits: none on the direct route (one kernel, and a memset when
 * num_bad_dev is given); the sort route has what srs_sort_soa_device has for
 * num_queries records. */
#define SRS_SEARCH_QUERIES_SORTED 1 /* flags bit: a hint, see above */
/* The search kernel's shape, for tests of its edges: queries per workgroup,
 * the slots of its LDS sample, and the most keys of a table range that is
 * staged whole. */
#define SRS_SEARCH_QUERY_TILE 1024
#define SRS_SEARCH_LDS_SAMPLES 2048
#define SRS_SEARCH_LDS_RANGE 2047
int srs_search_sorted_device(int64_t num, int key_kind, int up, const void* sorted_keys,
                             int64_t num_segments, const int64_t* offsets,
                             int64_t num_queries, const void* queries,
                             const int64_t* query_segments, int64_t* lower_out,
                             int64_t* upper_out, int64_t* num_bad_dev, int32_t flags,
                             void* stream);

/* Merge: two sorted record sets combined into one, stably, in one call. Let
 * T be the key transform of (key_kind, up), exactly search-sorted's (floats
 * in the total order, so -0.0 sorts before +0.0; up == 0 means that BOTH
 * inputs are sorted descending; uint64 keys have their own kind; NaN keys are
 * outside the contract). keys_a[0, num_a) and keys_b[0, num_b) each have T
 * non-decreasing: anything a total-order call of this library wrote. Payload
 * column c of A and of B has the same width payload_sizes[c] (1, 2, 4 or 8);
 * 0 .. SRS_MAX_PAYLOADS columns, every key kind. The inputs are never
 * written.
 * Output: num_a + num_b records in keys_out and in every payloads_out[c],
 * equal to the stable sort by T of A followed by B: among equal keys all of
 * A's records come first, in A's order, then B's in B's order. source_out
 * (may be NULL, num_a + num_b int64) receives every output record's position
 * in that concatenation, i for A[i] and num_a + j for B[j]: the argsort of
 * the concatenation, with which a caller gathers columns it did not pass.
 * Out of place only: every output is checked against every input column and
 * against every other output, and an overlap is SRS_ERR_INVALID_ARG.
 * An input that is not sorted gives an unspecified result, but nothing
 * outside the given columns is read or written and every source_out value
 * lies in [0, num_a + num_b).
 * num_a + num_b <= 0 is a no-op. One empty side is legal, its pointers may
 * then be NULL, and the call is an ordered copy of the other side.
 * Checked before any device access: key_kind, the payload sizes,
 * num_payloads out of range, negative counts, (num_a + num_b) * 16
 * overflowing, NULL columns of a side that is not empty, NULL outputs,
 * misaligned pointers (keys and payloads to their element size, source_out
 * to 8 bytes), and the overlaps above.
 * Host waits: none. Nothing is read back; the call queues three launches on
 * `stream` (the column descriptor, the split of every tile boundary, one
 * workgroup per SRS_MERGE_TILE output records) and returns.
 * The only workspace is 8 bytes per tile. */
#define SRS_MERGE_TILE 4096 /* output records per workgroup, for tests of the kernel's edges */
int srs_merge_soa_device(int64_t num_a, int64_t num_b, int key_kind, int up,
                         const void* keys_a, const void* keys_b, int32_t num_payloads,
                         const void* const* payloads_a, const void* const* payloads_b,
                         const uint32_t* payload_sizes, void* keys_out,
                         void* const* payloads_out, int64_t* source_out, void* stream);

/* ---- multi-GPU shard primitives (top-radix-bits partition) --
 * A node-wide sort of one array spread over N GPUs: every rank histograms
 * its keys' top bits (srs_key_histogram_device), the histograms are summed
 * (RCCL all-reduce), contiguous bucket ranges are assigned to ranks, every
 * rank partitions its keys by destination (srs_partition_device), the groups
 * are exchanged (RCCL all-to-all) and each rank sorts what it received
 * (srs_sort_soa_device). Concatenating the ranks in order gives the sorted
 * array. The reference has no multi-device path; these have no counterpart. */

/* Adds the histogram of the transformed top `bits` (1..12) bits of `num`
 * device keys into the device array hist[2^bits] (uint64). Asynchronous. */
int srs_key_histogram_device(int64_t num, int key_kind, int up, const void* keys,
                             int bits, uint64_t* hist, void* stream);

/* Stable partition of a key column and its payload columns into num_parts
 * (<= 512) groups: a key whose transformed top `bits` (1..16) bits equal b
 * goes to group part_of_bucket[b] (DEVICE int32 array of 2^bits entries;
 * non-decreasing makes every group a contiguous key range). Groups are
 * written back to back, group 0 first, to keys_out / payloads_out (device,
 * not aliasing the inputs); part_counts (HOST array of num_parts int64)
 * receives the group sizes. Returns after the counts are known; the data
 * movement completes on `stream`. */
int srs_partition_device(int64_t num, int key_kind, int up, const void* keys,
                         int32_t num_payloads, const void* const* payloads,
                         const uint32_t* payload_sizes, int bits,
                         const int32_t* part_of_bucket, int32_t num_parts,
                         void* keys_out, void* const* payloads_out,
                         int64_t* part_counts, void* stream);

/* ---- the multi-GPU shard sort (C ABI) ----------------------
 * One array spread over N GPUs is sorted across them: rank r ends with the
 * r-th key range, so concatenating the ranks' outputs gives the sorted array
 * (stable). The protocol is the one above: histogram all-reduce, 512
 * key-range groups, chunked partition, rounds of grouped send/recv over
 * xGMI, each round's range sorted on a side stream while the later rounds
 * are in flight. RCCL is loaded at first use (librccl.so.1); without it the
 * RCCL communicators return SRS_ERR_NO_DEVICE. The reference has no
 * multi-device path. This is the only implementation of the protocol (the
 * Python bench drives it through ctypes).
 *
 * Communicators: one process per GPU (srs_shard_unique_id on one rank, the
 * 128 bytes passed to every rank, srs_shard_comm_init on each with its GPU
 * current), or one process driving several GPUs (srs_shard_comm_init_all,
 * then srs_shard_sort_multi).
 *
 * Failures: every rank returns an error if any rank fails (invalid or
 * disagreeing arguments, an allocation, a partition or a round sort), with
 * the communicator still usable afterwards; a rank never returns early while
 * its peers wait for its messages. A transport failure (RCCL error, timeout)
 * aborts the communicator (ncclCommAbort): later sorts on it fail and it
 * must be destroyed. Host waits on peers are bounded by SRS_SHARD_TIMEOUT_S
 * seconds (default 600). */
#define SRS_SHARD_ID_BYTES 128
typedef struct srs_shard_comm_s* srs_shard_comm;
int srs_shard_unique_id(void* id);
int srs_shard_comm_init(int32_t world, int32_t rank, const void* id, srs_shard_comm* comm);
int srs_shard_comm_init_all(int32_t num_devices, const int32_t* devices, srs_shard_comm* comms);
int srs_shard_comm_destroy(srs_shard_comm comm);

/* `world` communicators over the CURRENT device whose collectives and peer
 * messages travel through host memory (threads of one process; drive them
 * with srs_shard_sort_multi). Every kernel of the protocol runs as with
 * RCCL; only the transport differs. For tests and for machines with fewer
 * GPUs than ranks (RCCL puts no two ranks on one device). */
int srs_shard_comm_init_staged(int32_t world, srs_shard_comm* comms);

/* Exchange rounds (1..64) and partition chunks (1..16) of later sorts on
 * this communicator; 0 = the default (from 2 ranks up 8 rounds and 4
 * chunks; at one rank 8 rounds and 1 chunk). Every rank must use the same values (checked: a mismatch
 * fails every rank with SRS_ERR_INVALID_ARG). */
int srs_shard_set_options(srs_shard_comm comm, int32_t rounds, int32_t chunks);

/* Message options of later sorts on this communicator. self_messages = 1:
 * this rank's own pieces travel as transport messages to itself (a send and
 * a receive inside the round's group, as a peer's do) instead of device
 * copies, so that one rank exercises every transport call of the exchange
 * (the receive buffer then never aliases the partition buffer).
 * max_message_bytes: the largest single message, a multiple of 64 in
 * [64, 2^30]; 0 = the default 256 MiB (RCCL corrupts messages above 1 GiB,
 * DESIGN.md §7). Every rank must use the same cap (checked like the options
 * above); self messages are a rank's own choice. */
int srs_shard_set_message_options(srs_shard_comm comm, int32_t self_messages,
                                  int64_t max_message_bytes);

/* This rank's part of the shard sort of device columns (inputs untouched):
 * *keys_out / payloads_out[k] receive device pointers to this rank's sorted
 * key range and *num_out its length; the memory belongs to the communicator
 * and stays valid until its next sort or its destruction. Work runs on
 * `stream` (and the communicator's own streams); the call returns when the
 * sort is complete. Every rank of the communicator must call it. */
int srs_shard_sort_device(srs_shard_comm comm, int64_t num, int key_kind, int up,
                          const void* keys, int32_t num_payloads, const void* const* payloads,
                          const uint32_t* payload_sizes, void** keys_out, void** payloads_out,
                          int64_t* num_out, void* stream);

/* All ranks of a single-process communicator set at once (one host thread
 * per rank; synchronous): rank i sorts nums[i] records at keys[i] and
 * payloads[i * num_payloads + k]; outputs as above, per rank. */
int srs_shard_sort_multi(int32_t num_devices, const srs_shard_comm* comms, const int64_t* nums,
                         int key_kind, int up, const void* const* keys, int32_t num_payloads,
                         const void* const* payloads, const uint32_t* payload_sizes,
                         void** keys_out, void** payloads_out, int64_t* nums_out);

/* The last successful sort on this communicator as JSON: transport, world,
 * rank, chunks, rounds, groups, records in / out, record bytes, "stamps_ms"
 * (HIP-event times since its start of: hist, plan, partition<c>,
 * round<r>_recv, round<r>_sort_start, round<r>_sort_end, end) and
 * "bytes_to_peer_per_round" ([round][peer] bytes this rank sent; itself too
 * with self messages), self_messages, max_message_bytes, sends / recvs (the
 * transport calls posted) and deferred_frees (workspace buffers that grew
 * during the exchange; their old memory is freed after it). */
int srs_shard_last_report(srs_shard_comm comm, char* buf, int64_t cap);

/* Test hook: the next sort on this communicator fails at `point` (0 = none,
 * 1 = argument error, 2 = allocation before the exchange, 3 = partition
 * after the first messages, 4 = the last round's sort, 5 = transport
 * failure after the first messages: aborts). */
int srs_shard_debug_inject(srs_shard_comm comm, int32_t point);

/* The shard plan of one rank, host only (no GPU): from every rank's chunk
 * histograms (chunk_hists[src][chunk][2^min(12, key_bits)] of the
 * transformed top key bits), this rank's record count and whether its own
 * pieces travel as self messages (srs_shard_set_message_options), the JSON of
 * group_of_bin, rank_of_group, chunk_bounds, total (records received),
 * "posts" (every message group in posting order: its (round, chunk) pieces
 * and msgs = [op (0 send, 1 receive, 2 own-piece copy), peer, partitioned
 * offset, receive offset, records]) and "rounds" (each round's receive
 * range, its sort segments and known top bits). The same code plans the
 * device sort; tests drive the protocol with it on CPU (gloo). */
int srs_debug_shard_plan(int32_t world, int32_t rank, int32_t chunks, int32_t rounds,
                         int32_t key_bits, int32_t self_messages, const uint64_t* chunk_hists,
                         int64_t num, char* json, int64_t cap);

/* ---- host arrays over several GPUs --------------------------------------- */

/* Devices the host-pointer entry points (srs_sort_soa, srs_sort_soa_leaf)
 * may use. 0 devices (the default) = the calling thread's current device.
 * With G > 1 devices a large SoA sort (>= 2^22 keys) splits the host array
 * G ways: chunk g goes over device g's own PCIe link, the chunks are
 * partitioned into G key ranges (a stable top-bits radix level), range h is
 * gathered on device h over xGMI, sorted there and copied back to its place.
 * The result is the same array a one-device sort gives. A device may be
 * listed more than once (its shards then share it). The environment
 * variable SRS_HOST_DEVICES ("all" or "0,1,2") sets the initial list. The
 * reference sorts on one host thread and has no counterpart. */
int srs_set_host_devices(int32_t num_devices, const int32_t* devices);

/* ---- device memory for sort buffers --------------------------------------- */

/* Allocates `bytes` of device memory on the current device for arrays the
 * sort will write (out-of-place outputs, in-place arrays). The scatter's
 * write rate depends on where a buffer sits in HBM (the same
 * kernel writes some allocations ~13 % slower); buffers of 256 MB and more
 * are probed with the sort's write pattern and re-placed (up to 6 tries,
 * while free memory allows) when slower than the fastest placement seen.
 * The sort's own workspace is placed the same way. SRS_PLACE=0 turns the
 * probing off. srs_free_device releases it. No counterpart in the
 * reference (host arrays only). */
int srs_alloc_device(uint64_t bytes, void** ptr);
int srs_free_device(void* ptr);

/* ---- synthetic data (bench / tests) ------------------------------------- */

/* keys[i] = splitmix64(seed + first_index + i) truncated/reinterpreted to the
 * key kind (floats: uniform in [-1,1) on a 2^-23 / 2^-52 grid); payload column
 * c gets the low bytes of splitmix64(bits(key[i]) ^ c * 0xD1B54A32D192ED03)
 * (a function of the key). */
int srs_fill_synthetic_device(int64_t num, int key_kind, uint64_t seed,
                              uint64_t first_index, void* keys,
                              int32_t num_payloads, void* const* payloads,
                              const uint32_t* payload_sizes, void* stream);

/* ---- diagnostics ---------------------------------------------------------- */

/* Thread-local description of the last error (never NULL). */
const char* srs_last_error(void);

/* Library version string ("srs_amd <semver> gfx950"). */
const char* srs_version(void);

/* Per-kernel timing with HIP events recorded on the launch stream around
 * every kernel launch (enable 1; off by default; 2: around the scatter
 * launches only, as bench.py's timed region). srs_kernel_stats fills, for kernel
 * name `name` ("count", "scatter", "local", "scan", ...), the number of
 * launches and the summed device milliseconds since the last reset; the
 * stream must have completed. Returns SRS_ERR_INVALID_ARG for unknown names. */
int srs_set_kernel_timing(int enable);
int srs_reset_kernel_stats(void);
int srs_kernel_stats(const char* name, int64_t* launches, double* total_ms,
                     double* elements);

/* The super-group column scan: a level over one large segment
 * scans sums of 64 scan groups once it has at least min_groups groups of 32
 * tiles (default 256, i.e. 33.5 M keys; <= 0 restores it). Process-wide;
 * tests lower it so that the path runs at small sizes. */
int srs_debug_set_super_scan(int64_t min_groups);

/* Test hook, process-wide and read on every call, like
 * srs_debug_set_super_scan: the size rules that pick a sort's first level
 * (DESIGN.md §2), so that the plain, balanced, stripe and gathered levels run
 * at small sizes. It affects every entry point that ends in the sort driver
 * (the device and host sorts, and the top-k, row-wise, ragged, unique, search
 * and shard calls where they sort). Tests restore the defaults in a `finally`
 * or a fixture. A value <= 0 restores that field's default; with every field
 * at its default each decision of the driver is what it is without the hook.
 *   general_min_n  sorts of at least this many records (and above the
 *                  single-workgroup capacity) skip both one-launch starts and
 *                  start with a plain level over one segment (default: off)
 *   balanced_min_n the fewest records for which the key sample is taken
 *                  (default 2^24)
 *   stripe_min_n   the fewest records for the stripe first level (default
 *                  2^25)
 *   stripe_pairs   the stripe length in tile pairs of 8192 records, 1 .. 244
 *                  (default: 3904 << b1 records, itself 61, 122 or 244 pairs
 *                  for the digit widths 7, 8, 9 the planner produces); the
 *                  rule n >= 2 stripes stays. A stripe level runs only after
 *                  a plain start.
 *   first_bits     the plain stripe level's digit width b1, 1 .. 9 (default:
 *                  chosen from n, 7 .. 9 at the sizes the planner takes
 *                  stripes at)
 * Returns SRS_ERR_INVALID_ARG for stripe_pairs > 244 or first_bits > 9. */
int srs_debug_set_first_level(int64_t general_min_n, int64_t balanced_min_n,
                              int64_t stripe_min_n, int64_t stripe_pairs, int first_bits);

/* What the last sort above the single-workgroup capacity did on the current
 * device: out[0] = its start (0 plain, 1 the mid-size launch, 2 the mid-level
 * launch; -1: no such sort has run), out[1] = the first level's kind (0 a
 * plain digit, 1 the 16-bit digit table, 3 the split table, 2 a range
 * level), out[2] = 1 when the stripe level and the gathered level ran,
 * out[3] = the stripe count K, out[4] = the stripe level's digit width b1,
 * out[5] = the gathered level's tile count (out[3..5] are 0 without
 * stripes). */
int srs_debug_last_first_level(int64_t* out);

/* Global levels run in this process so far (every device, every entry point
 * that takes the general level driver): counts[0] = all of them, counts[1] =
 * those scattered by the tile-pair kernel, counts[2] = of those, the ones
 * that ran without the tile-offset pass (the scatter summed its offsets from
 * the count rows; SRS_PAIR_ROW_OFFS=0 turns that off). Tests
 * take differences around a call to prove which path a sort took. */
int srs_debug_level_counts(int64_t* counts);

/* Segments the local-level fallback kernels took in the last sort on the
 * current device: counts[0] = handed to the stable kernel, counts[1] = handed
 * on to the LSD kernel. Synchronizes the device. Tests use it to prove that
 * an input exercised a given path. */
int srs_debug_last_fallbacks(int64_t* counts);

/* Local-level segment counts of the last (non-small) sort on the current
 * device: counts[0] = segments of the local level, counts[1] = of those, the
 * ones the direct local kernel handed to the fast kernel.
 * Synchronizes the device. Tests use it to prove the direct kernel ran. */
int srs_debug_last_local_counts(int64_t* counts);

/* The same by LDS class: counts[0] / counts[1] = small (<= 4096 records) /
 * large (<= 8192) segments of the local level, counts[2] / counts[3] = of
 * those, the ones the direct kernel of the class handed to the fast kernel.
 * Synchronizes the device. */
int srs_debug_last_local_classes(int64_t* counts);

/* Placement diagnostics. srs_debug_alloc allocates `bytes` of
 * device memory on the current device the way mode says (0 = hipMalloc,
 * 1 = physically contiguous, 2 = one hipMemCreate handle mapped at 1 GiB
 * alignment, 3 / 4 = 2 MB handles mapped in a shuffled order / in order; the
 * workspace's own big buffers follow SRS_WS_ALLOC = malloc|contig|vmm|
 * vmmshuf|vmm2m);
 * srs_debug_free releases it. srs_debug_workspace reports the current
 * device's TMP and TMP2 buffers (NULL / 0 when not allocated). */
int srs_debug_alloc(uint64_t bytes, int mode, void** ptr);
int srs_debug_free(void* ptr);
int srs_debug_workspace(void** tmp, uint64_t* tmp_bytes, void** tmp2, uint64_t* tmp2_bytes);
/* Milliseconds of one pass of the scatter's write pattern (512 runs of 8
 * elements per 4096-element tile into 16 MB windows) over [ptr, ptr + bytes)
 * of device memory: the rate the sort's scatter and local passes can write
 * that memory at. Synchronizes the device. */
int srs_debug_probe_write(void* ptr, uint64_t bytes, float* ms);

/* The balanced first level's digit table, planned on the host from a
 * 65536-bin histogram of the top 16 transformed key bits (the sample the
 * sort takes of large inputs) for `num` input keys of key_bits (32 / 64):
 * *mode 0 (no table), 1 (table = 65536 group ids, one per 16-bit bin) or 3
 * (table = 512 split entries: first group | lg << 16 per top-9-bit bin);
 * rbits = 512 per-group unsorted bit counts; *overflow = keys the next
 * level is predicted to leave above the LDS capacity (overflow_other: for
 * the other table). Host only (no GPU); tests check the plan with it. */
int srs_debug_plan_table(const uint32_t* hist, int64_t num, int key_bits, int32_t* mode,
                         int32_t* groups, double* overflow, double* overflow_other,
                         int32_t* table, int32_t* rbits);

/* Release cached device workspaces (for leak checks / shutdown). */
int srs_release_workspace(void);

/* Test hook, process-wide, like srs_debug_set_super_scan: the top-k select
 * stops refining once the boundary bucket holds <= max_candidates records
 * (<= 0 restores the default, 2^20), so that multi-pass refinement runs at
 * small n. */
int srs_debug_set_topk_candidates(int64_t max_candidates);

/* Select passes over the input and records handed to the finishing sort in
 * the last top-k on the current device (synchronizes the device). Tests use
 * it to prove which path an input took. info[0] = passes, info[1] = records
 * sorted, info[2] = 1 if the call took the full-sort route. */
int srs_debug_last_topk(int64_t* info);

/* Test hook, process-wide: the route srs_topk_rows_soa_device takes. -1: the
 * library's rule; 0: resident (row_len <= 8192), 1: stream (row_len > 8192,
 * min(k, row_len) <= srs_topk_rows_max_k()), 2: the row-by-row loop. A call
 * whose shape the forced route cannot take returns SRS_ERR_UNSUPPORTED. */
int srs_debug_set_topk_rows_route(int route);

/* What the last row-wise top-k on the current device did (synchronizes the
 * device): info[0] = route, info[1] = kernel launches enqueued (-1 on the
 * loop route: not counted), info[2] = the most select (histogram) passes over
 * the key row that any row needed (written by the kernel; 0: every row was
 * sorted whole), info[3] = host read-backs during the call. */
int srs_debug_last_topk_rows(int64_t* info);

/* Test hook, process-wide: the route srs_sort_rows_soa_device takes. -1: the
 * library's rule; 0: the rows kernel (row_len <= 8192), 1: the local lists
 * (2 <= row_len <= 8192), 2: the global levels (row_len > 8192). A call whose
 * shape the forced route cannot take returns SRS_ERR_UNSUPPORTED. Needs no
 * device. */
int srs_debug_set_sort_rows_route(int route);

/* What the last row-wise sort on the current device did (host state only: no
 * synchronization): info[0] = route, info[1] = kernel launches enqueued (-1:
 * not counted), info[2] = host read-backs during the call, info[3] = 1 if the
 * prepare pass ran (strided rows or an index column made dense). */
int srs_debug_last_sort_rows(int64_t* info);

/* Test hook, process-wide: the longest segment srs_sort_ragged_soa_device
 * leaves to its wave-per-segment kernel. -1: the default (256); 0: that
 * kernel is off (no launch, every segment of >= 1 record takes the work
 * lists); 1 .. 256: the maximum. Anything else returns SRS_ERR_INVALID_ARG.
 * Needs no device. */
int srs_debug_set_sort_ragged_short_max(int32_t len);

/* What the last ragged sort on the current device did (host state only: no
 * synchronization): info[0] = segments left to the short kernel
 * (num_segments - listed - empty - bad), info[1] / info[2] / info[3] = the
 * small-class / large-class / big list lengths as first read back, info[4] =
 * host read-backs during the call, info[5] = 1 if the prepare pass ran. */
int srs_debug_last_sort_ragged(int64_t* info);

/* Test hook, process-wide: the route srs_topk_ragged_soa_device takes. -1:
 * the library's rule; 0: the kernels (k <= srs_topk_rows_max_k(), num <
 * 2^31), 1: the ragged sort and the head copy. A call whose shape the forced
 * route cannot take returns SRS_ERR_UNSUPPORTED; any other value of the hook
 * returns SRS_ERR_INVALID_ARG. Needs no device. */
int srs_debug_set_topk_ragged_route(int route);

/* What the last ragged top-k on the current device did (synchronizes the
 * device): info[0] = route, info[1] = segments of 1 .. 256 records (the wave
 * kernel's), info[2] = longer segments (the list's), info[3] = the most
 * select (histogram) passes any listed segment took (written by the kernel;
 * 0 on the sort route), info[4] = host read-backs during the call, info[5] =
 * kernel launches queued (-1 on the sort route: not counted). */
int srs_debug_last_topk_ragged(int64_t* info);

/* What the last unique call on the current device did (host state only: no
 * synchronization): info[0] = launches the unique stage queued after the
 * sort (the tally, the scan, the write: 3), info[1] = its host read-backs (0
 * or 1), info[2] = 1 if an index column travelled through the sort, info[3]
 * = 1 if S went to workspace columns. */
int srs_debug_last_unique(int64_t* info);

/* Test hook, process-wide: the route srs_search_sorted_device takes in its
 * flat form. -1: the library's rule; 0: direct, the kernel runs on the
 * caller's queries; 1: the queries are sorted first, with an index column
 * (the hint SRS_SEARCH_QUERIES_SORTED is then ignored). The segmented form
 * is always route 0 and ignores the hook. Any other value returns
 * SRS_ERR_INVALID_ARG. Needs no device. */
int srs_debug_set_search_route(int route);

/* What the last search on the current device did (host state only: no
 * synchronization): info[0] = the route taken, info[1] = launches of the
 * search stage (the kernel, and the memset of num_bad_dev when given), info[2]
 * = host read-backs during the call (0 on route 0; -1 on route 1: the sort's,
 * not counted), info[3] = 1 if the queries were sorted by the call. */
int srs_debug_last_search(int64_t* info);

/* What the last merge on the current device did (host state only: no
 * synchronization): info[0] = launches queued (the descriptor, the split, the
 * tiles: 3), info[1] = host read-backs (0), info[2] = tiles, info[3] = bytes
 * of the workspace buffers the call uses (the split array and the column
 * descriptor, as allocated). */
int srs_debug_last_merge(int64_t* info);

#ifdef __cplusplus
}
#endif

#endif /* SRS_C_API_H_ */
