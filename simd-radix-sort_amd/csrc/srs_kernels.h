// srs_kernels.h — host-side launch wrappers for the kernels in srs_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srs_common.h"

namespace srs {

void launch_plan(const Seg* big, int64_t nbig, SegPlan* plan, int64_t* tcount,
                 int64_t* gcount, unsigned long long* var_or, uint64_t* elems, int force_bits,
                 int tmp2, hipStream_t st, const int32_t* nt_over = nullptr);
void launch_plan_small(const Seg* big, int64_t nbig, SegPlan* plan, int64_t* tbase,
                       int64_t* gbase, unsigned long long* var_or, uint64_t* totals,
                       unsigned long long* n_big_next, int force_bits, int tmp2,
                       hipStream_t st, const int32_t* nt_over = nullptr);
constexpr int64_t kPlanSmallMax = 16384;  // plan_small_kernel: one workgroup loops over these
void launch_seg_map2(const int64_t* tbase, int64_t ntiles, int32_t* tile_seg,
                     const int64_t* gbase, int64_t ngroups, int32_t* group_seg, int64_t nbig,
                     hipStream_t st);
void launch_start(const SortDesc& d, SortDesc* out, Seg seg0, int to_local, Seg* big, Seg* local,
                  Seg* local2, ListCounters* ctr, hipStream_t st);
void launch_plan_bases(SegPlan* plan, int64_t nbig, const int64_t* tbase,
                       const int64_t* gbase, hipStream_t st);
void launch_count(int key_size, const SortDesc* d, const SegPlan* plan,
                  const int32_t* tile_seg, int64_t ntiles, uint16_t* hist,
                  unsigned long long* var_or, unsigned long long* var_and, int lut,
                  hipStream_t st, const GTile* gt = nullptr, const int32_t* torder = nullptr);
int64_t scan_temp_elems(int64_t n);
void launch_excl_scan(const uint64_t* x, uint64_t* y, int64_t n, uint64_t* temp,
                      uint64_t* total, hipStream_t st);
// rows launch_offsets' super-group scan adds behind gsum's and gofs' group rows
int64_t super_rows(int64_t ngroups);
// the scan groups from which a one-segment level takes it (<= 0: the default, 256)
void set_super_scan_min_groups(int64_t g);
void launch_offsets(SegPlan* plan, int64_t nbig, const int32_t* group_seg, int64_t ngroups,
                    const uint16_t* hist, uint32_t* gsum, uint64_t* gofs, uint64_t* sbase,
                    uint64_t* offs, uint32_t* offs32, const unsigned long long* var_or,
                    Seg* big_next, Seg* local, Seg* local2, Seg* copy, ListCounters* ctr,
                    const int32_t* lut_rbits, hipStream_t st, int mode = 0,
                    uint32_t* prun = nullptr, bool tile_rows = true);  // false: no tile_offs_kernel
void launch_scatter(int key_size, const SortDesc* d, const SegPlan* plan,
                    const int32_t* tile_seg, const uint64_t* offs, const uint32_t* offs32,
                    int64_t ntiles, int lut, int ncols, hipStream_t st,
                    const GTile* gt = nullptr);
// the same level's scatter with two count tiles per workgroup (lut 0 or 2;
// 4- or 8-byte keys; the key plus one column or C2's pair word; no canon zero).
// row_hist != nullptr: a level without tile offset rows (launch_offsets'
// tile_rows off, segments < 2^32 keys): every workgroup sums its tiles'
// offsets from the count rows, the group offsets and the bucket bases
void launch_scatter_pairs(int key_size, const SortDesc* d, const SegPlan* plan,
                          const int32_t* tile_seg, const uint64_t* offs, const uint32_t* offs32,
                          int64_t ntiles, int lut, hipStream_t st, const GTile* gt = nullptr,
                          const uint16_t* row_hist = nullptr, const uint64_t* row_gofs = nullptr,
                          const uint64_t* row_sbase = nullptr);
// stripe first level -> the second level's segment list (W->big, n_big),
// tile counts (nt_over) and gathered tile table (gt); see GTile
void launch_stripe_tables(const uint32_t* prun, int64_t nstripes, int nb, uint32_t* ptile,
                          uint64_t* btot, uint32_t* bnt, int rbits, int buf, Seg* big,
                          int32_t* nt_over, uint32_t* btile, ListCounters* ctr,
                          const uint64_t* sbase, const SegPlan* plan, GTile* gt,
                          const int32_t* lut_rbits, hipStream_t st, int32_t* torder = nullptr,
                          int64_t tiles_cap = 0);  // torder: tiles_cap entries + nstripes of scratch
void launch_key_hist(int key_size, int64_t n, const void* keys, const SortDesc& d, int bits,
                     unsigned long long* hist, hipStream_t st);
// rec16: AoS records of 16 bytes held as two slice columns in TMP / TMP2
// (the local pass then writes whole records, one 16-byte store each)
void launch_local(int key_size, const SortDesc* d, const Seg* segs, int64_t nsegs, int big_class,
                  Seg* fallback, unsigned long long* fallback_count, hipStream_t st,
                  bool rec16 = false);
// the direct kernel (no canon-zero, 4/8-byte keys; pm 0: one 8-byte SoA
// payload, 1: 16-byte AoS records as slices, 2: desc->pair; big: the large
// class, up to kLocalCap records): segments it does not take go to `redo`,
// large buckets to `fallback`; launch_local_list then runs the fast kernel
// of the same class over `redo`
void launch_local_direct(int key_size, int pm, const SortDesc* d, const Seg* segs, int64_t nsegs,
                         Seg* redo, unsigned long long* redo_count, Seg* fallback,
                         unsigned long long* fallback_count, hipStream_t st, bool big = false);
void launch_local_list(int key_size, const SortDesc* d, const Seg* segs,
                       const unsigned long long* nsegs, int grid, Seg* fallback,
                       unsigned long long* fallback_count, hipStream_t st, bool big = false);
void launch_local_stable(int key_size, const SortDesc* d, const Seg* segs,
                         const unsigned long long* nsegs, int big_class, Seg* fallback,
                         unsigned long long* fallback_count, int grid, hipStream_t st);
// n <= kLocalCap: the whole sort in one single-workgroup launch
void launch_small_sort(int key_size, const SortDesc& d, Seg g, int64_t* taken, hipStream_t st);
// kLocalCap < n <= 64 tiles: one launch with grid barriers (mid_sort_kernel;
// every workgroup resident, else an error and the caller takes the general
// path); big buckets (> kLocalCap) are appended to `big` with ctr->n_big, and
// their count reaches the host early through `flag` (MidFlag, host memory).
// bar: mid_bar_words() u64 of device memory, zeroed once when allocated and
// left ready by every launch (a call whose barrier timed out posts its seq
// to flag->err). part: mid_part_bytes(n); hist: T x kMaxBins u32
constexpr int kMidMaxKeys = 256 * kTile;
int mid_bar_words();
int64_t mid_part_bytes(int64_t n);
hipError_t launch_mid_sort(int key_size, const SortDesc& d, int64_t n, int src,
                           unsigned long long* part, uint32_t* hist, ListCounters* ctr, Seg* big,
                           unsigned long long* taken, MidFlag* flag, unsigned long long seq,
                           unsigned long long* bar, hipStream_t st);
// kMidMaxKeys < n <= kMidLevelMaxKeys: the FIRST level in one launch
// (mid_level_kernel: count, column scans and scatter into TMP with grid
// barriers, the workgroups looping over tiles). The buckets go to the work
// lists as a level's would; their lengths reach the host through `flag`
// before the scatter ends (MidFlag n_big / n_local / n_local2 / n_copy), so
// the caller enqueues the LDS pass without a read-back. Writes the
// descriptor to d_out and resets ctr. part: mid_level_part_bytes(); hist: T x
// kMaxBins u32. Every workgroup resident, else an error (the general path).
constexpr int kMidLevelMaxKeys = 1024 * kTile;
int64_t mid_level_part_bytes();
hipError_t launch_mid_level(int key_size, const SortDesc& d, int64_t n, int src,
                            unsigned long long* part, uint32_t* hist, ListCounters* ctr, Seg* big,
                            Seg* local, Seg* local2, Seg* copy, SortDesc* d_out, MidFlag* flag,
                            unsigned long long seq, unsigned long long* bar, hipStream_t st);
void launch_local_lsd(int key_size, const SortDesc* d, const Seg* segs,
                      const unsigned long long* nsegs, int grid, hipStream_t st);
int64_t sample_partial_bytes();
void launch_key_minmax(const void* keys, int key_bytes, int elem_bytes, int64_t n, uint64_t mpos,
                       uint64_t mneg, const uint64_t* hi, unsigned long long* mm, hipStream_t st);
bool launch_sample_hist16(const void* keys, int key_bytes, int elem_bytes, int64_t n,
                          int64_t stride, int chunk, int64_t blocks, uint64_t mpos, uint64_t mneg,
                          uint32_t* partial, uint32_t* hist, hipStream_t st);
void launch_fill(int64_t n, int kind, uint64_t seed, uint64_t first, void* keys,
                 int npay, const Col* pays, hipStream_t st);
void launch_set_desc(const SortDesc& d, SortDesc* out, hipStream_t st);
// placement probe: ms of the scatter's write pattern over a buffer (sync)
float probe_write_ms(void* buf, size_t bytes, hipStream_t st);
// diagnostics: phase of each XCD's walk over its block range (xcd_remap)
void set_xcd_rotation(int mode);
// the copy list (finished segments not in OUT) home in one launch, column by
// column with each buffer's stride (AoS slice columns back into records)
// (chunks / cbase: nsegs u64 each; scan_temp: scan_temp_elems(nsegs) u64;
// total: one u64)
void launch_copy_list(const SortDesc* d, const Seg* segs, int64_t nsegs, uint64_t* chunks,
                      uint64_t* cbase, uint64_t* scan_temp, uint64_t* total, hipStream_t st);


// ---- top-k select ------------------------------------------
// What the select kernels know of the key column and of the prefix found so
// far: record i's key is at keys + i * stride; a key matches when its
// transformed bits u satisfy u >> psh == pv (all != 0: no prefix yet, every
// key matches).
struct SelectArgs {
  const char* keys;
  uint32_t stride;
  int32_t all;
  int64_t n;
  uint64_t pv;
  int32_t psh;
  int32_t shift, bits;  // select_hist: digit = (u >> shift) & (2^bits - 1), bits <= kHistMaxBits
  int32_t key_bits;
  uint64_t mpos, mneg;  // SortDesc's key transform
};
// select_hist's output row: 2^kHistMaxBits u64 bins, then the OR of the
// matching keys and the OR of their complements (zeroed by the caller)
constexpr int kSelOrSlot = 1 << kHistMaxBits;
constexpr int kSelHistWords = kSelOrSlot + 2;
void launch_select_hist(int key_size, const SelectArgs& a, unsigned long long* hist,
                        hipStream_t st);
// counts: 2 * ntiles u64 (ntiles = ceil(n / kTile)): per tile the keys below
// the prefix, then per tile the keys equal to it
void launch_select_tally(int key_size, const SelectArgs& a, uint64_t* counts, hipStream_t st);
// tbase: the exclusive scan of the tally's row; tbase == nullptr (with
// a.all): an ordered copy of the first `limit` records. Columns: d's BUF_IN
// -> BUF_OUT views, cols[0] the key column; no destination record >= limit
// is written.
void launch_select_gather(int key_size, const SelectArgs& a, const SortDesc* d,
                          const uint64_t* tbase, int64_t limit, int64_t* idx_out, hipStream_t st);

// ---- unique --------------------------------------------------
// The run boundaries of a SORTED key column (a.keys, a.stride, a.n; the
// prefix fields are unused): record i is a run head when i == 0 or its raw
// bits differ from record i - 1's.
// counts: ntiles u64 (ntiles = ceil(n / kTile)), the heads per tile
void launch_run_tally(int key_size, const SelectArgs& a, uint64_t* counts, hipStream_t st);
// tbase: the exclusive scan of the tally's counts, *total its total U. Head
// number j (record i) writes unique_out[j] = its key and offsets_out[j] = i
// (offsets_out or null; offsets_out[U] = n); with inverse_out, record i's run
// number goes to inverse_out[idx[i]] (idx: n int64, the records' input
// positions); num_unique (or null) receives U. No slot >= n (> n of
// offsets_out) is written.
void launch_run_write(int key_size, const SelectArgs& a, const uint64_t* tbase,
                      const uint64_t* total, void* unique_out, int64_t* offsets_out,
                      const int64_t* idx, int64_t* inverse_out, int64_t* num_unique,
                      hipStream_t st);

// ---- row-wise top-k ----------------------------------------
// One workgroup per row, everything decided on the device. Record i of row r
// of a column of width w is at in + (r * row_stride + i) * w; result j of row
// r at out + (r * kk + j) * w. col[0] is the key column.
struct TopkRowsCol {
  const char* in;
  char* out;
  uint32_t width;
};
struct TopkRowsArgs {
  int64_t rows, row_len, row_stride, kk;  // kk = min(k, row_len)
  int32_t ncols;
  int32_t key_bits;
  uint64_t mpos, mneg;  // SortDesc's key transform
  // LDS slots for the selected records (a power of two >= kk): the select
  // refines until the records below the boundary bucket and the bucket itself
  // fit. select == 0: the whole row fits, no histogram is allocated.
  int32_t cap;
  int32_t select;
  int64_t* idx_out;                 // or null
  unsigned long long* max_passes;   // the most select passes any row took (atomicMax)
  TopkRowsCol col[SRS_MAX_COLS];
};
// the most records a streamed row can select, and with it the largest kk of
// the stream route (a row's selected set is at most its kk - 1 sure records
// plus a boundary bucket: 2 * kTopkRowsMaxK slots always end the refinement)
constexpr int kTopkRowsMaxK = 2048;
constexpr int kTopkRowsStreamCap = 2 * kTopkRowsMaxK;
// below this many selected records a further select pass costs more than the
// LDS sort saves
constexpr int kTopkRowsMinCap = 256;
// rows up to this many records are sorted whole by one wave each, four rows
// to a workgroup
constexpr int kRowsWaveMax = 256;
// Fills a.cap and a.select for the shape and launches. stream == false:
// row_len <= kLocalCap, the row is held in registers; true: kk <=
// kTopkRowsMaxK and row_len < 2^31, the row is read from memory once per pass.
hipError_t launch_topk_rows(int key_size, TopkRowsArgs& a, bool stream, hipStream_t st);

// ---- row-wise sort -----------------------------------------
// The work list of `rows` dense rows of row_len records: row r becomes
// Seg{r * row_len, row_len, rbits, buf} at list[r], and *ctr the counters of
// that one list (cls 0: the small local class, 1: the large one, 2: the big
// list). list holds at least `rows` entries.
hipError_t launch_rows_segs(Seg* list, int64_t rows, int64_t row_len, int rbits, int buf, int cls,
                            ListCounters* ctr, hipStream_t st);
// Strided rows made dense: record i of row r of column c moves from
// col[c].in + (r * row_stride + i) * width to col[c].out + (r * row_len + i) *
// width; idx_out (or null) receives i at r * row_len + i.
struct RowsPrepareArgs {
  int64_t rows, row_len, row_stride;
  int32_t ncols;
  int64_t* idx_out;
  TopkRowsCol col[SRS_MAX_COLS];
};
hipError_t launch_rows_prepare(const RowsPrepareArgs& a, hipStream_t st);

// ---- ragged sort --------------------------------------------
// Segment i of nseg is records [offsets[i], offsets[i + 1]) of every column
// (dense, num records; col[0] the key column); offsets is a device array the
// kernels read. A segment is VALID when 0 <= offsets[i] <= offsets[i + 1] <=
// num; every kernel below tests that itself and touches no record of a
// segment that is not, so no column is accessed outside [0, num) whatever
// the offsets hold. SHORT segments (1 .. short_max records) belong to the
// short kernel, LISTED ones (more than short_max) to the work lists.
struct RaggedArgs {
  int64_t num, nseg;
  const int64_t* offsets;
  int32_t ncols;
  int32_t key_bits;
  uint64_t mpos, mneg;  // SortDesc's key transform
  int32_t short_max;    // 0 .. kRowsWaveMax (0: every segment of >= 1 record is listed)
  int64_t* idx_out;     // or null
  TopkRowsCol col[SRS_MAX_COLS];
};
// One wave per segment: every short segment sorted from col[].in to col[].out
// (and its in-segment positions to idx_out). a.short_max >= 1.
hipError_t launch_ragged_short(int key_size, const RaggedArgs& a, hipStream_t st);
// One thread per segment: listed segments go through emit_child as
// Seg{start, len, rbits, buf}; *ctr (zeroed by the caller) also counts the
// bad, the empty and the listed segments. At most `cap` segments are listed
// (valid offsets list at most num / (short_max + 1)); any further one counts
// as bad, so the lists need `cap` entries each.
hipError_t launch_ragged_segs(const int64_t* offsets, int64_t nseg, int64_t num, int short_max,
                              int rbits, int buf, int64_t cap, Seg* big, Seg* local, Seg* local2,
                              Seg* copy, ListCounters* ctr, hipStream_t st);
// The listed segments' records copied from col[].in to col[].out and their
// in-segment positions written to idx_out, element-parallel over [0, num);
// no position of a short, empty or bad segment, or outside the segments, is
// written.
hipError_t launch_ragged_prepare(const RaggedArgs& a, hipStream_t st);

// ---- ragged top-k --------------------------------------------
// The first min(k, len) records of every segment of §14's offsets: result j of
// segment i is at i * k + j of col[].out (and of idx_out), a fixed stride of k
// slots per segment; slots from min(k, len) on are never written. Validity
// is §14's: every kernel tests a segment's two offsets itself.
struct TopkRaggedCounters {
  unsigned long long n_bad;      // segments with a bad bound, or past the list's capacity
  unsigned long long n_empty;
  unsigned long long n_short;    // valid, 1 .. kRowsWaveMax records: the wave kernel's
  unsigned long long n_long;     // valid and longer: entries of the list
  unsigned long long n_offer;    // long segments that asked for a list slot
  unsigned long long max_passes; // the most select passes any listed segment took
};
struct TopkRaggedArgs {
  int64_t num, nseg, k;
  const int64_t* offsets;
  int32_t ncols;
  int32_t key_bits;
  uint64_t mpos, mneg;  // SortDesc's key transform
  int32_t cap;          // the long kernel's LDS slots (launch-wide, from k alone)
  int64_t* idx_out;     // or null
  int64_t* counts_out;  // or null: min(k, len) per valid segment, 0 for the others
  // the indices of the segments longer than kRowsWaveMax, list_cap entries
  // (null: nothing is listed, the sort route)
  int64_t* list;
  unsigned long long list_cap;
  TopkRaggedCounters* ctr;  // zeroed by the caller
  // the sort route's head copy: the sorted columns are col[].in, and the
  // sorted in-segment positions idx_in (or null)
  const int64_t* idx_in;
  TopkRowsCol col[SRS_MAX_COLS];
};
// One thread per segment: counts_out, the counters, and the list of long
// segments. At most list_cap segments are listed (valid offsets give no more
// than num / (kRowsWaveMax + 1) long segments); any further one counts as bad.
hipError_t launch_topk_ragged_classify(const TopkRaggedArgs& a, hipStream_t st);
// One wave per segment: every valid segment of 1 .. kRowsWaveMax records
// sorted whole in LDS, its first min(k, len) records written.
hipError_t launch_topk_ragged_short(int key_size, const TopkRaggedArgs& a, hipStream_t st);
// One workgroup per listed segment, grid-stride over the list, whose length
// it reads from a.ctr->n_long: §12's streamed select with the segment's own
// length. Fills a.cap from a.k (k <= kTopkRowsMaxK, num < 2^31).
hipError_t launch_topk_ragged_long(int key_size, TopkRaggedArgs& a, hipStream_t st);
// The sort route: record j < min(k, len) of every valid segment copied from
// col[].in + (start + j) to col[].out + (i * k + j) (idx_in to idx_out
// likewise), element-parallel over [0, num).
hipError_t launch_topk_ragged_heads(const TopkRaggedArgs& a, hipStream_t st);

// ---- search-sorted -------------------------------------------
// The lower and upper bounds of nq query keys in a dense column of num keys
// whose transformed keys do not decrease. Query j's results go to slot j of
// lower / upper (either may be null), or to slot idx[j] when idx is given
// (the sort route: queries is then the sorted copy, idx its input positions;
// no slot >= nq is written). Segmented (offsets != null): query j is searched
// in [offsets[qseg[j]], offsets[qseg[j] + 1]) and its results are positions
// inside that segment; a query whose id is outside [0, nseg) or whose segment
// has a bad bound (§14's rule) receives -1 and adds one to *num_bad (or null;
// zeroed by the caller). No key outside [0, num) is read whatever the table,
// the offsets and the ids hold, and every result lies in [0, num] ([0, len]).
struct SearchArgs {
  const char* keys;
  int64_t num;
  const char* queries;
  int64_t nq;
  const int64_t* idx;      // or null
  int64_t* lower;          // or null
  int64_t* upper;          // or null
  const int64_t* offsets;  // or null: the flat form
  const int64_t* qseg;
  int64_t nseg;
  int64_t* num_bad;        // or null
  int32_t key_bits;
  uint64_t mpos, mneg;     // SortDesc's key transform
};
constexpr int kSearchThreads = 256;
constexpr int kSearchItems = 4;
constexpr int kSearchTile = kSearchThreads * kSearchItems;  // queries per workgroup
// the LDS sample's slots; a tile whose table range has at most kSearchFit keys
// stages the range itself
constexpr int kSearchSamples = 2048;
constexpr int kSearchFit = kSearchSamples - 1;
hipError_t launch_search(int key_size, const SearchArgs& a, hipStream_t st);

// ---- merge ---------------------------------------------------
// The stable merge of two dense record sets A (num_a) and B (num_b) whose
// transformed keys do not decrease, A's records first among equal keys. The
// columns travel in *desc: column c of A is cols[c]'s BUF_IN view, of B its
// BUF_TMP view, of the output its BUF_OUT view (dense: stride == width;
// cols[0] the key column). split: ntiles + 1 int64, ntiles = ceil((num_a +
// num_b) / kMergeTile): split[t] = the records of A among the first min(t *
// kMergeTile, n) of the output. source (or null) receives every output
// record's position in A followed by B. No record outside [0, num_a) of A,
// [0, num_b) of B and [0, num_a + num_b) of the outputs is accessed whatever
// the keys and the split array hold.
struct MergeArgs {
  int64_t num_a, num_b;
  const SortDesc* desc;
  int64_t* split;
  int64_t* source;      // or null
  int32_t key_bits;
  uint64_t mpos, mneg;  // SortDesc's key transform
};
constexpr int kMergeThreads = 256;
constexpr int kMergeItems = 16;
constexpr int kMergeTile = kMergeThreads * kMergeItems;  // output records per workgroup
// One thread per tile boundary: the merge path's diagonal bisected.
hipError_t launch_merge_split(int key_size, const MergeArgs& a, hipStream_t st);
// One workgroup per tile: both key ranges staged in LDS, ranked against each
// other, every column written in output order.
hipError_t launch_merge_tile(int key_size, const MergeArgs& a, hipStream_t st);

}  // namespace srs
