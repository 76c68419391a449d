// srs_batch.hip — the batched calls on top of the sort driver (srs_driver.h):
// top-k, row-wise top-k, row-wise sort, ragged sort, ragged top-k, unique and
// search-sorted, with their validation, C entry points and debug hooks.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <thread>

#include "srs_driver.h"

namespace srs {
namespace {

// ---------------------------------------------------------------------------
// top-k: select the records that can be among the first k by
// walking down the key's digits, compact them in input order, sort that set
// ---------------------------------------------------------------------------
// The select stops refining once the boundary bucket holds this many
// records: the finishing sort of k + 2^20 records of a small k is then the
// single-launch sort (kMidMaxKeys), ~0.1 ms, where one more pass would read
// the whole key column again (srs_debug_set_topk_candidates).
constexpr int64_t kTopkCandidates = kMidMaxKeys;
std::atomic<int64_t> g_topk_candidates{kTopkCandidates};
// Above k = num / 2 the select saves less than it costs: those calls sort
// everything. Measured at 1e9 u64 + u64 records the two routes cross at
// k = 0.52-0.54 num (the byte model, 24 n + 176 k against the
// sort's 112 n + 32 k, said 0.61); at num / 2 the select still wins by 3-6 %.
// Inputs of one local sort (num <= kLocalCap) are sorted whole as well.
constexpr int64_t kTopkFullPercent = 50;
// (SRS_TOPK_FULL_PCT overrides the percentage, for crossover measurements:
// tools/topk_bench.py; read on every call)
int64_t topk_full_percent() { return knob_int("SRS_TOPK_FULL_PCT", kTopkFullPercent); }

// The columns a top-k call moves, with their views in the input and in the
// caller's output: SoA columns as they are; an AoS record as its key and the
// rest of its bytes in aligned power-of-two pieces of up to 8 bytes, so that
// the compact set is always SoA columns with the key column first.
struct TopkLayout {
  int nc = 0;
  uint32_t width[SRS_MAX_COLS];
  char* in[SRS_MAX_COLS];
  char* out[SRS_MAX_COLS];
  uint32_t stride[SRS_MAX_COLS];  // of both views
};

void topk_layout(const Request& R, TopkLayout& L) {
  if (!R.aos) {
    L.nc = R.ncols;
    for (int c = 0; c < R.ncols; c++) {
      L.width[c] = L.stride[c] = R.widths[c];
      L.in[c] = (char*)R.in_cols[c];
      L.out[c] = (char*)R.out_cols[c];
    }
    return;
  }
  const uint32_t E = R.elem_size;
  uint32_t off = 0, w = (uint32_t)key_size_of(R.kind);
  while (off < E) {
    L.width[L.nc] = w;
    L.stride[L.nc] = E;
    L.in[L.nc] = (char*)R.in_cols[0] + off;
    L.out[L.nc] = (char*)R.out_cols[0] + off;
    L.nc++;
    off += w;
    w = std::min<uint32_t>(8, off & (~off + 1));  // (E is a power of two: never past the record)
  }
}

// The gather's descriptor (W->seldesc): d's first nc columns, the key first.
void set_gather_desc(Workspace* W, SortDesc& d, int nc, hipStream_t st) {
  d.key = d.cols[0];
  d.ncols = nc;
  launch_set_desc(d, (SortDesc*)W->seldesc.p, st);
}

// (under the caller's workspace lock and WsUse)
int topk_locked(Workspace* W, const Request& R, int64_t k, int64_t* idx_out, hipStream_t st) {
  const int64_t n = R.num;
  k = std::min(k, n);
  const int ks = key_size_of(R.kind);
  const bool full = n <= kLocalCap || (__int128)k * 100 > (__int128)n * topk_full_percent();
  if (k >= n && !idx_out) {  // the plain out-of-place sort
    W->topk_info[0] = 0;
    W->topk_info[1] = n;
    W->topk_info[2] = 1;
    return sort_locked(W, R, st);
  }
  TopkLayout L;
  topk_layout(R, L);
  SortDesc kd = init_desc(R.kind, R.up);
  SelectArgs a;
  memset(&a, 0, sizeof a);
  a.keys = L.in[0];
  a.stride = L.stride[0];
  a.n = n;
  a.all = 1;
  a.key_bits = kd.key_bits;
  a.mpos = kd.mpos;
  a.mneg = kd.mneg;

  // ---- which records: the prefix of the boundary bucket ---------------------
  int64_t passes = 0, limit = n;  // limit: records the compact set holds
  if (!full) {
    SRS_TRY(ensure(W->selhist, kSelHistWords * sizeof(uint64_t)));
    if (!W->h_sel)
      HIP_TRY(hipHostMalloc((void**)&W->h_sel, kSelHistWords * sizeof(uint64_t), hipHostMallocDefault));
    const int kb = kd.key_bits;
    const uint64_t kmask = kb == 64 ? ~0ull : ((1ull << kb) - 1);
    const int64_t maxc = g_topk_candidates.load();
    uint64_t prefix = 0;  // the fixed top bits, in place
    int fixed = 0, top = kb;  // the next digit ends below bit `top`
    int64_t k_rem = k, cand = n;  // the rank wanted inside the prefix's bucket; its size
    bool resolved = false;        // the bucket's keys are all equal
    for (;;) {
      a.bits = std::min(kHistMaxBits, top);
      a.shift = top - a.bits;
      a.all = fixed == 0;
      a.psh = fixed ? kb - fixed : 0;
      a.pv = fixed ? prefix >> a.psh : 0;
      HIP_TRY(hipMemsetAsync(W->selhist.p, 0, kSelHistWords * sizeof(uint64_t), st));
      {
        TimedScope ts("select_hist", (double)n, st);
        launch_select_hist(ks, a, (unsigned long long*)W->selhist.p, st);
      }
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(W->h_sel, W->selhist.p, kSelHistWords * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, st));
      SRS_TRY(sync_poll(st));
      passes++;
      const unsigned long long* h = W->h_sel;
      int64_t below = 0;
      int b = 0;
      const int nb = 1 << a.bits;
      for (; b < nb; b++) {
        if (below + (int64_t)h[b] >= k_rem) break;
        below += (int64_t)h[b];
      }
      if (b == nb) return fail(SRS_ERR_INTERNAL, "top-k: the histogram holds fewer keys than its bucket");
      k_rem -= below;
      cand = (int64_t)h[b];
      prefix |= (uint64_t)b << a.shift;
      fixed = kb - a.shift;
      // where the bucket's parent still varies below this digit: the next
      // digit starts at its highest varying bit, the bits between are shared
      const uint64_t low = (1ull << a.shift) - 1;  // (shift <= 52)
      const uint64_t vand = ~h[kSelOrSlot + 1] & kmask;
      const uint64_t var = (h[kSelOrSlot] ^ vand) & low;
      if (var == 0) {
        resolved = true;
        prefix |= vand & low;
        fixed = kb;
      }
      if (resolved || cand == k_rem || cand <= maxc) break;
      const int hb = 63 - __builtin_clzll(var);
      prefix |= vand & low & ~((2ull << hb) - 1);
      fixed = kb - (hb + 1);
      top = hb + 1;
    }
    a.all = 0;
    a.psh = kb - fixed;
    a.pv = prefix >> a.psh;
    // everything below the prefix, and the bucket itself (a bucket of equal
    // keys: only its first k_rem records, in input order)
    limit = (k - k_rem) + (resolved ? k_rem : cand);
  }
  const int64_t m = limit;

  // ---- the compact columns ---------------------------------------------------
  const int nsc = L.nc + (idx_out ? 1 : 0);
  size_t off[SRS_MAX_COLS + 1], bytes = 0;
  for (int c = 0; c < nsc; c++) {
    off[c] = bytes;
    bytes += align_up((size_t)m * (c < L.nc ? L.width[c] : 8), 256);
  }
  SRS_TRY(ensure(W->sel, bytes, ws_alloc_mode()));
  SRS_TRY(ensure(W->seldesc, sizeof(SortDesc)));
  char* sel = (char*)W->sel.p;
  int64_t* sel_idx = idx_out ? (int64_t*)(sel + off[L.nc]) : nullptr;
  Request S;  // the compact set's sort, in place
  S.num = m;
  S.kind = R.kind;
  S.up = R.up;
  S.thresh = 0;  // (the total order for floats at every size)
  S.aos = false;
  S.elem_size = 0;
  S.ncols = nsc;
  for (int c = 0; c < nsc; c++) {
    S.in_cols[c] = S.out_cols[c] = sel + off[c];
    S.widths[c] = c < L.nc ? L.width[c] : 8;
  }
  W->topk_info[0] = passes;
  W->topk_info[1] = m;
  W->topk_info[2] = full ? 1 : 0;

  if (full && !R.aos && !idx_out) {
    // SoA columns: sorted straight into the compact columns
    Request F = R;
    F.thresh = 0;
    for (int c = 0; c < nsc; c++) F.out_cols[c] = S.out_cols[c];
    SRS_TRY(sort_locked(W, F, st));
  } else {
    SortDesc d = init_desc(R.kind, R.up);
    for (int c = 0; c < L.nc; c++)
      d.cols[c] = Col{{L.in[c], sel + off[c], nullptr, nullptr}, L.width[c],
                      {L.stride[c], L.width[c], L.width[c], L.width[c]}};
    set_gather_desc(W, d, L.nc, st);
    const uint64_t* tbase = nullptr;
    if (!full) {
      const int64_t ntiles = (n + kTile - 1) / kTile;
      const int64_t rows = 2 * ntiles;
      SRS_TRY(ensure(W->selcnt, (size_t)(2 * rows + scan_temp_elems(rows) + 1) * sizeof(uint64_t)));
      uint64_t* counts = (uint64_t*)W->selcnt.p;
      uint64_t* bases = counts + rows;
      uint64_t* temp = bases + rows;
      {
        TimedScope ts("select_tally", (double)n, st);
        launch_select_tally(ks, a, counts, st);
      }
      launch_excl_scan(counts, bases, rows, temp, temp + scan_temp_elems(rows), st);
      tbase = bases;
    }
    {
      TimedScope ts("select_gather", (double)m, st);
      launch_select_gather(ks, a, (const SortDesc*)W->seldesc.p, tbase, limit, sel_idx, st);
    }
    HIP_TRY(hipGetLastError());
    SRS_TRY(sort_locked(W, S, st));
  }

  // ---- the first k records to the caller's arrays ----------------------------
  SortDesc d = init_desc(R.kind, R.up);
  for (int c = 0; c < nsc; c++) {
    const uint32_t w = S.widths[c];
    char* out = c < L.nc ? L.out[c] : (char*)idx_out;
    d.cols[c] = Col{{sel + off[c], out, nullptr, nullptr}, w, {w, c < L.nc ? L.stride[c] : 8u, w, w}};
  }
  set_gather_desc(W, d, nsc, st);
  SelectArgs f = a;
  f.keys = sel;
  f.stride = (uint32_t)ks;
  f.n = k;
  f.all = 1;
  {
    TimedScope ts("select_gather", (double)k, st);
    launch_select_gather(ks, f, (const SortDesc*)W->seldesc.p, nullptr, k, nullptr, st);
  }
  HIP_TRY(hipGetLastError());
  return SRS_OK;
}

int topk_device(const Request& R, int64_t k, int64_t* idx_out, hipStream_t st) {
  WsScope ws;
  SRS_TRY(ws.begin(st));
  return topk_locked(ws.W, R, k, idx_out, st);
}

// ---- validation of the out-of-place calls -------------------------------------
// What they check of their arrays, all before the first device access (the
// alignment rule: check_col_alignment, srs_api.hip).
struct OutCheck {
  const char* what;        // the call's name in the overlap message
  const void* out0;        // the key (or record) output
  const int64_t* idx_out;  // or null
  int64_t in_recs, out_recs;  // records the inputs hold and the outputs receive
  bool rows;               // a row-wise or ragged call (its alignment message)
  const char* shape_err;   // the caller's shape error, or null
};

// Some output's first out_recs records (indices_out last) overlap [p, p + bytes).
bool outputs_overlap(const Request& R, const int64_t* idx_out, int64_t out_recs, const void* p,
                     size_t bytes) {
  for (int o = 0; o <= R.ncols; o++) {
    const uintptr_t x = (uintptr_t)(o < R.ncols ? R.out_cols[o] : (const void*)idx_out);
    const size_t xn = (size_t)out_recs * (o < R.ncols ? R.widths[o] : 8);
    const uintptr_t y = (uintptr_t)p;
    if (x && xn && bytes && x < y + bytes && y < x + xn) return true;
  }
  return false;
}

// In order: the column count with indices_out; then, unless out_recs <= 0
// (the call will do nothing), the caller's shape error if any, NULL arrays,
// alignment, and the outputs' out_recs records clear of the inputs' in_recs.
int validate_outputs(const Request& R, const OutCheck& A) {
  if (A.idx_out && !R.aos && R.ncols - 1 > SRS_MAX_PAYLOADS - 1)
    return fail(SRS_ERR_UNSUPPORTED,
                "indices_out travels as one more payload column: at most 63 payload columns "
                "with it");
  if (A.out_recs <= 0) return SRS_OK;
  if (A.shape_err) return fail(SRS_ERR_INVALID_ARG, A.shape_err);
  if (!R.in_cols[0]) return fail(SRS_ERR_INVALID_ARG, R.aos ? "elements is NULL" : "keys is NULL");
  if (!A.out0) return fail(SRS_ERR_INVALID_ARG, R.aos ? "elements_out is NULL" : "keys_out is NULL");
  for (int c = 0; c < R.ncols; c++) {
    if (!R.in_cols[c] || !R.out_cols[c]) return fail(SRS_ERR_INVALID_ARG, "payload pointer is NULL");
    SRS_TRY(check_col_alignment(R, c, A.rows));
  }
  if ((uintptr_t)A.idx_out % 8 != 0) return fail(SRS_ERR_INVALID_ARG, "indices_out must be 8-byte aligned");
  for (int c = 0; c < R.ncols; c++)
    if (outputs_overlap(R, A.idx_out, A.out_recs, R.in_cols[c], (size_t)A.in_recs * R.widths[c]))
      return fail(SRS_ERR_INVALID_ARG, std::string(A.what) + " outputs must not overlap the inputs");
  return SRS_OK;
}

int topk_validate(const Request& R, int64_t k, const void* out0, const int64_t* idx_out) {
  return validate_outputs(R, {"top-k", out0, idx_out, R.num, std::min(k, R.num), false, nullptr});
}

// The row-wise calls: R describes one row (R.num = row_len; the columns
// point at row 0), kk the records every row writes.
int rows_validate(const char* what, const Request& R, int64_t rows, int64_t row_stride, int64_t kk,
                  const void* out0, const int64_t* idx_out) {
  const bool work = rows > 0 && R.num > 0 && kk > 0;
  int64_t cells = 0;
  const char* shape = row_stride < R.num ? "row_stride < row_len"
                      : __builtin_mul_overflow(rows, row_stride, &cells) || cells > (INT64_MAX >> 4)
                          ? "rows * row_stride overflows"
                          : nullptr;
  if (!work || shape) return validate_outputs(R, {what, out0, idx_out, 0, work, true, shape});
  return validate_outputs(
      R, {what, out0, idx_out, (rows - 1) * row_stride + R.num, rows * kk, true, nullptr});
}

// ---------------------------------------------------------------------------
// row-wise top-k: the first k records of every row of a
// matrix. Rows that fit one workgroup's registers (resident) and longer rows
// with k <= kTopkRowsMaxK (stream) take one launch, a workgroup per row, with
// nothing read back; everything else goes row by row through topk_locked.
// ---------------------------------------------------------------------------
enum { ROWS_RESIDENT = 0, ROWS_STREAM = 1, ROWS_LOOP = 2 };
std::atomic<int> g_topk_rows_route{-1};  // srs_debug_set_topk_rows_route
// The stream route puts one workgroup on a row, so a few very long rows leave
// most of the chip idle while the loop's select runs each row on all of it.
// Measured (tools/topk_rows_bench.py --sweep): the routes
// cross at 11-16 rows of 2^20 records, 35-49 of 2^22, 116-129 of 2^24 and
// ~350 of 2^26, i.e. near 12 * (row_len / 2^20)^0.8 rows; below that many
// rows the loop is taken. Rows shorter than 2^20 were not measured: stream.
constexpr int64_t kTopkRowsLoopLen = int64_t(1) << 20;
bool topk_rows_prefers_loop(int64_t rows, int64_t row_len) {
  if (row_len < kTopkRowsLoopLen) return false;
  return (double)rows < 12.0 * std::pow((double)row_len / (double)kTopkRowsLoopLen, 0.8);
}

// What TopkRowsArgs, RowsPrepareArgs and RaggedArgs share: zeroed, then the
// request's columns and the index output.
template <class Args>
void init_rows_args(Args& a, const Request& R, int64_t* idx_out) {
  memset(&a, 0, sizeof a);
  a.ncols = R.ncols;
  a.idx_out = idx_out;
  for (int c = 0; c < R.ncols; c++)
    a.col[c] = TopkRowsCol{(const char*)R.in_cols[c], (char*)R.out_cols[c], R.widths[c]};
}

// The request sorted in place on its outputs, where a prepare pass has put
// the records, with idx_out (or null) as one more 8-byte payload column.
void sort_outputs_in_place(Request& Q, int64_t* idx_out) {
  for (int c = 0; c < Q.ncols; c++) Q.in_cols[c] = Q.out_cols[c];
  if (!idx_out) return;
  Q.in_cols[Q.ncols] = Q.out_cols[Q.ncols] = idx_out;
  Q.widths[Q.ncols++] = 8;
}

// The one-launch routes' kernel (launch_topk_rows): the first kk records of
// every row's sorted order, kk <= row_len (kk == row_len: the rows sorted
// whole). pass: the buffer of the kernel's pass counter.
int launch_rows_kernel(DevBuf& pass, const Request& R, int64_t rows, int64_t row_stride,
                       int64_t kk, int64_t* idx_out, bool stream, hipStream_t st) {
  SRS_TRY(ensure(pass, sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(pass.p, 0, sizeof(unsigned long long), st));
  SortDesc kd = init_desc(R.kind, R.up);
  TopkRowsArgs a;
  init_rows_args(a, R, idx_out);
  a.rows = rows;
  a.row_len = R.num;
  a.row_stride = row_stride;
  a.kk = kk;
  a.key_bits = kd.key_bits;
  a.mpos = kd.mpos;
  a.mneg = kd.mneg;
  a.max_passes = (unsigned long long*)pass.p;
  {
    TimedScope ts("topk_rows", (double)rows * (double)R.num, st);
    HIP_TRY(launch_topk_rows(key_size_of(R.kind), a, stream, st));
  }
  return SRS_OK;
}

int topk_rows_device(const Request& R, int64_t rows, int64_t row_stride, int64_t k,
                     int64_t* idx_out, hipStream_t st) {
  const int64_t n = R.num, kk = std::min(k, n);
  const bool can_resident = n <= kLocalCap;
  const bool can_stream = !can_resident && kk <= kTopkRowsMaxK && n < (int64_t(1) << 31);
  int route = g_topk_rows_route.load();
  if (route < 0) {
    route = can_resident ? ROWS_RESIDENT
            : can_stream && !topk_rows_prefers_loop(rows, n) ? ROWS_STREAM
                                                                                  : ROWS_LOOP;
  } else if (route == ROWS_RESIDENT && !can_resident) {
    return fail(SRS_ERR_UNSUPPORTED, "top-k rows: the resident route takes row_len <= 8192");
  } else if (route == ROWS_STREAM && !can_stream) {
    return fail(SRS_ERR_UNSUPPORTED,
                "top-k rows: the stream route takes 8192 < row_len < 2^31 and min(k, row_len) <= "
                "kTopkRowsMaxK");
  }
  WsScope ws;
  SRS_TRY(ws.begin(st));
  Workspace* W = ws.W;
  int64_t* info = W->topk_rows_info;
  info[0] = route;
  info[1] = info[2] = info[3] = 0;

  if (route == ROWS_LOOP) {
    // correct and slow: every row is one single-array top-k, with its select
    // passes' read-backs (info[1]: its launches are not counted)
    info[1] = -1;
    for (int64_t r = 0; r < rows; r++) {
      Request Q = R;
      for (int c = 0; c < R.ncols; c++) {
        Q.in_cols[c] = (char*)R.in_cols[c] + r * row_stride * (int64_t)R.widths[c];
        Q.out_cols[c] = (char*)R.out_cols[c] + r * kk * (int64_t)R.widths[c];
      }
      SRS_TRY(topk_locked(W, Q, k, idx_out ? idx_out + r * kk : nullptr, st));
      info[2] = std::max(info[2], W->topk_info[0]);
      info[3] += W->topk_info[0];
    }
    W->rows_pass_pending = false;
    return SRS_OK;
  }

  SRS_TRY(launch_rows_kernel(W->rowspass, R, rows, row_stride, kk, idx_out, route == ROWS_STREAM,
                             st));
  info[1] = 1;
  W->rows_pass_pending = true;
  return SRS_OK;
}

// ---------------------------------------------------------------------------
// row-wise sort: every row of a matrix sorted, out of place.
// Route 0 is the rows kernel above with kk = row_len; routes 1 and 2 make the
// rows segments of the sort's work lists on the device (launch_rows_segs) and
// run the sort's own LDS chain / global levels over them.
// ---------------------------------------------------------------------------
enum { SORT_ROWS_KERNEL = 0, SORT_ROWS_LOCAL = 1, SORT_ROWS_LEVELS = 2 };
std::atomic<int> g_sort_rows_route{-1};  // srs_debug_set_sort_rows_route
// Rows of 257 .. kLocalCap records: the rows kernel below this length, the
// local lists from it. Measured at 2^26 records (tools/sort_rows_bench.py
// --sweep): the rows kernel sorts a row padded to a power of
// two and wins at 1024 records and below on every column set; from 1025 the
// chain's direct kernel (a 4- or 8-byte key and one 8-byte payload, no index
// column) wins at every length measured, 1.13x at 1025 to 3.2x at 8192. The
// chain's general kernel, which every other column set takes, wins once the
// rows kernel pads past 4096 records (2.1x at 4097) but loses 1.5-2.3x at
// 1152-2048: those sets cross at kSortRowsLocalMinGeneral.
constexpr int64_t kSortRowsLocalMin = 1025;
constexpr int64_t kSortRowsLocalMinGeneral = kLocalCapSmall + 1;
int64_t sort_rows_local_min(const Request& R, bool with_indices) {
  const int ks = key_size_of(R.kind);
  const bool direct = !with_indices && R.ncols == 2 && R.widths[1] == 8 && (ks == 4 || ks == 8);
  return direct ? kSortRowsLocalMin : kSortRowsLocalMinGeneral;
}

// Routes 1 and 2. Q is the whole matrix as one request of dense columns
// (Q.num = rows * row_len; the index column, when asked for, is its last
// payload): in place on the outputs after the prepare pass (IN aliases OUT,
// the segments start in OUT), or out of place from the caller's dense input
// (the segments start in IN). *readbacks: host waits of the levels.
int sort_rows_lists(Workspace* W, const Request& Q, int64_t rows, int64_t row_len,
                    int64_t* readbacks, hipStream_t st) {
  W->last_small = false;
  const bool inplace = is_inplace(Q);
  // ---- the lists: one segment per row, all in one list ----------------------
  const int cls = row_len > kLocalCap ? 2 : row_len > kLocalCapSmall ? 1 : 0;
  SRS_TRY(ensure_lists(W, cls == 2 ? rows : 0, cls == 0 ? rows : 0, cls == 1 ? rows : 0));
  SortDesc d;
  SortDesc* d_desc = nullptr;
  SRS_TRY(list_begin(W, Q, inplace, cls == 2, st, &d, &d_desc));
  Seg* list = (Seg*)(cls == 2 ? W->big[0].p : cls == 1 ? W->local2.p : W->local.p);
  HIP_TRY(launch_rows_segs(list, rows, row_len, d.key_bits, inplace ? BUF_OUT : BUF_IN, cls,
                           (ListCounters*)W->ctr.p, st));
  W->h_ctr->local_elems = cls == 2 ? 0 : (uint64_t)Q.num;
  const LevelState S = level_state(d, key_size_of(Q.kind), false, cls == 2 ? rows : 0,
                                   cls == 0 ? rows : 0, cls == 1 ? rows : 0, 0, row_len);
  return list_finish(W, Q, d, d_desc, S, 0, false, readbacks, st);
}

// R describes one row (R.num = row_len; the columns point at row 0).
int sort_rows_device(const Request& R, int64_t rows, int64_t row_stride, int64_t* idx_out,
                     hipStream_t st) {
  const int64_t len = R.num;
  int route = g_sort_rows_route.load();
  if (route < 0) {
    route = len > kLocalCap ? SORT_ROWS_LEVELS
            : len <= kRowsWaveMax || len < sort_rows_local_min(R, idx_out != nullptr)
                ? SORT_ROWS_KERNEL
                : SORT_ROWS_LOCAL;
  } else if (route == SORT_ROWS_KERNEL && len > kLocalCap) {
    return fail(SRS_ERR_UNSUPPORTED, "sort rows: the rows kernel takes row_len <= 8192");
  } else if (route == SORT_ROWS_LOCAL && (len < 2 || len > kLocalCap)) {
    return fail(SRS_ERR_UNSUPPORTED, "sort rows: the local lists take 2 <= row_len <= 8192");
  } else if (route == SORT_ROWS_LEVELS && len <= kLocalCap) {
    return fail(SRS_ERR_UNSUPPORTED, "sort rows: the levels take row_len > 8192");
  }
  WsScope ws;
  SRS_TRY(ws.begin(st));
  Workspace* W = ws.W;
  int64_t* info = W->sort_rows_info;
  info[0] = route;
  info[1] = info[2] = info[3] = 0;

  if (route == SORT_ROWS_KERNEL) {
    SRS_TRY(launch_rows_kernel(W->sortrowspass, R, rows, row_stride, len, idx_out, false, st));
    info[1] = 1;
    return SRS_OK;
  }

  info[1] = -1;  // (the chain's launches are not counted)
  Request Q = R;
  Q.num = rows * len;
  const bool prepare = row_stride != len || idx_out != nullptr;
  if (prepare) {
    // strided rows and the index column land dense in the outputs, which are
    // then sorted in place (no workspace column, and the
    // in-place segment lists are the ones srs_sort_segments_device runs)
    RowsPrepareArgs a;
    init_rows_args(a, R, idx_out);
    a.rows = rows;
    a.row_len = len;
    a.row_stride = row_stride;
    {
      TimedScope ts("rows_prepare", (double)Q.num, st);
      HIP_TRY(launch_rows_prepare(a, st));
    }
    info[3] = 1;
    sort_outputs_in_place(Q, idx_out);
  }
  return sort_rows_lists(W, Q, rows, len, &info[2], st);
}

// ---------------------------------------------------------------------------
// ragged sort: segments [offsets[i], offsets[i + 1]) of dense
// columns, the offsets on the device. One classify pass (ragged_segs_kernel)
// lists the segments longer than short_max and counts the bad and the empty
// ones; its counters come back through W->h_ctr while the short kernel, which
// owns every segment of 1 .. short_max records, is already queued behind the
// copy. Listed segments then run the sort's levels and LDS chain exactly as
// the rows of sort_rows_lists do.
// ---------------------------------------------------------------------------
std::atomic<int> g_sort_ragged_short_max{-1};  // srs_debug_set_sort_ragged_short_max

// Host wait for an event with sync_poll's manners.
int event_poll(hipEvent_t ev) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return SRS_OK;
    if (q != hipErrorNotReady) HIP_TRY(q);
    const auto dt = std::chrono::steady_clock::now() - t0;
    if (dt > std::chrono::milliseconds(20)) break;
    if (dt < std::chrono::microseconds(200)) cpu_relax();
    else std::this_thread::yield();
  }
  HIP_TRY(hipEventSynchronize(ev));
  return SRS_OK;
}

// What ragged_segs_kernel and run_lists_tail may index of the lists: valid
// offsets list at most num / (short_max + 1) segments, the kernel lists no
// more than that of any others.
int64_t ragged_list_cap(int64_t num, int64_t nseg, int short_max) {
  return std::min(nseg, num / ((int64_t)short_max + 1));
}

// R: the dense columns (R.num = num records each). Under the caller's
// workspace lock and WsUse; `what` names the call in the bad-offsets error,
// *seen (or null) receives the classify pass's counters.
int sort_ragged_locked(Workspace* W, const Request& R, int64_t nseg, const int64_t* offsets,
                       int64_t* idx_out, int short_max, const char* what, ListCounters* seen,
                       hipStream_t st) {
  const int64_t num = R.num;
  const int64_t cap = ragged_list_cap(num, nseg, short_max);
  W->last_small = false;
  int64_t* info = W->sort_ragged_info;
  for (int i = 0; i < 6; i++) info[i] = 0;
  const int ks = key_size_of(R.kind);
  const bool with_idx = idx_out != nullptr;
  const SortDesc kd = init_desc(R.kind, R.up);

  RaggedArgs a;
  init_rows_args(a, R, idx_out);
  a.num = num;
  a.nseg = nseg;
  a.offsets = offsets;
  a.key_bits = kd.key_bits;
  a.mpos = kd.mpos;
  a.mneg = kd.mneg;
  a.short_max = short_max;

  // ---- classify, and the one read-back of the counters ----------------------
  SRS_TRY(ensure_lists(W, (size_t)cap, (size_t)cap, (size_t)cap));
  ListCounters* d_ctr = (ListCounters*)W->ctr.p;
  if (!W->ev_ragged) HIP_TRY(hipEventCreateWithFlags(&W->ev_ragged, hipEventDisableTiming));
  HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(ListCounters), st));
  {
    TimedScope ts("ragged_segs", (double)nseg, st);
    HIP_TRY(launch_ragged_segs(offsets, nseg, num, short_max, kd.key_bits,
                               with_idx ? BUF_OUT : BUF_IN, cap, (Seg*)W->big[0].p,
                               (Seg*)W->local.p, (Seg*)W->local2.p, (Seg*)W->copy.p, d_ctr, st));
  }
  HIP_TRY(hipMemcpyAsync(W->h_ctr, d_ctr, sizeof(ListCounters), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(W->ev_ragged, st));
  if (short_max > 0) {
    // (queued behind the copy, so the host's wait below does not include it)
    TimedScope ts("ragged_short", (double)num, st);
    HIP_TRY(launch_ragged_short(ks, a, st));
  }
  SRS_TRY(event_poll(W->ev_ragged));
  const ListCounters c = *W->h_ctr;
  info[4] = 1;
  info[1] = (int64_t)c.n_local;
  info[2] = (int64_t)c.n_local2;
  info[3] = (int64_t)c.n_big;
  info[0] = nseg - (int64_t)c.n_listed - (int64_t)c.n_empty - (int64_t)c.n_bad;
  if (seen) *seen = c;
  if (c.n_bad > 0)
    return fail(SRS_ERR_INVALID_ARG,
                std::string(what) + ": " + std::to_string(c.n_bad) +
                    " segment(s) with offsets that decrease or leave [0, num] (skipped; the "
                    "outputs are unspecified)");
  if (c.n_listed == 0) return SRS_OK;

  // ---- the listed segments: the sort's levels and LDS chain -----------------
  // Without indices they sort IN -> OUT; with indices the prepare pass moves
  // them to the outputs with their iota, and they sort in place there.
  Request Q = R;
  if (with_idx) sort_outputs_in_place(Q, idx_out);
  SortDesc d;
  SortDesc* d_desc = nullptr;
  SRS_TRY(list_begin(W, Q, with_idx, c.n_big > 0, st, &d, &d_desc));
  if (with_idx) {
    TimedScope ts("ragged_prepare", (double)num, st);
    HIP_TRY(launch_ragged_prepare(a, st));
    info[5] = 1;
  }
  const LevelState S = level_state(d, ks, false, (int64_t)c.n_big, (int64_t)c.n_local,
                                   (int64_t)c.n_local2, (int64_t)c.n_copy);
  return list_finish(W, Q, d, d_desc, S, 0, false, &info[4], st);
}

int sort_ragged_device(const Request& R, int64_t nseg, const int64_t* offsets, int64_t* idx_out,
                       hipStream_t st) {
  int short_max = g_sort_ragged_short_max.load();
  if (short_max < 0) short_max = kRowsWaveMax;
  if ((nseg + 255) / 256 > 0x7fffffff)
    return fail(SRS_ERR_UNSUPPORTED, "sort ragged: more than 2^39 segments");
  WsScope ws;
  SRS_TRY(ws.begin(st));
  return sort_ragged_locked(ws.W, R, nseg, offsets, idx_out, short_max, "sort ragged", nullptr, st);
}

// ---------------------------------------------------------------------------
// ragged top-k: the first min(k, len) records of every
// segment of device offsets, at a stride of k slots per segment. Route 0 is
// three kernels with everything decided on the device (classify, a wave per
// short segment, a workgroup per listed long one) and one read-back of the
// counters behind all of them; route 1 sorts the segments into workspace
// columns (sort_ragged_locked) and copies the heads.
// ---------------------------------------------------------------------------
enum { TOPK_RAGGED_KERNELS = 0, TOPK_RAGGED_SORT = 1 };
std::atomic<int> g_topk_ragged_route{-1};  // srs_debug_set_topk_ragged_route

std::string topk_ragged_bad(unsigned long long n_bad) {
  return "top-k ragged: " + std::to_string(n_bad) +
         " segment(s) with offsets that decrease or leave [0, num] (skipped; the outputs are "
         "unspecified)";
}

// R: the dense input columns (R.num = num records each); R.out_cols the
// caller's outputs of nseg * k records.
int topk_ragged_device(const Request& R, int64_t nseg, const int64_t* offsets, int64_t k,
                       int64_t* idx_out, int64_t* counts_out, hipStream_t st) {
  const int64_t num = R.num;
  const bool can_kernels = k <= kTopkRowsMaxK && num < (int64_t(1) << 31);
  int route = g_topk_ragged_route.load();
  if (route < 0) route = can_kernels ? TOPK_RAGGED_KERNELS : TOPK_RAGGED_SORT;
  else if (route == TOPK_RAGGED_KERNELS && !can_kernels)
    return fail(SRS_ERR_UNSUPPORTED,
                "top-k ragged: the kernel route takes k <= kTopkRowsMaxK and num < 2^31");
  if ((nseg + 255) / 256 > 0x7fffffff)
    return fail(SRS_ERR_UNSUPPORTED, "top-k ragged: more than 2^39 segments");
  WsScope ws;
  SRS_TRY(ws.begin(st));
  Workspace* W = ws.W;
  int64_t* info = W->topk_ragged_info;
  for (int i = 0; i < 6; i++) info[i] = 0;
  info[0] = route;
  const int ks = key_size_of(R.kind);
  const SortDesc kd = init_desc(R.kind, R.up);

  TopkRaggedArgs a;
  init_rows_args(a, R, idx_out);
  a.num = num;
  a.nseg = nseg;
  a.k = k;
  a.offsets = offsets;
  a.key_bits = kd.key_bits;
  a.mpos = kd.mpos;
  a.mneg = kd.mneg;
  a.counts_out = counts_out;
  SRS_TRY(ensure(W->tkrctr, sizeof(TopkRaggedCounters)));
  a.ctr = (TopkRaggedCounters*)W->tkrctr.p;
  HIP_TRY(hipMemsetAsync(a.ctr, 0, sizeof(TopkRaggedCounters), st));

  if (route == TOPK_RAGGED_SORT) {
    // ---- the ragged sort into workspace columns, then the heads ---------------
    info[5] = -1;
    {
      TimedScope ts("topk_ragged_classify", (double)nseg, st);
      HIP_TRY(launch_topk_ragged_classify(a, st));  // (counts_out only: nothing is listed)
    }
    const int nsc = R.ncols + (idx_out ? 1 : 0);
    size_t off[SRS_MAX_COLS + 1], bytes = 0;
    for (int c = 0; c < nsc; c++) {
      off[c] = bytes;
      bytes += align_up((size_t)num * (c < R.ncols ? R.widths[c] : 8), 256);
    }
    SRS_TRY(ensure(W->tkrcols, bytes, ws_alloc_mode()));
    char* cols = (char*)W->tkrcols.p;
    Request Q = R;
    Q.thresh = 0;
    for (int c = 0; c < R.ncols; c++) Q.out_cols[c] = cols + off[c];
    int64_t* idx_ws = idx_out ? (int64_t*)(cols + off[R.ncols]) : nullptr;
    ListCounters seen{};
    const int rc = sort_ragged_locked(W, Q, nseg, offsets, idx_ws, kRowsWaveMax, "top-k ragged",
                                      &seen, st);
    info[1] = W->sort_ragged_info[0];
    info[2] = (int64_t)std::min<unsigned long long>(seen.n_listed, (unsigned long long)nseg);
    info[4] = W->sort_ragged_info[4];
    SRS_TRY(rc);
    for (int c = 0; c < R.ncols; c++) a.col[c].in = cols + off[c];
    a.idx_in = idx_ws;
    TimedScope ts("topk_ragged_heads", (double)num, st);
    HIP_TRY(launch_topk_ragged_heads(a, st));
    return SRS_OK;
  }

  // ---- classify, the wave kernel, the list's workgroups, one read-back -------
  const int64_t list_cap = ragged_list_cap(num, nseg, kRowsWaveMax);
  SRS_TRY(ensure(W->tkrlist, (size_t)std::max<int64_t>(list_cap, 1) * sizeof(int64_t)));
  a.list = (int64_t*)W->tkrlist.p;
  a.list_cap = (unsigned long long)list_cap;
  if (!W->h_tkr)
    HIP_TRY(hipHostMalloc((void**)&W->h_tkr, sizeof(TopkRaggedCounters), hipHostMallocDefault));
  if (!W->ev_ragged) HIP_TRY(hipEventCreateWithFlags(&W->ev_ragged, hipEventDisableTiming));
  {
    TimedScope ts("topk_ragged_classify", (double)nseg, st);
    HIP_TRY(launch_topk_ragged_classify(a, st));
  }
  {
    TimedScope ts("topk_ragged_short", (double)num, st);
    HIP_TRY(launch_topk_ragged_short(ks, a, st));
  }
  info[5] = 2;
  if (list_cap > 0) {
    TimedScope ts("topk_ragged_long", (double)num, st);
    HIP_TRY(launch_topk_ragged_long(ks, a, st));
    info[5] = 3;
  }
  HIP_TRY(hipMemcpyAsync(W->h_tkr, a.ctr, sizeof(TopkRaggedCounters), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(W->ev_ragged, st));
  SRS_TRY(event_poll(W->ev_ragged));
  const TopkRaggedCounters c = *W->h_tkr;
  info[1] = (int64_t)c.n_short;
  info[2] = (int64_t)c.n_long;
  info[3] = (int64_t)c.max_passes;
  info[4] = 1;
  if (c.n_bad > 0) return fail(SRS_ERR_INVALID_ARG, topk_ragged_bad(c.n_bad));
  return SRS_OK;
}

// ---------------------------------------------------------------------------
// unique: the stable sort S of the input (into the caller's
// sorted columns or workspace columns, with an index column when the argsort
// or the inverse is asked for), then the run boundaries of S's key column in
// three launches (run_tally_kernel, launch_excl_scan, run_write_kernel) with
// nothing read back unless the caller wants U on the host.
// ---------------------------------------------------------------------------
// One output array of a unique call, for the overlap tests.
struct UniqueOut {
  const void* p;
  size_t bytes;
};

// R: the input columns, R.out_cols the caller's sorted columns (sorted: they
// were given). Everything is checked before the first device access.
int unique_validate(const Request& R, bool sorted, const int64_t* idx_out, const void* unique_out,
                    const int64_t* offsets_out, const int64_t* inverse_out,
                    const int64_t* nu_dev) {
  const int64_t num = R.num;
  if (num > (INT64_MAX >> 4)) return fail(SRS_ERR_INVALID_ARG, "num + 1 overflows");
  if (!R.in_cols[0]) return fail(SRS_ERR_INVALID_ARG, "keys is NULL");
  if (!unique_out) return fail(SRS_ERR_INVALID_ARG, "unique_out is NULL");
  for (int c = 0; c < R.ncols; c++) {
    if (!R.in_cols[c] || (sorted && !R.out_cols[c]))
      return fail(SRS_ERR_INVALID_ARG, "payload pointer is NULL");
    SRS_TRY(check_col_alignment(R, c, true));
  }
  if ((uintptr_t)unique_out % R.widths[0] != 0)
    return fail(SRS_ERR_INVALID_ARG, "device arrays must be aligned to their element size");
  if ((uintptr_t)idx_out % 8 != 0) return fail(SRS_ERR_INVALID_ARG, "indices_out must be 8-byte aligned");
  if ((uintptr_t)offsets_out % 8 != 0)
    return fail(SRS_ERR_INVALID_ARG, "offsets_out must be 8-byte aligned");
  if ((uintptr_t)inverse_out % 8 != 0)
    return fail(SRS_ERR_INVALID_ARG, "inverse_out must be 8-byte aligned");
  if ((uintptr_t)nu_dev % 8 != 0)
    return fail(SRS_ERR_INVALID_ARG, "num_unique_dev must be 8-byte aligned");
  UniqueOut outs[SRS_MAX_COLS + 5];
  int no = 0;
  for (int c = 0; sorted && c < R.ncols; c++) outs[no++] = {R.out_cols[c], (size_t)num * R.widths[c]};
  outs[no++] = {unique_out, (size_t)num * R.widths[0]};
  if (idx_out) outs[no++] = {idx_out, (size_t)num * 8};
  if (offsets_out) outs[no++] = {offsets_out, ((size_t)num + 1) * 8};
  if (inverse_out) outs[no++] = {inverse_out, (size_t)num * 8};
  if (nu_dev) outs[no++] = {nu_dev, 8};
  auto over = [](const void* p, size_t pn, const void* q, size_t qn) {
    const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
    return x < y + qn && y < x + pn;
  };
  for (int o = 0; o < no; o++)
    for (int c = 0; c < R.ncols; c++)
      if (over(outs[o].p, outs[o].bytes, R.in_cols[c], (size_t)num * R.widths[c]))
        return fail(SRS_ERR_INVALID_ARG, "unique outputs must not overlap the inputs");
  for (int o = 0; o < no; o++)
    for (int q = o + 1; q < no; q++)
      if (over(outs[o].p, outs[o].bytes, outs[q].p, outs[q].bytes))
        return fail(SRS_ERR_INVALID_ARG, "unique outputs must not overlap each other");
  return SRS_OK;
}

int unique_device(const Request& R, bool sorted, int64_t* idx_out, void* unique_out,
                  int64_t* offsets_out, int64_t* inverse_out, int64_t* nu_dev, int64_t* nu_host,
                  hipStream_t st) {
  const int64_t n = R.num;
  const int ks = key_size_of(R.kind);
  const bool with_idx = idx_out != nullptr || inverse_out != nullptr;
  WsScope ws;
  SRS_TRY(ws.begin(st));
  Workspace* W = ws.W;
  int64_t* info = W->unique_info;
  info[0] = info[1] = 0;
  info[2] = with_idx ? 1 : 0;
  info[3] = sorted ? 0 : 1;

  // ---- S: the caller's sorted columns, or workspace columns ------------------
  const size_t key_bytes = sorted ? 0 : align_up((size_t)n * ks, 256);  // (no payloads then)
  const size_t idx_bytes = with_idx && !idx_out ? (size_t)n * 8 : 0;
  if (key_bytes + idx_bytes > 0) SRS_TRY(ensure(W->uniqcols, key_bytes + idx_bytes, ws_alloc_mode()));
  char* dst[SRS_MAX_COLS];
  for (int c = 0; c < R.ncols; c++) dst[c] = sorted ? (char*)R.out_cols[c] : (char*)W->uniqcols.p;
  int64_t* idx_col = !with_idx ? nullptr
                     : idx_out ? idx_out
                               : (int64_t*)((char*)W->uniqcols.p + key_bytes);
  const SortDesc kd = init_desc(R.kind, R.up);
  SelectArgs a;
  memset(&a, 0, sizeof a);
  a.stride = (uint32_t)ks;
  a.n = n;
  a.all = 1;
  a.key_bits = kd.key_bits;
  a.mpos = kd.mpos;
  a.mneg = kd.mneg;
  if (!with_idx) {
    Request F = R;
    F.thresh = 0;  // (the total order for floats at every size)
    for (int c = 0; c < R.ncols; c++) F.out_cols[c] = dst[c];
    SRS_TRY(sort_locked(W, F, st));
  } else {
    // the ordered copy adds the index column (as top-k's full route), the
    // columns are then sorted where they are
    SRS_TRY(ensure(W->seldesc, sizeof(SortDesc)));
    SortDesc d = init_desc(R.kind, R.up);
    for (int c = 0; c < R.ncols; c++) {
      const uint32_t w = R.widths[c];
      d.cols[c] = Col{{(char*)R.in_cols[c], dst[c], nullptr, nullptr}, w, {w, w, w, w}};
    }
    set_gather_desc(W, d, R.ncols, st);
    a.keys = (const char*)R.in_cols[0];
    {
      TimedScope ts("select_gather", (double)n, st);
      launch_select_gather(ks, a, (const SortDesc*)W->seldesc.p, nullptr, n, idx_col, st);
    }
    HIP_TRY(hipGetLastError());
    Request S = R;
    S.thresh = 0;
    for (int c = 0; c < R.ncols; c++) S.in_cols[c] = S.out_cols[c] = dst[c];
    S.in_cols[R.ncols] = S.out_cols[R.ncols] = idx_col;
    S.widths[R.ncols] = 8;
    S.ncols = R.ncols + 1;
    SRS_TRY(sort_locked(W, S, st));
  }

  // ---- the run boundaries of S's key column ----------------------------------
  const int64_t ntiles = (n + kTile - 1) / kTile;
  SRS_TRY(ensure(W->uniqcnt, (size_t)(2 * ntiles + scan_temp_elems(ntiles) + 1) * sizeof(uint64_t)));
  uint64_t* counts = (uint64_t*)W->uniqcnt.p;
  uint64_t* bases = counts + ntiles;
  uint64_t* temp = bases + ntiles;
  uint64_t* total = temp + scan_temp_elems(ntiles);
  a.keys = dst[0];
  {
    TimedScope ts("run_tally", (double)n, st);
    launch_run_tally(ks, a, counts, st);
  }
  launch_excl_scan(counts, bases, ntiles, temp, total, st);
  {
    TimedScope ts("run_write", (double)n, st);
    launch_run_write(ks, a, bases, total, unique_out, offsets_out, idx_col, inverse_out, nu_dev, st);
  }
  HIP_TRY(hipGetLastError());
  info[0] = 3;
  if (nu_host) {
    if (!W->h_uniq) HIP_TRY(hipHostMalloc((void**)&W->h_uniq, sizeof(int64_t), hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(W->h_uniq, total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SRS_TRY(sync_poll(st));
    info[1] = 1;
    *nu_host = *W->h_uniq;
  }
  return SRS_OK;
}

// ---------------------------------------------------------------------------
// search-sorted: one kernel over the caller's queries (route
// 0), or over a sorted copy of them that carries their positions, the results
// written back through that index column (route 1)
// ---------------------------------------------------------------------------
static_assert(kSearchTile == SRS_SEARCH_QUERY_TILE && kSearchSamples == SRS_SEARCH_LDS_SAMPLES &&
                  kSearchFit == SRS_SEARCH_LDS_RANGE,
              "srs_c_api.h states the search kernel's shape");
enum { SEARCH_DIRECT = 0, SEARCH_SORT = 1 };
std::atomic<int> g_search_route{-1};  // srs_debug_set_search_route

// The route of a flat call without the hint, from the measured grid (DESIGN.md
// §17; tools/search_bench.py): against a table of 2^20 keys the direct kernel
// wins at every query count (1.1-6x), against 2^22 keys and more sorting the
// queries first wins from 2^22 queries on (1.05-4.5x at 2^22 .. 2^30 queries,
// more the larger the table), with 8-byte keys already at 2^20 queries (1.25x;
// 4-byte keys lose 1.6x there: their sort of 2^20 records has a floor of 0.25
// ms). Below either bound the direct kernel wins by 1.2-8x.
constexpr int64_t kSearchSortMinTable = int64_t(1) << 22;
constexpr int64_t kSearchSortMinQueries = int64_t(1) << 22;
constexpr int64_t kSearchSortMinQueries8 = int64_t(1) << 20;  // 8-byte keys
bool search_prefers_sort(int64_t num, int64_t nq, int ks) {
  return num >= kSearchSortMinTable &&
         nq >= (ks == 8 ? kSearchSortMinQueries8 : kSearchSortMinQueries);
}

struct SearchCall {
  int64_t num, nseg, nq;
  int kind, up;
  const void* keys;
  const int64_t* offsets;
  const void* queries;
  const int64_t* qseg;
  int64_t* lower;
  int64_t* upper;
  int64_t* num_bad;
  int32_t flags;
};

// Everything is checked before the first device access (nq > 0).
int search_validate(const SearchCall& C) {
  const size_t ks = (size_t)key_size_of(C.kind);
  if (C.num > (INT64_MAX >> 4)) return fail(SRS_ERR_INVALID_ARG, "num overflows");
  if (C.nq > (INT64_MAX >> 4)) return fail(SRS_ERR_INVALID_ARG, "num_queries * 8 overflows");
  const bool seg = C.offsets != nullptr;
  if (seg != (C.qseg != nullptr))
    return fail(SRS_ERR_INVALID_ARG, "offsets and query_segments must both be set or both NULL");
  if (seg && C.nseg < 1) return fail(SRS_ERR_INVALID_ARG, "num_segments must be at least 1");
  if (seg && C.nseg > (INT64_MAX >> 4))
    return fail(SRS_ERR_INVALID_ARG, "num_segments + 1 overflows");
  if (C.num > 0 && !C.keys) return fail(SRS_ERR_INVALID_ARG, "sorted_keys is NULL");
  if (!C.queries) return fail(SRS_ERR_INVALID_ARG, "queries is NULL");
  if (!C.lower && !C.upper)
    return fail(SRS_ERR_INVALID_ARG, "lower_out and upper_out are both NULL");
  if ((uintptr_t)C.keys % ks != 0 || (uintptr_t)C.queries % ks != 0)
    return fail(SRS_ERR_INVALID_ARG, "device arrays must be aligned to their element size");
  if ((uintptr_t)C.offsets % 8 != 0) return fail(SRS_ERR_INVALID_ARG, "offsets must be 8-byte aligned");
  if ((uintptr_t)C.qseg % 8 != 0)
    return fail(SRS_ERR_INVALID_ARG, "query_segments must be 8-byte aligned");
  if ((uintptr_t)C.lower % 8 != 0) return fail(SRS_ERR_INVALID_ARG, "lower_out must be 8-byte aligned");
  if ((uintptr_t)C.upper % 8 != 0) return fail(SRS_ERR_INVALID_ARG, "upper_out must be 8-byte aligned");
  if ((uintptr_t)C.num_bad % 8 != 0)
    return fail(SRS_ERR_INVALID_ARG, "num_bad_dev must be 8-byte aligned");
  const int64_t num = std::max<int64_t>(C.num, 0);
  const UniqueOut ins[4] = {{C.keys, (size_t)num * ks},
                            {C.queries, (size_t)C.nq * ks},
                            {C.offsets, seg ? ((size_t)C.nseg + 1) * 8 : 0},
                            {C.qseg, seg ? (size_t)C.nq * 8 : 0}};
  const UniqueOut outs[3] = {{C.lower, C.lower ? (size_t)C.nq * 8 : 0},
                             {C.upper, C.upper ? (size_t)C.nq * 8 : 0},
                             {C.num_bad, C.num_bad ? (size_t)8 : 0}};
  auto over = [](const UniqueOut& p, const UniqueOut& q) {
    const uintptr_t x = (uintptr_t)p.p, y = (uintptr_t)q.p;
    return p.bytes && q.bytes && x < y + q.bytes && y < x + p.bytes;
  };
  for (const UniqueOut& o : outs)
    for (const UniqueOut& i : ins)
      if (over(o, i)) return fail(SRS_ERR_INVALID_ARG, "search outputs must not overlap the inputs");
  for (int o = 0; o < 3; o++)
    for (int q = o + 1; q < 3; q++)
      if (over(outs[o], outs[q]))
        return fail(SRS_ERR_INVALID_ARG, "search outputs must not overlap each other");
  return SRS_OK;
}

int search_device(const SearchCall& C, hipStream_t st) {
  const int ks = key_size_of(C.kind);
  const bool seg = C.offsets != nullptr;
  const int forced = g_search_route.load();
  const int route = seg                                      ? SEARCH_DIRECT
                    : forced >= 0                            ? forced
                    : (C.flags & SRS_SEARCH_QUERIES_SORTED)  ? SEARCH_DIRECT
                    : search_prefers_sort(C.num, C.nq, ks)   ? SEARCH_SORT
                                                             : SEARCH_DIRECT;
  // (the direct route touches no workspace buffer: the lock for the report
  // below, but no place in the workspace's stream order)
  WsScope ws;
  SRS_TRY(route == SEARCH_SORT ? ws.begin(st) : ws.lock());
  Workspace* W = ws.W;
  int64_t* info = W->search_info;
  info[0] = route;
  info[1] = 0;
  info[2] = route == SEARCH_SORT ? -1 : 0;
  info[3] = route == SEARCH_SORT ? 1 : 0;

  const SortDesc kd = init_desc(C.kind, C.up);
  SearchArgs a;
  memset(&a, 0, sizeof a);
  a.keys = (const char*)C.keys;
  a.num = std::max<int64_t>(C.num, 0);
  a.queries = (const char*)C.queries;
  a.nq = C.nq;
  a.lower = C.lower;
  a.upper = C.upper;
  a.offsets = C.offsets;
  a.qseg = C.qseg;
  a.nseg = C.nseg;
  a.num_bad = seg ? C.num_bad : nullptr;
  a.key_bits = kd.key_bits;
  a.mpos = kd.mpos;
  a.mneg = kd.mneg;

  if (route == SEARCH_SORT) {
    // the ordered copy adds the index column (as unique's), the two columns
    // are then sorted where they are
    const size_t key_bytes = align_up((size_t)C.nq * ks, 256);
    SRS_TRY(ensure(W->searchcols, key_bytes + (size_t)C.nq * 8, ws_alloc_mode()));
    char* qcopy = (char*)W->searchcols.p;
    int64_t* idx_col = (int64_t*)(qcopy + key_bytes);
    SRS_TRY(ensure(W->seldesc, sizeof(SortDesc)));
    SortDesc d = init_desc(C.kind, C.up);
    const uint32_t w = (uint32_t)ks;
    d.cols[0] = Col{{(char*)C.queries, qcopy, nullptr, nullptr}, w, {w, w, w, w}};
    set_gather_desc(W, d, 1, st);
    SelectArgs g;
    memset(&g, 0, sizeof g);
    g.keys = (const char*)C.queries;
    g.stride = w;
    g.n = C.nq;
    g.all = 1;
    g.key_bits = kd.key_bits;
    g.mpos = kd.mpos;
    g.mneg = kd.mneg;
    {
      TimedScope ts("select_gather", (double)C.nq, st);
      launch_select_gather(ks, g, (const SortDesc*)W->seldesc.p, nullptr, C.nq, idx_col, st);
    }
    HIP_TRY(hipGetLastError());
    Request S;
    SRS_TRY(build_soa(S, C.nq, C.kind, C.up, 0, qcopy, 0, nullptr, nullptr, nullptr, nullptr));
    S.in_cols[1] = S.out_cols[1] = idx_col;
    S.widths[1] = 8;
    S.ncols = 2;
    SRS_TRY(sort_locked(W, S, st));
    a.queries = qcopy;
    a.idx = idx_col;
  }
  if (C.num_bad) {
    HIP_TRY(hipMemsetAsync(C.num_bad, 0, sizeof(int64_t), st));
    info[1]++;
  }
  {
    TimedScope ts("search", (double)C.nq, st);
    HIP_TRY(launch_search(ks, a, st));
  }
  info[1]++;
  return SRS_OK;
}

// ---------------------------------------------------------------------------
// merge: the split of A at every tile boundary, then one
// workgroup per tile of the output; the columns' three views travel in the
// gather's descriptor (A: BUF_IN, B: BUF_TMP, the output: BUF_OUT)
// ---------------------------------------------------------------------------
static_assert(kMergeTile == SRS_MERGE_TILE, "srs_c_api.h states the merge kernel's tile");

struct MergeCall {
  int64_t num_a, num_b;
  int kind, up;
  int ncols;  // the key column and the payload columns
  const void* a[SRS_MAX_COLS];
  const void* b[SRS_MAX_COLS];
  void* out[SRS_MAX_COLS];
  uint32_t widths[SRS_MAX_COLS];
  int64_t* source;
};

// The raw arguments of srs_merge_soa_device, checked, into C: everything is
// checked here, before the first device access. Messages name the argument
// (and the payload column) at fault.
int merge_validate(MergeCall& C, int64_t num_a, int64_t num_b, int key_kind, int up,
                   const void* keys_a, const void* keys_b, int32_t num_payloads,
                   const void* const* payloads_a, const void* const* payloads_b,
                   const uint32_t* payload_sizes, void* keys_out, void* const* payloads_out,
                   int64_t* source_out) {
  memset(&C, 0, sizeof C);
  if (key_size_of(key_kind) == 0) return fail(SRS_ERR_INVALID_ARG, "invalid key_kind");
  if (num_payloads < 0 || num_payloads > SRS_MAX_PAYLOADS)
    return fail(SRS_ERR_INVALID_ARG, "num_payloads out of range");
  if (num_payloads > 0 && !payload_sizes)
    return fail(SRS_ERR_INVALID_ARG, "payload_sizes is NULL");
  C.widths[0] = (uint32_t)key_size_of(key_kind);
  for (int i = 0; i < num_payloads; i++) {
    const uint32_t w = payload_sizes[i];
    if (w != 1 && w != 2 && w != 4 && w != 8)
      return fail(SRS_ERR_UNSUPPORTED, "payload_sizes[" + std::to_string(i) +
                                           "]: payload sizes must be 1, 2, 4 or 8 bytes");
    C.widths[1 + i] = w;
  }
  if (num_a < 0) return fail(SRS_ERR_INVALID_ARG, "num_a is negative");
  if (num_b < 0) return fail(SRS_ERR_INVALID_ARG, "num_b is negative");
  int64_t n = 0;
  if (__builtin_add_overflow(num_a, num_b, &n) || n > (INT64_MAX >> 4))
    return fail(SRS_ERR_INVALID_ARG, "(num_a + num_b) * 16 overflows");
  C.num_a = num_a;
  C.num_b = num_b;
  C.kind = key_kind;
  C.up = up ? 1 : 0;
  C.ncols = 1 + num_payloads;
  C.source = source_out;
  if (n == 0) return SRS_OK;  // (a no-op looks at none of the arrays)
  if (num_payloads > 0 && num_a > 0 && !payloads_a)
    return fail(SRS_ERR_INVALID_ARG, "payloads_a is NULL");
  if (num_payloads > 0 && num_b > 0 && !payloads_b)
    return fail(SRS_ERR_INVALID_ARG, "payloads_b is NULL");
  if (num_payloads > 0 && !payloads_out) return fail(SRS_ERR_INVALID_ARG, "payloads_out is NULL");
  C.a[0] = num_a > 0 ? keys_a : nullptr;
  C.b[0] = num_b > 0 ? keys_b : nullptr;
  C.out[0] = keys_out;
  for (int i = 0; i < num_payloads; i++) {
    C.a[1 + i] = num_a > 0 ? payloads_a[i] : nullptr;
    C.b[1 + i] = num_b > 0 ? payloads_b[i] : nullptr;
    C.out[1 + i] = payloads_out[i];
  }
  // column c's name on one side: keys_a, payloads_b[3], ...
  auto name = [](int c, const char* side) {
    return c == 0 ? std::string("keys_") + side
                  : std::string("payloads_") + side + "[" + std::to_string(c - 1) + "]";
  };
  for (int c = 0; c < C.ncols; c++) {
    if (num_a > 0 && !C.a[c]) return fail(SRS_ERR_INVALID_ARG, name(c, "a") + " is NULL");
    if (num_b > 0 && !C.b[c]) return fail(SRS_ERR_INVALID_ARG, name(c, "b") + " is NULL");
    if (!C.out[c]) return fail(SRS_ERR_INVALID_ARG, name(c, "out") + " is NULL");
  }
  for (int c = 0; c < C.ncols; c++) {
    const uintptr_t w = C.widths[c];
    const char* bad = (uintptr_t)C.a[c] % w != 0     ? "a"
                      : (uintptr_t)C.b[c] % w != 0   ? "b"
                      : (uintptr_t)C.out[c] % w != 0 ? "out"
                                                     : nullptr;
    if (bad)
      return fail(SRS_ERR_INVALID_ARG,
                  name(c, bad) + " must be aligned to its element size (" + std::to_string(w) +
                      " bytes)");
  }
  if ((uintptr_t)C.source % 8 != 0) return fail(SRS_ERR_INVALID_ARG, "source_out must be 8-byte aligned");
  UniqueOut ins[2 * SRS_MAX_COLS], outs[SRS_MAX_COLS + 1];
  int ni = 0, no = 0;
  for (int c = 0; c < C.ncols; c++) {
    ins[ni++] = {C.a[c], (size_t)C.num_a * C.widths[c]};
    ins[ni++] = {C.b[c], (size_t)C.num_b * C.widths[c]};
    outs[no++] = {C.out[c], (size_t)n * C.widths[c]};
  }
  if (C.source) outs[no++] = {C.source, (size_t)n * 8};
  auto over = [](const UniqueOut& p, const UniqueOut& q) {
    const uintptr_t x = (uintptr_t)p.p, y = (uintptr_t)q.p;
    return p.bytes && q.bytes && x < y + q.bytes && y < x + p.bytes;
  };
  for (int o = 0; o < no; o++)
    for (int i = 0; i < ni; i++)
      if (over(outs[o], ins[i]))
        return fail(SRS_ERR_INVALID_ARG, "merge outputs must not overlap the inputs");
  for (int o = 0; o < no; o++)
    for (int q = o + 1; q < no; q++)
      if (over(outs[o], outs[q]))
        return fail(SRS_ERR_INVALID_ARG, "merge outputs must not overlap each other");
  return SRS_OK;
}

int merge_device(const MergeCall& C, hipStream_t st) {
  const int ks = key_size_of(C.kind);
  const int64_t n = C.num_a + C.num_b;
  const int64_t ntiles = (n + kMergeTile - 1) / kMergeTile;
  if (ntiles > 0x7fffffff) return fail(SRS_ERR_UNSUPPORTED, "num_a + num_b: more than 2^31 - 1 tiles");
  WsScope ws;
  SRS_TRY(ws.begin(st));  // (the split buffer and the descriptor are the workspace's)
  Workspace* W = ws.W;
  int64_t* info = W->merge_info;
  info[0] = info[1] = 0;
  info[2] = ntiles;
  SRS_TRY(ensure(W->mergesplit, (size_t)(ntiles + 1) * sizeof(int64_t)));
  SRS_TRY(ensure(W->seldesc, sizeof(SortDesc)));
  info[3] = (int64_t)(W->mergesplit.bytes + W->seldesc.bytes);

  SortDesc d = init_desc(C.kind, C.up);
  for (int c = 0; c < C.ncols; c++) {
    const uint32_t w = C.widths[c];
    d.cols[c] = Col{{(char*)C.a[c], (char*)C.out[c], (char*)C.b[c], nullptr}, w, {w, w, w, w}};
  }
  set_gather_desc(W, d, C.ncols, st);
  MergeArgs a;
  memset(&a, 0, sizeof a);
  a.num_a = C.num_a;
  a.num_b = C.num_b;
  a.desc = (const SortDesc*)W->seldesc.p;
  a.split = (int64_t*)W->mergesplit.p;
  a.source = C.source;
  a.key_bits = d.key_bits;
  a.mpos = d.mpos;
  a.mneg = d.mneg;
  {
    TimedScope ts("merge_split", (double)(ntiles + 1), st);
    HIP_TRY(launch_merge_split(ks, a, st));
  }
  {
    TimedScope ts("merge_tile", (double)n, st);
    HIP_TRY(launch_merge_tile(ks, a, st));
  }
  info[0] = 3;  // the descriptor, the split, the tiles
  return SRS_OK;
}

}  // namespace
}  // namespace srs

using namespace srs;

extern "C" {

int srs_topk_soa_device(int64_t num, int64_t k, int key_kind, int up, const void* keys,
                        int32_t num_payloads, const void* const* payloads,
                        const uint32_t* payload_sizes, void* keys_out, void* const* payloads_out,
                        int64_t* indices_out, void* stream) {
  Request R;
  SRS_TRY(build_soa(R, num, key_kind, up, 0, (void*)keys, num_payloads, (void* const*)payloads,
                    payload_sizes, keys_out, payloads_out));
  SRS_TRY(topk_validate(R, k, keys_out, indices_out));
  if (k <= 0 || num <= 0) return SRS_OK;
  return topk_device(R, k, indices_out, (hipStream_t)stream);
}

int srs_topk_aos_device(int64_t num, int64_t k, int key_kind, int up, const void* elements,
                        uint32_t elem_size, void* elements_out, int64_t* indices_out,
                        void* stream) {
  Request R;
  SRS_TRY(build_aos(R, num, key_kind, up, 0, (void*)elements, elem_size, elements_out));
  SRS_TRY(topk_validate(R, k, elements_out, indices_out));
  if (k <= 0 || num <= 0) return SRS_OK;
  return topk_device(R, k, indices_out, (hipStream_t)stream);
}

int srs_topk_rows_soa_device(int64_t rows, int64_t row_len, int64_t row_stride, int64_t k,
                             int key_kind, int up, const void* keys, int32_t num_payloads,
                             const void* const* payloads, const uint32_t* payload_sizes,
                             void* keys_out, void* const* payloads_out, int64_t* indices_out,
                             void* stream) {
  Request R;
  SRS_TRY(build_soa(R, row_len, key_kind, up, 0, (void*)keys, num_payloads,
                    (void* const*)payloads, payload_sizes, keys_out, payloads_out));
  SRS_TRY(rows_validate("top-k", R, rows, row_stride, std::min(k, row_len), keys_out, indices_out));
  if (rows <= 0 || row_len <= 0 || k <= 0) return SRS_OK;
  return topk_rows_device(R, rows, row_stride, k, indices_out, (hipStream_t)stream);
}

int srs_sort_rows_soa_device(int64_t rows, int64_t row_len, int64_t row_stride, int key_kind,
                             int up, const void* keys, int32_t num_payloads,
                             const void* const* payloads, const uint32_t* payload_sizes,
                             void* keys_out, void* const* payloads_out, int64_t* indices_out,
                             void* stream) {
  Request R;
  SRS_TRY(build_soa(R, row_len, key_kind, up, 0, (void*)keys, num_payloads,
                    (void* const*)payloads, payload_sizes, keys_out, payloads_out));
  SRS_TRY(rows_validate("sort rows", R, rows, row_stride, row_len, keys_out, indices_out));
  if (rows <= 0 || row_len <= 0) return SRS_OK;
  return sort_rows_device(R, rows, row_stride, indices_out, (hipStream_t)stream);
}

int srs_sort_ragged_soa_device(int64_t num, int64_t num_segments, const int64_t* offsets,
                               int key_kind, int up, const void* keys, int32_t num_payloads,
                               const void* const* payloads, const uint32_t* payload_sizes,
                               void* keys_out, void* const* payloads_out, int64_t* indices_out,
                               void* stream) {
  Request R;
  SRS_TRY(build_soa(R, num, key_kind, up, 0, (void*)keys, num_payloads, (void* const*)payloads,
                    payload_sizes, keys_out, payloads_out));
  const bool work = num > 0 && num_segments > 0;
  const char* shape = num_segments > (INT64_MAX >> 4) ? "num_segments + 1 overflows" : nullptr;
  SRS_TRY(validate_outputs(R, {"sort ragged", keys_out, indices_out, work ? num : 0,
                               work ? num : 0, true, shape}));
  if (!work) return SRS_OK;
  if (!offsets) return fail(SRS_ERR_INVALID_ARG, "offsets is NULL");
  if ((uintptr_t)offsets % 8 != 0) return fail(SRS_ERR_INVALID_ARG, "offsets must be 8-byte aligned");
  if (outputs_overlap(R, indices_out, num, offsets, ((size_t)num_segments + 1) * sizeof(int64_t)))
    return fail(SRS_ERR_INVALID_ARG, "sort ragged outputs must not overlap the offsets");
  return sort_ragged_device(R, num_segments, offsets, indices_out, (hipStream_t)stream);
}

int srs_topk_ragged_soa_device(int64_t num, int64_t num_segments, const int64_t* offsets,
                               int64_t k, int key_kind, int up, const void* keys,
                               int32_t num_payloads, const void* const* payloads,
                               const uint32_t* payload_sizes, void* keys_out,
                               void* const* payloads_out, int64_t* indices_out,
                               int64_t* counts_out, void* stream) {
  Request R;
  SRS_TRY(build_soa(R, num, key_kind, up, 0, (void*)keys, num_payloads, (void* const*)payloads,
                    payload_sizes, keys_out, payloads_out));
  const bool work = num > 0 && num_segments > 0 && k > 0;
  int64_t slots = 0;
  const char* shape = !work ? nullptr
                      : num_segments > (INT64_MAX >> 4) ? "num_segments + 1 overflows"
                      : __builtin_mul_overflow(num_segments, k, &slots) || slots > (INT64_MAX >> 4)
                          ? "num_segments * k overflows"
                          : nullptr;
  SRS_TRY(validate_outputs(R, {"top-k ragged", keys_out, indices_out, work ? num : 0,
                               work ? (shape ? 1 : slots) : 0, true, shape}));
  if (!work) return SRS_OK;
  if (!offsets) return fail(SRS_ERR_INVALID_ARG, "offsets is NULL");
  if ((uintptr_t)offsets % 8 != 0) return fail(SRS_ERR_INVALID_ARG, "offsets must be 8-byte aligned");
  if ((uintptr_t)counts_out % 8 != 0)
    return fail(SRS_ERR_INVALID_ARG, "counts_out must be 8-byte aligned");
  const size_t offs_bytes = ((size_t)num_segments + 1) * sizeof(int64_t);
  if (outputs_overlap(R, indices_out, slots, offsets, offs_bytes))
    return fail(SRS_ERR_INVALID_ARG, "top-k ragged outputs must not overlap the offsets");
  if (counts_out) {
    // counts_out: one more output of num_segments int64 (outputs_overlap's test)
    const uintptr_t x = (uintptr_t)counts_out;
    const size_t xn = (size_t)num_segments * sizeof(int64_t);
    auto over = [&](const void* p, size_t bytes) {
      const uintptr_t y = (uintptr_t)p;
      return bytes && x < y + bytes && y < x + xn;
    };
    for (int c = 0; c < R.ncols; c++)
      if (over(R.in_cols[c], (size_t)num * R.widths[c]))
        return fail(SRS_ERR_INVALID_ARG, "top-k ragged counts_out must not overlap the inputs");
    if (over(offsets, offs_bytes))
      return fail(SRS_ERR_INVALID_ARG, "top-k ragged counts_out must not overlap the offsets");
  }
  return topk_ragged_device(R, num_segments, offsets, k, indices_out, counts_out,
                            (hipStream_t)stream);
}

int srs_unique_soa_device(int64_t num, int key_kind, int up, const void* keys,
                          int32_t num_payloads, const void* const* payloads,
                          const uint32_t* payload_sizes, void* keys_sorted_out,
                          void* const* payloads_sorted_out, int64_t* indices_out,
                          void* unique_out, int64_t* offsets_out, int64_t* inverse_out,
                          int64_t* num_unique_dev, int64_t* num_unique_host, void* stream) {
  Request R;
  SRS_TRY(build_soa(R, num, key_kind, up, 0, (void*)keys, num_payloads, (void* const*)payloads,
                    payload_sizes, keys_sorted_out, payloads_sorted_out));
  const bool sorted = keys_sorted_out != nullptr;
  if (!sorted && num_payloads > 0)
    return fail(SRS_ERR_INVALID_ARG,
                "payloads need keys_sorted_out and payloads_sorted_out: num_payloads must be 0 "
                "without them");
  if ((indices_out || inverse_out) && num_payloads > SRS_MAX_PAYLOADS - 1)
    return fail(SRS_ERR_UNSUPPORTED,
                "indices_out and inverse_out travel as one more payload column: at most 63 "
                "payload columns with them");
  if (num <= 0) {
    if (num_unique_host) *num_unique_host = 0;
    return SRS_OK;
  }
  SRS_TRY(unique_validate(R, sorted, indices_out, unique_out, offsets_out, inverse_out,
                          num_unique_dev));
  return unique_device(R, sorted, indices_out, unique_out, offsets_out, inverse_out,
                       num_unique_dev, num_unique_host, (hipStream_t)stream);
}

int srs_debug_last_unique(int64_t* info) {
  if (!info) return fail(SRS_ERR_INVALID_ARG, "info is NULL");
  Workspace* W = nullptr;
  WsLock lk;
  SRS_TRY(acquire_ws(&W, &lk));
  for (int i = 0; i < 4; i++) info[i] = W->unique_info[i];
  return SRS_OK;
}

int srs_search_sorted_device(int64_t num, int key_kind, int up, const void* sorted_keys,
                             int64_t num_segments, const int64_t* offsets, int64_t num_queries,
                             const void* queries, const int64_t* query_segments,
                             int64_t* lower_out, int64_t* upper_out, int64_t* num_bad_dev,
                             int32_t flags, void* stream) {
  if (key_size_of(key_kind) == 0) return fail(SRS_ERR_INVALID_ARG, "invalid key_kind");
  if (flags & ~SRS_SEARCH_QUERIES_SORTED) return fail(SRS_ERR_INVALID_ARG, "unknown flags bits");
  if (num_queries <= 0) return SRS_OK;
  const SearchCall C = {num, num_segments, num_queries, key_kind, up ? 1 : 0, sorted_keys, offsets,
                        queries, query_segments, lower_out, upper_out, num_bad_dev, flags};
  SRS_TRY(search_validate(C));
  return search_device(C, (hipStream_t)stream);
}

int srs_debug_set_search_route(int route) {
  if (route < -1 || route > SEARCH_SORT)
    return fail(SRS_ERR_INVALID_ARG, "route must be -1, 0 or 1");
  g_search_route.store(route);
  return SRS_OK;
}

int srs_debug_last_search(int64_t* info) {
  if (!info) return fail(SRS_ERR_INVALID_ARG, "info is NULL");
  Workspace* W = nullptr;
  WsLock lk;
  SRS_TRY(acquire_ws(&W, &lk));
  for (int i = 0; i < 4; i++) info[i] = W->search_info[i];
  return SRS_OK;
}

int srs_merge_soa_device(int64_t num_a, int64_t num_b, int key_kind, int up, const void* keys_a,
                         const void* keys_b, int32_t num_payloads,
                         const void* const* payloads_a, const void* const* payloads_b,
                         const uint32_t* payload_sizes, void* keys_out, void* const* payloads_out,
                         int64_t* source_out, void* stream) {
  MergeCall C;
  SRS_TRY(merge_validate(C, num_a, num_b, key_kind, up, keys_a, keys_b, num_payloads, payloads_a,
                         payloads_b, payload_sizes, keys_out, payloads_out, source_out));
  if (num_a + num_b <= 0) return SRS_OK;
  return merge_device(C, (hipStream_t)stream);
}

int srs_debug_last_merge(int64_t* info) {
  if (!info) return fail(SRS_ERR_INVALID_ARG, "info is NULL");
  Workspace* W = nullptr;
  WsLock lk;
  SRS_TRY(acquire_ws(&W, &lk));
  for (int i = 0; i < 4; i++) info[i] = W->merge_info[i];
  return SRS_OK;
}

int srs_debug_set_topk_ragged_route(int route) {
  if (route < -1 || route > TOPK_RAGGED_SORT)
    return fail(SRS_ERR_INVALID_ARG, "route must be -1, 0 or 1");
  g_topk_ragged_route.store(route);
  return SRS_OK;
}

int srs_debug_last_topk_ragged(int64_t* info) {
  if (!info) return fail(SRS_ERR_INVALID_ARG, "info is NULL");
  Workspace* W = nullptr;
  WsLock lk;
  SRS_TRY(acquire_ws(&W, &lk));
  HIP_TRY(hipDeviceSynchronize());
  for (int i = 0; i < 6; i++) info[i] = W->topk_ragged_info[i];
  return SRS_OK;
}

int srs_debug_set_topk_candidates(int64_t max_candidates) {
  g_topk_candidates.store(max_candidates > 0 ? max_candidates : kTopkCandidates);
  return SRS_OK;
}

int srs_debug_last_topk(int64_t* info) {
  if (!info) return fail(SRS_ERR_INVALID_ARG, "info is NULL");
  Workspace* W = nullptr;
  WsLock lk;
  SRS_TRY(acquire_ws(&W, &lk));
  HIP_TRY(hipDeviceSynchronize());
  for (int i = 0; i < 3; i++) info[i] = W->topk_info[i];
  return SRS_OK;
}

int srs_debug_set_topk_rows_route(int route) {
  if (route < -1 || route > ROWS_LOOP) return fail(SRS_ERR_INVALID_ARG, "route must be -1, 0, 1 or 2");
  g_topk_rows_route.store(route);
  return SRS_OK;
}

int srs_debug_last_topk_rows(int64_t* info) {
  if (!info) return fail(SRS_ERR_INVALID_ARG, "info is NULL");
  Workspace* W = nullptr;
  WsLock lk;
  SRS_TRY(acquire_ws(&W, &lk));
  HIP_TRY(hipDeviceSynchronize());
  if (W->rows_pass_pending) {
    unsigned long long passes = 0;
    HIP_TRY(hipMemcpy(&passes, W->rowspass.p, sizeof passes, hipMemcpyDeviceToHost));
    W->topk_rows_info[2] = (int64_t)passes;
    W->rows_pass_pending = false;
  }
  for (int i = 0; i < 4; i++) info[i] = W->topk_rows_info[i];
  return SRS_OK;
}

int64_t srs_topk_rows_max_k(void) { return kTopkRowsMaxK; }

int srs_debug_set_sort_rows_route(int route) {
  if (route < -1 || route > SORT_ROWS_LEVELS)
    return fail(SRS_ERR_INVALID_ARG, "route must be -1, 0, 1 or 2");
  g_sort_rows_route.store(route);
  return SRS_OK;
}

int srs_debug_last_sort_rows(int64_t* info) {
  if (!info) return fail(SRS_ERR_INVALID_ARG, "info is NULL");
  Workspace* W = nullptr;
  WsLock lk;
  SRS_TRY(acquire_ws(&W, &lk));
  for (int i = 0; i < 4; i++) info[i] = W->sort_rows_info[i];
  return SRS_OK;
}

int srs_debug_set_sort_ragged_short_max(int32_t len) {
  if (len < -1 || len > kRowsWaveMax)
    return fail(SRS_ERR_INVALID_ARG, "short_max must be -1 (default) or 0 .. 256");
  g_sort_ragged_short_max.store(len);
  return SRS_OK;
}

int srs_debug_last_sort_ragged(int64_t* info) {
  if (!info) return fail(SRS_ERR_INVALID_ARG, "info is NULL");
  Workspace* W = nullptr;
  WsLock lk;
  SRS_TRY(acquire_ws(&W, &lk));
  for (int i = 0; i < 6; i++) info[i] = W->sort_ragged_info[i];
  return SRS_OK;
}

}  // extern "C"
