// srs_driver.h — the host driver's internal interface: what srs_api.hip
// defines and the library's other units call (srs_batch.hip: top-k, the
// row-wise and the ragged calls; srs_shard.hip: the four functions at the
// end). Declarations and plain structs; the definitions and their comments
// are in srs_api.hip.
#pragma once

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/srs_c_api.h"
#include "srs_kernels.h"

namespace srs {

int fail(int code, const std::string& msg);  // sets srs_last_error; returns code

#define HIP_TRY(expr)                                                            \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess)                                                        \
      return fail(e_ == hipErrorOutOfMemory ? SRS_ERR_OUT_OF_MEMORY : SRS_ERR_HIP, \
                  std::string(#expr " -> ") + hipGetErrorString(e_));            \
  } while (0)

#define SRS_TRY(expr)          \
  do {                         \
    int r_ = (expr);           \
    if (r_ != SRS_OK) return r_; \
  } while (0)

int64_t knob_int(const char* name, int64_t dflt);
int ws_alloc_mode();  // SRS_WS_ALLOC: how the big workspace buffers are backed

// kernel timing (optional; HIP events around every launch on its stream)
struct TimingRec {
  std::string name;
  std::string name2;  // optional second family (per-level names: "scatter.L1")
  hipEvent_t a, b;
  double elems;
};
struct TimedScope {
  bool on = false;
  TimingRec rec;
  hipStream_t st;
  TimedScope(const char* name, double elems, hipStream_t s, int level = 0);
  ~TimedScope();
};

// the per-device workspace (grown on demand, reused across calls)
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int mode = 0;  // how p was allocated (BigAlloc); 0 = hipMalloc
};
int ensure(DevBuf& b, size_t bytes, int mode = 0, bool placed = false);
void cpu_relax();
int sync_poll(hipStream_t st);
size_t align_up(size_t x, size_t a);
size_t col_offsets(int64_t n, int ncols, const uint32_t* widths, std::vector<size_t>* off);

struct Workspace {
  DevBuf tmp;         // TMP data buffer (same footprint as the input)
  DevBuf tmp2;        // TMP2: AoS records as SoA slice columns (SortDesc::tmp2)
  DevBuf stage;       // device copy of host arrays (host-pointer API)
  DevBuf desc;        // SortDesc
  DevBuf big[2], local, local2, copy, fallback, fallback2, redo, redo2;
  DevBuf plan, tcount, gcount, tbase, gbase, var, sbase;
  DevBuf tile_seg, group_seg, hist, offs, gsum, gofs, scan_tmp, totals, ctr;
  DevBuf shist, lut, lut_rbits;  // balanced first level (sampled histogram, digit table)
  // stripe first level: piece sizes and tile prefixes, bucket totals, the
  // second level's tile counts and gathered tile table (GTile)
  DevBuf prun, ptile, btot, bnt, btile, nt_over, gtile, gorder;
  int64_t gorder_cap = 0;
  DevBuf mid;  // mid-size single launch: the tiles' key OR / AND, their digit counts
  DevBuf midbar;  // and its grid barrier's words (zeroed once)
  // top-k: the compact columns of the selected records, the select pass's
  // histogram row, the tally's tile counts / bases / scan temp, the gather's
  // column descriptor; the row's pinned copy; what the last call did
  DevBuf sel, selhist, selcnt, seldesc;
  unsigned long long* h_sel = nullptr;
  int64_t topk_info[3] = {0, 0, 0};
  // row-wise top-k: the kernel's pass counter (one u64); what the last call did
  DevBuf rowspass;
  int64_t topk_rows_info[4] = {0, 0, 0, 0};
  bool rows_pass_pending = false;  // info[2] is still in rowspass
  // row-wise sort: the rows kernel's pass counter (unused, its own word so
  // that the top-k hook's stays that call's); what the last call did
  DevBuf sortrowspass;
  int64_t sort_rows_info[4] = {0, 0, 0, 0};
  // ragged sort: what the last call did; the event behind its counter copy
  int64_t sort_ragged_info[6] = {0, 0, 0, 0, 0, 0};
  hipEvent_t ev_ragged = nullptr;
  // ragged top-k: the device counters and their pinned copy, the list of long
  // segments, the sort route's columns of num records; what the last call did
  DevBuf tkrctr, tkrlist, tkrcols;
  TopkRaggedCounters* h_tkr = nullptr;
  int64_t topk_ragged_info[6] = {0, 0, 0, 0, 0, 0};
  // unique: the sorted columns (and the index column) the caller did not ask
  // for; the tile counts / bases / scan temp / total; the count's pinned copy;
  // what the last call did
  DevBuf uniqcols, uniqcnt;
  int64_t* h_uniq = nullptr;
  int64_t unique_info[4] = {0, 0, 0, 0};
  // search-sorted: the sort route's copy of the queries and its index column;
  // what the last call did
  DevBuf searchcols;
  int64_t search_info[4] = {0, 0, 0, 0};
  // merge: the tile boundaries' split of A (int64 per boundary); what the last
  // call did
  DevBuf mergesplit;
  int64_t merge_info[4] = {0, 0, 0, 0};
  hipStream_t side = nullptr;  // medium sorts: the large local class's stream
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  ListCounters* h_ctr = nullptr;
  uint64_t* h_totals = nullptr;
  MidFlag* h_mid = nullptr;        // the mid-size launch's early answer
  unsigned long long mid_seq = 0;  // (its sequence numbers)
  // Stream order of the workspace: the last call's kernels may still be
  // queued on its stream when the call returns. `idle` is recorded on that
  // stream at the end of every call; the next call's stream waits for it
  // before its first workspace write (WsUse).
  hipEvent_t idle = nullptr;
  bool idle_pending = false;
  // single-launch small sorts (run_small): which fallback bodies ran, for
  // srs_debug_last_fallbacks. One slot per stream: small sorts skip the
  // workspace's stream-order wait, so sorts on different streams must not
  // share a slot (the map is only touched under `mu`).
  std::map<hipStream_t, DevBuf> small_taken;
  bool last_small = false;
  hipStream_t last_small_stream = nullptr;
  // what the last sort above kLocalCap did first (srs_debug_last_first_level)
  int64_t first_level_info[6] = {-1, 0, 0, 0, 0, 0};
  // one call at a time per device (calls on different devices run in
  // parallel: the multi-GPU host split sorts its shards from several threads)
  std::mutex mu;
  // Freed when the last holder lets go (srs_release_workspace only drops the
  // registry's reference, so a call that has looked the workspace up keeps
  // it alive until it returns).
  ~Workspace();
};

// A workspace held for one call: the reference keeps it alive, the lock
// (taken after the lookup, released first) makes the call its only user.
struct WsLock {
  std::shared_ptr<Workspace> ref;
  std::unique_lock<std::mutex> lk;
};
// The current device's workspace, locked for this call.
int acquire_ws(Workspace** out, WsLock* lk);

// Holds the workspace for one call on stream `st` (under W->mu): waits on the
// device for the previous call's work on the workspace (any stream), and
// marks the end of this call's work when it goes out of scope, also on error.
struct WsUse {
  Workspace* W = nullptr;
  hipStream_t st = nullptr;
  int begin(Workspace* w, hipStream_t s);
  ~WsUse();
};

// One call's hold on the current device's workspace: the lock, then (begin)
// its place in the workspace's stream order. `use` goes first on scope exit.
struct WsScope {
  Workspace* W = nullptr;
  WsLock lk;
  WsUse use;
  int lock() { return acquire_ws(&W, &lk); }
  int begin(hipStream_t st);
};

struct Request {
  int64_t num;
  int kind;
  int up;
  int64_t thresh;
  bool aos;
  uint32_t elem_size;                // AoS record size
  void* in_cols[SRS_MAX_PAYLOADS + 1];
  void* out_cols[SRS_MAX_PAYLOADS + 1];
  uint32_t widths[SRS_MAX_PAYLOADS + 1];
  int ncols;                         // SoA: 1 + payloads; AoS: 1
  const int64_t* seg_bounds = nullptr;  // optional: sort [b[i], b[i+1]) independently
  int64_t nsegs = 0;
  int known_top_bits = 0;               // every segment's keys agree on these top bits
  int leaf_mode = SRS_LEAF_SORTED;      // SRS_LEAF_UNSORTED: CmpSorterNoSort
};
int build_soa(Request& R, int64_t num, int kind, int up, int64_t thresh, void* keys, int32_t np,
              void* const* pays, const uint32_t* sizes, void* keys_out, void* const* pays_out);
int build_aos(Request& R, int64_t num, int kind, int up, int64_t thresh, void* elems,
              uint32_t esz, void* elems_out);
int key_size_of(int kind);
SortDesc init_desc(int kind, int up);  // zeroed, with the key transform of (kind, up)
void set_columns(const Request& R, SortDesc& d, char* tmp, char* tmp2, bool aos_cols,
                 size_t slice_bytes, const size_t* tmp_off, bool inplace, bool pair = false);
bool is_inplace(const Request& R);
// one device column's word alignment (rows: the row-wise calls' message)
int check_col_alignment(const Request& R, int c, bool rows);
int copy_through(const Request& R, hipStream_t st);
// a sort under the caller's workspace lock and WsUse, on the same stream
int sort_locked(Workspace* W, const Request& R, hipStream_t st);

struct LevelState {
  int64_t nbig, n_local, n_local2, n_copy;
  int cur;
  int ncols;               // columns moved with the keys (SortDesc::ncols)
  int tmp2;                // SortDesc::tmp2
  int64_t known_len = -1;  // the length of the single big segment, when the host knows it
  int pair_tiles = 0;      // the scatter takes two count tiles per workgroup (pair_tiles_mode)
  bool row_offs = false;   // and sums its tile offsets from the count rows (SRS_PAIR_ROW_OFFS)
  int level = 0;           // global levels run so far (per-level timing names)
  int64_t ntiles = 0;      // tiles of the last level run
};
enum TableKind {
  TABLE_NONE = 0,   // a plain digit
  TABLE_ANY = 1,    // a digit table of any kind (SortDesc::digit_lut)
  TABLE_SMALL = 2,  // a small kind (key ranges, split table: the kernels with the small LDS table)
};
// How a level reads and hands on its segments: 1 a stripe level (its
// segments are stripes of the input, partitioned each on its own; the next
// level's segments are the buckets, read through a gathered tile table); 2
// that gathered level. See GTile (srs_common.h).
enum StripeMode { STRIPE_NONE = 0, STRIPE_LEVEL = 1, STRIPE_GATHERED = 2 };
struct LevelSpec {
  int bits = 0;                     // the digit's width; 0: the plan kernel chooses per segment
  bool plain = false;               // bits > 0: a plain digit of that width (else the table's)
  TableKind table = TABLE_NONE;
  const int32_t* rbits = nullptr;   // a table level: its groups' rbits (device)
  StripeMode stripe = STRIPE_NONE;
  const GTile* gt = nullptr;        // gathered level
  const int32_t* nt_over = nullptr; // gathered level: tiles per segment
  const int32_t* torder = nullptr;  // gathered level: the count's tile order (stripe-major)
  int key_bits = 0;                 // stripe level
  bool home = false;                // every bucket of this level is final: scatter to OUT
};
int pair_tiles_mode(const SortDesc& d, int ks, bool aos_slices);
int run_level(Workspace* W, int ks, const SortDesc* d_desc, LevelState& S, hipStream_t st,
              const LevelSpec& M = LevelSpec());
int ensure_lists(Workspace* W, size_t n_big, size_t n_local, size_t n_local2);
// The list driver (a sort whose segments the caller puts into the work
// lists): list_begin, the caller's own list launches, list_finish.
LevelState level_state(const SortDesc& d, int ks, bool aos_slices, int64_t nbig = 0,
                       int64_t n_local = 0, int64_t n_local2 = 0, int64_t n_copy = 0,
                       int64_t known_len = -1);
int list_begin(Workspace* W, const Request& Q, bool inplace, bool levels, hipStream_t st,
               SortDesc* d, SortDesc** d_desc);
int list_finish(Workspace* W, const Request& Q, const SortDesc& d, const SortDesc* d_desc,
                LevelState S, int level, bool aos_cols, int64_t* readbacks, hipStream_t st);

// for srs_shard.hip:
int set_error(int code, const std::string& msg);  // (fail, under its older name)
int reserve_segments_workspace(int64_t num, int ncols, const uint32_t* widths);
// workspace frees of this thread held back while peers' messages are queued
// on the device (a hipFree would wait for them, unbounded)
void defer_workspace_frees(bool on);
int64_t release_deferred_frees();

}  // namespace srs
