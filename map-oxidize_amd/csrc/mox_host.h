// Host side of libmox.so: the engine object and the helpers shared by the
// pass driver (mox_engine.hip), the multi-GPU exchange / gather / engine group
// (mox_multi.hip), the device bytewise table sort (mox_bsort.hip) and the
// device top-k (mox_topk.hip), the device text rendering (mox_text.hip) and
// the device-resident accumulator (mox_accum.hip), the device lookup
// (mox_lookup.hip), the device filter (mox_filter.hip), the device ranking
// (mox_rank.hip), the device re-keying (mox_rekey.hip), the device search
// of the sorted result (mox_find.hip), the device join against the total
// (mox_join.hip) and the device histograms of the result (mox_hist.hip); the buffers
// of the calls over the result are grown, laid out and freed in one place
// (mox_result.hip, mox_carve.h).  The device-side
// helpers those kernels share are in mox_dev.h and mox_pack.h (the two
// packers); the host-side ones (result_begin, table_reserve and the
// declarations around it, Received: the hand-off to the reduce-only pass) are below.
// Internal: the public interface is include/mox.h.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/mox.h"
#include "mox_carve.h"
#include "mox_internal.h"
#include "mox_table.h"

using namespace mox;

extern "C" {
__global__ void k_map(Corpus c, Work w, uint64_t nrows, uint32_t resume);
__global__ void k_init(Work w, unsigned long long w_n, uint32_t flags);
__global__ void k_ctl_out(const Ctl* src, Ctl* dst);
__global__ void k_sample(Corpus c, Work w, uint32_t npieces);
__global__ void k_dict_hist(Work w);
__global__ void k_dict_pick(Work w, uint32_t max_words);
__global__ void k_dict_build(Work w, uint32_t max_words);
__global__ void k_dict_zero(Work w);
__global__ void k_unicode(Corpus c, Work w, Tables T);
__global__ void k_hist(Work w);
__global__ void k_scatter(Work w);
__global__ void k_reduce(Work w);
__global__ void k_reduce_z(Work w);
__global__ void k_split_count(Work w);
__global__ void k_unit_scan(Work w);
__global__ void k_split_scatter(Work w);
__global__ void k_unit_uniq_scan(Work w);
__global__ void k_final_scan(Work w);
__global__ void k_reduce_small(Work w);
__global__ void k_reduce_sort1(Work w);
__global__ void k_reduce_sort2(Work w);
__global__ void k_mat(Work w, Corpus c);
__global__ void k_xcount(Work w, uint32_t P, XCnt* xcnt);
__global__ void k_xpack_short(Work w, WRec* out);
__global__ void k_xpack_long(Work w, XDir dir, unsigned long long* cur, uint8_t* blob);
__global__ void k_xsample(Work w, uint64_t* out);
__global__ void k_xsplit(const uint64_t* blocks, uint32_t P, uint64_t* sp, uint32_t* flag);
__global__ void k_xcount_r(Work w, XSplit x, XCnt* xcnt);
__global__ void k_xpack_r(Work w, XSplit x, XDir dir, unsigned long long* cur, WRec* out, uint8_t* blob);
__global__ void k_xingest(Work w, XDir dir, uint64_t n_short);
__global__ void k_gather_offs(const uint8_t* recv, GDir d, uint64_t* out);
}

namespace mox_host {
// Buffer-growth reruns of one pass: every overflow kind grows its buffers in
// one step, but an attempt that overflowed early (cold regions, the split
// layout) does not reach the later checks (table, bytes), so the kinds can be
// met one attempt after another
constexpr int GROW_RETRIES = 8;


// thread-local last error (mox_last_error) and the status-returning setter
extern thread_local std::string g_err;
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIPCHK(expr)                                                                             \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return fail(MOX_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

#define RCCLCHK(expr)                                                                            \
  do {                                                                                           \
    ncclResult_t r_ = (expr);                                                                    \
    if (r_ != ncclSuccess) return fail(MOX_ERCCL, "%s failed: %s", #expr, ncclGetErrorString(r_)); \
  } while (0)

inline uint64_t next_pow2(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};
// Capacities of the size-dependent pass buffers.
struct Caps {
  uint64_t cold_cap, spill_cap, w_cap, u_cap, arena_cap, long_cap, table_cap, bytes_cap, split_k_cap, split_w_cap;
};
struct XPlan;  // mox_multi.hip
struct Group;  // mox_multi.hip

}  // namespace mox_host

using namespace mox_host;

struct mox_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  // async passes: pass k + 1's dictionary is built on dstream while pass k's
  // reduce tail runs on stream (ev_dready: the next dictionary is built).  The
  // dictionary buffers are double-buffered (dsets): a side build writes the set
  // the previous pass did not use, and the pass before that one has completed
  // on the host by then (mox_run_range_async completes pass k - 1 before it
  // returns), so the side stream waits for nothing.  (A side build that waited
  // for pass k's k_map, to run beside the reduce tail only, measured 1.1 %
  // slower end to end: profiles/r05/c2_side_dict_overlap.txt.)
  hipStream_t dstream = nullptr;
  hipEvent_t ev_dready = nullptr;
  struct DictSet {
    WRec* cand = nullptr;
    uint32_t* dict_hist = nullptr;
    WRec* dict_list = nullptr;
    uint32_t* dict_tag = nullptr;
    uint4* dict_key = nullptr;
    unsigned long long* dict_tot = nullptr;
  } dsets[2];
  int dcur = 0;  // the set the last enqueued pass used (it is in e->w)
  uint32_t flags = 0, dict_words = DICT_MAX_WORDS, sample_pieces = 192;
  int n_cu = 256;
  bool sync_each = false;
  bool verbose = false;         // MOX_VERBOSE: one line per pass attempt on stderr
  int test_fail_alloc = 0;     // MOX_TEST_FAIL_ALLOC=k: the k-th sized allocation fails once (tests)
  uint64_t next_cold_cap = 0;  // region capacity learnt from spills of an earlier run
  Caps grow_hint{};            // capacities an overflowed, superseded async pass asked for (next run)
  Work w{};
  Tables tables{};
  Ctl* h_ctl = nullptr;       // pinned
  Ctl* h_ctl_init = nullptr;  // pinned
  // pinned, 64 bytes: the totals accumulate, filter and re-key read back (each
  // runs on the engine's one host thread and has consumed them before it returns)
  uint64_t* h_tot = nullptr;
  // engine-owned corpus staging for host inputs
  uint8_t* d_text = nullptr;
  size_t d_text_cap = 0;
  hipStream_t file_stream[16]{};  // mox_count_file readers (up to MAX_FILE_READERS); [0] = the shared copy stream
  hipEvent_t file_ev[16][2]{};    // copy of reader t's buffer k done (shared copy stream)
  hipEvent_t file_land = nullptr; // overlapped file pass: copies of a byte prefix done (shared copy stream)
  uint8_t* file_pin[16][2]{};
  size_t file_pin_bytes = 0;      // size of each pinned reader buffer
  // last run
  bool have_result = false;
  // where the result table lives (the pass's t_* buffers, or the gather buffers)
  struct Res {
    const uint64_t* counts = nullptr;
    const uint64_t* offs = nullptr;
    const uint8_t* bytes = nullptr;
    uint64_t n = 0, nb = 0, tokens = 0;
    bool pass = false;       // true: the t_* buffers of the last pass (an exchange can start from it)
    bool exchanged = false;  // true: the final table of an exchange (this rank's words are final: gatherable)
    bool sorted = false;     // true: in bytewise order (bsort_table)
    bool ranked = false;     // true: ordered by count (mox_rank_result): the implicit MOX_F_SORT_BYTES sort leaves it alone
    bool folded = false;     // true: already part of the accumulator (mox_accumulate takes a result once)
  } res;
  // mox_accumulate (mox_accum.hip): the running total as a saved table (a_tab:
  // counts, offs, bytes; table_reserve) and the packer's tile counts
  struct Acc {
    bool have = false, sorted = false, ranked = false;
    uint64_t n = 0, nb = 0, tokens = 0, passes = 0;
  } acc;
  DevBuf a_tab[3], a_tc;
  DevBuf g_counts, g_offs, g_bytes, g_recv;  // mox_gather (root)
  DevBuf s_counts, s_offs, s_bytes, s_tmp;    // device bytewise sort (mox_bsort.hip): output + scratch
  DevBuf h_bsort;                             // pinned: the sort's digit histograms + totals
  DevBuf k_tmp, k_out;                        // device top-k (mox_topk.hip): scratch, output block
  // device text rendering (mox_text.hip): scanned tile lengths, two device slices,
  // their pinned host copies and the events "slice copied"
  DevBuf tx_pre, tx_slice[2], tx_pin[2];
  hipEvent_t tx_ev[2]{};
  // device lookup (mox_lookup.hip): scratch (outputs, query words, their hash set),
  // the pinned block the offsets go up and the outputs come back through
  DevBuf l_tmp, l_pin;
  // device filter (mox_filter.hip): two sets of output buffers (counts, offs,
  // bytes; table_reserve; a call writes the set the result does not live in:
  // table_other_set) and the scratch (tile arrays, keep masks, list bitmap)
  DevBuf f_tab[2][3], f_tmp;
  // device ranking (mox_rank.hip): two sets of output buffers (as f_tab), the
  // scratch (keys, row indices, digit counts, tile bytes) and the pinned block
  // maxima / totals
  DevBuf r_tab[2][3], r_tmp;
  DevBuf h_rmax;
  // device re-keying (mox_rekey.hip): the packer's tile counts (the wire image
  // goes to x_recv_short / x_recv_blob)
  DevBuf q_tc;
  // device search (mox_find.hip): scratch (outputs, keys, scanned tile sums), the
  // pinned block the key offsets go up and the outputs come back through
  DevBuf fd_tmp, fd_pin;
  // device join (mox_join.hip): scratch (control block, the hash set over the
  // result's rows, matched and substituted counts); the match bitmap, the tile
  // arrays and the output are the filter's (f_tmp, f_tab)
  DevBuf j_tmp;
  // device histograms (mox_hist.hip): scratch (the derived keys, the tile heads
  // and tile sums), the bins on the device, the pinned block of the totals
  DevBuf hg_tmp, hg_out, hg_pin;
  Corpus last_corpus{};
  mox_stats stats{};
  hipEvent_t ev[12]{};
  // mox_run_range_async: two pass slots (the newest pass is enqueued before the
  // previous one is completed, so the GPU runs them back to back)
  struct AsyncSlot {
    bool pending = false;
    Corpus c{};
    Ctl* h_ctl = nullptr;                  // pinned copy of this pass's control block
    hipEvent_t ev_map0 = nullptr, ev_map1 = nullptr, ev_done = nullptr;
  } aslot[2];
  int anext = 0;
  // multi-GPU, one process per GPU (mox_comm_init)
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  XCnt* d_xcnt = nullptr;                 // [0, MAX_RANKS) sent, [MAX_RANKS, 2 MAX_RANKS) received
  XCnt* h_xcnt = nullptr;                 // pinned mirror
  unsigned long long* d_xcur = nullptr;   // 3 MAX_RANKS pack cursors
  uint64_t* d_xs = nullptr;               // sorted exchange: MAX_RANKS x XS_BLOCK sample blocks sent (one copy per peer)
  uint64_t* d_xr = nullptr;               // ... and received
  uint64_t* d_xsp = nullptr;              // MAX_RANKS splitters (k_xsplit), then the skew flag word
  uint32_t* h_xflag = nullptr;            // pinned copy of the skew flag
  hipEvent_t ev_xs = nullptr;             // engine group, copy transport: this member's sample block is written
  DevBuf x_send_short, x_send_blob, x_recv_short, x_recv_blob;  // device
  DevBuf hx_send, hx_recv;                // pinned host staging (host transport)
  Ctl* h_ctl_x = nullptr;                 // pinned control block of an exchange pass
  XPlan* xp = nullptr;                    // layout of the exchange in progress (mox_multi.hip)
  // engine group (mox_config.n_gpus > 1): this engine is member 0 and drives
  // the others from one host thread (mox_multi.hip)
  Group* grp = nullptr;
};

namespace mox_host {
// ---- mox_engine.hip
int dalloc(mox_engine* e, void** p, size_t bytes);
void dfree(void* p);
Caps caps_of(const Work& w);
Caps initial_caps(uint64_t n, int map_grid);
Caps caps_max(const Caps& a, const Caps& b);
int ensure_caps(mox_engine* e, const Caps& need);
Caps grow_for(mox_engine* e, const Ctl& h);
int check_failed(const Ctl& h);
void set_result(mox_engine* e, const Ctl& h);
int drain_async(mox_engine* e);
// Opens a call over the result: pending async passes are completed, there is a
// result, its device is current.  (Argument checks of the caller come first.)
inline int result_begin(mox_engine* e) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  if (int rc = drain_async(e)) return rc;
  if (!e->have_result) return fail(MOX_ESTATE, "no result: run first");
  HIPCHK(hipSetDevice(e->device));
  return MOX_OK;
}
int run_corpus(mox_engine* e, const Corpus& c);
Corpus make_corpus(const void* d_buf, size_t buf_len, size_t own_begin, size_t own_end, int at_end);
// Launch sequencing helpers: HIP-event timestamps (MOX_F_TIMING) and, with
// MOX_SYNC_EACH=1, a synchronisation + name after every launch (hang / fault
// triage).
struct Seq {
  mox_engine* e;
  hipStream_t s;
  bool timing, sync_each, map_only;
  hipEvent_t map_ev[2] = {nullptr, nullptr};  // async passes: their own map events
  void rec(int i) const;
  void step(const char* name) const;
};
Seq seq_of(mox_engine* e);
// zero: the pass holds weighted records with count 0 (k_reduce_z instead of k_reduce; mox_kernels.hip)
void launch_reduce_tail(mox_engine* e, const Corpus& c, const Seq& q, bool zero);
int finish_pass(mox_engine* e, const Seq& q);
int engine_create_one(const mox_config* cfg, int device, mox_engine** out);
int stage_host_range(mox_engine* e, const uint8_t* text, size_t len);
int stage_file_range(mox_engine* e, int fd, uint64_t off, size_t len);
// MOX_F_SORT_BYTES before a fetch: the implicit device sort (mox_fetch_table, mox_fetch_rows, mox_find_ranges).
int sort_for_fetch(mox_engine* e, bool* host_sort);
// ---- mox_result.hip
int grow_dev(DevBuf& b, size_t bytes);
int grow_pinned(DevBuf& b, size_t bytes);
void free_bufs(std::initializer_list<DevBuf*> bufs);  // device buffers: freed and reset
// b grown to hold what layout(Carve&) takes, then laid out by the same calls (mox_carve.h).
template <class F>
int carve_dev(DevBuf& b, F&& layout) {
  Carve size;
  layout(size);
  if (int rc = grow_dev(b, size.used)) return rc;
  Carve place{(uint8_t*)b.p};
  layout(place);
  return MOX_OK;
}
// The slack every buffer of a result table carries past its contents (mox_dev.h:
// what the kernels may read past a word because of it).
constexpr size_t TABLE_SLACK = 64;
// Buffers for a table of n rows and nb bytes.
int table_reserve(DevBuf& counts, DevBuf& offs, DevBuf& bytes, uint64_t n, uint64_t nb);
// Of two sets of table buffers (counts, offs, bytes), the one the result r does not live in.
DevBuf* table_other_set(DevBuf (*sets)[3], const mox_engine::Res& r);
// r's table is the one in set[0..2], an operator's buffers: no pass table and no
// exchanged one; the order flags and folded stay the caller's.
void res_point_at(mox_engine::Res& r, DevBuf* set, uint64_t n, uint64_t nb, uint64_t tokens);
// The grid cap of the kernels over table tiles: 8 workgroups per CU, or fewer with the environment variable env (tests).
uint64_t grid_cap(const mox_engine* e, const char* env);
// true when the environment variable env is a non-zero number: a call fails there on purpose (tests).
bool test_fail_hook(const char* env);
// Every buffer the calls over the result own (device and pinned), and the text's events.
void result_free(mox_engine* e);
// ---- mox_multi.hip
void group_destroy(mox_engine* e);
int group_create(mox_engine* e, const mox_config* cfg);
int group_count_host(mox_engine* e, const uint8_t* text, size_t len);
int group_count_file(mox_engine* e, const char* path);
int group_count_fd(mox_engine* e, int fd, uint64_t off, uint64_t len);  // bytes [off, off + len) of an open file
// What a reduce-only pass takes over: rs WRecs in x_recv_short, rb bytes of
// long-word blobs in x_recv_blob (r_long headers in all, laid out as dir says);
// zero: a WRec may have count 0 (the pass takes k_reduce_z).
struct Received {
  uint64_t rs = 0, rb = 0, r_long = 0;
  XDir dir{};
  bool zero = false;
};
// One source (dir.P = 1): rs WRecs, r_long headers and behind them long_bytes bytes of words, each padded to 8.
Received received_one(uint64_t rs, uint64_t r_long, uint64_t long_bytes, bool zero);
int received_reserve(mox_engine* e, const Received& rx);  // x_recv_short / x_recv_blob hold what rx describes
int reduce_received(mox_engine* e, const Received& rx, const mox_stats& local, std::chrono::steady_clock::time_point t0);
// The stats the pass over a packed result starts from (accumulate, re-key): the run's, with rx's records and no retries.
mox_stats packed_stats(mox_engine* e, const Received& rx);
void xplan_free(mox_engine* e);
// ---- mox_bsort.hip
int bsort_table(mox_engine* e);  // the result table in bytewise order, on the device
// ---- mox_lookup.hip
int lookup_device(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, uint64_t n, uint64_t* counts, uint64_t* index,
                  mox_lookup_info* info, const uint64_t** d_index);
// ---- mox_rank.hip
// The stable order of n u64 keys on the device (the ranking's radix sort of (key ^ flip,
// row) pairs over r_tmp).  Valid until the next call that uses r_tmp.
struct RankOrder {
  const uint64_t* keys = nullptr;       // [n] key ^ flip in ascending order; NULL: no pass ran (every key is 0), the order is the source's
  const uint32_t* rows = nullptr;       // [n] the source row of each; NULL with keys
  uint64_t flip = 0, max_key = 0;       // max_key: the largest key as given (not flipped)
  uint32_t passes = 0;                  // ceil(bitlen(max_key) / 8)
  const uint32_t* d_counted = nullptr;  // device: the rows the last pass counted (the caller checks it against n); NULL with keys
  void* extra = nullptr;                // device: the caller's extra bytes behind the sort's scratch
};
// cap: the grid cap of every launch; extra: bytes of the caller's own scratch in r_tmp.  n >= 1.
int rank_order(mox_engine* e, const uint64_t* d_keys, uint64_t n, uint64_t flip, uint64_t cap, size_t extra, RankOrder* out);
// ---- mox_join.hip
// Sums over the rows of the result whose word the other table holds.
struct JoinSums {
  uint64_t matched = 0, tokens_result = 0, tokens_total = 0, tokens_min = 0, tag_mismatch = 0;
};
int join_match(mox_engine* e, const mox_engine::Res& r, const uint64_t* t_counts, const uint64_t* t_offs, const uint8_t* t_bytes,
               uint64_t t_n, uint32_t counts_mode, uint32_t* matched, uint64_t cap, JoinSums* sums, const uint64_t** subst);
}  // namespace mox_host
