// Device join (mox_join_total): the device-resident result R matched against
// the accumulator's total T on the GPU, so that "which of this window's words
// are new", "which were seen before, and how often overall" and the overlap
// sums of two corpora are answered without fetching either table (DESIGN.md
// §4, "Joining the result against the total").  Nothing sized by a table goes
// up or comes down: one 64-byte control block comes back.
//
// This file holds the match; the compaction of the kept rows is the filter's
// own (mox_filter.hip: k_fl_count / k_fl_scan / k_fl_emit over the match bitmap
// as the list bitmap), driven by mox_join_total there.
//
// The set is built over R and T is streamed past it: the lookup's shape
// (mox_lookup.hip) with R's rows in the place of the uploaded queries, and the
// same code (mox_wordset.h, which describes the set, the joint probe of the
// stream, the probe bounds and the loads inside the slack contract).  R is
// usually the small side (a window against the stream's total), so its set can
// stay cache-resident while T is read sequentially once, and T's size is not
// limited by a slot's index bits.
//
//  1. k_jn_build (ws_build): the set of R's rows.  A slot holds the hash's
//     upper 32 bits above row + 1 in 32.  At a load of at most 1/4 the set
//     costs 32 to 64 bytes per row of R (8 bytes per slot, 4 n <= slots < 8 n)
//     next to the 8 (or 16, with substituted counts) bytes per row of the count
//     arrays.  At 2 n (load <= 1/2, half the memory) k_jn_stream measured 26 %
//     (Zipf window) and 14 % (high cardinality) slower and k_jn_build 21 % and
//     6 %: probes that miss are twice as long, and most of T's rows miss
//     (DESIGN.md §8).  R's words are distinct, so nothing is linked: an equal
//     word met during the build sets JnCtl::err to 4, which the host turns
//     into MOX_EHIP.
//  2. k_jn_stream (ws_stream): one pass over T.  A match at R row j stores T's
//     count at jc[j] and sets bit j of the match bitmap (atomicOr: 32 rows
//     share a word).  Both tables hold distinct words, so every j has at most
//     one writer.
//  3. k_jn_apply: one pass over R's rows.  From the bitmap, R's count and jc it
//     writes the substituted count array (MOX_JOIN_COUNTS_TOTAL / _MIN only)
//     and sums matched rows, both sides' matched tokens and the min tokens:
//     integer wave sums, then LDS, then one atomic per workgroup and sum
//     (unsigned wrapping: independent of order).  tag_mismatch is summed the
//     same way at the end of the two kernels that probe (SUM_MISMATCH).
//
// The only stores are jc[j], the bitmap, the slots, the substituted counts and
// the control block: no table is written.
//
// Scratch: mox_engine::j_tmp = [control block | slots | jc | substituted
// counts]; the bitmap is the filter's list bitmap in f_tmp.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_jn_build    79 VGPRs,  92 SGPRs, 2052 B LDS, no scratch, no spills (6 waves / SIMD)
//   k_jn_stream  156 VGPRs, 106 SGPRs, 2056 B LDS, no scratch, 26 SGPRs spilled to VGPR lanes, no VGPR spills (3 waves / SIMD)
//   k_jn_apply    21 VGPRs,  32 SGPRs,  128 B LDS, no scratch, no spills (8 waves / SIMD)
#include <algorithm>
#include <cstdlib>

#include "mox_dev.h"
#include "mox_host.h"
#include "mox_wordset.h"

namespace {

struct JnCtl : WsCtl {         // err 4: R holds a word twice
  unsigned long long sums[4];  // k_jn_apply: matched rows, R's / T's / min tokens over them
};
static_assert(sizeof(JnCtl) == 64, "one copy brings it back");

// R, its set and the outputs.
struct JnSet {
  WsTab R;
  unsigned long long* slots;
  uint64_t mask;      // slots - 1
  uint64_t* jc;       // jc[j]: T's count of R's row j, where bit j is set
  uint32_t* matched;  // bit j: T holds R's row j
  JnCtl* ctl;
};

// The join's word set (mox_wordset.h): the keys are R's rows.
struct JnWords {
  static constexpr int IDX_BITS = 32;  // slot: row + 1 below the hash's upper 32 bits
  static constexpr bool SUM_MISMATCH = true;  // tag_mismatch: a counter per lane, one atomic per wave
  static __device__ __forceinline__ const uint64_t* offs(const JnSet& S) { return S.R.offs; }
  static __device__ __forceinline__ const uint8_t* bytes(const JnSet& S) { return S.R.bytes; }
  static __device__ __forceinline__ uint64_t n(const JnSet& S) { return S.R.n; }
  static __device__ __forceinline__ void claimed(const JnSet&, uint64_t) {}
  static __device__ __forceinline__ void equal(const JnSet& S, uint64_t, uint64_t) {
    atomicMax(&S.ctl->err, 4ull);  // a result's words are distinct
  }
  // T's count goes to jc and the row's bit is set
  static __device__ __forceinline__ void match(const JnSet& S, const WsTab& T, uint64_t j, uint64_t ti) {
    S.jc[j] = T.counts[ti];
    atomicOr(S.matched + (j >> 5), 1u << (j & 31));
  }
  static __device__ __forceinline__ void built(const JnSet&, uint32_t) {}
};
static_assert(MOX_JOIN_MAX_WORDS + 1ull <= (1ull << JnWords::IDX_BITS) - 1ull, "a slot holds every row + 1");

}  // namespace

extern "C" __global__ __launch_bounds__(WS_T) void k_jn_build(JnSet S) { ws_build<JnWords>(S); }

extern "C" __global__ __launch_bounds__(WS_T) void k_jn_stream(WsTab T, JnSet S) { ws_stream<JnWords>(T, S); }

// The four sums over R's matched rows, and with subst the count every row of R
// carries into the new result: T's (MOX_JOIN_COUNTS_TOTAL) or the smaller of
// both (MOX_JOIN_COUNTS_MIN) for a matched row, its own for the others.
extern "C" __global__ __launch_bounds__(WS_T) void k_jn_apply(JnSet S, uint32_t counts_mode, uint64_t* __restrict__ subst) {
  __shared__ uint64_t s_w[WS_WAVES][4];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint64_t v[4] = {0, 0, 0, 0};
  for (uint64_t i = (uint64_t)blockIdx.x * WS_T + t; i < S.R.n; i += (uint64_t)gridDim.x * WS_T) {
    const bool m = (S.matched[i >> 5] >> (i & 31)) & 1u;
    const uint64_t c = S.R.counts[i];
    uint64_t out = c;
    if (m) {
      const uint64_t tc = S.jc[i], mn = tc < c ? tc : c;
      v[0]++;
      v[1] += c;
      v[2] += tc;
      v[3] += mn;
      out = counts_mode == MOX_JOIN_COUNTS_TOTAL ? tc : mn;
    }
    if (subst) subst[i] = out;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    v[k] = wave_sum(v[k]);
    if (lane == 0) s_w[wv][k] = v[k];
  }
  __syncthreads();
  if (t < 4) {
    uint64_t s = 0;
    for (int w = 0; w < WS_WAVES; w++) s += s_w[w][t];
    if (s) atomicAdd(&S.ctl->sums[t], (unsigned long long)s);
  }
}

namespace mox_host {

// The match of mox_join_total (mox_filter.hip): bit j of matched (r.n bits,
// zeroed by the caller, in device memory) is set where the table t holds the
// word of r's row j; *sums are the sums over those rows.  With counts_mode
// MOX_JOIN_COUNTS_TOTAL / _MIN *subst is the array of the r.n counts the rows
// carry into the new result (in j_tmp, valid until the next join).  Both
// tables hold rows; every grid is capped at cap workgroups.  Synchronises.
int join_match(mox_engine* e, const mox_engine::Res& r, const uint64_t* t_counts, const uint64_t* t_offs, const uint8_t* t_bytes,
               uint64_t t_n, uint32_t counts_mode, uint32_t* matched, uint64_t cap, JoinSums* sums, const uint64_t** subst) {
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  const bool sub = counts_mode != MOX_JOIN_COUNTS_RESULT;
  // device scratch: [control block | slots] (zeroed together) | jc | substituted counts
  const uint64_t nslots = ws_slots(r.n);
  const size_t sl_b = 8 * nslots;
  JnSet S{};
  uint64_t* d_subst;
  if (int rc = carve_dev(e->j_tmp, [&](Carve& c) {
        S.ctl = (JnCtl*)c.take_bytes(sizeof(JnCtl) + sl_b);
        S.jc = c.take<uint64_t>(r.n);
        d_subst = sub ? c.take<uint64_t>(r.n) : nullptr;
      }))
    return rc;
  S.R = WsTab{r.counts, r.offs, r.bytes, r.n};
  S.slots = (unsigned long long*)(S.ctl + 1);
  S.mask = nslots - 1;
  S.matched = matched;
  HIPCHK(hipMemsetAsync(S.ctl, 0, sizeof(JnCtl) + sl_b, st));
  const uint64_t rtiles = (r.n + WS_TILE - 1) / WS_TILE, ttiles = (t_n + WS_TILE - 1) / WS_TILE;
  hipLaunchKernelGGL(k_jn_build, dim3((uint32_t)std::min(rtiles, cap)), dim3(WS_T), 0, st, S);
  q.step("k_jn_build");
  const WsTab T{t_counts, t_offs, t_bytes, t_n};
  hipLaunchKernelGGL(k_jn_stream, dim3((uint32_t)std::min(ttiles, cap)), dim3(WS_T), 0, st, T, S);
  q.step("k_jn_stream");
  // (a workgroup per tile of rows, not per WS_T rows: the four atomics of each workgroup meet on four addresses)
  hipLaunchKernelGGL(k_jn_apply, dim3((uint32_t)std::min(rtiles, cap)), dim3(WS_T), 0, st, S, counts_mode, d_subst);
  q.step("k_jn_apply");
  HIPCHK(hipGetLastError());
  JnCtl h;
  HIPCHK(hipMemcpyAsync(&h, S.ctl, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (h.err || h.sums[0] > std::min(r.n, t_n))
    return fail(MOX_EHIP, "join: inconsistent row set (error %llu, %llu matched of %llu and %llu rows)", h.err, h.sums[0],
                (unsigned long long)r.n, (unsigned long long)t_n);
  sums->matched = h.sums[0];
  sums->tokens_result = h.sums[1];
  sums->tokens_total = h.sums[2];
  sums->tokens_min = h.sums[3];
  sums->tag_mismatch = h.tag_mismatch;
  *subst = d_subst;
  return MOX_OK;
}

}  // namespace mox_host
