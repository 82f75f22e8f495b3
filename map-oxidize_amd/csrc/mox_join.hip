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
// (mox_lookup.hip) with R's rows in the place of the uploaded queries.  R is
// usually the small side (a window against the stream's total), so its set can
// stay cache-resident while T is read sequentially once, and T's size is not
// limited by a slot's index bits.
//
//  1. k_jn_build: an open-addressing set of R's rows, the power of two >= 4 n
//     slots (at least 4,096), linear probing: the load is at most 1/4, the
//     lookup's, and the set costs 32 to 64 bytes per row of R (8 bytes per
//     slot, 4 n <= slots < 8 n) next to the 8 (or 16, with substituted counts)
//     bytes per row of the count arrays.  At 2 n (load <= 1/2, half the
//     memory) k_jn_stream measured 26 % (Zipf window) and 14 % (high
//     cardinality) slower and k_jn_build 21 % and 6 %: probes that miss are
//     twice as long, and most of T's rows miss.
//     A slot is one 64-bit word {tag: the hash's upper 32 bits,
//     row + 1: 32 bits}, 0 = empty, claimed with one compare-and-swap that
//     publishes both at once; a slot never changes once it is non-zero, so
//     nothing waits for another lane's store.  R's words are distinct, so
//     nothing is linked: an equal word met during the build sets JnCtl::err,
//     which the host turns into MOX_EHIP.  The kernel also ORs R's lengths into
//     the length filter (a bit per length below 64, a flag for the longer
//     ones).
//  2. k_jn_stream: one grid-stride pass over T, tiles of JN_TILE consecutive
//     rows, one lane per row.  A row whose length no R word has is dropped on
//     its two offsets alone.  The others are hashed and probed; behind an equal
//     tag the length and the bytes are compared exactly.  A match at R row j
//     stores T's count at jc[j] and sets bit j of the match bitmap (atomicOr:
//     32 rows share a word).  Both tables hold distinct words, so every j has
//     at most one writer.  The lookup's four-words-per-lane joint probe is
//     used: a lane's four rows of at most 16 bytes take a straight-line path
//     (one 16-byte load, at most two hash terms, the first slot) and their
//     probes advance together, one load latency per step for all four.  It
//     fits: the kernel takes the registers k_lk_stream takes (3 waves / SIMD,
//     no scratch, no VGPR spills).
//  3. k_jn_apply: one pass over R's rows.  From the bitmap, R's count and jc it
//     writes the substituted count array (MOX_JOIN_COUNTS_TOTAL / _MIN only)
//     and sums matched rows, both sides' matched tokens and the min tokens:
//     integer wave sums, then LDS, then one atomic per workgroup and sum
//     (unsigned wrapping: independent of order).  tag_mismatch is summed the
//     same way at the end of the two kernels that probe.
//
// Words of up to JN_LANE_MAX bytes are hashed and compared by their lane,
// longer ones are listed in LDS and taken by whole waves afterwards, as in
// k_lk_stream.  Every probe loop is bounded by the slot count.
//
// Loads stay inside the slack contract (mox_dev.h, mox_wordhash.h): at most 15
// bytes past a word's end, masked by its length; a zero-length word loads
// nothing.  The only stores are jc[j], the bitmap, the slots, the substituted
// counts and the control block: no table is written.
//
// Scratch: mox_engine::j_tmp = [control block | slots | jc | substituted
// counts]; the bitmap is the filter's list bitmap in f_tmp.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_jn_build    79 VGPRs, 104 SGPRs, 2052 B LDS, no scratch, no spills (6 waves / SIMD)
//   k_jn_stream  153 VGPRs, 106 SGPRs, 2056 B LDS, no scratch, 24 SGPRs spilled to VGPR lanes, no VGPR spills (3 waves / SIMD)
//   k_jn_apply    21 VGPRs,  32 SGPRs,  128 B LDS, no scratch, no spills (8 waves / SIMD)
#include <algorithm>
#include <cstdlib>

#include "mox_dev.h"
#include "mox_host.h"
#include "mox_wordhash.h"

namespace {

constexpr int JN_T = 256;                    // threads of the three kernels
constexpr int JN_WAVES = JN_T / 64;
constexpr int JN_PER = 4;                    // rows per thread and tile
constexpr uint32_t JN_TILE = JN_T * JN_PER;  // rows per tile (tests/join_cases.py TILE)
constexpr uint32_t JN_LANE_MAX = 64;         // a longer word is hashed and compared by a whole wave
constexpr uint64_t JN_SLOTS_PER_ROW = 4;     // slots: the power of two >= 4 n (load <= 1/4) ...
constexpr uint64_t JN_MIN_SLOTS = 4096;      // ... and at least 32 KiB of them
constexpr uint64_t JN_ROW_MASK = 0xFFFFFFFFull;  // slot: row + 1 below the hash's upper 32 bits
static_assert(JN_TILE == 1024, "tests/join_cases.py TILE");
static_assert(MOX_JOIN_MAX_WORDS + 1ull <= JN_ROW_MASK, "a slot holds every row + 1");
static_assert(JN_TILE <= 65536, "s_big holds 16-bit rows");
static_assert(JN_PER == 4, "k_jn_stream's joint probe loop names its four rows");

struct JnCtl {
  unsigned long long lenmask;       // bit L: an R word of L < 64 bytes
  unsigned long long longer;        // an R word of 64 bytes or more
  unsigned long long err;           // 1: k_jn_build's probe bound exhausted, 2: k_jn_stream's, 3: a slot holds no row, 4: R holds a word twice
  unsigned long long tag_mismatch;  // probes with an equal tag and different bytes (both kernels)
  unsigned long long sums[4];       // k_jn_apply: matched rows, R's / T's / min tokens over them
};
static_assert(sizeof(JnCtl) == 64, "one copy brings it back");

// A table in generic form (mox_engine::Res, or the accumulator's buffers).
struct JnTab {
  const uint64_t* counts;
  const uint64_t* offs;
  const uint8_t* bytes;
  uint64_t n;
};
// R, its set and the outputs.
struct JnSet {
  JnTab R;
  unsigned long long* slots;
  uint64_t mask;      // slots - 1
  uint64_t* jc;       // jc[j]: T's count of R's row j, where bit j is set
  uint32_t* matched;  // bit j: T holds R's row j
  JnCtl* ctl;
};

// R's row i (bytes at o, len; hash h) into the set: claims the first empty slot
// of its probe sequence.  tm += the equal tags with different bytes met.
template <bool WAVE>
__device__ __forceinline__ void jn_insert(const JnSet& S, uint64_t i, uint64_t o, uint64_t len, uint64_t h, uint32_t& tm) {
  const bool first = !WAVE || (threadIdx.x & 63) == 0;
  const uint64_t tag = h >> 32;
  const unsigned long long mine = (tag << 32) | (i + 1);
  uint64_t s = h & S.mask;
  for (uint64_t p = 0; p <= S.mask; p++, s = (s + 1) & S.mask) {
    unsigned long long cur = __hip_atomic_load(S.slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (WAVE) cur = __shfl(cur, 0);  // one view of the slot for the whole wave
    if (cur == 0) {
      unsigned long long old = 0;
      if (first) old = atomicCAS(S.slots + s, 0ull, mine);
      if (WAVE) old = __shfl(old, 0);
      if (old == 0) return;
      cur = old;  // lost the swap: the winner's tag and row, which never change
    }
    if ((cur >> 32) == tag) {
      const uint64_t j = (cur & JN_ROW_MASK) - 1;
      if (j >= S.R.n) {
        if (first) S.ctl->err = 3;
        return;
      }
      const uint64_t oj = S.R.offs[j], lj = S.R.offs[j + 1] - oj;
      if (lj == len && lk_equal<WAVE>(S.R.bytes, oj, S.R.bytes, o, len)) {
        if (first) atomicMax(&S.ctl->err, 4ull);  // a result's words are distinct
        return;
      }
      if (first) tm++;
    }
  }
  if (first) atomicMax(&S.ctl->err, 1ull);
}

// T's row ti (bytes at o, len; hash h) against the set: on a match its count
// goes to jc and the row's bit is set.
template <bool WAVE>
__device__ __forceinline__ void jn_find(const JnSet& S, const JnTab& T, uint64_t ti, uint64_t o, uint64_t len, uint64_t h, uint32_t& tm) {
  const bool first = !WAVE || (threadIdx.x & 63) == 0;
  const uint64_t tag = h >> 32;
  uint64_t s = h & S.mask;
  for (uint64_t p = 0; p <= S.mask; p++, s = (s + 1) & S.mask) {
    const unsigned long long cur = S.slots[s];
    if (cur == 0) return;  // no row of R is this word
    if ((cur >> 32) == tag) {
      const uint64_t j = (cur & JN_ROW_MASK) - 1;
      if (j >= S.R.n) {
        if (first) S.ctl->err = 3;
        return;
      }
      const uint64_t oj = S.R.offs[j], lj = S.R.offs[j + 1] - oj;
      if (lj == len && lk_equal<WAVE>(T.bytes, o, S.R.bytes, oj, len)) {
        if (first) {
          S.jc[j] = T.counts[ti];
          atomicOr(S.matched + (j >> 5), 1u << (j & 31));
        }
        return;
      }
      if (first) tm++;
    }
  }
  if (first) atomicMax(&S.ctl->err, 2ull);
}

// tag_mismatch += the workgroup's tm: one atomic per wave that met any.
__device__ __forceinline__ void jn_add_mismatch(JnCtl* ctl, uint32_t tm) {
  tm = wave_sum(tm);
  if ((threadIdx.x & 63) == 0 && tm) atomicAdd(&ctl->tag_mismatch, (unsigned long long)tm);
}

}  // namespace

// R's rows into the set; the length filter into the control block.  Tiles of
// JN_TILE rows, one lane per row, the words over JN_LANE_MAX bytes by whole
// waves afterwards.
extern "C" __global__ __launch_bounds__(JN_T) void k_jn_build(JnSet S) {
  __shared__ uint16_t s_big[JN_TILE];  // rows (inside the tile) of the words over JN_LANE_MAX bytes
  __shared__ uint32_t s_nbig;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t nt = (S.R.n + JN_TILE - 1) / JN_TILE;
  uint64_t lm = 0, lg = 0;
  uint32_t tm = 0;
  for (uint64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const uint64_t base = tile * JN_TILE;
    if (t == 0) s_nbig = 0;
    __syncthreads();
    for (int j = 0; j < JN_PER; j++) {
      const uint64_t i = base + (uint32_t)j * JN_T + t;
      if (i < S.R.n) {
        const uint64_t o = S.R.offs[i], len = S.R.offs[i + 1] - o;
        if (len < 64) lm |= 1ull << len;
        else lg = 1;
        if (len <= JN_LANE_MAX) jn_insert<false>(S, i, o, len, lk_hash<false>(S.R.bytes, o, len), tm);
        else s_big[atomicAdd(&s_nbig, 1u)] = (uint16_t)((uint32_t)j * JN_T + t);
      }
    }
    __syncthreads();
    const uint32_t nbig = s_nbig;
    for (uint32_t x = wv; x < nbig; x += JN_WAVES) {
      const uint64_t i = base + s_big[x];
      const uint64_t o = S.R.offs[i], len = S.R.offs[i + 1] - o;
      jn_insert<true>(S, i, o, len, lk_hash<true>(S.R.bytes, o, len), tm);
    }
    __syncthreads();  // the LDS list is the next tile's
  }
  for (int o = 32; o > 0; o >>= 1) {
    lm |= __shfl_xor(lm, o);
    lg |= __shfl_xor(lg, o);
  }
  if (lane == 0) {
    if (lm) atomicOr(&S.ctl->lenmask, (unsigned long long)lm);
    if (lg) atomicOr(&S.ctl->longer, 1ull);
  }
  jn_add_mismatch(S.ctl, tm);
}

// One pass over T's rows against the set (the control block's length filter is
// k_jn_build's, complete at this launch).
extern "C" __global__ __launch_bounds__(JN_T) void k_jn_stream(JnTab T, JnSet S) {
  __shared__ uint16_t s_big[JN_TILE];
  __shared__ uint32_t s_nbig[2];  // by tile parity: the other one is cleared between a tile's two barriers
  const uint32_t t = threadIdx.x, wv = t >> 6;
  const uint64_t lenmask = S.ctl->lenmask;
  const bool longer = S.ctl->longer != 0;
  const uint64_t nt = (T.n + JN_TILE - 1) / JN_TILE;
  uint32_t tm = 0;
  // a tile's offsets are loaded while the tile before it is worked on
  uint64_t o[JN_PER], len[JN_PER];
  auto load_offs = [&](uint64_t tile, uint64_t* oo, uint64_t* ll) {
#pragma unroll
    for (int j = 0; j < JN_PER; j++) {
      const uint64_t i = tile * JN_TILE + (uint32_t)j * JN_T + t;
      const bool in = tile < nt && i < T.n;
      oo[j] = in ? __builtin_nontemporal_load(T.offs + i) : 0ull;
      ll[j] = in ? __builtin_nontemporal_load(T.offs + i + 1) - oo[j] : ~0ull;  // (no word is 2^64 - 1 bytes long)
    }
  };
  load_offs(blockIdx.x, o, len);
  if (t < 2) s_nbig[t] = 0;
  __syncthreads();
  uint32_t par = 0;
  for (uint64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const uint64_t base = tile * JN_TILE;
    uint64_t w0[JN_PER], w1[JN_PER], h[JN_PER], o_next[JN_PER], len_next[JN_PER];
    unsigned long long cur[JN_PER];
    bool fast[JN_PER], slow[JN_PER];
    load_offs(tile + gridDim.x, o_next, len_next);
    // Rows of 1..16 bytes that pass the length filter take a straight-line
    // path: the 16 bytes from the word's start on (up to 15 past its end,
    // inside the slack), then the four first slots.  A lane without such a row
    // loads the buffer's first bytes and some slot instead, and ignores them.
#pragma unroll
    for (int j = 0; j < JN_PER; j++) {
      const bool pass = len[j] < 64 ? (lenmask >> len[j]) & 1ull : (longer && len[j] != ~0ull);
      fast[j] = pass && len[j] - 1 < 16;
      slow[j] = pass && !fast[j];
      const Key16 k = *reinterpret_cast<const Key16*>(T.bytes + (fast[j] ? o[j] : 0ull));
      w0[j] = k.lo;
      w1[j] = k.hi;
    }
#pragma unroll
    for (int j = 0; j < JN_PER; j++) {
      const uint64_t l = fast[j] ? len[j] : 1ull;
      uint64_t acc = lk_term(mask_low(w0[j], l), LK_POS);  // lk_hash<false>, unrolled for at most two words
      if (l > 8) acc += lk_term(mask_low(w1[j], l - 8), 2 * LK_POS);
      h[j] = lk_finish(acc, l);
      cur[j] = S.slots[h[j] & S.mask];
    }
    // The four rows' probes go on together, one round of slot loads per step.
    uint64_t sl[JN_PER];
    bool pend[JN_PER];
#pragma unroll
    for (int j = 0; j < JN_PER; j++) {
      pend[j] = fast[j];
      sl[j] = h[j] & S.mask;
    }
    for (uint64_t p = 0;; p++) {
#pragma unroll
      for (int j = 0; j < JN_PER; j++) {
        if (!pend[j]) continue;
        const unsigned long long c = cur[j];
        if (c == 0) {
          pend[j] = false;  // an empty slot: no row of R is this word
        } else if ((c >> 32) == (h[j] >> 32)) {
          const uint64_t rj = (c & JN_ROW_MASK) - 1;
          if (rj >= S.R.n) {
            S.ctl->err = 3;
            pend[j] = false;
          } else {
            const uint64_t orr = S.R.offs[rj], lr = S.R.offs[rj + 1] - orr;
            if (lr == len[j] && lk_equal<false>(T.bytes, o[j], S.R.bytes, orr, lr)) {
              S.jc[rj] = T.counts[base + (uint32_t)j * JN_T + t];
              atomicOr(S.matched + (rj >> 5), 1u << (rj & 31));
              pend[j] = false;
            } else {
              tm++;
            }
          }
        }
      }
      if (!(pend[0] || pend[1] || pend[2] || pend[3])) break;
      if (p >= S.mask) {
        atomicMax(&S.ctl->err, 2ull);
        break;
      }
#pragma unroll
      for (int j = 0; j < JN_PER; j++)
        if (pend[j]) {
          sl[j] = (sl[j] + 1) & S.mask;
          cur[j] = S.slots[sl[j]];
        }
    }
#pragma unroll
    for (int j = 0; j < JN_PER; j++)
      if (slow[j]) {
        const uint64_t i = base + (uint32_t)j * JN_T + t;
        if (len[j] <= JN_LANE_MAX) jn_find<false>(S, T, i, o[j], len[j], lk_hash<false>(T.bytes, o[j], len[j]), tm);
        else s_big[atomicAdd(&s_nbig[par], 1u)] = (uint16_t)((uint32_t)j * JN_T + t);
      }
    __syncthreads();
    const uint32_t nbig = s_nbig[par];
    if (t == 0) s_nbig[par ^ 1] = 0;  // last read before the previous tile's second barrier, next added to behind this tile's
    for (uint32_t x = wv; x < nbig; x += JN_WAVES) {
      const uint64_t i = base + s_big[x];
      const uint64_t ob = T.offs[i], lb = T.offs[i + 1] - ob;
      jn_find<true>(S, T, i, ob, lb, lk_hash<true>(T.bytes, ob, lb), tm);
    }
    __syncthreads();  // the LDS list has been read
    par ^= 1;
#pragma unroll
    for (int j = 0; j < JN_PER; j++) {
      o[j] = o_next[j];
      len[j] = len_next[j];
    }
  }
  jn_add_mismatch(S.ctl, tm);
}

// The four sums over R's matched rows, and with subst the count every row of R
// carries into the new result: T's (MOX_JOIN_COUNTS_TOTAL) or the smaller of
// both (MOX_JOIN_COUNTS_MIN) for a matched row, its own for the others.
extern "C" __global__ __launch_bounds__(JN_T) void k_jn_apply(JnSet S, uint32_t counts_mode, uint64_t* __restrict__ subst) {
  __shared__ uint64_t s_w[JN_WAVES][4];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint64_t v[4] = {0, 0, 0, 0};
  for (uint64_t i = (uint64_t)blockIdx.x * JN_T + t; i < S.R.n; i += (uint64_t)gridDim.x * JN_T) {
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
    for (int w = 0; w < JN_WAVES; w++) s += s_w[w][t];
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
  const uint64_t nslots = std::max<uint64_t>(JN_MIN_SLOTS, next_pow2(JN_SLOTS_PER_ROW * r.n));
  const size_t sl_b = 8 * nslots;
  JnSet S{};
  uint64_t* d_subst;
  if (int rc = carve_dev(e->j_tmp, [&](Carve& c) {
        S.ctl = (JnCtl*)c.take_bytes(sizeof(JnCtl) + sl_b);
        S.jc = c.take<uint64_t>(r.n);
        d_subst = sub ? c.take<uint64_t>(r.n) : nullptr;
      }))
    return rc;
  S.R = JnTab{r.counts, r.offs, r.bytes, r.n};
  S.slots = (unsigned long long*)(S.ctl + 1);
  S.mask = nslots - 1;
  S.matched = matched;
  HIPCHK(hipMemsetAsync(S.ctl, 0, sizeof(JnCtl) + sl_b, st));
  const uint64_t rtiles = (r.n + JN_TILE - 1) / JN_TILE, ttiles = (t_n + JN_TILE - 1) / JN_TILE;
  hipLaunchKernelGGL(k_jn_build, dim3((uint32_t)std::min(rtiles, cap)), dim3(JN_T), 0, st, S);
  q.step("k_jn_build");
  const JnTab T{t_counts, t_offs, t_bytes, t_n};
  hipLaunchKernelGGL(k_jn_stream, dim3((uint32_t)std::min(ttiles, cap)), dim3(JN_T), 0, st, T, S);
  q.step("k_jn_stream");
  // (a workgroup per tile of rows, not per JN_T rows: the four atomics of each workgroup meet on four addresses)
  hipLaunchKernelGGL(k_jn_apply, dim3((uint32_t)std::min(rtiles, cap)), dim3(JN_T), 0, st, S, counts_mode, d_subst);
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
