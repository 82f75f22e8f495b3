// A hash set over the words of one table (the keys) and the pass of another
// table past it: the shape of the device lookup (mox_lookup.hip: the keys are
// the uploaded queries, the table is the result) and of the device join
// (mox_join.hip: the keys are the result's rows, the table is the total).
// Everything is forced inline, as in mox_dev.h: ws_build<P> and ws_stream<P>
// are the bodies of an operator's two kernels, and what an operator does
// differently is its policy P (below).  The hash and the exact compare are
// mox_wordhash.h's.
//
//  Build (ws_build): an open-addressing set of the keys, the power of two
//     >= 4 n slots (at least 4,096: ws_slots), linear probing, so the load is
//     at most 1/4 and most probes end at their first slot.  A slot is one
//     64-bit word {tag: the hash's upper 64 - P::IDX_BITS bits, key index + 1:
//     P::IDX_BITS bits}, 0 = empty, claimed with one compare-and-swap that
//     publishes both at once.  The swap returns the slot's content, and a slot
//     never changes once it is non-zero, so the loser knows the winner from the
//     swap alone: nothing here waits for another lane's or workgroup's store,
//     and the bytes a loser compares were in memory before the launch.  A key
//     that meets a claimant with its tag, its length and its bytes claims
//     nothing and is handed to P::equal.  The kernel also ORs the key lengths
//     into the length filter (a bit per length below 64, a flag for the longer
//     ones).  Tiles of WS_TILE keys, one lane per key.
//  Stream (ws_stream): one grid-stride pass over the table, tiles of WS_TILE
//     consecutive rows, one lane per row.  A row whose length no key has is
//     dropped on its two offsets alone, without touching its bytes.  The
//     others are hashed and probed; behind an equal tag the length and the
//     bytes are compared exactly, and a match is handed to P::match.  A lane
//     holds four rows of its tile; those of at most 16 bytes (nearly every word
//     of a text) take a straight-line path -- one 16-byte load per word, the
//     hash of at most two 8-byte words, the first slot -- and their probes then
//     advance together, so that the four rows' loads are in flight at once and
//     a step of the probe costs one load latency for all four, not four in
//     series.  The next tile's offsets are loaded while a tile is worked on.
//
// Words of up to WS_LANE_MAX bytes are hashed and compared by their lane.
// Longer ones (a table word reaches 16 MiB) are listed in LDS and taken by
// whole waves afterwards: the 64 lanes load 64 consecutive 8-byte words.
//
// Every probe loop is bounded by the slot count (at most a quarter of the slots
// is ever taken, so an empty one ends each probe long before that); an exhausted
// bound sets WsCtl::err, and the host answers any non-zero err with MOX_EHIP.
// An equal tag with different bytes adds one to WsCtl::tag_mismatch: counted
// per lane and added with one atomic per wave at the end of either kernel
// (P::SUM_MISMATCH), or with one atomic each.  The sum is the same; which of
// the two an operator takes is a matter of its kernels' speed.
//
// Loads stay inside the slack contract (mox_dev.h, mox_wordhash.h): at most 15
// bytes past a word's end (the stream's 16-byte load of a short word likewise),
// masked by the length before use; a zero-length word loads nothing.  The key
// bytes are read as table bytes are, so their buffer carries the slack too.
//
// The policy P of an operator, static members only:
//   P::IDX_BITS                 the slot's split; the operator asserts that every key index + 1 fits
//   P::SUM_MISMATCH             tag_mismatch summed per wave at a kernel's end, not one atomic each
//   P::offs(S), bytes(S), n(S)  the key table of the set S
//   P::claimed(S, i)            key i took a slot
//   P::equal(S, i, j)           build: key i is the word of key j, which holds the slot
//   P::match(S, T, j, ti)       stream: the table's row ti is the word of key j
//   P::built(S, nd)             build's end, once per wave: nd of the wave's keys took a slot
// claimed, equal and match are called by one lane per word.  The set S is the
// operator's own struct; this header uses S.slots, S.mask (slots - 1) and
// S.ctl, a pointer to a control block that begins with WsCtl.
#pragma once
#include <algorithm>

#include "mox_dev.h"
#include "mox_host.h"
#include "mox_wordhash.h"

namespace mox {

constexpr int WS_T = 256;                    // threads of every kernel here
constexpr int WS_WAVES = WS_T / 64;
constexpr int WS_PER = 4;                    // rows per thread and tile
constexpr uint32_t WS_TILE = WS_T * WS_PER;  // rows per tile (tests/lookup_cases.py, tests/join_cases.py: TILE)
constexpr uint32_t WS_LANE_MAX = 64;         // a longer word is hashed and compared by a whole wave
constexpr uint64_t WS_SLOTS_PER_KEY = 4;     // slots: the power of two >= 4 n (load <= 1/4) ...
constexpr uint64_t WS_MIN_SLOTS = 4096;      // ... and at least 32 KiB of them
static_assert(WS_TILE == 1024, "tests/lookup_cases.py and tests/join_cases.py TILE");
static_assert(WS_TILE <= 65536, "s_big holds 16-bit rows");
static_assert(WS_PER == 4, "ws_stream's joint probe loop names its four rows");

// the slots of a set of n keys
inline uint64_t ws_slots(uint64_t n) { return std::max<uint64_t>(WS_MIN_SLOTS, mox_host::next_pow2(WS_SLOTS_PER_KEY * n)); }

// A table in generic form (mox_engine::Res, or the accumulator's buffers).
struct WsTab {
  const uint64_t* counts;
  const uint64_t* offs;
  const uint8_t* bytes;
  uint64_t n;
};

// The head of an operator's 64-byte control block; four words of its own follow.
struct WsCtl {
  unsigned long long lenmask;       // bit L: a key of L < 64 bytes
  unsigned long long longer;        // a key of 64 bytes or more
  unsigned long long err;           // 1: the build's probe bound exhausted, 2: the stream's, 3: a slot holds no key; from 4 on: the operator's
  unsigned long long tag_mismatch;  // probes with an equal tag and different bytes (both kernels)
};

// An equal tag with different bytes: counted in the lane's tm, which the kernel
// adds to tag_mismatch at its end (ws_add_mismatch), or added there at once.
template <class P, class Set>
__device__ __forceinline__ void ws_mismatch(const Set& S, uint32_t& tm) {
  if (P::SUM_MISMATCH) tm++;
  else atomicAdd(&S.ctl->tag_mismatch, 1ull);
}

// Key i (bytes at o, len; hash h) into the set: claims the first empty slot of
// its probe sequence, unless it meets an equal claimant before.  Returns 1 when
// it claimed a slot.  tm += the equal tags with different bytes met.
template <class P, bool WAVE, class Set>
__device__ __forceinline__ uint32_t ws_insert(const Set& S, uint64_t i, uint64_t o, uint64_t len, uint64_t h, uint32_t& tm) {
  const bool first = !WAVE || (threadIdx.x & 63) == 0;
  const uint64_t tag = h >> P::IDX_BITS;
  const unsigned long long mine = (tag << P::IDX_BITS) | (i + 1);
  uint64_t s = h & S.mask;
  for (uint64_t p = 0; p <= S.mask; p++, s = (s + 1) & S.mask) {
    unsigned long long cur = __hip_atomic_load(S.slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (WAVE) cur = __shfl(cur, 0);  // one view of the slot for the whole wave
    if (cur == 0) {
      unsigned long long old = 0;
      if (first) old = atomicCAS(S.slots + s, 0ull, mine);
      if (WAVE) old = __shfl(old, 0);
      if (old == 0) {
        if (first) P::claimed(S, i);
        return 1;
      }
      cur = old;  // lost the swap: the winner's tag and index, which never change
    }
    if ((cur >> P::IDX_BITS) == tag) {
      const uint64_t j = (cur & ((1ull << P::IDX_BITS) - 1ull)) - 1;
      if (j >= P::n(S)) {
        if (first) S.ctl->err = 3;
        return 0;
      }
      const uint64_t oj = P::offs(S)[j], lj = P::offs(S)[j + 1] - oj;
      if (lj == len && lk_equal<WAVE>(P::bytes(S), oj, P::bytes(S), o, len)) {
        if (first) P::equal(S, i, j);
        return 0;
      }
      if (first) ws_mismatch<P>(S, tm);
    }
  }
  if (first) atomicMax(&S.ctl->err, 1ull);
  return 0;
}

// The table's row ti (bytes at o, len; hash h) against the set.
template <class P, bool WAVE, class Set>
__device__ __forceinline__ void ws_find(const Set& S, const WsTab& T, uint64_t ti, uint64_t o, uint64_t len, uint64_t h, uint32_t& tm) {
  const bool first = !WAVE || (threadIdx.x & 63) == 0;
  const uint64_t tag = h >> P::IDX_BITS;
  uint64_t s = h & S.mask;
  for (uint64_t p = 0; p <= S.mask; p++, s = (s + 1) & S.mask) {
    const unsigned long long cur = S.slots[s];
    if (cur == 0) return;  // no key is this word
    if ((cur >> P::IDX_BITS) == tag) {
      const uint64_t j = (cur & ((1ull << P::IDX_BITS) - 1ull)) - 1;
      if (j >= P::n(S)) {
        if (first) S.ctl->err = 3;
        return;
      }
      const uint64_t oj = P::offs(S)[j], lj = P::offs(S)[j + 1] - oj;
      if (lj == len && lk_equal<WAVE>(T.bytes, o, P::bytes(S), oj, len)) {
        if (first) P::match(S, T, j, ti);
        return;
      }
      if (first) ws_mismatch<P>(S, tm);
    }
  }
  if (first) atomicMax(&S.ctl->err, 2ull);
}

// tag_mismatch += the workgroup's tm: one atomic per wave that met any.
__device__ __forceinline__ void ws_add_mismatch(WsCtl* ctl, uint32_t tm) {
  tm = wave_sum(tm);
  if ((threadIdx.x & 63) == 0 && tm) atomicAdd(&ctl->tag_mismatch, (unsigned long long)tm);
}

// The body of a build kernel (WS_T threads): the keys into the set, the length
// filter into the control block.
template <class P, class Set>
__device__ __forceinline__ void ws_build(const Set& S) {
  __shared__ uint16_t s_big[WS_TILE];  // rows (inside the tile) of the keys over WS_LANE_MAX bytes
  __shared__ uint32_t s_nbig;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t* offs = P::offs(S);
  const uint8_t* bytes = P::bytes(S);
  const uint64_t n = P::n(S), nt = (n + WS_TILE - 1) / WS_TILE;
  uint64_t lm = 0, lg = 0;
  uint32_t nd = 0, tm = 0;
  for (uint64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const uint64_t base = tile * WS_TILE;
    if (t == 0) s_nbig = 0;
    __syncthreads();
    for (int j = 0; j < WS_PER; j++) {
      const uint64_t i = base + (uint32_t)j * WS_T + t;
      if (i < n) {
        const uint64_t o = offs[i], len = offs[i + 1] - o;
        if (len < 64) lm |= 1ull << len;
        else lg = 1;
        if (len <= WS_LANE_MAX) nd += ws_insert<P, false>(S, i, o, len, lk_hash<false>(bytes, o, len), tm);
        else s_big[atomicAdd(&s_nbig, 1u)] = (uint16_t)((uint32_t)j * WS_T + t);
      }
    }
    __syncthreads();
    const uint32_t nbig = s_nbig;
    for (uint32_t x = wv; x < nbig; x += WS_WAVES) {
      const uint64_t i = base + s_big[x];
      const uint64_t o = offs[i], len = offs[i + 1] - o;
      const uint32_t c = ws_insert<P, true>(S, i, o, len, lk_hash<true>(bytes, o, len), tm);
      if (lane == 0) nd += c;
    }
    __syncthreads();  // the LDS list is the next tile's
  }
  for (int o = 32; o > 0; o >>= 1) {
    lm |= __shfl_xor(lm, o);
    lg |= __shfl_xor(lg, o);
    nd += __shfl_xor(nd, o);
  }
  if (lane == 0) {
    if (lm) atomicOr(&S.ctl->lenmask, (unsigned long long)lm);
    if (lg) atomicOr(&S.ctl->longer, 1ull);
    P::built(S, nd);
  }
  if (P::SUM_MISMATCH) ws_add_mismatch(S.ctl, tm);
}

// The body of a stream kernel (WS_T threads): one pass over T's rows against
// the set (the control block's length filter is the build's, complete at this
// launch).
template <class P, class Set>
__device__ __forceinline__ void ws_stream(const WsTab& T, const Set& S) {
  __shared__ uint16_t s_big[WS_TILE];
  __shared__ uint32_t s_nbig[2];  // by tile parity: the other one is cleared between a tile's two barriers
  const uint32_t t = threadIdx.x, wv = t >> 6;
  const uint64_t lenmask = S.ctl->lenmask;
  const bool longer = S.ctl->longer != 0;
  const uint64_t nt = (T.n + WS_TILE - 1) / WS_TILE;
  uint32_t tm = 0;
  // a tile's offsets are loaded while the tile before it is worked on: the
  // loads are in flight together with that tile's byte and slot loads
  uint64_t o[WS_PER], len[WS_PER];
  auto load_offs = [&](uint64_t tile, uint64_t* oo, uint64_t* ll) {
#pragma unroll
    for (int j = 0; j < WS_PER; j++) {
      const uint64_t i = tile * WS_TILE + (uint32_t)j * WS_T + t;
      const bool in = tile < nt && i < T.n;
      oo[j] = in ? __builtin_nontemporal_load(T.offs + i) : 0ull;
      ll[j] = in ? __builtin_nontemporal_load(T.offs + i + 1) - oo[j] : ~0ull;  // (no key is 2^64 - 1 bytes long)
    }
  };
  load_offs(blockIdx.x, o, len);
  if (t < 2) s_nbig[t] = 0;
  __syncthreads();
  uint32_t par = 0;
  for (uint64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const uint64_t base = tile * WS_TILE;
    uint64_t w0[WS_PER], w1[WS_PER], h[WS_PER], o_next[WS_PER], len_next[WS_PER];
    unsigned long long cur[WS_PER];
    bool fast[WS_PER], slow[WS_PER];
    load_offs(tile + gridDim.x, o_next, len_next);
    // Rows of 1..16 bytes that pass the length filter take a straight-line
    // path, so that the four rows' loads are in flight together: the 16 bytes
    // from the word's start on (up to 15 past its end, inside the slack), then
    // the four first slots.  A lane without such a row loads the buffer's
    // first bytes and some slot instead, and ignores them.
#pragma unroll
    for (int j = 0; j < WS_PER; j++) {
      const bool pass = len[j] < 64 ? (lenmask >> len[j]) & 1ull : (longer && len[j] != ~0ull);
      fast[j] = pass && len[j] - 1 < 16;
      slow[j] = pass && !fast[j];
      const Key16 k = *reinterpret_cast<const Key16*>(T.bytes + (fast[j] ? o[j] : 0ull));
      w0[j] = k.lo;
      w1[j] = k.hi;
    }
#pragma unroll
    for (int j = 0; j < WS_PER; j++) {
      const uint64_t l = fast[j] ? len[j] : 1ull;
      uint64_t acc = lk_term(mask_low(w0[j], l), LK_POS);  // lk_hash<false>, unrolled for at most two words
      if (l > 8) acc += lk_term(mask_low(w1[j], l - 8), 2 * LK_POS);
      h[j] = lk_finish(acc, l);
      cur[j] = S.slots[h[j] & S.mask];
    }
    // The four rows' probes go on together, one round of slot loads per step
    // (one row after the other would put every step's load latency in series).
    uint64_t sl[WS_PER];
    bool pend[WS_PER];
#pragma unroll
    for (int j = 0; j < WS_PER; j++) {
      pend[j] = fast[j];
      sl[j] = h[j] & S.mask;
    }
    for (uint64_t p = 0;; p++) {
#pragma unroll
      for (int j = 0; j < WS_PER; j++) {
        if (!pend[j]) continue;
        const unsigned long long c = cur[j];
        if (c == 0) {
          pend[j] = false;  // an empty slot: no key is this word
        } else if ((c >> P::IDX_BITS) == (h[j] >> P::IDX_BITS)) {
          const uint64_t kj = (c & ((1ull << P::IDX_BITS) - 1ull)) - 1;
          if (kj >= P::n(S)) {
            S.ctl->err = 3;
            pend[j] = false;
          } else {
            const uint64_t ok = P::offs(S)[kj], lk = P::offs(S)[kj + 1] - ok;
            if (lk == len[j] && lk_equal<false>(T.bytes, o[j], P::bytes(S), ok, lk)) {
              P::match(S, T, kj, base + (uint32_t)j * WS_T + t);
              pend[j] = false;
            } else {
              ws_mismatch<P>(S, tm);
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
      for (int j = 0; j < WS_PER; j++)
        if (pend[j]) {
          sl[j] = (sl[j] + 1) & S.mask;
          cur[j] = S.slots[sl[j]];
        }
    }
#pragma unroll
    for (int j = 0; j < WS_PER; j++)
      if (slow[j]) {
        const uint64_t i = base + (uint32_t)j * WS_T + t;
        if (len[j] <= WS_LANE_MAX) ws_find<P, false>(S, T, i, o[j], len[j], lk_hash<false>(T.bytes, o[j], len[j]), tm);
        else s_big[atomicAdd(&s_nbig[par], 1u)] = (uint16_t)((uint32_t)j * WS_T + t);
      }
    __syncthreads();
    const uint32_t nbig = s_nbig[par];
    if (t == 0) s_nbig[par ^ 1] = 0;  // last read before the previous tile's second barrier, next added to behind this tile's
    for (uint32_t x = wv; x < nbig; x += WS_WAVES) {
      const uint64_t i = base + s_big[x];
      const uint64_t ob = T.offs[i], lb = T.offs[i + 1] - ob;
      ws_find<P, true>(S, T, i, ob, lb, lk_hash<true>(T.bytes, ob, lb), tm);
    }
    __syncthreads();  // the LDS list has been read
    par ^= 1;
#pragma unroll
    for (int j = 0; j < WS_PER; j++) {
      o[j] = o_next[j];
      len[j] = len_next[j];
    }
  }
  if (P::SUM_MISMATCH) ws_add_mismatch(S.ctl, tm);
}

}  // namespace mox
