// Device lookup (mox_lookup_words): the counts of given words read out of the
// device-resident result, so that a vocabulary, a watch list or one word is
// answered without fetching the table ("Looking words up").
// Only the query words go up and one count (and index) per query comes back.
//
// Order-agnostic: the queries become a hash set in device memory and the
// result's words are streamed past it once, so the same code serves a table
// in engine order, in rank order after a gather and in bytewise order.
//
//  1. k_lk_build: an open-addressing set of the queries, the power of two >= 4 n
//     slots (at least 4,096), linear probing.  A slot is one 64-bit word {tag: the hash's upper
//     LK_TAG_BITS bits, query index + 1: LK_IDX_BITS bits}, 0 = empty, claimed
//     with one compare-and-swap that publishes both at once.  The swap returns
//     the slot's content, and a slot never changes once it is non-zero, so the
//     loser knows the winner from the swap alone: nothing here waits for
//     another lane's or workgroup's store, and the bytes a loser compares were
//     uploaded before the launch.  A query equal to its slot's claimant (same
//     tag, same length, same bytes) links to it (rep[i] = the claimant) and
//     claims nothing: the set holds distinct words only.  The kernel also ORs
//     the query lengths into the length filter (a bit per length below 64, a
//     flag for the longer ones).
//  2. k_lk_stream: one grid-stride pass over the result, tiles of LK_TILE
//     consecutive words, one lane per word.  A word whose length no query has
//     is dropped on its two offsets alone, without touching its bytes.  The
//     others are hashed and probed; behind an equal tag the length and the
//     bytes are compared exactly, and a match stores the word's count and table
//     index at the representative query.  Table words are distinct, so every
//     representative has at most one writer.  A lane holds four words of its
//     tile; those of at most 16 bytes (nearly every word of a text) take a
//     straight-line path -- one 16-byte load per word, the hash of at most two
//     8-byte words, the first slot -- and their probes then advance together, so
//     that the four words' loads are in flight at once and a step of the probe
//     costs one load latency for all four, not four in series.  The next tile's
//     offsets are loaded while a tile is worked on.
//  3. k_lk_finish: representatives' outputs copied to their duplicates, and
//     the found positions counted.  One copy brings counts, the control block
//     and the indices to the host.
//
// Words of up to LK_LANE_MAX bytes are hashed and compared by their lane.
// Longer ones (a table word reaches 16 MiB) are listed in LDS and taken by
// whole waves afterwards: the 64 lanes load 64 consecutive 8-byte words
// (mox_dev.h: funnel).  The hash is made for that: a sum
// over the word's 8-byte little-endian words (the last one masked by the
// length) of a bijection of (word ^ position key), plus a multiple of the
// length, then a 64-bit avalanche and fnv_finish (the forced-collision build
// truncates it there).  A sum has no serial chain, so a wave hashes a long
// word 64 words at a time and the lane path gives the same value.  The length
// is part of the hash and of every compare: "ab" and "ab\0" are different
// words.
//
// Every probe loop is bounded by the slot count (at most a quarter of the slots
// is ever taken, so an empty one ends each probe long before that); an exhausted
// bound sets LkCtl::err, which the host turns into MOX_EHIP.
//
// Loads: a word at byte offset o is read as aligned 8-byte words from o & ~7
// and a funnel shift, up to 15 bytes past its end (k_lk_stream's path for
// words of at most 16 bytes: the 16 bytes from o on, in one load of any
// alignment).  That is inside the slack of every bytes buffer a result can
// live in (mox_dev.h: the slack contract), which the query buffer here
// carries too; what is read past a word is masked before it is used.  A
// zero-length word loads nothing.
//
// Scratch (mox_engine::l_tmp, l_pin) is O(n + query bytes): the output block,
// the representatives, the query offsets and bytes and the slots.  Nothing is
// sized by the table, and the result is only read.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_lk_build    82 VGPRs,  94 SGPRs, 2052 B LDS, no scratch, no spills (5 waves / SIMD)
//   k_lk_stream  158 VGPRs, 106 SGPRs, 2056 B LDS, no scratch, 25 SGPRs spilled to VGPR lanes (3 waves / SIMD)
//   k_lk_finish   20 VGPRs,  28 SGPRs,    4 B LDS, no scratch, no spills (8 waves / SIMD)
#include <algorithm>
#include <cstdlib>

#include "mox_dev.h"
#include "mox_host.h"
#include "mox_wordhash.h"

namespace {

constexpr int LK_T = 256;                    // threads of the three kernels
constexpr int LK_WAVES = LK_T / 64;
constexpr int LK_PER = 4;                    // words per thread and tile
constexpr uint32_t LK_TILE = LK_T * LK_PER;  // words per tile (tests/lookup_cases.py TILE)
constexpr uint32_t LK_LANE_MAX = 64;         // a longer word is hashed and compared by a whole wave
constexpr int LK_IDX_BITS = 21;              // slot: query index + 1 ...
constexpr int LK_TAG_BITS = 43;              // ... below the hash's upper bits
constexpr uint64_t LK_SLOTS_PER_QUERY = 4;     // slots: the power of two >= 4 n (load <= 1/4: most probes end at their first slot) ...
constexpr uint64_t LK_MIN_SLOTS = 4096;        // ... and at least 32 KiB of them
constexpr uint64_t LK_IDX_MASK = (1ull << LK_IDX_BITS) - 1ull;
static_assert(LK_TILE == 1024, "tests/lookup_cases.py TILE");
static_assert(LK_IDX_BITS + LK_TAG_BITS == 64 && MOX_LOOKUP_MAX + 1ull <= LK_IDX_MASK, "a slot holds every query index + 1");
static_assert(LK_TILE <= 65536, "s_big holds 16-bit rows");
static_assert(LK_PER == 4, "k_lk_stream's joint probe loop names its four words");

struct LkCtl {
  unsigned long long lenmask;       // bit L: a query of L < 64 bytes
  unsigned long long longer;        // a query of 64 bytes or more
  unsigned long long err;           // 1: k_lk_build's probe bound exhausted, 2: k_lk_stream's, 3: a slot holds no query
  unsigned long long tag_mismatch;  // probes with an equal tag and different bytes (both kernels)
  unsigned long long distinct;      // queries that claimed a slot
  unsigned long long found;         // query positions whose word the result holds
  unsigned long long pad[2];
};
static_assert(sizeof(LkCtl) == 64, "copied with the counts");

// The result in generic form (mox_engine::Res).
struct LkTab {
  const uint64_t* counts;
  const uint64_t* offs;
  const uint8_t* bytes;
  uint64_t n;
};
// The uploaded queries, their set and the outputs.
struct LkSet {
  const uint64_t* qoffs;
  const uint8_t* qbytes;
  uint64_t nq;
  unsigned long long* slots;
  uint64_t mask;  // slots - 1
  uint32_t* rep;
  uint64_t* o_counts;
  uint64_t* o_index;
  LkCtl* ctl;
};

// (the word hash and the exact compare, lk_hash and lk_equal, are shared with the join: mox_wordhash.h)

// Query i (bytes at o, len; hash h) into the set: claims the first empty slot
// of its probe sequence, or links to an equal claimant met before it.
// Returns 1 when it claimed a slot (a distinct word), 0 for a duplicate.
template <bool WAVE>
__device__ __forceinline__ uint32_t lk_insert(const LkSet& S, uint64_t i, uint64_t o, uint64_t len, uint64_t h) {
  const bool first = !WAVE || (threadIdx.x & 63) == 0;
  const uint64_t tag = h >> LK_IDX_BITS;
  const unsigned long long mine = (tag << LK_IDX_BITS) | (i + 1);
  uint64_t s = h & S.mask;
  for (uint64_t p = 0; p <= S.mask; p++, s = (s + 1) & S.mask) {
    unsigned long long cur = __hip_atomic_load(S.slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (WAVE) cur = __shfl(cur, 0);  // one view of the slot for the whole wave
    if (cur == 0) {
      unsigned long long old = 0;
      if (first) old = atomicCAS(S.slots + s, 0ull, mine);
      if (WAVE) old = __shfl(old, 0);
      if (old == 0) {
        if (first) S.rep[i] = (uint32_t)i;
        return 1;
      }
      cur = old;  // lost the swap: the winner's tag and index, which never change
    }
    if ((cur >> LK_IDX_BITS) == tag) {
      const uint64_t j = (cur & LK_IDX_MASK) - 1;
      if (j >= S.nq) {
        if (first) S.ctl->err = 3;
        break;
      }
      const uint64_t oj = S.qoffs[j], lj = S.qoffs[j + 1] - oj;
      if (lj == len && lk_equal<WAVE>(S.qbytes, oj, S.qbytes, o, len)) {
        if (first) S.rep[i] = (uint32_t)j;
        return 0;
      }
      if (first) atomicAdd(&S.ctl->tag_mismatch, 1ull);
    }
  }
  if (first) {
    S.rep[i] = (uint32_t)i;
    atomicMax(&S.ctl->err, 1ull);
  }
  return 0;
}

// Table word ti (bytes at o, len; hash h) against the set: on a match its
// count and index go to the representative query.
template <bool WAVE>
__device__ __forceinline__ void lk_find(const LkSet& S, const LkTab& T, uint64_t ti, uint64_t o, uint64_t len, uint64_t h) {
  const bool first = !WAVE || (threadIdx.x & 63) == 0;
  const uint64_t tag = h >> LK_IDX_BITS;
  uint64_t s = h & S.mask;
  for (uint64_t p = 0; p <= S.mask; p++, s = (s + 1) & S.mask) {
    const unsigned long long cur = S.slots[s];
    if (cur == 0) return;  // no query is this word
    if ((cur >> LK_IDX_BITS) == tag) {
      const uint64_t j = (cur & LK_IDX_MASK) - 1;
      if (j >= S.nq) {
        if (first) S.ctl->err = 3;
        return;
      }
      const uint64_t oj = S.qoffs[j], lj = S.qoffs[j + 1] - oj;
      if (lj == len && lk_equal<WAVE>(T.bytes, o, S.qbytes, oj, len)) {
        if (first) {
          S.o_counts[j] = T.counts[ti];
          S.o_index[j] = ti;
        }
        return;
      }
      if (first) atomicAdd(&S.ctl->tag_mismatch, 1ull);
    }
  }
  if (first) atomicMax(&S.ctl->err, 2ull);
}

}  // namespace

// The queries into the set; the length filter and the distinct count into the
// control block.  Tiles of LK_TILE queries, one lane per query, the queries
// over LK_LANE_MAX bytes by whole waves afterwards.
extern "C" __global__ __launch_bounds__(LK_T) void k_lk_build(LkSet S) {
  __shared__ uint16_t s_big[LK_TILE];  // rows (inside the tile) of the queries over LK_LANE_MAX bytes
  __shared__ uint32_t s_nbig;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t nt = (S.nq + LK_TILE - 1) / LK_TILE;
  uint64_t lm = 0, lg = 0;
  uint32_t nd = 0;
  for (uint64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const uint64_t base = tile * LK_TILE;
    if (t == 0) s_nbig = 0;
    __syncthreads();
    for (int j = 0; j < LK_PER; j++) {
      const uint64_t i = base + (uint32_t)j * LK_T + t;
      if (i < S.nq) {
        const uint64_t o = S.qoffs[i], len = S.qoffs[i + 1] - o;
        if (len < 64) lm |= 1ull << len;
        else lg = 1;
        if (len <= LK_LANE_MAX) nd += lk_insert<false>(S, i, o, len, lk_hash<false>(S.qbytes, o, len));
        else s_big[atomicAdd(&s_nbig, 1u)] = (uint16_t)((uint32_t)j * LK_T + t);
      }
    }
    __syncthreads();
    const uint32_t nbig = s_nbig;
    for (uint32_t x = wv; x < nbig; x += LK_WAVES) {
      const uint64_t i = base + s_big[x];
      const uint64_t o = S.qoffs[i], len = S.qoffs[i + 1] - o;
      const uint32_t c = lk_insert<true>(S, i, o, len, lk_hash<true>(S.qbytes, o, len));
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
    if (nd) atomicAdd(&S.ctl->distinct, (unsigned long long)nd);
  }
}

// One pass over the result's words against the set (the control block's
// length filter is k_lk_build's, complete at this launch).
extern "C" __global__ __launch_bounds__(LK_T) void k_lk_stream(LkTab T, LkSet S) {
  __shared__ uint16_t s_big[LK_TILE];
  __shared__ uint32_t s_nbig[2];  // by tile parity: the other one is cleared between a tile's two barriers
  const uint32_t t = threadIdx.x, wv = t >> 6;
  const uint64_t lenmask = S.ctl->lenmask;
  const bool longer = S.ctl->longer != 0;
  const uint64_t nt = (T.n + LK_TILE - 1) / LK_TILE;
  // a tile's offsets are loaded while the tile before it is worked on: the
  // loads are in flight together with that tile's byte and slot loads
  uint64_t o[LK_PER], len[LK_PER];
  auto load_offs = [&](uint64_t tile, uint64_t* oo, uint64_t* ll) {
#pragma unroll
    for (int j = 0; j < LK_PER; j++) {
      const uint64_t i = tile * LK_TILE + (uint32_t)j * LK_T + t;
      const bool in = tile < nt && i < T.n;
      oo[j] = in ? __builtin_nontemporal_load(T.offs + i) : 0ull;
      ll[j] = in ? __builtin_nontemporal_load(T.offs + i + 1) - oo[j] : ~0ull;  // (no query is 2^64 - 1 bytes long)
    }
  };
  load_offs(blockIdx.x, o, len);
  if (t < 2) s_nbig[t] = 0;
  __syncthreads();
  uint32_t par = 0;
  for (uint64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const uint64_t base = tile * LK_TILE;
    uint64_t w0[LK_PER], w1[LK_PER], h[LK_PER], o_next[LK_PER], len_next[LK_PER];
    unsigned long long cur[LK_PER];
    bool fast[LK_PER], slow[LK_PER];
    load_offs(tile + gridDim.x, o_next, len_next);
    // Words of 1..16 bytes that pass the length filter take a straight-line
    // path, so that the four words' loads are in flight together: the 16 bytes
    // from the word's start on (up to 15 past its end, inside the slack), then
    // the four first slots.  A lane without such a word loads the buffer's
    // first bytes and some slot instead, and ignores them.
#pragma unroll
    for (int j = 0; j < LK_PER; j++) {
      const bool pass = len[j] < 64 ? (lenmask >> len[j]) & 1ull : (longer && len[j] != ~0ull);
      fast[j] = pass && len[j] - 1 < 16;
      slow[j] = pass && !fast[j];
      const Key16 k = *reinterpret_cast<const Key16*>(T.bytes + (fast[j] ? o[j] : 0ull));
      w0[j] = k.lo;
      w1[j] = k.hi;
    }
#pragma unroll
    for (int j = 0; j < LK_PER; j++) {
      const uint64_t l = fast[j] ? len[j] : 1ull;
      uint64_t acc = lk_term(mask_low(w0[j], l), LK_POS);  // lk_hash<false>, unrolled for at most two words
      if (l > 8) acc += lk_term(mask_low(w1[j], l - 8), 2 * LK_POS);
      h[j] = lk_finish(acc, l);
      cur[j] = S.slots[h[j] & S.mask];
    }
    // The four words' probes go on together, one round of slot loads per step
    // (one word after the other would put every step's load latency in series).
    uint64_t sl[LK_PER];
    bool pend[LK_PER];
#pragma unroll
    for (int j = 0; j < LK_PER; j++) {
      pend[j] = fast[j];
      sl[j] = h[j] & S.mask;
    }
    for (uint64_t p = 0;; p++) {
#pragma unroll
      for (int j = 0; j < LK_PER; j++) {
        if (!pend[j]) continue;
        const unsigned long long c = cur[j];
        if (c == 0) {
          pend[j] = false;  // an empty slot: no query is this word
        } else if ((c >> LK_IDX_BITS) == (h[j] >> LK_IDX_BITS)) {
          const uint64_t qi = (c & LK_IDX_MASK) - 1;
          if (qi >= S.nq) {
            S.ctl->err = 3;
            pend[j] = false;
          } else {
            const uint64_t oq = S.qoffs[qi], lq = S.qoffs[qi + 1] - oq;
            if (lq == len[j] && lk_equal<false>(T.bytes, o[j], S.qbytes, oq, lq)) {
              const uint64_t i = base + (uint32_t)j * LK_T + t;
              S.o_counts[qi] = T.counts[i];
              S.o_index[qi] = i;
              pend[j] = false;
            } else {
              atomicAdd(&S.ctl->tag_mismatch, 1ull);
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
      for (int j = 0; j < LK_PER; j++)
        if (pend[j]) {
          sl[j] = (sl[j] + 1) & S.mask;
          cur[j] = S.slots[sl[j]];
        }
    }
#pragma unroll
    for (int j = 0; j < LK_PER; j++)
      if (slow[j]) {
        const uint64_t i = base + (uint32_t)j * LK_T + t;
        if (len[j] <= LK_LANE_MAX) lk_find<false>(S, T, i, o[j], len[j], lk_hash<false>(T.bytes, o[j], len[j]));
        else s_big[atomicAdd(&s_nbig[par], 1u)] = (uint16_t)((uint32_t)j * LK_T + t);
      }
    __syncthreads();
    const uint32_t nbig = s_nbig[par];
    if (t == 0) s_nbig[par ^ 1] = 0;  // last read before the previous tile's second barrier, next added to behind this tile's
    for (uint32_t x = wv; x < nbig; x += LK_WAVES) {
      const uint64_t i = base + s_big[x];
      const uint64_t ob = T.offs[i], lb = T.offs[i + 1] - ob;
      lk_find<true>(S, T, i, ob, lb, lk_hash<true>(T.bytes, ob, lb));
    }
    __syncthreads();  // the LDS list has been read
    par ^= 1;
#pragma unroll
    for (int j = 0; j < LK_PER; j++) {
      o[j] = o_next[j];
      len[j] = len_next[j];
    }
  }
}

// Duplicates take their representative's outputs (a representative's own are
// only read here); the found positions are counted.
extern "C" __global__ __launch_bounds__(LK_T) void k_lk_finish(LkSet S) {
  uint32_t nf = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * LK_T + threadIdx.x; i < S.nq; i += (uint64_t)gridDim.x * LK_T) {
    const uint64_t r = S.rep[i];
    if (r >= S.nq) {
      S.ctl->err = 3;
      continue;
    }
    const uint64_t idx = S.o_index[r];
    if (r != i) {
      S.o_counts[i] = S.o_counts[r];
      S.o_index[i] = idx;
    }
    nf += idx != MOX_LOOKUP_NONE ? 1u : 0u;
  }
  __shared__ uint32_t s_nf;
  if (threadIdx.x == 0) s_nf = 0;
  __syncthreads();
  nf = wave_sum(nf);
  if ((threadIdx.x & 63) == 0 && nf) atomicAdd(&s_nf, nf);
  __syncthreads();
  if (threadIdx.x == 0 && s_nf) atomicAdd(&S.ctl->found, (unsigned long long)s_nf);
}

namespace mox_host {

// mox_lookup_words; with d_index (mox_filter.hip) counts may be NULL, and
// *d_index is the index array in device memory (n entries in l_tmp, valid until
// the next lookup; NULL for n == 0): then only the control block comes back.
int lookup_device(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, uint64_t n, uint64_t* counts, uint64_t* index,
                  mox_lookup_info* info, const uint64_t** d_index) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  if (d_index) *d_index = nullptr;
  if (n > MOX_LOOKUP_MAX) return fail(MOX_EINVAL, "lookup: %llu words (at most MOX_LOOKUP_MAX = %u)", (unsigned long long)n, MOX_LOOKUP_MAX);
  if (n && (!offs || (!counts && !d_index))) return fail(MOX_EINVAL, "lookup: NULL argument");
  uint64_t nb = 0;
  for (uint64_t i = 0; i < n; i++)
    if (offs[i + 1] < offs[i]) return fail(MOX_EINVAL, "lookup: offsets decrease at word %llu", (unsigned long long)i);
  if (n) nb = offs[n] - offs[0];
  if (nb >> 32) return fail(MOX_EINVAL, "lookup: %llu query bytes (fewer than 2^32)", (unsigned long long)nb);
  if (nb && !bytes) return fail(MOX_EINVAL, "lookup: NULL argument");
  if (int rc = result_begin(e)) return rc;
  mox_lookup_info li{};
  li.queries = n;
  if (!n) {
    if (info) *info = li;
    return MOX_OK;
  }
  const mox_engine::Res& r = e->res;
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  int rc;
  // device scratch: [counts n | control block | index n] (the part that comes back) | rep | query offsets | slots | query bytes
  const uint64_t nslots = std::max<uint64_t>(LK_MIN_SLOTS, next_pow2(LK_SLOTS_PER_QUERY * n));
  const size_t out_b = 16 * n + sizeof(LkCtl), qo_b = 8 * (n + 1), sl_b = 8 * nslots;
  LkSet S{};
  uint8_t *out, *d_qbytes;
  uint64_t* d_qoffs;
  if ((rc = carve_dev(e->l_tmp, [&](Carve& c) {
         out = c.take_bytes(out_b);
         S.rep = c.take<uint32_t>(n);
         d_qoffs = c.take<uint64_t>(n + 1);
         S.slots = c.take<unsigned long long>(nslots);
         d_qbytes = c.take_bytes(nb + TABLE_SLACK);  // (the query bytes are read as table bytes are)
       })))
    return rc;
  if ((rc = grow_pinned(e->l_pin, std::max(out_b, qo_b)))) return rc;
  S.o_counts = (uint64_t*)out;
  S.ctl = (LkCtl*)(out + 8 * n);
  S.o_index = (uint64_t*)(out + 8 * n + sizeof(LkCtl));
  S.qoffs = d_qoffs;
  S.qbytes = d_qbytes;
  S.nq = n;
  S.mask = nslots - 1;
  // the offsets rebased to the first word, through the pinned block
  uint64_t* h_offs = (uint64_t*)e->l_pin.p;
  for (uint64_t i = 0; i <= n; i++) h_offs[i] = offs[i] - offs[0];
  HIPCHK(hipMemcpyAsync(d_qoffs, h_offs, qo_b, hipMemcpyHostToDevice, st));
  if (nb) HIPCHK(hipMemcpyAsync(d_qbytes, bytes + offs[0], nb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(S.o_counts, 0, 8 * n + sizeof(LkCtl), st));
  HIPCHK(hipMemsetAsync(S.o_index, 0xFF, 8 * n, st));  // MOX_LOOKUP_NONE
  HIPCHK(hipMemsetAsync(S.slots, 0, sl_b, st));
  const uint64_t cap = 8ull * (uint64_t)e->n_cu;
  const uint64_t qtiles = (n + LK_TILE - 1) / LK_TILE;
  hipLaunchKernelGGL(k_lk_build, dim3((uint32_t)std::min(qtiles, cap)), dim3(LK_T), 0, st, S);
  q.step("k_lk_build");
  if (r.n) {
    const uint64_t scap = grid_cap(e, "MOX_LOOKUP_GRID");
    const uint64_t ttiles = (r.n + LK_TILE - 1) / LK_TILE;
    const LkTab T{r.counts, r.offs, r.bytes, r.n};
    hipLaunchKernelGGL(k_lk_stream, dim3((uint32_t)std::min(ttiles, scap)), dim3(LK_T), 0, st, T, S);
    q.step("k_lk_stream");
  }
  hipLaunchKernelGGL(k_lk_finish, dim3((uint32_t)std::min((n + LK_T - 1) / LK_T, cap)), dim3(LK_T), 0, st, S);
  q.step("k_lk_finish");
  HIPCHK(hipGetLastError());
  // the one copy back: the counts and the control block, and the indices when they are asked for
  uint8_t* h_out = (uint8_t*)e->l_pin.p;
  if (counts) HIPCHK(hipMemcpyAsync(h_out, S.o_counts, index ? out_b : 8 * n + sizeof(LkCtl), hipMemcpyDeviceToHost, st));
  else HIPCHK(hipMemcpyAsync(h_out + 8 * n, S.ctl, sizeof(LkCtl), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  LkCtl h;
  memcpy(&h, h_out + 8 * n, sizeof h);
  if (h.err || h.distinct > n || h.found > n)
    return fail(MOX_EHIP, "lookup: inconsistent query set (error %llu, %llu distinct, %llu found of %llu)", h.err, h.distinct, h.found,
                (unsigned long long)n);
  if (counts) memcpy(counts, h_out, 8 * n);
  if (counts && index) memcpy(index, h_out + 8 * n + sizeof(LkCtl), 8 * n);
  if (d_index) *d_index = S.o_index;
  li.distinct = h.distinct;
  li.found = h.found;
  li.tag_mismatch = h.tag_mismatch;
  if (info) *info = li;
  return MOX_OK;
}

}  // namespace mox_host

extern "C" int mox_lookup_words(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, uint64_t n, uint64_t* counts,
                                uint64_t* index, mox_lookup_info* info) {
  return lookup_device(e, bytes, offs, n, counts, index, info, nullptr);
}
