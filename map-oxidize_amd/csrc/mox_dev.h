// Device-side helpers shared by the kernels over the device-resident result
// table (counts, offs, bytes): mox_bsort.hip, mox_topk.hip, mox_text.hip,
// mox_accum.hip, mox_lookup.hip, mox_filter.hip, mox_rank.hip, mox_rekey.hip,
// mox_find.hip, mox_join.hip, mox_hist.hip; mox_tiles.h builds on them the tile passes that filter,
// re-key, accumulate, rank and histogram share (the table view, tile sums, the scan of the tile
// arrays), mox_pack.h the pieces of the two receive-layout packers, mox_wordhash.h the word hash and compare of the lookup and the join,
// mox_wordset.h the set, the build and the stream that those two share.
// Everything is forced inline: a kernel that uses a helper compiles to what it compiled to
// with the helper's body written out.
//
// The slack contract.  Every bytes buffer a result can live in carries
// TABLE_SLACK (mox_host.h: 64) bytes past the table's nb bytes: t_bytes
// (realloc_sized), the gather, sort, accumulator, filter and rank outputs
// (table_reserve, mox_result.hip).  A word starts at an offset o <= nb, so a kernel may read
// past a word without a clamp as long as the read starts no later than the
// word's first byte and ends less than TABLE_SLACK bytes past o.  The readers
// that do: the 16 key bytes of a row as three aligned 8-byte loads from o & ~7
// (mox_pack.h's pk_short: up to 23 bytes past o for the accumulate packer; the
// re-keying packer the same from a window's start, which lies inside the
// word), a word as aligned 8-byte words from o & ~7 on (mox_pack.h's
// pk_long_lane / pk_long_wave and the lookup's long words: up to 15 bytes past
// the word's end), the 16 bytes from o on in one load (the lookup's
// short path, the filter's prefix: up to 15 bytes past a 1-byte word) and the
// sort's window (two aligned loads), and the histogram's keys (8-byte loads from
// o on, 8 bytes apart: up to 7 bytes past the word's end; the 4 bytes from o on: up
// to 3 bytes past a 1-byte word).  Whatever is read past a word is masked by
// the word's length (mask_low) before it is used, and nothing is ever written
// past a word: copy_lane and copy_wave touch [0, len) on both sides only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mox {

// loads and stores of any alignment
struct __attribute__((packed, aligned(1))) U64 {
  uint64_t v;
};
struct __attribute__((packed, aligned(1))) U32 {
  uint32_t v;
};
struct __attribute__((packed, aligned(1))) U16 {
  uint16_t v;
};
// the 16 bytes from any byte address on, in one load
struct __attribute__((packed, aligned(1))) Key16 {
  uint64_t lo, hi;
};

// sum over the wave's 64 lanes, on every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
// inclusive scan over the wave's 64 lanes
template <typename T>
__device__ __forceinline__ T wave_incscan(T x) {
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  return x;
}

// Exclusive scan in place of a[0, m) by one workgroup of THREADS threads, one
// value per thread and step, with a running carry; *total = the sum.  Every
// thread of the workgroup calls it with the same arguments.
template <typename T, int THREADS>
__device__ __forceinline__ void scan_one_wg(T* a, uint64_t m, T* total) {
  __shared__ T ws[THREADS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T carry = 0;
  for (uint64_t c = 0; c < m; c += THREADS) {
    const uint64_t i = c + threadIdx.x;
    const T v = i < m ? a[i] : (T)0;
    const T inc = wave_incscan<T>(v);
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    T pre = 0, tot = 0;
    for (int j = 0; j < THREADS / 64; j++) {
      if (j < wv) pre += ws[j];
      tot += ws[j];
    }
    if (i < m) a[i] = carry + pre + inc - v;
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

// d[0, len) = s[0, len), by one lane: 8-byte words from the first byte on (any
// alignment on either side), then a tail of 4, 2 and 1 bytes
__device__ __forceinline__ void copy_lane(uint8_t* d, const uint8_t* s, uint64_t len) {
  uint64_t x = 0;
  for (; x + 8 <= len; x += 8) reinterpret_cast<U64*>(d + x)->v = reinterpret_cast<const U64*>(s + x)->v;
  if (len & 4) {
    reinterpret_cast<U32*>(d + x)->v = reinterpret_cast<const U32*>(s + x)->v;
    x += 4;
  }
  if (len & 2) {
    reinterpret_cast<U16*>(d + x)->v = reinterpret_cast<const U16*>(s + x)->v;
    x += 2;
  }
  if (len & 1) d[x] = s[x];
}
// The same by the 64 lanes of a wave (every lane calls with the same
// arguments): 64 consecutive 8-byte words per step, then the tail bytes.
__device__ __forceinline__ void copy_wave(uint8_t* d, const uint8_t* s, uint64_t len) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = len / 8;
  for (uint64_t wi = lane; wi < nw; wi += 64) reinterpret_cast<U64*>(d + 8 * wi)->v = reinterpret_cast<const U64*>(s + 8 * wi)->v;
  if (lane < (len & 7)) d[8 * nw + lane] = s[8 * nw + lane];
}

// the low n bytes of a little-endian 8-byte word (n >= 8: all of it)
__device__ __forceinline__ uint64_t mask_low(uint64_t x, uint64_t n) { return n >= 8 ? x : x & ((1ull << (8 * n)) - 1ull); }
// The 8 bytes that start sh / 8 bytes into the aligned word a and go on in the
// next one, b (sh = 0, 8, ..., 56).
__device__ __forceinline__ uint64_t funnel(uint64_t a, uint64_t b, uint32_t sh) { return sh ? (a >> sh) | (b << (64 - sh)) : a; }
// 8-byte word i of the bytes from offset o on: q = the aligned word that holds
// o, sh = 8 (o & 7).  Reads q[i] and q[i + 1]: funnel(q[i], q[i + 1], sh),
// written out (through the nested call the accumulate packer compiles to
// different code).
__device__ __forceinline__ uint64_t word_at(const uint64_t* q, uint32_t sh, uint64_t i) {
  const uint64_t a = q[i], b = q[i + 1];
  return sh ? (a >> sh) | (b << (64 - sh)) : a;
}

}  // namespace mox
