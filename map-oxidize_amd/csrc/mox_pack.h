// Device-side pieces shared by the kernels that pack (word, count) rows of a
// device-resident table into the exchange's receive layout: the accumulator's
// packer (mox_accum.hip) and the re-keying packer (mox_rekey.hip).  The layout:
// a row of 1..16 bytes without a NUL byte is a zero-padded WRec; every other
// row is an XHdr (hash, length, count, offset) plus its bytes, padded with
// zeros to 8, in the blob's word area (reduce_pairs_impl, mox_multi.hip, writes
// it on the host).  Everything is forced inline, as in mox_dev.h: a kernel that
// uses a piece compiles to what it compiled to with the body written out.
//
// What the pieces read past a word.  A "word" here is the byte range
// [o, o + len) the caller packs: a whole word of the table (accumulate) or a
// window of one (re-key), which starts inside its word.  Either way o is no
// later than a word's last byte, so the slack contract (mox_dev.h) covers every
// read below: aligned 8-byte loads from o & ~7 on that end less than 24 bytes
// past o or less than 16 bytes past o + len.  What is read past o + len is
// masked by the length (mask_low) before the NUL test, the hash and every
// store; nothing is written past the padded word.
#pragma once
#include "mox_internal.h"
#include "mox_tiles.h"

namespace mox {

// non-zero exactly when some byte of v is zero
__device__ __forceinline__ uint64_t pk_haszero(uint64_t v) { return (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull; }

// Row classification.  len in 1..16: the key (k0, k1), masked by the length,
// and whether it is NUL-free (bytes past the length are filled with ones for
// the test).  Returns true for a short row (k0, k1 valid); false for every
// other row, a zero-length one included, which loads nothing.
// Reads: three aligned 8-byte loads from o & ~7, up to 23 bytes past o (the
// slack contract's "16 key bytes of a row").
__device__ __forceinline__ bool pk_short(const uint8_t* bytes, uint64_t o, uint64_t len, uint64_t& k0, uint64_t& k1) {
  if (len - 1 >= 16) return false;  // 0 or > 16 bytes
  const uint64_t* q = reinterpret_cast<const uint64_t*>(bytes + (o & ~7ull));
  const uint32_t sh = (uint32_t)(o & 7u) * 8u;
  const uint64_t a = q[0], b = q[1], c = q[2];
  k0 = sh ? (a >> sh) | (b << (64 - sh)) : a;  // (funnel, written out: three loads in flight whatever the length)
  k1 = sh ? (b >> sh) | (c << (64 - sh)) : b;
  k0 = mask_low(k0, len);
  k1 = len > 8 ? mask_low(k1, len - 8) : 0ull;
  const uint64_t f0 = len >= 8 ? 0ull : ~0ull << (8 * len);
  const uint64_t f1 = len >= 16 ? 0ull : (len <= 8 ? ~0ull : ~0ull << (8 * (len - 8)));
  return !(pk_haszero(k0 | f0) | pk_haszero(k1 | f1));
}

// A long row by one lane: dst[0, (len + 7) & ~7) = the word's bytes, zero
// padded, as 8-byte words (dst is 8-byte aligned), the last one masked.
// Returns the XHdr's hash: fnv_finish of the word's FNV-1a-64
// (mox_internal.h: fnv_step, and who has to agree on it).
// Reads: word_at for every 8-byte word of the word, so aligned loads from
// o & ~7 up to less than 16 bytes past o + len (the slack contract's "a word
// as aligned 8-byte words").
__device__ __forceinline__ uint64_t pk_long_lane(const uint8_t* bytes, uint64_t o, uint64_t len, uint8_t* dst) {
  const uint64_t* q = reinterpret_cast<const uint64_t*>(bytes + (o & ~7ull));
  const uint32_t sh = (uint32_t)(o & 7u) * 8u;
  uint64_t* d = reinterpret_cast<uint64_t*>(dst);
  uint64_t h = FNV0;
  for (uint64_t x = 0; 8 * x < len; x++) {
    const uint64_t m = len - 8 * x;
    const uint64_t v = mask_low(word_at(q, sh, x), m);
    d[x] = v;
    const uint32_t nb = m < 8 ? (uint32_t)m : 8u;
    for (uint32_t y = 0; y < nb; y++) h = fnv_step(h, (uint8_t)(v >> (8 * y)));
  }
  return fnv_finish(h);
}

// The same by the 64 lanes of a wave; every lane calls it with the same
// arguments and every lane gets the hash.  A step takes 64 consecutive 8-byte
// words: lane l loads, masks and stores word w0 + l (one coalesced 512-byte
// run each way), then the hash walks the 64 words lane by lane through __shfl.
// FNV-1a is a serial recurrence (h' = (h ^ b) * P), so only the loads and
// stores spread over the lanes; the multiply chain does not.
// Reads: as pk_long_lane (a lane past the last word loads nothing).
__device__ __forceinline__ uint64_t pk_long_wave(const uint8_t* bytes, uint64_t o, uint64_t len, uint8_t* dst) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t* q = reinterpret_cast<const uint64_t*>(bytes + (o & ~7ull));
  const uint32_t sh = (uint32_t)(o & 7u) * 8u;
  uint64_t* d = reinterpret_cast<uint64_t*>(dst);
  const uint64_t nw = (len + 7) / 8;
  uint64_t h = FNV0;
  for (uint64_t w0 = 0; w0 < nw; w0 += 64) {
    const uint64_t wi = w0 + lane;
    uint64_t v = 0;
    if (wi < nw) {
      v = mask_low(word_at(q, sh, wi), len - 8 * wi);
      d[wi] = v;
    }
    const uint32_t m = (uint32_t)(nw - w0 < 64 ? nw - w0 : 64);
    for (uint32_t l = 0; l < m; l++) {  // every lane walks the same chain: the word of lane l
      const uint64_t u = __shfl(v, (int)l);
      const uint64_t left = len - 8 * (w0 + l);
      if (left >= 8) {
#pragma unroll
        for (uint32_t y = 0; y < 8; y++) h = fnv_step(h, (uint8_t)(u >> (8 * y)));
      } else {
        for (uint32_t y = 0; y < (uint32_t)left; y++) h = fnv_step(h, (uint8_t)(u >> (8 * y)));
      }
    }
  }
  return fnv_finish(h);
}

// A place in a tile's output: short rows, long rows and padded long bytes
// before it.  As a running total, what the rounds so far placed (the same on
// every thread); as a row's place, .s is valid for a short row, .l and .b (its
// header's rank, its word's byte offset) for a long one.
struct PkAt {
  uint64_t s, l, b;
};
// One round of a packer of WAVES waves: every thread brings one row (is_s: a
// short row; is_l: a long row, pl = its length padded to 8; neither: no row;
// pl = 0 unless is_l) and gets its place; run advances by the round's totals.
// A row's rank is a ballot rank inside its wave plus the totals of the waves
// before it (LDS), a long word's byte offset a wave scan of the padded lengths:
// rows keep their order and no atomic places a record.  Every thread of the
// workgroup calls it; its first barrier also orders what the caller wrote to
// LDS before the round (the packers' cleared s_nbig) against what follows.
template <int WAVES>
__device__ __forceinline__ PkAt pk_ranks(bool is_s, bool is_l, uint64_t pl, PkAt& run) {
  __shared__ uint64_t s_w[WAVES][3];  // the round's short rows, long rows, long bytes per wave
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t ms = __ballot(is_s), ml = __ballot(is_l);
  const uint64_t below = lane ? ~0ull >> (64 - lane) : 0ull;
  const uint64_t inc = wave_incscan<uint64_t>(pl);
  __syncthreads();  // the previous round's s_w has been read
  if (lane == 63) {
    s_w[wv][0] = (uint64_t)__popcll(ms);
    s_w[wv][1] = (uint64_t)__popcll(ml);
    s_w[wv][2] = inc;
  }
  __syncthreads();
  uint64_t ps = run.s, pq = run.l, pb = run.b;
  for (uint32_t k = 0; k < (uint32_t)WAVES; k++) {
    if (k < wv) {
      ps += s_w[k][0];
      pq += s_w[k][1];
      pb += s_w[k][2];
    }
    run.s += s_w[k][0];
    run.l += s_w[k][1];
    run.b += s_w[k][2];
  }
  return PkAt{ps + __popcll(ms & below), pq + __popcll(ml & below), pb + inc - pl};
}

}  // namespace mox
