// The word hash and the exact word compare of the hash sets over table words:
// the device lookup (mox_lookup.hip: a set of the uploaded queries) and the
// device join (mox_join.hip: a set of the result's rows).  Everything is forced
// inline, as in mox_dev.h: a kernel that uses a helper compiles to what it
// compiled to with the helper's body written out.
//
// The hash is made for words of any length taken by one lane or by a whole
// wave: a sum over the word's 8-byte little-endian words (the last one masked
// by the length) of a bijection of (word ^ position key), plus a multiple of
// the length, then a 64-bit avalanche and fnv_finish (the forced-collision
// build truncates it there).  A sum has no serial chain, so a wave hashes a
// long word 64 words at a time and the lane path gives the same value.  The
// length is part of the hash and of every compare: "ab" and "ab\0" are
// different words.
//
// Loads: a word at byte offset o is read as aligned 8-byte words from o & ~7
// and a funnel shift, up to 15 bytes past its end: inside the slack of every
// bytes buffer a result can live in (mox_dev.h: the slack contract).  What is
// read past a word is masked before it is used.  A zero-length word loads
// nothing.
#pragma once
#include "mox_dev.h"
#include "mox_internal.h"

namespace mox {

constexpr uint64_t LK_POS = 0xD6E8FEB86659FD93ull;  // position key of 8-byte word i: (i + 1) LK_POS
constexpr uint64_t LK_MUL = 0xFF51AFD7ED558CCDull;
constexpr uint64_t LK_MUL2 = 0xC4CEB9FE1A85EC53ull;
constexpr uint64_t LK_LEN = 0x9E3779B97F4A7C15ull;

// one 8-byte word's share of the hash: a bijection of the word for each position
__device__ __forceinline__ uint64_t lk_term(uint64_t v, uint64_t poskey) {
  const uint64_t x = (v ^ poskey) * LK_MUL;
  return x ^ (x >> 32);
}
__device__ __forceinline__ uint64_t lk_finish(uint64_t acc, uint64_t len) {
  uint64_t h = acc + len * LK_LEN;
  h ^= h >> 33;
  h *= LK_MUL;
  h ^= h >> 33;
  h *= LK_MUL2;
  h ^= h >> 33;
  return mox::fnv_finish(h);
}

// The hash of bytes[o, o + len), by one lane / by the 64 lanes of a wave
// (WAVE: every lane of the wave calls with the same arguments).
template <bool WAVE>
__device__ __forceinline__ uint64_t lk_hash(const uint8_t* bytes, uint64_t o, uint64_t len) {
  const uint64_t* q = reinterpret_cast<const uint64_t*>(bytes + (o & ~7ull));
  const uint32_t sh = (uint32_t)(o & 7u) * 8u;
  uint64_t acc = 0;
  if (WAVE) {
    const uint64_t nw = (len + 7) / 8;
    for (uint64_t wi = threadIdx.x & 63; wi < nw; wi += 64)
      acc += lk_term(mask_low(funnel(q[wi], q[wi + 1], sh), len - 8 * wi), (wi + 1) * LK_POS);
    acc = wave_sum(acc);
  } else if (len) {
    uint64_t a = q[0], pk = LK_POS;
    for (uint64_t x = 0; 8 * x < len; x++, pk += LK_POS) {
      const uint64_t b = q[x + 1];
      acc += lk_term(mask_low(funnel(a, b, sh), len - 8 * x), pk);
      a = b;
    }
  }
  return lk_finish(acc, len);
}

// A[oa, oa + len) == B[ob, ob + len)
template <bool WAVE>
__device__ __forceinline__ bool lk_equal(const uint8_t* A, uint64_t oa, const uint8_t* B, uint64_t ob, uint64_t len) {
  const uint64_t* qa = reinterpret_cast<const uint64_t*>(A + (oa & ~7ull));
  const uint64_t* qb = reinterpret_cast<const uint64_t*>(B + (ob & ~7ull));
  const uint32_t sa = (uint32_t)(oa & 7u) * 8u, sb = (uint32_t)(ob & 7u) * 8u;
  if (WAVE) {
    const uint64_t nw = (len + 7) / 8;
    for (uint64_t w0 = 0; w0 < nw; w0 += 64) {
      const uint64_t wi = w0 + (threadIdx.x & 63);
      bool ne = false;
      if (wi < nw) ne = mask_low(funnel(qa[wi], qa[wi + 1], sa) ^ funnel(qb[wi], qb[wi + 1], sb), len - 8 * wi) != 0;
      if (__ballot(ne)) return false;
    }
    return true;
  }
  if (!len) return true;
  uint64_t a0 = qa[0], b0 = qb[0];
  for (uint64_t x = 0; 8 * x < len; x++) {
    const uint64_t a1 = qa[x + 1], b1 = qb[x + 1];
    if (mask_low(funnel(a0, a1, sa) ^ funnel(b0, b1, sb), len - 8 * x)) return false;
    a0 = a1;
    b0 = b1;
  }
  return true;
}

}  // namespace mox
