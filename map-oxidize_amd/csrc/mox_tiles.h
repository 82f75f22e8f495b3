// What the operators over the device-resident result share of the frame around
// their own per-row logic (mox_filter.hip and the join that runs its passes,
// mox_rekey.hip, mox_accum.hip, mox_rank.hip, mox_hist.hip): the table is cut
// into tiles, a counting pass sums K u64 values per tile (tile_sums), one
// workgroup scans the tile arrays (scan_tiles; mox_dev.h's scan_one_wg for a
// single array), and a placing pass puts every row at its tile's scanned base
// plus the totals of the waves before it plus its place inside its wave.  The
// placing round stays written out in its five kernels (mox_pack.h's pk_ranks,
// k_fl_emit, k_rk_emit, k_hg_bins): as a shared call it measured slower
// (profiles/tiles/README.md).  Everything on the device is forced inline, as in
// mox_dev.h.  Every thread of the workgroup calls a piece, with the same
// template arguments, outside divergent code; each use has LDS slots of its own.
#pragma once
#include "mox_dev.h"

namespace mox {

// A table in generic form (mox_engine::Res, or the accumulator's saved total)
// and nt, the number of its tiles.
struct TileTab {
  const uint64_t* counts;
  const uint64_t* offs;
  const uint8_t* bytes;
  uint64_t n, nt;
};
inline TileTab tile_tab(const uint64_t* counts, const uint64_t* offs, const uint8_t* bytes, uint64_t n, uint32_t tile) {
  return TileTab{counts, offs, bytes, n, (n + tile - 1) / tile};
}
template <class Res>
inline TileTab tile_tab(const Res& r, uint32_t tile) {
  return tile_tab(r.counts, r.offs, r.bytes, r.n, tile);
}

// The end of a counting pass over one tile by WAVES waves: tc[k * stride +
// tile] = the sum of v[k] over the workgroup's threads, k < K (stride: the
// distance between the K tile arrays, at least the number of tiles).  Its
// closing barrier makes the LDS slots the next tile's.
template <int K, int WAVES>
__device__ __forceinline__ void tile_sums(const uint64_t (&v)[K], uint64_t* tc, uint64_t stride, uint64_t tile) {
  __shared__ uint64_t s_w[WAVES][K];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const uint64_t s = wave_sum(v[k]);
    if (lane == 0) s_w[wv][k] = s;
  }
  __syncthreads();
  if (t < (uint32_t)K) {
    uint64_t s = 0;
    for (int w = 0; w < WAVES; w++) s += s_w[w][t];
    tc[(uint64_t)t * stride + tile] = s;
  }
  __syncthreads();
}

// Exclusive scans in place of the K tile arrays tc[k * nt + [0, nt)) by one
// workgroup of THREADS threads with running carries; total[k] = the sum of
// array k.  scan_one_wg widened: a step takes THREADS * PER tiles of all K
// arrays, PER consecutive ones per thread, behind one pair of barriers (one
// array after the other, 1,024 tiles per step, took 440 us for the three arrays
// and 89,159 tiles of a 91 M-word table: 264 dependent steps).  The sum of the
// waves before a thread's own is read off the running sum of all waves (with
// two sums, "if (j < wv) pre += ..." beside "tot += ...", the compiler merges
// the first with the carry once the body is inlined from here, loads all wave
// totals before it adds any, and k_fl_scan spills 28 VGPRs).
template <int K, int PER, int THREADS>
__device__ __forceinline__ void scan_tiles(uint64_t* tc, uint64_t nt, uint64_t* total) {
  __shared__ uint64_t ws[K][THREADS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint64_t carry[K] = {};
  for (uint64_t c = 0; c < nt; c += (uint64_t)THREADS * PER) {
    const uint64_t i0 = c + (uint64_t)PER * threadIdx.x;
    uint64_t sum[K], inc[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      uint64_t s = 0;
#pragma unroll
      for (int j = 0; j < PER; j++)
        if (i0 + j < nt) s += tc[(uint64_t)k * nt + i0 + j];
      sum[k] = s;
      inc[k] = wave_incscan<uint64_t>(s);
      if (lane == 63) ws[k][wv] = inc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
      uint64_t pre = 0, tot = 0;
      for (int j = 0; j < THREADS / 64; j++) {
        if (j == wv) pre = tot;
        tot += ws[k][j];
      }
      // the thread's run again (its own values, not yet overwritten), now as running sums
      uint64_t run = carry[k] + pre + inc[k] - sum[k];
#pragma unroll
      for (int j = 0; j < PER; j++)
        if (i0 + j < nt) {
          uint64_t* a = tc + (uint64_t)k * nt + i0 + j;
          const uint64_t v = *a;
          *a = run;
          run += v;
        }
      carry[k] += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) total[k] = carry[k];
  }
}

}  // namespace mox
