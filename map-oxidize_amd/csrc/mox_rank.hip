// Device ranking (mox_rank_result): the device-resident result reordered by
// count on the GPU, most frequent first (or least frequent first), words with
// equal counts in the order they had ("Ranking the result").
// Nothing is fetched; afterwards every reader of the result sees the ranked
// table.
//
// A stable LSD radix sort of (key, row index) pairs, then one materialising
// pass, written against mox_engine::Res in generic form: any result, whatever
// buffers it lives in and whatever its order.  The key is the count (ascending)
// or its complement (descending).  Rows go in tiles of RK_TILE consecutive rows,
// one workgroup per tile, grid-stride; wave w of a tile takes the tile's rows
// [w * 1024, (w + 1) * 1024) in RK_STEPS steps of 64 consecutive rows, so
// (wave, step, lane) order is row order.  No workgroup waits on another and no
// global atomic decides where a row lands: positions come from scans between
// launches, so no dispatch order or grid cap can hang a call and the output is
// a pure function of the table and the flags.
//
//  1. k_rk_max: the largest count, one value per workgroup (the host takes
//     the maximum of at most 8 per CU).  Only the ceil(bitlen(max) / 8) low
//     digits are sorted: the higher bytes are equal in every key.  A maximum of
//     0: no pass, the identity permutation.
//  2. Per digit, low to high:
//     k_rk_hist: per tile the 256 digit counts, th[digit * nt + tile].  A wave
//       counts in its own LDS row; lanes with the same digit are found by
//       eight ballots and their first lane adds their number, so that 64 equal
//       digits (every high byte of a Zipf table) cost one LDS update.
//     k_rk_scan_part / k_rk_scan_top / k_rk_scan_apply: the exclusive scan of
//       th in digit-major order: chunk sums, their scan by one workgroup, the
//       chunks' own scans on top of it.
//     k_rk_scatter: a row's position is its (digit, tile) base, plus the rows
//       of that digit in the tile's earlier waves, plus those in its wave's
//       earlier steps (the wave's running LDS count), plus those in lower lanes
//       of its step (ballot rank).  Pass 0 reads the counts themselves and
//       takes the row number as the index; every pass writes (u64 key, u32
//       index) to the other of two scratch arrays.
//     Steps 1 and 2 are the host function rank_order (mox_host.h), which takes
//     any u64 key array: the histograms (mox_hist.hip) sort their keys with it.
//  3. k_rk_len: per tile the bytes of its words in the new order; k_rk_offs (one
//     workgroup): their exclusive scan, the total behind them (= the table's
//     bytes, checked by the host).
//  4. k_rk_emit: in rounds of 256 rows, a row's byte offset is its tile's base
//     plus a scan of the lengths (k_rk_len ends in mox_tiles.h's tile_sums);
//     it writes the count, the offset and the
//     word's bytes; offs[n] = nb closes the table.  Words of up to RK_LANE_MAX
//     bytes are copied by their lane; longer ones (a table word reaches 16 MiB)
//     are listed in LDS and copied by whole waves after the round, 64
//     consecutive 8-byte words per step.
//
// Loads and stores: a word is copied as 8-byte words from its first byte on
// (any alignment on either side), then a tail of 4, 2 and 1 bytes (mox_dev.h:
// copy_lane, copy_wave), so nothing is read or written past a word.  Every
// index a kernel derives (a scattered position, a source row, an output byte
// range) is checked against the table before it is used.  The one-workgroup
// scans are mox_dev.h's scan_one_wg: a step is RK_TOP_T tiles = 4.2 M rows, or
// 16 times as many for the chunk sums (22 dependent steps for a 91 M-word table).
//
// Output: two sets of three buffers (mox_engine::r_tab, sized by
// table_reserve); a call writes the set the result does not live in, so a ranked result
// can be ranked again, and e->res is repointed only when everything has
// succeeded.  Scratch (r_tmp) is 24 bytes per row (two key and two index
// arrays) plus 1 KiB per tile.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_rk_max         10 VGPRs, 22 SGPRs,    32 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_rk_hist        32 VGPRs, 60 SGPRs,  4112 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_rk_scan_part   32 VGPRs, 28 SGPRs,    16 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_rk_scan_top    47 VGPRs, 62 SGPRs,    64 B LDS, no scratch, no spills (one workgroup)
//   k_rk_scan_apply  36 VGPRs, 48 SGPRs,    16 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_rk_scatter     56 VGPRs, 43 SGPRs, 12304 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_rk_len         22 VGPRs, 66 SGPRs,    32 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_rk_offs        70 VGPRs, 62 SGPRs,   128 B LDS, no scratch, no spills (one workgroup)
//   k_rk_emit        59 VGPRs, 82 SGPRs,  6184 B LDS, no scratch, no spills (8 waves / SIMD)
#include <algorithm>
#include <cstdlib>

#include "mox_host.h"
#include "mox_tiles.h"

namespace {

constexpr int RK_T = 256;                       // threads of the kernels over rows
constexpr int RK_WAVES = RK_T / 64;
constexpr int RK_STEPS = 16;                    // steps of 64 rows per wave and tile
constexpr uint32_t RK_WROWS = 64 * RK_STEPS;    // a wave's rows of a tile
constexpr uint32_t RK_TILE = RK_T * RK_STEPS;   // rows per tile (tests/rank_cases.py TILE)
constexpr int RK_DIGITS = 256;
// one word of padding per wave row: a digit's RK_WAVES entries lie on different banks
constexpr int RK_HROW = RK_DIGITS + 1;
constexpr uint32_t RK_CHUNK_PER = 16;                     // consecutive (digit, tile) counts per thread ...
constexpr uint32_t RK_CHUNK = RK_T * RK_CHUNK_PER;        // ... and per workgroup step of the scan
constexpr int RK_TOP_T = 1024;                            // threads of the one-workgroup scans (tests/rank_cases.py TOP_STEP)
constexpr uint32_t RK_ROUNDS = RK_TILE / RK_T;            // k_rk_emit: rounds of RK_T rows per tile
constexpr uint32_t RK_LANE_MAX = 64;                      // a longer word is copied by a whole wave
static_assert(RK_TILE == 4096, "tests/rank_cases.py TILE");
static_assert(RK_T == RK_DIGITS, "thread d owns digit d");
static_assert(RK_WROWS <= 65536, "s_rank holds 16-bit ranks");
static_assert((RK_DIGITS % RK_CHUNK_PER) == 0, "a thread's counts lie inside the array or outside it");

// The result in generic form (mox_engine::Res); nt = its tiles.
struct RkTab {
  const uint64_t* counts;
  const uint64_t* offs;
  const uint8_t* bytes;
  uint64_t n, nb, nt;
};
// One radix pass: key i is kin[i] ^ flip, its row iin[i] (pass 0: the counts
// and no index array, the row is i); digit = (key >> shift) & 255.
struct RkPass {
  const uint64_t* kin;
  const uint32_t* iin;
  uint64_t* kout;
  uint32_t* iout;
  uint64_t flip, n, nt;
  uint32_t shift;
};
// The order to materialise: output row r is source row idx[r] with count
// keys[r] ^ flip (no pass ran: both NULL, the order is the source's).
struct RkOrder {
  const uint64_t* keys;
  const uint32_t* idx;
  uint64_t flip;
};
struct RkOut {
  uint64_t* counts;
  uint64_t* offs;
  uint8_t* bytes;
};

// The lanes of the wave whose row is valid and whose digit equals this lane's
// (0 for a lane without a row).  Every lane of the wave calls it.
__device__ __forceinline__ uint64_t rk_peers(uint32_t d, bool valid) {
  uint64_t p = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = (d >> b) & 1u;
    const uint64_t m = __ballot(bit);
    p &= bit ? m : ~m;
  }
  return valid ? p : 0ull;
}

}  // namespace

// bm[workgroup] = the largest count of the workgroup's rows (0 without rows).
extern "C" __global__ __launch_bounds__(RK_T) void k_rk_max(const uint64_t* __restrict__ counts, uint64_t n, uint64_t* __restrict__ bm) {
  __shared__ uint64_t s_m[RK_WAVES];
  uint64_t m = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * RK_T + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RK_T) m = max(m, counts[i]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint64_t)__shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < RK_WAVES; w++) m = max(m, s_m[w]);
    bm[blockIdx.x] = m;
  }
}

// th[d * nt + tile] = rows of the tile whose digit is d.
extern "C" __global__ __launch_bounds__(RK_T) void k_rk_hist(RkPass P, uint32_t* __restrict__ th) {
  __shared__ uint32_t s_h[RK_WAVES][RK_HROW];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (uint64_t tile = blockIdx.x; tile < P.nt; tile += gridDim.x) {
    for (int w = 0; w < RK_WAVES; w++) s_h[w][t] = 0;
    __syncthreads();
    const uint64_t base = tile * RK_TILE + wv * RK_WROWS;
    for (int s = 0; s < RK_STEPS; s++) {
      const uint64_t i = base + (uint32_t)s * 64 + lane;
      const bool valid = i < P.n;
      const uint32_t d = valid ? (uint32_t)(((P.kin[i] ^ P.flip) >> P.shift) & 255u) : 0u;
      const uint64_t peers = rk_peers(d, valid);
      // the first of the lanes that share a digit counts for all of them (a wave's LDS accesses complete in order)
      if (valid && (peers & (0ull - peers)) == (1ull << lane)) s_h[wv][d] += (uint32_t)__popcll(peers);
    }
    __syncthreads();
    uint32_t c = 0;
    for (int w = 0; w < RK_WAVES; w++) c += s_h[w][t];
    th[(uint64_t)t * P.nt + tile] = c;
    __syncthreads();  // the LDS rows are the next tile's
  }
}

// cs[chunk] = the sum of the chunk's RK_CHUNK counts of th[0, m).
extern "C" __global__ __launch_bounds__(RK_T) void k_rk_scan_part(const uint32_t* __restrict__ th, uint64_t m, uint32_t* __restrict__ cs) {
  __shared__ uint32_t s_w[RK_WAVES];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t nc = (m + RK_CHUNK - 1) / RK_CHUNK;
  for (uint64_t c = blockIdx.x; c < nc; c += gridDim.x) {
    const uint64_t i0 = c * RK_CHUNK + (uint64_t)t * RK_CHUNK_PER;
    uint32_t s = 0;
    if (i0 < m) {  // (m is a multiple of RK_CHUNK_PER: the thread's counts all exist)
#pragma unroll
      for (uint32_t j = 0; j < RK_CHUNK_PER; j++) s += th[i0 + j];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) s_w[wv] = s;
    __syncthreads();
    if (t == 0) {
      uint32_t v = 0;
      for (int w = 0; w < RK_WAVES; w++) v += s_w[w];
      cs[c] = v;
    }
    __syncthreads();
  }
}

// Exclusive scan in place of the nc chunk sums; cs[nc] = the total (the rows).
extern "C" __global__ __launch_bounds__(RK_TOP_T) void k_rk_scan_top(uint32_t* cs, uint64_t nc) { scan_one_wg<uint32_t, RK_TOP_T>(cs, nc, cs + nc); }

// Exclusive scan in place of th[0, m): every chunk's own scan on top of its
// scanned sum cs[chunk].
extern "C" __global__ __launch_bounds__(RK_T) void k_rk_scan_apply(uint32_t* __restrict__ th, uint64_t m, const uint32_t* __restrict__ cs) {
  __shared__ uint32_t s_w[RK_WAVES];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t nc = (m + RK_CHUNK - 1) / RK_CHUNK;
  for (uint64_t c = blockIdx.x; c < nc; c += gridDim.x) {
    const uint64_t i0 = c * RK_CHUNK + (uint64_t)t * RK_CHUNK_PER;
    const bool in = i0 < m;
    uint32_t v[RK_CHUNK_PER], s = 0;
#pragma unroll
    for (uint32_t j = 0; j < RK_CHUNK_PER; j++) {
      v[j] = in ? th[i0 + j] : 0u;
      s += v[j];
    }
    const uint32_t inc = wave_incscan<uint32_t>(s);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t run = cs[c] + inc - s;
    for (uint32_t w = 0; w < wv; w++) run += s_w[w];
    if (in) {
#pragma unroll
      for (uint32_t j = 0; j < RK_CHUNK_PER; j++) {
        th[i0 + j] = run;
        run += v[j];
      }
    }
    __syncthreads();
  }
}

// Every (key, row) pair at its position of this digit's stable order (th:
// scanned by k_rk_scan_*).
extern "C" __global__ __launch_bounds__(RK_T) void k_rk_scatter(RkPass P, const uint32_t* __restrict__ th) {
  __shared__ uint32_t s_h[RK_WAVES][RK_HROW];  // a wave's running digit counts, then its digit bases
  __shared__ uint16_t s_rank[RK_TILE];         // a row's rank among its wave's rows of the same digit
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (uint64_t tile = blockIdx.x; tile < P.nt; tile += gridDim.x) {
    for (int w = 0; w < RK_WAVES; w++) s_h[w][t] = 0;
    __syncthreads();
    const uint64_t base = tile * RK_TILE + wv * RK_WROWS;
    for (int s = 0; s < RK_STEPS; s++) {
      const uint64_t i = base + (uint32_t)s * 64 + lane;
      const bool valid = i < P.n;
      const uint32_t d = valid ? (uint32_t)(((P.kin[i] ^ P.flip) >> P.shift) & 255u) : 0u;
      const uint64_t peers = rk_peers(d, valid);
      const uint32_t first = peers ? (uint32_t)__builtin_ctzll(peers) : lane;
      uint32_t before = 0;
      if (valid && first == lane) {  // (a wave's LDS accesses complete in order: the next step sees this one's counts)
        before = s_h[wv][d];
        s_h[wv][d] = before + (uint32_t)__popcll(peers);
      }
      before = __shfl(before, (int)first);
      const uint64_t below = lane ? ~0ull >> (64 - lane) : 0ull;
      s_rank[wv * RK_WROWS + (uint32_t)s * 64 + lane] = (uint16_t)(before + (uint32_t)__popcll(peers & below));
    }
    __syncthreads();
    {  // digit t: the tile's base, then one wave after the other
      uint32_t run = th[(uint64_t)t * P.nt + tile];
      for (int w = 0; w < RK_WAVES; w++) {
        const uint32_t c = s_h[w][t];
        s_h[w][t] = run;
        run += c;
      }
    }
    __syncthreads();
    for (int s = 0; s < RK_STEPS; s++) {
      const uint64_t i = base + (uint32_t)s * 64 + lane;
      if (i < P.n) {
        const uint64_t key = P.kin[i] ^ P.flip;
        const uint32_t d = (uint32_t)((key >> P.shift) & 255u);
        const uint64_t pos = (uint64_t)s_h[wv][d] + s_rank[wv * RK_WROWS + (uint32_t)s * 64 + lane];
        if (pos < P.n) {  // (always, for the counts the scan saw)
          P.kout[pos] = key;
          P.iout[pos] = P.iin ? P.iin[i] : (uint32_t)i;
        }
      }
    }
    __syncthreads();  // the LDS arrays are the next tile's
  }
}

// tb[tile] = the bytes of the words of output rows [tile * RK_TILE, ...).
extern "C" __global__ __launch_bounds__(RK_T) void k_rk_len(RkTab T, RkOrder O, uint64_t* __restrict__ tb) {
  const uint32_t t = threadIdx.x;
  for (uint64_t tile = blockIdx.x; tile < T.nt; tile += gridDim.x) {
    uint64_t nb = 0;
    for (uint32_t j = 0; j < RK_ROUNDS; j++) {
      const uint64_t r = tile * RK_TILE + j * RK_T + t;
      if (r < T.n) {
        const uint64_t src = O.idx ? O.idx[r] : r;
        if (src < T.n) nb += T.offs[src + 1] - T.offs[src];
      }
    }
    tile_sums<1, RK_WAVES>({nb}, tb, 0, tile);
  }
}

// Exclusive scan in place of the nt tile byte sums; tb[nt] = the table's bytes.
extern "C" __global__ __launch_bounds__(RK_TOP_T) void k_rk_offs(uint64_t* tb, uint64_t nt) { scan_one_wg<uint64_t, RK_TOP_T>(tb, nt, tb + nt); }

// The table in the new order (tb: k_rk_offs' output).
extern "C" __global__ __launch_bounds__(RK_T) void k_rk_emit(RkTab T, RkOrder O, const uint64_t* __restrict__ tb, RkOut out) {
  __shared__ uint64_t s_w[RK_WAVES];     // a round's bytes per wave
  __shared__ uint64_t s_big_d[RK_T];     // words over RK_LANE_MAX bytes of a round: byte offset in the output,
  __shared__ uint64_t s_big_s[RK_T];     // ... in the source,
  __shared__ uint64_t s_big_l[RK_T];     // ... length
  __shared__ uint32_t s_nbig;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (blockIdx.x == 0 && t == 0) out.offs[T.n] = T.nb;
  for (uint64_t tile = blockIdx.x; tile < T.nt; tile += gridDim.x) {
    uint64_t rb = tb[tile];  // running output byte offset
    for (uint32_t j = 0; j < RK_ROUNDS; j++) {
      const uint64_t r = tile * RK_TILE + j * RK_T + t;
      bool valid = r < T.n;
      uint64_t src = 0, o = 0, len = 0, cnt = 0;
      if (valid) {
        src = O.idx ? O.idx[r] : r;
        valid = src < T.n;  // (always, for a permutation)
      }
      if (valid) {
        o = T.offs[src];
        len = T.offs[src + 1] - o;
        cnt = O.keys ? (__builtin_nontemporal_load(O.keys + r) ^ O.flip) : T.counts[src];
      }
      const uint64_t inc = wave_incscan<uint64_t>(len);
      __syncthreads();  // the previous round's s_w and long-word list have been read
      if (lane == 63) s_w[wv] = inc;
      if (t == 0) s_nbig = 0;
      __syncthreads();
      uint64_t pb = rb;
      for (uint32_t w = 0; w < (uint32_t)RK_WAVES; w++) {
        if (w < wv) pb += s_w[w];
        rb += s_w[w];
      }
      if (valid) {
        const uint64_t bo = pb + inc - len;
        if (bo + len <= T.nb && o + len <= T.nb) {  // (always, for the lengths the scan saw)
          out.counts[r] = cnt;
          out.offs[r] = bo;
          if (len <= RK_LANE_MAX) {
            copy_lane(out.bytes + bo, T.bytes + o, len);
          } else {  // a whole wave below
            const uint32_t x = atomicAdd(&s_nbig, 1u);
            s_big_d[x] = bo;
            s_big_s[x] = o;
            s_big_l[x] = len;
          }
        }
      }
      __syncthreads();
      // words over RK_LANE_MAX bytes: one wave each
      const uint32_t nbig = s_nbig;
      for (uint32_t x = wv; x < nbig; x += RK_WAVES) {
        copy_wave(out.bytes + s_big_d[x], T.bytes + s_big_s[x], s_big_l[x]);
      }
    }
    __syncthreads();  // the LDS arrays are the next tile's
  }
}

namespace mox_host {

// The stable order of n u64 keys on the device by key ^ flip (steps 1 and 2 of
// the file's header): the ranking's, and the histogram's over its own keys.
// extra: bytes of the caller's own scratch, carved behind the sort's in r_tmp.
int rank_order(mox_engine* e, const uint64_t* d_keys, uint64_t n, uint64_t flip, uint64_t cap, size_t extra, RankOrder* out) {
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  int rc;
  const uint64_t nt = (n + RK_TILE - 1) / RK_TILE;
  const uint32_t grid = (uint32_t)std::min(nt, cap);
  // scratch: [block maxima] [keys A] [keys B] [rows A] [rows B] [digit counts 256 nt] [chunk sums nc + 1] [the caller's extra bytes]
  const uint64_t m = (uint64_t)RK_DIGITS * nt, nc = (m + RK_CHUNK - 1) / RK_CHUNK;
  uint64_t *bm, *keys[2];
  uint32_t *rows[2], *th, *cs;
  if ((rc = carve_dev(e->r_tmp, [&](Carve& c) {
         bm = c.take<uint64_t>(cap);
         for (auto& k : keys) k = c.take<uint64_t>(n);
         for (auto& r : rows) r = c.take<uint32_t>(n);
         th = c.take<uint32_t>(m);
         cs = c.take<uint32_t>(nc + 1);
         out->extra = c.take_bytes(extra);
       })))
    return rc;
  if ((rc = grow_pinned(e->h_rmax, 8 * (8 * (size_t)e->n_cu + 8)))) return rc;
  uint64_t* h_max = (uint64_t*)e->h_rmax.p;

  // 1. the largest key and the digits it has
  hipLaunchKernelGGL(k_rk_max, dim3(grid), dim3(RK_T), 0, st, d_keys, n, bm);
  q.step("k_rk_max");
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_max, bm, 8 * (size_t)grid, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  uint64_t max_key = 0;
  for (uint32_t g = 0; g < grid; g++) max_key = std::max<uint64_t>(max_key, h_max[g]);
  uint32_t passes = 0;
  while (passes < 8 && (max_key >> (8 * passes))) passes++;

  // 2. the radix passes, low digit first
  const uint32_t sgrid = (uint32_t)std::min(nc, cap);
  for (uint32_t k = 0; k < passes; k++) {
    const RkPass P{k ? keys[(k - 1) & 1] : d_keys, k ? rows[(k - 1) & 1] : nullptr, keys[k & 1], rows[k & 1], k ? 0ull : flip, n, nt, 8 * k};
    hipLaunchKernelGGL(k_rk_hist, dim3(grid), dim3(RK_T), 0, st, P, th);
    q.step("k_rk_hist");
    hipLaunchKernelGGL(k_rk_scan_part, dim3(sgrid), dim3(RK_T), 0, st, (const uint32_t*)th, m, cs);
    q.step("k_rk_scan_part");
    hipLaunchKernelGGL(k_rk_scan_top, dim3(1), dim3(RK_TOP_T), 0, st, cs, nc);
    q.step("k_rk_scan_top");
    hipLaunchKernelGGL(k_rk_scan_apply, dim3(sgrid), dim3(RK_T), 0, st, th, m, (const uint32_t*)cs);
    q.step("k_rk_scan_apply");
    hipLaunchKernelGGL(k_rk_scatter, dim3(grid), dim3(RK_T), 0, st, P, (const uint32_t*)th);
    q.step("k_rk_scatter");
    HIPCHK(hipGetLastError());
  }
  out->keys = passes ? keys[(passes - 1) & 1] : nullptr;
  out->rows = passes ? rows[(passes - 1) & 1] : nullptr;
  out->flip = passes ? flip : 0ull;
  out->max_key = max_key;
  out->passes = passes;
  out->d_counted = passes ? cs + nc : nullptr;
  return MOX_OK;
}

}  // namespace mox_host

extern "C" int mox_rank_result(mox_engine* e, uint32_t flags, mox_rank_info* info) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  if (flags & ~MOX_RANK_ASCENDING) return fail(MOX_EINVAL, "rank: unknown flags 0x%x", flags);
  if (int rc = result_begin(e)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const mox_engine::Res r = e->res;
  if (r.n > MOX_RANK_MAX_WORDS)
    return fail(MOX_EINVAL, "rank: %llu words (at most MOX_RANK_MAX_WORDS = 2^32 - 1)", (unsigned long long)r.n);
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  int rc;
  mox_rank_info ri{};
  ri.words = r.n;
  ri.tokens = r.tokens;
  auto finish = [&]() {
    ri.device_bytes = e->r_tmp.cap;
    for (auto& set : e->r_tab)
      for (DevBuf& b : set) ri.device_bytes += b.cap;
    ri.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = ri;
    return MOX_OK;
  };
  const bool fail_hook = test_fail_hook("MOX_TEST_FAIL_RANK");
  const char* hook_msg = "rank: injected failure before the output is written (MOX_TEST_FAIL_RANK)";
  if (r.n <= 1) {  // nothing can move: no launch reads a row but the one count
    if (r.n) HIPCHK(hipMemcpyAsync(&ri.max_count, r.counts, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (fail_hook) return fail(MOX_ENOMEM, "%s", hook_msg);
    e->res.pass = false;
    e->res.exchanged = false;
    e->res.ranked = true;
    return finish();
  }
  const RkTab T{r.counts, r.offs, r.bytes, r.n, r.nb, (r.n + RK_TILE - 1) / RK_TILE};
  const uint64_t cap = grid_cap(e, "MOX_RANK_GRID");
  const uint32_t grid = (uint32_t)std::min(T.nt, cap);
  // 1. and 2. the order (rank_order), with the tile bytes [nt + 1] behind its scratch
  const uint64_t flip = (flags & MOX_RANK_ASCENDING) ? 0ull : ~0ull;
  RankOrder ro;
  if ((rc = rank_order(e, T.counts, T.n, flip, cap, 8 * (T.nt + 1), &ro))) return rc;
  ri.max_count = ro.max_key;
  ri.digit_passes = ro.passes;
  const uint32_t passes = ro.passes;
  uint64_t* tb = (uint64_t*)ro.extra;
  const RkOrder O{ro.keys, ro.rows, ro.flip};

  // 3. the new offsets
  hipLaunchKernelGGL(k_rk_len, dim3(grid), dim3(RK_T), 0, st, T, O, tb);
  q.step("k_rk_len");
  hipLaunchKernelGGL(k_rk_offs, dim3(1), dim3(RK_TOP_T), 0, st, tb, T.nt);
  q.step("k_rk_offs");
  HIPCHK(hipGetLastError());
  uint64_t* h_tot = (uint64_t*)e->h_rmax.p;  // the rows the last pass counted (a u32: the low half of a zeroed word), the bytes of the new order
  h_tot[0] = h_tot[1] = 0;
  if (passes) HIPCHK(hipMemcpyAsync(h_tot, ro.d_counted, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h_tot + 1, tb + T.nt, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if ((passes && h_tot[0] != T.n) || h_tot[1] != T.nb)
    return fail(MOX_EHIP, "rank: inconsistent totals (%llu of %llu rows, %llu of %llu bytes)", (unsigned long long)h_tot[0],
                (unsigned long long)T.n, (unsigned long long)h_tot[1], (unsigned long long)T.nb);
  if (fail_hook) return fail(MOX_ENOMEM, "%s", hook_msg);

  // 4. the table, into the set of output buffers the result does not live in
  DevBuf* dst = table_other_set(e->r_tab, r);
  if ((rc = table_reserve(dst[0], dst[1], dst[2], T.n, T.nb))) return rc;
  const RkOut out{(uint64_t*)dst[0].p, (uint64_t*)dst[1].p, (uint8_t*)dst[2].p};
  hipLaunchKernelGGL(k_rk_emit, dim3(grid), dim3(RK_T), 0, st, T, O, (const uint64_t*)tb, out);
  q.step("k_rk_emit");
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  // the same words and counts in the new order: tokens, n, the bytes and folded are the source's
  mox_engine::Res& res = e->res;
  res_point_at(res, dst, r.n, r.nb, r.tokens);
  res.sorted = false;
  res.ranked = true;
  return finish();
}
