// Device histograms (mox_hist_result): the rows of the device-resident result
// binned by a derived u64 key -- the count, the word's bytes, its characters or
// its first character -- with the rows, the wrapping sum of the counts and the
// lowest row of every bin ("Histograms of the result").  The
// call only reads the table; 4 x bins numbers come back.
//
// Sort plus run-length, written against mox_engine::Res in generic form.  Rows
// go in tiles of HG_TILE consecutive rows (or sorted positions), one workgroup
// per tile, grid-stride, in HG_ROUNDS rounds of HG_T consecutive rows, so
// (round, thread) order is row order.  No workgroup waits on another and no
// global atomic decides where a bin lands or adds a count: positions come
// from scans between launches, so the output is a pure function of the table
// and the spec, whatever the grid.
//
//  1. k_hg_keys (BYTES, CHARS, FIRST; COUNT takes the counts themselves): a u64
//     key per row of the range.  BYTES reads two offsets, FIRST the 4 bytes
//     from the word's start on.  CHARS: the owning lane counts the character
//     starts of a word of up to HG_LANE_MAX bytes, 8 bytes at a time; longer
//     words (a table word reaches 16 MiB) are listed in LDS and counted by
//     whole waves after the round, 64 consecutive 8-byte words per step.
//     Only CHARS has that list: the other two keys run without a barrier.
//  2. rank_order (mox_rank.hip): the ranking's stable LSD radix sort of (key,
//     row) pairs, over the ceil(bitlen(max key) / 8) low digits.  A maximum
//     of 0: no pass, every row is in the one bin of key 0.
//  3. k_hg_count: sorted position p is a head when p == 0 or key[p] != key[p-1].
//     Per tile of positions: the heads, and the wrapping sum of the counts
//     gathered through the row indices.  k_hg_scan (one workgroup): both
//     arrays' exclusive scans; the totals behind them are the bins G and the
//     tokens, which the host reads to size the output.
//  4. k_hg_bins: the same heads again, scanned inside the tile on top of the
//     tile's bases (k_hg_count ends in mox_tiles.h's tile_sums); every head writes at its bin index the key, the absolute
//     row (the sort is stable: the head's row is the bin's lowest), its
//     position and the exclusive count prefix at it; (n, tokens) closes both.
//     k_hg_diff: bin_words and bin_tokens are the differences of neighbouring
//     positions and prefixes -- exact mod 2^64.
//
// Loads: a word is read as 8-byte words from its first byte on, 8 bytes apart
// (any alignment), so up to 7 bytes past its end; FIRST reads the 4 bytes from
// the first byte on, so up to 3 bytes past a 1-byte word: both inside the
// slack contract of mox_dev.h, and masked by the word's length (mask_low)
// before use.  Every index a kernel derives (a source row, a word's byte
// range, a bin index) is checked against the table or the output before it is
// used.
//
// Scratch: 8 bytes per row for a derived key and 16 bytes per tile (hg_tmp),
// 48 bytes per bin (hg_out), and the sort's r_tmp.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_hg_keys    42 VGPRs, 65 SGPRs,  6152 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_hg_count   32 VGPRs, 76 SGPRs,    64 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_hg_scan    80 VGPRs, 66 SGPRs,   128 B LDS, no scratch, no spills (one workgroup)
//   k_hg_bins    52 VGPRs, 82 SGPRs,    64 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_hg_diff    12 VGPRs, 22 SGPRs,     0 B LDS, no scratch, no spills (8 waves / SIMD)
#include <algorithm>
#include <cstdlib>

#include "mox_host.h"
#include "mox_tiles.h"

namespace {

constexpr int HG_T = 256;                        // threads of the kernels over rows
constexpr int HG_WAVES = HG_T / 64;
constexpr int HG_ROUNDS = 16;                    // rounds of HG_T rows per tile
constexpr uint32_t HG_TILE = HG_T * HG_ROUNDS;   // rows per tile (tests/hist_cases.py TILE)
constexpr int HG_TOP_T = 1024;                   // threads of the one-workgroup scan (tests/hist_cases.py TOP_STEP)
constexpr uint32_t HG_LANE_MAX = 64;             // a longer word is counted by a whole wave
static_assert(HG_TILE == 4096, "tests/hist_cases.py TILE");

// The result in generic form (mox_engine::Res) and the range [first, first + n) of its rows.
struct HgTab {
  const uint64_t* offs;
  const uint8_t* bytes;
  uint64_t rows, nb, first, n;
};
// The n rows of the range in key order: position p holds key keys[p] and the
// range's row rows[p] (both NULL: every key is 0, the order is the range's);
// counts = the range's counts, nt = its tiles.
struct HgSorted {
  const uint64_t* keys;
  const uint32_t* rows;
  const uint64_t* counts;
  uint64_t n, nt;
};
// The bins: g of them; pos and pre have g + 1 entries.
struct HgOut {
  uint64_t* keys;
  uint64_t* bin_words;
  uint64_t* bin_tokens;
  uint64_t* first_row;
  uint64_t* pos;
  uint64_t* pre;
  uint64_t g, first;
};

// The character starts among the low min(m, 8) bytes of x (m >= 1): a
// continuation byte has bit 7 set and bit 6 clear.
__device__ __forceinline__ uint32_t hg_starts(uint64_t x, uint64_t m) {
  x = mask_low(x, m);
  const uint64_t cont = x & ~(x << 1) & 0x8080808080808080ull;
  return (uint32_t)(m < 8 ? m : 8) - (uint32_t)__popcll(cont);
}

// MOX_HIST_FIRST of the word of len >= 1 bytes at p.
__device__ __forceinline__ uint64_t hg_first(const uint8_t* p, uint64_t len) {
  const uint32_t w = (uint32_t)mask_low(reinterpret_cast<const U32*>(p)->v, len);
  const uint32_t b0 = w & 255u, b1 = (w >> 8) & 255u, b2 = (w >> 16) & 255u, b3 = w >> 24;
  const bool c1 = len > 1 && (b1 & 0xC0u) == 0x80u;
  const bool c2 = c1 && len > 2 && (b2 & 0xC0u) == 0x80u;
  const bool c3 = c2 && len > 3 && (b3 & 0xC0u) == 0x80u;
  return ((uint64_t)b0 << 32) | (c1 ? (uint64_t)b1 << 24 : 0ull) | (c2 ? (uint64_t)b2 << 16 : 0ull) | (c3 ? (uint64_t)b3 << 8 : 0ull) |
         (uint64_t)(1u + c1 + c2 + c3);
}

__device__ __forceinline__ bool hg_head(const HgSorted& S, uint64_t p) { return p == 0 || (S.keys && S.keys[p] != S.keys[p - 1]); }

}  // namespace

// keys[i] = the key (mode: MOX_HIST_BYTES, _CHARS or _FIRST) of row T.first + i, i < T.n.
extern "C" __global__ __launch_bounds__(HG_T) void k_hg_keys(HgTab T, uint32_t mode, uint64_t* __restrict__ keys) {
  __shared__ uint64_t s_big_i[HG_T];  // words over HG_LANE_MAX bytes of a round: the row of the range,
  __shared__ uint64_t s_big_o[HG_T];  // ... byte offset,
  __shared__ uint64_t s_big_l[HG_T];  // ... length
  __shared__ uint32_t s_nbig;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t nt = (T.n + HG_TILE - 1) / HG_TILE;
  const bool chars = mode == MOX_HIST_CHARS;  // the only key with a long-word list: the others take no barrier
  for (uint64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    for (uint32_t j = 0; j < (uint32_t)HG_ROUNDS; j++) {
      const uint64_t i0 = tile * HG_TILE + j * HG_T;
      if (i0 >= T.n) break;  // (the whole workgroup)
      const uint64_t i = i0 + t;
      if (chars) {
        __syncthreads();  // the previous round's long-word list has been read
        if (t == 0) s_nbig = 0;
        __syncthreads();
      }
      if (i < T.n && T.first + i < T.rows) {
        const uint64_t o = T.offs[T.first + i], end = T.offs[T.first + i + 1];
        uint64_t key = 0;
        bool mine = true;
        if (o < end && end <= T.nb) {  // (always but for an empty word: its key is 0)
          const uint64_t len = end - o;
          if (mode == MOX_HIST_BYTES) {
            key = len;
          } else if (mode == MOX_HIST_FIRST) {
            key = hg_first(T.bytes + o, len);
          } else if (len <= HG_LANE_MAX) {
            for (uint64_t x = 0; x < len; x += 8) key += hg_starts(reinterpret_cast<const U64*>(T.bytes + o + x)->v, len - x);
          } else {  // a whole wave below
            const uint32_t x = atomicAdd(&s_nbig, 1u);
            s_big_i[x] = i;
            s_big_o[x] = o;
            s_big_l[x] = len;
            mine = false;
          }
        }
        if (mine) keys[i] = key;
      }
      if (!chars) continue;
      __syncthreads();
      // words over HG_LANE_MAX bytes: one wave each
      const uint32_t nbig = s_nbig;
      for (uint32_t x = wv; x < nbig; x += HG_WAVES) {
        const uint8_t* p = T.bytes + s_big_o[x];
        const uint64_t len = s_big_l[x], nw = (len + 7) / 8;
        uint64_t c = 0;
        for (uint64_t wi = lane; wi < nw; wi += 64) c += hg_starts(reinterpret_cast<const U64*>(p + 8 * wi)->v, len - 8 * wi);
        c = wave_sum(c);
        if (lane == 0) keys[s_big_i[x]] = c;
      }
    }
    if (chars) __syncthreads();  // the LDS arrays are the next tile's
  }
}

// tc[tile] = the heads among sorted positions [tile * HG_TILE, ...), tc[stride + tile] = the wrapping sum of their
// rows' counts (the host's th and tt: two arrays of nt + 1 in one block, stride = nt + 1).
extern "C" __global__ __launch_bounds__(HG_T) void k_hg_count(HgSorted S, uint64_t* __restrict__ tc, uint64_t stride) {
  const uint32_t t = threadIdx.x;
  for (uint64_t tile = blockIdx.x; tile < S.nt; tile += gridDim.x) {
    uint64_t h = 0, c = 0;
    for (uint32_t j = 0; j < (uint32_t)HG_ROUNDS; j++) {
      const uint64_t p = tile * HG_TILE + j * HG_T + t;
      if (p < S.n) {
        h += hg_head(S, p) ? 1u : 0u;
        const uint64_t row = S.rows ? S.rows[p] : p;
        if (row < S.n) c += S.counts[row];  // (always, for a permutation)
      }
    }
    tile_sums<2, HG_WAVES>({h, c}, tc, stride, tile);
  }
}

// Exclusive scans in place of the nt tile heads and tile sums; th[nt] = the bins, tt[nt] = the tokens.
extern "C" __global__ __launch_bounds__(HG_TOP_T) void k_hg_scan(uint64_t* th, uint64_t* tt, uint64_t nt) {
  scan_one_wg<uint64_t, HG_TOP_T>(th, nt, th + nt);
  __syncthreads();
  scan_one_wg<uint64_t, HG_TOP_T>(tt, nt, tt + nt);
}

// Every head at its bin index: the key, the absolute row, the position and the
// exclusive count prefix (th, tt: k_hg_scan's output); (n, tokens) behind them.
extern "C" __global__ __launch_bounds__(HG_T) void k_hg_bins(HgSorted S, const uint64_t* __restrict__ th, const uint64_t* __restrict__ tt, HgOut O) {
  __shared__ uint64_t s_h[HG_WAVES], s_c[HG_WAVES];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (blockIdx.x == 0 && t == 0) {
    O.pos[O.g] = S.n;
    O.pre[O.g] = tt[S.nt];
  }
  for (uint64_t tile = blockIdx.x; tile < S.nt; tile += gridDim.x) {
    uint64_t hb = th[tile], cb = tt[tile];  // the running bin index and count prefix
    for (uint32_t j = 0; j < (uint32_t)HG_ROUNDS; j++) {
      const uint64_t p = tile * HG_TILE + j * HG_T + t;
      uint64_t key = 0, row = 0, cnt = 0;
      bool head = false;
      if (p < S.n) {
        key = S.keys ? S.keys[p] : 0ull;
        head = hg_head(S, p);
        row = S.rows ? S.rows[p] : p;
        if (row < S.n) cnt = S.counts[row];
      }
      const uint64_t hi = wave_incscan<uint64_t>(head ? 1u : 0u), ci = wave_incscan<uint64_t>(cnt);
      __syncthreads();  // the previous round's sums have been read
      if (lane == 63) {
        s_h[wv] = hi;
        s_c[wv] = ci;
      }
      __syncthreads();
      uint64_t ph = hb, pc = cb;
      for (uint32_t w = 0; w < (uint32_t)HG_WAVES; w++) {
        if (w < wv) {
          ph += s_h[w];
          pc += s_c[w];
        }
        hb += s_h[w];
        cb += s_c[w];
      }
      if (head) {
        const uint64_t b = ph + hi - 1;
        if (b < O.g) {  // (always, for the heads the scan saw)
          O.keys[b] = key;
          O.first_row[b] = O.first + row;
          O.pos[b] = p;
          O.pre[b] = pc + ci - cnt;
        }
      }
    }
    __syncthreads();  // the LDS arrays are the next tile's
  }
}

// bin_words and bin_tokens: the differences of neighbouring positions and prefixes.
extern "C" __global__ __launch_bounds__(HG_T) void k_hg_diff(HgOut O) {
  for (uint64_t b = (uint64_t)blockIdx.x * HG_T + threadIdx.x; b < O.g; b += (uint64_t)gridDim.x * HG_T) {
    O.bin_words[b] = O.pos[b + 1] - O.pos[b];
    O.bin_tokens[b] = O.pre[b + 1] - O.pre[b];
  }
}

namespace {

// The table and its four arrays of n in one host block.
mox_hist_table* hist_table_new(uint64_t n) {
  const size_t head = (sizeof(mox_hist_table) + 15) & ~(size_t)15;
  uint8_t* p = (uint8_t*)malloc(head + 32 * (size_t)n + 8);
  if (!p) return nullptr;
  mox_hist_table* t = (mox_hist_table*)p;
  uint64_t* a = (uint64_t*)(p + head);
  t->n = n;
  t->words = t->tokens = 0;
  t->keys = a;
  t->bin_words = a + n;
  t->bin_tokens = a + 2 * n;
  t->first_row = a + 3 * n;
  return t;
}

}  // namespace

extern "C" void mox_hist_free(mox_hist_table* t) { free(t); }

extern "C" int mox_hist_result(mox_engine* e, const mox_hist* h, mox_hist_table** out, mox_hist_info* info) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  if (!h || !out) return fail(MOX_EINVAL, "hist: NULL argument");
  if (h->key > MOX_HIST_FIRST) return fail(MOX_EINVAL, "hist: unknown key %u", h->key);
  if (h->flags & ~MOX_HIST_RANGE) return fail(MOX_EINVAL, "hist: unknown flags 0x%x", h->flags);
  for (uint64_t w : h->reserved)
    if (w) return fail(MOX_EINVAL, "hist: a reserved word is not 0");
  const bool ranged = (h->flags & MOX_HIST_RANGE) != 0;
  if (!ranged && (h->first || h->rows)) return fail(MOX_EINVAL, "hist: first / rows given without MOX_HIST_RANGE");
  if (int rc = result_begin(e)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const mox_engine::Res& r = e->res;
  const uint64_t first = ranged ? std::min(h->first, r.n) : 0;
  const uint64_t n = ranged ? std::min(h->rows, r.n - first) : r.n;
  if (n > MOX_HIST_MAX_WORDS)
    return fail(MOX_EINVAL, "hist: %llu rows (at most MOX_HIST_MAX_WORDS = 2^32 - 1)", (unsigned long long)n);
  mox_hist_info hi{};
  hi.words = n;
  auto finish = [&](mox_hist_table* t) {
    hi.device_bytes = e->hg_tmp.cap + e->hg_out.cap + e->r_tmp.cap;
    hi.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = hi;
    *out = t;
    return MOX_OK;
  };
  if (!n) {  // nothing runs on the device
    mox_hist_table* t = hist_table_new(0);
    if (!t) return fail(MOX_ENOMEM, "hist: host memory");
    return finish(t);
  }
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  int rc;
  const uint64_t cap = grid_cap(e, "MOX_HIST_GRID");
  const uint64_t nt = (n + HG_TILE - 1) / HG_TILE;
  const uint32_t grid = (uint32_t)std::min(nt, cap);
  const bool fail_hook = test_fail_hook("MOX_TEST_FAIL_HIST");
  // scratch: [derived keys n] [tile heads nt + 1 | tile sums nt + 1] (one block: k_hg_count takes its base and the stride nt + 1)
  uint64_t *d_keys, *th, *tt;
  if ((rc = carve_dev(e->hg_tmp, [&](Carve& c) {
         d_keys = c.take<uint64_t>(h->key == MOX_HIST_COUNT ? 0 : n);
         th = c.take<uint64_t>(2 * (nt + 1));
         tt = th + nt + 1;
       })))
    return rc;
  if ((rc = grow_pinned(e->hg_pin, 64))) return rc;

  // 1. the keys
  const uint64_t* keys_in = r.counts + first;
  if (h->key != MOX_HIST_COUNT) {
    const HgTab T{r.offs, r.bytes, r.n, r.nb, first, n};
    hipLaunchKernelGGL(k_hg_keys, dim3(grid), dim3(HG_T), 0, st, T, h->key, d_keys);
    q.step("k_hg_keys");
    HIPCHK(hipGetLastError());
    keys_in = d_keys;
  }

  // 2. their stable order
  RankOrder ro;
  if ((rc = rank_order(e, keys_in, n, 0, cap, 0, &ro))) return rc;
  hi.max_key = ro.max_key;
  hi.digit_passes = ro.passes;

  // 3. the heads and the sums per tile, the bins and the tokens
  const HgSorted S{ro.keys, ro.rows, r.counts + first, n, nt};
  hipLaunchKernelGGL(k_hg_count, dim3(grid), dim3(HG_T), 0, st, S, th, nt + 1);
  q.step("k_hg_count");
  hipLaunchKernelGGL(k_hg_scan, dim3(1), dim3(HG_TOP_T), 0, st, th, tt, nt);
  q.step("k_hg_scan");
  HIPCHK(hipGetLastError());
  uint64_t* h_tot = (uint64_t*)e->hg_pin.p;  // the rows the last pass counted (a u32: the low half of a zeroed word), the bins, the tokens
  h_tot[0] = h_tot[1] = h_tot[2] = 0;
  if (ro.d_counted) HIPCHK(hipMemcpyAsync(h_tot, ro.d_counted, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h_tot + 1, th + nt, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h_tot + 2, tt + nt, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t g = h_tot[1], tokens = h_tot[2];
  if ((ro.d_counted && h_tot[0] != n) || g < 1 || g > n || (!ro.passes && g != 1) || (!ranged && tokens != r.tokens))
    return fail(MOX_EHIP, "hist: inconsistent totals (%llu of %llu rows, %llu bins, %llu of %llu tokens)", (unsigned long long)h_tot[0],
                (unsigned long long)n, (unsigned long long)g, (unsigned long long)tokens, (unsigned long long)r.tokens);
  if (fail_hook) return fail(MOX_ENOMEM, "hist: injected failure before the bins are written (MOX_TEST_FAIL_HIST)");

  // 4. the bins: [keys g] [bin_words g] [bin_tokens g] [first_row g] (what comes back) [positions g + 1] [prefixes g + 1]
  uint64_t *o, *d_pos, *d_pre;
  if ((rc = carve_dev(e->hg_out, [&](Carve& c) {
         o = c.take<uint64_t>(4 * g);
         d_pos = c.take<uint64_t>(g + 1);
         d_pre = c.take<uint64_t>(g + 1);
       })))
    return rc;
  const HgOut O{o, o + g, o + 2 * g, o + 3 * g, d_pos, d_pre, g, first};
  mox_hist_table* t = hist_table_new(g);
  if (!t) return fail(MOX_ENOMEM, "hist: host memory for %llu bins", (unsigned long long)g);
  auto drop = [&](int code) {
    free(t);
    return code;
  };
  hipLaunchKernelGGL(k_hg_bins, dim3(grid), dim3(HG_T), 0, st, S, (const uint64_t*)th, (const uint64_t*)tt, O);
  q.step("k_hg_bins");
  hipLaunchKernelGGL(k_hg_diff, dim3((uint32_t)std::min<uint64_t>((g + HG_T - 1) / HG_T, cap)), dim3(HG_T), 0, st, O);
  q.step("k_hg_diff");
  hipError_t he = hipGetLastError();
  if (he == hipSuccess) he = hipMemcpyAsync((void*)t->keys, o, 32 * g, hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) return drop(fail(MOX_EHIP, "hist: %s", hipGetErrorString(he)));
  // the identities of the contract, in O(bins)
  uint64_t sw = 0, stok = 0;
  bool bad = false;
  for (uint64_t b = 0; b < g && !bad; b++) {
    sw += t->bin_words[b];
    stok += t->bin_tokens[b];
    bad = !t->bin_words[b] || t->bin_words[b] > n || t->first_row[b] < first || t->first_row[b] - first >= n ||
          (b && t->keys[b] <= t->keys[b - 1]) || (h->key == MOX_HIST_COUNT && t->bin_tokens[b] != t->keys[b] * t->bin_words[b]);
  }
  if (bad || sw != n || stok != tokens || t->keys[g - 1] != ro.max_key)
    return drop(fail(MOX_EHIP, "hist: inconsistent totals (%llu of %llu rows and %llu of %llu tokens in %llu bins)", (unsigned long long)sw,
                     (unsigned long long)n, (unsigned long long)stok, (unsigned long long)tokens, (unsigned long long)g));
  t->words = n;
  t->tokens = tokens;
  hi.tokens = tokens;
  hi.bins = g;
  return finish(t);
}
