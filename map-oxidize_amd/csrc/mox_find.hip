// Device search of the sorted result (mox_find_ranges): row ranges of given
// keys in the bytewise-sorted device-resident table by binary search, O(q log n)
// loads instead of a pass over the words ("Searching the sorted
// result").  Only the keys go up; first, last (and the sum of the counts in
// between) come back per key.  The result is only read.
//
//  1. k_fd_search: one lane per key.  A lower-bound search over offs / bytes:
//     a step loads offs[mid] and offs[mid + 1], then the word's bytes, and
//     compares word and key 8 bytes at a time as byte-swapped (big-endian)
//     unsigned 64-bit integers masked to the shorter length, then the lengths:
//     Rust String Ord, bytes unsigned, a proper prefix first.  The loop over a
//     word's 8-byte pieces ends at the first difference; keys of any length take
//     this one path.  The serial case: a long key against a table whose words
//     share its long prefix costs O(len / 8) loads per step on that one lane
//     (300-byte words that differ in their last byte: 38 pieces per step).
//     EXACT then compares the row at the lower bound once more for equality;
//     PREFIX runs a second search from the lower bound on in which "the word's
//     first len(key) bytes equal the key" counts as inside; LOWER stops at
//     the bound.  Every loop is bounded by ceil(log2(n + 1)) + 1 steps; an
//     exhausted bound, or first > last, sets FdCtl::err, which the host turns
//     into MOX_EHIP.  The kernel also raises FdCtl::big when a range holds a
//     whole tile of FD_TILE rows aligned at a multiple of FD_TILE.
//  2. k_fd_tiles, k_fd_scan (only launched when sums are asked for; both return
//     on their first load when big is 0): the sums of the counts per tile, then
//     their exclusive scan by one workgroup (mox_dev.h: scan_one_wg), S[ntiles]
//     the total.  One streaming pass over 8 n bytes of counts; word bytes are
//     never read.
//  3. k_fd_sum (only launched when sums are asked for): one wave per key.  A
//     range that holds whole aligned tiles ft..lt takes them as S[lt] - S[ft]
//     (wrapping arithmetic makes the difference exact) and sums its partial
//     head and tail, at most 2 x (FD_TILE - 1) rows, directly, 64 lanes loading
//     consecutive counts; any other range is summed directly.  No atomic
//     touches a count and no order decides a sum: the outputs are a pure
//     function of the table and the keys.
//
// Loads: a word at byte offset o is read as aligned 8-byte words from o & ~7
// and a funnel shift (mox_dev.h), up to 15 bytes past the compared length:
// inside the slack of every bytes buffer a result can live in, which the key
// buffer here carries too.  What is read past the compared length is masked
// before it is used; a compare of zero bytes loads nothing.
//
// Scratch (mox_engine::fd_tmp, fd_pin) is O(q + key bytes + n / FD_TILE): the
// output block, the key offsets and bytes, the scanned tile sums.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_fd_search  56 VGPRs, 76 SGPRs,   0 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_fd_tiles   22 VGPRs, 34 SGPRs,  32 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_fd_scan    70 VGPRs, 62 SGPRs, 128 B LDS, no scratch, no spills (one workgroup)
//   k_fd_sum     26 VGPRs, 38 SGPRs,   0 B LDS, no scratch, no spills (8 waves / SIMD)
#include <algorithm>
#include <cstdlib>

#include "mox_dev.h"
#include "mox_host.h"

namespace {

constexpr int FD_T = 256;                 // threads of the kernels over keys and tiles
constexpr int FD_WAVES = FD_T / 64;
constexpr uint64_t FD_TILE = 1024;        // rows per tile of the count sums (tests/find_cases.py TILE)
constexpr int FD_PER = (int)(FD_TILE / FD_T);
constexpr int FD_SCAN_T = 1024;           // threads of the one-workgroup scan
static_assert(FD_TILE % FD_T == 0, "a tile is FD_PER rounds of the workgroup");

struct FdCtl {
  unsigned long long err;  // 1: a search's step bound exhausted, 2: first > last or last > n
  unsigned long long big;  // 1: some range holds a whole aligned tile
  unsigned long long pad[6];
};
static_assert(sizeof(FdCtl) == 64, "copied with the ranges");

// The result in generic form (mox_engine::Res); steps = the bound of a search loop.
struct FdTab {
  const uint64_t* counts;
  const uint64_t* offs;
  const uint8_t* bytes;
  uint64_t n;
  uint32_t steps;
};
// The uploaded keys and the outputs.
struct FdKeys {
  const uint64_t* koffs;
  const uint8_t* kbytes;
  uint64_t nq;
  uint32_t mode;
  uint64_t* first;
  uint64_t* last;
  uint64_t* sums;
  FdCtl* ctl;
};

// The first min(wlen, klen) bytes of the word at T.bytes + o against those of
// the key at K.kbytes + ko: < 0, 0, > 0 as the word's are smaller, equal, larger.
__device__ __forceinline__ int fd_cmp_common(const uint8_t* wb, uint64_t o, uint64_t wlen, const uint8_t* kb, uint64_t ko, uint64_t klen) {
  const uint64_t m = wlen < klen ? wlen : klen;
  if (!m) return 0;
  const uint64_t* qw = reinterpret_cast<const uint64_t*>(wb + (o & ~7ull));
  const uint64_t* qk = reinterpret_cast<const uint64_t*>(kb + (ko & ~7ull));
  const uint32_t sw = (uint32_t)(o & 7u) * 8u, sk = (uint32_t)(ko & 7u) * 8u;
  uint64_t w0 = qw[0], k0 = qk[0];
  for (uint64_t x = 0; 8 * x < m; x++) {
    const uint64_t w1 = qw[x + 1], k1 = qk[x + 1];
    // byte 0 of the piece is the most significant after the swap; the masked bytes are zero on both sides
    const uint64_t a = __builtin_bswap64(mask_low(funnel(w0, w1, sw), m - 8 * x));
    const uint64_t b = __builtin_bswap64(mask_low(funnel(k0, k1, sk), m - 8 * x));
    if (a != b) return a < b ? -1 : 1;
    w0 = w1;
    k0 = k1;
  }
  return 0;
}

// Rows [lo, hi) of the table: the first row that is not "before" the key.
// UPPER false: before = word < key (the lower bound).  UPPER true: before =
// word < key or the word starts with the key (the end of the key's prefix range).
template <bool UPPER>
__device__ __forceinline__ uint64_t fd_bound(const FdTab& T, const FdKeys& K, uint64_t ko, uint64_t klen, uint64_t lo, uint64_t hi) {
  for (uint32_t s = 0; s < T.steps && lo < hi; s++) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint64_t o = T.offs[mid], wlen = T.offs[mid + 1] - o;
    const int c = fd_cmp_common(T.bytes, o, wlen, K.kbytes, ko, klen);
    const bool before = UPPER ? c <= 0 : (c < 0 || (c == 0 && wlen < klen));
    if (before) lo = mid + 1;
    else hi = mid;
  }
  if (lo < hi) atomicMax(&K.ctl->err, 1ull);
  return lo;
}

}  // namespace

// first[i], last[i] of every key; FdCtl::big.
extern "C" __global__ __launch_bounds__(FD_T) void k_fd_search(FdTab T, FdKeys K) {
  bool big = false;
  for (uint64_t i = (uint64_t)blockIdx.x * FD_T + threadIdx.x; i < K.nq; i += (uint64_t)gridDim.x * FD_T) {
    const uint64_t ko = K.koffs[i], klen = K.koffs[i + 1] - ko;
    const uint64_t first = fd_bound<false>(T, K, ko, klen, 0, T.n);
    uint64_t last = first;
    if (K.mode == MOX_FIND_PREFIX) {
      last = fd_bound<true>(T, K, ko, klen, first, T.n);
    } else if (K.mode == MOX_FIND_EXACT && first < T.n) {
      const uint64_t o = T.offs[first], wlen = T.offs[first + 1] - o;
      if (wlen == klen && fd_cmp_common(T.bytes, o, wlen, K.kbytes, ko, klen) == 0) last = first + 1;
    }
    if (first > last || last > T.n) atomicMax(&K.ctl->err, 2ull);
    K.first[i] = first;
    K.last[i] = last;
    big |= last / FD_TILE > (first + FD_TILE - 1) / FD_TILE;
  }
  if (__ballot(big) && (threadIdx.x & 63) == 0) K.ctl->big = 1;
}

// S[tile] = the wrapping sum of the tile's counts (when some range holds a whole tile).
extern "C" __global__ __launch_bounds__(FD_T) void k_fd_tiles(FdTab T, const FdCtl* ctl, uint64_t ntiles, uint64_t* __restrict__ S) {
  __shared__ uint64_t s_w[FD_WAVES];
  if (!ctl->big) return;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < FD_PER; j++) {
      const uint64_t i = tile * FD_TILE + (uint32_t)j * FD_T + t;
      if (i < T.n) v += __builtin_nontemporal_load(T.counts + i);
    }
    v = wave_sum(v);
    if (lane == 0) s_w[wv] = v;
    __syncthreads();
    if (t == 0) {
      uint64_t x = 0;
      for (int w = 0; w < FD_WAVES; w++) x += s_w[w];
      S[tile] = x;
    }
    __syncthreads();  // the LDS row is the next tile's
  }
}

// Exclusive scan in place of the ntiles tile sums; S[ntiles] = the total.
extern "C" __global__ __launch_bounds__(FD_SCAN_T) void k_fd_scan(const FdCtl* ctl, uint64_t* S, uint64_t ntiles) {
  if (!ctl->big) return;
  scan_one_wg<uint64_t, FD_SCAN_T>(S, ntiles, S + ntiles);
}

// sums[i] = the wrapping sum of counts[first[i], last[i]), one wave per key.
extern "C" __global__ __launch_bounds__(FD_T) void k_fd_sum(FdTab T, FdKeys K, const uint64_t* __restrict__ S) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * FD_WAVES;
  for (uint64_t i = (uint64_t)blockIdx.x * FD_WAVES + (threadIdx.x >> 6); i < K.nq; i += nw) {
    const uint64_t first = K.first[i], last = K.last[i];
    if (first > last || last > T.n) continue;  // (k_fd_search has set the error word)
    const uint64_t ft = (first + FD_TILE - 1) / FD_TILE, lt = last / FD_TILE;
    // whole tiles ft .. lt - 1 from the scan; the rows before and behind them directly
    const bool whole = lt > ft;
    const uint64_t head_end = whole ? ft * FD_TILE : last, tail_begin = whole ? lt * FD_TILE : last;
    uint64_t v = 0;
    for (uint64_t r = first + lane; r < head_end; r += 64) v += T.counts[r];
    for (uint64_t r = tail_begin + lane; r < last; r += 64) v += T.counts[r];
    v = wave_sum(v);
    if (whole) v += S[lt] - S[ft];
    if (lane == 0) K.sums[i] = v;
  }
}

extern "C" int mox_find_ranges(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, uint64_t n, uint32_t mode, uint64_t* first,
                               uint64_t* last, uint64_t* sums, mox_find_info* info) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  if (mode > MOX_FIND_LOWER) return fail(MOX_EINVAL, "find: unknown mode %u", mode);
  if (n > MOX_FIND_MAX) return fail(MOX_EINVAL, "find: %llu keys (at most MOX_FIND_MAX = %u)", (unsigned long long)n, MOX_FIND_MAX);
  if (n && (!offs || !first || !last)) return fail(MOX_EINVAL, "find: NULL argument");
  uint64_t nb = 0;
  for (uint64_t i = 0; i < n; i++)
    if (offs[i + 1] < offs[i]) return fail(MOX_EINVAL, "find: offsets decrease at key %llu", (unsigned long long)i);
  if (n) nb = offs[n] - offs[0];
  if (nb >> 32) return fail(MOX_EINVAL, "find: %llu key bytes (fewer than 2^32)", (unsigned long long)nb);
  if (nb && !bytes) return fail(MOX_EINVAL, "find: NULL argument");
  if (int rc = result_begin(e)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  mox_find_info fi{};
  fi.queries = n;
  fi.device_bytes = e->fd_tmp.cap;
  if (!n) {
    if (info) *info = fi;
    return MOX_OK;
  }
  // bytewise order: the implicit MOX_F_SORT_BYTES sort of a fetch, else the caller's mox_sort_result
  bool host_sort = false;
  if (int rc = sort_for_fetch(e, &host_sort)) return rc;
  if (host_sort) return fail(MOX_ENOMEM, "find: the device sort's scratch does not fit, the result stays in engine order");
  const mox_engine::Res& r = e->res;
  if (!r.sorted && r.n > 1)
    return fail(MOX_ESTATE, "find: the result is %s, not in bytewise order: call mox_sort_result first", r.ranked ? "ranked by count" : "in engine order");
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  int rc;
  // device scratch: [first n | last n | control block | sums n] (the part that comes back) | key offsets | tile sums + total | key bytes
  const uint64_t ntiles = (r.n + FD_TILE - 1) / FD_TILE;
  const size_t head_b = 16 * n + sizeof(FdCtl), out_b = head_b + (sums ? 8 * n : 0), ko_b = 8 * (n + 1);
  uint8_t *out, *d_kbytes;
  uint64_t *d_koffs, *S;
  if ((rc = carve_dev(e->fd_tmp, [&](Carve& c) {
         out = c.take_bytes(head_b + 8 * n);
         d_koffs = c.take<uint64_t>(n + 1);
         S = c.take<uint64_t>(sums ? ntiles + 1 : 0);
         d_kbytes = c.take_bytes(nb + TABLE_SLACK);  // (the key bytes are read as table bytes are)
       })))
    return rc;
  if ((rc = grow_pinned(e->fd_pin, std::max(out_b, ko_b)))) return rc;
  FdKeys K{};
  K.first = (uint64_t*)out;
  K.last = (uint64_t*)(out + 8 * n);
  K.ctl = (FdCtl*)(out + 16 * n);
  K.sums = sums ? (uint64_t*)(out + head_b) : nullptr;
  K.koffs = d_koffs;
  K.kbytes = d_kbytes;
  K.nq = n;
  K.mode = mode;
  FdTab T{r.counts, r.offs, r.bytes, r.n, 1};
  while ((1ull << (T.steps - 1)) < r.n + 1) T.steps++;  // ceil(log2(n + 1)) + 1
  // the offsets rebased to the first key, through the pinned block
  uint64_t* h_offs = (uint64_t*)e->fd_pin.p;
  for (uint64_t i = 0; i <= n; i++) h_offs[i] = offs[i] - offs[0];
  HIPCHK(hipMemcpyAsync(d_koffs, h_offs, ko_b, hipMemcpyHostToDevice, st));
  if (nb) HIPCHK(hipMemcpyAsync(d_kbytes, bytes + offs[0], nb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(K.ctl, 0, sizeof(FdCtl), st));
  const uint64_t cap = grid_cap(e, "MOX_FIND_GRID");
  hipLaunchKernelGGL(k_fd_search, dim3((uint32_t)std::min((n + FD_T - 1) / FD_T, cap)), dim3(FD_T), 0, st, T, K);
  q.step("k_fd_search");
  if (sums) {
    if (ntiles) {
      hipLaunchKernelGGL(k_fd_tiles, dim3((uint32_t)std::min(ntiles, cap)), dim3(FD_T), 0, st, T, (const FdCtl*)K.ctl, ntiles, S);
      q.step("k_fd_tiles");
      hipLaunchKernelGGL(k_fd_scan, dim3(1), dim3(FD_SCAN_T), 0, st, (const FdCtl*)K.ctl, S, ntiles);
      q.step("k_fd_scan");
    }
    hipLaunchKernelGGL(k_fd_sum, dim3((uint32_t)std::min((n + FD_WAVES - 1) / FD_WAVES, cap)), dim3(FD_T), 0, st, T, K, (const uint64_t*)S);
    q.step("k_fd_sum");
  }
  HIPCHK(hipGetLastError());
  // the one copy back: the ranges and the control block, and the sums when they are asked for
  uint8_t* h_out = (uint8_t*)e->fd_pin.p;
  HIPCHK(hipMemcpyAsync(h_out, K.first, out_b, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  FdCtl h;
  memcpy(&h, h_out + 16 * n, sizeof h);
  const uint64_t* h_first = (const uint64_t*)h_out;
  const uint64_t* h_last = h_first + n;
  bool bad = h.err != 0;
  for (uint64_t i = 0; i < n && !bad; i++) {
    bad = h_first[i] > h_last[i] || h_last[i] > r.n;
    fi.matched += h_last[i] > h_first[i] ? 1u : 0u;
    fi.rows += h_last[i] - h_first[i];
  }
  if (bad) return fail(MOX_EHIP, "find: inconsistent ranges (error %llu, %llu rows)", h.err, (unsigned long long)r.n);
  memcpy(first, h_first, 8 * n);
  memcpy(last, h_last, 8 * n);
  if (sums) memcpy(sums, h_out + head_b, 8 * n);
  fi.tile_pass = sums && h.big ? 1 : 0;
  fi.device_bytes = e->fd_tmp.cap;
  fi.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (info) *info = fi;
  return MOX_OK;
}
