// Device top-k of the result table (mox_top_words): the k most frequent words
// selected on the GPU, so that only those words cross to the host.  The
// reference prints them from its HashMap (print_top_words, src/main.rs:184-192);
// mox_print_top_words does the same from a fetched table.  This is the
// selection half without the fetch.
//
// Exact and deterministic: the output depends only on the table's contents and
// order (count descending, equal counts by table index ascending).
//
//  1. Threshold T = the k-th largest count, by MSB-first radix select over the
//     count's eight 8-bit digits.  Level l: k_tk_hist histograms digit l of the
//     counts whose higher digits equal the prefix chosen so far (per-workgroup
//     LDS bins, a wave's most common digit added once per wave by ballot, then
//     one 64-bit global add per non-zero bin); k_tk_pick (one workgroup) walks
//     the bins from the top and updates the control block {prefix, above}.
//     The levels are queued back to back: the kernels read the control block,
//     the host does not.  Level 0 also ORs every count together, and a level
//     whose digit lies wholly above the highest set bit returns at once.
//  2. k_tk_ties: one more pass over the counts.  Counts > T (fewer than k) are
//     appended to the candidate list through an atomic cursor (their order is
//     settled by the sort below); counts == T are counted per tile of TK_TILE
//     consecutive indices, one wave per tile.
//  3. k_tk_scan (one workgroup): exclusive scan of the tile counts.
//  4. k_tk_emit: a tile's tied words whose global tie rank is < need = k -
//     above become candidates, in index order; a tile without ties, or whose
//     prefix is already >= need, is skipped without reading the table.
//  5. k_tk_sort (one workgroup): bitonic sort of the <= 4,096 candidates
//     {count, idx} in LDS by (count descending, idx ascending); writes the
//     counts, the words' source offsets and the exclusive scan of their
//     lengths, and the total byte length into the control block.
//  6. One host read of the control block sizes the output; k_tk_gather copies
//     the selected words' bytes (any alignment; several workgroups share a
//     long word) behind the counts and offsets, and one copy brings the block
//     to the host.
//
// mox_top_rows is the same selection over a row range of the table: the host
// passes the counts and offsets from the range's first row on (top_of_rows).
//
// Scratch is O(n / TK_TILE + k): the tile counts, and a fixed 200 KiB of
// control block, histograms, candidates and outputs.  The result table itself
// is only read.
#include <algorithm>
#include <cstdlib>

#include "mox_dev.h"
#include "mox_host.h"

namespace {

constexpr int TK_T = 256;                          // threads of the streaming kernels
constexpr int TK_WAVES = TK_T / 64;
constexpr int TK_PER = 64;                         // counts per lane and tile
constexpr uint64_t TK_TILE = 4096;                 // tie-count tile: 64 lanes x TK_PER consecutive indices, one wave
constexpr int TK_LEVELS = 8, TK_BINS = 256;        // 8-bit digits of a 64-bit count, most significant first
constexpr int TK_HIST_PER = 16;                    // counts per thread and grid step of k_tk_hist
constexpr uint32_t TK_MAX = MOX_TOP_MAX;
static_assert(TK_TILE == 64ull * TK_PER && TK_PER % 8 == 0, "one wave per tile, eight steps at a time");
static_assert((TK_MAX & (TK_MAX - 1)) == 0, "the candidate sort pads to a power of two");

struct TkCtl {
  uint64_t prefix;  // the digits of T chosen so far (after the last level: T)
  uint64_t above;   // counts greater than every count with this prefix (after the last level: counts > T)
  uint64_t ormask;  // OR of every count
  uint64_t cursor;  // candidates with a count > T appended so far
  uint64_t nbytes;  // byte length of the selected words
  uint64_t pad[3];
};
static_assert(sizeof(TkCtl) == 64, "read back in one copy");

struct __attribute__((aligned(16))) TkCand {
  uint64_t count, idx;
};

}  // namespace

// Level `level` of the radix select: digit (c >> shift) & 255 of the counts
// that carry the chosen prefix above it, into hist[level][.].  Per-workgroup
// LDS bins: the lanes that share the digit of the wave's first matching lane
// add their number once (nearly every count of a big table is 1: one bin),
// the others add themselves.
extern "C" __global__ __launch_bounds__(TK_T) void k_tk_hist(const uint64_t* __restrict__ counts, uint64_t n, int level,
                                                            TkCtl* ctl, unsigned long long* hist) {
  __shared__ uint32_t h[TK_BINS];
  const int t = threadIdx.x, lane = t & 63;
  const uint32_t shift = 56u - 8u * (uint32_t)level;
  uint64_t prefix = 0;
  if (level > 0) {
    if ((ctl->ormask >> shift) == 0) return;  // every count lies below this digit (k_tk_pick keeps digit 0)
    prefix = ctl->prefix >> (shift + 8);
  }
  h[t] = 0;
  __syncthreads();
  uint64_t orv = 0;
  const uint64_t step = (uint64_t)gridDim.x * TK_T * TK_HIST_PER;
  for (uint64_t b0 = (uint64_t)blockIdx.x * TK_T * TK_HIST_PER; b0 < n; b0 += step) {
    uint64_t v[TK_HIST_PER];
#pragma unroll
    for (int j = 0; j < TK_HIST_PER; j++) {
      const uint64_t i = b0 + (uint64_t)j * TK_T + t;
      v[j] = i < n ? __builtin_nontemporal_load(counts + i) : 0ull;
    }
#pragma unroll
    for (int j = 0; j < TK_HIST_PER; j++) {
      const uint64_t i = b0 + (uint64_t)j * TK_T + t;
      const uint64_t c = v[j];
      orv |= c;
      const bool m = i < n && (level == 0 || (c >> (shift + 8)) == prefix);
      const uint32_t d = (uint32_t)(c >> shift) & 0xFFu;
      const uint64_t act = __ballot(m);
      if (act) {
        const int leader = __ffsll((unsigned long long)act) - 1;
        const uint32_t d0 = __shfl(d, leader);
        const uint64_t same = __ballot(m && d == d0);
        if (lane == leader) atomicAdd(&h[d0], (uint32_t)__popcll(same));
        else if (m && d != d0) atomicAdd(&h[d], 1u);
      }
    }
  }
  if (level == 0) {
    for (int o = 32; o > 0; o >>= 1) orv |= __shfl_xor(orv, o);
    if (lane == 0 && orv) atomicOr((unsigned long long*)&ctl->ormask, (unsigned long long)orv);
  }
  __syncthreads();
  const uint32_t x = h[t];
  if (x) atomicAdd(&hist[level * TK_BINS + t], (unsigned long long)x);
}

// One workgroup after level `level`'s histogram: the digit d of T at this
// level is the largest one with (counts above it) < rem <= (counts at or above
// it), rem = kk - above being the rank still looked for among the counts that
// carry the prefix.  Thread t holds bin 255 - t, so an inclusive scan over the
// threads is the bins' suffix sum.
extern "C" __global__ __launch_bounds__(TK_BINS) void k_tk_pick(int level, uint64_t kk, TkCtl* ctl,
                                                                const unsigned long long* hist) {
  __shared__ uint64_t ws[TK_BINS / 64];
  const int t = threadIdx.x, wv = t >> 6;
  const uint32_t shift = 56u - 8u * (uint32_t)level;
  if (level > 0 && (ctl->ormask >> shift) == 0) return;  // digit 0, nothing above it
  const uint64_t rem = kk - ctl->above;
  const uint32_t bin = (uint32_t)(TK_BINS - 1 - t);
  const uint64_t x = hist[level * TK_BINS + bin];
  uint64_t inc = wave_incscan<uint64_t>(x);
  if ((t & 63) == 63) ws[wv] = inc;
  __syncthreads();
  for (int k = 0; k < wv; k++) inc += ws[k];
  // (rem >= 1 and at least rem counts carry the prefix: exactly one bin qualifies)
  if (inc >= rem && inc - x < rem) {
    ctl->above += inc - x;
    ctl->prefix |= (uint64_t)bin << shift;
  }
}

// One pass with T known: counts > T join the candidates (there are `above` <
// kk of them; their order in the list does not matter), counts == T are
// counted per tile, one wave per tile.
extern "C" __global__ __launch_bounds__(TK_T) void k_tk_ties(const uint64_t* __restrict__ counts, uint64_t n, uint64_t ntiles,
                                                            TkCtl* ctl, uint64_t* tcnt, TkCand* cand) {
  const int lane = threadIdx.x & 63;
  const uint64_t T = ctl->prefix;
  const uint64_t nw = (uint64_t)gridDim.x * TK_WAVES;
  for (uint64_t tile = (uint64_t)blockIdx.x * TK_WAVES + (threadIdx.x >> 6); tile < ntiles; tile += nw) {
    const uint64_t base = tile * TK_TILE;
    uint64_t eq = 0;
#pragma unroll 8
    for (int j = 0; j < TK_PER; j++) {
      const uint64_t i = base + (uint64_t)j * 64 + lane;
      if (i < n) {
        const uint64_t c = __builtin_nontemporal_load(counts + i);
        eq += c == T ? 1u : 0u;
        if (c > T) {
          const unsigned long long p = atomicAdd((unsigned long long*)&ctl->cursor, 1ull);
          if (p < TK_MAX) cand[p] = TkCand{c, i};
        }
      }
    }
    eq = wave_sum(eq);
    if (lane == 0) tcnt[tile] = eq;
  }
}

// Exclusive scan of a[0, nt) in place, a[nt] = the total: one workgroup,
// 1,024 values per step with a running carry (mox_dev.h; nt = n / TK_TILE values).
extern "C" __global__ __launch_bounds__(1024) void k_tk_scan(uint64_t* a, uint64_t nt) { scan_one_wg<uint64_t, 1024>(a, nt, a + nt); }

// The tied words (count == T) of global tie rank < need, in index order, into
// candidates [above, kk).  One wave per tile, 64 consecutive indices per step:
// a word's rank is the ties before its step plus those on lower lanes
// (ballot).  A tile without ties, or behind the need-th tie, is skipped on its
// scanned count alone, and a tile stops at the need-th tie.
extern "C" __global__ __launch_bounds__(TK_T) void k_tk_emit(const uint64_t* __restrict__ counts, uint64_t n, uint64_t ntiles,
                                                            uint64_t kk, const TkCtl* ctl, const uint64_t* tpre, TkCand* cand) {
  const int lane = threadIdx.x & 63;
  const uint64_t below = (1ull << lane) - 1ull;
  const uint64_t T = ctl->prefix, above = ctl->above, need = kk - above;
  const uint64_t nw = (uint64_t)gridDim.x * TK_WAVES;
  for (uint64_t tile = (uint64_t)blockIdx.x * TK_WAVES + (threadIdx.x >> 6); tile < ntiles; tile += nw) {
    const uint64_t pre = tpre[tile];
    if (pre >= need || tpre[tile + 1] == pre) continue;
    const uint64_t base = tile * TK_TILE + lane;
    uint64_t run = pre;  // ties before the step (the same on every lane)
    for (int j0 = 0; j0 < TK_PER && run < need; j0 += 8) {
      uint64_t v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const uint64_t i = base + (uint64_t)(j0 + u) * 64;
        v[u] = i < n ? counts[i] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const uint64_t i = base + (uint64_t)(j0 + u) * 64;
        const bool eq = i < n && v[u] == T;
        const uint64_t m = __ballot(eq);
        const uint64_t r = run + (uint64_t)__popcll(m & below);
        if (eq && r < need && above + r < TK_MAX) cand[above + r] = TkCand{T, i};
        run += (uint64_t)__popcll(m);
      }
    }
  }
}

// The kk candidates sorted by (count descending, idx ascending) in LDS, then
// per selected word its count, source byte offset and the exclusive scan of
// the lengths (o_offs[kk] = ctl->nbytes = the total).
extern "C" __global__ __launch_bounds__(1024) void k_tk_sort(const TkCand* cand, uint64_t kk, const uint64_t* offs, TkCtl* ctl,
                                                             uint64_t* o_counts, uint64_t* o_src, uint64_t* o_offs) {
  __shared__ uint64_t sc[TK_MAX], si[TK_MAX];  // 64 KiB of the CU's 160
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint32_t P = 1;
  while (P < kk) P <<= 1;
  for (uint32_t i = t; i < P; i += 1024) {
    // padding sorts last: no word has index 2^64 - 1
    sc[i] = i < kk ? cand[i].count : 0ull;
    si[i] = i < kk ? cand[i].idx : ~0ull;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = t; i < P; i += 1024) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint64_t ca = sc[i], cb = sc[l], ia = si[i], ib = si[l];
          const bool b_first = cb > ca || (cb == ca && ib < ia);  // l's record belongs before i's
          if (b_first == ((i & k) == 0)) {
            sc[i] = cb; sc[l] = ca;
            si[i] = ib; si[l] = ia;
          }
        }
      }
      __syncthreads();
    }
  for (uint32_t i = t; i < kk; i += 1024) o_counts[i] = sc[i];
  __syncthreads();
  uint64_t* ws = sc;  // the counts have left: their array holds the scan's wave totals
  uint64_t carry = 0;
  for (uint32_t c = 0; c < kk; c += 1024) {
    const uint32_t i = c + t;
    uint64_t len = 0;
    if (i < kk) {
      const uint64_t w = si[i], o = offs[w];
      len = offs[w + 1] - o;
      o_src[i] = o;
    }
    const uint64_t inc = wave_incscan<uint64_t>(len);
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    uint64_t pre = 0, tot = 0;
    for (int k = 0; k < 16; k++) {
      if (k < (int)wv) pre += ws[k];
      tot += ws[k];
    }
    if (i < kk) o_offs[i] = carry + pre + inc - len;
    carry += tot;
    __syncthreads();
  }
  if (t == 0) {
    o_offs[kk] = carry;
    ctl->nbytes = carry;
  }
}

// The output block [counts kk + 1 | offs kk + 1 | bytes], laid out like
// mox_fetch_table's host block.  Workgroup (w, y) copies word w's bytes y 256,
// y 256 + gridDim.y 256, ...: source and destination offsets are arbitrary, so
// byte by byte (consecutive lanes, consecutive bytes).
extern "C" __global__ __launch_bounds__(256) void k_tk_gather(uint64_t kk, const uint64_t* o_counts, const uint64_t* o_src,
                                                              const uint64_t* o_offs, const uint8_t* __restrict__ bytes,
                                                              uint64_t* out) {
  const uint64_t w = blockIdx.x;
  uint64_t* oc = out;
  uint64_t* oo = out + kk + 1;
  uint8_t* ob = reinterpret_cast<uint8_t*>(out + 2 * (kk + 1));
  const uint64_t dst = o_offs[w], len = o_offs[w + 1] - dst, src = o_src[w];
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    oc[w] = o_counts[w];
    oo[w] = dst;
    if (w + 1 == kk) {
      oc[kk] = 0;
      oo[kk] = dst + len;
    }
  }
  for (uint64_t b = (uint64_t)blockIdx.y * 256 + threadIdx.x; b < len; b += (uint64_t)gridDim.y * 256) ob[dst + b] = bytes[src + b];
}

// The top-k of n rows of the result (a result is open: result_begin): row i's
// count is r_counts[i] and its word bytes[r_offs[i], r_offs[i + 1]) of the
// result's bytes, so a row range of the table is the table's two arrays from
// its first row on -- the kernels load counts as 8-byte words and offsets are
// absolute.  Candidate indices, and with them the order of equal counts, are
// relative to the range's first row, which is table order.
static int top_of_rows(mox_engine* e, const uint64_t* r_counts, const uint64_t* r_offs, uint64_t n, size_t k, mox_table** out) {
  const mox_engine::Res& r = e->res;
  const uint64_t kk = std::min<uint64_t>(k, n);
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  uint64_t nb = 0;
  if (kk) {
    const uint64_t ntiles = (n + TK_TILE - 1) / TK_TILE;
    // scratch: [control block | histograms] (zeroed together) | candidates | counts, source offsets, offsets | tile counts + total
    const size_t hist_b = (size_t)TK_LEVELS * TK_BINS * 8;
    TkCtl* ctl;
    TkCand* cand;
    uint64_t *o_counts, *o_src, *o_offs, *tcnt;
    if (int rc = carve_dev(e->k_tmp, [&](Carve& c) {
          ctl = (TkCtl*)c.take_bytes(sizeof(TkCtl) + hist_b);
          cand = c.take<TkCand>(TK_MAX);
          o_counts = c.take<uint64_t>((size_t)TK_MAX + 1);
          o_src = c.take<uint64_t>((size_t)TK_MAX + 1);
          o_offs = c.take<uint64_t>((size_t)TK_MAX + 1);
          tcnt = c.take<uint64_t>(ntiles + 1);
        }))
      return rc;
    unsigned long long* hist = (unsigned long long*)(ctl + 1);
    HIPCHK(hipMemsetAsync(ctl, 0, sizeof(TkCtl) + hist_b, st));
    // k_tk_hist: a workgroup's LDS bins are 32-bit, so its share of the counts stays below 2^32
    const uint64_t hgrid = std::max<uint64_t>(std::min<uint64_t>((n + TK_T * TK_HIST_PER - 1) / (TK_T * TK_HIST_PER), 8ull * e->n_cu),
                                              (n >> 31) + 1);
    if (hgrid > 0x7FFFFFFFull) return fail(MOX_EINVAL, "top words: %llu words", (unsigned long long)n);
    const uint32_t wgrid = (uint32_t)std::min<uint64_t>((ntiles + TK_WAVES - 1) / TK_WAVES, 8ull * e->n_cu);
    for (int level = 0; level < TK_LEVELS; level++) {
      hipLaunchKernelGGL(k_tk_hist, dim3((uint32_t)hgrid), dim3(TK_T), 0, st, r_counts, n, level, ctl, hist);
      q.step("k_tk_hist");
      hipLaunchKernelGGL(k_tk_pick, dim3(1), dim3(TK_BINS), 0, st, level, kk, ctl, (const unsigned long long*)hist);
      q.step("k_tk_pick");
    }
    hipLaunchKernelGGL(k_tk_ties, dim3(wgrid), dim3(TK_T), 0, st, r_counts, n, ntiles, ctl, tcnt, cand);
    q.step("k_tk_ties");
    hipLaunchKernelGGL(k_tk_scan, dim3(1), dim3(1024), 0, st, tcnt, ntiles);
    q.step("k_tk_scan");
    hipLaunchKernelGGL(k_tk_emit, dim3(wgrid), dim3(TK_T), 0, st, r_counts, n, ntiles, kk, (const TkCtl*)ctl, (const uint64_t*)tcnt,
                       cand);
    q.step("k_tk_emit");
    hipLaunchKernelGGL(k_tk_sort, dim3(1), dim3(1024), 0, st, (const TkCand*)cand, kk, r_offs, ctl, o_counts, o_src, o_offs);
    q.step("k_tk_sort");
    HIPCHK(hipGetLastError());
    // the one round trip before the output is sized: the selected words' byte length
    TkCtl h;
    HIPCHK(hipMemcpyAsync(&h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    nb = h.nbytes;
    if (h.cursor != h.above || h.above >= kk || nb > r.nb)
      return fail(MOX_EHIP, "top words: inconsistent selection (above %llu, appended %llu, k %llu, %llu bytes)",
                  (unsigned long long)h.above, (unsigned long long)h.cursor, (unsigned long long)kk, (unsigned long long)nb);
    if (int rc = grow_dev(e->k_out, (kk + 1) * 16 + nb + 64)) return rc;
    // several workgroups per word once the words are long (up to 16 MiB each); one without a share of its word's bytes ends at once
    const uint32_t gy = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, nb / 16384));
    hipLaunchKernelGGL(k_tk_gather, dim3((uint32_t)kk, gy), dim3(256), 0, st, kk, (const uint64_t*)o_counts, (const uint64_t*)o_src,
                       (const uint64_t*)o_offs, r.bytes, (uint64_t*)e->k_out.p);
    q.step("k_tk_gather");
    HIPCHK(hipGetLastError());
  }
  const size_t bytes = sizeof(mox_table) + (kk + 1) * 8 * 2 + nb + 16;
  uint8_t* mem = (uint8_t*)malloc(bytes);
  if (!mem) return fail(MOX_ENOMEM, "host allocation of %zu bytes failed", bytes);
  mox_table* t = (mox_table*)mem;
  uint64_t* counts = (uint64_t*)(mem + sizeof(mox_table));
  uint64_t* offs = counts + kk + 1;
  t->n = kk;
  t->tokens = r.tokens;
  t->counts = counts;
  t->offs = offs;
  t->bytes = (uint8_t*)(offs + kk + 1);
  if (kk) {
    hipError_t er = hipMemcpyAsync(counts, e->k_out.p, (kk + 1) * 16 + nb, hipMemcpyDeviceToHost, st);
    if (er == hipSuccess) er = hipStreamSynchronize(st);
    if (er != hipSuccess) {
      free(mem);
      return fail(MOX_EHIP, "top words: copy to the host failed: %s", hipGetErrorString(er));
    }
  } else {
    offs[0] = 0;
  }
  *out = t;
  return MOX_OK;
}

static int top_args(mox_engine* e, size_t k, mox_table** out) {
  if (!e || !out) return fail(MOX_EINVAL, "NULL argument");
  *out = nullptr;
  if (k > MOX_TOP_MAX) return fail(MOX_EINVAL, "k = %zu (at most MOX_TOP_MAX = %d)", k, MOX_TOP_MAX);
  return result_begin(e);
}

extern "C" int mox_top_words(mox_engine* e, size_t k, mox_table** out) {
  if (int rc = top_args(e, k, out)) return rc;
  return top_of_rows(e, e->res.counts, e->res.offs, e->res.n, k, out);
}

extern "C" int mox_top_rows(mox_engine* e, uint64_t first, uint64_t n, size_t k, mox_table** out) {
  if (int rc = top_args(e, k, out)) return rc;
  const mox_engine::Res& r = e->res;
  const uint64_t lo = std::min(first, r.n), cnt = std::min(n, r.n - lo);
  return top_of_rows(e, r.counts + lo, r.offs + lo, cnt, k, out);
}
