// Device text rendering (mox_write_result / mox_result_text): the result table
// as final_result.txt text -- per word its bytes, ' ', the count in decimal,
// '\n' (the reference's write_final_result, src/main.rs:170-182) -- formatted
// on the GPU from the device-resident table, so that only the text crosses to
// the host and no host pass runs over the words.  Byte for byte what
// mox_write_final_result writes from a fetched table.
//
// Line i starts at text offset offs[i] - offs[0] + 2 i + D(i), D(i) = the sum
// of the decimal digit counts of the counts before i: the word bytes are
// already prefix-summed (offs), so only 2 + digits needs a scan.
//
//  1. k_tx_len: per tile of TX_TILE consecutive words (one wave per tile) the
//     tile's text bytes.  Digit count: a clz estimate corrected against a
//     powers-of-ten table.
//  2. k_tx_scan (one workgroup): exclusive scan of the tile lengths, the total
//     at [ntiles].
//  3. k_tx_emit(lo, hi, out): bytes [lo, hi) of the text into a slice buffer.
//     A slice is a byte range of the text, so every slice has the same size,
//     its file offset is lo, and a line longer than a slice is simply clipped.
//     A workgroup finds the first tile that reaches into [lo, hi) by binary
//     search in the scanned tile array and takes tiles grid-stride from there
//     up to the first one that starts at or after hi.  Per tile: the lanes load
//     their words' offsets and counts, a workgroup scan of 2 + digits gives
//     each line's start inside the tile, then
//       fast path (the tile's text fits TX_LDS bytes of LDS): the tile's source
//         bytes are one contiguous run [offs[b], offs[e]); they are loaded with
//         16-byte coalesced loads into LDS, each lane moves its words to their
//         lines (words over TX_COOP bytes: the whole workgroup, one after
//         another) and writes separator, digits and newline, and the composed
//         text leaves with 16-byte stores aligned on the destination (both LDS
//         images keep their global address's phase mod 16; byte head and tail);
//       slow path (long words): straight to global memory, one wave per word
//         with consecutive lanes on consecutive bytes, words over TX_BIG bytes
//         by the whole workgroup.
//     Every store is clipped to [lo, hi): each byte of the slice is written
//     exactly once and no byte outside it is touched.
//
// Host: two device slice buffers and two pinned host buffers; slice s + 1 is
// emitted and copied on the engine stream while the host writes slice s
// (pwrite at offset lo, or memcpy into the malloc'd text).  Scratch is
// 8 (ntiles + 1) bytes plus the four slice buffers, whatever n is.  The result
// table itself is only read.
#include <algorithm>
#include <cerrno>
#include <cstdlib>

#include "mox_dev.h"
#include "mox_host.h"

namespace {

constexpr int TX_T = 256;                 // threads of the kernels
constexpr int TX_WAVES = TX_T / 64;
constexpr uint64_t TX_TILE = 1024;         // words per tile
constexpr int TX_PER = 4;                 // words per thread and tile in k_tx_emit
constexpr uint32_t TX_LDS = 24576;         // fast path: most text bytes of a tile (two LDS images of this size + 16: 2 workgroups per CU)
constexpr uint32_t TX_COOP = 64;          // fast path: a longer word is moved by the whole workgroup
constexpr uint64_t TX_BIG = 4096;         // slow path: a longer word is copied by the whole workgroup
// default slice bytes (MOX_TEXT_SLICE overrides).  Against 32 and 128 MiB on the 1.22 GB HICARD text:
// mox_write_result is bound by the host's pwrite and the three sizes differ by less than its run-to-run
// spread (277-295 / 275-295 / 272-315 ms); mox_result_text and the 15 MB ZIPF text are fastest at 8 MiB in
// every run.  The kernels' share moves the other way (4.4 / 2.5 / 2.1 ms) and does not matter
constexpr uint64_t TX_SLICE = 8ull << 20;
constexpr uint64_t TX_SLICE_MIN = 256;
static_assert(TX_TILE == (uint64_t)TX_T * TX_PER && TX_TILE % 64 == 0, "k_tx_emit: TX_PER words per thread; k_tx_len: one wave per tile");
static_assert(TX_SLICE % 16 == 0 && TX_SLICE_MIN % 16 == 0, "slices start on 16-byte text offsets");

typedef uint32_t tx_u32x4 __attribute__((ext_vector_type(4)));

__constant__ uint64_t tx_pow10[20] = {1ull,
                                      10ull,
                                      100ull,
                                      1000ull,
                                      10000ull,
                                      100000ull,
                                      1000000ull,
                                      10000000ull,
                                      100000000ull,
                                      1000000000ull,
                                      10000000000ull,
                                      100000000000ull,
                                      1000000000000ull,
                                      10000000000000ull,
                                      100000000000000ull,
                                      1000000000000000ull,
                                      10000000000000000ull,
                                      100000000000000000ull,
                                      1000000000000000000ull,
                                      10000000000000000000ull};

// Decimal digits of c (0 renders as "0": one digit).  v = c | 1 has c's digit
// count (every power of ten above 1 is even); with b = v's bit length,
// t = floor(b 1233 / 4096) ~ floor(b log10 2) satisfies 10^(t-1) <= v < 10^(t+1).
__device__ __forceinline__ uint32_t tx_digits(uint64_t c) {
  const uint64_t v = c | 1ull;
  const uint32_t b = 64u - (uint32_t)__clzll((long long)v);
  const uint32_t t = (b * 1233u) >> 12;
  return t + (v >= tx_pow10[t] ? 1u : 0u);
}

// one text byte at text offset g, if the slice holds it
__device__ __forceinline__ void tx_put(uint8_t* out, uint64_t lo, uint64_t hi, uint64_t g, uint8_t v) {
  if (g >= lo && g < hi) out[g - lo] = v;
}

}  // namespace

// tlen[tile] = text bytes of the tile's words: their bytes + 2 + digits each.
extern "C" __global__ __launch_bounds__(TX_T) void k_tx_len(const uint64_t* __restrict__ counts, const uint64_t* __restrict__ offs,
                                                           uint64_t n, uint64_t ntiles, uint64_t* tlen) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * TX_WAVES;
  for (uint64_t tile = (uint64_t)blockIdx.x * TX_WAVES + (threadIdx.x >> 6); tile < ntiles; tile += nw) {
    const uint64_t base = tile * TX_TILE, end = base + TX_TILE < n ? base + TX_TILE : n;
    uint64_t s = 0;
#pragma unroll 8
    for (int j = 0; j < (int)(TX_TILE / 64); j++) {
      const uint64_t i = base + (uint64_t)j * 64 + lane;
      if (i < end) s += 2u + tx_digits(__builtin_nontemporal_load(counts + i));
    }
    s = wave_sum(s);
    if (lane == 0) tlen[tile] = s + (offs[end] - offs[base]);
  }
}

// Exclusive scan of a[0, nt) in place, a[nt] = the total: one workgroup,
// 1,024 values per step with a running carry (mox_dev.h).
extern "C" __global__ __launch_bounds__(1024) void k_tx_scan(uint64_t* a, uint64_t nt) { scan_one_wg<uint64_t, 1024>(a, nt, a + nt); }

// Text bytes [lo, hi) into out[0, hi - lo): lo is a multiple of 16 and out is
// 16-byte aligned, so a text offset and its address in out share their phase
// mod 16.  lo < pre[ntiles] (the text's length); hi may lie past it.
extern "C" __global__ __launch_bounds__(TX_T) void k_tx_emit(const uint64_t* __restrict__ counts, const uint64_t* __restrict__ offs,
                                                            const uint8_t* __restrict__ bytes, uint64_t n, uint64_t ntiles,
                                                            const uint64_t* __restrict__ pre, uint64_t lo, uint64_t hi,
                                                            uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[TX_LDS + 16];  // the tile's source bytes, at their address's phase mod 16
  __shared__ __attribute__((aligned(16))) uint8_t s_out[TX_LDS + 16];  // the tile's text, at its text offset's phase mod 16
  __shared__ uint32_t s_ex[TX_TILE];       // 2 + digits per word, then their exclusive scan
  __shared__ uint32_t s_rel[TX_TILE + 1];  // fast path: a word's first byte inside the tile's source run
  __shared__ uint32_t s_long[TX_LDS / (TX_COOP + 3) + 1];  // fast path: the words over TX_COOP bytes
  __shared__ uint32_t s_ws[TX_WAVES];
  __shared__ uint32_t s_nlong;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  // the first tile that reaches into the slice: the last one that starts at or before lo
  uint64_t first = 0, past = ntiles;  // pre[first] <= lo < pre[past]
  while (past - first > 1) {
    const uint64_t mid = first + (past - first) / 2;
    if (pre[mid] <= lo) first = mid; else past = mid;
  }
  for (uint64_t tile = first + blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t T0 = pre[tile];
    if (T0 >= hi) break;
    const uint64_t T1 = pre[tile + 1];
    const uint64_t base = tile * TX_TILE;
    const uint32_t nw = (uint32_t)(n - base < TX_TILE ? n - base : TX_TILE);
    const uint64_t S0 = offs[base];
    uint64_t c[TX_PER];
#pragma unroll
    for (int j = 0; j < TX_PER; j++) {
      const uint32_t k = (uint32_t)j * TX_T + t;
      c[j] = 0;
      uint32_t ex = 0;
      if (k < nw) {
        c[j] = __builtin_nontemporal_load(counts + base + k);
        ex = 2u + tx_digits(c[j]);
        s_rel[k] = (uint32_t)(__builtin_nontemporal_load(offs + base + k) - S0);
      }
      s_ex[k] = ex;
    }
    if (t == 0) {
      s_rel[nw] = (uint32_t)(offs[base + nw] - S0);
      s_nlong = 0;
    }
    __syncthreads();
    {  // exclusive scan of s_ex: thread t owns words [TX_PER t, TX_PER t + TX_PER)
      uint32_t v[TX_PER], sum = 0;
#pragma unroll
      for (int j = 0; j < TX_PER; j++) {
        v[j] = s_ex[TX_PER * t + j];
        sum += v[j];
      }
      const uint32_t inc = wave_incscan<uint32_t>(sum);
      if (lane == 63) s_ws[wv] = inc;
      __syncthreads();
      uint32_t run = inc - sum;
      for (uint32_t k = 0; k < wv; k++) run += s_ws[k];
#pragma unroll
      for (int j = 0; j < TX_PER; j++) {
        s_ex[TX_PER * t + j] = run;
        run += v[j];
      }
    }
    __syncthreads();
    const uint64_t c0 = T0 > lo ? T0 : lo, c1 = T1 < hi ? T1 : hi;  // the tile's part of the slice (not empty)
    if (T1 - T0 <= TX_LDS) {
      // ---- fast path: source run -> s_raw, lines composed in s_out, s_out -> out
      const uint32_t SL = s_rel[nw];
      const uint8_t* src = bytes + S0;
      const uint32_t sph = (uint32_t)((uintptr_t)src & 15u);
      {
        const uint32_t head = std::min(SL, (16u - sph) & 15u);
        if (t < head) s_raw[sph + t] = __builtin_nontemporal_load(src + t);
        const uint32_t nch = (SL - head) / 16u;
        const tx_u32x4* g = reinterpret_cast<const tx_u32x4*>(src + head);
        tx_u32x4* l = reinterpret_cast<tx_u32x4*>(s_raw + sph + head);
        for (uint32_t i = t; i < nch; i += TX_T) l[i] = __builtin_nontemporal_load(g + i);
        for (uint32_t p = head + 16u * nch + t; p < SL; p += TX_T) s_raw[sph + p] = __builtin_nontemporal_load(src + p);
      }
      __syncthreads();
      const uint32_t dph = (uint32_t)(T0 & 15u);
#pragma unroll
      for (int j = 0; j < TX_PER; j++) {
        const uint32_t k = (uint32_t)j * TX_T + t;
        if (k < nw) {
          const uint32_t rel = s_rel[k], len = s_rel[k + 1] - rel, dst = dph + rel + s_ex[k];
          if (len <= TX_COOP) {
            for (uint32_t b = 0; b < len; b++) s_out[dst + b] = s_raw[sph + rel + b];
          } else {
            s_long[atomicAdd(&s_nlong, 1u)] = k;
          }
          const uint32_t q = dst + len, d = tx_digits(c[j]);
          s_out[q] = ' ';
          uint32_t p = q + d;
          if (c[j] >> 32) {
            uint64_t v = c[j];
            do {
              s_out[p--] = (uint8_t)('0' + (uint32_t)(v % 10u));
              v /= 10u;
            } while (v);
          } else {
            uint32_t v = (uint32_t)c[j];
            do {
              s_out[p--] = (uint8_t)('0' + v % 10u);
              v /= 10u;
            } while (v);
          }
          s_out[q + d + 1] = '\n';
        }
      }
      __syncthreads();
      const uint32_t nl = s_nlong;
      for (uint32_t i = 0; i < nl; i++) {
        const uint32_t k = s_long[i];
        const uint32_t rel = s_rel[k], len = s_rel[k + 1] - rel, dst = dph + rel + s_ex[k];
        for (uint32_t b = t; b < len; b += TX_T) s_out[dst + b] = s_raw[sph + rel + b];
      }
      __syncthreads();
      {  // text [c0, c1) = s_out[dph + x0, dph + x1) -> out[c0 - lo, c1 - lo)
        const uint32_t x0 = (uint32_t)(c0 - T0), m = (uint32_t)(c1 - c0);
        const uint8_t* sb = s_out + dph + x0;
        uint8_t* ob = out + (c0 - lo);
        const uint32_t head = std::min(m, (16u - ((dph + x0) & 15u)) & 15u);
        if (t < head) ob[t] = sb[t];
        const uint32_t nch = (m - head) / 16u;
        const tx_u32x4* l = reinterpret_cast<const tx_u32x4*>(sb + head);
        tx_u32x4* g = reinterpret_cast<tx_u32x4*>(ob + head);
        for (uint32_t i = t; i < nch; i += TX_T) g[i] = l[i];
        for (uint32_t p = head + 16u * nch + t; p < m; p += TX_T) ob[p] = sb[p];
      }
    } else {
      // ---- slow path: straight to global memory, every byte clipped to the slice
      for (uint32_t k = wv; k < nw; k += TX_WAVES) {
        const uint64_t wo = offs[base + k], len = offs[base + k + 1] - wo;
        const uint64_t g0 = T0 + (wo - S0) + s_ex[k];  // the line's text offset
        if (g0 >= hi || g0 + len + 22 <= lo) continue;
        if (len <= TX_BIG) {
          const uint64_t b0 = g0 < lo ? lo - g0 : 0, b1 = std::min(len, hi - g0);
          for (uint64_t b = b0 + lane; b < b1; b += 64) out[g0 + b - lo] = bytes[wo + b];
        }
        if (lane == 0) {
          uint64_t v = counts[base + k];
          const uint32_t d = tx_digits(v);
          const uint64_t q = g0 + len;
          tx_put(out, lo, hi, q, ' ');
          for (uint32_t i = d; i >= 1; i--) {
            tx_put(out, lo, hi, q + i, (uint8_t)('0' + (uint32_t)(v % 10u)));
            v /= 10u;
          }
          tx_put(out, lo, hi, q + d + 1, '\n');
        }
      }
      for (uint32_t k = 0; k < nw; k++) {
        const uint64_t wo = offs[base + k], len = offs[base + k + 1] - wo;
        if (len <= TX_BIG) continue;
        const uint64_t g0 = T0 + (wo - S0) + s_ex[k];
        if (g0 >= hi || g0 + len <= lo) continue;
        const uint64_t b0 = g0 < lo ? lo - g0 : 0, b1 = std::min(len, hi - g0);
#pragma unroll 4
        for (uint64_t b = b0 + t; b < b1; b += TX_T) out[g0 + b - lo] = bytes[wo + b];
      }
    }
    __syncthreads();  // the LDS arrays are the next tile's
  }
}

namespace {

// Where the text goes: a file (pwrite at the slice's offset) or host memory.
struct TxSink {
  int fd = -1;
  uint8_t* mem = nullptr;
  int put(const uint8_t* p, uint64_t off, uint64_t len) const {
    if (mem) {
      memcpy(mem + off, p, len);
      return MOX_OK;
    }
    while (len) {
      const ssize_t w = pwrite(fd, p, len, (off_t)off);
      if (w < 0) {
        if (errno == EINTR) continue;
        return fail(MOX_EIO, "write failed: %s", strerror(errno));
      }
      p += w;
      off += (uint64_t)w;
      len -= (uint64_t)w;
    }
    return MOX_OK;
  }
};

uint64_t slice_bytes() {
  uint64_t s = TX_SLICE;
  if (const char* v = getenv("MOX_TEXT_SLICE")) s = strtoull(v, nullptr, 10);
  s = std::max<uint64_t>(s, TX_SLICE_MIN);
  s = std::min<uint64_t>(s, 1ull << 40);
  return s & ~15ull;
}

// Everything before the text exists: pending passes, state, the sort that
// MOX_F_SORT_BYTES asks for.
int tx_prepare(mox_engine* e) {
  if (int rc = result_begin(e)) return rc;
  if ((e->flags & MOX_F_SORT_BYTES) && !e->res.sorted && !e->res.ranked) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = bsort_table(e);
    e->stats.ms_sort = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc) return rc;  // MOX_ENOMEM: the result stays in engine order, nothing is written
  }
  return MOX_OK;
}

// Tile lengths and their scan; *total = the text's length.
int tx_measure(mox_engine* e, uint64_t* total) {
  const mox_engine::Res& r = e->res;
  *total = 0;
  if (!r.n) return MOX_OK;
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  const uint64_t ntiles = (r.n + TX_TILE - 1) / TX_TILE;
  if (int rc = grow_dev(e->tx_pre, (ntiles + 1) * 8)) return rc;
  uint64_t* pre = (uint64_t*)e->tx_pre.p;
  const uint32_t lgrid = (uint32_t)std::min<uint64_t>((ntiles + TX_WAVES - 1) / TX_WAVES, 8ull * e->n_cu);
  hipLaunchKernelGGL(k_tx_len, dim3(lgrid), dim3(TX_T), 0, st, r.counts, r.offs, r.n, ntiles, pre);
  q.step("k_tx_len");
  hipLaunchKernelGGL(k_tx_scan, dim3(1), dim3(1024), 0, st, pre, ntiles);
  q.step("k_tx_scan");
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(total, pre + ntiles, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // every line has a word byte, a space, a digit and a newline; at most the word and 22 more
  if (*total < r.nb + 3 * r.n || *total > r.nb + 22 * r.n)
    return fail(MOX_EHIP, "result text: inconsistent length %llu (%llu words, %llu bytes)", (unsigned long long)*total,
                (unsigned long long)r.n, (unsigned long long)r.nb);
  return MOX_OK;
}

// The slices of a text of `total` bytes (tx_measure has run), one after
// another into the sink: slice s + 1 is emitted and copied while s is written.
int tx_stream(mox_engine* e, uint64_t total, const TxSink& sink) {
  if (!total) return MOX_OK;
  const mox_engine::Res& r = e->res;
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  const uint64_t S = slice_bytes(), ns = (total + S - 1) / S;
  const size_t cap = (size_t)std::min<uint64_t>(S, (total + 15) & ~15ull);
  for (int k = 0; k < 2; k++) {
    if (k == 1 && ns < 2) break;
    if (int rc = grow_dev(e->tx_slice[k], cap)) return rc;
    if (int rc = grow_pinned(e->tx_pin[k], cap)) return rc;
    if (!e->tx_ev[k]) HIPCHK(hipEventCreateWithFlags(&e->tx_ev[k], hipEventDisableTiming));
  }
  const uint64_t ntiles = (r.n + TX_TILE - 1) / TX_TILE;
  // a slice reaches into at most S / (3 TX_TILE) + 3 tiles (only the table's last tile has fewer than TX_TILE lines)
  const uint32_t grid = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(ntiles, S / (3 * TX_TILE) + 3), 8ull * e->n_cu);
  auto issue = [&](uint64_t s) -> int {
    const uint64_t lo = s * S, hi = std::min(total, lo + S);
    const int k = (int)(s & 1);
    hipLaunchKernelGGL(k_tx_emit, dim3(grid), dim3(TX_T), 0, st, r.counts, r.offs, r.bytes, r.n, ntiles,
                       (const uint64_t*)e->tx_pre.p, lo, hi, (uint8_t*)e->tx_slice[k].p);
    q.step("k_tx_emit");
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->tx_pin[k].p, e->tx_slice[k].p, hi - lo, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(e->tx_ev[k], st));
    return MOX_OK;
  };
  int rc = issue(0);
  for (uint64_t s = 0; s < ns && !rc; s++) {
    if (s + 1 < ns) rc = issue(s + 1);  // its pinned buffer held slice s - 1, written below one turn ago
    if (rc) break;
    const int k = (int)(s & 1);
    const hipError_t er = hipEventSynchronize(e->tx_ev[k]);
    if (er != hipSuccess) {
      rc = fail(MOX_EHIP, "result text: slice %llu failed: %s", (unsigned long long)s, hipGetErrorString(er));
      break;
    }
    const uint64_t lo = s * S;
    rc = sink.put((const uint8_t*)e->tx_pin[k].p, lo, std::min(total, lo + S) - lo);
  }
  if (rc) {
    const std::string msg = g_err;
    (void)hipStreamSynchronize(st);  // nothing of this call stays queued behind an error
    g_err = msg;
  }
  return rc;
}

}  // namespace

extern "C" int mox_write_result(mox_engine* e, const char* path) {
  if (!e || !path) return fail(MOX_EINVAL, "NULL argument");
  if (int rc = tx_prepare(e)) return rc;
  const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (fd < 0) return fail(MOX_EIO, "cannot open %s: %s", path, strerror(errno));
  uint64_t total = 0;
  int rc = tx_measure(e, &total);
  if (!rc) {
    TxSink sink;
    sink.fd = fd;
    rc = tx_stream(e, total, sink);
  }
  if (close(fd) != 0 && !rc) rc = fail(MOX_EIO, "close failed: %s", strerror(errno));
  return rc;
}

extern "C" int mox_result_text(mox_engine* e, uint8_t** text, uint64_t* len) {
  if (!e || !text || !len) return fail(MOX_EINVAL, "NULL argument");
  *text = nullptr;
  *len = 0;
  if (int rc = tx_prepare(e)) return rc;
  uint64_t total = 0;
  if (int rc = tx_measure(e, &total)) return rc;
  uint8_t* mem = (uint8_t*)malloc(total ? total : 1);
  if (!mem) return fail(MOX_ENOMEM, "host allocation of %llu bytes failed", (unsigned long long)total);
  TxSink sink;
  sink.mem = mem;
  if (int rc = tx_stream(e, total, sink)) {
    free(mem);
    return rc;
  }
  *text = mem;
  *len = total;
  return MOX_OK;
}

extern "C" void mox_text_free(uint8_t* text) { free(text); }
