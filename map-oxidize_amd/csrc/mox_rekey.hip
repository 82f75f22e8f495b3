// Device re-keying (mox_rekey_result): every word of the device-resident
// result is replaced by a byte window of itself -- ASCII bytes of a set stripped
// from both ends, then a cap of max_chars characters -- and the rows whose
// windows are equal are summed, all on the GPU ("Re-keying the
// result").  "the", "the,", "(the)" and "the." become one row without the table
// ever reaching the host.
//
// It is the accumulator's pipeline (mox_accum.hip) with one source and a window
// per row: the table is packed into the exchange's receive layout for P = 1
// source in x_recv_short / x_recv_blob, and reduce_received (mox_multi.hip),
// the reduce-only pass of the exchange, of mox_reduce_pairs and of
// mox_accumulate, runs over it unchanged, k_reduce_z for zero counts included.
//
// The window of a row (o, len), by one lane (rq_window): leading bytes are
// dropped while they are < 128 and in the set, then trailing ones; the trailing
// walk stops at the window's start, so it never reads before the word's first
// byte.  With a cap K the window ends before its (K + 1)-th character start (a
// byte b with (b & 0xC0) != 0x80); a window of at most K bytes has at most K
// starts and is not walked.  The walks are serial, one byte per step: a
// 100,000-byte word of dashes costs its lane 100,000 steps, as a long word's
// hash already does.  A windowed row is classified by reduce_pairs_impl's rule
// (1..16 bytes without a NUL byte -> a zero-padded WRec; every other -> an
// XHdr{fnv_finish(h), length, count, offset} with h the map's FNV-1a-64, which
// mox_exchange picks owners by, plus the bytes padded to 8); an empty window
// drops the row.  Tiles of RQ_TILE consecutive rows, one workgroup per tile,
// grid-stride:
//
//  1. k_rekey_count: per tile its short rows, long rows and padded long bytes,
//     and the rows changed, the rows dropped and the counts dropped.
//  2. k_rekey_scan (one workgroup): exclusive scans of the first three tile
//     arrays, the six totals behind them.  One 48-byte copy to the host sizes
//     the wire buffers exactly and decides the no-op path (no row changed:
//     nothing else runs).
//  3. k_rekey_pack: every kept row's record at its scanned position, as
//     k_ac_pack places them: a row's rank among the tile's short / long rows is
//     a ballot rank inside its wave plus the wave totals before it (LDS), a
//     long word's byte offset a wave scan of the padded lengths.  No global
//     atomic decides a position, so the wire image is a pure function of the
//     table and the spec.  Long windows up to RQ_COOP bytes are hashed and
//     copied by their lane; longer ones are listed in LDS and taken by whole
//     waves afterwards (64 consecutive 8-byte words per step, the hash walking
//     them lane by lane), every lane of the wave computing the window again.
//     A short windowed row with count 0 raises the flag behind the totals: the
//     reduce pass then takes k_reduce_z.
//
// Key and word loads (mox_pack.h): as in the accumulator they are aligned
// 8-byte loads from the start's word on, up to 23 bytes past the start, but the
// start is the window's, which lies inside the word (a kept window has at least
// one byte).  It is therefore no later than the word's last byte, and the slack
// contract (mox_dev.h) still covers the over-read: no load leaves its
// allocation.  What is read past a window is masked by the window's length
// before the NUL test, the hash and every store.  The window walks read single
// bytes of the word.
//
// What the two packers have in common is in mox_pack.h, forced inline: the
// short-row classifier (pk_short), a round's ranks (pk_ranks; the table view
// and the scan are mox_tiles.h's TileTab and scan_tiles) and the copy +
// hash of a long word by one lane and by a whole wave (pk_long_lane,
// pk_long_wave); they take a byte range, so a window is an argument and nothing
// else.  What differs stays here and is no template over a "row window": the
// count kernel sums six values instead of three, the pack kernel drops rows and
// its wave pass derives the window again, and a shared body would carry the
// window through k_ac_pack's LDS list and registers.  So mox_accum.hip is
// untouched by the window, and its kernels and this file's compile to the
// resource usage they had with the pieces written out (profiles/pack/README.md).
//
// Resource usage (hipcc of ROCm 7.2.0: HIP 7.2.26015, AMD clang 22.0.0git
// roc-7.2.0; the Makefile's flags, -Rpass-analysis=kernel-resource-usage):
//   k_rekey_count  56 VGPRs,  65 SGPRs,   192 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_rekey_scan   55 VGPRs,  72 SGPRs,   768 B LDS, no scratch, no spills (one workgroup)
//   k_rekey_pack   84 VGPRs, 106 SGPRs, 12392 B LDS, no scratch, no spills (5 waves / SIMD)
#include <algorithm>
#include <cstdlib>

#include "mox_host.h"
#include "mox_pack.h"

namespace {

constexpr int RQ_T = 256;                    // threads of k_rekey_count / k_rekey_pack
constexpr int RQ_WAVES = RQ_T / 64;
constexpr int RQ_PER = 4;                    // rows per thread and tile
constexpr uint32_t RQ_TILE = RQ_T * RQ_PER;  // rows per tile (tests/rekey_cases.py TILE)
constexpr uint32_t RQ_COOP = 256;            // a longer long window is copied by a whole wave
constexpr int RQ_SCAN_PER = 4;               // k_rekey_scan: consecutive tiles per thread ...
constexpr uint32_t RQ_SCAN_STEP = 1024 * RQ_SCAN_PER;  // ... and tiles per step of its one workgroup
static_assert(RQ_TILE == 1024, "tests/rekey_cases.py TILE");
static_assert(RQ_SCAN_STEP == 4096, "tests/test_gpu_big_table.py REKEY_SCAN_STEP");
static_assert(RQ_TILE <= 65536, "s_big_k and s_big_r hold 16-bit rows");
static_assert(sizeof(mox_rekey) == 64 && sizeof(mox_rekey_info) == 112, "include/mox.h");

// The spec as the kernels take it: the effective set, the cap (0: none).
struct RqSpec {
  uint64_t set0, set1, max_chars;
};
// Where the records go: WRecs from shorts[0], headers from blob, the word bytes behind the nlong headers.
struct RqOut {
  mox::WRec* shorts;
  uint8_t* blob;
  uint64_t nlong;
};

__device__ __forceinline__ bool rq_trims(const RqSpec& P, uint32_t b) {
  return b < 128u && (((b < 64u ? P.set0 : P.set1) >> (b & 63u)) & 1ull);
}

// The window [ws, ws + wl) of the word [o, o + len): see the file header.
__device__ __forceinline__ void rq_window(const uint8_t* bytes, uint64_t o, uint64_t len, const RqSpec& P, uint64_t& ws, uint64_t& wl) {
  uint64_t s = o, e = o + len;
  for (; s < e && rq_trims(P, bytes[s]); s++) {}
  for (; e > s && rq_trims(P, bytes[e - 1]); e--) {}
  if (P.max_chars && e - s > P.max_chars) {
    uint64_t starts = 0, p = s;
    for (; p < e; p++)
      if ((bytes[p] & 0xC0u) != 0x80u) {
        if (starts == P.max_chars) break;
        starts++;
      }
    e = p;
  }
  ws = s;
  wl = e - s;
}

}  // namespace

// tc[k * nt + tile], k = 0: short rows, 1: long rows, 2: padded long bytes, 3:
// rows whose window is not the whole word, 4: rows dropped, 5: counts dropped
// (summed as u64) of the tile.
extern "C" __global__ __launch_bounds__(RQ_T) void k_rekey_count(TileTab T, RqSpec P, uint64_t* __restrict__ tc) {
  __shared__ uint64_t s_w[RQ_WAVES][6];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (uint64_t tile = blockIdx.x; tile < T.nt; tile += gridDim.x) {
    const uint64_t base = tile * RQ_TILE;
    uint64_t ns = 0, nl = 0, lb = 0, nc = 0, nd = 0, td = 0;
    for (int j = 0; j < RQ_PER; j++) {
      const uint64_t i = base + (uint32_t)j * RQ_T + t;
      if (i < T.n) {
        const uint64_t o = __builtin_nontemporal_load(T.offs + i), len = __builtin_nontemporal_load(T.offs + i + 1) - o;
        uint64_t ws, wl, k0, k1;
        rq_window(T.bytes, o, len, P, ws, wl);
        if (wl == 0) {
          nc++;
          nd++;
          td += __builtin_nontemporal_load(T.counts + i);
        } else {
          nc += wl != len;
          if (pk_short(T.bytes, ws, wl, k0, k1)) {
            ns++;
          } else {
            nl++;
            lb += (wl + 7) & ~7ull;
          }
        }
      }
    }
    ns = wave_sum(ns);
    nl = wave_sum(nl);
    lb = wave_sum(lb);
    nc = wave_sum(nc);
    nd = wave_sum(nd);
    td = wave_sum(td);
    if (lane == 0) {
      s_w[wv][0] = ns;
      s_w[wv][1] = nl;
      s_w[wv][2] = lb;
      s_w[wv][3] = nc;
      s_w[wv][4] = nd;
      s_w[wv][5] = td;
    }
    __syncthreads();
    if (t < 6) {
      uint64_t v = 0;
      for (int k = 0; k < RQ_WAVES; k++) v += s_w[k][t];
      tc[(uint64_t)t * T.nt + tile] = v;
    }
    __syncthreads();
  }
}

// Exclusive scans in place of the first three tile arrays (mox_tiles.h:
// scan_tiles, RQ_SCAN_STEP tiles per step of the one workgroup), plain sums of
// the other three; the six totals at tc[6 nt + k].  Also clears the word behind
// the totals, k_rekey_pack's zero-count flag.
extern "C" __global__ __launch_bounds__(1024) void k_rekey_scan(uint64_t* tc, uint64_t nt) {
  scan_tiles<3, RQ_SCAN_PER, 1024>(tc, nt, tc + 6 * nt);
  uint64_t sum3 = 0, sum4 = 0, sum5 = 0;
  for (uint64_t i = threadIdx.x; i < nt; i += 1024) {  // (after the scans: their registers are free)
    sum3 += tc[3 * nt + i];
    sum4 += tc[4 * nt + i];
    sum5 += tc[5 * nt + i];
  }
  tile_sums<3, 16>({sum3, sum4, sum5}, tc + 6 * nt + 3, 1, 0);  // the three totals side by side
  if (threadIdx.x == 0) tc[6 * nt + 6] = 0;  // k_rekey_pack's flag: a short windowed row with count 0
}

// Every kept row's record at its scanned position (tc: k_rekey_scan's output).
// tc[6 nt + 6] is set when a short windowed row has count 0 (such records need
// the reduce pass's k_reduce_z; mox_kernels.hip).
extern "C" __global__ __launch_bounds__(RQ_T) void k_rekey_pack(TileTab T, RqSpec P, uint64_t* __restrict__ tc, RqOut out) {
  __shared__ uint64_t s_big_b[RQ_TILE];   // long windows over RQ_COOP bytes: byte offset in the blob's word area,
  __shared__ uint16_t s_big_k[RQ_TILE];   // ... row inside the tile
  __shared__ uint16_t s_big_r[RQ_TILE];   // ... and header rank inside the tile
  __shared__ uint32_t s_nbig;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t nt = T.nt;
  mox::XHdr* const H0 = reinterpret_cast<mox::XHdr*>(out.blob);
  uint8_t* const area = out.blob + out.nlong * sizeof(mox::XHdr);
  for (uint64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const uint64_t base = tile * RQ_TILE;
    mox::WRec* S = out.shorts + tc[tile];
    mox::XHdr* H = H0 + tc[nt + tile];
    PkAt run{0, 0, tc[2 * nt + tile]};  // running short rank, long rank, byte offset
    if (t == 0) s_nbig = 0;
    for (int j = 0; j < RQ_PER; j++) {
      const uint64_t i = base + (uint32_t)j * RQ_T + t;
      uint64_t ws = 0, wl = 0, cnt = 0, k0 = 0, k1 = 0;
      bool is_s = false, is_l = false;
      if (i < T.n) {
        const uint64_t o = __builtin_nontemporal_load(T.offs + i), len = __builtin_nontemporal_load(T.offs + i + 1) - o;
        cnt = __builtin_nontemporal_load(T.counts + i);
        rq_window(T.bytes, o, len, P, ws, wl);
        if (wl) {  // (an empty window: the row is dropped)
          is_s = pk_short(T.bytes, ws, wl, k0, k1);
          is_l = !is_s;
        }
      }
      if (__ballot(is_s && cnt == 0) && lane == 0) tc[6 * nt + 6] = 1;
      const PkAt at = pk_ranks<RQ_WAVES>(is_s, is_l, is_l ? (wl + 7) & ~7ull : 0ull, run);
      if (is_s) {
        S[at.s] = mox::WRec{k0, k1, cnt};
      } else if (is_l) {
        if (wl <= RQ_COOP) {  // this lane
          H[at.l] = mox::XHdr{pk_long_lane(T.bytes, ws, wl, area + at.b), wl, cnt, at.b};
        } else {  // a whole wave below, which also writes the header
          const uint32_t x = atomicAdd(&s_nbig, 1u);
          s_big_b[x] = at.b;
          s_big_k[x] = (uint16_t)((uint32_t)j * RQ_T + t);
          s_big_r[x] = (uint16_t)at.l;  // at.l < RQ_TILE
        }
      }
    }
    __syncthreads();
    // long windows over RQ_COOP bytes: one wave each (every lane derives the same window)
    const uint32_t nbig = s_nbig;
    for (uint32_t x = wv; x < nbig; x += RQ_WAVES) {
      const uint64_t i = base + s_big_k[x];
      const uint64_t o = T.offs[i];
      uint64_t ws, wl;
      rq_window(T.bytes, o, T.offs[i + 1] - o, P, ws, wl);
      const uint64_t h = pk_long_wave(T.bytes, ws, wl, area + s_big_b[x]);
      if (lane == 0) H[s_big_r[x]] = mox::XHdr{h, wl, T.counts[i], s_big_b[x]};
    }
    __syncthreads();  // the LDS arrays are the next tile's
  }
}

extern "C" int mox_rekey_result(mox_engine* e, const mox_rekey* k, mox_rekey_info* info) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  if (!k) return fail(MOX_EINVAL, "rekey: the spec is NULL");
  if (k->flags & ~MOX_REKEY_TRIM_ASCII_PUNCT) return fail(MOX_EINVAL, "rekey: unknown flags 0x%x", k->flags);
  if (k->pad) return fail(MOX_EINVAL, "rekey: pad is not 0");
  for (uint64_t r : k->reserved)
    if (r) return fail(MOX_EINVAL, "rekey: a reserved word is not 0");
  if (int rc = result_begin(e)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const mox_engine::Res r = e->res;
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  int rc;
  RqSpec P{k->trim_set[0], k->trim_set[1], k->max_chars};
  if (k->flags & MOX_REKEY_TRIM_ASCII_PUNCT) {
    P.set0 |= MOX_REKEY_PUNCT_LO;
    P.set1 |= MOX_REKEY_PUNCT_HI;
  }
  const TileTab T = tile_tab(r, RQ_TILE);
  const uint64_t nt = T.nt;
  if ((rc = grow_dev(e->q_tc, (6 * nt + 8) * 8))) return rc;
  uint64_t* tc = (uint64_t*)e->q_tc.p;
  uint64_t* tot = e->h_tot;  // short rows, long rows, padded long bytes, rows changed, rows dropped, counts dropped, zero flag
  for (int i = 0; i < 7; i++) tot[i] = 0;
  const uint32_t grid = (uint32_t)std::min(nt, grid_cap(e, "MOX_REKEY_GRID"));
  if (nt) {
    hipLaunchKernelGGL(k_rekey_count, dim3(grid), dim3(RQ_T), 0, st, T, P, tc);
    q.step("k_rekey_count");
    hipLaunchKernelGGL(k_rekey_scan, dim3(1), dim3(1024), 0, st, tc, nt);
    q.step("k_rekey_scan");
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(tot, tc + 6 * nt, 48, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (tot[0] + tot[1] + tot[4] != r.n || tot[2] > r.nb + 8 * r.n || tot[3] > r.n || tot[4] > tot[3])
    return fail(MOX_EHIP, "rekey: inconsistent totals (%llu + %llu + %llu of %llu rows, %llu changed, %llu bytes of %llu)",
                (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)tot[4], (unsigned long long)r.n,
                (unsigned long long)tot[3], (unsigned long long)tot[2], (unsigned long long)r.nb);
  mox_rekey_info ki{};
  ki.words_in = r.n;
  ki.words_changed = tot[3];
  ki.words_dropped = tot[4];
  ki.tokens_in = r.tokens;
  ki.tokens_dropped = tot[5];
  ki.tokens_out = r.tokens - tot[5];
  auto finish = [&]() {
    ki.words_out = e->res.n;
    ki.bytes_out = e->res.nb;
    ki.device_bytes = e->q_tc.cap + e->x_recv_short.cap + e->x_recv_blob.cap;
    ki.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = ki;
    return MOX_OK;
  };
  if (!tot[3]) return finish();  // every window is its whole word: the result, its order and its flags stay
  Received rx = received_one(tot[0], tot[1], tot[2], false);
  if ((rc = received_reserve(e, rx))) return rc;
  const RqOut out{(WRec*)e->x_recv_short.p, (uint8_t*)e->x_recv_blob.p, rx.r_long};
  hipLaunchKernelGGL(k_rekey_pack, dim3(grid), dim3(RQ_T), 0, st, T, P, tc, out);
  q.step("k_rekey_pack");
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(tot + 6, tc + 6 * nt + 6, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // the table is packed: from here on its buffers may go
  if (test_fail_hook("MOX_TEST_FAIL_REKEY"))
    return fail(MOX_ENOMEM, "rekey: injected failure before the reduce pass (MOX_TEST_FAIL_REKEY)");
  rx.zero = tot[6] != 0;  // a short windowed row with count 0: k_reduce_z
  if ((rc = reduce_received(e, rx, packed_stats(e, rx), t0))) return rc;  // no result is left, as after a failed mox_reduce_pairs; the accumulator is intact
  // a reduce pass's table (set_result); a total that was folded stays folded
  e->res.folded = r.folded;
  e->res.tokens = ki.tokens_out;
  return finish();
}
