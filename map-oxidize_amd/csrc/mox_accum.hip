// Device-resident accumulation (mox_accumulate / mox_accumulate_file): the
// engine's result table is folded into a running total on the GPU, so windows,
// chunks of a file and whole files add up without a table ever reaching the
// host ("Accumulating results").
//
// The total is a saved table: (counts, offs, bytes) in buffers of its own
// (a_tab: counts, offs, bytes), copied device to device from the result after
// every fold.  A fold is total := reduce(total rows ++ result rows): both
// tables are packed into the exchange's receive layout for P = 2 sources
// (source 0 the total, source 1 the result) in x_recv_short / x_recv_blob, and
// reduce_received (mox_multi.hip), the reduce-only pass of the exchange and of
// mox_reduce_pairs, runs over them unchanged.
//
// The packer takes a table in generic form (counts, offs, bytes, n): any
// result, whatever buffers mox_engine::Res points at and whatever its order
// (engine order, sorted, gathered), so short and long rows may interleave.  A
// row is classified from its bytes, by reduce_pairs_impl's rule: 1..16 bytes
// without a NUL byte -> a zero-padded WRec; every other row -> an XHdr (the
// FNV-1a-64 of its bytes through fnv_finish, length, count, offset) plus its
// bytes, padded to 8, in its source's blob.  Tiles of AC_TILE consecutive rows
// (one workgroup per tile), tiles of source 0 first:
//
//  1. k_ac_count: per tile its short rows, long rows and padded long bytes.
//  2. k_ac_scan (one workgroup): exclusive scans of the three tile arrays,
//     separately per source, the six totals behind them.  One 48-byte copy to
//     the host sizes the wire buffers and the reduce pass's Caps exactly.
//  3. k_ac_pack: every record at its scanned position.  Rows are taken in row
//     order (256 at a time); a row's rank among the tile's short / long rows
//     is a ballot rank inside its wave plus the wave totals before it (LDS), and
//     a long word's byte offset a wave scan of the padded lengths: positions
//     are deterministic and there is no global atomic anywhere.  Long words up
//     to AC_COOP bytes are hashed and copied by their lane; longer ones are
//     listed in LDS and taken by whole waves afterwards, 64 consecutive 8-byte
//     words per step.  The hash has to be the map's own (k_map's long lane),
//     not merely some function of the bytes: after a fold the merge pass's
//     long table feeds mox_exchange, which picks a long word's owner rank by
//     this hash on every rank (mox_internal.h: fnv_step).
//
// The classifier, a round's ranks and both forms of the long-word copy + hash
// are mox_pack.h's (pk_short, pk_ranks, pk_long_lane, pk_long_wave), which the
// re-keying packer (mox_rekey.hip) uses too; the table view and the end of the
// count kernel are mox_tiles.h's (TileTab, tile_sums); the sums themselves, the
// scan, the LDS list of big words and the tile loop are this file's.
//
// Key loads (mox_pack.h has the detail): the 16 key bytes of a row at byte
// offset o come from three aligned 8-byte loads at o & ~7 and a funnel shift,
// so they read up to 23 bytes past o; a long word's copy reads whole 8-byte
// words the same way.  That is inside the slack of every bytes buffer a result
// can live in (mox_dev.h: the slack contract), so no load leaves its
// allocation and none is clamped.  What is read past a word is masked by the
// word's length before the NUL test, the hash and every store.
// A zero-length row (no result holds one) loads nothing: it becomes a header
// with no bytes.
//
// Resource usage (hipcc of ROCm 7.2.0: HIP 7.2.26015, AMD clang 22.0.0git
// roc-7.2.0; the Makefile's flags, -Rpass-analysis=kernel-resource-usage):
//   k_ac_count  38 VGPRs,  55 SGPRs,    96 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_ac_scan   92 VGPRs,  76 SGPRs,   128 B LDS, no scratch, no spills (one workgroup)
//   k_ac_pack   86 VGPRs, 106 SGPRs, 12392 B LDS, no scratch, no spills (5 waves / SIMD)
#include <algorithm>
#include <cerrno>
#include <cstdlib>

#include "mox_host.h"
#include "mox_pack.h"

namespace {

constexpr int AC_T = 256;                  // threads of k_ac_count / k_ac_pack
constexpr int AC_WAVES = AC_T / 64;
constexpr int AC_PER = 4;                  // rows per thread and tile
constexpr uint32_t AC_TILE = AC_T * AC_PER;  // rows per tile (tests/accum_cases.py TILE)
constexpr uint32_t AC_COOP = 256;          // a longer long word is copied by a whole wave
static_assert(AC_TILE == 1024, "tests/accum_cases.py TILE");

// Where the records go: source s's WRecs from shorts[sbase[s]], its headers at
// blob + bbase[s], its word bytes behind its nlong[s] headers.
struct AcOut {
  mox::WRec* shorts;
  uint8_t* blob;
  uint64_t sbase[2], bbase[2], nlong[2];
};

}  // namespace

// tc[0 * nt + tile] = short rows, tc[1 * nt + tile] = long rows, tc[2 * nt +
// tile] = padded long bytes of the tile; nt = a.nt + b.nt.
extern "C" __global__ __launch_bounds__(AC_T) void k_ac_count(TileTab a, TileTab b, uint64_t* tc) {
  const uint32_t t = threadIdx.x;
  const uint64_t nt = a.nt + b.nt;
  for (uint64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const bool first = tile < a.nt;
    const TileTab& s = first ? a : b;
    const uint64_t base = (first ? tile : tile - a.nt) * AC_TILE;
    uint64_t ns = 0, nl = 0, lb = 0;
#pragma unroll
    for (int j = 0; j < AC_PER; j++) {
      const uint64_t i = base + (uint32_t)j * AC_T + t;
      if (i < s.n) {
        const uint64_t o = __builtin_nontemporal_load(s.offs + i), len = __builtin_nontemporal_load(s.offs + i + 1) - o;
        uint64_t k0, k1;
        if (pk_short(s.bytes, o, len, k0, k1)) {
          ns++;
        } else {
          nl++;
          lb += (len + 7) & ~7ull;
        }
      }
    }
    tile_sums<3, AC_WAVES>({ns, nl, lb}, tc, nt, tile);
  }
}

// Exclusive scans in place of the three tile arrays, each in two segments
// (source 0's tiles [0, nt0), source 1's [nt0, nt0 + nt1)); the totals at
// tc[3 nt + 3 s + k], k = short rows, long rows, long bytes of source s.  One
// workgroup (mox_dev.h: scan_one_wg).  Also clears the word behind the totals,
// k_ac_pack's zero-count flag.
extern "C" __global__ __launch_bounds__(1024) void k_ac_scan(uint64_t* tc, uint64_t nt0, uint64_t nt1) {
  const uint64_t nt = nt0 + nt1;
  for (int k = 0; k < 3; k++)
    for (int s = 0; s < 2; s++) scan_one_wg<uint64_t, 1024>(tc + (uint64_t)k * nt + (s ? nt0 : 0), s ? nt1 : nt0, tc + 3 * nt + 3 * s + k);
  if (threadIdx.x == 0) tc[3 * nt + 6] = 0;  // k_ac_pack's flag: a short row with count 0
}

// Every row of both tables at its scanned position (tc: k_ac_scan's output).
// tc[3 nt + 6] is set when a short row has count 0 (such records need the
// reduce pass's k_reduce_z; mox_kernels.hip).
extern "C" __global__ __launch_bounds__(AC_T) void k_ac_pack(TileTab a, TileTab b, uint64_t* __restrict__ tc, AcOut out) {
  __shared__ uint64_t s_big_b[AC_TILE];   // long words over AC_COOP bytes: byte offset in the source's blob area,
  __shared__ uint16_t s_big_k[AC_TILE];   // ... row inside the tile
  __shared__ uint16_t s_big_r[AC_TILE];   // ... and header rank inside the tile
  __shared__ uint32_t s_nbig;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t nt = a.nt + b.nt;
  for (uint64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const bool first = tile < a.nt;
    const TileTab& s = first ? a : b;
    const int si = first ? 0 : 1;
    const uint64_t base = (first ? tile : tile - a.nt) * AC_TILE;
    mox::WRec* S = out.shorts + out.sbase[si] + tc[tile];
    mox::XHdr* H = reinterpret_cast<mox::XHdr*>(out.blob + out.bbase[si]) + tc[nt + tile];
    uint8_t* area = out.blob + out.bbase[si] + out.nlong[si] * sizeof(mox::XHdr);
    PkAt run{0, 0, tc[2 * nt + tile]};  // running short rank, long rank, byte offset
    if (t == 0) s_nbig = 0;
    for (int j = 0; j < AC_PER; j++) {
      const uint64_t i = base + (uint32_t)j * AC_T + t;
      uint64_t o = 0, len = 0, cnt = 0, k0 = 0, k1 = 0;
      bool is_s = false, is_l = false;
      if (i < s.n) {
        o = __builtin_nontemporal_load(s.offs + i);
        len = __builtin_nontemporal_load(s.offs + i + 1) - o;
        cnt = __builtin_nontemporal_load(s.counts + i);
        is_s = pk_short(s.bytes, o, len, k0, k1);
        is_l = !is_s;
      }
      if (__ballot(is_s && cnt == 0) && lane == 0) tc[3 * nt + 6] = 1;
      const PkAt at = pk_ranks<AC_WAVES>(is_s, is_l, is_l ? (len + 7) & ~7ull : 0ull, run);
      if (is_s) {
        S[at.s] = mox::WRec{k0, k1, cnt};
      } else if (is_l) {
        if (len <= AC_COOP) {  // this lane
          H[at.l] = mox::XHdr{pk_long_lane(s.bytes, o, len, area + at.b), len, cnt, at.b};
        } else {  // a whole wave below, which also writes the header
          const uint32_t x = atomicAdd(&s_nbig, 1u);
          s_big_b[x] = at.b;
          s_big_k[x] = (uint16_t)((uint32_t)j * AC_T + t);
          s_big_r[x] = (uint16_t)at.l;  // at.l < AC_TILE
        }
      }
    }
    __syncthreads();
    // long words over AC_COOP bytes: one wave each
    const uint32_t nbig = s_nbig;
    for (uint32_t x = wv; x < nbig; x += AC_WAVES) {
      const uint64_t i = base + s_big_k[x];
      const uint64_t o = s.offs[i], len = s.offs[i + 1] - o;
      const uint64_t h = pk_long_wave(s.bytes, o, len, area + s_big_b[x]);
      if (lane == 0) H[s_big_r[x]] = mox::XHdr{h, len, s.counts[i], s_big_b[x]};
    }
    __syncthreads();  // the LDS arrays are the next tile's
  }
}

namespace {

// The engine's result becomes the saved total (after a failed fold, and where
// nothing else is left of the result).
void acc_as_result(mox_engine* e) {
  mox_engine::Res& r = e->res;
  res_point_at(r, e->a_tab, e->acc.n, e->acc.nb, e->acc.tokens);
  r.sorted = e->acc.sorted;
  r.ranked = e->acc.ranked;
  r.folded = true;
  e->have_result = true;
}

// total := the engine's result (device to device), into buffers dst[0..2] that hold it.
int acc_save(mox_engine* e, DevBuf* dst) {
  const mox_engine::Res& r = e->res;
  hipStream_t s = e->stream;
  if (r.n) {
    HIPCHK(hipMemcpyAsync(dst[0].p, r.counts, 8 * r.n, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(dst[1].p, r.offs, 8 * (r.n + 1), hipMemcpyDeviceToDevice, s));
    if (r.nb) HIPCHK(hipMemcpyAsync(dst[2].p, r.bytes, r.nb, hipMemcpyDeviceToDevice, s));
  } else {
    HIPCHK(hipMemsetAsync(dst[1].p, 0, 8, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return MOX_OK;
}

void acc_commit(mox_engine* e, uint64_t passes) {
  e->acc.have = true;
  e->acc.n = e->res.n;
  e->acc.nb = e->res.nb;
  e->acc.tokens = e->res.tokens;
  e->acc.sorted = e->res.sorted;
  e->acc.ranked = e->res.ranked;
  e->acc.passes = passes;
  e->res.folded = true;
}

// Both tables into x_recv_short / x_recv_blob, then the reduce pass; fresh[0..2]
// receive the new total's buffers where the old ones are too small (allocated
// before the reduce pass, so that nothing can fail after it).
int acc_merge(mox_engine* e, DevBuf* fresh, bool* use_fresh) {
  const auto t0 = std::chrono::steady_clock::now();
  const mox_engine::Res& r = e->res;
  const TileTab ta = tile_tab((const uint64_t*)e->a_tab[0].p, (const uint64_t*)e->a_tab[1].p, (const uint8_t*)e->a_tab[2].p, e->acc.n, AC_TILE);
  const TileTab tb = tile_tab(r, AC_TILE);
  const uint64_t nt = ta.nt + tb.nt;
  hipStream_t s = e->stream;
  const Seq q = seq_of(e);
  int rc;
  uint64_t* tot = e->h_tot;
  for (int k = 0; k < 7; k++) tot[k] = 0;
  if ((rc = grow_dev(e->a_tc, (3 * nt + 8) * 8))) return rc;
  uint64_t* tc = (uint64_t*)e->a_tc.p;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(nt, 8ull * e->n_cu);
  if (nt) {
    hipLaunchKernelGGL(k_ac_count, dim3(grid), dim3(AC_T), 0, s, ta, tb, tc);
    q.step("k_ac_count");
    hipLaunchKernelGGL(k_ac_scan, dim3(1), dim3(1024), 0, s, tc, ta.nt, tb.nt);
    q.step("k_ac_scan");
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(tot, tc + 3 * nt, 48, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  // tot[3 s + k]: short rows, long rows, padded long bytes of source s
  if (tot[0] + tot[1] != ta.n || tot[3] + tot[4] != tb.n || tot[2] > e->acc.nb + 8 * ta.n || tot[5] > r.nb + 8 * tb.n)
    return fail(MOX_EHIP, "accumulate: inconsistent row counts (%llu + %llu of %llu, %llu + %llu of %llu)",
                (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)ta.n, (unsigned long long)tot[3],
                (unsigned long long)tot[4], (unsigned long long)tb.n);
  Received rx;
  rx.dir.P = 2;
  AcOut out{};
  for (int k = 0; k < 2; k++) {
    out.sbase[k] = rx.rs;
    out.bbase[k] = rx.dir.blob[k] = rx.rb;
    out.nlong[k] = rx.dir.nlong[k] = tot[3 * k + 1];
    rx.dir.hpre[k] = rx.r_long;
    rx.rs += tot[3 * k];
    rx.r_long += tot[3 * k + 1];
    rx.rb += tot[3 * k + 1] * sizeof(XHdr) + tot[3 * k + 2];
  }
  rx.dir.blob[2] = rx.rb;
  rx.dir.hpre[2] = rx.r_long;
  if ((rc = received_reserve(e, rx))) return rc;
  out.shorts = (WRec*)e->x_recv_short.p;
  out.blob = (uint8_t*)e->x_recv_blob.p;
  if (nt) {
    hipLaunchKernelGGL(k_ac_pack, dim3(grid), dim3(AC_T), 0, s, ta, tb, tc, out);
    q.step("k_ac_pack");
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(tot + 6, tc + 3 * nt + 6, 8, hipMemcpyDeviceToHost, s));  // completed by the synchronisation below
  }
  // the new total has at most the rows and bytes of both tables
  const uint64_t un = ta.n + tb.n, ub = e->acc.nb + r.nb;
  *use_fresh = e->a_tab[0].cap < 8 * un + TABLE_SLACK || e->a_tab[1].cap < 8 * (un + 1) + TABLE_SLACK || e->a_tab[2].cap < ub + TABLE_SLACK;
  if (*use_fresh && (rc = table_reserve(fresh[0], fresh[1], fresh[2], un, ub))) return rc;
  HIPCHK(hipStreamSynchronize(s));  // both sources are packed: from here on the run's buffers may go
  if (test_fail_hook("MOX_TEST_FAIL_ACCUM"))
    return fail(MOX_ENOMEM, "accumulate: injected failure before the reduce pass (MOX_TEST_FAIL_ACCUM)");
  rx.zero = tot[6] != 0;  // a short word with count 0 in either table: k_reduce_z
  return reduce_received(e, rx, packed_stats(e, rx), t0);
}

int accumulate_impl(mox_engine* e) {
  if (int rc = drain_async(e)) return rc;
  if (!e->have_result) return fail(MOX_ESTATE, "no result to accumulate: run first");
  if (e->res.folded) return fail(MOX_ESTATE, "the result is already part of the total: run again first");
  HIPCHK(hipSetDevice(e->device));
  DevBuf* cur = e->a_tab;
  if (!e->acc.have) {
    // an empty total: the result is saved as it is and stays the pass's own table
    if (int rc = table_reserve(cur[0], cur[1], cur[2], e->res.n, e->res.nb)) return rc;
    if (int rc = acc_save(e, cur)) return rc;
    acc_commit(e, 1);
    return MOX_OK;
  }
  DevBuf fresh[3];
  bool use_fresh = false;
  int rc = acc_merge(e, fresh, &use_fresh);
  if (!rc) {
    rc = acc_save(e, use_fresh ? fresh : cur);
    if (!rc) {
      if (use_fresh)
        for (int k = 0; k < 3; k++) {
          dfree(cur[k].p);
          cur[k] = fresh[k];
          fresh[k] = DevBuf{};
        }
      acc_commit(e, e->acc.passes + 1);
      return MOX_OK;
    }
  }
  // the total is what it was; the run's contribution is lost and the result is the total
  const std::string msg = g_err;
  for (DevBuf& b : fresh) dfree(b.p);
  (void)hipStreamSynchronize(e->stream);
  acc_as_result(e);
  g_err = msg;
  return rc;
}

}  // namespace

extern "C" int mox_accumulate(mox_engine* e) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  return accumulate_impl(e);
}

extern "C" int mox_accumulate_reset(mox_engine* e) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  if (int rc = drain_async(e)) return rc;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  // a result that lives in the total's buffers (after a failed fold) goes with them
  if (e->have_result && e->res.counts == (const uint64_t*)e->a_tab[0].p && e->a_tab[0].p) e->have_result = false;
  free_bufs({&e->a_tab[0], &e->a_tab[1], &e->a_tab[2], &e->a_tc});
  e->acc = mox_engine::Acc{};
  // the last run's result, if any, may be folded into the fresh total
  e->res.folded = false;
  return MOX_OK;
}

extern "C" int mox_accumulate_info(const mox_engine* e, mox_accum_info* out) {
  if (!e || !out) return fail(MOX_EINVAL, "NULL argument");
  out->passes = e->acc.passes;
  out->words = e->acc.n;
  out->tokens = e->acc.tokens;
  out->device_bytes = e->a_tab[0].cap + e->a_tab[1].cap + e->a_tab[2].cap + e->a_tc.cap;
  return MOX_OK;
}

extern "C" int mox_accumulate_file(mox_engine* e, const char* path, uint64_t chunk_bytes) {
  if (!e || !path) return fail(MOX_EINVAL, "NULL argument");
  if (chunk_bytes && chunk_bytes < 256) return fail(MOX_EINVAL, "chunk_bytes %llu: 0 (the whole file) or at least 256", (unsigned long long)chunk_bytes);
  HIPCHK(hipSetDevice(e->device));
  if (int rc = drain_async(e)) return rc;
  if (!chunk_bytes) {
    if (int rc = mox_run_file(e, path)) return rc;
    return accumulate_impl(e);
  }
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(MOX_EIO, "cannot open %s: %s", path, strerror(errno));
  struct stat st;
  if (fstat(fd, &st) != 0) {
    close(fd);
    return fail(MOX_EIO, "cannot stat %s: %s", path, strerror(errno));
  }
  const uint64_t len = (uint64_t)st.st_size;
  // cut search (ws_cuts' rule): 64 KiB windows read forward from each nominal cut
  std::vector<uint8_t> win(1 << 16);
  uint64_t wlo = 0, whi = 0;
  auto byte_at = [&](uint64_t p) -> int {
    if (p < wlo || p >= whi) {
      const ssize_t r = pread(fd, win.data(), win.size(), (off_t)p);
      if (r <= 0) return -1;
      wlo = p;
      whi = p + (uint64_t)r;
    }
    return win[p - wlo];
  };
  int rc = MOX_OK;
  uint64_t lo = 0, k = 1;
  for (;;) {
    // the next cut: the first position >= k chunk_bytes after an ASCII whitespace byte, past lo
    uint64_t hi = len;
    while (len && k <= (len - 1) / chunk_bytes) {
      uint64_t p = std::max(k * chunk_bytes, lo);
      k++;
      while (p < len) {
        const int b = byte_at(p - 1);
        if (b < 0) { rc = fail(MOX_EIO, "cannot read %s: %s", path, strerror(errno)); break; }
        if (b == ' ' || (b >= 9 && b <= 13)) break;
        p++;
      }
      if (rc || p >= len) break;
      if (p > lo) { hi = p; break; }
    }
    if (rc) break;
    const uint64_t n = hi - lo;
    if (e->grp) {
      rc = group_count_fd(e, fd, lo, n);  // the chunk split over the members, as mox_run_file splits a file
    } else {
      rc = stage_file_range(e, fd, lo, n);
      if (!rc) {
        rc = mox_run_range(e, n ? (const void*)e->d_text : nullptr, n, 0, n, 1);
        if (rc == MOX_EUTF8 && e->h_ctl->err_utf8 != ~0ull)  // the reference's InvalidData: the file's offset
          rc = fail(MOX_EUTF8, "stream did not contain valid UTF-8 (byte %llu)", (unsigned long long)(lo + e->h_ctl->err_utf8));
      }
    }
    if (!rc) rc = accumulate_impl(e);
    if (rc || hi >= len) break;
    lo = hi;
  }
  close(fd);
  return rc;
}
