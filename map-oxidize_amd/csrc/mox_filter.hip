// Device filter (mox_filter_result): the device-resident result made smaller
// on the GPU, so that a stop list, a count threshold, a length range or a
// prefix is applied without fetching the table ("Filtering the
// result").  The kept words, with their counts and in the order they had,
// become the engine's result; only the word list goes up and four totals come
// back.
//
// A stable stream compaction of (counts, offs, bytes), written against
// mox_engine::Res in generic form: any result, whatever buffers it lives in and
// whatever its order.  Rows go in tiles of FL_TILE consecutive rows, one
// workgroup per tile, grid-stride; a tile is 16 wave steps of 64 consecutive
// rows.  Positions come from scans only -- no global atomic decides where a row
// lands -- so the output is a pure function of the table and the predicate.
//
//  1. k_fl_mark (only with a word list): the table index of every list word
//     comes from the lookup (mox_lookup.hip: lookup_device leaves its index
//     array in device memory, nothing sized by the table comes down); one bit
//     per found index is set in an n-bit bitmap.  list_found counts the bits
//     that were newly set, which is the number of bits set.
//  2. k_fl_count: per row the count term, the length term (from the two
//     offsets alone), the bitmap, then the prefix.  The prefix is the only
//     term that touches the word bytes and is evaluated only for rows that
//     passed the others: the 16 bytes from the row's offset on, in one load,
//     masked to the prefix length.  The keep mask is stored, one ballot word
//     per wave step (bit i of the mask = row i), so that the emit pass does not
//     read word bytes again to decide.  Per tile: kept rows, kept bytes, kept
//     count sum.
//  3. k_fl_scan (one workgroup): exclusive scans of the three tile arrays, the
//     totals behind them (mox_tiles.h: scan_tiles).  One 32-byte copy to the host
//     sizes the output; MOX_FILTER_COUNT_ONLY ends here.
//  4. k_fl_emit: a kept row's output index is its tile's scanned base, plus
//     the wave totals before it (LDS), plus its ballot rank; its byte offset
//     the tile's byte base plus a wave scan of the kept lengths.  It writes the
//     count, the offset and the word's bytes; offs[kept] = bytes_kept closes
//     the table.  A tile that keeps nothing is skipped.  Words of up to
//     FL_LANE_MAX bytes are copied by their lane; longer ones (a table word
//     reaches 16 MiB) are listed in LDS and copied by whole waves afterwards,
//     64 consecutive 8-byte words per step.
//
// Loads and stores: a word is copied as 8-byte words from its first byte on
// (any alignment on either side), then a tail of 4, 2 and 1 bytes, so nothing
// is read or written past a word: neighbouring output words belong to other
// lanes (mox_dev.h: copy_lane, copy_wave).  Only the prefix load reads past a
// word, up to 15 bytes behind a 1-byte last word: inside the slack of every
// bytes buffer a result can live in (mox_dev.h: the slack contract), the
// filter's own output buffers included, and what is read past the prefix
// length is masked.
//
// Output: two sets of three buffers (mox_engine::f_tab); a call writes the set
// the result does not live in, so a filtered result can be filtered again, and
// e->res is repointed only when everything has succeeded.  Scratch (f_tmp) is
// O(n / 8): three tile arrays, the keep mask and the list bitmap.
//
// The device join (mox_join_total, at the end of this file) runs the same
// count, scan and emit passes: its match bitmap (mox_join.hip) is the list
// bitmap, and TileTab::counts may point at substituted counts.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_fl_mark   12 VGPRs, 26 SGPRs,     4 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_fl_count  43 VGPRs, 90 SGPRs,    96 B LDS, no scratch, no spills (8 waves / SIMD)
//   k_fl_scan   52 VGPRs, 72 SGPRs,   384 B LDS, no scratch, no spills (one workgroup)
//   k_fl_emit   98 VGPRs, 74 SGPRs, 10312 B LDS, no scratch, no spills (4 waves / SIMD)
#include <algorithm>
#include <cstdlib>

#include "mox_host.h"
#include "mox_tiles.h"

namespace {

constexpr int FL_T = 256;                    // threads of k_fl_mark / k_fl_count / k_fl_emit
constexpr int FL_WAVES = FL_T / 64;
constexpr int FL_PER = 4;                    // rows per thread and tile
constexpr uint32_t FL_TILE = FL_T * FL_PER;  // rows per tile (tests/filter_cases.py TILE)
constexpr uint32_t FL_STEPS = FL_TILE / 64;  // keep-mask words per tile
constexpr uint32_t FL_LANE_MAX = 64;         // a longer word is copied by a whole wave
constexpr int FL_SCAN_PER = 4;               // k_fl_scan: consecutive tiles per thread ...
constexpr uint32_t FL_SCAN_STEP = 1024 * FL_SCAN_PER;  // ... and tiles per step of its one workgroup
static_assert(FL_TILE == 1024, "tests/filter_cases.py TILE");
static_assert(FL_SCAN_STEP == 4096, "tests/test_gpu_big_table.py FILTER_SCAN_STEP");
static_assert(FL_TILE <= 65536, "s_big_k holds 16-bit rows");
static_assert(MOX_FILTER_PREFIX_MAX == 16, "the prefix is two 8-byte words");

// The predicate as the kernels take it: bounds with "no upper bound" resolved,
// the prefix as two masked 8-byte words, the list as a bitmap over table rows.
struct FlPred {
  uint64_t min_count, max_count, min_len, max_len;
  uint64_t p0, p1, m0, m1, plen;
  const uint32_t* listed;  // bit i: row i is a list word
  uint32_t list_mode;      // 0: no list term, 1: listed rows are dropped, 2: only listed rows survive
};
struct FlOut {
  uint64_t* counts;
  uint64_t* offs;
  uint8_t* bytes;
  uint64_t kept, bytes_kept;
};

}  // namespace

// One bit per list word the table holds: idx[q] is the word's table index
// (MOX_LOOKUP_NONE: absent; duplicates of a list word carry the same index).
// *found += the bits this launch set.
extern "C" __global__ __launch_bounds__(FL_T) void k_fl_mark(const uint64_t* idx, uint64_t nq, uint32_t* listed, uint64_t n,
                                                             unsigned long long* found) {
  __shared__ uint32_t s_nf;
  if (threadIdx.x == 0) s_nf = 0;
  __syncthreads();
  uint32_t nf = 0;
  for (uint64_t q = (uint64_t)blockIdx.x * FL_T + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * FL_T) {
    const uint64_t i = idx[q];
    if (i < n) {  // (MOX_LOOKUP_NONE is no row)
      const uint32_t bit = 1u << (i & 31);
      nf += (atomicOr(listed + (i >> 5), bit) & bit) ? 0u : 1u;
    }
  }
  nf = wave_sum(nf);
  if ((threadIdx.x & 63) == 0 && nf) atomicAdd(&s_nf, nf);
  __syncthreads();
  if (threadIdx.x == 0 && s_nf) atomicAdd(found, (unsigned long long)s_nf);
}

// keep[tile * FL_STEPS + step] = the ballot of "row is kept" over rows
// tile * FL_TILE + step * 64 + lane; tc[0 * nt + tile] = kept rows, tc[1 * nt +
// tile] = kept bytes, tc[2 * nt + tile] = kept count sum of the tile.
extern "C" __global__ __launch_bounds__(FL_T) void k_fl_count(TileTab T, FlPred P, uint64_t* __restrict__ keep, uint64_t* __restrict__ tc) {
  __shared__ uint64_t s_w[FL_WAVES][3];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (uint64_t tile = blockIdx.x; tile < T.nt; tile += gridDim.x) {
    const uint64_t base = tile * FL_TILE;
    uint64_t nk = 0, nb = 0, cs = 0;
#pragma unroll
    for (int j = 0; j < FL_PER; j++) {
      const uint64_t i = base + (uint32_t)j * FL_T + t;
      bool k = false;
      uint64_t len = 0, c = 0;
      if (i < T.n) {
        const uint64_t o = T.offs[i];
        len = T.offs[i + 1] - o;
        c = T.counts[i];
        k = c >= P.min_count && c <= P.max_count && len >= P.min_len && len <= P.max_len;
        if (k && P.list_mode) {
          const bool in = (P.listed[i >> 5] >> (i & 31)) & 1u;
          k = P.list_mode == 2 ? in : !in;
        }
        if (k && P.plen) {
          k = len >= P.plen;  // a word shorter than the prefix is dropped
          if (k) {
            const Key16 w = *reinterpret_cast<const Key16*>(T.bytes + o);
            k = (w.lo & P.m0) == P.p0 && (w.hi & P.m1) == P.p1;
          }
        }
      }
      const uint64_t m = __ballot(k);
      if (lane == 0) keep[tile * FL_STEPS + (uint32_t)j * FL_WAVES + wv] = m;
      if (k) {
        nk++;
        nb += len;
        cs += c;
      }
    }
    nk = wave_sum(nk);
    nb = wave_sum(nb);
    cs = wave_sum(cs);
    if (lane == 0) {
      s_w[wv][0] = nk;
      s_w[wv][1] = nb;
      s_w[wv][2] = cs;
    }
    __syncthreads();
    if (t < 3) {
      uint64_t v = 0;
      for (int k = 0; k < FL_WAVES; k++) v += s_w[k][t];
      tc[(uint64_t)t * T.nt + tile] = v;
    }
    __syncthreads();
  }
}

// Exclusive scans in place of the three tile arrays; the totals at tc[3 nt +
// k], k = kept rows, kept bytes, kept count sum.  One workgroup (mox_tiles.h:
// scan_tiles), FL_SCAN_STEP tiles of all three arrays per step.
extern "C" __global__ __launch_bounds__(1024) void k_fl_scan(uint64_t* tc, uint64_t nt) {
  scan_tiles<3, FL_SCAN_PER, 1024>(tc, nt, tc + 3 * nt);
}

// Every kept row at its scanned position (keep: k_fl_count's masks, tc:
// k_fl_scan's output).
extern "C" __global__ __launch_bounds__(FL_T) void k_fl_emit(TileTab T, const uint64_t* __restrict__ keep, const uint64_t* __restrict__ tc,
                                                             FlOut out) {
  __shared__ uint64_t s_w[FL_WAVES][2];   // a round's kept rows and kept bytes per wave
  __shared__ uint64_t s_big_b[FL_TILE];   // words over FL_LANE_MAX bytes: byte offset in the output,
  __shared__ uint16_t s_big_k[FL_TILE];   // ... row inside the tile
  __shared__ uint32_t s_nbig;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (blockIdx.x == 0 && t == 0) out.offs[out.kept] = out.bytes_kept;
  for (uint64_t tile = blockIdx.x; tile < T.nt; tile += gridDim.x) {
    const uint64_t base = tile * FL_TILE;
    uint64_t rk = tc[tile], rb = tc[T.nt + tile];  // running output row and byte offset
    // a tile that keeps nothing: the next tile's base is this one's (the same for every thread: no barrier is left out by some)
    if ((tile + 1 < T.nt ? tc[tile + 1] : out.kept) == rk) continue;
    if (t == 0) s_nbig = 0;
    for (int j = 0; j < FL_PER; j++) {
      const uint64_t i = base + (uint32_t)j * FL_T + t;
      const uint64_t m = keep[tile * FL_STEPS + (uint32_t)j * FL_WAVES + wv];  // (no bit of a row past the table is set)
      const bool k = (m >> lane) & 1ull;
      uint64_t o = 0, len = 0, cnt = 0;
      if (k) {
        o = __builtin_nontemporal_load(T.offs + i);
        len = __builtin_nontemporal_load(T.offs + i + 1) - o;
        cnt = __builtin_nontemporal_load(T.counts + i);
      }
      const uint64_t inc = wave_incscan<uint64_t>(len);
      __syncthreads();  // the previous round's s_w has been read (and s_nbig is zero)
      if (lane == 63) {
        s_w[wv][0] = (uint64_t)__popcll(m);
        s_w[wv][1] = inc;
      }
      __syncthreads();
      uint64_t pk = rk, pb = rb;
      for (uint32_t w = 0; w < (uint32_t)FL_WAVES; w++) {
        if (w < wv) {
          pk += s_w[w][0];
          pb += s_w[w][1];
        }
        rk += s_w[w][0];
        rb += s_w[w][1];
      }
      if (k) {
        const uint64_t below = lane ? ~0ull >> (64 - lane) : 0ull;
        const uint64_t r = pk + __popcll(m & below), bo = pb + inc - len;
        if (r < out.kept && bo + len <= out.bytes_kept) {  // (always, for the masks the scan saw)
          out.counts[r] = cnt;
          out.offs[r] = bo;
          if (len <= FL_LANE_MAX) {
            copy_lane(out.bytes + bo, T.bytes + o, len);
          } else {  // a whole wave below
            const uint32_t x = atomicAdd(&s_nbig, 1u);
            s_big_b[x] = bo;
            s_big_k[x] = (uint16_t)((uint32_t)j * FL_T + t);
          }
        }
      }
    }
    __syncthreads();
    // words over FL_LANE_MAX bytes: one wave each
    const uint32_t nbig = s_nbig;
    for (uint32_t x = wv; x < nbig; x += FL_WAVES) {
      const uint64_t i = base + s_big_k[x];
      const uint64_t o = T.offs[i];
      copy_wave(out.bytes + s_big_b[x], T.bytes + o, T.offs[i + 1] - o);
    }
    __syncthreads();  // the LDS arrays are the next tile's
  }
}

namespace {

// A call's scratch in f_tmp: [tile arrays 3 nt | totals 3 | list_found | pad 4] [keep masks 16 nt] [list bitmap]
struct FlTmp {
  uint64_t* tc;
  uint64_t* keep;
  uint32_t* listed;
};

// f_tmp grown and laid out for the table T, the totals and (with bitmap) the list bitmap zeroed.
int fl_scratch(mox_engine* e, const TileTab& T, bool bitmap, FlTmp* s) {
  const size_t bm_b = bitmap ? ((T.n + 63) / 64) * 8 + 8 : 0;
  if (int rc = carve_dev(e->f_tmp, [&](Carve& c) {
        s->tc = c.take<uint64_t>(3 * T.nt + 8);
        s->keep = c.take<uint64_t>(T.nt * FL_STEPS);
        s->listed = (uint32_t*)c.take_bytes(bm_b);
      }))
    return rc;
  if (T.n) {
    HIPCHK(hipMemsetAsync(s->tc + 3 * T.nt, 0, 64, e->stream));
    if (bitmap) HIPCHK(hipMemsetAsync(s->listed, 0, bm_b, e->stream));
  }
  return MOX_OK;
}

// The count pass and the scan over a table with rows; tot[0, 4) = kept rows,
// kept bytes, kept count sum, list words found.  Synchronises.
int fl_select(mox_engine* e, const TileTab& T, const FlPred& P, const FlTmp& s, uint32_t grid, uint64_t* tot) {
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  hipLaunchKernelGGL(k_fl_count, dim3(grid), dim3(FL_T), 0, st, T, P, s.keep, s.tc);
  q.step("k_fl_count");
  hipLaunchKernelGGL(k_fl_scan, dim3(1), dim3(1024), 0, st, s.tc, T.nt);
  q.step("k_fl_scan");
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(tot, s.tc + 3 * T.nt, 32, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return MOX_OK;
}

// The kept rows of T (tot: fl_select's) into the set of f_tab the result r does
// not live in: *dst.  Synchronises; e->res is the caller's to repoint.
int fl_emit(mox_engine* e, const mox_engine::Res& r, const TileTab& T, const FlTmp& s, uint32_t grid, const uint64_t* tot, DevBuf** dst_out) {
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  DevBuf* dst = table_other_set(e->f_tab, r);
  if (int rc = table_reserve(dst[0], dst[1], dst[2], tot[0], tot[1])) return rc;
  const FlOut out{(uint64_t*)dst[0].p, (uint64_t*)dst[1].p, (uint8_t*)dst[2].p, tot[0], tot[1]};
  if (T.n) {
    hipLaunchKernelGGL(k_fl_emit, dim3(grid), dim3(FL_T), 0, st, T, s.keep, s.tc, out);
    q.step("k_fl_emit");
    HIPCHK(hipGetLastError());
  } else {
    HIPCHK(hipMemsetAsync(out.offs, 0, 8, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  *dst_out = dst;
  return MOX_OK;
}

// device memory the filter (and the join, which shares it) holds
uint64_t fl_device_bytes(const mox_engine* e) {
  uint64_t b = e->f_tmp.cap;
  for (auto& set : e->f_tab)
    for (const DevBuf& d : set) b += d.cap;
  return b;
}

}  // namespace

extern "C" int mox_filter_result(mox_engine* e, const mox_filter* f, mox_filter_info* info) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  if (!f) return fail(MOX_EINVAL, "filter is NULL");
  for (uint64_t r : f->reserved)
    if (r) return fail(MOX_EINVAL, "filter: a reserved word is not 0");
  if (f->flags & ~MOX_FILTER_COUNT_ONLY) return fail(MOX_EINVAL, "filter: unknown flags 0x%x", f->flags);
  if (f->words_mode != MOX_FILTER_WORDS_DROP && f->words_mode != MOX_FILTER_WORDS_KEEP)
    return fail(MOX_EINVAL, "filter: unknown words_mode %u", f->words_mode);
  if (f->prefix_len > MOX_FILTER_PREFIX_MAX)
    return fail(MOX_EINVAL, "filter: a prefix of %llu bytes (at most MOX_FILTER_PREFIX_MAX = %d)", (unsigned long long)f->prefix_len,
                MOX_FILTER_PREFIX_MAX);
  if (f->prefix_len && !f->prefix) return fail(MOX_EINVAL, "filter: NULL prefix");
  const uint64_t nq = f->n_words;
  if (nq > MOX_LOOKUP_MAX) return fail(MOX_EINVAL, "filter: %llu list words (at most MOX_LOOKUP_MAX = %u)", (unsigned long long)nq, MOX_LOOKUP_MAX);
  if (nq && !f->word_offs) return fail(MOX_EINVAL, "filter: NULL word_offs");
  for (uint64_t i = 0; i < nq; i++)
    if (f->word_offs[i + 1] < f->word_offs[i]) return fail(MOX_EINVAL, "filter: list offsets decrease at word %llu", (unsigned long long)i);
  if (nq && f->word_offs[nq] != f->word_offs[0] && !f->words) return fail(MOX_EINVAL, "filter: NULL words");
  if (int rc = result_begin(e)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const mox_engine::Res r = e->res;
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  int rc;
  // the list words' table indices, left in device memory by the lookup
  const uint64_t* d_index = nullptr;
  if (nq && (rc = lookup_device(e, f->words, f->word_offs, nq, nullptr, nullptr, nullptr, &d_index))) return rc;

  FlPred P{};
  P.min_count = f->min_count;
  P.max_count = f->max_count ? f->max_count : ~0ull;
  P.min_len = f->min_len;
  P.max_len = f->max_len ? f->max_len : ~0ull;
  P.plen = f->prefix_len;
  if (P.plen) {
    uint8_t pb[16] = {0};
    memcpy(pb, f->prefix, P.plen);
    memcpy(&P.p0, pb, 8);
    memcpy(&P.p1, pb + 8, 8);
    P.m0 = P.plen >= 8 ? ~0ull : (1ull << (8 * P.plen)) - 1ull;
    P.m1 = P.plen <= 8 ? 0ull : P.plen >= 16 ? ~0ull : (1ull << (8 * (P.plen - 8))) - 1ull;
  }
  P.list_mode = f->words_mode == MOX_FILTER_WORDS_KEEP ? 2u : nq ? 1u : 0u;

  const TileTab T = tile_tab(r, FL_TILE);
  FlTmp s;
  if ((rc = fl_scratch(e, T, P.list_mode != 0, &s))) return rc;
  P.listed = s.listed;
  uint64_t* tot = e->h_tot;  // kept rows, kept bytes, kept count sum, list words found
  for (int k = 0; k < 4; k++) tot[k] = 0;
  const uint32_t grid = (uint32_t)std::min(T.nt, grid_cap(e, "MOX_FILTER_GRID"));
  if (T.n) {
    if (nq) {
      hipLaunchKernelGGL(k_fl_mark, dim3((uint32_t)std::min<uint64_t>((nq + FL_T - 1) / FL_T, 8ull * (uint64_t)e->n_cu)), dim3(FL_T), 0, st,
                         d_index, nq, s.listed, T.n, (unsigned long long*)(s.tc + 3 * T.nt + 3));
      q.step("k_fl_mark");
    }
    if ((rc = fl_select(e, T, P, s, grid, tot))) return rc;
  }
  if (tot[0] > r.n || tot[1] > r.nb || tot[3] > nq)
    return fail(MOX_EHIP, "filter: inconsistent totals (%llu of %llu rows, %llu of %llu bytes, %llu of %llu list words)",
                (unsigned long long)tot[0], (unsigned long long)r.n, (unsigned long long)tot[1], (unsigned long long)r.nb,
                (unsigned long long)tot[3], (unsigned long long)nq);
  mox_filter_info fi{};
  fi.words_in = r.n;
  fi.words_kept = tot[0];
  fi.tokens_in = r.tokens;
  fi.tokens_kept = tot[2];
  fi.bytes_kept = tot[1];
  fi.list_found = tot[3];
  auto finish = [&]() {
    fi.device_bytes = fl_device_bytes(e);
    fi.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = fi;
    return MOX_OK;
  };
  if (f->flags & MOX_FILTER_COUNT_ONLY) return finish();
  if (test_fail_hook("MOX_TEST_FAIL_FILTER"))
    return fail(MOX_ENOMEM, "filter: injected failure before the output is written (MOX_TEST_FAIL_FILTER)");
  DevBuf* dst;
  if ((rc = fl_emit(e, r, T, s, grid, tot, &dst))) return rc;
  // the kept words are the result: order, sorted and folded as the source had them
  mox_engine::Res& res = e->res;
  res_point_at(res, dst, tot[0], tot[1], tot[2]);
  return finish();
}

// The join's host side lives here, beside the compaction it shares with the
// filter; its kernels and the match are mox_join.hip's (join_match).
extern "C" int mox_join_total(mox_engine* e, const mox_join* j, mox_join_info* info) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  if (!j) return fail(MOX_EINVAL, "join is NULL");
  for (uint64_t r : j->reserved)
    if (r) return fail(MOX_EINVAL, "join: a reserved word is not 0");
  if (j->pad) return fail(MOX_EINVAL, "join: pad is not 0");
  if (j->flags & ~MOX_JOIN_COUNT_ONLY) return fail(MOX_EINVAL, "join: unknown flags 0x%x", j->flags);
  if (j->mode != MOX_JOIN_SEMI && j->mode != MOX_JOIN_ANTI) return fail(MOX_EINVAL, "join: unknown mode %u", j->mode);
  if (j->counts != MOX_JOIN_COUNTS_RESULT && j->counts != MOX_JOIN_COUNTS_TOTAL && j->counts != MOX_JOIN_COUNTS_MIN)
    return fail(MOX_EINVAL, "join: unknown counts value %u", j->counts);
  if (j->mode == MOX_JOIN_ANTI && j->counts != MOX_JOIN_COUNTS_RESULT)
    return fail(MOX_EINVAL, "join: MOX_JOIN_ANTI keeps words the total lacks: only MOX_JOIN_COUNTS_RESULT");
  if (int rc = result_begin(e)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const mox_engine::Res r = e->res;
  if (r.n > MOX_JOIN_MAX_WORDS)
    return fail(MOX_EINVAL, "join: a result of %llu words (at most MOX_JOIN_MAX_WORDS = %llu)", (unsigned long long)r.n, MOX_JOIN_MAX_WORDS);
  const uint64_t tn = e->acc.have ? e->acc.n : 0;  // an empty accumulator is an empty total
  const uint64_t cap = grid_cap(e, "MOX_JOIN_GRID");
  int rc;
  TileTab T = tile_tab(r, FL_TILE);
  FlTmp s;
  if ((rc = fl_scratch(e, T, true, &s))) return rc;
  // the match bitmap is the filter's list bitmap; with an empty side it stays zero and no kernel reads the total
  JoinSums js;
  const uint64_t* subst = nullptr;
  if (r.n && tn &&
      (rc = join_match(e, r, (const uint64_t*)e->a_tab[0].p, (const uint64_t*)e->a_tab[1].p, (const uint8_t*)e->a_tab[2].p, tn, j->counts,
                       s.listed, cap, &js, &subst)))
    return rc;
  if (subst) T.counts = subst;  // the kept rows carry the total's count or the smaller one
  FlPred P{};
  P.max_count = ~0ull;
  P.max_len = ~0ull;
  P.listed = s.listed;
  P.list_mode = j->mode == MOX_JOIN_SEMI ? 2u : 1u;
  uint64_t* tot = e->h_tot;  // kept rows, kept bytes, kept count sum
  for (int k = 0; k < 4; k++) tot[k] = 0;
  const uint32_t grid = (uint32_t)std::min(T.nt, cap);
  if (T.n && (rc = fl_select(e, T, P, s, grid, tot))) return rc;
  const uint64_t want = j->mode == MOX_JOIN_SEMI ? js.matched : r.n - js.matched;
  if (tot[0] != want || tot[1] > r.nb)
    return fail(MOX_EHIP, "join: inconsistent totals (%llu rows kept, %llu of %llu matched, %llu of %llu bytes)", (unsigned long long)tot[0],
                (unsigned long long)js.matched, (unsigned long long)r.n, (unsigned long long)tot[1], (unsigned long long)r.nb);
  mox_join_info ji{};
  ji.words_in = r.n;
  ji.words_total = tn;
  ji.words_matched = js.matched;
  ji.words_kept = tot[0];
  ji.tokens_in = r.tokens;
  ji.tokens_total = e->acc.have ? e->acc.tokens : 0;
  ji.tokens_matched_result = js.tokens_result;
  ji.tokens_matched_total = js.tokens_total;
  ji.tokens_min = js.tokens_min;
  ji.tokens_kept = tot[2];
  ji.bytes_kept = tot[1];
  ji.tag_mismatch = js.tag_mismatch;
  auto finish = [&]() {
    ji.device_bytes = fl_device_bytes(e) + e->j_tmp.cap;
    ji.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = ji;
    return MOX_OK;
  };
  if (j->flags & MOX_JOIN_COUNT_ONLY) return finish();
  if (test_fail_hook("MOX_TEST_FAIL_JOIN"))
    return fail(MOX_ENOMEM, "join: injected failure before the output is written (MOX_TEST_FAIL_JOIN)");
  DevBuf* dst;
  if ((rc = fl_emit(e, r, T, s, grid, tot, &dst))) return rc;
  // the kept rows are the result: order, sorted and folded as R had them; substituted counts are in no count order
  mox_engine::Res& res = e->res;
  res_point_at(res, dst, tot[0], tot[1], tot[2]);
  if (j->counts != MOX_JOIN_COUNTS_RESULT && tot[0] > 1) res.ranked = false;
  return finish();
}
