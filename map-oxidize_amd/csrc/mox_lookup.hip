// Device lookup (mox_lookup_words): the counts of given words read out of the
// device-resident result, so that a vocabulary, a watch list or one word is
// answered without fetching the table ("Looking words up").
// Only the query words go up and one count (and index) per query comes back.
//
// Order-agnostic: the queries become a hash set in device memory and the
// result's words are streamed past it once, so the same code serves a table
// in engine order, in rank order after a gather and in bytewise order.
//
//  1. k_lk_build (ws_build): the set of the queries.  A slot holds the hash's
//     upper 43 bits above the query index + 1 in 21.  A query equal to its
//     slot's claimant (same tag, same length, same bytes) links to it (rep[i] =
//     the claimant) and claims nothing: the set holds distinct words only,
//     whichever of the equal queries won the slot.  The queries that claimed a
//     slot are counted (LkCtl::distinct).
//  2. k_lk_stream (ws_stream): one pass over the result.  A match stores the
//     word's count and table index at the representative query.  Table words
//     are distinct, so every representative has at most one writer and the
//     stores are plain.
//  3. k_lk_finish: representatives' outputs copied to their duplicates, and
//     the found positions counted.  One copy brings counts, the control block
//     and the indices to the host.
//
// The set, its slot publication, the stream's four-words-per-lane joint probe,
// the whole-wave path of words over 64 bytes, the probe bounds and the loads
// inside the slack contract are mox_wordset.h's, shared with the join and
// described there; the hash and the exact compare are mox_wordhash.h's.  The
// query buffer carries the slack of a table's bytes, since it is read as one.
// An equal tag with different bytes adds to LkCtl::tag_mismatch with one atomic
// each, in both kernels: the join's per-lane counter cost k_lk_stream two VGPRs
// and up to 1.4 % of its time.
//
// Scratch (mox_engine::l_tmp, l_pin) is O(n + query bytes): the output block,
// the representatives, the query offsets and bytes and the slots.  Nothing is
// sized by the table, and the result is only read.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_lk_build    82 VGPRs,  98 SGPRs, 2052 B LDS, no scratch, no spills (5 waves / SIMD)
//   k_lk_stream  158 VGPRs, 106 SGPRs, 2056 B LDS, no scratch, 25 SGPRs spilled to VGPR lanes (3 waves / SIMD)
//   k_lk_finish   20 VGPRs,  28 SGPRs,    4 B LDS, no scratch, no spills (8 waves / SIMD)
#include <algorithm>
#include <cstdlib>

#include "mox_dev.h"
#include "mox_host.h"
#include "mox_wordset.h"

namespace {

struct LkCtl : WsCtl {
  unsigned long long distinct;  // queries that claimed a slot
  unsigned long long found;     // query positions whose word the result holds
  unsigned long long pad[2];
};
static_assert(sizeof(LkCtl) == 64, "copied with the counts");

// The uploaded queries, their set and the outputs.
struct LkSet {
  const uint64_t* qoffs;
  const uint8_t* qbytes;
  uint64_t nq;
  unsigned long long* slots;
  uint64_t mask;  // slots - 1
  uint32_t* rep;
  uint64_t* o_counts;
  uint64_t* o_index;
  LkCtl* ctl;
};

// The lookup's word set (mox_wordset.h): the keys are the queries.
struct LkWords {
  static constexpr int IDX_BITS = 21;  // slot: query index + 1 ...
  static constexpr int TAG_BITS = 43;  // ... below the hash's upper bits
  static constexpr bool SUM_MISMATCH = false;  // one atomic per tag mismatch (above)
  static __device__ __forceinline__ const uint64_t* offs(const LkSet& S) { return S.qoffs; }
  static __device__ __forceinline__ const uint8_t* bytes(const LkSet& S) { return S.qbytes; }
  static __device__ __forceinline__ uint64_t n(const LkSet& S) { return S.nq; }
  static __device__ __forceinline__ void claimed(const LkSet& S, uint64_t i) { S.rep[i] = (uint32_t)i; }
  static __device__ __forceinline__ void equal(const LkSet& S, uint64_t i, uint64_t j) { S.rep[i] = (uint32_t)j; }
  // the word's count and index go to the representative query
  static __device__ __forceinline__ void match(const LkSet& S, const WsTab& T, uint64_t j, uint64_t ti) {
    S.o_counts[j] = T.counts[ti];
    S.o_index[j] = ti;
  }
  static __device__ __forceinline__ void built(const LkSet& S, uint32_t nd) {
    if (nd) atomicAdd(&S.ctl->distinct, (unsigned long long)nd);
  }
};
static_assert(LkWords::IDX_BITS + LkWords::TAG_BITS == 64 && MOX_LOOKUP_MAX + 1ull <= (1ull << LkWords::IDX_BITS) - 1ull,
              "a slot holds every query index + 1");

}  // namespace

extern "C" __global__ __launch_bounds__(WS_T) void k_lk_build(LkSet S) { ws_build<LkWords>(S); }

extern "C" __global__ __launch_bounds__(WS_T) void k_lk_stream(WsTab T, LkSet S) { ws_stream<LkWords>(T, S); }

// Duplicates take their representative's outputs (a representative's own are
// only read here); the found positions are counted.
extern "C" __global__ __launch_bounds__(WS_T) void k_lk_finish(LkSet S) {
  uint32_t nf = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * WS_T + threadIdx.x; i < S.nq; i += (uint64_t)gridDim.x * WS_T) {
    const uint64_t r = S.rep[i];
    if (r >= S.nq) {
      S.ctl->err = 3;
      continue;
    }
    const uint64_t idx = S.o_index[r];
    if (r != i) {
      S.o_counts[i] = S.o_counts[r];
      S.o_index[i] = idx;
    }
    nf += idx != MOX_LOOKUP_NONE ? 1u : 0u;
  }
  __shared__ uint32_t s_nf;
  if (threadIdx.x == 0) s_nf = 0;
  __syncthreads();
  nf = wave_sum(nf);
  if ((threadIdx.x & 63) == 0 && nf) atomicAdd(&s_nf, nf);
  __syncthreads();
  if (threadIdx.x == 0 && s_nf) atomicAdd(&S.ctl->found, (unsigned long long)s_nf);
}

namespace mox_host {

// mox_lookup_words; with d_index (mox_filter.hip) counts may be NULL, and
// *d_index is the index array in device memory (n entries in l_tmp, valid until
// the next lookup; NULL for n == 0): then only the control block comes back.
int lookup_device(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, uint64_t n, uint64_t* counts, uint64_t* index,
                  mox_lookup_info* info, const uint64_t** d_index) {
  if (!e) return fail(MOX_EINVAL, "engine is NULL");
  if (d_index) *d_index = nullptr;
  if (n > MOX_LOOKUP_MAX) return fail(MOX_EINVAL, "lookup: %llu words (at most MOX_LOOKUP_MAX = %u)", (unsigned long long)n, MOX_LOOKUP_MAX);
  if (n && (!offs || (!counts && !d_index))) return fail(MOX_EINVAL, "lookup: NULL argument");
  uint64_t nb = 0;
  for (uint64_t i = 0; i < n; i++)
    if (offs[i + 1] < offs[i]) return fail(MOX_EINVAL, "lookup: offsets decrease at word %llu", (unsigned long long)i);
  if (n) nb = offs[n] - offs[0];
  if (nb >> 32) return fail(MOX_EINVAL, "lookup: %llu query bytes (fewer than 2^32)", (unsigned long long)nb);
  if (nb && !bytes) return fail(MOX_EINVAL, "lookup: NULL argument");
  if (int rc = result_begin(e)) return rc;
  mox_lookup_info li{};
  li.queries = n;
  if (!n) {
    if (info) *info = li;
    return MOX_OK;
  }
  const mox_engine::Res& r = e->res;
  hipStream_t st = e->stream;
  const Seq q = seq_of(e);
  int rc;
  // device scratch: [counts n | control block | index n] (the part that comes back) | rep | query offsets | slots | query bytes
  const uint64_t nslots = ws_slots(n);
  const size_t out_b = 16 * n + sizeof(LkCtl), qo_b = 8 * (n + 1), sl_b = 8 * nslots;
  LkSet S{};
  uint8_t *out, *d_qbytes;
  uint64_t* d_qoffs;
  if ((rc = carve_dev(e->l_tmp, [&](Carve& c) {
         out = c.take_bytes(out_b);
         S.rep = c.take<uint32_t>(n);
         d_qoffs = c.take<uint64_t>(n + 1);
         S.slots = c.take<unsigned long long>(nslots);
         d_qbytes = c.take_bytes(nb + TABLE_SLACK);  // (the query bytes are read as table bytes are)
       })))
    return rc;
  if ((rc = grow_pinned(e->l_pin, std::max(out_b, qo_b)))) return rc;
  S.o_counts = (uint64_t*)out;
  S.ctl = (LkCtl*)(out + 8 * n);
  S.o_index = (uint64_t*)(out + 8 * n + sizeof(LkCtl));
  S.qoffs = d_qoffs;
  S.qbytes = d_qbytes;
  S.nq = n;
  S.mask = nslots - 1;
  // the offsets rebased to the first word, through the pinned block
  uint64_t* h_offs = (uint64_t*)e->l_pin.p;
  for (uint64_t i = 0; i <= n; i++) h_offs[i] = offs[i] - offs[0];
  HIPCHK(hipMemcpyAsync(d_qoffs, h_offs, qo_b, hipMemcpyHostToDevice, st));
  if (nb) HIPCHK(hipMemcpyAsync(d_qbytes, bytes + offs[0], nb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(S.o_counts, 0, 8 * n + sizeof(LkCtl), st));
  HIPCHK(hipMemsetAsync(S.o_index, 0xFF, 8 * n, st));  // MOX_LOOKUP_NONE
  HIPCHK(hipMemsetAsync(S.slots, 0, sl_b, st));
  const uint64_t cap = 8ull * (uint64_t)e->n_cu;
  const uint64_t qtiles = (n + WS_TILE - 1) / WS_TILE;
  hipLaunchKernelGGL(k_lk_build, dim3((uint32_t)std::min(qtiles, cap)), dim3(WS_T), 0, st, S);
  q.step("k_lk_build");
  if (r.n) {
    const uint64_t scap = grid_cap(e, "MOX_LOOKUP_GRID");
    const uint64_t ttiles = (r.n + WS_TILE - 1) / WS_TILE;
    const WsTab T{r.counts, r.offs, r.bytes, r.n};
    hipLaunchKernelGGL(k_lk_stream, dim3((uint32_t)std::min(ttiles, scap)), dim3(WS_T), 0, st, T, S);
    q.step("k_lk_stream");
  }
  hipLaunchKernelGGL(k_lk_finish, dim3((uint32_t)std::min((n + WS_T - 1) / WS_T, cap)), dim3(WS_T), 0, st, S);
  q.step("k_lk_finish");
  HIPCHK(hipGetLastError());
  // the one copy back: the counts and the control block, and the indices when they are asked for
  uint8_t* h_out = (uint8_t*)e->l_pin.p;
  if (counts) HIPCHK(hipMemcpyAsync(h_out, S.o_counts, index ? out_b : 8 * n + sizeof(LkCtl), hipMemcpyDeviceToHost, st));
  else HIPCHK(hipMemcpyAsync(h_out + 8 * n, S.ctl, sizeof(LkCtl), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  LkCtl h;
  memcpy(&h, h_out + 8 * n, sizeof h);
  if (h.err || h.distinct > n || h.found > n)
    return fail(MOX_EHIP, "lookup: inconsistent query set (error %llu, %llu distinct, %llu found of %llu)", h.err, h.distinct, h.found,
                (unsigned long long)n);
  if (counts) memcpy(counts, h_out, 8 * n);
  if (counts && index) memcpy(index, h_out + 8 * n + sizeof(LkCtl), 8 * n);
  if (d_index) *d_index = S.o_index;
  li.distinct = h.distinct;
  li.found = h.found;
  li.tag_mismatch = h.tag_mismatch;
  if (info) *info = li;
  return MOX_OK;
}

}  // namespace mox_host

extern "C" int mox_lookup_words(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, uint64_t n, uint64_t* counts,
                                uint64_t* index, mox_lookup_info* info) {
  return lookup_device(e, bytes, offs, n, counts, index, info, nullptr);
}
