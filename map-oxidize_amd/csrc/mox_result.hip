// Host helpers of the calls over the device-resident result (sort, top-k, text,
// accumulate, lookup, filter, rank, re-key, find, join, histogram): their
// engine-owned buffers are grown and freed here, a result is pointed at a set
// of table buffers here, and the grid cap and the failure hook of the tests are
// read here.  Host code only, and nothing is hashed: one object serves
// libmox.so, libmox_check.so and libmox_hc.so.
#include "mox_host.h"

namespace mox_host {

int grow_dev(DevBuf& b, size_t bytes) {
  if (b.cap >= bytes && b.p) return MOX_OK;
  dfree(b.p);
  b.p = nullptr;
  b.cap = 0;
  size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
  hipError_t err = hipMalloc(&b.p, want);
  if (err != hipSuccess) {
    b.p = nullptr;
    (void)hipGetLastError();  // the failed allocation's error is not a later launch's (callers may fall back)
    return fail(MOX_ENOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(err));
  }
  b.cap = want;
  return MOX_OK;
}
int grow_pinned(DevBuf& b, size_t bytes) {
  if (b.cap >= bytes && b.p) return MOX_OK;
  if (b.p) (void)hipHostFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
  hipError_t err = hipHostMalloc(&b.p, want, hipHostMallocDefault);
  if (err != hipSuccess) return fail(MOX_ENOMEM, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(err));
  b.cap = want;
  return MOX_OK;
}
void free_bufs(std::initializer_list<DevBuf*> bufs) {
  for (DevBuf* b : bufs) {
    dfree(b->p);
    *b = DevBuf{};
  }
}
int table_reserve(DevBuf& counts, DevBuf& offs, DevBuf& bytes, uint64_t n, uint64_t nb) {
  int rc;
  if ((rc = grow_dev(counts, 8 * n + TABLE_SLACK)) || (rc = grow_dev(offs, 8 * (n + 1) + TABLE_SLACK)) || (rc = grow_dev(bytes, nb + TABLE_SLACK)))
    return rc;
  return MOX_OK;
}
DevBuf* table_other_set(DevBuf (*sets)[3], const mox_engine::Res& r) {
  return sets[(sets[0][0].p && r.counts == (const uint64_t*)sets[0][0].p) ? 1 : 0];
}
void res_point_at(mox_engine::Res& r, DevBuf* set, uint64_t n, uint64_t nb, uint64_t tokens) {
  r.counts = (const uint64_t*)set[0].p;
  r.offs = (const uint64_t*)set[1].p;
  r.bytes = (const uint8_t*)set[2].p;
  r.n = n;
  r.nb = nb;
  r.tokens = tokens;
  r.pass = false;
  r.exchanged = false;
}
uint64_t grid_cap(const mox_engine* e, const char* env) {
  uint64_t cap = 8ull * (uint64_t)e->n_cu;
  if (const char* g = getenv(env))
    if (atoll(g) > 0) cap = std::min<uint64_t>(cap, (uint64_t)atoll(g));
  return cap;
}
bool test_fail_hook(const char* env) {
  const char* x = getenv(env);
  return x && atoi(x);
}

void result_free(mox_engine* e) {
  free_bufs({&e->s_counts, &e->s_offs, &e->s_bytes, &e->s_tmp,                              // sort
             &e->k_tmp, &e->k_out,                                                          // top-k
             &e->tx_pre, &e->tx_slice[0], &e->tx_slice[1],                                  // text
             &e->a_tab[0], &e->a_tab[1], &e->a_tab[2], &e->a_tc,                            // accumulate
             &e->l_tmp,                                                                     // lookup
             &e->f_tab[0][0], &e->f_tab[0][1], &e->f_tab[0][2], &e->f_tab[1][0], &e->f_tab[1][1], &e->f_tab[1][2], &e->f_tmp,  // filter
             &e->r_tab[0][0], &e->r_tab[0][1], &e->r_tab[0][2], &e->r_tab[1][0], &e->r_tab[1][1], &e->r_tab[1][2], &e->r_tmp,  // rank
             &e->q_tc,                                                                      // re-key
             &e->fd_tmp,                                                                    // find
             &e->j_tmp,                                                                     // join
             &e->hg_tmp, &e->hg_out});                                                      // histogram
  e->acc = mox_engine::Acc{};
  for (DevBuf* b : {&e->h_bsort, &e->tx_pin[0], &e->tx_pin[1], &e->l_pin, &e->h_rmax, &e->fd_pin, &e->hg_pin}) {  // pinned
    if (b->p) (void)hipHostFree(b->p);
    *b = DevBuf{};
  }
  for (hipEvent_t& ev : e->tx_ev) {
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr;
  }
}

}  // namespace mox_host
